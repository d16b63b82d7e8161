"""The bf16 VGG networks op by op against float64, on the tensors the HIP networks themselves produced.

VGGStyleDiscriminator128 / 256 (compute_dtype='bf16') and VGGFeatureExtractor (compute_dtype='bf16') cannot be pinned end to end:
rounding flips compound through 19 conv / BatchNorm stages, so two float64 models of bf16 storage that differ only in their
accumulation precision are already 0.07 - 0.13 relative L2 apart on every gradient.  Here nothing compounds: a recorder
(tests/bf16_opwise.py) stands in for the autograd Functions the per-layer routes look up at call time, so one forward + backward of
the production route leaves every op's inputs, output and upstream gradient; each op is then replayed alone and compared with float64
of that one op.  Two anchors, both bit for bit: the recorded run equals the plain ``net(x)`` (whole-network driver; for the feature
extractor the unpatched forward), and every replay reproduces its recorded output and, where its input has a single consumer (every
op of the discriminators; all but the tapped features of the extractor), the recorded input gradient.

Bounds are derived from counts of roundings, nothing is fitted; every element of every tensor is checked.  EPS = 2^-24 (half an fp32
ulp, relative).  hulp(v) = 2^(floor(log2 |v|) - 8) is half a bf16 ulp of v, evaluated per value at |ref| + E where E is the error
before the store.  A is the same operation on absolute values in float64.  The build uses -ffp-contract=off, so every product and
sum below is its own rounding.

  conv forward      y64 = act(conv64(x, bf16(w)) + b): x the recorded bf16 input, w rounded as the packing does, b fp32.  The 4x4 / s2
                    reference is F.conv2d(stride=2, padding=1) of the 4x4 weight, so the pixel-unshuffle embedding, s2_channels and
                    the 3x3-embedded weight image are under test.  E = k EPS A + EPS |y64| with the rule of
                    tests/test_conv_ops_gpu.py::test_conv3x3_bf16: k = 2 * 9 * cin_k + 8, two roundings per product of the MFMA chain
                    over (tap, channel) of the operand the kernel walks (cin_k = cin rounded up to 16 for 3x3, 4 cin for the
                    unshuffled operand of a 4x4 conv), + 8 for the epilogue.  |y - y64| <= E + hulp(|y64| + E).  A LeakyReLU slope
                    <= 1 only shrinks an error; where the rounded pre-activation has the other sign, the branch difference is at most
                    the pre-activation's own error.
  conv data grad    dz = gy where the recorded output is > 0, else bf16(fp32(gy) * slope) (sr_lrelu_bwd_bf16: one product, one
                    rounding; modelled exactly), applied when act_slope != 1.  dx64 = conv_transpose64(dz, bf16(w)), same form with
                    k = 2 * 9 * roundup16(cout) + 8; pad channels of dx (conv0_0 / conv1_1: 3 real of 16) must be zero.
  conv weight grad  fp32 outputs.  dw64 = conv2d_weight64(x, dz), db64 = sum dz; A = the same sums of |x| |dz|.  The order-independent
                    rule of test_conv_ops_gpu.py (test_rdb_wgrad_bf16): any order of summing N products loses at most N - 1 roundings,
                    two roundings per MFMA product: k = 2 n H W + 3 over the n H W positions of the gradient grid (+3: scale, bias,
                    accumulate).  |dw - dw64| <= k EPS A + EPS |dw64|.  The 4x4 gradient arrives through the dw3 -> dw4 fold, which
                    moves values and sums nothing.
  BatchNorm + LeakyReLU, train mode.  M = n h w.  The reductions run in a fixed tree; a term passes through at most L additions on its
                    way to the root, so a sum S of M terms carries at most L EPS sum|terms| whatever the values.  L restated from the
                    kernels: the one-launch kernel (bn_small.h, M <= 32768: every configuration here) walks ceil(M / 1024) pixels
                    per thread, then 6 shuffle steps, then the 16 wave results in order: L = ceil(M / 1024) + 22; the two-stage
                    kernels (disc_bf16.hip) walk ceil(M / 8192) pixels per thread, 6 shuffle steps, 3 adds over the waves, then 64
                    partial sums in order: L = ceil(M / 8192) + 73.  + 6 for what surrounds a sum (up to four roundings inside a term,
                    1 / M and its product) as in tests/test_layout_ops_gpu.py::test_bn_lrelu_eval_mode's M + 6: K = L + 6.
                      mean      dmu  = K EPS sum|x| / M
                      variance  the kernels sum (x - mean^)^2; sum (x - mean^)^2 = sum (x - mean)^2 + M (mean - mean^)^2 exactly,
                                so dvar = K EPS var + dmu^2
                      invstd    relative error ris = dvar / (2 (var + eps)) + 3 EPS  (the add, rsqrtf to 1 ulp = 2 EPS)
                      y         E_bn = |gamma| invstd (|x - mean| ris + dmu) + 5 EPS (|gamma xhat| + |beta|)  (subtraction, two
                                products, the add, the LeakyReLU product);  |y - y64| <= E_bn + hulp(|y64| + E_bn)
                      running_mean against 0.9 old + 0.1 mean:            4 EPS (0.9 |old| + 0.1 |mean|) + 0.1 dmu
                      running_var  against 0.9 old + 0.1 var M / (M - 1): 4 EPS (0.9 |old| + 0.1 unbiased) + 0.1 dvar M / (M - 1)
                                (4: fp32(0.1) and 1 - fp32(0.1) are each within EPS of 0.1 / 0.9; the subtraction, product and add)
                      num_batches_tracked: exactly one more than before.
                    backward: dz = gy (a > 0 ? 1 : 0.2) from the op's own bf16 output a, a product in fp32.
                      dbeta  = sum dz,        bound K EPS sum|dz|
                      dgamma = sum dz xhat,   bound K EPS sum|dz xhat| + sum |dz| dxhat,  dxhat = invstd (|x - mean| ris + dmu): the
                                kernel's xhat is built from its own mean and invstd
                      dx = gamma invstd (dz - (dbeta + xhat dgamma) / M):
                                e_t = (e_dbeta + |xhat| e_dgamma + |dgamma| (dxhat + 2 EPS |xhat|)) / M
                                      + 6 EPS (|dz| + (|dbeta| + |xhat dgamma|) / M)
                                E = |gamma| invstd e_t + |dx64| (ris + 2 EPS);  |dx - dx64| <= E + hulp(|dx64| + E)
  BatchNorm, eval mode.  mean and variance are the running buffers (dmu = dvar = 0, ris = 3 EPS), nothing moves;
                    dx = gamma invstd dz with E = |dx64| (ris + 3 EPS).
  ReLU / LeakyReLU (LReLUFn16), max-pool, ToCB16, FromCB16, ChannelAffineFn: bit-exact against torch on the recorded values
                    (selections, conversions, or one product / one product and one add with one rounding each).
  LinearFn          the forms of tests/test_train_ops_gpu.py::test_linear: y within EPS ((ceil(nin / 256) + 11) |x| |w|^T + |z|);
                    dz exactly from the kernel's own y; dx within EPS (nout + 1) |dz| |w|, dw within EPS (n + 1) |dz|^T |x|,
                    db within EPS (n + 1) sum |dz|.

Every train-mode BatchNorm of these configurations has M <= 32768 and takes the one-launch kernel (bn_small.h);
test_batchnorm_general_path replays the same recorded ops with that kernel switched off, against the bounds of the two-stage tree.

Negative controls (test_negative_controls): six mutated references that the kernel's output must MISS under the same bounds.
"""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_restoration_amd as ira
from image_restoration_amd import _lib
from image_restoration_amd import hip_autograd as A
from image_restoration_amd import hip_autograd_bf16 as B
from image_restoration_amd.utils import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_opwise as W  # noqa: E402
from bf16_opwise import EPS, bf, cb16_to_nchw, check, hulp, nchw_to_cb16, worst  # noqa: E402

pytestmark = pytest.mark.gpu

TABLE = {B: ('ConvFn16', 'BNLReLUFn16', 'ToCB16', 'FromCB16', 'LReLUFn16', 'MaxPool2x2Fn16'), A: ('LinearFn', 'ChannelAffineFn')}
DISC = ['d128-n3', 'd128-n2-moved', 'd256-n2', 'd128-eval']
CONFIGS = DISC + ['vgg19']
TAPS = ['relu1_1', 'pool1', 'conv3_4', 'conv5_4']
WORST = {}


def _f32(v):
    return float(np.float32(v))


def _note(config, what, ratio):
    key = (config, what)
    WORST[key] = max(WORST.get(key, 0.0), ratio)


def _report(config):
    for (cfg, what), r in sorted(WORST.items()):
        if cfg == config:
            print(f'WORST {cfg:14s} {what:24s} got / bound = {r:.3f}')


# ------------------------------------------------------------------------------------------------------------------ recorded runs
class Run:
    pass


_RUNS = {}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _disc_run(dev, config):
    kind = 'VGGStyleDiscriminator256' if config.startswith('d256') else 'VGGStyleDiscriminator128'
    size = 256 if kind.endswith('256') else 128
    n = 3 if config == 'd128-n3' else 2
    net = ira.build_network(dict(type=kind, num_in_ch=3, num_feat=16, compute_dtype='bf16')).to(dev)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.vgg128_state_dict(61, 3, 16, size).items()}, strict=True)
    net.train()
    drv = copy.deepcopy(net)
    if config == 'd128-n2-moved':   # running buffers that have already moved: two train-mode forwards on other inputs
        for seed in (7, 8):
            xs = _t(synth.uniform_input(seed, (n, 3, size, size)), dev)
            with torch.no_grad():
                net(xs), drv(xs)
    if config == 'd128-eval':       # the frozen discriminator of the generator phase
        for m in (net, drv):
            m.eval()
            for p in m.parameters():
                p.requires_grad = False
    x = _t(synth.uniform_input(5, (n, 3, size, size)), dev)
    wgt = _t(synth.uniform_input(6, (n, 1)), dev) - 0.5
    run = Run()
    run.config, run.net, run.drv, run.train = config, net, drv, net.training
    run.before = {k: v.clone() for k, v in net.named_buffers()}
    run.xd = x.clone().requires_grad_(True)
    run.out_d = drv(run.xd)
    (run.out_d * wgt).sum().backward()
    rec = W.Recorder()
    with pytest.MonkeyPatch.context() as mp:
        rec.install(mp, TABLE)
        run.xr = x.clone().requires_grad_(True)
        run.out_r = net.forward_layers(run.xr)
        (run.out_r * wgt).sum().backward()
    run.rec = rec.finish()
    names = {id(p): k.rsplit('.', 1)[0] for k, p in net.named_parameters()}
    for r in rec.records:
        r.tag = next((names[id(a)] for a in r.args if id(a) in names), '')
    return run


def _vgg_run(dev, config):
    net = ira.build_network(dict(type='VGGFeatureExtractor', layer_name_list=TAPS, vgg_type='vgg19', compute_dtype='bf16',
                                 allow_random_init=True)).to(dev)
    x = _t(synth.uniform_input(5, (2, 3, 32, 48)), dev)
    run = Run()
    run.config, run.net, run.train = config, net, False
    run.xd = x.clone().requires_grad_(True)
    run.feats_d = net(run.xd)
    ups = [_t(synth.gaussian(10 + i, tuple(run.feats_d[k].shape)), dev) for i, k in enumerate(TAPS)]   # random upstream gradients, no loss
    torch.autograd.backward([run.feats_d[k] for k in TAPS], ups)
    rec = W.Recorder()
    with pytest.MonkeyPatch.context() as mp:
        rec.install(mp, TABLE)
        run.xr = x.clone().requires_grad_(True)
        run.feats_r = net(run.xr)
        torch.autograd.backward([run.feats_r[k] for k in TAPS], ups)
    run.rec = rec.finish()
    names = {id(p): k.rsplit('.', 1)[0].split('.')[-1] for k, p in net.named_parameters()}
    for r in rec.records:
        r.tag = next((names[id(a)] for a in r.args if id(a) in names), '')
    return run


def _run(dev, config):
    if config not in _RUNS:
        run = (_vgg_run if config == 'vgg19' else _disc_run)(dev, config)
        run.replays = {}
        _RUNS[config] = run
    return _RUNS[config]


def _replay(run, i):
    if i not in run.replays:
        run.replays[i] = W.Replay(run.rec.records[i])
    return run.replays[i]


def _ops(run, name):
    return [(i, r) for i, r in enumerate(run.rec.records) if r.name == name]


# ------------------------------------------------------------------------------------------------------------------------ anchors
@pytest.mark.parametrize('config', CONFIGS)
def test_the_recorder_observes_the_production_forward(cuda, config):
    """Bit for bit: logits (features), input gradient, parameter gradients and buffers of the recorded per-layer run equal the plain
    ``net(x)`` — the whole-network driver for the discriminators, the unpatched forward for the feature extractor."""
    run = _run(cuda, config)
    census = {}
    for r in run.rec.records:
        census[r.name] = census.get(r.name, 0) + 1
    if config == 'vgg19':
        assert list(run.feats_r) == TAPS
        for k in TAPS:
            assert torch.equal(run.feats_r[k], run.feats_d[k]), k
        assert torch.equal(run.xr.grad, run.xd.grad)
        assert census == {'ChannelAffineFn': 1, 'ToCB16': 1, 'ConvFn16': 16, 'LReLUFn16': 1, 'MaxPool2x2Fn16': 4, 'FromCB16': 4}, census
        return
    stages = 5 if config.startswith('d256') else 4
    assert census == {'ToCB16': 1, 'ConvFn16': 2 + 2 * stages, 'BNLReLUFn16': 1 + 2 * stages, 'FromCB16': 1, 'LinearFn': 2}, census
    assert torch.equal(run.out_r, run.out_d) and torch.equal(run.xr.grad, run.xd.grad)
    for (k, p), (_, q) in zip(run.net.named_parameters(), run.drv.named_parameters()):
        if run.train:
            assert p.grad is not None and torch.equal(p.grad, q.grad), k
        else:
            assert p.grad is None and q.grad is None, k
    for (k, a), (_, b) in zip(run.net.named_buffers(), run.drv.named_buffers()):
        assert torch.equal(a, b), k
        if k.endswith('num_batches_tracked'):
            assert int(a) == int(run.before[k]) + (1 if run.train else 0), k
        elif not run.train:
            assert torch.equal(a, run.before[k]), f'{k}: eval mode moved a running buffer'


@pytest.mark.parametrize('config', CONFIGS)
def test_every_replay_reproduces_its_recorded_op(cuda, config):
    """One ``apply`` on fresh leaf copies of the recorded inputs (train-mode BatchNorm on clones of the running buffers as they were):
    same output bits, same buffers afterwards, and the recorded ``.grad`` of every input that has a single consumer."""
    run = _run(cuda, config)
    skipped = []
    for i, r in enumerate(run.rec.records):
        rep = _replay(run, i)
        compared = W.assert_replay_reproduces(run.rec, r, rep)
        assert r.gy is not None and rep.grads, f'{r}: no gradient reached this op'
        if compared != len(rep.grads):
            skipped.append(repr(r))
    if config == 'vgg19':
        # relu1_1, pool1 and conv3_4 have two consumers each (FromCB16 and the next op); autograd's bf16 sum of their gradients is
        # torch's own.  conv5_4 is the last layer: FromCB16 is its only consumer
        assert len(skipped) == 2 * 3, skipped
    else:
        assert not skipped, skipped


# --------------------------------------------------------------------------------------------------------------------- convolution
def _conv_reference(rec, rep, mutate=None):
    """{what: (got, want, bound)} of one ConvFn16 op: forward, data gradient, weight and bias gradients (those the replay produced)."""
    x, wt, bias, slope, out_nchw = rec.vals[:5]
    assert not out_nchw and all(v in (False, 1.0, None) for v in rec.vals[5:])
    cout, cin, k, _ = wt.shape
    stride = 2 if k == 4 else 1
    slope32 = _f32(slope)
    x64 = cb16_to_nchw(x, cin)
    w64 = wt.detach().cpu().double() if mutate == 'fp32_weights' else bf(wt.detach().cpu())
    if mutate == 'shift_taps' and k == 4:
        w64 = torch.roll(w64, 1, dims=3)
    b64 = bias.detach().cpu().double() if bias is not None else None
    pre = F.conv2d(x64, w64, b64, stride, 1)
    y64 = torch.where(pre > 0, pre, slope32 * pre)
    Ay = F.conv2d(x64.abs(), w64.abs(), b64.abs() if bias is not None else None, stride, 1)
    cin_k = 4 * cin if k == 4 else (cin + 15) // 16 * 16
    E = (2 * 9 * cin_k + 8) * EPS * Ay + EPS * y64.abs()
    y = cb16_to_nchw(rep.out)
    assert y.size(1) == cout
    res = {'fwd': (y, y64, E + hulp(y64.abs() + E))}
    g = cb16_to_nchw(rec.gy)
    if slope != 1.0:
        msrc = g if mutate == 'mask_from_gy' else y
        dz = torch.where(msrc > 0, g, bf(g.float() * torch.tensor(slope, dtype=torch.float32)))
    else:
        dz = g
    if 0 in rep.grads:
        dx = cb16_to_nchw(rep.grads[0])
        assert bool((dx[:, cin:] == 0).all()), f'{rec}: pad channels of dx are not zero'
        dx64 = F.conv_transpose2d(dz, w64, None, stride, 1)
        Ad = F.conv_transpose2d(dz.abs(), w64.abs(), None, stride, 1)
        E = (2 * 9 * ((cout + 15) // 16 * 16) + 8) * EPS * Ad + EPS * dx64.abs()
        res['dx'] = (dx[:, :cin], dx64, E + hulp(dx64.abs() + E))
    n, _, ho, wo = dz.shape
    kw = 2 * n * ho * wo + 3
    if 1 in rep.grads:
        dw64 = torch.nn.grad.conv2d_weight(x64, wt.shape, dz, stride, 1)
        Aw = torch.nn.grad.conv2d_weight(x64.abs(), wt.shape, dz.abs(), stride, 1)
        res['dw'] = (rep.grads[1].cpu().double(), dw64, kw * EPS * Aw + EPS * dw64.abs())
    if 2 in rep.grads:
        db64 = dz.sum((0, 2, 3))
        res['db'] = (rep.grads[2].cpu().double(), db64, kw * EPS * dz.abs().sum((0, 2, 3)) + EPS * db64.abs())
    return res


@pytest.mark.parametrize('config', CONFIGS)
def test_convolutions(cuda, config):
    """Every ConvFn16 op of the network: 3x3 and 4x4 / s2, with and without bias, slope 0.2 / 1.0 / 0.0."""
    run = _run(cuda, config)
    seen = set()
    for i, r in _ops(run, 'ConvFn16'):
        k, slope, has_bias = r.vals[1].size(2), r.vals[3], r.vals[2] is not None
        seen.add((k, slope, has_bias))
        res = _conv_reference(r, _replay(run, i))
        assert 'dx' in res and (('dw' in res) == run.train) and (('db' in res) == (run.train and has_bias))
        for what, (got, want, bound) in res.items():
            _note(config, f'conv{k}x{k} {what}', check(got, want, bound, f'{config} {r} {what}'))
    if config == 'vgg19':
        assert seen == {(3, 0.0, True), (3, 1.0, True)}, seen
    else:
        assert seen == {(3, 0.2, True), (3, 1.0, False), (4, 1.0, False)}, seen
        cins = sorted(r.vals[1].size(1) for _, r in _ops(run, 'ConvFn16') if r.vals[1].size(2) == 4)
        assert {c % 64 == 0 for c in cins} == {True, False}, cins   # both sides of the zero-tap-skipping branch (s2_channels)
    _report(config)


# ------------------------------------------------------------------------------------------------------------ BatchNorm + LeakyReLU
def _bn_reference(rec, rep, mutate=None, general=False):
    """{what: (got, want, bound)} of one BNLReLUFn16 op (module docstring)."""
    x, gamma, beta, rm, rv, train, momentum, eps, slope = rec.vals
    assert momentum == 0.1 and slope == 0.2
    c = gamma.numel()
    z = cb16_to_nchw(x, c)
    n, _, h, w = z.shape
    M = n * h * w
    K = (-(-M // 8192) + 73 if general else -(-M // 1024) + 22) + 6
    assert general or M <= 32768
    v4 = lambda t: t.view(1, c, 1, 1)  # noqa: E731
    g64, b64 = gamma.detach().cpu().double(), beta.detach().cpu().double()
    rm64, rv64 = rm.cpu().double(), rv.cpu().double()
    eps32 = 1e-3 if mutate == 'eps' else _f32(eps)
    slope32 = _f32(slope)
    if train:
        mu, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
        dmu = K * EPS * z.abs().sum((0, 2, 3)) / M
        dvar = K * EPS * var + dmu ** 2
    else:
        mu, var = rm64, rv64
        dmu = dvar = torch.zeros(c, dtype=torch.float64)
    inv = 1.0 / torch.sqrt(var + eps32)
    ris = 0.5 * dvar / (var + eps32) + 3 * EPS
    d = z - v4(mu)
    xhat = d * v4(inv)
    pre = v4(g64) * xhat + v4(b64)
    y64 = torch.where(pre > 0, pre, slope32 * pre)
    dxhat = v4(inv) * (d.abs() * v4(ris) + v4(dmu))
    E = v4(g64.abs()) * dxhat + 5 * EPS * ((v4(g64) * xhat).abs() + v4(b64.abs()))
    a = cb16_to_nchw(rep.out)
    assert a.size(1) == c
    res = {'fwd': (a, y64, E + hulp(y64.abs() + E))}
    rm_new, rv_new = rep.fresh[3].cpu().double(), rep.fresh[4].cpu().double()
    if train:
        unb = var if mutate == 'biased_var' else var * M / (M - 1)
        res['running_mean'] = (rm_new, 0.9 * rm64 + 0.1 * mu, 4 * EPS * (0.9 * rm64.abs() + 0.1 * mu.abs()) + 0.1 * dmu)
        res['running_var'] = (rv_new, 0.9 * rv64 + 0.1 * unb, 4 * EPS * (0.9 * rv64.abs() + 0.1 * unb) + 0.1 * dvar * M / (M - 1))
    else:
        assert torch.equal(rep.fresh[3], rm) and torch.equal(rep.fresh[4], rv), f'{rec}: eval mode moved a running buffer'
    gy = cb16_to_nchw(rec.gy)
    dz = torch.where((gy if mutate == 'mask_from_gy' else a) > 0, gy, gy * slope32)
    if train:
        dbeta, dgamma = dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3))
        e_db = K * EPS * dz.abs().sum((0, 2, 3))
        e_dg = K * EPS * (dz * xhat).abs().sum((0, 2, 3)) + (dz.abs() * dxhat).sum((0, 2, 3))
        t = dz if mutate == 'no_1_over_M' else dz - (v4(dbeta) + xhat * v4(dgamma)) / M
        dx64 = v4(g64 * inv) * t
        e_t = ((v4(e_db) + xhat.abs() * v4(e_dg) + v4(dgamma.abs()) * (dxhat + 2 * EPS * xhat.abs())) / M
               + 6 * EPS * (dz.abs() + (v4(dbeta.abs()) + (xhat * v4(dgamma)).abs()) / M))
        E = v4(g64.abs() * inv) * e_t + dx64.abs() * (v4(ris) + 2 * EPS)
        if 1 in rep.grads:
            res['dgamma'] = (rep.grads[1].cpu().double(), dgamma, e_dg)
            res['dbeta'] = (rep.grads[2].cpu().double(), dbeta, e_db)
    else:
        dx64 = v4(g64 * inv) * dz
        E = dx64.abs() * (v4(ris) + 3 * EPS)
    res['dx'] = (cb16_to_nchw(rep.grads[0]), dx64, E + hulp(dx64.abs() + E))
    return res, M


@pytest.mark.parametrize('config', DISC)
def test_batchnorm_lrelu(cuda, config):
    """Every BNLReLUFn16 op: output, running buffers, dx, dgamma, dbeta (train mode); output and dx from the running buffers, which
    stay as they are (eval mode)."""
    run = _run(cuda, config)
    Ms = []
    for i, r in _ops(run, 'BNLReLUFn16'):
        assert r.vals[5] == run.train
        res, M = _bn_reference(r, _replay(run, i))
        Ms.append(M)
        assert set(res) == ({'fwd', 'running_mean', 'running_var', 'dx', 'dgamma', 'dbeta'} if run.train else {'fwd', 'dx'})
        for what, (got, want, bound) in res.items():
            _note(config, f'bn {what}', check(got, want, bound, f'{config} {r} M={M} {what}'))
    assert (max(Ms), min(Ms)) == {'d128-n3': (12288, 48), 'd128-n2-moved': (8192, 32), 'd256-n2': (32768, 32), 'd128-eval': (8192, 32)}[config]
    _report(config)


def test_batchnorm_general_path(cuda):
    """The same recorded BatchNorm ops through the two-stage reduction kernels (the path of n h w > 32768) against the same bounds: the
    one-launch kernel is switched off for the replays."""
    run = _run(cuda, 'd128-n3')
    lib = _lib.load()
    lib.sr_dev_set_bn_small.argtypes = [C.c_int]
    lib.sr_dev_set_bn_small.restype = None
    lib.sr_dev_set_bn_small(0)
    try:
        reps = [(r, W.Replay(r)) for _, r in _ops(run, 'BNLReLUFn16')]
        torch.cuda.synchronize()
    finally:
        lib.sr_dev_set_bn_small(1)
    for r, rep in reps:
        res, M = _bn_reference(r, rep, general=True)
        for what, (got, want, bound) in res.items():
            _note('d128-n3 general', f'bn {what}', check(got, want, bound, f'general path {r} M={M} {what}'))
    _report('d128-n3 general')


# ---------------------------------------------------------------------------------------------------------------------- linear head
@pytest.mark.parametrize('config', DISC)
def test_linear_head(cuda, config):
    run = _run(cuda, config)
    for i, r in _ops(run, 'LinearFn'):
        rep = _replay(run, i)
        x, wt, bias, slope = r.vals
        X, Wt, b64 = x.cpu().double(), wt.detach().cpu().double(), bias.detach().cpu().double()
        nb, nin = X.shape
        nout = Wt.size(0)
        z = X @ Wt.T + b64
        y64 = torch.where(z > 0, z, z * _f32(slope))
        zabs = X.abs() @ Wt.abs().T + b64.abs()
        Y = rep.out.cpu()
        _note(config, 'linear fwd', check(Y.double(), y64, EPS * ((-(-nin // 256) + 11) * zabs + z.abs()), f'{config} {r} fwd'))
        gy = r.gy.cpu()
        DZ = torch.where(Y > 0, gy, gy * torch.tensor(slope, dtype=torch.float32)).double()   # the kernel's own branch, one fp32 product
        _note(config, 'linear dx', check(rep.grads[0].cpu().double(), DZ @ Wt, EPS * (nout + 1) * (DZ.abs() @ Wt.abs()), f'{config} {r} dx'))
        if run.train:
            _note(config, 'linear dw', check(rep.grads[1].cpu().double(), DZ.T @ X, EPS * (nb + 1) * (DZ.abs().T @ X.abs()), f'{config} {r} dw'))
            _note(config, 'linear db', check(rep.grads[2].cpu().double(), DZ.sum(0), EPS * (nb + 1) * DZ.abs().sum(0), f'{config} {r} db'))
    _report(config)


# ------------------------------------------------------------------------------------------------------------------ bit-exact ops
@pytest.mark.parametrize('config', CONFIGS)
def test_layout_activation_and_pooling_ops_are_exact(cuda, config):
    run = _run(cuda, config)
    counts = {}
    for i, r in enumerate(run.rec.records):
        if r.name in ('ConvFn16', 'BNLReLUFn16', 'LinearFn'):
            continue
        counts[r.name] = counts.get(r.name, 0) + 1
        rep = _replay(run, i)
        out, gx, gy = rep.out.cpu(), rep.grads[0].cpu(), r.gy.cpu()
        x = r.vals[0].cpu()
        if r.name == 'ToCB16':
            assert torch.equal(out, nchw_to_cb16(x.to(torch.bfloat16))), f'{r}: not x.to(bfloat16) in CB16'
            assert gx.dtype == torch.float32 and torch.equal(gx.double(), cb16_to_nchw(gy, x.size(1))), f'{r}: backward'
        elif r.name == 'FromCB16':
            ch = r.vals[1]
            assert out.dtype == torch.float32 and torch.equal(out.double(), cb16_to_nchw(x, ch)), f'{r}: forward'
            assert torch.equal(gx, nchw_to_cb16(gy.to(torch.bfloat16))) and gx.shape == x.shape, f'{r}: backward is not gy.to(bfloat16)'
        elif r.name == 'LReLUFn16':
            s = torch.tensor(r.vals[1], dtype=torch.float32)
            y = torch.where(x.float() > 0, x, (x.float() * s).bfloat16())
            assert torch.equal(out, y), f'{r}: forward'
            assert torch.equal(gx, torch.where(y.float() > 0, gy, (gy.float() * s).bfloat16())), f'{r}: backward'
        elif r.name == 'MaxPool2x2Fn16':
            xr = cb16_to_nchw(x).requires_grad_(True)
            yr = F.max_pool2d(xr, 2, 2)
            yr.backward(cb16_to_nchw(gy))
            assert torch.equal(cb16_to_nchw(out), yr.detach()), f'{r}: forward'
            assert torch.equal(cb16_to_nchw(gx), xr.grad), f'{r}: backward'
        elif r.name == 'ChannelAffineFn':
            a, b = r.vals[1].cpu().view(1, -1, 1, 1), r.vals[2].cpu().view(1, -1, 1, 1)
            assert torch.equal(out, x * a + b), f'{r}: forward'
            assert torch.equal(gx, gy * a), f'{r}: backward'
        else:
            raise AssertionError(f'unexpected op {r}')
    want = ({'ChannelAffineFn': 1, 'ToCB16': 1, 'LReLUFn16': 1, 'MaxPool2x2Fn16': 4, 'FromCB16': 4} if config == 'vgg19'
            else {'ToCB16': 1, 'FromCB16': 1})
    assert counts == want, counts


# --------------------------------------------------------------------------------------------------------------- negative controls
def _miss(res, what):
    got, want, bound = res[what]
    return worst(got, want, bound)


@pytest.mark.parametrize('control', ['bn_eps_1e-3', 'bn_dx_without_1_over_M', 'running_var_biased', 'conv4x4_taps_shifted',
                                     'conv_fp32_weights', 'lrelu_mask_from_gy'])
def test_negative_controls(cuda, control):
    """Mutated references under the same bounds on the 128 network (n = 3): the correct kernel output must miss each of them."""
    run = _run(cuda, 'd128-n3')
    bns, convs = _ops(run, 'BNLReLUFn16'), _ops(run, 'ConvFn16')
    ratios = {}
    if control == 'bn_eps_1e-3':
        for i, r in bns:
            ratios[r.tag] = _miss(_bn_reference(r, _replay(run, i), 'eps')[0], 'fwd')
        must = list(ratios)
    elif control == 'bn_dx_without_1_over_M':
        for i, r in bns:
            ratios[r.tag] = _miss(_bn_reference(r, _replay(run, i), 'no_1_over_M')[0], 'dx')
        must = list(ratios)
    elif control == 'running_var_biased':
        for i, r in bns:
            ratios[r.tag] = _miss(_bn_reference(r, _replay(run, i), 'biased_var')[0], 'running_var')
        must = list(ratios)         # 1 / (M - 1) is 8e-5 at bn0_1 (M = 12288) and about 2 % at bn4_1 (M = 48)
    elif control == 'conv4x4_taps_shifted':
        for i, r in convs:
            if r.vals[1].size(2) == 4:
                ratios[r.tag] = _miss(_conv_reference(r, _replay(run, i), 'shift_taps'), 'fwd')
        must = list(ratios)
        assert len(must) == 5
    elif control == 'conv_fp32_weights':
        # the weights' own rounding noise grows like sqrt(products) against a worst-case chain bound that grows like their number:
        # asserted at the four narrowest layers (27 to 288 products per output), printed for the rest
        for i, r in convs:
            ratios[r.tag] = _miss(_conv_reference(r, _replay(run, i), 'fp32_weights'), 'fwd')
        must = ['conv0_0', 'conv0_1', 'conv1_0', 'conv2_0']
    else:
        for i, r in bns:
            ratios[r.tag] = _miss(_bn_reference(r, _replay(run, i), 'mask_from_gy')[0], 'dx')
        i, r = convs[0]
        assert r.tag == 'conv0_0' and r.vals[3] == 0.2
        ratios[r.tag] = _miss(_conv_reference(r, _replay(run, i), 'mask_from_gy'), 'dx')
        must = list(ratios)
    for k, v in ratios.items():
        print(f'CONTROL {control:24s} {k:10s} got / bound = {v:.3g}{"" if k in must else "   (not asserted)"}')
    for k in must:
        assert ratios[k] > 1.0, f'{control} stays inside the bound at {k} ({ratios[k]:.3f}): the bound cannot see it'
