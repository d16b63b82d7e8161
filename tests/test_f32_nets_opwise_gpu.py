"""The fp32 discriminators and the fp32 VGG feature extractor op by op against float64, on the tensors the HIP networks themselves
produced: the fp32 counterpart of tests/test_vgg_bf16_opwise_gpu.py.

fp32 is the default compute_dtype of VGGStyleDiscriminator128 / 256, UNetDiscriminatorSN and VGGFeatureExtractor.  End to end they are
held only relative to each tensor's maximum (tests/test_training_gpu.py, tests/test_unet_disc_gpu.py), and the extractor's input
gradient at 3e-2 relative L2 because one ReLU unit within rounding of 0 may take the other branch than the float64 oracle
(tests/test_perceptual_gpu.py).  Here nothing compounds and no branch can flip: the recorder of tests/bf16_opwise.py (with the
several-output Function and the CB8 views of tests/f32_opwise.py) stands in for the autograd Functions the per-layer routes look up in
hip_autograd at call time, one production forward + backward leaves every op's inputs, output and upstream gradient, and each op is
replayed alone against float64 of that one op; every mask is the op's own recorded output.

Anchors, bit for bit: the recorded run equals the plain ``net(x)`` (the whole-network driver for the VGG discriminators, the unpatched
forward for the U-Net and the extractor) in outputs, input gradient, parameter gradients and buffers; every replay reproduces its
recorded output, the buffers it updates in place and the recorded gradient of every input with a single consumer.  The U-Net's skip
sources (x0, x1, x2: the next strided conv and AddFn) and the extractor's tapped features that feed on (relu1_1, pool1, conv3_4: FromCB8
and the next op) have exactly two consumers; autograd adds the two gradients in float32, and a + b = b + a in IEEE arithmetic, so the
recorded ``.grad`` must equal the float32 sum of the two replayed gradients whatever order autograd took.

Bounds are counts of roundings, nothing is fitted; every element of every tensor is checked.  EPS = 2^-24.  A is the same operation on
absolute values in float64.  The library builds with -ffp-contract=off: every product and sum is its own rounding.

  ConvFn forward     tests/test_conv_ops_gpu.py: |y - y64| <= k EPS A + EPS |y64|, two roundings per product of the MFMA chain over
                     (tap, channel), + 8 for the epilogue: k = 2 * 9 * cin_pad + 8 for 3x3 (cin_pad: the CB8 channels of the source),
                     k = 2 * 16 * cin_pad + 4 + 8 for the 4x4 / s2 forward (+ 4: its four parity passes meet in the destination).  The
                     reference of a 4x4 conv is F.conv2d(stride=2, padding=1) of the 4x4 weight.  y64 = act(conv64(x, w) + b) on the
                     recorded fp32 x, w, b.
  ConvFn data grad   dz is modelled exactly from the op's own output: gy where y > 0, else fp32(gy * slope) (sr_lrelu_bwd_f32: one
                     product), applied when act_slope != 1.  dx64 = conv_transpose64(dz, w); k = 2 * 9 * roundup8(cout) + 8 for 3x3
                     and, by test_conv4x4s2_f32_dgrad's rule, k = 2 * 4 * roundup8(cout) + 8 for 4x4 / s2 (one parity pass per element:
                     four taps).  Pad channels of dx (3 real of 8 at the first conv) are zero.
  ConvFn weight, bias grad   the order-independent rule of test_conv_ops_gpu.py: any order of summing N products loses at most N - 1
                     roundings, two per MFMA product: k = 2 n H W + 3 over the gradient grid.
  BNLReLUFn, train   the derivation of tests/test_vgg_bf16_opwise_gpu.py's docstring (dmu, dvar = K EPS var + dmu^2, ris, E_bn,
                     running_mean, running_var, dbeta, dgamma, dx), written out once in f32_opwise.bn_train_reference, without the
                     hulp(...) store terms: an fp32 store rounds nothing that is not already counted.  K = L + 6, L restated from the fp32
                     kernels (f32_opwise.bn_tree_depth): bn_small.h (n h w <= 32768) walks ceil(M / 1024) pixels per thread, then 6
                     shuffle steps, then 16 wave results in order: L = ceil(M / 1024) + 22; train_ops.hip's two-stage path has a thread
                     stride of 128 * RED_SPLITS = 8192 pixels, 6 shuffle steps, 3 adds in block_sum and 64 partials in order in
                     bn_finalize_kernel: L = ceil(M / 8192) + 73.  Both restated counts were compared with the code and agree with it.
                     num_batches_tracked is exactly one more.
  BNLReLUFn, eval    the header of tests/test_layout_ops_gpu.py: forward 8 EPS (|xhat gamma| + |beta|) + EPS |y64|; dx = gamma invstd dz
                     within 7 EPS |dx64| + EPS |dx64|; the running buffers stay as they are.
  LinearFn           tests/test_train_ops_gpu.py::test_linear: y within EPS ((ceil(nin / 256) + 11) |x| |w|^T + |z|); dz exactly from
                     the kernel's own y; dx within EPS (nout + 1) |dz| |w|, dw within EPS (n + 1) |dz|^T |x|, db within EPS (n + 1) sum|dz|.
  Bilinear2xFn       test_train_ops_gpu.py::test_bilinear2x: forward within 6 EPS interp(|x|) of F.interpolate(scale_factor=2,
                     mode='bilinear', align_corners=False) in float64, backward within 20 EPS adjoint(|g|) of its autograd adjoint.
  SpectralNormBatchFn   recorded and replayed for the anchors; its arithmetic is pinned in test_train_ops_gpu.py::test_spectral_norm_*.
                     Here: the weights conv1 .. conv8 received are its outputs, the very tensors.
  AddFn, LReLUFn, MaxPool2x2Fn, ToCB8, FromCB8, ChannelAffineFn   bit-exact against a torch float32 emulation on the recorded values
                     (a selection, a movement, one product, or one product and one add).  Max-pool backward: the first maximum in scan
                     order takes the gradient (torch's rule, tests/test_layout_ops_gpu.py).  The extractor's normalisation is also held
                     against ((x + 1) / 2 - mean) / std in float64 from the constants themselves: a = fp32(0.5 / fp32(std)) is within 2
                     EPS, b = fp32(fp32(0.5 - fp32(mean)) / fp32(std)) within EPS |mean| / std + 3 EPS |b|, y = fp32(fp32(x a) + b) adds
                     two roundings: |y - y64| <= 4 EPS |x a| + 4 EPS |b| + EPS |mean| / std + EPS |y64| (one per term for the second order).

Which BatchNorm kernel runs is proven with the launch profiler (ids 161 / 162: bn_small.h forward / backward; 163: bn_reduce_kernel +
bn_finalize_kernel; 164 / 165: the two-stage path's apply kernels) on the whole-network driver: bn0_1 and bn1_0 of d128-n9 (both on
the 64 x 64 map, M = 36864) take the two-stage kernels, those of d256-n2 (M = 32768, the threshold itself) the one-launch kernel.
test_batchnorm_general_path replays every recorded train-mode BatchNorm with the one-launch kernel switched off, against the bounds of
the two-stage tree.

Negative controls (test_negative_controls): mutated references that the kernel's output must MISS under the same bounds.
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
from image_restoration_amd.utils import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_opwise as W  # noqa: E402
from f32_opwise import EPS, bn_train_reference, bn_tree_depth, cb8_to_nchw, check, nchw_to_cb8, worst  # noqa: E402

pytestmark = pytest.mark.gpu

TABLE = {A: ('ConvFn', 'BNLReLUFn', 'LinearFn', 'ToCB8', 'FromCB8', 'LReLUFn', 'MaxPool2x2Fn', 'ChannelAffineFn', 'Bilinear2xFn', 'AddFn',
             'SpectralNormBatchFn')}
DISC_TRAIN = ['d128-n3', 'd128-n9', 'd128-n2-moved', 'd256-n2']
DISC = DISC_TRAIN + ['d128-eval']
UNET = ['unet-skip', 'unet-noskip', 'unet-eval']
CONFIGS = DISC + UNET + ['vgg19']
TAPS = ['relu1_1', 'pool1', 'conv3_4', 'conv5_4']
VGG_MEAN, VGG_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BN_IDS = {161, 162, 163, 164, 165}
WORST = {}


def _f32(v):
    return float(np.float32(v))


def _note(config, what, ratio):
    key = (config, what)
    WORST[key] = max(WORST.get(key, 0.0), ratio)


def _report(config):
    for (cfg, what), r in sorted(WORST.items()):
        if cfg == config:
            print(f'WORST {cfg:16s} {what:24s} got / bound = {r:.3f}')


# ------------------------------------------------------------------------------------------------------------------ recorded runs
class Run:
    pass


_RUNS = {}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _record(run, net, x, forward, backward):
    """One recorded forward + backward of ``net``; tags every record with the parameter (or normalised weight) it carries."""
    rec = W.Recorder()
    with pytest.MonkeyPatch.context() as mp:
        rec.install(mp, TABLE)
        run.xr = x.clone().requires_grad_(True)
        run.out_r = forward(net, run.xr)
        backward(run.out_r)
    run.rec = rec.finish()
    names = {id(p): k.rsplit('.', 1)[0].split('.')[-1] for k, p in net.named_parameters()}
    for r in rec.records:
        if r.name == 'SpectralNormBatchFn':
            names.update({id(o): f'conv{i + 1}' for i, o in enumerate(r.out)})
    for r in rec.records:
        r.tag = next((names[id(a)] for a in r.args if id(a) in names), '')


def _freeze(*nets):
    for m in nets:
        m.eval()
        for p in m.parameters():
            p.requires_grad = False


def _disc_run(dev, config):
    kind = 'VGGStyleDiscriminator256' if config.startswith('d256') else 'VGGStyleDiscriminator128'
    size = 256 if kind.endswith('256') else 128
    n = {'d128-n3': 3, 'd128-eval': 3, 'd128-n9': 9}.get(config, 2)
    net = ira.build_network(dict(type=kind, num_in_ch=3, num_feat=8)).to(dev)
    assert net.compute_dtype == 'fp32'
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.vgg128_state_dict(61, 3, 8, size).items()}, strict=True)
    net.train()
    drv = copy.deepcopy(net)
    if config == 'd128-n2-moved':   # running buffers that have already moved: two train-mode forwards on other inputs
        for seed in (7, 8):
            xs = _t(synth.uniform_input(seed, (n, 3, size, size)), dev)
            with torch.no_grad():
                net(xs), drv(xs)
    if config == 'd128-eval':       # the frozen discriminator of the generator phase
        _freeze(net, drv)
    x = _t(synth.uniform_input(5, (n, 3, size, size)), dev)
    wgt = _t(synth.uniform_input(6, (n, 1)), dev) - 0.5
    run = Run()
    run.config, run.net, run.drv, run.train = config, net, drv, net.training
    run.before = {k: v.clone() for k, v in net.named_buffers()}
    run.xd = x.clone().requires_grad_(True)
    run.out_d = drv(run.xd)
    (run.out_d * wgt).sum().backward()
    _record(run, net, x, lambda m, t: m.forward_layers(t), lambda o: (o * wgt).sum().backward())
    return run


def _unet_run(dev, config):
    torch.manual_seed(11)
    net = ira.build_network(dict(type='UNetDiscriminatorSN', num_in_ch=3, num_feat=8, skip_connection=config != 'unet-noskip')).to(dev)
    assert net.compute_dtype == 'fp32'
    net.train()
    drv = copy.deepcopy(net)
    if config == 'unet-eval':
        _freeze(net, drv)
    x = _t(synth.uniform_input(5, (2, 3, 16, 24)), dev)
    wgt = _t(synth.signed_input(6, (2, 1, 16, 24)), dev)
    run = Run()
    run.config, run.net, run.drv, run.train = config, net, drv, net.training
    run.before = {k: v.clone() for k, v in net.named_buffers()}
    run.xd = x.clone().requires_grad_(True)
    run.out_d = drv(run.xd)
    (run.out_d * wgt).sum().backward()
    _record(run, net, x, lambda m, t: m(t), lambda o: (o * wgt).sum().backward())
    return run


def _vgg_run(dev, config):
    net = ira.build_network(dict(type='VGGFeatureExtractor', layer_name_list=TAPS, vgg_type='vgg19', use_input_norm=True, range_norm=True,
                                 allow_random_init=True)).to(dev)
    assert net.compute_dtype == 'fp32'
    x = _t(synth.uniform_input(5, (2, 3, 36, 52)), dev) * 2 - 1
    run = Run()
    run.config, run.net, run.train = config, net, False
    run.xd = x.clone().requires_grad_(True)
    run.feats_d = net(run.xd)
    ups = [_t(synth.gaussian(10 + i, tuple(run.feats_d[k].shape)), dev) for i, k in enumerate(TAPS)]   # random upstream gradients, no loss
    torch.autograd.backward([run.feats_d[k] for k in TAPS], ups)
    _record(run, net, x, lambda m, t: m(t), lambda feats: torch.autograd.backward([feats[k] for k in TAPS], ups))
    run.feats_r = run.out_r
    return run


def _run(dev, config):
    if config not in _RUNS:
        run = (_vgg_run if config == 'vgg19' else _unet_run if config in UNET else _disc_run)(dev, config)
        run.replays = {}
        _RUNS[config] = run
    return _RUNS[config]


def _replay(run, i):
    if i not in run.replays:
        run.replays[i] = W.Replay(run.rec.records[i])
    return run.replays[i]


def _ops(run, name):
    return [(i, r) for i, r in enumerate(run.rec.records) if r.name == name]


def _census(run):
    census = {}
    for r in run.rec.records:
        census[r.name] = census.get(r.name, 0) + 1
    return census


def _want_census(config):
    if config == 'vgg19':
        return {'ChannelAffineFn': 1, 'ToCB8': 1, 'ConvFn': 16, 'LReLUFn': 1, 'MaxPool2x2Fn': 4, 'FromCB8': 4}
    if config in UNET:
        want = {'SpectralNormBatchFn': 1, 'ToCB8': 1, 'ConvFn': 10, 'Bilinear2xFn': 3, 'FromCB8': 1}
        if config != 'unet-noskip':
            want['AddFn'] = 3
        return want
    stages = 5 if config.startswith('d256') else 4
    return {'ToCB8': 1, 'ConvFn': 2 + 2 * stages, 'BNLReLUFn': 1 + 2 * stages, 'FromCB8': 1, 'LinearFn': 2}


# ------------------------------------------------------------------------------------------------------------------------ anchors
@pytest.mark.parametrize('config', CONFIGS)
def test_the_recorder_observes_the_production_forward(cuda, config):
    """Bit for bit: outputs, input gradient, parameter gradients and buffers of the recorded per-layer run equal the plain ``net(x)``:
    the whole-network driver for the VGG discriminators, the unpatched forward for the U-Net and the feature extractor."""
    run = _run(cuda, config)
    assert _census(run) == _want_census(config), _census(run)
    if config == 'vgg19':
        assert list(run.feats_r) == TAPS
        for k in TAPS:
            assert torch.equal(run.feats_r[k], run.feats_d[k]), k
        assert torch.equal(run.xr.grad, run.xd.grad)
        return
    assert torch.equal(run.out_r, run.out_d) and torch.equal(run.xr.grad, run.xd.grad)
    for (k, p), (_, q) in zip(run.net.named_parameters(), run.drv.named_parameters()):
        if run.train:
            assert p.grad is not None and torch.equal(p.grad, q.grad), k
        else:
            assert p.grad is None and q.grad is None, k
    moved = 0
    for (k, a), (_, b) in zip(run.net.named_buffers(), run.drv.named_buffers()):
        assert torch.equal(a, b), k
        if k.endswith('num_batches_tracked'):
            assert int(a) == int(run.before[k]) + (1 if run.train else 0), k
        elif not run.train:
            assert torch.equal(a, run.before[k]), f'{k}: eval mode moved a buffer'
        else:
            moved += int(not torch.equal(a, run.before[k]))
    if run.train:
        assert moved == sum(1 for k, _ in run.net.named_buffers() if not k.endswith('num_batches_tracked')), 'a buffer did not move'
    if config in UNET:
        # the weights conv1 .. conv8 received are the outputs of the one SpectralNormBatchFn call, the very tensors
        (_, sn), = _ops(run, 'SpectralNormBatchFn')
        assert sn.vals[0] == run.train and len(sn.out) == 8
        convs = [r for _, r in _ops(run, 'ConvFn')]
        assert [r.tag for r in convs] == [f'conv{i}' for i in range(10)]
        for i in range(1, 9):
            assert convs[i].args[1] is sn.out[i - 1], f'conv{i} did not receive the normalised weight {i - 1}'
            assert tuple(convs[i].args[1].shape) == tuple(getattr(run.net, f'conv{i}').weight_orig.shape)


@pytest.mark.parametrize('config', CONFIGS)
def test_every_replay_reproduces_its_recorded_op(cuda, config):
    """One ``apply`` on fresh leaf copies of the recorded inputs (train-mode BatchNorm and spectral norm on clones of their buffers as
    they were): same output bits, same buffers afterwards, the recorded ``.grad`` of every input that has a single consumer, and for
    the tensors with two consumers the float32 sum of the two replayed gradients."""
    run = _run(cuda, config)
    shared = {}
    for i, r in enumerate(run.rec.records):
        rep = _replay(run, i)
        _, several = W.assert_replay_reproduces(run.rec, r, rep)
        if r.name == 'SpectralNormBatchFn' and not run.train:
            assert r.gy is None and not rep.grads     # frozen: nothing flows to weight_orig
        else:
            assert r.gy is not None and rep.grads, f'{r}: no gradient reached this op'
        for j in several:
            shared[id(r.args[j])] = r.args[j]
    for t in shared.values():
        uses = run.rec.consumers(t)
        assert len(uses) == 2, uses
        (i0, j0), (i1, j1) = uses
        assert torch.equal(_replay(run, i0).grads[j0] + _replay(run, i1).grads[j1], t.grad), \
            f'{run.rec.records[i0]} / {run.rec.records[i1]}: the recorded gradient is not the sum of the two replayed ones'
    # vgg19: relu1_1, pool1, conv3_4 (conv5_4 is the last layer: FromCB8 is its only consumer); U-Net with skips: x0, x1, x2
    assert len(shared) == (3 if config in ('vgg19', 'unet-skip', 'unet-eval') else 0), len(shared)


# --------------------------------------------------------------------------------------------------------------------- convolution
def _r8(c):
    return (c + 7) // 8 * 8


def _conv_reference(rec, rep, mutate=None):
    """{what: (got, want, bound)} of one ConvFn op: forward, data gradient, weight and bias gradients (those the replay produced)."""
    x, wt, bias, slope = rec.vals
    cout, cin, k, _ = wt.shape
    stride = 2 if k == 4 else 1
    slope32 = _f32(slope)
    cin_pad = x.size(1) * 8
    assert cin_pad == _r8(cin)
    x64 = cb8_to_nchw(x, cin)
    w64 = wt.detach().cpu().double()
    if mutate == 'shift_taps' and k == 4:
        w64 = torch.roll(w64, 1, dims=3)
    b64 = bias.detach().cpu().double() if bias is not None else None
    pre = F.conv2d(x64, w64, b64, stride, 1)
    y64 = torch.where(pre > 0, pre, slope32 * pre)
    Ay = F.conv2d(x64.abs(), w64.abs(), b64.abs() if bias is not None else None, stride, 1)
    kf = 2 * 9 * cin_pad + 8 if k == 3 else 2 * 16 * cin_pad + 4 + 8
    yfull = cb8_to_nchw(rep.out)
    assert yfull.size(1) == _r8(cout) and bool((yfull[:, cout:] == 0).all()), f'{rec}: pad channels of y are not zero'
    y = yfull[:, :cout]
    res = {'fwd': (y, y64, kf * EPS * Ay + EPS * y64.abs())}
    g = cb8_to_nchw(rec.gy, cout)
    if slope != 1.0 and mutate != 'unmasked_gy':
        dz = torch.where(y > 0, g, (g.float() * torch.tensor(slope, dtype=torch.float32)).double())
    else:
        dz = g
    if 0 in rep.grads:
        dx = cb8_to_nchw(rep.grads[0])
        assert dx.size(1) == cin_pad and bool((dx[:, cin:] == 0).all()), f'{rec}: pad channels of dx are not zero'
        dx64 = F.conv_transpose2d(dz, w64, None, stride, 1)
        Ad = F.conv_transpose2d(dz.abs(), w64.abs(), None, stride, 1)
        kd = 2 * 9 * _r8(cout) + 8 if k == 3 else 2 * 4 * _r8(cout) + 8
        res['dx'] = (dx[:, :cin], dx64, kd * EPS * Ad + EPS * dx64.abs())
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
    """Every ConvFn op of the network: 3x3 and 4x4 / s2, with and without bias, slope 0.2 / 1.0 / 0.0, raw and spectrally normalised
    weights, 3 -> nf, nf -> 1 and every width between."""
    run = _run(cuda, config)
    seen = set()
    for i, r in _ops(run, 'ConvFn'):
        k, slope, has_bias = r.vals[1].size(2), r.vals[3], r.vals[2] is not None
        seen.add((k, slope, has_bias))
        res = _conv_reference(r, _replay(run, i))
        assert 'dx' in res and (('dw' in res) == run.train) and (('db' in res) == (run.train and has_bias))
        for what, (got, want, bound) in res.items():
            _note(config, f'conv{k}x{k} {what}', check(got, want, bound, f'{config} {r} {what}'))
    if config == 'vgg19':
        assert seen == {(3, 0.0, True), (3, 1.0, True)}, seen
    elif config in UNET:
        assert seen == {(3, 0.2, True), (3, 0.2, False), (4, 0.2, False), (3, 1.0, True)}, seen
        sizes = sorted({tuple(r.vals[0].shape[2:4]) for _, r in _ops(run, 'ConvFn')})
        assert sizes == [(4, 6), (8, 12), (16, 24)], sizes     # conv3 (4x4 / s2) writes 2 x 3
    else:
        assert seen == {(3, 0.2, True), (3, 1.0, False), (4, 1.0, False)}, seen
    _report(config)


# ------------------------------------------------------------------------------------------------------------ BatchNorm + LeakyReLU
def _bn_reference(rec, rep, mutate=None, general=None):
    """{what: (got, want, bound)} of one BNLReLUFn op (module docstring); ``general``: which reduction tree bounds it (default: the
    one the entry point picks for this size)."""
    x, gamma, beta, rm, rv, train, momentum, eps, slope = rec.vals
    assert momentum == 0.1 and slope == 0.2
    c = gamma.numel()
    z = cb8_to_nchw(x, c)
    n, _, h, w = z.shape
    M = n * h * w
    general = M > 32768 if general is None else general
    assert general or M <= 32768
    K = bn_tree_depth(M, general) + 6
    v4 = lambda t: t.view(1, c, 1, 1)  # noqa: E731
    g64, b64 = gamma.detach().cpu().double(), beta.detach().cpu().double()
    rm64, rv64 = rm.cpu().double(), rv.cpu().double()
    eps32, slope32 = _f32(eps), _f32(slope)
    afull = cb8_to_nchw(rep.out)
    assert afull.size(1) == _r8(c) and bool((afull[:, c:] == 0).all()), f'{rec}: pad channels of y are not zero'
    a = afull[:, :c]
    gy = cb8_to_nchw(rec.gy, c)
    dx = cb8_to_nchw(rep.grads[0])
    assert bool((dx[:, c:] == 0).all()), f'{rec}: pad channels of dx are not zero'
    dx = dx[:, :c]
    if train:
        ref = bn_train_reference(z, g64, b64, rm64, rv64, eps32, slope32, K, a, gy, mutate)
        got = {'fwd': a, 'running_mean': rep.fresh[3].cpu().double(), 'running_var': rep.fresh[4].cpu().double(), 'dx': dx}
        if 1 in rep.grads:
            got['dgamma'], got['dbeta'] = rep.grads[1].cpu().double(), rep.grads[2].cpu().double()
        return {k: (v,) + ref[k] for k, v in got.items()}, M
    assert torch.equal(rep.fresh[3], rm) and torch.equal(rep.fresh[4], rv), f'{rec}: eval mode moved a running buffer'
    inv = 1.0 / torch.sqrt(rv64 + eps32)
    xhat = (z - v4(rm64)) * v4(inv)
    pre = v4(g64) * xhat + v4(b64)
    y64 = torch.where(pre > 0, pre, slope32 * pre)
    S = (v4(g64) * xhat).abs() + v4(b64.abs())
    dz = torch.where(a > 0, gy, gy * slope32)
    dx64 = v4(g64 * inv) * dz
    return {'fwd': (a, y64, 8 * EPS * S + EPS * y64.abs()), 'dx': (dx, dx64, 8 * EPS * dx64.abs())}, M


BN_M = {'d128-n3': (12288, 48), 'd128-n9': (36864, 144), 'd128-n2-moved': (8192, 32), 'd256-n2': (32768, 32), 'd128-eval': (12288, 48)}


@pytest.mark.parametrize('config', DISC)
def test_batchnorm_lrelu(cuda, config):
    """Every BNLReLUFn op on the kernel the entry point picks: output, running buffers, dx, dgamma, dbeta (train mode); output and dx
    from the running buffers, which stay as they are (eval mode)."""
    run = _run(cuda, config)
    Ms = []
    for i, r in _ops(run, 'BNLReLUFn'):
        assert r.vals[5] == run.train
        res, M = _bn_reference(r, _replay(run, i))
        Ms.append(M)
        assert set(res) == ({'fwd', 'running_mean', 'running_var', 'dx', 'dgamma', 'dbeta'} if run.train else {'fwd', 'dx'})
        for what, (got, want, bound) in res.items():
            _note(config, f'bn {what}', check(got, want, bound, f'{config} {r} M={M} {what}'))
    assert (max(Ms), min(Ms)) == BN_M[config]
    # bn0_1 and bn1_0 both sit on the 64 x 64 map (conv1_0 is 3x3 / s1): at n = 9 these two are past the hand-over, nothing else is
    assert [M > 32768 for M in Ms] == [config == 'd128-n9'] * 2 + [False] * (len(Ms) - 2)
    _report(config)


@pytest.fixture
def general_path():
    """Switches the one-launch BatchNorm kernel off (development hook) and back on afterwards."""
    lib = _lib.load()
    lib.sr_dev_set_bn_small.argtypes = [C.c_int]
    lib.sr_dev_set_bn_small.restype = None
    lib.sr_dev_set_bn_small(0)
    yield lib
    torch.cuda.synchronize()
    lib.sr_dev_set_bn_small(1)


@pytest.mark.parametrize('config', DISC_TRAIN)
def test_batchnorm_general_path(cuda, config, general_path):
    """Every recorded train-mode BatchNorm through the two-stage reduction kernels (the path of n h w > 32768), against the bounds of
    that tree: the one-launch kernel is switched off for the replays."""
    run = _run(cuda, config)
    reps = [(r, W.Replay(r)) for _, r in _ops(run, 'BNLReLUFn')]
    torch.cuda.synchronize()
    for r, rep in reps:
        res, M = _bn_reference(r, rep, general=True)
        for what, (got, want, bound) in res.items():
            _note(f'{config} general', f'bn {what}', check(got, want, bound, f'general path {config} {r} M={M} {what}'))
    _report(f'{config} general')


def _profiled(lib, fn, cap=1024):
    """Runs fn() under the launch profiler; returns its records."""
    _lib.check(lib.sr_profile_start(cap), 'sr_profile_start')
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        recs = (_lib.LaunchRecord * cap)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, cap, C.byref(cnt)), 'sr_profile_stop')
    assert cnt.value < cap
    return [recs[i] for i in range(cnt.value)]


@pytest.mark.parametrize('config', ['d128-n9', 'd256-n2'])
def test_batchnorm_kernel_on_the_production_route(cuda, config):
    """The whole-network driver's forward + backward under the launch profiler: which BatchNorm kernels ran, in order.  n = 9 puts
    bn0_1 and bn1_0 (the 64 x 64 map, M = 36864) on the two-stage kernels and everything deeper on the one-launch kernel; the 256
    network at n = 2 has the two of them at M = 32768, the threshold itself, still on the one-launch kernel."""
    run = _run(cuda, config)
    lib = _lib.load()
    net = ira.build_network(dict(type=type(run.drv).__name__, num_in_ch=3, num_feat=8)).to(cuda)
    net.load_state_dict(run.drv.state_dict(), strict=True)
    net.train()
    x = run.xd.detach().clone().requires_grad_(True)

    def step():
        net(x).sum().backward()
    recs = [r for r in _profiled(lib, step) if r.kernel_id in BN_IDS]
    ids = [r.kernel_id for r in recs]
    nbn = _want_census(config)['BNLReLUFn']
    if config == 'd128-n9':
        assert ids == [163, 163, 164] * 2 + [161] * (nbn - 2) + [162] * (nbn - 2) + [163, 165] * 2, ids
        assert all(r.n * r.h * r.w == 36864 for r in recs if r.kernel_id in (163, 164, 165))
    else:
        assert ids == [161] * nbn + [162] * nbn, ids
        assert recs[0].n * recs[0].h * recs[0].w == 32768 and recs[-1].n * recs[-1].h * recs[-1].w == 32768
    assert max(r.n * r.h * r.w for r in recs if r.kernel_id in (161, 162)) <= 32768
    assert lib.sr_kernel_name(163).decode() == 'bn_reduce_kernel' and lib.sr_kernel_name(161).decode().startswith('bn_small_kernel')


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
        assert (1 in rep.grads) == run.train and (2 in rep.grads) == run.train
        if run.train:
            _note(config, 'linear dw', check(rep.grads[1].cpu().double(), DZ.T @ X, EPS * (nb + 1) * (DZ.abs().T @ X.abs()), f'{config} {r} dw'))
            _note(config, 'linear db', check(rep.grads[2].cpu().double(), DZ.sum(0), EPS * (nb + 1) * DZ.abs().sum(0), f'{config} {r} db'))
    _report(config)


# ----------------------------------------------------------------------------------------------------------------- bilinear x2
def _bilinear_reference(rec, rep, mutate=None):
    align = mutate == 'align_corners'
    x = cb8_to_nchw(rec.vals[0])
    xr = x.clone().requires_grad_(True)
    yr = F.interpolate(xr, scale_factor=2, mode='bilinear', align_corners=align)
    yabs = F.interpolate(x.abs(), scale_factor=2, mode='bilinear', align_corners=align)
    g = cb8_to_nchw(rec.gy)
    yr.backward(g)
    xa = x.clone().requires_grad_(True)
    F.interpolate(xa, scale_factor=2, mode='bilinear', align_corners=align).backward(g.abs())
    return {'fwd': (cb8_to_nchw(rep.out), yr.detach(), 6 * EPS * yabs), 'bwd': (cb8_to_nchw(rep.grads[0]), xr.grad, 20 * EPS * xa.grad)}


@pytest.mark.parametrize('config', UNET)
def test_bilinear2x(cuda, config):
    run = _run(cuda, config)
    sizes = []
    for i, r in _ops(run, 'Bilinear2xFn'):
        sizes.append(tuple(r.vals[0].shape[2:4]))
        for what, (got, want, bound) in _bilinear_reference(r, _replay(run, i)).items():
            _note(config, f'bilinear2x {what}', check(got, want, bound, f'{config} {r} {sizes[-1]} {what}'))
    assert sizes == [(2, 3), (4, 6), (8, 12)], sizes
    _report(config)


# ------------------------------------------------------------------------------------------------------------------ bit-exact ops
def _affine_reference(rec, rep, mutate=None):
    """The extractor's input normalisation against ((x + 1) / 2 - mean) / std from the constants themselves (module docstring)."""
    x = rec.vals[0].cpu().double()
    mean, std = torch.tensor(VGG_MEAN, dtype=torch.float64), torch.tensor(VGG_STD, dtype=torch.float64)
    if mutate == 'swap_mean_std':
        mean, std = std, mean
    a, b = (0.5 / std).view(1, 3, 1, 1), ((0.5 - mean) / std).view(1, 3, 1, 1)
    y64 = x * a + b
    bound = 4 * EPS * (x * a).abs() + 4 * EPS * b.abs() + EPS * (mean / std).abs().view(1, 3, 1, 1) + EPS * y64.abs()
    return rep.out.cpu().double(), y64, bound


@pytest.mark.parametrize('config', CONFIGS)
def test_layout_activation_pooling_and_add_ops_are_exact(cuda, config):
    run = _run(cuda, config)
    counts = {}
    f32 = torch.float32
    for i, r in enumerate(run.rec.records):
        if r.name in ('ConvFn', 'BNLReLUFn', 'LinearFn', 'Bilinear2xFn', 'SpectralNormBatchFn'):
            continue
        counts[r.name] = counts.get(r.name, 0) + 1
        rep = _replay(run, i)
        out, gx, gy = rep.out.cpu(), rep.grads[0].cpu(), r.gy.cpu()
        x = r.vals[0].cpu()
        assert out.dtype == f32 and gx.dtype == f32 and gx.shape == x.shape
        if r.name == 'ToCB8':
            assert torch.equal(out, nchw_to_cb8(x)), f'{r}: forward is not x in CB8 with zero pad channels'
            assert torch.equal(gx.double(), cb8_to_nchw(gy, x.size(1))), f'{r}: backward'
        elif r.name == 'FromCB8':
            assert torch.equal(out.double(), cb8_to_nchw(x, r.vals[1])), f'{r}: forward'
            assert torch.equal(gx, nchw_to_cb8(gy)), f'{r}: backward is not gy in CB8 with zero pad channels'
        elif r.name == 'LReLUFn':
            s = torch.tensor(r.vals[1], dtype=f32)
            y = torch.where(x > 0, x, x * s)
            assert torch.equal(out, y), f'{r}: forward'
            assert torch.equal(gx, torch.where(y > 0, gy, gy * s)), f'{r}: backward'
        elif r.name == 'MaxPool2x2Fn':
            xr = cb8_to_nchw(x).requires_grad_(True)
            yr = F.max_pool2d(xr, 2, 2)
            yr.backward(cb8_to_nchw(gy))
            assert torch.equal(cb8_to_nchw(out), yr.detach()), f'{r}: forward'
            assert torch.equal(cb8_to_nchw(gx), xr.grad), f'{r}: backward'
        elif r.name == 'ChannelAffineFn':
            a, b = r.vals[1].cpu().view(1, -1, 1, 1), r.vals[2].cpu().view(1, -1, 1, 1)
            assert torch.equal(out, x * a + b), f'{r}: forward'
            assert torch.equal(gx, gy * a), f'{r}: backward'
            _note(config, 'input norm fwd', check(*_affine_reference(r, rep), f'{config} {r} against the constants'))
        elif r.name == 'AddFn':
            assert torch.equal(out, x + r.vals[1].cpu()), f'{r}: forward'
            assert torch.equal(gx, gy) and torch.equal(rep.grads[1].cpu(), gy), f'{r}: backward'
        else:
            raise AssertionError(f'unexpected op {r}')
    want = {k: v for k, v in _want_census(config).items() if k not in ('ConvFn', 'BNLReLUFn', 'LinearFn', 'Bilinear2xFn', 'SpectralNormBatchFn')}
    assert counts == want, counts
    if config == 'vgg19':
        pools = [tuple(r.vals[0].shape[2:4]) for _, r in _ops(run, 'MaxPool2x2Fn')]
        assert pools == [(36, 52), (18, 26), (9, 13), (4, 6)], pools    # 9 x 13 -> 4 x 6: the odd row and column take no gradient
        _report(config)


# --------------------------------------------------------------------------------------------------------------- negative controls
def _miss(res, what):
    got, want, bound = res[what]
    return worst(got, want, bound)


@pytest.mark.parametrize('control', ['bn_eps_1e-3', 'bn_dx_without_1_over_M', 'running_var_biased', 'conv4x4_taps_shifted',
                                     'unet_without_skip_add', 'bilinear_align_corners', 'vgg_norm_mean_std_swapped',
                                     'conv_dx_from_unmasked_gy'])
def test_negative_controls(cuda, control):
    """Mutated references under the same bounds: the correct kernel output must miss each of them."""
    ratios = {}
    if control in ('bn_eps_1e-3', 'bn_dx_without_1_over_M', 'running_var_biased'):
        run = _run(cuda, 'd128-n3')
        mutate, what = {'bn_eps_1e-3': ('eps', 'fwd'), 'bn_dx_without_1_over_M': ('no_1_over_M', 'dx'),
                        'running_var_biased': ('biased_var', 'running_var')}[control]
        for i, r in _ops(run, 'BNLReLUFn'):     # 1 / (M - 1) is 8e-5 at bn0_1 (M = 12288) and about 2 % at bn4_1 (M = 48)
            ratios[r.tag] = _miss(_bn_reference(r, _replay(run, i), mutate)[0], what)
        assert len(ratios) == 9
    elif control == 'conv4x4_taps_shifted':
        for config in ('d128-n3', 'unet-skip'):
            run = _run(cuda, config)
            for i, r in _ops(run, 'ConvFn'):
                if r.vals[1].size(2) == 4:
                    ratios[f'{config} {r.tag}'] = _miss(_conv_reference(r, _replay(run, i), 'shift_taps'), 'fwd')
        assert len(ratios) == 5 + 3
    elif control == 'unet_without_skip_add':
        run = _run(cuda, 'unet-skip')
        for i, r in _ops(run, 'AddFn'):         # bit-exact op: the bound is zero
            out = _replay(run, i).out.cpu().double()
            ratios[f'add {tuple(out.shape[2:4])}'] = worst(out, r.vals[0].cpu().double(), torch.zeros_like(out))
        assert len(ratios) == 3
    elif control == 'bilinear_align_corners':
        run = _run(cuda, 'unet-skip')
        for i, r in _ops(run, 'Bilinear2xFn'):
            res = _bilinear_reference(r, _replay(run, i), 'align_corners')
            ratios[f'{tuple(r.vals[0].shape[2:4])} fwd'], ratios[f'{tuple(r.vals[0].shape[2:4])} bwd'] = _miss(res, 'fwd'), _miss(res, 'bwd')
        assert len(ratios) == 6
    elif control == 'vgg_norm_mean_std_swapped':
        run = _run(cuda, 'vgg19')
        (i, r), = _ops(run, 'ChannelAffineFn')
        ratios['norm'] = worst(*_affine_reference(r, _replay(run, i), 'swap_mean_std'))
    else:
        for config in ('d128-n3', 'unet-skip', 'vgg19'):
            run = _run(cuda, config)
            for i, r in _ops(run, 'ConvFn'):
                if r.vals[3] != 1.0:
                    ratios[f'{config} {r.tag}'] = _miss(_conv_reference(r, _replay(run, i), 'unmasked_gy'), 'dx')
        assert len(ratios) == 1 + 9 + 14
    for k, v in ratios.items():
        print(f'CONTROL {control:28s} {k:22s} got / bound = {v:.3g}')
    for k, v in ratios.items():
        assert v > 1.0, f'{control} stays inside the bound at {k} ({v:.3f}): the bound cannot see it'
