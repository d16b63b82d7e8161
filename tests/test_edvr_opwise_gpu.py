"""The fp32 EDVR op by op against float64, on the tensors the HIP network itself produced: what tests/test_f32_nets_opwise_gpu.py does
for the discriminators, for the largest network that trains through per-layer autograd Functions.

End to end EDVR is held as one relative L2 number per tensor (tests/test_edvr_gpu.py, tests/test_pcd_gpu.py), at batch 1.  Here nothing
compounds and no branch can flip: the recorder of tests/edvr_opwise.py stands in for every Function of the fp32 route (those looked up in
hip_autograd at call time and the five ``edvr_arch._CB8Ops`` binds when the class is created), one production forward + backward (eval
mode without no_grad, a random fp32 upstream gradient) leaves every op's inputs, output and upstream gradient, and each op is replayed
alone against float64 of that one op on the recorded fp32 values; every LeakyReLU / ReLU mask is the op's own recorded output; every
element of every tensor is checked.

Configurations (tests/edvr_opwise.py::CONFIGS; num_extract_block = num_reconstruct_block = 1):
  tsa-b2            nf 64, dg 8, 3 frames, (2, 3, 3, 12, 36): the copy path of center_over_t and the sum over t at b = 2; level 1 wider
                    than one 32-column strip; a 3 x 9 level 3; partial row tiles on every level; DCNFn with windows; 192 -> 64 1x1 convs
  predeblur-hr-b1   + with_predeblur, hr_in, (1, 3, 3, 32, 48), frames N(0, 0.1^2): the stride-0 view path; four more ConvS2Fn; the
                    resblock ``extra`` additions; the AddFn(out, x_center) exit
  nf16-dg2-notsa    nf 16, dg 2, 5 frames, no TSA, (2, 5, 3, 8, 12): the split-by-copy DCN route (non-contiguous NCHW slices through
                    FromCB8 / ToCB8, DCNFn without windows), one CB8 block per deformable group, the 1x1 fusion over t * 16 channels
Weights as tests/test_edvr_gpu.py::_state_dict draws them.  Seeds: for each configuration the seeds 20, 21, ... of the weights (the
input's is one more) were tried in that order with the float64 restatement tests/edvr_restate.py on the CPU, never with the code under
test, and the first kept whose level-1 offsets of the first frame have a mean |offset| in [0.5, 3] px and at least 1 % of the samples
outside the image: tsa-b2 20 (0.926 px, 6.0 %), nf16-dg2-notsa 20 (0.828 px, 11.1 %), predeblur-hr-b1 22 (2.532 px, 40.7 %; 20 and 21
give 4.5 and 5.7 px).  test_the_case_deforms asserts both conditions; tests/test_edvr_opwise_host.py repeats the search.

Anchors, bit for bit: the recorded run equals the unpatched ``net(x)`` + backward in the output and in every gradient that no
atomicAdd reaches (below); every replay reproduces its recorded output (BilinearUpFn from the pre-call value of ``acc``) and the recorded
gradient of every argument with a single consumer.  sr_dcn_bwd_data_f32 forms dx by atomicAdd, the one result of this route whose last
bits depend on arrival order (tests/test_dcn_ops_gpu.py::test_reproducibility exempts it for that reason), so two backward passes need
not agree bit for bit in what lies upstream of a deformable conv's dx: the input gradient and the parameters of everything before the
cascade's DCN.  Those gradients are held, for BOTH runs, by the 10x rule against float64 (test_whole_network), and op by op here.

Bounds are counts of roundings from the kernel's operation order, taken from the test that derives them; nothing is fitted.  EPS =
2^-24, A is the same operation on absolute values in float64, every bound also carries EPS |reference| unless noted.
  ConvFn            tests/test_f32_nets_opwise_gpu.py / tests/test_conv_ops_gpu.py: forward k = 2 * 9 cin_pad + 8, data gradient
                    k = 2 * 9 roundup8(cout) + 8 on dz formed exactly as sr_lrelu_bwd_f32 does, weight and bias gradient k = 2 n H W + 3.
  ConvS2Fn          tests/test_edvr_ops_gpu.py: forward as ConvFn against F.conv2d(stride=2); dx k = 2 * 9 roundup8(cout) + 8 + 1;
                    dweight / dbias the chain of _wgrad_f32_plan at the full resolution + 1.
  Conv1x1Fn         tests/test_convd_ops_gpu.py, ksize 1: forward k = 2 cin_pad + 8, dx k = 2 roundup8(cout) + 8, dweight / dbias
                    k = _wgradd_chain(n, h, w, cout, cin, 1, 1).
  Pool3x3s2Fn, TSACorrFn, TSAGateFn   tests/test_edvr_ops_gpu.py (tests/edvr_opwise.py::pool_spec, corr_spec, gate_spec cite each).
  Bilinear2xFn      6 EPS interp(|x|), 20 EPS adjoint(|g|).     BilinearUpFn   tests/test_msrresnet_gpu.py + one rounding for acc.
  ToCB8, FromCB8, PixelShuffleFn, AddFn   bit-exact against a float32 emulation.
  DCNFn forward     tests/test_dcn_ops_gpu.py at arbitrary offsets: k = 2 * 9 cin + K_SAMPLE + 1 + K_EPI + K_SIGMOID and the coordinate
                    term sum |W| EPS (|h_im| + |w_im| + 2) |m| sum |v|.  The value is continuous across cells, so the reference takes
                    its own float64 cell.
  DCNFn backward at the network's arbitrary offsets.  d/d(offset) jumps where a coordinate crosses an integer, so the float64
                    reference is FORCED to the cell the device takes: h_im = fl(float(y - 1 + i) + offset), the `inside` test and
                    floor(h_im) are computed in float32 on the CPU in the kernel's order (edvr_opwise.cells32), and the reference
                    evaluates the bilinear polynomial of that cell at the float64 position (lh64 = h_im64 - h_low may lie a rounding
                    outside [0, 1]).  Every quantity is then a polynomial in lh, lw, and the device's lh = h_im32 - h_low (exact
                    subtraction) differs from lh64 by the one rounding of h_im: at most EPS |h_im|; hh = fl(1 - lh) adds EPS.  A
                    bilinear weight hh hw, hh lw, lh hw, lh lw is therefore off by at most EPS (|h_im| + 1) + EPS (|w_im| + 1) before
                    its own product rounding, and a derivative weight (one of hh, lh, hw, lw) by at most EPS (|coordinate| + 1): each
                    carries EPS (|h_im| + |w_im| + 2).  The dyadic-offset bounds of tests/test_dcn_ops_gpu.py extend by that term and
                    by one rounding where a weight is a product (S = sum of |v| over the valid corners, A_col = sum_co |W| |dz|,
                    K_COL = 2 roundup8(cout) + 8, cpg = cin / dg, mag = |h_im| + |w_im| + 2):
                      dweight  (chain + K_SAMPLE + 1 + K_SIGMOID + 1) EPS sum |dz| |col| + EPS sum |dz| mag m S
                      dbias    (chain + 1) EPS sum |dz|
                      dmask    EPS m (1 - m) ((2 cpg + 8 + K_COL + K_DSIG) sum_c A_col sum |w| |v| + sum_c A_col mag S), the logit's
                               factor with K_DSIG = 7 + 4 e^logit per element instead of the 37 that test counts for logits in [-2, 2]:
                               m carries 4 EPS, 1 - m one rounding and 4 EPS m / (1 - m) = 4 EPS e^logit, two products
                      doffset  EPS m sum_c A_col S (2 cpg + 8 + K_COL + K_SIGMOID + mag)
                      dx       (J + 2 + 1 + K_COL + K_SIGMOID) EPS scatter(|w| m A_col) + EPS scatter(mag m A_col), J the largest
                               number of atomicAdds that reach one element, counted from the forced cells
                    No element is excluded.  tests/test_edvr_opwise_host.py shows that this reference is autograd of
                    tests/dcn_restate.py wherever the float32 and float64 cells agree.

Tensors with several consumers and the torch plumbing between the Functions (torch.cat, view, reshape, contiguous, expand, * 2.0,
slicing, frame selection): the gradient that must arrive at every Function's output, at the input and at every parameter is rebuilt
from the REPLAYED gradients of its consumers through the plumbing's own adjoint (edvr_opwise.contributions) and compared with the
recorded ``.grad``.  Movements and * 2 are exact.  Where m contributions reach an element: m = 1 the number itself; m = 2 the float32
sum (a + b = b + a); m > 2 within (m - 1) EPS sum |g_i| of the float64 sum (m - 1 float32 additions in whatever order autograd took;
feat_l1, the sum over t of the centre pyramid, ``aligned``).  A replayed DCN dx is known only up to its arrival order, 2 J EPS
scatter(|w| m A_col) between two runs; where one contributes, that slack is added.

Negative controls (test_negative_controls): mutated references that the device result must MISS under the same bounds.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from image_restoration_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edvr_opwise as O  # noqa: E402
from edvr_opwise import CONFIGS, EPS, r8  # noqa: E402
from f32_opwise import cb8_to_nchw, check, nchw_to_cb8, worst  # noqa: E402
from test_conv_ops_gpu import _wgrad_f32_plan  # noqa: E402
from test_convd_ops_gpu import _wgradd_chain  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = set(O.FUNCTIONS)
WANT_NAMES = {'tsa-b2': ALL, 'predeblur-hr-b1': ALL - {'BilinearUpFn'},
              'nf16-dg2-notsa': ALL - {'Pool3x3s2Fn', 'TSACorrFn', 'TSAGateFn'}}
# parameters whose gradient no DCN dx reaches (module docstring): the cascade's own layers and everything after the alignment
NO_ATOMICS = ('fusion', 'reconstruction.', 'upconv', 'conv_hr', 'conv_last', 'pcd_align.cas_')
EXACT = ('ToCB8', 'FromCB8', 'PixelShuffleFn', 'AddFn')
WORST = {}


@pytest.fixture(scope='module')
def cuda():
    return torch.device('cuda:0')


def _note(config, what, ratio):
    WORST[(config, what)] = max(WORST.get((config, what), 0.0), ratio)


def _report(config):
    for (cfg, what), r in sorted(WORST.items()):
        if cfg == config:
            print(f'WORST {cfg:16s} {what:28s} got / bound = {r:.3f}')


# ------------------------------------------------------------------------------------------------------------------ recorded runs
class Run:
    pass


_RUNS = {}


def _run(dev, name):
    """One unpatched forward + backward, one recorded, and one forward whose Function outputs are leaves (the plumbing), once per
    configuration; the float64 and float32 restatements on the CPU."""
    if name in _RUNS:
        return _RUNS[name]
    run = Run()
    run.name, run.kw = name, CONFIGS[name][0]
    net, run.sd, run.x, run.gy = O.make_case(name)
    run.net = net = net.to(dev).eval()
    gyd = run.gy.to(dev)
    xd = run.x.to(dev).requires_grad_(True)
    y = net(xd)
    y.backward(gyd)
    torch.cuda.synchronize()
    run.plain = [y.detach().clone(), xd.grad.clone()] + [p.grad.clone() for p in net.parameters()]
    for p in net.parameters():
        p.grad = None
    rec = O.Recorder()
    with pytest.MonkeyPatch.context() as mp:
        rec.install(mp)
        run.xr = run.x.to(dev).requires_grad_(True)
        run.yr = net(run.xr)
        run.yr.backward(gyd)
    torch.cuda.synchronize()
    run.rec = rec.finish()
    run.recorded = [run.yr.detach(), run.xr.grad] + [p.grad for p in net.parameters()]
    prec = O.Recorder(detach=True)
    with pytest.MonkeyPatch.context() as mp:
        prec.install(mp)
        run.xp = run.x.to(dev).requires_grad_(True)
        run.yp = net(run.xp)
    run.prec = prec
    names = {id(p): k.rsplit('.', 1)[0] for k, p in net.named_parameters()}
    for r in list(rec.records) + list(prec.records):
        r.tag = next((names[id(a)] for a in r.args if id(a) in names), '')
    run.replays, run.results = {}, {}
    run.offs = {}
    run.f64 = O.restated(run.sd, run.x, run.gy, run.kw, torch.float64, run.offs)
    run.f32 = O.restated(run.sd, run.x, run.gy, run.kw, torch.float32)
    _RUNS[name] = run
    return run


def _replay(run, i):
    if i not in run.replays:
        run.replays[i] = O.Replay(run.rec.records[i])
    return run.replays[i]


def _leaves(run):
    """(leaves of the plumbing run, the recorded gradient of each, labels): every Function output, the input, every parameter."""
    recs, params = run.rec.records, list(run.net.parameters())
    return ([r.out for r in run.prec.records] + [run.xp] + params, [r.gy for r in recs] + [run.xr.grad] + [p.grad for p in params],
            [f'{i} {r}' for i, r in enumerate(recs)] + ['input'] + [k for k, _ in run.net.named_parameters()])


def _contribs(run):
    if not hasattr(run, 'contribs'):
        recs = run.rec.records
        for i, _ in _ops(run, 'DCNFn'):
            _results(run, i)
        run.contribs = O.contributions(run.prec.records, _leaves(run)[0], lambda i: _replay(run, i).grads,
                                       lambda i, j: recs[i].dx_order if recs[i].name == 'DCNFn' and j == 0 else None)
    return run.contribs


def _ops(run, *names):
    return [(i, r) for i, r in enumerate(run.rec.records) if r.name in names]


def _d(t):
    return t.detach().cpu().double()


def _padded(t, c, what):
    """CB8 -> NCHW float64 of the first c channels; the pad channels must be zero."""
    full = cb8_to_nchw(t)
    assert bool((full[:, c:] == 0).all()), f'{what}: pad channels are not zero'
    return full[:, :c]


# --------------------------------------------------------------------------------------------------- one recorded op against float64
def _conv_results(r, rep, mutate=None):
    x, wt, bias, slope = r.vals
    cout, cin, k, _ = wt.shape
    assert x.size(1) * 8 == r8(cin) and bias is not None
    x64 = cb8_to_nchw(x, cin)
    n, _, h, w = x64.shape
    stride = 2 if r.name == 'ConvS2Fn' else 1
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    if r.name == 'ConvFn':
        assert k == 3
        k_w, extra = 2 * n * ho * wo + 3, 0
    elif r.name == 'ConvS2Fn':
        assert k == 3
        k_w, extra = max(p[4] for p in _wgrad_f32_plan(_lib.load(), n, h, w, cout, r8(cin), 9)) + 1, 1
    else:
        assert k == 1
        k_w, extra = _wgradd_chain(n, h, w, cout, cin, 1, 1), 0
    y = _padded(rep.out, cout, f'{r} y')
    spec = O.conv_spec(x64, _d(wt), _d(bias), slope, stride, y, cb8_to_nchw(r.gy, cout), k_w, extra, mutate)
    got = {'fwd': y, 'dx': _padded(rep.grads[0], cin, f'{r} dx'), 'dw': _d(rep.grads[1]), 'db': _d(rep.grads[2])}
    return {q: (got[q],) + spec[q] for q in got}


def _dcn_inputs(r):
    x, off, mask, wt, bias, slope, dg, logit = r.vals[:8]
    windows = r.vals[8] if len(r.vals) > 8 else None
    assert logit is True and bias is not None
    cin = wt.size(1)
    assert x.size(1) * 8 == cin
    if windows is not None:
        assert r.args[1] is r.args[2] and windows == ((0, 18 * dg // 8), (18 * dg // 8, (9 * dg + 7) // 8))
        co = cb8_to_nchw(off)
        off64, logit64 = co[:, :18 * dg], co[:, 18 * dg:27 * dg]
    else:
        assert r.args[1] is not r.args[2]
        off64, logit64 = cb8_to_nchw(off, 18 * dg), cb8_to_nchw(mask, 9 * dg)
    return cb8_to_nchw(x), off64, logit64, _d(wt), _d(bias), slope, dg, windows


def _dcn_results(r, rep, mutate=None):
    x64, off64, logit64, w64, b64, slope, dg, windows = _dcn_inputs(r)
    n, cin, h, w = x64.shape
    cout = w64.size(0)
    y = _padded(rep.out, cout, f'{r} y')
    chain = _wgradd_chain(n, h, w, cout, 9 * cin, 1, 1)
    spec = O.dcn_spec(x64, off64, logit64, w64, b64, slope, dg, y, cb8_to_nchw(r.gy, cout), chain, mutate)
    if windows is not None:
        g = _padded(rep.grads[1], 27 * dg, f'{r} d(offsets, logits)')
        assert 2 not in rep.grads
        doff, dmask = g[:, :18 * dg], g[:, 18 * dg:]
    else:
        doff, dmask = _padded(rep.grads[1], 18 * dg, f'{r} doffset'), _padded(rep.grads[2], 9 * dg, f'{r} dmask')
    got = {'fwd': y, 'dx': cb8_to_nchw(rep.grads[0]), 'doffset': doff, 'dmask': dmask, 'dweight': _d(rep.grads[3]), 'dbias': _d(rep.grads[4])}
    res = {q: (got[q],) + spec[q] for q in got}
    print(f'{r}: {"windows" if windows is not None else "split by copy"}, {tuple(x64.shape)}, dg {dg}, at most {spec["J"]} adds reach one '
          'element of dx')
    return res, spec['dx order']


def _exact(r, rep):
    """ToCB8, FromCB8, PixelShuffleFn, AddFn against a float32 emulation: a movement, or one float32 addition."""
    out, gx, gy, x = rep.out.cpu(), rep.grads[0].cpu(), r.gy.cpu(), r.vals[0].cpu()
    assert out.dtype == gx.dtype == torch.float32 and gx.shape == x.shape
    if r.name == 'ToCB8':
        assert torch.equal(out, nchw_to_cb8(x)), f'{r}: forward is not x in CB8 with zero pad channels'
        assert torch.equal(gx.double(), cb8_to_nchw(gy, x.size(1))), f'{r}: backward'
    elif r.name == 'FromCB8':
        assert torch.equal(out.double(), cb8_to_nchw(x, r.vals[1])), f'{r}: forward'
        assert torch.equal(gx, nchw_to_cb8(gy)), f'{r}: backward is not gy in CB8 with zero pad channels'
    elif r.name == 'PixelShuffleFn':
        c, s = r.vals[1], r.vals[2]
        assert x.size(1) * 8 == c * s * s and out.size(1) * 8 == c
        assert torch.equal(cb8_to_nchw(out), F.pixel_shuffle(cb8_to_nchw(x), s)), f'{r}: forward'
        assert torch.equal(cb8_to_nchw(gx), F.pixel_unshuffle(cb8_to_nchw(gy), s)), f'{r}: backward'
    else:
        assert torch.equal(out, x + r.vals[1].cpu()), f'{r}: forward'
        assert torch.equal(gx, gy) and torch.equal(rep.grads[1].cpu(), gy), f'{r}: backward'
    return {}


def _results(run, i, mutate=None):
    """{quantity: (got, reference, bound)} of record i, computed once (``mutate``: a negative control, not kept)."""
    if mutate is None and i in run.results:
        return run.results[i]
    r, rep = run.rec.records[i], _replay(run, i)
    assert r.gy is not None and rep.grads, f'{r}: no gradient reached this op'
    if r.name in ('ConvFn', 'ConvS2Fn', 'Conv1x1Fn'):
        res = _conv_results(r, rep, mutate)
    elif r.name == 'DCNFn':
        res, order = _dcn_results(r, rep, mutate)
        if mutate is None:
            r.dx_order = nchw_to_cb8(order.float() * (1 + 2.0 ** -20)).to(rep.out.device)
    elif r.name == 'Bilinear2xFn':
        spec = O.up2_spec(cb8_to_nchw(r.vals[0]), cb8_to_nchw(r.gy), mutate)
        res = {'fwd': (cb8_to_nchw(rep.out),) + spec['fwd'], 'dx': (cb8_to_nchw(rep.grads[0]),) + spec['dx']}
    elif r.name == 'Pool3x3s2Fn':
        spec = O.pool_spec(cb8_to_nchw(r.vals[0]), cb8_to_nchw(r.gy), mutate)
        res = {'fwd': (cb8_to_nchw(rep.out),) + spec['fwd'], 'dx': (cb8_to_nchw(rep.grads[0]),) + spec['dx']}
    elif r.name == 'TSACorrFn':
        spec = O.corr_spec(*(cb8_to_nchw(v) for v in r.vals[:3]), r.vals[3], cb8_to_nchw(r.gy), mutate)
        got = {'fwd': rep.out, 'd_emb': rep.grads[0], 'd_emb_ref': rep.grads[1], 'd_aligned': rep.grads[2]}
        res = {q: (cb8_to_nchw(v),) + spec[q] for q, v in got.items()}
    elif r.name == 'TSAGateFn':
        spec = O.gate_spec(*(cb8_to_nchw(v) for v in r.vals), cb8_to_nchw(r.gy))
        got = {'fwd': rep.out, 'd_feat': rep.grads[0], 'd_attn': rep.grads[1], 'd_add': rep.grads[2]}
        res = {q: (cb8_to_nchw(v),) + spec[q] for q, v in got.items()}
    elif r.name == 'BilinearUpFn':
        assert r.vals[1] == 4 and not torch.equal(r.vals[2], r.post[2]), f'{r}: acc is updated in place'
        spec = O.up4_spec(_d(r.vals[0]), _d(r.vals[2]), _d(r.gy))
        got = {'fwd': rep.out, 'dx': rep.grads[0], 'd_acc': rep.grads[2]}
        res = {q: (_d(v),) + spec[q] for q, v in got.items()}
    else:
        assert r.name in EXACT, r.name
        res = _exact(r, rep)
    if mutate is None:
        run.results[i] = res
    return res


def _check_ops(run, *names):
    done = 0
    for i, r in _ops(run, *names):
        for q, (got, want, bound) in _results(run, i).items():
            _note(run.name, f'{r.name} {q}', check(got, want, bound, f'{run.name} {r} {q}'))
        done += 1
    return done


# ------------------------------------------------------------------------------------------------------------------------ anchors
@pytest.mark.parametrize('config', list(CONFIGS))
def test_the_case_deforms(cuda, config):
    run = _run(cuda, config)
    dg = run.kw['deformable_groups']
    mean_l1, outside = O.deforms(run.offs['l1'], dg)
    print(f'{config}: mean |offset| at level 1 = {mean_l1:.3f} px, samples outside the image: {100 * outside:.1f} %')
    assert 0.5 <= mean_l1 <= 3.0 and outside >= 0.01
    assert all(float(v.abs().max()) > 0 for k, v in run.sd.items() if 'conv_offset' in k)


@pytest.mark.parametrize('config', list(CONFIGS))
def test_the_recorder_observes_the_production_forward_and_backward(cuda, config):
    run = _run(cuda, config)
    assert {r.name for r in run.rec.records} == WANT_NAMES[config]
    keys = ['output', 'grad input'] + [f'grad {k}' for k, _ in run.net.named_parameters()]
    assert len(keys) == len(run.plain) == len(run.recorded)
    assert torch.equal(run.plain[0], run.recorded[0]), 'the recorded forward is not the production forward'
    moved = []
    for k, a, b in zip(keys[1:], run.plain[1:], run.recorded[1:]):
        assert a is not None and b is not None and a.shape == b.shape, k
        if k.startswith('grad ') and k[5:].startswith(NO_ATOMICS):
            assert torch.equal(a, b), f'{k}: the recorded gradient is not the production gradient'
        elif not torch.equal(a, b):
            moved.append((k, float((a.double() - b.double()).norm() / b.double().norm())))
    print(f'{config}: {len(moved)} of {len(keys) - 1} gradients upstream of an atomicAdd differ between the two backward passes'
          + (f', at most {max(m for _, m in moved):.2e} relative L2' if moved else ''))
    # the plumbing run is the same forward: op for op the same output bits
    assert [r.name for r in run.prec.records] == [r.name for r in run.rec.records]
    for a, b in zip(run.prec.records, run.rec.records):
        assert torch.equal(a.out_val, b.out_val) and a.tag == b.tag, f'{b}'
    assert torch.equal(run.yp.detach(), run.recorded[0])
    # routes
    windows = [len(r.vals) > 8 for _, r in _ops(run, 'DCNFn')]
    assert len(windows) == 4 and all(windows) == (config != 'nf16-dg2-notsa') and any(windows) == (config != 'nf16-dg2-notsa')
    strided = [r for r in run.rec.records if r.name == 'ToCB8' and not r.strides[0][1]]
    assert len(strided) == (8 if config == 'nf16-dg2-notsa' else 0), 'the split-by-copy route feeds ToCB8 non-contiguous NCHW slices'


@pytest.mark.parametrize('config', list(CONFIGS))
def test_every_replay_reproduces_its_recorded_op(cuda, config):
    run = _run(cuda, config)
    contribs = _contribs(run)
    compared = 0
    for i, (r, pr) in enumerate(zip(run.rec.records, run.prec.records)):
        rep = _replay(run, i)

        def single(j):
            return len(contribs.get(id(pr.args[j]), ())) == 1
        compared += O.assert_replay_reproduces(r, rep, single)
        if r.name == 'DCNFn':
            assert not single(0), 'a DCN dx with a single consumer would need its own rule (atomicAdd)'
        if r.name == 'BilinearUpFn':
            assert rep.fresh[2].grad_fn is None and torch.equal(rep.fresh[2].detach(), r.vals[2]), 'the replay starts from the pre-call acc'
    print(f'{config}: {len(run.rec.records)} ops replayed, {compared} single-consumer gradients compared bit for bit')
    assert compared >= len(run.rec.records) // 2


@pytest.mark.parametrize('config', list(CONFIGS))
def test_gradients_through_the_plumbing(cuda, config):
    """The gradient arriving at every Function output, at the input and at every parameter, rebuilt from the replayed gradients of
    its consumers (module docstring)."""
    run = _run(cuda, config)
    recs = run.rec.records
    params = list(run.net.parameters())
    leaves, recorded, labels = _leaves(run)
    contribs = _contribs(run)
    assert not contribs[id(leaves[len(recs) - 1])] and torch.equal(recorded[len(recs) - 1], run.gy.to(cuda)), 'the last op feeds nothing'
    big = {}
    for leaf, got, label in zip(leaves[:len(recs) - 1] + leaves[len(recs):], recorded[:len(recs) - 1] + recorded[len(recs):],
                                labels[:len(recs) - 1] + labels[len(recs):]):
        cs = contribs[id(leaf)]
        assert cs and got is not None, f'{label}: nothing consumes it'
        ok, ratio, m = O.sum_rule(cs, got)
        if m > 2 or any(s is not None for _, _, s in cs):
            big[label] = (m, ratio)
            print(f'{config} {label}: up to {m} contributions per element, err / bound = {ratio:.3f}')
            _note(config, f'sum of {min(m, 9)} gradients', ratio)
        assert ok, f'{label}: the recorded gradient is not the sum of its consumers\' replayed gradients (m = {m}, {ratio:.3f})'
    for p, k in zip(params, labels[len(recs) + 1:]):
        assert len(contribs[id(p)]) == 1, f'{k} is carried by {len(contribs[id(p)])} records'
    t = run.kw['num_frame']
    assert max(m for m, _ in big.values()) == 2 * t + 3, 'feat_l1: two expands over t, two concatenations and a DCN read it, and conv_l2_1'
    _report(config)


# ---------------------------------------------------------------------------------------------------------------- op by op
@pytest.mark.parametrize('config', list(CONFIGS))
def test_convolutions(cuda, config):
    """ConvFn (3x3, slopes 0.1 / 1.0 / 0.0, 3 -> nf, 2 nf -> nf, nf -> 27 dg, nf -> 3), ConvS2Fn, Conv1x1Fn."""
    run = _run(cuda, config)
    assert _check_ops(run, 'ConvFn', 'ConvS2Fn', 'Conv1x1Fn') == len(_ops(run, 'ConvFn', 'ConvS2Fn', 'Conv1x1Fn'))
    slopes = {r.vals[3] for _, r in _ops(run, 'ConvFn')}
    assert slopes == {0.1, 1.0, 0.0}, slopes
    couts = {r.vals[1].size(0) for _, r in _ops(run, 'ConvFn')}
    assert {3, 27 * run.kw['deformable_groups']} <= couts
    assert len(_ops(run, 'ConvS2Fn')) == (6 if config == 'predeblur-hr-b1' else 2)
    if config == 'tsa-b2':
        assert {r.vals[1].size(1) for _, r in _ops(run, 'Conv1x1Fn')} == {192, 128, 64}
    if config == 'nf16-dg2-notsa':
        assert [r.vals[1].size(1) for _, r in _ops(run, 'Conv1x1Fn')] == [80]
    _report(config)


@pytest.mark.parametrize('config', list(CONFIGS))
def test_deformable_convolutions(cuda, config):
    run = _run(cuda, config)
    assert _check_ops(run, 'DCNFn') == 4
    _report(config)


@pytest.mark.parametrize('config', list(CONFIGS))
def test_resampling_pooling_and_attention(cuda, config):
    run = _run(cuda, config)
    names = ('Bilinear2xFn', 'Pool3x3s2Fn', 'TSACorrFn', 'TSAGateFn', 'BilinearUpFn')
    assert _check_ops(run, *names) == len(_ops(run, *names))
    if config == 'tsa-b2':
        assert sorted({tuple(r.vals[0].shape[2:4]) for _, r in _ops(run, 'Bilinear2xFn')}) == [(3, 9), (6, 18)]
        assert [tuple(r.vals[0].shape[2:4]) for _, r in _ops(run, 'Pool3x3s2Fn')] == [(12, 36), (6, 18)]
    _report(config)


@pytest.mark.parametrize('config', list(CONFIGS))
def test_every_recorded_op_is_checked(cuda, config):
    """Coverage: every record goes through its check (the bit-exact ones here), none is left out, every parameter sits in one record."""
    run = _run(cuda, config)
    for i, r in enumerate(run.rec.records):
        for q, (got, want, bound) in _results(run, i).items():
            _note(config, f'{r.name} {q}', check(got, want, bound, f'{config} {r} {q}'))
    assert len(run.results) == len(run.rec.records)
    assert {r.name for r in run.rec.records} == WANT_NAMES[config]
    carried = {}
    for r in run.rec.records:
        for a in r.args:
            if isinstance(a, torch.nn.Parameter):
                carried[id(a)] = carried.get(id(a), 0) + 1
    assert all(carried.get(id(p), 0) == 1 for p in run.net.parameters()), 'a parameter is carried by no record, or by several'
    assert sum(1 for r in run.rec.records if r.name in EXACT) > 0
    _report(config)


# ------------------------------------------------------------------------------------------------------------- the whole network
def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@pytest.mark.parametrize('config', list(CONFIGS))
def test_whole_network_within_10x_the_float32_distance(cuda, config):
    """The rule of tests/test_edvr_gpu.py at batch 2 (and on the batch-1 configuration), for the unpatched and the recorded run: every
    tensor's relative L2 distance to the float64 restatement is at most 10x that of the float32 restatement."""
    run = _run(cuda, config)
    names = ['output', 'grad input'] + [f'grad {k}' for k in run.sd]
    f64, f32 = [run.f64[0]] + run.f64[1], [run.f32[0]] + run.f32[1]
    assert len(names) == len(f64) == len(run.plain) == len(run.recorded)
    bad = []
    for name, a64, a32, hp, hr in zip(names, f64, f32, run.plain, run.recorded):
        d32, dp, dr = _rel(a32, a64), _rel(hp.cpu(), a64), _rel(hr.cpu(), a64)
        print(f'{config} {name}: float32 restatement {d32:.3e}, HIP {dp:.3e} / recorded {dr:.3e} (relative L2 to float64)')
        if not (dp <= 10 * d32 and dr <= 10 * d32):
            bad.append((name, dp, dr, d32))
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------- negative controls
CONTROLS = {
    # control: (configurations, Function names, mutation, quantity)
    'dcn_offsets_swapped': (('tsa-b2', 'nf16-dg2-notsa'), ('DCNFn',), 'swap', ('fwd', 'doffset')),
    'dcn_mask_group_shifted': (('tsa-b2', 'nf16-dg2-notsa'), ('DCNFn',), 'mask_group', ('fwd',)),
    'avg_pool_valid_count': (('tsa-b2',), ('Pool3x3s2Fn',), 'valid_count', ('fwd',)),
    'up2_align_corners': (tuple(CONFIGS), ('Bilinear2xFn',), 'align_corners', ('fwd', 'dx')),
    'conv_s2_odd_positions': (tuple(CONFIGS), ('ConvS2Fn',), 'odd', ('fwd',)),
    'tsa_corr_other_clip': (('tsa-b2',), ('TSACorrFn',), 'other_clip', ('fwd',)),
    'upconv_lrelu_slope': (tuple(CONFIGS), ('ConvFn',), 'slope', ('fwd',)),
}


@pytest.mark.parametrize('control', list(CONTROLS) + ['sum_over_t_one_frame'])
def test_negative_controls(cuda, control):
    """Mutated references under the same bounds: the device result must miss each of them."""
    ratios = {}
    if control == 'sum_over_t_one_frame':
        for config in ('tsa-b2', 'nf16-dg2-notsa'):
            run = _run(cuda, config)
            recs = run.rec.records
            leaves, recorded, labels = _leaves(run)
            full = _contribs(run)
            # feat_l1, feat_l2, feat_l3: the outputs whose consumers include the expand over t
            one = O.contributions(run.prec.records, leaves, lambda i: _replay(run, i).grads,
                                  lambda i, j: recs[i].dx_order if recs[i].name == 'DCNFn' and j == 0 else None, one_frame=True)
            for leaf, got, label in zip(leaves, recorded, labels):
                if len(one[id(leaf)]) < len(full[id(leaf)]):
                    ok, ratio, _ = O.sum_rule(one[id(leaf)], got)
                    ratios[f'{config} {label}'] = float('inf') if not ok and ratio <= 1 else ratio
                    assert not ok
        assert len(ratios) == 6
    else:
        configs, names, mutate, quantities = CONTROLS[control]
        for config in configs:
            run = _run(cuda, config)
            for i, r in _ops(run, *names):
                if control == 'upconv_lrelu_slope' and r.tag not in ('upconv1', 'upconv2'):
                    continue
                res = _results(run, i, mutate)
                for q in quantities:
                    ratios[f'{config} {i} {r} {q}'] = worst(*res[q])
        want = {'dcn_offsets_swapped': 16, 'dcn_mask_group_shifted': 8, 'avg_pool_valid_count': 2, 'up2_align_corners': 36,
                'conv_s2_odd_positions': 10, 'tsa_corr_other_clip': 1, 'upconv_lrelu_slope': 6}[control]
        assert len(ratios) == want, len(ratios)
    for k, v in ratios.items():
        print(f'CONTROL {control:24s} {k:44s} got / bound = {v:.3g}')
    for k, v in ratios.items():
        assert v > 1.0, f'{control} stays inside the bound at {k} ({v:.3f}): the bound cannot see it'
