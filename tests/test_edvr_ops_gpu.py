"""Every entry point of include/sr_hip_edvr.h through hip_ops, against float64 on the CPU.

Conventions (tests/test_convd_ops_gpu.py, tests/test_dcn_ops_gpu.py): windows sit in buffers whose other blocks hold SENTINEL
and must come back unchanged; every input is an fp32 value, so the float64 reference starts from the same numbers; source pad
channels (cin not a multiple of 8) hold large finite values the zero weights must cancel.

Bounds are derived, not fitted.  EPS = 2^-24; |y - y64| <= k EPS A + EPS |y64| with A the same operation on absolute values in
float64 and k counted from the kernel's own operation order; every check prints its largest error / bound ratio.
  sr_conv3x3s2_f32     k = 2 * 9 * cin_pad + 8: two roundings per product of the one MFMA chain over (cin block, tap, channel),
                       bias and LeakyReLU (the count of sr_convd_f32), against F.conv2d(stride=2, padding=1)
  ConvS2Fn backward    dz = gy * LeakyReLU'(y), one rounding, on the branch of the device's saved output; then the bounds of the
                       stride-1 operators on the zero-inserted gradient (tests/test_conv_ops_gpu.py): dx k = 2 * 9 *
                       roundup8(cout) + 8 (+1 for dz), dweight / dbias the chain of _wgrad_f32_plan at the full resolution (+1)
  zero insert          bit-exact, zeros everywhere else
  pool forward         max bit-exact against torch's CPU float32 max_pool2d; avg k = 9: 8 adds of the row-major sum (pad adds
                       exact zeros) and one correctly rounded division
  pool backward        per covering window one add of g_max, one division and one add of g_avg / 9: k = 3 * 4 on the same
                       adjoint of |g|
  TSA correlation      s = sum_c emb * emb_ref, channels ascending in one lane: c rounded products and c adds (the first onto 0, exact), k = 2 c on A = sum |emb|
                       |emb_ref|; the sigmoid's slope is at most 1/4 and m = 1 / (1 + expf(-s)) carries K_SIGMOID = 4 EPS relative
                       (counted in tests/test_dcn_ops_gpu.py): bound_p = k EPS A / 4 + 4 EPS p.  out is one rounding from
                       aligned * p for the kernel's own p.  Backward: d_aligned = g p (bound_p |g| and one rounding); S = sum_c g
                       * aligned (k = 2 c on sum |g| |aligned|), q = p (1 - p) (|dq| <= bound_p + 2 EPS q), ds = S q (one
                       rounding): bound_ds = q 2c EPS A_S + |S| bound_p + 3 EPS |S| q; d_emb = ds * emb_ref (one rounding);
                       d_emb_ref = sum_t ds_t emb_t, t ascending: the per-frame terms plus 2 t EPS sum_t |ds_t emb_t|
  gate                 out = (feat * m) * 2 + attn_add: m 4 EPS, two roundings (the * 2 is exact): k = 6 on 2 |feat| m + |add|.
                       d_feat = g * (2 m): k = 5.  d_attn = ((g feat) 2) (m (1 - m)): 1 + 4 + (4 e^attn + 1) + 1 + 1 relative,
                       elementwise (1 - m inherits m's error magnified by m / (1 - m) = e^attn).
                       CB8 windows always hold a multiple of 8 floats per pixel, so no element count can be ragged against the
                       16-byte vector; the shapes are ragged against the 256-thread workgroup.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from image_restoration_amd import _lib
from image_restoration_amd import hip_autograd as A
from image_restoration_amd import hip_ops as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_conv_ops_gpu import _wgrad_f32_plan  # noqa: E402
from test_dcn_ops_gpu import EPS, SENTINEL, _cb8_buf, _check, _f32, _nchw, _sentinel_kept  # noqa: E402
from test_edvr_host import _s2_instance  # noqa: E402

pytestmark = pytest.mark.gpu

K_SIGMOID = 4
SLOPE = float(np.float32(0.1))


@pytest.fixture(scope='module')
def cuda():
    return torch.device('cuda:0')


def _randn(rng, shape, scale=1.0):
    return _f32(rng.standard_normal(shape) * scale)


def _out_buf(n, c, h, w, cuda):
    """A NaN-filled window of roundup8(c) channels between SENTINEL blocks."""
    return _cb8_buf(torch.full((n, (c + 7) // 8 * 8, h, w), float('nan'), dtype=torch.float64), cuda)


# ------------------------------------------------------------------------------------------------------ stride-2 conv
# (n, cin, cout, H, W): the issue's five; cin with pad channels on the COT 2 / 8-row instance at four output rows; then the
# 8-row instances as the default network runs them, for COT 1 and COT 2: 3 strips x 3 row tiles x 32 images = 288 >= 256 tiles
# under the 8-row rule, 18 output rows (row-tile boundaries at 8 and 16, the last tile two rows), 65 output columns (two full
# strips and one column), so all four waves of a tile store and every staged source row of the 17-row tile is read
S2_CASES = [(2, 16, 24, 13, 70), (2, 64, 64, 18, 132), (1, 8, 96, 2, 2), (1, 8, 96, 1, 5), (3, 24, 32, 8, 64), (1, 12, 64, 7, 9),
            (32, 8, 32, 35, 130), (32, 8, 64, 35, 130)]


def _s2_spikes(h, w, th):
    """Source positions around every output row-tile boundary B (rows 2B - 1, 2B, 2B + 1) and every 32-column output boundary
    (the same columns), each with the outputs that read it."""
    ho, wo = (h + 1) // 2, (w + 1) // 2
    src = []
    for B in range(th, ho, th):
        src += [(sy, 2 * (wo // 2)) for sy in (2 * B - 1, 2 * B, 2 * B + 1) if sy < h]
    for Cb in range(32, wo, 32):
        src += [(2 * (ho // 2), sx) for sx in (2 * Cb - 1, 2 * Cb, 2 * Cb + 1) if sx < w]
    if not src:
        src = [(h - 1, w - 1)]
    out = []
    for sy, sx in src:
        readers = [(oy, ox) for oy in range(ho) for ox in range(wo) if abs(2 * oy - sy) <= 1 and abs(2 * ox - sx) <= 1]
        out.append(((sy, sx), readers))
    return out


def test_s2_cases_reach_every_instance_built():
    assert {_s2_instance(cout, n, h, w) for n, _, cout, h, w in S2_CASES} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    # both 8-row instances also run with more than one row tile, a partial last one and all four waves storing
    for cot, case in ((1, S2_CASES[6]), (2, S2_CASES[7])):
        n, _, cout, h, w = case
        assert _s2_instance(cout, n, h, w) == (cot, 2) and (h + 1) // 2 > 16 and ((h + 1) // 2) % 8 and (w + 1) // 2 > 64
        assert len([1 for (sy, _), _ in _s2_spikes(h, w, 8) if sy in (15, 16, 17, 31, 32, 33)]) == 6


@pytest.mark.parametrize('idx', range(len(S2_CASES)), ids=[f'n{c[0]}-{c[1]}to{c[2]}-{c[3]}x{c[4]}' for c in S2_CASES])
def test_conv3x3s2_forward(cuda, idx):
    n, cin, cout, h, w = S2_CASES[idx]
    rng = np.random.default_rng(100 + idx)
    cin_pad, cout_pad = (cin + 7) // 8 * 8, (cout + 7) // 8 * 8
    ho, wo = (h + 1) // 2, (w + 1) // 2
    wt = _randn(rng, (cout, cin, 3, 3), (1.0 / (cin * 9)) ** 0.5)
    wt[:, -1] = 0.5                            # the spiked source channel: +1/2 on every tap
    bias = _randn(rng, (cout,), 0.5)
    k = 2 * 9 * cin_pad + 8

    def conv(x):
        c = F.conv2d(x[:, :cin], wt, bias, stride=2, padding=1)
        a = F.conv2d(x[:, :cin].abs(), wt.abs(), bias.abs(), stride=2, padding=1)
        return torch.where(c > 0, c, SLOPE * c), a
    x = _randn(rng, (n, cin_pad, h, w))
    x[:, cin:] = _randn(rng, (n, cin_pad - cin, h, w), 100.0)
    y0, A0 = conv(x)
    bound0 = k * EPS * A0 + EPS * y0.abs()
    spike = 64.0 * float(bound0.max()) / (0.5 * SLOPE) + 64.0
    spikes = _s2_spikes(h, w, 4 * _s2_instance(cout, n, h, w)[1])
    xs = x.clone()
    for (sy, sx), _ in spikes:
        xs[-1, cin - 1, sy, sx] = spike
    y64, Aabs = conv(xs)

    in_buf, in_win = _cb8_buf(xs, cuda)
    out_buf, out_win = _out_buf(n, cout, ho, wo, cuda)
    pack = H.PackedConvK if idx % 2 == 0 else H.PackedConv
    pc = pack(wt.float().to(cuda), bias.float().to(cuda))
    assert pc.src_channels == cin_pad
    H.conv3x3s2(in_win, pc, out=out_win, act_slope=SLOPE)
    torch.cuda.synchronize()
    got = _nchw(out_win, cout_pad)
    bound = _check(got[:, :cout], y64, k * EPS * Aabs, f'conv3x3s2 {S2_CASES[idx]}')
    assert bool((got[:, cout:] == 0).all()), 'pad couts are written as zeros'
    _sentinel_kept(out_win, 'conv3x3s2 out')
    assert torch.equal(in_buf.cpu(), _cb8_buf(xs, torch.device('cpu'))[0]), 'source changed'
    for (sy, sx), readers in spikes:            # each spike is seen across its boundary
        assert readers
        for oy, ox in readers:
            delta = (y64[-1, :, oy, ox] - y0[-1, :, oy, ox]).abs()
            assert bool((delta > 4 * bound[-1, :, oy, ox]).all()), ((sy, sx), (oy, ox))


@pytest.mark.parametrize('idx', [0, 1])
def test_zero_insert_is_bit_exact(cuda, idx):
    n, _, c, h, w = S2_CASES[idx]
    rng = np.random.default_rng(200 + idx)
    ho, wo = (h + 1) // 2, (w + 1) // 2
    dy = _randn(rng, (n, c, ho, wo))
    _, dy_win = _cb8_buf(dy, cuda, pad_fill=3.0)
    _, out_win = _out_buf(n, c, h, w, cuda)
    H.zero_insert2(dy_win, h, w, out=out_win)
    torch.cuda.synchronize()
    cp = (c + 7) // 8 * 8
    want = torch.zeros((n, cp, h, w), dtype=torch.float64)
    want[:, :, ::2, ::2] = _nchw(dy_win, cp)
    assert torch.equal(_nchw(out_win, cp), want)
    _sentinel_kept(out_win, 'zero_insert2 out')


@pytest.mark.parametrize('idx', [0, 1])
def test_conv_s2_fn_backward(cuda, idx):
    n, cin, cout, h, w = S2_CASES[idx]
    rng = np.random.default_rng(300 + idx)
    lib = _lib.load()
    ho, wo = (h + 1) // 2, (w + 1) // 2
    x = _randn(rng, (n, cin, h, w))
    wt = _randn(rng, (cout, cin, 3, 3), (1.0 / (cin * 9)) ** 0.5)
    bias = _randn(rng, (cout,), 0.5)
    gy = _randn(rng, (n, cout, ho, wo))
    xd = H.nchw_to_cb8(x.float().to(cuda)).buf.requires_grad_(True)
    wd, bd = wt.float().to(cuda).requires_grad_(True), bias.float().to(cuda).requires_grad_(True)
    y = A.ConvS2Fn.apply(xd, wd, bd, SLOPE)
    gyd = H.nchw_to_cb8(gy.float().to(cuda)).buf
    y.backward(gyd)
    torch.cuda.synchronize()
    ydev = H.cb8_to_nchw(H.CB8(y.detach()), cout).cpu().double()
    dz = gy * torch.where(ydev > 0, torch.ones_like(ydev), torch.full_like(ydev, SLOPE))
    dx64 = torch.nn.grad.conv2d_input(x.shape, wt, dz, stride=2, padding=1)
    Ax = torch.nn.grad.conv2d_input(x.shape, wt.abs(), dz.abs(), stride=2, padding=1)
    dw64 = torch.nn.grad.conv2d_weight(x, wt.shape, dz, stride=2, padding=1)
    Aw = torch.nn.grad.conv2d_weight(x.abs(), wt.shape, dz.abs(), stride=2, padding=1)
    kx = 2 * 9 * ((cout + 7) // 8 * 8) + 8 + 1
    kw = max(p[4] for p in _wgrad_f32_plan(lib, n, h, w, cout, cin, 9)) + 1
    _check(H.cb8_to_nchw(H.CB8(xd.grad), cin).cpu().double(), dx64, kx * EPS * Ax, f'ConvS2Fn dx {S2_CASES[idx]}')
    _check(wd.grad.cpu().double(), dw64, kw * EPS * Aw, f'ConvS2Fn dweight {S2_CASES[idx]}')
    _check(bd.grad.cpu().double(), dz.sum((0, 2, 3)), kw * EPS * dz.abs().sum((0, 2, 3)), f'ConvS2Fn dbias {S2_CASES[idx]}')


# ---------------------------------------------------------------------------------------------------------------- pool
POOL_CASES = [(2, 16, 9, 11), (1, 8, 1, 1), (2, 24, 12, 70), (1, 8, 2, 3)]


def _pool_ref(x):
    return torch.cat([F.max_pool2d(x, 3, 2, 1), F.avg_pool2d(x, 3, 2, 1)], dim=1)


@pytest.mark.parametrize('case', POOL_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_pool_forward(cuda, case):
    n, c, h, w = case
    rng = np.random.default_rng(sum(case))
    x = _randn(rng, case)
    ho, wo = (h + 1) // 2, (w + 1) // 2
    _, xw = _cb8_buf(x, cuda)
    _, ow = _out_buf(n, 2 * c, ho, wo, cuda)
    H.pool3x3s2(xw, out=ow)
    torch.cuda.synchronize()
    got = _nchw(ow, 2 * c)
    assert torch.equal(got[:, :c], F.max_pool2d(x.float(), 3, 2, 1).double()), 'max is bit-exact'
    _check(got[:, c:], F.avg_pool2d(x, 3, 2, 1), 9 * EPS * F.avg_pool2d(x.abs(), 3, 2, 1), f'avg pool {case}')
    _sentinel_kept(ow, 'pool out')


@pytest.mark.parametrize('quantised', [False, True], ids=['random', 'ties'])
@pytest.mark.parametrize('case', POOL_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_pool_backward(cuda, case, quantised):
    n, c, h, w = case
    rng = np.random.default_rng(sum(case) + 7)
    x = _randn(rng, case)
    if quantised:
        x = (x * 2).round() / 2                  # multiples of 0.5: windows tie
    ho, wo = (h + 1) // 2, (w + 1) // 2
    g = _randn(rng, (n, 2 * c, ho, wo))
    xr = x.clone().requires_grad_(True)
    want, = torch.autograd.grad(_pool_ref(xr), xr, g)
    Aabs, = torch.autograd.grad(_pool_ref(xr), xr, g.abs())
    if quantised and h * w > 1:
        mp = F.max_pool2d(x, 3, 2, 1)
        assert n * c * ho * wo > int(torch.unique(mp).numel()), 'the quantised input repeats values'
    _, xw = _cb8_buf(x, cuda)
    _, gw = _cb8_buf(g, cuda)
    _, o1 = _out_buf(n, c, h, w, cuda)
    _, o2 = _out_buf(n, c, h, w, cuda)
    H.pool3x3s2_bwd(xw, gw, out=o1)
    H.pool3x3s2_bwd(xw, gw, out=o2)
    torch.cuda.synchronize()
    _check(_nchw(o1, c), want, 12 * EPS * Aabs, f'pool backward {case} {"ties" if quantised else "random"}')
    assert torch.equal(o1.buf.cpu(), o2.buf.cpu()), 'two runs are bit-identical'
    _sentinel_kept(o1, 'pool dx')


# ----------------------------------------------------------------------------------------------------- TSA correlation
CORR_CASES = [(2, 3, 16, 5, 7), (1, 5, 64, 4, 36), (1, 1, 8, 1, 1)]


def _corr_inputs(case, cuda):
    b, t, c, h, w = case
    rng = np.random.default_rng(sum(case) + 31)
    emb, ref, al = _randn(rng, (b * t, c, h, w)), _randn(rng, (b, c, h, w)), _randn(rng, (b * t, c, h, w))
    corr = (emb.view(b, t, c, h, w) * ref.unsqueeze(1)).sum(2)
    emb = _f32((emb * (8.0 / float(corr.abs().max()))).numpy())       # correlations span [-8, 8]
    return emb, ref, al


def _corr_forward64(emb, ref, al, case):
    b, t, c, h, w = case
    e5, a5 = emb.view(b, t, c, h, w), al.view(b, t, c, h, w)
    s = (e5 * ref.unsqueeze(1)).sum(2)
    return s, torch.sigmoid(s), (a5 * torch.sigmoid(s).unsqueeze(2)).reshape(b * t, c, h, w)


@pytest.mark.parametrize('case', CORR_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_tsa_corr(cuda, case):
    b, t, c, h, w = case
    emb, ref, al = _corr_inputs(case, cuda)
    s64, p64, out64 = _corr_forward64(emb, ref, al, case)
    smax, smin = float(s64.max()), float(s64.min())
    print(f'correlations in [{smin:.2f}, {smax:.2f}]')
    assert 7.9 <= float(s64.abs().max()) <= 8.1
    if b * t * h * w >= 50:
        assert smin <= -4 and smax >= 4, 'both tails of the sigmoid are exercised'
    _, ew = _cb8_buf(emb, cuda)
    _, rw = _cb8_buf(ref, cuda)
    _, aw = _cb8_buf(al, cuda)
    _, ow = _out_buf(b * t, c, h, w, cuda)
    prob, _ = H.tsa_corr(ew, rw, aw, t, out=ow)
    torch.cuda.synchronize()
    As = (emb.view(b, t, c, h, w).abs() * ref.abs().unsqueeze(1)).sum(2)
    bound_p = 0.25 * 2 * c * EPS * As + K_SIGMOID * EPS * p64
    pd = prob.cpu().double()
    _check(pd, p64, bound_p, f'tsa_corr p {case}')
    got = _nchw(ow, c)
    exact = al.view(b, t, c, h, w) * pd.unsqueeze(2)
    _check(got, exact.reshape(b * t, c, h, w), torch.zeros_like(got), f'tsa_corr out vs aligned * own p {case}')
    _sentinel_kept(ow, 'tsa_corr out')

    # backward, against float64 autograd
    rng = np.random.default_rng(sum(case) + 32)
    g = _randn(rng, (b * t, c, h, w))
    e_, r_, a_ = (v.clone().requires_grad_(True) for v in (emb, ref, al))
    de64, dr64, da64 = torch.autograd.grad(_corr_forward64(e_, r_, a_, case)[2], (e_, r_, a_), g)
    _, gw = _cb8_buf(g, cuda)
    runs = [H.tsa_corr_bwd(gw, ew, rw, aw, prob) for _ in range(2)]
    torch.cuda.synchronize()
    dal, demb, dref = runs[0]
    assert all(torch.equal(u.buf, v.buf) for u, v in zip(*runs)), 'two runs are bit-identical'
    g5, a5, e5 = g.view(b, t, c, h, w), al.view(b, t, c, h, w), emb.view(b, t, c, h, w)
    bp = bound_p.unsqueeze(2)
    _check(_nchw(dal, c), da64, (g5.abs() * bp).reshape(b * t, c, h, w), f'tsa_corr d_aligned {case}')
    S, AS = (g5 * a5).sum(2), (g5.abs() * a5.abs()).sum(2)
    q = p64 * (1 - p64)
    bound_ds = q * 2 * c * EPS * AS + S.abs() * bound_p + 3 * EPS * S.abs() * q
    ds = S * q
    _check(_nchw(demb, c), de64, (ref.abs().unsqueeze(1) * bound_ds.unsqueeze(2)).reshape(b * t, c, h, w), f'tsa_corr d_emb {case}')
    bound_ref = (e5.abs() * bound_ds.unsqueeze(2)).sum(1) + 2 * t * EPS * (e5 * ds.unsqueeze(2)).abs().sum(1)
    _check(_nchw(dref, c), dr64, bound_ref, f'tsa_corr d_emb_ref {case}')


# ---------------------------------------------------------------------------------------------------------------- gate
GATE_CASES = [(2, 16, 5, 7), (1, 8, 1, 1), (3, 24, 9, 13)]


@pytest.mark.parametrize('case', GATE_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_tsa_gate(cuda, case):
    n, c, h, w = case
    rng = np.random.default_rng(sum(case) + 41)
    feat, attn, add, g = _randn(rng, case), _randn(rng, case, 2.0).clamp(-4, 4), _randn(rng, case), _randn(rng, case)
    m = torch.sigmoid(attn)
    _, fw = _cb8_buf(feat, cuda)
    _, tw = _cb8_buf(attn, cuda)
    _, dw_ = _cb8_buf(add, cuda)
    _, gw = _cb8_buf(g, cuda)
    _, ow = _out_buf(n, c, h, w, cuda)
    H.tsa_gate(fw, tw, dw_, out=ow)
    df, da = H.tsa_gate_bwd(gw, fw, tw)
    torch.cuda.synchronize()
    _check(_nchw(ow, c), feat * m * 2 + add, 6 * EPS * (2 * feat.abs() * m + add.abs()), f'tsa_gate {case}')
    _sentinel_kept(ow, 'tsa_gate out')
    _check(_nchw(df, c), g * 2 * m, 5 * EPS * (2 * g.abs() * m), f'tsa_gate d_feat {case}')
    want = g * feat * 2 * m * (1 - m)
    _check(_nchw(da, c), want, (8 + 4 * torch.exp(attn)) * EPS * want.abs(), f'tsa_gate d_attn {case}')


def test_autograd_functions_match_their_ops(cuda):
    """Pool3x3s2Fn, TSACorrFn and TSAGateFn are the wrappers above plus reshapes: the frames-to-channels view of TSACorrFn."""
    b, t, c, h, w = 2, 3, 16, 4, 8
    rng = np.random.default_rng(5)
    emb, ref, al = (H.nchw_to_cb8(_randn(rng, s).float().to(cuda)).buf.requires_grad_(True)
                    for s in ((b * t, c, h, w), (b, c, h, w), (b * t, c, h, w)))
    out = A.TSACorrFn.apply(emb, ref, al, t)
    assert tuple(out.shape) == (b, t * c // 8, h, w, 8)
    _, direct = H.tsa_corr(H.CB8(emb.detach()), H.CB8(ref.detach()), H.CB8(al.detach()), t)
    assert torch.equal(out.detach().reshape(-1), direct.buf.reshape(-1))
    pooled = A.Pool3x3s2Fn.apply(out)
    gate = A.TSAGateFn.apply(pooled, pooled, pooled)
    gate.sum().backward()
    torch.cuda.synchronize()
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) for v in (emb, ref, al))
    assert tuple(ref.grad.shape) == tuple(ref.shape)
    assert math.isfinite(float(gate.sum()))
