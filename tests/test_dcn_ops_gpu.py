"""Every kernel of include/sr_hip_dcn.h against the float64 restatement tests/dcn_restate.py, on its production dispatch paths.

sr_dcn_fwd_f32 runs dcn_fwd_f32_kernel<COT, PT> (dcn_ops.hip): four instances, chosen by cout and the launch size; the choice
cannot be observed on the device, so it is restated in tests/test_dcn_host.py (_dcn_instance, pinned there against the code
object) and test_dispatch_coverage checks that the cases below reach all four, on both sides of the 4-row / 8-row switch.

Conventions (tests/test_convd_ops_gpu.py): blocks outside a window hold SENTINEL and must come back unchanged; pad channels of
the offset and mask tensors hold arbitrary finite values and must not matter; batch >= 2.  Every input is an fp32 value, so the
float64 reference starts from the same numbers.

Bounds are derived, not fitted.  EPS = 2^-24.  For every output element let A be the same operation on absolute values in
float64 (|bias| + sum |W| |mask| sum_c w_c |v_c|).  Then |y - y64| <= k EPS A + EPS |y64| (+ the coordinate term) with k counted
from the kernel's own operation order:
  forward   k = 2 * 9 * cin + K_SAMPLE + K_EPI (+ K_SIGMOID with a logit mask)
            2 * 9 * cin  two roundings per product of the one MFMA chain over (cin block, tap, channel)
            K_SAMPLE = 8 the sample ((w1 v1 + w2 v2) + w3 v3) + w4 v4: four products, three adds; times the mask: one more.
                         The weights themselves are exact at dyadic offsets (checked on the CPU in test_dyadic_offsets_are_exact).
            K_EPI = 2    bias add and LeakyReLU product (a slope <= 1 only shrinks an error; where the rounded pre-activation
                         has the other sign than the exact one the branch difference is at most its own error)
            K_SIGMOID = 4  m = 1 / (1 + expf(-l)): HIP's documented expf accuracy is 1 ulp = 2 EPS relative (HIP programming
                         guide, "Math API: single precision", maximum ulp error of expf), which reaches m damped by
                         e / (1 + e) <= 1; one add and one correctly rounded IEEE division (this build has no fast-math and
                         hipcc divides fp32 correctly rounded by default): 2 + 1 + 1
  arbitrary offsets add one rounding to K_SAMPLE (the weight products are no longer exact) and, per sample,
            EPS (|h_im| + |w_im| + 2) S with S = |mask| * (sum of |v| over the valid corners), a bound of the sample's slope in
            either coordinate and in either of 1 - lh, 1 - lw: the fp32 roundings of h_im and w_im (each relative to its
            coordinate) and of 1 - lh and 1 - lw (each relative to 1).  This deviates from the single term
            EPS max(|h_im|, |w_im|, 1) S of the feature request, which covers one coordinate and neither 1 - l rounding; it is
            counted from the sampler's operations and is at most (2 max + 2) / max of that term.  The value is continuous
            across cell boundaries and across the `inside` test, so a floor or a test that differs between fp32 and float64
            is covered by the same term.
  zero offsets with unit mask must meet sr_convd_f32's plain-conv bound k = 2 * 9 * cin + 8 against float64 F.conv2d: the
            sampler then reproduces x exactly (weights 1, 0, 0, 0 and products by 1).
  backward  (dyadic offsets: every sample is at least 1/8 away from the kinks of floor)
            dz = gy * LeakyReLU'(y): one rounding; the reference takes the same branch as the device's saved output.
            dcol = Wt dz by sr_convd_f32 ksize 1:  K_COL = 2 * roundup8(cout) + 8 on A_col = sum_co |W| |dz|
            dweight  k = chain(ksize 1, cin = 9 cin) + K_SAMPLE (+ K_SIGMOID) + 1 on sum |dz| |col|, the chain count of
                     sr_convd_wgrad_f32 from tests/test_convd_ops_gpu.py (_wgradd_chain); dbias  k = chain + 1 on sum |dz|
            dmask    k = 2 cpg + 7 + K_COL on sum_c A_col sum_c' w |v|: cpg product-and-add terms in channel order, the
                     unmasked sample's 7 roundings, dcol's error.  With a logit mask the factor m (1 - m) adds K_DSIG = 37: m
                     carries 4 EPS; 1 - m one rounding plus 4 EPS m / (1 - m) <= 4 e^2 < 30 for logits in [-2, 2]; two
                     products.
            doffset  k = 2 cpg + 7 + 1 + K_COL (+ K_SIGMOID) on |m| sum_c A_col S_c (every coordinate weight is at most 1 in
                     magnitude, so S bounds sum |weight| |v|): seven roundings of the four-term coordinate derivative, one of
                     dcol * m
            dx       k = J + 2 + K_COL (+ K_SIGMOID) on the same scatter of absolute values, J = the largest number of
                     atomicAdds that reach one element in the case (counted from the case's offsets in float64): one rounding
                     per add in whatever order they arrive, two products per contribution.

Sensitivity is asserted, not assumed.  Every forward case weights the last source channel by +1/2 on every tap and plants
spikes in the last image on that channel; offsets at chosen output pixels fetch them with the centre tap from 7 columns across
a 32-column strip boundary, from across a row-tile boundary, from the image's last row and column, and from just outside
(h_im = -1/2 and H - 1/2).  Each spike's contribution must exceed four bounds: a kernel that clamps samples to a staged halo,
drops partially outside samples, or skips the last image or block fails.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from image_restoration_amd import hip_autograd as A
from image_restoration_amd import hip_ops as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_restate as R  # noqa: E402
from test_convd_ops_gpu import _wgradd_chain  # noqa: E402
from test_dcn_host import _dcn_instance  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
TINY = 1e-30
SENTINEL = 12345.0
K_SAMPLE, K_EPI, K_SIGMOID, K_DSIG = 8, 2, 4, 37
SPIKE = 64.0


@pytest.fixture(scope='module')
def cuda():
    return torch.device('cuda:0')


def _f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).double()


def _cb8_buf(x, cuda, pad_fill=0.0, guard=1):
    """NCHW float64 -> device buffer [n][guard + blocks + guard][h][w][8]: x in the middle window (pad channels = pad_fill),
    SENTINEL blocks around it.  Returns (buffer, window)."""
    n, c, h, w = x.shape
    nb = (c + 7) // 8
    buf = torch.full((n, nb + 2 * guard, h, w, 8), SENTINEL, dtype=torch.float32)
    xp = torch.full((n, nb * 8, h, w), pad_fill, dtype=torch.float64)
    xp[:, :c] = x
    buf[:, guard:guard + nb] = xp.reshape(n, nb, 8, h, w).permute(0, 1, 3, 4, 2).float()
    buf = buf.to(cuda)
    return buf, H.CB8(buf, guard, nb)


def _nchw(win, c):
    b = win.buf[:, win.cb0:win.cb0 + win.cbn].cpu().double()
    n, nb, h, w, _ = b.shape
    return b.permute(0, 1, 4, 2, 3).reshape(n, nb * 8, h, w)[:, :c]


def _sentinel_kept(win, what):
    b = win.buf.cpu()
    assert bool((b[:, :win.cb0] == SENTINEL).all()) and bool((b[:, win.cb0 + win.cbn:] == SENTINEL).all()), (what, 'wrote outside')


def _check(got, ref, bound, what):
    bound = bound + EPS * ref.abs() + TINY
    err = (got - ref).abs()
    bad = ~(err <= bound)
    ratio = float((err / bound).nan_to_num(1e30).max())
    print(f'{what}: max err / bound = {ratio:.3f}, max err = {float(err.max()):.3e}')
    assert not bool(bad.any()), (what, int(bad.sum()), ratio, float(err.nan_to_num(1e30).max()))
    return bound


# ----------------------------------------------------------------------------------------------------------------- cases
def _offsets(rng, kind, shape):
    if kind == 'dyadic':   # an integer in [-3, 3] plus a multiple of 1/16 in [2/16, 14/16]
        return _f32(rng.integers(-3, 4, shape) + rng.integers(2, 15, shape) / 16.0)
    if kind == 'arbitrary':
        return _f32(rng.standard_normal(shape) * 2.0)
    return torch.zeros(shape, dtype=torch.float64)


def _make(cin, dg, cout, n, h, w, kind, logit, seed, th=None):
    """The float64 operands of one case (every value an fp32 number), far-sample spikes planted when ``th`` (the tile height
    of the launch) is given.  Returns a dict; 'mask_in' is what the device gets (values or logits), 'mask' the values."""
    rng = np.random.default_rng(seed)
    x = _f32(rng.standard_normal((n, cin, h, w)))
    wt = _f32(rng.standard_normal((cout, cin, 3, 3)) * (1.0 / (cin * 9)) ** 0.5)
    wt[:, -1] = 0.5
    bias = _f32(rng.standard_normal((cout,)) * 0.5)
    off = _offsets(rng, kind, (n, 18 * dg, h, w))
    if kind == 'zero':
        mask_in = torch.ones((n, 9 * dg, h, w), dtype=torch.float64)
    elif logit:
        mask_in = _f32(rng.uniform(-2.0, 2.0, (n, 9 * dg, h, w)))
    else:
        mask_in = _f32(rng.uniform(0.0, 1.0, (n, 9 * dg, h, w)))
    spikes = []
    if th is not None and kind != 'zero':
        g = dg - 1
        ch_h, ch_w, ch_m = 18 * g + 8, 18 * g + 9, 9 * g + 4          # the centre tap (k = 4) of the last group
        B = th if h > th else None
        want = [((h // 2, 34.0), (h // 2, 27))] if w > 34 else []      # 7 columns across the strip boundary at 32
        if B is not None:
            want.append(((float(min(B + 1, h - 1)), 5.0), (B - 3, 5)))  # across the row-tile boundary
        want += [((h - 1.0, w - 1.0), (h - 2, w - 5)),                 # the image's last row and column
                 ((-0.5, 9.0), (1, 9)), ((h - 0.5, 11.0), (h - 2, 11))]  # just outside: one corner row in the image, weight 1/2
        for (ys, xs), (yo, xo) in want:
            x[-1, -1, int(min(max(math.ceil(ys) if ys < 0 else math.floor(ys), 0), h - 1)), int(xs)] += SPIKE
            off[-1, ch_h, yo, xo], off[-1, ch_w, yo, xo] = ys - yo, xs - xo   # centre tap: h_im = yo + oh, w_im = xo + ow
            mask_in[-1, ch_m, yo, xo] = 2.0 if logit else 1.0
            spikes.append((yo, xo))
    mask = torch.sigmoid(mask_in) if (logit and kind != 'zero') else mask_in
    return dict(x=x, wt=wt, bias=bias, off=off, mask_in=mask_in, mask=mask, spikes=spikes, dg=dg, logit=logit and kind != 'zero')


def _coord_term(c):
    """sum |W| EPS (|h_im| + |w_im| + 2) S, S = |mask| * sum of |v| over the valid corners  (module docstring)."""
    x, off, dg = c['x'], c['off'], c['dg']
    n, cin, h, w = x.shape
    h_im, w_im = R.positions(off, dg)
    mag = h_im.abs() + w_im.abs() + 2                                                            # [n, dg, 9, h, w]
    S = R.columns(x.abs(), off, c['mask'].abs(), dg, corner_weights='ones').reshape(n, dg, cin // dg, 9, h, w)
    T = (S * mag.unsqueeze(2)).reshape(n, cin, 9, h, w)
    cout = c['wt'].shape[0]
    return EPS * torch.einsum('ock,nckhw->nohw', c['wt'].abs().reshape(cout, cin, 9), T)


def _run_forward(cuda, c, use_bias, slope, out_guard=1):
    x, wt, off, dg = c['x'], c['wt'], c['off'], c['dg']
    n, cin, h, w = x.shape
    cout = wt.shape[0]
    _, xw = _cb8_buf(x, cuda)
    _, ow = _cb8_buf(off, cuda, pad_fill=7.5)
    _, mw = _cb8_buf(c['mask_in'], cuda, pad_fill=-3.25)
    _, yw = _cb8_buf(torch.zeros((n, cout, h, w), dtype=torch.float64), cuda, guard=out_guard)
    yw.buf[:, yw.cb0:yw.cb0 + yw.cbn] = SENTINEL / 2
    pc = H.PackedConvK(wt.float().to(cuda), c['bias'].float().to(cuda) if use_bias else None)
    H.dcn_fwd(xw, ow, mw, pc, dg, mask_is_logit=c['logit'], act_slope=slope, out=yw)
    torch.cuda.synchronize()
    _sentinel_kept(yw, 'dcn_fwd')
    return _nchw(yw, cout)


# (cin, dg, cout, n, h, w).  The launch's instance (_dcn_instance): the two sizes of every channel combination run 4-row tiles
# (COT 2 for cout 64, COT 1 for 24 / 32); the last four are the two sides of the 4-row / 8-row switch (256 and 252 tiles at the
# 8-row rule, H = 5: a partial 8-row tile) for both COT.
COMBOS = [(64, 8, 64), (32, 2, 32), (16, 1, 24), (128, 8, 64)]
SIZES = [(2, 13, 35), (2, 5, 70)]
SWITCH = [(16, 2, 64, 64, 5, 128), (16, 2, 64, 63, 5, 128), (16, 1, 24, 64, 5, 128), (16, 1, 24, 63, 5, 128)]
FWD_CASES = [c + s for c in COMBOS for s in SIZES] + SWITCH
# (with bias, act_slope, mask as logits), dealt round-robin so that every option meets every offset kind and both sizes
VARIANTS = [(True, 1.0, False), (False, 0.1, True), (True, 0.1, False), (False, 1.0, True), (True, 0.1, True), (False, 1.0, False),
            (True, 1.0, True), (False, 0.1, False)]


def _cid(c):
    return '{}g{}to{}-n{}-{}x{}'.format(*c)


def test_dispatch_coverage():
    inst = {c: _dcn_instance(c[2], c[3], c[4], c[5]) for c in FWD_CASES}
    assert {v[:2] for v in inst.values()} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    assert inst[SWITCH[0]][:2] == (2, 2) and inst[SWITCH[1]][:2] == (2, 1) and inst[SWITCH[2]][:2] == (1, 2) \
        and inst[SWITCH[3]][:2] == (1, 1)
    for c in FWD_CASES[:8]:
        assert inst[c][1] == 1 and inst[c][2] >= 2 and c[4] % 4 != 0 and c[5] % 32 != 0 and c[5] > 64 - 32   # partial last tiles
    assert all(c[5] > 64 for c in FWD_CASES if c[4] == 5)                                               # >= 3 strips
    assert {(c[0] // c[1]) // 8 for c in COMBOS} == {1, 2}                                               # blocks per group


def test_dyadic_offsets_are_exact():
    """The fp32 coordinates and the four bilinear weights of the dyadic offsets are exact (no coordinate term in their bound)."""
    rng = np.random.default_rng(3)
    off = _offsets(rng, 'dyadic', (2, 36, 13, 70))
    h64, w64 = R.positions(off, 2)
    h32, w32 = R.positions(off.float(), 2)
    assert torch.equal(h32.double(), h64) and torch.equal(w32.double(), w64)
    for a32, a64 in ((h32, h64), (w32, w64)):
        l32, l64 = a32 - torch.floor(a32), a64 - torch.floor(a64)
        assert torch.equal(l32.double(), l64) and torch.equal((1 - l32).double(), 1 - l64)
        assert float((l64 - 0.5).abs().max()) <= 0.375                                                  # 1/8 away from the kinks
    lh32, lw32 = h32 - torch.floor(h32), w32 - torch.floor(w32)
    lh64, lw64 = lh32.double(), lw32.double()
    for p32, p64 in (((1 - lh32) * (1 - lw32), (1 - lh64) * (1 - lw64)), ((1 - lh32) * lw32, (1 - lh64) * lw64),
                     (lh32 * (1 - lw32), lh64 * (1 - lw64)), (lh32 * lw32, lh64 * lw64)):
        assert torch.equal(p32.double(), p64)


@pytest.mark.parametrize('kind', ['dyadic', 'arbitrary', 'zero'])
@pytest.mark.parametrize('case', FWD_CASES, ids=_cid)
def test_forward(cuda, case, kind):
    cin, dg, cout, n, h, w = case
    idx = FWD_CASES.index(case) + ['dyadic', 'arbitrary', 'zero'].index(kind) * 3
    use_bias, slope, logit = VARIANTS[idx % len(VARIANTS)]
    th = 4 * _dcn_instance(cout, n, h, w)[1]
    c = _make(cin, dg, cout, n, h, w, kind, logit, 100 + idx, th=th)
    got = _run_forward(cuda, c, use_bias, slope)
    bias = c['bias'] if use_bias else None
    if kind == 'zero':    # the plain-conv bound of sr_convd_f32 against float64 F.conv2d
        z = F.conv2d(c['x'], c['wt'], bias, padding=1)
        Aabs = F.conv2d(c['x'].abs(), c['wt'].abs(), bias.abs() if use_bias else None, padding=1)
        k = 2 * 9 * cin + 8
    else:
        z = R.modulated_deform_conv(c['x'], c['off'], c['mask'], c['wt'], bias, dg)
        Aabs = R.modulated_deform_conv(c['x'].abs(), c['off'], c['mask'].abs(), c['wt'].abs(), bias.abs() if use_bias else None, dg)
        k = 2 * 9 * cin + K_SAMPLE + K_EPI + (K_SIGMOID if c['logit'] else 0)
    bound = k * EPS * Aabs
    if kind == 'arbitrary':   # the weight products (1 - lh)(1 - lw), ... are no longer exact: one more rounding per sample
        bound = bound + EPS * Aabs + _coord_term(c)
    ref = F.leaky_relu(z, slope) if slope != 1.0 else z
    bound = _check(got, ref, bound, f'forward {_cid(case)} {kind} bias={use_bias} slope={slope} logit={c["logit"]}')
    if c['spikes']:
        x0 = c['x'].clone()
        x0[-1, -1] = torch.where(x0[-1, -1] > SPIKE / 2, x0[-1, -1] - SPIKE, x0[-1, -1])
        z0 = R.modulated_deform_conv(x0, c['off'], c['mask'], c['wt'], bias, dg)
        assert len(c['spikes']) >= 4
        for yo, xo in c['spikes']:
            contrib = (z[-1, :, yo, xo] - z0[-1, :, yo, xo]).abs() * (slope if slope != 1.0 else 1.0)
            assert bool((contrib > 4 * bound[-1, :, yo, xo]).all()), ('spike', yo, xo, float(contrib.min()), float(bound[-1, :, yo, xo].max()))


def test_forward_reads_two_windows_of_one_tensor(cuda):
    """The DCNv2Pack layout at dg = 8: offsets in blocks [0, 18) and mask logits in blocks [18, 27) of one 216-channel tensor
    with its own image stride, next to SENTINEL blocks."""
    cin, dg, cout, n, h, w = 64, 8, 64, 2, 13, 35
    c = _make(cin, dg, cout, n, h, w, 'dyadic', True, 7, th=4)
    both = torch.cat([c['off'], c['mask_in']], dim=1)
    buf, win = _cb8_buf(both, cuda)
    _, xw = _cb8_buf(c['x'], cuda)
    pc = H.PackedConvK(c['wt'].float().to(cuda), c['bias'].float().to(cuda))
    out = H.dcn_fwd(xw, H.CB8(buf, 1, 18), H.CB8(buf, 19, 9), pc, dg, mask_is_logit=True, act_slope=0.1)
    z = R.modulated_deform_conv(c['x'], c['off'], c['mask'], c['wt'], c['bias'], dg)
    Aabs = R.modulated_deform_conv(c['x'].abs(), c['off'], c['mask'], c['wt'].abs(), c['bias'].abs(), dg)
    _check(_nchw(out, cout), F.leaky_relu(z, 0.1), (2 * 9 * cin + K_SAMPLE + K_EPI + K_SIGMOID) * EPS * Aabs, 'windows')
    # the same image of sr_conv3x3_pack_f32 serves unchanged
    out2 = H.dcn_fwd(xw, H.CB8(buf, 1, 18), H.CB8(buf, 19, 9), H.PackedConv(c['wt'].float().to(cuda), c['bias'].float().to(cuda)), dg,
                     mask_is_logit=True, act_slope=0.1)
    assert torch.equal(out.buf, out2.buf)


def test_refusals(cuda):
    from image_restoration_amd import _lib
    import ctypes as C
    lib = _lib.load()
    c = _make(16, 2, 8, 2, 5, 9, 'dyadic', False, 1)
    _, xw = _cb8_buf(c['x'], cuda)
    _, ow = _cb8_buf(c['off'], cuda)
    _, mw = _cb8_buf(c['mask_in'], cuda)
    pc = H.PackedConvK(c['wt'].float().to(cuda), None)
    out = H.CB8.empty(2, 8, 5, 9, cuda)

    def desc(**kw):
        d = H._dcn_desc(_lib.DcnDesc(), xw, ow, mw, 2, False, 8)
        d.wpacked, d.out, d.out_img_stride = pc.w.data_ptr(), out.ptr, out.img_stride
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    st = torch.cuda.current_stream().cuda_stream
    assert lib.sr_dcn_fwd_f32(C.byref(desc()), st) == 0
    for kw in (dict(ksize=5), dict(stride=2), dict(padding=0), dict(dilation=2), dict(groups=2), dict(deformable_groups=4),
               dict(x=xw.ptr + 4), dict(offset=ow.ptr + 8), dict(out=out.ptr + 4), dict(wpacked=None)):
        assert lib.sr_dcn_fwd_f32(C.byref(desc(**kw)), st) == -1, kw           # SR_EINVAL
        assert lib.sr_last_error().decode() != ''
    cols = torch.empty(16, device=cuda)
    assert lib.sr_dcn_cols_f32(C.byref(desc()), cols.data_ptr(), 64, st) == -3  # SR_ENOSPACE
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------------------------- backward
BWD_CASES = [(64, 8, 64, 2, 13, 35), (32, 2, 32, 2, 5, 70), (16, 1, 24, 2, 13, 35), (128, 8, 64, 2, 5, 70)]
BWD_VARIANTS = [(True, 0.1, True), (True, 1.0, False), (False, 0.1, False), (True, 1.0, True)]   # bias, act_slope, logit


def _device_leaves(cuda, c, use_bias, req=(True, True, True, True, True)):
    def leaf(t, need, pad=0.0):
        n, ch, h, w = t.shape
        nb = (ch + 7) // 8
        tp = torch.full((n, nb * 8, h, w), pad, dtype=torch.float64)
        tp[:, :ch] = t
        return tp.reshape(n, nb, 8, h, w).permute(0, 1, 3, 4, 2).float().contiguous().to(cuda).requires_grad_(need)
    xs = leaf(c['x'], req[0])
    os_ = leaf(c['off'], req[1], 7.5)
    ms = leaf(c['mask_in'], req[2], -3.25)
    ws = c['wt'].float().to(cuda).requires_grad_(req[3])
    bs = c['bias'].float().to(cuda).requires_grad_(req[4]) if use_bias else None
    return xs, os_, ms, ws, bs


def _cb8_to_nchw(t, ch):
    n, nb, h, w, _ = t.shape
    return t.detach().cpu().double().permute(0, 1, 4, 2, 3).reshape(n, nb * 8, h, w)[:, :ch]


def _run_backward(cuda, c, use_bias, slope, gy, req=(True, True, True, True, True)):
    xs, os_, ms, ws, bs = _device_leaves(cuda, c, use_bias, req)
    y = A.DCNFn.apply(xs, os_, ms, ws, bs, slope, c['dg'], c['logit'])
    n, cout, h, w = gy.shape
    gyd = gy.reshape(n, cout // 8, 8, h, w).permute(0, 1, 3, 4, 2).float().contiguous().to(cuda)
    y.backward(gyd)
    torch.cuda.synchronize()
    g = lambda t: None if t is None or t.grad is None else t.grad  # noqa: E731
    return y.detach(), g(xs), g(os_), g(ms), g(ws), g(bs)


@pytest.fixture(scope='module')
def bwd_runs(cuda):
    """Every backward case once on the device (twice for the reproducibility test) and once in float64, shared by the tests."""
    runs = {}
    for case, (use_bias, slope, logit) in zip(BWD_CASES, BWD_VARIANTS):
        cin, dg, cout, n, h, w = case
        c = _make(cin, dg, cout, n, h, w, 'dyadic', logit, 900 + cin + dg)
        gy = _f32(np.random.default_rng(17 + cin).standard_normal((n, cout, h, w)))
        dev = [_run_backward(cuda, c, use_bias, slope, gy) for _ in range(2)]
        runs[case] = (c, use_bias, slope, gy, dev)
    return runs


def _reference_grads(c, use_bias, slope, gy, y_dev):
    """float64 autograd of the restatement; the LeakyReLU branch is the device's saved output's (dz = gy * slope where y <= 0)."""
    leaves = [c['x'].clone().requires_grad_(True), c['off'].clone().requires_grad_(True), c['mask_in'].clone().requires_grad_(True),
              c['wt'].clone().requires_grad_(True), c['bias'].clone().requires_grad_(True)]
    x, off, mi, wt, b = leaves
    z = R.modulated_deform_conv(x, off, torch.sigmoid(mi) if c['logit'] else mi, wt, b if use_bias else None, c['dg'])
    dz = gy * torch.where(y_dev > 0, torch.ones_like(gy), torch.full_like(gy, slope)) if slope != 1.0 else gy
    grads = torch.autograd.grad(z, leaves[:4] + ([b] if use_bias else []), dz)
    return dz, grads


def _refs_and_bounds(case, c, use_bias, slope, gy, y):
    """{name: (float64 gradient, bound without the EPS |ref| term)} for dx, doffset, dmask, dweight, dbias (module docstring),
    given the device's saved output ``y`` (CB8)."""
    cin, dg, cout, n, h, w = case
    cpg = cin // dg
    ksig = K_SIGMOID if c['logit'] else 0
    x, off, m, wt = c['x'], c['off'], c['mask'], c['wt']
    dz, ref = _reference_grads(c, use_bias, slope, gy, _cb8_to_nchw(y, cout))
    adz = dz.abs() * (1 + EPS)
    cols_abs = R.columns(x.abs(), off, m.abs(), dg)                                       # |mask| sum w |v|
    samp_abs = R.columns(x.abs(), off, torch.ones_like(m), dg)                            # sum w |v|
    S = R.columns(x.abs(), off, torch.ones_like(m), dg, corner_weights='ones')            # sum |v| over valid corners
    Acol = torch.einsum('ock,nohw->nckhw', wt.abs().reshape(cout, cin, 9), adz)
    K_COL = 2 * ((cout + 7) // 8 * 8) + 8
    chain = _wgradd_chain(n, h, w, cout, 9 * cin, 1, 1)
    out = {}
    Aw = torch.einsum('nohw,nckhw->ock', adz, cols_abs).reshape(cout, cin, 3, 3)
    out['dweight'] = (ref[3], (chain + K_SAMPLE + ksig + 1) * EPS * Aw)
    if use_bias:
        out['dbias'] = (ref[4], (chain + 1) * EPS * adz.sum(dim=(0, 2, 3)))
    Am = (Acol * samp_abs).reshape(n, dg, cpg, 9, h, w).sum(dim=2).reshape(n, 9 * dg, h, w)
    km = 2 * cpg + 7 + K_COL
    if c['logit']:
        Am, km = Am * m * (1 - m), km + K_DSIG
    out['dmask'] = (ref[2], km * EPS * Am)
    Ao = (Acol * S).reshape(n, dg, cpg, 9, h, w).sum(dim=2) * m.reshape(n, dg, 9, h, w)   # both channels of a pair: S
    Ao = Ao.unsqueeze(3).expand(n, dg, 9, 2, h, w).reshape(n, 18 * dg, h, w)
    out['doffset'] = (ref[1], (2 * cpg + 8 + K_COL + ksig) * EPS * Ao)
    xa = x.abs().clone().requires_grad_(True)
    Ax, = torch.autograd.grad(R.columns(xa, off, m.abs(), dg), xa, Acol)
    xo = torch.ones_like(x).requires_grad_(True)
    J, = torch.autograd.grad(R.columns(xo, off, torch.ones_like(m), dg, corner_weights='ones'), xo,
                             torch.ones((n, cin, 9, h, w), dtype=torch.float64))
    jmax = int(J.max())
    print(f'dx {_cid(case)}: at most {jmax} adds reach one element')
    out['dx'] = (ref[0], (jmax + 2 + K_COL + ksig) * EPS * Ax)
    return out


@pytest.mark.parametrize('case', BWD_CASES, ids=_cid)
def test_backward(cuda, bwd_runs, case):
    c, use_bias, slope, gy, dev = bwd_runs[case]
    cin, dg, cout, n, h, w = case
    what = f'{_cid(case)} bias={use_bias} slope={slope} logit={c["logit"]}'
    for run, (y, dx, doff, dmsk, dw, db) in enumerate(dev):
        rb = _refs_and_bounds(case, c, use_bias, slope, gy, y)
        _check(dw.detach().cpu().double(), *rb['dweight'], f'dweight run {run} {what}')
        if use_bias:
            _check(db.detach().cpu().double(), *rb['dbias'], f'dbias run {run} {what}')
        else:
            assert db is None
        _check(_cb8_to_nchw(dmsk, 9 * dg), *rb['dmask'], f'dmask run {run} {what}')
        _check(_cb8_to_nchw(doff, 18 * dg), *rb['doffset'], f'doffset run {run} {what}')
        _check(_cb8_to_nchw(dx, cin), *rb['dx'], f'dx run {run} {what}')
        for t, ch in ((doff, 18 * dg), (dmsk, 9 * dg)):   # pad channels of the offset / mask gradients are zero
            full = t.detach().cpu().permute(0, 1, 4, 2, 3).reshape(n, -1, h, w)
            assert full.shape[1] == ch or float(full[:, ch:].abs().max()) == 0.0


@pytest.mark.parametrize('case', BWD_CASES, ids=_cid)
def test_reproducibility(bwd_runs, case):
    """Two runs are bit-identical in y, doffset, dmask, dweight and dbias; dx only has to meet its bound both times
    (test_backward checks both runs)."""
    _, use_bias, _, _, dev = bwd_runs[case]
    (y0, _, do0, dm0, dw0, db0), (y1, _, do1, dm1, dw1, db1) = dev
    assert torch.equal(y0, y1) and torch.equal(do0, do1) and torch.equal(dm0, dm1) and torch.equal(dw0, dw1)
    assert (db0 is None and db1 is None) or torch.equal(db0, db1)


@pytest.mark.parametrize('req', [(True, False, False, False, False), (False, True, True, False, False),
                                 (False, False, False, True, True), (False, True, False, True, False)])
def test_needs_input_grad_subsets_skip_work_but_change_no_value(cuda, bwd_runs, req):
    case = BWD_CASES[1]
    c, use_bias, slope, gy, dev = bwd_runs[case]
    full = dev[0]
    got = _run_backward(cuda, c, use_bias, slope, gy, req)
    assert torch.equal(got[0], full[0])
    for i, need in enumerate(req):
        g, f = got[1 + i], full[1 + i]
        if not need:
            assert g is None
        elif i == 0:    # dx: arrival order may differ; it has to meet its bound again
            _check(_cb8_to_nchw(g, case[0]), *_refs_and_bounds(case, c, use_bias, slope, gy, got[0])['dx'], 'dx of a subset')
        else:
            assert torch.equal(g, f), i
    if req[1] != req[2]:   # offsets without mask: the mask gradient is simply not returned
        assert (got[2] is None) != (got[3] is None)


def test_backward_through_two_windows_lands_in_one_gradient_tensor(cuda, bwd_runs):
    """DCNv2Pack's call: offsets and logits are windows of one tensor; its gradient is one tensor the kernel writes both windows
    of, bit-identical to the separate-tensor run."""
    case = BWD_CASES[0]
    c, use_bias, slope, gy, dev = bwd_runs[case]
    assert c['logit'] and c['dg'] == 8
    xs, os_, ms, ws, bs = _device_leaves(cuda, c, use_bias)
    co = torch.cat([os_.detach(), ms.detach()], dim=1).contiguous().requires_grad_(True)
    y = A.DCNFn.apply(xs, co, co, ws, bs, slope, 8, True, ((0, 18), (18, 9)))
    n, cout, h, w = gy.shape
    y.backward(gy.reshape(n, cout // 8, 8, h, w).permute(0, 1, 3, 4, 2).float().contiguous().to(cuda))
    torch.cuda.synchronize()
    assert torch.equal(y.detach(), dev[0][0])
    assert torch.equal(co.grad[:, :18], dev[0][2]) and torch.equal(co.grad[:, 18:], dev[0][3])
    assert torch.equal(ws.grad, dev[0][4])


@pytest.mark.parametrize('case,logit', [((32, 2, 32, 2, 5, 70), False), ((64, 8, 64, 2, 13, 35), True)], ids=['32g2', '64g8'])
def test_backward_data_keeps_to_its_windows(cuda, case, logit):
    """sr_dcn_bwd_data_f32 with dx, doffset and dmask as windows between SENTINEL blocks (dx's window zeroed, as the contract
    asks): the blocks outside come back unchanged, the pad channels of the last offset / mask block are not written (dg = 2:
    36 and 18 channels in 5 and 3 blocks), and the three gradients equal those of the unguarded call bit for bit (dx: within
    twice its bound, its adds may arrive in another order).  The columns and dcol are whole tensors by contract (no window)."""
    cin, dg, cout, n, h, w = case
    c = _make(cin, dg, cout, n, h, w, 'dyadic', logit, 31)
    _, xw = _cb8_buf(c['x'], cuda)
    _, ow = _cb8_buf(c['off'], cuda, pad_fill=7.5)
    _, mw = _cb8_buf(c['mask_in'], cuda, pad_fill=-3.25)
    dz = _f32(np.random.default_rng(5).standard_normal((n, cout, h, w)))
    _, dzw = _cb8_buf(dz, cuda)
    dcol = H.convd(dzw, H.PackedDcnT(c['wt'].float().to(cuda)))
    _, dxw = _cb8_buf(torch.zeros_like(c['x']), cuda)
    _, dow = _cb8_buf(torch.zeros_like(c['off']), cuda, pad_fill=SENTINEL)
    _, dmw = _cb8_buf(torch.zeros_like(c['mask_in']), cuda, pad_fill=SENTINEL)
    H.dcn_bwd_data(dcol, xw, ow, mw, dg, mask_is_logit=logit, dx=dxw, doffset=dow, dmask=dmw)
    torch.cuda.synchronize()
    for win, ch, what in ((dxw, cin, 'dx'), (dow, 18 * dg, 'doffset'), (dmw, 9 * dg, 'dmask')):
        _sentinel_kept(win, what)
        full = _nchw(win, win.cbn * 8)
        assert win.cbn * 8 == ch or bool((full[:, ch:] == SENTINEL).all()), (what, 'wrote pad channels')
    do2, dm2 = H.CB8.zeros(n, 18 * dg, h, w, cuda), H.CB8.zeros(n, 9 * dg, h, w, cuda)
    dx2 = H.dcn_bwd_data(dcol, xw, ow, mw, dg, mask_is_logit=logit, want_dx=True, doffset=do2, dmask=dm2)
    assert torch.equal(_nchw(dow, 18 * dg), _nchw(do2, 18 * dg)) and torch.equal(_nchw(dmw, 9 * dg), _nchw(dm2, 9 * dg))
    # dx against float64: the scatter of dcol as the device holds it (exact inputs), k = J + 2 (+ K_SIGMOID), module docstring
    dcol64 = _nchw(dcol, 9 * cin).reshape(n, 9, cin, h, w).permute(0, 2, 1, 3, 4)
    xr = c['x'].clone().requires_grad_(True)
    ref, = torch.autograd.grad(R.columns(xr, c['off'], c['mask'], dg), xr, dcol64)
    xa = c['x'].abs().clone().requires_grad_(True)
    Ax, = torch.autograd.grad(R.columns(xa, c['off'], c['mask'].abs(), dg), xa, dcol64.abs())
    xo = torch.ones_like(c['x']).requires_grad_(True)
    J, = torch.autograd.grad(R.columns(xo, c['off'], torch.ones_like(c['mask']), dg, corner_weights='ones'), xo,
                             torch.ones((n, cin, 9, h, w), dtype=torch.float64))
    k = int(J.max()) + 2 + (K_SIGMOID if logit else 0)
    for got, what in ((_nchw(dxw, cin), 'guarded dx'), (_nchw(dx2, cin), 'plain dx')):
        _check(got, ref, k * EPS * Ax, what)
