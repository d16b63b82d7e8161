"""The entry points of include/sr_hip_flow_bwd.h on the GPU, each against float64 at the bound its header states.  EPS = 2^-24.

  data gradient    K = 49 * 8 * ceil(cout / 8) fused multiply-adds from a zero accumulator: with A the same transposed
                   convolution of the absolute values, |got - exact| <= K * EPS * A; an element whose mask is not > 0 is exactly 0.
  weight gradient  the header's plan restated (``wgrad_plan``): T = 32 * RW / 4 terms per wave, 2 + NP reduction adds, then the
                   scale and the accumulating add: (T + 2 + NP) * EPS * sum|dy * x| * |scale| + 2 * EPS * (|scale * sum| + |preload|).
  level adjoint    d_up is bit for bit (g_res + g_in[6:8]) + dflow with dflow the existing flow-warp backward's; g_prev is the
                   float64 2 * U^T of that d_up, rounded once: EPS * |exact|.
  resize adjoint   elementwise the float64 transpose of the matrix the forward's float32 coordinate rule defines, rounded once;
                   and <R f, g> = <f, R^T g> with R f the forward kernel's output (one rounding per element on either side).
Each kernel has a negative control that leaves its bound: a reference without one tap (the convolutions) or with one corner
shifted (the adjoints)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
TINY = 1e-30
NAN = float('nan')
PAIRS = H.CONV7X7_SHAPES
PAIR_IDS = [f'{ci}to{co}' for ci, co in PAIRS]
MAPS = ((1, 1), (2, 2), (3, 2), (7, 9), (19, 37), (33, 70))      # below the halo, ragged tails each way, more than one tile
MAP_IDS = [f'{h}x{w}' for h, w in MAPS]


def _rng(seed):
    return np.random.default_rng(seed)


def _to_cb8(x, cuda, slack=1, pad=0.0):
    """[N, C, H, W] numpy -> CB8 window with ``slack`` NaN blocks on either side; pad channels of the last block hold ``pad``."""
    n, c, h, w = x.shape
    cb = (c + 7) // 8
    buf = torch.full((n, cb + 2 * slack, h, w, 8), NAN, dtype=torch.float32)
    xp = torch.full((n, cb * 8, h, w), pad, dtype=torch.float32)
    xp[:, :c] = torch.from_numpy(np.asarray(x, np.float32))
    buf[:, slack:slack + cb] = xp.reshape(n, cb, 8, h, w).permute(0, 1, 3, 4, 2)
    return H.CB8(buf.to(cuda), slack, cb)


def _from_cb8(t, c=None):
    b = t.buf[:, t.cb0:t.cb0 + t.cbn].cpu()
    n, cb, h, w, _ = b.shape
    return b.permute(0, 1, 4, 2, 3).reshape(n, cb * 8, h, w)[:, :c].double().numpy()


def _slack_untouched(t):
    return bool(torch.isnan(t.buf[:, :t.cb0]).all() and torch.isnan(t.buf[:, t.cb0 + t.cbn:]).all())


# ------------------------------------------------------------------------------------------------------- data gradient
_dgrad_cache = {}


def _dgrad_case(cin, cout, h, w, n):
    key = (cin, cout, h, w, n)
    if key not in _dgrad_cache:
        rng = _rng(7000 + 100 * cin + cout + 3 * h + n)
        dy = rng.standard_normal((n, cout, h, w)).astype(np.float32)
        wt = (rng.standard_normal((cout, cin, 7, 7)) / np.sqrt(49 * cout)).astype(np.float32)
        mask = rng.standard_normal((n, cin, h, w)).astype(np.float32)
        mask[mask < -0.8] = 0.0                              # exact zeros are "not positive" too
        td, tw = torch.from_numpy(dy).double(), torch.from_numpy(wt).double()
        want = F.conv_transpose2d(td, tw, padding=3).numpy()
        mag = F.conv_transpose2d(td.abs(), tw.abs(), padding=3).numpy()
        _dgrad_cache[key] = (dy, wt, mask, want, mag)      # computed once, shared, never modified
    return _dgrad_cache[key]


@pytest.mark.parametrize('hw', MAPS, ids=MAP_IDS)
@pytest.mark.parametrize('pair', PAIRS, ids=PAIR_IDS)
def test_conv7x7_dgrad_matches_float64(cuda, pair, hw):
    cin, cout = pair
    h, w = hw
    lib = _lib.load()
    assert lib.sr_conv7x7_dgrad_instance(cout, cin) == (1 if cin == 64 else 0)
    for n in (1, 2):
        dy, wt, mask, want, mag = _dgrad_case(cin, cout, h, w, n)
        pc = H.PackedConv7x7(torch.from_numpy(wt).to(cuda), None, mode=1)
        assert pc.mode == 1 and pc.w.numel() == lib.sr_conv7x7_dgrad_packed_floats(cout, cin)
        bound = 49 * 8 * ((cout + 7) // 8) * EPS * mag + TINY
        for use_mask in (False, True):
            src = _to_cb8(dy, cuda)                              # pad channels of dy (cout = 2) are finite: zeros
            out = H.CB8(torch.full((n, cin // 8 + 2, h, w, 8), NAN, dtype=torch.float32, device=cuda), 1, cin // 8)
            m = _to_cb8(mask, cuda) if use_mask else None
            H.conv7x7_dgrad(src, pc, out=out, mask=m)
            got = _from_cb8(out)
            ref = np.where(mask > 0, want, 0.0) if use_mask else want
            err = np.abs(got - ref)
            assert np.isfinite(got).all() and (err <= bound).all(), (pair, hw, n, use_mask, float((err / bound).max()))
            if use_mask:
                assert (got[mask <= 0] == 0).all()
            assert _slack_untouched(out) and _slack_untouched(src)                    # nothing outside the window is written
    # negative control: the reference without the centre tap of the last dy channel leaves the bound
    wd = np.zeros_like(wt)
    wd[-1, :, 3, 3] = wt[-1, :, 3, 3]
    dropped = F.conv_transpose2d(torch.from_numpy(dy).double(), torch.from_numpy(wd).double(), padding=3).numpy()
    assert (np.abs(dropped) > 4 * bound).any(), (pair, hw)


def test_conv7x7_dgrad_batches_and_reruns_are_bit_identical(cuda):
    for cin, cout in PAIRS:
        dy, wt, mask, want, mag = _dgrad_case(cin, cout, 19, 37, 2)
        pc = H.PackedConv7x7(torch.from_numpy(wt).to(cuda), None, mode=1)
        run = lambda a, b: H.conv7x7_dgrad(_to_cb8(a, cuda, 0), pc, mask=_to_cb8(b, cuda, 0)).buf   # noqa: E731
        both, again = run(dy, mask), run(dy, mask)
        one = [run(dy[i:i + 1], mask[i:i + 1]) for i in range(2)]
        assert torch.equal(both, again) and torch.equal(both, torch.cat(one, 0)), (cin, cout)


def test_conv7x7_dgrad_wrapper_refusals(cuda):
    with pytest.raises(ValueError, match='not supported'):
        H.PackedConv7x7(torch.zeros(16, 8, 7, 7, device=cuda), None, mode=1)
    with pytest.raises(ValueError, match='mode 2 is not supported'):
        H.PackedConv7x7(torch.zeros(32, 8, 7, 7, device=cuda), None, mode=2)
    fwd, bwd = H.PackedConv7x7(torch.zeros(32, 8, 7, 7, device=cuda)), H.PackedConv7x7(torch.zeros(32, 8, 7, 7, device=cuda), None, mode=1)
    with pytest.raises(ValueError, match='mode 1'):
        H.conv7x7_dgrad(H.CB8.zeros(1, 32, 4, 4, cuda), fwd)
    with pytest.raises(ValueError, match='mode 0'):
        H.conv7x7(H.CB8.zeros(1, 8, 4, 4, cuda), bwd)
    with pytest.raises(ValueError, match='channel blocks'):
        H.conv7x7_dgrad(H.CB8.zeros(1, 16, 4, 4, cuda), bwd)
    with pytest.raises(ValueError, match='mask does not fit'):
        H.conv7x7_dgrad(H.CB8.zeros(1, 32, 4, 4, cuda), bwd, mask=H.CB8.zeros(1, 8, 4, 5, cuda))


# ----------------------------------------------------------------------------------------------------- weight gradient
def wgrad_plan(n, h, w, cout, cin):
    """The plan include/sr_hip_flow_bwd.h states: (RW, NP, slab bytes)."""
    cdiv = lambda a, b: -(-a // b)   # noqa: E731
    ct, it, tx = cdiv(cout, 32), cdiv(cin, 32), cdiv(w, 32)
    chunks = min(max(cdiv(1024, n * tx * ct * it * 7), 1), cdiv(h, 4))
    rw = 4 * cdiv(cdiv(h, chunks), 4)
    chunks = cdiv(h, rw)
    np_ = n * chunks * tx
    return rw, np_, 4 * np_ * (ct * it * 49 * 1024 + ct * 64)


_wgrad_cache = {}


def _wgrad_case(cin, cout, h, w, n):
    key = (cin, cout, h, w, n)
    if key not in _wgrad_cache:
        rng = _rng(9000 + 100 * cin + cout + 3 * h + n)
        x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
        dy = rng.standard_normal((n, cout, h, w)).astype(np.float32)
        xp = np.zeros((n, cin, h + 6, w + 6))
        xp[:, :, 3:3 + h, 3:3 + w] = x
        d2 = dy.astype(np.float64).transpose(1, 0, 2, 3).reshape(cout, -1)
        dw, mag = np.zeros((cout, cin, 7, 7)), np.zeros((cout, cin, 7, 7))
        for ty in range(7):
            for tx in range(7):
                s = xp[:, :, ty:ty + h, tx:tx + w].transpose(1, 0, 2, 3).reshape(cin, -1)
                dw[:, :, ty, tx] = d2 @ s.T
                mag[:, :, ty, tx] = np.abs(d2) @ np.abs(s).T
        _wgrad_cache[key] = (x, dy, dw, mag, d2.sum(1), np.abs(d2).sum(1))
    return _wgrad_cache[key]


def _check_wgrad(cuda, cin, cout, h, w, n):
    x, dy, dw, mag, db, bmag = _wgrad_case(cin, cout, h, w, n)
    rw, np_, slab_bytes = wgrad_plan(n, h, w, cout, cin)
    assert _lib.load().sr_conv7x7_wgrad_slab_bytes(n, h, w, cout, cin) == slab_bytes
    depth = 32 * rw // 4 + 2 + np_
    src, d = _to_cb8(x, cuda), _to_cb8(dy, cuda, pad=NAN)          # pad couts of dy are computed and discarded: NaN is harmless
    scale = -0.75
    gw, gb = H.conv7x7_wgrad(src, d, cout, cin, scale=scale)
    assert tuple(gw.shape) == (cout, cin, 7, 7) and tuple(gb.shape) == (cout,)
    bw = depth * EPS * mag * abs(scale) + 2 * EPS * np.abs(scale * dw) + TINY
    bb = depth * EPS * bmag * abs(scale) + 2 * EPS * np.abs(scale * db) + TINY
    ew, eb = np.abs(gw.double().cpu().numpy() - scale * dw), np.abs(gb.double().cpu().numpy() - scale * db)
    assert (ew <= bw).all() and (eb <= bb).all(), ((cin, cout), (h, w), n, float((ew / bw).max()), float((eb / bb).max()))
    # reruns are bit-identical; no bias wanted: the weight gradient does not change
    gw2, gb2 = H.conv7x7_wgrad(src, d, cout, cin, scale=scale)
    gw3, none = H.conv7x7_wgrad(src, d, cout, cin, scale=scale, want_bias=False)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2) and torch.equal(gw, gw3) and none is None
    # accumulate into preloaded buffers (what a FlatAdam arena is): pre + scale * sum, one more rounding
    rng = _rng(h + w)
    pw = torch.from_numpy(rng.standard_normal((cout, cin, 7, 7)).astype(np.float32)).to(cuda)
    pb = torch.from_numpy(rng.standard_normal(cout).astype(np.float32)).to(cuda)
    aw, ab = pw.clone(), pb.clone()
    assert H.conv7x7_wgrad(src, d, cout, cin, scale=scale, out=(aw.data_ptr(), ab.data_ptr())) is None
    assert torch.equal(aw, pw + gw) and torch.equal(ab, pb + gb)       # the same scaled sum, added in fp32
    assert _slack_untouched(src) and _slack_untouched(d)
    return bw, dw, scale


@pytest.mark.parametrize('hw', MAPS, ids=MAP_IDS)
@pytest.mark.parametrize('pair', PAIRS, ids=PAIR_IDS)
def test_conv7x7_wgrad_matches_float64(cuda, pair, hw):
    cin, cout = pair
    for n in (1, 2):
        bw, dw, scale = _check_wgrad(cuda, cin, cout, hw[0], hw[1], n)
    # negative control: the reference without its centre tap leaves the bound
    assert (np.abs(scale * dw[:, :, 3, 3]) > 4 * bw[:, :, 3, 3]).any(), (pair, hw)


@pytest.mark.parametrize('pair', ((32, 64), (16, 2)), ids=['32to64', '16to2'])
def test_conv7x7_wgrad_strips_of_several_steps(cuda, pair):
    """Maps tall enough that a workgroup's strip has more than 4 rows: the staging loop wraps its two buffers (RW = 16: four
    steps), which none of the small maps reaches (their plan is RW = 4)."""
    cin, cout = pair
    h, w, n = (160, 70, 2) if cout == 64 else (320, 70, 4)
    assert wgrad_plan(n, h, w, cout, cin)[0] >= 12
    _check_wgrad(cuda, cin, cout, h, w, n)


def test_conv7x7_wgrad_wrapper_refusals(cuda):
    with pytest.raises(ValueError, match='not supported'):
        H.conv7x7_wgrad(H.CB8.zeros(1, 8, 4, 4, cuda), H.CB8.zeros(1, 16, 4, 4, cuda), 16, 8)
    with pytest.raises(ValueError, match='do not fit'):
        H.conv7x7_wgrad(H.CB8.zeros(1, 8, 4, 4, cuda), H.CB8.zeros(1, 32, 4, 5, cuda), 32, 8)


# ------------------------------------------------------------------------------------------------------- level adjoint
LEVEL_MAPS = ((2, 2), (4, 6), (8, 10), (34, 70))


def _up_matrix(n_out):
    """U of one axis, [n_out, n_out / 2], from the forward's float64 coordinate rule; ``shift`` moves one corner (the control)."""
    n_in = n_out // 2
    u = np.zeros((n_out, n_in))
    for d in range(n_out):
        s = d * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        i0 = min(int(s), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        f = s - i0
        u[d, i0] += 1.0 - f
        u[d, i1] += f
    return u


def _block(x, cuda, lead, tail):
    """A one-block CB8 tensor [N, 1, H, W, 8] in the middle of a flat NaN buffer: (the buffer, the view's data pointer, view)."""
    n, c, h, w = x.shape
    xp = np.zeros((n, 8, h, w), np.float32)
    xp[:, :c] = x
    flat = torch.full((lead + xp.size + tail,), NAN, dtype=torch.float32)
    flat[lead:lead + xp.size] = torch.from_numpy(xp).permute(0, 2, 3, 1).reshape(-1)
    flat = flat.to(cuda)
    return flat, flat[lead:lead + xp.size].view(n, 1, h, w, 8)


@pytest.mark.parametrize('kind', ['grid64', 'arbitrary'])
@pytest.mark.parametrize('hw', LEVEL_MAPS, ids=[f'{h}x{w}' for h, w in LEVEL_MAPS])
def test_level_input_bwd_is_warp_bwd_then_float64_upT(cuda, hw, kind):
    h, w = hw
    lib = _lib.load()
    for n in (1, 2):
        rng = _rng(300 + h + 7 * n + (kind == 'grid64'))
        supp = rng.standard_normal((n, 3, h, w)).astype(np.float32)
        flow = rng.uniform(-3.0, 3.0, (n, h, w, 2))
        flow = (np.round(flow * 64) / 64 if kind == 'grid64' else flow * 1.37).astype(np.float32)
        _, _, _, _, gx_on, gy_on = R.warp_coords(flow, h, w, 'border')
        clipped = 1.0 - float((gx_on & gy_on).mean())
        # a stated share of the samples is clipped on some axis: at least 2 %, and on the maps large enough to have an interior at
        # most 90 %, so that both branches of the clipping rule are met
        assert clipped >= 0.02 and (h * w < 80 or clipped <= 0.9), clipped
        g_in = rng.standard_normal((n, 8, h, w)).astype(np.float32)
        g_res = rng.standard_normal((n, 2, h, w)).astype(np.float32)
        t_supp = torch.from_numpy(supp).to(cuda)
        t_flow = torch.from_numpy(flow).to(cuda)
        up = H.CB8(_block(flow.transpose(0, 3, 1, 2), cuda, 16, 16)[1])
        gi, gr = H.CB8(_block(g_in, cuda, 16, 16)[1]), H.CB8(_block(g_res, cuda, 16, 16)[1])
        # the wrapper
        g_prev = H.spynet_level_input_bwd(t_supp, up, gi, gr)
        assert tuple(g_prev.buf.shape) == (n, 1, h // 2, w // 2, 8)
        # the C entry point on buffers with NaN slack around both destinations
        dflat = torch.full((8 + n * h * w * 2 + 8,), NAN, dtype=torch.float32, device=cuda)
        pflat = torch.full((16 + n * (h // 2) * (w // 2) * 8 + 16,), NAN, dtype=torch.float32, device=cuda)
        H.launch('sr_spynet_level_input_bwd_f32', cuda, t_supp.data_ptr(), up.ptr, gi.ptr, gr.ptr, dflat[8:].data_ptr(),
                 pflat[16:].data_ptr(), n, h, w)
        assert torch.isnan(dflat[:8]).all() and torch.isnan(dflat[-8:]).all() and torch.isnan(pflat[:16]).all() \
            and torch.isnan(pflat[-16:]).all()
        d_up = dflat[8:-8].view(n, h, w, 2)
        got = pflat[16:-16].view(n, 1, h // 2, w // 2, 8)
        assert torch.equal(got, g_prev.buf)                      # reruns are bit-identical
        # d_up: the composition, bit for bit
        _, dflow = H.flow_warp_bwd(t_supp, t_flow, torch.from_numpy(np.ascontiguousarray(g_in[:, 3:6])).to(cuda), 'border', want_dx=False)
        comp = (torch.from_numpy(g_res).to(cuda) + torch.from_numpy(np.ascontiguousarray(g_in[:, 6:8])).to(cuda)).permute(0, 2, 3, 1) + dflow
        assert torch.equal(d_up, comp), (hw, kind, n)
        # and dflow is the float64 restatement's on the kernel's own (float32) positions
        _, want_dflow, _, _ = R.flow_warp_bwd(supp, flow, g_in[:, 3:6], 'border', coord_dtype=np.float32)
        assert (np.abs(dflow.double().cpu().numpy() - want_dflow) <= EPS * np.abs(want_dflow) + 1e-12).all()
        # g_prev: 2 * Uy^T d_up Ux in float64, rounded once; pad channels 0
        uy, ux = _up_matrix(h), _up_matrix(w)
        d64 = d_up.double().cpu().numpy()
        want = 2.0 * np.einsum('yp,nyxc,xq->npqc', uy, d64, ux)
        mag = 2.0 * np.einsum('yp,nyxc,xq->npqc', uy, np.abs(d64), ux)
        gp = got[:, 0].double().cpu().numpy()
        bound = EPS * np.abs(want) + 1e-13 * mag + TINY
        err = np.abs(gp[..., :2] - want)
        assert (err <= bound).all(), (hw, kind, n, float((err / bound).max()))
        assert (gp[..., 2:] == 0).all()
        # batch independence
        if n == 2:
            one = H.spynet_level_input_bwd(t_supp[:1].contiguous(), H.CB8(up.buf[:1].contiguous()), H.CB8(gi.buf[:1].contiguous()),
                                           H.CB8(gr.buf[:1].contiguous()))
            assert torch.equal(one.buf, g_prev.buf[:1])
    # negative control: U^T with one corner of one fine row shifted leaves the bound
    bad = uy.copy()
    bad[h - 1] = np.roll(bad[h - 1], 1) if h > 2 else bad[h - 1] * 0.5
    wrong = 2.0 * np.einsum('yp,nyxc,xq->npqc', bad, d64, ux)
    assert (np.abs(wrong - want) > 4 * bound).any(), (hw, kind)


def test_level_input_bwd_refusals(cuda):
    img = torch.zeros(1, 3, 4, 6, device=cuda)
    blk = H.CB8.zeros(1, 8, 4, 6, cuda)
    with pytest.raises(ValueError, match='not even'):
        H.spynet_level_input_bwd(torch.zeros(1, 3, 5, 6, device=cuda), H.CB8.zeros(1, 8, 5, 6, cuda), H.CB8.zeros(1, 8, 5, 6, cuda),
                                 H.CB8.zeros(1, 8, 5, 6, cuda))
    with pytest.raises(ValueError, match='g_in must be one CB8 block'):
        H.spynet_level_input_bwd(img, blk, H.CB8.zeros(1, 16, 4, 6, cuda), blk)


# ------------------------------------------------------------------------------------------------------ resize adjoint
def _resize_matrix(n_in, n_out, shift_row=None):
    """R of one axis, [n_out, n_in], from the forward's float32 coordinate rule (include/sr_hip_degrade.h)."""
    f32 = np.float32
    scale = f32(n_in) / f32(n_out)
    r = np.zeros((n_out, n_in))
    for d in range(n_out):
        s = f32(f32(f32(d) + f32(0.5)) * scale) - f32(0.5)
        i0 = int(np.floor(s))
        f = float(f32(s - f32(np.floor(s))))
        if s < 0:
            i0, f = 0, 0.0
        if i0 >= n_in - 1:
            i0, f = n_in - 1, 0.0
        i1 = min(i0 + 1, n_in - 1)
        if d == shift_row:
            i0, i1 = max(i0 - 1, 0), max(i1 - 1, 0)
        r[d, i0] += 1.0 - f
        r[d, i1] += f
    return r


@pytest.mark.parametrize('sizes', [((70, 90), (96, 96)), ((96, 96), (70, 90)), ((1, 1), (3, 2)), ((5, 4), (5, 4))],
                         ids=['70x90to96x96', '96x96to70x90', '1x1to3x2', 'same'])
def test_resize_adjoint_is_the_transpose(cuda, sizes):
    (hs, ws), (hd, wd) = sizes
    rng = _rng(hs + wd)
    n, c = 2, 2
    f = rng.standard_normal((n, c, hs, ws)).astype(np.float32)
    g = rng.standard_normal((n, c, hd, wd)).astype(np.float32)
    lead = 32
    flat = torch.full((lead + f.size + lead,), NAN, dtype=torch.float32, device=cuda)
    tg = torch.from_numpy(g).to(cuda)
    H.launch('sr_resize_bilinear_adjoint_f32', cuda, tg.data_ptr(), flat[lead:].data_ptr(), n * c, hs, ws, hd, wd)
    assert torch.isnan(flat[:lead]).all() and torch.isnan(flat[-lead:]).all()
    got_t = H.resize_bilinear_adjoint(tg, (hs, ws))
    assert torch.equal(got_t.reshape(-1), flat[lead:-lead])                  # reruns are bit-identical
    got = got_t.double().cpu().numpy()
    ry, rx = _resize_matrix(hs, hd), _resize_matrix(ws, wd)
    want = np.einsum('dy,ncde,ex->ncyx', ry, g.astype(np.float64), rx)
    mag = np.einsum('dy,ncde,ex->ncyx', ry, np.abs(g).astype(np.float64), rx)
    bound = EPS * np.abs(want) + 1e-13 * mag + TINY
    err = np.abs(got - want)
    assert (err <= bound).all(), (sizes, float((err / bound).max()))
    # <R f, g> = <f, R^T g> with R f the forward kernel's own output
    tf = torch.from_numpy(f).to(cuda)
    rf = H.resize_bilinear(tf, (hd, wd)).double().cpu().numpy()
    lhs, rhs = float((rf * g).sum()), float((f.astype(np.float64) * got).sum())
    slack = EPS * (float(np.abs(rf * g).sum()) + float(np.abs(f * got).sum())) + TINY
    assert abs(lhs - rhs) <= slack, (sizes, lhs, rhs, slack)
    # negative control: the matrix with one destination row's corners shifted leaves the bound
    if hs > 1:
        wrong = np.einsum('dy,ncde,ex->ncyx', _resize_matrix(hs, hd, shift_row=hd - 1), g.astype(np.float64), rx)
        assert (np.abs(wrong - want) > 4 * bound).any(), sizes
