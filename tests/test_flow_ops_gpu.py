"""The entry points of include/sr_hip_flow.h on the GPU, each against float64 (tests/flow_restate.py) with a bound counted from
the roundings of the operation order the header states.  EPS = 2^-24.

  conv7x7      K = 49 * cin fused multiply-adds from a zero accumulator, + bias, ReLU, + res1: with A the same convolution of
               the absolute values (+ |bias| + |res1|),  |got - exact| <= (K + 3) * EPS * A + EPS * |exact|.
  warp         the blend is evaluated in float64 and rounded once: EPS * max|x| when the sampling position is exact (flows
               that are multiples of 1/64); an arbitrary flow adds the rounding of the position, EPS * |position|, times the
               local difference of x (at most 2 max|x|), on both axes.
  warp bwd     dflow: a float64 sum rounded once; dx: d float atomic adds of products with exact weights (positions on the 1/64
               grid): d * EPS * sum|terms|, d and the sum counted by the restatement.
Negative controls leave their bounds: a dropped tap, a wrong padding mode, a shifted position."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
TINY = 1e-30
NAN = float('nan')


def _rng(seed):
    return np.random.default_rng(seed)


def _to_cb8(x, cuda, before=0, after=0, fill=NAN):
    """[N, C, H, W] numpy -> CB8 window of a buffer with ``before`` / ``after`` slack blocks and pad channels, all ``fill``."""
    n, c, h, w = x.shape
    cb = (c + 7) // 8
    buf = torch.full((n, before + cb + after, h, w, 8), fill, dtype=torch.float32)
    xp = torch.full((n, cb * 8, h, w), fill, dtype=torch.float32)
    xp[:, :c] = torch.from_numpy(np.asarray(x, np.float32))
    buf[:, before:before + cb] = xp.reshape(n, cb, 8, h, w).permute(0, 1, 3, 4, 2)
    return H.CB8(buf.to(cuda), before, cb)


def _from_cb8(t, c=None):
    """The window's channels as float64 numpy [N, C, H, W] (all channels of the window when c is None)."""
    b = t.buf[:, t.cb0:t.cb0 + t.cbn].cpu()
    n, cb, h, w, _ = b.shape
    x = b.permute(0, 1, 4, 2, 3).reshape(n, cb * 8, h, w)
    return x[:, :c].double().numpy()


# ------------------------------------------------------------------------------------------------------------ conv7x7
CONV_MAPS = ((1, 1), (2, 2), (3, 2), (7, 9), (19, 37))     # below the halo, the level-0 sizes, one tile + a ragged tail each way
_conv_cache = {}


def _conv_case(cin, cout, h, w, n=1, seed=0):
    key = (cin, cout, h, w, n, seed)
    if key not in _conv_cache:
        rng = _rng(1000 * cin + 10 * cout + h + seed)
        x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
        wt = (rng.standard_normal((cout, cin, 7, 7)) / np.sqrt(49 * cin)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        res = rng.standard_normal((n, cout, h, w)).astype(np.float32)
        pre, mag = R.conv7x7(x, wt, b)                     # computed once, shared, never modified
        _conv_cache[key] = (x, wt, b, res, pre, mag)
    return _conv_cache[key]


@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('hw', CONV_MAPS, ids=[f'{h}x{w}' for h, w in CONV_MAPS])
@pytest.mark.parametrize('pair', H.CONV7X7_SHAPES, ids=[f'{ci}to{co}' for ci, co in H.CONV7X7_SHAPES])
def test_conv7x7_matches_float64(cuda, pair, hw, relu):
    cin, cout = pair
    h, w = hw
    x, wt, b, res, pre, mag = _conv_case(cin, cout, h, w)
    inst = H.conv7x7_instance(cout, cin)
    assert inst == {(8, 32): 0, (32, 64): 1, (64, 32): 0, (32, 16): 0, (16, 2): 2}[pair]     # every instance is reached
    pc = H.PackedConv7x7(torch.from_numpy(wt).to(cuda), torch.from_numpy(b).to(cuda))
    assert pc.instance == inst and pc.w.numel() == _lib.load().sr_conv7x7_packed_floats(cout, cin)
    use_res = cout == 2
    src = _to_cb8(x, cuda, before=1, after=1)              # NaN slack blocks around the window
    cob = (cout + 7) // 8
    out = H.CB8(torch.full((1, cob + 2, h, w, 8), NAN, dtype=torch.float32, device=cuda), 1, cob)
    r1 = _to_cb8(res, cuda, before=1, after=0, fill=0.0) if use_res else None
    H.conv7x7(src, pc, out=out, relu=relu, res1=r1)
    got = _from_cb8(out)
    want = np.maximum(pre, 0) if relu else pre
    A = mag.copy()
    if use_res:
        want, A = want + res, A + np.abs(res)
    bound = (49 * cin + 3) * EPS * A + EPS * np.abs(want) + TINY
    err = np.abs(got[:, :cout] - want)
    assert np.isfinite(got).all() and (err <= bound).all(), (pair, hw, float((err / bound).max()))
    assert (got[:, cout:] == 0).all()                                          # pad channels of the last block are written 0
    assert torch.isnan(out.buf[:, 0]).all() and torch.isnan(out.buf[:, -1]).all()   # nothing outside the window is written
    # negative control: the reference without the centre tap of the last channel block leaves the bound
    if not relu:
        wd = np.zeros_like(wt[:, -8:])
        wd[:, :, 3, 3] = wt[:, -8:, 3, 3]
        dropped, _ = R.conv7x7(x[:, -8:], wd, np.zeros(cout))
        assert (np.abs(dropped) > 4 * bound).any(), (pair, hw)


def test_conv7x7_batches_and_reruns_are_bit_identical(cuda):
    for cin, cout in H.CONV7X7_SHAPES:
        x, wt, b, res, pre, mag = _conv_case(cin, cout, 9, 35, n=2, seed=7)
        pc = H.PackedConv7x7(torch.from_numpy(wt).to(cuda), torch.from_numpy(b).to(cuda))
        both = H.conv7x7(_to_cb8(x, cuda), pc, relu=True).buf
        again = H.conv7x7(_to_cb8(x, cuda), pc, relu=True).buf
        one = [H.conv7x7(_to_cb8(x[i:i + 1], cuda), pc, relu=True).buf for i in range(2)]
        assert torch.equal(both, again) and torch.equal(both, torch.cat(one, 0)), (cin, cout)
        err = np.abs(_from_cb8(H.CB8(both), cout) - np.maximum(pre, 0))
        assert (err <= (49 * cin + 3) * EPS * mag + EPS * np.abs(pre) + TINY).all()


def test_conv7x7_refuses_what_it_does_not_serve(cuda):
    with pytest.raises(ValueError, match='not supported'):
        H.PackedConv7x7(torch.zeros(16, 8, 7, 7, device=cuda))
    pc = H.PackedConv7x7(torch.zeros(32, 8, 7, 7, device=cuda))
    with pytest.raises(ValueError, match='channels'):
        H.conv7x7(H.CB8.zeros(1, 16, 4, 4, cuda), pc)
    with pytest.raises(ValueError, match='does not fit'):
        H.conv7x7(H.CB8.zeros(1, 8, 4, 4, cuda), pc, out=H.CB8.zeros(1, 32, 4, 5, cuda))


# --------------------------------------------------------------------------------------------------------------- warp
WARP_SHAPES = ((1, 1), (1, 5), (5, 1), (2, 2), (7, 9), (33, 70))
WARP_C = (1, 3, 8, 11)


def _run_warp(x, flow, pm, layout, cuda, slack=0):
    """The kernel's output as float64 numpy [N, C, H, W]; CB8 sources carry NaN pad channels, NCHW ones ``slack`` NaN floats
    behind the tensor."""
    n, c, h, w = x.shape
    fl = torch.from_numpy(flow).to(cuda)
    if layout == 'cb8':
        out = H.flow_warp(_to_cb8(x, cuda), fl, pm, channels=c)
        full = _from_cb8(out)
        assert (full[:, c:] == 0).all()                    # NaN pad channels of x do not leak; pad channels of out are 0
        return full[:, :c]
    store = torch.full((x.size + slack,), NAN, dtype=torch.float32, device=cuda)
    xt = store[:x.size].view(n, c, h, w)
    xt.copy_(torch.from_numpy(x))
    return H.flow_warp(xt, fl, pm).cpu().double().numpy()


@pytest.mark.parametrize('layout', ['nchw', 'cb8'])
@pytest.mark.parametrize('pm', ['zeros', 'border'])
def test_warp_matches_float64(cuda, pm, layout):
    for (h, w) in WARP_SHAPES:
        for c in WARP_C:
            rng = _rng(h * 100 + w + c)
            x = rng.standard_normal((2, c, h, w)).astype(np.float32)
            M = float(np.abs(x).max())
            # zero flow and integer shifts: bit for bit the copied (or zeroed / edge) source
            for sx, sy in ((0, 0), (1, 0), (-2, 1)):
                flow = np.broadcast_to(np.array([sx, sy], np.float32), (2, h, w, 2)).copy()
                got = _run_warp(x, flow, pm, layout, cuda)
                want = R.flow_warp(x, flow.astype(np.float64), pm)
                assert np.array_equal(got, want), ('shift', h, w, c, sx, sy)
                if (sx, sy) == (0, 0):
                    assert np.array_equal(got, x.astype(np.float64))
            # positions on the 1/64 grid are exact: only the blend's one rounding remains
            flow = (rng.integers(-3 * 64, 3 * 64 + 1, (2, h, w, 2)) / 64.0).astype(np.float32)
            got = _run_warp(x, flow, pm, layout, cuda)
            want = R.flow_warp(x, flow.astype(np.float64), pm)
            assert (np.abs(got - want) <= EPS * M * (1 + 2.0 ** -20) + TINY).all(), ('grid', h, w, c)
            # arbitrary flows: + the rounding of the position times the local difference, on both axes
            flow = rng.uniform(-4, 4, (2, h, w, 2)).astype(np.float32)
            got = _run_warp(x, flow, pm, layout, cuda)
            want = R.flow_warp(x, flow.astype(np.float64), pm)
            bound = EPS * M + 2 * EPS * (max(h, w) + 4) * (2 * M) + TINY
            assert (np.abs(got - want) <= bound).all(), ('any', h, w, c)
            assert (np.abs(got - R.flow_warp(x, flow, pm, coord_dtype=np.float32)) <= EPS * M * (1 + 2.0 ** -20) + TINY).all()
            # negative controls: the other padding mode and a position shifted by 1/64 leave the bound (where x varies)
            if h * w >= 63:
                other = R.flow_warp(x, flow.astype(np.float64), 'border' if pm == 'zeros' else 'zeros')
                assert (np.abs(got - other) > 4 * bound).any()
                moved = R.flow_warp(x, flow.astype(np.float64) + 1 / 64, pm)
                assert (np.abs(got - moved) > 4 * bound).any()


@pytest.mark.parametrize('layout', ['nchw', 'cb8'])
def test_warp_far_outside_and_on_the_last_pixel(cuda, layout):
    for (h, w) in WARP_SHAPES:
        rng = _rng(h + w)
        x = rng.standard_normal((2, 3, h, w)).astype(np.float32)
        for far in ((1e4, 1e4), (-1e4, 3e3), (3e38, -3e38), (float('inf'), float('inf'))):
            flow = np.broadcast_to(np.array(far, np.float32), (2, h, w, 2)).copy()
            got = _run_warp(x, flow, 'zeros', layout, cuda)
            if (h, w) != (1, 1):
                assert (got == 0).all(), (h, w, far)
            got = _run_warp(x, flow, 'border', layout, cuda)
            ey, ex = (h - 1 if far[1] > 0 else 0), (w - 1 if far[0] > 0 else 0)
            assert np.array_equal(got, np.broadcast_to(x[:, :, ey:ey + 1, ex:ex + 1], x.shape).astype(np.float64)), (h, w, far)
        # every sample exactly on (h - 1, w - 1): the far corners have weight 0 and lie behind the tensor, in NaN slack
        gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        flow = np.stack([w - 1 - gx, h - 1 - gy], -1).astype(np.float32)[None].repeat(2, 0)
        for pm in ('zeros', 'border'):
            got = _run_warp(x, flow, pm, layout, cuda, slack=4 * w + 8)
            assert np.array_equal(got, np.broadcast_to(x[:, :, -1:, -1:], x.shape).astype(np.float64)), (h, w, pm)


def _grid_flow(rng, n, h, w, spread):
    """A flow whose positions lie on the 1/64 grid, at least 1/64 from every integer (so from every clip edge too)."""
    gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    tx = rng.integers(-spread, w + spread, (n, h, w)) + rng.integers(1, 64, (n, h, w)) / 64.0
    ty = rng.integers(-spread, h + spread, (n, h, w)) + rng.integers(1, 64, (n, h, w)) / 64.0
    return np.stack([tx - gx, ty - gy], -1).astype(np.float32)


def _run_bwd(x, flow, g, pm, layout, cuda):
    c = x.shape[1]
    fl = torch.from_numpy(flow).to(cuda)
    if layout == 'cb8':
        dx, df = H.flow_warp_bwd(_to_cb8(x, cuda), fl, _to_cb8(g, cuda), pm, channels=c)
        full = _from_cb8(dx)
        assert (full[:, c:] == 0).all()
        return full[:, :c], df.cpu().double().numpy(), df
    dx, df = H.flow_warp_bwd(torch.from_numpy(x).to(cuda), fl, torch.from_numpy(g).to(cuda), pm)
    return dx.cpu().double().numpy(), df.cpu().double().numpy(), df


@pytest.mark.parametrize('layout', ['nchw', 'cb8'])
@pytest.mark.parametrize('pm', ['zeros', 'border'])
def test_warp_backward_matches_float64(cuda, pm, layout):
    for (h, w) in WARP_SHAPES:
        for c in (3, 11):
            rng = _rng(7 * h + w + c)
            x = rng.standard_normal((2, c, h, w)).astype(np.float32)
            g = rng.standard_normal((2, c, h, w)).astype(np.float32)
            flow = _grid_flow(rng, 2, h, w, 2)
            dx64, df64, count, absterms = R.flow_warp_bwd(x, flow.astype(np.float64), g, pm)
            dx, df, raw = _run_bwd(x, flow, g, pm, layout, cuda)
            assert (np.abs(df - df64) <= EPS * np.abs(df64) * (1 + 2.0 ** -20) + 1e-12).all(), ('dflow', h, w, c)   # (+ the float64 sum's own)
            bound = count * EPS * absterms + TINY
            assert (np.abs(dx - dx64) <= bound).all(), ('dx', h, w, c, float((np.abs(dx - dx64) / bound).max()))
            assert (dx[count == 0] == 0).all()
            dx2, _, raw2 = _run_bwd(x, flow, g, pm, layout, cuda)
            assert torch.equal(raw, raw2)                              # the gather is bit-reproducible
            assert (np.abs(dx - dx2) <= bound).all()                   # the scatter within its bound
            if h == 1:
                assert (df[..., 1] == 0).all()                         # an axis of size 1 passes no gradient
            if w == 1:
                assert (df[..., 0] == 0).all()
            if pm == 'border' and h > 1 and w > 1:
                gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
                ix, iy = gx + flow[..., 0].astype(np.float64), gy + flow[..., 1].astype(np.float64)
                assert (df[..., 0][(ix < 0) | (ix > w - 1)] == 0).all() and (df[..., 1][(iy < 0) | (iy > h - 1)] == 0).all()
            # negative control: the gradients of the other padding mode leave the bounds
            if h * w >= 63:
                ox, of, _, _ = R.flow_warp_bwd(x, flow.astype(np.float64), g, 'border' if pm == 'zeros' else 'zeros')
                assert (np.abs(dx - ox) > 4 * bound).any() and (np.abs(df - of) > 4 * EPS * np.abs(df64) + 1e-6).any()


@pytest.mark.parametrize('layout', ['nchw', 'cb8'])
def test_warp_backward_many_adds_to_one_address(cuda, layout):
    h, w, c = 33, 70, 3
    rng = _rng(11)
    x = rng.standard_normal((1, c, h, w)).astype(np.float32)
    g = rng.standard_normal((1, c, h, w)).astype(np.float32)
    flow = np.full((1, h, w, 2), 1000.0, np.float32)           # border: every sample is clipped onto pixel (h - 1, w - 1)
    dx64, df64, count, absterms = R.flow_warp_bwd(x, flow.astype(np.float64), g, 'border')
    assert count[0, :, -1, -1].tolist() == [2310] * c and count.sum() == 2310 * c
    dx, df, _ = _run_bwd(x, flow, g, 'border', layout, cuda)
    bound = count * EPS * absterms + TINY
    assert (np.abs(dx - dx64) <= bound).all() and (df == 0).all() and not df64.any()
    dx2, _, _ = _run_bwd(x, flow, g, 'border', layout, cuda)
    assert (np.abs(dx - dx2) <= bound).all()


def test_flow_warp_op_is_an_autograd_function_over_the_kernels(cuda):
    from image_restoration_amd.ops.flow_warp import flow_warp
    rng = _rng(3)
    x = rng.standard_normal((2, 5, 7, 9)).astype(np.float32)
    flow = _grid_flow(rng, 2, 7, 9, 1)
    g = rng.standard_normal((2, 5, 7, 9)).astype(np.float32)
    for pm in ('zeros', 'border'):
        xt = torch.from_numpy(x).to(cuda).requires_grad_()
        ft = torch.from_numpy(flow).to(cuda).requires_grad_()
        y = flow_warp(xt, ft, padding_mode=pm)
        assert type(y.grad_fn).__name__ == 'FlowWarpBackward'
        y.backward(torch.from_numpy(g).to(cuda))
        M = float(np.abs(x).max())
        assert (np.abs(y.detach().cpu().double().numpy() - R.flow_warp(x, flow.astype(np.float64), pm)) <= EPS * M * 1.001).all()
        dx64, df64, count, absterms = R.flow_warp_bwd(x, flow.astype(np.float64), g, pm)
        assert (np.abs(xt.grad.cpu().double().numpy() - dx64) <= count * EPS * absterms + TINY).all()
        assert (np.abs(ft.grad.cpu().double().numpy() - df64) <= EPS * np.abs(df64) * 1.001 + 1e-12).all()
    with pytest.raises(ValueError, match='reflection'):
        flow_warp(xt, ft, padding_mode='reflection')
    with pytest.raises(ValueError, match='must agree'):
        flow_warp(xt, ft[:, :5])


# ------------------------------------------------------------------------------------------------------ SpyNet pieces
LEVEL_CASES = ((2, 2, False), (3, 2, False), (4, 4, True), (6, 4, True), (14, 18, True), (40, 70, True))


@pytest.mark.parametrize('case', LEVEL_CASES, ids=[f'{h}x{w}{"_prev" if p else ""}' for h, w, p in LEVEL_CASES])
def test_level_input_matches_float64(cuda, case):
    h, w, has_prev = case
    rng = _rng(h * w)
    ref = rng.standard_normal((2, 3, h, w)).astype(np.float32)
    supp = rng.standard_normal((2, 3, h, w)).astype(np.float32)
    prev = rng.uniform(-3, 3, (2, 2, h // 2, w // 2)).astype(np.float32) if has_prev else None
    fp = _to_cb8(prev, cuda) if has_prev else None            # NaN in channels 2..7 of the flow block
    out, up = H.spynet_level_input(torch.from_numpy(ref).to(cuda), torch.from_numpy(supp).to(cuda), fp)
    got, gup = _from_cb8(out), _from_cb8(up)
    want, wup = R.level_input(ref, supp, None if prev is None else prev.astype(np.float64))
    assert np.array_equal(got[:, :3], ref.astype(np.float64))
    assert np.array_equal(got[:, 6:8], gup[:, :2]) and (gup[:, 2:] == 0).all()
    assert (np.abs(gup[:, :2] - wup) <= EPS * np.abs(wup) * (1 + 2.0 ** -20) + 1e-13).all()          # float64 blend, rounded once
    if not has_prev:
        assert (gup == 0).all() and np.array_equal(got[:, 3:6], supp.astype(np.float64))     # level 0: up = 0, warp = supp
    M, U = float(np.abs(supp).max()), float(np.abs(wup).max())
    # the blend's rounding + the position's rounding and up's own rounding, each times the local difference, on both axes
    bound = EPS * M + 2 * EPS * (max(h, w) + U) * (2 * M) + 2 * EPS * U * (2 * M) + TINY
    assert (np.abs(got[:, 3:6] - want[:, 3:6]) <= bound).all()
    if has_prev and h * w >= 63:          # negative control: warping with zeros padding instead of border leaves the bound
        other = R.flow_warp(supp, wup.transpose(0, 2, 3, 1), 'zeros')
        assert (np.abs(got[:, 3:6] - other) > 4 * bound).any()


def test_preprocess_and_avgpool_match_float64(cuda):
    rng = _rng(5)
    for (h, w) in ((2, 2), (6, 10), (34, 70)):
        x = rng.uniform(0, 1, (2, 3, h, w)).astype(np.float32)
        xt = torch.from_numpy(x).to(cuda)
        mean, std = R.MEAN.tolist(), R.STD.tolist()
        y = H.spynet_preprocess(xt, mean, std)
        want = (x.astype(np.float64) - R.MEAN[None, :, None, None]) / R.STD[None, :, None, None]
        assert (np.abs(y.cpu().double().numpy() - want) <= 2 * EPS * (np.abs(x) + 0.5) / R.STD.min()).all()     # subtract, divide
        m32, s32 = torch.tensor(mean, device=cuda).view(1, 3, 1, 1), torch.tensor(std, device=cuda).view(1, 3, 1, 1)
        assert torch.equal(y, (xt - m32) / s32)                                     # the same two fp32 operations as torch
        p = H.avgpool2x2(y)
        wantp = R.avgpool2(y.cpu().double().numpy())
        mag = R.avgpool2(np.abs(y.cpu().double().numpy()))
        assert tuple(p.shape) == (2, 3, h // 2, w // 2) and (np.abs(p.cpu().double().numpy() - wantp) <= 3 * EPS * mag + TINY).all()
    with pytest.raises(ValueError, match='not even'):
        H.avgpool2x2(torch.zeros(1, 3, 5, 4, device=cuda))
