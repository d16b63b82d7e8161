"""The entry points of include/sr_hip_vsr_bwd.h on the GPU.

sr_vsr_prop_input_bwd_f32 against float64 from the definition (flow_restate.flow_warp_bwd with the coordinates evaluated in fp32
as the device does), under the header's two bounds:
    |dflow - exact| <= 2^-24 |exact| + 2^-50 * sum |terms|
    |dprev - (before + exact)| <= (d + 1) * 2^-24 * (|before| + sum |terms|),  d the contributions to the element
with windows at a non-zero block offset of wider tensors, flow and dflow as slices with an image stride and sentinels around
every destination.

sr_vsr_trunk_keep_f32 bit for bit against the forward header's trunk call and, with the Winograd switch off, its stack bit for
bit against the convs issued one by one.

sr_vsr_trunk_bwd_f32 against the float64 restatement tests/vsr_grad_restate.py forced with the device's own masks, read from the
stack.  Relative L2 per parameter tensor and for the input gradient; bound: 10 x the distance the fp32 torch restatement shows on
the CPU when forced with its own masks (the largest over the tensors of the case) — the project's standing margin over a measured
fp32 distance.  Both figures are printed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as FR  # noqa: E402
import vsr_grad_restate as G  # noqa: E402
import vsr_restate as V  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float('nan')
U = 2.0 ** -24
PROP_BWD_ID = 178


@pytest.fixture(scope='module')
def lib():
    lib = _lib.load()
    lib.sr_dev_set_wino_f32.argtypes = [C.c_int]
    lib.sr_dev_set_wino_f32.restype = C.c_int
    yield lib
    lib.sr_dev_set_wino_f32(1)


@pytest.fixture(autouse=True)
def switches(lib):
    yield
    lib.sr_dev_set_wino_f32(1)


def _profiled(lib, fn):
    _lib.check(lib.sr_profile_start(1024), 'sr_profile_start')
    try:
        fn()
    finally:
        recs = (_lib.LaunchRecord * 1024)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, 1024, C.byref(cnt)), 'sr_profile_stop')
    return [recs[i].kernel_id for i in range(min(cnt.value, 1024))]


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _nchw(t):
    """A CB8 tensor [N, CB, H, W, 8] as float64 numpy [N, 8 CB, H, W]."""
    n, cb, h, w, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(n, cb * 8, h, w).double().cpu().numpy()


# ------------------------------------------------------------------------------------- adjoint of the step input
FLOWS = ('smooth', 'integer', 'leaving', 'naninf', 'samecell')


def _flow(kind, rng, n, h, w):
    """fp32 [n, 2, h, w]."""
    gy, gx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    f = np.zeros((n, 2, h, w))
    if kind == 'smooth':                      # sub-pixel, slowly varying
        f[:, 0] = 0.3 + 0.45 * np.sin(0.3 * gy + 0.2 * gx) + rng.uniform(-0.05, 0.05, (n, h, w))
        f[:, 1] = -0.2 + 0.45 * np.cos(0.25 * gx - 0.1 * gy) + rng.uniform(-0.05, 0.05, (n, h, w))
    elif kind == 'integer':                   # exactly on integers; every third pixel exactly on W - 1 / H - 1, every fifth on 0
        f[:, 0] = rng.integers(-2, 3, (n, h, w))
        f[:, 1] = rng.integers(-2, 3, (n, h, w))
        f[:, 0][:, :, ::3] = (w - 1 - gx)[:, ::3]
        f[:, 1][:, ::3] = (h - 1 - gy)[::3]
        f[:, 0][:, :, 1::5] = (0 - gx)[:, 1::5]
    elif kind == 'leaving':                   # out of the image on each side, wholly and by half a pixel
        f[:, 0] = rng.uniform(-1, 1, (n, h, w))
        f[:, 1] = rng.uniform(-1, 1, (n, h, w))
        f[:, 0][:, ::4] = -(gx[::4] + 0.5)                 # x = -0.5: the left corner column is outside
        f[:, 0][:, 1::4] = (w - 0.5 - gx)[1::4]            # x = W - 0.5: the right one
        f[:, 1][:, :, ::4] = -(gy[:, ::4] + 0.25)
        f[:, 1][:, :, 1::4] = (h - 0.75 - gy)[:, 1::4]
        f[:, 0][:, 2::4, 2::4] = w + 3.0                   # wholly outside, each side
        f[:, 0][:, 3::4, 2::4] = -(w + 3.0)
        f[:, 1][:, 2::4, 3::4] = h + 3.0
        f[:, 1][:, 3::4, 3::4] = -(h + 3.0)
    elif kind == 'naninf':
        f[:, 0] = rng.uniform(-1, 1, (n, h, w))
        f[:, 1] = rng.uniform(-1, 1, (n, h, w))
        f[:, 0][:, ::2, ::3] = np.nan
        f[:, 1][:, 1::2, ::3] = np.inf
        f[:, 0][:, ::2, 1::3] = -np.inf
    else:                                     # every pixel of an image samples one cell: H * W contributions per corner
        cy, cx = (h - 1) // 2, (w - 1) // 2
        f[:, 0] = cx + 0.25 - gx
        f[:, 1] = cy + 0.5 - gy
    return f.astype(np.float32)


def _prop_reference(prev, flow, g):
    """(dprev terms, dflow [n, 2, h, w], count, sum |dprev terms|, sum |dflow terms| [n, 2, h, w]) in float64 from the definition,
    coordinates in fp32 as the device evaluates them; a position that is not finite or outside (-1, W) x (-1, H) gives nothing."""
    n, c, h, w = prev.shape
    fl = np.ascontiguousarray(flow.transpose(0, 2, 3, 1))
    with np.errstate(invalid='ignore'):
        ix = (np.arange(w, dtype=np.float32)[None, None, :] + fl[..., 0]).astype(np.float32) if w > 1 else np.zeros(fl.shape[:3], np.float32)
        iy = (np.arange(h, dtype=np.float32)[None, :, None] + fl[..., 1]).astype(np.float32) if h > 1 else np.zeros(fl.shape[:3], np.float32)
        valid = (ix > -1) & (ix < w) & (iy > -1) & (iy < h)
    safe = np.where(valid[..., None], fl, np.float32(0))             # an invalid pixel is computed at flow 0 and then dropped
    gm = g * valid[:, None]
    dx, dflow, count, absterms = FR.flow_warp_bwd(prev, safe, gm, 'zeros', coord_dtype=np.float32)
    x0, y0, fx, fy, _, _ = FR.warp_coords(safe, h, w, 'zeros')
    av = [np.abs(FR._corner(prev, y0 + oy, x0 + ox)[0]) for oy, ox in ((0, 0), (0, 1), (1, 0), (1, 1))]
    fxe, fye, ag = fx[:, None], fy[:, None], np.abs(gm)
    tx = (ag * ((1 - fye) * (av[1] + av[0]) + fye * (av[3] + av[2]))).sum(1) * (w > 1)
    ty = (ag * ((1 - fxe) * (av[2] + av[0]) + fxe * (av[3] + av[1]))).sum(1) * (h > 1)
    dflow = dflow.transpose(0, 3, 1, 2) * valid[:, None]
    return dx, dflow, count, absterms, np.stack([tx, ty], 1)


def _to_cb8(a, dev):
    n, c, h, w = a.shape
    return torch.from_numpy(np.ascontiguousarray(a.reshape(n, c // 8, 8, h, w).transpose(0, 1, 3, 4, 2))).float().to(dev)


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('fb', [1, 8, 9])
@pytest.mark.parametrize('shape', [(1, 1), (5, 7), (33, 40)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_prop_input_bwd_matches_float64(cuda, lib, shape, fb, n):
    h, w = shape
    rng = np.random.default_rng(100 * h + 10 * fb + n)
    c = 8 * fb
    prev = rng.standard_normal((n, c, h, w)).astype(np.float32).astype(np.float64)
    g = rng.standard_normal((n, c, h, w)).astype(np.float32).astype(np.float64)
    before = rng.standard_normal((n, c, h, w)).astype(np.float32).astype(np.float64)
    # windows at block offset 1 of wider tensors; everything around them is a sentinel
    prev_wide = torch.full((n, fb + 2, h, w, 8), NAN, device=cuda)
    prev_wide[:, 1:1 + fb] = _to_cb8(prev, cuda)
    g_wide = torch.full((n, fb + 3, h, w, 8), NAN, device=cuda)
    g_wide[:, 2:2 + fb] = _to_cb8(g, cuda)
    worst = {}
    for kind in FLOWS:
        flow = _flow(kind, rng, n, h, w)
        want_dx, want_df, count, absterms, abs_df = _prop_reference(prev, flow, g)
        flows = torch.full((n, 2, 2, h, w), NAN, device=cuda)          # the flow is step 1 of 2: an image stride of 4 h w
        flows[:, 1] = torch.from_numpy(flow).to(cuda)

        def run(want_dprev=True, want_dflow=True, images=slice(0, n)):
            k = images.stop - images.start
            dprev_wide = torch.full((k, fb + 2, h, w, 8), 777.0, device=cuda)
            dprev_wide[:, 1:1 + fb] = _to_cb8(before[images], cuda)
            dflows = torch.full((k, 3, 2, h, w), NAN, device=cuda)
            H.vsr_prop_input_bwd(H.CB8(g_wide[images].contiguous(), 2, fb), H.CB8(prev_wide[images].contiguous(), 1, fb), flows[images][:, 1],
                                 H.CB8(dprev_wide, 1, fb) if want_dprev else None, dflows[:, 2] if want_dflow else None)
            # nothing outside the destinations; a destination that was not asked for is untouched
            assert bool((dprev_wide[:, 0] == 777.0).all()) and bool((dprev_wide[:, 1 + fb] == 777.0).all()), kind
            assert bool(torch.isnan(dflows[:, :2]).all()), kind
            if not want_dprev:
                assert _same(dprev_wide[:, 1:1 + fb], _to_cb8(before[images], cuda)), kind
            if not want_dflow:
                assert bool(torch.isnan(dflows[:, 2]).all()), kind
            return dprev_wide[:, 1:1 + fb], dflows[:, 2]

        ids = _profiled(lib, lambda: run())
        assert ids == [PROP_BWD_ID], ids                                  # one launch
        dprev, dflow = run()
        # dflow: the float64 value rounded once
        got = dflow.double().cpu().numpy()
        err_df = np.abs(got - want_df)
        bound_df = U * np.abs(want_df) + 2.0 ** -50 * abs_df
        worst[kind + ' dflow'] = float((err_df / np.maximum(bound_df, 1e-300)).max()) if err_df.max() > 0 else 0.0
        assert (err_df <= bound_df).all(), (kind, float(err_df.max()))
        if kind in ('leaving', 'naninf') and h * w > 1:
            assert int((got == 0).all(1).sum()) > 0, kind                # some pixel lies wholly outside: exactly 0
        # dprev: added onto the prefill, within the atomic bound
        err_dx = np.abs(_nchw(dprev) - (before + want_dx))
        bound_dx = (count + 1) * U * (np.abs(before) + absterms)
        worst[kind + ' dprev'] = float((err_dx / bound_dx).max())
        assert (err_dx <= bound_dx).all(), (kind, float((err_dx / bound_dx).max()))
        if kind == 'samecell':
            assert int(count.max()) == h * w
        # two runs: dflow bit for bit, dprev within twice the bound
        dprev2, dflow2 = run()
        assert _same(dflow2, dflow), kind
        assert (np.abs(_nchw(dprev2) - _nchw(dprev)) <= 2 * bound_dx).all(), kind
        # a batch is its images one by one: dflow bit for bit
        if n > 1:
            for i in range(n):
                _, df1 = run(images=slice(i, i + 1))
                assert _same(df1, dflow[i:i + 1]), (kind, i)
        # a NULL dprev or a NULL dflow leaves the other result as it was
        _, dflow3 = run(want_dprev=False)
        assert _same(dflow3, dflow), kind
        dprev3, _ = run(want_dflow=False)
        assert (np.abs(_nchw(dprev3) - (before + want_dx)) <= bound_dx).all(), kind
        # the generic warp backward's dflow on the same data: both within their bound of the same float64 value
        if not np.isnan(flow).any():
            _, other = H.flow_warp_bwd(H.CB8(prev_wide[:, 1:1 + fb].contiguous()), flows[:, 1].permute(0, 2, 3, 1).contiguous(),
                                       H.CB8(g_wide[:, 2:2 + fb].contiguous()), 'zeros', want_dx=False)
            diff = np.abs(other.permute(0, 3, 1, 2).double().cpu().numpy() - got)
            assert (diff <= 2 * bound_df).all(), (kind, float(diff.max()))
    print(f'{h}x{w} fb={fb} n={n}: worst error / bound ' + ', '.join(f'{k} {v:.2f}' for k, v in worst.items()))


@pytest.mark.parametrize('fb', [1, 9])
@pytest.mark.parametrize('shape', [(1, 1), (5, 7), (33, 40)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_prop_input_bwd_dprev_is_exact_on_whole_pixel_flows(cuda, shape, fb):
    """The float-atomic dprev bit for bit, where it cannot depend on the order of the adds: on a zero flow and on a uniform
    whole-pixel flow the fractions are exactly 0, so three corner weights are 0.0 (skipped) and the fourth is 1, and a translation
    maps distinct pixels to distinct elements.  Every element of dprev then receives at most one add, of a term that is g itself:
    dprev = before + term in one fp32 addition.  (The reference's `count` also counts zero-weight corners and is not used here.)"""
    (h, w), n = shape, 3
    rng = np.random.default_rng(1000 * h + 10 * fb + 3)
    c = 8 * fb
    prev, g, before = (rng.standard_normal((n, c, h, w)).astype(np.float32).astype(np.float64) for _ in range(3))
    prev_wide = torch.full((n, fb + 2, h, w, 8), NAN, device=cuda)
    prev_wide[:, 1:1 + fb] = _to_cb8(prev, cuda)
    g_wide = torch.full((n, fb + 3, h, w, 8), NAN, device=cuda)
    g_wide[:, 2:2 + fb] = _to_cb8(g, cuda)
    for name, (fx, fy) in (('zero', (0.0, 0.0)), ('shifted', (2.0, -1.0))):
        flow = np.empty((n, 2, h, w), np.float32)
        flow[:, 0], flow[:, 1] = fx, fy
        term = _prop_reference(prev, flow, g)[0]
        assert np.array_equal(term.astype(np.float32).astype(np.float64), term), name      # exact in fp32: one term, weight 1
        assert np.abs(term).max() > 0, name                                                # part of the image stays inside
        if name == 'shifted' and h * w > 1:
            assert int((term == 0).all(1).sum()) > 0, name                                 # and part of it gets nothing
        want = before.astype(np.float32) + term.astype(np.float32)                         # one fp32 addition
        flows = torch.full((n, 2, 2, h, w), NAN, device=cuda)
        flows[:, 1] = torch.from_numpy(flow).to(cuda)
        dprev_wide = torch.full((n, fb + 2, h, w, 8), 777.0, device=cuda)
        dprev_wide[:, 1:1 + fb] = _to_cb8(before, cuda)
        dflows = torch.full((n, 3, 2, h, w), NAN, device=cuda)
        H.vsr_prop_input_bwd(H.CB8(g_wide, 2, fb), H.CB8(prev_wide, 1, fb), flows[:, 1], H.CB8(dprev_wide, 1, fb), dflows[:, 2])
        assert bool((dprev_wide[:, 0] == 777.0).all()) and bool((dprev_wide[:, 1 + fb] == 777.0).all()), name
        assert _same(dprev_wide[:, 1:1 + fb], _to_cb8(want, cuda)), name


# ------------------------------------------------------------------------------------------------------ trunk, kept
def _trunk_case(num_feat, num_block, segs, n, h, w, dev, seed=3):
    """(cfg, device parameters in state_dict order, numpy state dict, source window inside a wider NaN tensor, its blocks)."""
    rng = np.random.default_rng(seed)
    sd = V.trunk_weights(rng, 't', 3 + segs * num_feat, num_feat, num_block, 0.5)
    params = [torch.from_numpy(sd[k]).to(dev) for k in V.trunk_keys('t', num_block)]
    cbn = 1 + segs * num_feat // 8
    wide = torch.full((n, cbn + 2, h, w, 8), NAN, device=dev)
    gen = torch.Generator().manual_seed(seed)
    wide[:, 1:1 + cbn] = torch.randn((n, cbn, h, w, 8), generator=gen).to(dev)
    wide[:, 1, :, :, 3:] = 0.0                              # the frame block's pad channels
    return H.vsr_trunk_cfg(num_feat, num_block, segs), params, sd, wide, cbn


def _source_nchw(wide, cbn):
    """The real channels of the source window as float64 [N, 3 + segs * num_feat, H, W]."""
    win = _nchw(wide[:, 1:1 + cbn])
    return np.concatenate([win[:, :3], win[:, 8:]], 1)


def _keep(cfg, blob, wide, cbn, dev):
    n, _, h, w, _ = wide.shape
    fb = cfg.num_feat // 8
    out = torch.full((n, fb + 2, h, w, 8), NAN, device=dev)
    _, stack = H.vsr_trunk_keep(cfg, blob, H.CB8(wide, 1, cbn), H.CB8(out, 1, fb))
    assert bool(torch.isnan(out[:, 0]).all()) and bool(torch.isnan(out[:, fb + 1]).all())
    return out, stack


def _plain(cfg, blob, wide, cbn, dev):
    n, _, h, w, _ = wide.shape
    fb = cfg.num_feat // 8
    out = torch.full((n, fb + 2, h, w, 8), NAN, device=dev)
    H.vsr_trunk(cfg, blob, H.CB8(wide, 1, cbn), H.CB8(out, 1, fb))
    return out


@pytest.mark.parametrize('segs', [1, 2], ids=['cin72', 'cin136'])
@pytest.mark.parametrize('num_block', [0, 1, 2])
@pytest.mark.parametrize('shape', [(9, 11), (33, 40), (13, 37)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_trunk_keep_is_the_trunk_bit_for_bit_and_keeps_the_activations(cuda, lib, shape, num_block, segs):
    (h, w), n, nf = shape, 2, 64
    cfg, params, sd, wide, cbn = _trunk_case(nf, num_block, segs, n, h, w, cuda)
    blob = H.vsr_trunk_pack(cfg, params)
    assert H.vsr_trunk_keep_bytes(cfg, n, h, w) == 2 * num_block * ((4 * n * nf * h * w + 255) // 256 * 256)
    try:
        for mode in (0, 1, 3) if shape == (13, 37) else (0, 1):       # 13x37: the forced Winograd variant, as tests/test_vsr_host.py
            lib.sr_dev_set_wino_f32(mode)
            want = _plain(cfg, blob, wide, cbn, cuda)
            box = []
            ids = _profiled(lib, lambda: box.append(_keep(cfg, blob, wide, cbn, cuda)))
            assert ids == _profiled(lib, lambda: _plain(cfg, blob, wide, cbn, cuda)) and len(ids) == 1 + 2 * num_block, (mode, ids)
            out, stack = box[0]
            assert _same(out[:, 1:1 + nf // 8], want[:, 1:1 + nf // 8]), mode
            if mode != 0:
                continue
            # the stack, with the direct kernels: the convs issued one by one, bit for bit, and the restatement's activations
            acts = H.vsr_trunk_stack_views(cfg, stack, n, h, w)
            assert len(acts) == 2 * num_block
            src = H.CB8(wide[:, 1:1 + cbn].contiguous())
            x = H.conv3x3(src, H.PackedConv(params[0], params[1], first_seg=3, seg=nf), act_slope=0.1)
            mine = [x]
            for i in range(num_block):
                w1, b1, w2, b2 = params[2 + 4 * i:6 + 4 * i]
                t = H.conv3x3(x, H.PackedConv(w1, b1), act_slope=0.0)
                x = H.conv3x3(t, H.PackedConv(w2, b2), res1=x, beta1=1.0)
                mine += [t, x]
            assert _same(out[:, 1:1 + nf // 8], mine[-1].buf)
            for k, a in enumerate(acts):
                assert _same(a.buf, mine[k].buf), k
            tp = {k: torch.from_numpy(v).double() for k, v in sd.items()}
            _, ref = G.trunk(tp, 't', torch.from_numpy(_source_nchw(wide, cbn)), num_block, G._Masks(None, []))
            for k, a in enumerate(acts):
                assert np.abs(_nchw(a.buf) - ref[k].numpy()).max() <= 1e-4 * max(1.0, float(ref[k].abs().max())), k
    finally:
        lib.sr_dev_set_wino_f32(1)


# --------------------------------------------------------------------------------------------------- trunk backward
def _trunk_grads(sd, x, dout, num_block, dtype, forced=None):
    """({name: gradient}, masks) of L = sum(trunk(x) * dout) in ``dtype``; the input's gradient under 'x'."""
    params = {k: torch.from_numpy(v).to(dtype).requires_grad_() for k, v in sd.items()}
    xt = torch.from_numpy(x).to(dtype).requires_grad_()
    rec = []
    y, _ = G.trunk(params, 't', xt, num_block, G._Masks(forced, rec))
    grads = torch.autograd.grad((y * torch.from_numpy(dout).to(dtype)).sum(), list(params.values()) + [xt])
    return {k: v.double().numpy() for k, v in zip(list(params) + ['x'], grads)}, rec


def _run_bwd(cfg, dblob, wide, cbn, out, stack, dout_wide, dev, want=None, accumulate=False, targets=None, want_din=True):
    """One sr_vsr_trunk_bwd_f32 call on windows of wider tensors -> ({index: gradient tensor}, din window or None)."""
    n, _, h, w, _ = wide.shape
    fb = cfg.num_feat // 8
    nparams = 2 * (1 + 2 * cfg.num_block)
    shapes = [(cfg.num_feat, 3 + cfg.cin_segs * cfg.num_feat, 3, 3), (cfg.num_feat,)] + [(cfg.num_feat, cfg.num_feat, 3, 3), (cfg.num_feat,)] * (2 * cfg.num_block)
    if targets is None:
        targets = {i: torch.full(shapes[i], NAN, device=dev) for i in range(nparams) if want is None or i in want}
    din_wide = torch.full((n, cbn + 2, h, w, 8), NAN, device=dev)
    H.vsr_trunk_bwd(cfg, dblob, H.CB8(wide, 1, cbn), H.CB8(out, 1, fb), stack, H.CB8(dout_wide, 1, fb),
                    H.CB8(din_wide, 1, cbn) if want_din else None, [targets[i].data_ptr() if i in targets else None for i in range(nparams)],
                    accumulate)
    assert bool(torch.isnan(din_wide[:, 0]).all()) and bool(torch.isnan(din_wide[:, 1 + cbn]).all())
    if not want_din:
        assert bool(torch.isnan(din_wide).all())
    return targets, din_wide[:, 1:1 + cbn]


@pytest.mark.parametrize('segs', [1, 2], ids=['cin_segs1', 'cin_segs2'])
@pytest.mark.parametrize('num_block', [0, 1, 2])
@pytest.mark.parametrize('case', [(64, 9, 11), (64, 33, 40), (24, 9, 11)], ids=lambda c: f'nf{c[0]}_{c[1]}x{c[2]}')
def test_trunk_bwd_matches_the_forced_restatement(cuda, lib, case, num_block, segs):
    """Measured on the MI355X (worst over the parameter tensors and the input gradient | the fp32 torch restatement on the CPU
    against float64, both forced with the fp32 run's masks | the bound), the largest of each group of cases:
        num_feat 64,  9x11:  7.63e-07 | 3.61e-07 | 3.61e-06   (num_block 2, cin_segs 2)
        num_feat 64, 33x40:  7.99e-07 | 7.04e-07 | 7.04e-06   (num_block 2, cin_segs 2)
        num_feat 24,  9x11:  4.95e-07 | 3.45e-07 | 3.45e-06   (num_block 2, cin_segs 2)
    over all 18 cases the device's distance is 0.6 to 2.2 times the CPU's."""
    (nf, h, w), n = case, 2
    cfg, params, sd, wide, cbn = _trunk_case(nf, num_block, segs, n, h, w, cuda, seed=5)
    fb = nf // 8
    blob, dblob = H.vsr_trunk_pack(cfg, params), H.vsr_trunk_pack_dgrad(cfg, params)
    out, stack = _keep(cfg, blob, wide, cbn, cuda)
    gen = torch.Generator().manual_seed(17)
    dout_wide = torch.full((n, fb + 2, h, w, 8), NAN, device=cuda)
    dout_wide[:, 1:1 + fb] = torch.randn((n, fb, h, w, 8), generator=gen).to(cuda)
    box = []
    ids = _profiled(lib, lambda: box.append(_run_bwd(cfg, dblob, wide, cbn, out, stack, dout_wide, cuda)))
    names = [lib.sr_kernel_name(i).decode() for i in ids]
    convs = sum(nm.startswith('conv_f32_kernel') for nm in names)
    wgrads = sum(nm.startswith('wgrad') for nm in names)
    masks_run = sum(i == 90 for i in ids)                             # sr_cb8_relu_mask_f32: only where no block carries the mask
    assert convs == 1 + 2 * num_block and wgrads >= 1 + 2 * num_block and masks_run == (num_block == 0), names
    assert len(ids) == convs + wgrads + masks_run, names
    grads, din = box[0]
    # the device's own masks, from the stack (num_block = 0: the output is the first conv's activation)
    acts = H.vsr_trunk_stack_views(cfg, stack, n, h, w)
    masks = [_nchw(out[:, 1:1 + fb]) > 0] if num_block == 0 else [_nchw(acts[0].buf) > 0] + [_nchw(acts[1 + 2 * b].buf) > 0 for b in range(num_block)]
    x, dout = _source_nchw(wide, cbn), _nchw(dout_wide[:, 1:1 + fb])
    want, _ = _trunk_grads(sd, x, dout, num_block, torch.float64, forced=masks)
    # the yardstick: fp32 torch on the CPU against float64, both on the fp32 run's own masks
    cpu32, own = _trunk_grads({k: v for k, v in sd.items()}, x.astype(np.float32), dout.astype(np.float32), num_block, torch.float32)
    cpu64, _ = _trunk_grads(sd, x, dout, num_block, torch.float64, forced=own)
    cpu_dist = max(G.rel_l2(cpu32, cpu64).values())
    got = {k: grads[i].double().cpu().numpy() for i, k in enumerate(V.trunk_keys('t', num_block))}
    dn = _nchw(din)
    assert float(np.abs(dn[:, 3:8]).max()) == 0.0                     # the frame block's pad channels
    got['x'] = np.concatenate([dn[:, :3], dn[:, 8:]], 1)
    dist = G.rel_l2(got, want)
    worst = max(dist, key=dist.get)
    print(f'trunk bwd nf={nf} nb={num_block} segs={segs} {h}x{w}: device vs forced float64 {dist[worst]:.3e} ({worst}), CPU fp32 forced '
          f'{cpu_dist:.3e}, bound {10 * cpu_dist:.3e}')
    assert all(np.abs(v).max() > 0 for v in want.values())
    assert dist[worst] <= 10 * cpu_dist, dist
    # two runs are bit-identical: no atomics in this call
    grads2, din2 = _run_bwd(cfg, dblob, wide, cbn, out, stack, dout_wide, cuda)
    assert _same(din2, din) and all(_same(grads2[i], grads[i]) for i in grads)
    # a NULL target changes no other result bit; so does a NULL din
    some = {i for i in grads if i not in (0, 1) and i % 4 != 3} if num_block else {0}
    grads3, din3 = _run_bwd(cfg, dblob, wide, cbn, out, stack, dout_wide, cuda, want=some)
    assert set(grads3) == some and _same(din3, din) and all(_same(grads3[i], grads[i]) for i in some)
    grads4, _ = _run_bwd(cfg, dblob, wide, cbn, out, stack, dout_wide, cuda, want_din=False)
    assert all(_same(grads4[i], grads[i]) for i in grads)
    # accumulate: two calls into one target are the sum of two stored results, bit for bit
    dout_b = torch.full_like(dout_wide, NAN)
    dout_b[:, 1:1 + fb] = torch.randn((n, fb, h, w, 8), generator=gen).to(cuda)
    grads_b, _ = _run_bwd(cfg, dblob, wide, cbn, out, stack, dout_b, cuda)
    acc, _ = _run_bwd(cfg, dblob, wide, cbn, out, stack, dout_wide, cuda)
    _run_bwd(cfg, dblob, wide, cbn, out, stack, dout_b, cuda, accumulate=True, targets=acc)
    assert all(_same(acc[i], grads[i] + grads_b[i]) for i in grads)


def test_wrappers_refuse_misfits(cuda):
    g, prev = H.CB8.zeros(1, 16, 4, 5, cuda), H.CB8.zeros(1, 16, 4, 5, cuda)
    flow = torch.zeros((1, 2, 4, 5), device=cuda)
    with pytest.raises(ValueError, match='nothing to compute'):
        H.vsr_prop_input_bwd(g, prev, flow)
    with pytest.raises(ValueError, match='flow must be'):
        H.vsr_prop_input_bwd(g, prev, torch.zeros((1, 4, 5, 2), device=cuda), dprev=H.CB8.zeros(1, 16, 4, 5, cuda))
    with pytest.raises(ValueError, match='dprev does not fit'):
        H.vsr_prop_input_bwd(g, prev, flow, dprev=H.CB8.zeros(1, 8, 4, 5, cuda))
    with pytest.raises(ValueError, match='must not be a source'):
        H.vsr_prop_input_bwd(g, prev, flow, dprev=prev)
    cfg = H.vsr_trunk_cfg(64, 1, 1)
    with pytest.raises(ValueError, match='stack is too small'):
        H.vsr_trunk_keep(cfg, torch.zeros(16, dtype=torch.uint8, device=cuda), H.CB8.zeros(1, 72, 8, 8, cuda), H.CB8.zeros(1, 64, 8, 8, cuda),
                         stack=torch.zeros(16, dtype=torch.uint8, device=cuda))
