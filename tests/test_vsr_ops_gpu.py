"""The two entry points of include/sr_hip_vsr.h on the GPU.

sr_vsr_prop_input_f32 is compared BIT FOR BIT with the existing ops it replaces — hip_ops.flow_warp (CB8, zeros), which
tests/test_flow_ops_gpu.py pins against float64, and hip_ops.nchw_to_cb8 — so no tolerance is needed.  Sources and destinations are
windows inside wider NaN-filled tensors with non-dense image strides.

sr_vsr_trunk_f32 is compared bit for bit with the same convs issued one by one through hip_ops.conv3x3 under
sr_dev_set_wino_f32(0) (the same direct kernels on the same descriptors), and on the Winograd route against the float64
restatement tests/vsr_restate.py under the project's rule err_on <= 4 * err_off + 2^-20 (tests/test_wino_f32_gpu.py has the
derivation).  The launch profile is read as tests/test_rrdbnet_infer_gpu.py reads it.  The Winograd switch is restored by a
fixture finalizer and in ``finally``.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vsr_restate as V  # noqa: E402

pytestmark = pytest.mark.gpu

WINO_IDS = {2: 106, 3: 107, 4: 108}   # sr_dev_set_wino_f32(mode) -> kernel id of its tile variant
PROP_ID = 159
NAN = float('nan')


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


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------- propagation input
FLOWS = ('zero', 'integer', 'grid64', 'arbitrary', 'huge', 'inf', 'nan')


def _flow(kind, gen, b, h, w, dev):
    shape = (b, 2, h, w)
    if kind == 'zero':
        f = torch.zeros(shape)
    elif kind == 'integer':
        f = torch.randint(-3, 4, shape, generator=gen).float()
    elif kind == 'grid64':
        f = torch.randint(-256, 257, shape, generator=gen).float() / 64
    elif kind == 'arbitrary':
        f = torch.randn(shape, generator=gen) * 3
    elif kind == 'huge':
        f = torch.where(torch.rand(shape, generator=gen) < 0.5, torch.tensor(1e4), torch.tensor(-1e4))
        f[:, :, ::2, ::2] = torch.randn(shape, generator=gen)[:, :, ::2, ::2]
    elif kind == 'inf':
        f = torch.randn(shape, generator=gen)
        f[:, 0, ::2] = float('inf')
        f[:, 1, :, ::3] = float('-inf')
    else:                                   # a position that is not a number samples nothing: zeros, as flow_warp_kernel
        f = torch.randn(shape, generator=gen)
        f[:, 0, ::2] = NAN
        f[:, 1, :, ::3] = NAN
    return f.to(dev)


def _prop_case(num_feat, h, w, b, dev, seed):
    """Operands as windows of wider NaN-filled tensors: the frame is x[:, 1] of a 3-frame clip, the flow step 1 of 2, the previous
    feature blocks [1, 1 + fb) of fb + 2, the destinations blocks [1, 2 + fb) of fb + 3."""
    gen = torch.Generator().manual_seed(seed)
    fb = num_feat // 8
    clip = torch.rand((b, 3, 3, h, w), generator=gen).to(dev)
    prev_wide = torch.full((b, fb + 2, h, w, 8), NAN, device=dev)
    prev_wide[:, 1:1 + fb] = torch.randn((b, fb, h, w, 8), generator=gen).to(dev)
    return gen, fb, clip, prev_wide


def _run_prop(clip, frame_idx, prev_wide, flows, step, fb, dev, with_frame=True):
    b, _, _, h, w = clip.shape
    dst = torch.full((b, fb + 3, h, w, 8), NAN, device=dev)
    H.vsr_prop_input(clip[:, frame_idx], None if prev_wide is None else H.CB8(prev_wide, 1, fb),
                     None if flows is None else flows[:, step], H.CB8(dst, 2, fb), H.CB8(dst, 1, 1) if with_frame else None)
    return dst


@pytest.mark.parametrize('b', [1, 2])
@pytest.mark.parametrize('shape', [(1, 1), (1, 5), (5, 1), (7, 9), (33, 70)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('num_feat', [8, 24, 64])
def test_prop_input_is_flow_warp_and_the_frame_block_bit_for_bit(cuda, num_feat, shape, b):
    h, w = shape
    gen, fb, clip, prev_wide = _prop_case(num_feat, h, w, b, cuda, 1000 * num_feat + 10 * h + w + b)
    prev = H.CB8(prev_wide[:, 1:1 + fb].contiguous())
    frame_want = H.nchw_to_cb8(clip[:, 1].contiguous()).buf
    assert float(frame_want[..., 3:].abs().max()) == 0.0
    for kind in FLOWS:
        flows = torch.full((b, 2, 2, h, w), NAN, device=cuda)
        flows[:, 1] = _flow(kind, gen, b, h, w, cuda)
        dst = _run_prop(clip, 1, prev_wide, flows, 1, fb, cuda)
        want = H.flow_warp(prev, flows[:, 1].permute(0, 2, 3, 1).contiguous(), 'zeros').buf
        assert _same(dst[:, 2:2 + fb], want), kind
        assert _same(dst[:, 1:2], frame_want), kind
        assert bool(torch.isnan(dst[:, 0]).all()) and bool(torch.isnan(dst[:, 2 + fb]).all()), kind   # nothing outside the windows
        assert not bool(torch.isnan(dst[:, 1:2 + fb]).any()), kind     # NaN neighbours of the source window do not leak
        if kind in ('huge', 'inf', 'nan') and h * w > 1:
            assert int((dst[:, 2:2 + fb] == 0).all(-1).all(1).sum()) > 0, kind     # some pixel lies wholly outside
    # without the frame block that block stays untouched
    dst = _run_prop(clip, 1, prev_wide, flows, 1, fb, cuda, with_frame=False)
    assert bool(torch.isnan(dst[:, 1]).all()) and _same(dst[:, 2:2 + fb], want)
    # the first step of a branch: exact zeros, the frame still written
    dst = _run_prop(clip, 1, None, None, 0, fb, cuda)
    assert _same(dst[:, 2:2 + fb], torch.zeros_like(dst[:, 2:2 + fb])) and _same(dst[:, 1:2], frame_want)
    assert bool(torch.isnan(dst[:, 0]).all()) and bool(torch.isnan(dst[:, 2 + fb]).all())


def test_prop_input_comparison_sees_swapped_planes_and_a_wrong_frame(cuda):
    """The comparison above fails for the two mistakes it is there to catch: shown once by feeding the comparison side the wrong
    input."""
    b, h, w, num_feat = 2, 7, 9, 24
    gen, fb, clip, prev_wide = _prop_case(num_feat, h, w, b, cuda, 5)
    prev = H.CB8(prev_wide[:, 1:1 + fb].contiguous())
    flows = torch.randn((b, 2, 2, h, w), generator=gen).to(cuda) * 2
    dst = _run_prop(clip, 1, prev_wide, flows, 1, fb, cuda)
    good = H.flow_warp(prev, flows[:, 1].permute(0, 2, 3, 1).contiguous(), 'zeros').buf
    swapped = H.flow_warp(prev, flows[:, 1].flip(1).permute(0, 2, 3, 1).contiguous(), 'zeros').buf
    other_step = H.flow_warp(prev, flows[:, 0].permute(0, 2, 3, 1).contiguous(), 'zeros').buf
    assert _same(dst[:, 2:2 + fb], good)
    assert not _same(dst[:, 2:2 + fb], swapped) and not _same(dst[:, 2:2 + fb], other_step)
    assert _same(dst[:, 1:2], H.nchw_to_cb8(clip[:, 1].contiguous()).buf)
    assert not _same(dst[:, 1:2], H.nchw_to_cb8(clip[:, 0].contiguous()).buf)
    assert not _same(dst[:, 1:2], H.nchw_to_cb8(clip[:, 2].contiguous()).buf)


def test_prop_input_refusals(cuda):
    clip = torch.zeros((1, 2, 3, 4, 5), device=cuda)
    out = H.CB8.empty(1, 16, 4, 5, cuda)
    prev = H.CB8.empty(1, 16, 4, 5, cuda)
    with pytest.raises(ValueError, match='come together'):
        H.vsr_prop_input(clip[:, 0], prev, None, out)
    with pytest.raises(ValueError, match='flow must be'):
        H.vsr_prop_input(clip[:, 0], prev, torch.zeros((1, 4, 5, 2), device=cuda), out)
    with pytest.raises(ValueError, match='prev does not fit'):
        H.vsr_prop_input(clip[:, 0], H.CB8.empty(1, 8, 4, 5, cuda), torch.zeros((1, 2, 4, 5), device=cuda), out)
    lib = _lib.load()
    d = _lib.VsrPropDesc()
    d.frame, d.warp_out, d.n, d.h, d.w, d.fb = 256, 4096, 1, 4, 5, 2
    d.prev = 512                                            # prev without flow
    assert lib.sr_vsr_prop_input_f32(C.byref(d), None) == -1 and b'both' in lib.sr_last_error()


# ------------------------------------------------------------------------------------------------------ trunk driver
def _trunk_case(num_feat, num_block, segs, n, h, w, dev, seed=3):
    """(cfg, device parameters in state_dict order, numpy state dict, source window inside a wider NaN tensor)."""
    rng = np.random.default_rng(seed)
    cin = 3 + segs * num_feat
    sd = V.trunk_weights(rng, 't', cin, num_feat, num_block, 0.5)
    params = [torch.from_numpy(sd[k]).to(dev) for k in V.trunk_keys('t', num_block)]
    cbn = 1 + segs * num_feat // 8
    wide = torch.full((n, cbn + 2, h, w, 8), NAN, device=dev)
    gen = torch.Generator().manual_seed(seed)
    wide[:, 1:1 + cbn] = torch.randn((n, cbn, h, w, 8), generator=gen).to(dev)
    wide[:, 1, :, :, 3:] = 0.0                              # the frame block's pad channels
    return H.vsr_trunk_cfg(num_feat, num_block, segs), params, sd, wide, cbn


def _per_layer(params, src, num_feat, num_block):
    pc = H.PackedConv(params[0], params[1], first_seg=3, seg=num_feat)
    x = H.conv3x3(src, pc, act_slope=0.1)
    for i in range(num_block):
        w1, b1, w2, b2 = params[2 + 4 * i:6 + 4 * i]
        t = H.conv3x3(x, H.PackedConv(w1, b1), act_slope=0.0)
        x = H.conv3x3(t, H.PackedConv(w2, b2), res1=x, beta1=1.0)
    return x.buf


def _nchw_source(wide, cbn, segs, num_feat):
    """The real channels of the source window as [N, 3 + segs * num_feat, H, W] float64."""
    win = wide[:, 1:1 + cbn].permute(0, 1, 4, 2, 3).reshape(wide.size(0), cbn * 8, wide.size(2), wide.size(3))
    return torch.cat([win[:, :3], win[:, 8:]], 1).double().cpu().numpy()


def _run_trunk(cfg, blob, wide, cbn, dev):
    n, _, h, w, _ = wide.shape
    fb = cfg.num_feat // 8
    out = torch.full((n, fb + 2, h, w, 8), NAN, device=dev)
    H.vsr_trunk(cfg, blob, H.CB8(wide, 1, cbn), H.CB8(out, 1, fb))
    assert bool(torch.isnan(out[:, 0]).all()) and bool(torch.isnan(out[:, fb + 1]).all())
    return out[:, 1:1 + fb]


@pytest.mark.parametrize('segs', [1, 2], ids=['cin72', 'cin136'])
@pytest.mark.parametrize('num_block', [0, 1, 3])
def test_trunk_driver_is_the_per_layer_composition_bit_for_bit(cuda, lib, num_block, segs):
    n, h, w, nf = 2, 13, 37, 64
    cfg, params, sd, wide, cbn = _trunk_case(nf, num_block, segs, n, h, w, cuda)
    blob = H.vsr_trunk_pack(cfg, params)
    try:
        lib.sr_dev_set_wino_f32(0)
        want = _per_layer(params, H.CB8(wide[:, 1:1 + cbn].contiguous()), nf, num_block)
        box = []
        ids = _profiled(lib, lambda: box.append(_run_trunk(cfg, blob, wide, cbn, cuda)))
        got = _run_trunk(cfg, blob, wide, cbn, cuda)
        last = _run_trunk(cfg, blob, wide[n - 1:].contiguous(), cbn, cuda)
    finally:
        lib.sr_dev_set_wino_f32(1)
    names = [lib.sr_kernel_name(i).decode() for i in ids]
    assert len(ids) == 1 + 2 * num_block and all(nm.startswith('conv_f32_kernel') for nm in names), names   # no copy kernel
    assert _same(got, want) and _same(box[0], want)
    assert _same(last, got[n - 1:])                         # image n - 1 alone: the bits of its slice of the batch
    ref = V.trunk(sd, 't', _nchw_source(wide, cbn, segs, nf), num_block)
    g = got.permute(0, 1, 4, 2, 3).reshape(n, nf, h, w).double().cpu().numpy()
    err = float(np.abs(g - ref).max())
    print(f'trunk nb={num_block} cin_pad={8 + segs * nf}: max|driver - float64| = {err:.3e}, max|ref| = {np.abs(ref).max():.2f}')
    assert err <= 1e-4 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize('num_feat', [64, 32, 24])
def test_trunk_driver_on_the_winograd_route(cuda, lib, num_feat):
    n, h, w, num_block, segs = 2, 13, 37, 2, 1
    cfg, params, sd, wide, cbn = _trunk_case(num_feat, num_block, segs, n, h, w, cuda, seed=11)
    blob = H.vsr_trunk_pack(cfg, params)
    assert H.vsr_trunk_wino_convs(cfg) == [V.wino_eligible(co, ci) for co, ci, _ in V.trunk_convs(num_feat, num_block, segs)]
    ref = V.trunk(sd, 't', _nchw_source(wide, cbn, segs, num_feat), num_block)
    runs = {}
    try:
        for mode in (0, 1, 3):
            lib.sr_dev_set_wino_f32(mode)
            box = []
            ids = _profiled(lib, lambda: box.append(_run_trunk(cfg, blob, wide, cbn, cuda)))
            runs[mode] = (box[0], ids)
    finally:
        lib.sr_dev_set_wino_f32(1)

    def err(t):
        return float(np.abs(t.permute(0, 1, 4, 2, 3).reshape(n, num_feat, h, w).double().cpu().numpy() - ref).max())
    err_off = err(runs[0][0])
    for mode in (1, 3):
        out, ids = runs[mode]
        expect = V.trunk_wino_launches(num_feat, num_block, segs, h, w, mode)
        got = sum(i in WINO_IDS.values() for i in ids)
        e = err(out)
        print(f'nf={num_feat} mode {mode}: wino launches {got} (rule {expect}) err_off {err_off:.3e} err {e:.3e} bound '
              f'{4 * err_off + 2.0 ** -20:.3e}')
        assert len(ids) == 1 + 2 * num_block
        assert got == expect and all(i == WINO_IDS[3] for i in ids if i in WINO_IDS.values())
        assert e <= 4 * err_off + 2.0 ** -20
    # at this size the default mode declines: no Winograd launch and the bits of mode 0
    assert _same(runs[1][0], runs[0][0])
    assert V.trunk_wino_launches(num_feat, num_block, segs, h, w, 3) == (0 if num_feat == 24 else 1 + 2 * num_block)


def test_trunk_refusals(cuda):
    lib = _lib.load()
    for bad in ((20, 1, 1), (64, -1, 1), (64, 1, 3), (0, 1, 1)):
        cfg = H.vsr_trunk_cfg(*bad)
        assert lib.sr_vsr_trunk_num_params(C.byref(cfg)) == -1 and lib.sr_vsr_trunk_packed_bytes(C.byref(cfg)) == 0
        assert lib.sr_vsr_trunk_workspace_bytes(C.byref(cfg), 1, 8, 8) == 0
    cfg = H.vsr_trunk_cfg(64, 1, 1)
    blob = torch.zeros(lib.sr_vsr_trunk_packed_bytes(C.byref(cfg)), dtype=torch.uint8, device=cuda)
    src, out = H.CB8.zeros(1, 72, 8, 8, cuda), H.CB8.zeros(1, 64, 8, 8, cuda)
    with pytest.raises(ValueError, match='do not fit'):
        H.vsr_trunk(cfg, blob, H.CB8.zeros(1, 64, 8, 8, cuda), out)
    rc = lib.sr_vsr_trunk_f32(C.byref(cfg), blob.data_ptr(), src.ptr, src.img_stride, out.ptr, out.img_stride, 1, 8, 8, None, 0, None)
    assert rc == -3 and b'workspace' in lib.sr_last_error()             # SR_ENOSPACE, nothing launched


def test_prop_input_launch_record(cuda, lib):
    """The profiler branch: one record with kernel id 159, its shape, and the algorithmic FLOPs and bytes the entry point states."""
    b, h, w, num_feat = 2, 7, 9, 24
    gen, fb, clip, prev_wide = _prop_case(num_feat, h, w, b, cuda, 9)
    flows = torch.randn((b, 2, 2, h, w), generator=gen).to(cuda)
    recs = {}

    def profiled(fn):
        _lib.check(lib.sr_profile_start(16), 'sr_profile_start')
        try:
            fn()
        finally:
            buf = (_lib.LaunchRecord * 16)()
            cnt = C.c_int(0)
            _lib.check(lib.sr_profile_stop(buf, 16, C.byref(cnt)), 'sr_profile_stop')
        return [buf[i] for i in range(cnt.value)]
    recs['warp'] = profiled(lambda: _run_prop(clip, 1, prev_wide, flows, 1, fb, cuda))
    recs['first'] = profiled(lambda: _run_prop(clip, 1, None, None, 0, fb, cuda, with_frame=False))
    px = b * h * w
    for key, flops, nbytes in (('warp', 64.0 * fb * px, 4.0 * px * (40 * fb + 2 * fb + 11)), ('first', 0.0, 4.0 * px * 8 * fb)):
        assert [r.kernel_id for r in recs[key]] == [PROP_ID], key
        r = recs[key][0]
        assert (r.cin, r.cout, r.n, r.h, r.w) == (num_feat, num_feat, b, h, w) and r.flops == flops and r.bytes == nbytes, key
    assert lib.sr_kernel_name(PROP_ID).decode() == 'vsr_prop_input_kernel'
