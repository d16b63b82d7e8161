"""The entry points of include/sr_hip_vsr_bf16.h on the GPU.

sr_rvsr_prop_input_bf16 is compared BIT FOR BIT with hip_ops.flow_warp (fp32, zeros padding, pinned against float64 by
tests/test_flow_ops_gpu.py) on the widened previous feature followed by ``.to(torch.bfloat16)``, and its frame block with
``frame.to(torch.bfloat16)`` and 13 zero channels, so no tolerance is needed.  Sources and destinations are windows inside wider
tensors whose slack holds the bf16 NaN pattern 0x7FC1, with non-dense image strides.

sr_rvsr_trunk_bf16 is compared bit for bit with the same convs issued one by one through hip_ops.conv3x3_bf16 on
hip_ops.PackedConvBF16 images, and its segmented first conv (cin_pad 80 and 144) against float64 on bf16-exact operands under the
plain bf16 conv bound of tests/test_edvr_bf16_ops_gpu.py: E = k EPS A + EPS |y64|, |y - y64| <= E + hulp(|y64| + E), with
k = 2 * 9 * cin + 8 and A the absolute-value convolution.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_opwise as O  # noqa: E402
import vsr_restate as V  # noqa: E402

pytestmark = pytest.mark.gpu

PROP_ID = 167
NAN_BITS = 0x7FC1
BF16_CONV_IDS = set(range(16, 32)) | {42, 43, 50, 64}    # sr_conv3x3_bf16's instances (tests/test_edvr_bf16_gpu.py)


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _profiled(lib, fn, cap=64):
    _lib.check(lib.sr_profile_start(cap), 'sr_profile_start')
    try:
        fn()
    finally:
        recs = (_lib.LaunchRecord * cap)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, cap, C.byref(cnt)), 'sr_profile_stop')
    return [recs[i] for i in range(min(cnt.value, cap))]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return a.dtype == b.dtype == torch.bfloat16 and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _nan_filled(shape, dev):
    return torch.full(shape, NAN_BITS, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _is_nan_fill(t):
    return bool((_bits(t) == NAN_BITS).all())


def _to_nchw(cb):
    n, fb, h, w, _ = cb.shape
    return cb.permute(0, 1, 4, 2, 3).reshape(n, fb * 16, h, w)


def _to_cb16(x):
    n, c, h, w = x.shape
    return x.reshape(n, c // 16, 16, h, w).permute(0, 1, 3, 4, 2).contiguous()


# ------------------------------------------------------------------------------------------------- propagation input
FLOWS = ('zero', 'integer', 'grid64', 'arbitrary', 'huge', 'inf')


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
    else:
        f = torch.randn(shape, generator=gen)
        f[:, 0, ::2] = float('inf')
        f[:, 1, :, ::3] = float('-inf')
    return f.to(dev)


def _prop_case(num_feat, h, w, b, dev, seed):
    """Operands as windows of wider NaN-filled tensors: the frame is x[:, 1] of a 3-frame clip, the flow step 1 of 2, the previous
    feature blocks [1, 1 + fb) of fb + 2, the destinations blocks [1, 2 + fb) of fb + 3."""
    gen = torch.Generator().manual_seed(seed)
    fb = num_feat // 16
    clip = torch.rand((b, 3, 3, h, w), generator=gen).to(dev)
    prev_wide = _nan_filled((b, fb + 2, h, w, 16), dev)
    prev_wide[:, 1:1 + fb] = torch.randn((b, fb, h, w, 16), generator=gen).to(dev).bfloat16()
    return gen, fb, clip, prev_wide


def _run_prop(clip, frame_idx, prev_wide, flows, step, fb, dev, with_frame=True):
    b, _, _, h, w = clip.shape
    dst = _nan_filled((b, fb + 3, h, w, 16), dev)
    H.vsr_prop_input_bf16(clip[:, frame_idx], None if prev_wide is None else H.CB16(prev_wide, 1, fb),
                          None if flows is None else flows[:, step], H.CB16(dst, 2, fb), H.CB16(dst, 1, 1) if with_frame else None)
    return dst


def _warp_want(prev_wide, fb, flow):
    """bf16(the fp32 flow-warp entry point on the widened previous feature), back in CB16."""
    wide = _to_nchw(prev_wide[:, 1:1 + fb].float()).contiguous()
    return _to_cb16(H.flow_warp(wide, flow.permute(0, 2, 3, 1).contiguous(), 'zeros').to(torch.bfloat16))


def _frame_want(frame):
    n, _, h, w = frame.shape
    blk = torch.zeros((n, 1, h, w, 16), dtype=torch.bfloat16, device=frame.device)
    blk[:, 0, :, :, :3] = frame.permute(0, 2, 3, 1).to(torch.bfloat16)
    return blk


@pytest.mark.parametrize('b', [1, 2])
@pytest.mark.parametrize('shape', [(1, 1), (1, 5), (5, 1), (7, 9), (33, 70)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('num_feat', [16, 48, 64])
def test_prop_input_is_the_rounded_flow_warp_and_the_frame_block_bit_for_bit(cuda, num_feat, shape, b):
    h, w = shape
    gen, fb, clip, prev_wide = _prop_case(num_feat, h, w, b, cuda, 1000 * num_feat + 10 * h + w + b)
    frame_want = _frame_want(clip[:, 1])
    for kind in FLOWS:
        flows = torch.full((b, 2, 2, h, w), float('nan'), device=cuda)
        flows[:, 1] = _flow(kind, gen, b, h, w, cuda)
        dst = _run_prop(clip, 1, prev_wide, flows, 1, fb, cuda)
        want = _warp_want(prev_wide, fb, flows[:, 1])
        assert _same(dst[:, 2:2 + fb], want), kind
        assert _same(dst[:, 1:2], frame_want), kind
        assert _is_nan_fill(dst[:, 0]) and _is_nan_fill(dst[:, 2 + fb]), kind     # nothing outside the windows
        assert not bool(torch.isnan(dst[:, 1:2 + fb].float()).any()), kind          # NaN neighbours of the source window do not leak
        assert _same(_run_prop(clip, 1, prev_wide, flows, 1, fb, cuda), dst), kind  # the rerun
        if kind in ('huge', 'inf') and h * w > 1:
            assert int((dst[:, 2:2 + fb] == 0).all(-1).all(1).sum()) > 0, kind      # some pixel lies wholly outside
    # without the frame block that block stays untouched
    dst = _run_prop(clip, 1, prev_wide, flows, 1, fb, cuda, with_frame=False)
    assert _is_nan_fill(dst[:, 1]) and _same(dst[:, 2:2 + fb], want)
    # the first step of a branch: exact zeros, the frame still written
    dst = _run_prop(clip, 1, None, None, 0, fb, cuda)
    assert _same(dst[:, 2:2 + fb], torch.zeros_like(dst[:, 2:2 + fb])) and _same(dst[:, 1:2], frame_want)
    assert _is_nan_fill(dst[:, 0]) and _is_nan_fill(dst[:, 2 + fb])


def test_prop_input_comparison_sees_swapped_planes_a_wrong_step_and_a_wrong_frame(cuda):
    """The comparison above fails for the mistakes it is there to catch: shown once by feeding the comparison side the wrong input."""
    b, h, w, num_feat = 2, 7, 9, 48
    gen, fb, clip, prev_wide = _prop_case(num_feat, h, w, b, cuda, 5)
    flows = torch.randn((b, 2, 2, h, w), generator=gen).to(cuda) * 2
    dst = _run_prop(clip, 1, prev_wide, flows, 1, fb, cuda)
    assert _same(dst[:, 2:2 + fb], _warp_want(prev_wide, fb, flows[:, 1]))
    assert not _same(dst[:, 2:2 + fb], _warp_want(prev_wide, fb, flows[:, 1].flip(1)))
    assert not _same(dst[:, 2:2 + fb], _warp_want(prev_wide, fb, flows[:, 0]))
    assert _same(dst[:, 1:2], _frame_want(clip[:, 1]))
    assert not _same(dst[:, 1:2], _frame_want(clip[:, 0])) and not _same(dst[:, 1:2], _frame_want(clip[:, 2]))
    # the result is a rounding of the fp32 warp, not the fp32 warp of a rounding: some value needs the last step
    fp32 = H.flow_warp(_to_nchw(prev_wide[:, 1:1 + fb].float()).contiguous(), flows[:, 1].permute(0, 2, 3, 1).contiguous(), 'zeros')
    assert not torch.equal(fp32, fp32.bfloat16().float())


def test_prop_input_launch_record(cuda, lib):
    """The profiler branch: one record with kernel id 167, its shape, and the algorithmic FLOPs and bytes the entry point states."""
    b, h, w, num_feat = 2, 7, 9, 48
    gen, fb, clip, prev_wide = _prop_case(num_feat, h, w, b, cuda, 9)
    flows = torch.randn((b, 2, 2, h, w), generator=gen).to(cuda)
    recs = {'warp': _profiled(lib, lambda: _run_prop(clip, 1, prev_wide, flows, 1, fb, cuda)),
            'first': _profiled(lib, lambda: _run_prop(clip, 1, None, None, 0, fb, cuda, with_frame=False))}
    px = b * h * w
    for key, flops, nbytes in (('warp', 128.0 * fb * px, px * (160.0 * fb + 8.0 * fb + 44.0)), ('first', 0.0, px * 32.0 * fb)):
        assert [r.kernel_id for r in recs[key]] == [PROP_ID], key
        r = recs[key][0]
        assert (r.cin, r.cout, r.n, r.h, r.w) == (num_feat, num_feat, b, h, w) and r.flops == flops and r.bytes == nbytes, key
    assert lib.sr_kernel_name(PROP_ID).decode() == 'vsr_prop_input_bf16_kernel'


def test_prop_input_refusals(cuda, lib):
    clip = torch.zeros((1, 2, 3, 4, 5), device=cuda)
    out, prev = H.CB16.empty(1, 32, 4, 5, cuda), H.CB16.empty(1, 32, 4, 5, cuda)
    flow = torch.zeros((1, 2, 4, 5), device=cuda)
    with pytest.raises(ValueError, match='come together'):
        H.vsr_prop_input_bf16(clip[:, 0], prev, None, out)
    with pytest.raises(ValueError, match='flow must be'):
        H.vsr_prop_input_bf16(clip[:, 0], prev, torch.zeros((1, 4, 5, 2), device=cuda), out)
    with pytest.raises(ValueError, match='flow must be'):
        H.vsr_prop_input_bf16(clip[:, 0], prev, flow.bfloat16(), out)
    with pytest.raises(ValueError, match='prev does not fit'):
        H.vsr_prop_input_bf16(clip[:, 0], H.CB16.empty(1, 16, 4, 5, cuda), flow, out)
    with pytest.raises(ValueError, match='warp_out does not fit'):
        H.vsr_prop_input_bf16(clip[:, 0], None, None, H.CB8.empty(1, 32, 4, 5, cuda))
    with pytest.raises(ValueError, match='warp_out does not fit'):
        H.vsr_prop_input_bf16(clip[:, 0], None, None, H.CB16.empty(1, 32, 4, 6, cuda))
    with pytest.raises(ValueError, match='one-block window'):
        H.vsr_prop_input_bf16(clip[:, 0], None, None, out, H.CB16.empty(1, 32, 4, 5, cuda))
    with pytest.raises(ValueError, match='dense images'):
        H.vsr_prop_input_bf16(clip[:, 0].bfloat16(), None, None, out)
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        H.vsr_prop_input_bf16(clip[:, 0].cpu(), None, None, out)
    d = _lib.RvsrPropDesc()
    d.frame, d.warp_out, d.n, d.h, d.w, d.fb = 256, 4096, 1, 4, 5, 2
    d.prev = 512                                            # prev without flow
    assert lib.sr_rvsr_prop_input_bf16(C.byref(d), None) == -1 and b'both' in lib.sr_last_error()


# ------------------------------------------------------------------------------------------------------ trunk driver
def _trunk_case(num_feat, num_block, segs, n, h, w, dev, seed=3, exact=False):
    """(cfg, device parameters in state_dict order, numpy state dict, source window inside a wider NaN tensor).  ``exact``: the
    weights are rounded to bf16 first, so the images hold them exactly."""
    rng = np.random.default_rng(seed)
    cin = 3 + segs * num_feat
    sd = V.trunk_weights(rng, 't', cin, num_feat, num_block, 0.5)
    if exact:
        sd = {k: (torch.from_numpy(v).bfloat16().float().numpy() if k.endswith('weight') else v) for k, v in sd.items()}
    params = [torch.from_numpy(sd[k]).to(dev) for k in V.trunk_keys('t', num_block)]
    cbn = 1 + segs * num_feat // 16
    wide = _nan_filled((n, cbn + 2, h, w, 16), dev)
    gen = torch.Generator().manual_seed(seed)
    wide[:, 1:1 + cbn] = torch.randn((n, cbn, h, w, 16), generator=gen).to(dev).bfloat16()
    wide[:, 1, :, :, 3:] = 0.0                              # the frame block's pad channels
    return H.vsr_trunk_cfg(num_feat, num_block, segs), params, sd, wide, cbn


def _per_layer(params, src, num_feat, num_block):
    pc = H.PackedConvBF16(params[0], params[1], first_seg=3, seg=num_feat)
    x = H.conv3x3_bf16(src, pc, act_slope=0.1)
    for i in range(num_block):
        w1, b1, w2, b2 = params[2 + 4 * i:6 + 4 * i]
        t = H.conv3x3_bf16(x, H.PackedConvBF16(w1, b1), act_slope=0.0)
        x = H.conv3x3_bf16(t, H.PackedConvBF16(w2, b2), res1=x, beta1=1.0)
    return x.buf


def _run_trunk(cfg, blob, wide, cbn, dev):
    n, _, h, w, _ = wide.shape
    fb = cfg.num_feat // 16
    out = _nan_filled((n, fb + 2, h, w, 16), dev)
    H.vsr_trunk_bf16(cfg, blob, H.CB16(wide, 1, cbn), H.CB16(out, 1, fb))
    assert _is_nan_fill(out[:, 0]) and _is_nan_fill(out[:, fb + 1])
    return out[:, 1:1 + fb]


@pytest.mark.parametrize('case', [(64, 0, 1), (64, 0, 2), (64, 1, 1), (64, 1, 2), (64, 3, 1), (64, 3, 2), (16, 2, 1)],
                         ids=lambda c: f'nf{c[0]}_nb{c[1]}_segs{c[2]}')
def test_trunk_driver_is_the_per_layer_composition_bit_for_bit(cuda, lib, case):
    nf, num_block, segs = case
    n, h, w = 2, 13, 37
    cfg, params, sd, wide, cbn = _trunk_case(nf, num_block, segs, n, h, w, cuda)
    blob = H.vsr_trunk_pack_bf16(cfg, params)
    assert blob.numel() == lib.sr_rvsr_trunk_packed_bytes_bf16(C.byref(cfg))
    assert lib.sr_rvsr_trunk_workspace_bytes_bf16(C.byref(cfg), n, h, w) == 3 * ((2 * n * nf * h * w + 255) // 256 * 256)
    want = _per_layer(params, H.CB16(wide[:, 1:1 + cbn].contiguous()), nf, num_block)
    box = []
    recs = _profiled(lib, lambda: box.append(_run_trunk(cfg, blob, wide, cbn, cuda)))
    got = _run_trunk(cfg, blob, wide, cbn, cuda)
    last = _run_trunk(cfg, blob, wide[n - 1:].contiguous(), cbn, cuda)
    ids = [r.kernel_id for r in recs]
    assert len(ids) == 1 + 2 * num_block and set(ids) <= BF16_CONV_IDS, ids      # plain conv launches, no copy, no chain
    assert not bool(torch.isnan(got.float()).any())
    assert _same(got, want) and _same(box[0], want)
    assert _same(last, got[n - 1:])                         # image n - 1 alone: the bits of its slice of the batch


@pytest.mark.parametrize('segs', [1, 2], ids=['cin_pad80', 'cin_pad144'])
def test_first_conv_against_float64(cuda, lib, segs):
    """num_block = 0 on bf16-exact inputs and weights: what is left is fp32 accumulation and the one rounding of the output."""
    nf, n, h, w = 64, 2, 13, 37
    cfg, params, sd, wide, cbn = _trunk_case(nf, 0, segs, n, h, w, cuda, seed=7, exact=True)
    assert cbn * 16 == 16 + segs * nf
    got = O.cb16_to_nchw(_run_trunk(cfg, H.vsr_trunk_pack_bf16(cfg, params), wide, cbn, cuda))
    win = O.cb16_to_nchw(wide[:, 1:1 + cbn])
    x = torch.cat([win[:, :3], win[:, 16:]], 1)              # the real channels: the frame, then the feature windows
    wt, bias = torch.from_numpy(sd['t.main.0.weight']).double(), torch.from_numpy(sd['t.main.0.bias']).double()
    cin = 3 + segs * nf

    def bound_and_ref(weight):
        y = F.leaky_relu(F.conv2d(x, weight, bias, padding=1), 0.1)
        a = F.conv2d(x.abs(), weight.abs(), bias.abs(), padding=1)
        e = (2 * 9 * cin + 8) * O.EPS * a + O.EPS * y.abs()
        return y, e + O.hulp(y.abs() + e)
    y64, bound = bound_and_ref(wt)
    O.check(got, y64, bound, f'first conv cin_pad={16 + segs * nf}')
    # two weight rows swapped on the reference side: the same result no longer fits
    swapped = wt.clone()
    swapped[[0, 1]] = swapped[[1, 0]]
    y_bad, bound_bad = bound_and_ref(swapped)
    assert O.worst(got, y_bad, bound_bad) > 1.0
    # and two input channels of the second segment kind (the last feature window) swapped
    swapped = wt.clone()
    swapped[:, [cin - 1, cin - 2]] = swapped[:, [cin - 2, cin - 1]]
    y_bad, bound_bad = bound_and_ref(swapped)
    assert O.worst(got, y_bad, bound_bad) > 1.0


def test_trunk_refusals(cuda, lib):
    for bad in ((24, 1, 1), (8, 1, 1), (64, -1, 1), (64, 1, 3), (0, 1, 1)):
        cfg = H.vsr_trunk_cfg(*bad)
        assert lib.sr_rvsr_trunk_packed_bytes_bf16(C.byref(cfg)) == 0
        assert lib.sr_rvsr_trunk_workspace_bytes_bf16(C.byref(cfg), 1, 8, 8) == 0
    with pytest.raises(ValueError, match='CB16'):
        H.vsr_trunk_pack_bf16(H.vsr_trunk_cfg(24, 1, 1), [torch.zeros(1, device=cuda)] * 6)
    cfg = H.vsr_trunk_cfg(64, 1, 1)
    with pytest.raises(ValueError, match='parameters, the config has 6'):
        H.vsr_trunk_pack_bf16(cfg, [torch.zeros(1, device=cuda)] * 5)
    with pytest.raises(ValueError, match='contiguous fp32'):
        H.vsr_trunk_pack_bf16(cfg, [torch.zeros(1, device=cuda, dtype=torch.float64)] * 6)
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        H.vsr_trunk_pack_bf16(cfg, [torch.zeros(1)] * 6)
    with pytest.raises(ValueError, match='blob too small'):
        H.vsr_trunk_pack_bf16(cfg, [torch.zeros(1, device=cuda)] * 6, torch.zeros(16, dtype=torch.uint8, device=cuda))
    blob = torch.zeros(lib.sr_rvsr_trunk_packed_bytes_bf16(C.byref(cfg)), dtype=torch.uint8, device=cuda)
    src, out = H.CB16.zeros(1, 80, 8, 8, cuda), H.CB16.zeros(1, 64, 8, 8, cuda)
    with pytest.raises(ValueError, match='do not fit'):
        H.vsr_trunk_bf16(cfg, blob, H.CB16.zeros(1, 64, 8, 8, cuda), out)
    with pytest.raises(ValueError, match='do not fit'):
        H.vsr_trunk_bf16(cfg, blob, H.CB8.zeros(1, 72, 8, 8, cuda), H.CB8.zeros(1, 64, 8, 8, cuda))
    with pytest.raises(ValueError, match='do not fit'):
        H.vsr_trunk_bf16(cfg, blob, src, H.CB16.zeros(1, 64, 8, 9, cuda))
    rc = lib.sr_rvsr_trunk_bf16(C.byref(cfg), blob.data_ptr(), src.ptr, src.img_stride, out.ptr, out.img_stride, 1, 8, 8, None, 0, None)
    assert rc == -3 and b'workspace' in lib.sr_last_error()             # SR_ENOSPACE, nothing launched
