"""Every instance of include/sr_hip_ridnet.h's kernels against float64, on the path each takes in production.

sr_convd_f32 runs convd_f32_kernel<COT, PT, KS, DIL> (ridnet_ops.hip): 20 instances, COT 32-cout sub-tiles per workgroup, tiles
of 4 * PT rows x 32 columns, KS x KS taps DIL apart.  sr_convd_wgrad_f32 runs wgradd_f32_kernel<CT, IT, KT, DIL>: 15 instances
of which wgradd_plan reaches 10.  Neither choice can be observed on the device (every ksize-3 launch has profiler id 81), so
both are restated here from the host code (_convd_instance, _wgradd_plan, each citing its lines) and pinned on the host by
tests/test_convd_plan_host.py: the restated weight-gradient plan reproduces sr_convd_wgrad_slab_bytes, and the instance sets
the restatements can produce are the ones the code object holds.  test_dispatch_coverage (last) checks the cases below reach
every instance, each 8-row instance with >= 3 row tiles the last of which is partial, both sides of the 4-row switch (255 and
256 tiles, H = 4 and 5), every reachable weight-gradient plan, and for each dilation a ring that wraps within a workgroup.

Bounds are derived, not fitted (the conventions of tests/test_conv_ops_gpu.py).  EPS = 2^-24.  For every output element let
A be the same operation on absolute values in float64: A = |alpha| (conv(|x|, |w|) + |bias|) + |beta1 r1| + |beta2 r2|
(+ |prior out| when accumulating).  Then |y - y64| <= k EPS A + EPS |y64| with
  - convolutions: k = 2 * taps * cin_pad + 8: two roundings per product of the one MFMA chain over (cin block, tap), plus the
    epilogue's bias add, activation, alpha, two residual multiply-adds, accumulate and mask.  A slope <= 1 (activation or mask)
    only shrinks an error; where the rounded pre-activation has the other sign than the exact one, the branch difference is at
    most the pre-activation's own error.  post_act = 1 moves the activation after the residual adds: the same count.
  - weight gradients, from the kernel's summation order (_wgradd_plan): one wave's accumulator sums rows_per_wg * 32 / KS
    products (KS = 4 / (CT IT) waves split a strip row), two roundings each; sr::wgrad_reduce then sums `chunk` splits in stage 1
    and `sch` chunks in stage 2 (_reduce_chain, restated in tests/test_conv_ops_gpu.py); +3 for scale, bias and accumulate:
    k = 2 rows_per_wg 32 / KS + chunk + sch + 3.
  - the streaming helpers make one rounding (a product) or none per output: bit for bit against the float32 product.
  - the MeanShift ends: the bounds of tests/test_ridnet_gpu.py.

Channel contract.  A source's pad channels (cin .. cin_pad) meet zero weights: they hold arbitrary finite values here and must
not matter.  The pad channels of the last output block (cout .. roundup8(cout)) receive the epilogue of a zero convolution:
alpha act(0) + beta1 r1 + beta2 r2 (+ prior, masked), and 0 in out_pre; the float64 reference pads the weight with zero rows and
checks them.  Blocks outside a window hold SENTINEL and must come back unchanged; outside the source they must not be read.

Sensitivity is asserted, not assumed.  Every convolution case weights the last source channel by +1/2 on every tap and plants
spikes in the last image on that channel: on the d-th row above and below an (4 * PT)-row tile boundary and on the d-th column
left and right of a 32-column strip boundary, the farthest halo rows and columns another tile has to stage.  At the output
across the boundary that reads each spike, the spike's contribution must exceed four bounds: a kernel that drops or shifts a
halo row or column between tiles, the last channel block or the last image fails.  Weight-gradient cases put spikes in the last
image's last row and column and on both sides of the last row-split boundary, one tap apart.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from image_restoration_amd import _lib, hip_ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_conv_ops_gpu import _reduce_chain  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
TINY = 1e-30
SENTINEL = 12345.0


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------ dispatch, restated
def _group_couts(cout):
    """group_couts (ridnet_ops.hip:260): couts per weight-image group."""
    return 64 if (cout + 31) // 32 * 32 % 64 == 0 else 32


def _convd_instance(ksize, d, cout, n, h, w):
    """(COT, PT, row_tiles) of one sr_convd_f32 launch writing `cout` channels: sr_convd_f32 (ridnet_ops.hip:352, 363-364:
    tiles_x = ceil(W / 32), gc = group_couts(cout), groups = roundup32(cout) / gc) and convd_dispatch (ridnet_ops.hip:251-255:
    8-row tiles; 4-row tiles when tiles_x * tiles_y * n * groups < 256 and H > 4; COT 2 for 64-cout groups).  `ksize` and `d`
    pick the template's KS and DIL only (ridnet_ops.hip:366-371)."""
    gc = _group_couts(cout)
    groups = (cout + 31) // 32 * 32 // gc
    tiles_x, tiles_y = _cdiv(w, 32), _cdiv(h, 8)
    small = tiles_x * tiles_y * n * groups < 256 and h > 4
    if small:
        tiles_y = _cdiv(h, 4)
    return (2 if gc == 64 else 1), (1 if small else 2), tiles_y


def _convd_tiles(ksize, d, cout, n, h, w):
    """Workgroups along x of the launch at the 8-row rule (the quantity the 4-row switch compares with 256)."""
    gc = _group_couts(cout)
    return _cdiv(w, 32) * _cdiv(h, 8) * n * ((cout + 31) // 32 * 32 // gc)


def _wgradd_plan(n, h, w, cout, cin, ksize, d):
    """(CT, IT, rows_per_wg, row_splits, splits) of sr_convd_wgrad_f32, restated from wgradd_plan (ridnet_ops.hip:568-593):
    2x2 tile pairs when both tile counts are even and the ring is narrow (ksize 1 or d <= 2), 2x1 when only the cout tiles are
    even and the ring is wide, else 1x1; rows per workgroup halved from H while fewer than 512 workgroups; splits = workgroups *
    (4 / (CT IT)) waves per pair."""
    cin_pad = (cin + 7) // 8 * 8
    cts, its = _cdiv(cout, 32), _cdiv(cin_pad, 32)
    wide = ksize == 1 or d <= 2
    if cts % 2 == 0 and its % 2 == 0 and wide:
        ct, it = 2, 2
    elif cts % 2 == 0 and not wide:
        ct, it = 2, 1
    else:
        ct, it = 1, 1
    grows, gi = cts // ct, its // it
    strips_total = n * _cdiv(w, 32)
    groups = grows * gi
    rows = h
    while rows > 4 and strips_total * _cdiv(h, rows) * groups < 512:
        rows = (rows + 1) // 2
    row_splits = _cdiv(h, rows)
    splits = strips_total * row_splits * (4 // (ct * it))
    return ct, it, rows, row_splits, splits


def _wgradd_slab_bytes(n, h, w, cout, cin, ksize, d):
    """wgradd_bytes (ridnet_ops.hip:627-630) of the restated plan: slab, bias slab and sr::wgrad_reduce's two partial buffers
    (ridnet_ops.hip:566, 590-591), each rounded up to 256 bytes."""
    ct, it, _, _, splits = _wgradd_plan(n, h, w, cout, cin, ksize, d)
    cts, its = _cdiv(cout, 32), _cdiv((cin + 7) // 8 * 8, 32)
    groups, grows = (cts // ct) * (its // it), cts // ct
    al = lambda b: (b + 255) // 256 * 256  # noqa: E731
    return (al(groups * splits * ct * it * ksize * ksize * 1024 * 4) + al(grows * splits * ct * 32 * 4) + al(64 * 4 * 9 * 1024 * 4)
            + al(4096 * 4))


def _wgradd_chain(n, h, w, cout, cin, ksize, d):
    """k of the weight-gradient bound: the longest fp32 chain of one dweight element (module docstring)."""
    ct, it, rows, _, splits = _wgradd_plan(n, h, w, cout, cin, ksize, d)
    cts, its = _cdiv(cout, 32), _cdiv((cin + 7) // 8 * 8, 32)
    P = ct * it
    chunk, sch = _reduce_chain(splits, (cts // ct) * (its // it), its // it, P, ct, ksize * ksize)
    return 2 * rows * 32 // (4 // P) + chunk + sch + 3


# ------------------------------------------------------------------------------------------------------ CB8 helpers
def _to_cb8(x, blocks, cb0, cuda, fill=SENTINEL):
    """NCHW float64 (channels <= 8 * (blocks - cb0)) -> device buffer [n][blocks][h][w][8] holding x at block cb0; the blocks
    outside x's hold `fill`, the pad channels of x's last block zero."""
    n, c, h, w = x.shape
    nb = (c + 7) // 8
    buf = torch.full((n, blocks, h, w, 8), fill, dtype=torch.float32)
    xp = torch.zeros((n, nb * 8, h, w), dtype=torch.float64)
    xp[:, :c] = x
    buf[:, cb0:cb0 + nb] = xp.reshape(n, nb, 8, h, w).permute(0, 1, 3, 4, 2).float()
    return buf.to(cuda)


def _from_cb8(buf, cb0, c):
    n, _, h, w, _ = buf.shape
    nb = (c + 7) // 8
    return buf[:, cb0:cb0 + nb].cpu().double().permute(0, 1, 4, 2, 3).reshape(n, nb * 8, h, w)[:, :c]


def _ptr(buf, cb0):
    return buf.data_ptr() + cb0 * buf.shape[2] * buf.shape[3] * 8 * 4


def _stride(buf):
    return buf.shape[1] * buf.shape[2] * buf.shape[3] * 8


def _rand(rng, shape):
    return torch.from_numpy(rng.standard_normal(shape)).float().double()


def _check(got, ref, A, k, what):
    bound = k * EPS * A + EPS * ref.abs() + TINY
    err = (got - ref).abs()
    bad = ~(err <= bound)
    assert not bool(bad.any()), (what, int(bad.sum()), float((err / bound).nan_to_num(1e30).max()), float(err.nan_to_num(1e30).max()))
    return bound


def _sentinel_kept(buf, lo, hi, what):
    b = buf.cpu()
    assert bool((b[:, :lo] == SENTINEL).all()) and bool((b[:, hi:] == SENTINEL).all()), (what, 'wrote outside its window')


def _profiled_ids(lib, fn):
    _lib.check(lib.sr_profile_start(64), 'sr_profile_start')
    try:
        fn()
    finally:
        recs = (_lib.LaunchRecord * 64)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, 64, C.byref(cnt)), 'sr_profile_stop')
    return [recs[i].kernel_id for i in range(min(cnt.value, 64))]


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------ sr_convd_f32
# (ksize, d, cin, cout, n, h, w, forward options, data-gradient options).  Options: post (post_act), slope (act_slope), alpha,
# res1 / res2 (betas), res_cbn, acc (accumulate), mask = (mask_cb0, mask_cbn, mask_slope), pre (out_pre).  The instance each
# launch takes (_convd_instance; forward writes cout channels, the data gradient roundup8(cin)):
#   "PT 2" cases: cin 3..16 -> cout 40 / 64 at >= 256 tiles: forward (2, 2), data gradient (1, 2), 6 row tiles, the last partial
#   "PT 1" cases: cin 40..128 -> cout 3 / 13 / 24 / 96 below 256 tiles: forward (1, 1), data gradient (2, 1)
CONVD = [
    (3, 1, 3, 40, 2, 43, 700, dict(slope=0.2, alpha=0.5, res1=0.75, res2=-1.25, res_cbn=3, pre=True),
     dict(acc=True, mask=(0, 1, 0.0))),
    (3, 1, 64, 24, 3, 9, 33, dict(post=1, slope=0.0, res1=1.0),
     dict(acc=True, alpha=0.5, mask=(2, 5, 0.2))),
    (3, 1, 8, 96, 1, 43, 480, dict(slope=0.0, res1=1.0, mask=(4, 6, 0.0)),          # 3 groups at 270 tiles: (1, 2)
     dict(post=1, slope=0.2, alpha=-0.5, res1=0.5)),
    (3, 2, 16, 64, 2, 43, 700, dict(post=1, slope=0.2, alpha=1.5, res1=1.0, res2=0.5, res_cbn=5, acc=True, mask=(1, 6, 0.0)),
     dict(mask=(0, 2, 0.0), pre=True, slope=0.0)),
    (3, 2, 64, 13, 2, 17, 40, dict(slope=0.0, alpha=0.5, res1=1.0, pre=True, acc=True),
     dict(post=1, slope=0.0, res1=1.0)),
    (3, 3, 8, 40, 2, 45, 700, dict(slope=0.2, res1=1.0, res2=0.25, acc=True, mask=(2, 3, 0.2)),
     dict(post=1, slope=0.2, alpha=0.5, res1=1.0)),
    (3, 3, 128, 96, 1, 15, 70, dict(slope=0.0, alpha=0.5, res1=1.0, res_cbn=7, pre=True),
     dict(acc=True, mask=(3, 10, 0.0))),
    (3, 4, 16, 64, 2, 43, 700, dict(post=1, slope=0.0, res1=1.0, res2=-1.0, res_cbn=6, mask=(0, 8, 0.0)),
     dict(pre=True, slope=0.2, alpha=0.5, res1=1.0)),
    (3, 4, 40, 3, 3, 11, 37, dict(slope=0.2, alpha=0.5, res1=1.0, acc=True, mask=(0, 1, 0.2), pre=True),
     dict(post=1, acc=True, slope=0.0, mask=(1, 3, 0.0))),
    (1, 1, 8, 40, 2, 43, 700, dict(post=1, slope=0.0, res1=1.0),
     dict(acc=True, mask=(0, 1, 0.0), pre=True)),
    (1, 1, 64, 13, 2, 17, 40, dict(slope=0.2, alpha=0.5, res1=1.0, res2=0.5, res_cbn=1, acc=True, mask=(1, 1, 0.2), pre=True),
     dict(post=1, slope=0.2, res1=1.0)),
    # the 4-row switch: 255 and 256 tiles; H = 4 (never 4-row) and H = 5
    (3, 2, 8, 8, 1, 120, 544, dict(slope=0.2, res1=1.0), dict(acc=True)),
    (3, 2, 8, 8, 1, 64, 1024, dict(slope=0.2, res1=1.0), dict(acc=True)),
    (3, 3, 3, 24, 2, 4, 40, dict(pre=True, slope=0.0, res1=1.0), dict(acc=True, mask=(0, 1, 0.0))),
    (3, 3, 3, 24, 2, 5, 40, dict(post=1, slope=0.0, res1=1.0), dict(acc=True, mask=(0, 1, 0.2))),
]


def _cid(c):
    return f'k{c[0]}d{c[1]}-{c[2]}to{c[3]}-n{c[4]}-{c[5]}x{c[6]}'


def _launches(case):
    """[(kind, launch cout, (COT, PT, row_tiles), 8-row tile count)] of a case: the forward and the data-gradient launch."""
    ks, d, cin, cout, n, h, w = case[:7]
    cin_pad = (cin + 7) // 8 * 8
    return [('fwd', cout, _convd_instance(ks, d, cout, n, h, w), _convd_tiles(ks, d, cout, n, h, w)),
            ('dgrad', cin_pad, _convd_instance(ks, d, cin_pad, n, h, w), _convd_tiles(ks, d, cin_pad, n, h, w))]


def _boundary(size, tile, d):
    """A tile boundary B with its farthest halo lines B - d and B - 1 + d inside [0, size), the last one that fits; None when
    there is only one tile."""
    for b in range((size - 1) // tile * tile, 0, -tile):
        if b - d >= 0 and b - 1 + d < size:
            return b
    return None


def _spikes(ks, d, h, w, th):
    """[(source (y, x), output (y, x) across the boundary that reads it)] for tile height th and 32-column strips."""
    out = []
    B = _boundary(h, th, d)
    C0 = _boundary(w, 32, d)
    xc, yc = w // 2, h // 2
    r = d if ks == 3 else 0
    if B is not None:
        out += [((B - r, xc), (B, xc)), ((B - 1 + r, xc), (B - 1, xc))]
    if C0 is not None:
        out += [((yc, C0 - r), (yc, C0)), ((yc, C0 - 1 + r), (yc, C0 - 1))]
    if not out:
        out = [((h - 1, w - 1), (h - 1, w - 1))]
    return out


def _run_convd(lib, cuda, ks, d, src_c, dst_c, n, h, w, o, mode, seed):
    """One sr_convd_f32 launch of src_c -> dst_c channels (mode 0: forward with bias; mode 1: the data gradient of a forward
    conv dst_c -> src_c, through the flipped mode-1 image) against float64; returns the kernel ids launched."""
    rng = np.random.default_rng(seed)
    taps = ks * ks
    pad = d * (ks - 1) // 2
    src_pad, dst_pad = (src_c + 7) // 8 * 8, (dst_c + 7) // 8 * 8
    if mode == 0:
        wt = _rand(rng, (dst_c, src_c, ks, ks)) * (1.0 / (src_c * taps)) ** 0.5
        wt[:, -1] = 0.5                       # the spiked source channel: +1/2 on every tap
        bias = _rand(rng, (dst_c,)) * 0.5
        wfull = torch.zeros(dst_pad, src_pad, ks, ks, dtype=torch.float64)
        wfull[:dst_c, :src_c] = wt
        bfull = torch.zeros(dst_pad, dtype=torch.float64)
        bfull[:dst_c] = bias

        def conv(x):
            return (F.conv2d(x, wfull, bfull, padding=pad, dilation=d),
                    F.conv2d(x.abs(), wfull.abs(), bfull.abs(), padding=pad, dilation=d))
    else:
        wt = _rand(rng, (src_c, dst_c, ks, ks)) * (1.0 / (src_c * taps)) ** 0.5   # the forward conv dst_c -> src_c
        wt[-1] = 0.5
        bias = None
        wfull = torch.zeros(src_pad, dst_pad, ks, ks, dtype=torch.float64)
        wfull[:src_c, :dst_c] = wt

        def conv(x):
            return (F.conv_transpose2d(x, wfull, padding=pad, dilation=d),
                    F.conv_transpose2d(x.abs(), wfull.abs(), padding=pad, dilation=d))
    k = 2 * taps * src_pad + 8
    post, slope, alpha = o.get('post', 0), o.get('slope', 1.0), o.get('alpha', 1.0)
    res_cbn = o.get('res_cbn', 0)
    dst_blocks = dst_pad // 8
    ops = {}
    for name in ('res1', 'res2'):
        if name in o:
            ops[name] = _rand(rng, (n, dst_pad, h, w))
    if o.get('acc'):
        ops['prior'] = _rand(rng, (n, dst_pad, h, w))
    if 'mask' in o:
        mcb0, mcbn, mslope = o['mask']
        m = _rand(rng, (n, mcbn * 8, h, w))
        z = rng.random(m.shape)
        m[torch.from_numpy(z < 0.1)] = 0.0
        m[torch.from_numpy((z >= 0.1) & (z < 0.2))] = -0.0
        ops['mask'] = m
    resmask = torch.ones(1, dst_pad, 1, 1, dtype=torch.float64)
    if res_cbn:
        resmask[:, res_cbn * 8:] = 0

    def act(v):
        return torch.where(v > 0, v, slope * v)

    def epilogue(c, a):
        A = abs(alpha) * a
        if post:
            v = alpha * c
        else:
            v = alpha * act(c)
        pre = v
        for name in ('res1', 'res2'):
            if name in ops:
                v = v + resmask * o[name] * ops[name]
                A = A + resmask * abs(o[name]) * ops[name].abs()
        if post:
            v = act(v)
        if 'prior' in ops:
            v = v + ops['prior']
            A = A + ops['prior'].abs()
        if 'mask' in ops:
            lo, hi = mcb0 * 8, min((mcb0 + mcbn) * 8, dst_pad)
            v = v.clone()
            v[:, lo:hi] = torch.where(ops['mask'][:, :hi - lo] > 0, v[:, lo:hi], mslope * v[:, lo:hi])
        return v, A, pre

    inst = _convd_instance(ks, d, dst_c if mode == 0 else dst_pad, n, h, w)
    spikes = _spikes(ks, d, h, w, 4 * inst[1])
    x = _rand(rng, (n, src_pad, h, w))          # pad channels hold finite values the zero weights must cancel
    x[:, src_c:] = torch.from_numpy(rng.standard_normal((n, src_pad - src_c, h, w))) * 100.0
    if 'mask' in ops:                           # the outputs across the boundaries pass the mask
        for _, (oy, ox) in spikes:
            ops['mask'][-1, :, oy, ox] = 1.0
    y0, A0, _ = epilogue(*conv(x))
    spike = 64.0 * (k * EPS * float(A0.max()) + EPS * float(y0.abs().max())) / (0.5 * 0.2 * max(abs(alpha), 1e-3)) + 64.0
    xs = x.clone()
    for (sy, sx), _ in spikes:
        xs[-1, src_c - 1, sy, sx] = spike
    y64, A, pre64 = epilogue(*conv(xs))

    in_buf = _to_cb8(xs, 1 + src_pad // 8 + 1, 1, cuda)
    out_buf = _to_cb8(ops.get('prior', torch.full((n, dst_pad, h, w), float('nan'), dtype=torch.float64)), 2 + dst_blocks + 1, 2, cuda)
    if mode == 0:
        pc = hip_ops.PackedConvK(wt.float().to(cuda), bias.float().to(cuda), mode=0)
    else:
        pc = hip_ops.PackedConvK(wt.float().to(cuda), None, mode=1)
    assert pc.src_channels == src_pad and pc.cout == (dst_c if mode == 0 else dst_pad)
    dd = _lib.ConvdDesc()
    b = dd.base
    b.in_, b.in_img_stride, b.cin_pad, b.in_h, b.in_w = _ptr(in_buf, 1), _stride(in_buf), src_pad, h, w
    b.wpacked, b.bpacked, b.cout = pc.w.data_ptr(), (pc.b.data_ptr() if pc.b is not None else None), pc.cout
    b.out, b.out_img_stride, b.n, b.act_slope, b.alpha = _ptr(out_buf, 2), _stride(out_buf), n, slope, alpha
    keep = []
    for name in ('res1', 'res2'):
        if name in ops:
            rb = _to_cb8(ops[name], dst_blocks + 2, 1, cuda)
            keep.append(rb)
            setattr(b, name, _ptr(rb, 1))
            setattr(b, name + '_img_stride', _stride(rb))
            setattr(b, 'beta' + name[-1], o[name])
    b.res_cbn = res_cbn
    b.accumulate = int('prior' in ops)
    if 'mask' in ops:
        mb = _to_cb8(ops['mask'], mcb0 + mcbn + 2, 1, cuda)
        keep.append(mb)
        b.mask_src, b.mask_img_stride, b.mask_cb0, b.mask_cbn, b.mask_slope = _ptr(mb, 1), _stride(mb), mcb0, mcbn, mslope
    dd.ksize, dd.dilation, dd.post_act = ks, d, post
    pre_buf = None
    if o.get('pre'):
        pre_buf = _to_cb8(torch.full((n, dst_pad, h, w), float('nan'), dtype=torch.float64), dst_blocks + 2, 1, cuda)
        dd.out_pre, dd.out_pre_img_stride = _ptr(pre_buf, 1), _stride(pre_buf)
    ids = _profiled_ids(lib, lambda: _lib.check(lib.sr_convd_f32(C.byref(dd), _st()), 'sr_convd_f32'))
    torch.cuda.synchronize()
    what = (ks, d, src_c, dst_c, n, h, w, mode, inst)
    assert ids == [81 if ks == 3 else 82], ids
    _sentinel_kept(out_buf, 2, 2 + dst_blocks, what)
    _sentinel_kept(in_buf, 1, 1 + src_pad // 8, what)
    got = _from_cb8(out_buf, 2, dst_pad)
    bound = _check(got, y64, A, k, what)
    if pre_buf is not None:
        _sentinel_kept(pre_buf, 1, 1 + dst_blocks, what)
        _check(_from_cb8(pre_buf, 1, dst_pad), pre64, abs(alpha) * conv(xs)[1], k, (what, 'out_pre'))
    # sensitivity: every spike's contribution at the output across its boundary exceeds four bounds
    delta = (y64 - y0)[-1, (dst_pad - 8):]
    for (sy, sx), (oy, ox) in spikes:
        r = float((delta[:, oy, ox].abs() / bound[-1, (dst_pad - 8):, oy, ox]).max())
        assert r > 4.0, (what, 'spike', (sy, sx), 'at', (oy, ox), r)
    return ids


@pytest.mark.parametrize('case', CONVD, ids=[_cid(c) for c in CONVD])
def test_convd_forward(cuda, lib, case):
    ks, d, cin, cout, n, h, w, fo, _ = case
    _run_convd(lib, cuda, ks, d, cin, cout, n, h, w, fo, 0, sum(map(ord, _cid(case))))


@pytest.mark.parametrize('case', CONVD, ids=[_cid(c) for c in CONVD])
def test_convd_data_gradient(cuda, lib, case):
    ks, d, cin, cout, n, h, w, _, go = case
    _run_convd(lib, cuda, ks, d, cout, cin, n, h, w, go, 1, 7 + sum(map(ord, _cid(case))))


# ------------------------------------------------------------------------------------------------------ production size, exact
def _cb8_rand(g, n, c, h, w, cuda, zeros=False):
    t = torch.randn((n, c // 8, h, w, 8), generator=g, dtype=torch.float32)
    if zeros:                          # ReLU outputs: full of exact zeros
        t = torch.relu(t)
    return hip_ops.CB8(t.to(cuda))


def _phase(t, a, b, d):
    return hip_ops.CB8(t.buf[:, t.cb0:t.cb0 + t.cbn, a::d, b::d].contiguous())


def _bits(t):
    return t.buf[:, t.cb0:t.cb0 + t.cbn].view(torch.int32)


# (cin, cout): the 64 -> 64 layers of MergeRun / EResidualBlockNoBN and the 128 -> 64 aggregation
@pytest.mark.parametrize('d', [1, 2, 3, 4])
@pytest.mark.parametrize('cin,cout', [(64, 64), (128, 64)])
def test_production_size_equals_conv3x3_bit_for_bit(cuda, d, cin, cout):
    """16 x 128^2, the 8-row path with 16 row tiles.  A dilated 3x3 splits into d^2 independent dense 3x3 convs, one per
    polyphase grid (rows a, a + d, ..., columns b, b + d, ...): zero padding of a phase is the image's, since a - d < 0 and
    a + d ceil((H - a) / d) >= H.  sr_conv3x3_f32 on a phase runs the same MFMA chain per output (chunk by chunk, tap by tap,
    the same weight image) and the same epilogue operations, so each phase of the sr_convd_f32 output equals it bit for bit,
    forward and data gradient, with the epilogues RIDNet uses: res1 (+ out_pre against a call without the residual), ReLU after
    the residual add (against a float32 ReLU of the linear conv3x3 epilogue), and the ReLU mask (slope 0)."""
    n, H, W = 16, 128, 128
    assert _convd_instance(3, d, cout, n, H, W)[1:] == (2, 16) and _convd_instance(3, d, cin, n, H, W)[1:] == (2, 16)
    g = torch.Generator().manual_seed(100 * d + cin)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (cin * 9)) ** 0.5).to(cuda)
    bias = (torch.randn(cout, generator=g) * 0.1).to(cuda)
    x = _cb8_rand(g, n, cin, H, W, cuda, zeros=True)
    r1 = _cb8_rand(g, n, cout, H, W, cuda)
    msk = _cb8_rand(g, n, cin, H, W, cuda, zeros=True)
    dy = _cb8_rand(g, n, cout, H, W, cuda)
    pk = hip_ops.PackedConvK(wt, bias)
    pk1 = hip_ops.PackedConvK(wt, None, mode=1)
    p3, p31 = hip_ops.PackedConv(wt, bias), hip_ops.PackedConv(wt, None, mode=1)
    pre = hip_ops.CB8.empty(n, cout, H, W, cuda)
    out_res = hip_ops.convd(x, pk, d, act_slope=0.0, res1=r1, beta1=1.0, out_pre=pre)
    out_post = hip_ops.convd(x, pk, d, post_act=True, act_slope=0.0, res1=r1, beta1=1.0)
    dx = hip_ops.convd(dy, pk1, d, mask=msk, mask_slope=0.0)
    for a in range(d):
        for b in range(d):
            xp, rp, mp, dyp = _phase(x, a, b, d), _phase(r1, a, b, d), _phase(msk, a, b, d), _phase(dy, a, b, d)
            want = hip_ops.conv3x3(xp, p3, act_slope=0.0, res1=rp, beta1=1.0)
            assert torch.equal(_bits(_phase(out_res, a, b, d)), _bits(want)), ('res1', d, a, b)
            want = hip_ops.conv3x3(xp, p3, act_slope=0.0)
            assert torch.equal(_bits(_phase(pre, a, b, d)), _bits(want)), ('out_pre', d, a, b)
            lin = hip_ops.conv3x3(xp, p3, act_slope=1.0, res1=rp, beta1=1.0)
            want = torch.where(lin.buf > 0, lin.buf, lin.buf * 0.0)
            assert torch.equal(_phase(out_post, a, b, d).buf.view(torch.int32), want.view(torch.int32)), ('post_act', d, a, b)
            want = hip_ops.conv3x3(dyp, p31, mask=mp, mask_slope=0.0)
            assert torch.equal(_bits(_phase(dx, a, b, d)), _bits(want)), ('dgrad', d, a, b)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ sr_convd_wgrad_f32
# (ksize, d, cin, cout, n, h, w, options): options scale, bias (False: dbias NULL), acc (arena accumulate).  Plans
# (_wgradd_plan, CT x IT): ksize 1 and d <= 2 take 2x2 when both tile counts (32 channels) are even, else 1x1; d 3 / 4 take 2x1
# when the cout tiles are even, else 1x1.  The 16 x 128^2 8 -> 8 cases run 16 rows per workgroup: the ring of 2 + d (k - 1)
# rows wraps within one workgroup.
WGRADD = [
    (3, 1, 64, 64, 2, 19, 45, dict(scale=0.5)),
    (3, 1, 24, 40, 2, 19, 45, dict(acc=True)),
    (3, 2, 128, 64, 1, 13, 70, dict(bias=False)),
    (3, 2, 3, 24, 3, 21, 33, dict(scale=-2.0, acc=True)),
    (3, 3, 40, 128, 1, 17, 50, dict()),
    (3, 3, 64, 3, 2, 23, 40, dict(bias=False, acc=True)),
    (3, 4, 24, 64, 2, 19, 45, dict(scale=0.25)),
    (3, 4, 64, 24, 2, 19, 45, dict(acc=True)),
    (1, 1, 64, 128, 1, 17, 50, dict(scale=2.0)),
    (1, 1, 40, 3, 2, 11, 37, dict(bias=False)),
    (1, 1, 8, 8, 16, 128, 128, dict()),
    (3, 1, 8, 8, 16, 128, 128, dict(acc=True)),
    (3, 2, 8, 8, 16, 128, 128, dict(scale=0.5)),
    (3, 3, 8, 8, 16, 128, 128, dict(bias=False)),
    (3, 4, 8, 8, 16, 128, 128, dict()),
]


def _wid(c):
    return f'k{c[0]}d{c[1]}-{c[2]}to{c[3]}-n{c[4]}-{c[5]}x{c[6]}'


@pytest.mark.parametrize('case', WGRADD, ids=[_wid(c) for c in WGRADD])
def test_convd_weight_gradient(cuda, lib, case):
    ks, d, cin, cout, n, h, w, o = case
    rng = np.random.default_rng(sum(map(ord, _wid(case))))
    scale, want_bias, acc = o.get('scale', 1.0), o.get('bias', True), o.get('acc', False)
    ct, it, rows, row_splits, splits = _wgradd_plan(n, h, w, cout, cin, ks, d)
    assert row_splits >= 2, 'every case crosses a row-split boundary'
    k = _wgradd_chain(n, h, w, cout, cin, ks, d)
    pad = d * (ks - 1) // 2
    prior_w = _rand(rng, (cout, cin, ks, ks)) if acc else None
    prior_b = _rand(rng, (cout,)) if acc else None

    def ref(x, dy):
        gw = torch.nn.grad.conv2d_weight(x, (cout, cin, ks, ks), dy, padding=pad, dilation=d) * scale
        aw = torch.nn.grad.conv2d_weight(x.abs(), (cout, cin, ks, ks), dy.abs(), padding=pad, dilation=d) * abs(scale)
        gb, ab = dy.sum((0, 2, 3)) * scale, dy.abs().sum((0, 2, 3)) * abs(scale)
        if acc:
            gw, aw, gb, ab = gw + prior_w, aw + prior_w.abs(), gb + prior_b, ab + prior_b.abs()
        return gw, aw, gb, ab

    # spikes: last image; last row and column (centre tap), and across the last row-split boundary R: x row R - d with dy
    # row R (tap row 0), x row R - 1 + d with dy row R - 1 (tap row 2), in a strip's last column
    R = _boundary(h, rows, pad if ks == 3 else 1)
    assert R is not None
    c0 = min(31, w - 1)
    pairs = [((h - 1, w - 1), (h - 1, w - 1), (1, 1) if ks == 3 else (0, 0))]
    if ks == 3:
        pairs += [((R - d, c0), (R, c0), (0, 1)), ((R - 1 + d, c0), (R - 1, c0), (2, 1))]
    else:
        pairs += [((R, c0), (R, c0), (0, 0)), ((R - 1, c0), (R - 1, c0), (0, 0))]

    def spiked(x, dy, v):
        x, dy = x.clone(), dy.clone()
        for (xy, xx), (gy, gx), _ in pairs:
            x[-1, -1, xy, xx] = v
            dy[-1, :, gy, gx] = v
        return x, dy
    x, dy = _rand(rng, (n, cin, h, w)), _rand(rng, (n, cout, h, w))
    g0, a0, _, _ = ref(x, dy)
    b0 = k * EPS * float(a0[:, -1].max()) + EPS * float(g0[:, -1].abs().max())
    x, dy = spiked(x, dy, math.sqrt(64 * b0 / abs(scale)) + 4.0)
    g64, A, gb64, Ab = ref(x, dy)

    cin_pad = (cin + 7) // 8 * 8
    xb = _to_cb8(x, 1 + cin_pad // 8 + 1, 1, cuda)
    yb = _to_cb8(dy, 1 + (cout + 7) // 8 + 1, 1, cuda)
    nbytes = lib.sr_convd_wgrad_slab_bytes(n, h, w, cout, cin, ks, d)
    assert nbytes == _wgradd_slab_bytes(n, h, w, cout, cin, ks, d)
    slab = torch.empty(nbytes, dtype=torch.uint8, device=cuda)

    def run():
        dw = (prior_w.float() if acc else torch.full((cout, cin, ks, ks), float('nan'))).to(cuda)
        db = ((prior_b.float() if acc else torch.full((cout,), float('nan'))).to(cuda)) if want_bias else None
        dd = _lib.ConvdWgradDesc()
        bb = dd.base
        bb.x, bb.x_img_stride, bb.cin_pad, bb.in_h, bb.in_w, bb.upsample = _ptr(xb, 1), _stride(xb), cin_pad, h, w, 0
        bb.dy, bb.dy_img_stride = _ptr(yb, 1), _stride(yb)
        bb.cout, bb.cin, bb.first_seg, bb.seg, bb.n, bb.scale = cout, cin, cin, 0, n, scale
        bb.dweight, bb.dbias, bb.accumulate = dw.data_ptr(), (db.data_ptr() if db is not None else None), int(acc)
        bb.slab, bb.slab_bytes = slab.data_ptr(), nbytes
        dd.ksize, dd.dilation = ks, d
        ids = _profiled_ids(lib, lambda: _lib.check(lib.sr_convd_wgrad_f32(C.byref(dd), _st()), 'sr_convd_wgrad_f32'))
        torch.cuda.synchronize()
        assert ids == [83 if ks == 3 else 84], ids
        return dw, db
    dw, db = run()
    dw2, db2 = run()
    assert torch.equal(dw.view(torch.int32), dw2.view(torch.int32)), 'weight gradient not bit-reproducible'
    if want_bias:
        assert torch.equal(db.view(torch.int32), db2.view(torch.int32))
    what = (case, (ct, it, rows, row_splits, splits), k)
    bound = _check(dw.cpu().double(), g64, A, k, what)
    if want_bias:
        _check(db.cpu().double(), gb64, Ab, k, (what, 'bias'))
    gns, _, _, _ = ref(*spiked(x, dy, 0.0))
    for _, _, (ty, tx) in pairs:
        r = float(((g64 - gns)[:, -1, ty, tx].abs() / bound[:, -1, ty, tx]).max())
        assert r > 4.0, (what, 'spike at tap', (ty, tx), r)


# ------------------------------------------------------------------------------------------------------ streaming helpers
def _cb8_window(t, extra, cuda):
    """NCHW float32 -> CB8 window at block 1 of a buffer with `extra` sentinel blocks on both sides."""
    n, c, h, w = t.shape
    buf = torch.full((n, c // 8 + 2 * extra, h, w, 8), SENTINEL, dtype=torch.float32)
    buf[:, extra:extra + c // 8] = t.reshape(n, c // 8, 8, h, w).permute(0, 1, 3, 4, 2)
    return hip_ops.CB8(buf.to(cuda), extra, c // 8)


def _nchw(t):
    return t.buf[:, t.cb0:t.cb0 + t.cbn].permute(0, 1, 4, 2, 3).reshape(t.n, t.channels, t.h, t.w).cpu()


def _window_kept(t, what):
    b = t.buf.cpu()
    assert bool((b[:, :t.cb0] == SENTINEL).all()) and bool((b[:, t.cb0 + t.cbn:] == SENTINEL).all()), what


def _ieee_mask(g, shape):
    """A mask with exact +0, -0 and NaN besides normal values (a ReLU output is full of zeros)."""
    m = torch.randn(shape, generator=g)
    z = torch.rand(shape, generator=g)
    m[z < 0.15] = 0.0
    m[(z >= 0.15) & (z < 0.3)] = -0.0
    m[(z >= 0.3) & (z < 0.35)] = float('nan')
    return m


HELPER_SHAPES = [(1, 8, 1, 1), (2, 24, 7, 9), (3, 64, 5, 33), (2, 128, 9, 3), (16, 64, 128, 128)]


@pytest.mark.parametrize('n,nf,h,w', HELPER_SHAPES, ids=[f'n{s[0]}-c{s[1]}-{s[2]}x{s[3]}' for s in HELPER_SHAPES])
@pytest.mark.parametrize('slope', [0.0, 0.2])
@pytest.mark.parametrize('inplace', [False, True])
def test_relu_mask_bit_for_bit(cuda, n, nf, h, w, slope, inplace):
    """out = mask > 0 ? g : slope * g: one float32 product or none per element, so the float32 torch.where(m > 0, ...) is the
    exact result; +0, -0 and NaN in the mask take the slope branch.  In place (out = g) as ridnet_autograd calls it."""
    g = torch.Generator().manual_seed(n * 1000 + nf + h + w + int(slope * 10))
    gr = torch.randn((n, nf, h, w), generator=g)
    m = _ieee_mask(g, (n, nf, h, w))
    gd, md = _cb8_window(gr, 1, cuda), _cb8_window(m, 2, cuda)
    out = hip_ops.relu_mask(gd, md, slope=slope, out=gd if inplace else None)
    torch.cuda.synchronize()
    want = torch.where(m > 0, gr, gr * torch.tensor(slope, dtype=torch.float32))
    assert torch.equal(_nchw(out).view(torch.int32), want.view(torch.int32))
    _window_kept(gd, 'g window')
    _window_kept(md, 'mask window')
    if not inplace:
        assert torch.equal(_nchw(gd), gr), 'the source changed'


@pytest.mark.parametrize('n,nf,h,w', HELPER_SHAPES, ids=[f'n{s[0]}-c{s[1]}-{s[2]}x{s[3]}' for s in HELPER_SHAPES])
@pytest.mark.parametrize('inplace', [False, True])
def test_ca_scale_bit_for_bit(cuda, n, nf, h, w, inplace):
    """out = u * s[n][c]: one float32 product per element; in place (out = u) and on channel-slice windows."""
    g = torch.Generator().manual_seed(n * 100 + nf + h * 3 + w)
    u = torch.randn((n, nf, h, w), generator=g)
    s = torch.rand((n, nf), generator=g)
    s[0, 0] = 0.0
    ud = _cb8_window(u, 1, cuda)
    out = hip_ops.ca_scale(ud, s.to(cuda), out=ud if inplace else None)
    torch.cuda.synchronize()
    want = u * s[:, :, None, None]
    assert torch.equal(_nchw(out).view(torch.int32), want.view(torch.int32))
    _window_kept(ud, 'u window')


# ------------------------------------------------------------------------------------------------------ MeanShift ends
U32 = EPS


def _within(got, want, bound, what):
    err = (got.double() - want.double()).abs()
    assert bool((err <= bound + 1e-30).all()), (what, float(err.max()), float((err / (bound + 1e-30)).max()))


# per-image pixel counts 4095 / 4096 / 4097 / 8193 around the kMeanPixels = 4096 bands (one grid row per image), and
# 16 x 128^2 (64 partials)
MEAN_SHAPES = [(2, 45, 91), (3, 64, 64), (2, 17, 241), (2, 3, 2731), (16, 128, 128)]


@pytest.mark.parametrize('n,h,w', MEAN_SHAPES, ids=[f'n{s[0]}-{s[1]}x{s[2]}' for s in MEAN_SHAPES])
def test_mean_shift_bands(cuda, lib, n, h, w):
    """The MeanShift forward and both adjoints against float64 with tests/test_ridnet_gpu.py's bounds, at band edges.  The
    last pixel of every image carries a spike in the gradient, so a band that is dropped, or a band boundary off by one,
    moves dW / db by far more than the bound; SR_ENOSPACE one byte short; accumulate with db = NULL."""
    g = torch.Generator().manual_seed(n * 10 + h + w)
    x = torch.rand(n, 3, h, w, generator=g, dtype=torch.float64).float()
    W = (torch.eye(3, dtype=torch.float64) + 0.05 * torch.randn(3, 3, generator=g, dtype=torch.float64)).float().view(3, 3, 1, 1)
    b = (torch.randn(3, generator=g, dtype=torch.float64) * 100).float()
    xd, Wd, bd = x.to(cuda), W.to(cuda), b.to(cuda)
    W2 = W.double()[:, :, 0, 0]
    s = hip_ops.ridnet_sub_mean(xd, Wd, bd)
    want = torch.einsum('ck,nkhw->nchw', W2, x.double()) + b.double()[None, :, None, None]
    sb = 4 * U32 * (torch.einsum('ck,nkhw->nchw', W2.abs(), x.double().abs()) + b.double().abs()[None, :, None, None])
    got = _nchw(s)
    _within(got[:, :3], want, sb, 'sub_mean')
    assert torch.equal(got[:, 3:], torch.zeros_like(got[:, 3:]))
    t = torch.randn((n, 8, h, w), generator=g, dtype=torch.float64) * 50
    t[:, 3:] = float('nan')
    td = _cb8_window(t.float(), 1, cuda)
    y = hip_ops.ridnet_add_mean(xd, td, Wd, bd)
    t3 = t[:, :3].float().double()
    mix = torch.einsum('ck,nkhw->nchw', W2, t3) + b.double()[None, :, None, None]
    _within(y.cpu(), x.double() + mix, 5 * U32 * (x.double().abs() + torch.einsum('ck,nkhw->nchw', W2.abs(), t3.abs())
                                                   + b.double().abs()[None, :, None, None]), 'add_mean')
    P = n * h * w
    gy = torch.randn((n, 3, h, w), generator=g).float()
    gy[:, :, -1, -1] = 1e4                # the last pixel of each image: the last band's
    dW, db = torch.empty(3, 3, 1, 1, device=cuda), torch.empty(3, device=cuda)
    dt = hip_ops.ridnet_add_mean_bwd(gy.to(cuda), td, Wd, dW.data_ptr(), db.data_ptr())
    g64 = gy.double()
    _within(dW.cpu()[:, :, 0, 0], torch.einsum('nchw,nkhw->ck', g64, t3),
            (P + 80) * U32 * torch.einsum('nchw,nkhw->ck', g64.abs(), t3.abs()), 'add dW')
    _within(db.cpu(), g64.sum((0, 2, 3)), (P + 80) * U32 * g64.abs().sum((0, 2, 3)), 'add db')
    dtc = _nchw(dt)
    _within(dtc[:, :3], torch.einsum('ck,nchw->nkhw', W2, g64), 4 * U32 * torch.einsum('ck,nchw->nkhw', W2.abs(), g64.abs()), 'dt')
    assert torch.equal(dtc[:, 3:], torch.zeros_like(dtc[:, 3:]))
    gs = torch.randn((n, 8, h, w), generator=g)
    gs[:, :3, -1, -1] = 1e4
    gsd = _cb8_window(gs, 1, cuda)
    dW2, db2 = torch.empty_like(dW), torch.empty_like(db)
    res = torch.randn((n, 3, h, w), generator=g)
    dx = hip_ops.ridnet_sub_mean_bwd(xd, gsd, Wd, dW2.data_ptr(), db2.data_ptr(), want_dx=True, dx_res=res.to(cuda))
    gs3 = gs[:, :3].double()
    _within(dW2.cpu()[:, :, 0, 0], torch.einsum('nchw,nkhw->ck', gs3, x.double()),
            (P + 80) * U32 * torch.einsum('nchw,nkhw->ck', gs3.abs(), x.double().abs()), 'sub dW')
    _within(db2.cpu(), gs3.sum((0, 2, 3)), (P + 80) * U32 * gs3.abs().sum((0, 2, 3)), 'sub db')
    _within(dx.cpu(), torch.einsum('ck,nchw->nkhw', W2, gs3) + res.double(),
            5 * U32 * (torch.einsum('ck,nchw->nkhw', W2.abs(), gs3.abs()) + res.double().abs()), 'dx')
    # accumulate with db = NULL adds into dW only
    acc = dW2.clone()
    hip_ops.ridnet_sub_mean_bwd(xd, gsd, Wd, acc.data_ptr(), None, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(acc, dW2 + dW2)
    # the workspace one byte short is refused before any launch
    need = lib.sr_ridnet_mean_workspace_bytes(n, h, w)
    assert need == (n * _cdiv(h * w, 4096) * 12 * 4 + 255) // 256 * 256
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    keep = dW2.clone()
    rc = lib.sr_ridnet_sub_mean_bwd_f32(xd.data_ptr(), gsd.ptr, gsd.img_stride, Wd.data_ptr(), dW2.data_ptr(), None, 0, None, None,
                                        n, h, w, ws.data_ptr(), need - 1, _st())
    assert rc == -3     # SR_ENOSPACE
    gyd = gy.to(cuda)
    rc = lib.sr_ridnet_add_mean_bwd_f32(gyd.data_ptr(), td.ptr, td.img_stride, Wd.data_ptr(), dW2.data_ptr(), None, 0,
                                        dt.ptr, dt.img_stride, n, h, w, ws.data_ptr(), need - 1, _st())
    assert rc == -3
    torch.cuda.synchronize()
    assert torch.equal(dW2, keep)


# ------------------------------------------------------------------------------------------------------ coverage
def test_dispatch_coverage():
    """The cases of this module reach, by the restated dispatch: all 20 convd instances (forward or data gradient); each 8-row
    instance with >= 3 row tiles, the last partial; 255 and 256 tiles and H = 4 and 5; the 10 reachable weight-gradient plans;
    and for every dilation a weight-gradient case whose rows_per_wg exceeds the ring depth 2 + d (k - 1)."""
    fwd, deep, tiles, heights = set(), set(), set(), set()
    for case in CONVD:
        ks, d, _, _, n, h, w = case[:7]
        for _, _, (cot, pt, ty), t8 in _launches(case):
            fwd.add((cot, pt, ks, d))
            tiles.add(t8)
            heights.add((h, pt))
            if pt == 2 and ty >= 3 and h % 8:
                deep.add((cot, pt, ks, d))
    want = {(cot, pt, ks, d) for cot in (1, 2) for pt in (1, 2) for ks, d in ((1, 1), (3, 1), (3, 2), (3, 3), (3, 4))}
    assert len(want) == 20 and fwd == want, sorted(want - fwd)
    assert deep == {i for i in want if i[1] == 2}, sorted({i for i in want if i[1] == 2} - deep)
    assert {255, 256} <= tiles and {(4, 2), (5, 1)} <= heights
    plans, ring = set(), {}
    for ks, d, cin, cout, n, h, w, _ in WGRADD:
        ct, it, rows, _, _ = _wgradd_plan(n, h, w, cout, cin, ks, d)
        plans.add((ct, it, ks, d))
        ring[(ks, d)] = max(ring.get((ks, d), 0), rows - (2 + d * (ks - 1)))
    reachable = {(2, 2, 1, 1), (1, 1, 1, 1), (2, 2, 3, 1), (1, 1, 3, 1), (2, 2, 3, 2), (1, 1, 3, 2), (2, 1, 3, 3), (1, 1, 3, 3),
                 (2, 1, 3, 4), (1, 1, 3, 4)}
    assert plans == reachable, sorted(reachable - plans)
    assert all(v > 0 for v in ring.values()) and len(ring) == 5, ring
    print(f'convd instances {len(fwd)}/20, 8-row instances with >= 3 row tiles {len(deep)}/10, '
          f'wgradd plans {len(plans)}/10')
