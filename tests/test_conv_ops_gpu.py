"""Every convolution entry point against float64 references of the same operation, one case per dispatch path, with the
path proven by the launch profiler: sr_conv3x3_f32 (every default instance, crossed with upsample, LeakyReLU, alpha,
residuals and res_cbn, accumulate, a mask window, channel-slice source and destination, concat segmentation and the
data-gradient packing), sr_conv4x4s2_f32 / _dgrad_f32 / sr_conv4x4s2_wgrad_f32 at even and odd sizes (odd sizes mix the
stacked-batch and generic launches over the four parity passes of one output), sr_conv3x3_wgrad_f32 (segmentation,
upsample, scale, accumulate, no bias, a production-sized case), sr_conv4x4s2_weight_as_3x3_f32 (data movement), sr_conv3x3_bf16
(every tile shape and group width, NCHW, few-cout, streaming, s2 on both sides, unshuffled output and residual, res1_keep_sign),
sr_conv3x3_wgrad_bf16 (every instance at W <= 16, <= 32 and wider) and sr_rdb_wgrad_bf16.

Tolerances are bounds, not fits.  EPS = 2^-24.  For every output element let A be the same convolution of the absolute
values in float64 (same taps, same padding): A = |alpha| (conv(|x|, |w|) + |bias|) + |beta1 r1| + |beta2 r2| (+ |prior out|
when accumulating).  Then |y - y64| <= k EPS A + EPS |y64|, where k counts the fp32 roundings of the longest chain:
  - the MFMA sum over (cin, tap): two roundings per product (the internal rounding of v_mfma_f32_32x32x2_f32 is not
    documented), so 2 * taps * cin_pad;
  - one per separate pass through memory: the 4x4/s2 forward sums four parity passes in its destination (+4);
  - the epilogue: bias add, activation, alpha, two residual multiply-adds, accumulate, mask (+8).
  A LeakyReLU slope <= 1 and a mask slope <= 1 only shrink an error; where the rounded pre-activation has the other sign
  than the exact one, the branch difference is at most the pre-activation's own error.
fp32 weight gradients follow the kernel's summation order, restated from the host code (_wgrad_f32_plan): one wave sums
rows_per_wg x 32 / KS products (two roundings each), the slab reduction then adds `chunk` splits in stage 1 and `sch` chunks
in stage 2, +3 for scale, bias and accumulate: k = 2 rows_per_wg 32 / KS + chunk + sch + 3.  bf16 weight gradients (wgrad_bf16.hip)
walk imgs_per_wg images of rows_per_wg rows of a 64-pixel strip per workgroup; k = 2 imgs_per_wg rows_per_wg 64 + KS + chunk +
sch + 3 (_wgrad_bf16_plan).  The fused dense-block weight gradient plans its work inside the library; its bound is the
order-independent one, k = 2 n H W + 3: any order of summing N products loses at most (N - 1) roundings.
bf16 paths: every operand is rounded to bf16 before the float64 reference (the products are then exact in fp32); a bf16
destination adds its own rounding, 2^-8 |y64|.

Sensitivity is asserted, not assumed: every case plants one spike at the border pixel (0, 0) of the last input channel of
the last image, weighted by a corner tap of +-1/2, such that its contribution at the output it reaches through that tap
exceeds four bounds there: a kernel that drops a halo tap, the tail channel block or the last image fails.  Weight-gradient
cases put the spike in the last image, last row and last column of both the source and the output gradient.
"""
import ctypes as C
import math
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from image_restoration_amd import _lib

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
TINY = 1e-30
SEEN = set()  # kernel ids launched by this module (test_dispatch_coverage)
F32_3X3_IDS = {14, 1, 44, 45, 41, 15, 4, 0}
F32_4X4_IDS = {2, 6, 46, 47}
SENTINEL = 12345.0  # blocks outside a channel slice: must stay as they are, and must not leak into the result


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _profiled(lib, fn):
    """Runs fn() under the launch profiler; returns the kernel ids it launched (in order)."""
    _lib.check(lib.sr_profile_start(256), 'sr_profile_start')
    try:
        fn()
    finally:
        recs = (_lib.LaunchRecord * 256)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, 256, C.byref(cnt)), 'sr_profile_stop')
    ids = [recs[i].kernel_id for i in range(min(cnt.value, 256))]
    SEEN.update(ids)
    return ids


# ------------------------------------------------------------------------------------------------------ CB8 layout helpers
def _seg_positions(cin, first_seg, seg, blk=8):
    """Padded channel position of each reference channel of a segmented concat source (sr_conv3x3_pack_f32: segments start
    on multiples of 8 channels; sr_conv3x3_pack_bf16: of 16)."""
    pos, p = [], 0
    for c in range(first_seg):
        pos.append(p + c)
    p = (first_seg + blk - 1) // blk * blk
    while len(pos) < cin:
        for c in range(seg):
            pos.append(p + c)
        p += (seg + blk - 1) // blk * blk
    return pos, p


def _to_cb8(x, blocks, cb0, cuda, fill=SENTINEL):
    """NCHW (channels <= 8 * (blocks - cb0)) -> device buffer [n][blocks][h][w][8] with x at block cb0; the other blocks and
    the pad channels of x's last block: `fill` outside x's blocks, zero inside."""
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


def _f32(a):
    return a.float().double()


def _check(got, ref, A, k, what):
    bound = k * EPS * A + EPS * ref.abs() + TINY
    err = (got - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), (what, int(bad.sum()), float((err / bound).max()), float(err.max()))
    return bound


def _plant(x, value):
    """The spike: border pixel (0, 0) of the last channel of the last image."""
    x = x.clone()
    x[-1, -1, 0, 0] = value
    return x


def _assert_sensitive(delta, bound, what):
    """delta = the spike's contribution to the reference; it must exceed four bounds somewhere in the last channel block."""
    ratio = (delta.abs() / bound)
    assert float(ratio.max()) > 4.0, (what, 'the spike does not reach four bounds', float(ratio.max()))


# ------------------------------------------------------------------------------------------------------ sr_conv3x3_f32
# (id, n, cin, cout, h, w, options).  Why each shape takes its path (conv_f32.hip, sr_conv3x3_f32; default settings):
#   14  out_nchw, cout <= 4, no residual: conv_fewcout_f32_kernel
#    1  out_nchw with a residual: launch<1, 2, 3, true>
#   44  64-cout groups, W 9..16 -> launch_small WT 16.  PT 2 ('big') when n (H + 1) / 16 * ceil(W / 16) * groups >= 128:
#       n 16, H 63, W 16, cout 128 gives 1024 / 16 * 1 * 2 = 128 (PT 2); the other WT-16 cases are PT 1
#   45  64-cout groups, W <= 8 -> launch_small WT 8.  PT 2 when n (H + 1) / 32 * ceil(W / 8) * groups >= 128:
#       n 16, H 127, W 8, cout 128: 2048 / 32 * 2 = 128 (PT 2)
#   41  64-cout groups, W > 16, tiles_x * ceil(H / 8) * n * groups < 256 and H > 4: 4-row tiles, COT 2
#   15  32-cout groups, the same small-launch rule: 4-row tiles, COT 1
#    4  64-cout groups otherwise (>= 256 workgroups, or H <= 4): launch<2, 2, 3>
#    0  32-cout groups otherwise: launch<1, 2, 3> (8-row tiles, the rows8 default)
C3 = [
    (14, 2, 64, 3, 17, 33, dict(out_nchw=True, slope=0.2, alpha=0.5)),
    (14, 1, 16, 4, 1, 1, dict(out_nchw=True)),
    (14, 3, 8, 1, 16, 7, dict(out_nchw=True, slope=0.0, upsample=True)),
    (1, 2, 32, 3, 9, 33, dict(out_nchw=True, res1=0.25, slope=0.2)),
    (1, 1, 16, 4, 2, 3, dict(out_nchw=True, res1=1.0, res2=-0.5)),
    (44, 2, 16, 64, 7, 9, dict(slope=0.2, alpha=0.5, res1=0.2)),
    (44, 3, 64, 64, 15, 16, dict(accumulate=True, mask=(1, 4))),
    (44, 16, 16, 128, 63, 16, dict(slope=0.2)),
    (44, 9, 24, 64, 8, 16, dict(in_slice=(1, 2), out_slice=(2, 1), res1=0.2, res2=1.0, res_cbn=3, slope=0.2)),
    (45, 1, 8, 64, 1, 1, dict()),
    (45, 2, 16, 64, 1, 2, dict(slope=0.0)),
    (45, 10, 64, 64, 3, 3, dict(in_slice=(2, 0), out_slice=(1, 2), slope=0.2, res1=0.2, res_cbn=5)),
    (45, 2, 16, 64, 4, 4, dict(upsample=True, slope=0.2)),
    (45, 16, 16, 128, 127, 8, dict(alpha=0.2)),
    (45, 3, 56, 64, 7, 8, dict(seg=(20, 12), slope=0.2)),
    (41, 2, 64, 64, 17, 33, dict(slope=0.2, alpha=0.2, res1=1.0, res2=0.2, res_cbn=4)),
    (41, 1, 32, 128, 9, 17, dict(accumulate=True, res1=0.5, mask=(3, 5))),
    (41, 2, 16, 64, 8, 9, dict(upsample=True, slope=0.2)),
    (41, 2, 64, 64, 16, 33, dict(mode1=3)),
    (15, 2, 32, 32, 17, 33, dict(slope=0.2, res1=0.2)),
    (15, 3, 16, 32, 7, 8, dict(accumulate=True, mask=(1, 3), out_slice=(1, 1))),
    (15, 2, 64, 32, 9, 9, dict(upsample=True, alpha=0.5)),
    (15, 1, 64, 96, 15, 16, dict(slope=0.0, res1=1.0, res_cbn=7)),
    (4, 2, 64, 64, 3, 33, dict(slope=0.2)),
    (4, 8, 64, 128, 65, 96, dict(slope=0.2, alpha=0.2, res1=1.0)),
    (4, 1, 128, 64, 2, 40, dict(seg=(64, 32), accumulate=True, in_slice=(1, 1))),
    (4, 2, 64, 64, 1, 17, dict(upsample=True, res1=0.5, res2=0.5, res_cbn=2)),
    (0, 1, 32, 32, 3, 17, dict(slope=0.2)),
    (0, 9, 16, 96, 33, 64, dict(slope=0.2, res1=0.2, out_slice=(1, 2))),
    (0, 2, 64, 32, 1, 1, dict(accumulate=True, mask=(0, 2))),
    (0, 1, 64, 32, 2, 33, dict(mode1=3, accumulate=True, mask=(1, 2))),
]


def _c3_id(c):
    i, n, cin, cout, h, w, o = c
    return f'k{i}-n{n}-{cin}to{cout}-{h}x{w}-' + '-'.join(sorted(o)) if o else f'k{i}-n{n}-{cin}to{cout}-{h}x{w}'


def _rand(rng, shape):
    return _f32(torch.from_numpy(rng.standard_normal(shape)))


def _pack3x3(lib, wt, bias, cout, cin, first_seg, seg, mode, cuda):
    """sr_conv3x3_pack_f32 of an OIHW float64 weight (cout x cin of the FORWARD conv)."""
    cin_pad = lib.sr_conv3x3_cin_pad(cin, first_seg, seg)
    nw = lib.sr_conv3x3_packed_weight_floats(cout, cin_pad) if mode == 0 else \
        lib.sr_conv3x3_packed_weight_floats(cin_pad, (cout + 7) // 8 * 8)
    wpk = torch.empty(nw, dtype=torch.float32, device=cuda)
    wdev = wt.float().contiguous().to(cuda)
    bdev = bias.float().to(cuda) if bias is not None else None
    bpk = torch.empty(lib.sr_conv3x3_packed_bias_floats(cout), dtype=torch.float32, device=cuda) if bias is not None else None
    _lib.check(lib.sr_conv3x3_pack_f32(wdev.data_ptr(), bdev.data_ptr() if bdev is not None else None, cout, cin, first_seg, seg,
                                       mode, wpk.data_ptr(), bpk.data_ptr() if bpk is not None else None, _st()), 'sr_conv3x3_pack_f32')
    return wpk, bpk


def _epilogue(rng, n, dst_c, H, W, o, slope, alpha):
    """The descriptor's epilogue in float64: returns (y64 as a function of the conv, A as a function of |conv|, operands)."""
    res_cbn = o.get('res_cbn', 0)
    resmask = torch.ones(1, dst_c, 1, 1, dtype=torch.float64)
    if res_cbn:
        resmask[:, res_cbn * 8:] = 0
    ops = {}
    for name in ('res1', 'res2'):
        if name in o:
            ops[name] = _rand(rng, (n, dst_c, H, W))
    if o.get('accumulate'):
        ops['prior'] = _rand(rng, (n, dst_c, H, W))
    if 'mask' in o:
        ops['mask'] = _rand(rng, (n, o['mask'][1] * 8, H, W))

    def y_of(c, a):
        v = torch.where(c > 0, c, slope * c) * alpha
        A = abs(alpha) * a
        for name in ('res1', 'res2'):
            if name in ops:
                v = v + resmask * o[name] * ops[name]
                A = A + resmask * abs(o[name]) * ops[name].abs()
        if 'prior' in ops:
            v = v + ops['prior']
            A = A + ops['prior'].abs()
        if 'mask' in ops:
            lo = o['mask'][0] * 8
            hi = min(lo + o['mask'][1] * 8, dst_c)
            v = v.clone()
            v[:, lo:hi] = torch.where(ops['mask'][:, :hi - lo] > 0, v[:, lo:hi], 0.2 * v[:, lo:hi])
        return v, A
    return y_of, ops


@pytest.mark.parametrize('case', C3, ids=[_c3_id(c) for c in C3])
def test_conv3x3_f32(cuda, lib, case):
    kid, n, cin, cout, h, w, o = case
    rng = np.random.default_rng(sum(map(ord, _c3_id(case))))
    up = o.get('upsample', False)
    slope, alpha = o.get('slope', 1.0), o.get('alpha', 1.0)
    H, W = (2 * h, 2 * w) if up else (h, w)
    mode1 = o.get('mode1')
    if mode1:
        # data-gradient packing of a conv with `cout` inputs and mode1 outputs: the launch convolves dY (mode1 channels) into
        # dX (cout channels).  Output (1, 1) of dX reads dY (0, 0) through the flipped corner tap w[co][ci][2][2].
        wt = _rand(rng, (mode1, cout, 3, 3)) * 0.125
        wt[-1, :, 2, 2] = torch.from_numpy(np.where(rng.random(cout) < 0.5, -0.5, 0.5))
        bias, first_seg, seg, src_c, dst_c = None, cout, 0, mode1, cout
        k = 2 * 9 * ((mode1 + 7) // 8 * 8) + 8

        def conv(x):
            xu = F.interpolate(x, scale_factor=2, mode='nearest') if up else x
            return F.conv_transpose2d(xu, wt, padding=1), F.conv_transpose2d(xu.abs(), wt.abs(), padding=1)
    else:
        first_seg, seg = o.get('seg', (cin, 0))
        wt = _rand(rng, (cout, cin, 3, 3)) * 0.125
        wt[:, -1, 0, 0] = torch.from_numpy(np.where(rng.random(cout) < 0.5, -0.5, 0.5))
        bias = _rand(rng, (cout,)) * 0.5
        src_c, dst_c = cin, cout
        k = 2 * 9 * lib.sr_conv3x3_cin_pad(cin, first_seg, seg) + 8

        def conv(x):
            xu = F.interpolate(x, scale_factor=2, mode='nearest') if up else x
            return F.conv2d(xu, wt, bias, padding=1), F.conv2d(xu.abs(), wt.abs(), bias.abs(), padding=1)
    y_of, ops = _epilogue(rng, n, dst_c, H, W, o, slope, alpha)
    x = _rand(rng, (n, src_c, h, w))
    y0, A0 = y_of(*conv(x))
    gain = 0.5 * abs(alpha) * 0.2 * (slope if 0 < slope < 1 else 1.0)
    spike = 8 * (k * EPS * float(A0.max()) + EPS * float(y0.abs().max())) / gain + 4.0
    x = _plant(x, spike)
    y64, A = y_of(*conv(x))

    # device operands: every source and destination is a window of a wider buffer when the case asks for a slice
    in_extra, out_extra = o.get('in_slice', (0, 0)), o.get('out_slice', (0, 0))
    if mode1:
        src = x
    else:
        pos, cp = _seg_positions(cin, first_seg, seg)
        src = torch.zeros((n, cp, h, w), dtype=torch.float64)
        src[:, pos] = x
    src_blocks = (src.shape[1] + 7) // 8
    xin = _to_cb8(src, in_extra[0] + src_blocks + in_extra[1], in_extra[0], cuda)
    dst_blocks = (dst_c + 7) // 8
    out_nchw = o.get('out_nchw', False)
    if out_nchw:
        out = torch.full((n, dst_c, H, W), SENTINEL, dtype=torch.float32, device=cuda)
    else:
        base = ops.get('prior', torch.zeros((n, dst_c, H, W), dtype=torch.float64))
        out = _to_cb8(base, out_extra[0] + dst_blocks + out_extra[1], out_extra[0], cuda)
    if mode1:
        wpk, bpk = _pack3x3(lib, wt, None, mode1, cout, cout, 0, 1, cuda)
    else:
        wpk, bpk = _pack3x3(lib, wt, bias, cout, cin, first_seg, seg, 0, cuda)
    d = _lib.ConvDesc()
    d.in_, d.in_img_stride, d.cin_pad, d.in_h, d.in_w = _ptr(xin, in_extra[0]), _stride(xin), src_blocks * 8, h, w
    d.upsample = int(up)
    d.wpacked, d.bpacked, d.cout = wpk.data_ptr(), (bpk.data_ptr() if bpk is not None else None), dst_c
    if out_nchw:
        d.out, d.out_img_stride, d.out_nchw = out.data_ptr(), dst_c * H * W, 1
    else:
        d.out, d.out_img_stride = _ptr(out, out_extra[0]), _stride(out)
    d.n, d.act_slope, d.alpha = n, slope, alpha
    keep = []
    for name in ('res1', 'res2'):
        if name in ops:
            rb = _to_cb8(ops[name], dst_blocks + 1, 1, cuda)  # residuals are channel slices of a wider tensor as well
            keep.append(rb)
            setattr(d, name, _ptr(rb, 1))
            setattr(d, name + '_img_stride', _stride(rb))
            setattr(d, 'beta' + name[-1], o[name])
    d.res_cbn = o.get('res_cbn', 0)
    d.accumulate = int('prior' in ops)
    if 'mask' in ops:
        mb = _to_cb8(ops['mask'], o['mask'][1], 0, cuda)
        keep.append(mb)
        d.mask_src, d.mask_img_stride, d.mask_cb0, d.mask_cbn, d.mask_slope = mb.data_ptr(), _stride(mb), o['mask'][0], o['mask'][1], 0.2
    ids = _profiled(lib, lambda: _lib.check(lib.sr_conv3x3_f32(C.byref(d), _st()), 'sr_conv3x3_f32'))
    torch.cuda.synchronize()
    assert ids == [kid], (ids, kid)

    if out_nchw:
        got = out.cpu().double()
    else:
        got = _from_cb8(out, out_extra[0], dst_c)
        oc = out.cpu()
        assert bool((oc[:, :out_extra[0]] == SENTINEL).all()) and bool((oc[:, out_extra[0] + dst_blocks:] == SENTINEL).all()), \
            'wrote outside its channel slice'
    bound = _check(got, y64, A, k, _c3_id(case))
    y_ns, _ = y_of(*conv(_plant(x, 0.0)))
    _assert_sensitive((y64 - y_ns)[-1:], bound[-1:], _c3_id(case))


# ------------------------------------------------------------------------------------------------------ 4x4 / stride 2
def _group_couts(cout):
    cp = (cout + 31) // 32 * 32
    return 64 if cp % 64 == 0 else 32


def _ids_4x4(gc, W, passes):
    """Kernel id of each parity pass (conv_f32.hip): launch_small<2> (46: WT 16, 47: WT 8) needs 64-cout groups, W <= 16 and a
    parity sub-image of exactly the compute size (vH == H, vW == W); the generic launch<COT, 2, 2> is 6 (COT 2) or 2 (COT 1)."""
    return [(46 if W > 8 else 47) if gc == 64 and W <= 16 and vh == hh and vw == ww else (6 if gc == 64 else 2)
            for (hh, ww, vh, vw) in passes]


# (n, cin, cout, in_h, in_w, options): even and odd sizes down to 2 and 3, W = (in_w - 2) // 2 + 1 on both sides of 8, 16, 32
F4 = [
    (3, 8, 64, 2, 2, dict()),
    (3, 8, 64, 3, 3, dict(slope=0.2)),
    (2, 16, 64, 17, 17, dict(slope=0.2, alpha=0.5)),
    (2, 16, 64, 16, 18, dict()),
    (2, 16, 128, 33, 32, dict(slope=0.2)),
    (2, 24, 64, 34, 35, dict(alpha=0.2)),
    (2, 16, 32, 31, 65, dict(slope=0.0)),
    (1, 24, 64, 66, 67, dict(slope=0.2)),
    (2, 8, 96, 9, 16, dict(slope=0.2)),
    (5, 64, 64, 16, 16, dict(slope=0.2, alpha=0.5)),
]


@pytest.mark.parametrize('case', F4, ids=[f'n{c[0]}-{c[1]}to{c[2]}-{c[3]}x{c[4]}' for c in F4])
def test_conv4x4s2_f32_forward(cuda, lib, case):
    n, cin, cout, h, w, o = case
    rng = np.random.default_rng(n * 1000 + cin * 10 + h * 7 + w)
    slope, alpha = o.get('slope', 1.0), o.get('alpha', 1.0)
    wt = _rand(rng, (cout, cin, 4, 4)) * 0.125
    wt[:, -1, 1, 1] = torch.from_numpy(np.where(rng.random(cout) < 0.5, -0.5, 0.5))  # output (0, 0) reads input (0, 0) there
    bias = _rand(rng, (cout,)) * 0.5
    cin_pad = (cin + 7) // 8 * 8
    k = 2 * 16 * cin_pad + 4 + 8

    def ref(x):
        c = F.conv2d(x, wt, bias, stride=2, padding=1)
        a = F.conv2d(x.abs(), wt.abs(), bias.abs(), stride=2, padding=1)
        return torch.where(c > 0, c, slope * c) * alpha, abs(alpha) * a
    x = _rand(rng, (n, cin, h, w))
    y0, A0 = ref(x)
    gain = 0.5 * abs(alpha) * (slope if 0 < slope < 1 else 1.0)
    x = _plant(x, 8 * (k * EPS * float(A0.max()) + EPS * float(y0.abs().max())) / gain + 4.0)
    y64, A = ref(x)
    H, W = y64.shape[2:]
    wpk = torch.empty(lib.sr_conv4x4s2_packed_weight_floats(cout, cin, 0), dtype=torch.float32, device=cuda)
    bpk = torch.empty(lib.sr_conv3x3_packed_bias_floats(cout), dtype=torch.float32, device=cuda)
    wdev, bdev = wt.float().contiguous().to(cuda), bias.float().to(cuda)
    _lib.check(lib.sr_conv4x4s2_pack_f32(wdev.data_ptr(), bdev.data_ptr(), cout, cin, 0, wpk.data_ptr(), bpk.data_ptr(), _st()), 'pack')
    xin = _to_cb8(x, cin_pad // 8, 0, cuda)
    ob = (cout + 7) // 8
    out = torch.full((n, ob + 1, H, W, 8), SENTINEL, dtype=torch.float32, device=cuda)
    d = _lib.ConvDesc()
    d.in_, d.in_img_stride, d.cin_pad, d.in_h, d.in_w = xin.data_ptr(), _stride(xin), cin_pad, h, w
    d.wpacked, d.bpacked, d.cout = wpk.data_ptr(), bpk.data_ptr(), cout
    d.out, d.out_img_stride, d.n, d.act_slope, d.alpha = out.data_ptr(), _stride(out), n, slope, alpha
    ids = _profiled(lib, lambda: _lib.check(lib.sr_conv4x4s2_f32(C.byref(d), _st()), 'sr_conv4x4s2_f32'))
    torch.cuda.synchronize()
    passes = [(H, W, (h - ry + 1) // 2, (w - rx + 1) // 2) for ry in (0, 1) for rx in (0, 1)]
    assert ids == _ids_4x4(_group_couts(cout), W, passes), ids
    assert bool((out[:, ob:].cpu() == SENTINEL).all())
    bound = _check(_from_cb8(out, 0, cout), y64, A, k, case)
    y_ns, _ = ref(_plant(x, 0.0))
    _assert_sensitive((y64 - y_ns)[-1:], bound[-1:], case)


# (n, conv cin, conv cout, out_h, out_w, options): the data gradient writes dX (conv cin channels, out_h x out_w); its parity
# pass (py, px) computes a ((out_h - py + 1) / 2) x ((out_w - px + 1) / 2) sub-image from all of dY: odd sizes mix launches
D4 = [
    (3, 64, 8, 2, 2, dict()),
    (3, 64, 16, 3, 3, dict(accumulate=True)),
    (2, 64, 16, 17, 18, dict(mask=(1, 6), alpha=0.5)),
    (2, 64, 16, 33, 31, dict(accumulate=True, mask=(2, 4))),
    (2, 128, 8, 32, 34, dict()),
    (2, 32, 16, 30, 66, dict(accumulate=True)),
    (1, 64, 8, 67, 66, dict(mask=(0, 8), alpha=0.2)),
    (2, 96, 24, 15, 9, dict(accumulate=True, mask=(3, 9))),
]


@pytest.mark.parametrize('case', D4, ids=[f'n{c[0]}-{c[1]}from{c[2]}-{c[3]}x{c[4]}' for c in D4])
def test_conv4x4s2_f32_dgrad(cuda, lib, case):
    n, cin, cout, oh, ow, o = case
    rng = np.random.default_rng(n * 999 + cin + oh * 5 + ow)
    alpha = o.get('alpha', 1.0)
    h, w = (oh - 2) // 2 + 1, (ow - 2) // 2 + 1
    wt = _rand(rng, (cout, cin, 4, 4)) * 0.125
    wt[-1, :, 1, 1] = torch.from_numpy(np.where(rng.random(cin) < 0.5, -0.5, 0.5))  # dY (0, 0) reaches dX (0, 0) through it
    cpy = (cout + 7) // 8 * 8
    k = 2 * 4 * cpy + 8
    y_of, ops = _epilogue(rng, n, cin, oh, ow, o, 1.0, alpha)

    def ref(dy):
        c = torch.nn.grad.conv2d_input((n, cin, oh, ow), wt, dy, stride=2, padding=1)
        a = torch.nn.grad.conv2d_input((n, cin, oh, ow), wt.abs(), dy.abs(), stride=2, padding=1)
        return y_of(c, a)
    dy = _rand(rng, (n, cout, h, w))
    y0, A0 = ref(dy)
    dy = _plant(dy, 8 * (k * EPS * float(A0.max()) + EPS * float(y0.abs().max())) / (0.5 * abs(alpha) * 0.2) + 4.0)
    y64, A = ref(dy)
    wpk = torch.empty(lib.sr_conv4x4s2_packed_weight_floats(cout, cin, 1), dtype=torch.float32, device=cuda)
    wdev = wt.float().contiguous().to(cuda)
    _lib.check(lib.sr_conv4x4s2_pack_f32(wdev.data_ptr(), None, cout, cin, 1, wpk.data_ptr(), None, _st()), 'pack')
    din = _to_cb8(dy, cpy // 8, 0, cuda)
    cin_pad = (cin + 7) // 8 * 8
    ob = cin_pad // 8
    out = _to_cb8(ops.get('prior', torch.zeros((n, cin, oh, ow), dtype=torch.float64)), 1 + ob, 1, cuda)
    d = _lib.ConvDesc()
    d.in_, d.in_img_stride, d.cin_pad, d.in_h, d.in_w = din.data_ptr(), _stride(din), cpy, h, w
    d.wpacked, d.cout = wpk.data_ptr(), cin_pad
    d.out, d.out_img_stride, d.out_h, d.out_w = _ptr(out, 1), _stride(out), oh, ow
    d.n, d.act_slope, d.alpha, d.accumulate = n, 1.0, alpha, int('prior' in ops)
    if 'mask' in ops:
        mb = _to_cb8(ops['mask'], o['mask'][1], 0, cuda)
        d.mask_src, d.mask_img_stride, d.mask_cb0, d.mask_cbn, d.mask_slope = mb.data_ptr(), _stride(mb), o['mask'][0], o['mask'][1], 0.2
    ids = _profiled(lib, lambda: _lib.check(lib.sr_conv4x4s2_dgrad_f32(C.byref(d), _st()), 'sr_conv4x4s2_dgrad_f32'))
    torch.cuda.synchronize()
    passes = [((oh - py + 1) // 2, (ow - px + 1) // 2, h, w) for py in (0, 1) for px in (0, 1)]
    assert ids == [_ids_4x4(_group_couts(cin_pad), p[1], [p])[0] for p in passes], ids
    assert bool((out[:, :1].cpu() == SENTINEL).all())
    bound = _check(_from_cb8(out, 1, cin), y64, A, k, case)
    y_ns, _ = ref(_plant(dy, 0.0))
    _assert_sensitive((y64 - y_ns)[-1:], bound[-1:], case)


# ------------------------------------------------------------------------------------------------------ weight gradients
def _cdiv(a, b):
    return -(-a // b)


def _reduce_chain(splits, groups, gi, P, CT, ntap):
    """Serial chains of wgrad_reduce (wgrad_f32.hip): stage 1 sums `chunk` splits per block, stage 2 the `sch` chunks."""
    sch = _cdiv(splits, 64)
    cap = min((64 * 4 * 9 * 1024) // (groups * P * ntap * 1024), 4096 // ((groups // gi) * CT * 32), 64)
    sch = min(sch, cap)
    chunk = _cdiv(splits, sch)
    return chunk, _cdiv(splits, chunk)


def _wgrad_f32_plan(lib, n, H, W, cout, cin_pad, ntap):
    """The launches sr_conv3x3_wgrad_f32 / sr_conv4x4s2_wgrad_f32 (one parity pass) make, restated from run_groups and
    launch_group (wgrad_f32.hip): [(kernel id, rows_per_wg, row_splits, splits, longest fp32 chain of one dweight element)].
    A workgroup of CT x IT tiles runs KS = 4 / (CT IT) waves per pair that split each 32-pixel strip row, so one wave's
    accumulator sums rows_per_wg * 32 / KS products (two roundings each); the slab then holds splits = n * strips *
    row_splits * KS partial tiles, which stage 1 sums `chunk` at a time and stage 2 `sch` at a time; +3: scale, bias,
    accumulate."""
    slab_bytes = lib.sr_conv3x3_wgrad_slab_bytes(n, H, W)
    part = 64 * 4 * 9 * 1024 * 4 + 64 * 64 * 4 + 4096
    wslab = (slab_bytes - part) // 64 * 63 // 256 * 256
    tile_cap = wslab // (4 * 9 * 1024 * 4)
    st = n * _cdiv(W, 32)
    cts, its = _cdiv(cout, 32), _cdiv(cin_pad, 32)
    launches = []  # (CT, IT, grows, gi)

    def row_chunk(rows_left, gi, P):
        rows = max(max(tile_cap // st, 1) // gi, 1)
        rows = min(rows, max(64 * 4 // (gi * P), 1), 64)
        return min(rows, rows_left)
    r0, rows2 = 0, cts // 2
    while r0 < rows2:
        gi = its // 2
        nr = row_chunk(rows2 - r0, gi if gi > 0 else 1, 4)
        if gi > 0:
            fit = tile_cap // st
            if fit >= gi:
                launches.append((2, 2, nr, gi))
            else:
                launches += [(2, 2, 1, min(fit, gi - g0)) for g0 in range(0, gi, fit)]
        if its % 2:
            launches.append((2, 1, nr, 1))
        r0 += nr
    if cts % 2:
        i0 = 0
        if its // 4 > 0:
            launches.append((1, 4, 1, its // 4))
            i0 = its // 4 * 4
        if its - i0 >= 2:
            launches.append((1, 2, 1, 1))
            i0 += 2
        if its - i0 >= 1:
            launches.append((1, 1, 1, 1))
    plan = []
    for CT, IT, grows, gi in launches:
        groups, P = grows * gi, CT * IT
        KS = 4 // P
        rows = H
        while rows > 4 and st * _cdiv(H, rows) * groups < 512:
            rows = (rows + 1) // 2
        row_splits = _cdiv(H, rows)
        splits = st * row_splits * KS
        chunk, sch = _reduce_chain(splits, groups, gi, P, CT, ntap)
        kid = 8 + ((3 if IT == 2 else 4) if CT == 2 else (2 if IT == 4 else 1 if IT == 2 else 0))
        plan.append((kid, rows, row_splits, splits, 2 * rows * 32 // KS + chunk + sch + 3))
    return plan


def _wgrad_spike(x, dy, value):
    """Last image, last row, last column: of the last source channel and of every output-gradient channel."""
    x, dy = x.clone(), dy.clone()
    x[-1, -1, -1, -1] = value
    dy[-1, :, -1, -1] = value
    return x, dy


def _run_wgrad(lib, cuda, entry, x_cb8, cin_pad, h, w, up, dy_cb8, cout, cin, first_seg, seg, n, scale, dw, db, accumulate, H, W):
    nbytes = lib.sr_conv3x3_wgrad_slab_bytes(n, H, W)
    slab = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    d = _lib.WgradDesc()
    d.x, d.x_img_stride, d.cin_pad, d.in_h, d.in_w, d.upsample = _ptr(x_cb8, 1), _stride(x_cb8), cin_pad, h, w, int(up)
    d.dy, d.dy_img_stride = dy_cb8.data_ptr(), _stride(dy_cb8)
    d.cout, d.cin, d.first_seg, d.seg, d.n, d.scale = cout, cin, first_seg, seg, n, scale
    d.dweight, d.dbias, d.accumulate = dw.data_ptr(), (db.data_ptr() if db is not None else None), int(accumulate)
    d.slab, d.slab_bytes = slab.data_ptr(), nbytes
    ids = _profiled(lib, lambda: _lib.check(getattr(lib, entry)(C.byref(d), _st()), entry))
    torch.cuda.synchronize()
    return ids


def _wgrad_case(cuda, lib, entry, n, cin, cout, h, w, o, ks):
    rng = np.random.default_rng(n * 77 + cin * 3 + cout + h * 11 + w + ks)
    up = o.get('upsample', False)
    first_seg, seg = o.get('seg', (cin, 0))
    scale = o.get('scale', 1.0)
    want_bias = o.get('bias', True)
    accumulate = o.get('accumulate', False)
    if ks == 3:
        H, W = (2 * h, 2 * w) if up else (h, w)
        cin_pad = lib.sr_conv3x3_cin_pad(cin, first_seg, seg)
    else:
        H, W = (h - 2) // 2 + 1, (w - 2) // 2 + 1
        cin_pad = (cin + 7) // 8 * 8
    plan = _wgrad_f32_plan(lib, n, H, W, cout, cin_pad, 9 if ks == 3 else 4)
    k = max(p[4] for p in plan)
    prior_w = _rand(rng, (cout, cin, ks, ks)) if accumulate else None
    prior_b = _rand(rng, (cout,)) if accumulate else None

    def ref(x, dy):
        xu = F.interpolate(x, scale_factor=2, mode='nearest') if up else x
        stride, pad = (1, 1) if ks == 3 else (2, 1)
        g = torch.nn.grad.conv2d_weight(xu, (cout, cin, ks, ks), dy, stride=stride, padding=pad) * scale
        a = torch.nn.grad.conv2d_weight(xu.abs(), (cout, cin, ks, ks), dy.abs(), stride=stride, padding=pad) * abs(scale)
        gb, ab = dy.sum((0, 2, 3)) * scale, dy.abs().sum((0, 2, 3)) * abs(scale)
        if accumulate:
            g, a, gb, ab = g + prior_w, a + prior_w.abs(), gb + prior_b, ab + prior_b.abs()
        return g, a, gb, ab
    x, dy = _rand(rng, (n, cin, h, w)), _rand(rng, (n, cout, H, W))
    g0, a0, _, _ = ref(x, dy)
    b0 = k * EPS * float(a0[:, -1].max()) + EPS * float(g0[:, -1].abs().max())
    x, dy = _wgrad_spike(x, dy, math.sqrt(8 * b0 / abs(scale)) + 4.0)
    g64, A, gb64, Ab = ref(x, dy)

    pos, cp = _seg_positions(cin, first_seg, seg) if ks == 3 else (list(range(cin)), cin_pad)
    src = torch.zeros((n, cp, h, w), dtype=torch.float64)
    src[:, pos] = x
    x_cb8 = _to_cb8(src, 1 + cp // 8, 1, cuda)
    dy_cb8 = _to_cb8(dy, (cout + 7) // 8, 0, cuda)
    fill = float('nan')
    dw = (prior_w.float() if accumulate else torch.full((cout, cin, ks, ks), fill)).to(cuda)
    db = ((prior_b.float() if accumulate else torch.full((cout,), fill)).to(cuda)) if want_bias else None
    ids = _run_wgrad(lib, cuda, entry, x_cb8, cin_pad, h, w, up, dy_cb8, cout, cin, first_seg, seg, n, scale, dw, db, accumulate, H, W)
    assert ids == [p[0] for p in plan] * (1 if ks == 3 else 4), (ids, plan)
    bound = _check(dw.cpu().double(), g64, A, k, (entry, n, cin, cout, h, w))
    if want_bias:
        _check(db.cpu().double(), gb64, Ab, k, (entry, 'bias'))
    gns, _, _, _ = ref(*_wgrad_spike(x, dy, 0.0))
    _assert_sensitive((g64 - gns)[:, -1], bound[:, -1], (entry, n, cin, cout, h, w))
    return plan


# (n, cin, cout, h, w, options).  The last case is production-sized: 16 x 128 x 128 with 64 -> 32 channels is one 1 x 2 tile group
# (id 9, KS 2) over 64 strips, so the row halving stops at rows_per_wg 16 (64 strips x 8 row splits = 512 workgroups) and the slab
# holds 64 x 8 x 2 = 1024 splits: stage 1 sums them in chunks of 64 and stage 2 sums 16 chunks (the test asserts this plan)
W3 = [
    (2, 64, 64, 16, 16, dict()),
    (3, 56, 32, 9, 17, dict(seg=(20, 12), scale=0.5)),
    (2, 16, 64, 7, 8, dict(upsample=True, accumulate=True, bias=False)),
    (1, 24, 3, 3, 33, dict(scale=-0.25)),
    (2, 128, 64, 33, 40, dict(seg=(64, 32), accumulate=True)),
    (1, 8, 8, 1, 1, dict()),
    (9, 64, 96, 8, 8, dict(scale=0.125, accumulate=True)),
    (2, 128, 32, 9, 20, dict(scale=2.0)),
    (16, 64, 32, 128, 128, dict(scale=1.0 / 16)),
]


@pytest.mark.parametrize('case', W3, ids=[f'n{c[0]}-{c[1]}to{c[2]}-{c[3]}x{c[4]}-' + '-'.join(sorted(c[5])) for c in W3])
def test_conv3x3_wgrad_f32(cuda, lib, case):
    n, cin, cout, h, w, o = case
    plan = _wgrad_case(cuda, lib, 'sr_conv3x3_wgrad_f32', n, cin, cout, h, w, o, 3)
    if n == 16:
        assert [p[:4] for p in plan] == [(9, 16, 8, 1024)], plan


W4 = [
    (3, 8, 64, 2, 2, dict()),
    (2, 16, 32, 3, 5, dict(scale=0.5)),
    (2, 64, 64, 17, 18, dict(accumulate=True)),
    (2, 24, 128, 33, 66, dict(scale=-2.0, bias=False)),
    (4, 64, 64, 16, 16, dict(scale=0.25)),
]


@pytest.mark.parametrize('case', W4, ids=[f'n{c[0]}-{c[1]}to{c[2]}-{c[3]}x{c[4]}-' + '-'.join(sorted(c[5])) for c in W4])
def test_conv4x4s2_wgrad_f32(cuda, lib, case):
    n, cin, cout, h, w, o = case
    _wgrad_case(cuda, lib, 'sr_conv4x4s2_wgrad_f32', n, cin, cout, h, w, o, 4)


# ------------------------------------------------------------------------------------------------------ 4x4/s2 as a 3x3 conv
# A 4x4 / stride-2 / pad-1 conv of x is a 3x3 / pad-1 conv of the pixel-unshuffled u[(2 ry + rx) C + c][a][b] = x[c][2a + ry][2b + rx]:
# input row 2Y - 1 + ky is u row Y - 1 + t of parity r with (ky -> t, r) = 0 -> (0, 1), 1 -> (1, 0), 2 -> (1, 1), 3 -> (2, 0)
_K4 = {0: (0, 1), 1: (1, 0), 2: (1, 1), 3: (2, 0)}


def _w3_of(w4):
    cout, cin = w4.shape[:2]
    w3 = np.zeros((cout, 4 * cin, 3, 3), dtype=w4.dtype)
    for ky, (ty, ry) in _K4.items():
        for kx, (tx, rx) in _K4.items():
            w3[:, (2 * ry + rx) * cin:(2 * ry + rx + 1) * cin, ty, tx] = w4[:, :, ky, kx]
    return w3


def _w4_of(w3, cin):
    w4 = np.empty((w3.shape[0], cin, 4, 4), dtype=w3.dtype)
    for ky, (ty, ry) in _K4.items():
        for kx, (tx, rx) in _K4.items():
            w4[:, :, ky, kx] = w3[:, (2 * ry + rx) * cin:(2 * ry + rx + 1) * cin, ty, tx]
    return w4


@pytest.mark.parametrize('cout,cin', [(1, 1), (3, 5), (64, 64), (17, 130)])
def test_conv4x4s2_weight_as_3x3(cuda, lib, cout, cin):
    rng = np.random.default_rng(cout * 131 + cin)
    w4 = (rng.integers(-128, 128, (cout, cin, 4, 4)) / 64.0).astype(np.float32)
    w4[w4 == 0] = 0.5
    w4d = torch.from_numpy(w4).to(cuda)
    w3d = torch.full((cout, 4 * cin, 3, 3), float('nan'), dtype=torch.float32, device=cuda)
    _lib.check(lib.sr_conv4x4s2_weight_as_3x3_f32(w4d.data_ptr(), w3d.data_ptr(), cout, cin, 0, _st()), 'weight_as_3x3')
    w3 = w3d.cpu().numpy()
    want = _w3_of(w4)
    assert np.array_equal(w3.view(np.uint32), want.view(np.uint32))
    # the restatement itself: the 3x3 conv of the unshuffled input is the 4x4/s2 conv (exact: small integers and k/64 weights)
    x = torch.from_numpy(rng.integers(-4, 5, (1, cin, 6, 8)).astype(np.float64))
    u = x.reshape(1, cin, 3, 2, 4, 2).permute(0, 3, 5, 1, 2, 4).reshape(1, 4 * cin, 3, 4)
    assert torch.equal(F.conv2d(x, torch.from_numpy(w4).double(), stride=2, padding=1),
                       F.conv2d(u, torch.from_numpy(want).double(), padding=1))
    # adjoint: the fold-back of a dense 3x3 gradient reads the 16 live taps
    g3 = rng.standard_normal((cout, 4 * cin, 3, 3)).astype(np.float32)
    g3d = torch.from_numpy(g3).to(cuda)
    g4d = torch.full((cout, cin, 4, 4), float('nan'), dtype=torch.float32, device=cuda)
    _lib.check(lib.sr_conv4x4s2_weight_as_3x3_f32(g4d.data_ptr(), g3d.data_ptr(), cout, cin, 1, _st()), 'weight_as_3x3 adjoint')
    assert np.array_equal(g4d.cpu().numpy().view(np.uint32), _w4_of(g3, cin).view(np.uint32))
    assert np.array_equal(g3d.cpu().numpy(), g3)


# ------------------------------------------------------------------------------------------------------ bf16 (CB16) layout helpers
def _bf(t):
    """Rounds to bf16 (round to nearest even) and back to float64: the operands the kernel actually multiplies."""
    return t.float().bfloat16().double()


def _to_cb16(x, cuda, blocks=None):
    """NCHW (bf16-representable values) -> device CB16 buffer [n][C/16][h][w][16]; pad channels zero."""
    n, c, h, w = x.shape
    nb = (c + 15) // 16 if blocks is None else blocks
    xp = torch.zeros((n, nb * 16, h, w), dtype=torch.float32)
    xp[:, :c] = x
    return xp.reshape(n, nb, 16, h, w).permute(0, 1, 3, 4, 2).contiguous().bfloat16().to(cuda)


def _from_cb16(buf, c):
    n, nb, h, w, _ = buf.shape
    return buf.cpu().double().permute(0, 1, 4, 2, 3).reshape(n, nb * 16, h, w)[:, :c]


def _unshuffle(x):
    """[n][C][2h][2w] -> [n][4C][h][w], channel (2 ry + rx) C + c (sr_cb16_unshuffle2_bf16, out_unshuffle2)."""
    n, c, hh, ww = x.shape
    return x.reshape(n, c, hh // 2, 2, ww // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(n, 4 * c, hh // 2, ww // 2)


def _shuffle(u):
    n, c4, h, w = u.shape
    return u.reshape(n, 2, 2, c4 // 4, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c4 // 4, 2 * h, 2 * w)


def _bf16_bound(A, y64, k, out_bf16):
    b = k * EPS * A + EPS * y64.abs()
    return b + 2.0 ** -8 * (y64.abs() + b) + TINY if out_bf16 else b + TINY


# ------------------------------------------------------------------------------------------------------ sr_conv3x3_bf16
# (id, n, cin, cout, h, w, options).  sr_conv3x3_bf16 (conv_bf16.hip) picks, with wgs(rows) = ceil(W / 32) ceil(H / rows) n groups:
#   R16_W8 (8 waves, PT 2: id 24 / 26 for 32- / 64-cout groups) when H % 16 == 0, cin <= 256 and wgs(16) >= 256;
#   R32_W8 (8 waves, PT 4: 25 / 27) when H % 32 == 0 and wgs(32) >= 256 (here: cin > 256);
#   R16_W4 (PT 4: 17 / 19) when H % 16 == 0 and wgs(16) >= 256 (cin > 256, H % 32 != 0);
#   R8_W4 (PT 2: 16 / 18) when wgs(8) >= 256 or H <= 4;  R4_W4 (PT 1: 42 / 43) otherwise.
# NCHW output: cout <= 4 without residual or mask -> the few-cout kernel (50); otherwise 8 waves PT 4 when H % 32 == 0 (29 / 31)
# and 4 waves PT 2 if not (20 / 22) — ids 21, 23, 28 and 30 (NCHW on the other tile shapes) are not instantiated by the dispatch.
# The streaming kernel (64) takes cout 64, cin <= 64 and H % 16 == 0 on >= 24 tiles of 16 x 32 per CU: 48 images of 256 x 256
# are 6144 tiles, 24 per CU of the MI355X's 256.  res1_u2 and res1_keep_sign need a plain destination of even size.  s2 marks a 4x4/s2 conv on the pixel-unshuffled operand (weights: sr_conv4x4s2_weight_as_3x3_f32,
# restated by _w3_of), on the input side (forward) or the output side (data gradient; mode-1 packing).
B3 = [
    (24, 32, 64, 32, 16, 256, dict(slope=0.2)),
    (26, 32, 64, 64, 16, 256, dict(slope=0.2, res1=0.2)),
    (25, 64, 288, 32, 32, 128, dict(alpha=0.5)),
    (27, 64, 288, 64, 32, 128, dict(slope=0.2, res2=1.0)),
    (17, 86, 288, 32, 48, 32, dict(slope=0.0)),
    (19, 86, 288, 64, 48, 32, dict(res1=1.0, res2=0.5)),
    (16, 2, 32, 32, 3, 33, dict(slope=0.0)),
    (18, 2, 48, 64, 2, 40, dict(res1=0.2, slope=0.2)),
    (42, 2, 32, 32, 9, 17, dict(slope=0.2, alpha=0.2)),
    (43, 2, 32, 64, 7, 9, dict(upsample=True, slope=0.2)),
    (50, 2, 64, 3, 17, 33, dict(nchw=True, slope=0.2)),
    (20, 2, 32, 8, 9, 17, dict(nchw=True)),
    (29, 2, 32, 8, 32, 40, dict(nchw=True, slope=0.2)),
    (22, 2, 32, 64, 7, 9, dict(nchw=True)),
    (31, 1, 32, 64, 32, 33, dict(nchw=True, alpha=0.5)),
    (64, 48, 16, 64, 256, 256, dict(slope=0.2, alpha=0.7)),
    (18, 2, 256, 64, 4, 4, dict(s2='fwd', slope=0.2)),
    (18, 2, 256, 64, 4, 4, dict(s2='bwd')),
    (26, 128, 256, 64, 16, 64, dict(s2='fwd', slope=0.2)),
    (18, 2, 32, 64, 4, 6, dict(u2=True, slope=0.2)),
    (43, 2, 32, 64, 10, 12, dict(res1=1.0, res1_u2=True, slope=0.2)),
    (43, 2, 32, 64, 10, 18, dict(keep_sign=True, slope=0.2)),
    (16, 2, 32, 32, 4, 34, dict(keep_sign=True, slope=0.2, alpha=0.5)),
]


def _b3_id(c):
    i, n, cin, cout, h, w, o = c
    return f'k{i}-n{n}-{cin}to{cout}-{h}x{w}-' + '-'.join(f'{k}' if v is True else f'{k}{v}' for k, v in sorted(o.items()))


@pytest.mark.parametrize('case', B3, ids=[_b3_id(c) for c in B3])
def test_conv3x3_bf16(cuda, lib, case):
    kid, n, cin, cout, h, w, o = case
    from image_restoration_amd import hip_ops as HO
    rng = np.random.default_rng(sum(map(ord, _b3_id(case))))
    up, s2 = o.get('upsample', False), o.get('s2')
    slope, alpha = o.get('slope', 1.0), o.get('alpha', 1.0)
    H, W = (2 * h, 2 * w) if up else (h, w)
    imgs = sorted({0, n - 1})  # images are independent: the float64 reference covers the first and the last
    sign = lambda m: torch.from_numpy(np.where(rng.random(m) < 0.5, -0.5, 0.5))  # noqa: E731
    bias = _bf(_rand(rng, (cout,)) * 0.5) if s2 != 'bwd' else None
    if s2:
        C = cin // 4
        if s2 == 'fwd':
            # a 4x4/s2 conv of X [n][C][2h][2w]; the kernel reads X pixel-unshuffled.  X (1, 1) of the last channel is the last
            # unshuffled channel (parity 3) and reaches output (0, 0) through tap (2, 2)
            w4 = _bf(_rand(rng, (cout, C, 4, 4)) * 0.125)
            w4[:, -1, 2, 2] = sign(cout)
            wt = torch.from_numpy(_w3_of(w4.numpy()))
            X = _bf(_rand(rng, (n, C, 2 * h, 2 * w))).float()

            def conv(X):
                return (F.conv2d(X[imgs].double(), w4, bias, stride=2, padding=1),
                        F.conv2d(X[imgs].double().abs(), w4.abs(), bias.abs(), stride=2, padding=1))

            def plant(X, v):
                X = X.clone()
                X[-1, -1, 1, 1] = v
                return X
            src_of = _unshuffle
            dst_c, k = cout, 2 * 9 * cin + 8
        else:
            # the data gradient of a 4x4/s2 conv with C inputs and cout outputs, written pixel-unshuffled (4C channels)
            w4 = _bf(_rand(rng, (cout, C, 4, 4)) * 0.125)
            w4[-1, :, 1, 1] = sign(C)
            wt = torch.from_numpy(_w3_of(w4.numpy()))
            X = _bf(_rand(rng, (n, cout, h, w))).float()

            def conv(dY):
                shp = (len(imgs), C, 2 * h, 2 * w)
                dY = dY[imgs].double()
                return (_unshuffle(torch.nn.grad.conv2d_input(shp, w4, dY, stride=2, padding=1)),
                        _unshuffle(torch.nn.grad.conv2d_input(shp, w4.abs(), dY.abs(), stride=2, padding=1)))
            plant = _plant
            src_of = lambda x: x  # noqa: E731
            dst_c, k = cin, 2 * 9 * ((cout + 15) // 16 * 16) + 8
    else:
        wt = _bf(_rand(rng, (cout, cin, 3, 3)) * 0.125)
        wt[:, -1, 0, 0] = sign(cout)
        X = _bf(torch.from_numpy(rng.standard_normal((n, cin, h, w), dtype=np.float32))).float()

        def conv(x):
            x = x[imgs].double()
            xu = F.interpolate(x, scale_factor=2, mode='nearest') if up else x
            return F.conv2d(xu, wt, bias, padding=1), F.conv2d(xu.abs(), wt.abs(), bias.abs(), padding=1)
        plant, src_of = _plant, (lambda x: x)
        dst_c, k = cout, 2 * 9 * ((cin + 15) // 16 * 16) + 8
    ops = {}
    if o.get('keep_sign'):
        o = dict(o, res1=1.0)
    for name in ('res1', 'res2'):
        if name in o:
            scale = 16.0 if o.get('keep_sign') else 1.0  # keep_sign: large residuals, so conv + res1 often rounds back to res1
            ops[name] = _bf(torch.from_numpy(rng.standard_normal((n, dst_c, H, W), dtype=np.float32)) * scale).float()

    def y_of(c, a):
        v = torch.where(c > 0, c, slope * c) * alpha
        A = abs(alpha) * a
        for name in ('res1', 'res2'):
            if name in ops:
                r = ops[name][imgs].double()
                v = v + o[name] * r
                A = A + abs(o[name]) * r.abs()
        return v, A
    c0, a0 = conv(X)
    y0, A0 = y_of(c0, a0)
    out_bf16 = not o.get('nchw')
    gain = 0.5 * abs(alpha) * (slope if 0 < slope < 1 else 1.0)
    spike = float(_bf(torch.tensor(8 * float(_bf16_bound(A0, y0, k, out_bf16).max()) / gain + 4.0)))
    X = plant(X, spike)
    c, a = conv(X)
    y64, A = y_of(c, a)

    # device operands
    src = HO.CB16(_to_cb16(src_of(X), cuda))
    pc = HO.PackedConvBF16(wt.float().to(cuda), bias.float().to(cuda) if bias is not None else None,
                           mode=1 if s2 == 'bwd' else 0)
    kw = dict(upsample=up, act_slope=slope, alpha=alpha)
    if s2:
        kw.update(s2_channels=C, s2_side=1 if s2 == 'bwd' else 0)
    for name in ('res1', 'res2'):
        if name in ops:
            r = ops[name]
            kw[name] = HO.CB16(_to_cb16(_unshuffle(r) if (name == 'res1' and o.get('res1_u2')) else r, cuda))
            kw['beta' + name[-1]] = o[name]
    if o.get('res1_u2'):
        kw['res1_u2'] = True
    if o.get('keep_sign'):
        kw['res1_keep_sign'] = True
    out = None
    if o.get('nchw'):
        kw['out_nchw'] = torch.full((n, dst_c, H, W), SENTINEL, dtype=torch.float32, device=cuda)
    elif o.get('u2'):
        kw['out_unshuffle2'] = True
    else:
        out = HO.CB16(torch.full((n, (dst_c + 15) // 16, H, W, 16), SENTINEL, dtype=torch.bfloat16, device=cuda))
    res = {}
    ids = _profiled(lib, lambda: res.setdefault('out', HO.conv3x3_bf16(src, pc, out, **kw)))
    torch.cuda.synchronize()
    assert ids == [kid], (ids, kid)
    ret = res['out']
    if o.get('nchw'):
        got = ret.cpu().double()
    elif o.get('u2'):
        got = _shuffle(_from_cb16(ret.buf, 4 * dst_c))
    else:
        got = _from_cb16(ret.buf, dst_c)
    got = got[imgs]
    bound = _bf16_bound(A, y64, k, out_bf16)
    err = (got - y64).abs()
    if o.get('keep_sign'):
        # <= 1 bf16 ulp more than the rounding (the step to the next bf16 above res1), and the sign of the activation survives
        ulp = torch.exp2(torch.floor(torch.log2(got.abs().clamp_min(2.0 ** -126))) - 7)
        assert bool((err <= bound + ulp).all()), (_b3_id(case), float(((err - ulp) / bound).max()))
        r1 = ops['res1'][imgs].double()
        pre_pos = c > (k * EPS * a + EPS * c.abs())
        assert bool(pre_pos.any())
        assert bool(((got - r1)[pre_pos] > 0).all()), (_b3_id(case), 'sign(out - res1) lost where conv + bias > 0')
    else:
        bad = err > bound
        assert not bool(bad.any()), (_b3_id(case), int(bad.sum()), float((err / bound).max()))
    y_ns, _ = y_of(*conv(plant(X, 0.0)))
    _assert_sensitive((y64 - y_ns)[-1:], bound[-1:], _b3_id(case))


# ------------------------------------------------------------------------------------------------------ bf16 weight gradients
_WG_BF16 = {  # (CT, IT) -> (KS, R, kernel id) of the launch_group<CT, IT, KS, R, NSTG> instances (wgrad_bf16.hip)
    (2, 4): (1, 1, 37), (2, 2): (2, 2, 36), (2, 1): (4, 2, 35), (1, 5): (1, 1, 39), (1, 4): (2, 1, 34), (1, 3): (2, 1, 38),
    (1, 2): (4, 2, 33), (1, 1): (8, 2, 32)}


def _wgrad_bf16_plan(n, H, W, cout, cin_pad):
    """The launches of sr_conv3x3_wgrad_bf16, restated from its host code for layers of <= 3 cout tiles (one launch row):
    [(kernel id, imgs_per_wg, rows_per_wg, splits, longest fp32 chain)].  2 x 4 groups first when cin spans >= 4 tiles of a
    two-tile cout row, then 2 x 2 / 2 x 1 for the rest of the row; a single cout tile walks cin in 5 (conv4 of a dense block: left
    == 5 or >= 9), 4, 3, 2, 1 tiles."""
    cts, its = _cdiv(cout, 32), _cdiv(cin_pad, 32)
    assert cts <= 3
    launches = []
    c0 = 0
    while c0 < cts:
        cn = 2 if cts - c0 >= 2 else 1
        i0 = 0
        if cn == 2 and its >= 4 and its // 4 <= 32:
            launches.append((2, 4, 1, its // 4))
            i0 = its // 4 * 4
        while i0 < its:
            left = its - i0
            if cn == 2:
                it = 2 if left >= 2 else 1
            else:
                it = 5 if (left == 5 or left >= 9) else 4 if left >= 4 else left
            launches.append((cn, it, 1, 1))
            i0 += it
        c0 += cn
    nseg = 1 if W <= 16 else 2 if W <= 32 else 4
    m = _cdiv(28000, H * nseg * 288 + 2000)
    ipw_min = 1 if m < 3 else min(m, n)
    strips = _cdiv(W, 64)
    plan = []
    for CT, IT, grows, gi in launches:
        KS, R, kid = _WG_BF16[(CT, IT)]
        groups, P = grows * gi, CT * IT
        ipw = min(max(n * strips * groups // 256, ipw_min), n)
        st = _cdiv(n, ipw) * strips
        want = 1 if ipw_min > 1 else max(256 // (st * groups), 1)
        rows = _cdiv(_cdiv(H, want), R) * R
        splits = st * _cdiv(H, rows)
        chunk, sch = _reduce_chain(splits, groups, gi, P, CT, 9)
        plan.append((kid, ipw, rows, splits, 2 * ipw * rows * 64 // KS + KS + chunk + sch + 3))
    return plan


# (n, cin, cout, h, w, options): every instance, at W <= 16, <= 32 and wider (the NSEG = 1 / 2 / 4 forms of each)
WB = [
    (2, 128, 64, 8, 16, dict()),
    (2, 96, 64, 9, 32, dict(scale=0.5)),
    (2, 160, 32, 7, 40, dict(seg=(64, 32))),
    (1, 128, 32, 16, 70, dict()),
    (2, 96, 32, 5, 12, dict(bias=False)),
    (2, 64, 32, 12, 20, dict(accumulate=True)),
    (3, 32, 32, 3, 3, dict()),
    (2, 192, 96, 8, 24, dict(scale=-0.25)),
    (1, 320, 32, 6, 66, dict()),
    (2, 64, 64, 6, 8, dict(upsample=True, accumulate=True, bias=False)),
    (9, 64, 32, 8, 8, dict()),
]


@pytest.mark.parametrize('case', WB, ids=[f'n{c[0]}-{c[1]}to{c[2]}-{c[3]}x{c[4]}-' + '-'.join(sorted(c[5])) for c in WB])
def test_conv3x3_wgrad_bf16(cuda, lib, case):
    n, cin, cout, h, w, o = case
    rng = np.random.default_rng(n * 31 + cin + cout * 7 + h * 3 + w)
    up = o.get('upsample', False)
    first_seg, seg = o.get('seg', (cin, 0))
    scale, want_bias, accumulate = o.get('scale', 1.0), o.get('bias', True), o.get('accumulate', False)
    H, W = (2 * h, 2 * w) if up else (h, w)
    cin_pad = lib.sr_conv3x3_cin_pad16(cin, first_seg, seg)
    plan = _wgrad_bf16_plan(n, H, W, cout, cin_pad)
    k = max(p[4] for p in plan)
    prior_w = _rand(rng, (cout, cin, 3, 3)) if accumulate else None
    prior_b = _rand(rng, (cout,)) if accumulate else None

    def ref(x, dy):
        xu = F.interpolate(x, scale_factor=2, mode='nearest') if up else x
        g = torch.nn.grad.conv2d_weight(xu, (cout, cin, 3, 3), dy, padding=1) * scale
        a = torch.nn.grad.conv2d_weight(xu.abs(), (cout, cin, 3, 3), dy.abs(), padding=1) * abs(scale)
        gb, ab = dy.sum((0, 2, 3)) * scale, dy.abs().sum((0, 2, 3)) * abs(scale)
        if accumulate:
            g, a, gb, ab = g + prior_w, a + prior_w.abs(), gb + prior_b, ab + prior_b.abs()
        return g, a, gb, ab
    x, dy = _bf(_rand(rng, (n, cin, h, w))), _bf(_rand(rng, (n, cout, H, W)))
    g0, a0, _, _ = ref(x, dy)
    b0 = k * EPS * float(a0[:, -1].max()) + EPS * float(g0[:, -1].abs().max())
    x, dy = _wgrad_spike(x, dy, float(_bf(torch.tensor(math.sqrt(8 * b0 / abs(scale)) + 4.0))))
    g64, A, gb64, Ab = ref(x, dy)
    pos, cp = _seg_positions(cin, first_seg, seg, 16)
    src = torch.zeros((n, cp, h, w), dtype=torch.float64)
    src[:, pos] = x
    xb, dyb = _to_cb16(src, cuda), _to_cb16(dy, cuda)
    dw = (prior_w.float() if accumulate else torch.full((cout, cin, 3, 3), float('nan'))).to(cuda)
    db = ((prior_b.float() if accumulate else torch.full((cout,), float('nan'))).to(cuda)) if want_bias else None
    nbytes = lib.sr_conv3x3_wgrad_slab_bytes_bf16(n, H, W)
    slab = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    d = _lib.WgradDesc()
    d.x, d.x_img_stride, d.cin_pad, d.in_h, d.in_w, d.upsample = xb.data_ptr(), cp * h * w, cin_pad, h, w, int(up)
    d.dy, d.dy_img_stride = dyb.data_ptr(), dyb.shape[1] * H * W * 16
    d.cout, d.cin, d.first_seg, d.seg, d.n, d.scale = cout, cin, first_seg, seg, n, scale
    d.dweight, d.dbias, d.accumulate = dw.data_ptr(), (db.data_ptr() if db is not None else None), int(accumulate)
    d.slab, d.slab_bytes = slab.data_ptr(), nbytes
    ids = _profiled(lib, lambda: _lib.check(lib.sr_conv3x3_wgrad_bf16(C.byref(d), _st()), 'sr_conv3x3_wgrad_bf16'))
    torch.cuda.synchronize()
    assert ids == [p[0] for p in plan], (ids, plan)
    bound = _check(dw.cpu().double(), g64, A, k, ('wgrad_bf16', case))
    if want_bias:
        _check(db.cpu().double(), gb64, Ab, k, ('wgrad_bf16 bias', case))
    gns, _, _, _ = ref(*_wgrad_spike(x, dy, 0.0))
    _assert_sensitive((g64 - gns)[:, -1], bound[:, -1], ('wgrad_bf16', case))


@pytest.mark.parametrize('accumulate', [0, 1])
def test_rdb_wgrad_bf16(cuda, lib, accumulate):
    """The five weight gradients of a dense block in one launch (id 40) against float64: cat = [x | x1..x4] (CB16), D = [dY5 |
    dY4 | dY3 | dY2 | dY1] in one buffer of the same image stride; conv5's gradient is scaled by scale5."""
    n, h, w, nf, gc, scale5 = 2, 16, 16, 64, 32, 0.25
    rng = np.random.default_rng(40 + accumulate)
    ch = nf + 4 * gc
    cat, D = _bf(_rand(rng, (n, ch, h, w))), _bf(_rand(rng, (n, ch, h, w)))
    k = 2 * n * h * w + 3  # order-independent: at most n h w products per element (see the module docstring)
    couts = {k_: (nf if k_ == 5 else gc) for k_ in range(1, 6)}
    dy_at = {5: 0, 4: nf, 3: nf + gc, 2: nf + 2 * gc, 1: nf + 3 * gc}
    priors = {k_: (_rand(rng, (couts[k_], nf + (k_ - 1) * gc, 3, 3)), _rand(rng, (couts[k_],))) for k_ in range(1, 6)}

    def ref(cat, D):
        out = {}
        for k_ in range(1, 6):
            x = cat[:, :nf + (k_ - 1) * gc]
            dy = D[:, dy_at[k_]:dy_at[k_] + couts[k_]]
            s = scale5 if k_ == 5 else 1.0
            g = torch.nn.grad.conv2d_weight(x, (couts[k_], x.shape[1], 3, 3), dy, padding=1) * s
            a = torch.nn.grad.conv2d_weight(x.abs(), (couts[k_], x.shape[1], 3, 3), dy.abs(), padding=1) * s
            gb, ab = dy.sum((0, 2, 3)) * s, dy.abs().sum((0, 2, 3)) * s
            if accumulate:
                g, a, gb, ab = g + priors[k_][0], a + priors[k_][0].abs(), gb + priors[k_][1], ab + priors[k_][1].abs()
            out[k_] = (g, a, gb, ab)
        return out
    r0 = ref(cat, D)
    b0 = k * EPS * float(r0[5][1][:, -1].max()) + EPS * float(r0[5][0][:, -1].abs().max())
    spike = float(_bf(torch.tensor(math.sqrt(8 * b0 / scale5) + 4.0)))

    def plant(cat, D, v):
        cat, D = cat.clone(), D.clone()
        cat[-1, -1, -1, -1] = v  # the last channel of x4: read by conv5 only
        D[-1, :nf, -1, -1] = v
        return cat, D
    cat, D = plant(cat, D, spike)
    r = ref(cat, D)
    catd, Dd = _to_cb16(cat, cuda), _to_cb16(D, cuda)
    dws, keep = (C.c_void_p * 10)(), []
    for k_ in range(1, 6):
        cin_k = nf + (k_ - 1) * gc
        wgt = (priors[k_][0].float() if accumulate else torch.full((couts[k_], cin_k, 3, 3), float('nan'))).to(cuda)
        bgt = (priors[k_][1].float() if accumulate else torch.full((couts[k_],), float('nan'))).to(cuda)
        keep.append((wgt, bgt))
        dws[2 * (k_ - 1)], dws[2 * (k_ - 1) + 1] = wgt.data_ptr(), bgt.data_ptr()
    nbytes = lib.sr_rdb_wgrad_slab_bytes_bf16(n, h, w, nf, gc)
    slab = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    ids = _profiled(lib, lambda: _lib.check(lib.sr_rdb_wgrad_bf16(catd.data_ptr(), Dd.data_ptr(), ch * h * w, n, h, w, nf, gc, dws,
                                                                  scale5, accumulate, slab.data_ptr(), nbytes, _st()), 'sr_rdb_wgrad_bf16'))
    torch.cuda.synchronize()
    assert ids == [40], ids
    for k_ in range(1, 6):
        g, a, gb, ab = r[k_]
        bound = _check(keep[k_ - 1][0].cpu().double(), g, a, k, ('rdb', k_))
        _check(keep[k_ - 1][1].cpu().double(), gb, ab, k, ('rdb bias', k_))
        if k_ == 5:
            gns = ref(*plant(cat, D, 0.0))[5][0]
            _assert_sensitive((g - gns)[:, -1], bound[:, -1], 'rdb conv5')


BF16_CONV_IDS = {16, 17, 18, 19, 24, 25, 26, 27, 20, 22, 29, 31, 42, 43, 50, 64}
WGRAD_IDS = {8, 9, 10, 11, 12} | set(range(32, 41))


def test_dispatch_coverage(request):
    """Every default instance of every convolution entry point was launched by the cases above.  SEEN is filled by the other
    tests of this module, so the check needs the whole module: under a selection (-k, a single test) it is skipped."""
    whole = len(C3) + len(F4) + len(D4) + len(W3) + len(W4) + 4 + len(B3) + len(WB) + 2
    ran = sum(1 for it in request.session.items if it.module is request.module and it.name != 'test_dispatch_coverage')
    if ran < whole:
        pytest.skip(f'needs the whole module ({ran} of {whole} cases selected)')
    missing = (F32_3X3_IDS | F32_4X4_IDS | BF16_CONV_IDS | WGRAD_IDS) - SEEN
    assert not missing, sorted(missing)
