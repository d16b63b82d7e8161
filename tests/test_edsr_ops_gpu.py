"""The entry points of include/sr_hip_edsr.h on the MI355X: the CB16 pixel shuffle (a pure permutation: bit equality against
F.pixel_shuffle, with a negative control) and the two image shifts against float64."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from image_restoration_amd import _lib, hip_ops

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24    # unit roundoff of fp32
UBF = 2.0 ** -8     # unit roundoff of bf16 (8 significand bits: spacing 2^-7 relative, half of it)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _profiled(lib, fn, cap=64):
    _lib.check(lib.sr_profile_start(cap), 'sr_profile_start')
    try:
        fn()
    finally:
        recs = (_lib.LaunchRecord * cap)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, cap, C.byref(cnt)), 'sr_profile_stop')
    return [(recs[i].kernel_id, recs[i].bytes) for i in range(min(cnt.value, cap))]


def _to_cb16(x, slack=0):
    """NCHW bf16 (CPU) -> CB16 storage [n][blocks + slack][h][w][16] on the CPU: zero pad channels, NaN in the slack blocks that
    make the image stride non-dense."""
    n, c, h, w = x.shape
    cb = (c + 15) // 16
    buf = torch.full((n, cb + slack, h, w, 16), float('nan'), dtype=torch.bfloat16)
    pad = torch.zeros(n, cb * 16, h, w, dtype=torch.bfloat16)
    pad[:, :c] = x
    buf[:, :cb] = pad.view(n, cb, 16, h, w).permute(0, 1, 3, 4, 2)
    return buf


def _from_cb16(buf, cb):
    n, _, h, w, _ = buf.shape
    return buf[:, :cb].permute(0, 1, 4, 2, 3).reshape(n, cb * 16, h, w)


# (c, n, h, w): one and several channel blocks, c % 16 != 0 (pad channels in the last block), ragged sizes, rows longer than one
# 64-pixel tile (w = 70, 131) and exactly one tile (64)
SHUFFLE_CASES = [(16, 2, 1, 1), (16, 2, 7, 5), (32, 3, 9, 13), (64, 2, 5, 70), (256, 2, 3, 64), (8, 2, 4, 3), (40, 2, 6, 131)]


@pytest.mark.parametrize('r', [2, 3])
@pytest.mark.parametrize('slack', [0, 1])
@pytest.mark.parametrize('c,n,h,w', SHUFFLE_CASES)
def test_cb16_pixel_shuffle_is_a_bit_exact_permutation(cuda, r, slack, c, n, h, w):
    """Bit for bit against F.pixel_shuffle on bf16 data.  The destination starts as NaN: every value of the image, pad channels
    included, is written (pads 0); with slack, both image strides are larger than the images and the NaN between the images
    stays NaN on both sides.  The negative control swaps one channel pair of the expected tensor and must not compare equal."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(1000 * r + c + w)
    x = torch.randn(n, c * r * r, h, w, generator=g).bfloat16()
    want = F.pixel_shuffle(x.float(), r).bfloat16()
    src = _to_cb16(x, slack).to(cuda)
    cbd = (c + 15) // 16
    dst = torch.full((n, cbd + slack, h * r, w * r, 16), float('nan'), dtype=torch.bfloat16, device=cuda)
    src_before = src.clone()
    ids = _profiled(lib, lambda: _lib.check(lib.sr_cb16_pixel_shuffle_bf16(
        src.data_ptr(), src[0].numel(), dst.data_ptr(), dst[0].numel(), n, c, h, w, r, _st()), 'sr_cb16_pixel_shuffle_bf16'))
    assert [i for i, _ in ids] == [98]
    assert ids[0][1] == 32.0 * n * h * w * ((c * r * r + 15) // 16 + r * r * cbd)
    got = _from_cb16(dst.cpu(), cbd)
    assert torch.equal(got[:, :c].view(torch.int16), want.view(torch.int16))
    assert torch.count_nonzero(got[:, c:]) == 0 and not torch.isnan(got).any()
    if slack:
        assert torch.isnan(dst[:, cbd:]).all()
    assert torch.equal(src.view(torch.int16), src_before.view(torch.int16))     # the source is only read
    # negative control
    if c >= 2:
        bad = want.clone()
        bad[:, [0, 1]] = bad[:, [1, 0]]
        assert not torch.equal(got[:, :c].view(torch.int16), bad.view(torch.int16))
    # through the wrapper (dense strides)
    if not slack:
        out = hip_ops.pixel_shuffle_bf16(hip_ops.CB16(src), c, r)
        assert torch.equal(out.buf.view(torch.int16), dst.view(torch.int16))


def test_cb16_pixel_shuffle_rejects_bad_arguments(cuda):
    lib = _lib.load()
    a = hip_ops.CB16.zeros(1, 64, 4, 4, cuda)
    b = hip_ops.CB16.zeros(1, 16, 8, 8, cuda)
    ok = (a.ptr, a.img_stride, b.ptr, b.img_stride, 1, 16, 4, 4, 2, _st())
    assert lib.sr_cb16_pixel_shuffle_bf16(*ok) == 0
    for i, v in ((8, 4), (8, 1), (4, 0), (5, 0), (6, 0), (7, 0), (0, None), (2, None), (1, a.img_stride - 8), (3, b.img_stride - 8),
                 (0, a.ptr + 2), (2, b.ptr + 8), (1, a.img_stride + 4), (6, 65536)):
        args = list(ok)
        args[i] = v
        assert lib.sr_cb16_pixel_shuffle_bf16(*args) == -1, (i, v)
        assert b'sr_cb16_pixel_shuffle_bf16' in lib.sr_last_error()
    torch.cuda.synchronize()


SHIFT_CASES = [(1, 1, 1), (2, 5, 13), (3, 70, 97), (2, 128, 128)]
MEANS = [((0.4488, 0.4371, 0.4040), 255.0), ((0.5, 0.25, 0.125), 1.0), ((0.0, -0.3, 1.5), 0.37)]


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('n,h,w', SHIFT_CASES)
@pytest.mark.parametrize('mean,rng', MEANS)
def test_shift_in_matches_float64(cuda, bf16, n, h, w, mean, rng):
    """(x - mean) * range in fp32: two roundings, |err| <= 2u |result| (+ the conversion of mean to fp32, u |mean| range); the
    bf16 form adds one rounding to nearest of the fp32 value (2^-8 relative).  Pad channels are exact zeros; the destination
    starts as NaN, so every element was written."""
    lib = _lib.load()
    x = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(h * w + n))
    m64 = torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)
    want = (x.double() - m64) * rng
    xd = x.to(cuda)
    ids = _profiled(lib, lambda: hip_ops.edsr_shift_in(xd, mean, rng, bf16=bf16))
    assert [i for i, _ in ids] == [99]
    out = hip_ops.edsr_shift_in(xd, mean, rng, bf16=bf16)
    buf = out.buf.cpu()
    assert tuple(buf.shape) == (n, 1, h, w, 16 if bf16 else 8)
    got = buf[:, 0].permute(0, 3, 1, 2).double()
    assert torch.count_nonzero(got[:, 3:]) == 0 and not torch.isnan(got).any()
    bound = 2 * U32 * want.abs() + U32 * m64.abs() * abs(rng)
    if bf16:
        bound = bound + UBF * want.abs() * (1 + 4 * U32)
    assert bool(((got[:, :3] - want).abs() <= bound).all()), float(((got[:, :3] - want).abs() - bound).max())
    if not bf16:   # the reference's own fp32 expression, bit for bit
        ref32 = (x - torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)) * rng
        assert torch.equal(got[:, :3].float(), ref32)


@pytest.mark.parametrize('n,h,w', SHIFT_CASES)
@pytest.mark.parametrize('mean,rng', MEANS)
def test_shift_out_matches_float64(cuda, n, h, w, mean, rng):
    """y / range + mean in fp32, in place: a correctly rounded division and one addition, |err| <= u |y / range| + u |result|
    (+ u |mean| for the conversion of mean); equal to torch's fp32 expression bit for bit."""
    lib = _lib.load()
    y = (torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(h + w)) * 100)
    m64 = torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)
    want = y.double() / rng + m64
    yd = y.to(cuda)
    ids = _profiled(lib, lambda: hip_ops.edsr_shift_out(yd, mean, rng))
    assert [i for i, _ in ids] == [100]
    got = yd.cpu()
    bound = U32 * (y.double() / rng).abs() + U32 * want.abs() + U32 * m64.abs()
    assert bool(((got.double() - want).abs() <= bound).all())
    assert torch.equal(got, y / rng + torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1))
