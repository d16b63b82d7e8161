"""Restatements of the five degradation stages of include/sr_hip_degrade.h in plain torch / numpy, the yardstick of
tests/test_degrade_ops_gpu.py and tests/test_degrade_pipeline_gpu.py.  They compute in the dtype of their input (float64 for the
yardstick, float32 to measure what fp32 arithmetic alone costs) and are themselves checked against the reference's recorded
outputs in tests/test_degrade_host.py (tests/golden/g_zc_degrade.npz).
"""
import math

import numpy as np
import torch
from torch.nn import functional as F


# ---------------------------------------------------------------------------------------------------------------- filter2d
def filter2d(x, kernels):
    """Correlation with reflect border; kernels [1 or B, k, k]."""
    b, c, h, w = x.shape
    k = kernels.size(-1)
    xp = F.pad(x, (k // 2,) * 4, mode='reflect') if k > 1 else x
    kb = kernels.expand(b, k, k) if kernels.size(0) == 1 else kernels
    wgt = kb.reshape(b, 1, k, k).repeat_interleave(c, dim=0)
    return F.conv2d(xp.reshape(1, b * c, h + k - 1, w + k - 1), wgt, groups=b * c).reshape(b, c, h, w)


def filter2d_abs(x, kernels):
    """sum |kernel * x| per output pixel: the scale of the rounding bound."""
    return filter2d(x.abs(), kernels.abs())


# ------------------------------------------------------------------------------------------------------------------ resize
def source_coords(src_len, dst_len):
    """(i0, i1, f) per destination index, the coordinate arithmetic in float32 exactly as the header states it."""
    f32 = np.float32
    scale = f32(src_len) / f32(dst_len)
    d = np.arange(dst_len, dtype=np.float32)
    s = (d + f32(0.5)) * scale - f32(0.5)
    fl = np.floor(s)
    i0 = fl.astype(np.int64)
    f = (s - fl).astype(np.float32)
    neg = s < 0
    i0[neg], f[neg] = 0, 0
    top = i0 >= src_len - 1
    i0[top], f[top] = src_len - 1, 0
    return i0, np.minimum(i0 + 1, src_len - 1), f


def _resize_one(x, hd, wd):
    """x [..., hs, ws] -> [..., hd, wd]; the blend in the dtype of x."""
    hs, ws = x.shape[-2:]
    y0, y1, fy = source_coords(hs, hd)
    x0, x1, fx = source_coords(ws, wd)
    fy = torch.from_numpy(fy).to(x.dtype)[:, None]
    fx = torch.from_numpy(fx).to(x.dtype)[None, :]
    a, b = x[..., y0, :][..., :, x0], x[..., y0, :][..., :, x1]
    c, d = x[..., y1, :][..., :, x0], x[..., y1, :][..., :, x1]
    return (1 - fy) * ((1 - fx) * a + fx * b) + fy * ((1 - fx) * c + fx * d)


def resize_bilinear(x, size, src_sizes=None, dst_sizes=None):
    b = x.size(0)
    hd, wd = size
    out = torch.zeros((b, x.size(1), hd, wd), dtype=x.dtype)
    for i in range(b):
        hs, ws = (x.shape[2:] if src_sizes is None else src_sizes[i])
        h, w = (size if dst_sizes is None else dst_sizes[i])
        out[i, :, :h, :w] = _resize_one(x[i, :, :hs, :ws], h, w)
    return out


# ------------------------------------------------------------------------------------------------------------------- noise
def add_gaussian_noise(x, noise, noise_gray, sigma, gray, clip, rounds):
    b = x.size(0)
    n = noise
    if gray is not None:
        n = torch.where(gray.view(b, 1, 1, 1) != 0, noise_gray.expand_as(noise), noise)
    out = x + n * sigma.view(b, 1, 1, 1) / 255.
    if clip and rounds:
        out = torch.clamp((out * 255.0).round(), 0, 255) / 255.
    elif clip:
        out = torch.clamp(out, 0, 1)
    elif rounds:
        out = (out * 255.0).round() / 255.
    return out


# ------------------------------------------------------------------------------------------------------------------ finish
def finish_pre_round(x, jitter=None, gray=None):
    """Steps 1 and 2: the value that gets rounded."""
    b = x.size(0)
    if jitter is not None:
        x = torch.clamp(x + jitter.view(b, 3, 1, 1), 0, 1)
    if gray is not None:
        g = (0.299 * x[:, 0:1] + 0.587 * x[:, 1:2]) + 0.114 * x[:, 2:3]
        x =torch.where(gray.view(b, 1, 1, 1) != 0, g.expand_as(x), x)
    return x


def finish_round(x, mean=None, std=None):
    """Steps 3 and 4."""
    x = torch.clamp((x * 255.0).round(), 0, 255) / 255.
    if mean is not None or std is not None:
        m = x.new_tensor([0.] * 3 if mean is None else mean).view(1, 3, 1, 1)
        s = x.new_tensor([1.] * 3 if std is None else std).view(1, 3, 1, 1)
        x = (x - m) / s
    return x


def finish(x, jitter=None, gray=None, mean=None, std=None):
    return finish_round(finish_pre_round(x, jitter, gray), mean, std)


# ---------------------------------------------------------------------------------------------------------------- DiffJPEG
_Y = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
               [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
               [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], dtype=np.float64).T
_C = np.full((8, 8), 99, dtype=np.float64)
_C[:4, :4] = np.array([[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]).T
_TO_YCC = np.array([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]])
_TO_RGB = np.array([[1., 0., 1.402], [1, -0.344136, -0.714136], [1, 1.772, 0]])


def quality_to_factor(q):
    return (5000. / q if q < 50 else 200. - q * 2) / 100.


def _consts(dtype, device='cpu'):
    """The constants as the reference holds them: float32 Parameters (the DCT basis as the rounded PRODUCT of two cosines), which
    ``.double()`` widens without changing their values."""
    n = np.arange(8)
    cosm = np.cos((2 * n[:, None] + 1) * n[None, :] * math.pi / 16)        # [position][frequency]
    basis = (cosm[:, None, :, None] * cosm[None, :, None, :]).astype(np.float32)      # [x][y][u][v]
    alpha = np.array([1 / math.sqrt(2)] + [1.] * 7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(device=device, dtype=dtype)      # noqa: E731
    return t(basis), t(np.outer(alpha, alpha) * 0.25), t(np.outer(alpha, alpha)), t(_Y), t(_C), t(_TO_YCC), t(_TO_RGB)


def _blocks(p):
    b, h, w = p.shape
    return p.reshape(b, h // 8, 8, w // 8, 8).permute(0, 1, 3, 2, 4)        # [B, h/8, w/8, 8, 8]


def _unblocks(p):
    b, nh, nw = p.shape[:3]
    return p.permute(0, 1, 3, 2, 4).reshape(b, nh * 8, nw * 8)


def diffjpeg(x, factor, differentiable, coef_fp32=False):
    """DiffJPEG.forward on x [B, 3, H, W] with factors [B] (a tensor of the dtype of x).  Returns (out, quotients, pre) with
    quotients = (qy [B, Hp/8, Wp/8, 8, 8], qcb, qcr [B, Hp/16, Wp/16, 8, 8]) before rounding and pre [B, 3, Hp, Wp] the RGB values
    before the clamp on the 0..255 scale, Hp and Wp the padded size.

    ``coef_fp32``: the reference divides ``image.float()`` by the table (diffjpeg.py:169, :199), so even its float64 run rounds the
    DCT coefficients to float32 first.  The recorded outputs are reproduced with it; the yardstick (the default) does not round."""
    basis, scale, alpha2, ytab, ctab, to_ycc, to_rgb = _consts(x.dtype, x.device)
    b, _, h, w = x.shape
    hp, wp = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    xp = F.pad(x, (0, wp - w, 0, hp - h)) * 255
    ycc = torch.einsum('bchw,dc->bdhw', xp, to_ycc)
    planes = [ycc[:, 0], F.avg_pool2d(ycc[:, 1:2], 2)[:, 0] + 128, F.avg_pool2d(ycc[:, 2:3], 2)[:, 0] + 128]
    fac = factor.view(b, 1, 1, 1, 1)
    quot, rec = [], []
    for i, p in enumerate(planes):
        blk = _blocks(p) - 128
        coef = torch.einsum('...xy,xyuv->...uv', blk, basis) * scale
        table = (ytab if i == 0 else ctab) * fac
        q = (coef.float().to(x.dtype) if coef_fp32 else coef) / table
        r = torch.round(q)
        if differentiable:
            r = r + (q - r) ** 3
        deq = r * table
        rec.append(_unblocks(0.25 * torch.einsum('...xy,uvxy->...uv', deq * alpha2, basis) + 128))
        quot.append(q)
    up = lambda p: p.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)   # noqa: E731
    img = torch.stack([rec[0], up(rec[1]) - 128, up(rec[2]) - 128], dim=1)
    pre = torch.einsum('bchw,dc->bdhw', img, to_rgb)
    out = torch.clamp(pre, 0, 255) / 255
    return out[:, :, :h, :w], tuple(quot), pre


def diffjpeg_ragged(x, factor, differentiable, sizes):
    """The same per sample on its own rectangle of the padded buffer; zero outside.  Returns (out, [per-sample (quotients, pre)])."""
    out = torch.zeros_like(x)
    extra = []
    for i, (h, w) in enumerate(sizes):
        o, q, pre = diffjpeg(x[i:i + 1, :, :h, :w], factor[i:i + 1], differentiable)
        out[i:i + 1, :, :h, :w] = o
        extra.append((q, pre))
    return out, extra


def macroblock_quotients(quot):
    """[B, Hp/16, Wp/16, 384]: the six blocks of every macroblock."""
    qy, qcb, qcr = quot
    b, nh, nw = qcb.shape[:3]
    y = qy.reshape(b, nh, 2, nw, 2, 64).permute(0, 1, 3, 2, 4, 5).reshape(b, nh, nw, 256)
    return torch.cat([y, qcb.reshape(b, nh, nw, 64), qcr.reshape(b, nh, nw, 64)], dim=-1)


def tie_exposed(quot):
    """[B, Hp/16, Wp/16] bool: macroblocks with a quotient so close to a half-integer that fp32 rounding may flip its rounding."""
    q = macroblock_quotients(quot).double()
    frac = q - torch.floor(q)
    return ((frac - 0.5).abs() < 1e-4 + 2.0 ** -17 * q.abs()).any(dim=-1)


def pixel_mask(mb_mask, h, w):
    """A per-macroblock mask [B, nh, nw] as a per-pixel mask [B, 1, h, w]."""
    return mb_mask.repeat_interleave(16, dim=1).repeat_interleave(16, dim=2)[:, None, :h, :w]


def clamp_exposed(pre, margin=1e-3):
    """[B, Hp/16, Wp/16] bool: macroblocks with a value before the clamp within ``margin`` of 0 or 255 in some channel."""
    p = pre.double()
    near = ((p.abs() < margin) | ((p - 255).abs() < margin)).any(dim=1)
    b, hp, wp = near.shape
    return near.reshape(b, hp // 16, 16, wp // 16, 16).any(dim=4).any(dim=2)


# ------------------------------------------------------------------------------------------------------------- test images
def smooth_noise_image(seed, b, h, w, dtype=torch.float64):
    """Seeded images in [0, 1] with real AC energy: a few low-frequency waves per channel plus uniform noise."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.arange(h, dtype=torch.float64)[:, None] / 16
    xx = torch.arange(w, dtype=torch.float64)[None, :] / 16
    ph = torch.rand((b, 3, 4), generator=g, dtype=torch.float64) * 6.283
    img = 0.5 + 0.22 * torch.sin(2.1 * yy + 1.3 * xx + ph[..., 0, None, None]) + 0.15 * torch.cos(0.7 * yy - 2.9 * xx + ph[..., 1, None, None])
    img = img + 0.12 * (torch.rand((b, 3, h, w), generator=g, dtype=torch.float64) - 0.5)
    return img.clamp(0, 1).float().to(dtype)   # fp32-representable, so the device sees the same numbers
