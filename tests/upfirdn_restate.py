"""The float64 yardstick of upfirdn2d and of the fused bias + LeakyReLU for the GPU tests, written from the definitions in
include/sr_hip_stylegan2.h (not from the product's modules, and with no convolution call): differentiable torch code.

upfirdn2d, per plane: insert up - 1 zeros after every sample, pad (a negative pad crops), out'[u] = sum_j P[u + j] * f[k - 1 - j]
as an explicit sum of shifted slices, keep every down-th sample."""
import torch
import torch.nn.functional as F


def upfirdn2d(x, k, up, down, pad):
    """x [N, C, H, W], k [kh, kw], up = (ux, uy), down = (dx, dy), pad = (px0, px1, py0, py1)."""
    n, c, h, w = x.shape
    kh, kw = k.shape
    z = x.new_zeros((n, c, h * up[1], w * up[0]))
    z[:, :, ::up[1], ::up[0]] = x
    z = F.pad(z, tuple(pad))
    fh, fw = z.size(2) - kh + 1, z.size(3) - kw + 1
    if fh <= 0 or fw <= 0:
        raise ValueError('non-positive output size')
    out = x.new_zeros((n, c, fh, fw))
    for jy in range(kh):
        for jx in range(kw):
            out = out + z[:, :, jy:jy + fh, jx:jx + fw] * k[kh - 1 - jy, kw - 1 - jx]
    return out[:, :, ::down[1], ::down[0]]


def out_size(h, w, kh, kw, up, down, pad):
    return (h * up[1] + pad[2] + pad[3] - kh) // down[1] + 1, (w * up[0] + pad[0] + pad[1] - kw) // down[0] + 1


def taps(kh, kw, up):
    """T of the bound: the most taps an output can meet."""
    return -(-kh // up[1]) * -(-kw // up[0])


def grad_call(g, k, in_hw, up, down, pad):
    """The adjoint as the header states it: factors swapped, filter flipped, pads (k - pad0 - 1, in * up - out * down + pad0 - up + 1)."""
    kh, kw = k.shape
    (ih, iw), (oh, ow) = in_hw, g.shape[2:]
    gp = (kw - pad[0] - 1, iw * up[0] - ow * down[0] + pad[0] - up[0] + 1, kh - pad[2] - 1, ih * up[1] - oh * down[1] + pad[2] - up[1] + 1)
    return upfirdn2d(g, torch.flip(k, [0, 1]), down, up, gp), gp


def bias_act(x, b, slope, scale, ref=None):
    """lrelu(x + b[c], slope) * scale with the sign from ref where given; the channel is dimension 1."""
    t = x if b is None else x + b.view(1, -1, *([1] * (x.dim() - 2)))
    s = t if ref is None else ref
    return torch.where(s > 0, t, t * slope) * scale
