"""``filter2D``, ``DiffJPEG`` and the ``*_pt`` noise functions of the reference on the HIP kernels of include/sr_hip_degrade.h,
plus the bilinear resize and the tail of the plate degradation the reference runs through cv2 on the host.

Every function is one launch over the batch on the current stream.  There is no CPU path: a CPU tensor raises SrHipError.
Only ``DiffJPEG(differentiable=True)`` has a gradient (``DiffJPEGFunction``: sr_diffjpeg_bwd_f32 recomputes the quotients from
the saved input); the other stages make training data and are not differentiated.

Differences from the reference, on purpose:
  * ``DiffJPEG.forward`` leaves a ``quality`` tensor as the caller passed it; the reference overwrites it with the factors
    (utils/diffjpeg.py:477-478).
  * gray noise takes one plane per sample, ``noise_gray`` [B, 1, H, W]; the reference draws a single [H, W] plane and views it as
    [B, 1, H, W], which only works for B = 1 (data/degradations.py:617-618).
"""
import torch
from torch.autograd import Function

from ... import hip_ops as H


def filter2D(img, kernel):
    """PyTorch version of cv2.filter2D: ``img`` (b, c, h, w), ``kernel`` (1 or b, k, k), reflect border."""
    if kernel.size(-1) % 2 != 1:
        raise ValueError('Wrong kernel size')
    return H.filter2d(img, kernel)


def resize_bilinear(x, size, src_sizes=None, dst_sizes=None):
    """cv2.resize(INTER_LINEAR) / F.interpolate(bilinear, align_corners=False) of a batch to ``size`` = (h, w).  ``src_sizes`` /
    ``dst_sizes`` ([B, 2] of (h_i, w_i)) make the batch ragged: sample i is read from / written to its own rectangle."""
    return H.resize_bilinear(x, size, src_sizes, dst_sizes)


def add_gaussian_noise_pt(img, sigma=10, gray_noise=0, clip=True, rounds=False, noise=None, noise_gray=None):
    """Add Gaussian noise: ``sigma`` a number or [B] on the 0..255 scale, ``gray_noise`` a number or [B] of 0 / 1.  The draws are
    torch.randn on the device of ``img`` unless ``noise`` [B, C, H, W] (and ``noise_gray`` [B, 1, H, W]) are passed in."""
    H._need_cuda(img, 'add_gaussian_noise_pt')
    b, _, h, w = img.shape
    if torch.is_tensor(gray_noise):
        gray = H._per_sample(gray_noise, b, img, 'add_gaussian_noise_pt: gray_noise')
        wanted = noise_gray is not None or bool((gray != 0).any())      # (reads the flags back, as the reference's torch.sum(...) > 0)
    else:
        wanted = gray_noise > 0
        gray = torch.ones(b, dtype=torch.float32, device=img.device) if wanted else None
    if noise is None:
        noise = torch.randn(img.shape, dtype=img.dtype, device=img.device)
    if not wanted:
        gray = noise_gray = None
    elif noise_gray is None:   # drawn like the reference: only when some sample asks for it
        noise_gray = torch.randn((b, 1, h, w), dtype=img.dtype, device=img.device)
    return H.add_gaussian_noise(img, noise, sigma, noise_gray, gray, clip, rounds)


def random_add_gaussian_noise_pt(img, sigma_range=(0, 1.0), gray_prob=0, clip=True, rounds=False):
    b = img.size(0)
    sigma = torch.rand(b, dtype=img.dtype, device=img.device) * (sigma_range[1] - sigma_range[0]) + sigma_range[0]
    gray = (torch.rand(b, dtype=img.dtype, device=img.device) < gray_prob).float()
    return add_gaussian_noise_pt(img, sigma, gray, clip, rounds)


def degrade_finish(x, jitter=None, gray=None, mean=None, std=None):
    """Jitter shift + clip, gray where set, clamp(round(v * 255), 0, 255) / 255, (v - mean) / std."""
    return H.degrade_finish(x, jitter, gray, mean, std)


def quality_to_factor(quality):
    """The quantisation factor of a JPEG quality (a number or a tensor of qualities)."""
    if torch.is_tensor(quality):
        q = quality.to(torch.float32)
        return torch.where(q < 50, 5000. / q, 200. - q * 2) / 100.
    return (5000. / quality if quality < 50 else 200. - quality * 2) / 100.


class DiffJPEGFunction(Function):
    """sr_diffjpeg_f32 with the differentiable rounding and its gradient sr_diffjpeg_bwd_f32; saves the input only."""

    @staticmethod
    def forward(ctx, x, factor, sizes):
        ctx.save_for_backward(x, factor)
        ctx.sizes = sizes
        return H.diffjpeg(x, factor, sizes, differentiable=True)

    @staticmethod
    def backward(ctx, grad_out):
        x, factor = ctx.saved_tensors
        return H.diffjpeg_bwd(x, factor, grad_out, ctx.sizes), None, None


class DiffJPEG(torch.nn.Module):
    """The reference's DiffJPEG (slightly different from libjpeg, as the reference notes): ``forward(x, quality)`` with ``x`` RGB
    [B, 3, H, W] in [0, 1] and ``quality`` a number or a [B] tensor, which is left unchanged.  ``sizes`` makes the batch ragged."""

    def __init__(self, differentiable=True):
        super().__init__()
        self.differentiable = bool(differentiable)

    def forward(self, x, quality, sizes=None):
        H._need_cuda(x, 'DiffJPEG')
        b = x.size(0)
        factor = quality_to_factor(quality)
        factor = H._per_sample(factor, b, x, 'DiffJPEG: quality')
        x = x.contiguous()
        if self.differentiable and x.requires_grad and torch.is_grad_enabled():
            return DiffJPEGFunction.apply(x, factor, H.ragged_sizes(sizes, b, x.size(2), x.size(3), x.device, 'DiffJPEG: sizes'))
        return H.diffjpeg(x, factor, sizes, differentiable=self.differentiable)
