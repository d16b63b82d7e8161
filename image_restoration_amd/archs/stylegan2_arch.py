"""The resampling and activation modules of the reference's basicsr/archs/stylegan2_arch.py (lines 26-131 and 591-604) on
``ops.upfirdn2d`` and ``ops.fused_act``: make_resample_kernel, UpFirDnUpsample, UpFirDnDownsample, UpFirDnSmooth and
ScaledLeakyReLU, with the reference's constructor arguments, pad rules and ``__repr__``.  Nothing here is registered in
ARCH_REGISTRY (the reference registers none of them); the generator, the equalised layers and the discriminator are not part
of this module.
"""
import torch
from torch import nn

from ..ops.fused_act import fused_leaky_relu
from ..ops.upfirdn2d import upfirdn2d


def make_resample_kernel(k):
    """The 2D resampling filter of a 1D magnitude list: its outer product with itself (a 2D list is taken as it is),
    normalised to sum 1, in fp32."""
    k = torch.tensor(k, dtype=torch.float32)
    if k.ndim == 1:
        k = k[None, :] * k[:, None]
    return k / k.sum()


class _UpFirDn(nn.Module):
    """kernel (a plain attribute, as in the reference: not a buffer, absent from the state_dict) + factors + pad."""
    up = down = 1

    def forward(self, x):
        if x.dtype != torch.float32:
            raise ValueError(f'{self.__class__.__name__}: {x.dtype} is not supported; supported: fp32')
        if self.kernel.device != x.device:
            self.kernel = self.kernel.to(x.device)
        return upfirdn2d(x, self.kernel, up=self.up, down=self.down, pad=self.pad)


class UpFirDnUpsample(_UpFirDn):
    """Up-sampling by ``factor``: the filter times factor^2, pad ((p + 1) // 2 + factor - 1, p // 2), p = k - factor."""

    def __init__(self, resample_kernel, factor=2):
        super().__init__()
        self.kernel = make_resample_kernel(resample_kernel) * (factor ** 2)
        self.factor = self.up = factor
        pad = self.kernel.shape[0] - factor
        self.pad = ((pad + 1) // 2 + factor - 1, pad // 2)

    def __repr__(self):
        return f'{self.__class__.__name__}(factor={self.factor})'


class UpFirDnDownsample(_UpFirDn):
    """Down-sampling by ``factor``: pad ((p + 1) // 2, p // 2), p = k - factor."""

    def __init__(self, resample_kernel, factor=2):
        super().__init__()
        self.kernel = make_resample_kernel(resample_kernel)
        self.factor = self.down = factor
        pad = self.kernel.shape[0] - factor
        self.pad = ((pad + 1) // 2, pad // 2)

    def __repr__(self):
        return f'{self.__class__.__name__}(factor={self.factor})'


class UpFirDnSmooth(_UpFirDn):
    """The blur beside a strided or transposed convolution of ``kernel_size``: factors 1, the filter times upsample_factor^2 and
    pad ((p + 1) // 2 + u - 1, p // 2 + 1) with p = k - u - (kernel_size - 1) when up-sampling, pad ((p + 1) // 2, p // 2) with
    p = k - d + (kernel_size - 1) when down-sampling."""

    def __init__(self, resample_kernel, upsample_factor=1, downsample_factor=1, kernel_size=1):
        super().__init__()
        self.upsample_factor = upsample_factor
        self.downsample_factor = downsample_factor
        self.kernel = make_resample_kernel(resample_kernel)
        if upsample_factor > 1:
            self.kernel = self.kernel * (upsample_factor ** 2)
            pad = (self.kernel.shape[0] - upsample_factor) - (kernel_size - 1)
            self.pad = ((pad + 1) // 2 + upsample_factor - 1, pad // 2 + 1)
        elif downsample_factor > 1:
            pad = (self.kernel.shape[0] - downsample_factor) + (kernel_size - 1)
            self.pad = ((pad + 1) // 2, pad // 2)
        else:
            raise NotImplementedError

    def __repr__(self):
        return f'{self.__class__.__name__}(upsample_factor={self.upsample_factor}, downsample_factor={self.downsample_factor})'


class ScaledLeakyReLU(nn.Module):
    """leaky_relu(x, negative_slope) * sqrt(2): the fused activation without a bias."""

    def __init__(self, negative_slope=0.2):
        super().__init__()
        self.negative_slope = negative_slope

    def forward(self, x):
        return fused_leaky_relu(x, None, self.negative_slope, 2 ** 0.5)
