"""``modulated_deform_conv`` / ``ModulatedDeformConv`` / ``ModulatedDeformConvPack`` of the reference
(basicsr/ops/dcn/deform_conv.py:121-383) on the HIP kernels of include/sr_hip_dcn.h.

Supported configuration: kernel 3x3, stride 1, padding 1, dilation 1, groups 1, fp32 CUDA tensors, in_channels /
deformable_groups a multiple of 8.  Anything else raises ValueError naming this configuration; a CPU tensor raises
NotImplementedError as the reference does.  There is no fallback to another implementation.
"""
import math

import torch
from torch import nn
from torch.nn.modules.utils import _pair, _single

from ... import hip_autograd as A

SUPPORTED = ('kernel 3x3, stride 1, padding 1, dilation 1, groups 1, fp32, in_channels / deformable_groups a multiple of 8')


def _one(v):
    """An int or an (a, a) pair -> a; None when the two differ."""
    a, b = _pair(v)
    return a if a == b else None


def check_config(cin, ksize, stride, padding, dilation, groups, deformable_groups, dtype=torch.float32):
    """Raises ValueError unless this is the supported configuration."""
    got = (tuple(_pair(ksize)), _one(stride), _one(padding), _one(dilation), groups)
    if got != ((3, 3), 1, 1, 1, 1) or dtype != torch.float32 or deformable_groups < 1 or cin % (8 * deformable_groups) != 0:
        raise ValueError(f'modulated_deform_conv: kernel {tuple(_pair(ksize))}, stride {stride}, padding {padding}, dilation '
                         f'{dilation}, groups {groups}, deformable_groups {deformable_groups}, in_channels {cin}, {dtype} is not '
                         f'supported; supported: {SUPPORTED}')


def modulated_deform_conv(input, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, *,
                          deterministic=False):
    """The reference's ``modulated_deform_conv`` (ModulatedDeformConvFunction.apply, deform_conv.py:121-189): NCHW in, NCHW out.
    ``offset`` [N, 18 * dg, H, W] with (h, w) interleaved per tap inside each group's 18 channels, ``mask`` [N, 9 * dg, H, W].
    ``deterministic`` is this project's own key: the input gradient is then summed in 64-bit integers
    (include/sr_hip_dcn_det.h) and two backward passes agree bit for bit; the forward and the other gradients are the same."""
    for t in (input, offset, mask, weight):
        if t.dtype != torch.float32:
            check_config(input.size(1), weight.shape[2:], stride, padding, dilation, groups, deformable_groups, t.dtype)
    check_config(input.size(1), weight.shape[2:], stride, padding, dilation, groups, deformable_groups)
    dg = deformable_groups
    n, _, h, w = input.shape
    if tuple(offset.shape) != (n, 18 * dg, h, w) or tuple(mask.shape) != (n, 9 * dg, h, w) or weight.size(1) != input.size(1):
        raise ValueError(f'modulated_deform_conv: offset {tuple(offset.shape)} / mask {tuple(mask.shape)} / weight '
                         f'{tuple(weight.shape)} do not fit input {tuple(input.shape)} with deformable_groups {dg}')
    if not input.is_cuda:
        raise NotImplementedError
    extra = (None, True) if deterministic else ()
    y = A.DCNFn.apply(A.ToCB8.apply(input), A.ToCB8.apply(offset), A.ToCB8.apply(mask), weight, bias, 1.0, dg, False, *extra)
    return A.FromCB8.apply(y, weight.size(0))


class ModulatedDeformConv(nn.Module):
    """Parameters and forward of the reference's ModulatedDeformConv (deform_conv.py:293-337): weight U(+-1/sqrt(cin * 9)),
    bias zero.  ``deterministic`` (an attribute, not a constructor argument: the signature is the reference's) selects the
    bit-reproducible input gradient of ``modulated_deform_conv``."""

    deterministic = False

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1,
                 bias=True):
        super().__init__()
        check_config(in_channels, kernel_size, stride, padding, dilation, groups, deformable_groups)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride = stride
        self.padding = padding
        self.dilation = dilation
        self.groups = groups
        self.deformable_groups = deformable_groups
        self.with_bias = bias
        # enable compatibility with nn.Conv2d
        self.transposed = False
        self.output_padding = _single(0)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.init_weights()

    def init_weights(self):
        n = self.in_channels
        for k in self.kernel_size:
            n *= k
        stdv = 1. / math.sqrt(n)
        self.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.zero_()

    def forward(self, x, offset, mask):
        return modulated_deform_conv(x, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups,
                                     self.deformable_groups, deterministic=self.deterministic)


class ModulatedDeformConvPack(ModulatedDeformConv):
    """ModulatedDeformConv that computes its own offsets and mask with ``conv_offset`` (deform_conv.py:340-383): a 3x3 conv to
    27 * dg channels, zero-initialised, whose first two thirds are the offsets (used unpermuted) and whose last third is the
    mask logit.  ``conv_offset`` is an nn.Conv2d used as a parameter container: the arithmetic is one sr_conv3x3_f32."""

    _version = 2

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.conv_offset = nn.Conv2d(self.in_channels, self.deformable_groups * 3 * self.kernel_size[0] * self.kernel_size[1],
                                     kernel_size=self.kernel_size, stride=_pair(self.stride), padding=_pair(self.padding),
                                     dilation=_pair(self.dilation), bias=True)
        self.init_weights()

    def init_weights(self):
        super().init_weights()
        if hasattr(self, 'conv_offset'):
            self.conv_offset.weight.data.zero_()
            self.conv_offset.bias.data.zero_()

    def offsets_cb8(self, feat):
        """conv_offset on the CB8 tensor ``feat``: its CB8 output of 27 * dg channels (offsets, then mask logits)."""
        return A.ConvFn.apply(feat, self.conv_offset.weight, self.conv_offset.bias, 1.0)

    def deform_cb8(self, x, co, act_slope=1.0):
        """The deformable conv of the CB8 tensor ``x`` at the offsets and mask logits ``co`` (offsets_cb8's output), with
        LeakyReLU(act_slope) in the epilogue.  When dg % 4 == 0 the two parts are channel-block windows of ``co`` and are read
        in place with the sigmoid in the sampler; otherwise they are split by a copy first."""
        dg = self.deformable_groups
        det = self.deterministic   # DCNFn's trailing flag goes behind ``windows``, and only when set
        if dg % 4 == 0:
            windows = ((0, 18 * dg // 8), (18 * dg // 8, (9 * dg + 7) // 8))
            return A.DCNFn.apply(x, co, co, self.weight, self.bias, act_slope, dg, True, windows, *((True,) if det else ()))
        nchw = A.FromCB8.apply(co, 27 * dg)
        offset, logit = A.ToCB8.apply(nchw[:, :18 * dg]), A.ToCB8.apply(nchw[:, 18 * dg:])
        return A.DCNFn.apply(x, offset, logit, self.weight, self.bias, act_slope, dg, True, *((None, True) if det else ()))

    def offset_absmean(self, co):
        """mean |offset| over the real offset channels of ``co`` (one device reduction and a host sync)."""
        dg = self.deformable_groups
        off = co.detach()[:, :18 * dg // 8] if dg % 4 == 0 else A.FromCB8.apply(co.detach(), 27 * dg)[:, :18 * dg]
        return float(A.mean(off.abs()))

    def forward(self, x):
        if x.dtype != torch.float32:
            check_config(self.in_channels, self.kernel_size, self.stride, self.padding, self.dilation, self.groups,
                         self.deformable_groups, x.dtype)
        if not x.is_cuda:
            raise NotImplementedError
        xc = A.ToCB8.apply(x)
        return A.FromCB8.apply(self.deform_cb8(xc, self.offsets_cb8(xc)), self.out_channels)
