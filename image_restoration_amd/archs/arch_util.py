"""Parameter containers and initialisers for the HIP-backed architectures.

``Conv3x3Params`` only OWNS an OIHW weight and a bias with nn.Conv2d's state_dict keys
and default initialisation; it has no forward — the arithmetic of every layer is issued
by the owning network through libsr_hip.so.
"""
import logging
import math

import torch
from torch import nn
from torch.nn import init

from .. import _lib
from .. import hip_autograd as A
from .. import hip_ops as H
from ..ops.dcn import ModulatedDeformConvPack
from ..ops.flow_warp import flow_warp  # noqa: F401  (the reference's arch_util.flow_warp, :112-143)


class Conv3x3Params(nn.Module):
    """weight [cout, cin, 3, 3] + bias [cout], initialised like nn.Conv2d(cin, cout, 3, 1, 1)
    (kaiming_uniform(a=sqrt(5)) / U(+-1/sqrt(fan_in))), which the reference keeps for the six
    non-RDB convs of RRDBNet (rrdbnet_arch.py:94-101)."""

    def __init__(self, cin, cout, bias=True, ksize=3):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = cin, cout, ksize
        self.weight = nn.Parameter(torch.empty(cout, cin, ksize, ksize))
        self.bias = nn.Parameter(torch.empty(cout)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in = self.in_channels * self.kernel_size * self.kernel_size
            bound = 1 / math.sqrt(fan_in)
            init.uniform_(self.bias, -bound, bound)

    def extra_repr(self):
        return f'{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride=1, padding=1 [HIP]'

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('Conv3x3Params is a parameter container; the owning network launches the HIP kernels')


@torch.no_grad()
def default_init_weights(module_list, scale=1, bias_fill=0, **kwargs):
    """kaiming_normal_ * scale, bias = bias_fill — the RDB initialisation of the reference
    (arch_util.py:12-40, called with scale 0.1 at rrdbnet_arch.py:30)."""
    if not isinstance(module_list, list):
        module_list = [module_list]
    for module in module_list:
        for m in module.modules():
            if isinstance(m, (Conv3x3Params, nn.Conv2d, nn.Linear)):
                init.kaiming_normal_(m.weight, **kwargs)
                m.weight.data *= scale
                if m.bias is not None:
                    m.bias.data.fill_(bias_fill)
            elif isinstance(m, nn.modules.batchnorm._BatchNorm):
                init.constant_(m.weight, 1)
                if m.bias is not None:
                    m.bias.data.fill_(bias_fill)


def _bn_scale(bn_weight, running_var, eps):
    """``gamma / sqrt(var + eps)`` of an eval-mode BatchNorm, in float64 on the host."""
    return bn_weight.detach().cpu().double() / torch.sqrt(running_var.detach().cpu().double() + float(eps))


def fold_batchnorm(weight, bn_weight, bn_bias, running_mean, running_var, eps, bias=None):
    """(w', b') of eval-mode BatchNorm behind a conv of any rank, in float64 on the host, rounded once to fp32 (CPU tensors):
    ``w' = w * s``, ``b' = (b - mean) * s + beta``, ``s = gamma / sqrt(var + eps)``; ``bias`` None is a bias-free conv."""
    scale = _bn_scale(bn_weight, running_var, eps)
    w = weight.detach().cpu().double() * scale.view(-1, *([1] * (weight.dim() - 1)))
    if bias is None:
        b = bn_bias.detach().cpu().double() - running_mean.detach().cpu().double() * scale
    else:
        b = (bias.detach().cpu().double() - running_mean.detach().cpu().double()) * scale + bn_bias.detach().cpu().double()
    return w.float(), b.float()


def bn_prologue(bn):
    """(scale, shift) of eval-mode ``bn`` in front of a conv as fp32 CPU tensors: ``scale = gamma / sqrt(var + eps)``, ``shift =
    beta - mean * scale`` in float64, rounded once.  The kernels apply ``max(x * scale + shift, 0)``."""
    scale = _bn_scale(bn.weight, bn.running_var, bn.eps)
    shift = bn.bias.detach().cpu().double() - bn.running_mean.detach().cpu().double() * scale
    return scale.float(), shift.float()


def refuse_inference_only(net_name, training, tensors, params, what):
    """The refusals of a forward-only network whose BatchNorm layers run from their running statistics (TOFlow, DUF): training
    mode, a forward that would need a graph, CPU inputs.  ``what``: what the network does with those layers."""
    if training:
        raise NotImplementedError(f'{net_name} runs in eval mode only: its BatchNorm layers are {what} their running statistics '
                                  'and batch statistics are not built; call .eval()')
    if torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(p.requires_grad for p in params)):
        raise NotImplementedError(f'{net_name} runs inference only: there is no backward; run under torch.no_grad() (or clear '
                                  'requires_grad on the input and the parameters)')
    if not all(t.is_cuda for t in tensors):
        raise _lib.SrHipError(f'{net_name}.forward runs only on a HIP device (no CPU fallback): move the module and inputs with '
                              '.to("cuda")')


def make_layer(basic_block, num_basic_block, **kwarg):
    """nn.Sequential of `num_basic_block` blocks (reference arch_util.py:43-56) — gives the
    ``body.{i}.`` state_dict prefix."""
    return nn.Sequential(*[basic_block(**kwarg) for _ in range(num_basic_block)])


def upscale_stages(upscale):
    """Pixel-shuffle factors of the reference's Upsample (arch_util.py:90-109): 2^n -> n stages of 2 (none for 1), 3 -> one
    of 3; None for a scale it does not support (the caller raises in its own words)."""
    if upscale == 3:
        return [3]
    if isinstance(upscale, int) and upscale >= 1 and upscale & (upscale - 1) == 0:
        return [2] * (int(upscale).bit_length() - 1)
    return None


def resize_flow(flow, size_type, sizes, interp_mode='bilinear', align_corners=False):
    """Resize a flow [N, 2, H, W] by a ratio or to a shape (reference arch_util.py:146-181): the x channel is scaled by
    out_w / w and the y channel by out_h / h (sr_channel_affine_f32), then the map is resized (sr_resize_bilinear_f32, whose
    half-pixel rule is F.interpolate's ``align_corners=False``).  ``sizes``: [ratio_h, ratio_w] or [out_h, out_w].  ValueError
    for another ``size_type``, interpolation or ``align_corners=True``; device fp32 tensors only (no gradient)."""
    if size_type not in ('ratio', 'shape'):
        raise ValueError(f'Size type should be ratio or shape, but got type {size_type}.')
    if interp_mode != 'bilinear' or align_corners:
        raise ValueError(f"resize_flow: interp_mode '{interp_mode}', align_corners={align_corners} is not supported; supported: "
                         "'bilinear', align_corners=False")
    if flow.dim() != 4 or flow.size(1) != 2 or flow.dtype != torch.float32:
        raise ValueError(f'resize_flow: expected an fp32 [N, 2, H, W] flow, got {flow.dtype} {tuple(flow.shape)}')
    H._need_cuda(flow, 'resize_flow')
    n, _, h, w = flow.shape
    if size_type == 'ratio':
        oh, ow = int(h * sizes[0]), int(w * sizes[1])
    else:
        oh, ow = int(sizes[0]), int(sizes[1])
    flow = flow.detach().contiguous()
    ratio = torch.tensor([ow / w, oh / h], dtype=torch.float32, device=flow.device)
    scaled = torch.empty_like(flow)
    H.launch('sr_channel_affine_f32', flow.device, flow.data_ptr(), scaled.data_ptr(), ratio.data_ptr(), None, n, 2, h * w)
    return H.resize_bilinear(scaled, (oh, ow))


class ResidualBlockNoBN(nn.Module):
    """Parameters of ``x + res_scale * conv2(relu(conv1(x)))`` (reference arch_util.py:59-87): conv1 / conv2 are
    num_feat -> num_feat 3x3 convs with bias, initialised kaiming_normal * 0.1, bias 0 (``pytorch_init=False``) or like
    nn.Conv2d.  No forward: the owning network (MSRResNet) issues the two convs through libsr_hip.so."""

    def __init__(self, num_feat=64, res_scale=1, pytorch_init=False):
        super().__init__()
        self.res_scale = res_scale
        self.conv1 = Conv3x3Params(num_feat, num_feat)
        self.conv2 = Conv3x3Params(num_feat, num_feat)
        if not pytorch_init:
            default_init_weights([self.conv1, self.conv2], 0.1)


class DCNv2Pack(ModulatedDeformConvPack):
    """Modulated deformable conv for deformable alignment (reference arch_util.py:204-227): unlike ModulatedDeformConvPack the
    offsets and the mask come from another feature map, ``feat``.  ``conv_offset`` is one sr_conv3x3_f32; the deformable conv
    reads the two windows of its output in place with the sigmoid in the sampler (include/sr_hip_dcn.h).

    Difference from the reference: its warning when mean|offset| > 50 costs a device reduction and a host synchronisation, so it
    is evaluated in training mode only (the reference evaluates it on every call)."""

    def forward_cb8(self, x, feat, act_slope=1.0):
        """CB8 in, CB8 out; LeakyReLU(act_slope) fused into the deformable conv's epilogue."""
        co = self.offsets_cb8(feat)
        if self.training:
            offset_absmean = self.offset_absmean(co)
            if offset_absmean > 50:
                logging.getLogger('basicsr').warning(f'Offset abs mean is {offset_absmean}, larger than 50.')
        return self.deform_cb8(x, co, act_slope)

    def forward_cb16(self, x, feat, act_slope=1.0):
        """The bf16 inference path: hip_ops.CB16 in, CB16 out.  ``conv_offset`` is one sr_conv3x3_bf16 that stores its 27 * dg
        outputs as fp32 NCHW planes (offsets keep fp32 resolution), which sr_dcn_fwd_bf16 reads in place with the sigmoid in the
        sampler.  No offset warning: this path is inference."""
        dg = self.deformable_groups
        co = torch.empty((feat.n, 27 * dg, feat.h, feat.w), dtype=torch.float32, device=feat.device)
        H.conv3x3_bf16(feat, H.packed_conv_bf16(self.conv_offset), out_nchw=co)
        return H.dcn_fwd_bf16(x, co[:, :18 * dg], co[:, 18 * dg:], H.packed_conv_bf16(self), dg, mask_is_logit=True,
                              act_slope=act_slope)

    def forward(self, x, feat):
        if x.dtype != torch.float32 or feat.dtype != torch.float32:
            raise ValueError(f'DCNv2Pack: {x.dtype} / {feat.dtype} input is not supported; supported: fp32')
        if not (x.is_cuda and feat.is_cuda):
            raise NotImplementedError
        return A.FromCB8.apply(self.forward_cb8(A.ToCB8.apply(x), A.ToCB8.apply(feat)), self.out_channels)
