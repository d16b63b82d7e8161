"""``FusedLeakyReLU`` / ``fused_leaky_relu`` of the reference (basicsr/ops/fused_act/fused_act.py) on the HIP kernels
sr_fused_bias_act_f32 / sr_fused_bias_act_bwd_f32 (include/sr_hip_stylegan2.h), differentiable twice.

``out = lrelu(input + bias[c], negative_slope) * scale`` with the channel on dimension 1 of a tensor of rank >= 2.

Supported: fp32 CUDA tensors, a bias with as many values as dimension 1 has (or None: the activation alone).  Another dtype or
bias length raises ValueError naming this; a CPU tensor raises NotImplementedError (the reference has no CPU path either).

Derivatives.  With m = 1 where out > 0 and negative_slope elsewhere, the backward is gx = m * scale * g and gbias[c] = the sum
of gx over every other dimension (one pass).  Both are linear in g, so the gradient of the backward with respect to g is the
forward entry point with ``ref = out`` fed ``ggx + ggbias[c]``; ``out`` gets no second-order gradient (m is piecewise
constant) and a third derivative is not provided.
"""
import torch
from torch import nn
from torch.autograd import Function

from ... import hip_ops as H

SUPPORTED = 'fp32 CUDA tensors of rank >= 2 with the channel on dimension 1, a bias of that many values or None'


def _check(input, bias):
    what = None
    if input.dim() < 2:
        what = f'an input of rank {input.dim()}'
    elif input.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        what = f'input {input.dtype} / bias {None if bias is None else bias.dtype}'
    elif bias is not None and (bias.dim() != 1 or bias.numel() != input.size(1)):
        what = f'a bias of shape {tuple(bias.shape)} for {input.size(1)} channels (dimension 1 of {tuple(input.shape)})'
    if what is not None:
        raise ValueError(f'fused_leaky_relu: {what} is not supported; supported: {SUPPORTED}')
    if not input.is_cuda:
        raise NotImplementedError('fused_leaky_relu has no CPU path')


class FusedLeakyReLUFunctionBackward(Function):

    @staticmethod
    def forward(ctx, grad_output, out, negative_slope, scale, want_bias=True):
        ctx.save_for_backward(out)
        ctx.negative_slope, ctx.scale = negative_slope, scale
        grad_input, grad_bias = H.fused_bias_act_bwd(grad_output.contiguous(), out, negative_slope, scale, want_bias)
        return grad_input, (grad_bias if want_bias else grad_output.new_zeros(0))

    @staticmethod
    def backward(ctx, gradgrad_input, gradgrad_bias):
        out, = ctx.saved_tensors
        if gradgrad_input is None:
            gradgrad_input = torch.zeros_like(out)
        if gradgrad_bias is not None and gradgrad_bias.numel() != out.size(1):
            gradgrad_bias = None
        bias = None if gradgrad_bias is None else gradgrad_bias.contiguous()
        gradgrad_out = H.fused_bias_act(gradgrad_input.contiguous(), bias, out, ctx.negative_slope, ctx.scale)
        return gradgrad_out, None, None, None, None


class FusedLeakyReLUFunction(Function):

    @staticmethod
    def forward(ctx, input, bias, negative_slope, scale):
        _check(input, bias)
        out = H.fused_bias_act(input.contiguous(), None if bias is None else bias.detach().contiguous(), None, negative_slope, scale)
        ctx.save_for_backward(out)
        ctx.negative_slope, ctx.scale, ctx.has_bias = negative_slope, scale, bias is not None
        return out

    @staticmethod
    def backward(ctx, grad_output):
        out, = ctx.saved_tensors
        grad_input, grad_bias = FusedLeakyReLUFunctionBackward.apply(grad_output, out, ctx.negative_slope, ctx.scale, ctx.has_bias)
        return grad_input, (grad_bias if ctx.has_bias else None), None, None


class FusedLeakyReLU(nn.Module):
    """The reference's module: a zero-initialised bias of ``channel`` values, then lrelu(negative_slope) * scale."""

    def __init__(self, channel, negative_slope=0.2, scale=2 ** 0.5):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(channel))
        self.negative_slope = negative_slope
        self.scale = scale

    def forward(self, input):
        return fused_leaky_relu(input, self.bias, self.negative_slope, self.scale)


def fused_leaky_relu(input, bias, negative_slope=0.2, scale=2 ** 0.5):
    return FusedLeakyReLUFunction.apply(input, bias, negative_slope, scale)
