"""``upfirdn2d`` / ``UpFirDn2d`` / ``upfirdn2d_native`` of the reference (basicsr/ops/upfirdn2d/upfirdn2d.py) on the HIP kernel
sr_upfirdn2d_f32 (include/sr_hip_stylegan2.h), differentiable twice.

Per plane and axis: insert ``up - 1`` zeros after each sample, pad by ``(pad0, pad1)`` (a negative pad crops), convolve with
the filter (correlate with the flipped filter), keep every ``down``-th sample; the output has
``(in * up + pad0 + pad1 - k) // down + 1`` samples.

Supported: fp32, filter sides 1..16, factors 1..8, any pads with a positive output size.  Anything else raises ValueError naming
this.  A CPU tensor takes ``upfirdn2d_native`` as in the reference; a CUDA tensor takes the kernel and never the native path.
The kernel argument gets no gradient.

Derivatives.  The operator is linear in the input, y = A x.  Its adjoint A^T g is the same operator with the factors swapped,
the filter flipped and the pads ``(k - pad0 - 1, in * up - out * down + pad0 - up + 1)`` per axis (``UpFirDn2dBackward``); the
derivative of that is A again, so the second derivative is the forward call.  A third derivative is not provided.
"""
import torch
from torch.autograd import Function
from torch.nn import functional as F

from ... import hip_ops as H

SUPPORTED = 'fp32, filter sides 1..16, factors 1..8, pads that give a positive output size'


def _check(input, kernel, up, down, pad, fp32=True):
    """Raises ValueError unless this is a supported call; returns the output size."""
    what = None
    if input.dim() != 4 or kernel.dim() != 2:
        what = f'input of rank {input.dim()} / kernel of rank {kernel.dim()} (needs NCHW and [kh, kw])'
    elif fp32 and (input.dtype != torch.float32 or kernel.dtype != torch.float32):
        what = f'input {input.dtype} / kernel {kernel.dtype}'
    elif not all(1 <= k <= 16 for k in kernel.shape):
        what = f'filter {tuple(kernel.shape)}'
    elif not all(isinstance(f, int) and 1 <= f <= 8 for f in (*up, *down)):
        what = f'up {tuple(up)} / down {tuple(down)}'
    if what is None:
        oh, ow = H.upfirdn2d_out_size(input.size(2), input.size(3), kernel.size(0), kernel.size(1), up, down, pad)
        if oh > 0 and ow > 0:
            return oh, ow
        what = f'output size {oh}x{ow} (input {tuple(input.shape[2:])}, filter {tuple(kernel.shape)}, up {tuple(up)}, down {tuple(down)}, ' \
               f'pad {tuple(pad)})'
    raise ValueError(f'upfirdn2d: {what} is not supported; supported: {SUPPORTED}')


def grad_pad(in_size, out_size, kernel_size, up, down, pad):
    """The pads (x0, x1, y0, y1) with which the factor-swapped, filter-flipped call is the adjoint.  Sizes are (h, w)."""
    (in_h, in_w), (out_h, out_w), (kh, kw) = in_size, out_size, kernel_size
    return (kw - pad[0] - 1, in_w * up[0] - out_w * down[0] + pad[0] - up[0] + 1,
            kh - pad[2] - 1, in_h * up[1] - out_h * down[1] + pad[2] - up[1] + 1)


class UpFirDn2dBackward(Function):
    """grad_input = A^T grad_output: sr_upfirdn2d_f32 with (down, up) for (up, down), the flipped filter and ``g_pad``.  Its own
    backward is the forward operator on the incoming second-order gradient."""

    @staticmethod
    def forward(ctx, grad_output, kernel, grad_kernel, up, down, pad, g_pad, in_size, out_size):
        ctx.save_for_backward(kernel)
        ctx.up, ctx.down, ctx.pad = up, down, pad
        grad_input = H.upfirdn2d(grad_output.contiguous(), grad_kernel, down, up, g_pad)
        if tuple(grad_input.shape) != tuple(in_size):
            raise RuntimeError(f'upfirdn2d: gradient of shape {tuple(grad_input.shape)} for an input of shape {tuple(in_size)}')
        return grad_input

    @staticmethod
    def backward(ctx, gradgrad_input):
        kernel, = ctx.saved_tensors
        return (H.upfirdn2d(gradgrad_input.contiguous(), kernel, ctx.up, ctx.down, ctx.pad),) + (None,) * 8


class UpFirDn2d(Function):
    """``UpFirDn2d.apply(input, kernel, (ux, uy), (dx, dy), (px0, px1, py0, py1))`` on a CUDA tensor (a CPU tensor is an
    SrHipError: the kernel has no CPU fallback; ``upfirdn2d`` sends CPU tensors to ``upfirdn2d_native``)."""

    @staticmethod
    def forward(ctx, input, kernel, up, down, pad):
        up, down, pad = tuple(up), tuple(down), tuple(pad)
        out_size = _check(input, kernel, up, down, pad)
        kernel = kernel.detach().contiguous()
        ctx.save_for_backward(kernel, torch.flip(kernel, [0, 1]).contiguous())
        ctx.up, ctx.down, ctx.pad, ctx.in_size, ctx.out_size = up, down, pad, tuple(input.shape), out_size
        ctx.g_pad = grad_pad(input.shape[2:], out_size, kernel.shape, up, down, pad)
        return H.upfirdn2d(input.contiguous(), kernel, up, down, pad)

    @staticmethod
    def backward(ctx, grad_output):
        kernel, grad_kernel = ctx.saved_tensors
        grad_input = UpFirDn2dBackward.apply(grad_output, kernel, grad_kernel, ctx.up, ctx.down, ctx.pad, ctx.g_pad, ctx.in_size,
                                             ctx.out_size)
        return grad_input, None, None, None, None


def upfirdn2d(input, kernel, up=1, down=1, pad=(0, 0)):
    """The reference's ``upfirdn2d``: one factor and one pad pair for both axes."""
    if input.device.type == 'cpu':
        _check(input, kernel, (up, up), (down, down), (pad[0], pad[1], pad[0], pad[1]))
        return upfirdn2d_native(input, kernel, up, up, down, down, pad[0], pad[1], pad[0], pad[1])
    return UpFirDn2d.apply(input, kernel, (up, up), (down, down), (pad[0], pad[1], pad[0], pad[1]))


def upfirdn2d_native(input, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1):
    """The definition in plain torch, for any floating dtype and device: a zero tensor of the up-sampled, padded size that
    receives the samples at their strided positions (a negative pad shifts and crops), one conv2d with the flipped filter over
    the planes as a batch, then the strided selection."""
    out_h, out_w = _check(input, kernel, (up_x, up_y), (down_x, down_y), (pad_x0, pad_x1, pad_y0, pad_y1), fp32=False)
    n, c, in_h, in_w = input.shape
    kh, kw = kernel.shape
    ph, pw = in_h * up_y + pad_y0 + pad_y1, in_w * up_x + pad_x0 + pad_x1
    # sample (sy, sx) sits at (sy * up_y + pad_y0, sx * up_x + pad_x0) of the padded plane when that lies inside it
    ys = torch.arange(in_h, device=input.device) * up_y + pad_y0
    xs = torch.arange(in_w, device=input.device) * up_x + pad_x0
    ky, kx = (ys >= 0) & (ys < ph), (xs >= 0) & (xs < pw)
    padded = input.new_zeros((n * c, 1, ph, pw))
    padded[:, 0, ys[ky][:, None], xs[kx][None, :]] = input.reshape(n * c, in_h, in_w)[:, ky][:, :, kx]
    full = F.conv2d(padded, torch.flip(kernel, [0, 1]).to(input.dtype).view(1, 1, kh, kw))
    return full[:, :, ::down_y, ::down_x].reshape(n, c, out_h, out_w)
