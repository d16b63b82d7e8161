"""``flow_warp(x, flow, interp_mode='bilinear', padding_mode='zeros', align_corners=True)`` with the reference's signature.

The reference adds the flow to a pixel grid, normalises to [-1, 1] by ``max(size - 1, 1)`` and calls F.grid_sample with
``align_corners=True``, which un-normalises by ``(size - 1) / 2``: the sampling position is the pixel position plus the flow,
except on an axis of size 1, where it is 0 whatever the flow says.  Device tensors take sr_flow_warp_f32 /
sr_flow_warp_bwd_f32 (never a torch path); CPU tensors take ``flow_warp_native``, plain torch written from that definition.
Supported: fp32, bilinear, zeros or border padding, align_corners=True; everything else is a ValueError.
"""
import torch
from torch.autograd import Function

from ... import hip_ops as H

_SUPPORTED = "supported: fp32, interp_mode='bilinear', padding_mode 'zeros' or 'border', align_corners=True"


def _check(x, flow, interp_mode, padding_mode, align_corners):
    if x.dtype != torch.float32 or flow.dtype != torch.float32:
        raise ValueError(f'flow_warp: {x.dtype} / {flow.dtype} input is not supported; {_SUPPORTED}')
    if interp_mode != 'bilinear':
        raise ValueError(f"flow_warp: interp_mode '{interp_mode}' is not supported; {_SUPPORTED}")
    if padding_mode not in ('zeros', 'border'):
        raise ValueError(f"flow_warp: padding_mode '{padding_mode}' is not supported; {_SUPPORTED}")
    if align_corners is not True:
        raise ValueError(f'flow_warp: align_corners={align_corners} is not supported; {_SUPPORTED}')
    if x.dim() != 4 or flow.dim() != 4 or flow.size(3) != 2 or flow.size(0) != x.size(0):
        raise ValueError(f'flow_warp: expected x [N, C, H, W] and flow [N, H, W, 2], got {tuple(x.shape)} and {tuple(flow.shape)}')
    if tuple(x.shape[-2:]) != tuple(flow.shape[1:3]):
        raise ValueError(f'flow_warp: the flow is {flow.size(1)}x{flow.size(2)}, x is {x.size(2)}x{x.size(3)}; they must agree')


def flow_warp_native(x, flow, padding_mode='zeros'):
    """The definition in plain torch (differentiable by autograd): explicit corner sums, no grid_sample."""
    n, c, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(h, dtype=x.dtype, device=x.device), torch.arange(w, dtype=x.dtype, device=x.device),
                            indexing='ij')
    never = torch.zeros((n, h, w), dtype=torch.bool, device=x.device)   # an axis of size 1: position 0, gradient 0, still in the graph
    ix = gx + flow[..., 0] if w > 1 else torch.where(never, flow[..., 0], torch.zeros_like(flow[..., 0]))
    iy = gy + flow[..., 1] if h > 1 else torch.where(never, flow[..., 1], torch.zeros_like(flow[..., 1]))
    if padding_mode == 'border':
        ix, iy = ix.clamp(0, w - 1), iy.clamp(0, h - 1)
    x0, y0 = ix.detach().floor(), iy.detach().floor()
    fx, fy = (ix - x0).unsqueeze(1), (iy - y0).unsqueeze(1)
    flat = x.reshape(n, c, h * w)

    def corner(yy, xx):
        ok = ((xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)).unsqueeze(1)
        idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).long().reshape(n, 1, h * w).expand(n, c, h * w)
        v = flat.gather(2, idx).reshape(n, c, h, w)
        return torch.where(ok, v, torch.zeros_like(v))

    top = (1 - fx) * corner(y0, x0) + fx * corner(y0, x0 + 1)
    bot = (1 - fx) * corner(y0 + 1, x0) + fx * corner(y0 + 1, x0 + 1)
    return (1 - fy) * top + fy * bot


class FlowWarp(Function):
    """sr_flow_warp_f32 and its gradients sr_flow_warp_bwd_f32 (dx by float atomics, dflow a gather); saves x and flow."""

    @staticmethod
    def forward(ctx, x, flow, padding_mode):
        x, flow = x.contiguous(), flow.contiguous()
        ctx.save_for_backward(x, flow)
        ctx.padding_mode = padding_mode
        return H.flow_warp(x, flow, padding_mode)

    @staticmethod
    def backward(ctx, g):
        x, flow = ctx.saved_tensors
        dx, dflow = H.flow_warp_bwd(x, flow, g.contiguous(), ctx.padding_mode, want_dx=ctx.needs_input_grad[0],
                                    want_dflow=ctx.needs_input_grad[1])
        return dx, dflow, None


def flow_warp(x, flow, interp_mode='bilinear', padding_mode='zeros', align_corners=True):
    """Warp an image or feature map ``x`` (n, c, h, w) with the optical flow ``flow`` (n, h, w, 2), in pixels."""
    _check(x, flow, interp_mode, padding_mode, align_corners)
    if x.is_cuda != flow.is_cuda:
        raise ValueError(f'flow_warp: x is on {x.device}, flow on {flow.device}')
    if not x.is_cuda:
        return flow_warp_native(x, flow, padding_mode)
    return FlowWarp.apply(x, flow, padding_mode)
