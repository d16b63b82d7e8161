"""Autograd for SpyNet (archs/spynet_arch.py) on libsr_hip.so: ONE autograd Function for the whole network, on the GradRouter
scaffold of archs/hip_generator.py.  Only the parameters are differentiated: the frames are data.

The forward is ``net.run_forward(ref, supp, keep=...)``, which saves per level the level's ``supp``, its input block, the four
post-ReLU activations and ``up``.  The backward (include/sr_hip_flow_bwd.h) undoes the final resize when the frame is not a
multiple of 32 (the ratio scaling, then the resize adjoint), then walks the levels from fine to coarse.  In a level, with ``g`` the
gradient of the level's output flow: per conv, from the last to the first, the weight gradient (sr_conv7x7_wgrad_f32, through the
router) and then the data gradient masked by the activation that fed the conv (sr_conv7x7_dgrad_f32); after the first conv the
level-input adjoint (sr_spynet_level_input_bwd_f32) turns the gradient of the input block and ``g`` (which reaches ``up`` through
the last conv's res1) into the coarser level's ``g``.  Level 0 stops after its first conv's weight gradient: its incoming flow is
the constant zero.  Nothing below the lowest parameter that wants a gradient is run.

Frozen parameters get None; with an optim.FlatAdam arena attached (``net._grad_sink``) the gradients are added into the arena in
place.  No kernel of the backward uses an atomic: two backward passes of the same graph give bit-identical gradients.  Once
differentiable."""
import torch
from torch.autograd.function import once_differentiable

from .. import hip_ops
from .hip_generator import GradRouter


def run_backward(net, saved, dy, router):
    """The adjoint of SpyNet.run_forward with respect to the parameters: ``dy`` = dL/dflow [N, 2, h, w]."""
    h, w, h_floor, w_floor = saved['size']
    convs = [net.basic_module[level].convs() for level in range(len(saved['levels']))]
    wanted = [(level, i) for level, cs in enumerate(convs) for i, c in enumerate(cs)
              if router.to_sink or router.need_p[router.index[id(c.weight)]] or router.need_p[router.index[id(c.bias)]]]
    if not wanted:
        return
    stop = wanted[0]                        # the coarsest (level, conv) that wants a gradient: nothing below it is run
    g = dy
    if (h_floor, w_floor) != (h, w):
        ratio = torch.tensor([float(w) / float(w_floor), float(h) / float(h_floor)], dtype=torch.float32, device=dy.device)
        g = torch.empty_like(dy)
        hip_ops.launch('sr_channel_affine_f32', dy.device, dy.data_ptr(), g.data_ptr(), ratio.data_ptr(), None, dy.size(0), 2, h * w)
        g = hip_ops.resize_bilinear_adjoint(g, (h_floor, w_floor))
    g = hip_ops.nchw_to_cb8(g)              # one block: channels 0, 1, the rest 0
    for level in range(len(convs) - 1, stop[0] - 1, -1):
        sv = saved['levels'][level]
        srcs = [sv['x0']] + sv['acts']
        d = g
        for i in range(4, -1, -1):
            router.wgrad(convs[level][i], srcs[i], d)
            if (level, i) == stop or (level == 0 and i == 0):
                return
            d = hip_ops.conv7x7_dgrad(d, net.packed(convs[level][i], 1), mask=srcs[i] if i > 0 else None)
        g = hip_ops.spynet_level_input_bwd(sv['supp'], sv['up'], d, g)


class SpyNetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, ref, supp, *params):
        saved = {}
        flow = net.run_forward(ref, supp, keep=saved)
        ctx.net, ctx.saved, ctx.params = net, saved, params
        return flow

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dy = dy.contiguous().float()
        router = GradRouter(ctx.net, ctx.params, ctx.needs_input_grad[3:])
        with torch.cuda.device(dy.device):
            run_backward(ctx.net, ctx.saved, dy, router)
        return (None, None, None) + tuple(router.grads)


def spynet_apply(net, ref, supp):
    """``net(ref, supp)`` with a graph: the flow [N, 2, h, w] with a grad_fn whose backward fills the parameter gradients."""
    return SpyNetFunction.apply(net, ref, supp, *net._param_list())
