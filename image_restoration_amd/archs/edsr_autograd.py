"""Autograd bridge of EDSR (fp32): ONE torch.autograd.Function for the whole network.

forward  -> the per-layer launches of EDSR.run_forward, keeping the CB8 activations the backward reads
backward -> data gradients as sr_conv3x3_f32 launches on the data-gradient weight images, the ReLU backward fused as the
            epilogue mask (mask_src = the saved ReLU output), the identity path of each residual block as the conv's res1 term and
            the long skip around the trunk as res2 of the first block's conv; sr_cb8_pixel_unshuffle_f32 for the shuffles; weight
            gradients from sr_conv3x3_wgrad_f32.  The two shifts have no parameters: the output one scales the incoming
            gradient by 1 / img_range (carried as conv_last's alpha / wgrad scale), the input one scales dL/dx by img_range
            (conv_first's alpha).

This stands where the reference relies on autograd through nn.Conv2d / ReLU / PixelShuffle (edsr_arch.py:50-61 under
sr_model.py).  Parameter gradients are returned to autograd as ordinary tensors (``requires_grad_(False)`` toggling works), or,
with an optim.FlatAdam arena attached (``net._grad_sink``), added straight into the arena (hip_generator.WholeNetFunction /
GradRouter).
"""
from .. import hip_ops
from .hip_generator import WholeNetFunction, residual_block_backward


class _EDSRFunction(WholeNetFunction):

    @staticmethod
    def run_backward(net, sv, dy, router, need_x):
        nf, nb = net.num_feat, net.num_block
        rng = float(net.img_range)
        # conv_last: y = conv / img_range + mean, so its pre-shift gradient is dy / img_range
        g = hip_ops.nchw_to_cb8(dy)
        src_last = sv['ups'][-1] if sv['ups'] else sv['trunk']
        router.wgrad(net.conv_last, src_last, g, scale=1.0 / rng)
        g = hip_ops.conv3x3(g, net.packed(net.conv_last, 1), alpha=1.0 / rng)
        # upsampling stages, last first (no activation in them)
        ups = net.ups()
        for k in range(len(ups) - 1, -1, -1):
            conv, r = ups[k]
            g = hip_ops.pixel_unshuffle(g, nf, r)
            src = sv['ups'][k - 1] if k > 0 else sv['trunk']
            router.wgrad(conv, src, g)
            g = hip_ops.conv3x3(g, net.packed(conv, 1))
        # trunk output = conv_after_body(body) + feat0: g also reaches feat0 directly (g_skip)
        g_skip = g
        body_out = sv['blocks'][-1][1] if nb > 0 else sv['feat0']
        router.wgrad(net.conv_after_body, body_out, g)
        if nb > 0:
            g = hip_ops.conv3x3(g, net.packed(net.conv_after_body, 1))
        else:
            g = hip_ops.conv3x3(g, net.packed(net.conv_after_body, 1), res1=g_skip, beta1=1.0)
        # residual blocks, last first; block 0 also takes the long skip (res2)
        for b in range(net.num_block - 1, -1, -1):
            g = residual_block_backward(net, sv, b, g, router, **(dict(res2=g_skip, beta2=1.0) if b == 0 else {}))
        router.wgrad(net.conv_first, sv['x'], g)
        if not need_x:
            return None
        # x' = (x - mean) * img_range
        return hip_ops.cb8_to_nchw(hip_ops.conv3x3(g, net.packed(net.conv_first, 1), alpha=rng), 3)


edsr_apply = _EDSRFunction.net_apply
