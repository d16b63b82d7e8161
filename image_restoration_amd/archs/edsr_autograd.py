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
with an optim.FlatAdam arena attached (``net._grad_sink``), added straight into the arena.
"""
import torch

from .. import _lib, hip_ops


class _EDSRFunction(torch.autograd.Function):

    @staticmethod
    def forward(ctx, net, x, *params):
        y, saved = net.run_forward(x, keep=True)
        ctx.net, ctx.saved, ctx.params = net, saved, params
        return y

    @staticmethod
    def backward(ctx, dy):
        net, sv, params = ctx.net, ctx.saved, ctx.params
        dy = dy.contiguous().float()
        dev = dy.device
        need_x = ctx.needs_input_grad[1]
        need_p = ctx.needs_input_grad[2:]
        nf, nb = net.num_feat, net.num_block
        rng = float(net.img_range)
        convs = net.convs()
        sink = getattr(net, '_grad_sink', None)
        grads = [None] * len(params)
        to_sink = sink is not None and any(need_p)
        if to_sink and not all(need_p):
            raise _lib.SrHipError('flat-arena mode needs every generator parameter to require grad')

        def wgrad(i, src, d, scale=1.0):
            """weight / bias gradient of conv i (state_dict order) from its source and its pre-activation output gradient."""
            conv = convs[i]
            iw, ib = 2 * i, 2 * i + 1
            if to_sink:
                hip_ops.conv3x3_wgrad(src, d, conv.out_channels, conv.in_channels, scale=scale,
                                      out=(sink.grad_ptrs[iw], sink.grad_ptrs[ib]))
            elif need_p[iw] or need_p[ib]:
                dw, db = hip_ops.conv3x3_wgrad(src, d, conv.out_channels, conv.in_channels, scale=scale)
                grads[iw] = dw if need_p[iw] else None
                grads[ib] = db if need_p[ib] else None

        with torch.cuda.device(dev):
            # conv_last: y = conv / img_range + mean, so its pre-shift gradient is dy / img_range
            g = hip_ops.nchw_to_cb8(dy)
            i_last = len(convs) - 1
            src_last = sv['ups'][-1] if sv['ups'] else sv['trunk']
            wgrad(i_last, src_last, g, scale=1.0 / rng)
            g = hip_ops.conv3x3(g, net.packed(convs[i_last], 1), alpha=1.0 / rng)
            # upsampling stages, last first (no activation in them)
            ups = net.ups()
            i_up0 = 2 + 2 * nb
            for k in range(len(ups) - 1, -1, -1):
                conv, r = ups[k]
                g = hip_ops.pixel_unshuffle(g, nf, r)
                src = sv['ups'][k - 1] if k > 0 else sv['trunk']
                wgrad(i_up0 + k, src, g)
                g = hip_ops.conv3x3(g, net.packed(conv, 1))
            # trunk output = conv_after_body(body) + feat0: g also reaches feat0 directly (g_skip)
            g_skip = g
            body_out = sv['blocks'][-1][1] if nb > 0 else sv['feat0']
            wgrad(1 + 2 * nb, body_out, g)
            if nb > 0:
                g = hip_ops.conv3x3(g, net.packed(net.conv_after_body, 1))
            else:
                g = hip_ops.conv3x3(g, net.packed(net.conv_after_body, 1), res1=g_skip, beta1=1.0)
            # residual blocks, last first: f' = f + rs*conv2(relu(conv1(f)))
            for b in range(nb - 1, -1, -1):
                blk = net.body[b]
                t, _ = sv['blocks'][b]
                f_in = sv['blocks'][b - 1][1] if b > 0 else sv['feat0']
                rs = float(blk.res_scale)
                wgrad(1 + 2 * b + 1, t, g, scale=rs)
                dt = hip_ops.conv3x3(g, net.packed(blk.conv2, 1), alpha=rs, mask=t, mask_slope=0.0)   # d(conv1 pre-act)
                wgrad(1 + 2 * b, f_in, dt)
                # d(block input) = conv1 data gradient + the identity path (res1); block 0 also takes the long skip (res2)
                if b > 0:
                    g = hip_ops.conv3x3(dt, net.packed(blk.conv1, 1), res1=g, beta1=1.0)
                else:
                    g = hip_ops.conv3x3(dt, net.packed(blk.conv1, 1), res1=g, beta1=1.0, res2=g_skip, beta2=1.0)
            wgrad(0, sv['x'], g)
            dx = None
            if need_x:
                # x' = (x - mean) * img_range
                dx = hip_ops.cb8_to_nchw(hip_ops.conv3x3(g, net.packed(convs[0], 1), alpha=rng), 3)
        ctx.saved = None
        return (None, dx) + tuple(grads)


def edsr_apply(net, x):
    return _EDSRFunction.apply(net, x, *net._param_list())
