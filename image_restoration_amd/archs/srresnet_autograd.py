"""Autograd bridge of MSRResNet: ONE torch.autograd.Function for the whole network.

forward  -> the per-layer launches of MSRResNet.run_forward, keeping the CB8 activations the backward reads
backward -> data gradients as sr_conv3x3_f32 launches on the data-gradient weight images, the ReLU / LeakyReLU backward
            fused as the epilogue mask (mask_src = the saved activation), the identity path of each residual block as the
            conv's res1 term; sr_cb8_pixel_unshuffle_f32 for the shuffles, sr_bilinear_up_bwd_f32 for the base term;
            weight gradients from sr_conv3x3_wgrad_f32.

This stands where the reference relies on autograd through nn.Conv2d / ReLU / LeakyReLU / PixelShuffle / interpolate
(srresnet_arch.py:55-68 under sr_model.py / srgan_model.py).  Parameter gradients are returned to autograd as ordinary
tensors (``requires_grad_(False)`` toggling works), or, with an optim.FlatAdam arena attached (``net._grad_sink``), added
straight into the arena.
"""
import torch

from .. import _lib, hip_ops
from .srresnet_arch import LRELU


class _MSRResNetFunction(torch.autograd.Function):

    @staticmethod
    def forward(ctx, net, x, *params):
        y, saved = net.run_forward(x, keep=True)
        ctx.net, ctx.saved, ctx.x_shape, ctx.params = net, saved, tuple(x.shape), params
        return y

    @staticmethod
    def backward(ctx, dy):
        net, sv, params = ctx.net, ctx.saved, ctx.params
        dy = dy.contiguous().float()
        dev = dy.device
        need_x = ctx.needs_input_grad[1]
        need_p = ctx.needs_input_grad[2:]
        nf, s = net.num_feat, net.upscale
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
            # conv_last: its gradient is dy itself (the bilinear base adds, it does not scale)
            g = hip_ops.nchw_to_cb8(dy)
            i_last = len(convs) - 1
            wgrad(i_last, sv['hr'], g)
            g = hip_ops.conv3x3(g, net.packed(convs[i_last], 1), mask=sv['hr'], mask_slope=LRELU)     # d(conv_hr pre-act)
            src_hr = sv['ups'][-1]
            wgrad(i_last - 1, src_hr, g)
            g = hip_ops.conv3x3(g, net.packed(convs[i_last - 1], 1), mask=src_hr, mask_slope=LRELU)   # d(last upconv, shuffled)
            # upsampling stages, last first
            ups = net.ups()
            i_up0 = 1 + 2 * net.num_block
            for k in range(len(ups) - 1, -1, -1):
                conv, r = ups[k]
                g = hip_ops.pixel_unshuffle(g, nf, r)                                                  # d(upconv pre-act)
                src = sv['ups'][k - 1] if k > 0 else (sv['blocks'][-1][1] if sv['blocks'] else sv['feat0'])
                wgrad(i_up0 + k, src, g)
                if k > 0:
                    g = hip_ops.conv3x3(g, net.packed(conv, 1), mask=src, mask_slope=LRELU)
                elif net.num_block > 0:
                    g = hip_ops.conv3x3(g, net.packed(conv, 1))                                         # d(body output)
                else:
                    g = hip_ops.conv3x3(g, net.packed(conv, 1), mask=sv['feat0'], mask_slope=LRELU)
            # residual blocks, last first: f' = f + rs*conv2(relu(conv1(f)))
            for b in range(net.num_block - 1, -1, -1):
                blk = net.body[b]
                t, _ = sv['blocks'][b]
                f_in = sv['blocks'][b - 1][1] if b > 0 else sv['feat0']
                rs = float(blk.res_scale)
                wgrad(1 + 2 * b + 1, t, g, scale=rs)
                dt = hip_ops.conv3x3(g, net.packed(blk.conv2, 1), alpha=rs, mask=t, mask_slope=0.0)   # d(conv1 pre-act)
                wgrad(1 + 2 * b, f_in, dt)
                # d(block input) = conv1 data gradient + the identity path (res1); block 0 also takes conv_first's LeakyReLU
                if b > 0:
                    g = hip_ops.conv3x3(dt, net.packed(blk.conv1, 1), res1=g, beta1=1.0)
                else:
                    g = hip_ops.conv3x3(dt, net.packed(blk.conv1, 1), res1=g, beta1=1.0, mask=sv['feat0'], mask_slope=LRELU)
            wgrad(0, sv['x'], g)
            dx = None
            if need_x:
                dx = hip_ops.cb8_to_nchw(hip_ops.conv3x3(g, net.packed(convs[0], 1)), net.num_in_ch)
                hip_ops.bilinear_up_bwd(dy, s, out=dx)   # + the adjoint of the bilinear base
        ctx.saved = None
        return (None, dx) + tuple(grads)


def msrresnet_apply(net, x):
    return _MSRResNetFunction.apply(net, x, *net._param_list())
