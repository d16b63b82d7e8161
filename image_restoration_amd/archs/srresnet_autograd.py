"""Autograd bridge of MSRResNet: ONE torch.autograd.Function for the whole network.

forward  -> the per-layer launches of MSRResNet.run_forward, keeping the CB8 activations the backward reads
backward -> data gradients as sr_conv3x3_f32 launches on the data-gradient weight images, the ReLU / LeakyReLU backward
            fused as the epilogue mask (mask_src = the saved activation), the identity path of each residual block as the
            conv's res1 term; sr_cb8_pixel_unshuffle_f32 for the shuffles, sr_bilinear_up_bwd_f32 for the base term;
            weight gradients from sr_conv3x3_wgrad_f32.

This stands where the reference relies on autograd through nn.Conv2d / ReLU / LeakyReLU / PixelShuffle / interpolate
(srresnet_arch.py:55-68 under sr_model.py / srgan_model.py).  Parameter gradients are returned to autograd as ordinary
tensors (``requires_grad_(False)`` toggling works), or, with an optim.FlatAdam arena attached (``net._grad_sink``), added
straight into the arena (hip_generator.WholeNetFunction / GradRouter).
"""
from .. import hip_ops
from .hip_generator import WholeNetFunction, residual_block_backward
from .srresnet_arch import LRELU


class _MSRResNetFunction(WholeNetFunction):

    @staticmethod
    def run_backward(net, sv, dy, router, need_x):
        nf, s = net.num_feat, net.upscale
        # conv_last: its gradient is dy itself (the bilinear base adds, it does not scale)
        g = hip_ops.nchw_to_cb8(dy)
        router.wgrad(net.conv_last, sv['hr'], g)
        g = hip_ops.conv3x3(g, net.packed(net.conv_last, 1), mask=sv['hr'], mask_slope=LRELU)     # d(conv_hr pre-act)
        src_hr = sv['ups'][-1]
        router.wgrad(net.conv_hr, src_hr, g)
        g = hip_ops.conv3x3(g, net.packed(net.conv_hr, 1), mask=src_hr, mask_slope=LRELU)         # d(last upconv, shuffled)
        # upsampling stages, last first
        ups = net.ups()
        for k in range(len(ups) - 1, -1, -1):
            conv, r = ups[k]
            g = hip_ops.pixel_unshuffle(g, nf, r)                                                  # d(upconv pre-act)
            src = sv['ups'][k - 1] if k > 0 else (sv['blocks'][-1][1] if sv['blocks'] else sv['feat0'])
            router.wgrad(conv, src, g)
            if k > 0:
                g = hip_ops.conv3x3(g, net.packed(conv, 1), mask=src, mask_slope=LRELU)
            elif net.num_block > 0:
                g = hip_ops.conv3x3(g, net.packed(conv, 1))                                         # d(body output)
            else:
                g = hip_ops.conv3x3(g, net.packed(conv, 1), mask=sv['feat0'], mask_slope=LRELU)
        # residual blocks, last first; block 0 also takes conv_first's LeakyReLU
        for b in range(net.num_block - 1, -1, -1):
            g = residual_block_backward(net, sv, b, g, router, **(dict(mask=sv['feat0'], mask_slope=LRELU) if b == 0 else {}))
        router.wgrad(net.conv_first, sv['x'], g)
        if not need_x:
            return None
        dx = hip_ops.cb8_to_nchw(hip_ops.conv3x3(g, net.packed(net.conv_first, 1)), net.num_in_ch)
        return hip_ops.bilinear_up_bwd(dy, s, out=dx)   # + the adjoint of the bilinear base


msrresnet_apply = _MSRResNetFunction.net_apply
