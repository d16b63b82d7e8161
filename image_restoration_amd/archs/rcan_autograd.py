"""Autograd bridge of RCAN: ONE torch.autograd.Function for the whole network.

forward  -> the per-layer launches of RCAN.run_forward, keeping the CB8 activations and attention statistics the backward reads
backward -> per RCAB, last first: sr_ca_bwd_f32 (sum_hw g*u, the sigmoid / W2 / ReLU / W1 adjoints, the attention's weight
            gradients), sr_ca_bwd_apply_f32 (the gradient at conv 2's output), conv 2's data gradient with the ReLU mask fused
            (mask_src = the saved conv 0 output), conv 0's data gradient with the block's identity path as res1 (and, for the
            first block of a group, the group's identity path as res2); sr_cb8_pixel_unshuffle_f32 for the shuffles; weight
            gradients from sr_conv3x3_wgrad_f32.

This stands where the reference relies on autograd through nn.Conv2d / ReLU / AdaptiveAvgPool2d / Sigmoid / PixelShuffle
(rcan_arch.py:8-135 under sr_model.py).  Parameter gradients are returned to autograd as ordinary tensors
(``requires_grad_(False)`` toggling works), or, with an optim.FlatAdam arena attached (``net._grad_sink``), added straight into
the arena (hip_generator.WholeNetFunction / GradRouter).
"""
from .. import hip_ops
from .hip_generator import WholeNetFunction


class _RCANFunction(WholeNetFunction):

    @staticmethod
    def run_backward(net, sv, dy, router, need_x):
        nf = net.num_feat
        wgrad = router.wgrad
        af = net.affine(dy.device)
        g = hip_ops.nchw_to_cb8(net._channel_affine(dy, af['out_a'], None))   # d(conv_last output) = dy / img_range
        feat_last = sv['ups'][-1]
        wgrad(net.conv_last, feat_last, g)
        g = hip_ops.conv3x3(g, net.packed(net.conv_last, 1))
        ups = net.ups()
        for k in range(len(ups) - 1, -1, -1):
            conv, r = ups[k]
            g = hip_ops.pixel_unshuffle(g, nf, r)
            src = sv['ups'][k - 1] if k > 0 else sv['res']
            wgrad(conv, src, g)
            g = hip_ops.conv3x3(g, net.packed(conv, 1))
        g_res = g                                                   # dL/d(conv_after_body output + x0)
        groups = net.blocks()
        wgrad(net.conv_after_body, sv['body'], g_res)
        g = hip_ops.conv3x3(g_res, net.packed(net.conv_after_body, 1))
        for gi in range(len(groups) - 1, -1, -1):
            grp, rcabs = groups[gi]
            g_in, blocks = sv['groups'][gi]
            g_grp = g                                               # dL/d(group output): also the group identity's gradient
            wgrad(grp.conv, blocks[-1][5], g_grp)
            g = hip_ops.conv3x3(g_grp, net.packed(grp.conv, 1))
            for b in range(len(rcabs) - 1, -1, -1):
                blk = rcabs[b]
                t, u, p, hb, s, _ = blocks[b]
                f_in = blocks[b - 1][5] if b > 0 else g_in
                rs = float(blk.res_scale)
                ca = blk.ca
                # (dW1, db1, dW2, db2) destinations of the channel attention's parameters, and whether they accumulate
                targets, acc = router.targets((ca.fc1.weight, ca.fc1.bias, ca.fc2.weight, ca.fc2.bias))
                q = hip_ops.ca_bwd(g, u, rs, ca.fc1.weight, ca.fc2.weight, p, hb, s, grads=targets, accumulate=acc)
                du = hip_ops.ca_bwd_apply(g, s, q, rs)
                wgrad(blk.conv2, t, du)
                dt = hip_ops.conv3x3(du, net.packed(blk.conv2, 1), mask=t, mask_slope=0.0)
                del du
                wgrad(blk.conv1, f_in, dt)
                # d(block input) = conv 0's data gradient + the block identity (res1) [+ the group identity (res2)]
                if b > 0:
                    g = hip_ops.conv3x3(dt, net.packed(blk.conv1, 1), res1=g, beta1=1.0)
                elif gi > 0:
                    g = hip_ops.conv3x3(dt, net.packed(blk.conv1, 1), res1=g, beta1=1.0, res2=g_grp, beta2=1.0)
                else:   # group 0's input is conv_first's output, whose long skip to conv_after_body adds g_res as well
                    g = hip_ops.conv3x3(dt, net.packed(blk.conv1, 1), out=g_res, accumulate=True, res1=g, beta1=1.0,
                                        res2=g_grp, beta2=1.0)
        wgrad(net.conv_first, sv['x'], g)
        if not need_x:
            return None
        dxs = hip_ops.cb8_to_nchw(hip_ops.conv3x3(g, net.packed(net.conv_first, 1)), net.num_in_ch)
        return net._channel_affine(dxs, af['in_a'], None)            # d/dx of (x - mean) * img_range


rcan_apply = _RCANFunction.net_apply
