"""Autograd bridge of RIDNet: ONE torch.autograd.Function for the whole network.

forward  -> the per-layer launches of RIDNet.run_forward, keeping every CB8 activation and attention statistic the backward reads
backward -> sr_ridnet_add_mean_bwd_f32 (add_mean's dW / db and the tail gradient), then per EAM, last first:
            sr_ca_bwd_f32 + sr_ca_bwd_apply_f32 (res_scale 1) and sr_cb8_relu_mask_f32 (the ReLU after block2's add, masked by the
            block output itself); the data gradients of every conv with the ReLU masks fused from the saved outputs
            (mask_src, slope 0) and the identity paths as res1 / accumulate; weight gradients from sr_conv3x3_wgrad_f32 (dense
            3x3) and sr_convd_wgrad_f32 (dilated, 1x1); finally sr_ridnet_sub_mean_bwd_f32 (sub_mean's dW / db, and dL/dx with the
            global residual).

This stands where the reference relies on autograd through nn.Conv2d / ReLU / cat / AdaptiveAvgPool2d / Sigmoid
(ridnet_arch.py:8-180 under sr_model.py).  Parameter gradients go back to autograd as ordinary tensors (``requires_grad_(False)``
toggling works) or, with an optim.FlatAdam arena attached (``net._grad_sink``), are added straight into the arena
(hip_generator.WholeNetFunction / GradRouter).
"""
from .. import hip_ops
from .hip_generator import WholeNetFunction


class _RIDNetFunction(WholeNetFunction):

    @staticmethod
    def run_backward(net, sv, dy, router, need_x):
        mid = net.mid_channels
        wgrad, targets = router.wgrad, router.targets
        (dwa, dba), acc = targets((net.add_mean.weight, net.add_mean.bias))
        g_t = hip_ops.ridnet_add_mean_bwd(dy, sv['tail'], net.add_mean.weight, dwa, dba, acc)     # dL/d(tail output)
        wgrad(net.tail, sv['feat'], g_t)
        g = hip_ops.conv3x3(g_t, net.packed(net.tail, 1))                                          # dL/d(body output)
        del g_t
        eams = list(net.body)
        for k in range(len(eams) - 1, -1, -1):
            eam, e = eams[k], sv['eams'][k]
            mg, b1p, b2p, ca = eam.merge, eam.block1, eam.block2, eam.ca
            # channel attention out = b2 * s(b2); b2 = relu(conv1x1(u2) + b1)
            (dw1, db1, dw2, db2), acc = targets((ca.fc1.weight, ca.fc1.bias, ca.fc2.weight, ca.fc2.bias))
            q = hip_ops.ca_bwd(g, e['b2'], 1.0, ca.fc1.weight, ca.fc2.weight, e['p'], e['hb'], e['s'], grads=(dw1, db1, dw2, db2),
                               accumulate=acc)
            g2 = hip_ops.ca_bwd_apply(g, e['s'], q, 1.0)
            g2 = hip_ops.relu_mask(g2, e['b2'], out=g2)                      # dL/d(block2's pre-activation sum)
            wgrad(b2p.body[4], e['u2'], g2)
            gu2 = hip_ops.convd(g2, net.packed(b2p.body[4], 1), 1, mask=e['u2'], mask_slope=0.0)
            wgrad(b2p.body[2], e['u1'], gu2)
            gu1 = hip_ops.conv3x3(gu2, net.packed(b2p.body[2], 1), mask=e['u1'], mask_slope=0.0)
            del gu2
            wgrad(b2p.body[0], e['b1'], gu1)
            # block1 output b1 = relu(conv2(t) + m) feeds block2's body and its identity
            gb1 = hip_ops.conv3x3(gu1, net.packed(b2p.body[0], 1), res1=g2, beta1=1.0, mask=e['b1'], mask_slope=0.0)
            del gu1, g2
            wgrad(b1p.conv2, e['t'], gb1)
            gt = hip_ops.conv3x3(gb1, net.packed(b1p.conv2, 1), mask=e['t'], mask_slope=0.0)
            wgrad(b1p.conv1, e['m'], gt)
            gm = hip_ops.conv3x3(gt, net.packed(b1p.conv1, 1), res1=gb1, beta1=1.0)   # dL/dm, m = relu(agg conv) + f_in
            del gt, gb1
            gagg = hip_ops.relu_mask(gm, e['agg'])
            wgrad(mg.aggregation[0], e['cat'], gagg)
            gcat = hip_ops.conv3x3(gagg, net.packed(mg.aggregation[0], 1), mask=e['cat'], mask_slope=0.0)
            del gagg
            g1b, g2b = gcat.slice(0, mid), gcat.slice(mid, mid)
            wgrad(mg.dilation1[2], e['d1a'], g1b, dilation=2)
            gd1a = hip_ops.convd(g1b, net.packed(mg.dilation1[2], 1), 2, mask=e['d1a'], mask_slope=0.0)
            wgrad(mg.dilation2[2], e['d2a'], g2b, dilation=4)
            gd2a = hip_ops.convd(g2b, net.packed(mg.dilation2[2], 1), 4, mask=e['d2a'], mask_slope=0.0)
            del gcat, g1b, g2b
            f_in = e['f_in']
            wgrad(mg.dilation1[0], f_in, gd1a)
            wgrad(mg.dilation2[0], f_in, gd2a, dilation=3)
            # dL/d(EAM input) = identity (gm) + both branches; the first EAM's input is relu(head), masked here
            g = hip_ops.conv3x3(gd1a, net.packed(mg.dilation1[0], 1), res1=gm, beta1=1.0)
            hip_ops.convd(gd2a, net.packed(mg.dilation2[0], 1), 3, out=g, accumulate=True,
                          mask=sv['head'] if k == 0 else None, mask_slope=0.0)
            del gd1a, gd2a, gm
        wgrad(net.head, sv['s'], g)
        g_s = hip_ops.conv3x3(g, net.packed(net.head, 1))                                          # dL/d(sub_mean output)
        (dws, dbs), acc = targets((net.sub_mean.weight, net.sub_mean.bias))
        return hip_ops.ridnet_sub_mean_bwd(sv['x'], g_s, net.sub_mean.weight, dws, dbs, acc, want_dx=need_x,
                                           dx_res=dy if need_x else None)


ridnet_apply = _RIDNetFunction.net_apply
