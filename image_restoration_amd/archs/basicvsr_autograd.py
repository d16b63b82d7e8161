"""Autograd for BasicVSR's propagation (archs/basicvsr_arch.py) on libsr_hip.so: ONE autograd Function over
``(x, flows_forward, flows_backward, *parameters)``, on the GradRouter scaffold of archs/hip_generator.py.  It is the second of two
chained Functions: ``get_flow`` goes through SpyNet's (archs/spynet_autograd.py) when a ``spynet.*`` parameter requires grad, the
flows then carry a grad_fn, and autograd itself feeds the flow gradients returned here into it.  The parameters and the two flow
tensors are differentiated; the frames are data.

The forward is ``net.run_forward(x, ff, fb, keep=...)``: the launches of inference, with sr_vsr_trunk_keep_f32 (the same driver) as
the trunk call.  It keeps, with fb = num_feat / 8 and per low-resolution pixel of one image of the batch:

    per frame and branch    the trunk input of the step (1 + fb blocks: the frame block and the warped feature) and the trunk's
                            stack (the first conv's output, per block the ReLU output and the block output but the last): with the
                            step's output in the per-clip feature tensor about (2 + 2 * num_block) maps of num_feat channels,
                            4 * num_feat * (2 + 2 * num_block) + 32 bytes
    per frame, the head     the fused feature (num_feat), the two shuffled maps (4 * num_feat and 16 * 64) and conv_hr's output
                            (16 * 64): 4 * (5 * num_feat + 2048) bytes

so a clip of n frames keeps about b * n * h * w * (8 * num_feat * (2 + 2 * num_block) + 20 * num_feat + 8256) bytes: 9.4 GiB for
the REDS recipe (15 frames of 64 x 64, batch 4, num_feat 64, num_block 30), 7.3 GiB of it the trunks' stacks.

The backward (include/sr_hip_vsr_bwd.h):

    1. the head, batched over all frames in the forward's chunks, written like MSRResNet's: per conv the weight gradient through
       the router, then the data gradient on the mode-1 image with the LeakyReLU mask of the saved activation as its epilogue,
       sr_cb8_pixel_unshuffle_f32 for the shuffles.  The 1x1 fusion's data gradient writes the gradient of the whole per-clip
       feature tensor in the forward's own layout; the bilinear base reaches only the frames and is not run.
    2. the forward branch from the last frame to the first, 3. the backward branch from the first frame to the last.  Per step:
       sr_vsr_trunk_bwd_f32 on that frame's window of the feature gradient (the weight gradients of the branch's shared trunk: stored
       by the first step visited, added into by the later ones, in that order, by the kernels' accumulate mode), then
       sr_vsr_prop_input_bwd_f32, which scatters the gradient of the warped feature into the previous step's window of the same
       gradient tensor and stores dflow straight into its slice of the [b, n - 1, 2, h, w] flow gradient.  The first step of a
       branch warped nothing: its trunk backward stops at the first conv's weight gradient.

A frozen parameter gets None and its weight-gradient launch is skipped; dflow is computed only when that flow input needs a
gradient; a branch with neither is not walked.  With an optim.FlatAdam arena attached (``net._grad_sink``) the gradients are added
into the arena in place.

The scatter into the previous step's window (float atomics, sr_vsr_prop_input_bwd_f32) is the ONE step of the whole backward that
is not bit-reproducible: two backward passes of the same graph agree within that kernel's bound, carried through the steps before
it, not bit for bit.  Everything else — the head, the trunk backward, dflow, SpyNet's backward — is.  With
``net.set_autograd(True, deterministic=True)`` that step is sr_vsr_prop_input_bwd_det_f32 (include/sr_hip_vsr_det.h: the same terms
summed as 64-bit integers, three launches instead of one), and two backward passes agree bit for bit.  Once differentiable."""
import torch
from torch.autograd.function import once_differentiable

from .. import hip_ops
from ..hip_ops import CB8
from .hip_generator import GradRouter

_LRELU = 0.1


def _head_backward(net, feats, dfeats, dy, acts, router):
    """The adjoint of ``_reconstruct`` on one chunk of frames: ``dy`` [s, 3, 4h, 4w] -> the chunk of the feature gradient."""
    fused, up1, up2, hr = acts
    g = hip_ops.nchw_to_cb8(dy)                # conv_last: its gradient is dy itself (the bilinear base adds)
    for conv, src in ((net.conv_last, hr), (net.conv_hr, up2)):
        router.wgrad(conv, src, g)
        g = hip_ops.conv3x3(g, net.packed(conv, 1), mask=src, mask_slope=_LRELU)
    for conv, src, channels in ((net.upconv2, up1, 64), (net.upconv1, fused, net.num_feat)):
        g = hip_ops.pixel_unshuffle(g, channels, 2)                                        # d(upconv pre-activation)
        router.wgrad(conv, src, g)
        g = hip_ops.conv3x3(g, net.packed(conv, 1), mask=src, mask_slope=_LRELU)
    router.wgrad(net.fusion, CB8(feats), g)                                                # g: d(fusion pre-activation)
    hip_ops.convd(g, net.packed(net.fusion, 1), out=CB8(dfeats))


def _branch_backward(net, trunk, steps, feats, dfeats, dtin, flows, dflows, cb0, order, router):
    """One branch against its direction.  ``order``: the frames as the forward visited them."""
    params = trunk._param_list()
    wanted = router.to_sink or any(router.need_p[router.index[id(p)]] for p in params)
    if not wanted and dflows is None:
        return
    b, fb = dtin.size(0), net.num_feat // 8
    cfg, dblob = trunk.cfg(), trunk.packed_dgrad(feats.device)
    prop_bwd = hip_ops.vsr_prop_input_bwd_det if net._deterministic else hip_ops.vsr_prop_input_bwd
    for k in range(len(order) - 1, -1, -1):
        i = order[k]
        if k == 0 and not wanted:
            break
        tin, stack = steps[i]
        targets, accumulate = router.shared_targets(params) if wanted else ((None,) * len(params), False)
        win = slice(i * b, (i + 1) * b)
        hip_ops.vsr_trunk_bwd(cfg, dblob, CB8(tin), CB8(feats[win], cb0, fb), stack, CB8(dfeats[win], cb0, fb),
                              CB8(dtin) if k > 0 else None, targets, accumulate)
        if k > 0:
            j = order[k - 1]
            pwin, at = slice(j * b, (j + 1) * b), min(i, j)
            prop_bwd(CB8(dtin, 1, fb), CB8(feats[pwin], cb0, fb), flows[:, at], CB8(dfeats[pwin], cb0, fb),
                     None if dflows is None else dflows[:, at])


def run_backward(net, saved, dy, router, need_ff, need_fb):
    """The adjoint of BasicVSR.run_forward: ``dy`` = dL/dy [b, n, 3, 4h, 4w] -> (dflows_forward, dflows_backward), each None
    unless needed; the parameter gradients go through ``router``."""
    x, feats = saved['x'], saved['feats']
    b, n, _, h, w = x.shape
    fb = net.num_feat // 8
    dy = dy.transpose(0, 1).reshape(n * b, 3, 4 * h, 4 * w)       # frame-major, as the head ran
    dfeats = torch.empty_like(feats)
    for s, e, acts in saved['head']:
        _head_backward(net, feats[s:e], dfeats[s:e], dy[s:e], acts, router)
    ff, fbw = saved['flows_forward'], saved['flows_backward']
    dff = torch.empty_like(ff) if need_ff else None
    dfb = torch.empty_like(fbw) if need_fb else None
    dtin = torch.empty((b, 1 + fb, h, w, 8), dtype=torch.float32, device=x.device)
    _branch_backward(net, net.forward_trunk, saved['forward'], feats, dfeats, dtin, ff, dff, fb, list(range(n)), router)
    _branch_backward(net, net.backward_trunk, saved['backward'], feats, dfeats, dtin, fbw, dfb, 0, list(range(n - 1, -1, -1)), router)
    return dff, dfb


class BasicVSRFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, x, flows_forward, flows_backward, *params):
        saved = {}
        y = net.run_forward(x, flows_forward.detach().contiguous(), flows_backward.detach().contiguous(), keep=saved)
        ctx.net, ctx.saved, ctx.params = net, saved, params
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dy = dy.contiguous().float()
        router = GradRouter(ctx.net, ctx.params, ctx.needs_input_grad[4:])
        with torch.cuda.device(dy.device):
            dff, dfb = run_backward(ctx.net, ctx.saved, dy, router, ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        return (None, None, dff, dfb) + tuple(router.grads)


def basicvsr_apply(net, x, flows_forward, flows_backward):
    """``net.propagate(x, flows_forward, flows_backward)`` with a graph: the output with a grad_fn whose backward fills the gradients
    of the parameters (``spynet.*`` get None here: they are reached through the flows) and of the two flow tensors."""
    return BasicVSRFunction.apply(net, x, flows_forward, flows_backward, *net._param_list())
