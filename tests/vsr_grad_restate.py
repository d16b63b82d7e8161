"""A differentiable restatement of BasicVSR's ``propagate`` in torch (float64 by default, fp32 on request) under plain autograd,
written from the definition: every activation as a product with an explicit mask, the warp as an explicit four-corner blend on
explicit cells with the fraction still differentiable.  The yardstick of the recurrent backward
(tests/test_vsr_bwd_ops_gpu.py, tests/test_basicvsr_backward_gpu.py).

The network has kinks: a ReLU or LeakyReLU flips, a warp sample changes its cell.  Two evaluations in different precisions that
fall on different sides of one kink have gradients that differ by far more than rounding, so a comparison across precisions pins
the kinks.  ``forced`` does that, in the manner of tests/spynet_grad_restate.py: the activation masks and the warp cells come from
outside (the device's own saved activations, and flow_restate.warp_coords on the fp32 flows: the kernel's rule), and the
restatement differentiates the piece of the function those select.  With ``forced=None`` it uses its own and records them, and
then it is ``vsr_restate.basicvsr_propagate`` (tests/test_vsr_bwd_host.py checks that, and its gradients against the reference's
own, tests/golden/g_zh_basicvsr_grad.npz).

Weights and clips are the seeded ones of tests/vsr_restate.py; the flows of the two cases are the fixture's
(tests/golden/g_ze_basicvsr.npz); ``grad_output`` is a seeded normal g, the loss is sum(y * g)."""
import os
import sys

import numpy as np
import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as FR  # noqa: E402
import vsr_restate as V  # noqa: E402

# (tag, b, n, h, w, num_feat, num_block): the golden case, and three channel blocks (an odd count) with one residual block
CASES = (('b1_n3_33x40', 1, 3, 33, 40, 64, 2), ('b2_n2_34x33', 2, 2, 34, 33, 24, 1))
FLOW_KEYS = ('flows_forward', 'flows_backward')


def case(tag):
    return CASES[[c[0] for c in CASES].index(tag)]


def case_data(g, tag):
    """(state dict of numpy fp32 arrays without spynet.*, clip, flows_forward, flows_backward) of a case from the fixture
    g_ze_basicvsr ``g``: its seeds, its trunk scale and its recorded flows."""
    idx = [c[0] for c in CASES].index(tag)
    _, b, n, h, w, nf, nb = CASES[idx]
    sd = V.basicvsr_weights(int(g['weight_seed']), nf, nb, float(g['trunk_scale']))
    x = V.clip_input(int(g['input_seed']) + idx, b, n, h, w)
    return sd, x, g[f'basicvsr_{tag}_flows_forward'], g[f'basicvsr_{tag}_flows_backward']


def grad_output(tag, seed=7):
    _, b, n, h, w, _, _ = case(tag)
    return np.random.default_rng(seed).standard_normal((b, n, 3, 4 * h, 4 * w))


def parameters(sd, dtype=torch.float64):
    """The weights as leaf tensors that require grad, in state_dict order."""
    return {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_() for k, v in sd.items()}


def cells_of(flow32):
    """(x0, y0) of a step from its fp32 flow [b, 2, h, w]: flow_restate.warp_coords, the kernel's rule."""
    flow32 = np.asarray(flow32, np.float32)
    h, w = flow32.shape[2:]
    x0, y0, _, _, _, _ = FR.warp_coords(np.ascontiguousarray(flow32.transpose(0, 2, 3, 1)), h, w, 'zeros')
    return x0, y0


def warp(feat, flow, cells):
    """Zeros-mode warp of ``feat`` [b, C, h, w] by ``flow`` [b, 2, h, w] on the given cells: the blend over the four corners
    written out, the fraction position - cell differentiable with respect to the flow."""
    n, _, h, w = feat.shape
    x0, y0 = (torch.from_numpy(np.asarray(a)) for a in cells)
    gy, gx = torch.meshgrid(torch.arange(h, dtype=flow.dtype), torch.arange(w, dtype=flow.dtype), indexing='ij')
    zero = torch.zeros((), dtype=flow.dtype)
    fx = gx + flow[:, 0] - x0.to(flow.dtype) if w > 1 else zero.expand(n, h, w)
    fy = gy + flow[:, 1] - y0.to(flow.dtype) if h > 1 else zero.expand(n, h, w)
    ni = torch.arange(n)[:, None, None].expand(n, h, w)

    def corner(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = feat[ni, :, yy.clamp(0, h - 1), xx.clamp(0, w - 1)]          # [b, h, w, C]
        return torch.where(ok[..., None], v, zero).permute(0, 3, 1, 2)
    v00, v01, v10, v11 = corner(y0, x0), corner(y0, x0 + 1), corner(y0 + 1, x0), corner(y0 + 1, x0 + 1)
    fx, fy = fx[:, None], fy[:, None]
    return (1 - fy) * ((1 - fx) * v00 + fx * v01) + fy * ((1 - fx) * v10 + fx * v11)


class _Masks:
    """Hands out the activation masks of one stage in order: the forced ones, or those of the evaluation itself (recorded)."""

    def __init__(self, forced, out):
        self.forced, self.out, self.k = forced, out, 0

    def act(self, pre, slope):
        m = torch.from_numpy(np.asarray(self.forced[self.k])) if self.forced is not None else pre.detach() > 0
        self.k += 1
        self.out.append(m.numpy())
        m = m.to(pre.dtype)
        return pre * (m + slope * (1 - m))


def trunk(params, prefix, x, num_block, masks):
    """ConvResidualBlocks; ``masks``: a _Masks of 1 + num_block entries (the first conv's LeakyReLU, each block's ReLU)."""
    x = masks.act(F.conv2d(x, params[f'{prefix}.main.0.weight'], params[f'{prefix}.main.0.bias'], padding=1), 0.1)
    acts = [x]
    for i in range(num_block):
        p = f'{prefix}.main.2.{i}'
        t = masks.act(F.conv2d(x, params[p + '.conv1.weight'], params[p + '.conv1.bias'], padding=1), 0.0)
        x = x + F.conv2d(t, params[p + '.conv2.weight'], params[p + '.conv2.bias'], padding=1)
        acts += [t, x]
    return x, acts


def propagate(params, x, flows_forward, flows_backward, num_block, forced=None, record=None):
    """BasicVSR.forward after get_flow in the dtype of ``params``: x numpy [b, n, 3, h, w], the flows torch tensors
    [b, n - 1, 2, h, w] (leaves that require grad, for their gradients) -> [b, n, 3, 4h, 4w].
    ``forced``: dict(masks={('backward' | 'forward', i): [1 + num_block bool arrays], ('head', i): [4 bool arrays]},
    cells={('backward' | 'forward', i): (x0, y0)}) or None; ``record`` (a dict) receives the same structure with what this
    evaluation chose itself (cells from its flows rounded to fp32)."""
    dtype = next(iter(params.values())).dtype
    xt = torch.from_numpy(np.asarray(x)).to(dtype)
    b, n, _, h, w = xt.shape
    num_feat = params['fusion.weight'].shape[0]
    rec = dict(masks={}, cells={}) if record is None else record
    rec.setdefault('masks', {})
    rec.setdefault('cells', {})

    def step(branch, i, feat, flow):
        if flow is not None:
            cells = forced['cells'][(branch, i)] if forced is not None else cells_of(flow.detach().float().numpy())
            rec['cells'][(branch, i)] = cells
            feat = warp(feat, flow, cells)
        rec['masks'][(branch, i)] = []
        masks = _Masks(None if forced is None else forced['masks'][(branch, i)], rec['masks'][(branch, i)])
        return trunk(params, f'{branch}_trunk', torch.cat([xt[:, i], feat], 1), num_block, masks)[0]

    out_l = [None] * n
    feat = torch.zeros((b, num_feat, h, w), dtype=dtype)
    for i in range(n - 1, -1, -1):
        feat = step('backward', i, feat, flows_backward[:, i] if i < n - 1 else None)
        out_l[i] = feat
    feat = torch.zeros((b, num_feat, h, w), dtype=dtype)
    outs = []
    for i in range(n):
        feat = step('forward', i, feat, flows_forward[:, i - 1] if i > 0 else None)
        rec['masks'][('head', i)] = []
        masks = _Masks(None if forced is None else forced['masks'][('head', i)], rec['masks'][('head', i)])
        out = masks.act(F.conv2d(torch.cat([out_l[i], feat], 1), params['fusion.weight'], params['fusion.bias']), 0.1)
        out = masks.act(F.pixel_shuffle(F.conv2d(out, params['upconv1.weight'], params['upconv1.bias'], padding=1), 2), 0.1)
        out = masks.act(F.pixel_shuffle(F.conv2d(out, params['upconv2.weight'], params['upconv2.bias'], padding=1), 2), 0.1)
        out = masks.act(F.conv2d(out, params['conv_hr.weight'], params['conv_hr.bias'], padding=1), 0.1)
        out = F.conv2d(out, params['conv_last.weight'], params['conv_last.bias'], padding=1)
        outs.append(out + torch.from_numpy(V.bilinear_x4(np.asarray(x[:, i], np.float64))).to(dtype))
    return torch.stack(outs, 1)


def gradients(sd, x, flows_forward, flows_backward, g, num_block, dtype=torch.float64, forced=None, record=None):
    """({name: dL/d(parameter or flow tensor) as float64 numpy}, y) for L = sum(y * g); the flows under FLOW_KEYS."""
    params = parameters(sd, dtype)
    ff = torch.from_numpy(np.asarray(flows_forward)).to(dtype).requires_grad_()
    fb = torch.from_numpy(np.asarray(flows_backward)).to(dtype).requires_grad_()
    y = propagate(params, x, ff, fb, num_block, forced, record)
    leaves = list(params.values()) + [ff, fb]
    grads = torch.autograd.grad((y * torch.from_numpy(np.asarray(g)).to(dtype)).sum(), leaves)
    return {k: v.double().numpy() for k, v in zip(list(params) + list(FLOW_KEYS), grads)}, y.detach()


def rel_l2(a, b):
    """Per tensor |a - b| / |b|."""
    return {k: float(np.linalg.norm(a[k] - b[k]) / max(np.linalg.norm(b[k]), 1e-300)) for k in b}


def cb8_to_nchw(t):
    """A device CB8 tensor [N, C / 8, H, W, 8] as numpy [N, C, H, W]."""
    n, cb, h, w, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(n, cb * 8, h, w).cpu().numpy()


# ------------------------------------------------------------------------------------------------------ the fixture
def sample_index(shape, count=1024):
    """Flat indices of a strided sample of a tensor (the whole tensor up to ``count`` elements): a stride near size / count that
    is coprime to every extent of the tensor, to 9 (the taps) and to the size, so that the 1024 samples are distinct and walk
    through every residue of co (at most 256), ci (at most 128) and the tap."""
    size = int(np.prod(shape))
    if size <= count:
        return np.arange(size, dtype=np.int64)
    step = size // count + 1            # count * step >= size: the walk reaches the end of the tensor
    while any(np.gcd(step, int(d)) != 1 for d in tuple(shape) + (9, size)):
        step += 1
    return (np.arange(count, dtype=np.int64) * step + 3) % size


def summary(grads):
    """What the fixture keeps of a set of gradients: per tensor its L2 norm and the strided sample of sample_index."""
    return {k: dict(norm=float(np.linalg.norm(v)), vals=v.reshape(-1)[sample_index(v.shape)].copy()) for k, v in grads.items()}
