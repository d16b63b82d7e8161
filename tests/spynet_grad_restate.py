"""A differentiable restatement of SpyNet in torch (float64 by default), written from the definition: the ReLU as a product with an
explicit mask, the warp as an explicit four-corner blend on explicit cells, the upsampling and the final resize as products with
the matrices their coordinate rules define.  The yardstick of SpyNet's backward (tests/test_spynet_backward_gpu.py).

SpyNet has kinks: a ReLU flips, a warp sample changes its cell or crosses the border.  Two evaluations in different precisions
that fall on different sides of one kink have gradients that differ by far more than rounding, so a comparison across precisions
has to pin the kinks.  ``forced`` does that: per level the four ReLU masks and the warp's cells and clip flags come from outside
(from the device's own saved activations and ``up``), and the restatement differentiates the piece of the function those select.
With ``forced=None`` it uses its own, and then it is SpyNet itself: ``tests/test_flow_bwd_host.py`` checks its forward against
flow_restate.spynet and its gradients against plain torch autograd (F.relu, F.grid_sample, F.interpolate), and against the
reference's own float64 gradients (tests/golden/g_zg_spynet_grad.npz).

The rule for cells and clip flags is flow_restate.warp_coords on the fp32 flow: the kernel's rule."""
import os
import sys

import numpy as np
import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as R  # noqa: E402

WEIGHT_SEED = 20260           # the seeded weights and inputs of tests/golden/g_zd_spynet.npz (tools/make_golden_spynet.py)
INPUT_SEED = 77
LAST_SCALE = 16.0
CASES = (('b2_64x64', 2, 64, 64), ('96x64', 1, 96, 64), ('64x96', 1, 64, 96), ('70x90', 1, 70, 90))
GRAD_CASES = ('b2_64x64', '96x64', '70x90')


def case_inputs(tag):
    i = [c[0] for c in CASES].index(tag)
    _, n, h, w = CASES[i]
    return R.spynet_inputs(INPUT_SEED + i, n, h, w)


def parameters(dtype=torch.float64, seed=WEIGHT_SEED):
    """The seeded weights as leaf tensors that require grad (the buffers mean / std left out), in state_dict order."""
    sd = R.spynet_weights(seed, LAST_SCALE)
    return {k: torch.from_numpy(v).to(dtype).requires_grad_() for k, v in sd.items() if k not in ('mean', 'std')}


def grad_output(tag, seed=5):
    _, n, h, w = CASES[[c[0] for c in CASES].index(tag)]
    return np.random.default_rng(seed).standard_normal((n, 2, h, w))


def _up_matrix(n_out):
    n_in = n_out // 2
    u = np.zeros((n_out, n_in))
    for d in range(n_out):
        s = d * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        i0 = min(int(s), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        u[d, i0] += 1.0 - (s - i0)
        u[d, i1] += s - i0
    return u


def _resize_matrix(n_in, n_out):
    r = np.zeros((n_out, n_in))
    for d in range(n_out):
        s = max((d + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = min(int(np.floor(s)), n_in - 1)
        f = 0.0 if i0 >= n_in - 1 else s - i0
        r[d, i0] += 1.0 - f
        r[d, min(i0 + 1, n_in - 1)] += f
    return r


def cells_of(up32):
    """(x0, y0, gx_on, gy_on) of a level from its fp32 ``up`` [N, 2, H, W]: flow_restate.warp_coords, the kernel's rule."""
    up32 = np.asarray(up32, np.float32)
    h, w = up32.shape[2:]
    x0, y0, _, _, gx_on, gy_on = R.warp_coords(np.ascontiguousarray(up32.transpose(0, 2, 3, 1)), h, w, 'border')
    return x0, y0, gx_on, gy_on


def _warp(supp, up, cells):
    """Border-mode warp of the constant ``supp`` [N, 3, H, W] by ``up`` on the given cells: where an axis is clipped its fraction
    is the constant 0 (the clipped position is a cell corner), elsewhere position - cell."""
    n, _, h, w = supp.shape
    x0, y0, gx_on, gy_on = (torch.from_numpy(np.asarray(a)) for a in cells)
    gy, gx = torch.meshgrid(torch.arange(h, dtype=up.dtype), torch.arange(w, dtype=up.dtype), indexing='ij')
    zero = torch.zeros((), dtype=up.dtype)
    fx = torch.where(gx_on, gx + up[:, 0] - x0.to(up.dtype), zero) if w > 1 else zero.expand(n, h, w)
    fy = torch.where(gy_on, gy + up[:, 1] - y0.to(up.dtype), zero) if h > 1 else zero.expand(n, h, w)
    ni = torch.arange(n)[:, None, None].expand(n, h, w)

    def corner(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = supp[ni, :, yy.clamp(0, h - 1), xx.clamp(0, w - 1)]          # [N, H, W, 3]
        return torch.where(ok[..., None], v, zero).permute(0, 3, 1, 2)
    v00, v01, v10, v11 = corner(y0, x0), corner(y0, x0 + 1), corner(y0 + 1, x0), corner(y0 + 1, x0 + 1)
    fx, fy = fx[:, None], fy[:, None]
    return (1 - fy) * ((1 - fx) * v00 + fx * v01) + fy * ((1 - fx) * v10 + fx * v11)


def spynet(params, ref, supp, forced=None, record=None):
    """The flow [N, 2, h, w] in the dtype of ``params``.  ``forced``: per level dict(masks=[4 bool arrays], cells=(x0, y0, gx_on,
    gy_on)) or None; ``record`` (a list) receives the same structure with what this evaluation chose itself (its ``up`` rounded
    to fp32 for the cells) plus ``up``."""
    dtype = next(iter(params.values())).dtype
    ref, supp = np.asarray(ref, np.float64), np.asarray(supp, np.float64)
    h, w = ref.shape[2:]
    hf, wf = -(-h // 32) * 32, -(-w // 32) * 32
    if (hf, wf) != (h, w):
        ref, supp = R.resize_half_pixel(ref, hf, wf), R.resize_half_pixel(supp, hf, wf)
    nm = lambda t: (t - R.MEAN[None, :, None, None]) / R.STD[None, :, None, None]   # noqa: E731
    refs, supps = [nm(ref)], [nm(supp)]
    for _ in range(5):
        refs.insert(0, R.avgpool2(refs[0]))
        supps.insert(0, R.avgpool2(supps[0]))
    flow = None
    for level in range(6):
        r, s = torch.from_numpy(refs[level]).to(dtype), torch.from_numpy(supps[level]).to(dtype)
        n, _, lh, lw = r.shape
        if flow is None:
            up = torch.zeros((n, 2, lh, lw), dtype=dtype)
        else:
            uy, ux = torch.from_numpy(_up_matrix(lh)).to(dtype), torch.from_numpy(_up_matrix(lw)).to(dtype)
            up = 2.0 * torch.einsum('yp,ncpq,xq->ncyx', uy, flow, ux)
        cells = forced[level]['cells'] if forced is not None else cells_of(up.detach().float().numpy())
        x = torch.cat([r, _warp(s, up, cells), up], 1)
        masks = []
        for i in range(5):
            pre = F.conv2d(x, params[f'basic_module.{level}.basic_module.{2 * i}.weight'],
                           params[f'basic_module.{level}.basic_module.{2 * i}.bias'], padding=3)
            if i == 4:
                flow = pre + up
                break
            m = torch.from_numpy(np.asarray(forced[level]['masks'][i])) if forced is not None else pre.detach() > 0
            masks.append(m)
            x = pre * m.to(dtype)
        if record is not None:
            record.append(dict(masks=[m.numpy() for m in masks], cells=cells, up=up.detach().numpy()))
    if (hf, wf) != (h, w):
        ry, rx = torch.from_numpy(_resize_matrix(hf, h)).to(dtype), torch.from_numpy(_resize_matrix(wf, w)).to(dtype)
        flow = torch.einsum('dy,ncyx,ex->ncde', ry, flow, rx) * torch.tensor([w / wf, h / hf], dtype=dtype)[None, :, None, None]
    return flow


def plain(params, ref, supp):
    """SpyNet with torch's own ops (the reference's composition): F.interpolate, F.grid_sample, F.conv2d, F.relu, F.avg_pool2d."""
    dtype = next(iter(params.values())).dtype
    ref, supp = torch.from_numpy(np.asarray(ref)).to(dtype), torch.from_numpy(np.asarray(supp)).to(dtype)
    h, w = ref.shape[2:]
    hf, wf = -(-h // 32) * 32, -(-w // 32) * 32
    if (hf, wf) != (h, w):
        ref = F.interpolate(ref, size=(hf, wf), mode='bilinear', align_corners=False)
        supp = F.interpolate(supp, size=(hf, wf), mode='bilinear', align_corners=False)
    mean, std = torch.from_numpy(R.MEAN).to(dtype).view(1, 3, 1, 1), torch.from_numpy(R.STD).to(dtype).view(1, 3, 1, 1)
    refs, supps = [(ref - mean) / std], [(supp - mean) / std]
    for _ in range(5):
        refs.insert(0, F.avg_pool2d(refs[0], 2, 2))
        supps.insert(0, F.avg_pool2d(supps[0], 2, 2))
    flow = None
    for level in range(6):
        n, _, lh, lw = refs[level].shape
        up = torch.zeros((n, 2, lh, lw), dtype=dtype) if flow is None else \
            2.0 * F.interpolate(flow, scale_factor=2, mode='bilinear', align_corners=True)
        gy, gx = torch.meshgrid(torch.arange(lh, dtype=dtype), torch.arange(lw, dtype=dtype), indexing='ij')
        grid = torch.stack((2 * (gx + up[:, 0]) / max(lw - 1, 1) - 1, 2 * (gy + up[:, 1]) / max(lh - 1, 1) - 1), 3)
        warped = F.grid_sample(supps[level], grid, mode='bilinear', padding_mode='border', align_corners=True)
        x = torch.cat([refs[level], warped, up], 1)
        for i in range(5):
            x = F.conv2d(x, params[f'basic_module.{level}.basic_module.{2 * i}.weight'],
                         params[f'basic_module.{level}.basic_module.{2 * i}.bias'], padding=3)
            if i < 4:
                x = F.relu(x)
        flow = x + up
    if (hf, wf) != (h, w):
        flow = F.interpolate(flow, size=(h, w), mode='bilinear', align_corners=False)
        flow = flow * torch.tensor([w / wf, h / hf], dtype=dtype)[None, :, None, None]
    return flow


def gradients(fn, params, ref, supp, g, **kw):
    """{name: dL/dparam as float64 numpy} for L = sum(flow * g)."""
    flow = fn(params, ref, supp, **kw)
    grads = torch.autograd.grad((flow * torch.from_numpy(np.asarray(g)).to(flow.dtype)).sum(), list(params.values()))
    return {k: v.double().numpy() for k, v in zip(params, grads)}, flow.detach()


def rel_l2(a, b):
    """Per parameter tensor |a - b| / |b|."""
    return {k: float(np.linalg.norm(a[k] - b[k]) / max(np.linalg.norm(b[k]), 1e-300)) for k in b}


def summary(grads, seed=11):
    """What the fixture keeps of a set of gradients: per tensor its norm, its sum and 16 seeded entries; the biases in full."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, v in grads.items():
        idx = rng.integers(0, v.size, 16)
        out[k] = dict(norm=float(np.linalg.norm(v)), sum=float(v.sum()), idx=idx, vals=v.reshape(-1)[idx].copy())
        if k.endswith('bias'):
            out[k]['full'] = v.copy()
    return out
