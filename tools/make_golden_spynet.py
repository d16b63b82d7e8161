"""Records the reference's own ``flow_warp`` and ``SpyNet`` (through tools/ref_loader.py, in float64) into
tests/golden/g_zd_spynet.npz.  Build container only: the reference does not travel to the GPU box.

flow_warp: both padding modes over a small grid of shapes; inputs, outputs and autograd gradients.
SpyNet: batch 2 at 64x64 (the smallest size that runs) and single pairs at 96x64, 64x96 (odd level-0 sizes) and 70x90 (pre-resize
to 96x96 and the rescale).  Per case the output, the flow after each level (levels 0-4; level 5 is the output, or for 70x90 is
covered by it) and the reference's own fp32-versus-float64 distances.  Neither weights nor inputs are stored: both come from
seeded generators in tests/flow_restate.py, the fixture keeps the seeds and a checksum of the weights.

Default init gives flows below one pixel, which tests no warping, so the last conv of every level has its bias drawn from
U(-0.5, 0.5) and its weight scaled (flow_restate.spynet_weights).  This tool asserts that the recipe does its job — flow peak >= 8
px at the finest level, >= 10 % of the warp samples outside the image at every level but the first, and an output that moves by
>= 0.5 px somewhere when the weights are zeroed and the biases kept — and raises the scale if the last fails.
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import flow_restate as R  # noqa: E402
import ref_loader  # noqa: E402

WEIGHT_SEED, INPUT_SEED, WARP_SEED = 20260, 77, 5
CASES = (('b2_64x64', 2, 64, 64), ('96x64', 1, 96, 64), ('64x96', 1, 64, 96), ('70x90', 1, 70, 90))
WARP_SHAPES = ((1, 1), (1, 5), (5, 1), (2, 2), (7, 9))


def run(net, ref, supp):
    """(output, [flow after each level], [fraction of warp samples outside the image per level])."""
    levels, outside = [], []

    def hook(_, inp, out):
        up = inp[0][:, 6:8]
        levels.append((out + up).detach())
        h, w = up.shape[2:]
        gy, gx = torch.meshgrid(torch.arange(h, dtype=up.dtype), torch.arange(w, dtype=up.dtype), indexing='ij')
        ix, iy = gx + up[:, 0], gy + up[:, 1]
        outside.append(float(((ix < 0) | (ix > w - 1) | (iy < 0) | (iy > h - 1)).double().mean()))
    handles = [m.register_forward_hook(hook) for m in net.basic_module]
    with torch.no_grad():
        out = net(ref, supp)
    for hd in handles:
        hd.remove()
    return out, levels, outside


def build(spy, sd, dtype):
    net = spy.SpyNet().to(dtype).eval()
    net.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}, strict=True)
    return net


def main():
    ref_loader.load_reference()
    spy = importlib.import_module('basicsr.archs.spynet_arch')
    arch_util = importlib.import_module('basicsr.archs.arch_util')
    out = {'weight_seed': np.int64(WEIGHT_SEED), 'input_seed': np.int64(INPUT_SEED)}

    # ---- flow_warp
    rng = np.random.default_rng(WARP_SEED)
    for (h, w) in WARP_SHAPES:
        x = rng.standard_normal((2, 3, h, w)).astype(np.float32)
        flow = rng.uniform(-3, 3, (2, h, w, 2)).astype(np.float32)
        g = rng.standard_normal((2, 3, h, w)).astype(np.float32)
        tag = f'warp_{h}x{w}'
        out[tag + '_x'], out[tag + '_flow'], out[tag + '_g'] = x, flow, g
        for pm in ('zeros', 'border'):
            xt = torch.from_numpy(x).double().requires_grad_()
            ft = torch.from_numpy(flow).double().requires_grad_()
            y = arch_util.flow_warp(xt, ft, interp_mode='bilinear', padding_mode=pm)
            dx, df = torch.autograd.grad(y, (xt, ft), torch.from_numpy(g).double())
            out[f'{tag}_{pm}_out'], out[f'{tag}_{pm}_dx'], out[f'{tag}_{pm}_dflow'] = y.detach().numpy(), dx.numpy(), df.numpy()

    # ---- SpyNet
    scale = 16.0
    while True:
        sd = R.spynet_weights(WEIGHT_SEED, scale)
        net64, net32 = build(spy, sd, torch.float64), build(spy, sd, torch.float32)
        zeroed = {k: (np.zeros_like(v) if k.endswith('weight') else v) for k, v in sd.items()}
        netz = build(spy, zeroed, torch.float64)
        results, ok = {}, True
        for i, (tag, n, h, w) in enumerate(CASES):
            ref, supp = R.spynet_inputs(INPUT_SEED + i, n, h, w)
            r64, s64 = torch.from_numpy(ref).double(), torch.from_numpy(supp).double()
            o64, l64, outside = run(net64, r64, s64)
            o32, l32, _ = run(net32, torch.from_numpy(ref), torch.from_numpy(supp))
            oz, _, _ = run(netz, r64, s64)
            peak = float(l64[-1].abs().max())
            moved = float((o64 - oz).abs().max())
            print(f'{tag}: scale {scale} peak {peak:.2f} px, outside {["%.2f" % f for f in outside]}, weights move the output by '
                  f'{moved:.2f} px, fp32 distance {float((o32.double() - o64).abs().max()):.2e}')
            assert peak >= 8.0, (tag, peak)
            assert min(outside[1:]) >= 0.10, (tag, outside)
            ok = ok and moved >= 0.5
            results[tag] = (o64, l64, o32, l32)
        if ok:
            break
        scale *= 2
    out['last_scale'] = np.float64(scale)
    out['weight_checksum'] = np.array(R.weights_checksum(sd))
    for tag, (o64, l64, o32, l32) in results.items():
        out[f'spy_{tag}_out'] = o64.numpy()
        for lv in range(5):
            out[f'spy_{tag}_level{lv}'] = l64[lv].numpy()
        out[f'spy_{tag}_fp32_dist'] = np.array([float((a.double() - b).abs().max()) for a, b in zip(l32, l64)]
                                               + [float((o32.double() - o64).abs().max())])
    path = os.path.join(ROOT, 'tests', 'golden', 'g_zd_spynet.npz')
    np.savez(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 900 * 1024


if __name__ == '__main__':
    main()
