"""Records the reference SpyNet's own float64 autograd gradients (through tools/ref_loader.py) into
tests/golden/g_zg_spynet_grad.npz.  Build container only: the reference does not travel to the GPU box.

Loss sum(flow * g) with a seeded normal g, the seeded weights of tests/flow_restate.py (tests/spynet_grad_restate.py names the
seeds), three shapes: batch 2 at 64x64, 96x64 and 70x90 (the pre-resize to 96x96 and the rescale).  Per parameter tensor the
fixture keeps the gradient's norm, its sum and 16 seeded entries; the biases are stored in full.  It pins the restatement
tests/spynet_grad_restate.py to the reference (tests/test_flow_bwd_host.py).

SpyNet has kinks (a ReLU flips, a warp sample changes cell); a case in which float32 and float64 fall on different sides of one
says nothing about rounding.  Per shape the tool takes the first input seed from 100 on for which the reference's own fp32 and
float64 gradients agree to 2e-5 in relative L2 on every parameter tensor — no kink was crossed there — asserts that, and stores
the seed and the distance."""
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
import spynet_grad_restate as G  # noqa: E402

SHAPES = (('b2_64x64', 2, 64, 64), ('96x64', 1, 96, 64), ('70x90', 1, 70, 90))
AGREE = 2e-5


def reference_grads(spy, sd, ref, supp, g, dtype):
    net = spy.SpyNet().to(dtype).train()
    net.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}, strict=True)
    flow = net(torch.from_numpy(ref).to(dtype), torch.from_numpy(supp).to(dtype))
    (flow * torch.from_numpy(g).to(dtype)).sum().backward()
    return {k: p.grad.double().numpy() for k, p in net.named_parameters()}


def main():
    ref_loader.load_reference()
    spy = importlib.import_module('basicsr.archs.spynet_arch')
    sd = R.spynet_weights(G.WEIGHT_SEED, G.LAST_SCALE)
    out = {'weight_seed': np.int64(G.WEIGHT_SEED), 'last_scale': np.float64(G.LAST_SCALE),
           'weight_checksum': np.array(R.weights_checksum(sd))}
    for tag, n, h, w in SHAPES:
        g = np.random.default_rng(5).standard_normal((n, 2, h, w))
        for seed in range(100, 140):
            ref, supp = R.spynet_inputs(seed, n, h, w)
            g64 = reference_grads(spy, sd, ref, supp, g, torch.float64)
            g32 = reference_grads(spy, sd, ref, supp, g, torch.float32)
            dist = max(G.rel_l2(g32, g64).values())
            print(f'{tag}: input seed {seed}: reference fp32 vs float64 gradients {dist:.2e}')
            if dist <= AGREE:
                break
        assert dist <= AGREE, (tag, dist)
        out[f'{tag}_input_seed'], out[f'{tag}_fp32_dist'] = np.int64(seed), np.float64(dist)
        for k, s in G.summary(g64).items():
            out[f'{tag}/{k}/norm'], out[f'{tag}/{k}/sum'] = np.float64(s['norm']), np.float64(s['sum'])
            out[f'{tag}/{k}/idx'], out[f'{tag}/{k}/vals'] = s['idx'], s['vals']
            if 'full' in s:
                out[f'{tag}/{k}/full'] = s['full']
    path = os.path.join(ROOT, 'tests', 'golden', 'g_zg_spynet_grad.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 300 * 1024


if __name__ == '__main__':
    main()
