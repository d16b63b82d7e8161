"""Records the reference BasicVSR's own float64 parameter and flow gradients (through tools/ref_loader.py) into
tests/golden/g_zh_basicvsr_grad.npz.  Build container only: the reference does not travel to the GPU box.

Case b1_n3_33x40 of tests/vsr_grad_restate.py: the seeded weights and clip of tests/golden/g_ze_basicvsr.npz, its recorded fp32
flows fed back as leaves (``get_flow`` of the instance is replaced, as tools/make_golden_basicvsr.py does), loss sum(y * g) with
the seeded normal g of ``grad_output``.  The gradients of the 30 parameter tensors outside ``spynet.*`` and of the two flow
tensors are about 2.9 MB as fp32, so per tensor the fixture keeps its L2 norm and the strided sample of
``vsr_grad_restate.sample_index`` (the tool asserts that a weight's sample visits every output channel, input channel and tap),
as float64.  Seeds and the weight checksum are stored, not weights.

The tool asserts that tests/vsr_grad_restate.py reproduces the reference's float64 gradients to 1e-9 in relative L2 on every
tensor before anything is sampled, and records the reference's own fp32-versus-float64 distance of the gradients."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import flow_restate as FR  # noqa: E402
import ref_loader  # noqa: E402
import vsr_grad_restate as G  # noqa: E402

TAG = 'b1_n3_33x40'


def reference_grads(mod, sd, x, ff, fb, g, num_feat, num_block, dtype):
    net = mod.BasicVSR(num_feat=num_feat, num_block=num_block).to(dtype).train()
    net.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}, strict=False)
    fft = torch.from_numpy(ff).to(dtype).requires_grad_()
    fbt = torch.from_numpy(fb).to(dtype).requires_grad_()
    net.get_flow = lambda _x: (fft, fbt)
    y = net(torch.from_numpy(x).to(dtype))
    (y * torch.from_numpy(g).to(dtype)).sum().backward()
    grads = {k: p.grad.double().numpy() for k, p in net.named_parameters() if not k.startswith('spynet.')}
    grads.update(flows_forward=fft.grad.double().numpy(), flows_backward=fbt.grad.double().numpy())
    return grads


def main():
    ref_loader.load_reference()
    mod = importlib.import_module('basicsr.archs.basicvsr_arch')
    fix = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'g_ze_basicvsr.npz')))
    _, b, n, h, w, nf, nb = G.case(TAG)
    sd, x, ff, fb = G.case_data(fix, TAG)
    g = G.grad_output(TAG)
    g64 = reference_grads(mod, sd, x, ff, fb, g, nf, nb, torch.float64)
    g32 = reference_grads(mod, sd, x, ff, fb, g, nf, nb, torch.float32)
    mine, _ = G.gradients(sd, x, ff, fb, g, nb)
    assert list(mine) == list(g64) and len(mine) == 32
    restate, dist = max(G.rel_l2(mine, g64).values()), max(G.rel_l2(g32, g64).values())
    print(f'{TAG}: restatement vs reference float64 gradients {restate:.2e}; reference fp32 vs float64 {dist:.2e}')
    assert restate <= 1e-9, restate
    out = {'tag': np.array(TAG), 'weight_seed': fix['weight_seed'], 'input_seed': fix['input_seed'], 'trunk_scale': fix['trunk_scale'],
           'grad_seed': np.int64(7), 'weight_checksum': np.array(FR.weights_checksum(sd)), 'fp32_dist': np.float64(dist),
           'names': np.array(list(g64))}
    for k, v in g64.items():
        if v.ndim == 4 and k.endswith('weight'):
            co, ci, tap = np.unravel_index(G.sample_index(v.shape), (v.shape[0], v.shape[1], v.shape[2] * v.shape[3]))
            assert len(set(co)) == v.shape[0] and len(set(ci)) == v.shape[1] and len(set(tap)) == v.shape[2] * v.shape[3], k
    for k, s in G.summary(g64).items():
        out[f'{k}/norm'], out[f'{k}/vals'] = np.float64(s['norm']), s['vals']
    path = os.path.join(ROOT, 'tests', 'golden', 'g_zh_basicvsr_grad.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == '__main__':
    main()
