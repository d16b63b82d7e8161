"""Records the reference's own ``BasicVSR`` (through tools/ref_loader.py) into tests/golden/g_ze_basicvsr.npz.  Build container
only: the reference does not travel to the GPU box.

State dict: the key list and shapes of ``BasicVSR()`` and a checksum of its freshly initialised parameters under INIT_SEED.

Per case (num_block 2, num_feat 64; sides must exceed 32, and these are the smallest shapes that still hit partial rows, odd
widths, SpyNet's pre-resize and the batch / frame indexing): both flow tensors in full, the output, and the reference's own
fp32-versus-float64 distance of the output.  The float64 run does not use the float64 flows as they are: they are rounded to fp32
first and fed back (``get_flow`` of that instance is replaced by a function returning them), so that the stored fp32 flows ARE the
flows of the recorded output and the restatement reproduces it from the fixture alone.  The fp32 run is the reference's plain
forward, its own fp32 SpyNet included, so the recorded distance covers the flow estimator's rounding too.

Weights and inputs are not stored: seeded generators in tests/vsr_restate.py and tests/flow_restate.py, the fixture keeps the seeds
and a checksum.  To stay under the 1 MiB limit of a committed file the outputs are stored as float64 values ROUNDED TO FP32 (in
full for the first case, on the lattice [..., oy::3, ox::3] for the second: a stride of 3 is coprime to the two x2 shuffles, so it
visits all 16 pixel-shuffle phases); every bound on them therefore carries an extra 2^-24 * |value|.

The tool asserts that the fixture can tell errors apart: zeroing the flows and zeroing the backward branch's features each move
the output by at least 100 times the reference's fp32 distance of the case; if not, the trunk weight scale is doubled and
recorded.  It also asserts that tests/vsr_restate.py reproduces the reference's float64 output to 1e-10 before rounding.
"""
import hashlib
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
import vsr_restate as V  # noqa: E402
import ref_loader  # noqa: E402

INIT_SEED, WEIGHT_SEED, SPYNET_SEED, SPYNET_SCALE, INPUT_SEED = 31, 4242, 20260, 16.0, 500
LATTICE = {V.CASES[0][0]: (0, 0, 1), V.CASES[1][0]: (1, 2, 3)}   # (oy, ox, stride) per case


def params_checksum(net):
    h = hashlib.sha256()
    for k, v in net.state_dict().items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v.detach().numpy()).tobytes())
    return h.hexdigest()


def full_state_dict(scale):
    sd = {'spynet.' + k: v for k, v in FR.spynet_weights(SPYNET_SEED, SPYNET_SCALE).items()}
    sd.update(V.basicvsr_weights(WEIGHT_SEED, V.NUM_FEAT, V.NUM_BLOCK, scale))
    return sd


def build(mod, sd, dtype):
    net = mod.BasicVSR(num_feat=V.NUM_FEAT, num_block=V.NUM_BLOCK).to(dtype).eval()
    net.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}, strict=True)
    return net


def main():
    ref_loader.load_reference()
    mod = importlib.import_module('basicsr.archs.basicvsr_arch')
    out = {'init_seed': np.int64(INIT_SEED), 'weight_seed': np.int64(WEIGHT_SEED), 'spynet_seed': np.int64(SPYNET_SEED),
           'spynet_scale': np.float64(SPYNET_SCALE), 'input_seed': np.int64(INPUT_SEED)}
    torch.manual_seed(INIT_SEED)
    fresh = mod.BasicVSR()
    out['basicvsr_keys'] = np.array(list(fresh.state_dict()))
    out['basicvsr_shapes'] = np.array([','.join(str(d) for d in v.shape) for v in fresh.state_dict().values()])
    out['basicvsr_init_checksum'] = np.array(params_checksum(fresh))

    scale = 0.5
    while True:
        sd = full_state_dict(scale)
        net64, net32 = build(mod, sd, torch.float64), build(mod, sd, torch.float32)
        results, ok = {}, True
        for i, (tag, b, n, h, w) in enumerate(V.CASES):
            x = V.clip_input(INPUT_SEED + i, b, n, h, w)
            with torch.no_grad():
                ff, fb = (f.float() for f in type(net64).get_flow(net64, torch.from_numpy(x).double()))
                net64.get_flow = lambda _x, ff=ff, fb=fb: (ff.double(), fb.double())
                o64 = net64(torch.from_numpy(x).double()).numpy()
                del net64.get_flow
                o32 = net32(torch.from_numpy(x)).double().numpy()
            dist = float(np.abs(o32 - o64).max())
            ffn, fbn = ff.numpy(), fb.numpy()
            mine = V.basicvsr_propagate(sd, x, ffn, fbn)
            restate = float(np.abs(mine - o64).max())
            no_flow = float(np.abs(V.basicvsr_propagate(sd, x, np.zeros_like(ffn), np.zeros_like(fbn)) - o64).max())
            no_back = float(np.abs(V.basicvsr_propagate(sd, x, ffn, fbn, zero_backward=True) - o64).max())
            print(f'{tag}: scale {scale} flow peak {max(np.abs(ffn).max(), np.abs(fbn).max()):.2f} px, fp32 distance {dist:.2e}, '
                  f'restatement {restate:.1e}, zero flows move the output by {no_flow:.2e}, zero backward features by {no_back:.2e}')
            assert restate <= 1e-10, (tag, restate)
            ok = ok and no_flow >= 100 * dist and no_back >= 100 * dist
            results[tag] = (ffn, fbn, o64, dist)
        if ok:
            break
        scale *= 2
    out['trunk_scale'] = np.float64(scale)
    out['weight_checksum'] = np.array(FR.weights_checksum(sd))
    for tag, (ffn, fbn, o64, dist) in results.items():
        oy, ox, st = LATTICE[tag]
        out[tag + '_flows_forward'], out[tag + '_flows_backward'] = ffn, fbn
        out[tag + '_out'] = o64[..., oy::st, ox::st].astype(np.float32)      # float64 rounded to fp32: + 2^-24 |value| on every bound
        out[tag + '_lattice'] = np.array([oy, ox, st], dtype=np.int64)
        out[tag + '_fp32_dist'] = np.float64(dist)
    path = os.path.join(ROOT, 'tests', 'golden', 'g_ze_basicvsr.npz')
    np.savez(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == '__main__':
    main()
