"""Records the reference's own ``TOFlow`` (basicsr/archs/tof_arch.py, through tools/ref_loader.py) into
tests/golden/g_zi_tof.npz.  Build container only: the reference does not travel to the GPU box.

Per case of tests/tof_restate.CASES (16x16 with batch 2, 32x48, 48x80) the 8-bit input clip, the reference's float64 flows
[6 b, 2, h, w] (the six pairs are the same for both settings of ``adapt_official_weights``: reference frame 3 against frames 0, 1,
2, 4, 5, 6, so they are stored once), and per setting its float64 output and its own fp32-versus-float64 distances for output and
flows.  The reference's fp32 results are kept as those distances only, to keep the file below 1 MiB, which is also why only the
smallest case has batch 2.  Weights are not stored: they come from the seeded ``synth.tof_state_dict``, the fixture keeps the
seed, a checksum and the key, shape and order lists of the reference's state_dict.

Default init gives flows far below a pixel and an output that is the reference frame to 1e-2, so the seeded weights are scaled
(see synth.tof_state_dict).  This tool asserts that the recipe does its job: the finest-level flow of some pair exceeds 1 px and
all stay below 8 px, and the output departs from the denormalised reference frame by at least 0.05.
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
import tof_restate as T  # noqa: E402
from image_restoration_amd.utils import synth  # noqa: E402


def run(net, lrs):
    """(output, flows [6 b, 2, h, w] with image 6 b + k) of the reference network."""
    flows = []
    handle = net.spynet.register_forward_hook(lambda _m, _i, out: flows.append(out.detach()))
    with torch.no_grad():
        out = net(lrs)
    handle.remove()
    return out, torch.stack(flows, 1).flatten(0, 1)        # [b, 6, ...] -> image 6 b + k


def main():
    ref_loader.load_reference()
    tof = importlib.import_module('basicsr.archs.tof_arch')
    sd = synth.tof_state_dict(T.WEIGHT_SEED)
    ref_sd = tof.TOFlow().state_dict()
    out = {'weight_seed': np.int64(T.WEIGHT_SEED), 'input_seed': np.int64(T.INPUT_SEED),
           'weight_checksum': np.array(R.weights_checksum(sd)),
           'keys': np.array(list(ref_sd)), 'shapes': np.array([','.join(str(d) for d in v.shape) for v in ref_sd.values()]),
           'num_params': np.int64(sum(p.numel() for p in tof.TOFlow().parameters()))}
    assert list(ref_sd) == list(sd) and all(tuple(ref_sd[k].shape) == sd[k].shape for k in sd)
    # the reference's initial parameters under a seed: three probes a seeded fresh network must reproduce
    torch.manual_seed(11)
    fresh = tof.TOFlow().state_dict()
    for k in ('spynet.basic_module.0.basic_module.0.weight', 'spynet.basic_module.3.basic_module.12.bias', 'conv_2.weight', 'conv_4.bias'):
        out['init_' + k] = fresh[k].flatten()[:8].numpy()
    nets = {}
    for adapt in (False, True):
        for dtype in (torch.float64, torch.float32):
            net = tof.TOFlow(adapt_official_weights=adapt).to(dtype).eval()
            net.load_state_dict({k: torch.from_numpy(v).to(dtype if v.dtype == np.float32 else torch.int64) for k, v in sd.items()},
                                strict=True)
            nets[adapt, dtype] = net
    for i, (tag, b, h, w) in enumerate(T.CASES):
        u8 = T.clip_u8(T.INPUT_SEED + i, b, h, w)
        out[f'{tag}_clip_u8'] = u8
        x = torch.from_numpy(T.decode(u8))
        for adapt in (False, True):
            o64, f64 = run(nets[adapt, torch.float64], x.double())
            o32, f32 = run(nets[adapt, torch.float32], x)
            s = f'{tag}_adapt{int(adapt)}'
            if adapt:
                assert np.array_equal(f64.numpy(), out[f'{tag}_flows'])      # the same six pairs
            else:
                out[f'{tag}_flows'] = f64.numpy()
            out[s + '_out'] = o64.numpy()
            out[s + '_out_fp32_dist'] = np.float64((o32.double() - o64).abs().max())
            out[s + '_flows_fp32_dist'] = np.float64((f32.double() - f64).abs().max())
            lr_ref = x[:, 3].double()
            depart = float((o64 - lr_ref).abs().max())
            peak = float(f64.abs().max())
            print(f'{s}: flow peak {peak:.2f} px, |out - lr_ref| {depart:.3f}, out in [{float(o64.min()):.2f}, {float(o64.max()):.2f}], '
                  f'fp32 distance out {float(out[s + "_out_fp32_dist"]):.2e} flows {float(out[s + "_flows_fp32_dist"]):.2e}')
            assert 1.0 < peak < 8.0, (s, peak)
            assert depart >= 0.05, (s, depart)
    path = os.path.join(ROOT, 'tests', 'golden', 'g_zi_tof.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1000 * 1024


if __name__ == '__main__':
    main()
