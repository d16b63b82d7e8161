"""Records the reference's own ``DUF`` (basicsr/archs/duf_arch.py, through tools/ref_loader.py) and its ``duf_downsample``
(basicsr/data/data_util.py) into tests/golden/g_zj_duf.npz.  Build container only: the reference does not travel to the GPU box.

Per case of tests/duf_restate.CASES (num_layer, scale, b, h, w, adapt_official_weights) the 8-bit input clip, the reference's
float64 output, its own fp32-versus-float64 distance, and what the seeded weights must show (below) as numbers; for the first
case also the float64 filter logits and residual (forward hooks), to localise a failure.  Weights are not stored: they come from
the seeded ``synth.duf_state_dict``; the fixture keeps the seed, a checksum per (num_layer, scale) and the key and shape lists of
the reference's state_dict.  For the DUF test set: the reference's Gaussian kernels (sigma 0.8, 1.2, 1.6) and its downsampling
of a seeded 2x3x40x52 input at scales 2, 3 and 4, in float64.

Default init makes every BatchNorm the identity, the 25 filter weights near uniform and the residual invisible, so the seeded
recipe draws the BatchNorm tensors and scales conv3d_f2 / conv3d_r2 (see synth.duf_state_dict).  This tool asserts that the
recipe does its job on every case: the output is finite, the fp32 distance lies in (1e-8, 1e-4), some softmax weight exceeds 0.5
while the mean peak weight stays below 0.99, |res| reaches 0.05, the output departs from the nearest-neighbour upsampled centre
frame by at least 0.05, and between 20 % and 80 % of the elements pass the ReLU at the input of every dense block.
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
import duf_restate as D  # noqa: E402
import flow_restate as R  # noqa: E402
import ref_loader  # noqa: E402
from image_restoration_amd.utils import synth  # noqa: E402

DOWNSAMPLE_SEED, DOWNSAMPLE_SHAPE = 5, (2, 3, 40, 52)


def run(net, x):
    """(output, logits [b, 25 s2, h, w], res [b, 3 s2, h, w], ReLU pass fractions at the first BatchNorm of every dense block)."""
    kept, fractions, handles = {}, [], []
    handles.append(net.conv3d_f2.register_forward_hook(lambda _m, _i, out: kept.__setitem__('logits', out.detach()[:, :, 0].clone())))
    handles.append(net.conv3d_r2.register_forward_hook(lambda _m, _i, out: kept.__setitem__('res', out.detach()[:, :, 0].clone())))
    blocks = list(net.dense_block1.dense_blocks) + [net.dense_block2.temporal_reduce1, net.dense_block2.temporal_reduce2,
                                                    net.dense_block2.temporal_reduce3]
    for seq in blocks:
        handles.append(seq[0].register_forward_hook(lambda _m, _i, out: fractions.append(float((out > 0).double().mean()))))
    with torch.no_grad():
        out = net(x)
    for h in handles:
        h.remove()
    return out, kept['logits'], kept['res'], np.array(fractions)


def main():
    ns = ref_loader.load_reference()
    duf = importlib.import_module('basicsr.archs.duf_arch')
    out = {'weight_seed': np.int64(D.WEIGHT_SEED), 'input_seed': np.int64(D.INPUT_SEED)}
    for num_layer, scale in sorted({(c[1], c[2]) for c in D.CASES}):
        sd = synth.duf_state_dict(D.WEIGHT_SEED, num_layer, scale)
        ref_sd = duf.DUF(scale, num_layer).state_dict()
        assert list(ref_sd) == list(sd) and all(tuple(ref_sd[k].shape) == sd[k].shape for k in sd)
        tag = f'l{num_layer}_x{scale}'
        out[tag + '_checksum'] = np.array(R.weights_checksum(sd))
        out[tag + '_keys'] = np.array(list(ref_sd))
        out[tag + '_shapes'] = np.array([','.join(str(d) for d in v.shape) for v in ref_sd.values()])
        out[tag + '_num_params'] = np.int64(sum(p.numel() for p in duf.DUF(scale, num_layer).parameters()))
    # the reference's initial parameters under a seed: probes a seeded fresh network must reproduce
    torch.manual_seed(11)
    fresh = duf.DUF(4, 16).state_dict()
    for k in ('conv3d1.weight', 'dense_block1.dense_blocks.2.5.weight', 'dense_block2.temporal_reduce3.2.bias', 'conv3d_f2.weight'):
        out['init_' + k] = fresh[k].flatten()[:8].numpy()
    for i, (tag, num_layer, scale, b, h, w, adapt) in enumerate(D.CASES):
        sd = synth.duf_state_dict(D.WEIGHT_SEED, num_layer, scale)
        nets = {}
        for dtype in (torch.float64, torch.float32):
            net = duf.DUF(scale, num_layer, adapt).to(dtype).eval()
            net.load_state_dict({k: torch.from_numpy(v).to(dtype if v.dtype == np.float32 else torch.int64) for k, v in sd.items()},
                                strict=True)
            nets[dtype] = net
        u8 = D.clip_u8(D.INPUT_SEED + i, b, h, w)
        out[f'{tag}_clip_u8'] = u8
        x = torch.from_numpy(D.decode(u8))
        o64, l64, r64, frac = run(nets[torch.float64], x.double())
        o32 = run(nets[torch.float32], x)[0]
        s2 = scale * scale
        peak = torch.softmax(l64.view(b, 25, s2, h, w), 1).max(1)[0]
        depart = float(np.abs(o64.numpy() - D.nearest_up(x[:, 3].double().numpy(), scale)).max())
        dist = float((o32.double() - o64).abs().max())
        out[tag + '_out'] = o64.numpy()
        out[tag + '_fp32_dist'] = np.float64(dist)
        out[tag + '_peak_max'] = np.float64(peak.max())
        out[tag + '_peak_mean'] = np.float64(peak.mean())
        out[tag + '_res_absmax'] = np.float64(r64.abs().max())
        out[tag + '_depart'] = np.float64(depart)
        out[tag + '_fractions'] = frac
        if i == 0:
            out[tag + '_logits'] = l64.numpy()
            out[tag + '_res'] = r64.numpy()
        print(f'{tag}: out in [{float(o64.min()):.2f}, {float(o64.max()):.2f}], fp32 distance {dist:.2e}, peak weight max '
              f'{float(peak.max()):.3f} mean {float(peak.mean()):.3f}, |res| {float(r64.abs().max()):.3f}, departs {depart:.3f}, ReLU pass '
              f'{frac.min():.2f}..{frac.max():.2f}, |logits| {float(l64.abs().max()):.1f}')
        assert bool(torch.isfinite(o64).all()) and 1e-8 < dist < 1e-4, (tag, dist)
        assert float(peak.max()) > 0.5 and float(peak.mean()) < 0.99, tag
        assert float(r64.abs().max()) >= 0.05 and depart >= 0.05, tag
        assert frac.min() >= 0.2 and frac.max() <= 0.8 and len(frac) == D.BLOCKS[num_layer][0] + 3, (tag, frac)
    # the DUF test set's blur and downsampling
    xin = np.random.default_rng(DOWNSAMPLE_SEED).uniform(0, 1, DOWNSAMPLE_SHAPE)
    out['down_seed'] = np.int64(DOWNSAMPLE_SEED)
    for scale in (2, 3, 4):
        out[f'gauss_x{scale}'] = np.asarray(ns.data_util.generate_gaussian_kernel(13, 0.4 * scale), np.float64)
        out[f'down_x{scale}'] = ns.data_util.duf_downsample(torch.from_numpy(xin), 13, scale).numpy()
    path = os.path.join(ROOT, 'tests', 'golden', 'g_zj_duf.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1000 * 1024


if __name__ == '__main__':
    main()
