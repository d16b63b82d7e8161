"""Records the reference's own ``IconVSR`` (through tools/ref_loader.py) into tests/golden/g_zf_iconvsr.npz, a file of its own
next to g_ze_basicvsr.npz so that each stays under the 1 MiB limit of a committed file.  Build container only.

The reference's deformable convolution is a compiled extension with no CPU forward.  Its Python entry point,
``modulated_deform_conv`` as basicsr/archs/arch_util.py names it, is replaced at run time by tests/dcn_restate.py's restatement of
the kernel's semantics (plain torch ops in the dtype of its inputs); everything else — the reference's IconVSR,
EDVRFeatureExtractor, PCDAlignment, TSAFusion, DCNv2Pack.forward, SpyNet — runs in place, in float64 and in fp32.

State dict: key list, shapes and a checksum of the freshly initialised parameters of ``IconVSR()`` under INIT_SEED.

Case b1 n6 34x38, keyframe_stride 4, num_block 2 (padded to 36x40, keyframes 0, 4, 5): the keyframe indices, both flow tensors in
full, the keyframe features and the output on the lattice [..., oy::3, ox::3], and the reference's own fp32-versus-float64
distances of the output and of the keyframe features.  As for BasicVSR the float64 run is fed its own flows rounded to fp32, and
float64 values are stored rounded to fp32 (+ 2^-24 * |value| on every bound).  Weights and inputs come from seeded generators in
tests/vsr_restate.py and tests/flow_restate.py; the extractor's weights are drawn for the recorded (key, shape) list, because the
reference's own initialisation zeroes the offset convs.

Asserted here: tests/vsr_restate.py reproduces keyframe features and output to 1e-10 before rounding; zeroed keyframe features,
zeroed flows and zeroed backward features each move the output by >= 100 x the fp32 distance (else the trunk scale is doubled);
the deformable offsets are not trivial (the keyframe features move by >= 100 x their fp32 distance when the offset convs are zeroed).
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
import dcn_restate as D  # noqa: E402
import flow_restate as FR  # noqa: E402
import vsr_restate as V  # noqa: E402
import ref_loader  # noqa: E402

INIT_SEED, WEIGHT_SEED, EDVR_SEED, SPYNET_SEED, SPYNET_SCALE, INPUT_SEED = 32, 4243, 77, 20260, 16.0, 507
OY, OX, ST = 1, 2, 3


def checksum(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v.detach().numpy()).tobytes())
    return h.hexdigest()


def dcn_hook(x, offset, mask, weight, bias, stride, padding, dilation, groups, deformable_groups):
    assert (stride, padding, dilation, groups) == (1, 1, 1, 1) and tuple(weight.shape[2:]) == (3, 3)
    return D.modulated_deform_conv(x, offset, mask, weight, bias, deformable_groups)


def main():
    ref_loader.load_reference()
    mod = importlib.import_module('basicsr.archs.basicvsr_arch')
    arch_util = importlib.import_module('basicsr.archs.arch_util')
    arch_util.modulated_deform_conv = dcn_hook
    tag, b, n, h, w, stride = V.ICON_CASE
    out = {'init_seed': np.int64(INIT_SEED), 'weight_seed': np.int64(WEIGHT_SEED), 'edvr_seed': np.int64(EDVR_SEED),
           'spynet_seed': np.int64(SPYNET_SEED), 'spynet_scale': np.float64(SPYNET_SCALE), 'input_seed': np.int64(INPUT_SEED)}
    torch.manual_seed(INIT_SEED)
    fresh = mod.IconVSR()
    keys = list(fresh.state_dict())
    shapes = [tuple(v.shape) for v in fresh.state_dict().values()]
    out['iconvsr_keys'] = np.array(keys)
    out['iconvsr_shapes'] = np.array([','.join(str(d) for d in s) for s in shapes])
    out['iconvsr_init_checksum'] = np.array(checksum(fresh.state_dict()))
    ekeys = [k[5:] for k in keys if k.startswith('edvr.')]
    eshapes = [s for k, s in zip(keys, shapes) if k.startswith('edvr.')]
    x = V.clip_input(INPUT_SEED, b, n, h, w)
    xp = V.pad_spatial(x)
    idx = V.keyframes(n, stride)
    scale = 0.5
    while True:
        edvr = V.extractor_weights(EDVR_SEED, ekeys, eshapes)
        sd = {'edvr.' + k: v for k, v in edvr.items()}
        sd.update({'spynet.' + k: v for k, v in FR.spynet_weights(SPYNET_SEED, SPYNET_SCALE).items()})
        sd.update(V.iconvsr_weights(WEIGHT_SEED, V.NUM_FEAT, V.NUM_BLOCK, scale))
        nets = {}
        for dt in (torch.float64, torch.float32):
            net = mod.IconVSR(num_block=V.NUM_BLOCK, keyframe_stride=stride).to(dt).eval()
            net.load_state_dict({k: torch.from_numpy(v).to(dt) for k, v in sd.items()}, strict=True)
            nets[dt] = net
        net64, net32 = nets[torch.float64], nets[torch.float32]
        with torch.no_grad():
            xp64 = torch.from_numpy(xp).double()
            assert torch.equal(net64.pad_spatial(torch.from_numpy(x).double()), xp64)
            ff, fb = (f.float() for f in type(net64).get_flow(net64, xp64))
            kf64 = net64.get_keyframe_feature(xp64, idx)
            kf32 = net32.get_keyframe_feature(torch.from_numpy(xp), idx)
            net64.get_flow = lambda _x, ff=ff, fb=fb: (ff.double(), fb.double())
            o64 = net64(torch.from_numpy(x).double()).numpy()
            del net64.get_flow
            o32 = net32(torch.from_numpy(x)).double().numpy()
        assert sorted(kf64) == idx == [0, 4, 5] and o64.shape == (b, n, 3, 4 * h, 4 * w)
        dist = float(np.abs(o32 - o64).max())
        dist_kf = max(float((kf32[i].double() - kf64[i]).abs().max()) for i in idx)
        ffn, fbn = ff.numpy(), fb.numpy()
        mine_kf = V.keyframe_features(edvr, xp, idx)
        restate_kf = max(float(np.abs(mine_kf[i] - kf64[i].numpy()).max()) for i in idx)
        crop = (Ellipsis, slice(0, 4 * h), slice(0, 4 * w))
        mine = V.iconvsr_propagate(sd, xp, ffn, fbn, mine_kf)[crop]
        restate = float(np.abs(mine - o64).max())
        zeros = {i: np.zeros_like(f) for i, f in mine_kf.items()}
        no_kf = float(np.abs(V.iconvsr_propagate(sd, xp, ffn, fbn, zeros)[crop] - o64).max())
        no_flow = float(np.abs(V.iconvsr_propagate(sd, xp, 0 * ffn, 0 * fbn, mine_kf)[crop] - o64).max())
        flat = {k: (np.zeros_like(v) if 'conv_offset' in k else v) for k, v in edvr.items()}
        no_off = max(float(np.abs(V.keyframe_features(flat, xp, idx)[i] - mine_kf[i]).max()) for i in idx)
        print(f'{tag}: scale {scale} flow peak {max(np.abs(ffn).max(), np.abs(fbn).max()):.2f} px, |keyframe feature| max '
              f'{max(float(k.abs().max()) for k in kf64.values()):.2f}; fp32 distance output {dist:.2e} keyframe features {dist_kf:.2e}; '
              f'restatement output {restate:.1e} features {restate_kf:.1e}; zero keyframe features move the output by {no_kf:.2e}, '
              f'zero flows by {no_flow:.2e}; zeroed offset convs move the keyframe features by {no_off:.2e}')
        assert restate <= 1e-10 and restate_kf <= 1e-10, (restate, restate_kf)
        assert no_off >= 100 * dist_kf, (no_off, dist_kf)
        if no_kf >= 100 * dist and no_flow >= 100 * dist:
            break
        scale *= 2
    out['trunk_scale'] = np.float64(scale)
    out['weight_checksum'] = np.array(FR.weights_checksum(sd))
    out[tag + '_keyframe_idx'] = np.array(idx, dtype=np.int64)
    out[tag + '_flows_forward'], out[tag + '_flows_backward'] = ffn, fbn
    out[tag + '_lattice'] = np.array([OY, OX, ST], dtype=np.int64)
    out[tag + '_out'] = o64[..., OY::ST, OX::ST].astype(np.float32)
    out[tag + '_keyframe_feats'] = np.stack([kf64[i].numpy()[..., OY::ST, OX::ST] for i in idx]).astype(np.float32)
    out[tag + '_fp32_dist'] = np.float64(dist)
    out[tag + '_keyframe_fp32_dist'] = np.float64(dist_kf)
    path = os.path.join(ROOT, 'tests', 'golden', 'g_zf_iconvsr.npz')
    np.savez(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == '__main__':
    main()
