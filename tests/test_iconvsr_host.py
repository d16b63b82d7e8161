"""IconVSR on the host (no GPU): registry, constructor defaults, key list, shapes and init checksum against what the reference's
own IconVSR recorded (tests/golden/g_zf_iconvsr.npz, tools/make_golden_iconvsr.py), the float64 restatement — keyframe features
through tests/edvr_restate.py and tests/dcn_restate.py, propagation through tests/vsr_restate.py — against the recorded keyframe
features and output, the refusals before the device check, the keyframe rule and the spatial padding."""
import hashlib
import inspect
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import image_restoration_amd as ira
from image_restoration_amd import _lib
from image_restoration_amd.archs.basicvsr_arch import EDVRFeatureExtractor, IconVSR
from image_restoration_amd.archs.edvr_arch import EDVR
from image_restoration_amd.utils.registry import ARCH_REGISTRY

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as FR  # noqa: E402
import vsr_restate as V  # noqa: E402


def _checksum(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v.detach().numpy()).tobytes())
    return h.hexdigest()


def test_registry_defaults_state_dict_and_init_are_the_references(golden):
    g = golden('g_zf_iconvsr')
    assert ARCH_REGISTRY.get('IconVSR') is IconVSR
    sig = inspect.signature(IconVSR.__init__)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [
        ('num_feat', 64), ('num_block', 15), ('keyframe_stride', 5), ('temporal_padding', 2), ('spynet_path', None), ('edvr_path', None)]
    torch.manual_seed(int(g['init_seed']))
    net = ira.build_network(dict(type='IconVSR'))
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in g['iconvsr_keys']] and len(sd) == 294
    assert [','.join(str(d) for d in v.shape) for v in sd.values()] == [str(v) for v in g['iconvsr_shapes']]
    assert _checksum(sd) == str(g['iconvsr_init_checksum'])       # the same draws in the same order as the reference
    # the extractor's share of EDVR's key list (tests/test_edvr_host.py pins that against the reference too)
    part = ('conv_first.', 'feature_extraction.', 'conv_l2_', 'conv_l3_', 'pcd_align.', 'fusion.')
    edvr = EDVR(num_frame=5, num_extract_block=5, num_reconstruct_block=0).state_dict()
    assert [k for k in sd if k.startswith('edvr.')] == ['edvr.' + k for k in edvr if k.startswith(part)]
    # temporal_padding 3 widens the fusion convs only
    wide = IconVSR(num_block=0, temporal_padding=3).state_dict()
    assert tuple(wide['edvr.fusion.feat_fusion.weight'].shape) == (64, 7 * 64, 1, 1) and list(wide)[:60] == list(sd)[:60]
    # the seeded weights of the fixture load strictly
    small = IconVSR(num_block=V.NUM_BLOCK, keyframe_stride=V.ICON_CASE[5])
    small.load_state_dict({k: torch.from_numpy(v) for k, v in _fixture_weights(g).items()}, strict=True)


def _fixture_weights(g):
    keys, shapes = [str(k) for k in g['iconvsr_keys']], [tuple(int(d) for d in str(s).split(',')) for s in g['iconvsr_shapes']]
    ek = [(k[5:], s) for k, s in zip(keys, shapes) if k.startswith('edvr.')]
    sd = {'edvr.' + k: v for k, v in V.extractor_weights(int(g['edvr_seed']), [k for k, _ in ek], [s for _, s in ek]).items()}
    sd.update({'spynet.' + k: v for k, v in FR.spynet_weights(int(g['spynet_seed']), float(g['spynet_scale'])).items()})
    sd.update(V.iconvsr_weights(int(g['weight_seed']), V.NUM_FEAT, V.NUM_BLOCK, float(g['trunk_scale'])))
    assert FR.weights_checksum(sd) == str(g['weight_checksum'])
    return sd


def test_restatement_reproduces_the_reference(golden):
    """Keyframe features from tests/edvr_restate.py / tests/dcn_restate.py on windows built from the definition, then the
    restated propagation on those features and the fixture's flows: both equal what the reference's own IconVSR recorded."""
    g = golden('g_zf_iconvsr')
    tag, b, n, h, w, stride = V.ICON_CASE
    sd = _fixture_weights(g)
    x = V.pad_spatial(V.clip_input(int(g['input_seed']), b, n, h, w))
    idx = V.keyframes(n, stride)
    assert idx == [int(i) for i in g[tag + '_keyframe_idx']] == [0, 4, 5] and x.shape == (b, n, 3, 36, 40)
    assert V.mirrored_windows(6, idx, 2) == {0: [4, 3, 0, 1, 2], 4: [2, 3, 4, 5, 2], 5: [3, 4, 5, 2, 1]}
    assert V.mirrored_windows(8, [0, 7], 3) == {0: [6, 5, 4, 0, 1, 2, 3], 7: [4, 5, 6, 7, 3, 2, 1]}
    oy, ox, st = (int(v) for v in g[tag + '_lattice'])
    feats = V.keyframe_features({k[5:]: v for k, v in sd.items() if k.startswith('edvr.')}, x, idx)
    want_kf = g[tag + '_keyframe_feats'].astype(np.float64)
    for k, i in enumerate(idx):
        got = feats[i][..., oy::st, ox::st]
        assert (np.abs(got - want_kf[k]) <= 1e-10 + 2.0 ** -24 * np.abs(want_kf[k])).all(), i
    ff, fb = g[tag + '_flows_forward'], g[tag + '_flows_backward']
    out = V.iconvsr_propagate(sd, x, ff, fb, feats)[..., :4 * h, :4 * w]
    want = g[tag + '_out'].astype(np.float64)
    got = out[..., oy::st, ox::st]
    assert got.shape == want.shape and (np.abs(got - want) <= 1e-10 + 2.0 ** -24 * np.abs(want)).all(), float(np.abs(got - want).max())
    dist, dist_kf = float(g[tag + '_fp32_dist']), float(g[tag + '_keyframe_fp32_dist'])
    assert 1e-8 < dist < 1e-3 and dist_kf < 1e-3 * np.abs(want_kf).max()
    # the fixture tells errors apart: a window off by one frame, a wrong centre, zeroed features
    shifted = V.keyframe_features({k[5:]: v for k, v in sd.items() if k.startswith('edvr.')}, np.roll(x, 1, axis=1), [4])
    assert np.abs(shifted[4][..., oy::st, ox::st] - want_kf[1]).max() >= 100 * dist_kf
    zeros = {i: np.zeros_like(f) for i, f in feats.items()}
    assert np.abs(V.iconvsr_propagate(sd, x, ff, fb, zeros)[..., :4 * h, :4 * w][..., oy::st, ox::st] - want).max() >= 100 * dist


def test_edvr_path_loads_params(tmp_path):
    src = EDVRFeatureExtractor(5, 64, None)
    path = str(tmp_path / 'edvr.pth')
    torch.save({'params': src.state_dict()}, path)
    net = ira.build_network(dict(type='IconVSR', num_block=0, edvr_path=path))
    for k, v in src.state_dict().items():
        assert torch.equal(net.edvr.state_dict()[k], v), k


def test_refusals_come_before_the_device_check():
    for bad, needle in ((dict(temporal_padding=1), 'temporal_padding'), (dict(temporal_padding=4), 'temporal_padding'),
                        (dict(num_feat=32), 'hard-codes 64'), (dict(num_feat=128), 'hard-codes 64'), (dict(keyframe_stride=0), 'keyframe_stride')):
        with pytest.raises(ValueError, match=needle):
            IconVSR(num_block=0, **bad)
    for tp, need in ((2, 5), (3, 7)):
        net = IconVSR(num_block=0, temporal_padding=tp).eval()
        with pytest.raises(ValueError, match='reference fails'):
            net(torch.zeros(1, need - 1, 3, 40, 40))
        for x, needle in ((torch.zeros(1, need, 4, 40, 40), r'\[b, n, 3, h, w\]'), (torch.zeros(1, need, 3, 40, 40).double(), 'supported: fp32'),
                          (torch.zeros(1, need, 3, 32, 40), 'too small')):
            with pytest.raises(ValueError, match=needle):
                net(x)
        with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
            net(torch.zeros(1, need, 3, 40, 40))
    flows = torch.zeros(1, 4, 2, 34, 40)
    with pytest.raises(ValueError, match='multiples of 4'):
        net = IconVSR(num_block=0).eval()
        net.propagate(torch.zeros(1, 5, 3, 34, 40), flows, flows)


def test_keyframes_and_pad_spatial():
    net = IconVSR(num_block=0, keyframe_stride=4)
    assert net.keyframes(6) == V.keyframes(6, 4) == [0, 4, 5] and net.keyframes(9) == [0, 4, 8] and net.keyframes(5) == [0, 4]
    assert IconVSR(num_block=0).keyframes(100) == list(range(0, 100, 5)) + [99]
    x = torch.randn(2, 3, 3, 34, 38)
    p = net.pad_spatial(x)
    assert tuple(p.shape) == (2, 3, 3, 36, 40)
    assert torch.equal(p, F.pad(x.view(-1, 3, 34, 38), [0, 2, 0, 2], mode='reflect').view(2, 3, 3, 36, 40))
    assert np.array_equal(V.pad_spatial(x.numpy()), p.numpy())
    y = torch.randn(1, 2, 3, 36, 40)
    assert net.pad_spatial(y) is y
