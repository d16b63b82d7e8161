"""IconVSR on the GPU against what the reference's own IconVSR recorded (tests/golden/g_zf_iconvsr.npz,
tools/make_golden_iconvsr.py: case b1 n6 34x38, keyframe_stride 4 — padded to 36x40, keyframes 0, 4, 5; num_block 2), and the
network's contracts.

Nothing on the yardstick's side comes from the code under test.  The keyframe features of the device are compared on their own
with the recorded ones.  ``propagate`` is fed the fixture's flows and keyframe features computed in float64 by
tests/edvr_restate.py / tests/dcn_restate.py on windows built from the definition (tests/test_iconvsr_host.py shows that these
equal the recorded features to 1e-10), and ``forward`` runs the project's own SpyNet and extractor; both are compared with the
recorded output.

Bounds: 10 x the reference's recorded fp32-versus-float64 distance — of the keyframe features for the features, of the output for
the outputs — the project's standing margin, plus 2^-24 * |value| because the fixture stores float64 values rounded to fp32.
Forced Winograd in the trunks: err_on <= 4 * err_off + 2^-20 on the direct route's measured error.  The keyframe features are of
magnitude 60 with deformable offsets of several pixels (the fixture tool asserts that zeroed offset convs move them by >= 100 x
their fp32 distance), and the reference's own fp32 distance on them is 2.6e-2: sampling positions next to a pixel boundary.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import image_restoration_amd as ira
from image_restoration_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as FR  # noqa: E402
import vsr_restate as V  # noqa: E402

pytestmark = pytest.mark.gpu
TAG, B, N, H, W, STRIDE = V.ICON_CASE


@pytest.fixture(scope='module')
def lib():
    lib = _lib.load()
    lib.sr_dev_set_wino_f32.argtypes = [C.c_int]
    lib.sr_dev_set_wino_f32.restype = C.c_int
    yield lib
    lib.sr_dev_set_wino_f32(1)


@pytest.fixture(autouse=True)
def switches(lib):
    yield
    lib.sr_dev_set_wino_f32(1)


@pytest.fixture(scope='module')
def setup(cuda, golden):
    g = golden('g_zf_iconvsr')
    keys, shapes = [str(k) for k in g['iconvsr_keys']], [tuple(int(d) for d in str(s).split(',')) for s in g['iconvsr_shapes']]
    ek = [(k[5:], s) for k, s in zip(keys, shapes) if k.startswith('edvr.')]
    edvr = V.extractor_weights(int(g['edvr_seed']), [k for k, _ in ek], [s for _, s in ek])
    sd = {'edvr.' + k: v for k, v in edvr.items()}
    sd.update({'spynet.' + k: v for k, v in FR.spynet_weights(int(g['spynet_seed']), float(g['spynet_scale'])).items()})
    sd.update(V.iconvsr_weights(int(g['weight_seed']), V.NUM_FEAT, V.NUM_BLOCK, float(g['trunk_scale'])))
    assert FR.weights_checksum(sd) == str(g['weight_checksum'])
    net = ira.build_network(dict(type='IconVSR', num_block=V.NUM_BLOCK, keyframe_stride=STRIDE))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net = net.to(cuda).eval()
    x = torch.from_numpy(V.clip_input(int(g['input_seed']), B, N, H, W)).to(cuda)
    return net, sd, x, g, edvr


def _nchw(t):
    """raw CB8 [b, cb, h, w, 8] -> float64 [b, 8 cb, h, w]."""
    b, cb, h, w, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(b, cb * 8, h, w).double().cpu().numpy()


def _cb8(a, dev):
    """float64 [b, c, h, w] -> raw CB8 fp32 [b, c / 8, h, w, 8] on the device."""
    b, c, h, w = a.shape
    return torch.from_numpy(a.astype(np.float32)).view(b, c // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous().to(dev)


def test_keyframe_features_and_outputs_against_the_reference(cuda, lib, setup):
    net, sd, x, g, edvr = setup
    oy, ox, st = (int(v) for v in g[TAG + '_lattice'])
    dist, dist_kf = float(g[TAG + '_fp32_dist']), float(g[TAG + '_keyframe_fp32_dist'])
    xp = net.pad_spatial(x)
    assert tuple(xp.shape) == (B, N, 3, 36, 40) and np.array_equal(xp.cpu().numpy(), V.pad_spatial(x.cpu().numpy()))
    keys = net.keyframes(N)
    assert keys == [int(i) for i in g[TAG + '_keyframe_idx']] == [0, 4, 5]
    bad = []
    # 1. the keyframe branch on its own
    feats = net.get_keyframe_feature(xp, keys)
    assert sorted(feats) == keys and all(tuple(f.shape) == (B, 8, 36, 40, 8) for f in feats.values())
    want_kf = g[TAG + '_keyframe_feats'].astype(np.float64)
    for k, i in enumerate(keys):
        e = float(np.abs(_nchw(feats[i])[..., oy::st, ox::st] - want_kf[k]).max())
        bound = 10 * dist_kf + 2.0 ** -24 * float(np.abs(want_kf[k]).max())
        print(f'{TAG} keyframe {i}: feature err {e:.3e} bound {bound:.3e} (reference fp32 distance {dist_kf:.3e}, max |feature| '
              f'{np.abs(want_kf[k]).max():.1f})')
        if e > bound:
            bad.append(f'keyframe {i} features {e:.3e} > {bound:.3e}')
    # 2. propagate on the fixture's flows and on keyframe features that do not come from the device; forward on the device's own
    ind = V.keyframe_features(edvr, xp.double().cpu().numpy(), keys)
    ind_dev = {i: _cb8(f, cuda) for i, f in ind.items()}
    ff, fb = torch.from_numpy(g[TAG + '_flows_forward']).to(cuda), torch.from_numpy(g[TAG + '_flows_backward']).to(cuda)
    want = g[TAG + '_out'].astype(np.float64)
    rnd = 2.0 ** -24 * float(np.abs(want).max())
    errs = {}
    try:
        for mode in (0, 3):
            lib.sr_dev_set_wino_f32(mode)
            y_prop, y_fwd = net.propagate(xp, ff, fb, ind_dev, crop=(H, W)), net(x)
            assert tuple(y_prop.shape) == tuple(y_fwd.shape) == (B, N, 3, 4 * H, 4 * W) and y_prop.grad_fn is None
            errs[mode] = [float(np.abs(y[..., oy::st, ox::st].double().cpu().numpy() - want).max()) for y in (y_prop, y_fwd)]
    finally:
        lib.sr_dev_set_wino_f32(1)
    for k, route in enumerate(('propagate', 'forward')):
        e0, e3 = errs[0][k], errs[3][k]
        b0, b3 = 10 * dist + rnd, 4 * e0 + 2.0 ** -20
        print(f'{TAG} {route}: direct err {e0:.3e} bound {b0:.3e} | forced Winograd err {e3:.3e} bound {b3:.3e} '
              f'(reference fp32 distance {dist:.3e})')
        if e0 > b0:
            bad.append(f'{route} direct {e0:.3e} > {b0:.3e}')
        if e3 > b3:
            bad.append(f'{route} forced Winograd {e3:.3e} > {b3:.3e}')
    assert not bad, bad
    gf, gb = net.get_flow(xp)
    assert float((gf - ff).abs().max()) <= 2e-4 and float((gb - fb).abs().max()) <= 2e-4       # as tests/test_basicvsr_gpu.py


def test_contracts(cuda, setup):
    net, sd, x, g, edvr = setup
    y = net(x)
    assert tuple(y.shape) == (B, N, 3, 4 * H, 4 * W) and y.grad_fn is None        # cropped to 4h x 4w of the unpadded input
    xp = net.pad_spatial(x)
    ff, fb = net.get_flow(xp)
    full = net.propagate(xp, ff, fb)
    assert tuple(full.shape) == (B, N, 3, 144, 160) and torch.equal(full[..., :4 * H, :4 * W], y)
    assert torch.equal(net.propagate(xp, ff, fb, net.get_keyframe_feature(xp, net.keyframes(N)), crop=(H, W)), y)
    # batch 2 is two batch-1 clips, bit for bit
    x2 = torch.cat([x, x.flip(1)], 0)
    y2 = net(x2)
    assert torch.equal(y2[0:1], y) and torch.equal(y2[1:2], net(x2[1:2]))
    # train mode with grad refuses; no_grad in train mode runs
    net.train()
    try:
        with pytest.raises(NotImplementedError, match='follow-up'):
            net(x)
        with torch.no_grad():
            assert torch.equal(net(x), y)
    finally:
        net.eval()
    # in-place updates of a fusion conv, a trunk and the extractor are seen by the next forward
    seen = [y]
    for p in (net.backward_fusion.weight, net.forward_trunk.main[2][0].conv1.weight, net.edvr.fusion.feat_fusion.weight):
        with torch.no_grad():
            p.mul_(1.25)
        out = net(x)
        assert all(not torch.equal(out, s) for s in seen)
        seen.append(out)
    with torch.no_grad():
        for p in (net.backward_fusion.weight, net.forward_trunk.main[2][0].conv1.weight, net.edvr.fusion.feat_fusion.weight):
            p.div_(1.25)
