"""IconVSR's bf16 inference forward on the GPU (fixture tests/golden/g_zf_iconvsr.npz: b1 n6 34x38 padded to 36x40, keyframe_stride
4, keyframes 0, 4, 5, num_block 2), by the project's bf16 network bound:
    max |y_hip - y64| <= 2 max |y_model - y64| + 4 fp32 ulp of max |y64|,
y64 = tests/vsr_restate.py in float64, y_model = tests/vsr_bf16_restate.py (bf16 round trips where the HIP path stores or rounds).

CPU proxies (the model with float32 accumulation, measured before any GPU run; tests/test_vsr_bf16_host.py asserts the first and the
last): whole network, keyframe features from the bf16 extractor model, proxy / bound 0.41 (d_model 5.1e-2 on outputs of magnitude
1.03: the keyframe features, of magnitude 60 with deformable offsets of several pixels, move by up to 23 under bf16 rounding);
keyframe features alone 0.61 / 0.58 / 0.61; ``propagate`` on float64 keyframe features (rounded once to bf16) 0.45 (d_model 2.3e-3).
0.41 <= 0.75, so the case is checked whole — ``propagate`` on the fixture's flows with the device's own bf16 keyframe features.
The split form (``propagate`` on float64 keyframe features, the far tighter bound) is checked as well: it pins the propagation and the
head on their own, as §31 did in fp32; ``forward`` (own SpyNet, own extractor) is checked against restatements fed the device flows.
"""
import os
import sys

import numpy as np
import pytest
import torch

import image_restoration_amd as ira

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as FR  # noqa: E402
import vsr_bf16_restate as B  # noqa: E402
import vsr_restate as V  # noqa: E402

pytestmark = pytest.mark.gpu
TAG, BATCH, N, H, W, STRIDE = V.ICON_CASE


def _build(sd, dev):
    net = ira.build_network(dict(type='IconVSR', num_block=V.NUM_BLOCK, keyframe_stride=STRIDE))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.to(dev).eval()


@pytest.fixture(scope='module')
def setup(cuda, golden):
    g = golden('g_zf_iconvsr')
    keys, shapes = [str(k) for k in g['iconvsr_keys']], [tuple(int(d) for d in str(s).split(',')) for s in g['iconvsr_shapes']]
    ek = [(k[5:], s) for k, s in zip(keys, shapes) if k.startswith('edvr.')]
    edvr = V.extractor_weights(int(g['edvr_seed']), [k for k, _ in ek], [s for _, s in ek])
    sd = {'edvr.' + k: v for k, v in edvr.items()}
    sd.update({'spynet.' + k: v for k, v in FR.spynet_weights(int(g['spynet_seed']), float(g['spynet_scale'])).items()})
    sd.update(V.iconvsr_weights(int(g['weight_seed']), V.NUM_FEAT, V.NUM_BLOCK, float(g['trunk_scale'])))
    net = _build(sd, cuda)
    assert net.set_compute_dtype('bf16') is net
    x = torch.from_numpy(V.clip_input(int(g['input_seed']), BATCH, N, H, W)).to(cuda)
    return net, sd, x, g, edvr


def _cb16(a, dev):
    """float64 [b, c, h, w] -> raw CB16 bf16 [b, c / 16, h, w, 16] on the device (one rounding)."""
    b, c, h, w = a.shape
    return torch.from_numpy(a.astype(np.float32)).view(b, c // 16, 16, h, w).permute(0, 1, 3, 4, 2).contiguous().to(dev).bfloat16()


def _check(tag, y, ym, y64, bad):
    bound = B.network_bound(ym, y64)
    yh = y.double().cpu().numpy()
    d_model, d_hip = float(np.abs(ym - y64).max()), float(np.abs(yh - y64).max())
    print(f'{TAG} {tag}: max|y64| {np.abs(y64).max():.3f}, model {d_model:.4e}, HIP {d_hip:.4e}, HIP / bound {d_hip / bound:.3f}, '
          f'HIP vs model {float(np.abs(yh - ym).max()):.4e}')
    if d_hip > bound:
        bad.append(f'{tag}: {d_hip:.4e} > {bound:.4e}')
    return bound


def test_network_within_twice_the_model_distance(cuda, setup):
    net, sd, x, g, edvr = setup
    xp = net.pad_spatial(x)
    xp_np = xp.double().cpu().numpy()
    keys = net.keyframes(N)
    assert keys == [0, 4, 5] and tuple(xp.shape) == (BATCH, N, 3, 36, 40)
    feats = net.get_keyframe_feature(xp, keys)
    assert all(f.dtype == torch.bfloat16 and tuple(f.shape) == (BATCH, 4, 36, 40, 16) for f in feats.values())
    ff, fb = g[TAG + '_flows_forward'], g[TAG + '_flows_backward']
    ffd, fbd = torch.from_numpy(ff).to(cuda), torch.from_numpy(fb).to(cuda)
    kf64 = V.keyframe_features(edvr, xp_np, keys)
    kfm = B.keyframe_features(edvr, xp_np, keys)
    bad = []
    # 1. whole, on the fixture's flows: the device's own bf16 keyframe features against the model's
    y64 = V.iconvsr_propagate(sd, xp_np, ff, fb, kf64)
    y = net.propagate(xp, ffd, fbd)
    assert tuple(y.shape) == (BATCH, N, 3, 144, 160) and y.dtype == torch.float32 and y.grad_fn is None
    _check('propagate, own keyframe features', y, B.iconvsr_propagate(sd, xp_np, ff, fb, kfm), y64, bad)
    # 2. split: propagate on float64 keyframe features rounded once to bf16
    y = net.propagate(xp, ffd, fbd, {i: _cb16(f, cuda) for i, f in kf64.items()})
    _check('propagate, float64 keyframe features', y, B.iconvsr_propagate(sd, xp_np, ff, fb, kf64), y64, bad)
    # 3. forward: own SpyNet (fp32), own extractor; the restatements are fed the device flows
    gf, gb = net.get_flow(xp)
    assert float((gf.cpu() - torch.from_numpy(ff)).abs().max()) <= 2e-4
    gfn, gbn = gf.cpu().numpy(), gb.cpu().numpy()
    y = net(x)
    assert tuple(y.shape) == (BATCH, N, 3, 4 * H, 4 * W)
    crop = (Ellipsis, slice(0, 4 * H), slice(0, 4 * W))
    _check('forward', y, B.iconvsr_propagate(sd, xp_np, gfn, gbn, kfm)[crop], V.iconvsr_propagate(sd, xp_np, gfn, gbn, kf64)[crop], bad)
    assert not bad, bad


def test_contracts(cuda, setup):
    net, sd, x, g, edvr = setup
    y = net(x)                                                              # eval mode, grad enabled
    assert tuple(y.shape) == (BATCH, N, 3, 4 * H, 4 * W) and y.grad_fn is None and not y.requires_grad
    xp = net.pad_spatial(x)
    ff, fb = net.get_flow(xp)
    full = net.propagate(xp, ff, fb)
    assert tuple(full.shape) == (BATCH, N, 3, 144, 160) and torch.equal(full[..., :4 * H, :4 * W], y)
    assert torch.equal(net.propagate(xp, ff, fb, net.get_keyframe_feature(xp, net.keyframes(N)), crop=(H, W)), y)
    assert torch.equal(net(x), y)
    x2 = torch.cat([x, x.flip(1)], 0)                                       # batch 2 is two batch-1 clips, bit for bit
    y2 = net(x2)
    assert torch.equal(y2[0:1], y) and torch.equal(y2[1:2], net(x2[1:2]))
    net.train()
    try:
        with pytest.raises(NotImplementedError, match='fp32'):
            net(x)
        with torch.no_grad():
            assert torch.equal(net(x), y)
    finally:
        net.eval()
    # fp32 afterwards is the fp32 forward's bits again; the flows are the same bits in both modes
    ref = _build(sd, cuda)
    y32 = ref(x)
    assert torch.equal(ref.get_flow(xp)[0], ff) and not torch.equal(y32, y)
    try:
        assert torch.equal(net.set_compute_dtype('fp32')(x), y32)
    finally:
        net.set_compute_dtype('bf16')
    # in-place updates of a fusion conv, a trunk and the extractor are seen by the next forward (on the twin: the shared network
    # keeps the fixture's weights)
    twin = ref.set_compute_dtype('bf16')
    seen = [twin(x)]
    assert torch.equal(seen[0], y)
    for p in (twin.backward_fusion.weight, twin.forward_trunk.main[2][0].conv1.weight, twin.edvr.fusion.feat_fusion.weight):
        with torch.no_grad():
            p.mul_(1.25)
        out = twin(x)
        assert all(not torch.equal(out, s) for s in seen)
        seen.append(out)
