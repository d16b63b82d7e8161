"""BasicVSR's bf16 inference forward on the GPU, by the yardstick of the project's bf16 networks.

y64 is tests/vsr_restate.py in float64 (no rounding anywhere); y_model is tests/vsr_bf16_restate.py, the same float64 computation
with a bf16 round trip wherever the HIP path stores or rounds a tensor.  The HIP forward must stay within
    max |y_hip - y64| <= 2 max |y_model - y64| + 4 fp32 ulp of max |y64|.
``propagate`` runs on the fixture's flows (tests/golden/g_ze_basicvsr.npz: >= 4 px, they really warp); ``forward`` runs the project's
own fp32 SpyNet, and its y64 and y_model are the restatements fed the same device flows.  Both fixture cases, num_block 2.

CPU proxy (the model with its convolutions accumulated in float32, measured before any GPU run; tests/test_vsr_bf16_host.py asserts
it): proxy / bound 0.47 (b1 n3 33x40, d_model 1.04e-4) and 0.51 (b2 n2 34x33, d_model 1.02e-4) on outputs of magnitude 0.96.
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
import vsr_bf16_restate as B  # noqa: E402
import vsr_restate as V  # noqa: E402

pytestmark = pytest.mark.gpu

# sr_conv3x3_bf16's instances, the bf16 pixel shuffle, sr_conv1x1_bf16's kernels (tests/test_edvr_bf16_gpu.py), the bf16 step input
BF16_IDS = set(range(16, 32)) | {42, 43, 50, 64} | {98} | set(range(124, 130)) | {167}


@pytest.fixture(scope='module')
def state(golden):
    g = golden('g_ze_basicvsr')
    sd = {'spynet.' + k: v for k, v in FR.spynet_weights(int(g['spynet_seed']), float(g['spynet_scale'])).items()}
    sd.update(V.basicvsr_weights(int(g['weight_seed']), V.NUM_FEAT, V.NUM_BLOCK, float(g['trunk_scale'])))
    return g, sd


def _build(sd, dev):
    net = ira.build_network(dict(type='BasicVSR', num_feat=V.NUM_FEAT, num_block=V.NUM_BLOCK)).to(dev).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net


@pytest.fixture(scope='module')
def net(cuda, state):
    net = _build(state[1], cuda)
    assert net.set_compute_dtype('bf16') is net and net.compute_dtype == 'bf16'
    return net


def _clip(g, tag):
    idx = [c[0] for c in V.CASES].index(tag)
    _, b, n, h, w = V.CASES[idx]
    return V.clip_input(int(g['input_seed']) + idx, b, n, h, w)


@pytest.mark.parametrize('case', V.CASES, ids=[c[0] for c in V.CASES])
def test_network_within_twice_the_model_distance(cuda, net, state, case):
    g, sd = state
    tag, b, n, h, w = case
    x_np = _clip(g, tag)
    x = torch.from_numpy(x_np).to(cuda)
    ff, fb = g[tag + '_flows_forward'], g[tag + '_flows_backward']
    assert max(np.abs(ff).max(), np.abs(fb).max()) >= 4.0
    gf, gb = net.get_flow(x)
    assert gf.dtype == torch.float32 and float((gf.cpu() - torch.from_numpy(ff)).abs().max()) <= 2e-4       # SpyNet stays fp32
    routes = {'propagate': (net.propagate(x, torch.from_numpy(ff).to(cuda), torch.from_numpy(fb).to(cuda)), ff, fb),
              'forward': (net(x), gf.cpu().numpy(), gb.cpu().numpy())}
    bad = []
    for route, (y, f_fwd, f_bwd) in routes.items():
        assert tuple(y.shape) == (b, n, 3, 4 * h, 4 * w) and y.dtype == torch.float32 and y.grad_fn is None
        y64 = V.basicvsr_propagate(sd, x_np, f_fwd, f_bwd)
        ym = B.basicvsr_propagate(sd, x_np, f_fwd, f_bwd)
        bound = B.network_bound(ym, y64)
        yh = y.double().cpu().numpy()
        d_model, d_hip = float(np.abs(ym - y64).max()), float(np.abs(yh - y64).max())
        print(f'{tag} {route}: max|y64| {np.abs(y64).max():.3f}, model {d_model:.4e}, HIP {d_hip:.4e}, HIP / bound {d_hip / bound:.3f}, '
              f'HIP vs model {float(np.abs(yh - ym).max()):.4e}')
        if d_hip > bound:
            bad.append(f'{route}: {d_hip:.4e} > {bound:.4e}')
        # the bound tells errors apart: the float64 result on zeroed flows is far outside it
        assert float(np.abs(V.basicvsr_propagate(sd, x_np, 0 * f_fwd, 0 * f_bwd) - y64).max()) > 2 * bound
    assert not bad, bad


def test_contracts(cuda, net, state):
    g, sd = state
    x = torch.from_numpy(_clip(g, V.CASES[1][0])).to(cuda)                  # b = 2, n = 2, 34x33
    y = net(x)                                                              # eval mode, grad enabled: no no_grad needed
    assert y.grad_fn is None and not y.requires_grad and y.dtype == torch.float32
    ff, fb = net.get_flow(x)
    assert torch.equal(net.propagate(x, ff, fb), y)                         # forward is propagate after get_flow, bit for bit
    assert torch.equal(net(x), y)                                           # the rerun
    for k in range(2):                                                      # batch 2 is two batch-1 clips
        assert torch.equal(net(x[k:k + 1]), y[k:k + 1]), k
    net.train()
    try:
        with pytest.raises(NotImplementedError, match='fp32'):
            net(x)
        with torch.no_grad():
            assert torch.equal(net(x), y)
    finally:
        net.eval()
    # the flows are the fp32 network's bits, and fp32 afterwards is the fp32 forward's bits again
    ref = _build(sd, cuda)
    y32 = ref(x)
    rf, rb = ref.get_flow(x)
    assert torch.equal(rf, ff) and torch.equal(rb, fb) and not torch.equal(y32, y)
    try:
        assert torch.equal(net.set_compute_dtype('fp32')(x), y32)
    finally:
        net.set_compute_dtype('bf16')
    assert torch.equal(net(x), y)


def test_weight_images_follow_a_parameter_update(cuda, state):
    g, sd = state
    x = torch.from_numpy(_clip(g, V.CASES[1][0])).to(cuda)
    net, twin = _build(sd, cuda).set_compute_dtype('bf16'), _build(sd, cuda).set_compute_dtype('bf16')
    seen = [net(x)]
    assert torch.equal(twin(x), seen[0])
    for p in (net.forward_trunk.main[2][1].conv2.weight, net.backward_trunk.main[0].bias, net.fusion.weight, net.conv_hr.weight):
        with torch.no_grad():
            p.mul_(1.25)
        out = net(x)
        assert all(not torch.equal(out, s) for s in seen)
        seen.append(out)
    twin.load_state_dict(net.state_dict())
    assert torch.equal(twin(x), seen[-1])


def test_only_bf16_kernels_run_between_the_step_input_and_conv_last(cuda, net, state):
    g, sd = state
    lib = _lib.load()
    x = torch.from_numpy(_clip(g, V.CASES[0][0])).to(cuda)                  # b = 1, n = 3
    net(x)                                                                  # packs the weights (not profiled below)
    _lib.check(lib.sr_profile_start(1024), 'sr_profile_start')
    try:
        net(x)
    finally:
        recs = (_lib.LaunchRecord * 1024)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, 1024, C.byref(cnt)), 'sr_profile_stop')
    ids = [recs[i].kernel_id for i in range(cnt.value)]
    print(len(ids), 'profiled launches:', sorted({lib.sr_kernel_name(i).decode() for i in ids}))
    first = ids.index(167)
    last = len(ids) - 1 - ids[::-1].index(50)                               # conv_last: the few-cout kernel storing fp32 NCHW
    assert 167 not in ids[:first] and not set(ids[:first]) & BF16_IDS       # SpyNet: fp32 kernels only, all before the first step
    assert set(ids[first:last + 1]) <= BF16_IDS, sorted(set(ids[first:last + 1]) - BF16_IDS)
    assert ids[last + 1:] == [72], ids[last + 1:]                           # the x4 base of the fp32 frames
    n, nb = 3, V.NUM_BLOCK
    assert ids.count(167) == 2 * n and 159 not in ids                       # one step input per step and branch
    body = ids[first:last + 1]
    assert len(body) == 2 * n * (2 + 2 * nb) + 1 + 2 + 2 + 2                # steps; fusion, 2 x (upconv, shuffle), conv_hr, conv_last
