"""SpyNet's backward on the GPU (archs/spynet_autograd.py over include/sr_hip_flow_bwd.h), the whole network at once.

Loss sum(flow * g) with a seeded normal g, the seeded weights and inputs of tests/flow_restate.py, per parameter tensor in
relative L2 against tests/spynet_grad_restate.py in float64 FORCED with the device's own ReLU masks (saved activations > 0) and
warp cells (flow_restate.warp_coords on the saved fp32 ``up``).  Unforced the comparison would fail on arithmetic, not on bugs:
the fp32-versus-float64 distance of the torch restatement itself jumps to 1e-4 .. 2e-3 when one ReLU flips or one warp sample
changes cell (tried on the CPU, weight seed 7, input seeds 11-18: three of seven cases), and is 1.2e-6 .. 2.6e-6 in all seven when
forced.

Bound: 10 x the distance the torch restatement shows in fp32 on the CPU when it is forced with its own masks — the project's
standing margin over a measured fp32 distance; the case's figure is the largest over its parameter tensors (the device sums in
another order than torch's CPU convolutions, so a single tensor's CPU figure does not bound the same tensor on the device).
Both distances are printed.  Measured on an MI355X:
    b2_64x64   device 1.47e-06   cpu fp32 1.32e-06   bound 1.32e-05
    96x64      device 1.54e-06   cpu fp32 1.48e-06   bound 1.48e-05
    70x90      device 2.19e-06   cpu fp32 1.63e-06   bound 1.63e-05
"""
import os
import sys

import numpy as np
import pytest
import torch

from image_restoration_amd.archs.spynet_arch import SpyNet

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as R  # noqa: E402
import spynet_grad_restate as G  # noqa: E402

pytestmark = pytest.mark.gpu


def _net(cuda):
    net = SpyNet().to(cuda)
    sd = R.spynet_weights(G.WEIGHT_SEED, G.LAST_SCALE)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.train().set_autograd(True)


def _nchw(t, c):
    b = t.buf[:, t.cb0:t.cb0 + t.cbn].cpu()
    n, cb, h, w, _ = b.shape
    return b.permute(0, 1, 4, 2, 3).reshape(n, cb * 8, h, w)[:, :c].numpy()


def _device_grads(net, ref, supp, g):
    net.zero_grad(set_to_none=True)
    flow = net(ref, supp)
    assert flow.grad_fn is not None and flow.requires_grad and flow.dtype == torch.float32
    (flow * g).sum().backward()
    return {k: p.grad.clone() for k, p in net.named_parameters()}, flow.detach()


def _forced_from_device(net, ref, supp):
    """The device's own ReLU masks and warp cells, read from what the forward saves."""
    keep = {}
    with torch.no_grad():
        net.run_forward(ref, supp, keep=keep)
    forced = []
    for sv in keep['levels']:
        masks = [_nchw(a, a.channels) > 0 for a in sv['acts']]
        forced.append(dict(masks=masks, cells=G.cells_of(_nchw(sv['up'], 2))))
    return forced


_cache = {}


def _case(cuda, tag):
    if tag not in _cache:
        ref, supp = G.case_inputs(tag)
        g = G.grad_output(tag)
        net = _net(cuda)
        tr, ts = torch.from_numpy(ref).to(cuda), torch.from_numpy(supp).to(cuda)
        tg = torch.from_numpy(g).float().to(cuda)
        grads, flow = _device_grads(net, tr, ts, tg)
        _cache[tag] = (net, tr, ts, tg, grads, flow, ref, supp, g)
    return _cache[tag]


@pytest.mark.parametrize('tag', G.GRAD_CASES)
def test_gradients_match_the_forced_float64_restatement(cuda, tag):
    net, tr, ts, tg, grads, flow, ref, supp, g = _case(cuda, tag)
    g32 = tg.double().cpu().numpy()                           # the g the device saw
    # the yardstick's own fp32 distance, forced with its own masks (about 2 s)
    rec = []
    cpu32, _ = G.gradients(G.spynet, G.parameters(torch.float32), ref, supp, g32, record=rec)
    cpu64, _ = G.gradients(G.spynet, G.parameters(), ref, supp, g32, forced=rec)
    cpu_dist = G.rel_l2(cpu32, cpu64)
    # the device against float64 forced with the device's masks and cells
    want, want_flow = G.gradients(G.spynet, G.parameters(), ref, supp, g32, forced=_forced_from_device(net, tr, ts))
    got = {k: v.double().cpu().numpy() for k, v in grads.items()}
    dist = G.rel_l2(got, want)
    bound = 10.0 * max(cpu_dist.values())
    worst = max(dist, key=dist.get)
    print(f'\n{tag}: device vs forced float64 {max(dist.values()):.2e} (worst {worst}); torch fp32 vs forced float64 on the CPU '
          f'{max(cpu_dist.values()):.2e}; bound {bound:.2e}')
    assert set(got) == set(want) and len(got) == 60
    assert float((flow.double().cpu() - want_flow).abs().max()) <= 1e-3      # the forced forward is the device's forward
    for k in want:
        assert np.isfinite(got[k]).all() and dist[k] <= bound, (tag, k, dist[k], bound)


def test_backward_is_bit_reproducible_and_accumulates(cuda):
    net, tr, ts, tg, grads, flow, *_ = _case(cuda, 'b2_64x64')
    again, flow2 = _device_grads(net, tr, ts, tg)
    assert torch.equal(flow, flow2)
    for k in grads:
        assert torch.equal(grads[k], again[k]), k
    # a second backward without zero_grad accumulates into .grad
    (net(tr, ts) * tg).sum().backward()
    for k, p in net.named_parameters():
        assert torch.equal(p.grad, grads[k] + grads[k]), k
    # eval mode and no_grad keep the inference path
    with torch.no_grad():
        assert net(tr, ts).grad_fn is None
    net.eval()
    try:
        out = net(tr, ts)
        assert out.grad_fn is None and torch.equal(out, flow)
    finally:
        net.train()
    with pytest.raises(NotImplementedError, match='image gradients'):
        net(tr.clone().requires_grad_(), ts)
    net.set_autograd(False)
    try:
        with pytest.raises(NotImplementedError, match='backward'):
            net(tr, ts)
    finally:
        net.set_autograd(True)
    net.zero_grad(set_to_none=True)


def test_frozen_levels_get_no_gradient(cuda):
    net, tr, ts, tg, grads, *_ = _case(cuda, 'b2_64x64')
    try:
        for k, p in net.named_parameters():
            p.requires_grad_(k.startswith('basic_module.5.'))
        net.zero_grad(set_to_none=True)
        (net(tr, ts) * tg).sum().backward()
        for k, p in net.named_parameters():
            if k.startswith('basic_module.5.'):
                assert torch.equal(p.grad, grads[k]), k                  # level 5's gradients are unchanged
            else:
                assert p.grad is None, k
    finally:
        for p in net.parameters():
            p.requires_grad_(True)
        net.zero_grad(set_to_none=True)


def test_thirty_adam_steps_lower_the_loss(cuda):
    """One 64x64 pair towards a fixed target flow: the loss falls, so the pack cache sees the optimiser's in-place updates (a
    stale forward or data-gradient image would leave the loss where it was or send it up)."""
    net = _net(cuda)
    ref, supp = G.case_inputs('b2_64x64')
    tr, ts = torch.from_numpy(ref[:1]).to(cuda), torch.from_numpy(supp[:1]).to(cuda)
    with torch.no_grad():
        target = 0.5 * net(tr, ts)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        loss = ((net(tr, ts) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f'\nloss {losses[0]:.4f} -> {losses[-1]:.4f}')
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
