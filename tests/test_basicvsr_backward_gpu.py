"""BasicVSR's training path on the GPU: ``set_autograd(True)``, the two chained autograd Functions, the gradients of every
parameter and of the flows passed to ``propagate``, the contracts around them and the two optimiser routes.

Yardstick: tests/vsr_grad_restate.py in float64, forced with the device's own activation masks (from what the training forward
kept) and the warp cells of the fp32 flows, so that both sides differentiate the same piece of the function.  Relative L2 per
tensor; bound: 10 x the distance the fp32 torch restatement shows on the CPU against float64 when both are forced with the fp32
run's own masks and cells (the largest over the tensors of the case) — the project's standing margin over a measured fp32
distance.  The whole-network test compares the ``spynet.*`` gradients of ``net(x)`` with the same flow gradients fed through
SpyNet's Function by hand; the only difference either way is the order of the float atomics upstream, so its bound is 10 x the
relative L2 between two runs of the by-hand path.  Every figure is printed next to its bound."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import image_restoration_amd as ira
from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H
from image_restoration_amd.archs.spynet_autograd import spynet_apply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as FR  # noqa: E402
import vsr_grad_restate as G  # noqa: E402

pytestmark = pytest.mark.gpu

TAGS = [c[0] for c in G.CASES]
SPYNET_BWD_IDS = set(range(169, 177))
PROP_BWD_ID = 178
_cache = {}


def _case(golden, cuda, tag):
    """Per case, built once: the network with the seeded weights in train mode with autograd on, the clip, the fixture's flows,
    the seeded g — and the CPU yardstick."""
    if tag in _cache:
        return _cache[tag]
    fix = golden('g_ze_basicvsr')
    _, b, n, h, w, nf, nb = G.case(tag)
    sd, x, ff, fb = G.case_data(fix, tag)
    full = {'spynet.' + k: v for k, v in FR.spynet_weights(int(fix['spynet_seed']), float(fix['spynet_scale'])).items()}
    full.update(sd)
    net = ira.build_network(dict(type='BasicVSR', num_feat=nf, num_block=nb)).to(cuda)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in full.items()}, strict=True)
    net.train().set_autograd(True)
    g = G.grad_output(tag)
    c = dict(net=net, sd=sd, x=x, ff=ff, fb=fb, g=g, xd=torch.from_numpy(x).to(cuda), gd=torch.from_numpy(g).float().to(cuda),
             names=list(sd), shape=(b, n, h, w, nf, nb))
    # the yardstick: fp32 torch on the CPU against float64, both on the fp32 run's own masks and cells
    own = {}
    cpu32, _ = G.gradients(sd, x, ff, fb, g.astype(np.float32), nb, dtype=torch.float32, record=own)
    cpu64, _ = G.gradients(sd, x, ff, fb, g, nb, forced=own)
    c['cpu_dist'] = max(G.rel_l2(cpu32, cpu64).values())
    _cache[tag] = c
    return c


def _forced(c, keep, ff, fb):
    """What pins the kinks of one training forward: the device's masks from ``keep``, the cells from the fp32 flows."""
    b, n, h, w, nf, nb = c['shape']
    cfg = H.vsr_trunk_cfg(nf, nb, 1)
    masks, cells = {}, {}
    for branch in ('backward', 'forward'):
        for i, (tin, stack) in keep[branch].items():
            acts = H.vsr_trunk_stack_views(cfg, stack, b, h, w)
            masks[(branch, i)] = [G.cb8_to_nchw(acts[0].buf) > 0] + [G.cb8_to_nchw(acts[1 + 2 * k].buf) > 0 for k in range(nb)]
    head = [np.concatenate([G.cb8_to_nchw(acts[k].buf) for _, _, acts in keep['head']]) > 0 for k in range(4)]
    for i in range(n):
        masks[('head', i)] = [m[i * b:(i + 1) * b] for m in head]
        if i < n - 1:
            cells[('backward', i)] = G.cells_of(fb[:, i])
        if i > 0:
            cells[('forward', i)] = G.cells_of(ff[:, i - 1])
    return dict(masks=masks, cells=cells)


def _zero_grad(net):
    for p in net.parameters():
        p.grad = None


def _leaves_run(c, ff_np, fb_np, cuda):
    """One propagate with the two flow tensors as leaves and L = sum(y * g): ({name: gradient as float64 numpy}, y)."""
    net = c['net']
    _zero_grad(net)
    ff = torch.from_numpy(ff_np).to(cuda).requires_grad_()
    fb = torch.from_numpy(fb_np).to(cuda).requires_grad_()
    y = net.propagate(c['xd'], ff, fb)
    assert y.grad_fn is not None
    (y * c['gd']).sum().backward()
    got = {k: dict(net.named_parameters())[k].grad.double().cpu().numpy() for k in c['names']}
    got.update(flows_forward=ff.grad.double().cpu().numpy(), flows_backward=fb.grad.double().cpu().numpy())
    return got, y.detach()


def _check_against_restatement(c, got, keep, ff, fb, what, skip=()):
    b, n, h, w, nf, nb = c['shape']
    want, _ = G.gradients(c['sd'], c['x'], ff, fb, c['g'], nb, forced=_forced(c, keep, ff, fb))
    dist = {k: v for k, v in G.rel_l2(got, {k: v for k, v in want.items() if k in got}).items() if k not in skip}
    worst = max(dist, key=dist.get)
    print(f'{what}: device vs forced float64 {dist[worst]:.3e} ({worst}), CPU fp32 forced {c["cpu_dist"]:.3e}, '
          f'bound {10 * c["cpu_dist"]:.3e}')
    assert dist[worst] <= 10 * c['cpu_dist'], dist
    return dist[worst]


@pytest.mark.parametrize('tag', TAGS)
def test_flows_as_leaves_against_the_forced_restatement(cuda, golden, tag):
    """Measured on the MI355X (worst tensor: device vs forced float64 | CPU fp32 forced | bound):
        b1_n3_33x40:  2.74e-06 (flows_forward)  | 2.53e-06 | 2.53e-05
        b2_n2_34x33:  1.37e-06 (flows_backward) | 1.28e-06 | 1.28e-05"""
    c = _case(golden, cuda, tag)
    b, n, h, w, nf, nb = c['shape']
    got, y = _leaves_run(c, c['ff'], c['fb'], cuda)
    assert len(c['names']) == 2 * 2 * (1 + 2 * nb) + 10 and len(got) == len(c['names']) + 2
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in got.values())
    assert all(p.grad is None for k, p in c['net'].named_parameters() if k.startswith('spynet.'))     # reached through the flows only
    keep = {}
    y_keep = c['net'].run_forward(c['xd'], torch.from_numpy(c['ff']).to(cuda), torch.from_numpy(c['fb']).to(cuda), keep=keep)
    assert torch.equal(y_keep, y) and set(keep) == {'x', 'flows_forward', 'flows_backward', 'feats', 'backward', 'forward', 'head'}
    assert sorted(keep['backward']) == sorted(keep['forward']) == list(range(n)) and all(len(a) == 4 for _, _, a in keep['head'])
    _check_against_restatement(c, got, keep, c['ff'], c['fb'], f'{tag} flows as leaves')


def _own_flows(c):
    with torch.no_grad():
        ff, fb = c['net'].get_flow(c['xd'])
    return ff.cpu().numpy(), fb.cpu().numpy()


def _spynet_by_hand(c, dff, dfb, cuda):
    """The flow gradients fed through SpyNet's Function by hand: {spynet.* name: gradient}."""
    net, x = c['net'], c['xd']
    b, n, _, h, w = x.shape
    _zero_grad(net)
    x_1, x_2 = x[:, :-1].reshape(-1, 3, h, w), x[:, 1:].reshape(-1, 3, h, w)
    flows = spynet_apply(net.spynet, torch.cat([x_1, x_2]), torch.cat([x_2, x_1]))       # [backward pairs, forward pairs]
    gflow = torch.cat([torch.from_numpy(dfb).float().reshape(-1, 2, h, w), torch.from_numpy(dff).float().reshape(-1, 2, h, w)]).to(cuda)
    flows.backward(gflow)
    return {k: p.grad.double().cpu().numpy() for k, p in net.named_parameters() if k.startswith('spynet.')}


@pytest.mark.parametrize('tag', TAGS)
def test_whole_network_joins_the_two_functions(cuda, golden, tag):
    """Measured on the MI355X (worst spynet.* tensor of net(x) vs by hand | two by-hand runs | bound):
        b1_n3_33x40:  6.85e-07 | 7.91e-07 | 7.91e-06
        b2_n2_34x33:  0 | 0 | 0    with two frames the only warped step of a branch is the first one its backward visits: no
                                   scatter lies upstream of a flow gradient, and everything on the way is bit-reproducible"""
    c = _case(golden, cuda, tag)
    net = c['net']
    _zero_grad(net)
    y = net(c['xd'])
    assert y.grad_fn is not None and y.requires_grad
    (y * c['gd']).sum().backward()
    whole = {k: p.grad.double().cpu().numpy() for k, p in net.named_parameters() if k.startswith('spynet.')}
    assert len(whole) == 60 and all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in whole.values())
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in net.parameters())
    # by hand, twice: propagate on the network's own flows as leaves, then SpyNet's Function on the flow gradients
    ff, fb = _own_flows(c)
    hands = []
    for _ in range(2):
        got, _ = _leaves_run(c, ff, fb, cuda)
        hands.append(_spynet_by_hand(c, got['flows_forward'], got['flows_backward'], cuda))
    runs = max(G.rel_l2(hands[1], hands[0]).values())
    dist = G.rel_l2(whole, hands[0])
    worst = max(dist, key=dist.get)
    print(f'{tag} whole network: spynet.* of net(x) vs by hand {dist[worst]:.3e} ({worst}); two by-hand runs {runs:.3e}, bound {10 * runs:.3e}')
    assert dist[worst] <= 10 * runs, dist


def _records(lib, fn):
    _lib.check(lib.sr_profile_start(4096), 'sr_profile_start')
    try:
        fn()
    finally:
        recs = (_lib.LaunchRecord * 4096)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, 4096, C.byref(cnt)), 'sr_profile_stop')
    return [recs[i] for i in range(min(cnt.value, 4096))]


@pytest.mark.parametrize('tag', TAGS)
def test_spynet_frozen(cuda, golden, tag):
    c = _case(golden, cuda, tag)
    net, lib = c['net'], _lib.load()
    b, n, h, w, nf, nb = c['shape']
    for p in net.spynet.parameters():
        p.requires_grad_(False)
    try:
        _zero_grad(net)
        ff, fb = net.get_flow(c['xd'])
        assert ff.grad_fn is None and fb.grad_fn is None and not ff.requires_grad
        box = []
        recs = _records(lib, lambda: box.append(net(c['xd'])))
        recs += _records(lib, lambda: (box[0] * c['gd']).sum().backward())
        ids = [r.kernel_id for r in recs]
        assert not SPYNET_BWD_IDS & set(ids)                              # no SpyNet backward kernel
        steps = [r for r in recs if r.kernel_id == PROP_BWD_ID]
        assert len(steps) == 2 * (n - 1)
        assert all(r.flops == 8.0 * b * h * w * nf for r in steps)        # the scatter alone: no dflow work
        assert all(p.grad is None for p in net.spynet.parameters())
        got = {k: dict(net.named_parameters())[k].grad.double().cpu().numpy() for k in c['names']}
        keep = {}
        ffn, fbn = ff.cpu().numpy(), fb.cpu().numpy()
        with torch.no_grad():
            net.run_forward(c['xd'], ff, fb, keep=keep)
        _check_against_restatement(c, got, keep, ffn, fbn, f'{tag} spynet frozen')
    finally:
        for p in net.spynet.parameters():
            p.requires_grad_(True)


def test_contracts(cuda, golden):
    c = _case(golden, cuda, TAGS[1])
    net, x, gd = c['net'], c['xd'], c['gd']
    try:
        # eval() and no_grad keep the inference path; the training forward's output is the inference output, bit for bit
        net.eval()
        y_eval = net(x)
        assert y_eval.grad_fn is None and not y_eval.requires_grad
        net.train()
        with torch.no_grad():
            y_ng = net(x)
        assert y_ng.grad_fn is None and torch.equal(y_ng, y_eval)
        _zero_grad(net)
        y = net(x)
        assert y.grad_fn is not None and torch.equal(y.detach(), y_eval)
        # a second backward without zero_grad accumulates into .grad
        (y * gd).sum().backward()
        first = {k: p.grad.clone() for k, p in net.named_parameters()}
        (net(x) * gd).sum().backward()
        for k, p in net.named_parameters():
            rel = float((p.grad - 2 * first[k]).norm() / (2 * first[k]).norm())
            assert rel <= 1e-4, (k, rel)                                 # twice the first, up to the order of the atomics
        # a clip that requires grad is refused; set_autograd(False) restores the refusal
        with pytest.raises(NotImplementedError, match='frames are data'):
            net(x.clone().requires_grad_())
        assert net.set_autograd(False) is net and net.spynet._autograd is False
        with pytest.raises(NotImplementedError, match='follow-up'):
            net(x)
        with torch.no_grad():
            assert torch.equal(net(x), y_eval)
    finally:
        net.train().set_autograd(True)
        _zero_grad(net)


def test_flat_adam_arena_receives_the_gradients(cuda, golden):
    from image_restoration_amd import optim
    c = _case(golden, cuda, TAGS[1])
    ref, x, gd = c['net'], c['xd'], c['gd']
    b, n, h, w, nf, nb = c['shape']
    runs = []
    for _ in range(2):
        _zero_grad(ref)
        (ref(x) * gd).sum().backward()
        runs.append({k: p.grad.double().cpu().numpy() for k, p in ref.named_parameters()})
    again = max(G.rel_l2(runs[1], runs[0]).values())
    net = ira.build_network(dict(type='BasicVSR', num_feat=nf, num_block=nb)).to(cuda)
    net.load_state_dict(ref.state_dict(), strict=True)
    net.train().set_autograd(True)
    adam = optim.FlatAdam(list(net.parameters()), lr=1e-4, betas=(0.9, 0.99), modules=[net])
    assert net._grad_sink is not None
    adam.zero_grad()
    (net(x) * gd).sum().backward()
    arena = {k: p.grad.double().cpu().numpy() for k, p in net.named_parameters()}
    dist = G.rel_l2(arena, runs[0])
    worst = max(dist, key=dist.get)
    print(f'arena vs autograd-mode gradients {dist[worst]:.3e} ({worst}); two autograd-mode runs {again:.3e}, bound {10 * again:.3e}')
    assert dist[worst] <= 10 * again, dist


def test_ten_adam_steps_lower_an_l1_loss(cuda, golden):
    c = _case(golden, cuda, TAGS[1])
    b, n, h, w, nf, nb = c['shape']
    net = ira.build_network(dict(type='BasicVSR', num_feat=nf, num_block=nb)).to(cuda)
    net.load_state_dict(c['net'].state_dict(), strict=True)
    net.train().set_autograd(True)
    x = c['xd']
    gen = torch.Generator().manual_seed(3)
    target = torch.rand((b, n, 3, 4 * h, 4 * w), generator=gen).to(cuda)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = (net(x) - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float((net(x) - target).abs().mean()))
    print('L1 losses over ten Adam steps:', ' '.join(f'{v:.5f}' for v in losses))
    assert losses[-1] < losses[0]
