"""BasicVSR on the GPU against the reference's own outputs (tests/golden/g_ze_basicvsr.npz) and its contracts.

Bounds.  Direct route: 10 x the reference's recorded fp32-versus-float64 distance of the case — the project's standing margin: a
different fp32 summation order passes, a wrong tap or frame does not (the fixture tool asserts that zeroed flows or zeroed backward
features move the output by >= 100 x that distance) — plus 2^-24 * |value|, because the fixture stores float64 outputs rounded to
fp32.  Forced Winograd in the trunks: err_on <= 4 * err_off + 2^-20 on the direct route's measured error (tests/test_wino_f32_gpu.py
has the derivation).  Every measured error is printed next to its bound.
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
def state(golden):
    g = golden('g_ze_basicvsr')
    sd = {'spynet.' + k: v for k, v in FR.spynet_weights(int(g['spynet_seed']), float(g['spynet_scale'])).items()}
    sd.update(V.basicvsr_weights(int(g['weight_seed']), V.NUM_FEAT, V.NUM_BLOCK, float(g['trunk_scale'])))
    assert FR.weights_checksum(sd) == str(g['weight_checksum'])
    return g, {k: torch.from_numpy(v) for k, v in sd.items()}


@pytest.fixture(scope='module')
def net(cuda, state):
    net = ira.build_network(dict(type='BasicVSR', num_feat=V.NUM_FEAT, num_block=V.NUM_BLOCK)).to(cuda).eval()
    net.load_state_dict(state[1], strict=True)
    return net


def _clip(g, tag, dev):
    idx = [c[0] for c in V.CASES].index(tag)
    _, b, n, h, w = V.CASES[idx]
    return torch.from_numpy(V.clip_input(int(g['input_seed']) + idx, b, n, h, w)).to(dev)


def _err(y, want, lattice):
    """(max |y - want| on the fixture's lattice, the part of the bound that comes from the fixture's fp32 rounding)."""
    oy, ox, st = (int(v) for v in lattice)
    got = y[..., oy::st, ox::st].double().cpu().numpy()
    assert got.shape == want.shape
    return float(np.abs(got - want).max()), float(2.0 ** -24 * np.abs(want).max())


@pytest.mark.parametrize('case', V.CASES, ids=[c[0] for c in V.CASES])
def test_network_against_the_reference(cuda, lib, net, state, case):
    g = state[0]
    tag, b, n, h, w = case
    x = _clip(g, tag, cuda)
    ff, fb = torch.from_numpy(g[tag + '_flows_forward']).to(cuda), torch.from_numpy(g[tag + '_flows_backward']).to(cuda)
    want, dist = g[tag + '_out'].astype(np.float64), float(g[tag + '_fp32_dist'])
    errs = {}
    try:
        for mode in (0, 3):
            lib.sr_dev_set_wino_f32(mode)
            y_prop, y_fwd = net.propagate(x, ff, fb), net(x)
            assert y_prop.shape == y_fwd.shape == (b, n, 3, 4 * h, 4 * w) and y_prop.grad_fn is None
            errs[mode] = (_err(y_prop, want, g[tag + '_lattice']), _err(y_fwd, want, g[tag + '_lattice']))
    finally:
        lib.sr_dev_set_wino_f32(1)
    bad = []
    for k, route in enumerate(('propagate', 'forward')):
        e0, rnd = errs[0][k]
        e3, _ = errs[3][k]
        b0, b3 = 10 * dist + rnd, 4 * e0 + 2.0 ** -20
        print(f'{tag} {route}: direct err {e0:.3e} bound {b0:.3e} | forced Winograd err {e3:.3e} bound {b3:.3e} '
              f'(reference fp32 distance {dist:.3e})')
        if e0 > b0:
            bad.append(f'{route} direct {e0:.3e} > {b0:.3e}')
        if e3 > b3:
            bad.append(f'{route} forced Winograd {e3:.3e} > {b3:.3e}')
    assert not bad, bad
    # the flows of the project's own SpyNet are the fixture's within 10 x the reference's own fp32 distance of SpyNet (below 2e-5 px, g_zd_spynet)
    gf, gb = net.get_flow(x)
    assert float((gf - ff).abs().max()) <= 2e-4 and float((gb - fb).abs().max()) <= 2e-4


def test_contracts(cuda, lib, net, state, tmp_path):
    g = state[0]
    x = _clip(g, V.CASES[1][0], cuda)                       # b = 2, n = 2, 34x33
    y = net(x)
    # forward is propagate after get_flow, bit for bit; eval mode needs no no_grad
    ff, fb = net.get_flow(x)
    assert ff.shape == fb.shape == (2, 1, 2, 34, 33)
    assert torch.equal(net.propagate(x, ff, fb), y) and y.grad_fn is None and not y.requires_grad
    # batch 2 is two batch-1 clips, bit for bit
    for k in range(2):
        assert torch.equal(net(x[k:k + 1]), y[k:k + 1]), k
    # train mode with grad refuses, and names training; no_grad in train mode runs
    net.train()
    try:
        with pytest.raises(NotImplementedError, match='follow-up'):
            net(x)
        with torch.no_grad():
            assert torch.equal(net(x), y)
    finally:
        net.eval()
    # a checkpoint round trip through build_network with spynet_path
    spy = str(tmp_path / 'spynet.pth')
    torch.save({'params': {k: v.cpu() for k, v in net.spynet.state_dict().items() if k not in ('mean', 'std')}}, spy)
    ckpt = str(tmp_path / 'net.pth')
    torch.save({'params': {k: v.cpu() for k, v in net.state_dict().items()}}, ckpt)
    torch.manual_seed(1)
    other = ira.build_network(dict(type='BasicVSR', num_feat=V.NUM_FEAT, num_block=V.NUM_BLOCK, spynet_path=spy)).to(cuda).eval()
    assert torch.equal(other.get_flow(x)[0], ff) and not torch.equal(other(x), y)       # SpyNet loaded, the rest is fresh
    other.load_state_dict(torch.load(ckpt)['params'], strict=True)
    assert torch.equal(other(x), y)
    # an in-place update of one trunk weight is seen by the next forward (and undone again)
    wt = other.forward_trunk.main[2][1].conv2.weight
    with torch.no_grad():
        wt.mul_(1.5)
    y2 = other(x)
    assert not torch.equal(y2, y)
    with torch.no_grad():
        wt.div_(1.5)
        other.backward_trunk.main[0].bias.add_(0.25)
    assert not torch.equal(other(x), y) and not torch.equal(other(x), y2)
