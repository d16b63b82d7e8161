"""SpyNet on the GPU against the reference's own float64 outputs (tests/golden/g_zd_spynet.npz, recorded by
tools/make_golden_spynet.py), level by level and at the output.  The bound of a case is 10 x the reference's own recorded
fp32-versus-float64 distance for that case (at its output), at every level and at the output — the project's standing margin: a
different summation order in fp32 is allowed, a wrong tap is not.  The distance the reference shows at each level is printed.  Weights and inputs come from the seeded
generators of tests/flow_restate.py, as in the tool."""
import os
import sys

import numpy as np
import pytest
import torch

import image_restoration_amd as ira
from image_restoration_amd.archs.spynet_arch import SpyNet

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = (('b2_64x64', 2, 64, 64), ('96x64', 1, 96, 64), ('64x96', 1, 64, 96), ('70x90', 1, 70, 90))
_nets = {}


def _net(g, cuda):
    if 'net' not in _nets:
        sd = R.spynet_weights(int(g['weight_seed']), float(g['last_scale']))
        assert R.weights_checksum(sd) == str(g['weight_checksum'])
        net = SpyNet().to(cuda).eval()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        _nets['net'] = net
    return _nets['net']


def _inputs(g, tag, n, h, w, cuda):
    ref, supp = R.spynet_inputs(int(g['input_seed']) + [c[0] for c in CASES].index(tag), n, h, w)
    return torch.from_numpy(ref).to(cuda), torch.from_numpy(supp).to(cuda)


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_spynet_matches_the_reference_level_by_level(golden, cuda, case):
    g = golden('g_zd_spynet')
    tag, n, h, w = case
    net = _net(g, cuda)
    ref, supp = _inputs(g, tag, n, h, w, cuda)
    levels = []
    with torch.no_grad():
        out = net.run_forward(ref, supp, levels)
    assert len(levels) == 6 and tuple(out.shape) == (n, 2, h, w)
    dist = g[f'spy_{tag}_fp32_dist']
    for lv in range(5):
        err = float(np.abs(levels[lv].cpu().double().numpy() - g[f'spy_{tag}_level{lv}']).max())
        print(f'{tag} level {lv}: max error {err:.3e}, reference fp32 distance at this level {dist[lv]:.3e}')
        assert err <= 10 * dist[6], (tag, lv, err, dist[6])
    err = float(np.abs(out.cpu().double().numpy() - g[f'spy_{tag}_out']).max())
    print(f'{tag} output: max error {err:.3e}, reference fp32 distance {dist[6]:.3e}')
    assert err <= 10 * dist[6], (tag, err, dist[6])
    assert torch.equal(out, net(ref, supp))                       # forward() is run_forward


def test_spynet_inference_contract(golden, cuda, tmp_path):
    g = golden('g_zd_spynet')
    net = _net(g, cuda)
    ref, supp = _inputs(g, 'b2_64x64', 2, 64, 64, cuda)
    assert any(p.requires_grad for p in net.parameters()) and torch.is_grad_enabled()
    out = net(ref, supp)                                          # eval mode needs no torch.no_grad()
    assert out.grad_fn is None and not out.requires_grad and out.dtype == torch.float32
    # batch 2 is two batch-1 forwards, bit for bit
    one = torch.cat([net(ref[i:i + 1], supp[i:i + 1]) for i in range(2)], 0)
    assert torch.equal(out, one)
    # a forward that would need a graph is refused and names the follow-up
    net.train()
    try:
        with pytest.raises(NotImplementedError, match='backward'):
            net(ref, supp)
        with torch.no_grad():
            assert torch.equal(net(ref, supp), out)
    finally:
        net.eval()
    # a {'params': ...} checkpoint round trip through load_path, and the registry
    path = str(tmp_path / 'spynet.pth')
    torch.save({'params': {k: v.cpu() for k, v in net.state_dict().items() if k not in ('mean', 'std')}}, path)
    again = ira.build_network(dict(type='SpyNet', load_path=path)).to(cuda).eval()
    assert isinstance(again, SpyNet) and torch.equal(again(ref, supp), out)
    # in-place parameter updates are seen by the pack cache
    with torch.no_grad():
        again.basic_module[5].basic_module[8].bias.add_(1.0)
    moved = again(ref, supp)
    assert float((moved - out).abs().max()) > 0.5
    with pytest.raises(ValueError, match='too small'):
        net(ref[:, :, :32], supp[:, :, :32])
