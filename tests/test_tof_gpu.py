"""TOFlow and SPyNetTOF on the GPU against the reference's own float64 results (tests/golden/g_zi_tof.npz,
tools/make_golden_tof.py): output and flows within 10x the reference's own fp32-versus-float64 distance, the rule DESIGN
section 16 uses for GFPGANv1OCR.  The margin covers the different summation order and the BatchNorm fold.  The measured ratio
(error / the reference's own distance) of each case is printed (run with -s)."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import image_restoration_amd as ira
from image_restoration_amd import _lib
from image_restoration_amd.archs.tof_arch import SPyNetTOF, TOFlow
from image_restoration_amd.utils import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tof_restate as T  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 10.0


@pytest.fixture(scope='module')
def fixture(golden):
    g = golden('g_zi_tof')
    sd = synth.tof_state_dict(int(g['weight_seed']))
    return g, sd


def _net(sd, cuda, adapt=False, frozen=True):
    """The fixture's network in eval mode; ``frozen``: no parameter requires grad, so a forward needs no graph and is not refused."""
    net = TOFlow(adapt_official_weights=adapt).eval()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return net.to(cuda).requires_grad_(not frozen)


@pytest.mark.parametrize('adapt', [False, True], ids=['adapt0', 'adapt1'])
@pytest.mark.parametrize('case', T.CASES, ids=[c[0] for c in T.CASES])
def test_toflow_matches_the_reference(cuda, fixture, case, adapt):
    g, sd = fixture
    tag, b, h, w = case
    net = _net(sd, cuda, adapt)
    x = torch.from_numpy(T.decode(g[f'{tag}_clip_u8'])).to(cuda)
    keep = {}
    out = net(x, keep)
    assert out.shape == (b, 3, h, w) and out.dtype == torch.float32 and out.grad_fn is None
    s = f'{tag}_adapt{int(adapt)}'
    err_o = float(np.abs(out.cpu().double().numpy() - g[s + '_out']).max())         # every pixel of every image
    err_f = float(np.abs(keep['flows'].cpu().double().numpy() - g[tag + '_flows']).max())
    d_o, d_f = float(g[s + '_out_fp32_dist']), float(g[s + '_flows_fp32_dist'])
    print(f'TOFlow {s}: output error {err_o:.3e} = {err_o / d_o:.2f} x the reference fp32 distance {d_o:.3e}; '
          f'flows {err_f:.3e} = {err_f / d_f:.2f} x {d_f:.3e}')
    assert err_o <= MARGIN * d_o and err_f <= MARGIN * d_f, (s, err_o / d_o, err_f / d_f)
    assert torch.equal(net(x), out)                                                 # a rerun is bit-identical


@pytest.mark.parametrize('case', T.CASES, ids=[c[0] for c in T.CASES])
def test_spynet_tof_alone_matches_the_reference(cuda, fixture, case):
    g, sd = fixture
    tag, b, h, w = case
    spy = SPyNetTOF().eval()
    spy.load_state_dict({k[len('spynet.'):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k.startswith('spynet.')}, strict=True)
    spy.to(cuda).requires_grad_(False)
    x = torch.from_numpy(T.decode(g[f'{tag}_clip_u8'])).to(cuda)
    mean, std = (torch.from_numpy(sd[k]).to(cuda) for k in ('mean', 'std'))
    clip = (x.view(-1, 3, h, w) - mean) / std                                   # TOFlow.normalize, as the caller does
    clip = clip.view(b, 7, 3, h, w)
    others = [0, 1, 2, 4, 5, 6]
    ref = clip[:, 3:4].expand(b, 6, 3, h, w).reshape(6 * b, 3, h, w)
    supp = clip[:, others].reshape(6 * b, 3, h, w)
    flow = spy(ref, supp)
    assert flow.shape == (6 * b, 2, h, w) and flow.grad_fn is None
    err, d = float(np.abs(flow.cpu().double().numpy() - g[tag + '_flows']).max()), float(g[f'{tag}_adapt0_flows_fp32_dist'])
    print(f'SPyNetTOF {tag}: flows {err:.3e} = {err / d:.2f} x the reference fp32 distance {d:.3e}')
    assert err <= MARGIN * d, (tag, err / d)
    one = spy(ref[4:5].contiguous(), supp[4:5].contiguous())
    assert torch.equal(one[0], flow[4])                                             # independent of the batch


def test_batch_of_two_equals_two_single_runs(cuda, fixture):
    g, sd = fixture
    for adapt in (False, True):
        net = _net(sd, cuda, adapt)
        x = torch.from_numpy(T.decode(T.clip_u8(3, 2, 32, 16))).to(cuda)
        k2, k0, k1 = {}, {}, {}
        both, a, b = net(x, k2), net(x[0:1], k0), net(x[1:2], k1)
        assert torch.equal(both, torch.cat([a, b])) and torch.equal(k2['flows'], torch.cat([k0['flows'], k1['flows']]))


def test_batchnorm_buffer_edit_is_seen_and_checkpoint_round_trips(cuda, fixture, tmp_path):
    g, sd = fixture
    tag, b, h, w = T.CASES[0]
    net = _net(sd, cuda)
    x = torch.from_numpy(T.decode(g[f'{tag}_clip_u8'])).to(cuda)
    before = net(x)
    key = 'spynet.basic_module.3.basic_module.1.running_var'
    with torch.no_grad():
        net.state_dict()[key].mul_(4.0)                                             # in place: the same storage, a new version
    after = net(x)
    sd2 = dict(sd)
    sd2[key] = (sd[key] * np.float32(4.0)).astype(np.float32)
    want, _ = T.toflow(sd2, T.decode(g[f'{tag}_clip_u8']))
    d = float(g[f'{tag}_adapt0_out_fp32_dist'])
    assert float((after - before).abs().max()) > 100 * d                            # the edit matters
    assert float(np.abs(after.cpu().double().numpy() - want).max()) <= MARGIN * d
    # round trip through a checkpoint file, strict
    path = str(tmp_path / 'tof.pth')
    torch.save({'params': net.state_dict()}, path)
    net2 = TOFlow().eval().requires_grad_(False)
    net2.load_state_dict(torch.load(path, map_location='cpu')['params'], strict=True)
    assert torch.equal(net2.to(cuda)(x), after)


def test_device_refusals(cuda, fixture):
    _, sd = fixture
    net = _net(sd, cuda, frozen=False)
    x = torch.zeros(1, 7, 3, 16, 16, device=cuda)
    with pytest.raises(ValueError, match=r'\[b, 7, 3, h, w\]'):
        net(x[:, :5])
    with pytest.raises(ValueError, match=r'\[b, 7, 3, h, w\]'):
        net(x.half())
    with pytest.raises(ValueError, match='multiple'):
        net(torch.zeros(1, 7, 3, 16, 24, device=cuda))
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        with torch.no_grad():
            net(x.cpu())
    with pytest.raises(NotImplementedError, match='inference'):
        net(x)                                                                      # grad enabled, parameters require grad
    with pytest.raises(NotImplementedError, match=r'\.eval\(\)'):
        with torch.no_grad():
            net.train()(x)
    net.eval()
    with torch.no_grad():
        assert net(x).shape == (1, 3, 16, 16)
    for p in net.parameters():
        p.requires_grad_(False)
    assert net(x).grad_fn is None                                                   # nothing requires grad: no graph is needed


def test_synthetic_option_file_runs_end_to_end(cuda, tmp_path):
    from image_restoration_amd.test import test_pipeline
    opt = yaml.safe_load(open(os.path.join(ROOT, 'options', 'test', 'TOF', 'test_TOF_synthetic.yml')))
    opt['name'] = 'tof_test'
    opt['datasets']['test'].update(num_samples=2, gt_size=32)
    p = tmp_path / 'opt.yml'
    yaml.safe_dump(opt, open(p, 'w'))
    model = test_pipeline(str(tmp_path), ['-opt', str(p)])
    assert type(model).__name__ == 'VideoBaseModel' and isinstance(model.net_g, TOFlow)
    assert list(model.metric_results) == ['00000000', '00000001']
    psnr = model.validation_summary['total']['psnr']
    assert np.isfinite(psnr) and psnr > 10.0, psnr
    assert isinstance(ira.build_network(dict(type='TOFlow', adapt_official_weights=True)), TOFlow)
