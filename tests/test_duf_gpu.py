"""DUF on the GPU against the reference's own float64 results (tests/golden/g_zj_duf.npz, tools/make_golden_duf.py): every pixel
within 10x the reference's own fp32-versus-float64 distance, the rule of tests/test_tof_gpu.py.  The margin covers the different
summation order, the BatchNorm fold and prologue arrays, and the device's expf.  The measured ratio (error / the reference's own
distance) of each case is printed (run with -s)."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import image_restoration_amd as ira
from image_restoration_amd import _lib
from image_restoration_amd.archs.duf_arch import DUF, DynamicUpsamplingFilter
from image_restoration_amd.utils import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import duf_restate as D  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 10.0


@pytest.fixture(scope='module')
def g(golden):
    return golden('g_zj_duf')


def _net(seed, num_layer, scale, adapt, cuda, frozen=True, sd=None):
    """The fixture's network in eval mode; ``frozen``: no parameter requires grad, so a forward needs no graph and is not refused."""
    sd = synth.duf_state_dict(seed, num_layer, scale) if sd is None else sd
    net = DUF(scale, num_layer, adapt).eval()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return net.to(cuda).requires_grad_(not frozen)


@pytest.mark.parametrize('case', D.CASES, ids=[c[0] for c in D.CASES])
def test_duf_matches_the_reference(cuda, g, case):
    tag, num_layer, scale, b, h, w, adapt = case
    net = _net(int(g['weight_seed']), num_layer, scale, adapt, cuda)
    x = torch.from_numpy(D.decode(g[f'{tag}_clip_u8'])).to(cuda)
    keep = {}
    out = net(x, keep)
    assert out.shape == (b, 3, scale * h, scale * w) and out.dtype == torch.float32 and out.grad_fn is None
    err, d = float(np.abs(out.cpu().double().numpy() - g[tag + '_out']).max()), float(g[tag + '_fp32_dist'])   # every pixel
    line = f'DUF {tag}: output error {err:.3e} = {err / d:.2f} x the reference fp32 distance {d:.3e}'
    if tag + '_logits' in g:                                                          # where a failure would come from
        el = float(np.abs(keep['logits'].cpu().double().numpy() - g[tag + '_logits']).max())
        er = float(np.abs(keep['res'].cpu().double().numpy() - g[tag + '_res']).max())
        line += f'; logits {el:.3e}, res {er:.3e}'
    print(line)
    assert err <= MARGIN * d, (tag, err / d)
    assert torch.equal(net(x), out)                                                   # a rerun is bit-identical


def test_batch_of_two_equals_two_single_runs(cuda, g):
    tag, num_layer, scale, b, h, w, adapt = D.CASES[0]
    net = _net(int(g['weight_seed']), num_layer, scale, adapt, cuda)
    x = torch.from_numpy(D.decode(g[f'{tag}_clip_u8'])).to(cuda)
    assert b == 2 and torch.equal(net(x), torch.cat([net(x[0:1]), net(x[1:2])]))


def test_batchnorm_buffer_edit_is_seen_and_checkpoint_round_trips(cuda, g, tmp_path):
    tag, num_layer, scale, b, h, w, adapt = D.CASES[0]
    sd = synth.duf_state_dict(int(g['weight_seed']), num_layer, scale)
    net = _net(0, num_layer, scale, adapt, cuda, sd=sd)
    x = torch.from_numpy(D.decode(g[f'{tag}_clip_u8'])).to(cuda)
    before = net(x)
    d = float(g[tag + '_fp32_dist'])
    # one BatchNorm that becomes a prologue, one that is folded into the 1x1x1 conv
    for key in ('dense_block1.dense_blocks.1.0.running_var', 'dense_block2.temporal_reduce2.3.running_var'):
        with torch.no_grad():
            net.state_dict()[key].mul_(4.0)                                           # in place: the same storage, a new version
        after = net(x)
        sd = dict(sd)
        sd[key] = (sd[key] * np.float32(4.0)).astype(np.float32)
        want = D.duf(sd, D.decode(g[f'{tag}_clip_u8']), num_layer, scale, adapt)
        assert float((after - before).abs().max()) > 100 * d, key                    # the edit matters
        assert float(np.abs(after.cpu().double().numpy() - want).max()) <= MARGIN * d, key
        before = after
    path = str(tmp_path / 'duf.pth')
    torch.save({'params': net.state_dict()}, path)
    net2 = DUF(scale, num_layer, adapt).eval().requires_grad_(False)
    net2.load_state_dict(torch.load(path, map_location='cpu')['params'], strict=True)
    assert torch.equal(net2.to(cuda)(x), after)


@pytest.mark.parametrize('s', [2, 3, 4])
def test_dynamic_upsampling_filter_alone(cuda, s):
    rng = np.random.default_rng(s)
    n, h, w = 2, 6, 11
    x = rng.uniform(0, 1, (n, 3, h, w)).astype(np.float32)
    f = D.softmax_taps(rng.standard_normal((n, 25, s * s, h, w)) * 3).astype(np.float32)
    want = D.dynamic_filter(x, f)
    mod = DynamicUpsamplingFilter((5, 5))
    got = mod(torch.from_numpy(x).to(cuda), torch.from_numpy(f).to(cuda))
    assert got.shape == (n, 3 * s * s, h, w) and got.dtype == torch.float32
    # 25 products and 25 additions of values in [0, 1] with weights that sum to 1: (25 + 1) * 2^-24 to first order
    assert float(np.abs(got.cpu().double().numpy() - want).max()) <= 26 * 2.0 ** -24
    with pytest.raises(ValueError, match='filters'):
        mod(torch.from_numpy(x).to(cuda), torch.from_numpy(f[:, :24]).to(cuda))
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        mod(torch.from_numpy(x), torch.from_numpy(f))


def test_device_refusals(cuda):
    net = DUF(4, 16).to(cuda).eval()
    x = torch.zeros(1, 7, 3, 8, 8, device=cuda)
    for bad in (x[:, :5], x[:, :, :2], x[0], x.half()):
        with pytest.raises(ValueError, match=r'\[b, 7, 3, h, w\]'):
            net(bad)
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        with torch.no_grad():
            net(x.cpu())
    with pytest.raises(NotImplementedError, match='inference'):
        net(x)                                                                        # grad enabled, parameters require grad
    with pytest.raises(NotImplementedError, match=r'\.eval\(\)'):
        with torch.no_grad():
            net.train()(x)
    net.eval()
    with torch.no_grad():
        assert net(x).shape == (1, 3, 32, 32)
    net.requires_grad_(False)
    assert net(x).grad_fn is None                                                     # nothing requires grad: no graph is needed


def test_synthetic_option_file_runs_end_to_end(cuda, tmp_path):
    from image_restoration_amd.test import test_pipeline
    opt = yaml.safe_load(open(os.path.join(ROOT, 'options', 'test', 'DUF', 'test_DUF_synthetic.yml')))
    opt['name'] = 'duf_test'
    opt['datasets']['test'].update(num_samples=2, gt_size=32)
    p = tmp_path / 'opt.yml'
    yaml.safe_dump(opt, open(p, 'w'))
    model = test_pipeline(str(tmp_path), ['-opt', str(p)])
    assert type(model).__name__ == 'VideoBaseModel' and isinstance(model.net_g, DUF) and model.net_g.num_layer == 16
    assert list(model.metric_results) == ['00000000', '00000001']
    psnr = model.validation_summary['total']['psnr_y']
    assert np.isfinite(psnr), psnr
    assert isinstance(ira.build_network(dict(type='DUF', scale=2, num_layer=28)), DUF)
