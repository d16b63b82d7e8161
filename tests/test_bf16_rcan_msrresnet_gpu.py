"""The bf16 forward of RCAN and MSRResNet on the MI355X against a float64 model of bf16 storage.

The yardstick follows tests/test_edsr_gpu.py: a float64 restatement of each network with a bf16 round trip wherever the HIP
path stores a tensor (the shifted or converted input, every conv output after its epilogue, the excite output, the packed conv
weights) and none where it does not (the attention's p, h, s and its fp32 weights, conv_last's output, MSRResNet's bilinear
base).  The exact restatement is first shown to reproduce the fixtures; then
    max|y_hip - y64| <= 2 * max|y_model - y64| + 4 fp32 ulp of max|y64|.
The model accumulates exactly and the kernels in fp32; what separates them is values that round the other way at a bf16 tie."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import image_restoration_amd as ira
from image_restoration_amd import _lib
from image_restoration_amd.utils import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23
RCAN_SMALL = dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_group=2, num_block=2, squeeze_factor=4)
RCAN_BIG = dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_group=10, num_block=20, squeeze_factor=16, upscale=4)
MSR_BIG = dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=16, upscale=4)
# launch-profiler ids of the bf16 path: sr_conv3x3_bf16's kernels, the CB16 shuffle, the attention
BF16_IDS = set(range(16, 32)) | {42, 43, 50, 64, 98, 102, 103, 104}


def _ident(t):
    return t


def _bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _sd_t(sd, dt):
    return {k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in sd.items()}


def _load(net, sd, dev):
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return net.to(dev)


def _stages(s):
    return [(0, 3)] if s == 3 else [(2 * k, 2) for k in range(int(round(np.log2(s))))]


# ---------------------------------------------------------------------------------------------------- float64 restatements
def restate_rcan(x, sd, cfg, r=_ident, rw=_ident):
    """RCAN.forward from the reference's layer list (rcan_arch.py:8-135) in the dtype of ``x`` and ``sd``.  ``r`` is applied
    wherever the bf16 path stores an activation, ``rw`` to every 3x3 conv weight; the attention's weights stay as they are."""
    def cv(t, name):
        return F.conv2d(t, rw(sd[name + '.weight']), sd[name + '.bias'], padding=1)
    mean = torch.tensor(cfg.get('rgb_mean', (0.4488, 0.4371, 0.4040)), dtype=torch.float32).to(x.dtype).view(1, 3, 1, 1)
    rng, rs = cfg.get('img_range', 255.), cfg.get('res_scale', 1)
    x0 = feat = r(cv(r((x - mean) * rng), 'conv_first'))
    for g in range(cfg['num_group']):
        g_in = feat
        for b in range(cfg['num_block']):
            pre = f'body.{g}.residual_group.{b}.rcab.'
            u = r(cv(r(torch.relu(cv(feat, pre + '0'))), pre + '2'))
            p = u.mean((2, 3), keepdim=True)
            hid = torch.relu(F.conv2d(p, sd[pre + '3.attention.1.weight'], sd[pre + '3.attention.1.bias']))
            s = torch.sigmoid(F.conv2d(hid, sd[pre + '3.attention.3.weight'], sd[pre + '3.attention.3.bias']))
            feat = r(feat + rs * (u * s))
        feat = r(cv(feat, f'body.{g}.conv') + g_in)
    feat = r(cv(feat, 'conv_after_body') + x0)
    for idx, f in _stages(cfg['upscale']):
        feat = F.pixel_shuffle(r(cv(feat, f'upsample.{idx}')), f)
    return cv(feat, 'conv_last') / rng + mean


def restate_msr(x, sd, cfg, r=_ident, rw=_ident):
    """MSRResNet.forward from the reference's layer list (srresnet_arch.py:9-68); ``r`` / ``rw`` as in restate_rcan.  The
    bilinear base comes from the unrounded input."""
    def cv(t, name):
        return F.conv2d(t, rw(sd[name + '.weight']), sd[name + '.bias'], padding=1)
    s = cfg['upscale']
    feat = r(F.leaky_relu(cv(r(x), 'conv_first'), 0.1))
    for b in range(cfg['num_block']):
        feat = r(feat + cv(r(torch.relu(cv(feat, f'body.{b}.conv1'))), f'body.{b}.conv2'))
    for name, f in ([('upconv1', 2), ('upconv2', 2)] if s == 4 else [('upconv1', s)]):
        feat = r(F.leaky_relu(F.pixel_shuffle(cv(feat, name), f), 0.1))   # (the activation and r commute with the shuffle)
    out = cv(r(F.leaky_relu(cv(feat, 'conv_hr'), 0.1)), 'conv_last')
    return out + F.interpolate(x, scale_factor=s, mode='bilinear', align_corners=False)


def _rcan_cfg(s):
    return dict(RCAN_SMALL, upscale=s)


def _msr_cfg(s):
    return dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=2, upscale=s)


def _rcan_small(s, dev, **kw):
    cfg = _rcan_cfg(s)
    return _load(ira.build_network(dict(type='RCAN', **cfg, **kw)), synth.rcan_state_dict(200 + s, **cfg), dev)


def _msr_small(s, dev, **kw):
    cfg = _msr_cfg(s)
    return _load(ira.build_network(dict(type='MSRResNet', **cfg, **kw)), synth.msrresnet_state_dict(100 + s, **cfg), dev)


def _big_sd(g, make, cfg):
    sd = make(int(g['big_seed']), **cfg)
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v, np.float32).tobytes())
    assert h.hexdigest() == str(g['big_weights_sha256'])
    return sd


@pytest.fixture(scope='module')
def big(golden):
    """The default-width nets on the fixtures' big_x (RCAN 10 x 20, nf 64 on 16x16; MSRResNet nf 64, 16 blocks on 32x32):
    weights, input, the exact float64 restatement and the float64 model of bf16 storage, computed once."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    out = {}
    for name, fx, make, cfg, fn in (('rcan', 'g_v_rcan', synth.rcan_state_dict, RCAN_BIG, restate_rcan),
                                    ('msr', 'g_u_msrresnet', synth.msrresnet_state_dict, MSR_BIG, restate_msr)):
        g = golden(fx)
        sd = _big_sd(g, make, cfg)
        x = torch.from_numpy(g['big_x'])
        with torch.no_grad():
            sd64 = _sd_t(sd, torch.float64)
            y64 = fn(x.double(), sd64, cfg)
            ybf = fn(x.double(), sd64, cfg, r=_bf16_round, rw=_bf16_round)
        out[name] = dict(sd=sd, x=x, y64=y64, ybf=ybf, big_y=g['big_y'])
    return out


def test_the_restatements_reproduce_the_fixtures(golden, big):
    """The precondition of every bound below (the yardstick must be the network; this part needs no bf16 code).  RCAN: the
    fixture stores the reference's float32 output and that run's distance from its float64 run, so the exact restatement is
    within that distance (plus the storage rounding of a float32).  MSRResNet: the fixture stores the float64 output itself and
    the restatement is the same sequence of torch ops.  The summation order of a float64 convolution on the CPU depends on
    the BLAS code path, which moves outputs by one or two units in the last place, so the comparison allows 16 ulp of float64
    at the output's magnitude (3.6e-15; float32 rounding would be 6e-8)."""
    g = golden('g_v_rcan')
    for s in (2, 3, 4):
        cfg = _rcan_cfg(s)
        y = restate_rcan(torch.from_numpy(g[f'fwd_x{s}_x']).double(), _sd_t(synth.rcan_state_dict(200 + s, **cfg), torch.float64), cfg)
        ref = torch.from_numpy(g[f'fwd_x{s}_y']).double()
        assert float((y - ref).abs().max()) <= float(g[f'fwd_x{s}_y32_err']) + ULP * float(ref.abs().max())
    g = golden('g_u_msrresnet')
    for s in (2, 3, 4):
        cfg = _msr_cfg(s)
        y = restate_msr(torch.from_numpy(g[f'fwd_x{s}_x']).double(), _sd_t(synth.msrresnet_state_dict(100 + s, **cfg), torch.float64), cfg)
        ref = torch.from_numpy(g[f'fwd_x{s}_y64'])
        err = float((y - ref).abs().max())
        print(f'MSRResNet x{s} restatement: bit-equal {torch.equal(y, ref)}, max|d| {err:.3e}')
        assert y.dtype == ref.dtype == torch.float64 and err <= 16 * 2.0 ** -52 * float(ref.abs().max())
    # the default-width nets against the reference's float32 outputs (the bar of the fp32 tests)
    for name in ('rcan', 'msr'):
        assert float((big[name]['y64'] - torch.from_numpy(big[name]['big_y']).double()).abs().max()) < 1e-4


# ----------------------------------------------------------------------------------------------------------- the bf16 forward
def _bf16_check(y_hip, y_model, y64, what):
    y_hip, y_model, y64 = (np.asarray(t, np.float64) for t in (y_hip, y_model, y64))
    assert y_hip.shape == y64.shape, what
    err, model = float(np.abs(y_hip - y64).max()), float(np.abs(y_model - y64).max())
    floor = 4 * ULP * float(np.abs(y64).max())
    print(f'{what}: |bf16 - y64| {err:.3e}  |model - y64| {model:.3e}  ratio {err / model:.3f}  '
          f'|bf16 - model| {float(np.abs(y_hip - y_model).max()):.3e}  max|y64| {float(np.abs(y64).max()):.3f}')
    assert err <= 2 * model + floor, (what, err, model)


@pytest.mark.parametrize('s', [2, 3, 4])
def test_rcan_bf16_forward_matches_the_model_of_bf16_storage(cuda, golden, s):
    g = golden('g_v_rcan')
    cfg = _rcan_cfg(s)
    sd64 = _sd_t(synth.rcan_state_dict(200 + s, **cfg), torch.float64)
    x = torch.from_numpy(g[f'fwd_x{s}_x'])
    with torch.no_grad():
        y64 = restate_rcan(x.double(), sd64, cfg)
        y_model = restate_rcan(x.double(), sd64, cfg, r=_bf16_round, rw=_bf16_round)
    net = _rcan_small(s, cuda, compute_dtype='bf16').eval()
    with torch.no_grad():
        y = net(x.to(cuda))
    assert y.dtype == torch.float32
    _bf16_check(y.cpu().numpy(), y_model.numpy(), y64.numpy(), f'RCAN bf16 x{s}')
    # eval mode with grad enabled: still the forward-only path, no graph; reruns are bit-identical
    y2 = net(x.to(cuda))
    assert y2.grad_fn is None and not y2.requires_grad and torch.equal(y2, y)


@pytest.mark.parametrize('s', [2, 3, 4])
def test_msrresnet_bf16_forward_matches_the_model_of_bf16_storage(cuda, golden, s):
    g = golden('g_u_msrresnet')
    cfg = _msr_cfg(s)
    sd64 = _sd_t(synth.msrresnet_state_dict(100 + s, **cfg), torch.float64)
    x = torch.from_numpy(g[f'fwd_x{s}_x'])
    with torch.no_grad():
        y_model = restate_msr(x.double(), sd64, cfg, r=_bf16_round, rw=_bf16_round)
    net = _msr_small(s, cuda, compute_dtype='bf16').eval()
    with torch.no_grad():
        y = net(x.to(cuda))
    assert y.dtype == torch.float32
    _bf16_check(y.cpu().numpy(), y_model.numpy(), g[f'fwd_x{s}_y64'], f'MSRResNet bf16 x{s}')
    y2 = net(x.to(cuda))
    assert y2.grad_fn is None and not y2.requires_grad and torch.equal(y2, y)


def test_rcan_bf16_default_width_net(cuda, big):
    b = big['rcan']
    net = _load(ira.build_network(dict(type='RCAN', compute_dtype='bf16', **RCAN_BIG)), b['sd'], cuda).eval()
    with torch.no_grad():
        y = net(b['x'].to(cuda))
        assert torch.equal(net(b['x'].to(cuda)), y)
    assert y.shape == (1, 3, 64, 64)
    _bf16_check(y.cpu().numpy(), b['ybf'].numpy(), b['y64'].numpy(), 'RCAN bf16 10x20 nf64')


def test_msrresnet_bf16_default_width_net(cuda, big):
    b = big['msr']
    net = _load(ira.build_network(dict(type='MSRResNet', compute_dtype='bf16', **MSR_BIG)), b['sd'], cuda).eval()
    with torch.no_grad():
        y = net(b['x'].to(cuda))
        assert torch.equal(net(b['x'].to(cuda)), y)
    assert y.shape == (1, 3, 128, 128)
    _bf16_check(y.cpu().numpy(), b['ybf'].numpy(), b['y64'].numpy(), 'MSRResNet bf16 nf64 nb16')


def test_msrresnet_bf16_with_five_channels(cuda):
    """num_in_ch = num_out_ch = 5: the converted input fills 5 of 16 channels, conv_last stores 5 fp32 NCHW planes through the
    general NCHW store of sr_conv3x3_bf16 (more than 4 outputs: not the few-output kernel), the bilinear base has 5 planes."""
    cfg = dict(num_in_ch=5, num_out_ch=5, num_feat=16, num_block=1, upscale=2)
    sd = synth.msrresnet_state_dict(105, **cfg)
    x = torch.from_numpy(synth.uniform_input(106, (2, 5, 9, 13)))
    with torch.no_grad():
        sd64 = _sd_t(sd, torch.float64)
        y64 = restate_msr(x.double(), sd64, cfg)
        y_model = restate_msr(x.double(), sd64, cfg, r=_bf16_round, rw=_bf16_round)
    net = _load(ira.build_network(dict(type='MSRResNet', compute_dtype='bf16', **cfg)), sd, cuda).eval()
    with torch.no_grad():
        y = net(x.to(cuda))
    assert y.shape == (2, 5, 18, 26) and y.dtype == torch.float32
    _bf16_check(y.cpu().numpy(), y_model.numpy(), y64.numpy(), 'MSRResNet bf16 5 channels')


def test_rcan_x8_fixture_net_is_refused_in_bf16():
    """The fixture's x8 net is 8 features wide: below one CB16 block."""
    cfg = dict(RCAN_SMALL, upscale=8, num_feat=8)
    assert ira.build_network(dict(type='RCAN', **cfg)).compute_dtype == 'fp32'
    with pytest.raises(ValueError, match='16'):
        ira.build_network(dict(type='RCAN', compute_dtype='bf16', **cfg))


@pytest.mark.parametrize('kind', ['RCAN', 'MSRResNet'])
def test_bf16_refuses_a_forward_that_needs_a_graph(cuda, kind):
    net = (_rcan_small if kind == 'RCAN' else _msr_small)(2, cuda, compute_dtype='bf16').train()
    x = torch.rand(1, 3, 8, 8, device=cuda)
    with pytest.raises(NotImplementedError, match='fp32'):
        net(x)
    for p in net.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match='fp32'):
        net(x.clone().requires_grad_(True))
    with torch.no_grad():     # train mode under no_grad is a plain forward
        y = net(x)
    assert y.grad_fn is None and y.shape == (1, 3, 16, 16) and y.dtype == torch.float32
    with pytest.raises(ValueError):
        net(torch.rand(1, 4, 8, 8, device=cuda))


@pytest.mark.parametrize('kind', ['RCAN', 'MSRResNet'])
def test_bf16_images_follow_a_parameter_update(cuda, kind):
    """The bf16 weight images are rounded from the fp32 parameters at pack time and repacked when a parameter changes; the
    attention reads its fp32 parameters directly."""
    small = _rcan_small if kind == 'RCAN' else _msr_small
    net = small(2, cuda, compute_dtype='bf16').eval()
    x = torch.rand(1, 3, 9, 7, device=cuda)
    with torch.no_grad():
        y0 = net(x)
        net.conv_last.weight.mul_(2.0)
        y1 = net(x)
        if kind == 'RCAN':
            net.body[0].residual_group[0].ca.fc2.bias.add_(1.0)
            y2 = net(x)
            assert not torch.equal(y1, y2)
        twin = small(2, cuda, compute_dtype='bf16').eval()
        twin.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
        assert not torch.equal(y0, y1) and torch.equal(net(x), twin(x))


def test_tiled_forward_on_the_bf16_msrresnet_equals_the_whole_image(cuda):
    from image_restoration_amd.tiling import tiled_forward
    net = _msr_small(3, cuda, compute_dtype='bf16').eval()
    x = torch.rand(1, 3, 21, 26, generator=torch.Generator().manual_seed(5)).to(cuda)
    with torch.no_grad():
        whole = net(x)
        tiled = tiled_forward(net, x, tile=32, pad=4, scale=3)     # a single tile
        assert tiled.shape == (1, 3, 63, 78) and torch.equal(tiled, whole)
        assert tiled_forward(net, x, tile=12, pad=2, scale=3).shape == (1, 3, 63, 78)   # and a real split runs


def test_rcan_bf16_launch_sequence(cuda):
    """Under the launch profiler the x4 forward is: the input shift, conv_first, per group (per RCAB two convs, the squeeze's
    two launches, one excite) and the group conv, conv_after_body, two (conv, shuffle) stages, conv_last, the output shift.
    Nothing between the input shift and conv_last is an fp32 kernel."""
    lib = _lib.load()
    net = _rcan_small(4, cuda, compute_dtype='bf16').eval()
    x = torch.rand(2, 3, 9, 11, device=cuda)
    with torch.no_grad():
        net(x)   # packs the weights (not profiled below)
        _lib.check(lib.sr_profile_start(256), 'sr_profile_start')
        try:
            net(x)
        finally:
            recs = (_lib.LaunchRecord * 256)()
            cnt = C.c_int(0)
            _lib.check(lib.sr_profile_stop(recs, 256, C.byref(cnt)), 'sr_profile_stop')
    ids = [recs[i].kernel_id for i in range(cnt.value)]
    ng, nb = RCAN_SMALL['num_group'], RCAN_SMALL['num_block']
    assert len(ids) == 1 + 1 + ng * (5 * nb + 1) + 1 + 4 + 1 + 1, ids
    assert ids[0] == 99 and ids[-1] == 100 and all(k in BF16_IDS for k in ids[1:-1]), ids
    conv = BF16_IDS - {98, 102, 103, 104}
    pos = 2
    for _ in range(ng):
        for _ in range(nb):
            assert ids[pos] in conv and ids[pos + 1] in conv and ids[pos + 2:pos + 5] == [102, 103, 104], (pos, ids)
            pos += 5
        assert ids[pos] in conv
        pos += 1
    assert ids[pos] in conv and ids[pos + 1] in conv and ids[pos + 2] == 98 and ids[pos + 3] in conv and ids[pos + 4] == 98
    assert ids[pos + 5] in conv and pos + 7 == len(ids)


@pytest.mark.parametrize('kind,rel', [('RCAN', 'RCAN/test_RCAN_x4_bf16.yml'), ('MSRResNet', 'SRResNet_SRGAN/test_MSRResNet_x4_bf16.yml')])
def test_the_test_entry_point_runs_the_bf16_option_files(cuda, tmp_path, kind, rel):
    """python -m image_restoration_amd.test -opt <the new option file> with its dataset and checkpoint pointed at a temporary
    folder: images are written, PSNR is reported, and the saved PNG is the bf16 network's output."""
    from PIL import Image
    from image_restoration_amd.test import test_pipeline
    from image_restoration_amd.utils.img_util import tensor2img
    rng = np.random.default_rng(1)
    (tmp_path / 'gt').mkdir(), (tmp_path / 'lq').mkdir()
    for i in range(2):
        gt = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
        Image.fromarray(gt).save(tmp_path / 'gt' / f'p{i}.png')
        Image.fromarray(gt.reshape(12, 4, 16, 4, 3).mean((1, 3)).astype(np.uint8)).save(tmp_path / 'lq' / f'p{i}.png')
    opt = yaml.safe_load(open(os.path.join(ROOT, 'options', 'test', rel)))
    assert opt['network_g']['compute_dtype'] == 'bf16'
    cfg = {k: v for k, v in opt['network_g'].items() if k not in ('type', 'compute_dtype')}
    sd = (synth.rcan_state_dict if kind == 'RCAN' else synth.msrresnet_state_dict)(5, **cfg)
    ck = tmp_path / 'net_g.pth'
    torch.save({'params': {k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
    opt['name'] = f'{kind.lower()}_x4_bf16_tiny'
    opt['datasets'] = dict(test_1=dict(name='pairs', type='PairedImageDataset', dataroot_gt=str(tmp_path / 'gt'),
                                       dataroot_lq=str(tmp_path / 'lq'), io_backend=dict(type='disk')))
    opt['path'].update(pretrain_network_g=str(ck))
    opt['val']['suffix'] = 'x4'
    p = tmp_path / 'test.yml'
    yaml.safe_dump(opt, open(p, 'w'))
    model = test_pipeline(str(tmp_path), ['-opt', str(p)])
    assert model.net_g.compute_dtype == 'bf16'
    vis = tmp_path / 'results' / opt['name'] / 'visualization' / 'pairs'
    assert sorted(os.listdir(vis)) == ['p0_x4.png', 'p1_x4.png']
    assert set(model.metric_results) == {'psnr', 'ssim'} and np.isfinite(model.metric_results['psnr'])
    net = _load(ira.build_network(dict(opt['network_g'])), sd, cuda).eval()
    lq = torch.from_numpy(np.asarray(Image.open(tmp_path / 'lq' / 'p1.png')).transpose(2, 0, 1).astype(np.float32) / 255.)[None]
    with torch.no_grad():
        want = tensor2img([net(lq.to(cuda)).cpu()], rgb2bgr=False)
    assert np.array_equal(np.asarray(Image.open(vis / 'p1_x4.png')), want)
