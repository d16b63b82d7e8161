"""NIQE on the device (sr_niqe_luma_f32 / sr_niqe_moments_f32 + metrics/niqe.py's host fit) against the reference's run
(tests/golden/g_t_niqe.npz) and against the host form, and through validation and inference.

Bounds.  Y and MSCN are bit-exact (the float32-emulation contract, metrics/niqe.py).  The moments are float64 sums of
at most 96^2 non-negative terms (or counts, which are exact) whose order differs from the host's: relative error
<= 9216 * 2^-53 ~ 1e-12.  Features and score against the reference: the contract of tests/test_niqe_host.py.  Device
against host on the same image: Y and MSCN are bit-identical, so only the moments' 1e-12 remains; rhatnorm and the
features move by ~1e-12 relative (an alpha flip would need rhatnorm within ~1e-12 of a grid midpoint), and the score, a
smooth function of the feature mean and covariance, by a small multiple of that: asserted at 1e-8 relative.
"""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_niqe_host import FIXTURE, SCORE_RTOL, case_image, check_features  # noqa: E402

import image_restoration_amd as ira  # noqa: E402
from image_restoration_amd.metrics import calculate_niqe, niqe_device  # noqa: E402
from image_restoration_amd.metrics import niqe as N  # noqa: E402
from image_restoration_amd.utils import synth  # noqa: E402
from image_restoration_amd.utils.img_util import tensor2img  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOMENT_RTOL = 1e-12
HOST_DEVICE_RTOL = 1e-8


@pytest.fixture(scope='module')
def g():
    return dict(np.load(FIXTURE))


def to_device(img_bgr_u8, dev):
    """uint8 BGR HWC -> [1, 3, H, W] RGB float in [0, 1] whose tensor2img quantisation gives the image back."""
    return torch.from_numpy(np.ascontiguousarray(img_bgr_u8[:, :, ::-1].transpose(2, 0, 1)).astype(np.float32) / 255.)[None].to(dev)


def seeded(seed, h, w):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.random((1, 3, h, w), dtype=np.float32))
    x = torch.nn.functional.avg_pool2d(x, 5, 1, 2, count_include_pad=False)  # some spatial structure
    return (0.8 * x + 0.2 * torch.from_numpy(rng.random((1, 3, h, w), dtype=np.float32))).clamp(0, 1)


@pytest.mark.parametrize('name', ['small0', 'small4', 'tall4', 'flat'])
def test_device_luma_and_mscn_are_bit_exact(cuda, g, name):
    x = to_device(g[f'{name}/img'], cuda)
    y, mom, (m1, m2) = N._device_stages(x, int(g[f'{name}/crop']), g['gaussian_window'], want_mscn=True)
    np.testing.assert_array_equal(y[0].cpu().numpy(), g[f'{name}/y'])
    np.testing.assert_array_equal(m1[0].cpu().numpy(), g[f'{name}/mscn1'])
    np.testing.assert_array_equal(m2[0].cpu().numpy(), g[f'{name}/mscn2'])
    # moments against a float64 recomputation from the reference's MSCN
    mom = mom[:, 0].cpu().numpy()
    for s, (key, block) in enumerate((('mscn1', 96), ('mscn2', 48))):
        want = N._moments(N._fields(g[f'{name}/{key}'], block))
        np.testing.assert_array_equal(mom[s][..., [0, 2]], want[..., [0, 2]])  # counts are exact
        np.testing.assert_allclose(mom[s], want, rtol=MOMENT_RTOL, atol=0)


@pytest.mark.parametrize('name', ['small0', 'small4', 'tall4', 'large'])
def test_device_features_and_score_match_reference(cuda, g, name):
    x = to_device(case_image(g, name), cuda)
    crop = int(g[f'{name}/crop'])
    _, mom, _ = N._device_stages(x, crop, g['gaussian_window'])
    mom = mom[:, 0].cpu().numpy()
    f1, r1 = N._features(mom[0], 96)
    f2, r2 = N._features(mom[1], 48)
    rh_ref = np.concatenate([g[f'{name}/rhatnorm1'], g[f'{name}/rhatnorm2']], axis=1).astype(np.float64)
    check_features(np.concatenate([f1, f2], axis=1), g[f'{name}/feat'], np.concatenate([r1, r2], axis=1), rh_ref)
    score = niqe_device(x, crop, pris_params=FIXTURE)[0]
    ref = float(g[f'{name}/score'])
    assert abs(score - ref) <= SCORE_RTOL * ref, (score, ref)


def test_device_flat_patch_is_refused(cuda, g):
    x = to_device(g['flat/img'], cuda)
    with pytest.raises(ValueError, match='at least 2 blocks'):
        niqe_device(x, 0, pris_params=FIXTURE)


@pytest.mark.parametrize('hw', [(1356, 2040), (512, 512)])
def test_device_equals_host_on_large_images(cuda, hw):
    x = seeded(hw[0] + hw[1], *hw)
    dev = niqe_device(x.to(cuda), 4, pris_params=FIXTURE)[0]
    host = calculate_niqe(tensor2img([x]), 4, pris_params=FIXTURE)
    # Y and MSCN of the device are the host's bit for bit (the host's are the reference's: tests/test_niqe_host.py)
    window = N.load_niqe_params(FIXTURE)['gaussian_window']
    y_dev, _, (m1_dev, m2_dev) = N._device_stages(x.to(cuda), 4, window, want_mscn=True)
    y_host = N._luma(tensor2img([x]), 4, 'HWC')
    m1_host, m2_host, _, _ = N._host_stages(y_host, window)
    np.testing.assert_array_equal(y_dev[0].cpu().numpy(), y_host)
    np.testing.assert_array_equal(m1_dev[0].cpu().numpy(), m1_host)
    np.testing.assert_array_equal(m2_dev[0].cpu().numpy(), m2_host)
    assert np.isfinite(dev) and abs(dev - host) <= HOST_DEVICE_RTOL * abs(host), (dev, host)


def test_batch_strides_dtypes_and_odd_sizes(cuda):
    xs = [seeded(10 + i, 201, 307) for i in range(3)]
    batch = torch.cat(xs).to(cuda)
    one = [niqe_device(x.to(cuda), 3, pris_params=FIXTURE)[0] for x in xs]
    assert niqe_device(batch, 3, pris_params=FIXTURE) == one  # bit for bit
    _, mb, _ = N._device_stages(batch, 3, N.load_niqe_params(FIXTURE)['gaussian_window'])
    _, m1, _ = N._device_stages(batch[1:2], 3, N.load_niqe_params(FIXTURE)['gaussian_window'])
    assert torch.equal(mb[:, 1:2], m1)
    # odd size with a border crop: the host form on the tensor2img image
    for i, x in enumerate(xs):
        host = calculate_niqe(tensor2img([x]), 3, pris_params=FIXTURE)
        assert abs(one[i] - host) <= HOST_DEVICE_RTOL * abs(host), (i, one[i], host)
    # non-contiguous views and bf16 inputs
    nhwc = batch.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not nhwc.is_contiguous() and niqe_device(nhwc, 3, pris_params=FIXTURE) == one
    wide = torch.zeros(3, 3, 201, 400, device=cuda)
    wide[..., 50:357] = batch
    assert niqe_device(wide[..., 50:357], 3, pris_params=FIXTURE) == one
    b16 = batch.bfloat16()
    assert niqe_device(b16, 3, pris_params=FIXTURE) == niqe_device(b16.float(), 3, pris_params=FIXTURE)
    # one channel: grey, used as is
    grey = batch[:1, 1:2]
    host = calculate_niqe(tensor2img([grey.cpu()]), 3, input_order='HW', pris_params=FIXTURE)
    dev = niqe_device(grey, 3, pris_params=FIXTURE)[0]
    assert abs(dev - host) <= HOST_DEVICE_RTOL * abs(host), (dev, host)
    with pytest.raises(ValueError, match='at least one 96x96 block'):
        niqe_device(batch[..., :101], 3, pris_params=FIXTURE)
    with pytest.raises(ValueError, match='1 or 3 channels'):
        niqe_device(torch.zeros(1, 2, 128, 128, device=cuda), 0, pris_params=FIXTURE)


def _tiny_setup(tmp_path):
    from PIL import Image
    (tmp_path / 'gt').mkdir(), (tmp_path / 'lq').mkdir()
    for i in range(2):
        gt = (np.asarray(seeded(100 + i, 224, 320)[0].permute(1, 2, 0)) * 255).round().astype(np.uint8)
        Image.fromarray(gt).save(tmp_path / 'gt' / f'p{i}.png')
        Image.fromarray(gt.reshape(56, 4, 80, 4, 3).mean((1, 3)).astype(np.uint8)).save(tmp_path / 'lq' / f'p{i}.png')
    cfg = dict(num_in_ch=3, num_out_ch=3, scale=4, num_feat=32, num_block=1, num_grow_ch=32)
    sd = synth.rrdbnet_state_dict(5, **cfg)
    ck = tmp_path / 'net_g.pth'
    torch.save({'params': {k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
    return cfg, sd, ck


def _run_test_pipeline(tmp_path, ck, datasets, metrics, name):
    from image_restoration_amd.test import test_pipeline
    opt = yaml.safe_load(open(os.path.join(ROOT, 'options', 'test', 'ESRGAN', 'test_ESRGAN_x4_woGT_niqe.yml')))
    opt['name'] = name
    opt['datasets'] = datasets
    opt['network_g'].update(num_feat=32, num_block=1, num_grow_ch=32)
    opt['path'].update(pretrain_network_g=str(ck))
    opt['val'].update(save_img=False, metrics=metrics)
    p = tmp_path / f'{name}.yml'
    yaml.safe_dump(opt, open(p, 'w'))
    return test_pipeline(str(tmp_path), ['-opt', str(p)])


def test_validation_scores_niqe_without_gt_and_keeps_psnr(cuda, tmp_path):
    """SRModel.nondist_validation: NIQE from the device output on an LQ-only folder equals niqe_device of the network's output;
    on a paired set, PSNR next to NIQE is the value the PSNR-only configuration gives."""
    from PIL import Image
    cfg, sd, ck = _tiny_setup(tmp_path)
    niqe_opt = dict(type='calculate_niqe', crop_border=4, pris_params=FIXTURE)
    lq_only = dict(test_1=dict(name='lq_only', type='SingleImageDataset', dataroot_lq=str(tmp_path / 'lq'), io_backend=dict(type='disk')))
    model = _run_test_pipeline(tmp_path, ck, lq_only, dict(niqe=niqe_opt), 'woGT')
    net = ira.build_network(dict(type='RRDBNet', **cfg)).to(cuda).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    want = []
    for i in range(2):
        lq = torch.from_numpy(np.asarray(Image.open(tmp_path / 'lq' / f'p{i}.png')).transpose(2, 0, 1).astype(np.float32) / 255.)[None]
        with torch.no_grad():
            want.append(niqe_device(net(lq.to(cuda)), 4, pris_params=FIXTURE)[0])
    assert set(model.metric_results) == {'niqe'}
    assert abs(model.metric_results['niqe'] - np.mean(want)) <= 1e-12 * abs(np.mean(want)), (model.metric_results, want)
    pairs = dict(test_1=dict(name='pairs', type='PairedImageDataset', dataroot_gt=str(tmp_path / 'gt'), dataroot_lq=str(tmp_path / 'lq'),
                             io_backend=dict(type='disk')))
    psnr_opt = dict(type='calculate_psnr', crop_border=4, test_y_channel=False)
    only = _run_test_pipeline(tmp_path, ck, pairs, dict(psnr=psnr_opt), 'psnr_only').metric_results
    both = _run_test_pipeline(tmp_path, ck, pairs, dict(psnr=psnr_opt, niqe=niqe_opt), 'psnr_niqe').metric_results
    assert set(both) == {'psnr', 'niqe'} and both['psnr'] == only['psnr']
    assert abs(both['niqe'] - model.metric_results['niqe']) <= 1e-12 * abs(model.metric_results['niqe'])


def test_inference_prints_niqe_of_the_device_output(cuda, tmp_path, capsys):
    from PIL import Image
    from image_restoration_amd import inference
    cfg, sd, ck = _tiny_setup(tmp_path)
    src = tmp_path / 'lq' / 'p0.png'
    net = ira.build_network(dict(type='RRDBNet', **cfg)).to(cuda).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    img = inference.imread_bgr(str(src))
    common = ['--input', str(src), '--model_path', str(ck), '--num_feat', '32', '--num_block', '1', '--niqe_params', FIXTURE]
    for tile in (0, 32):
        y = inference.restore_tensor(net, img, tile, 8)
        want = niqe_device(y, 0, pris_params=FIXTURE)[0]
        capsys.readouterr()
        inference.main(common + ['--output', str(tmp_path / f'out{tile}.png'), '--tile', str(tile), '--tile_pad', '8'])
        lines = [ln for ln in capsys.readouterr().out.splitlines() if 'NIQE' in ln]
        assert len(lines) == 1 and lines[0].endswith(f'NIQE {want:.4f}'), (lines, want)
        assert np.array_equal(np.asarray(Image.open(tmp_path / f'out{tile}.png'))[:, :, ::-1],
                              tensor2img(y, rgb2bgr=True, min_max=(0, 1)))
