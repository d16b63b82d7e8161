"""The option-file route of the recurrent video networks on the GPU: VideoRecurrentTestDataset + VideoRecurrentModel on two tiny
synthetic folders (5 frames of 36x40): ``flip_seq`` averaging and ``center_frame_only`` slicing against the network called
directly, the saved image names, PSNR per folder, and the shipped option file through the test entry point."""
import os

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = dict(type='BasicVSR', num_feat=16, num_block=1)
FOLDERS, FRAMES, H, W = ('000', '011'), 5, 36, 40


def _video_set(root):
    rng = np.random.default_rng(7)
    for folder in FOLDERS:
        for kind, s in (('gt', 4), ('lq', 1)):
            d = os.path.join(root, kind, folder)
            os.makedirs(d)
            for f in range(FRAMES):
                Image.fromarray(rng.integers(0, 256, (H * s, W * s, 3), dtype=np.uint8)).save(os.path.join(d, f'{f:08d}.png'))
    return dict(name='REDS4', type='VideoRecurrentTestDataset', dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'),
                io_backend=dict(type='disk'), cache_data=True, num_frame=1, padding='reflection_circle', scale=4, phase='val')


def _opt(tmp_path, **val):
    return dict(name='vsr_test', model_type='VideoRecurrentModel', scale=4, num_gpu=1, is_train=False, dist=False, rank=0, world_size=1,
                network_g=dict(NET), path=dict(pretrain_network_g=None, strict_load_g=True, visualization=str(tmp_path / 'vis')),
                val=dict(val))


def test_model_test_flip_seq_and_center_frame_against_the_network(cuda, tmp_path):
    from torch.utils.data import DataLoader
    from image_restoration_amd.data import VideoRecurrentTestDataset
    from image_restoration_amd.metrics import calculate_psnr
    from image_restoration_amd.models import build_model
    from image_restoration_amd.utils.img_util import tensor2img
    ds = VideoRecurrentTestDataset(_video_set(str(tmp_path / 'data')))
    assert len(ds) == 2 and [ds[i]['folder'] for i in range(2)] == list(FOLDERS)
    item = ds[1]
    assert tuple(item['lq'].shape) == (FRAMES, 3, H, W) and tuple(item['gt'].shape) == (FRAMES, 3, 4 * H, 4 * W)
    torch.manual_seed(3)
    model = build_model(_opt(tmp_path))
    assert type(model).__name__ == 'VideoRecurrentModel'
    net = model.net_g
    lq = item['lq'].unsqueeze(0).to(cuda)
    net.eval()
    plain = net(lq)
    both = net(torch.cat([lq, lq.flip(1)], 1))
    flipped = 0.5 * (both[:, :FRAMES] + both[:, FRAMES:].flip(1))
    net.train()
    for val, want in ((dict(), plain), (dict(flip_seq=True), flipped), (dict(center_frame_only=True), plain[:, FRAMES // 2]),
                      (dict(flip_seq=True, center_frame_only=True), flipped[:, FRAMES // 2])):
        model.opt['val'] = val
        model.feed_data(dict(lq=item['lq'].unsqueeze(0), gt=item['gt'].unsqueeze(0)))
        model.test()
        assert torch.equal(model.output, want) and model.output.grad_fn is None, val
        assert net.training                                   # test() hands the network back in train mode, as the reference
    assert not torch.equal(flipped, plain)
    # validation: per folder, per frame, images under the expected names
    model.opt['val'] = dict(metrics=dict(psnr=dict(type='calculate_psnr', crop_border=0, test_y_channel=False)))
    model.validation(DataLoader(ds, batch_size=1, shuffle=False, num_workers=0), 0, None, True)
    assert list(model.metric_results) == list(FOLDERS)
    vis = tmp_path / 'vis' / 'REDS4'
    for k, folder in enumerate(FOLDERS):
        t = model.metric_results[folder]
        assert tuple(t.shape) == (FRAMES, 1) and bool(torch.isfinite(t).all())
        assert sorted(os.listdir(vis / folder)) == [f'{f:08d}_vsr_test.png' for f in range(FRAMES)]
        out = net.eval()(ds[k]['lq'].unsqueeze(0).to(cuda))
        net.train()
        for f in (0, FRAMES - 1):
            host = calculate_psnr(tensor2img([out[:, f].cpu()]), tensor2img([ds[k]['gt'][f].unsqueeze(0)]), 0)
            assert abs(float(t[f, 0]) - host) <= 1e-3, (folder, f)
            saved = np.asarray(Image.open(vis / folder / f'{f:08d}_vsr_test.png'))
            assert saved.shape == (4 * H, 4 * W, 3) and np.array_equal(saved, tensor2img([out[:, f].cpu()], rgb2bgr=False))
    summary = model.validation_summary
    means = [float(model.metric_results[f][:, 0].double().mean()) for f in FOLDERS]
    assert [summary['folders'][f]['psnr'] for f in FOLDERS] == pytest.approx(means, abs=1e-5)
    assert summary['total']['psnr'] == pytest.approx(sum(means) / 2, abs=1e-5)
    # center_frame_only: one row per folder, one image named after the folder
    model.opt['val'] = dict(center_frame_only=True, suffix='mid', metrics=dict(psnr=dict(type='calculate_psnr', crop_border=0)))
    model.validation(DataLoader(ds, batch_size=1), 0, None, True)
    assert all(tuple(t.shape) == (1, 1) for t in model.metric_results.values())
    assert 'FOLDER_mid.png'.replace('FOLDER', '011') in os.listdir(vis / '011')


def test_shipped_option_file_through_the_test_entry_point(cuda, tmp_path):
    from image_restoration_amd.archs import build_network
    from image_restoration_amd.test import test_pipeline
    opt = yaml.safe_load(open(os.path.join(ROOT, 'options', 'test', 'BasicVSR', 'test_BasicVSR_REDS.yml')))
    assert opt['model_type'] == 'VideoRecurrentModel' and opt['datasets']['test']['type'] == 'VideoRecurrentTestDataset'
    assert opt['datasets']['test']['cache_data'] and opt['network_g'] == dict(type='BasicVSR', num_feat=64, num_block=30, spynet_path=None)
    dopt = _video_set(str(tmp_path / 'data'))
    torch.manual_seed(4)
    ckpt = str(tmp_path / 'net.pth')
    torch.save({'params': build_network(dict(NET)).state_dict()}, ckpt)
    opt['name'] = 'vsr_cli'
    opt['datasets']['test'].update(dataroot_gt=dopt['dataroot_gt'], dataroot_lq=dopt['dataroot_lq'])
    del opt['datasets']['test']['meta_info_file']
    opt['network_g'] = dict(NET)
    opt['path']['pretrain_network_g'] = ckpt
    p = tmp_path / 'opt.yml'
    yaml.safe_dump(opt, open(p, 'w'))
    model = test_pipeline(str(tmp_path), ['-opt', str(p)])
    assert type(model).__name__ == 'VideoRecurrentModel' and list(model.metric_results) == list(FOLDERS)
    vis = tmp_path / 'results' / 'vsr_cli' / 'visualization' / 'REDS4'
    for folder in FOLDERS:
        assert sorted(os.listdir(vis / folder)) == [f'{f:08d}_vsr_cli.png' for f in range(FRAMES)]
    assert set(model.validation_summary['total']) == {'psnr'} and np.isfinite(model.validation_summary['total']['psnr'])


def test_iconvsr_through_the_recurrent_model(cuda, tmp_path):
    """The same model and dataset drive IconVSR: 5 frames are the smallest clip temporal_padding 2 takes; 36x40 needs no padding."""
    from image_restoration_amd.data import VideoRecurrentTestDataset
    from image_restoration_amd.models import build_model
    ds = VideoRecurrentTestDataset(_video_set(str(tmp_path / 'data')))
    opt = _opt(tmp_path)
    opt['network_g'] = dict(type='IconVSR', num_block=1, keyframe_stride=2)
    torch.manual_seed(5)
    model = build_model(opt)
    item = ds[0]
    model.feed_data(dict(lq=item['lq'].unsqueeze(0), gt=item['gt'].unsqueeze(0)))
    model.test()
    want = model.net_g.eval()(item['lq'].unsqueeze(0).to(cuda))
    model.net_g.train()
    assert tuple(model.output.shape) == (1, FRAMES, 3, 4 * H, 4 * W) and torch.equal(model.output, want)
