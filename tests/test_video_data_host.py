"""REDSDataset, VideoTestDataset, SyntheticClipDataset and the host half of DeviceClipPipeline (no GPU).

The reference's REDSDataset cannot be imported here (its package needs cv2, which is not installed), so what a seeded run can
observe of it is restated below from basicsr/data/reds_dataset.py:99-187 and transforms.py:26-158: the calls on Python's ``random``
in their order.  The frames written for the test carry their clip position and pixel coordinates in their channels, so an item
shows which frames, which window and which symmetry it was made from."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

from image_restoration_amd.data import DeviceClipPipeline, REDSDataset, SyntheticClipDataset, VideoTestDataset
from image_restoration_amd.utils.registry import DATASET_REGISTRY

FRAMES, LQ_H, LQ_W, SCALE, GT_SIZE = 7, 12, 16, 4, 16
PATCH = GT_SIZE // SCALE


def _frame(f, h, w, ystep, xstep):
    """RGB uint8: R = 30 * frame, G = ystep * row, B = xstep * column."""
    a = np.zeros((h, w, 3), np.uint8)
    a[..., 0] = 30 * f
    a[..., 1] = (np.arange(h) * ystep)[:, None]
    a[..., 2] = (np.arange(w) * xstep)[None, :]
    return a


def _lq(f):
    return _frame(f, LQ_H, LQ_W, 10, 10)


def _gt(f):
    return _frame(f, LQ_H * SCALE, LQ_W * SCALE, 5, 3)


@pytest.fixture(scope='module')
def clips(tmp_path_factory):
    root = tmp_path_factory.mktemp('reds')
    for clip in ('001', '002'):
        for kind, make in (('lq', _lq), ('gt', _gt)):
            d = root / kind / clip
            d.mkdir(parents=True)
            for f in range(FRAMES):
                Image.fromarray(make(f)).save(d / f'{f:08d}.png')
    meta = root / 'meta.txt'
    meta.write_text(''.join(f'{c} {FRAMES} ({LQ_H * SCALE},{LQ_W * SCALE},3)\n' for c in ('001', '002')))
    return root, meta


def _opt(clips, **kw):
    root, meta = clips
    opt = dict(name='REDS', type='REDSDataset', dataroot_gt=str(root / 'gt'), dataroot_lq=str(root / 'lq'), dataroot_flow=None,
               meta_info_file=str(meta), val_partition='REDS4', io_backend=dict(type='disk'), num_frame=3, gt_size=GT_SIZE,
               interval_list=[1], random_reverse=False, use_flip=True, use_rot=True, scale=SCALE, phase='train')
    opt.update(kw)
    return opt


def _reference_draws(centre, num_frame, interval_list, random_reverse, use_flip, use_rot):
    """The reference's calls on ``random`` for one item, in its order."""
    half, last = num_frame // 2, FRAMES - 1
    interval = random.choice(interval_list)
    start, end = centre - half * interval, centre + half * interval
    redrawn = 0
    while start < 0 or end > last:
        centre = random.randint(0, last)
        start, end = centre - half * interval, centre + half * interval
        redrawn += 1
    neighbours = list(range(start, end + 1, interval))
    if random_reverse and random.random() < 0.5:
        neighbours.reverse()
    top = random.randint(0, LQ_H - PATCH)        # paired_random_crop
    left = random.randint(0, LQ_W - PATCH)
    hflip = use_flip and random.random() < 0.5   # augment
    vflip = use_rot and random.random() < 0.5
    rot90 = use_rot and random.random() < 0.5
    return centre, neighbours, (top, left), (hflip, vflip, rot90), redrawn, interval


def _sym(a, hflip, vflip, rot90):
    if hflip:
        a = a[:, ::-1]
    if vflip:
        a = a[::-1]
    if rot90:
        a = a.transpose(1, 0, 2)
    return a


def _chw(a):
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.float32) / 255.).transpose(2, 0, 1).copy())


@pytest.mark.parametrize('kw', [dict(), dict(interval_list=[1, 2], random_reverse=True), dict(num_frame=5, interval_list=[1]),
                                dict(use_flip=False), dict(use_rot=False, random_reverse=True)])
def test_reds_items_follow_the_reference_draw_order(clips, kw):
    ds = REDSDataset(_opt(clips, **kw))
    o = ds.opt
    assert len(ds) == 2 * FRAMES and ds.keys[0] == '001/00000000' and ds.keys[-1] == f'002/{FRAMES - 1:08d}'
    redraws, intervals, reversals, ends = 0, set(), 0, set()
    for seed in range(6):
        for index in (0, 1, 3, FRAMES - 2, FRAMES - 1, FRAMES + 2):
            random.seed(seed * 100 + index)
            centre, nbrs, (top, left), sym, redrawn, interval = _reference_draws(index % FRAMES, o['num_frame'], o['interval_list'],
                                                                                 o['random_reverse'], o['use_flip'], o['use_rot'])
            after = random.random()
            random.seed(seed * 100 + index)
            item = ds[index]
            assert random.random() == after                                   # the same number of draws was taken
            assert set(item) == {'lq', 'gt', 'key'} and item['key'] == ds.keys[index]
            lq, gt = item['lq'], item['gt']
            assert lq.dtype == torch.float32 and gt.dtype == torch.float32
            assert tuple(lq.shape) == (o['num_frame'], 3, PATCH, PATCH) and tuple(gt.shape) == (3, GT_SIZE, GT_SIZE)
            assert [int(round(float(f[0, 0, 0]) * 255 / 30)) for f in lq] == nbrs   # channel 0 (R after BGR -> RGB) names the frame
            want_lq = torch.stack([_chw(_sym(_lq(n)[top:top + PATCH, left:left + PATCH], *sym)) for n in nbrs])
            want_gt = _chw(_sym(_gt(centre)[top * SCALE:top * SCALE + GT_SIZE, left * SCALE:left * SCALE + GT_SIZE], *sym))
            assert torch.equal(lq, want_lq) and torch.equal(gt, want_gt)
            redraws += redrawn
            intervals.add(interval)
            reversals += nbrs[0] > nbrs[-1]
            if redrawn:
                ends.add(index % FRAMES)
    assert redraws > 0 and {0, FRAMES - 1} <= ends                           # the centre was re-drawn near both ends of a clip
    assert intervals == set(o['interval_list'])
    assert (reversals > 0) == bool(o['random_reverse'])


def test_reds_device_items_carry_the_same_draws(clips):
    host = REDSDataset(_opt(clips, interval_list=[1, 2], random_reverse=True))
    for mode in (True, 'full'):
        dev = REDSDataset(_opt(clips, interval_list=[1, 2], random_reverse=True, device_augment=mode))
        for index in (0, 4, FRAMES + 6):
            random.seed(index)
            centre, nbrs, (top, left), (h, v, r), _, _ = _reference_draws(index % FRAMES, 3, [1, 2], True, True, True)
            after = random.random()
            random.seed(index)
            item = dev[index]
            assert random.random() == after
            assert int(item['sym']) == int(h) | int(v) << 1 | int(r) << 2 and item['sym'].dtype == np.int32
            assert item['lq_u8'].dtype == np.uint8 and item['gt_u8'].dtype == np.uint8 and item['key'] == host.keys[index]
            bgr_lq = np.stack([_lq(n)[..., ::-1] for n in nbrs])                    # decode order
            bgr_gt = _gt(centre)[..., ::-1]
            if mode == 'full':
                assert item['window'].tolist() == [top, left] and item['window'].dtype == np.int32
                assert np.array_equal(item['lq_u8'], bgr_lq) and np.array_equal(item['gt_u8'], bgr_gt)
            else:
                assert 'window' not in item
                assert np.array_equal(item['lq_u8'], bgr_lq[:, top:top + PATCH, left:left + PATCH])
                assert np.array_equal(item['gt_u8'], bgr_gt[top * SCALE:top * SCALE + GT_SIZE, left * SCALE:left * SCALE + GT_SIZE])
            assert item['lq_u8'].flags['C_CONTIGUOUS'] and item['gt_u8'].flags['C_CONTIGUOUS']


def test_reds_validation_partition_and_refusals(clips, tmp_path):
    meta = tmp_path / 'meta.txt'
    meta.write_text(''.join(f'{c} 3 (8,8,3)\n' for c in ('000', '001', '011', '015', '020', '239', '240', '269')))
    reds4 = REDSDataset(_opt(clips, meta_info_file=str(meta), val_partition='REDS4'))
    assert sorted({k.split('/')[0] for k in reds4.keys}) == ['001', '239', '240', '269'] and len(reds4) == 12
    official = REDSDataset(_opt(clips, meta_info_file=str(meta), val_partition='official'))
    assert sorted({k.split('/')[0] for k in official.keys}) == ['000', '001', '011', '015', '020', '239']
    assert official.last_frame == {c: 2 for c in ('000', '001', '011', '015', '020', '239')}
    with pytest.raises(ValueError, match='Wrong validation partition'):
        REDSDataset(_opt(clips, val_partition='REDS5'))
    with pytest.raises(NotImplementedError, match='supported: dataroot_flow: null .* io_backend.type: disk'):
        REDSDataset(_opt(clips, dataroot_flow='datasets/REDS/flow'))
    with pytest.raises(NotImplementedError, match='supported: dataroot_flow: null .* io_backend.type: disk'):
        REDSDataset(_opt(clips, io_backend=dict(type='lmdb')))
    with pytest.raises(AssertionError, match='odd'):
        REDSDataset(_opt(clips, num_frame=4))
    with pytest.raises(ValueError, match='smaller than patch size'):
        REDSDataset(_opt(clips, gt_size=64))[0]
    assert DATASET_REGISTRY.get('REDSDataset') is REDSDataset and DATASET_REGISTRY.get('VideoTestDataset') is VideoTestDataset


# ------------------------------------------------------------------------------------------------------ VideoTestDataset
def _vopt(clips, **kw):
    root, _ = clips
    opt = dict(name='REDS4', type='VideoTestDataset', dataroot_gt=str(root / 'gt'), dataroot_lq=str(root / 'lq'),
               io_backend=dict(type='disk'), cache_data=False, num_frame=5, padding='reflection_circle', scale=SCALE, phase='val')
    opt.update(kw)
    return opt


ENDS = {   # 7 frames, windows of 5: the first two and the last two centres
    'replicate': {0: [0, 0, 0, 1, 2], 1: [0, 0, 1, 2, 3], 5: [3, 4, 5, 6, 6], 6: [4, 5, 6, 6, 6]},
    'reflection': {0: [2, 1, 0, 1, 2], 1: [1, 0, 1, 2, 3], 5: [3, 4, 5, 6, 5], 6: [4, 5, 6, 5, 4]},
    'reflection_circle': {0: [4, 3, 0, 1, 2], 1: [4, 0, 1, 2, 3], 5: [3, 4, 5, 6, 2], 6: [4, 5, 6, 3, 2]},
    'circle': {0: [3, 4, 0, 1, 2], 1: [4, 0, 1, 2, 3], 5: [3, 4, 5, 6, 2], 6: [4, 5, 6, 2, 3]},
}


@pytest.mark.parametrize('padding', sorted(ENDS))
@pytest.mark.parametrize('cache', [False, True])
def test_video_test_items(clips, padding, cache):
    ds = VideoTestDataset(_vopt(clips, padding=padding, cache_data=cache))
    assert len(ds) == 2 * FRAMES
    assert ds.data_info['folder'] == ['001'] * FRAMES + ['002'] * FRAMES
    assert ds.data_info['border'] == [1, 1, 0, 0, 0, 1, 1] * 2
    for base, folder in ((0, '001'), (FRAMES, '002')):
        for i in range(FRAMES):
            item = ds[base + i]
            assert set(item) == {'lq', 'gt', 'folder', 'idx', 'border', 'lq_path'}
            assert item['folder'] == folder and item['idx'] == f'{i}/{FRAMES}' and item['border'] == int(i < 2 or i > 4)
            assert item['lq_path'].endswith(f'lq/{folder}/{i:08d}.png')
            assert tuple(item['lq'].shape) == (5, 3, LQ_H, LQ_W) and tuple(item['gt'].shape) == (3, LQ_H * SCALE, LQ_W * SCALE)
            got = [int(round(float(f[0, 0, 0]) * 255 / 30)) for f in item['lq']]
            assert got == ENDS[padding].get(i, list(range(i - 2, i + 3))), (padding, i)
            assert torch.equal(item['gt'], _chw(_gt(i))) and torch.equal(item['lq'][2], _chw(_lq(i)))


def test_meta_info_route_and_folder_scan_agree(clips, tmp_path):
    scan = VideoTestDataset(_vopt(clips, num_frame=3))
    meta = tmp_path / 'test_meta.txt'
    meta.write_text('001 7 (48,64,3)\n002 7 (48,64,3)\n')
    listed = VideoTestDataset(_vopt(clips, num_frame=3, meta_info_file=str(meta)))
    assert scan.data_info == listed.data_info
    for i in (0, 6, 9):
        a, b = scan[i], listed[i]
        assert torch.equal(a['lq'], b['lq']) and torch.equal(a['gt'], b['gt']) and {k: a[k] for k in ('folder', 'idx', 'border', 'lq_path')} \
            == {k: b[k] for k in ('folder', 'idx', 'border', 'lq_path')}
    meta.write_text('002 7 (48,64,3)\n')
    assert set(VideoTestDataset(_vopt(clips, meta_info_file=str(meta))).data_info['folder']) == {'002'}
    with pytest.raises(AssertionError, match='lmdb'):
        VideoTestDataset(_vopt(clips, io_backend=dict(type='lmdb')))
    with pytest.raises(ValueError, match='unknown padding'):
        VideoTestDataset(_vopt(clips, padding='mirror'))[0]


# ------------------------------------------------------------------------------------------- the clip pipeline's host half
def test_clip_pipeline_replicates_origin_and_symmetry_per_frame():
    pipe = DeviceClipPipeline(dict(scale=4, gt_size=16))
    sym = torch.tensor([5, 0, 3], dtype=torch.int64)
    origin = torch.tensor([[1, 2], [8, 12], [0, 0]], dtype=torch.int64)
    sym_t, origin_t = pipe.per_frame(sym, origin, 3)
    assert sym_t.dtype == torch.int32 and sym_t.tolist() == [5, 5, 5, 0, 0, 0, 3, 3, 3] and sym_t.is_contiguous()
    assert origin_t.dtype == torch.int32 and origin_t.tolist() == [[1, 2]] * 3 + [[8, 12]] * 3 + [[0, 0]] * 3 and origin_t.is_contiguous()
    assert pipe.per_frame(sym, None, 2)[1] is None and pipe.per_frame(sym, None, 1)[0].tolist() == [5, 0, 3]
    assert pipe.output_shapes(3, 5) == ((3, 5, 3, 4, 4), (3, 3, 16, 16))
    passthrough = dict(lq=torch.zeros(1), gt=torch.zeros(1))
    assert pipe(passthrough) is passthrough                                  # a host-augmented batch passes through
    with pytest.raises(ValueError, match=r'\[B, t, H, W, 3\]'):
        pipe(dict(lq_u8=torch.zeros((2, 4, 4, 3), dtype=torch.uint8), gt_u8=torch.zeros((2, 16, 16, 3), dtype=torch.uint8), sym=sym[:2]))
    from image_restoration_amd import _lib
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        pipe(dict(lq_u8=torch.zeros((2, 3, 4, 4, 3), dtype=torch.uint8), gt_u8=torch.zeros((2, 16, 16, 3), dtype=torch.uint8), sym=sym[:2]))
    from image_restoration_amd.data import DevicePatchPipeline
    from image_restoration_amd.train import device_pipeline_class
    assert device_pipeline_class(dict(type='REDSDataset')) is DeviceClipPipeline
    assert device_pipeline_class(dict(type='PairedImageDataset')) is DevicePatchPipeline


def test_synthetic_clips_are_translated_textures_with_box_average_lq():
    ds = SyntheticClipDataset(dict(num_samples=5, gt_size=32, scale=4, num_frame=3, max_motion=2, seed=3))
    assert len(ds) == 5
    moved = 0
    for i in range(5):
        a, b = ds[i], ds[i]
        assert torch.equal(a['lq'], b['lq']) and torch.equal(a['gt'], b['gt']) and a['key'] == f'synthetic/{i:08d}'
        lq, gt = a['lq'], a['gt']
        assert tuple(lq.shape) == (3, 3, 8, 8) and tuple(gt.shape) == (3, 32, 32) and lq.dtype == gt.dtype == torch.float32
        assert float(gt.min()) >= 0 and float(gt.max()) < 1
        box = gt.view(3, 8, 4, 8, 4).mean(dim=(2, 4))
        assert torch.allclose(lq[1], box, atol=1e-6)                         # the centre LQ frame is the x4 box average of the GT
        # the motion is a whole number of LQ pixels: some shift (dy, dx) maps frame 0 onto frame 1 and the same shift frame 1 onto 2
        hit = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3)
               if all(torch.equal(lq[k][:, max(0, dy):8 + min(0, dy), max(0, dx):8 + min(0, dx)],
                                  lq[k + 1][:, max(0, -dy):8 + min(0, -dy), max(0, -dx):8 + min(0, -dx)]) for k in (0, 1))]
        assert len(hit) == 1, (i, hit)
        moved += hit[0] != (0, 0)
    assert moved >= 3
    assert DATASET_REGISTRY.get('SyntheticClipDataset') is SyntheticClipDataset
    with pytest.raises(ValueError, match='odd'):
        SyntheticClipDataset(dict(num_frame=4))
