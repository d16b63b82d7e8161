"""DeviceClipPipeline against the host route of REDSDataset: same random draws, bit-identical tensors (the clip case of
tests/test_data_gpu.py::test_device_pipeline_is_bit_identical_to_the_host_pipeline).  Clips of 3 frames, batches of 3, random
uint8 frames (every byte value), host-cut windows and device-side cropping of whole frames, with and without normalisation."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

from image_restoration_amd.data import DeviceClipPipeline, REDSDataset
from image_restoration_amd.data import transforms as T

pytestmark = pytest.mark.gpu

FRAMES, LQ_H, LQ_W, GT_SIZE = 5, 13, 22, 32
PATCH = GT_SIZE // 4


def _clips(tmp_path):
    rng = np.random.default_rng(0)
    for clip in ('001', '002', '003'):
        for kind, (h, w) in (('lq', (LQ_H, LQ_W)), ('gt', (LQ_H * 4, LQ_W * 4))):
            d = tmp_path / kind / clip
            d.mkdir(parents=True)
            for f in range(FRAMES):
                Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(d / f'{f:08d}.png')
    meta = tmp_path / 'meta.txt'
    meta.write_text(''.join(f'{c} {FRAMES} ({LQ_H * 4},{LQ_W * 4},3)\n' for c in ('001', '002', '003')))
    return dict(name='REDS', type='REDSDataset', dataroot_gt=str(tmp_path / 'gt'), dataroot_lq=str(tmp_path / 'lq'), dataroot_flow=None,
                meta_info_file=str(meta), val_partition='REDS4', io_backend=dict(type='disk'), num_frame=3, gt_size=GT_SIZE,
                interval_list=[1, 2], random_reverse=True, use_flip=True, use_rot=True, scale=4, phase='train')


@pytest.mark.parametrize('mode,norm', [(True, False), ('full', False), ('full', True)])
def test_device_clip_pipeline_is_bit_identical_to_the_host_pipeline(cuda, tmp_path, mode, norm):
    base = _clips(tmp_path)
    if norm:
        base.update(mean=[0.4, 0.5, 0.45], std=[0.25, 0.5, 0.2])
    host, dev = REDSDataset(dict(base)), REDSDataset(dict(base, device_augment=mode))
    pipe = DeviceClipPipeline(base)
    seen = set()
    for rep in range(12):
        want, items = [], []
        for i in (rep % FRAMES, FRAMES + (rep + 2) % FRAMES, 2 * FRAMES + (rep + 3) % FRAMES):   # a batch of 3, one item per clip
            random.seed(1000 * rep + i)
            want.append(host[i])
            random.seed(1000 * rep + i)
            items.append(dev[i])
        batch = torch.utils.data.default_collate(items)
        assert tuple(batch['lq_u8'].shape) == ((3, 3, LQ_H, LQ_W, 3) if mode == 'full' else (3, 3, PATCH, PATCH, 3))
        seen |= set(int(s) for s in batch['sym'])
        out = pipe({k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in batch.items()})
        assert tuple(out['lq'].shape) == (3, 3, 3, PATCH, PATCH) and tuple(out['gt'].shape) == (3, 3, GT_SIZE, GT_SIZE)
        assert 'lq_u8' not in out and 'sym' not in out and 'window' not in out and out['key'] == [w['key'] for w in want]
        assert torch.equal(out['lq'].cpu(), torch.stack([w['lq'] for w in want]))
        assert torch.equal(out['gt'].cpu(), torch.stack([w['gt'] for w in want]))
    assert {s & T.SYM_TRANSPOSE for s in seen} == {0, T.SYM_TRANSPOSE}            # transposing and non-transposing symmetries


def test_a_window_in_the_last_row_and_column_of_every_frame(cuda, tmp_path):
    """The crop origin at (H - patch, W - patch) for one clip of the batch, the origin (0, 0) for another, each with a transposing
    and a non-transposing symmetry: the device takes the same windows of all t frames as numpy does."""
    base = _clips(tmp_path)
    dev = REDSDataset(dict(base, device_augment='full'))
    pipe = DeviceClipPipeline(base)
    random.seed(3)
    items = [dev[1], dev[FRAMES + 2], dev[2 * FRAMES + 3]]
    batch = torch.utils.data.default_collate(items)
    batch['window'] = torch.tensor([[LQ_H - PATCH, LQ_W - PATCH], [0, 0], [LQ_H - PATCH, 0]], dtype=torch.int32)
    batch['sym'] = torch.tensor([T.SYM_TRANSPOSE | T.SYM_HFLIP, T.SYM_VFLIP, 7], dtype=torch.int32)
    out = pipe({k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in batch.items()})
    for b in range(3):
        top, left = (int(v) for v in batch['window'][b])
        code = int(batch['sym'][b])
        for k in range(3):
            win = items[b]['lq_u8'][k][top:top + PATCH, left:left + PATCH]
            want = T.apply_symmetry(win, code)[..., ::-1].astype(np.float32) / 255.
            assert np.array_equal(out['lq'][b, k].cpu().numpy(), want.transpose(2, 0, 1)), (b, k)
        win = items[b]['gt_u8'][top * 4:top * 4 + GT_SIZE, left * 4:left * 4 + GT_SIZE]
        want = T.apply_symmetry(win, code)[..., ::-1].astype(np.float32) / 255.
        assert np.array_equal(out['gt'][b].cpu().numpy(), want.transpose(2, 0, 1)), b
