"""Training BasicVSR from option files, the host side (no GPU): the refusals of VideoRecurrentModel with ``is_train``,
REDSRecurrentDataset and the recurrent mode of SyntheticClipDataset, and the two shipped option files.

The reference's REDSRecurrentDataset cannot be imported here (its package needs cv2, which is not installed), so what a seeded run
can observe of it is restated below from basicsr/data/reds_dataset.py:298-365 and transforms.py:26-158: the calls on Python's
``random`` in their order.  The frames are those of tests/test_video_data_host.py: they carry their clip position and pixel
coordinates in their channels, so an item shows which frames, which window and which symmetry it was made from."""
import os
import random
import sys

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from image_restoration_amd.data import REDSRecurrentDataset, SyntheticClipDataset
from image_restoration_amd.models.video_recurrent_model import VideoRecurrentModel
from image_restoration_amd.utils.registry import DATASET_REGISTRY

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_video_data_host as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, SCALE, GT_SIZE, PATCH = D.FRAMES, D.SCALE, D.GT_SIZE, D.PATCH
CLIPS = ('000', '001', '002', '011')            # 000 and 011 are REDS4's held-out clips


# --------------------------------------------------------------------------------------------------------- the model
def test_training_refusals_name_what_is_supported():
    base = dict(is_train=True, network_g=dict(type='BasicVSR'), path={})
    with pytest.raises(NotImplementedError, match='follow-up') as e:          # before opt['train'] is read: there is none here
        VideoRecurrentModel(dict(base, num_gpu=0))
    assert 'HIP device' in str(e.value) and 'BasicVSR' in str(e.value)
    with pytest.raises(NotImplementedError, match='follow-up') as e:
        VideoRecurrentModel(dict(base, num_gpu=1, network_g=dict(type='IconVSR')))
    assert "'IconVSR'" in str(e.value) and 'supported: network_g.type BasicVSR' in str(e.value)
    with pytest.raises(NotImplementedError, match='follow-up') as e:
        VideoRecurrentModel(dict(base, num_gpu=1, network_g=dict(type='BasicVSR', compute_dtype='bf16')))
    assert "'bf16'" in str(e.value) and 'fp32' in str(e.value)


# -------------------------------------------------------------------------------------------------------- the dataset
@pytest.fixture(scope='module')
def clips(tmp_path_factory):
    root = tmp_path_factory.mktemp('reds_recurrent')
    for clip in CLIPS:
        for kind, make in (('lq', D._lq), ('gt', D._gt)):
            d = root / kind / clip
            d.mkdir(parents=True)
            for f in range(FRAMES):
                Image.fromarray(make(f)).save(d / f'{f:08d}.png')
    meta = root / 'meta.txt'
    meta.write_text(''.join(f'{c} {FRAMES} ({D.LQ_H * SCALE},{D.LQ_W * SCALE},3)\n' for c in CLIPS))
    return root, meta


def _opt(clips, **kw):
    root, meta = clips
    opt = dict(name='REDS', type='REDSRecurrentDataset', dataroot_gt=str(root / 'gt'), dataroot_lq=str(root / 'lq'),
               meta_info_file=str(meta), val_partition='REDS4', test_mode=False, io_backend=dict(type='disk'), num_frame=3,
               gt_size=GT_SIZE, interval_list=[1], random_reverse=False, use_flip=True, use_rot=True, scale=SCALE, phase='train')
    opt.update(kw)
    return opt


def _reference_draws(start, num_frame, interval_list, random_reverse, use_flip, use_rot):
    """The reference's calls on ``random`` for one item, in its order (its literal 100 is the clip's length here)."""
    interval = random.choice(interval_list)
    redrawn = start > FRAMES - num_frame
    if redrawn:
        start = random.randint(0, FRAMES - num_frame)
    neighbours = list(range(start, start + num_frame, interval))
    if random_reverse and random.random() < 0.5:
        neighbours.reverse()
    top = random.randint(0, D.LQ_H - PATCH)       # paired_random_crop
    left = random.randint(0, D.LQ_W - PATCH)
    hflip = use_flip and random.random() < 0.5    # augment
    vflip = use_rot and random.random() < 0.5
    rot90 = use_rot and random.random() < 0.5
    return neighbours, (top, left), (hflip, vflip, rot90), redrawn, interval


@pytest.mark.parametrize('kw', [dict(), dict(interval_list=[1, 2], random_reverse=True), dict(num_frame=5), dict(use_flip=False),
                                dict(use_rot=False, random_reverse=True), dict(num_frame=4)])
def test_recurrent_items_follow_the_reference_draw_order(clips, kw):
    assert DATASET_REGISTRY.get('REDSRecurrentDataset') is REDSRecurrentDataset
    ds = REDSRecurrentDataset(_opt(clips, **kw))
    o = ds.opt
    assert len(ds) == 2 * FRAMES and ds.keys[0] == '001/00000000' and ds.keys[-1] == f'002/{FRAMES - 1:08d}'
    redraws, kept, intervals, reversals = 0, 0, set(), 0
    for seed in range(6):
        for index in (0, 1, 3, FRAMES - 2, FRAMES - 1, FRAMES + 2):
            random.seed(seed * 100 + index)
            nbrs, (top, left), sym, redrawn, interval = _reference_draws(index % FRAMES, o['num_frame'], o['interval_list'],
                                                                        o['random_reverse'], o['use_flip'], o['use_rot'])
            after = random.random()
            random.seed(seed * 100 + index)
            item = ds[index]
            assert random.random() == after                                   # the same number of draws was taken
            assert set(item) == {'lq', 'gt', 'key'} and item['key'] == ds.keys[index]
            lq, gt = item['lq'], item['gt']
            t = len(nbrs)
            assert t == -(-o['num_frame'] // interval)                        # the reference's range: fewer frames for an interval > 1
            assert lq.dtype == torch.float32 and gt.dtype == torch.float32
            assert tuple(lq.shape) == (t, 3, PATCH, PATCH) and tuple(gt.shape) == (t, 3, GT_SIZE, GT_SIZE)
            assert [int(round(float(f[0, 0, 0]) * 255 / 30)) for f in lq] == nbrs == [int(round(float(f[0, 0, 0]) * 255 / 30)) for f in gt]
            assert min(nbrs) >= 0 and max(nbrs) <= FRAMES - 1
            want_lq = torch.stack([D._chw(D._sym(D._lq(n)[top:top + PATCH, left:left + PATCH], *sym)) for n in nbrs])
            want_gt = torch.stack([D._chw(D._sym(D._gt(n)[top * SCALE:top * SCALE + GT_SIZE, left * SCALE:left * SCALE + GT_SIZE], *sym))
                                   for n in nbrs])
            assert torch.equal(lq, want_lq) and torch.equal(gt, want_gt)
            redraws += redrawn
            kept += (not redrawn) and nbrs[0 if nbrs[0] < nbrs[-1] else -1] == index % FRAMES
            intervals.add(interval)
            reversals += nbrs[0] > nbrs[-1]
    assert redraws > 0 and kept > 0                       # the short-clip randint branch was taken, and the plain one
    assert intervals == set(o['interval_list'])
    assert (reversals > 0) == bool(o['random_reverse'])


def test_partitions_in_both_test_modes_and_refusals(clips, tmp_path):
    train, held = REDSRecurrentDataset(_opt(clips)), REDSRecurrentDataset(_opt(clips, test_mode=True))
    assert {k.split('/')[0] for k in train.keys} == {'001', '002'} and {k.split('/')[0] for k in held.keys} == {'000', '011'}
    assert len(train) == len(held) == 2 * FRAMES
    official = REDSRecurrentDataset(_opt(clips, val_partition='official'))
    assert {k.split('/')[0] for k in official.keys} == set(CLIPS) and len(REDSRecurrentDataset(_opt(clips, val_partition='official', test_mode=True))) == 0
    random.seed(3)
    item = held[FRAMES + 1]
    assert item['key'] == '011/00000001' and tuple(item['gt'].shape) == (3, 3, GT_SIZE, GT_SIZE)
    with pytest.raises(ValueError, match='Wrong validation partition'):
        REDSRecurrentDataset(_opt(clips, val_partition='REDS5'))
    for kw, word in ((dict(dataroot_flow='flows'), 'dataroot_flow'), (dict(io_backend=dict(type='lmdb')), 'lmdb'),
                     (dict(device_augment=True), 'follow-up')):
        with pytest.raises(NotImplementedError, match=word):
            REDSRecurrentDataset(_opt(clips, **kw))
    with pytest.raises(ValueError, match='num_frame is 9'):
        REDSRecurrentDataset(_opt(clips, num_frame=9))
    # interval_list and random_reverse default as in the reference
    o = _opt(clips)
    del o['interval_list'], o['random_reverse']
    ds = REDSRecurrentDataset(o)
    assert ds.interval_list == [1] and ds.random_reverse is False


def test_synthetic_recurrent_clips_carry_every_ground_truth_frame():
    base = dict(num_samples=5, gt_size=32, scale=4, max_motion=2, seed=3)
    plain, rec = SyntheticClipDataset(dict(base, num_frame=5)), SyntheticClipDataset(dict(base, num_frame=5, recurrent=True))
    a, b = plain[2], rec[2]
    assert set(a) == {'lq', 'gt', 'key'} and tuple(a['gt'].shape) == (3, 32, 32)          # the default keeps today's items
    assert set(b) == {'lq', 'gt', 'key', 'folder'} and tuple(b['gt'].shape) == (5, 3, 32, 32) and tuple(b['lq'].shape) == (5, 3, 8, 8)
    assert torch.equal(b['lq'], a['lq']) and torch.equal(b['gt'][2], a['gt']) and b['key'] == a['key']
    want = b['gt'].reshape(5, 3, 8, 4, 8, 4).mean(dim=(3, 5))
    assert float((b['lq'] - want).abs().max()) <= 1e-6                                     # each LQ frame is its GT frame's box average
    assert rec.data_info['folder'].count(b['folder']) == 5 and len(set(rec.data_info['folder'])) == 5
    even = SyntheticClipDataset(dict(base, num_frame=4, recurrent=True))
    assert tuple(even[0]['gt'].shape) == (4, 3, 32, 32)
    with pytest.raises(ValueError, match='odd'):
        SyntheticClipDataset(dict(base, num_frame=4))
    with pytest.raises(ValueError, match='num_frame >= 2'):
        SyntheticClipDataset(dict(base, num_frame=1, recurrent=True))


# ------------------------------------------------------------------------------------------------------ option files
def test_shipped_option_files():
    from image_restoration_amd.utils.registry import MODEL_REGISTRY
    reds = yaml.safe_load(open(os.path.join(ROOT, 'options', 'train', 'BasicVSR', 'train_BasicVSR_REDS.yml')))
    assert reds['model_type'] == 'VideoRecurrentModel' and MODEL_REGISTRY.get(reds['model_type']) is VideoRecurrentModel
    assert reds['scale'] == 4 and reds['num_gpu'] == 8 and reds['manual_seed'] == 0
    tr = reds['datasets']['train']
    assert tr['type'] == 'REDSRecurrentDataset' and DATASET_REGISTRY.get(tr['type']) is REDSRecurrentDataset
    # the reference's recipe, value for value
    assert (tr['num_frame'], tr['gt_size'], tr['interval_list'], tr['random_reverse'], tr['use_flip'], tr['use_rot']) == (15, 256, [1], False, True, True)
    assert (tr['val_partition'], tr['test_mode'], tr['io_backend'], tr['batch_size_per_gpu'], tr['num_worker_per_gpu'], tr['dataset_enlarge_ratio']) == \
        ('REDS4', False, {'type': 'disk'}, 4, 6, 200)
    assert reds['datasets']['val']['type'] == 'VideoRecurrentTestDataset' and reds['datasets']['val']['cache_data'] is True
    assert reds['network_g'] == dict(type='BasicVSR', num_feat=64, num_block=30,
                                     spynet_path='experiments/pretrained_models/flownet/spynet_sintel_final-3d2a1287.pth')
    t = reds['train']
    assert t['optim_g'] == dict(type='Adam', lr=2e-4, weight_decay=0, betas=[0.9, 0.99])
    assert t['scheduler'] == dict(type='CosineAnnealingRestartLR', periods=[300000], restart_weights=[1], eta_min=1e-7)
    assert (t['total_iter'], t['warmup_iter'], t['fix_flow'], t['flow_lr_mul'], t['deterministic_backward']) == (300000, -1, 5000, 0.125, True)
    assert t['pixel_opt'] == dict(type='CharbonnierLoss', loss_weight=1.0, reduction='mean')
    assert reds['val']['val_freq'] == 5e3 and reds['val']['save_img'] is False
    assert reds['val']['metrics'] == dict(psnr=dict(type='calculate_psnr', crop_border=0, test_y_channel=False))
    assert reds['logger']['print_freq'] == 100 and reds['logger']['save_checkpoint_freq'] == 5e3

    syn = yaml.safe_load(open(os.path.join(ROOT, 'options', 'train', 'BasicVSR', 'train_BasicVSR_x4_synthetic.yml')))
    assert syn['model_type'] == 'VideoRecurrentModel' and syn['num_gpu'] == 1 and syn['network_g']['type'] == 'BasicVSR'
    assert syn['network_g']['num_block'] < 30 and syn['train']['fix_flow'] and syn['train']['flow_lr_mul'] != 1
    for phase in ('train', 'val'):
        d = syn['datasets'][phase]
        assert d['type'] == 'SyntheticClipDataset' and d['recurrent'] is True
        item = SyntheticClipDataset(dict(d, num_samples=2, scale=syn['scale']))[1]
        assert tuple(item['gt'].shape) == (d['num_frame'], 3, d['gt_size'], d['gt_size'])
    assert syn['val']['metrics'] and syn['val']['save_img'] is False
