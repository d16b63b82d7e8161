"""REDSDataset: training clips of the REDS layout, ``<root>/<clip>/<frame:08d>.png`` (behaviour of basicsr/data/reds_dataset.py:13-204).

Option keys of the reference: dataroot_gt, dataroot_lq, dataroot_flow, meta_info_file (lines ``<clip> <frames> (h,w,c)``),
val_partition (``REDS4`` | ``official``: clips left out of training), io_backend, num_frame, gt_size, interval_list, random_reverse,
use_flip, use_rot, scale.  An item is ``lq`` [t, c, h, w] and ``gt`` [c, h, w] (the centre frame), CHW RGB float32 in [0, 1], and ``key``.

What a seeded run can observe is kept: the draws from Python's ``random`` and their order — ``choice`` of the interval, ``randint``
of a new centre for as long as the window leaves the clip, ``random()`` for the reversal (only with random_reverse), ``randint`` of
the crop's top then left, then the three coins of ``augment``.

Deviations.  (1) The last frame index of a clip is ``frames - 1`` of its meta-info line, where the reference writes the literal 99
(REDS has 100 frames per clip, so REDS behaves the same; clips of another length work).  (2) Supported are ``dataroot_flow: null``
and ``io_backend.type: disk``; optical-flow inputs and LMDB raise NotImplementedError.  (3) PIL decodes instead of cv2.

Extension ``device_augment`` (as PairedImageDataset): the item carries the uint8 LQ windows [t, h, w, 3], the uint8 GT window and
the symmetry code (``true``), or the whole uint8 frames plus the window origin (``full``); data/device_pipeline.py:DeviceClipPipeline
finishes the batch on the device."""
import logging
import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from ..utils.registry import DATASET_REGISTRY
from . import transforms
from .image_source import ImageSource

_SUPPORTED = 'supported: dataroot_flow: null (LQ and GT frames only) and io_backend.type: disk'
VAL_PARTITIONS = {'REDS4': ['000', '011', '015', '020'], 'official': [f'{v:03d}' for v in range(240, 270)]}


@DATASET_REGISTRY.register()
class REDSDataset(ImageSource, Dataset):

    def __init__(self, opt):
        Dataset.__init__(self)
        if opt.get('dataroot_flow') is not None:
            raise NotImplementedError(f'REDSDataset: optical-flow inputs (dataroot_flow) are not built; {_SUPPORTED}')
        if opt['io_backend']['type'] == 'lmdb':
            raise NotImplementedError(f'REDSDataset: the lmdb backend is not built for clips; {_SUPPORTED}')
        self.gt_root, self.lq_root = opt['dataroot_gt'], opt['dataroot_lq']
        self._init_source(opt, (self.lq_root, self.gt_root), ('lq', 'gt'))
        if opt['num_frame'] % 2 != 1:
            raise AssertionError(f'num_frame should be odd number, but got {opt["num_frame"]}')
        self.num_frame = opt['num_frame']
        self.num_half_frames = opt['num_frame'] // 2
        if opt['val_partition'] not in VAL_PARTITIONS:
            raise ValueError(f'Wrong validation partition {opt["val_partition"]}.' f"Supported ones are ['official', 'REDS4'].")
        held_out = VAL_PARTITIONS[opt['val_partition']]
        self.keys, self.last_frame = [], {}
        with open(opt['meta_info_file']) as fin:
            for line in fin:
                if not line.strip():
                    continue
                folder, frame_num = line.split()[:2]
                if folder in held_out:
                    continue
                self.last_frame[folder] = int(frame_num) - 1
                self.keys.extend(f'{folder}/{i:08d}' for i in range(int(frame_num)))
        self.interval_list = opt['interval_list']
        self.random_reverse = opt['random_reverse']
        mode = opt.get('device_augment', False)
        self.device_augment = bool(mode)
        self.ship_whole_images = mode == 'full'
        logging.getLogger('basicsr').info(f'Temporal augmentation interval list: [{",".join(str(x) for x in self.interval_list)}]; '
                                          f'random reverse is {self.random_reverse}.')

    def __len__(self):
        return len(self.keys)

    def draw_clip(self, index):
        """(clip, centre frame, neighbour list) of item ``index``: the temporal draws."""
        clip_name, frame_name = self.keys[index].split('/')
        centre, last, half = int(frame_name), self.last_frame[clip_name], self.num_half_frames
        interval = random.choice(self.interval_list)
        start, end = centre - half * interval, centre + half * interval
        while start < 0 or end > last:   # a window that leaves the clip: another centre, as often as needed
            centre = random.randint(0, last)
            start, end = centre - half * interval, centre + half * interval
        neighbours = list(range(start, end + 1, interval))
        if self.random_reverse and random.random() < 0.5:
            neighbours.reverse()
        assert len(neighbours) == self.num_frame, f'Wrong length of neighbor list: {len(neighbours)}'
        return clip_name, centre, neighbours

    def __getitem__(self, index):
        scale, gt_size = self.opt['scale'], self.opt['gt_size']
        clip_name, centre, neighbours = self.draw_clip(index)
        gt_path = os.path.join(self.gt_root, clip_name, f'{centre:08d}.png')
        as_float = not self.device_augment
        gt = self.decode(gt_path, 'gt', as_float=as_float)
        lqs = [self.decode(os.path.join(self.lq_root, clip_name, f'{n:08d}.png'), 'lq', as_float=as_float) for n in neighbours]
        lq_patch = transforms.check_pair_geometry(gt.shape, lqs[0].shape, gt_size, scale, gt_path)
        top, left = transforms.draw_window(lqs[0].shape[0], lqs[0].shape[1], lq_patch)
        code = transforms.draw_symmetry(self.opt['use_flip'], self.opt['use_rot'])
        key = self.keys[index]
        if self.device_augment:
            item = {'sym': np.int32(code), 'key': key}
            if self.ship_whole_images:
                item['window'] = np.array([top, left], np.int32)
            else:
                (gt,), lqs = transforms.cut_pair([gt], lqs, top, left, lq_patch, scale, gt_size)
            item.update(lq_u8=np.ascontiguousarray(np.stack(lqs)), gt_u8=np.ascontiguousarray(gt))
            return item
        (gt,), lqs = transforms.cut_pair([gt], lqs, top, left, lq_patch, scale, gt_size)
        tensors = self.to_tensors(*[transforms.apply_symmetry(im, code) for im in lqs + [gt]])
        return {'lq': torch.stack(tensors[:-1], dim=0), 'gt': tensors[-1], 'key': key}


_SUPPORTED_RECURRENT = 'supported: dataroot_flow: null (LQ and GT frames only), io_backend.type: disk, device_augment: false'


@DATASET_REGISTRY.register()
class REDSRecurrentDataset(ImageSource, Dataset):
    """Training clips for the recurrent networks (behaviour of basicsr/data/reds_dataset.py:212-365): an item is ``lq`` [t, c, h, w]
    and ``gt`` [t, c, H, W] — every frame has its ground truth — and ``key``.

    Option keys of the reference: dataroot_gt, dataroot_lq, meta_info_file, val_partition, test_mode (true: ONLY the held-out
    clips), io_backend, num_frame, gt_size, interval_list (default [1]), random_reverse (default false), use_flip, use_rot, scale.

    The draws from Python's ``random`` and their order are kept: ``choice`` of the interval; when the key's frame exceeds
    ``frames - num_frame``, one ``randint(0, frames - num_frame)`` for the start; ``random()`` for the reversal (only with
    random_reverse); ``randint`` of the crop's top then left; the three coins of ``augment``.  The frames are
    ``range(start, start + num_frame, interval)``, as the reference writes it: fewer than num_frame for an interval above 1 (its
    recipes use [1]).

    Deviations, those of REDSDataset.  (1) ``frames`` is the clip's length in its meta-info line, where the reference writes the
    literal 100.  (2) ``dataroot_flow``, the lmdb backend and ``device_augment`` raise NotImplementedError.  (3) PIL decodes
    instead of cv2."""

    def __init__(self, opt):
        Dataset.__init__(self)
        if opt.get('dataroot_flow') is not None:
            raise NotImplementedError(f'REDSRecurrentDataset: optical-flow inputs (dataroot_flow) are not built; {_SUPPORTED_RECURRENT}')
        if opt['io_backend']['type'] == 'lmdb':
            raise NotImplementedError(f'REDSRecurrentDataset: the lmdb backend is not built for clips; {_SUPPORTED_RECURRENT}')
        if opt.get('device_augment', False):
            raise NotImplementedError('REDSRecurrentDataset: device_augment for recurrent clips is the follow-up; '
                                      f'{_SUPPORTED_RECURRENT}')
        self.gt_root, self.lq_root = opt['dataroot_gt'], opt['dataroot_lq']
        self._init_source(opt, (self.lq_root, self.gt_root), ('lq', 'gt'))
        self.num_frame = opt['num_frame']
        if opt['val_partition'] not in VAL_PARTITIONS:
            raise ValueError(f'Wrong validation partition {opt["val_partition"]}.' f"Supported ones are ['official', 'REDS4'].")
        held_out = VAL_PARTITIONS[opt['val_partition']]
        self.keys, self.frames = [], {}
        with open(opt['meta_info_file']) as fin:
            for line in fin:
                if not line.strip():
                    continue
                folder, frame_num = line.split()[:2]
                if (folder in held_out) != bool(opt['test_mode']):
                    continue
                if int(frame_num) < self.num_frame:
                    raise ValueError(f'REDSRecurrentDataset: clip {folder} has {frame_num} frames, num_frame is {self.num_frame}')
                self.frames[folder] = int(frame_num)
                self.keys.extend(f'{folder}/{i:08d}' for i in range(int(frame_num)))
        self.interval_list = opt.get('interval_list', [1])
        self.random_reverse = opt.get('random_reverse', False)
        logging.getLogger('basicsr').info(f'Temporal augmentation interval list: [{",".join(str(x) for x in self.interval_list)}]; '
                                          f'random reverse is {self.random_reverse}.')

    def __len__(self):
        return len(self.keys)

    def draw_clip(self, index):
        """(clip, frame list) of item ``index``: the temporal draws."""
        clip_name, frame_name = self.keys[index].split('/')
        interval = random.choice(self.interval_list)
        start, room = int(frame_name), self.frames[clip_name] - self.num_frame
        if start > room:
            start = random.randint(0, room)
        neighbours = list(range(start, start + self.num_frame, interval))
        if self.random_reverse and random.random() < 0.5:
            neighbours.reverse()
        return clip_name, neighbours

    def __getitem__(self, index):
        scale, gt_size = self.opt['scale'], self.opt['gt_size']
        clip_name, neighbours = self.draw_clip(index)
        lqs = [self.decode(os.path.join(self.lq_root, clip_name, f'{n:08d}.png'), 'lq') for n in neighbours]
        gt_paths = [os.path.join(self.gt_root, clip_name, f'{n:08d}.png') for n in neighbours]
        gts = [self.decode(path, 'gt') for path in gt_paths]
        lq_patch = transforms.check_pair_geometry(gts[0].shape, lqs[0].shape, gt_size, scale, gt_paths[-1])
        top, left = transforms.draw_window(lqs[0].shape[0], lqs[0].shape[1], lq_patch)
        gts, lqs = transforms.cut_pair(gts, lqs, top, left, lq_patch, scale, gt_size)
        code = transforms.draw_symmetry(self.opt['use_flip'], self.opt['use_rot'])
        tensors = self.to_tensors(*[transforms.apply_symmetry(im, code) for im in lqs + gts])
        t = len(lqs)
        return {'lq': torch.stack(tensors[:t], dim=0), 'gt': torch.stack(tensors[t:], dim=0), 'key': self.keys[index]}
