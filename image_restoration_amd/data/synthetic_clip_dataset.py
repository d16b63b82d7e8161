"""Synthetic training clips with REDSDataset's sample dict (``lq`` [t, c, h, w], ``gt`` [c, h, w] of the centre frame, ``key``), so
the EDVR quick start runs without REDS: one random texture per clip (uniform noise, numpy PCG64), translated from frame to frame by
the clip's own motion, a whole number of LQ pixels per frame, and the LQ frames are the x``scale`` box average of the GT frames.
The motion is free of sub-pixel parts on both grids, so every LQ frame is exactly the box average of a GT window.

``recurrent: true`` gives REDSRecurrentDataset's sample dict instead — ``gt`` [t, c, H, W], the ground truth of every frame — for
the networks that return the whole clip (BasicVSR), and accepts any ``num_frame`` >= 2.  Such a set also serves as a validation set of
VideoRecurrentModel: every clip is a folder of its own (``folder`` in the item, ``data_info['folder']`` one entry per frame).  The
default (false) keeps the items above.

``video_test: true`` (not recurrent) adds what VideoBaseModel's validation reads from a VideoTestDataset item — ``folder``, ``idx``
and ``lq_path`` — and ``data_info['folder']``, every clip a folder of one centre frame; with ``scale: 1`` the LQ frames are the GT
frames, the input of a network that restores pre-upsampled frames (TOFlow)."""
import numpy as np
import torch
from torch.utils import data

from ..utils.registry import DATASET_REGISTRY


@DATASET_REGISTRY.register()
class SyntheticClipDataset(data.Dataset):

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.length = int(opt.get('num_samples', 256))
        self.gt_size = int(opt.get('gt_size', 128))
        self.scale = int(opt.get('scale', 4))
        self.num_frame = int(opt.get('num_frame', 5))
        self.max_motion = int(opt.get('max_motion', 2))   # LQ pixels per frame, each axis
        self.seed = int(opt.get('seed', 0))
        self.recurrent = bool(opt.get('recurrent', False))
        if self.recurrent:
            if self.num_frame < 2:
                raise ValueError(f'a recurrent clip needs num_frame >= 2, but got {self.num_frame}')
        elif self.num_frame % 2 != 1:
            raise ValueError(f'num_frame should be odd number, but got {self.num_frame}')
        self.video_test = bool(opt.get('video_test', False)) and not self.recurrent
        if self.recurrent:
            self.data_info = {'folder': [f'{i:08d}' for i in range(self.length) for _ in range(self.num_frame)]}
        elif self.video_test:
            self.data_info = {'folder': [f'{i:08d}' for i in range(self.length)]}
        if self.gt_size % self.scale:
            raise ValueError(f'gt_size={self.gt_size} must be a multiple of scale={self.scale}')

    def __len__(self):
        return self.length

    def __getitem__(self, index):
        rng = np.random.default_rng(self.seed * 1000003 + index)
        t, s, g = self.num_frame, self.scale, self.gt_size
        my, mx = (int(v) for v in rng.integers(-self.max_motion, self.max_motion + 1, size=2))
        reach = self.max_motion * (t - 1) * s
        texture = rng.random((3, g + reach, g + reach), dtype=np.float32)
        y0, x0 = (reach if my < 0 else 0), (reach if mx < 0 else 0)
        frames = np.stack([texture[:, y0 + k * my * s:y0 + k * my * s + g, x0 + k * mx * s:x0 + k * mx * s + g] for k in range(t)])
        lq = frames.reshape(t, 3, g // s, s, g // s, s).mean(axis=(3, 5), dtype=np.float32)
        if self.recurrent:
            return {'lq': torch.from_numpy(np.ascontiguousarray(lq)), 'gt': torch.from_numpy(np.ascontiguousarray(frames)),
                    'key': f'synthetic/{index:08d}', 'folder': f'{index:08d}'}
        item = {'lq': torch.from_numpy(np.ascontiguousarray(lq)), 'gt': torch.from_numpy(np.ascontiguousarray(frames[t // 2])),
                'key': f'synthetic/{index:08d}'}
        if self.video_test:
            item.update(folder=f'{index:08d}', idx='0/1', lq_path=f'synthetic/{index:08d}/{t // 2:08d}.png')
        return item
