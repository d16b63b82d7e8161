"""VideoTestDataset: every frame of every clip of ``<root>/<clip>/<frame>`` as the centre of a ``num_frame`` window (behaviour of
basicsr/data/video_test_dataset.py:11-129).

Option keys of the reference: dataroot_gt, dataroot_lq, io_backend (not lmdb), cache_data, name, meta_info_file (optional: the
clips to use, first word of each line; otherwise every sub-folder of the roots, sorted), num_frame, padding (``replicate`` |
``reflection`` | ``reflection_circle`` | ``circle``, data_util.generate_frame_indices).  An item is ``lq`` [t, c, h, w], ``gt``
[c, h, w] (CHW RGB float32 in [0, 1]), ``folder``, ``idx`` as ``'i/max'``, ``border`` (1 for the num_frame // 2 frames at either end
of a clip) and ``lq_path`` of the centre frame.  ``data_info`` lists the same per frame, as VideoBaseModel.validation reads it.

Deviations: any dataset name is taken (the reference refuses names other than Vid4 / REDS4 / REDSofficial although it treats them
alike); PIL decodes instead of cv2.  ``VideoTestDUFDataset`` below makes its LQ frames with the DUF downsampling and
``VideoRecurrentTestDataset`` hands out whole folders; the Vimeo90K test datasets are not built."""
import logging
import os

import torch
from torch.utils.data import Dataset

from ..utils.registry import DATASET_REGISTRY
from . import data_util
from .image_source import ImageSource


def _subfolders(root):
    with os.scandir(root) as it:
        return sorted(e.name for e in it if e.is_dir() and e.name[:1] != '.')


@DATASET_REGISTRY.register()
class VideoTestDataset(ImageSource, Dataset):

    def __init__(self, opt):
        Dataset.__init__(self)
        if opt['io_backend']['type'] == 'lmdb':
            raise AssertionError('No need to use lmdb during validation/test.')
        self.gt_root, self.lq_root = opt['dataroot_gt'], opt['dataroot_lq']
        self._init_source(opt, (self.lq_root, self.gt_root), ('lq', 'gt'))
        self.cache_data = opt['cache_data']
        self.data_info = {'lq_path': [], 'gt_path': [], 'folder': [], 'idx': [], 'border': []}
        log = logging.getLogger('basicsr')
        log.info(f'Generate data info for VideoTestDataset - {opt["name"]}')
        if opt.get('meta_info_file') is not None:
            with open(opt['meta_info_file']) as fin:
                names = [line.split()[0] for line in fin if line.strip()]
        else:
            names = _subfolders(self.lq_root)
            if names != _subfolders(self.gt_root):
                raise AssertionError(f'Different clips in lq ({self.lq_root}) and gt ({self.gt_root}) folders')
        self.imgs_lq, self.imgs_gt = {}, {}
        for name in names:
            lq_paths = [os.path.join(self.lq_root, name, f) for f in data_util.scandir(os.path.join(self.lq_root, name))]
            gt_paths = [os.path.join(self.gt_root, name, f) for f in data_util.scandir(os.path.join(self.gt_root, name))]
            max_idx = len(lq_paths)
            if max_idx != len(gt_paths):
                raise AssertionError(f'Different number of images in lq ({max_idx}) and gt folders ({len(gt_paths)})')
            self.data_info['lq_path'].extend(lq_paths)
            self.data_info['gt_path'].extend(gt_paths)
            self.data_info['folder'].extend([name] * max_idx)
            self.data_info['idx'].extend(f'{i}/{max_idx}' for i in range(max_idx))
            border = [0] * max_idx
            for i in range(opt['num_frame'] // 2):
                border[i] = 1
                border[max_idx - i - 1] = 1
            self.data_info['border'].extend(border)
            if self.cache_data:
                log.info(f'Cache {name} for VideoTestDataset...')
                self.imgs_lq[name] = self.read_sequence(lq_paths, 'lq')
                self.imgs_gt[name] = self.read_sequence(gt_paths, 'gt')
            else:
                self.imgs_lq[name] = lq_paths
                self.imgs_gt[name] = gt_paths

    def read_sequence(self, paths, key):
        """[t, c, h, w] RGB float32 in [0, 1] of the files in ``paths``."""
        return torch.stack(self.to_tensors(*[self.decode(p, key) for p in paths]), dim=0)

    def __len__(self):
        return len(self.data_info['gt_path'])

    def __getitem__(self, index):
        folder = self.data_info['folder'][index]
        idx, max_idx = (int(v) for v in self.data_info['idx'][index].split('/'))
        select = data_util.generate_frame_indices(idx, max_idx, self.opt['num_frame'], padding=self.opt['padding'])
        if self.cache_data:
            lq = self.imgs_lq[folder].index_select(0, torch.LongTensor(select))
            gt = self.imgs_gt[folder][idx]
        else:
            lq = self.read_sequence([self.imgs_lq[folder][i] for i in select], 'lq')
            gt = self.read_sequence([self.imgs_gt[folder][idx]], 'gt')[0]
        return {'lq': lq, 'gt': gt, 'folder': folder, 'idx': self.data_info['idx'][index],
                'border': self.data_info['border'][index], 'lq_path': self.data_info['lq_path'][index]}


@DATASET_REGISTRY.register()
class VideoTestDUFDataset(VideoTestDataset):
    """The test set of DUF (behaviour of basicsr/data/video_test_dataset.py:202-251): VideoTestDataset with two more keys,
    ``use_duf_downsampling`` (the LQ frames are made from the GT frames with data_util.duf_downsample, 13 taps) and ``scale``.
    Without ``cache_data`` the GT frames are cropped to a multiple of ``scale`` first, as the reference does; with it the cached
    frames are used as they are.  The returned keys are VideoTestDataset's."""

    def _mod_crop(self, frames):
        s = self.opt['scale']
        h, w = frames.shape[-2:]
        return frames[..., :h - h % s, :w - w % s]

    def __getitem__(self, index):
        folder = self.data_info['folder'][index]
        idx, max_idx = (int(v) for v in self.data_info['idx'][index].split('/'))
        select = data_util.generate_frame_indices(idx, max_idx, self.opt['num_frame'], padding=self.opt['padding'])
        down = self.opt['use_duf_downsampling']
        if self.cache_data:
            lq = (self.imgs_gt if down else self.imgs_lq)[folder].index_select(0, torch.LongTensor(select))
            gt = self.imgs_gt[folder][idx]
        else:
            if down:
                lq = self._mod_crop(self.read_sequence([self.imgs_gt[folder][i] for i in select], 'gt'))
            else:
                lq = self.read_sequence([self.imgs_lq[folder][i] for i in select], 'lq')
            gt = self._mod_crop(self.read_sequence([self.imgs_gt[folder][idx]], 'gt'))[0]
        if down:
            lq = data_util.duf_downsample(lq, kernel_size=13, scale=self.opt['scale'])
        return {'lq': lq, 'gt': gt, 'folder': folder, 'idx': self.data_info['idx'][index],
                'border': self.data_info['border'][index], 'lq_path': self.data_info['lq_path'][index]}


@DATASET_REGISTRY.register()
class VideoRecurrentTestDataset(VideoTestDataset):
    """The test set of the recurrent networks (behaviour of basicsr/data/video_test_dataset.py:255-287): an item is a whole
    folder, ``lq`` [t, c, h, w] and ``gt`` [t, c, 4h, 4w] with ``folder``; ``len`` is the number of folders.  ``padding`` and
    ``num_frame`` only shape ``data_info`` (``num_frame`` defaults to 1 here).  ``cache_data: true`` only, as the reference."""

    def __init__(self, opt):
        super().__init__(dict(opt, num_frame=opt.get('num_frame', 1)))
        self.folders = sorted(set(self.data_info['folder']))

    def __len__(self):
        return len(self.folders)

    def __getitem__(self, index):
        if not self.cache_data:
            raise NotImplementedError('Without cache_data is not implemented.')
        folder = self.folders[index]
        return {'lq': self.imgs_lq[folder], 'gt': self.imgs_gt[folder], 'folder': folder}
