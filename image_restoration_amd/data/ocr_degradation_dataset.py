"""OCRDegradationDataset: the plate training set of the reference, whose LQ images are made from the GT on the fly
(basicsr/data/ocr_degradation_dataset.py:18-292): blur, downsample by a random factor, Gaussian noise, JPEG, resize back, colour
jitter, gray, round, normalise.

Here the host only decodes, resizes the GT to ``input_height`` x ``input_width`` and DRAWS; the pixel work of the chain runs on
the device, one HIP launch per stage and batch (data/device_pipeline.py:DeviceDegradePipeline, include/sr_hip_degrade.h).  That is
the only mode: the dataset needs ``device_degrade: true`` (and the training loop ``prefetch_mode: cuda``).

An item carries
  gt_u8    uint8 [input_height, input_width, 3], BGR as decoded
  sym      int32, bit 0 the horizontal flip (square inputs; sr_patch_augment_u8_f32 takes a symmetry code only for square windows,
           so a non-square GT is flipped here, on uint8, and travels with sym = 0)
  kernel   float32 [blur_kernel_size, blur_kernel_size]
  scale    float64, the downsample factor (the low size is int(h // scale) x int(w // scale), in float64 as in the reference)
  sigma    float32, the noise level on the 0..255 scale (0 when noise_range is None: the stage is skipped)
  quality  float32, the JPEG quality (100 when jpeg_range is None: the stage is skipped)
  jitter   float32 [3], the colour shift in RGB order (zeros when none was drawn)
  gray     float32 0 / 1
  gt_path

The draws follow the reference's order (:229-259): flip (``random``), kernel kind (``random.choices``) and its parameters
(``numpy.random``), downsample factor, noise level and the gray-noise coin of random_generate_gaussian_noise, JPEG quality, the
jitter coin and its three shifts, the gray coin.  The noise itself is drawn on the device.

Differences from the reference, on purpose:
  * random_mixed_kernels is called there with ``min_kernel_size`` in the place of ``sigma_x_range`` (:234-241 against
    degradations.py:419-430), which cannot run; here blur_sigma is both sigma ranges, the rotation range is [-pi, pi] and the beta
    ranges are the defaults, as the call evidently means.  ``min_kernel_size`` is accepted and unused, as there.
  * the GT is resized on uint8 and shipped as uint8; the reference resizes the float image.
  * ``color_jitter_pt_prob``, ``random_mask`` and ``pad_input`` need torchvision or cv2 drawing and raise ValueError when set; so
    do the blur kinds that are not one linear kernel (data/degradations.py).
"""
import glob
import math
import os.path as osp

import numpy as np
from torch.utils.data import Dataset

from ..utils.registry import DATASET_REGISTRY
from . import degradations, transforms
from .image_source import ImageSource


def source_coords(src_len, dst_len):
    """(i0, i1, f) per destination index: the float32 coordinate arithmetic of sr_resize_bilinear_f32."""
    f32 = np.float32
    scale = f32(src_len) / f32(dst_len)
    s = (np.arange(dst_len, dtype=np.float32) + f32(0.5)) * scale - f32(0.5)
    fl = np.floor(s)
    i0 = fl.astype(np.int64)
    f = (s - fl).astype(np.float32)
    i0[s < 0], f[s < 0] = 0, 0
    top = i0 >= src_len - 1
    i0[top], f[top] = src_len - 1, 0
    return i0, np.minimum(i0 + 1, src_len - 1), f


def resize_bilinear_numpy(img, height, width):
    """Bilinear resize of an HWC image (any real dtype) to ``height`` x ``width``, half-pixel centres, no antialiasing: the
    coordinates in float32 as the kernel computes them, the blend in float64.  Returns float64."""
    y0, y1, fy = source_coords(img.shape[0], height)
    x0, x1, fx = source_coords(img.shape[1], width)
    v = img.astype(np.float64)
    fy, fx = fy.astype(np.float64)[:, None, None], fx.astype(np.float64)[None, :, None]
    top = (1 - fx) * v[y0][:, x0] + fx * v[y0][:, x1]
    bottom = (1 - fx) * v[y1][:, x0] + fx * v[y1][:, x1]
    return (1 - fy) * top + fy * bottom


def resize_bilinear_u8(img, height, width):
    if img.shape[:2] == (height, width):
        return np.ascontiguousarray(img)
    return np.clip(np.rint(resize_bilinear_numpy(img, height, width)), 0, 255).astype(np.uint8)


@DATASET_REGISTRY.register()
class OCRDegradationDataset(ImageSource, Dataset):

    def __init__(self, opt):
        Dataset.__init__(self)
        if not opt.get('device_degrade'):
            raise ValueError('OCRDegradationDataset degrades on the device only: set device_degrade: true (and prefetch_mode: cuda)')
        for key in ('color_jitter_pt_prob', 'random_mask', 'pad_input'):
            if opt.get(key):
                raise ValueError(f"OCRDegradationDataset: '{key}' is not supported (it needs torchvision or cv2 drawing on the host)")
        self.gt_folder = opt['dataroot_gt']
        self._init_source(opt, (self.gt_folder,), ('gt',))
        self.input_width, self.input_height = int(opt['input_width']), int(opt['input_height'])
        if self.io_backend_opt['type'] == 'lmdb':
            if not self.gt_folder.endswith('.lmdb'):
                raise ValueError(f"'dataroot_gt' should end with '.lmdb', but received {self.gt_folder}")
            with open(osp.join(self.gt_folder, 'meta_info.txt')) as fin:
                self.paths = [line.split('.')[0] for line in fin]
        else:
            self.paths = []
            for pattern in ('/*.jpg', '/*.png', '/*/*.jpg', '/*/*.png'):
                self.paths += sorted(glob.glob(self.gt_folder + pattern))
        self.blur_kernel_size = int(opt['blur_kernel_size'])
        self.min_kernel_size = opt.get('min_kernel_size')
        self.kernel_list, self.kernel_prob = list(opt['kernel_list']), list(opt['kernel_prob'])
        degradations.check_kernel_list(self.kernel_list)
        if self.blur_kernel_size % 2 != 1 or self.blur_kernel_size > 21:
            raise ValueError(f'blur_kernel_size {self.blur_kernel_size} is not supported: odd, at most 21')
        self.blur_sigma = opt['blur_sigma']
        self.downsample_range = opt['downsample_range']
        self.noise_range = opt.get('noise_range')
        self.jpeg_range = opt.get('jpeg_range')
        self.color_jitter_prob = opt.get('color_jitter_prob')
        self.color_jitter_shift = opt.get('color_jitter_shift', 20) / 255.
        self.gray_prob = opt.get('gray_prob')

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, index):
        gt_path = self.paths[index]
        gt = resize_bilinear_u8(self.decode(gt_path, 'gt', as_float=False), self.input_height, self.input_width)
        code = transforms.draw_symmetry(self.opt.get('use_hflip', False), False)
        if code and self.input_height != self.input_width:
            gt, code = np.ascontiguousarray(gt[:, ::-1]), 0
        kernel = degradations.draw_blur_kernel(self.kernel_list, self.kernel_prob, self.blur_kernel_size, self.blur_sigma, self.blur_sigma,
                                               [-math.pi, math.pi], noise_range=None)
        scale = np.random.uniform(self.downsample_range[0], self.downsample_range[1])
        sigma = 0.0
        if self.noise_range is not None:
            sigma = np.random.uniform(self.noise_range[0], self.noise_range[1])
            np.random.uniform()          # the gray-noise coin of random_generate_gaussian_noise (gray_prob = 0: never gray)
        quality = 100.0
        if self.jpeg_range is not None:
            quality = np.random.uniform(self.jpeg_range[0], self.jpeg_range[1])
        jitter = np.zeros(3, np.float32)
        if self.color_jitter_prob is not None and np.random.uniform() < self.color_jitter_prob:
            bgr = np.random.uniform(-self.color_jitter_shift, self.color_jitter_shift, 3).astype(np.float32)
            jitter = np.ascontiguousarray(bgr[::-1])      # drawn per BGR channel; the tensors are RGB
        gray = bool(self.gray_prob) and np.random.uniform() < self.gray_prob
        return dict(gt_u8=gt, sym=np.int32(code), kernel=kernel, scale=np.float64(scale), sigma=np.float32(sigma),
                    quality=np.float32(quality), jitter=jitter, gray=np.float32(gray),
                    gt_path=gt_path)
