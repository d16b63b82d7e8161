"""DevicePatchPipeline: the per-batch half of the training input pipeline on the MI355X.

``PairedImageDataset(device_augment: true)`` ships, per sample, the uint8 LQ / GT windows it cut (or, with ``device_augment: full``
on equally sized images, the whole uint8 images plus the window origin) and the symmetry code it drew.  This class turns the
collated batch — already in HBM, on the feed's copy stream — into the tensors the model trains on with one HIP launch per tensor
(sr_patch_augment_u8_f32): crop, hflip / vflip / transpose, BGR->RGB, HWC->CHW, /255, (x - mean) / std.  Same draws, same
arithmetic: the result is bit-identical to the host pipeline of the reference (basicsr/data/paired_image_dataset.py:67-98).

``DeviceDegradePipeline`` is the same idea for the plate set, whose LQ images do not exist on disk: the host ships the uint8 GT and
the drawn degradation, the device makes the LQ batch from it (include/sr_hip_degrade.h).
"""
import ctypes as C

import torch

from .. import _lib


def _f3(values):
    return None if values is None else (C.c_float * 3)(*[float(v) for v in values])


class DevicePatchPipeline:

    def __init__(self, dataset_opt):
        self.scale = int(dataset_opt.get('scale', 4))
        self.gt_size = int(dataset_opt['gt_size'])
        mean, std = dataset_opt.get('mean'), dataset_opt.get('std')
        if (mean is None) != (std is None):   # normalize() with one side missing: identity on the other, like ImageSource
            mean = mean if mean is not None else [0.0] * 3
            std = std if std is not None else [1.0] * 3
        self._mean, self._std = _f3(mean), _f3(std)

    def _launch(self, src, origin, origin_mul, sym, patch):
        if not src.is_cuda:
            raise _lib.SrHipError('DevicePatchPipeline runs only on a HIP device (no CPU fallback)')
        if src.dtype != torch.uint8 or src.dim() != 4 or src.size(3) != 3 or not src.is_contiguous():
            raise ValueError(f'expected a contiguous uint8 [B, H, W, 3] batch, got {src.dtype} {tuple(src.shape)}')
        b, h, w, _ = src.shape
        out = torch.empty(b, 3, patch, patch, dtype=torch.float32, device=src.device)
        top = left = None
        if origin is not None:
            top, left = origin[:, 0].contiguous(), origin[:, 1].contiguous()
        lib = _lib.load()
        with torch.cuda.device(src.device):
            _lib.check(lib.sr_patch_augment_u8_f32(
                src.data_ptr(), 0, h, w, top.data_ptr() if top is not None else None, left.data_ptr() if left is not None else None,
                origin_mul, sym.data_ptr() if sym is not None else None, out.data_ptr(), b, patch, patch, 1, self._mean, self._std,
                torch.cuda.current_stream(src.device).cuda_stream), 'sr_patch_augment_u8_f32')
        return out

    def __call__(self, batch):
        if 'lq_u8' not in batch:
            return batch   # a host-augmented batch passes through
        sym = batch['sym'].to(torch.int32).contiguous()
        origin = batch.get('window')          # [B, 2] (top, left) in LQ pixels when whole images were shipped
        if origin is not None:
            origin = origin.to(torch.int32)
        out = {k: v for k, v in batch.items() if k not in ('lq_u8', 'gt_u8', 'sym', 'window')}
        out['lq'] = self._launch(batch['lq_u8'], origin, 1, sym, self.gt_size // self.scale)
        out['gt'] = self._launch(batch['gt_u8'], origin, self.scale, sym, self.gt_size)
        return out


class DeviceClipPipeline(DevicePatchPipeline):
    """The same for clips (``REDSDataset(device_augment: true | full)``): the batch holds uint8 LQ windows [B, t, h, w, 3], one uint8
    GT window [B, H, W, 3] per clip and one symmetry code (and, with ``full``, one window origin) per clip.  A clip's frames share
    its crop and its symmetry, so the LQ side is the image case on the B * t frames with each clip's code and origin repeated t
    times — a reshape, not a new kernel: sr_patch_augment_u8_f32 once on the frames, once on the GT."""

    @staticmethod
    def per_frame(sym, origin, t):
        """Host half: the per-clip symmetry codes [B] and window origins [B, 2] (or None) as per-frame arrays [B * t], [B * t, 2]."""
        sym_t = sym.to(torch.int32).repeat_interleave(t).contiguous()
        origin_t = None if origin is None else origin.to(torch.int32).repeat_interleave(t, dim=0).contiguous()
        return sym_t, origin_t

    def output_shapes(self, b, t):
        lq = self.gt_size // self.scale
        return (b, t, 3, lq, lq), (b, 3, self.gt_size, self.gt_size)

    def __call__(self, batch):
        if 'lq_u8' not in batch:
            return batch
        clips = batch['lq_u8']
        if clips.dim() != 5 or clips.size(4) != 3:
            raise ValueError(f'expected a uint8 [B, t, H, W, 3] batch of clips, got {tuple(clips.shape)}')
        b, t, h, w, _ = clips.shape
        sym = batch['sym'].to(torch.int32).contiguous()
        origin = batch.get('window')
        if origin is not None:
            origin = origin.to(torch.int32)
        sym_t, origin_t = self.per_frame(sym, origin, t)
        lq_shape, _ = self.output_shapes(b, t)
        out = {k: v for k, v in batch.items() if k not in ('lq_u8', 'gt_u8', 'sym', 'window')}
        out['lq'] = self._launch(clips.reshape(b * t, h, w, 3), origin_t, 1, sym_t, self.gt_size // self.scale).view(lq_shape)
        out['gt'] = self._launch(batch['gt_u8'], origin, self.scale, sym, self.gt_size)
        return out


class DeviceDegradePipeline:
    """The degradation chain of ``OCRDegradationDataset(device_degrade: true)`` on the batch in HBM, one HIP launch per stage
    (include/sr_hip_degrade.h), on the feed's copy stream:

      GT   sr_patch_augment_u8_f32 (flip, BGR -> RGB, / 255), then sr_degrade_finish_f32 (gray where drawn and ``gt_gray``, round,
           normalise)
      LQ   from the flipped GT: sr_filter2d_f32 with each sample's kernel, sr_resize_bilinear_f32 down to
           (int(h // s_i), int(w // s_i)) per sample (a ragged batch), sr_add_gaussian_noise_f32 (clipped, noise drawn with
           torch.randn on the device), sr_diffjpeg_f32, sr_resize_bilinear_f32 back up, sr_degrade_finish_f32 (jitter, gray, round,
           normalise).

    The JPEG stage is the reference's DiffJPEG (utils/diffjpeg.py) with the drawn quality as a float, not libjpeg through
    cv2.imencode as the reference's host chain uses: the reference itself notes that the two differ slightly (diffjpeg.py:450).
    The noise and JPEG stages are skipped when the dataset has no ``noise_range`` / ``jpeg_range``."""

    def __init__(self, dataset_opt):
        self.height, self.width = int(dataset_opt['input_height']), int(dataset_opt['input_width'])
        self.mean, self.std = dataset_opt.get('mean'), dataset_opt.get('std')
        self.noise = dataset_opt.get('noise_range') is not None
        self.jpeg = dataset_opt.get('jpeg_range') is not None
        self.jitter = dataset_opt.get('color_jitter_prob') is not None
        self.gt_gray = bool(dataset_opt.get('gt_gray'))
        self.scale_low = float(dataset_opt['downsample_range'][0])
        if self.scale_low < 1:
            raise ValueError('downsample_range must not go below 1')

    def low_sizes(self, scale, h, w):
        """int32 [B, 2] of (int(h // s_i), int(w // s_i)), at least 1 x 1, computed on the device of ``scale`` in float64 with
        Python's floor division (no host synchronisation), and the buffer size that holds every sample: the size at the low end
        of ``downsample_range``."""
        s = scale.double()
        sizes = torch.stack([torch.div(torch.full_like(s, float(h)), s, rounding_mode='floor'),
                             torch.div(torch.full_like(s, float(w)), s, rounding_mode='floor')], dim=1).clamp_(min=1).to(torch.int32)
        return sizes.contiguous(), (max(int(h // self.scale_low), 1), max(int(w // self.scale_low), 1))

    def stages(self, gt, batch, noise=None):
        """The LQ chain on the converted GT [B, 3, H, W] through the Python ops; returns every intermediate by name."""
        from ..ops import degrade as D
        h, w = gt.shape[2:]
        dev_sizes, low = self.low_sizes(batch['scale'].to(gt.device), h, w)
        out = {'blur': D.filter2D(gt, batch['kernel'].float())}
        x = out['down'] = D.resize_bilinear(out['blur'], low, dst_sizes=dev_sizes)
        if self.noise:
            if noise is None:
                noise = torch.randn(x.shape, dtype=torch.float32, device=x.device)
            x = out['noise'] = D.add_gaussian_noise_pt(x, batch['sigma'].float(), 0, True, False, noise=noise)
        if self.jpeg:
            x = out['jpeg'] = D.DiffJPEG(differentiable=False)(x, batch['quality'].float(), sizes=dev_sizes)
        out['up'] = D.resize_bilinear(x, (h, w), src_sizes=dev_sizes)
        out['lq'] = D.degrade_finish(out['up'], batch['jitter'].float() if self.jitter else None, batch['gray'].float(), self.mean, self.std)
        out['sizes'] = dev_sizes
        return out

    def __call__(self, batch, noise=None):
        if 'gt_u8' not in batch or 'kernel' not in batch:
            return batch
        src = batch['gt_u8']
        if src.dim() != 4 or tuple(src.shape[1:]) != (self.height, self.width, 3):
            raise ValueError(f'expected a uint8 [B, {self.height}, {self.width}, 3] batch, got {tuple(src.shape)}')
        from ..ops import degrade as D
        gt = self._launch_rect(src, batch['sym'].to(torch.int32).contiguous())    # converted only: both images are normalised last
        keys = ('gt_u8', 'sym', 'kernel', 'scale', 'sigma', 'quality', 'jitter', 'gray')
        out = {k: v for k, v in batch.items() if k not in keys}
        out['lq'] = self.stages(gt, batch, noise)['lq']
        out['gt'] = D.degrade_finish(gt, None, batch['gray'].float() if self.gt_gray else None, self.mean, self.std)
        return out

    def _launch_rect(self, src, sym):
        """sr_patch_augment_u8_f32 on whole [B, H, W, 3] images (no crop, flip only).  The entry point takes a symmetry code for square
        windows only; a non-square batch was flipped by the dataset and its codes are zero."""
        if not src.is_cuda:
            raise _lib.SrHipError('DeviceDegradePipeline runs only on a HIP device (no CPU fallback)')
        if src.dtype != torch.uint8 or not src.is_contiguous():
            raise ValueError(f'expected a contiguous uint8 batch, got {src.dtype}')
        b, h, w, _ = src.shape
        out = torch.empty(b, 3, h, w, dtype=torch.float32, device=src.device)
        lib = _lib.load()
        with torch.cuda.device(src.device):
            _lib.check(lib.sr_patch_augment_u8_f32(src.data_ptr(), 0, h, w, None, None, 1, sym.data_ptr() if h == w else None, out.data_ptr(), b, h, w, 1,
                                                   None, None, torch.cuda.current_stream(src.device).cuda_stream),
                       'sr_patch_augment_u8_f32')
        return out
