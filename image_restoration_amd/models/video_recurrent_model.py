"""VideoRecurrentModel: VideoBaseModel for the networks that take a whole clip [b, n, c, h, w] and return every frame
(BasicVSR), tested from option files.

Behavioural counterpart of basicsr/models/video_recurrent_model.py:64-192: ``test()`` honours ``val.flip_seq`` (the clip and its
reversal run as one 2n-frame sequence, the two outputs of a frame are averaged) and ``val.center_frame_only``; the validation takes
one folder per ``dataset[idx]`` (strided over the ranks), scores every frame, and saves frame ``i`` as
``visualization/<dataset>/<folder>/<i:08d>_<suffix or experiment name>.png`` (with ``center_frame_only``:
``<folder>_<suffix or experiment name>.png``).  Metrics and the per-folder log are VideoBaseModel's.

``network_g.compute_dtype: bf16`` (an extension; the reference is fp32 only) runs BasicVSR / IconVSR on their bf16 forward.

Training (``is_train``; the reference's video_recurrent_model.py:17-62) runs BasicVSR in fp32 on a HIP device, on
``BasicVSR.set_autograd(True, deterministic=train.deterministic_backward)``:

``train.flow_lr_mul``  the parameters whose name contains ``spynet`` form a second Adam parameter group at ``lr * flow_lr_mul``
    (normal parameters first, as in the reference).  1 (the default) is one group.  Both groups step in ONE launch
    (sr_adam_step_groups_f32), as EDVRModel's.
``train.fix_flow``     below iteration ``fix_flow`` the parameters whose name contains ``spynet`` or ``edvr`` do not train; from
    iteration ``fix_flow`` on all of them.  While they are frozen the network computes no flow gradient and SpyNet's backward is
    not walked.
``train.deterministic_backward``  (an extension, default true) the step-input adjoint of the recurrent backward sums in 64-bit
    integers (include/sr_hip_vsr_det.h), so two runs from one seed take bit-identical steps and a resumed run continues the
    uninterrupted one's trajectory bit for bit; false selects the float-atomic scatter, which is neither.

The loss is taken on the whole output [b, n, 3, 4h, 4w] against ``gt`` of the same shape.  Validation inside training is
``dist_validation`` below; saving images while training raises, as in the reference.

Deviation, the one of EDVRModel: the reference freezes at ``current_iter == 1`` only, so a run resumed inside the warm-up trains
everything from there; here the freeze holds for every iteration below ``fix_flow``, resumed or not.

Not trained yet — NotImplementedError at construction, naming what is supported: a model on the CPU (``num_gpu: 0``), IconVSR
(the backward of its keyframe branch), ``compute_dtype: bf16``; Vimeo-90K recurrent clips have no dataset.  They are the
follow-up."""
import os
import os.path as osp
from collections import Counter, OrderedDict

import torch

from .. import watchdog
from ..utils.registry import ARCH_REGISTRY, MODEL_REGISTRY
from .video_base_model import VideoBaseModel


@MODEL_REGISTRY.register()
class VideoRecurrentModel(VideoBaseModel):

    def __init__(self, opt):
        self.fix_flow_iter = None
        self._flow_frozen = False
        if opt['is_train']:
            supported = 'supported: network_g.type BasicVSR in fp32 (no compute_dtype, or fp32) on a HIP device (num_gpu >= 1)'
            if opt['num_gpu'] == 0:
                raise NotImplementedError('VideoRecurrentModel trains on a HIP device only (num_gpu: 0 has no kernels to run); '
                                          f'{supported}.  IconVSR, bf16 and Vimeo-90K training are the follow-up')
            if opt['network_g'].get('type') != 'BasicVSR':
                raise NotImplementedError(f"VideoRecurrentModel cannot train network_g.type {opt['network_g'].get('type')!r}; "
                                          f'{supported}.  IconVSR training is the follow-up')
            if opt['network_g'].get('compute_dtype', 'fp32') != 'fp32':
                raise NotImplementedError(f"VideoRecurrentModel cannot train with compute_dtype {opt['network_g']['compute_dtype']!r}; "
                                          f'{supported}.  bf16 training is the follow-up')
            self.fix_flow_iter = opt['train'].get('fix_flow')
        # network_g.compute_dtype of a network that sets its dtype after construction (BasicVSR, IconVSR keep the reference's
        # constructor): taken out of a copy, so build_network sees the reference's keys and the caller's dict stays as it is
        net_opt, compute_dtype = dict(opt['network_g']), None
        if 'compute_dtype' in net_opt and hasattr(ARCH_REGISTRY.get(net_opt['type']), 'set_compute_dtype'):
            compute_dtype = net_opt.pop('compute_dtype')
            opt = dict(opt, network_g=net_opt)
        super().__init__(opt)
        if compute_dtype is not None:
            self.net_g.set_compute_dtype(compute_dtype)
        if self.is_train:   # the EMA shadow (built in init_training_settings) only ever runs under no_grad: it keeps the switch off
            self.net_g.set_autograd(True, deterministic=self.opt['train'].get('deterministic_backward', True))
        self.center_frame_only = False

    def setup_optimizers(self):
        train_opt = self.opt['train']
        flow_lr_mul = train_opt.get('flow_lr_mul', 1)
        self.logger.info(f'Multiple the learning rate for flow network with {flow_lr_mul}.')
        block = dict(train_opt['optim_g'])
        kind = block.pop('type')
        if kind != 'Adam':
            raise NotImplementedError(f'optimizer {kind} is not supperted yet.')
        if flow_lr_mul == 1:
            self.optimizer_g = self.gen.attach_adam(block, self.logger)
        else:   # normal parameters first, then the flow network at its own rate
            self.optimizer_g = self.gen.attach_adam(block, self.logger, group_of=lambda name: 1 if 'spynet' in name else 0,
                                                    group_lrs=[block['lr'], block['lr'] * flow_lr_mul])

    def optimize_parameters(self, current_iter):
        if self.fix_flow_iter:
            if current_iter < self.fix_flow_iter and not self._flow_frozen:
                self.logger.info(f'Fix flow network and feature extractor for {self.fix_flow_iter} iters.')
                for name, param in self.net_g.named_parameters():
                    if 'spynet' in name or 'edvr' in name:
                        param.requires_grad_(False)
                self._flow_frozen = True
            elif current_iter >= self.fix_flow_iter and self._flow_frozen:
                self.logger.warning('Train all the parameters.')
                self.net_g.requires_grad_(True)
                self._flow_frozen = False
        super().optimize_parameters(current_iter)

    def test(self):
        """One forward over the clip ``self.lq`` [b, n, c, h, w] without autograd."""
        val_opt = self.opt.get('val') or {}
        flip_seq = val_opt.get('flip_seq', False)
        self.center_frame_only = val_opt.get('center_frame_only', False)
        n = self.lq.size(1)
        lq = torch.cat([self.lq, self.lq.flip(1)], dim=1) if flip_seq else self.lq
        self.net_g.eval()
        with torch.no_grad():
            out = watchdog.guarded(lambda: self.net_g(lq), 'VideoRecurrentModel.test') if lq.is_cuda else self.net_g(lq)
            if flip_seq:
                out = 0.5 * (out[:, :n] + out[:, n:].flip(1))
            if self.center_frame_only:
                out = out[:, n // 2]
        self.output = out
        self.net_g.train()

    def dist_validation(self, dataloader, current_iter, tb_logger=None, save_img=False):
        from ..metrics import psnr_device, ssim_device
        from ..utils.img_util import tensor2img
        from ..utils.registry import METRIC_REGISTRY
        dataset = dataloader.dataset
        dataset_name = dataset.opt['name']
        val_opt = self.opt.get('val') or {}
        metrics = val_opt.get('metrics')
        if save_img and self.opt['is_train']:
            raise NotImplementedError('saving image is not supported during training.')
        center = val_opt.get('center_frame_only', False)
        if metrics is not None:
            self.metric_results = OrderedDict(
                (folder, torch.zeros(1 if center else frames, len(metrics), dtype=torch.float32, device=self.device))
                for folder, frames in Counter(dataset.data_info['folder']).items())
        rank, world = (self.opt['rank'], self.opt['world_size']) if self.distributed else (0, 1)
        for idx in range(rank, len(dataset), world):
            val_data = dataset[idx]
            folder = val_data['folder']
            self.feed_data(dict(lq=val_data['lq'].unsqueeze(0), gt=val_data['gt'].unsqueeze(0)))
            self.test()
            out, gt = self.output.detach(), self.gt
            if self.center_frame_only:
                out, gt = out.unsqueeze(1), gt[:, gt.size(1) // 2].unsqueeze(1)
            for i in range(out.size(1)):
                frame, frame_gt = out[:, i], gt[:, i]
                if save_img:
                    import numpy as np
                    from PIL import Image
                    name = folder if self.center_frame_only else f'{i:08d}'
                    path = osp.join(self.opt['path']['visualization'], dataset_name, folder,
                                    f'{name}_{val_opt.get("suffix") or self.opt["name"]}.png')
                    os.makedirs(osp.dirname(path), exist_ok=True)
                    Image.fromarray(np.ascontiguousarray(tensor2img([frame.cpu()], rgb2bgr=False))).save(path)
                if metrics is not None:
                    for m_idx, mopt in enumerate(metrics.values()):
                        mopt = dict(mopt)
                        mtype = mopt.pop('type')
                        if mtype in ('calculate_psnr', 'calculate_ssim') and not mopt.get('test_y_channel', False):
                            fn = psnr_device if mtype == 'calculate_psnr' else ssim_device
                            value = fn(frame.contiguous(), frame_gt.contiguous(), mopt.get('crop_border', 0))[0]
                        else:
                            value = METRIC_REGISTRY.get(mtype)(tensor2img([frame.cpu()]), tensor2img([frame_gt.cpu()]), **mopt)
                        self.metric_results[folder][i, m_idx] += float(value)
            del self.lq, self.output, self.gt
        if metrics is not None:
            if self.distributed:
                for tensor in self.metric_results.values():
                    torch.distributed.reduce(tensor, 0)
                torch.distributed.barrier()
            if rank == 0:
                self._log_validation_metric_values(current_iter, dataset_name, tb_logger)
