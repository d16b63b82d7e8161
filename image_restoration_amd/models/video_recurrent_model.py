"""VideoRecurrentModel: VideoBaseModel for the networks that take a whole clip [b, n, c, h, w] and return every frame
(BasicVSR), tested from option files.

Behavioural counterpart of basicsr/models/video_recurrent_model.py:64-192: ``test()`` honours ``val.flip_seq`` (the clip and its
reversal run as one 2n-frame sequence, the two outputs of a frame are averaged) and ``val.center_frame_only``; the validation takes
one folder per ``dataset[idx]`` (strided over the ranks), scores every frame, and saves frame ``i`` as
``visualization/<dataset>/<folder>/<i:08d>_<suffix or experiment name>.png`` (with ``center_frame_only``:
``<folder>_<suffix or experiment name>.png``).  Metrics and the per-folder log are VideoBaseModel's.

``network_g.compute_dtype: bf16`` (an extension; the reference is fp32 only) runs BasicVSR / IconVSR on their bf16 forward.

Inference only: building it with ``is_train`` raises NotImplementedError — the networks' backward exists
(``BasicVSR.set_autograd``, archs/basicvsr_autograd.py, on top of ``SpyNet.set_autograd``); training them from an option file
(``fix_flow`` / ``flow_lr_mul``, the recurrent REDS dataset) is the follow-up."""
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
        if opt['is_train']:
            raise NotImplementedError('VideoRecurrentModel tests only: training the recurrent video networks from an option file '
                                      '(fix_flow / flow_lr_mul, the recurrent REDS dataset, on BasicVSR.set_autograd) is the follow-up')
        # network_g.compute_dtype of a network that sets its dtype after construction (BasicVSR, IconVSR keep the reference's
        # constructor): taken out of a copy, so build_network sees the reference's keys and the caller's dict stays as it is
        net_opt, compute_dtype = dict(opt['network_g']), None
        if 'compute_dtype' in net_opt and hasattr(ARCH_REGISTRY.get(net_opt['type']), 'set_compute_dtype'):
            compute_dtype = net_opt.pop('compute_dtype')
            opt = dict(opt, network_g=net_opt)
        super().__init__(opt)
        if compute_dtype is not None:
            self.net_g.set_compute_dtype(compute_dtype)
        self.center_frame_only = False

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
