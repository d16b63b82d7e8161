"""VideoBaseModel: SRModel whose validation walks a video test set frame by frame and reports per folder.

Behavioural counterpart of basicsr/models/video_base_model.py:14-146 (``dist_validation``, which the reference also runs without
a launcher): ``dataset[idx]`` once per centre frame, strided over the ranks; ``metric_results[folder]`` is a
[frames x metrics] tensor on the device, reduced to rank 0 under data parallelism; the log shows, per metric, the average over
the folders of each folder's average over its frames, then every folder's own.  The image name is the centre frame's file stem
(for a dataset whose name contains ``vimeo``: ``<grandparent>_<parent>_<stem>``), saved under
``visualization/<dataset>/<folder>/<name>_<suffix or experiment name>.png``; saving during training is the reference's
NotImplementedError.

PSNR / SSIM without ``test_y_channel`` are reduced on the device from the fp32 output (metrics/psnr.py: tensor2img's
quantisation, no device -> host image copy); any other metric option takes the host route through tensor2img, as in SRModel.
The forward runs through ``SRModel.test``, i.e. inside ``watchdog.guarded``."""
import os.path as osp
from collections import Counter, OrderedDict

import torch

from ..utils.registry import MODEL_REGISTRY
from .sr_model import SRModel


@MODEL_REGISTRY.register()
class VideoBaseModel(SRModel):

    def validation(self, dataloader, current_iter, tb_logger=None, save_img=False):
        """Every rank takes part (the frames are strided over the ranks), unlike SRModel's rank-0 validation."""
        self.dist_validation(dataloader, current_iter, tb_logger, save_img)

    def nondist_validation(self, dataloader, current_iter, tb_logger=None, save_img=False):
        self.logger.warning('nondist_validation is not implemented. Run dist_validation.')
        self.dist_validation(dataloader, current_iter, tb_logger, save_img)

    @staticmethod
    def image_name(dataset_name, lq_path):
        if 'vimeo' in dataset_name.lower():
            parts = lq_path.split('/')
            return f'{parts[-3]}_{parts[-2]}_{parts[-1].split(".")[0]}'
        return osp.splitext(osp.basename(lq_path))[0]

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
        if metrics is not None:
            self.metric_results = OrderedDict(
                (folder, torch.zeros(frames, len(metrics), dtype=torch.float32, device=self.device))
                for folder, frames in Counter(dataset.data_info['folder']).items())
        rank, world = (self.opt['rank'], self.opt['world_size']) if self.distributed else (0, 1)
        for idx in range(rank, len(dataset), world):
            val_data = dataset[idx]
            folder, frame_idx = val_data['folder'], int(val_data['idx'].split('/')[0])
            self.feed_data(dict(lq=val_data['lq'].unsqueeze(0), gt=val_data['gt'].unsqueeze(0)))
            self.test()
            out, gt = self.output.detach(), self.gt
            if save_img:
                import os
                import numpy as np
                from PIL import Image
                name = self.image_name(dataset_name, val_data['lq_path'])
                path = osp.join(self.opt['path']['visualization'], dataset_name, folder,
                                f'{name}_{val_opt.get("suffix") or self.opt["name"]}.png')
                os.makedirs(osp.dirname(path), exist_ok=True)
                Image.fromarray(np.ascontiguousarray(tensor2img([out[0:1].cpu()], rgb2bgr=False))).save(path)
            if metrics is not None:
                for m_idx, mopt in enumerate(metrics.values()):
                    mopt = dict(mopt)
                    mtype = mopt.pop('type')
                    if mtype in ('calculate_psnr', 'calculate_ssim') and not mopt.get('test_y_channel', False):
                        fn = psnr_device if mtype == 'calculate_psnr' else ssim_device
                        value = fn(out[0:1], gt[0:1], mopt.get('crop_border', 0))[0]
                    else:
                        value = METRIC_REGISTRY.get(mtype)(tensor2img([out[0:1].cpu()]), tensor2img([gt[0:1].cpu()]), **mopt)
                    self.metric_results[folder][frame_idx, m_idx] += float(value)
            del self.lq, self.output, self.gt
        if metrics is not None:
            if self.distributed:
                for tensor in self.metric_results.values():
                    torch.distributed.reduce(tensor, 0)
                torch.distributed.barrier()
            if rank == 0:
                self._log_validation_metric_values(current_iter, dataset_name, tb_logger)

    def _log_validation_metric_values(self, current_iter, dataset_name, tb_logger):
        names = list(self.opt['val']['metrics'].keys())
        per_folder = OrderedDict((folder, tensor.mean(dim=0).cpu()) for folder, tensor in self.metric_results.items())
        total = OrderedDict((m, sum(avg[i].item() for avg in per_folder.values()) / len(per_folder)) for i, m in enumerate(names))
        self.validation_summary = dict(total=total, folders=OrderedDict((f, {m: avg[i].item() for i, m in enumerate(names)})
                                                                        for f, avg in per_folder.items()))
        log = f'Validation {dataset_name}\n'
        for i, (m, value) in enumerate(total.items()):
            log += f'\t # {m}: {value:.4f}' + ''.join(f'\t # {f}: {avg[i].item():.4f}' for f, avg in per_folder.items()) + '\n'
        self.logger.info(log)
        if tb_logger:
            for i, (m, value) in enumerate(total.items()):
                tb_logger.add_scalar(f'metrics/{m}', value, current_iter)
                for f, avg in per_folder.items():
                    tb_logger.add_scalar(f'metrics/{m}/{f}', avg[i].item(), current_iter)
