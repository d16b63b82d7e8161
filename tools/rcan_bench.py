#!/usr/bin/env python3
"""RCAN timings on one GPU; prints one JSON line.

    python tools/rcan_bench.py [--steps 10 --warmup 3] [--only forward,crop,train] [--compute_dtype fp32|bf16] [--torch]

* forward: the option files' net (x4, nf 64, 10 groups x 20 blocks, sf 16), batch 16 of 128x128 fp32: images/s from device
  events after warm-up, the share of the fp32 MFMA peak from 521.6 GFLOP per image (counted from shapes), and the share of the
  launch-profiler time spent in the channel-attention kernels (ids 74-76);
* crop: one 64x64 crop, x4: latency per forward (about 1,000 launches, launch-bound);
* train: one SRModel step (L1, Adam) of the x2 net, batch 16 of 48x48 LR patches.
--compute_dtype bf16 runs forward and crop on the bf16 path (train stays fp32): the share is then of the bf16 MFMA peak, the
attention kernels are ids 102-104, and every kernel's share of the profiled time is listed.  --torch adds the same forward in
plain PyTorch-ROCm on the same GPU in the same dtype (network and input cast to bf16 for bf16) and the max-abs distance.
Kernel times come from separate ``rocprofv3 --kernel-trace --stats`` runs of each ``--only`` item.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_restoration_amd as ira  # noqa: E402
from image_restoration_amd import _lib  # noqa: E402

GFLOP_PER_IMAGE = 521.6        # x4 yml net, 128x128 input
FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X dense fp32 matrix peak
BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X dense bf16 matrix peak (bench.py)
NET = dict(type='RCAN', num_in_ch=3, num_out_ch=3, num_feat=64, num_group=10, num_block=20, squeeze_factor=16)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def profile_split(fn, cap=8192):
    """Launch-profiler time per kernel id over one call of fn: (total ms, {id: (ms, bytes)})."""
    lib = _lib.load()
    _lib.check(lib.sr_profile_start(cap), 'sr_profile_start')
    try:
        fn()
    finally:
        recs = (_lib.LaunchRecord * cap)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, cap, C.byref(cnt)), 'sr_profile_stop')
    per = {}
    for i in range(min(cnt.value, cap)):
        ms, by = per.get(recs[i].kernel_id, (0.0, 0.0))
        per[recs[i].kernel_id] = (ms + recs[i].ms, by + recs[i].bytes)
    return sum(v[0] for v in per.values()), per, cnt.value


def torch_forward(x, sd, cfg):
    """RCAN.forward in plain torch ops (the reference's layer list) in the dtype of x and sd."""
    def cv(t, name):
        return F.conv2d(t, sd[name + '.weight'], sd[name + '.bias'], padding=1)
    mean = torch.tensor((0.4488, 0.4371, 0.4040), dtype=torch.float32, device=x.device).to(x.dtype).view(1, 3, 1, 1)
    x0 = feat = cv((x - mean) * 255., 'conv_first')
    for g in range(cfg['num_group']):
        g_in = feat
        for b in range(cfg['num_block']):
            pre = f'body.{g}.residual_group.{b}.rcab.'
            u = cv(torch.relu(cv(feat, pre + '0')), pre + '2')
            hid = torch.relu(F.conv2d(u.mean((2, 3), keepdim=True), sd[pre + '3.attention.1.weight'], sd[pre + '3.attention.1.bias']))
            feat = feat + u * torch.sigmoid(F.conv2d(hid, sd[pre + '3.attention.3.weight'], sd[pre + '3.attention.3.bias']))
        feat = cv(feat, f'body.{g}.conv') + g_in
    feat = cv(feat, 'conv_after_body') + x0
    for k in range(2):
        feat = F.pixel_shuffle(cv(feat, f'upsample.{2 * k}'), 2)
    return cv(feat, 'conv_last') / 255. + mean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default='forward,crop,train')
    ap.add_argument('--compute_dtype', default='fp32', choices=['fp32', 'bf16'])
    ap.add_argument('--torch', action='store_true', help='also time the forward in plain PyTorch-ROCm in the same dtype')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    out = {'device': torch.cuda.get_device_name(0), 'compute_dtype': args.compute_dtype}
    which = args.only.split(',')
    bf16 = args.compute_dtype == 'bf16'
    peak = BF16_MFMA_PEAK_TFLOPS if bf16 else FP32_MFMA_PEAK_TFLOPS
    ca_ids = (102, 104) if bf16 else (74, 76)
    if 'forward' in which or 'crop' in which:
        net = ira.build_network(dict(NET, upscale=4, **(dict(compute_dtype='bf16') if bf16 else {}))).to(dev).eval()
    if 'forward' in which:
        x = torch.rand(16, 3, 128, 128, device=dev)
        with torch.no_grad():
            ms = timed(lambda: net(x), args.steps, args.warmup)
            tot, per, n = profile_split(lambda: net(x))
        ips = 16 / (ms / 1e3)
        out['forward_b16_128_ms'] = round(ms, 2)
        out['forward_images_per_s'] = round(ips, 1)
        out['forward_tflops'] = round(ips * GFLOP_PER_IMAGE / 1e3, 1)
        out[f'forward_share_of_{args.compute_dtype}_mfma_peak'] = round(ips * GFLOP_PER_IMAGE / 1e3 / peak, 3)
        out['forward_launches'] = n
        out['forward_profiled_ms'] = round(tot, 2)
        ca = {k: v for k, v in per.items() if ca_ids[0] <= k <= ca_ids[1]}
        out['forward_ca_ms'] = {str(k): round(v[0], 3) for k, v in sorted(ca.items())}
        out['forward_ca_tb_per_s'] = {str(k): round(v[1] / (v[0] * 1e-3) / 1e12, 2) for k, v in sorted(ca.items()) if v[0] > 0}
        out['forward_ca_share'] = round(sum(v[0] for v in ca.values()) / tot, 4)
        if bf16:
            lib = _lib.load()
            out['forward_kernel_share'] = {f'{k}:{lib.sr_kernel_name(k).decode()}': round(v[0] / tot, 4)
                                           for k, v in sorted(per.items(), key=lambda kv: -kv[1][0])}
        if args.torch:
            tdt = torch.bfloat16 if bf16 else torch.float32
            sdt = {k: v.detach().to(tdt) for k, v in net.state_dict().items()}
            xt = x.to(tdt)
            with torch.no_grad():
                tms = timed(lambda: torch_forward(xt, sdt, NET), max(2, args.steps // 2), 2)
                out['max_abs_hip_vs_torch'] = float((net(x) - torch_forward(xt, sdt, NET).float()).abs().max())
            out['torch_forward_b16_128_ms'] = round(tms, 2)
            out['speedup_over_torch'] = round(tms / ms, 2)
            del sdt
    if 'crop' in which:
        x = torch.rand(1, 3, 64, 64, device=dev)
        with torch.no_grad():
            out['crop_64_latency_ms'] = round(timed(lambda: net(x), args.steps, args.warmup), 3)
    if 'train' in which:
        from image_restoration_amd.models import build_model
        opt = dict(name='bench', model_type='SRModel', scale=2, num_gpu=1, dist=False, rank=0, world_size=1, is_train=True,
                   network_g=dict(NET, upscale=2), path=dict(pretrain_network_g=None, strict_load_g=True),
                   train=dict(optim_g=dict(type='Adam', lr=1e-4, weight_decay=0, betas=[0.9, 0.99]),
                              scheduler=dict(type='MultiStepLR', milestones=[10 ** 9], gamma=0.5), total_iter=10 ** 9,
                              warmup_iter=-1, pixel_opt=dict(type='L1Loss', loss_weight=1.0, reduction='mean')))
        model = build_model(opt)
        lq, gt = torch.rand(16, 3, 48, 48, device=dev), torch.rand(16, 3, 96, 96, device=dev)
        it = [0]

        def step():
            it[0] += 1
            model.feed_data({'lq': lq, 'gt': gt})
            model.optimize_parameters(it[0])
        out['train_step_b16_48to96_ms'] = round(timed(step, args.steps, args.warmup), 2)
        tot, per, n = profile_split(step)
        ca = {k: v for k, v in per.items() if 74 <= k <= 80}
        out['train_step_launches'] = n
        out['train_step_ca_ms'] = {str(k): round(v[0], 3) for k, v in sorted(ca.items())}
        out['train_step_ca_share'] = round(sum(v[0] for v in ca.values()) / tot, 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
