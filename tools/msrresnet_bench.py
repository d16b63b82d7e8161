#!/usr/bin/env python3
"""MSRResNet timings on one GPU; prints one JSON line.

    python tools/msrresnet_bench.py [--steps 20 --warmup 5] [--only forward,plate,train]

* forward: x4, nf 64, nb 16, batch 16 of 128x128 fp32 (BASELINE config 1's shape): images/s from device events after
  warm-up, and the share of the fp32 MFMA peak from 83.1 GFLOP per image (counted from shapes);
* plate: one 64x64 crop, x4: latency per forward;
* train: one SRModel step (L1, Adam), batch 16 of 32x32 -> 128x128 (the reference's train_MSRResNet_x4.yml sizes).
Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run of ``--only forward``.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_restoration_amd as ira  # noqa: E402

GFLOP_PER_IMAGE = 83.1        # x4, nf 64, nb 16, 128x128 input
FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X dense fp32 matrix peak


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--only', default='forward,plate,train')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    out = {'device': torch.cuda.get_device_name(0)}
    which = args.only.split(',')
    net = ira.build_network(dict(type='MSRResNet', upscale=4)).to(dev).eval()
    if 'forward' in which:
        x = torch.rand(16, 3, 128, 128, device=dev)
        with torch.no_grad():
            ms = timed(lambda: net(x), args.steps, args.warmup)
        ips = 16 / (ms / 1e3)
        out['forward_b16_128_ms'] = round(ms, 3)
        out['forward_images_per_s'] = round(ips, 1)
        out['forward_tflops'] = round(ips * GFLOP_PER_IMAGE / 1e3, 1)
        out['forward_share_of_fp32_mfma_peak'] = round(ips * GFLOP_PER_IMAGE / 1e3 / FP32_MFMA_PEAK_TFLOPS, 3)
    if 'plate' in which:
        x = torch.rand(1, 3, 64, 64, device=dev)
        with torch.no_grad():
            out['plate_64_latency_ms'] = round(timed(lambda: net(x), args.steps, args.warmup), 3)
    if 'train' in which:
        from image_restoration_amd.models import build_model
        opt = dict(name='bench', model_type='SRModel', scale=4, num_gpu=1, dist=False, rank=0, world_size=1, is_train=True,
                   network_g=dict(type='MSRResNet', upscale=4), path=dict(pretrain_network_g=None, strict_load_g=True),
                   train=dict(optim_g=dict(type='Adam', lr=2e-4, weight_decay=0, betas=[0.9, 0.99]),
                              scheduler=dict(type='MultiStepLR', milestones=[10 ** 9], gamma=0.5), total_iter=10 ** 9,
                              warmup_iter=-1, pixel_opt=dict(type='L1Loss', loss_weight=1.0, reduction='mean')))
        model = build_model(opt)
        lq, gt = torch.rand(16, 3, 32, 32, device=dev), torch.rand(16, 3, 128, 128, device=dev)
        it = [0]

        def step():
            it[0] += 1
            model.feed_data({'lq': lq, 'gt': gt})
            model.optimize_parameters(it[0])
        out['train_step_b16_32to128_ms'] = round(timed(step, args.steps, args.warmup), 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
