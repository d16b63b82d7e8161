#!/usr/bin/env python3
"""MSRResNet timings on one GPU; prints one JSON line.

    python tools/msrresnet_bench.py [--steps 20 --warmup 5] [--only forward,plate,train] [--compute_dtype fp32|bf16] [--torch]

* forward: x4, nf 64, nb 16, batch 16 of 128x128 fp32 (BASELINE config 1's shape): images/s from device events after
  warm-up, and the share of the fp32 MFMA peak from 83.1 GFLOP per image (counted from shapes);
* plate: one 64x64 crop, x4: latency per forward;
* train: one SRModel step (L1, Adam), batch 16 of 32x32 -> 128x128 (the reference's train_MSRResNet_x4.yml sizes).
--compute_dtype bf16 runs forward and plate on the bf16 path (train stays fp32); the share is then of the bf16 MFMA peak.
--torch adds the same forward in plain PyTorch-ROCm on the same GPU in the same dtype (network and input cast to bf16 for bf16)
and the max-abs distance of the two outputs.
Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run of ``--only forward``.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_restoration_amd as ira  # noqa: E402

GFLOP_PER_IMAGE = 83.1        # x4, nf 64, nb 16, 128x128 input
FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X dense fp32 matrix peak
BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X dense bf16 matrix peak (bench.py)


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


def torch_forward(x, sd, num_block=16):
    """MSRResNet.forward (x4) in plain torch ops (the reference's layer list) in the dtype of x and sd."""
    def cv(t, name):
        return F.conv2d(t, sd[name + '.weight'], sd[name + '.bias'], padding=1)
    feat = F.leaky_relu(cv(x, 'conv_first'), 0.1)
    for b in range(num_block):
        feat = feat + cv(torch.relu(cv(feat, f'body.{b}.conv1')), f'body.{b}.conv2')
    for name in ('upconv1', 'upconv2'):
        feat = F.leaky_relu(F.pixel_shuffle(cv(feat, name), 2), 0.1)
    out = cv(F.leaky_relu(cv(feat, 'conv_hr'), 0.1), 'conv_last')
    return out + F.interpolate(x, scale_factor=4, mode='bilinear', align_corners=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--only', default='forward,plate,train')
    ap.add_argument('--compute_dtype', default='fp32', choices=['fp32', 'bf16'])
    ap.add_argument('--torch', action='store_true', help='also time the forward in plain PyTorch-ROCm in the same dtype')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    out = {'device': torch.cuda.get_device_name(0), 'compute_dtype': args.compute_dtype}
    which = args.only.split(',')
    bf16 = args.compute_dtype == 'bf16'
    peak = BF16_MFMA_PEAK_TFLOPS if bf16 else FP32_MFMA_PEAK_TFLOPS
    net = ira.build_network(dict(type='MSRResNet', upscale=4, **(dict(compute_dtype='bf16') if bf16 else {}))).to(dev).eval()
    if 'forward' in which:
        x = torch.rand(16, 3, 128, 128, device=dev)
        with torch.no_grad():
            ms = timed(lambda: net(x), args.steps, args.warmup)
        ips = 16 / (ms / 1e3)
        out['forward_b16_128_ms'] = round(ms, 3)
        out['forward_images_per_s'] = round(ips, 1)
        out['forward_tflops'] = round(ips * GFLOP_PER_IMAGE / 1e3, 1)
        out[f'forward_share_of_{args.compute_dtype}_mfma_peak'] = round(ips * GFLOP_PER_IMAGE / 1e3 / peak, 3)
        if args.torch:
            tdt = torch.bfloat16 if bf16 else torch.float32
            sdt = {k: v.detach().to(tdt) for k, v in net.state_dict().items()}
            xt = x.to(tdt)
            with torch.no_grad():
                tms = timed(lambda: torch_forward(xt, sdt), max(2, args.steps // 2), 2)
                out['max_abs_hip_vs_torch'] = float((net(x) - torch_forward(xt, sdt).float()).abs().max())
            out['torch_forward_b16_128_ms'] = round(tms, 3)
            out['speedup_over_torch'] = round(tms / ms, 2)
            del sdt
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
