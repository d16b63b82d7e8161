#!/usr/bin/env python3
"""Times the device degradation chain (include/sr_hip_degrade.h) stage by stage and as a whole at B = 16, 256 x 256, and the same
chain written with torch ops on the same device: grouped F.conv2d after a reflect pad, F.interpolate, and the fp32 restatement of
DiffJPEG (tests/degrade_restate.py).

    python tools/degrade_bench.py [--batch 16] [--size 256] [--iters 50] [--warmup 10]

Prints one JSON line: microseconds per stage and the bytes each HIP stage has to move per microsecond (inputs read once + outputs
written once; DESIGN.md section 7 measured 6.29 TB/s = 6.29 MB/us for a copy).  The torch chain downsamples every sample to the
same size (F.interpolate has no ragged batches); the HIP chain is timed at that same uniform size, through the ragged interface.
"""
import argparse
import json
import os
import sys

import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import degrade_restate as R  # noqa: E402
from image_restoration_amd.ops import degrade as D  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1000.0 / iters      # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--scale', type=float, default=4.0)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    b, s = args.batch, args.size
    low = int(s // args.scale)
    g = torch.Generator().manual_seed(0)
    gt = torch.rand((b, 3, s, s), generator=g).to(dev)
    kern = torch.rand((b, 21, 21), generator=g)
    kern = (kern / kern.sum(dim=(1, 2), keepdim=True)).to(dev)
    sizes = torch.tensor([[low, low]] * b, dtype=torch.int32, device=dev)
    noise = torch.randn((b, 3, low, low), generator=g).to(dev)
    sigma = (torch.rand(b, generator=g) * 20).to(dev)
    quality = (30 + torch.rand(b, generator=g) * 70).to(dev)
    jitter = ((torch.rand((b, 3), generator=g) - 0.5) * 40 / 255).to(dev)
    gray = torch.zeros(b, device=dev)
    mean = std = [0.5, 0.5, 0.5]
    jpeg = D.DiffJPEG(differentiable=False)
    factor = D.quality_to_factor(quality)

    blur = D.filter2D(gt, kern)
    down = D.resize_bilinear(blur, (low, low), dst_sizes=sizes)
    noisy = D.add_gaussian_noise_pt(down, sigma, 0, True, False, noise=noise)
    comp = jpeg(noisy, quality, sizes=sizes)
    up = D.resize_bilinear(comp, (s, s), src_sizes=sizes)

    def hip_chain():
        x = D.filter2D(gt, kern)
        x = D.resize_bilinear(x, (low, low), dst_sizes=sizes)
        x = D.add_gaussian_noise_pt(x, sigma, 0, True, False, noise=noise)
        x = jpeg(x, quality, sizes=sizes)
        x = D.resize_bilinear(x, (s, s), src_sizes=sizes)
        return D.degrade_finish(x, jitter, gray, mean, std)

    def torch_blur(x):
        xp = F.pad(x, (10, 10, 10, 10), mode='reflect')
        w = kern.view(b, 1, 21, 21).repeat_interleave(3, dim=0)
        return F.conv2d(xp.view(1, b * 3, s + 20, s + 20), w, groups=b * 3).view(b, 3, s, s)

    def torch_noise(x):
        return torch.clamp(x + noise * sigma.view(b, 1, 1, 1) / 255., 0, 1)

    def torch_finish(x):
        x = torch.clamp(x + jitter.view(b, 3, 1, 1), 0, 1)
        x = torch.clamp((x * 255.0).round(), 0, 255) / 255.
        return (x - 0.5) / 0.5

    def torch_chain():
        x = torch_blur(gt)
        x = F.interpolate(x, size=(low, low), mode='bilinear', align_corners=False)
        x = torch_noise(x)
        x = R.diffjpeg(x, factor, False)[0]
        x = F.interpolate(x, size=(s, s), mode='bilinear', align_corners=False)
        return torch_finish(x)

    big, small = 4.0 * b * 3 * s * s, 4.0 * b * 3 * low * low
    stages = {   # name: (hip, torch, bytes the HIP stage must move)
        'filter2d_k21': (lambda: D.filter2D(gt, kern), lambda: torch_blur(gt), 2 * big),
        'resize_down': (lambda: D.resize_bilinear(blur, (low, low), dst_sizes=sizes),
                        lambda: F.interpolate(blur, size=(low, low), mode='bilinear', align_corners=False), big + small),
        'noise': (lambda: D.add_gaussian_noise_pt(down, sigma, 0, True, False, noise=noise), lambda: torch_noise(down), 3 * small),
        'diffjpeg': (lambda: jpeg(noisy, quality, sizes=sizes), lambda: R.diffjpeg(noisy, factor, False)[0], 2 * small),
        'resize_up': (lambda: D.resize_bilinear(comp, (s, s), src_sizes=sizes),
                      lambda: F.interpolate(comp, size=(s, s), mode='bilinear', align_corners=False), big + small),
        'finish': (lambda: D.degrade_finish(up, jitter, gray, mean, std), lambda: torch_finish(up), 2 * big),
        'chain': (hip_chain, torch_chain, 6 * big + 8 * small),
    }
    result = {'batch': b, 'size': s, 'low': low, 'device': torch.cuda.get_device_name(0), 'stages': {}}
    with torch.no_grad():
        for name, (hip, ref, nbytes) in stages.items():
            t_hip, t_ref = timed(hip, args.iters, args.warmup), timed(ref, args.iters, args.warmup)
            result['stages'][name] = {'hip_us': round(t_hip, 2), 'torch_us': round(t_ref, 2), 'hip_bytes_per_us': round(nbytes / t_hip, 1),
                                      'bytes': nbytes}
    print(json.dumps(result))


if __name__ == '__main__':
    main()
