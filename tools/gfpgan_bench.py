#!/usr/bin/env python3
"""GFPGANv1OCR on one MI355X: the square 256^2 product configuration (num_style_feat 256, channel_multiplier 0.5, input_is_latent,
different_w, sft_half) with seeded weights and stored noise.  Prints one JSON line with
  - batch 16: images/s and the fraction of the fp32 MFMA peak at the reference's 34.64 GFLOP per image, and the FLOPs the
    launches actually execute (the encoder's blur + 3x3 / s2 runs as a 3x3 on the 4*cin-channel unshuffled source: 4x its MACs);
  - batch 1 (the service's case): the median latency of >= 20 timed forwards;
  - the per-kernel split of one batch-16 forward from the launch profiler (the launches that record themselves);
  - the same forward as a plain PyTorch-ROCm fp32 restatement on the same GPU (grouped convs as the reference runs them, the
    FIR through depthwise conv2d), batch 16 and batch 1, as the comparison.
    python tools/gfpgan_bench.py [--batch 16 --iters 20 --latency_runs 30]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
from collections import OrderedDict as OD

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import image_restoration_amd as ira  # noqa: E402
from image_restoration_amd import _lib  # noqa: E402
from image_restoration_amd.utils import synth  # noqa: E402
import gfpgan_restate as R  # noqa: E402

PEAK_TFLOPS = 157.3   # fp32 MFMA peak of one MI355X
REF_GFLOP = 34.64     # the reference's op count per 256^2 image (torch.utils.flop_counter on the CPU)
CFG = dict(input_width=256, input_height=256, num_style_feat=256, channel_multiplier=0.5, narrow=1, num_mlp=4, input_is_latent=True,
           different_w=True, sft_half=True)


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def latency(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def profile(fn, cap=8192):
    lib = _lib.load()
    _lib.check(lib.sr_profile_start(cap), 'sr_profile_start')
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        recs = (_lib.LaunchRecord * cap)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, cap, C.byref(cnt)), 'sr_profile_stop')
    return [recs[i] for i in range(min(cnt.value, cap))]


def grouped_modulated(x, style, sd, pre, demod=True, up=False):
    """The modulated conv as the reference runs it in PyTorch: per-sample weights, one grouped conv for the batch."""
    w = sd[f'{pre}.weight']
    mw, mb = sd[f'{pre}.modulation.weight'], sd[f'{pre}.modulation.bias']
    s = F.linear(style, mw * (1 / math.sqrt(mw.shape[1])), mb)
    _, co, ci, k, _ = w.shape
    n, _, h, ww = x.shape
    wn = (1 / math.sqrt(ci * k * k)) * w * s.view(n, 1, ci, 1, 1)
    if demod:
        wn = wn * torch.rsqrt(wn.pow(2).sum((2, 3, 4)) + 1e-8).view(n, co, 1, 1, 1)
    if up:
        wt = wn.transpose(1, 2).reshape(n * ci, co, k, k)
        y = F.conv_transpose2d(x.reshape(1, n * ci, h, ww), wt, stride=2, groups=n)
        return R.fir(y.view(n, co, *y.shape[2:]), 1, 1, 4.0)
    y = F.conv2d(x.reshape(1, n * ci, h, ww), wn.reshape(n * co, ci, k, k), padding=k // 2, groups=n)
    return y.view(n, co, h, ww)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--latency_runs', type=int, default=30)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    n = args.batch
    sd = synth.gfpgan_state_dict(0, **CFG)
    net = ira.build_network(dict(type='GFPGANv1OCR', **CFG))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net = net.to(dev).eval()
    x = torch.from_numpy(synth.signed_input(1, (n, 3, 256, 256))).to(dev)
    x1 = x[:1].contiguous()
    out = OD(config='256x256 nsf256 cm0.5 sft_half', batch=n)
    with torch.no_grad():
        fwd = lambda: net(x, return_rgb=False, randomize_noise=False)  # noqa: E731
        ms = timed(fwd, args.iters)
        recs = profile(fwd)
        lat = latency(lambda: net(x1, return_rgb=False, randomize_noise=False), args.latency_runs)
    out['hip_ms'] = round(ms, 3)
    out['hip_images_per_s'] = round(n / ms * 1e3, 1)
    out['hip_frac_of_fp32_peak_ref_flops'] = round(REF_GFLOP * n / ms / PEAK_TFLOPS, 4)
    exe = sum(r.flops for r in recs)
    out['executed_gflop_per_image_profiled'] = round(exe / n / 1e9, 2)
    out['hip_batch1_latency_ms_median'] = round(lat, 3)
    lib = _lib.load()
    by = OD()
    for r in recs:
        name = f'{r.kernel_id}:{lib.sr_kernel_name(r.kernel_id).decode()}'
        e = by.setdefault(name, [0, 0.0, 0.0])
        e[0] += 1
        e[1] += r.ms
        e[2] += r.flops
    tot = sum(v[1] for v in by.values())
    out['profiled_ms'] = round(tot, 3)
    out['kernels'] = {k: dict(launches=v[0], ms=round(v[1], 3), share=round(v[1] / tot, 4),
                              tflops=round(v[2] / v[1] / 1e9, 1) if v[1] > 0 and v[2] > 0 else None)
                      for k, v in sorted(by.items(), key=lambda kv: -kv[1][1])}
    # plain PyTorch-ROCm fp32 restatement on the same GPU
    R.modulated = grouped_modulated
    sdt = {k: torch.from_numpy(v).to(dev) for k, v in sd.items()}
    with torch.no_grad():
        tms = timed(lambda: R.forward(sdt, CFG, x, return_rgb=False), max(3, args.iters // 2))
        tlat = latency(lambda: R.forward(sdt, CFG, x1, return_rgb=False), args.latency_runs)
        ref = R.forward(sdt, CFG, x, return_rgb=False)['image']
        hip, _ = net(x, return_rgb=False, randomize_noise=False)
    out['torch_ms'] = round(tms, 3)
    out['torch_images_per_s'] = round(n / tms * 1e3, 1)
    out['torch_batch1_latency_ms_median'] = round(tlat, 3)
    out['speedup_batch'] = round(tms / ms, 2)
    out['speedup_batch1'] = round(tlat / lat, 2)
    out['max_abs_hip_vs_torch'] = float((hip - ref).abs().max())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
