#!/usr/bin/env python3
"""EDSR on one MI355X: Mx4 (64 features, 16 blocks) and Lx4 (256 features, 32 blocks) with seeded weights, batch 16 of 128x128,
in fp32 and bf16.  Prints one JSON line per (network, dtype) with
  - images/s and the fraction of the respective MFMA peak at the FLOPs derived from the shapes (2 * 9 * cin * cout per output
    pixel of every conv: 50,252,544 MAC per LR pixel for Lx4);
  - the per-kernel split of one forward from the launch profiler;
  - the same forward in plain PyTorch-ROCm on the same GPU (fp32 convs; for the bf16 rows the network and input cast to bf16),
    and the max-abs distance of the two outputs.
    python tools/edsr_bench.py [--batch 16 --size 128 --iters 10 --nets Mx4 Lx4 --dtypes fp32 bf16]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
from collections import OrderedDict as OD

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import image_restoration_amd as ira  # noqa: E402
from image_restoration_amd import _lib  # noqa: E402
from image_restoration_amd.utils import synth  # noqa: E402

PEAK_TFLOPS = {'fp32': 157.3, 'bf16': 2500.0}   # MFMA peaks of one MI355X (bench.py)
NETS = {
    'Mx4': dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=16, upscale=4, res_scale=1, img_range=255.,
                rgb_mean=(0.4488, 0.4371, 0.4040)),
    'Lx4': dict(num_in_ch=3, num_out_ch=3, num_feat=256, num_block=32, upscale=4, res_scale=0.1, img_range=255.,
                rgb_mean=(0.4488, 0.4371, 0.4040)),
}


def mac_per_lr_pixel(cfg):
    """Multiply-accumulates per low-resolution pixel, from the layer list."""
    nf, nb, s = cfg['num_feat'], cfg['num_block'], cfg['upscale']
    mac = 9 * 3 * nf + (2 * nb + 1) * 9 * nf * nf
    if s == 3:
        mac += 9 * nf * 9 * nf
        area = 9
    else:
        area = 1
        for _ in range(int(round(math.log2(s)))):
            mac += area * 9 * nf * 4 * nf
            area *= 4
    return mac + area * 9 * nf * 3


def timed(fn, iters, warmup=2, min_ms=500.0):
    """Mean ms per call over at least ``iters`` calls and at least ``min_ms`` of device time (a pilot run sets the count)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()

    def window(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / k
    pilot = window(2)
    return window(max(iters, int(math.ceil(min_ms / max(pilot, 1e-3)))))


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


def torch_forward(x, sd, cfg):
    """EDSR.forward in plain torch ops (the reference's layer list) in the dtype of x and sd."""
    def cv(t, name):
        return F.conv2d(t, sd[name + '.weight'], sd[name + '.bias'], padding=1)
    mean = torch.tensor(cfg['rgb_mean'], dtype=torch.float32, device=x.device).to(x.dtype).view(1, 3, 1, 1)
    first = feat = cv((x - mean) * cfg['img_range'], 'conv_first')
    for b in range(cfg['num_block']):
        feat = feat + cfg['res_scale'] * cv(torch.relu(cv(feat, f'body.{b}.conv1')), f'body.{b}.conv2')
    feat = cv(feat, 'conv_after_body') + first
    s = cfg['upscale']
    for idx, r in ([(0, 3)] if s == 3 else [(2 * k, 2) for k in range(int(round(math.log2(s))))]):
        feat = F.pixel_shuffle(cv(feat, f'upsample.{idx}'), r)
    return cv(feat, 'conv_last') / cfg['img_range'] + mean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--nets', nargs='+', default=['Mx4', 'Lx4'], choices=list(NETS))
    ap.add_argument('--dtypes', nargs='+', default=['fp32', 'bf16'], choices=['fp32', 'bf16'])
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    lib = _lib.load()
    n, hw = args.batch, args.size
    x = torch.from_numpy(synth.uniform_input(1, (n, 3, hw, hw))).to(dev)
    for name in args.nets:
        cfg = NETS[name]
        sd = synth.edsr_state_dict(0, **cfg)
        tflop = 2.0 * mac_per_lr_pixel(cfg) * n * hw * hw / 1e12
        fp32_ms = None
        for dt in args.dtypes:
            net = ira.build_network(dict(type='EDSR', compute_dtype=dt, **cfg))
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            net = net.to(dev).eval()
            out = OD(net=name, dtype=dt, batch=n, size=hw, mac_per_lr_pixel=mac_per_lr_pixel(cfg), tflop_per_batch=round(tflop, 3))
            with torch.no_grad():
                ms = timed(lambda: net(x), args.iters)
                recs = profile(lambda: net(x))
                hip = net(x)
            out['hip_ms'] = round(ms, 3)
            out['hip_images_per_s'] = round(n / ms * 1e3, 2)
            out['hip_tflops'] = round(tflop / ms * 1e3, 1)
            out['hip_frac_of_mfma_peak'] = round(tflop / ms * 1e3 / PEAK_TFLOPS[dt], 4)
            if dt == 'fp32':
                fp32_ms = ms
            elif fp32_ms:
                out['speedup_over_hip_fp32'] = round(fp32_ms / ms, 2)
            by = OD()
            for r in recs:
                key = f'{r.kernel_id}:{lib.sr_kernel_name(r.kernel_id).decode()}'
                e = by.setdefault(key, [0, 0.0, 0.0, 0.0])
                e[0] += 1
                e[1] += r.ms
                e[2] += r.flops
                e[3] += r.bytes
            tot = sum(v[1] for v in by.values())
            out['profiled_ms'] = round(tot, 3)
            out['kernels'] = {k: dict(launches=v[0], ms=round(v[1], 3), share=round(v[1] / tot, 4),
                                      tflops=round(v[2] / v[1] / 1e9, 1) if v[1] > 0 and v[2] > 0 else None,
                                      gbs=round(v[3] / v[1] / 1e6, 1) if v[1] > 0 else None)
                              for k, v in sorted(by.items(), key=lambda kv: -kv[1][1])}
            tdt = torch.float32 if dt == 'fp32' else torch.bfloat16
            sdt = {k: torch.from_numpy(v).to(dev).to(tdt) for k, v in sd.items()}
            xt = x.to(tdt)
            with torch.no_grad():
                tms = timed(lambda: torch_forward(xt, sdt, cfg), max(2, args.iters // 2))
                ref = torch_forward(xt, sdt, cfg).float()
            out['torch_ms'] = round(tms, 3)
            out['torch_images_per_s'] = round(n / tms * 1e3, 2)
            out['speedup_over_torch'] = round(tms / ms, 2)
            out['max_abs_hip_vs_torch'] = float((hip - ref).abs().max())
            print(json.dumps(out), flush=True)
            del net, sdt, ref, hip
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
