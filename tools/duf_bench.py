#!/usr/bin/env python3
"""Times DUF inference (archs/duf_arch.py) on one GPU, in the manner of tools/tof_bench.py.

    python tools/duf_bench.py [--reps 7] [--warmup 2] [--out results.json]

Cases: the 16- and the 52-layer x4 network on one clip of 7 frames of 180x320 (a 720p centre frame out).  Per case, the launch
profiler off, each forward timed with device events (--warmup rounds, then --reps rounds): milliseconds per centre frame, median
[min, max].  Then the per-kernel split of one forward from the launch profiler (launches, milliseconds, share) and the achieved
fp32 MFMA rate of the convolution kernels on their algorithmic FLOP against the 157.3 TFLOP/s peak.

Last, the (3,3,3) kernel against the same convolution composed from what the library had before it: three sr_conv3x3_f32
launches on the shifted frames, the second and third with ``accumulate`` (two read-modify-writes of the output more), for
224 -> 32 channels on 7 frames of 180x320, alternating launch by launch; the two results are compared as well.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from image_restoration_amd import _lib  # noqa: E402
from image_restoration_amd import hip_ops as H  # noqa: E402
from image_restoration_amd.archs.duf_arch import DUF  # noqa: E402

PEAK_TFLOPS = 157.3
FRAMES, HEIGHT, WIDTH = 7, 180, 320
MFMA_IDS = (81, 82, 194, 196)     # sr_convd_f32 (ksize 3 / 1), duf_conv3d_f32_kernel, duf_pw_f32_kernel


def profile(fn):
    """{kernel name: dict(kernel_id, launches, ms, flops)} of one call of ``fn`` from the launch profiler."""
    lib = _lib.load()
    cap = 1 << 14
    _lib.check(lib.sr_profile_start(cap), 'sr_profile_start')
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        recs = (_lib.LaunchRecord * cap)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, cap, C.byref(cnt)), 'sr_profile_stop')
    split = {}
    for i in range(min(cnt.value, cap)):
        r = recs[i]
        name = lib.sr_kernel_name(r.kernel_id).decode() or f'id {r.kernel_id}'
        if r.kernel_id == 194:
            name += f' -> {r.cout}'
        e = split.setdefault(name, dict(kernel_id=int(r.kernel_id), launches=0, ms=0.0, flops=0.0))
        e['launches'] += 1
        e['ms'] += float(r.ms)
        e['flops'] += float(r.flops)
    return split


def timed(fn):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    e.record()
    e.synchronize()
    return a.elapsed_time(e)


def bench_network(num_layer, dev, args):
    torch.manual_seed(0)
    net = DUF(4, num_layer).to(dev).eval().requires_grad_(False)
    with torch.no_grad():
        for m in net.modules():                                          # BatchNorm that is not the identity
            if isinstance(m, nn.BatchNorm3d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
                m.running_mean.uniform_(-0.3, 0.3)
                m.running_var.uniform_(0.5, 2.0)
    x = torch.rand(1, FRAMES, 3, HEIGHT, WIDTH, device=dev)
    ms = []
    for r in range(args.warmup + args.reps):
        t = timed(lambda: net(x))
        if r >= args.warmup:
            ms.append(t)
    split = profile(lambda: net(x))
    total = sum(e['ms'] for e in split.values())
    mfma_ms = sum(e['ms'] for e in split.values() if e['kernel_id'] in MFMA_IDS)
    mfma_flops = sum(e['flops'] for e in split.values() if e['kernel_id'] in MFMA_IDS)
    row = dict(case=f'DUF-{num_layer} x4, 1 clip of {FRAMES} frames {HEIGHT}x{WIDTH}', ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms),
               profiled_ms=total, mfma_tflops=mfma_flops / (mfma_ms * 1e-3) / 1e12 if mfma_ms else 0.0, split=split)
    print(f'{row["case"]}: {row["ms"]:.2f} ms per centre frame [{row["ms_min"]:.2f}, {row["ms_max"]:.2f}]; convolutions '
          f'{mfma_flops / 1e9:.0f} GFLOP in {mfma_ms:.2f} ms = {row["mfma_tflops"]:.1f} TFLOP/s = {100 * row["mfma_tflops"] / PEAK_TFLOPS:.1f} % of the '
          f'fp32 MFMA peak')
    print(f'    launch profile of one forward: {sum(e["launches"] for e in split.values())} launches, {total:.2f} ms in kernels')
    for name, e in sorted(split.items(), key=lambda kv: -kv[1]['ms']):
        tf = e['flops'] / (e['ms'] * 1e-3) / 1e12 if e['ms'] > 0 and e['flops'] > 0 else 0.0
        e['tflops'], e['share'] = tf, e['ms'] / total if total else 0.0
        mfma = f', {tf:.1f} TFLOP/s = {100 * tf / PEAK_TFLOPS:.1f} % of the fp32 MFMA peak' if e['kernel_id'] in MFMA_IDS else ''
        print(f'      {name:36s} id {e["kernel_id"]:3d}  {e["launches"]:3d} launches  {e["ms"]:8.3f} ms  {100 * e["share"]:5.1f} %{mfma}')
    return row


def bench_conv333(dev, args, cin=224, cout=32):
    """sr_duf_conv3d_f32 (3,3,3) with temporal padding against three accumulating sr_conv3x3_f32 launches on shifted frames."""
    torch.manual_seed(1)
    t, h, w = FRAMES, HEIGHT, WIDTH
    wt = (torch.randn(cout, cin, 3, 3, 3, device=dev) / (27 * cin) ** 0.5)
    bias = torch.randn(cout, device=dev)
    src = H.ClipCB8(torch.randn(1, t, cin // 8, h, w, 8, device=dev))
    frames = src.buf[0]                                                  # the same memory as a batch of 7 CB8 images
    pc3 = H.PackedDufConv(wt, bias)
    taps = [H.PackedConv(wt[:, :, dt].contiguous(), bias if dt == 1 else None) for dt in range(3)]
    out_new = H.ClipCB8.empty(1, t, cout, h, w, dev)
    out_old = torch.empty(t, cout // 8, h, w, 8, device=dev)

    def new():
        H.duf_conv3d(src, pc3, out_new, 0, pad_t=1)

    def old():
        H.conv3x3(H.CB8(frames), taps[1], out=H.CB8(out_old))                                            # frame t
        H.conv3x3(H.CB8(frames[:t - 1]), taps[0], out=H.CB8(out_old[1:]), accumulate=True)              # frame t - 1
        H.conv3x3(H.CB8(frames[1:]), taps[2], out=H.CB8(out_old[:t - 1]), accumulate=True)              # frame t + 1

    new()
    old()
    diff = float((out_new.buf[0] - out_old).abs().max())
    ms = {'conv3d': [], 'composed': []}
    for r in range(args.warmup + args.reps):
        for name, fn in (('conv3d', new), ('composed', old)):
            v = timed(fn)
            if r >= args.warmup:
                ms[name].append(v)
    flops = 2.0 * 27 * cin * cout * t * h * w
    row = dict(case=f'conv (3,3,3) {cin} -> {cout}, {t} frames {h}x{w}', max_abs_diff=diff)
    for name, v in ms.items():
        row[name + '_ms'], row[name + '_ms_min'], row[name + '_ms_max'] = statistics.median(v), min(v), max(v)
        row[name + '_tflops'] = flops / (row[name + '_ms'] * 1e-3) / 1e12
    row['composed_over_conv3d'] = row['composed_ms'] / row['conv3d_ms']
    print(f'{row["case"]}: sr_duf_conv3d_f32 {row["conv3d_ms"]:.3f} ms [{row["conv3d_ms_min"]:.3f}, {row["conv3d_ms_max"]:.3f}] = '
          f'{row["conv3d_tflops"]:.1f} TFLOP/s; three sr_conv3x3_f32 with accumulate {row["composed_ms"]:.3f} ms '
          f'[{row["composed_ms_min"]:.3f}, {row["composed_ms_max"]:.3f}] = {row["composed_tflops"]:.1f} TFLOP/s; composed / conv3d '
          f'{row["composed_over_conv3d"]:.2f}; max |difference| {diff:.2e}')
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    results = [bench_network(n, dev, args) for n in (16, 52)]
    results.append(bench_conv333(dev, args))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
