#!/usr/bin/env python3
"""EDVR's bf16 inference forward on one MI355X: the measurements of DESIGN.md §25.  Prints one JSON line.

* ``forward``: ``EDVR()`` with default arguments on (1, frames, 3, height, width), eval, torch.no_grad(): the fp32 and the bf16
  forward timed in interleaved rounds in one process (HIP events after warm-up, the launch profiler off), median and minimum
  per dtype, and the ratio of the medians.
* ``kernels``: the bf16 forward split by kernel id from the launch profiler (a run of its own).
* ``dcn``: sr_dcn_fwd_bf16 next to sr_dcn_fwd_f32 at the level-1 shape (frames x 64 x height x width, 8 groups, N(0, 2^2) offsets).
* ``conv1x1``: sr_conv1x1_bf16 at 320 -> 64 on one height x width map, and its achieved GB/s against the bytes it must move.

    python tools/edvr_bf16_bench.py [--rounds 5 --iters 5 --frames 5 --height 180 --width 320 --fp32_only]
"""
import argparse
import json
import os
import statistics
import sys
from collections import OrderedDict as OD

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_restoration_amd as ira  # noqa: E402
from image_restoration_amd import hip_ops as H  # noqa: E402
from edvr_bench import profile, split, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--frames', type=int, default=5)
    ap.add_argument('--height', type=int, default=180)
    ap.add_argument('--width', type=int, default=320)
    ap.add_argument('--fp32_only', action='store_true', help='time the fp32 forward only (a tree without the bf16 key)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    t, h, w = args.frames, args.height // 4 * 4, args.width // 4 * 4
    out = OD(frames=t, height=h, width=w)
    x = torch.rand(1, t, 3, h, w, device=dev)
    dtypes = ['fp32'] if args.fp32_only else ['fp32', 'bf16']
    nets = {}
    for d in dtypes:
        torch.manual_seed(0)
        kw = {} if d == 'fp32' else dict(compute_dtype=d)
        nets[d] = ira.build_network(dict(type='EDVR', num_frame=t, **kw)).to(dev).eval()
    times = {d: [] for d in dtypes}
    with torch.no_grad():
        for d in dtypes:
            nets[d](x)   # packs the weights
        for _ in range(args.rounds):
            for d in dtypes:
                times[d].append(timed(lambda: nets[d](x), args.iters, warmup=1))
    fwd = OD((d, dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), rounds=[round(a, 3) for a in v]))
             for d, v in times.items())
    if 'bf16' in fwd:
        fwd['fp32_over_bf16'] = round(fwd['fp32']['median_ms'] / fwd['bf16']['median_ms'], 3)
    out['forward'] = fwd
    if args.fp32_only:
        print(json.dumps(out))
        return
    with torch.no_grad():
        tot, kernels = split(profile(lambda: nets['bf16'](x)))
    out['kernels'] = OD(profiled_ms=round(tot, 3), by_kernel=kernels)

    # ---- the deformable conv alone, level-1 shape
    dg = 8
    g = torch.Generator(device='cpu').manual_seed(1)
    xf = torch.randn((t, 64, h, w), generator=g)
    off = (torch.randn((t, 18 * dg, h, w), generator=g) * 2).to(dev)
    msk = torch.randn((t, 9 * dg, h, w), generator=g).to(dev)
    wt, b = (torch.randn((64, 64, 3, 3), generator=g) * 0.04).to(dev), torch.zeros(64, device=dev)
    x16, x8 = H.nchw_to_cb16(xf.to(dev)), H.nchw_to_cb8(xf.to(dev))
    off8, msk8 = H.nchw_to_cb8(off), H.nchw_to_cb8(msk)
    p16, p8 = H.PackedConvBF16(wt, b), H.PackedConv(wt, b)
    o16, o8 = H.CB16.empty(t, 64, h, w, dev), H.CB8.empty(t, 64, h, w, dev)
    d = OD()
    d['bf16_ms'] = timed(lambda: H.dcn_fwd_bf16(x16, off, msk, p16, dg, mask_is_logit=True, act_slope=0.1, out=o16), 20)
    d['fp32_ms'] = timed(lambda: H.dcn_fwd(x8, off8, msk8, p8, dg, mask_is_logit=True, act_slope=0.1, out=o8), 20)
    d['fp32_over_bf16'] = d['fp32_ms'] / d['bf16_ms']
    d['bf16_tflops'] = 2 * 9 * 64 * 64 * t * h * w / d['bf16_ms'] / 1e9
    out['dcn'] = {k: round(v, 4) for k, v in d.items()}

    # ---- the 1x1 conv at TSA's fusion shape
    xf = H.nchw_to_cb16(torch.randn((1, 320, h, w), generator=g).to(dev))
    pw = H.PackedConv1x1BF16((torch.randn((64, 320, 1, 1), generator=g) * 0.05).to(dev), b)
    po = H.CB16.empty(1, 64, h, w, dev)
    ms = timed(lambda: H.conv1x1_bf16(xf, pw, out=po, act_slope=0.1), 50)
    out['conv1x1'] = dict(ms=round(ms, 4), gb_per_s=round(2 * (320 + 64) * h * w / ms / 1e6, 1))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
