#!/usr/bin/env python3
"""EDVR on one MI355X: the measurements of DESIGN.md §24.  Prints one JSON line.

* ``conv_s2``: sr_conv3x3s2_f32 at EDVR's L1 -> L2 shape (5 x 64 x 180 x 320) next to sr_conv3x3_f32 on the same input, whose
  subsampled output was the only route before; and the backward's three launches (zero insert, data gradient, weight gradient).
* ``memory_bound``: achieved GB/s of the pool, correlation and gate kernels against the bytes they must move.
* ``forward``: ``EDVR()`` with default arguments on (1, 5, 3, 180, 320) under torch.no_grad(), and its split by kernel id from
  the launch profiler.

    python tools/edvr_bench.py [--iters 20 --frames 5 --height 180 --width 320]
"""
import argparse
import ctypes as C
import json
import os
import sys
from collections import OrderedDict as OD

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_restoration_amd as ira  # noqa: E402
from image_restoration_amd import _lib, hip_ops  # noqa: E402


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


def split(recs):
    lib = _lib.load()
    by = OD()
    for r in recs:
        e = by.setdefault(f'{r.kernel_id}:{lib.sr_kernel_name(r.kernel_id).decode()}', [0, 0.0])
        e[0] += 1
        e[1] += r.ms
    tot = sum(v[1] for v in by.values())
    return tot, {k: dict(launches=v[0], ms=round(v[1], 3), share=round(v[1] / tot, 4)) for k, v in by.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--frames', type=int, default=5)
    ap.add_argument('--height', type=int, default=180)
    ap.add_argument('--width', type=int, default=320)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    t, h, w = args.frames, args.height, args.width
    out = OD(frames=t, height=h, width=w)

    # ---- the stride-2 conv at L1 -> L2
    f = hip_ops.CB8.empty(t, 64, h, w, dev)
    f.buf.normal_()
    wt, b = torch.randn(64, 64, 3, 3, device=dev) * 0.04, torch.zeros(64, device=dev)
    pc, pct = hip_ops.PackedConv(wt, b), hip_ops.PackedConv(wt, None, mode=1)
    o2 = hip_ops.CB8.empty(t, 64, (h + 1) // 2, (w + 1) // 2, dev)
    o1 = hip_ops.CB8.empty(t, 64, h, w, dev)
    o2.buf.normal_()
    s2 = OD()
    s2['conv3x3s2_ms'] = timed(lambda: hip_ops.conv3x3s2(f, pc, o2, act_slope=0.1), args.iters)
    s2['conv3x3_full_ms'] = timed(lambda: hip_ops.conv3x3(f, pc, o1, act_slope=0.1), args.iters)
    s2['full_over_s2'] = s2['conv3x3_full_ms'] / s2['conv3x3s2_ms']
    s2['conv3x3s2_tflops'] = 2 * 9 * 64 * 64 * t * o2.h * o2.w / s2['conv3x3s2_ms'] / 1e9
    s2['zero_insert_ms'] = timed(lambda: hip_ops.zero_insert2(o2, h, w, out=o1), args.iters)
    s2['bwd_data_conv3x3_ms'] = timed(lambda: hip_ops.conv3x3(o1, pct), args.iters)
    s2['bwd_weight_wgrad_ms'] = timed(lambda: hip_ops.conv3x3_wgrad(f, o1, 64, 64), args.iters)
    out['conv_s2'] = {k: round(v, 4) for k, v in s2.items()}
    del o1

    # ---- the memory-bound kernels at EDVR's shapes: bytes that must move / time
    mb = OD()
    px = h * w

    def gbs(nbytes, ms):
        return round(nbytes / ms / 1e6, 1)
    a1 = hip_ops.CB8.empty(1, 64, h, w, dev)
    a1.buf.normal_()
    pool_out = hip_ops.CB8.empty(1, 128, (h + 1) // 2, (w + 1) // 2, dev)
    ms = timed(lambda: hip_ops.pool3x3s2(a1, out=pool_out), args.iters)
    mb['pool_fwd'] = dict(ms=round(ms, 4), gb_per_s=gbs(4 * 64 * (px + 2 * pool_out.h * pool_out.w), ms))
    pool_out.buf.normal_()
    dx = hip_ops.CB8.empty(1, 64, h, w, dev)
    ms = timed(lambda: hip_ops.pool3x3s2_bwd(a1, pool_out, out=dx), args.iters)
    mb['pool_bwd'] = dict(ms=round(ms, 4), gb_per_s=gbs(4 * 64 * (2 * px + 2 * pool_out.h * pool_out.w), ms))
    emb = hip_ops.CB8.empty(t, 64, h, w, dev)
    emb.buf.normal_().mul_(0.3)
    ref = hip_ops.CB8.empty(1, 64, h, w, dev)
    ref.buf.normal_().mul_(0.3)
    co = hip_ops.CB8.empty(t, 64, h, w, dev)
    ms = timed(lambda: hip_ops.tsa_corr(emb, ref, f, t, out=co), args.iters)
    mb['tsa_corr_fwd'] = dict(ms=round(ms, 4), gb_per_s=gbs(4 * px * (3 * t * 64 + 64 + t), ms))
    prob, _ = hip_ops.tsa_corr(emb, ref, f, t, out=co)
    ms = timed(lambda: hip_ops.tsa_corr_bwd(co, emb, ref, f, prob), args.iters)
    mb['tsa_corr_bwd'] = dict(ms=round(ms, 4), gb_per_s=gbs(4 * px * (5 * t * 64 + 2 * 64 + 2 * t), ms))
    ms = timed(lambda: hip_ops.tsa_gate(a1, dx, a1, out=dx), args.iters)
    mb['tsa_gate_fwd'] = dict(ms=round(ms, 4), gb_per_s=gbs(4 * 64 * px * 4, ms))
    ms = timed(lambda: hip_ops.tsa_gate_bwd(a1, dx, a1), args.iters)
    mb['tsa_gate_bwd'] = dict(ms=round(ms, 4), gb_per_s=gbs(4 * 64 * px * 5, ms))
    out['memory_bound'] = mb
    del f, emb, ref, co, a1, dx, pool_out, o2

    # ---- the whole network
    net = ira.build_network(dict(type='EDVR', num_frame=t)).to(dev).eval()
    x = torch.rand(1, t, 3, h // 4 * 4, w // 4 * 4, device=dev)
    with torch.no_grad():
        fwd = timed(lambda: net(x), max(3, args.iters // 4), warmup=2)
        tot, kernels = split(profile(lambda: net(x)))
    new = sum(v['ms'] for k, v in kernels.items() if 114 <= int(k.split(':')[0]) <= 122)
    out['forward'] = OD(ms=round(fwd, 2), profiled_ms=round(tot, 2), new_kernel_share=round(new / tot, 4), kernels=kernels)

    # one forward + backward, for the share of the zero-insert route
    xg = x.clone().requires_grad_(True)

    def step():
        net.zero_grad(set_to_none=True)
        net(xg).sum().backward()
    step()
    tot, kernels = split(profile(step))
    zi = kernels.get('115:cb8_zero_insert2_kernel', dict(ms=0.0))['ms']
    out['train_step'] = OD(profiled_ms=round(tot, 2), zero_insert_ms=zi, new_kernel_share=round(
        sum(v['ms'] for k, v in kernels.items() if 114 <= int(k.split(':')[0]) <= 122) / tot, 4), kernels=kernels)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
