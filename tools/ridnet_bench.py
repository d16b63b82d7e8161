#!/usr/bin/env python3
"""RIDNet on one MI355X: forward images/s (batch 16 of 128x128 noisy images, the default net), the per-kernel time split of one
forward from the launch profiler, the per-launch time of the dilated convs next to the dense 3x3 at the same shape
(64 -> 64, 16 x 128^2), and the time of one SRModel step (L1, Adam) at the same batch.  Prints one JSON line.

    python tools/ridnet_bench.py [--batch 16 --size 128 --iters 20]
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
from image_restoration_amd.utils import synth  # noqa: E402

PEAK_TFLOPS = 157.3   # fp32 MFMA peak of one MI355X


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    n, s = args.batch, args.size
    cfg = dict(in_channels=3, mid_channels=64, out_channels=3, num_block=4)
    net = ira.build_network(dict(type='RIDNet', **cfg))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.ridnet_state_dict(0, **cfg).items()}, strict=True)
    net = net.to(dev).eval()
    x = torch.from_numpy(synth.uniform_input(1, (n, 3, s, s))).to(dev)
    out = OD(batch=n, size=s)
    with torch.no_grad():
        ms = timed(lambda: net(x), args.iters)
        recs = profile(lambda: net(x))
    flops = sum(r.flops for r in recs)
    out['fwd_ms'] = round(ms, 3)
    out['fwd_images_per_s'] = round(n / ms * 1e3, 1)
    out['fwd_tflops'] = round(flops / ms / 1e9, 2)
    out['fwd_frac_of_fp32_peak'] = round(flops / ms / 1e9 / PEAK_TFLOPS, 3)
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
                              tflops=round(v[2] / v[1] / 1e9, 1) if v[1] > 0 and v[2] > 0 else None) for k, v in by.items()}
    ca = sum(v[1] for k, v in by.items() if int(k.split(':')[0]) in (74, 75, 89))
    out['ca_share'] = round(ca / tot, 4)

    # one conv layer, 64 -> 64 at n x s^2: the dense 3x3 (sr_conv3x3_f32) and the new path at dilation 1..4, and the 1x1
    f = hip_ops.CB8.empty(n, 64, s, s, dev)
    f.buf.normal_()
    w3 = torch.randn(64, 64, 3, 3, device=dev) * 0.04
    w1 = torch.randn(64, 64, 1, 1, device=dev) * 0.1
    b = torch.zeros(64, device=dev)
    pc3, pc1 = hip_ops.PackedConv(w3, b), hip_ops.PackedConvK(w1, b)
    o = hip_ops.CB8.empty(n, 64, s, s, dev)
    layer = OD()
    layer['dense3x3_conv3x3'] = timed(lambda: hip_ops.conv3x3(f, pc3, o, act_slope=0.0), args.iters)
    for d in (1, 2, 3, 4):
        layer[f'convd_d{d}'] = timed(lambda d=d: hip_ops.convd(f, pc3, d, o, act_slope=0.0), args.iters)
    layer['convd_1x1'] = timed(lambda: hip_ops.convd(f, pc1, 1, o, act_slope=0.0), args.iters)
    gflop = 2 * 9 * 64 * 64 * n * s * s / 1e9
    out['layer_ms'] = {k: round(v, 4) for k, v in layer.items()}
    out['layer_tflops'] = {k: round((gflop / 9 if k.endswith('1x1') else gflop) / v, 1) for k, v in layer.items()}
    out['dilated_over_dense'] = {f'd{d}': round(layer[f'convd_d{d}'] / layer['dense3x3_conv3x3'], 3) for d in (2, 3, 4)}
    for d in (1, 2, 3, 4):
        out.setdefault('wgrad_ms', {})[f'd{d}'] = round(timed(lambda d=d: hip_ops.convd_wgrad(f, o, 64, 64, 3, d), args.iters), 4)
    out['wgrad_ms']['dense3x3'] = round(timed(lambda: hip_ops.conv3x3_wgrad(f, o, 64, 64), args.iters), 4)
    del f, o

    # one SRModel step (L1, Adam) at the same batch
    from image_restoration_amd.models import build_model
    opt = OD(name='bench', model_type='SRModel', scale=1, num_gpu=1, manual_seed=0, is_train=True, dist=False, rank=0, world_size=1)
    opt['network_g'] = OD(type='RIDNet', **cfg)
    opt['path'] = OD(pretrain_network_g=None, strict_load_g=True, resume_state=None)
    tr = OD(ema_decay=0)
    tr['optim_g'] = OD(type='Adam', lr=1e-4, weight_decay=0, betas=[0.9, 0.99])
    tr['scheduler'] = OD(type='MultiStepLR', milestones=[10 ** 6], gamma=0.5)
    tr['total_iter'] = 10 ** 6
    tr['warmup_iter'] = -1
    tr['pixel_opt'] = OD(type='L1Loss', loss_weight=1.0, reduction='mean')
    opt['train'] = tr
    model = build_model(opt)
    gt = torch.from_numpy(synth.uniform_input(2, (n, 3, s, s)))
    lq = (gt + 0.1 * torch.from_numpy(synth.gaussian(3, (n, 3, s, s)))).clamp_(0, 1)
    it = [0]

    def step():
        it[0] += 1
        model.feed_data({'lq': lq, 'gt': gt})
        model.optimize_parameters(it[0])
    out['srmodel_step_ms'] = round(timed(step, max(3, args.iters // 4), warmup=2), 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
