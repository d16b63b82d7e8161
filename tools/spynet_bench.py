#!/usr/bin/env python3
"""Times SpyNet, its five 7x7 convolutions and flow warping (include/sr_hip_flow.h) against the same ops in PyTorch-ROCm
(nn.Conv2d 7x7, F.grid_sample, F.interpolate, F.avg_pool2d) on one GPU.

    python tools/spynet_bench.py [--pairs 8] [--reps 20] [--warmup 5] [--out results.json]

Rows: SpyNet on --pairs frame pairs at 180x320 (padded to 192x320 inside) and at 64x64; each conv of a basic module alone on
--pairs maps of 192x320 (bias + ReLU as in the network; the last one with its flow residual); flow_warp of 64 channels at 180x320.
Per row the HIP call and the PyTorch form run on the same tensors, interleaved in one process (HIP, PyTorch, HIP again); each is
timed with device events around one call, and the median over --reps calls after --warmup calls is reported.  Conv rows also
give TFLOP/s of the algorithmic 2 * 49 * cin * cout FLOP per pixel and its fraction of the 157.3 TFLOP/s fp32 MFMA peak.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image_restoration_amd import hip_ops as H  # noqa: E402
from image_restoration_amd.archs.spynet_arch import SpyNet  # noqa: E402
from image_restoration_amd.ops.flow_warp import flow_warp  # noqa: E402

PEAK_TFLOPS = 157.3


def timed(fn, reps, warmup):
    """Median milliseconds of one call, device events around each call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def torch_warp(x, flow, padding_mode):
    """flow_warp in PyTorch: the normalised grid and F.grid_sample(align_corners=True)."""
    h, w = x.shape[-2:]
    gy, gx = torch.meshgrid(torch.arange(h, device=x.device, dtype=x.dtype), torch.arange(w, device=x.device, dtype=x.dtype), indexing='ij')
    grid = torch.stack((2.0 * (gx + flow[..., 0]) / max(w - 1, 1) - 1.0, 2.0 * (gy + flow[..., 1]) / max(h - 1, 1) - 1.0), 3)
    return F.grid_sample(x, grid, mode='bilinear', padding_mode=padding_mode, align_corners=True)


class TorchSpyNet(nn.Module):
    """The same network as plain PyTorch modules, sharing the HIP network's parameters."""

    def __init__(self, net):
        super().__init__()
        self.levels = nn.ModuleList()
        for bm in net.basic_module:
            layers = []
            for i, p in enumerate(bm.convs()):
                conv = nn.Conv2d(p.in_channels, p.out_channels, 7, 1, 3)
                conv.weight, conv.bias = p.weight, p.bias
                layers += [conv] + ([nn.ReLU()] if i < 4 else [])
            self.levels.append(nn.Sequential(*layers))
        self.mean, self.std = net.mean, net.std

    def forward(self, ref, supp):
        h, w = ref.shape[-2:]
        hf, wf = math.ceil(h / 32) * 32, math.ceil(w / 32) * 32
        ref = F.interpolate(ref, size=(hf, wf), mode='bilinear', align_corners=False)
        supp = F.interpolate(supp, size=(hf, wf), mode='bilinear', align_corners=False)
        refs, supps = [(ref - self.mean) / self.std], [(supp - self.mean) / self.std]
        for _ in range(5):
            refs.insert(0, F.avg_pool2d(refs[0], 2, 2))
            supps.insert(0, F.avg_pool2d(supps[0], 2, 2))
        flow = ref.new_zeros(ref.size(0), 2, refs[0].size(2), refs[0].size(3))
        for lv in range(6):
            up = flow if lv == 0 else F.interpolate(flow, scale_factor=2, mode='bilinear', align_corners=True) * 2.0
            warped = torch_warp(supps[lv], up.permute(0, 2, 3, 1), 'border')
            flow = self.levels[lv](torch.cat([refs[lv], warped, up], 1)) + up
        flow = F.interpolate(flow, size=(h, w), mode='bilinear', align_corners=False)
        return flow * flow.new_tensor([w / wf, h / hf]).view(1, 2, 1, 1)


def backward_rows(net, ref_net, n, dev, row):
    """--backward: per conv of a basic module the masked data gradient (sr_conv7x7_dgrad_f32 against torch.nn.grad.conv2d_input
    and the mask product) and the weight + bias gradient (sr_conv7x7_wgrad_f32 against torch.nn.grad.conv2d_weight and a sum) on
    --pairs maps of 192x320; then forward + backward of the whole network, HIP autograd against PyTorch autograd of the same ops
    on the same parameters, at 180x320 and at 64x64."""
    for p in net.basic_module[5].convs():
        cin, cout = p.in_channels, p.out_channels
        x, dy = torch.randn(n, cin, 192, 320, device=dev), torch.randn(n, cout, 192, 320, device=dev)
        src, d, pc = H.nchw_to_cb8(x), H.nchw_to_cb8(dy), net.packed(p, 1)
        flops = 2.0 * 49 * cin * cout * n * 192 * 320
        w = p.weight.detach()
        row(f'dgrad7x7 {cout}->{cin} {n}x192x320', lambda: H.conv7x7_dgrad(d, pc, mask=src),
            lambda: torch.nn.grad.conv2d_input(x.shape, w, dy, padding=3) * (x > 0), flops, instance=pc.instance)
        row(f'wgrad7x7 {cin}->{cout} {n}x192x320', lambda: H.conv7x7_wgrad(src, d, cout, cin),
            lambda: (torch.nn.grad.conv2d_weight(x, w.shape, dy, padding=3), dy.sum((0, 2, 3))), flops)
        del x, dy, src, d
    net.train().set_autograd(True)
    ref_net.train()
    params = list(net.parameters())
    for h, w in ((180, 320), (64, 64)):
        a, b = torch.rand(n, 3, h, w, device=dev), torch.rand(n, 3, h, w, device=dev)
        g = torch.randn(n, 2, h, w, device=dev)

        def step(model):
            for q in params:
                q.grad = None
            (model(a, b) * g).sum().backward()
        step(net)
        mine = [q.grad.clone() for q in params]
        step(ref_net)
        diff = max(float((m - q.grad).norm() / q.grad.norm()) for m, q in zip(mine, params))
        hf, wf = math.ceil(h / 32) * 32, math.ceil(w / 32) * 32
        flops = 3 * 479808.0 * n * sum((hf >> k) * (wf >> k) for k in range(6))
        row(f'SpyNet fwd+bwd {n} pairs {h}x{w}', lambda: step(net), lambda: step(ref_net), flops, max_rel_l2_diff=diff)
    net.eval().set_autograd(False)
    ref_net.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=8)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--backward', action='store_true', help='time the backward rows instead: each data and weight gradient, '
                    'and forward + backward of the whole network')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('spynet_bench needs a GPU: timings are device timings')
    dev = torch.device('cuda:0')
    n = args.pairs
    torch.manual_seed(0)
    net = SpyNet().to(dev).eval()
    ref_net = TorchSpyNet(net).to(dev).eval()
    rows = []

    def row(name, hip, ref, flops=None, **extra):
        t_hip, t_ref = timed(hip, args.reps, args.warmup), timed(ref, args.reps, args.warmup)
        t_hip = min(t_hip, timed(hip, args.reps, args.warmup))          # interleaved: HIP, PyTorch, HIP again
        r = dict(case=name, hip_ms=t_hip, torch_ms=t_ref, **extra)
        if flops:
            r.update(flops=flops, hip_tflops=flops / t_hip / 1e9, torch_tflops=flops / t_ref / 1e9,
                     hip_of_peak=flops / t_hip / 1e9 / PEAK_TFLOPS)
        rows.append(r)

    if args.backward:
        backward_rows(net, ref_net, n, dev, row)
    with torch.no_grad():
        for h, w in (() if args.backward else ((180, 320), (64, 64))):
            a, b = torch.rand(n, 3, h, w, device=dev), torch.rand(n, 3, h, w, device=dev)
            diff = float((net(a, b) - ref_net(a, b)).abs().max())
            hf, wf = math.ceil(h / 32) * 32, math.ceil(w / 32) * 32
            flops = 479808.0 * n * sum((hf >> k) * (wf >> k) for k in range(6))
            row(f'SpyNet {n} pairs {h}x{w}', lambda: net(a, b), lambda: ref_net(a, b), flops, max_abs_diff=diff)
        for lv_conv, p in enumerate(() if args.backward else net.basic_module[5].convs()):
            cin, cout = p.in_channels, p.out_channels
            x = torch.randn(n, cin, 192, 320, device=dev)
            src, pc = H.nchw_to_cb8(x), net.packed(p)
            res = H.CB8.zeros(n, 8, 192, 320, dev) if cout == 2 else None
            tconv = ref_net.levels[5][2 * lv_conv]
            if cout == 2:
                hip, ref = (lambda: H.conv7x7(src, pc, res1=res)), (lambda: tconv(x))
            else:
                hip, ref = (lambda: H.conv7x7(src, pc, relu=True)), (lambda: F.relu(tconv(x)))
            row(f'conv7x7 {cin}->{cout} {n}x192x320', hip, ref, 2.0 * 49 * cin * cout * n * 192 * 320, instance=pc.instance)
            del x, src
        x, flow = torch.randn(n, 64, 180, 320, device=dev), torch.randn(n, 180, 320, 2, device=dev) * 4
        for pm in (() if args.backward else ('zeros', 'border')):
            row(f'flow_warp {n}x64x180x320 {pm}', lambda: flow_warp(x, flow, padding_mode=pm), lambda: torch_warp(x, flow, pm))
    print(f'{"case":36s} {"HIP ms":>9s} {"torch ms":>9s} {"HIP TFLOP/s":>12s} {"of peak":>8s} {"torch TFLOP/s":>14s}')
    for r in rows:
        tf = f'{r["hip_tflops"]:12.1f} {r["hip_of_peak"]:8.2f} {r["torch_tflops"]:14.1f}' if 'flops' in r else ''
        print(f'{r["case"]:36s} {r["hip_ms"]:9.3f} {r["torch_ms"]:9.3f} {tf}')
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(dict(pairs=n, reps=args.reps, warmup=args.warmup, peak_tflops=PEAK_TFLOPS, rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
