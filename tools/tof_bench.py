#!/usr/bin/env python3
"""Times TOFlow inference (archs/tof_arch.py) on one GPU, in the manner of tools/basicvsr_bench.py.

    python tools/tof_bench.py [--reps 7] [--warmup 2] [--out results.json]

Cases: one Vid4-sized step (7 frames of 576x720, batch 1) and batch 4 of 7 frames of 256x256.  Two variants on the same
parameters and input, the launch profiler off, each forward timed with device events; the variants alternate forward by forward
in one process (--warmup rounds, then --reps rounds); median [min, max] over the rounds:

    product     the network as shipped
    torch       the same network from its definition in PyTorch-ROCm fp32 ops: nn.Conv2d, nn.BatchNorm2d (eval), F.avg_pool2d,
                F.interpolate, F.grid_sample (written in this tool only)

Then the per-kernel split of one product forward from the launch profiler (launches, milliseconds, share), and per 9x9 layer its
TFLOP/s on the algorithmic 2 * 81 * cin * cout FLOP per pixel against the 157.3 TFLOP/s fp32 MFMA peak, with the 7x7 instances'
figures from the same profile beside it.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from image_restoration_amd import _lib  # noqa: E402
from image_restoration_amd.archs.tof_arch import TOFlow  # noqa: E402
from spynet_bench import torch_warp  # noqa: E402

PEAK_TFLOPS = 157.3
CASES = (('Vid4 step: 1 clip of 7 frames 576x720', 1, 576, 720), ('4 clips of 7 frames 256x256', 4, 256, 256))


class TorchTOFlow(nn.Module):
    """The same network as plain PyTorch modules, sharing the HIP network's parameters and buffers."""

    def __init__(self, net):
        super().__init__()
        self.ref_idx, self.adapt = net.ref_idx, net.adapt_official_weights
        self.register_buffer('mean', net.mean)
        self.register_buffer('std', net.std)

        def conv(p, k):
            c = nn.Conv2d(p.in_channels, p.out_channels, k, 1, k // 2, bias=p.bias is not None)
            c.weight, c.bias = p.weight, p.bias
            return c
        levels = []
        for module in net.spynet.basic_module:
            layers = []
            for cv, bn in module.conv_bn():
                layers += [conv(cv, 7), bn, nn.ReLU(inplace=True)]
            layers.append(conv(module.basic_module[12], 7))
            levels.append(nn.Sequential(*layers))
        self.levels = nn.ModuleList(levels)
        self.conv_1, self.conv_2, self.conv_3, self.conv_4 = conv(net.conv_1, 9), conv(net.conv_2, 9), conv(net.conv_3, 1), conv(net.conv_4, 1)

    def spynet(self, ref, supp):
        n, _, h, w = ref.shape
        ref, supp = [ref], [supp]
        for _ in range(3):
            ref.insert(0, F.avg_pool2d(ref[0], 2, 2))
            supp.insert(0, F.avg_pool2d(supp[0], 2, 2))
        flow = ref[0].new_zeros(n, 2, h // 16, w // 16)
        for i in range(4):
            up = F.interpolate(flow, scale_factor=2, mode='bilinear', align_corners=True) * 2.0
            flow = up + self.levels[i](torch.cat([ref[i], torch_warp(supp[i], up.permute(0, 2, 3, 1), 'zeros'), up], 1))
        return flow

    def forward(self, lrs):
        if self.adapt:
            lrs = lrs[:, [3, 0, 1, 2, 4, 5, 6]]
        b, t, _, h, w = lrs.shape
        lrs = ((lrs.reshape(-1, 3, h, w) - self.mean) / self.std).view(b, t, 3, h, w)
        lr_ref = lrs[:, self.ref_idx]
        others = [i for i in range(7) if i != self.ref_idx]
        supp = lrs[:, others].reshape(6 * b, 3, h, w)                     # the six pairs as one batch, as the product does
        ref = lr_ref.unsqueeze(1).expand(b, 6, 3, h, w).reshape(6 * b, 3, h, w)
        warped = torch_warp(supp, self.spynet(ref, supp).permute(0, 2, 3, 1), 'zeros').view(b, 6, 3, h, w)
        frames = [warped[:, k] for k in range(6)]
        frames.insert(self.ref_idx, lr_ref)
        hr = torch.cat(frames, 1)
        hr = F.relu(self.conv_1(hr))
        hr = F.relu(self.conv_2(hr))
        hr = F.relu(self.conv_3(hr))
        return (self.conv_4(hr) + lr_ref) * self.std + self.mean


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
        if r.kernel_id == 188:
            name += f' {r.cin}->{r.cout}'
        e = split.setdefault(name, dict(kernel_id=int(r.kernel_id), launches=0, ms=0.0, flops=0.0))
        e['launches'] += 1
        e['ms'] += float(r.ms)
        e['flops'] += float(r.flops)
    return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = TOFlow().to(dev).eval().requires_grad_(False)
    with torch.no_grad():
        for m in net.modules():                                          # BatchNorm that is not the identity
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
                m.running_mean.uniform_(-0.3, 0.3)
                m.running_var.uniform_(0.5, 2.0)
    ref = TorchTOFlow(net).to(dev).eval()
    results = []
    for case, b, h, w in CASES:
        x = torch.rand(b, 7, 3, h, w, device=dev)
        ms = {'product': [], 'torch': []}
        with torch.no_grad():
            diff = float((net(x) - ref(x)).abs().max())
            for r in range(args.warmup + args.reps):
                for name, fn in (('product', net), ('torch', ref)):
                    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn(x)
                    e.record()
                    e.synchronize()
                    if r >= args.warmup:
                        ms[name].append(a.elapsed_time(e))
            split = profile(lambda: net(x))
        total = sum(e['ms'] for e in split.values())
        row = dict(case=case, max_abs_diff_vs_torch=diff, profiled_ms=total, split=split)
        for name, v in ms.items():
            row[name + '_ms'], row[name + '_ms_min'], row[name + '_ms_max'] = statistics.median(v), min(v), max(v)
        row['torch_over_product'] = row['torch_ms'] / row['product_ms']
        print(f'{case}: product {row["product_ms"]:.2f} ms [{row["product_ms_min"]:.2f}, {row["product_ms_max"]:.2f}], torch '
              f'{row["torch_ms"]:.2f} ms [{row["torch_ms_min"]:.2f}, {row["torch_ms_max"]:.2f}], torch / product '
              f'{row["torch_over_product"]:.2f}; max |product - torch| {diff:.2e}')
        print(f'    launch profile of one forward: {sum(e["launches"] for e in split.values())} launches, {total:.2f} ms in kernels')
        for name, e in sorted(split.items(), key=lambda kv: -kv[1]['ms']):
            tf = e['flops'] / (e['ms'] * 1e-3) / 1e12 if e['ms'] > 0 and e['flops'] > 0 else 0.0
            e['tflops'], e['share'] = tf, e['ms'] / total if total else 0.0
            mfma = f', {tf:.1f} TFLOP/s = {100 * tf / PEAK_TFLOPS:.1f} % of the fp32 MFMA peak' if 'conv' in name and 'pack' not in name else ''
            print(f'      {name:36s} id {e["kernel_id"]:3d}  {e["launches"]:3d} launches  {e["ms"]:8.3f} ms  {100 * e["share"]:5.1f} %{mfma}')
        results.append(row)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
