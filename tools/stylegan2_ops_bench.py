#!/usr/bin/env python3
"""Times upfirdn2d and the fused bias + LeakyReLU (include/sr_hip_stylegan2.h) against their plain PyTorch forms on one GPU.

    python tools/stylegan2_ops_bench.py [--batch 16] [--reps 30] [--warmup 5] [--out results.json]

Shapes: batch 16 at the StyleGAN2 discriminator of the product's training configuration (256 x 256 input, channel_multiplier 1:
64 channels at 256^2, 128 at 128^2, 512 from 32^2 down).  Per case the HIP call and the PyTorch form run on the same tensors,
interleaved in one process; each is timed with device events around one call, and the median over --reps calls after --warmup
calls is reported with the GB/s of the bytes the call must move (source + destination, fp32) next to the chip's measured copy
rate (6.29 TB/s).  `fits_llc` says whether those bytes fit the 256 MiB last-level cache, where a repeated call need not go to
HBM at all.  The gradient call of each upfirdn2d case is the factor-swapped call on the output's gradient.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image_restoration_amd import hip_ops as H  # noqa: E402
from image_restoration_amd.archs.stylegan2_arch import make_resample_kernel  # noqa: E402
from image_restoration_amd.ops.upfirdn2d import upfirdn2d_native  # noqa: E402
from image_restoration_amd.ops.upfirdn2d.upfirdn2d import grad_pad  # noqa: E402

COPY_TBS = 6.29
LLC_BYTES = 256 * 2 ** 20


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('stylegan2_ops_bench needs a GPU: timings are device timings')
    dev = torch.device('cuda:0')
    n = args.batch
    k = make_resample_kernel((1, 3, 3, 1)).to(dev)
    # name, (C, H, W), up, down, pad: the blur in front of a stride-2 3x3 conv, the up-sampler, the down-sampler
    ufd_cases = [('smooth 64x256^2 (instance 1)', (64, 256, 256), (1, 1), (1, 1), (2, 2, 2, 2), k),
                 ('smooth 512x32^2 (instance 1)', (512, 32, 32), (1, 1), (1, 1), (2, 2, 2, 2), k),
                 ('upsample 128x128^2 (instance 2)', (128, 128, 128), (2, 2), (1, 1), (2, 1, 2, 1), (k * 4).contiguous()),
                 ('downsample 64x256^2 (instance 3)', (64, 256, 256), (1, 1), (2, 2), (1, 1, 1, 1), k)]
    rows = []
    for name, (c, h, w), up, down, pad, kern in ufd_cases:
        x = torch.randn((n, c, h, w), device=dev)
        y = H.upfirdn2d(x, kern, up, down, pad)
        g = torch.randn_like(y)
        flipped = torch.flip(kern, [0, 1]).contiguous()
        gp = grad_pad((h, w), y.shape[2:], kern.shape, up, down, pad)
        assert H.upfirdn2d(g, flipped, down, up, gp).shape == x.shape
        nbytes = 4 * (x.numel() + y.numel())
        for what, hip, ref in (
                ('forward', lambda: H.upfirdn2d(x, kern, up, down, pad), lambda: upfirdn2d_native(x, kern, *up, *down, *pad)),
                ('gradient', lambda: H.upfirdn2d(g, flipped, down, up, gp), lambda: upfirdn2d_native(g, flipped, *down, *up, *gp))):
            t_hip, t_ref = timed(hip, args.reps, args.warmup), timed(ref, args.reps, args.warmup)
            t_hip = min(t_hip, timed(hip, args.reps, args.warmup))          # interleaved: HIP, PyTorch, HIP again
            rows.append(dict(op='upfirdn2d', case=name, call=what, instance=H.upfirdn2d_instance(*kern.shape, *(up if what == 'forward' else down),
                                                                                                  *(down if what == 'forward' else up))[0],
                             hip_ms=t_hip, torch_ms=t_ref, bytes=nbytes, hip_gbs=nbytes / t_hip / 1e6, torch_gbs=nbytes / t_ref / 1e6,
                             fits_llc=nbytes <= LLC_BYTES))
        del x, y, g
    for c, h, w in ((64, 256, 256), (512, 32, 32)):
        x, g, b = torch.randn((n, c, h, w), device=dev), torch.randn((n, c, h, w), device=dev), torch.randn(c, device=dev)
        out = H.fused_bias_act(x, b)
        slope, scale = 0.2, 2 ** 0.5

        def torch_fwd():
            return F.leaky_relu(x + b.view(1, -1, 1, 1), slope) * scale

        def torch_bwd():
            gx = torch.where(out > 0, g, g * slope) * scale
            return gx, gx.sum((0, 2, 3))
        for what, hip, ref, nbytes in (('forward', lambda: H.fused_bias_act(x, b), torch_fwd, 8 * x.numel()),
                                       ('backward', lambda: H.fused_bias_act_bwd(g, out), torch_bwd, 12 * x.numel())):
            t_hip, t_ref = timed(hip, args.reps, args.warmup), timed(ref, args.reps, args.warmup)
            t_hip = min(t_hip, timed(hip, args.reps, args.warmup))
            rows.append(dict(op='fused_bias_act', case=f'{c}x{h}^2', call=what, hip_ms=t_hip, torch_ms=t_ref, bytes=nbytes,
                             hip_gbs=nbytes / t_hip / 1e6, torch_gbs=nbytes / t_ref / 1e6, fits_llc=nbytes <= LLC_BYTES))
        del x, g, out
    print(f'{"op":15s} {"case":34s} {"call":9s} {"HIP ms":>8s} {"GB/s":>7s} {"of copy":>8s} {"torch ms":>9s} {"GB/s":>7s}  fits LLC')
    for r in rows:
        print(f'{r["op"]:15s} {r["case"]:34s} {r["call"]:9s} {r["hip_ms"]:8.3f} {r["hip_gbs"]:7.0f} {r["hip_gbs"] / (COPY_TBS * 1e3):8.2f} '
              f'{r["torch_ms"]:9.3f} {r["torch_gbs"]:7.0f}  {r["fits_llc"]}')
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(dict(batch=n, reps=args.reps, warmup=args.warmup, copy_tbs=COPY_TBS, rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
