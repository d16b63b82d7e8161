#!/usr/bin/env python3
"""Times BasicVSR inference (archs/basicvsr_arch.py) on one GPU, in the manner of tools/spynet_bench.py.

    python tools/basicvsr_bench.py [--num-block 30] [--reps 20] [--warmup 5] [--other-tree DIR] [--out results.json]
    python tools/basicvsr_bench.py --backward [--num-block 30] [--batch 4] [--reps 5] [--warmup 2] [--out results.json]
    python tools/basicvsr_bench.py --backward --deterministic [--num-block 30] [--batch 4] [--reps 5] [--warmup 2] [--out results.json]

Cases: one 180x320 clip of 15 frames, and one 64x112 clip of 7 frames (below the Winograd size rule: the trunks run on the direct
kernels).  Three variants on the same parameters and input, the launch profiler off, each forward timed with device events;
the variants alternate forward by forward in one process (--warmup rounds, then --reps rounds), the median over the rounds is
reported:

    product     the network as shipped: sr_vsr_prop_input_f32 + sr_vsr_trunk_f32 per step
    per-layer   the same forward (the same step-input launch, the same windows) with every trunk conv issued through
                hip_ops.conv3x3 from Python (written in this tool only); with --wino-off both variants run the direct kernels, so
                the difference is the cost of issuing the convs from Python alone
    torch       the same network from its definition in PyTorch-ROCm ops: nn.Conv2d, F.grid_sample, F.pixel_shuffle, F.interpolate
                (written in this tool only; its SpyNet is tools/spynet_bench.py's)

    bf16        the product with set_compute_dtype('bf16'): sr_rvsr_prop_input_bf16 + sr_rvsr_trunk_bf16 per step and the head on the
                bf16 convs; SpyNet stays fp32 (same parameters, its own module)
    other fp32  with --other-tree: the product of another built checkout of this project (the parent commit, say), imported as a
                second copy of the package under another name so that it runs on its own libsr_hip.so in the same process
    other bf16  with --other-tree: that checkout's product with set_compute_dtype('bf16'), compared with this tree's bf16 row

Per variant the median and the spread (min, max) of the rounds are reported.  Also: one trunk call alone on one frame (ms, TFLOP/s on the algorithmic 2 * 9 * cin * cout FLOP per pixel, fraction of the 157.3
TFLOP/s fp32 MFMA peak) and sr_vsr_prop_input_f32 alone (ms and bytes/s on 32 bytes per corner, pixel and block, plus the store,
the frame and the flow), both from device events around 50 back-to-back calls; the same two for the bf16 entry points (fraction of
the 2500.0 TFLOP/s dense bf16 MFMA peak).

--backward times training instead (archs/basicvsr_autograd.py): forward plus backward of L = sum(y * g) at the REDS recipe's shape —
15 frames of 64x64, num_feat 64, --batch clips — of the product with set_autograd(True) and, as a yardstick, of the torch variant
above under PyTorch-ROCm autograd on the same device and parameters, the two alternating round by round; the largest relative L2
between their parameter gradients; the bytes the training forward keeps per clip; and the per-kernel split of one product step from
the launch profiler (count, milliseconds, share), with the share of the two step kernels (ids 159 and 178).

--backward --deterministic times the deterministic backward (set_autograd(True, deterministic=True): sr_vsr_prop_input_bwd_det_f32,
kernels 180-182) against the default one (kernel 178) at the same shape in one process, the two alternating round by round: the
step time of each as median [min, max], the time of the step-input adjoint's kernels per step from the launch profiler, whether two
deterministic passes agree bit for bit, and the largest relative L2 between the two modes' parameter gradients.
"""
import argparse
import importlib.util
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
from image_restoration_amd import hip_ops as H  # noqa: E402
from image_restoration_amd.archs.basicvsr_arch import BasicVSR  # noqa: E402
from spynet_bench import TorchSpyNet, timed, torch_warp  # noqa: E402

PEAK_TFLOPS = 157.3
PEAK_TFLOPS_BF16 = 2500.0


def other_basicvsr(tree):
    """BasicVSR of another checkout of this project, from a second copy of the package under the name ``sr_other_tree`` (relative
    imports keep it on its own modules and its own library)."""
    pkg = os.path.join(tree, 'image_restoration_amd')
    spec = importlib.util.spec_from_file_location('sr_other_tree', os.path.join(pkg, '__init__.py'), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules['sr_other_tree'] = mod
    spec.loader.exec_module(mod)
    arch = importlib.import_module('sr_other_tree.archs.basicvsr_arch')
    lib = importlib.import_module('sr_other_tree._lib')
    assert os.path.realpath(lib.LIB_PATH).startswith(os.path.realpath(tree)), lib.LIB_PATH
    return arch.BasicVSR


def per_layer_trunk(net, trunk, src, out):
    """ConvResidualBlocks with every conv issued through hip_ops.conv3x3; the last one writes the window ``out``."""
    first = H.cached_pack('bench first', trunk.main[0].weight, trunk.main[0].bias,
                          lambda: H.PackedConv(trunk.main[0].weight, trunk.main[0].bias, first_seg=3, seg=net.num_feat))
    blocks = list(trunk.main[2])
    x = H.conv3x3(src, first, out if not blocks else None, act_slope=0.1)
    for k, blk in enumerate(blocks):
        t = H.conv3x3(x, net.packed(blk.conv1), act_slope=0.0)
        x = H.conv3x3(t, net.packed(blk.conv2), out if k + 1 == len(blocks) else None, res1=x, beta1=1.0)
    return x


def per_layer_forward(net, x):
    """BasicVSR.forward as shipped (sr_vsr_prop_input_f32, windows of the per-clip tensor, the same reconstruction) except that
    every trunk conv is issued from Python through hip_ops.conv3x3: only how the convs are issued differs from the product."""
    ff, fb = net.get_flow(x)
    b, n, _, h, w = x.shape
    fbk = net.num_feat // 8
    feats = torch.empty((n * b, 2 * fbk, h, w, 8), device=x.device)
    tin = torch.empty((b, 1 + fbk, h, w, 8), device=x.device)
    frame_out, warp_out, src = H.CB8(tin, 0, 1), H.CB8(tin, 1, fbk), H.CB8(tin)
    for trunk, flows, cb0, order in ((net.backward_trunk, fb, 0, range(n - 1, -1, -1)), (net.forward_trunk, ff, fbk, range(n))):
        prev, last = None, None
        for i in order:
            H.vsr_prop_input(x[:, i], prev, None if prev is None else flows[:, min(i, last)], warp_out, frame_out)
            prev, last = per_layer_trunk(net, trunk, src, H.CB8(feats[i * b:(i + 1) * b], cb0, fbk)), i
    frames = x.transpose(0, 1).reshape(n * b, 3, h, w)
    y = torch.empty((n * b, 3, 4 * h, 4 * w), device=x.device)
    net._reconstruct(feats, frames, y)
    return y.view(n, b, 3, 4 * h, 4 * w).transpose(0, 1)


class TorchBasicVSR(nn.Module):
    """The same network as plain PyTorch modules, sharing the HIP network's parameters."""

    def __init__(self, net):
        super().__init__()
        self.num_feat = net.num_feat
        self.spynet = TorchSpyNet(net.spynet)

        def conv(p, k=3):
            c = nn.Conv2d(p.in_channels, p.out_channels, k, 1, k // 2)
            c.weight, c.bias = p.weight, p.bias
            return c

        def trunk(t):
            return conv(t.main[0]), nn.ModuleList(nn.ModuleList([conv(blk.conv1), conv(blk.conv2)]) for blk in t.main[2])
        self.b_first, self.b_blocks = trunk(net.backward_trunk)
        self.f_first, self.f_blocks = trunk(net.forward_trunk)
        self.fusion, self.upconv1, self.upconv2 = conv(net.fusion, 1), conv(net.upconv1), conv(net.upconv2)
        self.conv_hr, self.conv_last = conv(net.conv_hr), conv(net.conv_last)

    @staticmethod
    def run_trunk(first, blocks, x):
        x = F.leaky_relu(first(x), 0.1)
        for c1, c2 in blocks:
            x = x + c2(F.relu(c1(x)))
        return x

    def forward(self, x):
        b, n, c, h, w = x.shape
        x_1, x_2 = x[:, :-1].reshape(-1, c, h, w), x[:, 1:].reshape(-1, c, h, w)
        fb = self.spynet(x_1, x_2).view(b, n - 1, 2, h, w)
        ff = self.spynet(x_2, x_1).view(b, n - 1, 2, h, w)
        out_l, feat = [None] * n, x.new_zeros(b, self.num_feat, h, w)
        for i in range(n - 1, -1, -1):
            if i < n - 1:
                feat = torch_warp(feat, fb[:, i].permute(0, 2, 3, 1), 'zeros')
            feat = self.run_trunk(self.b_first, self.b_blocks, torch.cat([x[:, i], feat], 1))
            out_l[i] = feat
        feat = torch.zeros_like(feat)
        for i in range(n):
            if i > 0:
                feat = torch_warp(feat, ff[:, i - 1].permute(0, 2, 3, 1), 'zeros')
            feat = self.run_trunk(self.f_first, self.f_blocks, torch.cat([x[:, i], feat], 1))
            out = F.leaky_relu(self.fusion(torch.cat([out_l[i], feat], 1)), 0.1)
            out = F.leaky_relu(F.pixel_shuffle(self.upconv1(out), 2), 0.1)
            out = F.leaky_relu(F.pixel_shuffle(self.upconv2(out), 2), 0.1)
            out = self.conv_last(F.leaky_relu(self.conv_hr(out), 0.1))
            out_l[i] = out + F.interpolate(x[:, i], scale_factor=4, mode='bilinear', align_corners=False)
        return torch.stack(out_l, 1)


def burst(fn, calls=50):
    """Milliseconds per call of ``calls`` back-to-back calls between two device events (after a few warm-up calls)."""
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def kept_bytes(keep):
    """Bytes of the tensors a training forward kept (BasicVSR.run_forward's ``keep``), each storage once."""
    seen, total = set(), 0

    def walk(v):
        nonlocal total
        if isinstance(v, torch.Tensor):
            if v.untyped_storage().data_ptr() not in seen:
                seen.add(v.untyped_storage().data_ptr())
                total += v.untyped_storage().nbytes()
        elif hasattr(v, 'buf'):
            walk(v.buf)
        elif isinstance(v, dict):
            for u in v.values():
                walk(u)
        elif isinstance(v, (list, tuple)):
            for u in v:
                walk(u)
    walk({k: v for k, v in keep.items() if k not in ('x', 'flows_forward', 'flows_backward')})
    return total


def backward_bench(args, dev):
    """--backward: see the module docstring."""
    import ctypes as C
    from image_restoration_amd import _lib
    lib = _lib.load()
    n, h, w, b, nf, nb = 15, 64, 64, args.batch, 64, args.num_block
    torch.manual_seed(0)
    net = BasicVSR(num_feat=nf, num_block=nb).to(dev).train().set_autograd(True)
    ref = TorchBasicVSR(net).to(dev).train()
    x = torch.rand(b, n, 3, h, w, device=dev)
    g = torch.randn(b, n, 3, 4 * h, 4 * w, device=dev)
    params = list(net.parameters())

    def step(model):
        for q in params:
            q.grad = None
        (model(x) * g).sum().backward()
    step(net)
    mine = [q.grad.clone() for q in params]
    step(ref)
    rel = max(float((a - q.grad).norm() / q.grad.norm()) for a, q in zip(mine, params))
    for _ in range(args.warmup):
        step(net)
        step(ref)
    ms = {'product': [], 'torch': []}
    for _ in range(args.reps):
        ms['product'].append(timed(lambda: step(net), 1, 0))
        ms['torch'].append(timed(lambda: step(ref), 1, 0))
    keep = {}
    with torch.no_grad():
        ff, fb = net.get_flow(x)
        net.run_forward(x, ff, fb, keep=keep)
    kept = kept_bytes(keep)
    del keep
    cap = 1 << 16
    _lib.check(lib.sr_profile_start(cap), 'sr_profile_start')
    try:
        step(net)
        torch.cuda.synchronize()
    finally:
        recs = (_lib.LaunchRecord * cap)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, cap, C.byref(cnt)), 'sr_profile_stop')
    split = {}
    for i in range(min(cnt.value, cap)):
        name = lib.sr_kernel_name(recs[i].kernel_id).decode() or f'id {recs[i].kernel_id}'
        e = split.setdefault(name, dict(kernel_id=int(recs[i].kernel_id), launches=0, ms=0.0))
        e['launches'] += 1
        e['ms'] += float(recs[i].ms)
    total = sum(e['ms'] for e in split.values())
    steps = sum(e['ms'] for e in split.values() if e['kernel_id'] in (159, 178))
    r = dict(case=f'{b} clips of {n} frames {h}x{w}, num_feat {nf}, num_block {nb}', product_ms=statistics.median(ms['product']),
             product_ms_min=min(ms['product']), product_ms_max=max(ms['product']), torch_ms=statistics.median(ms['torch']),
             torch_ms_min=min(ms['torch']), torch_ms_max=max(ms['torch']), max_rel_l2_gradients=rel, kept_bytes_per_clip=kept / b,
             profiled_launches=int(cnt.value), profiled_ms=total, step_kernels_share=steps / total if total else None, split=split)
    r['torch_over_product'] = r['torch_ms'] / r['product_ms']
    print(f'{r["case"]}: forward + backward product {r["product_ms"]:.1f} ms [{r["product_ms_min"]:.1f}, {r["product_ms_max"]:.1f}], torch '
          f'{r["torch_ms"]:.1f} ms [{r["torch_ms_min"]:.1f}, {r["torch_ms_max"]:.1f}], torch / product {r["torch_over_product"]:.2f}; '
          f'max rel L2 of the parameter gradients {rel:.2e}; kept {kept / b / 2 ** 20:.0f} MiB per clip')
    print(f'    launch profile of one step: {cnt.value} launches, {total:.1f} ms in kernels, step kernels (159, 178) '
          f'{100 * steps / max(total, 1e-30):.1f} %')
    for name, e in sorted(split.items(), key=lambda kv: -kv[1]['ms']):
        print(f'    {name:44s} id {e["kernel_id"]:3d}  {e["launches"]:6d} launches {e["ms"]:9.2f} ms {100 * e["ms"] / max(total, 1e-30):5.1f} %')
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(dict(backward=True, reps=args.reps, warmup=args.warmup, rows=[r]), f, indent=1)


def deterministic_bench(args, dev):
    """--backward --deterministic: see the module docstring."""
    import ctypes as C
    from image_restoration_amd import _lib
    lib = _lib.load()
    n, h, w, b, nf, nb = 15, 64, 64, args.batch, 64, args.num_block
    torch.manual_seed(0)
    net = BasicVSR(num_feat=nf, num_block=nb).to(dev).train()
    x = torch.rand(b, n, 3, h, w, device=dev)
    g = torch.randn(b, n, 3, 4 * h, 4 * w, device=dev)
    params = list(net.parameters())
    modes = (('atomic', False), ('deterministic', True))

    def step(deterministic):
        net.set_autograd(True, deterministic=deterministic)
        for q in params:
            q.grad = None
        (net(x) * g).sum().backward()
    grads = {}
    for name, det in modes:
        step(det)
        grads[name] = [q.grad.clone() for q in params]
    step(True)
    same = all(torch.equal(a, q.grad) for a, q in zip(grads['deterministic'], params))
    rel = max(float((a - d).norm() / d.norm()) for a, d in zip(grads['atomic'], grads['deterministic']))
    for _ in range(args.warmup):
        for _, det in modes:
            step(det)
    ms = {name: [] for name, _ in modes}
    for _ in range(args.reps):                      # rows alternate: a drift of the clock reaches both alike
        for name, det in modes:
            ms[name].append(timed(lambda: step(det), 1, 0))
    kernels = {}
    cap = 1 << 16
    for name, det in modes:
        _lib.check(lib.sr_profile_start(cap), 'sr_profile_start')
        try:
            step(det)
            torch.cuda.synchronize()
        finally:
            recs = (_lib.LaunchRecord * cap)()
            cnt = C.c_int(0)
            _lib.check(lib.sr_profile_stop(recs, cap, C.byref(cnt)), 'sr_profile_stop')
        per = {}
        for i in range(min(cnt.value, cap)):
            if recs[i].kernel_id in (178, 180, 181, 182):
                e = per.setdefault(int(recs[i].kernel_id), dict(name=lib.sr_kernel_name(recs[i].kernel_id).decode(), launches=0, ms=0.0))
                e['launches'] += 1
                e['ms'] += float(recs[i].ms)
        kernels[name] = per
    rows = []
    for name, _ in modes:
        v = ms[name]
        rows.append(dict(mode=name, step_ms=statistics.median(v), step_ms_min=min(v), step_ms_max=max(v), step_input_kernels=kernels[name],
                         step_input_ms=sum(e['ms'] for e in kernels[name].values())))
    case = f'{b} clips of {n} frames {h}x{w}, num_feat {nf}, num_block {nb}'
    print(f'{case}: two deterministic backward passes bit-identical: {same}; max rel L2 atomic vs deterministic gradients {rel:.2e}')
    for r in rows:
        print(f'    {r["mode"]:14s} forward + backward {r["step_ms"]:.1f} ms [{r["step_ms_min"]:.1f}, {r["step_ms_max"]:.1f}]; step-input adjoint '
              f'{r["step_input_ms"]:.3f} ms per step: ' + ', '.join(f'{e["name"]} (id {k}) {e["launches"]} launches {e["ms"]:.3f} ms'
                                                                    for k, e in sorted(r['step_input_kernels'].items())))
    print(f'    deterministic / atomic step time {rows[1]["step_ms"] / rows[0]["step_ms"]:.4f}')
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(dict(backward=True, deterministic=True, case=case, reps=args.reps, warmup=args.warmup, bit_identical=same,
                           max_rel_l2_atomic_vs_deterministic=rel, rows=rows), f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--num-block', type=int, default=30)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--wino-off', action='store_true', help='sr_dev_set_wino_f32(0): the product path on the direct kernels too')
    ap.add_argument('--other-tree', default=None, help='root of another built checkout of this project: its fp32 and bf16 products as further rows')
    ap.add_argument('--backward', action='store_true', help='time forward + backward at the REDS recipe\'s shape instead, against '
                    'PyTorch-ROCm autograd, with the per-kernel split')
    ap.add_argument('--batch', type=int, default=4, help='clips per step of --backward')
    ap.add_argument('--deterministic', action='store_true', help='with --backward: the deterministic backward (set_autograd(True, '
                    'deterministic=True)) against the atomic one in one process, rows alternating')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('basicvsr_bench needs a GPU: timings are device timings')
    dev = torch.device('cuda:0')
    if args.deterministic and not args.backward:
        raise SystemExit('--deterministic times the backward: give --backward too')
    if args.backward:
        return deterministic_bench(args, dev) if args.deterministic else backward_bench(args, dev)
    if args.wino_off:
        from image_restoration_amd import _lib
        _lib.load().sr_dev_set_wino_f32(0)
    torch.manual_seed(0)
    net = BasicVSR(num_feat=64, num_block=args.num_block).to(dev).eval()
    ref = TorchBasicVSR(net).to(dev).eval()
    net16 = BasicVSR(num_feat=64, num_block=args.num_block).to(dev).eval().set_compute_dtype('bf16')
    net16.load_state_dict(net.state_dict())
    other = other16 = None
    if args.other_tree:
        cls = other_basicvsr(args.other_tree)
        other = cls(num_feat=64, num_block=args.num_block).to(dev).eval()
        other.load_state_dict(net.state_dict())
        other16 = cls(num_feat=64, num_block=args.num_block).to(dev).eval().set_compute_dtype('bf16')
        other16.load_state_dict(net.state_dict())
    nf, nb = 64, args.num_block
    rows = []
    with torch.no_grad():
        for n, h, w in ((15, 180, 320), (7, 64, 112)):
            x = torch.rand(1, n, 3, h, w, device=dev)
            y = net(x)
            d_layer, d_torch = float((per_layer_forward(net, x) - y).abs().max()), float((ref(x) - y).abs().max())
            variants = (('product', lambda: net(x)), ('per-layer', lambda: per_layer_forward(net, x)), ('torch', lambda: ref(x)),
                        ('bf16', lambda: net16(x)))
            y16 = net16(x)
            d_bf16, d_other, d_other16 = float((y16 - y).abs().max()), None, None
            if other is not None:
                variants += (('other fp32', lambda: other(x)), ('other bf16', lambda: other16(x)))
                d_other, d_other16 = float((other(x) - y).abs().max()), float((other16(x) - y16).abs().max())
            # interleaved at the level of single forwards: a round runs every variant once; median over the rounds
            for _ in range(args.warmup):
                for _, fn in variants:
                    fn()
            ms = {k: [] for k, _ in variants}
            for _ in range(args.reps):
                for k, fn in variants:
                    ms[k].append(timed(fn, 1, 0))
            r = dict(case=f'{n} frames {h}x{w}', frames=n, max_abs_diff_per_layer=d_layer, max_abs_diff_torch=d_torch,
                     max_abs_diff_bf16=d_bf16, max_abs_diff_other=d_other, max_abs_diff_other_bf16=d_other16)
            for k, _ in variants:
                r[k + '_ms'] = statistics.median(ms[k])
                r[k + '_ms_per_frame'] = statistics.median(ms[k]) / n
                r[k + '_ms_min'], r[k + '_ms_max'] = min(ms[k]), max(ms[k])
            # one trunk call and one step input alone
            tin = torch.randn(1, 9, h, w, 8, device=dev)
            tin[:, 0, :, :, 3:] = 0
            out = H.CB8.empty(1, nf, h, w, dev)
            t_trunk = burst(lambda: net.forward_trunk.run(H.CB8(tin), out))
            flops = 2.0 * 9 * h * w * nf * ((3 + nf) + 2 * nb * nf)
            prev, flow = H.CB8(torch.randn(1, 8, h, w, 8, device=dev)), torch.randn(1, 2, h, w, device=dev) * 4
            t_prop = burst(lambda: H.vsr_prop_input(x[:, 0], prev, flow, H.CB8(tin, 1, 8), H.CB8(tin, 0, 1)))
            nbytes = 4.0 * h * w * (5 * nf + 2 + 3 + 8)
            r.update(trunk_ms=t_trunk, trunk_tflops=flops / t_trunk / 1e9, trunk_of_peak=flops / t_trunk / 1e9 / PEAK_TFLOPS,
                     trunk_launches=1 + 2 * nb, prop_input_ms=t_prop, prop_input_gbytes_per_s=nbytes / t_prop / 1e6)
            # the same two on the bf16 entry points
            tin16 = torch.randn(1, 5, h, w, 16, device=dev).bfloat16()
            tin16[:, 0, :, :, 3:] = 0
            out16 = H.CB16.empty(1, nf, h, w, dev)
            t_trunk16 = burst(lambda: net16.forward_trunk.run(H.CB16(tin16), out16))
            prev16 = H.CB16(torch.randn(1, 4, h, w, 16, device=dev).bfloat16())
            t_prop16 = burst(lambda: H.vsr_prop_input_bf16(x[:, 0], prev16, flow, H.CB16(tin16, 1, 4), H.CB16(tin16, 0, 1)))
            nbytes16 = 1.0 * h * w * (5 * 2 * nf + 8 + 12 + 32)
            r.update(trunk_bf16_ms=t_trunk16, trunk_bf16_tflops=flops / t_trunk16 / 1e9,
                     trunk_bf16_of_peak=flops / t_trunk16 / 1e9 / PEAK_TFLOPS_BF16, prop_input_bf16_ms=t_prop16,
                     prop_input_bf16_gbytes_per_s=nbytes16 / t_prop16 / 1e6)
            rows.append(r)
    for r in rows:
        print(f'{r["case"]}: product {r["product_ms"]:.2f} ms ({r["product_ms_per_frame"]:.2f} / frame), per-layer '
              f'{r["per-layer_ms"]:.2f} ms ({r["per-layer_ms_per_frame"]:.2f}), torch {r["torch_ms"]:.2f} ms ({r["torch_ms_per_frame"]:.2f}); '
              f'max|diff| per-layer {r["max_abs_diff_per_layer"]:.2e} torch {r["max_abs_diff_torch"]:.2e}')
        print(f'    trunk call ({r["trunk_launches"]} launches) {r["trunk_ms"]:.3f} ms = {r["trunk_tflops"]:.1f} TFLOP/s '
              f'({r["trunk_of_peak"]:.2f} of peak); prop input {1000 * r["prop_input_ms"]:.1f} us = {r["prop_input_gbytes_per_s"]:.0f} GB/s')
        print(f'    bf16 {r["bf16_ms"]:.2f} ms ({r["bf16_ms_per_frame"]:.2f} / frame) [{r["bf16_ms_min"]:.2f}, {r["bf16_ms_max"]:.2f}]; product '
              f'rounds [{r["product_ms_min"]:.2f}, {r["product_ms_max"]:.2f}]; max|bf16 - fp32| {r["max_abs_diff_bf16"]:.2e}')
        if 'other fp32_ms' in r:
            print(f'    other fp32 {r["other fp32_ms"]:.2f} ms [{r["other fp32_ms_min"]:.2f}, {r["other fp32_ms_max"]:.2f}]; max|other - '
                  f'product| {r["max_abs_diff_other"]:.2e}')
            print(f'    other bf16 {r["other bf16_ms"]:.2f} ms [{r["other bf16_ms_min"]:.2f}, {r["other bf16_ms_max"]:.2f}]; max|other bf16 - '
                  f'bf16| {r["max_abs_diff_other_bf16"]:.2e}')
        print(f'    bf16 trunk call {r["trunk_bf16_ms"]:.3f} ms = {r["trunk_bf16_tflops"]:.1f} TFLOP/s ({r["trunk_bf16_of_peak"]:.3f} of the bf16 '
              f'peak); bf16 prop input {1000 * r["prop_input_bf16_ms"]:.1f} us = {r["prop_input_bf16_gbytes_per_s"]:.0f} GB/s')
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(dict(num_block=nb, wino_off=args.wino_off, reps=args.reps, warmup=args.warmup, peak_tflops=PEAK_TFLOPS, rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
