#!/usr/bin/env python3
"""Writes tests/golden/g_x_gfpgan.npz: the reference's GFPGANv1OCR (basicsr/archs/gfpganv1_ocr_arch.py with the StyleGAN2
modules of stylegan2_ocr_arch.py) run in place on seeded weights and inputs.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_gfpgan.py [--out tests/golden/g_x_gfpgan.npz]

The reference modules are imported from the read-only reference tree through tools/ref_loader.py's synthetic packages;
nothing of them is copied.  The reference's fused bias + LeakyReLU op has no CPU path (its compiled extension is absent), so a
``basicsr.ops.fused_act`` module of this tool's own is registered first: ``lrelu(x + bias.view(1, -1, 1, ...), slope) * scale``,
written from that definition.  ``upfirdn2d`` runs on its own native torch path on the CPU.  Weights come from
synth.gfpgan_state_dict (numpy PCG64; non-zero noise strengths, SFT scale biases away from 1) and load with strict=True.
Contents, per small config ``{c}`` in CONFIGS (batch 2 of different images in [-1, 1], stored noise):

* ``{c}_x``, ``{c}_seed``, ``{c}_weights_sha256``;
* ``{c}_image``, ``{c}_rgb{i}``, ``{c}_style_code``, ``{c}_cond{k}`` (scale, shift, scale, ...): the float64 run, stored as float32;
* ``{c}_image32_err`` / ``{c}_rgb32_err``: the max-abs distance of the reference's own float32 CPU run from its float64 run;
* ``keys_{name}`` / ``shapes_{name}``: state_dict keys (order included) and shapes (padded to 5 dims) of the product configs
  ``sq256_mlp4``, ``sq256_mlp8`` and ``rect256x64``, and ``init_mean`` / ``init_std`` / ``init_requires_grad`` of ``sq256_mlp4``
  under torch.manual_seed(0).
"""
import argparse
import hashlib
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_loader  # noqa: E402
from image_restoration_amd.utils import synth  # noqa: E402

BASE = dict(resample_kernel=(1, 3, 3, 1), decoder_load_path=None, fix_decoder=True, lr_mlp=0.01)
CONFIGS = {
    'sq': dict(input_width=32, input_height=32, num_style_feat=64, channel_multiplier=0.5, narrow=0.0625, num_mlp=2,
               input_is_latent=True, different_w=True, sft_half=True),
    'rect': dict(input_width=64, input_height=16, num_style_feat=32, channel_multiplier=0.5, narrow=0.0625, num_mlp=2,
                 input_is_latent=True, different_w=True, sft_half=True),
    'mlp': dict(input_width=16, input_height=16, num_style_feat=32, channel_multiplier=1, narrow=0.0625, num_mlp=3,
                input_is_latent=False, different_w=False, sft_half=False),
}
SEEDS = {'sq': 501, 'rect': 502, 'mlp': 503}
PRODUCT = {
    'sq256_mlp4': dict(input_width=256, input_height=256, num_style_feat=256, channel_multiplier=0.5, narrow=1, num_mlp=4,
                       input_is_latent=True, different_w=True, sft_half=True),
    'sq256_mlp8': dict(input_width=256, input_height=256, num_style_feat=256, channel_multiplier=0.5, narrow=1, num_mlp=8,
                       input_is_latent=True, different_w=True, sft_half=True),
    'rect256x64': dict(input_width=256, input_height=64, num_style_feat=256, channel_multiplier=0.5, narrow=1, num_mlp=4,
                       input_is_latent=True, different_w=True, sft_half=True),
}


def weights_sha256(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v, np.float32).tobytes())
    return h.hexdigest()


def install_fused_act():
    """basicsr.ops.fused_act without its compiled extension: out = lrelu(x + bias along dim 1, slope) * scale."""
    mod = types.ModuleType('basicsr.ops.fused_act')

    def fused_leaky_relu(x, bias, negative_slope=0.2, scale=2 ** 0.5):
        return F.leaky_relu(x + bias.view(1, -1, *([1] * (x.dim() - 2))), negative_slope) * scale

    class FusedLeakyReLU(torch.nn.Module):
        def __init__(self, channel, negative_slope=0.2, scale=2 ** 0.5):
            super().__init__()
            self.bias = torch.nn.Parameter(torch.zeros(channel))
            self.negative_slope, self.scale = negative_slope, scale

        def forward(self, x):
            return fused_leaky_relu(x, self.bias, self.negative_slope, self.scale)

    mod.fused_leaky_relu, mod.FusedLeakyReLU = fused_leaky_relu, FusedLeakyReLU
    sys.modules['basicsr.ops.fused_act'] = mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g_x_gfpgan.npz'))
    args = ap.parse_args()
    ref_loader.load_reference()
    install_fused_act()
    arch = importlib.import_module('basicsr.archs.gfpganv1_ocr_arch')
    a = {}
    for name, cfg in PRODUCT.items():
        net = arch.GFPGANv1OCR(**BASE, **cfg)
        sd = net.state_dict()
        a[f'keys_{name}'] = np.array(list(sd))
        a[f'shapes_{name}'] = np.array([list(v.shape) + [0] * (5 - v.dim()) for v in sd.values()], np.int64)
    torch.manual_seed(0)
    net = arch.GFPGANv1OCR(**BASE, **PRODUCT['sq256_mlp4'])
    sd = net.state_dict()
    a['init_mean'] = np.array([float(v.double().mean()) for v in sd.values()])
    a['init_std'] = np.array([float(v.double().std()) if v.numel() > 1 else 0.0 for v in sd.values()])
    req = dict((k, p.requires_grad) for k, p in net.named_parameters())
    a['init_requires_grad'] = np.array([req.get(k, False) for k in sd])

    for c, cfg in CONFIGS.items():
        sdn = synth.gfpgan_state_dict(SEEDS[c], **cfg)
        x = synth.signed_input(SEEDS[c] + 10, (2, 3, cfg['input_height'], cfg['input_width']))
        a[f'{c}_x'], a[f'{c}_seed'] = x, np.array(SEEDS[c])
        a[f'{c}_weights_sha256'] = np.array(weights_sha256(sdn))
        outs = {}
        for dt in (torch.float32, torch.float64):
            net = arch.GFPGANv1OCR(**BASE, **cfg).to(dt)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=True)
            conds = []
            hooks = [m.register_forward_hook(lambda m, i, o: conds.append(o.detach().clone()))
                     for pair in zip(net.condition_scale, net.condition_shift) for m in pair]
            styles = []
            hooks.append(net.final_linear.register_forward_hook(lambda m, i, o: styles.append(o.detach().clone())))
            with torch.no_grad():
                img, rgbs = net(torch.from_numpy(x).to(dt), return_rgb=True, randomize_noise=False)
            for h in hooks:
                h.remove()
            outs[dt] = (img, rgbs, styles[0], conds)
        img64, rgb64, st64, cond64 = outs[torch.float64]
        img32, rgb32, _, _ = outs[torch.float32]
        a[f'{c}_image'] = img64.float().numpy()
        a[f'{c}_image32_err'] = np.array(float((img32.double() - img64).abs().max()))
        a[f'{c}_rgb32_err'] = np.array(max(float((r32.double() - r64).abs().max()) for r32, r64 in zip(rgb32, rgb64)))
        for i, r in enumerate(rgb64):
            a[f'{c}_rgb{i}'] = r.float().numpy()
        a[f'{c}_style_code'] = st64.float().numpy()
        for k, t in enumerate(cond64):
            a[f'{c}_cond{k}'] = t.float().numpy()
        print(f'{c}: image {tuple(img64.shape)} max|y| {float(img64.abs().max()):.3f}  |y32 - y64| {float(a[f"{c}_image32_err"]):.2e}  '
              f'rgb {float(a[f"{c}_rgb32_err"]):.2e}')
    np.savez_compressed(args.out, **a)
    print(f'{args.out}: {os.path.getsize(args.out) / 1024:.1f} KiB, {len(a)} arrays')


if __name__ == '__main__':
    main()
