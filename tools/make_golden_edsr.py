#!/usr/bin/env python3
"""Writes tests/golden/g_y_edsr.npz: the reference's EDSR (basicsr/archs/edsr_arch.py) and SRModel run in place on seeded
weights and inputs.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_edsr.py [--out tests/golden/g_y_edsr.npz]

The reference modules are imported from the read-only reference tree through tools/ref_loader.py's synthetic packages;
nothing of them is copied.  Weights come from synth.edsr_state_dict (numpy PCG64, non-zero biases) and are loaded with
load_state_dict(strict=True).  Contents:

* ``keys_{M,L}x{2,3,4}`` / ``shapes_*``: state_dict keys and shapes of the six product configs (options/*/EDSR);
* ``init_mean`` / ``init_std``: per-tensor statistics of a freshly built Mx4 under torch.manual_seed(0);
* ``x{2,3,4}_*`` (the networks of SMALL below, batch 2 on ragged sizes): the input ``x``; ``y64`` the float64 output stored as
  float32; ``y32_err`` = max|y32 - y64| of the reference's own float32 run; ``R`` a seeded upstream gradient; ``dx64`` and
  ``grad64.<name>`` the gradients of sum(out * R) by autograd in float64, stored as float32; ``dx32_err`` and
  ``grad32_err.<name>`` the max-abs distances of the float32 run's gradients from them;
* ``SRModel[64]_*``: three optimize_parameters iterations (TRAIN_G, L1, Adam) in float32 and float64 with the quantities
  tools/make_golden_msrresnet.py stores (logs, learning rates, parameter checksums, Adam moment norms, final conv_last weight).
"""
import argparse
import importlib
import os
import sys
from collections import OrderedDict as OD

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_loader  # noqa: E402
from image_restoration_amd.utils import synth  # noqa: E402

PRODUCT = {f'{m}x{s}': dict(num_in_ch=3, num_out_ch=3, num_feat=nf, num_block=nb, upscale=s, res_scale=rs, img_range=255.,
                            rgb_mean=[0.4488, 0.4371, 0.4040])
           for m, nf, nb, rs in (('M', 64, 16, 1), ('L', 256, 32, 0.1)) for s in (2, 3, 4)}
# upscale -> (network, LR size, weight seed)
SMALL = {
    2: (dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=2, upscale=2, res_scale=1), (13, 17), 202),
    3: (dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=2, upscale=3, res_scale=0.1, img_range=1.0,
             rgb_mean=(0.5, 0.25, 0.125)), (9, 11), 203),
    4: (dict(num_in_ch=3, num_out_ch=3, num_feat=32, num_block=3, upscale=4, res_scale=0.1), (7, 10), 204),
}
TRAIN_G = dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=2, upscale=4, res_scale=0.1)
TRAIN_SEED = 281


def _checksums(net):
    return np.array([[float(p.detach().double().sum()), float(p.detach().double().norm())] for _, p in net.named_parameters()])


def train_opt():
    opt = OD(name='golden', model_type='SRModel', scale=4, num_gpu=0, manual_seed=0, is_train=True, dist=False, rank=0,
             world_size=1)
    opt['network_g'] = OD(type='EDSR', **TRAIN_G)
    opt['path'] = OD(pretrain_network_g=None, strict_load_g=True, resume_state=None)
    tr = OD(ema_decay=0.9)
    tr['optim_g'] = OD(type='Adam', lr=1e-3, weight_decay=0, betas=[0.9, 0.99])
    tr['scheduler'] = OD(type='MultiStepLR', milestones=[2, 3], gamma=0.5)
    tr['total_iter'] = 4
    tr['warmup_iter'] = -1
    tr['pixel_opt'] = OD(type='L1Loss', loss_weight=1.0, reduction='mean')
    opt['train'] = tr
    return opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g_y_edsr.npz'))
    args = ap.parse_args()
    ref = ref_loader.load_reference()
    arch = importlib.import_module('basicsr.archs.edsr_arch')   # registers EDSR with the reference's registry
    a = {}
    for name, cfg in PRODUCT.items():
        net = arch.EDSR(**cfg)
        a[f'keys_{name}'] = np.array(list(net.state_dict()))
        a[f'shapes_{name}'] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in net.state_dict().values()], np.int64)
    torch.manual_seed(0)
    net = arch.EDSR(**PRODUCT['Mx4'])
    a['init_mean'] = np.array([float(v.double().mean()) for v in net.state_dict().values()])
    a['init_std'] = np.array([float(v.double().std()) for v in net.state_dict().values()])

    for s, (cfg, (h, w), seed) in SMALL.items():
        sd = synth.edsr_state_dict(seed, **cfg)
        x = synth.uniform_input(seed + 10, (2, 3, h, w))
        R = np.random.default_rng(seed + 20).standard_normal((2, 3, s * h, s * w)).astype(np.float32)
        a[f'x{s}_x'], a[f'x{s}_R'] = x, R
        run = {}
        for dt in (torch.float64, torch.float32):
            net = arch.EDSR(**cfg).to(dt)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            xt = torch.from_numpy(x).to(dt).requires_grad_(True)
            y = net(xt)
            (y * torch.from_numpy(R).to(dt)).sum().backward()
            run[dt] = (y.detach().double(), xt.grad.double(), {k: p.grad.double() for k, p in net.named_parameters()})
        y64, dx64, g64 = run[torch.float64]
        y32, dx32, g32 = run[torch.float32]
        a[f'x{s}_y64'] = y64.float().numpy()
        a[f'x{s}_y32_err'] = np.array(float((y32 - y64).abs().max()))
        a[f'x{s}_dx64'] = dx64.float().numpy()
        a[f'x{s}_dx32_err'] = np.array(float((dx32 - dx64).abs().max()))
        for k in g64:
            a[f'x{s}_grad64.{k}'] = g64[k].float().numpy()
            a[f'x{s}_grad32_err.{k}'] = np.array(float((g32[k] - g64[k]).abs().max()))

    for dt in (torch.float32, torch.float64):
        mt = 'SRModel' if dt == torch.float32 else 'SRModel64'
        model = ref.SRModel(train_opt())
        for net in (model.net_g, getattr(model, 'net_g_ema', None)):
            if net is not None:
                net.to(dt)
        model.net_g.load_state_dict({k: torch.from_numpy(v) for k, v in synth.edsr_state_dict(TRAIN_SEED, **TRAIN_G).items()},
                                    strict=True)
        model.model_ema(0)
        logs, lrs = [], []
        for it in range(1, 4):
            model.update_learning_rate(it, warmup_iter=-1)
            lrs.append(model.get_current_learning_rate()[0])
            lq = torch.from_numpy(synth.uniform_input(900 + it, (4, 3, 32, 32))).to(dt)
            gt = torch.from_numpy(synth.uniform_input(950 + it, (4, 3, 128, 128))).to(dt)
            model.feed_data({'lq': lq, 'gt': gt})
            model.optimize_parameters(it)
            log = model.get_current_log()
            logs.append([log[k] for k in sorted(log)])
            a[f'{mt}_g_checksum_it{it}'] = _checksums(model.net_g)
        a[f'{mt}_log_keys'] = np.array(sorted(log))
        a[f'{mt}_logs'] = np.array(logs, dtype=np.float64)
        a[f'{mt}_lrs'] = np.array(lrs, dtype=np.float64)
        a[f'{mt}_ema_checksum'] = _checksums(model.net_g_ema)
        st = model.optimizer_g.state_dict()['state']
        a[f'{mt}_adam_g_exp_avg'] = np.array([float(st[i]['exp_avg'].double().norm()) for i in sorted(st)])
        a[f'{mt}_adam_g_exp_avg_sq'] = np.array([float(st[i]['exp_avg_sq'].double().norm()) for i in sorted(st)])
        a[f'{mt}_g_conv_last_weight'] = model.net_g.conv_last.weight.detach().double().numpy().copy()

    np.savez_compressed(args.out, **a)
    print(f'{args.out}: {os.path.getsize(args.out) / 1024:.1f} KiB, {len(a)} arrays')


if __name__ == '__main__':
    main()
