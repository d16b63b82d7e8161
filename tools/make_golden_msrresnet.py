#!/usr/bin/env python3
"""Writes tests/golden/g_u_msrresnet.npz: the reference's MSRResNet (basicsr/archs/srresnet_arch.py), SRModel and SRGANModel
run in place on seeded weights and inputs.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_msrresnet.py [--out tests/golden/g_u_msrresnet.npz]

The reference modules are imported from the read-only reference tree through tools/ref_loader.py's synthetic packages;
nothing of them is copied.  Weights come from synth.msrresnet_state_dict (numpy PCG64) and are loaded with
load_state_dict(strict=True).  Contents:

* ``keys_x{2,3,4}`` / ``shapes_x{2,3,4}``: state_dict keys and shapes of the default net (nf 64, nb 16) per upscale;
* ``fwd_x{s}_*``: nf 16, nb 2, batch 2 on ragged LR sizes: x, y (float32 and float64 runs); then, against a seeded upstream
  gradient ``gy``, dL/dx and every parameter gradient (``grad64.<name>``) by autograd through the reference in float64,
  stored rounded to float32;
* ``big_*``: the default net (x4) on one 32x32 input: x and y only.  Its weights are synth.msrresnet_state_dict(seed)
  and the tests regenerate them, checking the stored SHA-256 of their bytes;
* ``{SRModel,SRGANModel}[64]_*``: three optimize_parameters iterations (MSRResNet nf 16, nb 2, x4; VGGStyleDiscriminator128
  nf 8 with a vanilla GAN loss and no perceptual term, whose VGG needs torchvision), in float32 and float64, with the
  quantities tools/make_goldens.py g_i stores (logs, learning rates, parameter checksums, Adam moment norms, final
  conv_last weight).
"""
import argparse
import hashlib
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

SMALL = {2: (13, 17), 3: (9, 11), 4: (9, 11)}
SMALL_CFG = dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=2)
BIG_SEED, BIG_X_SEED = 71, 72
TRAIN_G = dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=2, upscale=4)


def weights_sha256(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v, np.float32).tobytes())
    return h.hexdigest()


def _checksums(net):
    return np.array([[float(p.detach().double().sum()), float(p.detach().double().norm())] for _, p in net.named_parameters()])


def train_opt(model_type):
    opt = OD(name='golden', model_type=model_type, scale=4, num_gpu=0, manual_seed=0, is_train=True, dist=False, rank=0,
             world_size=1)
    opt['network_g'] = OD(type='MSRResNet', **TRAIN_G)
    opt['network_d'] = OD(type='VGGStyleDiscriminator128', num_in_ch=3, num_feat=8)
    opt['path'] = OD(pretrain_network_g=None, strict_load_g=True, resume_state=None)
    tr = OD(ema_decay=0.9)
    tr['optim_g'] = OD(type='Adam', lr=1e-3, weight_decay=0, betas=[0.9, 0.99])
    tr['optim_d'] = OD(type='Adam', lr=1e-3, weight_decay=0, betas=[0.9, 0.99])
    tr['scheduler'] = OD(type='MultiStepLR', milestones=[2, 3], gamma=0.5)
    tr['total_iter'] = 4
    tr['warmup_iter'] = -1
    tr['pixel_opt'] = OD(type='L1Loss', loss_weight=1e-2, reduction='mean')
    tr['gan_opt'] = OD(type='GANLoss', gan_type='vanilla', real_label_val=1.0, fake_label_val=0.0, loss_weight=5e-3)
    tr['net_d_iters'] = 1
    tr['net_d_init_iters'] = 0
    opt['train'] = tr
    if model_type == 'SRModel':
        opt['train'].pop('gan_opt')
        opt.pop('network_d')
        opt['train'].pop('optim_d')
    return opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g_u_msrresnet.npz'))
    args = ap.parse_args()
    ref = ref_loader.load_reference()
    arch = importlib.import_module('basicsr.archs.srresnet_arch')   # registers MSRResNet with the reference's registry
    torch.manual_seed(0)
    a = {}
    for s in (2, 3, 4):
        net = arch.MSRResNet(upscale=s)
        a[f'keys_x{s}'] = np.array(list(net.state_dict()))
        a[f'shapes_x{s}'] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in net.state_dict().values()], np.int64)

    for s in (2, 3, 4):
        cfg = dict(SMALL_CFG, upscale=s)
        sd = synth.msrresnet_state_dict(100 + s, **cfg)
        h, w = SMALL[s]
        x = synth.uniform_input(110 + s, (2, 3, h, w))
        gy = np.random.default_rng(120 + s).standard_normal((2, 3, s * h, s * w)).astype(np.float32)
        a[f'fwd_x{s}_x'], a[f'fwd_x{s}_gy'] = x, gy
        for dt, tag in ((torch.float32, ''), (torch.float64, '64')):
            net = arch.MSRResNet(**cfg).to(dt)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            xt = torch.from_numpy(x).to(dt).requires_grad_(True)
            y = net(xt)
            y.backward(torch.from_numpy(gy).to(dt))
            a[f'fwd_x{s}_y{tag}'] = y.detach().numpy()
            if tag:   # gradients: the float64 values only, stored rounded to float32 (keeps the file under 1 MB)
                a[f'fwd_x{s}_dx64'] = xt.grad.float().numpy()
                for k, p in net.named_parameters():
                    a[f'fwd_x{s}_grad64.{k}'] = p.grad.float().numpy()

    cfg = dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=16, upscale=4)
    sd = synth.msrresnet_state_dict(BIG_SEED, **cfg)
    net = arch.MSRResNet(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    x = synth.uniform_input(BIG_X_SEED, (1, 3, 32, 32))
    with torch.no_grad():
        a['big_y'] = net(torch.from_numpy(x)).numpy()
    a['big_x'] = x
    a['big_weights_sha256'] = np.array(weights_sha256(sd))
    a['big_seed'] = np.array(BIG_SEED)

    runs = [(mt, cls, dt) for mt, cls in (('SRModel', ref.SRModel), ('SRGANModel', ref.SRGANModel))
            for dt in (torch.float32, torch.float64)]
    for mt0, cls, dt in runs:
        mt = mt0 if dt == torch.float32 else mt0 + '64'
        model = cls(train_opt(mt0))
        for net in (model.net_g, getattr(model, 'net_g_ema', None), getattr(model, 'net_d', None)):
            if net is not None:
                net.to(dt)
        model.net_g.load_state_dict({k: torch.from_numpy(v) for k, v in synth.msrresnet_state_dict(81, **TRAIN_G).items()},
                                    strict=True)
        model.model_ema(0)
        if hasattr(model, 'net_d'):
            model.net_d.load_state_dict({k: torch.from_numpy(v) for k, v in synth.vgg128_state_dict(82, 3, 8).items()}, strict=True)
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
            if hasattr(model, 'net_d'):
                a[f'{mt}_d_checksum_it{it}'] = _checksums(model.net_d)
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
