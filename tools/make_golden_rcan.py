#!/usr/bin/env python3
"""Writes tests/golden/g_v_rcan.npz: the reference's RCAN (basicsr/archs/rcan_arch.py) and SRModel run in place on seeded
weights and inputs.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_rcan.py [--out tests/golden/g_v_rcan.npz]

The reference modules are imported from the read-only reference tree through tools/ref_loader.py's synthetic packages;
nothing of them is copied.  Weights come from synth.rcan_state_dict (numpy PCG64) and are loaded with
load_state_dict(strict=True).  Contents:

* ``keys_x{2,3,4,8}`` / ``shapes_x{2,3,4,8}``: state_dict keys and shapes of the default net (nf 64, 10 groups x 16 blocks,
  sf 16) per upscale;
* ``fwd_x{s}_*``: nf 16 (x8: nf 8), 2 groups x 2 blocks, sf 4, batch 2 on ragged LR sizes: x, y of the float32 run and ``y32_err``, its
  max-abs distance from the float64 run's y; then, against the upstream gradient synth.gaussian(``gy_seed``) (the tests regenerate
  it and check ``gy_sha256``), dL/dx and every parameter gradient (``grad64.<name>``) by autograd through the reference in float64,
  stored rounded to float32; ``ca_margin`` / ``relu_margin``: per RCAB (forward order), the smallest |pre-activation| of its
  attention's hidden ReLU and of its conv ReLU in the float64 run;
* ``big_*``: the option files' net (nf 64, 10 groups x 20 blocks, sf 16, x4) on one 16x16 input: x and y only.  Its weights are
  synth.rcan_state_dict(seed) and the tests regenerate them, checking the stored SHA-256 of their bytes;
* ``SRModel[64]_*``: three optimize_parameters iterations (the small net at x2, L1, Adam), in float32 and float64, with the
  quantities tools/make_goldens.py g_i stores (logs, learning rates, parameter checksums, Adam moment norms, final conv_last
  weight), and per iteration the smallest |pre-activation| of every attention ReLU and conv ReLU of the float64 run.
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

SCALES = (2, 3, 4, 8)
SMALL = {2: (13, 17), 3: (9, 11), 4: (7, 9), 8: (4, 5)}
SMALL_CFG = dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_group=2, num_block=2, squeeze_factor=4)
BIG_CFG = dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_group=10, num_block=20, squeeze_factor=16, upscale=4)
BIG_SEED, BIG_X_SEED = 171, 172
TRAIN_G = dict(SMALL_CFG, upscale=2)


def small_cfg(s):
    """The small net at upscale s.  x8 runs at nf 8 (hid 2): one channel block, and three upsampling stages of gradients at
    a quarter of nf 16's size."""
    return dict(SMALL_CFG, upscale=s, num_feat=8 if s == 8 else 16)


def weights_sha256(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v, np.float32).tobytes())
    return h.hexdigest()


def _checksums(net):
    return np.array([[float(p.detach().double().sum()), float(p.detach().double().norm())] for _, p in net.named_parameters()])


class Margins:
    """Forward hooks on every RCAB's conv 0 and attention fc1: the smallest |pre-activation| of each, per call."""

    def __init__(self, net):
        self.ca, self.relu, self.hooks = [], [], []
        for m in net.modules():
            if type(m).__name__ == 'RCAB':
                self.hooks.append(m.rcab[0].register_forward_hook(lambda _m, _i, o: self.relu.append(float(o.detach().abs().min()))))
                self.hooks.append(m.rcab[3].attention[1].register_forward_hook(
                    lambda _m, _i, o: self.ca.append(float(o.detach().abs().min()))))

    def take(self):
        out = np.array(self.ca), np.array(self.relu)
        self.ca, self.relu = [], []
        return out

    def close(self):
        for h in self.hooks:
            h.remove()


def train_opt():
    opt = OD(name='golden', model_type='SRModel', scale=2, num_gpu=0, manual_seed=0, is_train=True, dist=False, rank=0, world_size=1)
    opt['network_g'] = OD(type='RCAN', **TRAIN_G)
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g_v_rcan.npz'))
    args = ap.parse_args()
    ref = ref_loader.load_reference()
    arch = importlib.import_module('basicsr.archs.rcan_arch')   # registers RCAN with the reference's registry
    torch.manual_seed(0)
    a = {}
    for s in SCALES:
        net = arch.RCAN(3, 3, upscale=s)
        a[f'keys_x{s}'] = np.array(list(net.state_dict()))
        a[f'shapes_x{s}'] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in net.state_dict().values()], np.int64)

    for s in SCALES:
        cfg = small_cfg(s)
        sd = synth.rcan_state_dict(200 + s, **cfg)
        h, w = SMALL[s]
        x = synth.uniform_input(210 + s, (2, 3, h, w))
        gy = synth.gaussian(220 + s, (2, 3, s * h, s * w))
        a[f'fwd_x{s}_x'], a[f'fwd_x{s}_gy_seed'] = x, np.array(220 + s)
        a[f'fwd_x{s}_gy_sha256'] = np.array(hashlib.sha256(gy.tobytes()).hexdigest())
        ys = {}
        for dt, tag in ((torch.float32, ''), (torch.float64, '64')):
            net = arch.RCAN(**cfg).to(dt)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            marg = Margins(net)
            xt = torch.from_numpy(x).to(dt).requires_grad_(True)
            y = net(xt)
            y.backward(torch.from_numpy(gy).to(dt))
            ys[tag] = y.detach()
            ca_m, relu_m = marg.take()
            marg.close()
            if tag:   # y and gradients: the float64 values only as the distance / rounded to float32 (keeps the file small)
                a[f'fwd_x{s}_y'] = ys[''].numpy()
                a[f'fwd_x{s}_y32_err'] = np.array(float((ys[''].double() - ys['64']).abs().max()))
                a[f'fwd_x{s}_ca_margin'], a[f'fwd_x{s}_relu_margin'] = ca_m, relu_m
                a[f'fwd_x{s}_dx64'] = xt.grad.float().numpy()
                for k, p in net.named_parameters():
                    a[f'fwd_x{s}_grad64.{k}'] = p.grad.float().numpy()

    sd = synth.rcan_state_dict(BIG_SEED, **BIG_CFG)
    net = arch.RCAN(**BIG_CFG)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    x = synth.uniform_input(BIG_X_SEED, (1, 3, 16, 16))
    with torch.no_grad():
        a['big_y'] = net(torch.from_numpy(x)).numpy()
    a['big_x'] = x
    a['big_weights_sha256'] = np.array(weights_sha256(sd))
    a['big_seed'] = np.array(BIG_SEED)

    for dt in (torch.float32, torch.float64):
        mt = 'SRModel' if dt == torch.float32 else 'SRModel64'
        model = ref.SRModel(train_opt())
        model.net_g.to(dt)
        model.net_g_ema.to(dt)
        model.net_g.load_state_dict({k: torch.from_numpy(v) for k, v in synth.rcan_state_dict(181, **TRAIN_G).items()}, strict=True)
        model.model_ema(0)
        marg = Margins(model.net_g)
        logs, lrs = [], []
        for it in range(1, 4):
            model.update_learning_rate(it, warmup_iter=-1)
            lrs.append(model.get_current_learning_rate()[0])
            lq = torch.from_numpy(synth.uniform_input(1900 + it, (4, 3, 24, 24))).to(dt)
            gt = torch.from_numpy(synth.uniform_input(1950 + it, (4, 3, 48, 48))).to(dt)
            model.feed_data({'lq': lq, 'gt': gt})
            model.optimize_parameters(it)
            ca_m, relu_m = marg.take()
            if dt == torch.float64:
                a[f'{mt}_ca_margin_it{it}'], a[f'{mt}_relu_margin_it{it}'] = ca_m, relu_m
            log = model.get_current_log()
            logs.append([log[k] for k in sorted(log)])
            a[f'{mt}_g_checksum_it{it}'] = _checksums(model.net_g)
        marg.close()
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
    for s in SCALES:
        print(f'x{s}: min CA margin {a[f"fwd_x{s}_ca_margin"].min():.3e}, min conv ReLU margin {a[f"fwd_x{s}_relu_margin"].min():.3e}, '
              f'|y32 - y64| {float(a[f"fwd_x{s}_y32_err"]):.2e}')
    for it in range(1, 4):
        print(f'SRModel it{it}: min CA margin {a[f"SRModel64_ca_margin_it{it}"].min():.3e}, '
              f'min conv ReLU margin {a[f"SRModel64_relu_margin_it{it}"].min():.3e}')


if __name__ == '__main__':
    main()
