#!/usr/bin/env python3
"""Writes tests/golden/g_w_ridnet.npz: the reference's RIDNet (basicsr/archs/ridnet_arch.py) and SRModel run in place on
seeded weights and inputs.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_ridnet.py [--out tests/golden/g_w_ridnet.npz]

The reference modules are imported from the read-only reference tree through tools/ref_loader.py's synthetic packages;
nothing of them is copied.  Weights come from synth.ridnet_state_dict (numpy PCG64) and are loaded with
load_state_dict(strict=True).  Contents:

* ``keys`` / ``shapes``: state_dict keys (named_parameters order) and shapes of the default net RIDNet(3, 64, 3);
  ``init_mean`` / ``init_std``: per tensor, the mean and standard deviation of the reference's own initialisation of that net
  (torch.manual_seed(0)); ``init_requires_grad``: whether each parameter requires grad there;
* ``fwd{i}_*`` for the small net (mid 16, 2 EAMs) on ragged batches: x, y of the float32 run and ``y32_err``, its max-abs
  distance from the float64 run's y; against the upstream gradient synth.gaussian(``gy_seed``) (the tests regenerate it and check
  ``gy_sha256``), dL/dx and every parameter gradient (``grad64.<name>``, MeanShift included) by autograd through the reference
  in float64, stored rounded to float32; ``relu_margin``: the smallest |pre-activation| of every ReLU call of the float64 run;
* ``big_*``: the default net on one 12x16 input: x and y only; its weights are synth.ridnet_state_dict(``big_seed``), checked
  by the stored SHA-256 of their bytes;
* ``SRModel[64]_*``: three optimize_parameters iterations of the small net at scale 1 (L1, Adam) in float32 and float64: logs,
  learning rates, parameter checksums per iteration, Adam moment norms, the final tail weight, and per iteration the smallest
  |pre-activation| of every ReLU of the float64 run.
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

SMALL_CFG = dict(in_channels=3, mid_channels=16, out_channels=3, num_block=2)
SMALL = [(2, 5, 13), (1, 11, 37)]       # (n, h, w): one side below 2*4 + 1
BIG_SEED, BIG_X_SEED = 311, 312


def weights_sha256(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v, np.float32).tobytes())
    return h.hexdigest()


def _checksums(net):
    return np.array([[float(p.detach().double().sum()), float(p.detach().double().norm())] for _, p in net.named_parameters()])


class Margins:
    """Forward pre-hooks on every nn.ReLU (all of the reference's ReLUs are modules, applied in place): the smallest
    |pre-activation| per call."""

    def __init__(self, net):
        self.vals, self.hooks = [], []
        for m in net.modules():
            if isinstance(m, torch.nn.ReLU):
                self.hooks.append(m.register_forward_pre_hook(lambda _m, i: self.vals.append(float(i[0].detach().abs().min()))))

    def take(self):
        out = np.array(self.vals)
        self.vals = []
        return out

    def close(self):
        for h in self.hooks:
            h.remove()


def train_opt():
    opt = OD(name='golden', model_type='SRModel', scale=1, num_gpu=0, manual_seed=0, is_train=True, dist=False, rank=0, world_size=1)
    opt['network_g'] = OD(type='RIDNet', **SMALL_CFG)
    opt['path'] = OD(pretrain_network_g=None, strict_load_g=True, resume_state=None)
    tr = OD(ema_decay=0.9)
    tr['optim_g'] = OD(type='Adam', lr=1e-4, weight_decay=0, betas=[0.9, 0.99])
    tr['scheduler'] = OD(type='MultiStepLR', milestones=[2, 3], gamma=0.5)
    tr['total_iter'] = 4
    tr['warmup_iter'] = -1
    tr['pixel_opt'] = OD(type='L1Loss', loss_weight=1.0, reduction='mean')
    opt['train'] = tr
    return opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g_w_ridnet.npz'))
    args = ap.parse_args()
    ref = ref_loader.load_reference()
    arch = importlib.import_module('basicsr.archs.ridnet_arch')   # registers RIDNet with the reference's registry
    torch.manual_seed(0)
    a = {}
    net = arch.RIDNet(3, 64, 3)
    named = list(net.named_parameters())
    a['keys'] = np.array([k for k, _ in named])
    a['shapes'] = np.array([list(p.shape) + [0] * (4 - p.dim()) for _, p in named], np.int64)
    a['init_mean'] = np.array([float(p.detach().double().mean()) for _, p in named])
    a['init_std'] = np.array([float(p.detach().double().std()) if p.numel() > 1 else 0.0 for _, p in named])
    a['init_requires_grad'] = np.array([bool(p.requires_grad) for _, p in named])
    assert list(net.state_dict()) == list(a['keys'])

    for i, (n, h, w) in enumerate(SMALL):
        sd = synth.ridnet_state_dict(400 + i, **SMALL_CFG)
        x = synth.uniform_input(410 + i, (n, 3, h, w))
        gy = synth.gaussian(420 + i, (n, 3, h, w))
        a[f'fwd{i}_x'], a[f'fwd{i}_gy_seed'] = x, np.array(420 + i)
        a[f'fwd{i}_gy_sha256'] = np.array(hashlib.sha256(gy.tobytes()).hexdigest())
        ys = {}
        for dt, tag in ((torch.float32, ''), (torch.float64, '64')):
            net = arch.RIDNet(**SMALL_CFG).to(dt)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            marg = Margins(net)
            xt = torch.from_numpy(x).to(dt).requires_grad_(True)
            y = net(xt)
            y.backward(torch.from_numpy(gy).to(dt))
            ys[tag] = y.detach()
            m = marg.take()
            marg.close()
            if tag:
                a[f'fwd{i}_y'] = ys[''].numpy()
                a[f'fwd{i}_y32_err'] = np.array(float((ys[''].double() - ys['64']).abs().max()))
                a[f'fwd{i}_relu_margin'] = m
                a[f'fwd{i}_dx64'] = xt.grad.float().numpy()
                for k, p in net.named_parameters():
                    a[f'fwd{i}_grad64.{k}'] = p.grad.float().numpy()

    sd = synth.ridnet_state_dict(BIG_SEED, in_channels=3, mid_channels=64, out_channels=3)
    net = arch.RIDNet(3, 64, 3)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    x = synth.uniform_input(BIG_X_SEED, (1, 3, 12, 16))
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
        model.net_g.load_state_dict({k: torch.from_numpy(v) for k, v in synth.ridnet_state_dict(481, **SMALL_CFG).items()},
                                    strict=True)
        model.model_ema(0)
        marg = Margins(model.net_g)
        logs, lrs = [], []
        for it in range(1, 4):
            model.update_learning_rate(it, warmup_iter=-1)
            lrs.append(model.get_current_learning_rate()[0])
            gt = synth.uniform_input(1950 + it, (4, 3, 24, 24))
            lq = np.clip(gt + 0.1 * synth.gaussian(1900 + it, (4, 3, 24, 24)), 0, 1).astype(np.float32)
            model.feed_data({'lq': torch.from_numpy(lq).to(dt), 'gt': torch.from_numpy(gt).to(dt)})
            model.optimize_parameters(it)
            m = marg.take()
            if dt == torch.float64:
                a[f'{mt}_relu_margin_it{it}'] = m
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
        a[f'{mt}_g_tail_weight'] = model.net_g.tail.weight.detach().double().numpy().copy()

    np.savez_compressed(args.out, **a)
    print(f'{args.out}: {os.path.getsize(args.out) / 1024:.1f} KiB, {len(a)} arrays')
    for i in range(len(SMALL)):
        print(f'fwd{i}: min ReLU margin {a[f"fwd{i}_relu_margin"].min():.3e}, |y32 - y64| {float(a[f"fwd{i}_y32_err"]):.2e}, '
              f'max|y| {np.abs(a[f"fwd{i}_y"]).max():.1f}')
    for it in range(1, 4):
        print(f'SRModel it{it}: min ReLU margin {a[f"SRModel64_relu_margin_it{it}"].min():.3e}')


if __name__ == '__main__':
    main()
