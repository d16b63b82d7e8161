#!/usr/bin/env python3
"""Writes tests/golden/g_z_edvr.npz: the reference's TSAFusion and PredeblurModule (basicsr/archs/edvr_arch.py) run in place in
float64 on the CPU on seeded weights and inputs, and the state_dict layout of its EDVR.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_edvr_golden.py [--out tests/golden/g_z_edvr.npz]

The reference's edvr_arch.py is imported from the read-only reference tree through synthetic parent packages, in the manner of
tools/ref_loader.py; nothing of it is copied.  Its arch_util imports the CUDA deformable-conv extension, so three modules of
this tool's own are registered first: ``basicsr.ops.dcn`` (a ModulatedDeformConvPack that only declares ``weight``, ``bias``
and ``conv_offset`` with the reference's shapes, enough for constructors and state_dict; it has no forward, so no golden of the
whole EDVR is possible), ``basicsr.utils`` with a ``get_root_logger``, and ``basicsr.utils.registry`` with an ARCH_REGISTRY
whose ``register()`` returns the class unchanged.

Weights come from numpy.random.default_rng with the scales of tests/test_pcd_gpu.py (weights N(0, 1.4^2 / fan_in), biases
N(0, 0.1^2)).  Contents, for ``{m}`` in ``tsa`` (TSAFusion(16, 3, 1) on (2, 3, 16, 12, 20)) and ``pre`` (PredeblurModule(3, 16,
hr_in=True) on (2, 3, 32, 48)):

* ``{m}_keys`` (the state_dict keys in order), ``{m}_w{i}`` (float32 parameter i), ``{m}_x`` (float32 input), ``{m}_gy``
  (float32 output gradient);
* ``{m}_y`` (float64 output), ``{m}_dx`` and ``{m}_dw{i}``: the float64 gradients of ``sum(y * gy)``, stored rounded to float32
  so that the file stays under 1 MiB (2^-25 relative per element, an order below the float32 distances the test measures);
* ``layout_default`` / ``layout_predeblur``: JSON lists of [key, shape] of the reference's ``EDVR()`` and
  ``EDVR(with_predeblur=True, hr_in=True)`` state_dicts, names and shapes only.
"""
import argparse
import importlib
import json
import logging
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_ROOT = os.environ.get('SR_REFERENCE_ROOT', '/root/reference')
CPR = os.path.join(REF_ROOT, 'Car_Plate-Restoration')


def _pkg(name, path=None):
    m = types.ModuleType(name)
    m.__path__ = [path] if path else []
    m.__package__ = name
    sys.modules[name] = m
    return m


class _PackStub(nn.Module):
    """Declares what the reference's ModulatedDeformConvPack owns (deform_conv.py:293-375): weight [cout, cin / groups, k, k],
    bias [cout], conv_offset = Conv2d(cin, dg * 3 * k * k, k, stride, padding)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1,
                 bias=True):
        super().__init__()
        k = kernel_size
        self.stride, self.padding, self.dilation, self.groups, self.deformable_groups = stride, padding, dilation, groups, deformable_groups
        self.weight = nn.Parameter(torch.zeros(out_channels, in_channels // groups, k, k))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        self.conv_offset = nn.Conv2d(in_channels, deformable_groups * 3 * k * k, k, stride, padding)


class _Registry:
    def register(self):
        return lambda cls: cls


def load_reference_edvr():
    if not os.path.isdir(CPR):
        raise FileNotFoundError(f'reference not mounted at {CPR}')
    sys.dont_write_bytecode = True
    _pkg('basicsr', os.path.join(CPR, 'basicsr'))
    utils = _pkg('basicsr.utils')
    utils.get_root_logger = lambda *a, **k: logging.getLogger('basicsr')
    reg = types.ModuleType('basicsr.utils.registry')
    reg.ARCH_REGISTRY = _Registry()
    sys.modules['basicsr.utils.registry'] = reg
    _pkg('basicsr.ops')
    dcn = types.ModuleType('basicsr.ops.dcn')
    dcn.ModulatedDeformConvPack, dcn.modulated_deform_conv = _PackStub, None
    sys.modules['basicsr.ops.dcn'] = dcn
    _pkg('basicsr.archs', os.path.join(CPR, 'basicsr', 'archs'))
    return importlib.import_module('basicsr.archs.edvr_arch')


def _seeded(module, rng):
    sd = {}
    for k, v in module.state_dict().items():
        if k.endswith('weight'):
            sc = 1.4 / np.sqrt(v.shape[1] * v.shape[2] * v.shape[3])
            sd[k] = torch.from_numpy((rng.standard_normal(tuple(v.shape)) * sc).astype(np.float32))
        else:
            sd[k] = torch.from_numpy((rng.standard_normal(tuple(v.shape)) * 0.1).astype(np.float32))
    return sd


def record(out, tag, module, x_shape, seed):
    rng = np.random.default_rng(seed)
    sd = _seeded(module, rng)
    x = torch.from_numpy(rng.standard_normal(x_shape).astype(np.float32))
    module.load_state_dict(sd, strict=True)
    module = module.double()
    xd = x.double().requires_grad_(True)
    y = module(xd)
    gy = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32))
    params = list(module.parameters())
    grads = torch.autograd.grad(y, [xd] + params, gy.double())
    out[f'{tag}_keys'] = np.array(list(sd))
    for i, k in enumerate(sd):
        assert tuple(params[i].shape) == tuple(sd[k].shape)
        out[f'{tag}_w{i}'] = sd[k].numpy()
        out[f'{tag}_dw{i}'] = grads[1 + i].numpy().astype(np.float32)
    out[f'{tag}_x'], out[f'{tag}_gy'] = x.numpy(), gy.numpy()
    out[f'{tag}_y'] = y.detach().numpy()
    out[f'{tag}_dx'] = grads[0].numpy().astype(np.float32)
    print(f'{tag}: {len(sd)} parameters, y {tuple(y.shape)} |y| max {float(y.detach().abs().max()):.3f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g_z_edvr.npz'))
    args = ap.parse_args()
    ref = load_reference_edvr()
    out = {}
    record(out, 'tsa', ref.TSAFusion(16, 3, 1), (2, 3, 16, 12, 20), 11)
    record(out, 'pre', ref.PredeblurModule(3, 16, hr_in=True), (2, 3, 32, 48), 12)
    for name, kw in (('default', {}), ('predeblur', dict(with_predeblur=True, hr_in=True))):
        layout = [[k, list(v.shape)] for k, v in ref.EDVR(**kw).state_dict().items()]
        out[f'layout_{name}'] = np.array(json.dumps(layout))
        print(f'layout_{name}: {len(layout)} entries')
    np.savez_compressed(args.out, **out)
    print(f'{args.out}: {os.path.getsize(args.out)} bytes')
    assert os.path.getsize(args.out) < (1 << 20)


if __name__ == '__main__':
    main()
