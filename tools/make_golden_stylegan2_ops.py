#!/usr/bin/env python3
"""Writes tests/golden/g_zb_stylegan2_ops.npz: the reference's own ``upfirdn2d_native`` (basicsr/ops/upfirdn2d/upfirdn2d.py) and
the ``kernel`` / ``pad`` of its resampling modules (basicsr/archs/stylegan2_arch.py), run in place in float64.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_stylegan2_ops.py [--out tests/golden/g_zb_stylegan2_ops.npz]

The reference modules are imported from the read-only reference tree through tools/ref_loader.py's synthetic packages; nothing
of them is copied.  Contents:

* ``n_cases`` and, per case ``i``: ``c{i}_x`` [N, C, H, W], ``c{i}_k`` [kh, kw] (non-symmetric values), ``c{i}_args`` = (up_x,
  up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1), ``c{i}_y``: the grid of FACTORS x FILTERS x PADS x INPUTS below, without
  the combinations whose output size is not positive;
* ``up_kernel`` / ``up_pad`` and ``down_kernel`` / ``down_pad``: UpFirDnUpsample((1, 3, 3, 1), 2), UpFirDnDownsample((1, 3, 3, 1), 2);
* ``smooth_{u2k3,d2k3,d2k1}_kernel`` / ``_pad``: UpFirDnSmooth((1, 3, 3, 1), ...) for (up 2, kernel 3), (down 2, kernel 3),
  (down 2, kernel 1).

The fused activation exists in the reference only as a compiled extension and has no golden.
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

FACTORS = [(1, 1, 1, 1), (2, 2, 1, 1), (1, 1, 2, 2), (3, 2, 1, 1), (1, 1, 2, 3), (2, 3, 3, 2)]   # up_x, up_y, down_x, down_y
FILTERS = [(4, 4), (3, 2), (1, 5)]                                                               # kh, kw
PADS = [(0, 0, 0, 0), (2, 1, 2, 1), (-1, 2, 3, -1), (5, 4, 6, 5)]                                # x0, x1, y0, y1
INPUTS = [(1, 2, 5, 7), (2, 1, 8, 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g_zb_stylegan2_ops.npz'))
    args = ap.parse_args()
    ref_loader.load_reference()
    ufd = importlib.import_module('basicsr.ops.upfirdn2d.upfirdn2d')
    arch = importlib.import_module('basicsr.archs.stylegan2_arch')
    rng = np.random.Generator(np.random.PCG64(20261019))
    a, i = {}, 0
    for shape in INPUTS:
        for kh, kw in FILTERS:
            for f in FACTORS:
                for pad in PADS:
                    oh = (shape[2] * f[1] + pad[2] + pad[3] - kh) // f[3] + 1
                    ow = (shape[3] * f[0] + pad[0] + pad[1] - kw) // f[2] + 1
                    if shape[2] * f[1] + pad[2] + pad[3] - kh < 0 or shape[3] * f[0] + pad[0] + pad[1] - kw < 0:
                        continue
                    x = rng.standard_normal(shape)
                    k = rng.standard_normal((kh, kw))
                    y = ufd.upfirdn2d_native(torch.from_numpy(x), torch.from_numpy(k), *f, *pad)
                    assert tuple(y.shape) == (shape[0], shape[1], oh, ow) and y.dtype == torch.float64
                    a[f'c{i}_x'], a[f'c{i}_k'], a[f'c{i}_args'], a[f'c{i}_y'] = x, k, np.array(f + pad, np.int64), y.numpy()
                    i += 1
    a['n_cases'] = np.array(i)
    mods = {'up': arch.UpFirDnUpsample((1, 3, 3, 1), 2), 'down': arch.UpFirDnDownsample((1, 3, 3, 1), 2),
            'smooth_u2k3': arch.UpFirDnSmooth((1, 3, 3, 1), upsample_factor=2, downsample_factor=1, kernel_size=3),
            'smooth_d2k3': arch.UpFirDnSmooth((1, 3, 3, 1), upsample_factor=1, downsample_factor=2, kernel_size=3),
            'smooth_d2k1': arch.UpFirDnSmooth((1, 3, 3, 1), upsample_factor=1, downsample_factor=2, kernel_size=1)}
    for name, m in mods.items():
        a[f'{name}_kernel'], a[f'{name}_pad'] = m.kernel.double().numpy(), np.array(m.pad, np.int64)
    np.savez_compressed(args.out, **a)
    print(f'{args.out}: {os.path.getsize(args.out) / 1024:.1f} KiB, {i} cases, {len(a)} arrays')


if __name__ == '__main__':
    main()
