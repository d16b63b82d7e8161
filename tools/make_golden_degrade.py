#!/usr/bin/env python3
"""Writes tests/golden/g_zc_degrade.npz: the reference's own blur-kernel generators (basicsr/data/degradations.py), ``filter2D``
(basicsr/utils/img_process_util.py) and ``DiffJPEG`` (basicsr/utils/diffjpeg.py), run in place in float64.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_degrade.py [--out tests/golden/g_zc_degrade.npz]

Runs only where the reference tree exists (tools/ref_loader.py's REF_ROOT); nothing of it is copied.  The three files are
executed in place, each under a private module name.  ``img_process_util.py`` and ``degradations.py`` import cv2, pyblur, scipy,
PIL and torchvision at the top, but the functions used here touch none of them: whichever of those is not installed gets an empty
stub in ``sys.modules`` for the duration of the import.

``diffjpeg.py`` keeps ``y_table`` and ``c_table`` as module-level Parameters, so ``.double()`` on one DiffJPEG converts them for
every other instance: a fresh copy of the module is loaded per dtype.

Contents:
* ``kern_{gauss,gen,plateau}_{iso,aniso}_k{7,11}``: bivariate_Gaussian / bivariate_generalized_Gaussian / bivariate_plateau at
  KERNEL_PARAMS, float64;
* ``f{i}_x`` [B, C, H, W], ``f{i}_k`` [1 or B, k, k], ``f{i}_y``: filter2D in float64 for FILTER_CASES;
* ``j{i}_x`` (float32-representable), ``j{i}_q`` (qualities [B]), ``j{i}_y0`` / ``j{i}_y1``: DiffJPEG(differentiable=False / True)
  .double() for JPEG_CASES; ``n_filter``, ``n_jpeg``.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ref_loader  # noqa: E402
import degrade_restate as R  # noqa: E402

KERNEL_PARAMS = dict(sig_x=2.3, sig_y=0.9, theta=0.7, beta_g=1.7, beta_p=2.5)
FILTER_CASES = [((2, 3, 11, 11), 21, True), ((3, 1, 13, 20), 7, False), ((1, 2, 4, 4), 7, True), ((2, 2, 9, 6), 3, True),
                ((1, 1, 5, 5), 1, False)]                                   # shape, k, one kernel per sample
JPEG_CASES = [((3, 16, 16), (10., 50., 90.)), ((1, 8, 8), (50.,)), ((1, 1, 1), (10.,)), ((2, 17, 33), (10., 90.)),
              ((1, 37, 53), (50.,))]
STUBS = {'cv2': (), 'pyblur': (), 'scipy': ('special',), 'scipy.special': (), 'scipy.stats': ('multivariate_normal',),
         'PIL': ('Image', 'ImageOps'), 'torchvision': (), 'torchvision.transforms': (),
         'torchvision.transforms.functional_tensor': ('rgb_to_grayscale',)}


def load_in_place(rel_path, name):
    """Executes one file of the reference under the private module name ``name``; missing third-party imports are stubbed."""
    added = []
    for mod, attrs in STUBS.items():
        if mod in sys.modules:
            continue
        try:
            importlib.import_module(mod)
        except Exception:
            stub = types.ModuleType(mod)
            stub.__path__ = []
            stub.__all__ = []
            for a in attrs:
                setattr(stub, a, None)
            sys.modules[mod] = stub
            added.append(mod)
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref_loader.CPR, rel_path))
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
    finally:
        for mod in added:
            del sys.modules[mod]
    return module


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g_zc_degrade.npz'))
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    deg = load_in_place('basicsr/data/degradations.py', '_ref_degradations')
    ipu = load_in_place('basicsr/utils/img_process_util.py', '_ref_img_process_util')
    a = {}
    p = KERNEL_PARAMS
    for k in (7, 11):
        for iso in (True, False):
            tag = f'{"iso" if iso else "aniso"}_k{k}'
            a[f'kern_gauss_{tag}'] = deg.bivariate_Gaussian(k, p['sig_x'], p['sig_y'], p['theta'], isotropic=iso)
            a[f'kern_gen_{tag}'] = deg.bivariate_generalized_Gaussian(k, p['sig_x'], p['sig_y'], p['theta'], p['beta_g'], isotropic=iso)
            a[f'kern_plateau_{tag}'] = deg.bivariate_plateau(k, p['sig_x'], p['sig_y'], p['theta'], p['beta_p'], isotropic=iso)
    gen = torch.Generator().manual_seed(20261020)
    for i, (shape, k, per_sample) in enumerate(FILTER_CASES):
        x = torch.randn(shape, generator=gen, dtype=torch.float64)
        kern = torch.randn((shape[0] if per_sample else 1, k, k), generator=gen, dtype=torch.float64)   # signed, not normalised
        a[f'f{i}_x'], a[f'f{i}_k'], a[f'f{i}_y'] = x.numpy(), kern.numpy(), ipu.filter2D(x, kern).numpy()
    a['n_filter'] = np.int64(len(FILTER_CASES))
    for i, ((b, h, w), qualities) in enumerate(JPEG_CASES):
        x = R.smooth_noise_image(100 + i, b, h, w)
        a[f'j{i}_x'], a[f'j{i}_q'] = x.float().numpy(), np.array(qualities, dtype=np.float64)
        for diff in (False, True):
            ref = load_in_place('basicsr/utils/diffjpeg.py', f'_ref_diffjpeg_f64_{i}_{int(diff)}')   # fresh tables per use
            jpeg = ref.DiffJPEG(differentiable=diff).double()
            with torch.no_grad():
                a[f'j{i}_y{int(diff)}'] = jpeg(x, torch.tensor(qualities, dtype=torch.float64)).numpy()
    a['n_jpeg'] = np.int64(len(JPEG_CASES))
    np.savez_compressed(args.out, **a)
    print(f'{args.out}: {len(a)} arrays, {os.path.getsize(args.out)} bytes')
    assert os.path.getsize(args.out) < 300 * 1024


if __name__ == '__main__':
    main()
