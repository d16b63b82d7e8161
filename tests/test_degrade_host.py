"""The device degradation chain on the host side (no GPU): the ABI of include/sr_hip_degrade.h (declared, bound, exported, in no
other header, each compute entry point mapped to the GPU test that pins it), the profiler names, the compiled resources read
from the code object, the kernel generators and the restatement tests/degrade_restate.py against the reference's own outputs
(tests/golden/g_zc_degrade.npz, tools/make_golden_degrade.py), the host resize, the seeded draws of the dataset, and every refusal.

The host side of degrade_ops.hip (argument checks) is also run under the host sanitizers by the stand-alone program
tests/helpers/degrade_host_checks.cpp; its result is reported in DESIGN.md."""
import ast
import math
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from image_restoration_amd import _lib
from image_restoration_amd.data import degradations as G
from image_restoration_amd.data import ocr_degradation_dataset as O
from image_restoration_amd.ops import degrade as D
from image_restoration_amd.utils.registry import DATASET_REGISTRY

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import degrade_restate as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_degrade.h')
OPTION_FILE = os.path.join(ROOT, 'options', 'train', 'RIDNet_plate', 'train_RIDNet_plate_degradation.yml')
SR_EINVAL = -1
_GPU = 'tests/test_degrade_ops_gpu.py::'
PINNED = {
    'sr_filter2d_f32': _GPU + 'test_filter2d_matches_float64',
    'sr_resize_bilinear_f32': _GPU + 'test_resize_matches_float64',
    'sr_add_gaussian_noise_f32': _GPU + 'test_noise_is_bit_identical_to_torch',
    'sr_diffjpeg_f32': _GPU + 'test_diffjpeg_forward_matches_float64',
    'sr_diffjpeg_bwd_f32': _GPU + 'test_diffjpeg_backward_matches_float64_autograd',
    'sr_degrade_finish_f32': _GPU + 'test_finish_matches_torch',
}
NAMES = ['filter2d_kernel', 'resize_bilinear_kernel', 'gaussian_noise_kernel<*>', 'diffjpeg_kernel', 'diffjpeg_bwd_kernel',
         'degrade_finish_kernel<*>']
KERNELS = ('filter2d_kernel', 'resize_bilinear_kernel', 'gaussian_noise_kernel', 'diffjpeg_kernel', 'diffjpeg_bwd_kernel',
           'degrade_finish_kernel')


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_every_declared_entry_point_is_bound_exported_and_pinned():
    declared = set(re.findall(r'\b(?:int|size_t)\s+(sr_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(_lib.DEGRADE_SIGNATURES) == set(PINNED) and len(declared) == 6
    others = set()
    for name in dir(_lib):
        if name.endswith('SIGNATURES') and name != 'DEGRADE_SIGNATURES':
            others |= set(getattr(_lib, name))
    assert others and not declared & others
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'sr_hip_degrade.h':
            text = open(os.path.join(ROOT, 'include', other)).read()
            assert not any(s in text for s in declared), other      # declared apart from the existing headers
    for s, target in PINNED.items():
        path, _, func = target.partition('::')
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith('test_')}
        assert func in tests, (s, target)


def test_profiler_ids_resolve_from_141():
    lib = _lib.load()
    assert [lib.sr_kernel_name(i).decode() for i in range(141, 147)] == NAMES
    for unnamed in (97, 101, 105, 109, 113, 123, 130, 138, 140, 147):
        assert lib.sr_kernel_name(unnamed).decode() == '', unnamed
    assert lib.sr_kernel_name(139).decode() == 'adam_groups_kernel'


def test_kernels_use_no_scratch_and_little_lds(tmp_path):
    llvm = '/opt/rocm/lib/llvm/bin'
    for tool in ('llvm-objdump', 'llvm-readelf'):
        if not os.path.exists(os.path.join(llvm, tool)):
            pytest.fail(f'{tool} is missing from {llvm}')
    lib = shutil.copy(os.path.join(ROOT, 'image_restoration_amd', 'lib', 'libsr_hip.so'), tmp_path / 'libsr_hip.so')
    subprocess.run([os.path.join(llvm, 'llvm-objdump'), '--offloading', lib], check=True, capture_output=True, cwd=tmp_path)
    found = {}
    for f in sorted(os.listdir(tmp_path)):
        if 'gfx950' not in f:
            continue
        notes = subprocess.run([os.path.join(llvm, 'llvm-readelf'), '--notes', str(tmp_path / f)], check=True, capture_output=True,
                               text=True).stdout
        cur, lds = None, 0
        for line in notes.splitlines():
            m = re.match(r'\s+(?:- )?\.(\w+):\s+(\S+)', line)
            if not m:
                continue
            key, val = m.groups()
            if key == 'group_segment_fixed_size':   # the keys of a kernel's entry are sorted: this one precedes its name
                lds = int(val)
            elif key == 'name' and val.startswith('_Z'):
                cur = found.setdefault(val, {}) if any(k in val for k in KERNELS) else None
                if cur is not None:
                    cur['group_segment_fixed_size'] = lds
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count'):
                cur[key] = int(val)
    for k in KERNELS:
        assert any(k in name for name in found), (k, sorted(found))
    assert len(found) == 8, sorted(found)          # the noise and finish kernels exist with 16-byte and with scalar accesses
    for name, md in found.items():
        assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 \
            and md.get('sgpr_spill_count', 0) == 0 and md['vgpr_count'] <= 128, (name, md)
        assert md['group_segment_fixed_size'] <= 64 * 1024, (name, md)
        if 'filter2d' in name:      # 36 rows x 85 floats of source window + the 21 x 21 kernel
            assert md['group_segment_fixed_size'] == (36 * 85 + 441) * 4
        if 'noise' in name or 'finish' in name or 'resize' in name:
            assert md['group_segment_fixed_size'] == 0


# ------------------------------------------------------------------------------------------------ the kernel generators
def test_kernel_generators_match_the_reference(golden):
    g = golden('g_zc_degrade')
    p = dict(sig_x=2.3, sig_y=0.9, theta=0.7, beta_g=1.7, beta_p=2.5)
    n = 0
    for k in (7, 11):
        for iso in (True, False):
            tag = f'{"iso" if iso else "aniso"}_k{k}'
            got = {'gauss': G.bivariate_Gaussian(k, p['sig_x'], p['sig_y'], p['theta'], isotropic=iso),
                   'gen': G.bivariate_generalized_Gaussian(k, p['sig_x'], p['sig_y'], p['theta'], p['beta_g'], isotropic=iso),
                   'plateau': G.bivariate_plateau(k, p['sig_x'], p['sig_y'], p['theta'], p['beta_p'], isotropic=iso)}
            for name, kern in got.items():
                want = g[f'kern_{name}_{tag}']
                assert kern.dtype == np.float64 and kern.shape == (k, k) == want.shape
                assert np.abs(kern - want).max() <= 1e-12, (name, tag)
                assert abs(kern.sum() - 1) <= 1e-12
                n += 1
    assert n == 12
    xy, xx, yy = G.mesh_grid(5)
    assert xy.shape == (5, 5, 2) and np.array_equal(xy[..., 0], xx) and np.array_equal(xy[..., 1], yy) and xx[0].tolist() == [-2, -1, 0, 1, 2]
    s = G.sigma_matrix2(2.0, 1.0, math.pi / 2)
    assert np.allclose(s, [[1, 0], [0, 4]], atol=1e-12)
    assert np.allclose(G.pdf2(np.eye(2), xy)[2, 2], 1.0)


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def test_draw_blur_kernel_is_seeded_sums_to_one_and_refuses_the_nonlinear_kinds():
    kinds = list(G.LINEAR_KINDS)
    prob = [1 / len(kinds)] * len(kinds)
    _seed(5)
    first = [G.draw_blur_kernel(kinds, prob, 21, (0.1, 10), (0.1, 10)) for _ in range(24)]
    _seed(5)
    again = [G.draw_blur_kernel(kinds, prob, 21, (0.1, 10), (0.1, 10)) for _ in range(24)]
    for a, b in zip(first, again):
        assert a.dtype == np.float32 and a.shape == (21, 21) and np.array_equal(a, b)
        assert abs(float(a.astype(np.float64).sum()) - 1) <= 441 * 2.0 ** -24          # float32 storage of a float64 kernel that sums to 1
    assert len({a.tobytes() for a in first}) > 12
    for kind in kinds:                                            # every supported kind on its own, padded
        _seed(1)
        kern = G.draw_blur_kernel([kind], [1.0], 11, (0.5, 3), (0.5, 3), pad_to=21)
        assert kern.shape == (21, 21) and float(np.abs(kern[:5]).max()) == 0 and abs(float(kern.astype(np.float64).sum()) - 1) <= 1e-5
    _seed(2)
    m = G.draw_blur_kernel(['motion'], [1.0], 7)
    assert np.count_nonzero(m) == 7 and np.allclose(m[m != 0], 1 / 7)
    assert np.array_equal(G.draw_blur_kernel(['average'], [1.0], 3), np.full((3, 3), 1 / 9, np.float32))
    for kind in G.UNSUPPORTED_KINDS:
        with pytest.raises(ValueError, match=kind):
            G.draw_blur_kernel([kind], [1.0], 21)
        with pytest.raises(ValueError, match=kind):
            G.check_kernel_list(['iso', kind])
    with pytest.raises(ValueError):
        G.pad_kernel_to(np.ones((5, 5)), 8)


# -------------------------------------------------------------------------------- the restatement against the reference
def test_restatement_reproduces_the_reference(golden):
    g = golden('g_zc_degrade')
    ks = set()
    for i in range(int(g['n_filter'])):
        x, k, y = (torch.from_numpy(g[f'f{i}_{n}']) for n in 'xky')
        assert x.dtype == torch.float64
        assert float((R.filter2d(x, k) - y).abs().max()) <= 1e-9
        ks.add((k.size(-1), k.size(0) == 1))
    assert {k for k, _ in ks} == {1, 3, 7, 21} and {s for _, s in ks} == {True, False}
    shapes = set()
    for i in range(int(g['n_jpeg'])):
        x = torch.from_numpy(g[f'j{i}_x']).double()
        fac = torch.tensor([R.quality_to_factor(q) for q in g[f'j{i}_q']], dtype=torch.float64)
        for d in (0, 1):
            want = torch.from_numpy(g[f'j{i}_y{d}'])
            out, quot, pre = R.diffjpeg(x, fac, bool(d), coef_fp32=True)
            assert out.shape == want.shape and float((out - want).abs().max()) <= 1e-9, (i, d)
            # the yardstick does not round the coefficients to float32 first: it moves by what that rounding is worth, no more
            pure = R.diffjpeg(x, fac, bool(d))[0]
            keep = ~R.pixel_mask(R.tie_exposed(quot), x.size(2), x.size(3))
            assert float(((pure - want).abs() * keep).max()) <= 1e-6, (i, d)
            assert pre.shape[2] % 16 == 0 and pre.shape[3] % 16 == 0 and R.macroblock_quotients(quot).shape[-1] == 384
        shapes.add(tuple(x.shape[2:]))
    assert shapes == {(16, 16), (8, 8), (1, 1), (17, 33), (37, 53)}
    assert D.quality_to_factor(10) == R.quality_to_factor(10) == 5.0 and D.quality_to_factor(90) == R.quality_to_factor(90)
    q = torch.tensor([10., 50., 90.])
    assert torch.equal(D.quality_to_factor(q), torch.tensor([5.0, 1.0, 0.2])) and q.tolist() == [10., 50., 90.]


def test_fixed_jpeg_seeds_expose_few_macroblocks():
    """The seeds the GPU tests use, checked on the CPU: at most 10 % of the macroblocks of a case have a quotient near a tie."""
    from test_degrade_ops_gpu import JPEG_CASES, jpeg_case
    for case in JPEG_CASES:
        x, fac, sizes = jpeg_case(case)
        for d in (False, True):
            if sizes is None:
                exposed = R.tie_exposed(R.diffjpeg(x, fac, d)[1])
                share = float(exposed.double().mean())
            else:
                parts = [R.tie_exposed(q) for q, _ in R.diffjpeg_ragged(x, fac, d, sizes)[1]]
                share = sum(int(p.sum()) for p in parts) / sum(p.numel() for p in parts)
            assert share <= 0.10, (case, d, share)
    from test_degrade_ops_gpu import BWD_CASES, _restate
    for case in BWD_CASES:                       # and few macroblocks with a value near the clamp's corners in the backward cases
        x, fac, sizes = jpeg_case(case)
        assert float(_restate(x, fac, True, sizes)[2].double().mean()) <= 0.10, case


# ------------------------------------------------------------------------------------------------------ the host resize
@pytest.mark.parametrize('src,dst', [((1, 1), (5, 7)), ((5, 7), (2, 3)), ((16, 16), (1, 1)), ((3, 4), (37, 53)), ((64, 64), (5, 5)),
                                     ((9, 11), (9, 11)), ((37, 53), (32, 48))])
def test_host_resize_equals_interpolate_in_float64(src, dst):
    """Same taps and weights as F.interpolate(bilinear, align_corners=False) on float64.  torch computes the coordinate in
    float64, the kernel's arithmetic in float32: a coordinate up to src_len carries at most 4 float32 roundings of that size, so
    the weight differs by at most 4 * 2^-24 * src_len and the blend by that times the largest tap difference (at most max|x|)."""
    rng = np.random.default_rng(src[0] * 100 + dst[1])
    img = rng.standard_normal((src[0], src[1], 3))
    got = O.resize_bilinear_numpy(img, dst[0], dst[1])
    want = F.interpolate(torch.from_numpy(img).permute(2, 0, 1)[None], size=dst, mode='bilinear', align_corners=False)[0].permute(1, 2, 0)
    tol = 4 * 2.0 ** -24 * max(src) * 2 * float(np.abs(img).max()) + 1e-15
    assert got.dtype == np.float64 and got.shape == (dst[0], dst[1], 3)
    assert float(np.abs(got - want.numpy()).max()) <= tol
    x = torch.from_numpy(img).permute(2, 0, 1)[None]
    assert np.array_equal(R.resize_bilinear(x, dst)[0].permute(1, 2, 0).numpy(), got)      # the restatement is the same arithmetic
    u8 = rng.integers(0, 256, (src[0], src[1], 3), dtype=np.uint8)
    r8 = O.resize_bilinear_u8(u8, dst[0], dst[1])
    assert r8.dtype == np.uint8 and r8.shape == (dst[0], dst[1], 3)
    if src == dst:
        assert np.array_equal(r8, u8)


# ----------------------------------------------------------------------------------------------------------- the dataset
def _write_pngs(folder, n, h=20, w=28):
    from PIL import Image
    rng = np.random.default_rng(11)
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(folder, f'plate_{i}.png'))


def _dataset_opt(folder, **kw):
    import yaml
    opt = yaml.safe_load(open(OPTION_FILE))['datasets']['train']
    opt.update(dataroot_gt=str(folder), phase='train', input_width=48, input_height=32, color_jitter_prob=0.5, gray_prob=0.3)
    opt.update(kw)
    return opt


def test_dataset_draws_are_seeded_and_items_have_the_documented_fields(tmp_path):
    _write_pngs(tmp_path, 3)
    ds = DATASET_REGISTRY.get('OCRDegradationDataset')(_dataset_opt(tmp_path, use_hflip=True))
    assert len(ds) == 3
    _seed(3)
    first = [ds[i % 3] for i in range(12)]
    _seed(3)
    again = [ds[i % 3] for i in range(12)]
    for a, b in zip(first, again):
        assert set(a) == {'gt_u8', 'sym', 'kernel', 'scale', 'sigma', 'quality', 'jitter', 'gray', 'gt_path'}
        for key in a:
            assert np.array_equal(a[key], b[key]), key
        assert a['gt_u8'].dtype == np.uint8 and a['gt_u8'].shape == (32, 48, 3) and a['kernel'].shape == (21, 21)
        assert a['kernel'].dtype == np.float32 and a['jitter'].shape == (3,) and a['sym'] in (0, 1) and a['gray'] in (0., 1.)
        assert 4 <= a['scale'] <= 12 and a['scale'].dtype == np.float64 and 0 <= a['sigma'] <= 20 and 30 <= a['quality'] <= 100
        assert float(np.abs(a['jitter']).max()) <= 20 / 255
    assert len({float(a['scale']) for a in first}) == 12
    # 32 x 48 is not square: the flip is applied here, on uint8, and the code that travels is 0; a square set ships the bit
    assert {int(a['sym']) for a in first} == {0}
    flipped = 0
    for s in range(8):
        _seed(s)
        coin = random.random() < 0.5
        _seed(s)
        item = ds[1]
        plain = O.resize_bilinear_u8(ds.decode(ds.paths[1], 'gt', as_float=False), 32, 48)
        assert np.array_equal(item['gt_u8'], plain[:, ::-1] if coin else plain)
        flipped += coin
    assert 0 < flipped < 8
    square = DATASET_REGISTRY.get('OCRDegradationDataset')(_dataset_opt(tmp_path, use_hflip=True, input_width=32))
    _seed(3)
    assert {int(square[i % 3]['sym']) for i in range(12)} == {0, 1}
    assert any(np.any(a['jitter'] != 0) for a in first) and any(not np.any(a['jitter']) for a in first)
    # the draws after the kernel come from numpy.random in the documented order
    _seed(9)
    item = ds[0]
    _seed(9)
    random.random()                                               # the flip
    G.draw_blur_kernel(ds.kernel_list, ds.kernel_prob, 21, ds.blur_sigma, ds.blur_sigma, [-math.pi, math.pi])
    assert item['scale'] == np.random.uniform(4.0, 12.0) and item['sigma'] == np.float32(np.random.uniform(0, 20))
    np.random.uniform()
    assert item['quality'] == np.float32(np.random.uniform(30, 100))
    from torch.utils.data import DataLoader
    batch = next(iter(DataLoader(ds, batch_size=3)))
    assert batch['gt_u8'].shape == (3, 32, 48, 3) and batch['kernel'].shape == (3, 21, 21) and batch['scale'].dtype == torch.float64
    assert batch['jitter'].shape == (3, 3) and batch['gray'].dtype == torch.float32 and batch['sym'].dtype == torch.int32


def test_dataset_refuses_what_it_cannot_do(tmp_path):
    _write_pngs(tmp_path, 1)
    cls = DATASET_REGISTRY.get('OCRDegradationDataset')
    with pytest.raises(ValueError, match='device_degrade'):
        cls(_dataset_opt(tmp_path, device_degrade=False))
    for key, val in (('color_jitter_pt_prob', 0.3), ('random_mask', True), ('pad_input', True)):
        with pytest.raises(ValueError, match=key):
            cls(_dataset_opt(tmp_path, **{key: val}))
    with pytest.raises(ValueError, match='pyblur'):
        cls(_dataset_opt(tmp_path, kernel_list=['iso', 'pyblur'], kernel_prob=[0.5, 0.5]))
    with pytest.raises(ValueError, match='blur_kernel_size'):
        cls(_dataset_opt(tmp_path, blur_kernel_size=23))
    cls(_dataset_opt(tmp_path, color_jitter_pt_prob=None, random_mask=False, pad_input=False, noise_range=None, jpeg_range=None))[0]


def test_option_file_and_pipeline_selection():
    import yaml
    from image_restoration_amd import train
    from image_restoration_amd.data import DeviceDegradePipeline, DevicePatchPipeline
    opt = yaml.safe_load(open(OPTION_FILE))
    block = opt['datasets']['train']
    assert opt['network_g']['type'] == 'RIDNet' and opt['scale'] == 1 and opt['model_type'] == 'SRModel'
    assert block['type'] == 'OCRDegradationDataset' and block['device_degrade'] is True and block['prefetch_mode'] == 'cuda'
    assert set(block['kernel_list']) <= set(G.LINEAR_KINDS) and abs(sum(block['kernel_prob']) - 1) < 1e-12
    assert (block['blur_kernel_size'], block['blur_sigma'], block['downsample_range'], block['noise_range'], block['jpeg_range']) \
        == (21, [0.1, 10], [4.0, 12.0], [0, 20], [30, 100])
    assert train.device_pipeline_class(block) is DeviceDegradePipeline
    assert train.device_pipeline_class(dict(type='PairedImageDataset')) is DevicePatchPipeline
    pipe = DeviceDegradePipeline(block)
    assert pipe.low_sizes(torch.tensor([4.0, 12.0, 5.3], dtype=torch.float64), 256, 256)[0].tolist() == [[64, 64], [21, 21], [48, 48]]
    assert pipe.low_sizes(torch.tensor([4.0]), 256, 250)[1] == (64, 62)
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        pipe(dict(gt_u8=torch.zeros((1, 256, 256, 3), dtype=torch.uint8), kernel=torch.zeros((1, 21, 21)), sym=torch.zeros(1)))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_python_ops_have_no_cpu_path_and_check_their_arguments():
    x = torch.zeros((2, 3, 16, 16))
    for call in (lambda: D.filter2D(x, torch.ones((1, 3, 3))), lambda: D.resize_bilinear(x, (4, 4)),
                 lambda: D.add_gaussian_noise_pt(x, 10.0), lambda: D.random_add_gaussian_noise_pt(x), lambda: D.DiffJPEG(False)(x, 50),
                 lambda: D.DiffJPEG(True)(x.requires_grad_(False), torch.tensor([50., 60.])), lambda: D.degrade_finish(x)):
        with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
            call()
    with pytest.raises(ValueError, match='Wrong kernel size'):
        D.filter2D(x, torch.ones((1, 4, 4)))
    from image_restoration_amd import hip_ops as H
    dev = torch.device('cpu')
    assert H.ragged_sizes(None, 2, 8, 8, dev) is None
    assert H.ragged_sizes([(1, 1), (8, 7)], 2, 8, 8, dev).tolist() == [[1, 1], [8, 7]]
    for bad in ([(0, 4), (4, 4)], [(4, 9), (4, 4)], [(9, 4), (4, 4)], [(4, 4)], [(4, -1), (1, 1)]):
        with pytest.raises(ValueError, match='sizes'):
            H.ragged_sizes(bad, 2, 8, 8, dev, 'sizes')


def test_every_entry_point_refuses_bad_arguments_before_launching():
    """No GPU is needed: each call returns SR_EINVAL from its argument checks."""
    lib = _lib.load()
    P, Q, S = 256, 4096, 512
    m3 = (np.float32(0.5) * np.ones(3, np.float32)).ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))

    def refused(name, args, needle):
        assert getattr(lib, name)(*args, None) == SR_EINVAL, (name, args)
        err = lib.sr_last_error()
        assert name.encode() in err and needle in err, (name, args, err)

    f = 'sr_filter2d_f32'
    for args, needle in (((None, P, Q, 1, 3, 16, 16, 3, 1), b'null'), ((P, None, Q, 1, 3, 16, 16, 3, 1), b'null'),
                         ((P, P, None, 1, 3, 16, 16, 3, 1), b'null'), ((P, P, Q, 0, 3, 16, 16, 3, 1), b'bad shape'),
                         ((P, P, Q, 1, 0, 16, 16, 3, 1), b'bad shape'), ((P, P, Q, 1, 3, 0, 16, 3, 1), b'bad shape'),
                         ((P, P, Q, 1, 3, 16, 16, 4, 1), b'not supported'), ((P, P, Q, 1, 3, 64, 64, 23, 1), b'not supported'),
                         ((P, P, Q, 1, 3, 16, 16, 0, 1), b'not supported'), ((P, P, Q, 1, 3, 10, 64, 21, 1), b'too small'),
                         ((P, P, Q, 1, 3, 64, 3, 7, 1), b'too small'), ((P, P, Q, 3, 3, 16, 16, 3, 2), b'kernel_batch'),
                         ((P, P, P, 1, 3, 16, 16, 3, 1), b'must not be x')):
        refused(f, args, needle)
    r = 'sr_resize_bilinear_f32'
    for args, needle in (((None, None, Q, None, 1, 3, 8, 8, 4, 4), b'null'), ((P, S, None, S, 1, 3, 8, 8, 4, 4), b'null'),
                         ((P, None, Q, None, 0, 3, 8, 8, 4, 4), b'bad shape'), ((P, None, Q, None, 1, 3, 0, 8, 4, 4), b'bad shape'),
                         ((P, None, Q, None, 1, 3, 8, 8, 4, 0), b'bad shape'), ((P, None, P, None, 1, 3, 8, 8, 4, 4), b'must not be src')):
        refused(r, args, needle)
    n = 'sr_add_gaussian_noise_f32'
    for args, needle in (((None, P, None, P, None, Q, 1, 3, 8, 8, 1, 0), b'null'), ((P, None, None, P, None, Q, 1, 3, 8, 8, 1, 0), b'null'),
                         ((P, P, None, None, None, Q, 1, 3, 8, 8, 1, 0), b'null'), ((P, P, None, P, None, None, 1, 3, 8, 8, 1, 0), b'null'),
                         ((P, P, None, P, P, Q, 1, 3, 8, 8, 1, 0), b'gray needs noise_gray'),
                         ((P, P, None, P, None, Q, 0, 3, 8, 8, 1, 0), b'bad shape'), ((P, P, None, P, None, Q, 1, 3, 8, 0, 1, 0), b'bad shape')):
        refused(n, args, needle)
    j = 'sr_diffjpeg_f32'
    for args, needle in (((None, None, P, Q, 1, 16, 16, 0), b'null'), ((P, S, None, Q, 1, 16, 16, 0), b'null'),
                         ((P, S, P, None, 1, 16, 16, 1), b'null'), ((P, None, P, Q, 0, 16, 16, 0), b'bad shape'),
                         ((P, None, P, Q, 1, 0, 16, 0), b'bad shape'), ((P, None, P, Q, 1, 16, -16, 0), b'bad shape')):
        refused(j, args, needle)
    jb = 'sr_diffjpeg_bwd_f32'
    for args, needle in (((None, None, P, P, Q, 1, 16, 16), b'null'), ((P, None, None, P, Q, 1, 16, 16), b'null'),
                         ((P, None, P, None, Q, 1, 16, 16), b'null'), ((P, None, P, P, None, 1, 16, 16), b'null'),
                         ((P, None, P, Q, Q, 0, 16, 16), b'bad shape'), ((P, None, P, Q, P, 1, 16, 16), b'must not be x')):
        refused(jb, args, needle)
    e = 'sr_degrade_finish_f32'
    for args, needle in (((None, None, None, Q, 1, 8, 8, m3, m3), b'null'), ((P, P, P, None, 1, 8, 8, None, None), b'null'),
                         ((P, None, None, Q, 0, 8, 8, m3, None), b'bad shape'), ((P, None, None, Q, 1, 0, 8, None, m3), b'bad shape')):
        refused(e, args, needle)
