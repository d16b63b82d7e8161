"""upfirdn2d and the fused bias + LeakyReLU on the host side (no GPU): the ABI of include/sr_hip_stylegan2.h (declared, bound,
exported, each compute entry point mapped to the GPU test that pins it), the profiler names, the compiled resources and the
instance set read from the code object, the restatement tests/upfirdn_restate.py and the CPU path against the reference's own
outputs (tests/golden/g_zb_stylegan2_ops.npz, tools/make_golden_stylegan2_ops.py), the modules against the reference's pads and
kernels, the gradient-pad rule against float64 autograd, and every refusal.

The host side of stylegan2_ops.hip (argument checks, dispatch, size query) is also run under the host sanitizers by the
stand-alone program tests/helpers/stylegan2_ops_host_checks.cpp; its result is reported in DESIGN.md."""
import ast
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H
from image_restoration_amd.archs import stylegan2_arch as S
from image_restoration_amd.ops.fused_act import FusedLeakyReLU, fused_leaky_relu
from image_restoration_amd.ops.upfirdn2d import UpFirDn2d, upfirdn2d, upfirdn2d_native
from image_restoration_amd.utils.registry import ARCH_REGISTRY

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upfirdn_restate as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_stylegan2.h')
SR_EINVAL, SR_ENOSPACE = -1, -3
D = torch.float64
_GPU = 'tests/test_stylegan2_ops_gpu.py::'
# every compute entry point -> the GPU test that compares it with its yardstick; the host-only queries are EXEMPT
PINNED = {
    'sr_upfirdn2d_f32': _GPU + 'test_upfirdn2d_stylegan2_instances_match_float64',
    'sr_fused_bias_act_f32': _GPU + 'test_activation_forward_backward_and_ref_are_ieee_exact',
    'sr_fused_bias_act_bwd_f32': _GPU + 'test_activation_forward_backward_and_ref_are_ieee_exact',
}
EXEMPT = {
    'sr_upfirdn2d_instance': 'host-only dispatch query: test_instances_built_are_the_instances_dispatched',
    'sr_fused_bias_act_workspace_bytes': 'host-only size query: test_workspace_size_query',
}
NAMES = ['upfirdn2d_kernelILi0ELi0ELi0EE', 'upfirdn2d_kernelILi1ELi1ELi4EE', 'upfirdn2d_kernelILi2ELi1ELi4EE',
         'upfirdn2d_kernelILi1ELi2ELi4EE', 'fused_bias_act_kernel<*,false>', 'fused_bias_act_kernel<*,true>',
         'fused_bias_act_finish_kernel']


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_every_declared_entry_point_is_bound_exported_and_pinned():
    declared = set(re.findall(r'\b(?:int|size_t)\s+(sr_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(_lib.STYLEGAN2_SIGNATURES) == set(PINNED) | set(EXEMPT) and len(declared) == 5
    assert not set(PINNED) & set(EXEMPT)
    others = set(_lib.SIGNATURES) | set(_lib.RIDNET_SIGNATURES) | set(_lib.GFPGAN_SIGNATURES) | set(_lib.EDSR_SIGNATURES) \
        | set(_lib.CA_BF16_SIGNATURES) | set(_lib.DCN_SIGNATURES) | set(_lib.EDVR_SIGNATURES) | set(_lib.EDVR_BF16_SIGNATURES)
    assert not declared & others
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'sr_hip_stylegan2.h':
            text = open(os.path.join(ROOT, 'include', other)).read()
            assert not any(s in text for s in declared), other      # declared apart from the existing headers
    for s, target in PINNED.items():
        path, _, func = target.partition('::')
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith('test_')}
        assert func in tests, (s, target)


def test_profiler_ids_resolve_and_130_stays_empty():
    lib = _lib.load()
    assert [lib.sr_kernel_name(i).decode() for i in range(131, 138)] == NAMES
    assert lib.sr_kernel_name(130).decode() == '' and lib.sr_kernel_name(138).decode() == ''
    assert lib.sr_kernel_name(129).decode() == 'tsa16_gate_kernel'


def _code_object_kernels(tmp_path):
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
                cur = found.setdefault(val, {}) if ('upfirdn2d_kernel' in val or 'fused_bias_act' in val) else None
                if cur is not None:
                    cur['group_segment_fixed_size'] = lds
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count'):
                cur[key] = int(val)
    return found


def test_instances_built_are_the_instances_dispatched(tmp_path):
    found = _code_object_kernels(tmp_path)
    ufd = sorted(k for k in found if 'upfirdn2d_kernel' in k)
    built = {tuple(int(v) for v in re.search(r'ILi(\d)ELi(\d)ELi(\d)E', k).groups()) for k in ufd}
    assert built == {(0, 0, 0), (1, 1, 4), (2, 1, 4), (1, 2, 4)} and len(ufd) == 4, ufd
    act = sorted(k for k in found if 'fused_bias_act_kernel' in k)
    assert {re.search(r'ILi(\d)ELb(\d)E', k).groups() for k in act} == {('1', '0'), ('1', '1'), ('4', '0'), ('4', '1')} and len(act) == 4
    assert len(found) == 9, sorted(found)                        # + the finish kernel
    for name, md in found.items():
        assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 \
            and md.get('sgpr_spill_count', 0) == 0 and md['vgpr_count'] <= 128, (name, md)
        # upfirdn2d's LDS is dynamic (sr_upfirdn2d_instance); the reducing activation kernels hold their 4 wave sums
        assert md['group_segment_fixed_size'] == (16 if 'Lb1E' in name else 0), (name, md)
    # every (filter, factors) the argument check admits lands on one of the four; the three special ones only on their own
    key = {0: (0, 0, 0), 1: (1, 1, 4), 2: (2, 1, 4), 3: (1, 2, 4)}
    reached = set()
    for kh, kw, ux, uy, dx, dy in itertools.product((1, 3, 4, 16), (1, 4, 5, 16), (1, 2, 8), (1, 2, 3), (1, 2, 8), (1, 2, 5)):
        inst, th, lds = H.upfirdn2d_instance(kh, kw, ux, uy, dx, dy)
        reached.add(key[inst])
        special = (kh, kw) == (4, 4) and ux == uy and dx == dy and (ux, dx) in ((1, 1), (2, 1), (1, 2))
        assert (inst != 0) == special and 1 <= th <= 32 and lds <= 63 * 1024 and (inst == 0 or th == 32), (kh, kw, ux, uy, dx, dy)
        assert inst == 0 or key[inst] == (ux, dx, 4)
    assert reached == built
    assert H.upfirdn2d_instance(4, 4, 1, 1, 1, 1) == (1, 32, (256 + 35 * 67) * 4)
    assert H.upfirdn2d_instance(4, 4, 2, 2, 1, 1) == (2, 32, (256 + 18 * 34) * 4)
    assert H.upfirdn2d_instance(4, 4, 1, 1, 2, 2) == (3, 32, (256 + 66 * 130) * 4)
    assert H.upfirdn2d_instance(16, 16, 1, 1, 8, 8) == (0, 2, (256 + 24 * 520) * 4)


def test_workspace_size_query():
    lib = _lib.load()
    q = lib.sr_fused_bias_act_workspace_bytes
    assert q(2, 3, 1) == 24 and q(2, 3, 1024) == 24 and q(2, 3, 1025) == 48 and q(16, 64, 256 * 256) == 16 * 64 * 64 * 4
    assert q(0, 3, 1) == 0 and q(2, 0, 1) == 0 and q(2, 3, 0) == 0 and q(1 << 16, 1 << 16, 1) == 0


# ----------------------------------------------------------------------------------------- the fixture of the reference
def _cases(g):
    for i in range(int(g['n_cases'])):
        a = [int(v) for v in g[f'c{i}_args']]
        yield torch.from_numpy(g[f'c{i}_x']), torch.from_numpy(g[f'c{i}_k']), (a[0], a[1]), (a[2], a[3]), tuple(a[4:]), \
            torch.from_numpy(g[f'c{i}_y'])


def test_restatement_and_native_reproduce_the_reference(golden):
    g = golden('g_zb_stylegan2_ops')
    seen = set()
    n = 0
    for x, k, up, down, pad, y in _cases(g):
        assert x.dtype == D and y.dtype == D
        for fn in (lambda: R.upfirdn2d(x, k, up, down, pad), lambda: upfirdn2d_native(x, k, *up, *down, *pad)):
            got = fn()
            assert got.shape == y.shape and got.dtype == D
            # float64 against float64: only the order of a few additions can differ
            assert float((got - y).abs().max()) <= 1e-13 * max(1.0, float(y.abs().max()))
        assert tuple(y.shape[2:]) == R.out_size(x.size(2), x.size(3), k.size(0), k.size(1), up, down, pad)
        seen.add((up, down, tuple(k.shape), min(pad) < 0))
        n += 1
    assert n == 135 and len({s[:2] for s in seen}) == 6 and {s[2] for s in seen} == {(4, 4), (3, 2), (1, 5)} and {s[3] for s in seen} == {True, False}


def test_upfirdn2d_on_cpu_tensors_reproduces_the_reference_within_fp32_rounding(golden):
    """The public function on fp32 CPU tensors (the native path), for the cases with one factor and one pad pair for both axes:
    the inputs are rounded to fp32 (storage), the arithmetic is fp32: (T + 2) EPS on the operation of absolute values, T taps of
    the dense convolution the native path runs (kh * kw) plus one rounding of each operand."""
    g = golden('g_zb_stylegan2_ops')
    eps, n = 2.0 ** -24, 0
    for x, k, up, down, pad, y in _cases(g):
        if up[0] != up[1] or down[0] != down[1] or pad[0] != pad[2] or pad[1] != pad[3]:
            continue
        got = upfirdn2d(x.float(), k.float(), up=up[0], down=down[0], pad=(pad[0], pad[1]))
        a = R.upfirdn2d(x.abs(), k.abs(), up, down, pad)
        assert got.dtype == torch.float32 and got.shape == y.shape
        assert bool(((got.double() - y).abs() <= (k.numel() + 4) * eps * a).all())
        n += 1
    assert n >= 18


def test_modules_reproduce_the_recorded_pads_and_kernels(golden):
    g = golden('g_zb_stylegan2_ops')
    mods = {'up': S.UpFirDnUpsample((1, 3, 3, 1), 2), 'down': S.UpFirDnDownsample((1, 3, 3, 1), 2),
            'smooth_u2k3': S.UpFirDnSmooth((1, 3, 3, 1), upsample_factor=2, downsample_factor=1, kernel_size=3),
            'smooth_d2k3': S.UpFirDnSmooth((1, 3, 3, 1), upsample_factor=1, downsample_factor=2, kernel_size=3),
            'smooth_d2k1': S.UpFirDnSmooth((1, 3, 3, 1), upsample_factor=1, downsample_factor=2, kernel_size=1)}
    for name, m in mods.items():
        assert tuple(int(v) for v in g[f'{name}_pad']) == tuple(m.pad), name
        assert m.kernel.dtype == torch.float32 and np.array_equal(m.kernel.double().numpy(), g[f'{name}_kernel']), name
        assert list(m.state_dict()) == [] and list(m.parameters()) == []
    assert repr(mods['up']) == 'UpFirDnUpsample(factor=2)' and repr(mods['down']) == 'UpFirDnDownsample(factor=2)'
    assert repr(mods['smooth_u2k3']) == 'UpFirDnSmooth(upsample_factor=2, downsample_factor=1)'
    assert (mods['up'].pad, mods['down'].pad, mods['smooth_u2k3'].pad, mods['smooth_d2k3'].pad, mods['smooth_d2k1'].pad) \
        == ((2, 1), (1, 1), (1, 1), (2, 2), (1, 1))
    with pytest.raises(NotImplementedError):
        S.UpFirDnSmooth((1, 3, 3, 1))
    assert float(S.make_resample_kernel([1, 3, 3, 1]).sum()) == 1.0 and S.make_resample_kernel([1, 3, 3, 1])[1, 2] == 9 / 64
    assert S.ScaledLeakyReLU().negative_slope == 0.2 and S.ScaledLeakyReLU(0.1).negative_slope == 0.1
    assert sorted(n for n in dir(S) if not n.startswith('_') and getattr(getattr(S, n), '__module__', None) == S.__name__) \
        == ['ScaledLeakyReLU', 'UpFirDnDownsample', 'UpFirDnSmooth', 'UpFirDnUpsample', 'make_resample_kernel']
    for name in ('UpFirDnUpsample', 'UpFirDnDownsample', 'UpFirDnSmooth', 'ScaledLeakyReLU', 'StyleGAN2Discriminator'):
        assert name not in ARCH_REGISTRY
    # CPU tensors take the native path through the modules: up-sampling a constant keeps it, as the filter's gain says
    x = torch.full((1, 2, 5, 6), 3.0)
    assert tuple(mods['up'](x).shape) == (1, 2, 10, 12) and float((mods['up'](x)[:, :, 2:-2, 2:-2] - 3.0).abs().max()) < 1e-6
    assert tuple(mods['down'](x).shape) == (1, 2, 2, 3) and float((mods['down'](x)[:, :, 1, 1] - 3.0).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------------ the gradient-pad rule
def test_gradient_pad_rule_over_the_grid():
    """up, down in {1, 2, 3}, kh in {1, 3, 4}, kw in {2, 4}, pad0 in {-1, 0, 2, 3}, pad1 in {-1, 1, 2}, inputs 5x7 and 8x7: in each
    of the 1290 combinations with a positive output size the swapped-factor call with the flipped filter and the pads of the rule
    equals float64 autograd's gradient of the restatement to 1e-12 (both are float64 sums of at most 16 products of O(1) terms)."""
    gen = torch.Generator().manual_seed(7)
    n = 0
    for up, down, kh, kw, p0, p1, (h, w) in itertools.product((1, 2, 3), (1, 2, 3), (1, 3, 4), (2, 4), (-1, 0, 2, 3), (-1, 1, 2),
                                                             ((5, 7), (8, 7))):
        pad = (p0, p1, p0, p1)
        if h * up + p0 + p1 - kh < 0 or w * up + p0 + p1 - kw < 0:
            continue
        x = torch.randn((1, 2, h, w), generator=gen, dtype=D).requires_grad_(True)
        k = torch.randn((kh, kw), generator=gen, dtype=D)
        y = R.upfirdn2d(x, k, (up, up), (down, down), pad)
        g = torch.randn(y.shape, generator=gen, dtype=D)
        want, = torch.autograd.grad(y, x, g)
        got, gp = R.grad_call(g, k, (h, w), (up, up), (down, down), pad)
        assert got.shape == want.shape, (up, down, kh, kw, pad, h, w, gp)
        assert float((got - want).abs().max()) <= 1e-12, (up, down, kh, kw, pad, h, w, gp)
        from image_restoration_amd.ops.upfirdn2d.upfirdn2d import grad_pad
        assert grad_pad((h, w), y.shape[2:], (kh, kw), (up, up), (down, down), pad) == gp
        n += 1
    assert n == 1290


# ------------------------------------------------------------------------------------------------------------ refusals
def test_upfirdn2d_refusals():
    x, k = torch.zeros((1, 2, 6, 9)), torch.ones((4, 4))
    pad4 = (1, 1, 1, 1)
    for bad in (lambda: upfirdn2d(x.double(), k.double()), lambda: upfirdn2d(x.bfloat16(), k.bfloat16()), lambda: upfirdn2d(x, k.double()),
                lambda: upfirdn2d(x, torch.ones((17, 4)), pad=(20, 20)), lambda: upfirdn2d(x, torch.ones((4, 0))),
                lambda: upfirdn2d(x, k, up=9, pad=(2, 1)), lambda: upfirdn2d(x, k, up=0), lambda: upfirdn2d(x, k, down=9),
                lambda: upfirdn2d(x, k, down=0), lambda: upfirdn2d(x, k, up=2.0), lambda: upfirdn2d(x, torch.ones((7, 4))),
                lambda: upfirdn2d(x, k, pad=(-3, -3)), lambda: upfirdn2d(x[0], k), lambda: upfirdn2d(x, k[0]),
                lambda: UpFirDn2d.apply(x, k, (1, 9), (1, 1), pad4), lambda: UpFirDn2d.apply(x, k, (1, 1), (1, 1), (0, 0, -2, -1)),
                lambda: UpFirDn2d.apply(x.half(), k.half(), (1, 1), (1, 1), pad4),
                lambda: upfirdn2d_native(x, k, 1, 1, 1, 1, -3, -3, 0, 0), lambda: upfirdn2d_native(x, k, 1, 9, 1, 1, 0, 0, 0, 0)):
        with pytest.raises(ValueError, match='supported: fp32, filter sides 1..16, factors 1..8'):
            bad()
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):            # a CPU tensor never reaches the kernel
        UpFirDn2d.apply(x, k, (1, 1), (1, 1), pad4)
    assert tuple(upfirdn2d(x, k, pad=(1, 1)).shape) == (1, 2, 5, 8)          # ... and the public function takes the native path
    with pytest.raises(ValueError, match='fp32'):
        S.UpFirDnDownsample((1, 3, 3, 1))(x.double())
    lib = _lib.load()

    def call(**kw):
        a = dict(x=256, xs=108, out=256, os=1 << 20, f=256, n=1, planes=2, h=6, w=9, minor=1, kh=4, kw=4, ux=1, uy=1, dx=1, dy=1,
                 px0=1, px1=1, py0=1, py1=1)
        a.update(kw)
        return lib.sr_upfirdn2d_f32(a['x'], a['xs'], a['out'], a['os'], a['f'], a['n'], a['planes'], a['h'], a['w'], a['minor'], a['kh'],
                                    a['kw'], a['ux'], a['uy'], a['dx'], a['dy'], a['px0'], a['px1'], a['py0'], a['py1'], None)
    for kw, needle in ((dict(x=None), b'null'), (dict(out=None), b'null'), (dict(f=None), b'null'), (dict(x=258), b'aligned'),
                       (dict(minor=2), b'minor'), (dict(n=0), b'bad shape'), (dict(planes=0), b'bad shape'), (dict(h=0), b'bad shape'),
                       (dict(w=-1), b'bad shape'), (dict(kh=17, py0=20), b'not supported'), (dict(kw=0), b'not supported'),
                       (dict(ux=9), b'not supported'), (dict(uy=0), b'not supported'), (dict(dx=9), b'not supported'),
                       (dict(dy=0), b'not supported'), (dict(px0=-3, px1=-3), b'not positive'), (dict(kh=7, py0=0, py1=0), b'not positive'),
                       (dict(xs=107), b'stride'), (dict(os=2 * 5 * 8 - 1), b'stride'), (dict(px0=2 ** 31 - 1), b'2^30'),
                       (dict(h=1 << 27, uy=8, xs=1 << 40), b'2^30'), (dict(n=1 << 16, planes=1 << 16, xs=1 << 40, os=1 << 40), b'grid')):
        assert call(**kw) == SR_EINVAL, kw
        err = lib.sr_last_error()
        assert b'sr_upfirdn2d_f32' in err and needle in err, (kw, err)
    th, lds = C.c_int(7), C.c_size_t(7)
    for bad in ((0, 4, 1, 1, 1, 1), (4, 17, 1, 1, 1, 1), (4, 4, 0, 1, 1, 1), (4, 4, 1, 9, 1, 1), (4, 4, 1, 1, 9, 1), (4, 4, 1, 1, 1, 0)):
        assert lib.sr_upfirdn2d_instance(*bad, C.byref(th), C.byref(lds)) == -1 and lib.sr_upfirdn2d_instance(*bad, None, None) == -1
        with pytest.raises(ValueError, match='supported: fp32, filter sides 1..16, factors 1..8'):
            H.upfirdn2d_instance(*bad)


def test_fused_act_refusals_and_cpu_tensors():
    x, b = torch.zeros((2, 3, 4, 5)), torch.zeros(3)
    with pytest.raises(NotImplementedError):
        fused_leaky_relu(x, b)
    with pytest.raises(NotImplementedError):
        FusedLeakyReLU(3)(x)
    with pytest.raises(NotImplementedError):
        S.ScaledLeakyReLU()(x)
    with pytest.raises(NotImplementedError):
        fused_leaky_relu(torch.zeros((2, 3)), b)
    for bad in (lambda: fused_leaky_relu(x.double(), b.double()), lambda: fused_leaky_relu(x.bfloat16(), b.bfloat16()),
                lambda: fused_leaky_relu(x, b.double()), lambda: fused_leaky_relu(x, torch.zeros(4)), lambda: fused_leaky_relu(x, torch.zeros(1)),
                lambda: fused_leaky_relu(x, torch.zeros((3, 1))), lambda: fused_leaky_relu(torch.zeros(3), b),
                lambda: FusedLeakyReLU(4)(x), lambda: fused_leaky_relu(torch.zeros((2, 4)), b)):
        with pytest.raises(ValueError, match='supported: fp32 CUDA tensors of rank >= 2 with the channel on dimension 1'):
            bad()
    m = FusedLeakyReLU(5, negative_slope=0.1, scale=1.5)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [('bias', (5,))] and float(m.bias.detach().abs().max()) == 0.0
    assert (m.negative_slope, m.scale) == (0.1, 1.5) and (FusedLeakyReLU(5).negative_slope, FusedLeakyReLU(5).scale) == (0.2, 2 ** 0.5)
    lib = _lib.load()
    fwd, bwd = lib.sr_fused_bias_act_f32, lib.sr_fused_bias_act_bwd_f32
    for args, needle in (((None, 256, None, 256, 1, 1, 1), b'null'), ((256, 256, None, None, 1, 1, 1), b'null'),
                         ((256, 257, None, 256, 1, 1, 1), b'aligned'), ((256, None, 258, 256, 1, 1, 1), b'aligned'),
                         ((256, 256, None, 256, 0, 1, 1), b'bad shape'), ((256, 256, None, 256, 1, 0, 1), b'bad shape'),
                         ((256, 256, None, 256, 1, 1, 0), b'bad shape'), ((256, 256, None, 256, 1 << 16, 1 << 16, 1), b'grid'),
                         ((256, 256, None, 256, 1, 1, 1 << 62), b'grid')):
        assert fwd(*args, 0.2, 1.0, None) == SR_EINVAL and b'sr_fused_bias_act_f32' in lib.sr_last_error() and needle in lib.sr_last_error(), args
    for args, ws, needle in (((None, 256, 256, 256, 1, 1, 1), (256, 4), b'null'), ((256, None, 256, 256, 1, 1, 1), (256, 4), b'null'),
                             ((256, 256, None, 256, 1, 1, 1), (256, 4), b'null'), ((256, 256, 256, 258, 1, 1, 1), (256, 4), b'aligned'),
                             ((256, 256, 256, 256, 1, 0, 1), (256, 4), b'bad shape'), ((256, 256, 256, 256, 1 << 16, 1 << 16, 1), (256, 4), b'grid'),
                             ((256, 256, 256, 256, 2, 3, 1025), (None, 48), b'workspace')):
        assert bwd(*args, 0.2, 1.0, *ws, None) == SR_EINVAL and needle in lib.sr_last_error(), args
    assert bwd(256, 256, 256, 256, 2, 3, 1025, 0.2, 1.0, 256, 47, None) == SR_ENOSPACE and b'48 needed' in lib.sr_last_error()
