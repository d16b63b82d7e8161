"""The deterministic step-input adjoint on the host side (no GPU): the ABI of include/sr_hip_vsr_det.h (declared, bound, exported, in
no other ledger, each entry point mapped to the GPU test that pins it, one hip_ops wrapper per stream-ordered entry point), the
profiler names at ids 180-182, every refusal of the C function and of the wrapper before any launch (dummy pointers, null stream),
the workspace formula, the compiled resources of the three kernels, the numpy model of the integer arithmetic
(tests/vsr_det_model.py) against the float64 definition under the header's bound on the GPU test's data, its range on the
one-cell flow, and the ``set_autograd(True, deterministic=True)`` contract that needs no device."""
import ast
import ctypes as C
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
from image_restoration_amd.archs.basicvsr_arch import BasicVSR, IconVSR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vsr_bwd_ops_gpu as B  # noqa: E402
import vsr_det_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_vsr_det.h')
SR_EINVAL, SR_ENOSPACE = -1, -3
PINNED = {
    'sr_vsr_prop_input_bwd_det_workspace_bytes': 'tests/test_vsr_det_ops_gpu.py::test_prop_input_bwd_det',
    'sr_vsr_prop_input_bwd_det_f32': 'tests/test_vsr_det_ops_gpu.py::test_prop_input_bwd_det',
}
KERNELS = ('vsr_prop_det_scale_kernel', 'vsr_prop_det_scatter_kernel', 'vsr_prop_det_finish_kernel')


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_every_declared_entry_point_is_bound_exported_and_pinned():
    text = open(HEADER).read()
    declared = set(re.findall(r'\b(?:int|size_t)\s+(sr_[a-z0-9_]+)\s*\(', text))
    assert declared == set(_lib.VSR_DET_SIGNATURES) == set(PINNED) and len(declared) == 2
    others = set()
    for name in dir(_lib):
        if name.endswith('SIGNATURES') and name != 'VSR_DET_SIGNATURES':
            others |= set(getattr(_lib, name))
    assert others and not declared & others
    # the header spells no function of the backward header it builds on, and no other header spells one of these
    assert not any(s in text for s in _lib.VSR_BWD_SIGNATURES)
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'sr_hip_vsr_det.h':
            assert not any(s in open(os.path.join(ROOT, 'include', other)).read() for s in declared), other
    for s, target in PINNED.items():
        path, _, func = target.partition('::')
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        assert func in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, (s, target)
    src = open(os.path.join(ROOT, 'image_restoration_amd', 'hip_ops.py')).read()
    ordered = {s for s, (res, args) in _lib.VSR_DET_SIGNATURES.items() if res is C.c_int and args and args[-1] is C.c_void_p}
    assert ordered == {'sr_vsr_prop_input_bwd_det_f32'}
    assert src.count("_launch_arg('sr_vsr_prop_input_bwd_det_f32'") == 1 and hasattr(H, 'vsr_prop_input_bwd_det')
    # the descriptor embeds the backward header's, then the workspace and its size
    assert C.sizeof(_lib.VsrPropBwdDetDesc) == C.sizeof(_lib.VsrPropBwdDesc) + 16 == 112
    assert _lib.VsrPropBwdDetDesc.workspace.offset == 96 and _lib.VsrPropBwdDetDesc.workspace_bytes.offset == 104
    assert 'sr_hip_vsr_det.h' in open(os.path.join(ROOT, 'image_restoration_amd', 'csrc', 'Makefile')).read()


def test_profiler_ids_180_to_182():
    lib = _lib.load()
    assert [lib.sr_kernel_name(i).decode() for i in (180, 181, 182)] == list(KERNELS)
    assert lib.sr_kernel_name(179).decode() == '' and lib.sr_kernel_name(183).decode() == ''
    assert lib.sr_kernel_name(178).decode() == 'vsr_prop_input_bwd_kernel'


# ------------------------------------------------------------------------------------------------------------ workspace
def test_workspace_formula():
    lib = _lib.load()
    up = lambda v: (v + 255) // 256 * 256   # noqa: E731
    for n, h, w, fb in ((1, 1, 1, 1), (3, 5, 7, 8), (3, 33, 40, 9), (4, 64, 64, 8), (65535, 1, 1, 1)):
        assert lib.sr_vsr_prop_input_bwd_det_workspace_bytes(n, h, w, fb) == up(64 * n * fb * h * w) + up(4 * n)
        assert H.vsr_prop_input_bwd_det_workspace_bytes(n, h, w, fb) == up(64 * n * fb * h * w) + up(4 * n)
    for bad in ((0, 4, 4, 1), (65536, 4, 4, 1), (1, 0, 4, 1), (1, 4, -1, 1), (1, 4, 4, 0), (1, 4, 4, 65535), (1, 16384, 16384, 1)):
        assert lib.sr_vsr_prop_input_bwd_det_workspace_bytes(*bad) == 0, bad


# ------------------------------------------------------------------------------------------------------------ refusals
def _desc(h=4, w=5, fb=2, n=1):
    dd = _lib.VsrPropBwdDetDesc()
    d = dd.d
    win = 8 * fb * h * w
    d.g, d.prev, d.flow, d.dprev, d.dflow = 256, 4096, 8192, 12288, 16384
    d.g_img_stride = d.prev_img_stride = d.dprev_img_stride = win
    d.flow_img_stride = d.dflow_img_stride = 2 * h * w
    d.n, d.h, d.w, d.fb = n, h, w, fb
    dd.workspace = 1 << 20
    dd.workspace_bytes = _lib.load().sr_vsr_prop_input_bwd_det_workspace_bytes(n, h, w, fb)
    return dd


def test_c_abi_refuses_before_any_launch():
    lib = _lib.load()
    fn = lib.sr_vsr_prop_input_bwd_det_f32
    err = lambda: lib.sr_last_error().decode()   # noqa: E731
    assert fn(None, None) == SR_EINVAL and 'null descriptor' in err() and 'sr_vsr_prop_input_bwd_det_f32' in err()
    for field, value, needle in (('g', None, 'null'), ('prev', None, 'null'), ('flow', None, 'null'), ('fb', 0, 'bad shape'),
                                 ('n', 0, 'bad shape'), ('n', 65536, 'bad shape'), ('h', -1, 'bad shape'), ('fb', 65535, 'bad shape'),
                                 ('g', 260, '16-byte aligned'), ('dprev', 12292, '16-byte aligned'), ('flow', 8193, '4-byte aligned'),
                                 ('dflow', 16386, '4-byte aligned'), ('prev_img_stride', 8 * 2 * 20 + 2, 'multiples of 4'),
                                 ('dprev', 256, 'must not be a source'), ('dprev', 4096, 'must not be a source'),
                                 ('dflow', 8192, 'must not be a source')):
        dd = _desc()
        setattr(dd.d, field, value)
        assert fn(C.byref(dd), None) == SR_EINVAL and needle in err(), (field, err())
    dd = _desc()
    dd.d.dprev = dd.d.dflow = None
    assert fn(C.byref(dd), None) == SR_EINVAL and 'nothing to compute' in err()
    for field in ('g_img_stride', 'prev_img_stride', 'dprev_img_stride', 'flow_img_stride', 'dflow_img_stride'):
        dd = _desc(n=2)
        setattr(dd.d, field, getattr(dd.d, field) - 4)
        assert fn(C.byref(dd), None) == SR_EINVAL and 'smaller than the image' in err(), field
    dd = _desc(h=16384, w=16384)
    assert fn(C.byref(dd), None) == SR_EINVAL and 'too large' in err()
    # the workspace: aligned, given and large enough when dprev is asked for
    dd = _desc()
    dd.workspace = (1 << 20) + 16
    assert fn(C.byref(dd), None) == SR_EINVAL and '256-byte aligned' in err()
    dd = _desc()
    dd.workspace_bytes -= 1
    assert fn(C.byref(dd), None) == SR_ENOSPACE and 'sr_vsr_prop_input_bwd_det_workspace_bytes' in err()
    dd = _desc()
    dd.workspace = None
    assert fn(C.byref(dd), None) == SR_ENOSPACE and 'workspace of 0 bytes' in err()


def test_wrapper_refuses_before_the_device():
    flow = torch.zeros(1, 2, 4, 5)
    with pytest.raises(ValueError, match='CB8 windows of one shape'):
        H.vsr_prop_input_bwd_det(None, None, flow)


# --------------------------------------------------------------------------------------------------- compiled kernels
def test_det_kernels_use_no_scratch_no_lds_and_at_most_64_vgprs(tmp_path):
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
        cur = None
        for line in notes.splitlines():
            m = re.match(r'\s+(?:- )?\.(\w+):\s+(\S+)', line)
            if not m:
                continue
            key, val = m.groups()
            if key == 'name' and val.startswith('_Z'):
                cur = found.setdefault(val, {}) if 'vsr_prop_det_' in val else None
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count',
                                             'group_segment_fixed_size'):
                cur[key] = int(val)
    assert len(found) == 3 and all(sum(k in name for name in found) == 1 for k in KERNELS), sorted(found)
    for name, md in found.items():
        assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 and md.get('sgpr_spill_count', 0) == 0, name
        assert md.get('group_segment_fixed_size', 0) == 0 and md['vgpr_count'] <= 64, (name, md)


# ------------------------------------------------------------------------------------------------------ the numpy model
def test_shift_rule():
    # e = ilogb(M) + 1 from the bits, denormals included; L = ceil(log2(4 h w))
    one = int(np.array(1.0, np.float32).view(np.uint32))
    assert M.shift_of(one, 1, 1) == (61 - 1 - 2, 1, 2)
    assert M.shift_of(int(np.array(1.5, np.float32).view(np.uint32)), 5, 7) == (61 - 1 - 8, 1, 8)      # 4 * 35 = 140 <= 256
    assert M.shift_of(int(np.array(0.5, np.float32).view(np.uint32)), 64, 64) == (61 - 0 - 14, 0, 14)
    assert M.shift_of(1, 33, 40) == (61 + 148 - 13, -148, 13)                                          # the smallest denormal, 2^-149
    assert M.shift_of(0x7f7fffff, 33, 40) == (61 - 128 - 13, 128, 13)


@pytest.mark.parametrize('case', [(5, 7, 8, 3), (33, 40, 9, 3), (1, 1, 1, 1)], ids=lambda c: 'x'.join(map(str, c)))
def test_model_is_within_the_header_bound_of_the_float64_definition(case):
    h, w, fb, n = case
    rng, prev, g0, before = M.case_data(h, w, fb, n)
    for kind in B.FLOWS:
        flow = B._flow(kind, rng, n, h, w)
        for name, g in M.g_variants(g0, n).items():
            if name != 'plain' and kind not in ('smooth', 'samecell'):
                continue
            model, info = M.det_dprev(before, g, flow)
            gf = np.where(np.isfinite(g), g, 0.0)
            want_dx, _, count, absterms, _ = B._prop_reference(prev, flow, gf)
            bound = M.det_bound(before, want_dx, count, absterms, [r['k'] for r in info])
            for i in range(n):
                bits = info[i]['bits']
                if bits == 0:
                    assert np.array_equal(model[i], before[i].astype(np.float32)), (kind, name, i)
                elif bits >= M.INF_BITS:
                    assert np.isnan(model[i]).all(), (kind, name, i)
                else:
                    err = np.abs(model[i].astype(np.float64) - (before[i] + want_dx[i]))
                    assert (err <= bound[i]).all(), (kind, name, i, float((err / bound[i]).max()))
                    # (the definition counts a pixel outside the image as a zero term of its own cell; the model skips it)
                    assert (info[i]['count'] <= count[i]).all(), (kind, name, i)
                    # the middle term of the bound is far below an fp32 ulp of M at these sizes
                    m = float(np.array(bits, np.uint32).view(np.float32))
                    assert float(count[i].max()) * 2.0 ** -(info[i]['k'] + 1) <= m * 2.0 ** (2 * info[i]['L'] - 63)
                    if kind == 'samecell':                                   # h * w contributions to one element: no overflow
                        assert int(count[i].max()) == h * w and float(info[i]['absacc'].max()) <= 2.0 ** 59


# ------------------------------------------------------------------------------------------- the set_autograd contract
def test_set_autograd_deterministic_contract_on_cpu_tensors():
    net = BasicVSR(num_feat=8, num_block=1)
    assert net._autograd is False and net._deterministic is False
    assert net.set_autograd(True, deterministic=True) is net and net._autograd is True and net._deterministic is True
    assert net.spynet._autograd is True
    assert net.set_autograd(True) is net and net._deterministic is False          # the default stays the atomic scatter
    assert net.set_autograd(True, True)._deterministic is True
    assert net.set_autograd(False, deterministic=True) is net and net._autograd is False and net._deterministic is False
    x = B_fake(torch.zeros(1, 3, 3, 40, 40))
    net.train()
    with pytest.raises(NotImplementedError, match='follow-up') as e:                # off: the refusal keeps its type and words
        net(x)
    assert 'set_autograd(True)' in str(e.value) and 'VideoRecurrentModel' in str(e.value)
    net.set_autograd(True, deterministic=True)
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        net(torch.zeros(1, 3, 3, 40, 40))
    icon = IconVSR(num_feat=64, num_block=1)
    for kw in (dict(), dict(deterministic=True)):
        with pytest.raises(NotImplementedError, match='follow-up'):
            icon.set_autograd(True, **kw)
    assert icon.set_autograd(False, deterministic=True) is icon and icon._autograd is False and icon._deterministic is False
    # the backward takes the wrapper the switch names
    src = open(os.path.join(ROOT, 'image_restoration_amd', 'archs', 'basicvsr_autograd.py')).read()
    assert 'hip_ops.vsr_prop_input_bwd_det if net._deterministic else hip_ops.vsr_prop_input_bwd' in src


class B_fake(torch.Tensor):
    """A CPU tensor that says it is on the device (as tests/test_vsr_bwd_host.py): reaches the checks behind ``is_cuda``."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    is_cuda = property(lambda self: True)
