"""The deterministic deformable-convolution input gradient on the host side (no GPU): the ABI of include/sr_hip_dcn_det.h (declared,
bound, exported, in no other ledger, each entry point mapped to the GPU test that pins it, one hip_ops wrapper per stream-ordered
entry point), the profiler names at ids 184-186, every refusal of the C function and of the wrapper before any launch (dummy
pointers, null stream), the workspace formula, the compiled resources of the three kernels, the numpy model of the integer
arithmetic (tests/dcn_det_model.py) against the float64 definition (tests/dcn_restate.py) under the header's bound, its range where
every pixel and tap samples one cell, and the switch contracts that need no device."""
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
import yaml

from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H
from image_restoration_amd.archs.arch_util import DCNv2Pack
from image_restoration_amd.archs.edvr_arch import EDVR, PCDAlignment
from image_restoration_amd.ops.dcn import ModulatedDeformConv, ModulatedDeformConvPack

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_det_model as M  # noqa: E402
import dcn_restate as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_dcn_det.h')
SR_EINVAL, SR_ENOSPACE = -1, -3
PINNED = {
    'sr_dcn_bwd_data_det_workspace_bytes': 'tests/test_dcn_det_ops_gpu.py::test_dx_is_the_model_bit_for_bit',
    'sr_dcn_bwd_data_det_f32': 'tests/test_dcn_det_ops_gpu.py::test_dx_is_the_model_bit_for_bit',
}
KERNELS = ('deform_det_scale_kernel', 'deform_det_scatter_kernel', 'deform_det_finish_kernel')


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_every_declared_entry_point_is_bound_exported_and_pinned():
    text = open(HEADER).read()
    declared = set(re.findall(r'\b(?:int|size_t)\s+(sr_[a-z0-9_]+)\s*\(', text))
    assert declared == set(_lib.DCN_DET_SIGNATURES) == set(PINNED) and len(declared) == 2
    others = set()
    for name in dir(_lib):
        if name.endswith('SIGNATURES') and name != 'DCN_DET_SIGNATURES':
            others |= set(getattr(_lib, name))
    assert others and not declared & others
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'sr_hip_dcn_det.h':
            assert not any(s in open(os.path.join(ROOT, 'include', other)).read() for s in declared), other
    for s, target in PINNED.items():
        path, _, func = target.partition('::')
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        assert func in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, (s, target)
    src = open(os.path.join(ROOT, 'image_restoration_amd', 'hip_ops.py')).read()
    ordered = {s for s, (res, args) in _lib.DCN_DET_SIGNATURES.items() if res is C.c_int and args and args[-1] is C.c_void_p}
    assert ordered == {'sr_dcn_bwd_data_det_f32'}
    assert src.count("_launch_arg('sr_dcn_bwd_data_det_f32'") == 1 and hasattr(H, 'dcn_bwd_data_det')
    # the descriptor embeds the atomic entry point's, then the workspace and its size
    assert C.sizeof(_lib.DcnBwdDetDesc) == C.sizeof(_lib.DcnBwdDesc) + 16
    assert _lib.DcnBwdDetDesc.workspace.offset == C.sizeof(_lib.DcnBwdDesc)
    assert _lib.DcnBwdDetDesc.workspace_bytes.offset == C.sizeof(_lib.DcnBwdDesc) + 8
    mk = open(os.path.join(ROOT, 'image_restoration_amd', 'csrc', 'Makefile')).read()
    assert 'sr_hip_dcn_det.h' in mk and os.path.exists(os.path.join(ROOT, 'image_restoration_amd', 'csrc', 'dcn_det_ops.hip'))


def test_profiler_ids_184_to_186():
    lib = _lib.load()
    assert [lib.sr_kernel_name(i).decode() for i in (184, 185, 186)] == list(KERNELS)
    assert lib.sr_kernel_name(183).decode() == '' and lib.sr_kernel_name(187).decode() == ''
    assert lib.sr_kernel_name(182).decode() == 'vsr_prop_det_finish_kernel'


# ------------------------------------------------------------------------------------------------------------ workspace
def test_workspace_formula():
    lib = _lib.load()
    up = lambda v: (v + 255) // 256 * 256   # noqa: E731
    for n, cin, h, w in ((1, 8, 1, 1), (3, 16, 5, 7), (3, 24, 33, 40), (4, 64, 64, 64), (65535, 8, 1, 1), (1, 8 * 7281, 1, 1)):
        want = up(8 * n * cin * h * w) + up(8 * n)
        assert lib.sr_dcn_bwd_data_det_workspace_bytes(n, cin, h, w) == want
        assert H.dcn_bwd_data_det_workspace_bytes(n, cin, h, w) == want
    for bad in ((0, 8, 4, 4), (65536, 8, 4, 4), (1, 0, 4, 4), (1, 12, 4, 4), (1, -8, 4, 4), (1, 8 * 7282, 1, 1), (1, 8, 0, 4), (1, 8, 4, -1),
                (1, 8, 4096, 4096), (1, 64, 1024, 2048), (1, 8, 65536, 65536)):
        assert lib.sr_dcn_bwd_data_det_workspace_bytes(*bad) == 0, bad


# ------------------------------------------------------------------------------------------------------------ refusals
def _desc(h=4, w=5, cin=16, dg=2, n=1):
    dd = _lib.DcnBwdDetDesc()
    b = dd.d
    f = b.fwd
    f.x, f.offset, f.mask = 1 << 20, 2 << 20, 3 << 20
    f.x_img_stride, f.offset_img_stride, f.mask_img_stride = cin * h * w, (18 * dg + 7) // 8 * 8 * h * w, (9 * dg + 7) // 8 * 8 * h * w
    f.n, f.cin, f.cout, f.h, f.w, f.deformable_groups = n, cin, 8, h, w, dg
    f.ksize, f.stride, f.padding, f.dilation, f.groups, f.act_slope = 3, 1, 1, 1, 1, 1.0
    b.dcol, b.dx, b.doffset, b.dmask = 4 << 20, 5 << 20, 6 << 20, 7 << 20
    b.dx_img_stride, b.doffset_img_stride, b.dmask_img_stride = f.x_img_stride, f.offset_img_stride, f.mask_img_stride
    dd.workspace = 8 << 20
    dd.workspace_bytes = _lib.load().sr_dcn_bwd_data_det_workspace_bytes(n, cin, h, w)
    return dd


def test_c_abi_refuses_before_any_launch():
    lib = _lib.load()
    fn = lib.sr_dcn_bwd_data_det_f32
    err = lambda: lib.sr_last_error().decode()   # noqa: E731
    assert fn(None, None) == SR_EINVAL and 'null descriptor' in err() and 'sr_dcn_bwd_data_det_f32' in err()
    # the atomic entry point's own rules of the forward descriptor and of dcol
    for field, value, needle in (('x', None, 'null'), ('offset', None, 'null'), ('mask', None, 'null'), ('n', 0, 'bad shape'),
                                 ('h', -1, 'bad shape'), ('cin', 12, 'multiple of 8'), ('deformable_groups', 4, 'multiple of 8'),
                                 ('ksize', 5, 'not supported'), ('stride', 2, 'not supported'), ('padding', 0, 'not supported'),
                                 ('dilation', 2, 'not supported'), ('groups', 2, 'not supported'), ('x', (1 << 20) + 4, '16-byte aligned'),
                                 ('mask_img_stride', 322, '16-byte aligned'), ('h', 1 << 14, 'too large')):
        dd = _desc()
        setattr(dd.d.fwd, field, value)
        if field == 'h' and value > 0:
            dd.d.fwd.w = 1 << 14
        assert fn(C.byref(dd), None) == SR_EINVAL and needle in err(), (field, err())
    for field, value, needle in (('dcol', None, 'null dcol'), ('dcol', (4 << 20) + 8, '16-byte aligned'), ('dx', (5 << 20) + 4, '16-byte aligned'),
                                 ('doffset', (6 << 20) + 8, '16-byte aligned'), ('dmask', None, 'go together'),
                                 ('doffset', None, 'go together'), ('dx_img_stride', 16 * 20 + 2, 'multiple of 4'),
                                 ('dx', 1 << 20, 'must not be a source'), ('dx', 4 << 20, 'must not be a source')):
        dd = _desc()
        setattr(dd.d, field, value)
        assert fn(C.byref(dd), None) == SR_EINVAL and needle in err(), (field, err())
    dd = _desc(n=2)
    dd.d.dx_img_stride -= 4
    assert fn(C.byref(dd), None) == SR_EINVAL and 'smaller than the image' in err()
    dd = _desc(n=65536)
    assert fn(C.byref(dd), None) == SR_EINVAL and 'bad shape' in err()
    # the workspace: aligned, given and large enough when dx is asked for
    dd = _desc()
    dd.workspace = (8 << 20) + 16
    assert fn(C.byref(dd), None) == SR_EINVAL and '256-byte aligned' in err()
    dd = _desc()
    dd.workspace_bytes -= 1
    assert fn(C.byref(dd), None) == SR_ENOSPACE and 'sr_dcn_bwd_data_det_workspace_bytes' in err()
    dd = _desc()
    dd.workspace = None
    assert fn(C.byref(dd), None) == SR_ENOSPACE and 'workspace of 0 bytes' in err()
    # nothing asked for is nothing done, as for the atomic entry point
    dd = _desc()
    dd.d.dx = dd.d.doffset = dd.d.dmask = None
    dd.workspace = None
    assert fn(C.byref(dd), None) == 0


def test_wrapper_refuses_before_the_device():
    with pytest.raises(ValueError, match='whole CB8 tensor of 9 \\* cin channels'):
        H.dcn_bwd_data_det(None, None, None, None, 1)
    buf = torch.zeros(1, 9, 2, 2, 8)
    with pytest.raises(ValueError, match='whole CB8 tensor of 9 \\* cin channels'):
        H.dcn_bwd_data_det(H.CB8(buf), H.CB8(buf), None, None, 1)
    with pytest.raises(ValueError, match='go together'):
        H.dcn_bwd_data_det(H.CB8(buf), H.CB8(buf, 0, 1), None, None, 1, doffset=H.CB8(buf))


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
                cur = found.setdefault(val, {}) if 'deform_det_' in val else None
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count',
                                             'group_segment_fixed_size'):
                cur[key] = int(val)
    assert len(found) == 3 and all(sum(k in name for name in found) == 1 for k in KERNELS), sorted(found)
    for name, md in found.items():
        assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 and md.get('sgpr_spill_count', 0) == 0, name
        assert md.get('group_segment_fixed_size', 0) == 0 and md['vgpr_count'] <= 64, (name, md)


# ------------------------------------------------------------------------------------------------------ the numpy model
def test_shift_rule():
    one = int(np.array(1.0, np.float32).view(np.uint32))
    half = int(np.array(0.5, np.float32).view(np.uint32))
    big = 0x7f7fffff
    assert M.level_of(1, 1) == 4 and M.level_of(5, 7) == 9 and M.level_of(33, 40) == 14 and M.level_of(256, 256) == 20
    assert M.scale_state(one, 0, True, 1, 1) == ('sum', 61 - 1 - 4, 1, 4)              # a logit mask: the factor is 1
    assert M.scale_state(one, half, False, 5, 7) == ('sum', 61 - 1 - 0 - 9, 1, 9)      # a raw mask: both exponents
    assert M.scale_state(1, 1, False, 33, 40) == ('sum', 61 + 148 + 148 - 14, -296, 14)   # the smallest denormals
    assert M.scale_state(big, big, False, 33, 40) == ('sum', 61 - 256 - 14, 256, 14)
    assert M.scale_state(0, one, False, 5, 7)[0] == 'zero' and M.scale_state(one, 0, False, 5, 7)[0] == 'zero'
    assert M.scale_state(0, 0, True, 5, 7)[0] == 'zero'
    assert M.scale_state(M.INF_BITS, one, False, 5, 7)[0] == 'nan' and M.scale_state(one, M.INF_BITS + 1, True, 5, 7)[0] == 'nan'
    assert M.scale_state(0, M.INF_BITS, False, 5, 7)[0] == 'nan'


def _definition(dcol, offset, m, dg):
    """(dx, count, sum |terms|) of the float64 definition at the device's fp32 positions: autograd of tests/dcn_restate.columns."""
    n, _, cin, h, w = dcol.shape
    off = torch.from_numpy(np.nan_to_num(M.exact_offsets(offset, dg), nan=-1e30, posinf=-1e30, neginf=-1e30))   # nothing sampled
    g = torch.from_numpy(dcol.astype(np.float64)).permute(0, 2, 1, 3, 4).contiguous()
    mm = torch.from_numpy(m.astype(np.float64))
    x = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)
    dx, = torch.autograd.grad(R.columns(x, off, mm, dg), x, g)
    absterms, = torch.autograd.grad(R.columns(x, off, mm.abs(), dg), x, g.abs())
    count, = torch.autograd.grad(R.columns(x, off, torch.ones_like(mm), dg, corner_weights='ones'), x, torch.ones_like(g))
    return dx.numpy(), count.numpy(), absterms.numpy()


def _sigmoid32(logits):
    return (1.0 / (1.0 + np.exp(-logits.astype(np.float64)))).astype(np.float32)


@pytest.mark.parametrize('case', [(5, 7, 16, 1, 3, False), (5, 7, 24, 3, 3, True), (33, 40, 16, 1, 1, False), (33, 40, 24, 3, 1, True),
                                  (1, 1, 8, 1, 1, False), (1, 1, 64, 8, 3, True)], ids=lambda c: 'x'.join(map(str, c)))
def test_model_is_within_the_header_bound_of_the_float64_definition(case):
    h, w, cin, dg, n, logit = case
    rng, dcol0, mask_in = M.case_data(h, w, cin, dg, n, logit)
    m = _sigmoid32(mask_in) if logit else mask_in
    if not logit:
        assert float(m.min()) < -1 and float(m.max()) > 1               # a raw mask outside [0, 1] and negative
    for kind in M.KINDS:
        offset = M.offsets_of(kind, rng, n, dg, h, w)
        variants = {'plain': dcol0}
        if kind in ('dyadic', 'onecell'):
            variants.update(M.dcol_variants(dcol0))
        for name, dcol in variants.items():
            model, info = M.det_dx(dcol, offset, m, dg, logit, mask_in)
            want, count, absterms = _definition(np.where(np.isfinite(dcol), dcol, np.float32(0)), offset, m, dg)
            bound = M.det_bound(want, count, absterms, [r['k'] for r in info])
            for i in range(n):
                rec = info[i]
                if rec['state'] == 'zero':
                    assert rec['md'] == 0 and not model[i].any(), (kind, name, i)
                elif rec['state'] == 'nan':
                    assert np.isnan(model[i]).all(), (kind, name, i)
                else:
                    err = np.abs(model[i].astype(np.float64) - want[i])
                    assert (err <= bound[i]).all(), (kind, name, i, float((err / np.maximum(bound[i], 1e-300)).max()))
                    # (the definition counts a corner of zero weight as a term of its cell; the model skips it)
                    assert (rec['count'] <= count[i]).all() and int(count[i].max()) <= 9 * h * w, (kind, name, i)
                    # the middle term of the bound against the header's worst case 4 Md Mm 2^(2 L - 62)
                    md = float(np.array(rec['md'], np.uint32).view(np.float32))
                    mx = 1.0 if logit else float(np.array(rec['mm'], np.uint32).view(np.float32))
                    assert float(count[i].max()) * 2.0 ** -(rec['k'] + 1) <= 4 * md * mx * 2.0 ** (2 * rec['L'] - 62)
                    if kind == 'onecell':                       # 9 h w terms to one element: no overflow
                        assert int(rec['count'].max()) == 9 * h * w and float(np.abs(rec['acc']).max()) <= 2.0 ** 61
            if name == 'mixed':
                assert [r['state'] for r in info] == ['sum', 'sum', 'zero']
            if name == 'nan':
                assert info[n - 1]['state'] == 'nan'


def test_a_nan_logit_and_a_non_finite_raw_mask_give_nan():
    h, w, cin, dg, n = 5, 7, 8, 1, 3
    rng, dcol, logits = M.case_data(h, w, cin, dg, n, True)
    offset = M.offsets_of('dyadic', rng, n, dg, h, w)
    logits[1, 3, 2, 2] = np.nan
    logits[2, 4, 1, 1] = np.inf                                         # an infinite logit is a mask of 1: finite
    with np.errstate(over='ignore'):
        m = _sigmoid32(logits)
    model, info = M.det_dx(dcol, offset, m, dg, True, logits)
    assert [r['state'] for r in info] == ['sum', 'nan', 'sum'] and np.isnan(model[1]).all() and np.isfinite(model[2]).all()
    raw = logits.copy()
    raw[1, 3, 2, 2] = 0.5
    model, info = M.det_dx(dcol, offset, raw, dg, False)
    assert [r['state'] for r in info] == ['sum', 'sum', 'nan'] and np.isnan(model[2]).all()


# -------------------------------------------------------------------------------------------------- the switch contracts
def test_the_flag_defaults_to_off_and_the_setters_return_self():
    for cls in (ModulatedDeformConv, ModulatedDeformConvPack, DCNv2Pack):
        assert cls.deterministic is False
        m = cls(8, 8, 3, padding=1)
        assert m.deterministic is False and 'deterministic' not in m.state_dict()
    pcd = PCDAlignment(num_feat=8, deformable_groups=1)
    packs = [m for m in pcd.modules() if isinstance(m, DCNv2Pack)]
    assert len(packs) == 4 and not any(m.deterministic for m in packs)
    assert pcd.set_deterministic(True) is pcd and all(m.deterministic is True for m in packs)
    assert pcd.set_deterministic(False) is pcd and not any(m.deterministic for m in packs)
    for dtype in ('fp32', 'bf16'):                                      # bf16 is forward only: the flag is accepted and does nothing
        net = EDVR(num_feat=16, num_frame=3, deformable_groups=2, num_extract_block=1, num_reconstruct_block=1, compute_dtype=dtype)
        packs = [m for m in net.modules() if isinstance(m, DCNv2Pack)]
        assert len(packs) == 4 and not any(m.deterministic for m in packs)
        assert net.set_deterministic() is net and all(m.deterministic is True for m in packs)
        assert net.set_deterministic(False) is net and not any(m.deterministic for m in packs)
    # the backward takes the wrapper the flag names, and the flag travels behind ``windows``
    src = open(os.path.join(ROOT, 'image_restoration_amd', 'hip_autograd.py')).read()
    assert 'H.dcn_bwd_data_det if ctx.deterministic else H.dcn_bwd_data' in src
    with pytest.raises(NotImplementedError):                            # a CPU tensor: the reference's refusal, with the key
        from image_restoration_amd.ops.dcn import modulated_deform_conv
        modulated_deform_conv(torch.zeros(1, 8, 2, 2), torch.zeros(1, 18, 2, 2), torch.zeros(1, 9, 2, 2), torch.zeros(8, 8, 3, 3),
                              None, 1, 1, 1, 1, 1, deterministic=True)
    with pytest.raises(TypeError):                                      # keyword-only
        modulated_deform_conv(torch.zeros(1, 8, 2, 2), torch.zeros(1, 18, 2, 2), torch.zeros(1, 9, 2, 2), torch.zeros(8, 8, 3, 3),
                              None, 1, 1, 1, 1, 1, True)


def test_the_option_files():
    plain = yaml.safe_load(open(os.path.join(ROOT, 'options', 'train', 'EDVR', 'train_EDVR_M_x4_synthetic.yml')))
    det = yaml.safe_load(open(os.path.join(ROOT, 'options', 'train', 'EDVR', 'train_EDVR_M_x4_synthetic_det.yml')))
    assert 'deterministic_backward' not in plain['train'] and det['train'].pop('deterministic_backward') is True
    assert det.pop('name') != plain.pop('name') and det == plain        # the twin differs in the name and the key alone


def _model_opt(**train_keys):
    from collections import OrderedDict as OD
    opt = OD(name='t', model_type='EDVRModel', scale=4, num_gpu=0, manual_seed=0, is_train=True, dist=False, rank=0, world_size=1)
    opt['network_g'] = OD(type='EDVR', num_in_ch=3, num_out_ch=3, num_feat=16, num_frame=3, deformable_groups=2, num_extract_block=1,
                          num_reconstruct_block=1, with_tsa=True)
    opt['path'] = OD(pretrain_network_g=None, strict_load_g=True, resume_state=None)
    tr = OD(ema_decay=0.9)
    tr['optim_g'] = OD(type='Adam', lr=1e-3, weight_decay=0, betas=[0.9, 0.99])
    tr['scheduler'] = OD(type='MultiStepLR', milestones=[2, 3], gamma=0.5)
    tr['pixel_opt'] = OD(type='CharbonnierLoss', loss_weight=1.0, reduction='sum')
    tr.update(train_keys)
    opt['train'] = tr
    return opt


def test_edvr_model_reads_the_key_and_defaults_to_off():
    from image_restoration_amd.models import build_model
    flags = {}
    for name, keys in (('absent', {}), ('false', dict(deterministic_backward=False)), ('true', dict(deterministic_backward=True))):
        model = build_model(_model_opt(**keys))
        flags[name] = [m.deterministic for m in model.get_bare_model(model.net_g).modules() if isinstance(m, DCNv2Pack)]
        assert len(flags[name]) == 4
        if hasattr(model, 'net_g_ema'):                                 # the EMA shadow only ever runs forward: its flag stays off
            assert not any(m.deterministic for m in model.net_g_ema.modules() if isinstance(m, DCNv2Pack))
    assert flags['absent'] == flags['false'] == [False] * 4 and flags['true'] == [True] * 4
    opt = _model_opt(deterministic_backward=True)                       # a test-time model never asks
    opt['is_train'] = False
    model = build_model(opt)
    assert not any(m.deterministic for m in model.net_g.modules() if isinstance(m, DCNv2Pack))
