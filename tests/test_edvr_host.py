"""EDVR on the host side (no GPU): registry and state_dict layout against the lists recorded from the reference's constructors
(tests/golden/g_z_edvr.npz, tools/make_edvr_golden.py), every refusal, the ledger, profiler names and compiled resources of
include/sr_hip_edvr.h, and the restated dispatch of sr_conv3x3s2_f32.

Dispatch.  The instance sr_conv3x3s2_f32 runs (COT 32-cout sub-tiles, tiles of 4 * PT output rows) cannot be observed on the
device (every launch has profiler id 114), so it is restated here (_s2_instance, from sr_conv3x3s2_f32 in edvr_ops.hip) and the
set the restatement can produce is checked against the instances the code object holds; tests/test_edvr_ops_gpu.py uses it to
show that its cases reach all four.

LDS.  The kernel's LDS is dynamic (the notes' group_segment_fixed_size is 0), so the library answers for it:
sr_conv3x3s2_lds_bytes runs the launch's own dispatch and returns the constant the launch passes as its dynamic LDS size; it is
held to the four sizes the file header of edvr_ops.hip states, 2 * (roundup1024((2 * 4 PT + 1) * 65 * 32) + 9 COT * 1024),
within the 160 KiB of a CU."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from image_restoration_amd import _lib, build_network
from image_restoration_amd import hip_ops as H
from image_restoration_amd.archs.edvr_arch import EDVR, PCDAlignment, PredeblurModule, TSAFusion
from image_restoration_amd.utils.registry import ARCH_REGISTRY

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dcn_host import _code_object_kernels  # noqa: E402
import edvr_restate as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_edvr.h')
SOURCE = os.path.join(ROOT, 'image_restoration_amd', 'csrc', 'edvr_ops.hip')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'g_z_edvr.npz')


def _cdiv(a, b):
    return -(-a // b)


def _s2_instance(cout, n, h, w):
    """(COT, PT) of one sr_conv3x3s2_f32 launch on an h x w source (edvr_ops.hip, sr_conv3x3s2_f32): the rule of
    convd_dispatch on the OUTPUT size ho = (h + 1) // 2, wo = (w + 1) // 2."""
    ho, wo = (h + 1) // 2, (w + 1) // 2
    cp = (cout + 31) // 32 * 32
    gc = 64 if cp % 64 == 0 else 32
    groups = cp // gc
    small = _cdiv(wo, 32) * _cdiv(ho, 8) * n * groups < 256 and ho > 4
    return gc // 32, (1 if small else 2)


# ------------------------------------------------------------------------------------------------- registry and layout
def _entries(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def test_registry_and_build_network():
    assert ARCH_REGISTRY.get('EDVR') is EDVR
    net = build_network({'type': 'EDVR', 'num_feat': 16, 'deformable_groups': 2, 'num_frame': 3, 'num_extract_block': 1,
                         'num_reconstruct_block': 1})
    assert isinstance(net, EDVR) and net.center_frame_idx == 1
    for name in ('PCDAlignment', 'TSAFusion', 'PredeblurModule'):
        assert name not in ARCH_REGISTRY


@pytest.mark.parametrize('name,kw', [('default', {}), ('predeblur', dict(with_predeblur=True, hr_in=True))])
def test_state_dict_layout_is_the_reference(name, kw):
    want = json.loads(str(np.load(GOLDEN)[f'layout_{name}']))
    got = _entries(EDVR(**kw))
    assert len(want) == {'default': 144, 'predeblur': 186}[name]
    assert got == want


def test_submodule_layouts_and_constructor_defaults():
    g = np.load(GOLDEN)
    assert [k for k, _ in _entries(TSAFusion(16, 3, 1))] == [str(k) for k in g['tsa_keys']]
    assert [k for k, _ in _entries(PredeblurModule(3, 16, hr_in=True))] == [str(k) for k in g['pre_keys']]
    for i, (k, s) in enumerate(_entries(TSAFusion(16, 3, 1))):
        assert tuple(s) == g[f'tsa_w{i}'].shape, k
    for i, (k, s) in enumerate(_entries(PredeblurModule(3, 16, hr_in=True))):
        assert tuple(s) == g[f'pre_w{i}'].shape, k
    m = EDVR()
    assert (m.center_frame_idx, m.hr_in, m.with_predeblur, m.with_tsa) == (2, False, False, True)
    assert EDVR(num_frame=7).center_frame_idx == 3 and EDVR(center_frame_idx=0).center_frame_idx == 0
    assert not hasattr(EDVR(with_tsa=False).fusion, 'temporal_attn1')
    assert tuple(EDVR(with_tsa=False).fusion.weight.shape) == (64, 320, 1, 1)
    sd = {k: torch.randn_like(v) for k, v in m.state_dict().items()}
    m2 = EDVR()
    m2.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m2.state_dict().items())


def test_restatement_is_the_reference_in_float64():
    """tests/edvr_restate.py, the yardstick of the whole-network GPU test, restates the reference: in float64 on the CPU it
    reproduces the output the reference's own TSAFusion and PredeblurModule gave when the golden was recorded."""
    g = np.load(GOLDEN)
    for tag, fn in (('tsa', lambda p, x: E.tsa_fusion(p, x, 1)), ('pre', lambda p, x: E.predeblur(p, x, True))):
        sd = {str(k): torch.from_numpy(g[f'{tag}_w{i}']).double() for i, k in enumerate(g[f'{tag}_keys'])}
        x = torch.from_numpy(g[f'{tag}_x']).double().requires_grad_(True)
        y = fn(sd, x)
        y64 = torch.from_numpy(g[f'{tag}_y'])
        assert float((y.detach() - y64).norm() / y64.norm()) < 1e-13, tag
        dx, = torch.autograd.grad(y, x, torch.from_numpy(g[f'{tag}_gy']).double())
        dx64 = torch.from_numpy(g[f'{tag}_dx']).double()
        assert float((dx - dx64).norm() / dx64.norm()) < 2.0 ** -24, tag   # the golden's gradients are rounded to float32


# ------------------------------------------------------------------------------------------------------------ refusals
def _small(**kw):
    args = dict(num_feat=16, deformable_groups=2, num_frame=3, num_extract_block=1, num_reconstruct_block=1)
    args.update(kw)
    return EDVR(**args)


@pytest.mark.parametrize('h,w', [(6, 8), (8, 10), (7, 7)])
def test_sizes_not_divisible_by_4_are_refused(h, w):
    with pytest.raises(ValueError, match='multiples of 4'):
        _small()(torch.zeros(1, 3, 3, h, w))
    with pytest.raises(ValueError, match='multiples of 4'):
        TSAFusion(16, 3, 1)(torch.zeros(1, 3, 16, h, w))
    with pytest.raises(ValueError, match='multiples of 4'):
        PredeblurModule(3, 16)(torch.zeros(1, 3, h, w))


@pytest.mark.parametrize('h,w', [(8, 16), (16, 24), (20, 32)])
def test_hr_in_sizes_not_divisible_by_16_are_refused(h, w):
    with pytest.raises(ValueError, match='multiples of 16'):
        _small(hr_in=True, with_predeblur=True)(torch.zeros(1, 3, 3, h, w))
    with pytest.raises(ValueError, match='multiples of 16'):
        PredeblurModule(3, 16, hr_in=True)(torch.zeros(1, 3, h, w))


@pytest.mark.parametrize('kw', [dict(num_feat=12), dict(num_feat=32, deformable_groups=8), dict(num_feat=24, deformable_groups=2),
                                dict(num_feat=64, deformable_groups=3), dict(num_feat=16, deformable_groups=0)])
def test_channel_counts_the_deformable_convs_refuse(kw):
    with pytest.raises(ValueError):
        _small(**kw)
    if kw.get('deformable_groups', 2) > 0:
        with pytest.raises(ValueError):
            PCDAlignment(kw['num_feat'], kw.get('deformable_groups', 2))


def test_hr_in_needs_the_predeblur_module():
    """Without the pre-deblur module nothing brings a high-resolution input down by 4, and the x4 output cannot be added to
    the centre frame (the reference fails there with a shape error in its last line)."""
    with pytest.raises(ValueError, match='with_predeblur'):
        _small(hr_in=True)
    assert _small(hr_in=True, with_predeblur=True).hr_in


def test_tsa_needs_whole_blocks_and_its_frame_count():
    with pytest.raises(ValueError, match='multiple of 8'):
        TSAFusion(12, 3, 1)
    with pytest.raises(ValueError, match='num_feat'):
        TSAFusion(16, 3, 1)(torch.zeros(1, 3, 8, 4, 4))
    with pytest.raises(ValueError, match='num_frame'):
        _small()(torch.zeros(1, 5, 3, 8, 8))


def test_cpu_tensors_are_not_implemented_and_bf16_is_refused():
    with pytest.raises(NotImplementedError):
        _small()(torch.zeros(1, 3, 3, 8, 8))
    with pytest.raises(NotImplementedError):
        TSAFusion(16, 3, 1)(torch.zeros(1, 3, 16, 8, 8))
    with pytest.raises(NotImplementedError):
        PredeblurModule(3, 16)(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match='supported: fp32'):
        _small()(torch.zeros(1, 3, 3, 8, 8, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match='supported: fp32'):
        TSAFusion(16, 3, 1)(torch.zeros(1, 3, 16, 8, 8, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match='supported: fp32'):
        PredeblurModule(3, 16)(torch.zeros(1, 3, 8, 8, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        _small()(torch.zeros(3, 3, 8, 8))


class _Win:
    """A stand-in for a CB8 window: the wrappers check shapes before they touch the device."""
    def __init__(self, n, cbn, h, w):
        self.n, self.cbn, self.h, self.w, self.channels = n, cbn, h, w, cbn * 8


def test_wrappers_raise_value_error_on_bad_arguments():
    with pytest.raises(ValueError):
        H.zero_insert2(_Win(1, 1, 3, 3), 8, 8)
    with pytest.raises(ValueError):
        H.tsa_corr(_Win(5, 1, 4, 4), _Win(2, 1, 4, 4), _Win(5, 1, 4, 4), 3)
    with pytest.raises(ValueError):
        H.tsa_gate(_Win(1, 1, 4, 4), _Win(1, 2, 4, 4), _Win(1, 1, 4, 4))
    with pytest.raises(ValueError):
        H.pool3x3s2_bwd(_Win(1, 1, 4, 4), _Win(1, 1, 2, 2))


# ------------------------------------------------------------------------------------------------------------- the ABI
NAMES = ['conv3x3s2_f32_kernel', 'cb8_zero_insert2_kernel', 'pool3x3s2_fwd_kernel', 'pool3x3s2_bwd_kernel', 'tsa_corr_fwd_kernel',
         'tsa_corr_bwd_kernel', 'tsa_corr_bwd_ref_kernel', 'tsa_gate_fwd_kernel', 'tsa_gate_bwd_kernel']


def test_every_declared_entry_point_is_bound_and_exported():
    declared = set(re.findall(r'\b(?:int|size_t)\s+(sr_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(_lib.EDVR_SIGNATURES) and len(declared) == 9
    others = set(_lib.SIGNATURES) | set(_lib.RIDNET_SIGNATURES) | set(_lib.GFPGAN_SIGNATURES) | set(_lib.EDSR_SIGNATURES) \
        | set(_lib.CA_BF16_SIGNATURES) | set(_lib.DCN_SIGNATURES)
    assert not declared & others
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    base = open(os.path.join(ROOT, 'include', 'sr_hip.h')).read()
    assert not any(s in base for s in declared)   # declared apart from sr_hip.h


def test_descriptor_matches_the_header():
    body = re.search(r'typedef struct sr_conv3x3s2_desc \{(.*?)\} sr_conv3x3s2_desc;', open(HEADER).read(), re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            fields += re.findall(r'(\w+)\s*(?:,|$)', decl.strip())
    assert fields == [('in' if n == 'in_' else n) for n, _ in _lib.ConvS2Desc._fields_]


def test_profiler_ids_resolve_and_113_stays_empty():
    lib = _lib.load()
    assert [lib.sr_kernel_name(i).decode() for i in range(114, 123)] == NAMES
    assert lib.sr_kernel_name(113).decode() == '' and lib.sr_kernel_name(123).decode() == ''
    assert lib.sr_kernel_name(112).decode() == 'dcn_bwd_data_kernel'


SR_EINVAL = -1   # include/sr_hip.h


def test_bad_arguments_return_einval():
    assert re.search(r'#define SR_EINVAL \(-1\)', open(os.path.join(ROOT, 'include', 'sr_hip.h')).read())
    lib = _lib.load()
    d = _lib.ConvS2Desc()
    assert lib.sr_conv3x3s2_f32(d, None) == SR_EINVAL and b'sr_conv3x3s2_f32' in lib.sr_last_error()
    assert lib.sr_conv3x3s2_f32(None, None) == SR_EINVAL
    d.in_, d.wpacked, d.out, d.cin_pad, d.cout, d.n, d.in_h, d.in_w = 16, 16, 16, 12, 8, 1, 4, 4
    assert lib.sr_conv3x3s2_f32(d, None) == SR_EINVAL and b'multiple of 8' in lib.sr_last_error()
    d.cin_pad, d.out = 8, 8
    assert lib.sr_conv3x3s2_f32(d, None) == SR_EINVAL and b'aligned' in lib.sr_last_error()
    assert lib.sr_cb8_zero_insert2_f32(None, 0, None, 0, 1, 1, 4, 4, None) == SR_EINVAL
    assert lib.sr_pool3x3s2_fwd_f32(None, 0, None, 0, None, 0, 1, 1, 4, 4, None) == SR_EINVAL
    assert lib.sr_pool3x3s2_bwd_f32(None, 0, None, 0, None, 0, None, 0, 1, 1, 4, 4, None) == SR_EINVAL
    assert lib.sr_tsa_corr_fwd_f32(16, 0, 16, 0, 16, 0, 16, 16, 0, 1, 1, 12, 4, 4, None) == SR_EINVAL
    assert b'multiple of 8' in lib.sr_last_error()
    assert lib.sr_tsa_corr_bwd_f32(None, 0, None, 0, None, 0, None, 0, None, None, None, 0, None, 0, None, 0, 1, 1, 8, 4, 4,
                                   None) == SR_EINVAL
    assert lib.sr_tsa_gate_fwd_f32(16, 0, 16, 0, 16, 0, 16, 0, 1, 0, 4, 4, None) == SR_EINVAL
    assert lib.sr_tsa_gate_bwd_f32(16, 0, 16, 0, 16, 0, 16, 0, 8, 0, 1, 1, 4, 4, None) == SR_EINVAL   # misaligned d_attn


class _Pack:
    """A stand-in for a weight image: conv3x3s2 checks it before it touches the device."""
    def __init__(self, mode=0, ksize=3, src_channels=8, cout=8):
        self.mode, self.ksize, self.src_channels, self.cout = mode, ksize, src_channels, cout


def test_conv3x3s2_wrapper_raises_value_error_on_bad_arguments():
    with pytest.raises(ValueError, match='forward image of a 3x3'):
        H.conv3x3s2(_Win(1, 1, 4, 4), _Pack(mode=1))
    with pytest.raises(ValueError, match='forward image of a 3x3'):
        H.conv3x3s2(_Win(1, 1, 4, 4), _Pack(ksize=1))
    with pytest.raises(ValueError, match='16 channels'):
        H.conv3x3s2(_Win(1, 2, 4, 4), _Pack(src_channels=8))
    with pytest.raises(ValueError, match='does not fit'):
        H.conv3x3s2(_Win(1, 1, 5, 7), _Pack(), out=_Win(1, 1, 2, 3))      # (5, 7) gives 3 x 4
    with pytest.raises(ValueError, match='does not fit'):
        H.conv3x3s2(_Win(1, 1, 4, 4), _Pack(cout=24), out=_Win(1, 2, 2, 2))


# -------------------------------------------------------------------------------------------------------- code objects
def test_new_kernels_use_no_scratch_no_spills_and_the_dispatch_reaches_the_instances_built(tmp_path):
    found = {k: v for k, v in _code_object_kernels(tmp_path, '').items() if any(n in k for n in NAMES)}
    conv = sorted(k for k in found if 'conv3x3s2_f32_kernel' in k)
    built = {tuple(int(v) for v in re.search(r'ILi(\d)ELi(\d)E', k).groups()) for k in conv}
    assert built == {(1, 1), (1, 2), (2, 1), (2, 2)} and len(conv) == 4, conv
    assert len(found) == 4 + 8, sorted(found)
    for name, md in found.items():
        assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 \
            and md.get('sgpr_spill_count', 0) == 0 and md['vgpr_count'] <= 256, (name, md)
        assert md.get('group_segment_fixed_size', 0) == 0, (name, md)   # the conv's LDS is dynamic, the others use none
    reached = {_s2_instance(cout, n, h, w) for cout in (24, 32, 64, 96) for n, h, w in ((2, 13, 70), (2, 18, 132), (1, 2, 2),
                                                                                        (5, 180, 320), (1, 7, 9))}
    assert reached == built
    assert _s2_instance(64, 5, 180, 320) == (2, 2) and _s2_instance(64, 2, 18, 132) == (2, 1) and _s2_instance(24, 2, 13, 70) == (1, 1)
    assert _s2_instance(64, 1, 7, 9) == (2, 2)      # ho = 4 never takes 4-row tiles
    assert _s2_instance(64, 64, 9, 256)[1] == 2 and _s2_instance(64, 63, 9, 256)[1] == 1   # 256 and 252 tiles at the 8-row rule


def test_lds_bytes_the_launch_requests():
    """sr_conv3x3s2_lds_bytes runs the launch's own dispatch (s2_plan) and returns the constant the launch passes as its dynamic
    LDS size: per instance the value the file header of edvr_ops.hip states, which is the layout's formula."""
    lib = _lib.load()
    text = open(SOURCE).read()
    stated = {(int(c), int(p)): int(v) for c, p, v in re.findall(r'COT (\d) / PT (\d)\s+(\d+)', text.split('#include')[0])}
    formula = {(cot, pt): 2 * (_cdiv((2 * 4 * pt + 1) * 65 * 32, 1024) * 1024 + 9 * cot * 1024) for cot in (1, 2) for pt in (1, 2)}
    assert stated == formula == {(1, 1): 57344, (1, 2): 90112, (2, 1): 75776, (2, 2): 108544}
    seen = set()
    for cout in (24, 32, 64, 96):
        for n, h, w in ((2, 13, 70), (2, 18, 132), (1, 2, 2), (5, 180, 320), (1, 7, 9), (32, 35, 130), (64, 9, 256), (63, 9, 256)):
            inst = _s2_instance(cout, n, h, w)
            seen.add(inst)
            assert lib.sr_conv3x3s2_lds_bytes(cout, n, h, w) == stated[inst], (cout, n, h, w)
    assert seen == set(stated) and max(stated.values()) <= 160 * 1024
    assert lib.sr_conv3x3s2_lds_bytes(64, 5, 180, 320) == 108544      # the default network's L1 -> L2 launch
    assert lib.sr_conv3x3s2_lds_bytes(0, 1, 4, 4) == 0 and lib.sr_conv3x3s2_lds_bytes(64, 1, 0, 4) == 0
