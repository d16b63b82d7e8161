"""The host side of EDVR's bf16 inference path (no GPU): the ABI of include/sr_hip_edvr_bf16.h (declared, bound, exported), the
profiler names, every refusal ahead of any launch, the dispatch function, the compiled resources read from the code object,
the constructor key, and generate_frame_indices."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H
from image_restoration_amd.archs.edvr_arch import EDVR
from image_restoration_amd.data.data_util import generate_frame_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_edvr_bf16.h')
SR_EINVAL = -1   # include/sr_hip.h
ABI = ['sr_dcn_fwd_bf16', 'sr_dcn_bf16_lds_bytes', 'sr_conv1x1_packed_weight_elems_bf16', 'sr_conv1x1_pack_bf16', 'sr_conv1x1_bf16',
       'sr_cb16_subsample2_bf16', 'sr_pool3x3s2_fwd_bf16', 'sr_tsa_corr_fwd_bf16', 'sr_tsa_gate_fwd_bf16']
NAMES = ['deform16_fwd_kernel', 'pw16_conv_kernel', 'cb16_subsample2_kernel', 'pool16_s2_fwd_kernel', 'tsa16_corr_kernel',
         'tsa16_gate_kernel']
SMALL = dict(num_feat=16, num_frame=3, deformable_groups=2, num_extract_block=1, num_reconstruct_block=1)


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_every_declared_entry_point_is_bound_and_exported():
    declared = set(re.findall(r'\b(?:int|size_t)\s+(sr_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(ABI) == set(_lib.EDVR_BF16_SIGNATURES)
    others = set(_lib.SIGNATURES) | set(_lib.RIDNET_SIGNATURES) | set(_lib.GFPGAN_SIGNATURES) | set(_lib.EDSR_SIGNATURES) \
        | set(_lib.CA_BF16_SIGNATURES) | set(_lib.DCN_SIGNATURES) | set(_lib.EDVR_SIGNATURES)
    assert not declared & others
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    for other in ('sr_hip.h', 'sr_hip_dcn.h', 'sr_hip_edvr.h'):
        text = open(os.path.join(ROOT, 'include', other)).read()
        assert not any(s in text for s in declared), other      # declared apart from the existing headers


def test_descriptor_matches_the_header():
    text = open(HEADER).read()
    body = re.search(r'typedef struct sr_dcn_bf16_desc \{(.*?)\} sr_dcn_bf16_desc;', text, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            fields += re.findall(r'(\w+)\s*(?:,|$)', decl.strip())
    assert fields == [n for n, _ in _lib.DcnBf16Desc._fields_]
    assert 'cpg = cin / deformable_groups a multiple of 8' in text    # the constraint is stated in the header


def test_profiler_ids_resolve_and_the_unnamed_ids_stay_unnamed():
    lib = _lib.load()
    assert [lib.sr_kernel_name(i).decode() for i in range(124, 130)] == NAMES
    for i in (97, 101, 105, 109, 113, 123, 130):
        assert lib.sr_kernel_name(i).decode() == '', i
    assert lib.sr_kernel_name(122).decode() == 'tsa_gate_bwd_kernel'


# ----------------------------------------------------------------------------------------------------------- refusals
def _dcn_desc(**kw):
    d = _lib.DcnBf16Desc()
    d.x, d.offset, d.mask, d.wpacked, d.out = 256, 256, 256, 256, 256
    d.n, d.cin, d.cout, d.h, d.w, d.deformable_groups = 1, 64, 64, 4, 4, 8
    d.x_img_stride, d.out_img_stride, d.offset_img_stride, d.mask_img_stride = 64 * 16, 64 * 16, 144 * 16, 72 * 16
    d.ksize, d.stride, d.padding, d.dilation, d.groups, d.act_slope = 3, 1, 1, 1, 1, 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize('kw,needle', [
    (dict(cin=48, deformable_groups=4, x_img_stride=48 * 16), b'multiple of 8'),          # cpg 12
    (dict(cin=24, deformable_groups=3, x_img_stride=24 * 16), b'multiple of 16'),         # cin % 16
    (dict(ksize=5), b'not supported'), (dict(ksize=1), b'not supported'), (dict(stride=2), b'not supported'),
    (dict(padding=0), b'not supported'), (dict(dilation=2), b'not supported'), (dict(groups=2), b'not supported'),
    (dict(x=0), b'null'), (dict(offset=0), b'null'), (dict(mask=0), b'null'), (dict(wpacked=0), b'null'), (dict(out=0), b'null'),
    (dict(x=264), b'aligned'), (dict(out=264), b'aligned'), (dict(wpacked=264), b'aligned'), (dict(bpacked=8), b'aligned'),
    (dict(offset=258), b'aligned'), (dict(x_img_stride=64 * 16 + 4), b'aligned'),
    (dict(x_img_stride=64 * 16 - 8), b'smaller than the image'), (dict(out_img_stride=64 * 16 - 8), b'smaller than the image'),
    (dict(offset_img_stride=144 * 16 - 1), b'smaller than the image'), (dict(mask_img_stride=72 * 16 - 1), b'smaller than the image'),
    (dict(h=0), b'bad shape'), (dict(w=0), b'bad shape'), (dict(n=0), b'bad shape'), (dict(cout=0), b'bad shape'),
    (dict(deformable_groups=0), b'bad shape'),
])
def test_dcn_refusals(kw, needle):
    """Every refusal returns SR_EINVAL with its message before anything is launched (the test needs no GPU; the pointers are small
    integers that no kernel could read)."""
    lib = _lib.load()
    assert lib.sr_dcn_fwd_bf16(C.byref(_dcn_desc(**kw)), None) == SR_EINVAL
    err = lib.sr_last_error()
    assert b'sr_dcn_fwd_bf16' in err and needle in err, err
    assert lib.sr_dcn_fwd_bf16(None, None) == SR_EINVAL


def test_the_other_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    ok = dict(x=256, xs=16 * 16 * 2, w=256, b=256, out=256, os=16 * 16, n=1, cin=32, cout=16, h=4, wd=4)

    def pw(**kw):
        a = dict(ok, **kw)
        return lib.sr_conv1x1_bf16(a['x'], a['xs'], a['w'], a['b'], a['out'], a['os'], a['n'], a['cin'], a['cout'], a['h'], a['wd'], 1.0, None)
    for kw, needle in ((dict(cin=24), b'multiple of 16'), (dict(x=0), b'null'), (dict(w=0), b'null'), (dict(out=0), b'null'),
                       (dict(x=260), b'aligned'), (dict(b=260), b'aligned'), (dict(xs=16 * 16 * 2 - 8), b'stride'),
                       (dict(os=16 * 16 - 8), b'stride'), (dict(xs=16 * 16 * 2 + 4), b'stride'), (dict(h=0), b'bad shape'),
                       (dict(wd=0), b'bad shape'), (dict(cout=0), b'bad shape')):
        assert pw(**kw) == SR_EINVAL and needle in lib.sr_last_error(), (kw, lib.sr_last_error())
    assert lib.sr_conv1x1_pack_bf16(256, None, 16, 24, 256, None, None) == SR_EINVAL and b'multiple of 16' in lib.sr_last_error()
    assert lib.sr_conv1x1_pack_bf16(None, None, 16, 32, 256, None, None) == SR_EINVAL
    # subsample / pool / gate: (pointers..., n, cb, h, w)
    assert lib.sr_cb16_subsample2_bf16(None, 256, 256, 64, 1, 1, 4, 4, None) == SR_EINVAL
    assert lib.sr_cb16_subsample2_bf16(256, 256, 264, 64, 1, 1, 4, 4, None) == SR_EINVAL and b'aligned' in lib.sr_last_error()
    assert lib.sr_cb16_subsample2_bf16(256, 248, 256, 64, 1, 1, 4, 4, None) == SR_EINVAL and b'stride' in lib.sr_last_error()
    assert lib.sr_cb16_subsample2_bf16(256, 256, 256, 56, 1, 1, 4, 4, None) == SR_EINVAL and b'stride' in lib.sr_last_error()
    assert lib.sr_cb16_subsample2_bf16(256, 256, 256, 64, 1, 1, 0, 4, None) == SR_EINVAL
    assert lib.sr_pool3x3s2_fwd_bf16(256, 256, 256, 128, None, 128, 1, 1, 4, 4, None) == SR_EINVAL
    assert lib.sr_pool3x3s2_fwd_bf16(256, 256, 256, 128, 264, 128, 1, 1, 4, 4, None) == SR_EINVAL and b'aligned' in lib.sr_last_error()
    assert lib.sr_pool3x3s2_fwd_bf16(256, 256, 256, 128, 256, 56, 1, 1, 4, 4, None) == SR_EINVAL and b'stride' in lib.sr_last_error()
    assert lib.sr_pool3x3s2_fwd_bf16(256, 256, 256, 128, 256, 128, 1, 1, 4, 0, None) == SR_EINVAL
    assert lib.sr_tsa_corr_fwd_bf16(256, 384, 256, 384, 256, 384, None, 256, 384, 1, 1, 24, 4, 4, None) == SR_EINVAL
    assert b'multiple of 16' in lib.sr_last_error()
    assert lib.sr_tsa_corr_fwd_bf16(256, 256, 256, 256, 256, 256, None, None, 256, 1, 1, 16, 4, 4, None) == SR_EINVAL
    assert lib.sr_tsa_corr_fwd_bf16(256, 256, 256, 248, 256, 256, None, 256, 256, 1, 1, 16, 4, 4, None) == SR_EINVAL
    assert b'stride' in lib.sr_last_error()
    assert lib.sr_tsa_corr_fwd_bf16(256, 256, 256, 256, 256, 256, 258, 256, 256, 1, 1, 16, 4, 4, None) == SR_EINVAL
    assert lib.sr_tsa_gate_fwd_bf16(256, 256, 256, 256, 264, 256, 256, 256, 1, 1, 4, 4, None) == SR_EINVAL and b'aligned' in lib.sr_last_error()
    assert lib.sr_tsa_gate_fwd_bf16(256, 256, 256, 256, 256, 256, 256, 248, 1, 1, 4, 4, None) == SR_EINVAL and b'stride' in lib.sr_last_error()
    assert lib.sr_tsa_gate_fwd_bf16(256, 256, 256, 256, 256, 256, 256, 256, 1, 0, 4, 4, None) == SR_EINVAL


class _Win:
    """A stand-in for a CB16 window: the wrappers check shapes before they touch the device."""
    def __init__(self, n, cbn, h, w):
        self.n, self.cbn, self.h, self.w, self.channels = n, cbn, h, w, cbn * 16
        self.ptr, self.img_stride, self.device = 256, cbn * h * w * 16, None


class _Pack:
    def __init__(self, ksize=3, src_channels=16, cout=16):
        self.mode, self.ksize, self.src_channels, self.cout, self.w, self.b = 0, ksize, src_channels, cout, None, None


def test_wrappers_raise_value_error_on_bad_arguments():
    with pytest.raises(ValueError, match='1x1 weight'):
        H.conv1x1_bf16(_Win(1, 1, 4, 4), _Pack(ksize=3))
    with pytest.raises(ValueError, match='32 channels'):
        H.conv1x1_bf16(_Win(1, 2, 4, 4), _Pack(ksize=1))
    with pytest.raises(ValueError, match='does not fit'):
        H.conv1x1_bf16(_Win(1, 1, 4, 4), _Pack(ksize=1, cout=24), out=_Win(1, 1, 4, 4))
    with pytest.raises(ValueError, match='3x3 weight'):
        H.dcn_fwd_bf16(_Win(1, 1, 4, 4), None, None, _Pack(ksize=1), 2)
    with pytest.raises(ValueError, match='multiple of 8'):
        H.dcn_fwd_bf16(_Win(1, 3, 4, 4), None, None, _Pack(src_channels=48), 4)
    with pytest.raises(ValueError, match='does not fit'):
        H.subsample2_bf16(_Win(1, 1, 5, 7), out=_Win(1, 1, 2, 3))
    with pytest.raises(ValueError, match='does not fit'):
        H.pool3x3s2_bf16(_Win(1, 1, 4, 4), out=_Win(1, 1, 2, 2))
    with pytest.raises(ValueError, match='frames are not'):
        H.tsa_corr_bf16(_Win(5, 1, 4, 4), _Win(2, 1, 4, 4), _Win(5, 1, 4, 4), 3)
    with pytest.raises(ValueError, match='shapes differ'):
        H.tsa_gate_bf16(_Win(1, 1, 4, 4), _Win(1, 1, 4, 4), _Win(1, 2, 4, 4))


# ------------------------------------------------------------------------------------------------- dispatch and sizes
def test_dispatch_function_and_pack_sizes():
    """COT = 2 when roundup32(cout) is a multiple of 64, else 1; 4-row tiles; LDS = 36 KiB of columns + 2 * 9 * COT KiB of weights."""
    assert H.dcn_bf16_instance(64, 5, 180, 320) == (2, 4, 36864 + 2 * 18432) == (2, 4, 73728)
    assert H.dcn_bf16_instance(16, 1, 1, 1) == (1, 4, 36864 + 2 * 9216) == (1, 4, 55296)
    assert H.dcn_bf16_instance(24, 1, 9, 33)[0] == 1 and H.dcn_bf16_instance(32, 2, 5, 7)[0] == 1
    assert H.dcn_bf16_instance(96, 1, 8, 8)[0] == 1 and H.dcn_bf16_instance(128, 1, 8, 8)[0] == 2
    assert H.dcn_bf16_instance(0, 1, 8, 8)[2] == 0 and H.dcn_bf16_instance(64, 1, 0, 8)[2] == 0
    assert 2 * 73728 <= 160 * 1024          # two workgroups per CU at either COT
    lib = _lib.load()
    assert lib.sr_conv1x1_packed_weight_elems_bf16(64, 320) == 64 * 320
    assert lib.sr_conv1x1_packed_weight_elems_bf16(1, 16) == 32 * 16 and lib.sr_conv1x1_packed_weight_elems_bf16(24, 32) == 32 * 32
    assert lib.sr_conv1x1_packed_weight_elems_bf16(16, 24) == 0 and lib.sr_conv1x1_packed_weight_elems_bf16(0, 16) == 0


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
                cur = found.setdefault(val, {}) if any(n in val for n in NAMES + ['pw16_pack']) else None
                if cur is not None:
                    cur['group_segment_fixed_size'] = lds
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count'):
                cur[key] = int(val)
    return found


def test_new_kernels_use_no_scratch_no_spills_and_only_dynamic_lds(tmp_path):
    found = _code_object_kernels(tmp_path)
    deform = sorted(k for k in found if 'deform16_fwd_kernel' in k)
    assert {int(re.search(r'ILi(\d)E', k).group(1)) for k in deform} == {1, 2} and len(deform) == 2, deform
    assert sum('pw16_conv_kernel' in k for k in found) == 2
    assert len(found) == 2 + 2 + 4 + 2, sorted(found)     # + subsample, pool, corr, gate + the two 1x1 pack kernels
    for name, md in found.items():
        assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 \
            and md.get('sgpr_spill_count', 0) == 0 and md['vgpr_count'] <= 256, (name, md)
        assert md['group_segment_fixed_size'] == 0, (name, md)   # the MFMA kernels' LDS is dynamic (the dispatch function), the others use none
    # the instances the dispatch can return are the instances built
    assert {H.dcn_bf16_instance(c, 1, 8, 8)[0] for c in (1, 16, 24, 32, 64, 96, 128)} == {1, 2}


# ------------------------------------------------------------------------------------------------------ the constructor
def test_constructor_accepts_and_refuses():
    assert EDVR(**SMALL).compute_dtype == 'fp32'
    assert EDVR(**SMALL, compute_dtype='bf16').compute_dtype == 'bf16'
    import inspect
    assert list(inspect.signature(EDVR.__init__).parameters)[-1] == 'compute_dtype'
    for bad in ('fp16', 'float32', None, 16):
        with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
            EDVR(**SMALL, compute_dtype=bad)
    with pytest.raises(ValueError, match='CB16'):
        EDVR(**dict(SMALL, num_feat=24, deformable_groups=1), compute_dtype='bf16')
    EDVR(**dict(SMALL, num_feat=24, deformable_groups=1))                         # fine in fp32
    with pytest.raises(ValueError, match='8 \\* deformable_groups'):
        EDVR(**dict(SMALL, num_feat=16, deformable_groups=4), compute_dtype='bf16')   # the existing rule still applies
    with pytest.raises(ValueError, match='hr_in needs with_predeblur'):
        EDVR(**SMALL, hr_in=True, compute_dtype='bf16')
    for kw in (dict(with_predeblur=True, hr_in=True), dict(with_tsa=False), dict(with_predeblur=True)):
        EDVR(**SMALL, **kw, compute_dtype='bf16')


def test_state_dict_is_identical_with_and_without_the_key():
    for kw in (dict(), dict(with_predeblur=True, hr_in=True), dict(with_tsa=False)):
        torch.manual_seed(3)
        a = EDVR(**SMALL, **kw)
        torch.manual_seed(3)
        b = EDVR(**SMALL, **kw, compute_dtype='bf16')
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        assert all(sa[k].shape == sb[k].shape and sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]) for k in sa)
        b.load_state_dict(sa, strict=True)


def test_fp32_refusals_come_first_in_bf16():
    net = EDVR(**SMALL, compute_dtype='bf16')
    with pytest.raises(ValueError, match='5-dimensional'):
        net(torch.zeros(3, 3, 8, 8))
    with pytest.raises(ValueError, match='multiples of 4'):
        net(torch.zeros(1, 3, 3, 6, 8))
    with pytest.raises(ValueError, match='3 frames|frames, expected'):
        net(torch.zeros(1, 5, 3, 8, 8))
    with pytest.raises(NotImplementedError):
        net(torch.zeros(1, 3, 3, 8, 8))                # a CPU tensor
    with pytest.raises(ValueError, match='multiples of 16'):
        EDVR(**SMALL, with_predeblur=True, hr_in=True, compute_dtype='bf16')(torch.zeros(1, 3, 3, 8, 8))


# ------------------------------------------------------------------------------------------------- generate_frame_indices
@pytest.mark.parametrize('mode,want', [('replicate', [0, 0, 0, 1, 2]), ('reflection', [2, 1, 0, 1, 2]),
                                       ('reflection_circle', [4, 3, 0, 1, 2]), ('circle', [3, 4, 0, 1, 2])])
def test_frame_indices_at_the_first_frame(mode, want):
    assert generate_frame_indices(0, 10, 5, padding=mode) == want


@pytest.mark.parametrize('mode,want', [('replicate', [7, 8, 9, 9, 9]), ('reflection', [7, 8, 9, 8, 7]),
                                       ('reflection_circle', [7, 8, 9, 6, 5]), ('circle', [7, 8, 9, 5, 6])])
def test_frame_indices_at_the_last_frame(mode, want):
    assert generate_frame_indices(9, 10, 5, padding=mode) == want


def test_frame_indices_inside_and_refusals():
    for mode in ('replicate', 'reflection', 'reflection_circle', 'circle'):
        assert generate_frame_indices(4, 10, 5, padding=mode) == [2, 3, 4, 5, 6]
        assert generate_frame_indices(1, 10, 3, padding=mode) == [0, 1, 2]
    assert generate_frame_indices(1, 10, 5, padding='reflection') == [1, 0, 1, 2, 3]
    assert generate_frame_indices(8, 10, 5, padding='circle') == [6, 7, 8, 9, 5]
    assert generate_frame_indices(0, 10, 7, padding='reflection_circle') == [6, 5, 4, 0, 1, 2, 3]
    with pytest.raises(ValueError, match='odd'):
        generate_frame_indices(0, 10, 4)
    with pytest.raises(ValueError, match='padding'):
        generate_frame_indices(0, 10, 5, padding='mirror')
