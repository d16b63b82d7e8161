"""Modulated deformable convolution on the host side (no GPU): the restatement tests/dcn_restate.py against closed forms and
gradcheck, the module surface (state_dict keys, shapes, order and initialisation against literal lists taken from the
reference's constructors: deform_conv.py:293-375, arch_util.py:204, edvr_arch.py:21-54), the refusals, and the ledger, profiler
names, compiled resources and dispatch of include/sr_hip_dcn.h.

Dispatch.  The instance sr_dcn_fwd_f32 runs (COT 32-cout sub-tiles, tiles of 4 * PT rows) cannot be observed on the device
(every launch has profiler id 110), so it is restated here (_dcn_instance, from sr_dcn_fwd_f32 in dcn_ops.hip) and the set the
restatement can produce is checked against the instances the code object holds; tests/test_dcn_ops_gpu.py uses it to cover
both sides of the 4-row / 8-row switch and both COT instances."""
import math
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from image_restoration_amd import _lib
from image_restoration_amd.archs.arch_util import DCNv2Pack
from image_restoration_amd.archs.edvr_arch import PCDAlignment
from image_restoration_amd.ops.dcn import ModulatedDeformConv, ModulatedDeformConvPack, modulated_deform_conv
from image_restoration_amd.utils.registry import ARCH_REGISTRY

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_restate as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_dcn.h')
D = torch.float64


def _cdiv(a, b):
    return -(-a // b)


def _dcn_instance(cout, n, h, w):
    """(COT, PT, row tiles) of one sr_dcn_fwd_f32 launch (dcn_ops.hip, sr_dcn_fwd_f32): gc = 64 when roundup32(cout) is a
    multiple of 64, else 32; groups = roundup32(cout) / gc; 8-row tiles, 4-row tiles when ceil(W / 32) * ceil(H / 8) * n *
    groups < 256 and H > 4 (the rule of convd_dispatch); COT = gc / 32."""
    cp = (cout + 31) // 32 * 32
    gc = 64 if cp % 64 == 0 else 32
    groups = cp // gc
    small = _cdiv(w, 32) * _cdiv(h, 8) * n * groups < 256 and h > 4
    return gc // 32, (1 if small else 2), _cdiv(h, 4 if small else 8)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=D) * 2 - 1) * scale


def _case(n=2, cin=16, cout=5, h=6, w=7, dg=2, seed=0):
    x, wt, b = _rand((n, cin, h, w), seed), _rand((cout, cin, 3, 3), seed + 1, 0.3), _rand((cout,), seed + 2)
    return x, wt, b


# ---------------------------------------------------------------------------------------------------- the restatement
def test_zero_offsets_unit_mask_is_conv2d():
    x, wt, b = _case()
    off, m = torch.zeros((2, 36, 6, 7), dtype=D), torch.ones((2, 18, 6, 7), dtype=D)
    assert torch.allclose(R.modulated_deform_conv(x, off, m, wt, b, 2), F.conv2d(x, wt, b, padding=1), rtol=0, atol=1e-13)


def test_half_mask_is_half_conv_plus_bias():
    x, wt, b = _case()
    off, m = torch.zeros((2, 36, 6, 7), dtype=D), torch.full((2, 18, 6, 7), 0.5, dtype=D)
    want = 0.5 * F.conv2d(x, wt, None, padding=1) + b.view(1, -1, 1, 1)
    assert torch.allclose(R.modulated_deform_conv(x, off, m, wt, b, 2), want, rtol=0, atol=1e-13)


@pytest.mark.parametrize('dh,dw', [(2, -3), (-1, 1), (0, 4)])
def test_integer_offset_is_conv_of_the_shifted_zero_filled_image(dh, dw):
    x, wt, b = _case()
    n, c, h, w = x.shape
    off = torch.zeros((2, 36, h, w), dtype=D)
    off[:, 0::2], off[:, 1::2] = dh, dw
    # every tap reads the zero-extended image (dh, dw) further on, also where the unshifted tap would lie in the padding: the
    # conv of the image shifted on the unbounded zero-filled plane, i.e. a crop of the conv of the generously padded image
    P = 6
    full = F.conv2d(F.pad(x, (P, P, P, P)), wt, b, padding=1)
    got = R.modulated_deform_conv(x, off, torch.ones((2, 18, h, w), dtype=D), wt, b, 2)
    assert torch.allclose(got, full[:, :, P + dh:P + dh + h, P + dw:P + dw + w], rtol=0, atol=1e-13)


def test_spike_pins_the_channel_order_and_the_group_stride():
    """One spike at (3, 3) of channel 8 (group 1 of dg = 2, cpg = 8); only W[0, 8, tap 5 = (i 1, j 2)] is 1.  Output pixel (1, 1)
    reads that tap at (1 + oh, 2 + ow) and finds the spike only with oh = 2 in channel 18 * 1 + 2 * 5 = 28 and ow = 1 in channel
    29, under the mask of channel 9 * 1 + 5 = 14.  The other candidates: the pair swapped, group 0's channels (stride 18 missed),
    the planar order (all h, then all w: 18 + 5 and 18 + 9 + 5), the neighbouring taps."""
    n, cin, h, w = 1, 16, 6, 7
    x = torch.zeros((n, cin, h, w), dtype=D)
    x[0, 8, 3, 3] = 1.0
    wt = torch.zeros((1, cin, 3, 3), dtype=D)
    wt[0, 8, 1, 2] = 1.0

    def out(ch_h, ch_w, mask_ch):
        off = torch.zeros((n, 36, h, w), dtype=D)
        off[0, ch_h], off[0, ch_w] = 2.0, 1.0
        m = torch.zeros((n, 18, h, w), dtype=D)
        m[0, mask_ch] = 0.25
        return float(R.modulated_deform_conv(x, off, m, wt, None, 2)[0, 0, 1, 1])

    assert out(28, 29, 14) == 0.25
    for ch_h, ch_w in ((29, 28), (10, 11), (23, 32), (26, 27), (30, 31), (27, 28)):
        assert out(ch_h, ch_w, 14) == 0.0, (ch_h, ch_w)
    for mask_ch in (5, 13, 15):
        assert out(28, 29, mask_ch) == 0.0, mask_ch


@pytest.mark.parametrize('h_im,want', [(-1.0, 0.0), (-0.5, 0.5 * 3.0), (4.5, 0.5 * 7.0), (5.0, 0.0)])
def test_border_rule_and_per_corner_validity(h_im, want):
    """H = 5, a column of values 3 (row 0) .. 7 (row 4): h_im = -1 and H are outside (> -1, < H); -0.5 and H - 0.5 are inside
    with one corner in the image, weight 1/2."""
    h, w = 5, 8
    x = torch.zeros((1, 8, h, w), dtype=D)
    x[0, 0, :, 2] = torch.arange(3.0, 8.0, dtype=D)
    wt = torch.zeros((1, 8, 3, 3), dtype=D)
    wt[0, 0, 1, 1] = 1.0
    off = torch.zeros((1, 18, h, w), dtype=D)
    off[0, 8] = h_im - 2.0    # centre tap k = 4 at output (2, 2): h_im = 2 + off
    y = R.modulated_deform_conv(x, off, torch.ones((1, 9, h, w), dtype=D), wt, None, 1)
    assert float(y[0, 0, 2, 2]) == want
    off[0, 8], off[0, 9] = 0.0, h_im - 2.0 + (w - h if h_im > 0 else 0)   # the same rule along w (W = 8)
    x2 = torch.zeros_like(x)
    x2[0, 0, 2, :] = torch.arange(3.0, 11.0, dtype=D)
    y = R.modulated_deform_conv(x2, off, torch.ones((1, 9, h, w), dtype=D), wt, None, 1)
    assert float(y[0, 0, 2, 2]) == {0.0: 0.0, 1.5: 1.5, 3.5: 0.5 * 10.0}[want]


def test_gradcheck():
    n, cin, h, w, dg = 1, 16, 4, 5, 2
    g = torch.Generator().manual_seed(5)
    x = _rand((n, cin, h, w), 1).requires_grad_(True)
    frac = torch.rand((n, 18 * dg, h, w), generator=g, dtype=D) * 0.6 + 0.2            # away from the kinks of floor
    off = (torch.randint(-2, 3, (n, 18 * dg, h, w), generator=g).to(D) + frac).requires_grad_(True)
    m = torch.rand((n, 9 * dg, h, w), generator=g, dtype=D).requires_grad_(True)
    wt, b = _rand((3, cin, 3, 3), 2, 0.3).requires_grad_(True), _rand((3,), 3).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda *a: R.modulated_deform_conv(*a, dg), (x, off, m, wt, b), eps=1e-6, atol=1e-7)


# ------------------------------------------------------------------------------------------------------ module surface
def _entries(m):
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


PACK_KEYS = [('weight', (64, 64, 3, 3)), ('bias', (64,)), ('conv_offset.weight', (216, 64, 3, 3)), ('conv_offset.bias', (216,))]
C128, C64 = (64, 128, 3, 3), (64, 64, 3, 3)
PCD_KEYS = (
    [(f'offset_conv1.l{i}.{p}', s) for i in (3, 2, 1) for p, s in (('weight', C128), ('bias', (64,)))]
    + [(f'offset_conv2.l{i}.{p}', s) for i in (3, 2, 1) for p, s in (('weight', C64 if i == 3 else C128), ('bias', (64,)))]
    + [(f'offset_conv3.l{i}.{p}', s) for i in (2, 1) for p, s in (('weight', C64), ('bias', (64,)))]
    + [(f'dcn_pack.l{i}.{k}', s) for i in (3, 2, 1) for k, s in PACK_KEYS]
    + [(f'feat_conv.l{i}.{p}', s) for i in (2, 1) for p, s in (('weight', C128), ('bias', (64,)))]
    + [(f'cas_offset_conv1.{p}', s) for p, s in (('weight', C128), ('bias', (64,)))]
    + [(f'cas_offset_conv2.{p}', s) for p, s in (('weight', C64), ('bias', (64,)))]
    + [(f'cas_dcnpack.{k}', s) for k, s in PACK_KEYS])


def _check_pack_init(m, cin):
    stdv = 1.0 / math.sqrt(cin * 9)
    w = m.weight.detach()
    assert float(w.abs().max()) <= stdv and abs(float(w.std()) - stdv / math.sqrt(3)) < 0.05 * stdv and abs(float(w.mean())) < 0.05 * stdv
    assert float(m.bias.detach().abs().max()) == 0.0
    assert float(m.conv_offset.weight.detach().abs().max()) == 0.0 and float(m.conv_offset.bias.detach().abs().max()) == 0.0


def test_pack_modules_have_the_reference_layout_and_init():
    torch.manual_seed(0)
    for cls in (ModulatedDeformConvPack, DCNv2Pack):
        m = cls(64, 64, 3, padding=1, deformable_groups=8)
        assert _entries(m) == PACK_KEYS and cls._version == 2
        _check_pack_init(m, 64)
        assert (m.stride, m.padding, m.dilation, m.groups, m.deformable_groups, m.with_bias) == (1, 1, 1, 1, 8, True)
        assert m.kernel_size == (3, 3) and m.transposed is False and m.output_padding == (0,)
    plain = ModulatedDeformConv(32, 24, 3, 1, 1, 1, 1, 2, False)
    assert _entries(plain) == [('weight', (24, 32, 3, 3))] and plain.bias is None
    assert issubclass(DCNv2Pack, ModulatedDeformConvPack) and issubclass(ModulatedDeformConvPack, ModulatedDeformConv)


def test_pcd_alignment_has_the_reference_layout_and_init():
    torch.manual_seed(0)
    m = PCDAlignment(64, 8)
    assert _entries(m) == PCD_KEYS
    for name in ('dcn_pack.l3', 'dcn_pack.l2', 'dcn_pack.l1', 'cas_dcnpack'):
        _check_pack_init(m.get_submodule(name), 64)
    # the plain convs keep nn.Conv2d's default initialisation: kaiming_uniform(a = sqrt(5)) = U(+-1 / sqrt(fan_in)) for both
    for name, fan_in in (('offset_conv1.l3', 128 * 9), ('offset_conv3.l1', 64 * 9), ('cas_offset_conv2', 64 * 9)):
        c = m.get_submodule(name)
        bound = 1 / math.sqrt(fan_in)
        assert float(c.weight.abs().max()) <= bound and abs(float(c.weight.std()) - bound / math.sqrt(3)) < 0.05 * bound
        assert float(c.bias.abs().max()) <= bound and float(c.bias.abs().max()) > 0
    assert 'PCDAlignment' not in ARCH_REGISTRY and 'RRDBNet' in ARCH_REGISTRY   # not registered, as in the reference
    sd = {k: torch.randn_like(v) for k, v in m.state_dict().items()}
    m2 = PCDAlignment(64, 8)
    m2.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m2.state_dict().items())


@pytest.mark.parametrize('kw', [dict(kernel_size=5), dict(kernel_size=1), dict(stride=2), dict(padding=0), dict(padding=2),
                                dict(dilation=2), dict(groups=2), dict(deformable_groups=3), dict(in_channels=12),
                                dict(in_channels=32, deformable_groups=8)])
def test_unsupported_configurations_are_refused(kw):
    args = dict(in_channels=64, out_channels=64, kernel_size=3, stride=1, padding=1, dilation=1, groups=1, deformable_groups=8)
    args.update(kw)
    for cls in (ModulatedDeformConv, ModulatedDeformConvPack, DCNv2Pack):
        with pytest.raises(ValueError, match='kernel 3x3, stride 1, padding 1, dilation 1, groups 1, fp32'):
            cls(**args)
    x = torch.zeros((1, args['in_channels'], 4, 4))
    dg = args['deformable_groups']
    k = args['kernel_size']
    with pytest.raises(ValueError, match='supported: kernel 3x3, stride 1'):
        modulated_deform_conv(x, torch.zeros((1, 18 * dg, 4, 4)), torch.zeros((1, 9 * dg, 4, 4)),
                              torch.zeros((8, args['in_channels'], k, k)), None, args['stride'], args['padding'], args['dilation'],
                              args['groups'], dg)


def test_bf16_is_refused_and_cpu_tensors_are_not_implemented():
    m = DCNv2Pack(16, 16, 3, padding=1, deformable_groups=2)
    x = torch.zeros((1, 16, 4, 4))
    off, msk = torch.zeros((1, 36, 4, 4)), torch.zeros((1, 18, 4, 4))
    with pytest.raises(ValueError, match='supported'):
        modulated_deform_conv(x.bfloat16(), off.bfloat16(), msk.bfloat16(), m.weight.bfloat16(), None, 1, 1, 1, 1, 2)
    with pytest.raises(ValueError, match='supported'):
        m(x.bfloat16(), x.bfloat16())
    with pytest.raises(ValueError, match='supported'):
        ModulatedDeformConvPack(16, 16, 3, padding=1, deformable_groups=2)(x.bfloat16())
    with pytest.raises(ValueError, match='do not fit'):
        modulated_deform_conv(x, off[:, :18], msk, m.weight, None, 1, 1, 1, 1, 2)
    with pytest.raises(NotImplementedError):
        modulated_deform_conv(x, off, msk, m.weight, m.bias, 1, 1, 1, 1, 2)
    with pytest.raises(NotImplementedError):
        m(x, x)
    with pytest.raises(NotImplementedError):
        ModulatedDeformConv(16, 16, 3, 1, 1, deformable_groups=2)(x, off, msk)
    with pytest.raises(NotImplementedError):
        ModulatedDeformConvPack(16, 16, 3, padding=1, deformable_groups=2)(x)
    with pytest.raises(NotImplementedError):
        PCDAlignment(16, 2)([torch.zeros((1, 16, s, s)) for s in (8, 4, 2)], [torch.zeros((1, 16, s, s)) for s in (8, 4, 2)])


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_every_declared_entry_point_is_bound_and_exported():
    declared = set(re.findall(r'\b(sr_dcn_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(_lib.DCN_SIGNATURES) and len(declared) == 7
    others = set(_lib.SIGNATURES) | set(_lib.RIDNET_SIGNATURES) | set(_lib.GFPGAN_SIGNATURES) | set(_lib.EDSR_SIGNATURES) \
        | set(_lib.CA_BF16_SIGNATURES)
    assert not declared & others
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s


def test_profiler_ids_resolve_to_the_new_kernels():
    lib = _lib.load()
    assert [lib.sr_kernel_name(i).decode() for i in range(110, 113)] == ['dcn_fwd_f32_kernel', 'dcn_cols_kernel', 'dcn_bwd_data_kernel']
    assert lib.sr_kernel_name(105).decode() == '' and lib.sr_kernel_name(109).decode() == '' and lib.sr_kernel_name(113).decode() == ''
    assert lib.sr_kernel_name(106).decode() == 'conv_wino_f32_kernelILi4E'


def test_size_queries():
    lib = _lib.load()
    assert lib.sr_dcn_cols_bytes(2, 64, 13, 35) == 2 * 9 * 64 * 13 * 35 * 4
    assert lib.sr_dcn_cols_bytes(2, 12, 13, 35) == 0 and lib.sr_dcn_cols_bytes(0, 64, 1, 1) == 0
    # the ksize-1 forward image of 9 * cin outputs over roundup8(cout) inputs (sr_convk_packed_weight_floats' formula)
    for cout, cin in ((64, 64), (24, 16), (32, 32), (64, 128)):
        assert lib.sr_dcn_packed_t_weight_floats(cout, cin) == lib.sr_convk_packed_weight_floats(9 * cin, cout, 1, 0)


def _code_object_kernels(tmp_path, marker):
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
                cur = found.setdefault(val, {}) if marker in val else None
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count',
                                             'group_segment_fixed_size'):
                cur[key] = int(val)
    return found


def test_new_kernels_use_no_scratch_no_spills_and_the_dispatch_reaches_the_instances_built(tmp_path):
    found = _code_object_kernels(tmp_path, 'dcn_')
    fwd = sorted(k for k in found if 'dcn_fwd_f32_kernel' in k)
    built = {tuple(int(v) for v in re.search(r'ILi(\d)ELi(\d)E', k).groups()) for k in fwd}
    assert built == {(1, 1), (1, 2), (2, 1), (2, 2)} and len(fwd) == 4, fwd
    assert len(found) == 8, sorted(found)   # + cols, bwd_data, pack_t, weight_unpack
    for name, md in found.items():
        assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 \
            and md.get('sgpr_spill_count', 0) == 0 and md['vgpr_count'] <= 256, (name, md)
    reached = {_dcn_instance(cout, n, h, w)[:2] for cout in (24, 32, 64, 96) for n, h, w in ((2, 13, 35), (2, 5, 70), (2, 4, 40),
                                                                                              (5, 180, 320), (128, 8, 64), (2, 16, 24))}
    assert reached == built
    assert _dcn_instance(64, 2, 13, 35) == (2, 1, 4) and _dcn_instance(64, 128, 8, 64) == (2, 2, 1)
    assert _dcn_instance(64, 64, 5, 128)[1] == 2 and _dcn_instance(64, 63, 5, 128)[1] == 1   # 256 and 252 tiles at the 8-row rule
    assert _dcn_instance(64, 2, 4, 40)[1] == 2                                               # H = 4 never takes 4-row tiles
