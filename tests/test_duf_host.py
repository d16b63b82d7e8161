"""DUF on the host side (no GPU): the restatement tests/duf_restate.py against the reference's own float64 outputs
(tests/golden/g_zj_duf.npz, tools/make_golden_duf.py) and what the fixture must show, DUF's state_dict and initialisation, both
BatchNorm transforms, every refusal, the ABI of include/sr_hip_duf.h (declared, bound, exported, in no other header, each entry
point mapped to the GPU test that pins it), the profiler names, the compiled resources read from the code object, both option
files, the DUF downsampling and its dataset."""
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
from torch.nn import functional as F

import image_restoration_amd as ira
from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H
from image_restoration_amd.archs import duf_arch, tof_arch
from image_restoration_amd.archs.duf_arch import DUF, DenseBlocks, DenseBlocksTemporalReduce, DynamicUpsamplingFilter
from image_restoration_amd.data import data_util
from image_restoration_amd.utils import synth
from image_restoration_amd.utils.registry import ARCH_REGISTRY

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import duf_restate as D  # noqa: E402
import flow_restate as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_duf.h')
SR_EINVAL = -1
_OPS = 'tests/test_duf_ops_gpu.py::'
PINNED = {
    'sr_duf_conv3d_packed_floats': _OPS + 'test_conv3d_matches_float64',
    'sr_duf_conv3d_pack_f32': _OPS + 'test_conv3d_matches_float64',
    'sr_duf_conv3d_f32': _OPS + 'test_conv3d_matches_float64',
    'sr_duf_pw_packed_floats': _OPS + 'test_pw_matches_float64',
    'sr_duf_pw_pack_f32': _OPS + 'test_pw_matches_float64',
    'sr_duf_pw_f32': _OPS + 'test_pw_matches_float64',
    'sr_duf_filter_f32': _OPS + 'test_filter_matches_float64',
}
NAMES = ['duf_conv3d_f32_kernel', 'duf_conv_pack_kernel', 'duf_pw_f32_kernel', 'duf_filter_f32_kernel']


@pytest.fixture(scope='module')
def g(golden):
    return golden('g_zj_duf')


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('case', D.CASES, ids=[c[0] for c in D.CASES])
def test_restatement_reproduces_the_reference(g, case):
    tag, num_layer, scale, b, h, w, adapt = case
    i = [c[0] for c in D.CASES].index(tag)
    sd = synth.duf_state_dict(int(g['weight_seed']), num_layer, scale)
    assert R.weights_checksum(sd) == str(g[f'l{num_layer}_x{scale}_checksum'])
    u8 = g[f'{tag}_clip_u8']
    assert u8.shape == (b, 7, 3, h, w) and np.array_equal(u8, D.clip_u8(int(g['input_seed']) + i, b, h, w))
    x = D.decode(u8)
    keep = {}
    out = D.duf(sd, x, num_layer, scale, adapt, keep)
    want = g[tag + '_out']
    assert out.shape == want.shape == (b, 3, scale * h, scale * w) and np.abs(out - want).max() <= 1e-12       # every pixel
    # what the fixture must show, from the file and from the restatement's own intermediates
    assert np.isfinite(want).all() and 1e-8 < float(g[tag + '_fp32_dist']) < 1e-4
    peak = D.softmax_taps(keep['logits'].reshape(b, 25, scale * scale, h, w)).max(1)
    assert abs(peak.max() - float(g[tag + '_peak_max'])) <= 1e-9 and abs(peak.mean() - float(g[tag + '_peak_mean'])) <= 1e-9
    assert float(g[tag + '_peak_max']) > 0.5 and float(g[tag + '_peak_mean']) < 0.99
    assert abs(np.abs(keep['res']).max() - float(g[tag + '_res_absmax'])) <= 1e-9 and float(g[tag + '_res_absmax']) >= 0.05
    depart = np.abs(want - D.nearest_up(x[:, 3].astype(np.float64), scale)).max()
    assert abs(depart - float(g[tag + '_depart'])) <= 1e-12 and depart >= 0.05
    frac = g[tag + '_fractions']
    assert len(frac) == D.BLOCKS[num_layer][0] + 3 and frac.min() >= 0.2 and frac.max() <= 0.8
    assert np.abs(keep['fractions'] - frac).max() <= 1e-9
    if i == 0:
        assert np.abs(keep['logits'] - g[tag + '_logits']).max() <= 1e-12 and np.abs(keep['res'] - g[tag + '_res']).max() <= 1e-12
    else:
        assert tag + '_logits' not in g


def test_restated_pieces_are_the_reference_ops():
    """conv3d, BatchNorm3d, softmax, the dynamic filter and the pixel shuffle of the restatement against torch's float64 ops."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 5, 4, 6, 7))
    for kt, k, pad_t in ((1, 1, 0), (1, 3, 0), (3, 3, 1), (3, 3, 0)):
        wt, b = rng.standard_normal((4, 5, kt, k, k)), rng.standard_normal(4)
        want = F.conv3d(torch.from_numpy(x), torch.from_numpy(wt), torch.from_numpy(b), 1, (pad_t, k // 2, k // 2)).numpy()
        got, mag = D.conv3d(x, wt, b, pad_t, want_mag=True)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 and (mag >= np.abs(got) - 1e-12).all()
    gamma, beta, mean, var = rng.uniform(0.5, 1.5, 5), rng.standard_normal(5), rng.standard_normal(5), rng.uniform(0.5, 2, 5)
    for eps in (1e-5, 1e-3):
        want = F.batch_norm(torch.from_numpy(x), torch.from_numpy(mean), torch.from_numpy(var), torch.from_numpy(gamma),
                            torch.from_numpy(beta), False, 0.1, eps).numpy()
        assert np.abs(D.batchnorm_eval(x, gamma, beta, mean, var, eps) - want).max() <= 1e-12
    # the dynamic filter as the reference writes it: an im2col by a grouped conv with an identity kernel, then a matmul
    for s in (2, 3, 4):
        n, h, w, s2 = 2, 5, 6, s * s
        img, logits = rng.uniform(0, 1, (n, 3, h, w)), rng.standard_normal((n, 25 * s2, h, w)) * 4
        f = torch.softmax(torch.from_numpy(logits).view(n, 25, s2, h, w), 1)
        assert np.abs(D.softmax_taps(logits.reshape(n, 25, s2, h, w)) - f.numpy()).max() <= 1e-12
        expansion = torch.eye(25, dtype=torch.float64).view(25, 1, 5, 5).repeat(3, 1, 1, 1)
        expanded = F.conv2d(torch.from_numpy(img), expansion, padding=2, groups=3).view(n, 3, 25, h, w).permute(0, 3, 4, 1, 2)
        want = torch.matmul(expanded, f.permute(0, 3, 4, 1, 2)).permute(0, 3, 4, 1, 2).reshape(n, 3 * s2, h, w)
        assert np.abs(D.dynamic_filter(img, f.numpy()) - want.numpy()).max() <= 1e-12
        res = rng.standard_normal((n, 3 * s2, h, w))
        assert np.abs(D.tail(logits, res, img, s) - F.pixel_shuffle(want + torch.from_numpy(res), s).numpy()).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------ the network
@pytest.mark.parametrize('num_layer', [16, 28, 52])
def test_state_dict_and_init(g, num_layer):
    for scale in (2, 3, 4):
        tag = f'l{num_layer}_x{scale}'
        if tag + '_keys' not in g:
            continue
        net = DUF(scale, num_layer)
        own = net.state_dict()
        sd = synth.duf_state_dict(int(g['weight_seed']), num_layer, scale)
        assert list(own) == [str(k) for k in g[tag + '_keys']] == list(sd)
        assert [','.join(str(d) for d in v.shape) for v in own.values()] == [str(s) for s in g[tag + '_shapes']]
        assert sum(p.numel() for p in net.parameters()) == int(g[tag + '_num_params']) == duf_arch.num_parameters(num_layer, scale)
        nb = D.BLOCKS[num_layer][0]
        assert sum(k.endswith('num_batches_tracked') for k in own) == 2 * (nb + 3) + 1
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        assert int(net.state_dict()['bn3d2.num_batches_tracked']) == 100
    assert (net.num_block, net.num_grow_ch) == D.BLOCKS[num_layer] and net.channels == 64 + net.num_grow_ch * (net.num_block + 3)


def test_seeded_init_and_constructors(g):
    # a seeded fresh network has the reference's initial parameters (the same draws in the same order)
    torch.manual_seed(11)
    own = DUF(4, 16).state_dict()
    probes = [k for k in g if k.startswith('init_')]
    assert len(probes) == 4
    for k in probes:
        assert np.array_equal(own[k[5:]].flatten()[:8].numpy(), g[k]), k
    w = own['dense_block1.dense_blocks.2.5.weight']
    bound = 1 / (128 * 27) ** 0.5
    assert float(w.abs().max()) <= bound and abs(float(w.std()) - bound / 3 ** 0.5) <= 0.05 * bound
    net = DUF()
    assert (net.scale, net.num_layer) == (4, 52)
    bn = net.dense_block1.dense_blocks[3][0]
    assert isinstance(bn, torch.nn.BatchNorm3d) and bool((bn.weight == 1).all()) and (bn.eps, bn.momentum) == (1e-5, 0.1)
    assert isinstance(net.dense_block1, DenseBlocks) and isinstance(net.dense_block2, DenseBlocksTemporalReduce)
    assert net.dense_block2.temporal_reduce3[5].padding == (0, 1, 1) and net.dense_block1.dense_blocks[0][5].padding == (1, 1, 1)
    for mod in (DUF(2, 28, adapt_official_weights=True), DenseBlocks(2, adapt_official_weights=True),
                DenseBlocksTemporalReduce(adapt_official_weights=True)):
        bns = [m for m in mod.modules() if isinstance(m, torch.nn.BatchNorm3d)]
        assert bns and all((m.eps, m.momentum) == (1e-3, 1e-3) for m in bns)
    for bad in (17, 0, 64):
        with pytest.raises(ValueError, match=rf'Only supported \(16, 28, 52\) layers, but got {bad}\.'):
            DUF(4, bad)
    assert ARCH_REGISTRY.get('DUF') is DUF and isinstance(ira.build_network(dict(type='DUF', scale=3, num_layer=16)), DUF)
    with pytest.raises(TypeError):
        DynamicUpsamplingFilter([5, 5])
    with pytest.raises(ValueError, match='length'):
        DynamicUpsamplingFilter((5, 5, 5))


def test_batchnorm_transforms_match_float64_eval_batchnorm():
    rng = np.random.default_rng(3)
    for c, eps in ((64, 1e-5), (80, 1e-3)):
        x = rng.standard_normal((2, c, 3, 5, 6))
        wt, bias = rng.standard_normal((c, c, 1, 1, 1)).astype(np.float32), rng.standard_normal(c).astype(np.float32)
        gamma, beta = rng.uniform(0.2, 3, c).astype(np.float32), rng.standard_normal(c).astype(np.float32)
        mean, var = rng.standard_normal(c).astype(np.float32), rng.uniform(0.01, 4, c).astype(np.float32)
        t = [torch.from_numpy(v) for v in (gamma, beta, mean, var)]
        want_bn = F.batch_norm(torch.from_numpy(x), t[2].double(), t[3].double(), t[0].double(), t[1].double(), False, 0.1, eps).numpy()
        # the fold: BatchNorm behind a conv with a bias
        w2, b2 = tof_arch.fold_batchnorm(torch.from_numpy(wt), *t, eps, bias=torch.from_numpy(bias))
        assert w2.dtype == b2.dtype == torch.float32 and w2.shape == wt.shape
        w64, b64 = D.fold(wt, bias, gamma, beta, mean, var, eps)
        # rounded once from float64: half an ulp
        assert (np.abs(w2.numpy() - w64) <= 2.0 ** -24 * np.abs(w64)).all() and (np.abs(b2.numpy() - b64) <= 2.0 ** -24 * np.abs(b64) + 1e-30).all()
        pre, _ = D.conv3d(x, wt, bias)
        want = F.batch_norm(torch.from_numpy(pre), t[2].double(), t[3].double(), t[0].double(), t[1].double(), False, 0.1, eps).numpy()
        got, mag = D.conv3d(x, w64, b64, want_mag=True)
        assert (np.abs(got - want) <= 1e-12 * (mag + 1)).all()
        # the prologue arrays: BatchNorm in front of a conv
        bn = torch.nn.BatchNorm3d(c, eps=eps)
        with torch.no_grad():
            for p, v in zip((bn.weight, bn.bias, bn.running_mean, bn.running_var), t):
                p.copy_(v)
        scale, shift = duf_arch.bn_prologue(bn)
        s64, t64 = D.prologue_arrays(gamma, beta, mean, var, eps)
        assert scale.dtype == shift.dtype == torch.float32
        assert (np.abs(scale.numpy() - s64) <= 2.0 ** -24 * np.abs(s64)).all() and (np.abs(shift.numpy() - t64) <= 2.0 ** -24 * np.abs(t64) + 1e-30).all()
        assert np.abs(x * s64.reshape(1, -1, 1, 1, 1) + t64.reshape(1, -1, 1, 1, 1) - want_bn).max() <= 1e-12 * (np.abs(x).max() * s64.max() + 10)
    # the bias-free fold of TOFlow is what it was
    w4 = torch.from_numpy(rng.standard_normal((8, 4, 7, 7)).astype(np.float32))
    t8 = [torch.from_numpy(v[:8].copy()) for v in (gamma, beta, mean, var)]
    wa, ba = tof_arch.fold_batchnorm(w4, *t8, 1e-5)
    s = t8[0].double() / torch.sqrt(t8[3].double() + 1e-5)
    assert torch.equal(wa, (w4.double() * s.view(-1, 1, 1, 1)).float()) and torch.equal(ba, (t8[1].double() - t8[2].double() * s).float())


def test_python_refusals():
    net = DUF(4, 16).eval()
    x = torch.zeros(1, 7, 3, 8, 8)
    for bad in (x[:, :5], x[:, :, :2], x[0], x.half(), x.double(), torch.zeros(1, 5, 3, 8, 8), torch.zeros(1, 9, 3, 8, 8)):
        with pytest.raises(ValueError, match=r'\[b, 7, 3, h, w\]'):
            net(bad)
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        with torch.no_grad():
            net(x)
    with pytest.raises(NotImplementedError, match='inference'):
        net(x)                                                   # grad enabled and the parameters require grad
    net.requires_grad_(False)
    with pytest.raises(NotImplementedError, match='inference'):
        net(x.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match=r'\.eval\(\)'):
        with torch.no_grad():
            net.train()(x)                                       # training mode, even under no_grad
    mod = DynamicUpsamplingFilter((5, 5))
    img, f = torch.zeros(2, 3, 4, 4), torch.zeros(2, 25, 16, 4, 4)
    for bx, bf in ((img[:, :2], f), (img.double(), f), (img, f[:, :24]), (img, f[:, :, :5]), (img, f[:1]), (img, f.double()), (img, f[..., :3])):
        with pytest.raises(ValueError, match='DynamicUpsamplingFilter'):
            mod(bx, bf)
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        mod(img, f)
    with pytest.raises(NotImplementedError, match='inference'):
        mod(img.clone().requires_grad_(), f)
    with pytest.raises(NotImplementedError):
        DynamicUpsamplingFilter((3, 3))
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        H.PackedDufConv(torch.zeros(16, 64, 3, 3, 3))


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_every_declared_entry_point_is_bound_exported_and_pinned():
    declared = set(re.findall(r'\b(?:int|size_t)\s+(sr_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(_lib.DUF_SIGNATURES) == set(PINNED) and len(declared) == 7
    others = set()
    for name in dir(_lib):
        if name.endswith('SIGNATURES') and name != 'DUF_SIGNATURES':
            others |= set(getattr(_lib, name))
    assert others and not declared & others
    assert not any(o in s for o in others for s in declared)              # no new name contains an existing one
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    text = open(HEADER).read()
    # the new header spells no entry point of another companion header but the one it sends the head convs to
    assert not any(o in text for o in others - set(_lib.SIGNATURES) - {'sr_convd_f32'})
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'sr_hip_duf.h':
            assert not any(s in open(os.path.join(ROOT, 'include', other)).read() for s in declared), other
    for s, target in PINNED.items():
        path, _, func = target.partition('::')
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        assert func in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, (s, target)
    src = open(os.path.join(ROOT, 'image_restoration_amd', 'hip_ops.py')).read()
    for s, (res, args) in _lib.DUF_SIGNATURES.items():
        if res is C.c_int:
            assert src.count(f"_launch_arg('{s}'") == 1, s
    assert C.sizeof(_lib.DufConvDesc) == 112


def test_profiler_ids_resolve_from_194():
    lib = _lib.load()
    assert [lib.sr_kernel_name(i).decode() for i in range(194, 198)] == NAMES
    assert lib.sr_kernel_name(193).decode() == '' and lib.sr_kernel_name(198).decode() == ''
    assert lib.sr_kernel_name(192).decode() == 'tof_finish_kernel'


def test_kernels_use_no_scratch(tmp_path):
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
                cur = found.setdefault(val, {}) if re.search(r'\dduf_\w+_kernel', val) else None
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count',
                                             'group_segment_fixed_size'):
                cur[key] = int(val)
    # three instances of the 3D convolution (16, 32 and 64 couts per workgroup), one of everything else
    names = sorted(re.search(r'\d(duf_\w+?_kernel)', n).group(1) for n in found)
    assert names == sorted(NAMES + ['duf_conv3d_f32_kernel'] * 2), sorted(found)
    for name, md in found.items():
        assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 \
            and md.get('sgpr_spill_count', 0) == 0 and md['vgpr_count'] <= 256, (name, md)      # 256: two waves per SIMD
    lib_ = _lib.load()
    served = {(ci, co, kt) for ci in range(0, 460) for co in (8, 16, 24, 32, 48, 64, 128, 256) for kt in (1, 2, 3)
              if lib_.sr_duf_conv3d_packed_floats(co, ci, kt)}
    assert served == {(ci, co, kt) for ci in [3] + list(range(8, 449, 8)) for co in H.DUF_CONV3D_COUTS for kt in (1, 3)}
    assert {c for c in range(0, 450) if lib_.sr_duf_pw_packed_floats(c)} == set(range(8, 433, 8))


def test_c_abi_refuses_before_any_launch():
    """Every SR_EINVAL of every entry point, with fake aligned addresses: nothing is launched, so nothing is dereferenced."""
    lib = _lib.load()
    P, Q = 256, 4096

    def refused(rc, needle):
        assert rc == SR_EINVAL and needle in lib.sr_last_error(), (rc, lib.sr_last_error())

    # pack
    refused(lib.sr_duf_conv3d_pack_f32(P, None, 16, 12, 3, Q, None), b'(cin, cout, kt) = (12, 16, 3) is not supported')
    refused(lib.sr_duf_conv3d_pack_f32(P, None, 16, 64, 2, Q, None), b'is not supported')
    refused(lib.sr_duf_conv3d_pack_f32(None, None, 16, 64, 3, Q, None), b'null weight / packed')
    refused(lib.sr_duf_conv3d_pack_f32(P, None, 16, 64, 3, None, None), b'null weight / packed')
    refused(lib.sr_duf_conv3d_pack_f32(P, None, 16, 64, 3, Q + 4, None), b'16-byte aligned')
    refused(lib.sr_duf_pw_pack_f32(P, None, 440, Q, None), b'c = 440 is not supported')
    refused(lib.sr_duf_pw_pack_f32(P, None, 12, Q, None), b'is not supported')
    refused(lib.sr_duf_pw_pack_f32(None, None, 64, Q, None), b'null weight / packed')
    refused(lib.sr_duf_pw_pack_f32(P, None, 64, Q + 8, None), b'16-byte aligned')

    hw = 64

    def desc(**kw):
        d = _lib.DufConvDesc()
        d.in_, d.in_frame_stride, d.in_clip_stride, d.cin, d.cout, d.kt, d.pad_t = P, 64 * hw, 7 * 64 * hw, 64, 16, 3, 1
        d.b, d.t, d.h, d.w, d.packed, d.out, d.out_frame_stride, d.out_clip_stride, d.out_cb0, d.relu = 1, 7, 8, 8, Q, Q, 80 * hw, 7 * 80 * hw, 8, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for fn, base in ((lib.sr_duf_conv3d_f32, {}), (lib.sr_duf_pw_f32, dict(cout=64, kt=1, pad_t=0, out_cb0=0))):
        def call(**kw):
            return fn(C.byref(desc(**dict(base, **kw))), None)
        refused(fn(None, None), b'null descriptor')
        for k in ('in_', 'packed', 'out'):
            refused(call(**{k: None}), b'null in / packed / out')
        refused(call(scale=P), b'scale and shift come together')
        refused(call(shift=P), b'scale and shift come together')
        for k, v in (('b', 0), ('t', 0), ('h', 0), ('w', -1)):
            refused(call(**{k: v}), b'bad shape')
        for k in ('in_', 'packed', 'out'):
            refused(call(**{k: P + 8}), b'16-byte aligned')
        for k in ('in_frame_stride', 'in_clip_stride', 'out_frame_stride', 'out_clip_stride'):
            refused(call(**{k: 7 * 80 * hw + 2}), b'multiples of 4 floats')
        refused(call(relu=2), b'relu must be 0 or 1')
        refused(call(out_cb0=-1), b'out_cb0')
        refused(call(h=4096, w=4096, in_frame_stride=1 << 40, in_clip_stride=1 << 44, out_frame_stride=1 << 40, out_clip_stride=1 << 44),
                b'too large')
        refused(call(in_frame_stride=56 * hw), b'frame stride')
        refused(call(out_frame_stride=8 * hw), b'frame stride')
        refused(call(in_clip_stride=6 * 64 * hw), b'clip stride')
        refused(call(out_clip_stride=6 * 80 * hw), b'clip stride')
    for cin, cout, kt in ((12, 16, 3), (64, 48, 3), (456, 16, 3), (64, 16, 2)):
        refused(lib.sr_duf_conv3d_f32(C.byref(desc(cin=cin, cout=cout, kt=kt)), None), b'is not supported')
    refused(lib.sr_duf_conv3d_f32(C.byref(desc(kt=1, pad_t=1)), None), b'pad_t=1 does not go with kt=1')
    refused(lib.sr_duf_conv3d_f32(C.byref(desc(pad_t=2)), None), b'does not go with')
    refused(lib.sr_duf_conv3d_f32(C.byref(desc(pad_t=0, t=2)), None), b'leave no output frame')
    refused(lib.sr_duf_pw_f32(C.byref(desc(cin=64, cout=16, kt=1, pad_t=0)), None), b'(cin, cout) = (64, 16) is not supported')
    refused(lib.sr_duf_pw_f32(C.byref(desc(cin=440, cout=440, kt=1, pad_t=0)), None), b'is not supported')
    refused(lib.sr_duf_pw_f32(C.byref(desc(cin=64, cout=64, kt=3, pad_t=1, out_cb0=0)), None), b'kt must be 1 and pad_t 0')

    # filter: (logits, stride, res, stride, centre, stride, out, n, s, h, w, softmax, shuffle)
    ok = dict(lg=Q, ls=400 * hw, res=Q, rs=48 * hw, c=P, cs=3 * hw, out=P, n=1, s=4, h=8, w=8, softmax=1, shuffle=1)

    def filt(**kw):
        a = dict(ok, **kw)
        return lib.sr_duf_filter_f32(a['lg'], a['ls'], a['res'], a['rs'], a['c'], a['cs'], a['out'], a['n'], a['s'], a['h'], a['w'],
                                     a['softmax'], a['shuffle'], None)
    for k in ('lg', 'c', 'out'):
        refused(filt(**{k: None}), b'null logits / centre / out')
    for k, v in (('n', 0), ('n', 65536), ('h', 0), ('w', 0)):
        refused(filt(**{k: v}), b'bad shape')
    for s in (1, 5):
        refused(filt(s=s), b'is not supported; supported: 2, 3, 4')
    refused(filt(softmax=2), b'must be 0 or 1')
    refused(filt(shuffle=-1), b'must be 0 or 1')
    refused(filt(h=1 << 12, w=1 << 12, ls=1 << 40, rs=1 << 40, cs=1 << 40), b'too large')
    for k in ('lg', 'res'):
        refused(filt(**{k: Q + 4}), b'16-byte aligned')
    for k in ('ls', 'rs'):
        refused(filt(**{k: 400 * hw + 2}), b'multiples of 4 floats')
    refused(filt(ls=392 * hw), b'smaller than the image')
    refused(filt(rs=40 * hw), b'smaller than the image')
    refused(filt(cs=3 * hw - 1), b'smaller than the image')


# ------------------------------------------------------------------------------------------------------------- options
def test_option_files_parse_and_build():
    import image_restoration_amd.models  # noqa: F401  (fills MODEL_REGISTRY)
    from image_restoration_amd.data import SyntheticClipDataset
    from image_restoration_amd.utils.registry import DATASET_REGISTRY, MODEL_REGISTRY
    d = os.path.join(ROOT, 'options', 'test', 'DUF')
    off = yaml.safe_load(open(os.path.join(d, 'test_DUF_official.yml')))
    assert off['model_type'] == 'VideoBaseModel' and off['scale'] == 4
    assert off['network_g'] == dict(type='DUF', scale=4, num_layer=52, adapt_official_weights=True)
    ds = off['datasets']['test']
    assert (ds['type'], ds['num_frame'], ds['padding'], ds['cache_data'], ds['use_duf_downsampling'], ds['scale']) == \
        ('VideoTestDUFDataset', 7, 'reflection_circle', False, True, 4)
    assert ds['dataroot_gt'] == 'datasets/Vid4/GT' and ds['dataroot_lq'] == 'datasets/Vid4/BIx4' and ds['name'] == 'Vid4'
    assert off['path']['strict_load_g'] is True and off['path']['pretrain_network_g'].endswith('DUF_x4_52L_official-483d2c78.pth')
    assert {m['type'] for m in off['val']['metrics'].values()} == {'calculate_psnr', 'calculate_ssim'} and off['val']['save_img']
    assert all(m['crop_border'] == 8 and m['test_y_channel'] for m in off['val']['metrics'].values())
    syn = yaml.safe_load(open(os.path.join(d, 'test_DUF_synthetic.yml')))
    assert syn['model_type'] == 'VideoBaseModel' and syn['network_g'] == dict(type='DUF', scale=4, num_layer=16, adapt_official_weights=False)
    assert syn['path']['pretrain_network_g'] is None and syn['val']['metrics']['psnr_y']['test_y_channel'] is True
    for opt in (off, syn):
        assert MODEL_REGISTRY.get(opt['model_type']) is not None and DATASET_REGISTRY.get(opt['datasets']['test']['type']) is not None
        net = ira.build_network(dict(opt['network_g']))
        assert isinstance(net, DUF) and net.num_layer == opt['network_g']['num_layer'] and net.scale == opt['scale']
    sopt = dict(syn['datasets']['test'])
    sds = SyntheticClipDataset(sopt)
    item = sds[1]
    assert len(sds) == sopt['num_samples'] and tuple(item['lq'].shape) == (7, 3, 16, 16) and tuple(item['gt'].shape) == (3, 64, 64)
    assert item['folder'] == '00000001' and item['idx'] == '0/1'


# ------------------------------------------------------------------------------------------- the DUF test set's frames
@pytest.mark.parametrize('scale', [2, 3, 4])
def test_duf_downsample_and_gaussian_kernel_match_the_reference(g, scale):
    k = data_util.generate_gaussian_kernel(13, 0.4 * scale)
    assert k.shape == (13, 13) and k.dtype == np.float64 and np.abs(k - g[f'gauss_x{scale}']).max() <= 1e-12
    assert np.abs(D.gaussian_kernel(13, 0.4 * scale) - g[f'gauss_x{scale}']).max() <= 1e-12 and abs(k.sum() - 1) <= 1e-12
    x = np.random.default_rng(int(g['down_seed'])).uniform(0, 1, (2, 3, 40, 52))
    want = g[f'down_x{scale}']
    got = data_util.duf_downsample(torch.from_numpy(x), 13, scale)
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape == (2, 3, 40 // scale + (1 if 40 % scale else 0), 52 // scale + (1 if 52 % scale else 0))
    assert np.abs(got.numpy() - want).max() <= 1e-12 and np.abs(D.duf_downsample(x, 13, scale) - want).max() <= 1e-12
    five = data_util.duf_downsample(torch.from_numpy(x)[None], 13, scale)
    assert five.dim() == 5 and torch.equal(five[0], got)
    assert data_util.duf_downsample(torch.from_numpy(x).float(), 13, scale).dtype == torch.float32
    if scale == 2:
        with pytest.raises(ValueError, match=r'Only support scale \(2, 3, 4\)'):
            data_util.duf_downsample(torch.from_numpy(x), 13, 5)
        with pytest.raises(ValueError, match='does not fit'):
            data_util.generate_gaussian_kernel(13, 2.0)


def test_video_test_duf_dataset(tmp_path):
    from PIL import Image

    from image_restoration_amd.data import VideoTestDUFDataset
    from image_restoration_amd.utils.registry import DATASET_REGISTRY
    assert DATASET_REGISTRY.get('VideoTestDUFDataset') is VideoTestDUFDataset
    rng = np.random.default_rng(1)
    frames = {}
    for clip, n in (('calendar', 5), ('city', 5)):
        for i in range(n):
            gt = rng.integers(0, 256, (50, 45, 3), dtype=np.uint8)               # 50 x 45: not a multiple of 4
            frames[clip, i] = gt
            for root, img in (('GT', gt), ('LQ', gt[:12, :11])):
                os.makedirs(tmp_path / root / clip, exist_ok=True)
                Image.fromarray(img).save(tmp_path / root / clip / f'{i:08d}.png')
    opt = dict(name='Vid4', type='VideoTestDUFDataset', dataroot_gt=str(tmp_path / 'GT'), dataroot_lq=str(tmp_path / 'LQ'),
               io_backend=dict(type='disk'), cache_data=False, num_frame=5, padding='reflection_circle', use_duf_downsampling=True, scale=4)
    ds = VideoTestDUFDataset(opt)
    assert len(ds) == 10
    item = ds[1]
    assert set(item) == {'lq', 'gt', 'folder', 'idx', 'border', 'lq_path'}
    assert (item['folder'], item['idx'], item['border']) == ('calendar', '1/5', 1) and item['lq_path'].endswith(os.path.join('LQ', 'calendar', '00000001.png'))
    assert tuple(item['gt'].shape) == (3, 48, 44) and tuple(item['lq'].shape) == (5, 3, 12, 11) and item['lq'].dtype == torch.float32
    select = data_util.generate_frame_indices(1, 5, 5, padding='reflection_circle')
    gts = torch.stack([torch.from_numpy(frames['calendar', i][:48, :44].astype(np.float32) / 255.0).permute(2, 0, 1) for i in select])
    assert select == [4, 0, 1, 2, 3] and torch.equal(item['gt'], gts[2]) and torch.equal(item['lq'], data_util.duf_downsample(gts, 13, 4))
    # without the DUF downsampling the LQ folder is read
    plain = VideoTestDUFDataset(dict(opt, use_duf_downsampling=False))[7]
    assert tuple(plain['lq'].shape) == (5, 3, 12, 11) and plain['folder'] == 'city'
    assert plain['idx'] == '2/5' and torch.equal(plain['lq'][2], torch.from_numpy(frames['city', 2][:12, :11].astype(np.float32) / 255.0).permute(2, 0, 1))
    # cached: the frames as they are (no crop), as the reference
    cached = VideoTestDUFDataset(dict(opt, cache_data=True))[0]
    assert tuple(cached['gt'].shape) == (3, 50, 45) and cached['lq'].shape[0] == 5
