"""TOFlow on the host side (no GPU): the restatement tests/tof_restate.py against the reference's own float64 outputs
(tests/golden/g_zi_tof.npz, tools/make_golden_tof.py) and what the fixture must show, TOFlow's state_dict and initialisation, the
BatchNorm fold, every refusal, the ABI of include/sr_hip_tof.h (declared, bound, exported, in no other header, each entry point
mapped to the GPU test that pins it), the profiler names, the compiled resources read from the code object and both option
files."""
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

import image_restoration_amd as ira
from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H
from image_restoration_amd.archs import tof_arch
from image_restoration_amd.archs.tof_arch import SPyNetTOF, TOFlow
from image_restoration_amd.utils import synth
from image_restoration_amd.utils.registry import ARCH_REGISTRY

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tof_restate as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_tof.h')
SR_EINVAL = -1
_OPS = 'tests/test_tof_ops_gpu.py::'
PINNED = {
    'sr_tof_conv9x9_packed_floats': _OPS + 'test_conv9x9_matches_float64',
    'sr_tof_conv9x9_pack_f32': _OPS + 'test_conv9x9_matches_float64',
    'sr_tof_conv9x9_f32': _OPS + 'test_conv9x9_matches_float64',
    'sr_tof_level_input_f32': _OPS + 'test_level_input_matches_the_flow_header_bit_for_bit',
    'sr_tof_align_f32': _OPS + 'test_aligned_stack_is_the_per_frame_zeros_warp',
    'sr_tof_finish_f32': _OPS + 'test_finish_is_bit_identical_to_torch',
}
NAMES = ['tof_conv9x9_f32_kernel', 'tof_conv9x9_pack_kernel', 'tof_level_input_kernel', 'tof_align_kernel', 'tof_finish_kernel']


@pytest.fixture(scope='module')
def fixture(golden):
    g = golden('g_zi_tof')
    return g, synth.tof_state_dict(int(g['weight_seed']))


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('case', T.CASES, ids=[c[0] for c in T.CASES])
def test_restatement_reproduces_the_reference(fixture, case):
    g, sd = fixture
    tag, b, h, w = case
    assert T.R.weights_checksum(sd) == str(g['weight_checksum'])
    u8 = g[f'{tag}_clip_u8']
    assert u8.shape == (b, 7, 3, h, w) and np.array_equal(u8, T.clip_u8(int(g['input_seed']) + [c[0] for c in T.CASES].index(tag), b, h, w))
    x = T.decode(u8)
    for adapt in (False, True):
        out, flows = T.toflow(sd, x, adapt)
        s = f'{tag}_adapt{int(adapt)}'
        assert out.shape == (b, 3, h, w) and np.abs(out - g[s + '_out']).max() <= 1e-12            # every pixel, no mask
        assert flows.shape == (6 * b, 2, h, w) and np.abs(flows - g[tag + '_flows']).max() <= 1e-12
        # what the fixture must show: flows that warp, an output that is not the reference frame, and a measurable fp32 distance
        peak = np.abs(g[tag + '_flows']).reshape(6 * b, -1).max(1)
        assert peak.max() > 1.0 and peak.max() < 8.0
        assert np.abs(g[s + '_out'] - x[:, 3].astype(np.float64)).max() >= 0.05                    # denormalize(lr_ref) is frame 3
        assert 1e-8 < float(g[s + '_out_fp32_dist']) < 1e-5 and 1e-8 < float(g[s + '_flows_fp32_dist']) < 1e-4


def test_restated_pieces_are_the_reference_ops():
    """conv, BatchNorm, level input, stack and finish of the restatement against torch's float64 ops."""
    from torch.nn import functional as F
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 5, 6, 7))
    for k in (1, 7, 9):
        wt, b = rng.standard_normal((4, 5, k, k)), rng.standard_normal(4)
        want = F.conv2d(torch.from_numpy(x), torch.from_numpy(wt), torch.from_numpy(b), 1, k // 2).numpy()
        got, mag = T.conv(x, wt, b, want_mag=True)
        assert np.abs(got - want).max() <= 1e-12 and (mag >= np.abs(got) - 1e-12).all()
    gamma, beta, mean, var = rng.uniform(0.5, 1.5, 5), rng.standard_normal(5), rng.standard_normal(5), rng.uniform(0.5, 2, 5)
    want = F.batch_norm(torch.from_numpy(x), torch.from_numpy(mean), torch.from_numpy(var), torch.from_numpy(gamma), torch.from_numpy(beta),
                        False, 0.1, 1e-5).numpy()
    assert np.abs(T.batchnorm_eval(x, gamma, beta, mean, var) - want).max() <= 1e-12
    # level input: tof_arch.py:86-89 with grid_sample
    ref, supp, prev = rng.standard_normal((2, 3, 6, 10)), rng.standard_normal((2, 3, 6, 10)), rng.standard_normal((2, 2, 3, 5)) * 3
    up = F.interpolate(torch.from_numpy(prev), scale_factor=2, mode='bilinear', align_corners=True) * 2.0
    gy, gx = torch.meshgrid(torch.arange(6.).double(), torch.arange(10.).double(), indexing='ij')
    grid = torch.stack((2 * (gx + up[:, 0]) / 9 - 1, 2 * (gy + up[:, 1]) / 5 - 1), 3)
    warped = F.grid_sample(torch.from_numpy(supp), grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    got, got_up = T.level_input(ref, supp, prev)
    assert np.abs(got - torch.cat([torch.from_numpy(ref), warped, up], 1).numpy()).max() <= 1e-12 and np.abs(got_up - up.numpy()).max() <= 1e-12
    y, lr = rng.standard_normal((2, 3, 4, 4)), rng.standard_normal((2, 3, 4, 4))
    assert np.abs(T.finish(y, lr) - ((y + lr) * T.STD[None, :, None, None] + T.MEAN[None, :, None, None])).max() == 0


# ------------------------------------------------------------------------------------------------------ the network
def test_state_dict_and_init(fixture):
    g, sd = fixture
    torch.manual_seed(11)
    net = TOFlow()
    own = net.state_dict()
    assert list(own) == [str(k) for k in g['keys']] == list(sd) and len(own) == 114
    assert [','.join(str(d) for d in v.shape) for v in own.values()] == [str(s) for s in g['shapes']]
    assert sum(p.numel() for p in net.parameters()) == int(g['num_params']) == 1405899
    assert sum(k.endswith('num_batches_tracked') for k in own) == 16 and own['mean'].shape == own['std'].shape == (1, 3, 1, 1)
    # a seeded fresh network has the reference's initial parameters (the same draws in the same order)
    for k in g:
        if k.startswith('init_'):
            assert np.array_equal(own[k[5:]].flatten()[:8].numpy(), g[k]), k
    w = own['conv_2.weight']
    bound = 1 / (64 * 81) ** 0.5
    assert float(w.abs().max()) <= bound and abs(float(w.std()) - bound / 3 ** 0.5) <= 0.05 * bound
    bn = net.spynet.basic_module[0].basic_module[1]
    assert isinstance(bn, torch.nn.BatchNorm2d) and bool((bn.weight == 1).all()) and bool((bn.running_var == 1).all()) and bn.eps == 1e-5
    assert net.spynet.basic_module[2].basic_module[3].bias is None
    assert TOFlow().ref_idx == 3 and TOFlow(adapt_official_weights=True).ref_idx == 0 and TOFlow(True).adapt_official_weights
    assert ARCH_REGISTRY.get('TOFlow') is TOFlow and isinstance(ira.build_network(dict(type='TOFlow')), TOFlow)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    assert int(net.state_dict()['spynet.basic_module.0.basic_module.1.num_batches_tracked']) == 100


def test_spynet_tof_loads_a_params_checkpoint(tmp_path):
    src = SPyNetTOF()
    assert len(src.state_dict()) == 104
    path = str(tmp_path / 'spynet_tof.pth')
    torch.save({'params': src.state_dict()}, path)
    net = SPyNetTOF(load_path=path)
    for k, v in src.state_dict().items():
        assert torch.equal(net.state_dict()[k], v), k


def test_batchnorm_fold_matches_float64_eval_batchnorm():
    rng = np.random.default_rng(3)
    for cin, cout in ((8, 32), (32, 16)):
        x = rng.standard_normal((2, cin, 9, 11))
        wt = rng.standard_normal((cout, cin, 7, 7)).astype(np.float32)
        gamma, beta = rng.uniform(0.2, 3, cout).astype(np.float32), rng.standard_normal(cout).astype(np.float32)
        mean, var = rng.standard_normal(cout).astype(np.float32), rng.uniform(0.01, 4, cout).astype(np.float32)
        w2, b2 = tof_arch.fold_batchnorm(*(torch.from_numpy(t) for t in (wt, gamma, beta, mean, var)), 1e-5)
        assert w2.dtype == b2.dtype == torch.float32
        w64, b64 = T.fold(wt, gamma, beta, mean, var)
        # rounded once from float64: half an ulp
        assert (np.abs(w2.numpy() - w64) <= 2.0 ** -24 * np.abs(w64)).all() and (np.abs(b2.numpy() - b64) <= 2.0 ** -24 * np.abs(b64) + 1e-30).all()
        pre, _ = T.conv(x, wt)
        want = T.batchnorm_eval(pre, gamma, beta, mean, var)
        got, mag = T.conv(x, w64, b64, want_mag=True)
        assert (np.abs(got - want) <= 1e-12 * (mag + 1)).all()


def test_python_refusals():
    net = TOFlow().eval()
    x = torch.zeros(1, 7, 3, 16, 16)
    for bad in (x[:, :5], x[:, :, :2], x[0], x.half(), x.double()):
        with pytest.raises(ValueError, match=r'\[b, 7, 3, h, w\]'):
            net(bad)
    for side in ((16, 24), (8, 16), (40, 32)):
        with pytest.raises(ValueError, match='multiples of 16'):
            net(torch.zeros(1, 7, 3, *side))
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        with torch.no_grad():
            net(x)
    with pytest.raises(NotImplementedError, match='inference'):
        net(x)                                                   # grad enabled and the parameters require grad
    for p in net.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match='inference'):
        net(x.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match=r'\.eval\(\)'):
        with torch.no_grad():
            net.train()(x)                                       # training mode, even under no_grad
    spy = SPyNetTOF().eval()
    r = torch.zeros(2, 3, 16, 32)
    with pytest.raises(ValueError, match='same size'):
        spy(r, r[:1])
    with pytest.raises(ValueError, match=r'\[N, 3, H, W\]'):
        spy(r[:, :2], r[:, :2])
    with pytest.raises(ValueError, match='multiples of 16'):
        spy(r[:, :, :, :20], r[:, :, :, :20])
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        with torch.no_grad():
            spy(r, r)
    with pytest.raises(NotImplementedError, match=r'\.eval\(\)'):
        with torch.no_grad():
            spy.train()(r, r)
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        H.PackedConv9x9(torch.zeros(64, 64, 9, 9))


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_every_declared_entry_point_is_bound_exported_and_pinned():
    declared = set(re.findall(r'\b(?:int|size_t)\s+(sr_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(_lib.TOF_SIGNATURES) == set(PINNED) and len(declared) == 6
    others = set()
    for name in dir(_lib):
        if name.endswith('SIGNATURES') and name != 'TOF_SIGNATURES':
            others |= set(getattr(_lib, name))
    assert others and not declared & others
    assert not any(o in s for o in others for s in declared)              # no new name contains an existing one
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    text = open(HEADER).read()
    # the new header spells no entry point of another companion header (sr_hip.h's own sr_last_error / sr_kernel_name it may)
    assert not any(o in text for o in others - set(_lib.SIGNATURES))
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'sr_hip_tof.h':
            assert not any(s in open(os.path.join(ROOT, 'include', other)).read() for s in declared), other
    for s, target in PINNED.items():
        path, _, func = target.partition('::')
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        assert func in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, (s, target)
    src = open(os.path.join(ROOT, 'image_restoration_amd', 'hip_ops.py')).read()
    for s, (res, args) in _lib.TOF_SIGNATURES.items():
        if res is C.c_int:
            assert src.count(f"_launch_arg('{s}'") == 1, s
    assert C.sizeof(_lib.TofConv9x9Desc) == 72


def test_profiler_ids_resolve_from_188():
    lib = _lib.load()
    assert [lib.sr_kernel_name(i).decode() for i in range(188, 193)] == NAMES
    assert lib.sr_kernel_name(187).decode() == '' and lib.sr_kernel_name(193).decode() == ''
    assert lib.sr_kernel_name(186).decode() == 'deform_det_finish_kernel'


def test_kernels_use_no_scratch_and_one_conv_instance_is_compiled(tmp_path):
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
                cur = found.setdefault(val, {}) if re.search(r'\dtof_\w+_kernel', val) else None
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count'):
                cur[key] = int(val)
    assert sorted(re.search(r'\d(tof_\w+?_kernel)', n).group(1) for n in found) == sorted(NAMES), sorted(found)
    for name, md in found.items():
        assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 \
            and md.get('sgpr_spill_count', 0) == 0 and md['vgpr_count'] <= 128, (name, md)      # 128: two workgroups per CU
    # one 9x9 instance is compiled, and the pairs it serves are the two of TOFlow
    lib_ = _lib.load()
    served = {(ci, co) for ci in range(0, 72) for co in range(0, 72) if lib_.sr_tof_conv9x9_packed_floats(co, ci)}
    assert served == set(H.CONV9X9_SHAPES) == {(21, 64), (64, 64)}
    assert lib_.sr_tof_conv9x9_packed_floats(64, 21) == 3 * 81 * 512 + 64 and lib_.sr_tof_conv9x9_packed_floats(64, 64) == 8 * 81 * 512 + 64


def test_c_abi_refuses_before_any_launch():
    """Every SR_EINVAL of every entry point, with fake aligned addresses: nothing is launched, so nothing is dereferenced."""
    lib = _lib.load()
    P, Q = 256, 4096

    def refused(rc, needle):
        assert rc == SR_EINVAL and needle in lib.sr_last_error(), (rc, lib.sr_last_error())

    # pack
    refused(lib.sr_tof_conv9x9_pack_f32(P, None, 64, 24, Q, None), b'(cin, cout) = (24, 64) is not supported; supported: (21, 64), (64, 64)')
    refused(lib.sr_tof_conv9x9_pack_f32(None, None, 64, 64, Q, None), b'null weight / packed')
    refused(lib.sr_tof_conv9x9_pack_f32(P, None, 64, 64, None, None), b'null weight / packed')
    refused(lib.sr_tof_conv9x9_pack_f32(P, None, 64, 64, Q + 4, None), b'16-byte aligned')

    # conv
    def desc(**kw):
        d = _lib.TofConv9x9Desc()
        d.in_, d.in_img_stride, d.cin, d.cout, d.n, d.h, d.w, d.packed, d.out, d.out_img_stride, d.relu = P, 24 * 64, 21, 64, 1, 8, 8, Q, Q, 64 * 64, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    refused(lib.sr_tof_conv9x9_f32(None, None), b'null descriptor')
    for cin, cout in ((24, 64), (64, 32), (8, 64)):
        refused(lib.sr_tof_conv9x9_f32(C.byref(desc(cin=cin, cout=cout)), None), b'is not supported; supported: (21, 64), (64, 64)')
    for k in ('in_', 'packed', 'out'):
        refused(lib.sr_tof_conv9x9_f32(C.byref(desc(**{k: None})), None), b'null in / packed / out')
    for k, v in (('n', 0), ('h', 0), ('w', -1)):
        refused(lib.sr_tof_conv9x9_f32(C.byref(desc(**{k: v})), None), b'bad shape')
    for k in ('in_', 'packed', 'out'):
        refused(lib.sr_tof_conv9x9_f32(C.byref(desc(**{k: P + 8})), None), b'16-byte aligned')
    for k in ('in_img_stride', 'out_img_stride'):
        refused(lib.sr_tof_conv9x9_f32(C.byref(desc(**{k: 64 * 64 + 2})), None), b'multiples of 4 floats')
    refused(lib.sr_tof_conv9x9_f32(C.byref(desc(relu=2)), None), b'relu must be 0 or 1')
    refused(lib.sr_tof_conv9x9_f32(C.byref(desc(h=4096, w=4096, in_img_stride=1 << 40, out_img_stride=1 << 40)), None), b'too large')
    refused(lib.sr_tof_conv9x9_f32(C.byref(desc(in_img_stride=16 * 64)), None), b'smaller than the image')
    refused(lib.sr_tof_conv9x9_f32(C.byref(desc(out_img_stride=56 * 64)), None), b'smaller than the image')

    # level input: (ref, ref stride, supp, supp stride, group, skip, flow_prev, out, up_out, N, H, W)
    ok = dict(ref=P, rs=3 * 64, supp=P, ss=3 * 64, group=1, skip=1, prev=Q, out=Q, up=Q, N=2, H=8, W=8)

    def level(**kw):
        a = dict(ok, **kw)
        return lib.sr_tof_level_input_f32(a['ref'], a['rs'], a['supp'], a['ss'], a['group'], a['skip'], a['prev'], a['out'], a['up'], a['N'],
                                          a['H'], a['W'], None)
    for k in ('ref', 'supp', 'out', 'up'):
        refused(level(**{k: None}), b'null ref / supp / out / up_out')
    for k, v in (('N', 0), ('N', 65536), ('H', 0), ('W', 0)):
        refused(level(**{k: v}), b'bad shape')
    for kw in (dict(group=0), dict(group=3), dict(skip=-1), dict(skip=2)):
        refused(level(**kw), b'must be a multiple of group')
    refused(level(H=7), b'must be even above the coarsest level')
    refused(level(W=9), b'must be even above the coarsest level')
    refused(level(H=1 << 14, W=1 << 14, rs=1 << 40, ss=1 << 40), b'too large')
    refused(level(rs=3 * 64 - 1), b'group stride')
    refused(level(N=6, group=6, skip=3, ss=6 * 3 * 64), b'group stride')          # six pairs of a clip need seven frames
    for k in ('out', 'up', 'prev'):
        refused(level(**{k: Q + 4}), b'16-byte aligned')

    # aligned stack: (clip, flows, flow stride, out, out stride, b, ref_idx, h, w)
    ok = dict(clip=P, flows=Q, fs=8 * 64, out=Q, os=24 * 64, b=1, r=3, h=8, w=8)

    def align(**kw):
        a = dict(ok, **kw)
        return lib.sr_tof_align_f32(a['clip'], a['flows'], a['fs'], a['out'], a['os'], a['b'], a['r'], a['h'], a['w'], None)
    for k in ('clip', 'flows', 'out'):
        refused(align(**{k: None}), b'null clip / flows / out')
    for k, v in (('b', 0), ('b', 65536), ('h', 0), ('w', 0)):
        refused(align(**{k: v}), b'bad shape')
    for r in (-1, 7):
        refused(align(r=r), b'not one of the 7 frames')
    refused(align(h=1 << 13, w=1 << 13, fs=1 << 40, os=1 << 40), b'too large')
    for k in ('flows', 'out'):
        refused(align(**{k: Q + 8}), b'16-byte aligned')
    for k in ('fs', 'os'):
        refused(align(**{k: 24 * 64 + 2}), b'multiples of 4 floats')
    refused(align(fs=8 * 64 - 4), b'smaller than the image')
    refused(align(os=24 * 64 - 4), b'smaller than the image')

    # finish: (y, y stride, lr_ref, lr stride, out, n, h, w, mean3, std3)
    m3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    ok = dict(y=Q, ys=8 * 64, lr=P, ls=3 * 64, out=P, n=1, h=8, w=8, mean=m3, std=m3)

    def fin(**kw):
        a = dict(ok, **kw)
        return lib.sr_tof_finish_f32(a['y'], a['ys'], a['lr'], a['ls'], a['out'], a['n'], a['h'], a['w'], a['mean'], a['std'], None)
    for k in ('y', 'lr', 'out', 'mean', 'std'):
        refused(fin(**{k: None}), b'null y / lr_ref / out / mean3 / std3')
    for k, v in (('n', 0), ('n', 65536), ('h', 0), ('w', 0)):
        refused(fin(**{k: v}), b'bad shape')
    refused(fin(h=1 << 14, w=1 << 14, ys=1 << 40, ls=1 << 40), b'too large')
    refused(fin(y=Q + 4), b'16-byte aligned')
    refused(fin(ys=8 * 64 + 2), b'multiple of 4 floats')
    refused(fin(ys=8 * 64 - 4), b'smaller than the image')
    refused(fin(ls=3 * 64 - 1), b'smaller than the image')


# ------------------------------------------------------------------------------------------------------------- options
def test_option_files_parse_and_build():
    import image_restoration_amd.models  # noqa: F401  (fills MODEL_REGISTRY)
    from image_restoration_amd.data import SyntheticClipDataset
    from image_restoration_amd.utils.registry import DATASET_REGISTRY, MODEL_REGISTRY
    d = os.path.join(ROOT, 'options', 'test', 'TOF')
    off = yaml.safe_load(open(os.path.join(d, 'test_TOF_official.yml')))
    assert off['model_type'] == 'VideoBaseModel' and off['network_g'] == dict(type='TOFlow', adapt_official_weights=True)
    ds = off['datasets']['test']
    assert (ds['type'], ds['num_frame'], ds['padding'], ds['cache_data']) == ('VideoTestDataset', 7, 'reflection_circle', False)
    assert ds['dataroot_gt'] == 'datasets/Vid4/GT' and ds['dataroot_lq'] == 'datasets/Vid4/BIx4up_direct' and ds['name'] == 'Vid4'
    assert off['path']['strict_load_g'] is True and off['path']['pretrain_network_g'].endswith('tof_x4_vimeo90k_official-32c9e01f.pth')
    assert {m['type'] for m in off['val']['metrics'].values()} == {'calculate_psnr', 'calculate_ssim'} and off['val']['save_img']
    syn = yaml.safe_load(open(os.path.join(d, 'test_TOF_synthetic.yml')))
    assert syn['model_type'] == 'VideoBaseModel' and syn['network_g']['type'] == 'TOFlow' and syn['path']['pretrain_network_g'] is None
    for opt in (off, syn):
        assert MODEL_REGISTRY.get(opt['model_type']) is not None and DATASET_REGISTRY.get(opt['datasets']['test']['type']) is not None
        net = ira.build_network(dict(opt['network_g']))
        assert isinstance(net, TOFlow) and net.adapt_official_weights == opt['network_g']['adapt_official_weights']
    # the synthetic set gives what VideoBaseModel's validation reads: 7 frames at the GT size, a folder per clip
    sopt = dict(syn['datasets']['test'])
    sds = SyntheticClipDataset(sopt)
    item = sds[1]
    assert len(sds) == sopt['num_samples'] and sds.data_info['folder'] == [f'{i:08d}' for i in range(len(sds))]
    assert tuple(item['lq'].shape) == (7, 3, 64, 64) and tuple(item['gt'].shape) == (3, 64, 64) and torch.equal(item['lq'][3], item['gt'])
    assert item['folder'] == '00000001' and item['idx'] == '0/1' and item['lq_path'].endswith('.png')
    assert 'folder' not in SyntheticClipDataset(dict(sopt, video_test=False))[1]          # the default item is unchanged
