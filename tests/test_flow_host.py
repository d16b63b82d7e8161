"""Flow warping and SpyNet on the host side (no GPU): the restatement tests/flow_restate.py against the reference's own outputs
(tests/golden/g_zd_spynet.npz, tools/make_golden_spynet.py), the CPU path of ``flow_warp``, SpyNet's state_dict and
initialisation, every refusal, the ABI of include/sr_hip_flow.h (declared, bound, exported, in no other header, each compute
entry point mapped to the GPU test that pins it), the profiler names, the compiled resources read from the code object, and the
semantics of the existing resize kernel the image pyramid reuses.

The host side of flow_ops.hip (argument checks, dispatch, size queries) is also run under the host sanitizers by the stand-alone
program tests/helpers/flow_host_checks.cpp; its result is reported in DESIGN.md."""
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
from torch.nn import functional as F

import image_restoration_amd as ira
from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H
from image_restoration_amd.archs import arch_util
from image_restoration_amd.archs.spynet_arch import SpyNet
from image_restoration_amd.ops.flow_warp import flow_warp, flow_warp_native
from image_restoration_amd.utils.registry import ARCH_REGISTRY

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_flow.h')
SR_EINVAL = -1
_OPS, _NET = 'tests/test_flow_ops_gpu.py::', 'tests/test_spynet_gpu.py::'
PINNED = {
    'sr_conv7x7_instance': _OPS + 'test_conv7x7_matches_float64',
    'sr_conv7x7_packed_floats': _OPS + 'test_conv7x7_matches_float64',
    'sr_conv7x7_pack_f32': _OPS + 'test_conv7x7_matches_float64',
    'sr_conv7x7_f32': _OPS + 'test_conv7x7_matches_float64',
    'sr_flow_warp_f32': _OPS + 'test_warp_matches_float64',
    'sr_flow_warp_bwd_f32': _OPS + 'test_warp_backward_matches_float64',
    'sr_spynet_level_input_f32': _OPS + 'test_level_input_matches_float64',
    'sr_spynet_preprocess_f32': _OPS + 'test_preprocess_and_avgpool_match_float64',
    'sr_avgpool2x2_f32': _OPS + 'test_preprocess_and_avgpool_match_float64',
}
NAMES = ['conv7x7_f32_kernelILi1ELi4EE', 'conv7x7_f32_kernelILi2ELi2EE', 'conv7x7_fewcout_f32_kernel', 'conv7x7_pack_kernel',
         'flow_warp_kernel<*>', 'flow_warp_bwd_dx_kernel<*>', 'flow_warp_bwd_dflow_kernel<*>', 'spynet_level_input_kernel',
         'spynet_preprocess_kernel', 'avgpool2x2_kernel']
KERNELS = ('conv7x7_f32_kernel', 'conv7x7_fewcout_f32_kernel', 'conv7x7_pack_kernel', 'flow_warp_kernel', 'flow_warp_bwd_dx_kernel',
           'flow_warp_bwd_dflow_kernel', 'spynet_level_input_kernel', 'spynet_preprocess_kernel', 'avgpool2x2_kernel')
WARP_SHAPES = ((1, 1), (1, 5), (5, 1), (2, 2), (7, 9))
CASES = (('b2_64x64', 2, 64, 64), ('96x64', 1, 96, 64), ('64x96', 1, 64, 96), ('70x90', 1, 70, 90))


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('pm', ['zeros', 'border'])
def test_restatement_reproduces_the_reference_flow_warp(golden, pm):
    g = golden('g_zd_spynet')
    for h, w in WARP_SHAPES:
        tag = f'warp_{h}x{w}'
        x, flow, gr = g[tag + '_x'], g[tag + '_flow'], g[tag + '_g']
        out = R.flow_warp(x, flow.astype(np.float64), pm)
        dx, dflow, count, _ = R.flow_warp_bwd(x, flow.astype(np.float64), gr, pm)
        assert np.abs(out - g[f'{tag}_{pm}_out']).max() <= 1e-10, tag
        assert np.abs(dx - g[f'{tag}_{pm}_dx']).max() <= 1e-10, tag
        assert np.abs(dflow - g[f'{tag}_{pm}_dflow']).max() <= 1e-10, tag
        assert count.max() <= 4 * h * w and (h * w == 1 or count.max() >= 1)
    # an axis of size 1 ignores the flow, and its flow gradient is 0
    assert np.array_equal(g[f'warp_1x5_{pm}_dflow'][..., 1], np.zeros((2, 1, 5)))
    assert np.array_equal(g[f'warp_1x1_{pm}_out'], g['warp_1x1_x'].astype(np.float64))


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_restatement_reproduces_the_reference_spynet(golden, case):
    g = golden('g_zd_spynet')
    tag, n, h, w = case
    sd = R.spynet_weights(int(g['weight_seed']), float(g['last_scale']))
    assert R.weights_checksum(sd) == str(g['weight_checksum'])
    ref, supp = R.spynet_inputs(int(g['input_seed']) + [c[0] for c in CASES].index(tag), n, h, w)
    out, levels = R.spynet(sd, ref, supp)
    assert out.shape == (n, 2, h, w) and np.abs(out - g[f'spy_{tag}_out']).max() <= 1e-10
    for lv in range(5):
        assert np.abs(levels[lv] - g[f'spy_{tag}_level{lv}']).max() <= 1e-10, lv
    assert np.abs(levels[5]).max() >= 8.0                      # the recipe gives flows that warp
    dist = g[f'spy_{tag}_fp32_dist']
    assert dist.shape == (7,) and 1e-7 < dist[-1] < 2e-5


def test_cpu_flow_warp_agrees_with_the_reference(golden):
    g = golden('g_zd_spynet')
    for h, w in WARP_SHAPES:
        tag = f'warp_{h}x{w}'
        x = torch.from_numpy(g[tag + '_x']).requires_grad_()
        flow = torch.from_numpy(g[tag + '_flow']).requires_grad_()
        gr = torch.from_numpy(g[tag + '_g'])
        # roundings of the fp32 torch path: the position (2^-24 * |position| times the local difference of x) and the blend
        tol = 2.0 ** -24 * float(x.abs().max()) * (8 + 4 * (max(h, w) + 3))
        for pm in ('zeros', 'border'):
            y = flow_warp(x, flow, padding_mode=pm)
            assert y.dtype == torch.float32 and y.grad_fn is not None
            assert np.abs(y.detach().numpy() - g[f'{tag}_{pm}_out']).max() <= tol, (tag, pm)
            dx, df = torch.autograd.grad(y, (x, flow), gr)
            assert np.abs(dx.numpy() - g[f'{tag}_{pm}_dx']).max() <= 4 * tol * float(gr.abs().max()), (tag, pm)
            assert np.abs(df.numpy() - g[f'{tag}_{pm}_dflow']).max() <= 8 * tol * float(gr.abs().max()) * 3, (tag, pm)
    # the definition is the reference's grid_sample call
    x, flow = torch.randn(2, 4, 6, 5), torch.randn(2, 6, 5, 2) * 4
    gy, gx = torch.meshgrid(torch.arange(6.), torch.arange(5.), indexing='ij')
    grid = torch.stack((2 * (gx + flow[..., 0]) / 4 - 1, 2 * (gy + flow[..., 1]) / 5 - 1), 3)
    for pm in ('zeros', 'border'):
        want = F.grid_sample(x, grid, mode='bilinear', padding_mode=pm, align_corners=True)
        assert (flow_warp_native(x, flow, pm) - want).abs().max() <= 1e-5
    assert arch_util.flow_warp is flow_warp


# ------------------------------------------------------------------------------------------------------- SpyNet
def test_spynet_state_dict_and_init():
    torch.manual_seed(3)
    net = SpyNet()
    sd = net.state_dict()
    keys = list(sd)
    want = ['mean', 'std'] + [f'basic_module.{lv}.basic_module.{i}.{p}' for lv in range(6) for i in (0, 2, 4, 6, 8)
                              for p in ('weight', 'bias')]
    assert keys == want and len(keys) == 62
    assert sum(p.numel() for p in net.parameters()) == 1440300
    assert tuple(sd['mean'].shape) == tuple(sd['std'].shape) == (1, 3, 1, 1)
    assert sd['mean'].flatten().tolist() == pytest.approx([0.485, 0.456, 0.406]) and sd['std'].flatten().tolist() == pytest.approx(
        [0.229, 0.224, 0.225])
    for lv in range(6):
        for i, (cin, cout) in zip((0, 2, 4, 6, 8), R.CHANNELS):
            wt, b = sd[f'basic_module.{lv}.basic_module.{i}.weight'], sd[f'basic_module.{lv}.basic_module.{i}.bias']
            assert tuple(wt.shape) == (cout, cin, 7, 7) and tuple(b.shape) == (cout,)
            bound = 1 / (cin * 49) ** 0.5          # nn.Conv2d's default: U(+-1 / sqrt(fan_in)) for both
            assert float(wt.abs().max()) <= bound and float(b.abs().max()) <= bound
            if wt.numel() >= 1568:
                assert abs(float(wt.std()) - bound / 3 ** 0.5) <= 0.08 * bound and abs(float(wt.mean())) <= 0.05 * bound
    # the same draws as nn.Conv2d in the same order
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(8, 32, 7, 1, 3)
    assert torch.equal(conv.weight, sd['basic_module.0.basic_module.0.weight']) and torch.equal(conv.bias, sd['basic_module.0.basic_module.0.bias'])
    assert ARCH_REGISTRY.get('SpyNet') is SpyNet and isinstance(ira.build_network(dict(type='SpyNet')), SpyNet)
    # the seeded weights of the fixture load strictly
    net.load_state_dict({k: torch.from_numpy(v) for k, v in R.spynet_weights(1).items()}, strict=True)


def test_spynet_loads_a_params_checkpoint(tmp_path):
    src = SpyNet()
    path = str(tmp_path / 'spynet.pth')
    torch.save({'params': {k: v for k, v in src.state_dict().items() if k not in ('mean', 'std')}}, path)
    net = SpyNet(load_path=path)
    for k, v in src.state_dict().items():
        assert torch.equal(net.state_dict()[k], v), k


# ----------------------------------------------------------------------------------------------------- refusals
def test_flow_warp_refusals():
    x, flow = torch.zeros(1, 3, 4, 5), torch.zeros(1, 4, 5, 2)
    for bad, needle in ((dict(interp_mode='nearest'), 'nearest'), (dict(padding_mode='reflection'), 'reflection'),
                        (dict(align_corners=False), 'align_corners')):
        with pytest.raises(ValueError, match=needle) as e:
            flow_warp(x, flow, **bad)
        assert 'supported' in str(e.value)
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(ValueError, match='supported: fp32'):
            flow_warp(x.to(dt), flow.to(dt))
    with pytest.raises(ValueError, match='must agree'):
        flow_warp(x, torch.zeros(1, 5, 4, 2))
    with pytest.raises(ValueError, match='expected x'):
        flow_warp(x, torch.zeros(1, 4, 5, 3))


def test_spynet_refusals():
    net = SpyNet().eval()
    with pytest.raises(ValueError, match='same size'):
        net(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 96))
    with pytest.raises(ValueError, match=r'\[N, 3, H, W\]'):
        net(torch.zeros(1, 4, 64, 64), torch.zeros(1, 4, 64, 64))
    for side in ((16, 16), (32, 32), (32, 96), (96, 32)):
        with pytest.raises(ValueError, match='too small'):
            net(torch.zeros(1, 3, *side), torch.zeros(1, 3, *side))
    with pytest.raises(ValueError, match='supported: fp32'):
        net(torch.zeros(1, 3, 64, 64).half(), torch.zeros(1, 3, 64, 64).half())
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        net(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))


def test_wrapper_and_resize_flow_refusals():
    for cin, cout in ((8, 16), (16, 32), (3, 2), (64, 64), (8, 2)):
        with pytest.raises(ValueError, match='not supported'):
            H.conv7x7_instance(cout, cin)
    assert [H.conv7x7_instance(co, ci) for ci, co in H.CONV7X7_SHAPES] == [0, 1, 0, 0, 2]
    flow = torch.zeros(1, 2, 4, 4)
    with pytest.raises(ValueError, match='ratio or shape'):
        arch_util.resize_flow(flow, 'scale', [2, 2])
    with pytest.raises(ValueError, match='not supported'):
        arch_util.resize_flow(flow, 'ratio', [2, 2], interp_mode='nearest')
    with pytest.raises(ValueError, match='not supported'):
        arch_util.resize_flow(flow, 'shape', [8, 8], align_corners=True)
    with pytest.raises(ValueError, match=r'\[N, 2, H, W\]'):
        arch_util.resize_flow(torch.zeros(1, 3, 4, 4), 'shape', [8, 8])


def test_c_abi_refuses_before_any_launch():
    lib = _lib.load()
    P, Q = 256, 4096
    assert lib.sr_flow_warp_f32(P, P, Q, 1, 3, 8, 8, 0, 2, None) == SR_EINVAL           # reflection
    assert b'padding 2 is not supported' in lib.sr_last_error()
    assert lib.sr_flow_warp_f32(P, P, Q, 1, 3, 8, 8, 3, 0, None) == SR_EINVAL
    assert lib.sr_flow_warp_bwd_f32(P, P, None, Q, Q, 1, 3, 8, 8, 0, 0, None) == SR_EINVAL
    assert lib.sr_flow_warp_bwd_f32(P, P, P, None, None, 1, 3, 8, 8, 0, 0, None) == 0   # nothing wanted, nothing launched
    d = _lib.Conv7x7Desc()
    d.in_, d.in_img_stride, d.cin, d.cout, d.n, d.h, d.w, d.packed, d.out, d.out_img_stride = P, 8 * 64, 8, 16, 1, 8, 8, Q, Q, 16 * 64
    assert lib.sr_conv7x7_f32(C.byref(d), None) == SR_EINVAL
    assert b'(cin, cout) = (8, 16) is not supported; supported: (8, 32), (32, 64), (64, 32), (32, 16), (16, 2)' in lib.sr_last_error()
    assert lib.sr_conv7x7_pack_f32(P, None, 4, 16, Q, None) == SR_EINVAL
    assert lib.sr_spynet_level_input_f32(P, P, P, Q, Q, 1, 7, 8, None) == SR_EINVAL
    assert lib.sr_avgpool2x2_f32(P, Q, 3, 7, 8, None) == SR_EINVAL
    m3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    assert lib.sr_spynet_preprocess_f32(P, Q, 0, 8, 8, m3, m3, None) == SR_EINVAL


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_every_declared_entry_point_is_bound_exported_and_pinned():
    declared = set(re.findall(r'\b(?:int|size_t)\s+(sr_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(_lib.FLOW_SIGNATURES) == set(PINNED) and len(declared) == 9
    others = set()
    for name in dir(_lib):
        if name.endswith('SIGNATURES') and name != 'FLOW_SIGNATURES':
            others |= set(getattr(_lib, name))
    assert others and not declared & others
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'sr_hip_flow.h':
            text = open(os.path.join(ROOT, 'include', other)).read()
            assert not any(s in text for s in declared), other      # declared apart from the existing headers
    for s, target in PINNED.items():
        path, _, func = target.partition('::')
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith('test_')}
        assert func in tests, (s, target)
    # every stream-ordered entry point has one hip_ops wrapper that goes through launch
    src = open(os.path.join(ROOT, 'image_restoration_amd', 'hip_ops.py')).read()
    for s, (res, args) in _lib.FLOW_SIGNATURES.items():
        if res is C.c_int and args and args[-1] is C.c_void_p and s != 'sr_conv7x7_instance':
            assert src.count(f"_launch_arg('{s}'") == 1, s
    assert C.sizeof(_lib.Conv7x7Desc) == 88


def test_profiler_ids_resolve_from_148():
    lib = _lib.load()
    assert [lib.sr_kernel_name(i).decode() for i in range(148, 158)] == NAMES
    assert lib.sr_kernel_name(147).decode() == '' and lib.sr_kernel_name(158).decode() == ''
    assert lib.sr_kernel_name(146).decode() == 'degrade_finish_kernel<*>'


def test_kernels_use_no_scratch_and_the_conv_instances_are_the_dispatch(tmp_path):
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
                cur = found.setdefault(val, {}) if any(re.search(r'\d' + k + r'(I|E)', val) for k in KERNELS) else None
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count'):
                cur[key] = int(val)
    for k in KERNELS:
        assert any(k in name for name in found), (k, sorted(found))
    assert len(found) == 13, sorted(found)       # 3 conv instances, 6 warp kernels (two layouts each), pack, level, preprocess, pool
    for name, md in found.items():
        assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 \
            and md.get('sgpr_spill_count', 0) == 0 and md['vgpr_count'] <= 128, (name, md)      # 128: two workgroups per CU
    # the compiled conv instances are exactly what the dispatch can return
    inst = set()
    for name in found:
        if 'conv7x7_fewcout_f32_kernel' in name:
            inst.add(2)
        m = re.search(r'conv7x7_f32_kernelILi(\d)ELi(\d)EE', name)
        if m:
            inst.add({('1', '4'): 0, ('2', '2'): 1}[m.groups()])
    lib_ = _lib.load()
    reachable = {lib_.sr_conv7x7_instance(co, ci) for ci in range(0, 72) for co in range(0, 72)} - {-1}
    assert inst == reachable == {0, 1, 2}
    assert {lib_.sr_conv7x7_instance(co, ci) for ci, co in H.CONV7X7_SHAPES} == reachable


# ------------------------------------------------------------------------------- what the pyramid reuses, on the host
def test_pyramid_steps_are_the_reference_ops():
    """The restatement's resize (the rule sr_resize_bilinear_f32 documents: half-pixel centres, scale = in / out, clamped at 0) is
    F.interpolate(align_corners=False); its x2 upsampling is F.interpolate(scale_factor=2, align_corners=True); its pool is
    F.avg_pool2d — so SpyNet reuses the resize kernel for both resizes and needs no pad kernel."""
    x = torch.randn(2, 3, 70, 90, dtype=torch.float64)
    for size in ((96, 96), (64, 96), (35, 45)):
        want = F.interpolate(x, size=size, mode='bilinear', align_corners=False).numpy()
        assert np.abs(R.resize_half_pixel(x.numpy(), *size) - want).max() <= 1e-12
    f = torch.randn(2, 2, 3, 2, dtype=torch.float64)
    want = F.interpolate(f, scale_factor=2, mode='bilinear', align_corners=True).numpy()
    assert np.abs(R.upsample2_align(f.numpy()) - want).max() <= 1e-12
    f1 = torch.randn(1, 2, 1, 1, dtype=torch.float64)
    assert np.abs(R.upsample2_align(f1.numpy()) - F.interpolate(f1, scale_factor=2, mode='bilinear', align_corners=True).numpy()).max() == 0
    assert np.abs(R.avgpool2(x[:, :, :70, :90].numpy()) - F.avg_pool2d(x, 2, 2).numpy()).max() <= 1e-15
    # header of the reused kernel states the same rule
    text = open(os.path.join(ROOT, 'include', 'sr_hip_degrade.h')).read()
    assert "F.interpolate(mode='bilinear', align_corners=False)" in text and '(d + 0.5f) * scale - 0.5f' in text
