"""The bf16 forward of BasicVSR / IconVSR on the host side (no GPU): the ABI of include/sr_hip_vsr_bf16.h (declared, bound,
exported, in no other header, each entry point mapped to the GPU test that pins it), every C-side refusal, the restated blob and
workspace sizes, the profiler name, the compiled resources of the new kernel read from the code object; ``set_compute_dtype`` and
what it must leave alone (signatures, keys, initialisation); the option route on the CPU; and the rounding model
tests/vsr_bf16_restate.py: exact without rounding, its float32-accumulation proxy against the project's bf16 network bound, and
negative controls.

CPU proxies, measured on the committed fixtures before the first GPU run (proxy = max |y_acc32 - y64|, bound = 2 max |y_model - y64|
+ 4 fp32 ulp of max |y64|):
    BasicVSR b1 n3 33x40    d_model 1.04e-4    proxy / bound 0.47
    BasicVSR b2 n2 34x33    d_model 1.02e-4    proxy / bound 0.51
    IconVSR b1 n6 34x38, whole (keyframe features from the bf16 extractor model)    d_model 5.1e-2    proxy / bound 0.41
    IconVSR, keyframe features alone (magnitude 60)    d_model 22 / 23 / 18    proxy / bound 0.61 / 0.58 / 0.61
    IconVSR, propagate on float64 keyframe features rounded once to bf16    d_model 2.3e-3    proxy / bound 0.45
All are <= 0.75, so the GPU tests check IconVSR whole (and in the split form as well).  Negative controls (BasicVSR, distance from
y64 over the bound, first case): zeroed flows 7.3, swapped flow planes 7.1, zeroed backward features 13.9 (the second case, measured
once the same way: 7.1, 7.1, 15.4).

The bf16 host side of vsr_ops.hip (argument checks, size queries, plan building) is also run under the host sanitizers by the
stand-alone program tests/helpers/vsr_host_checks.cpp; its result is reported in DESIGN.md §33 and §35.
"""
import ast
import ctypes as C
import hashlib
import inspect
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
import flow_restate as FR  # noqa: E402
import vsr_bf16_restate as B  # noqa: E402
import vsr_restate as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_vsr_bf16.h')
SR_EINVAL, SR_ENOSPACE = -1, -3
_OPS = 'tests/test_vsr_bf16_ops_gpu.py::'
PINNED = {
    'sr_rvsr_prop_input_bf16': _OPS + 'test_prop_input_is_the_rounded_flow_warp_and_the_frame_block_bit_for_bit',
    'sr_rvsr_trunk_packed_bytes_bf16': _OPS + 'test_trunk_driver_is_the_per_layer_composition_bit_for_bit',
    'sr_rvsr_trunk_pack_bf16': _OPS + 'test_trunk_driver_is_the_per_layer_composition_bit_for_bit',
    'sr_rvsr_trunk_workspace_bytes_bf16': _OPS + 'test_trunk_driver_is_the_per_layer_composition_bit_for_bit',
    'sr_rvsr_trunk_bf16': _OPS + 'test_trunk_driver_is_the_per_layer_composition_bit_for_bit',
}
PACK_ENTRY_BYTES = 120     # sizeof(sr::PackEntry), sr_internal.h (tests/test_vsr_host.py)
PROXY_LIMIT = 0.75


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_every_declared_entry_point_is_bound_exported_and_pinned():
    declared = set(re.findall(r'\b(?:int|size_t)\s+(sr_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(_lib.VSR_BF16_SIGNATURES) == set(PINNED) and len(declared) == 5
    others = set()
    for name in dir(_lib):
        if name.endswith('SIGNATURES') and name != 'VSR_BF16_SIGNATURES':
            others |= set(getattr(_lib, name))
    assert others and not declared & others
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'sr_hip_vsr_bf16.h':
            text = open(os.path.join(ROOT, 'include', other)).read()
            assert not any(s in text for s in declared), other      # declared apart from the existing headers
    for s, target in PINNED.items():
        path, _, func = target.partition('::')
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith('test_')}
        assert func in tests, (s, target)
    # every stream-ordered entry point has one hip_ops wrapper that goes through _launch_arg
    src = open(os.path.join(ROOT, 'image_restoration_amd', 'hip_ops.py')).read()
    for s, (res, args) in _lib.VSR_BF16_SIGNATURES.items():
        if res is C.c_int and args and args[-1] is C.c_void_p:
            assert src.count(f"_launch_arg('{s}'") == 1, s
    assert sum(src.count(f"_launch_arg('{s}'") for s in declared) == 3
    assert C.sizeof(_lib.RvsrPropDesc) == 96 and C.sizeof(_lib.VsrTrunkCfg) == 12
    assert 'sr_hip_vsr_bf16.h' in open(os.path.join(ROOT, 'image_restoration_amd', 'csrc', 'Makefile')).read()


def test_c_abi_refuses_before_any_launch():
    lib = _lib.load()
    P, Q = 256, 4096

    def refused(rc, needle, code=SR_EINVAL):
        assert rc == code and needle in lib.sr_last_error(), (rc, lib.sr_last_error())
    prop = lib.sr_rvsr_prop_input_bf16
    refused(prop(None, None), b'null descriptor')
    d = _lib.RvsrPropDesc()
    refused(prop(C.byref(d), None), b'null frame')
    d.frame, d.warp_out, d.n, d.h, d.w, d.fb = P, Q, 1, 4, 5, 0
    refused(prop(C.byref(d), None), b'bad shape')
    d.fb, d.flow = 2, P
    refused(prop(C.byref(d), None), b'both')
    d.flow, d.prev = None, P
    refused(prop(C.byref(d), None), b'both')
    d.prev, d.h, d.w = None, 1 << 14, 1 << 14
    refused(prop(C.byref(d), None), b'too large')
    d.h, d.w, d.warp_out = 4, 5, Q + 4
    refused(prop(C.byref(d), None), b'16-byte aligned')
    d.warp_out, d.frame = Q, P + 2
    refused(prop(C.byref(d), None), b'4-byte aligned')
    d.frame, d.warp_out_img_stride = P, 4
    refused(prop(C.byref(d), None), b'multiples of 8')
    d.n, d.warp_out_img_stride, d.frame_img_stride = 2, 16, 60
    refused(prop(C.byref(d), None), b'smaller than the image')
    d.warp_out_img_stride, d.frame_img_stride = 16 * 20 * 2, 59
    refused(prop(C.byref(d), None), b'smaller than the image')
    cfg = H.vsr_trunk_cfg(64, 1, 1)
    trunk = lib.sr_rvsr_trunk_bf16
    refused(trunk(C.byref(cfg), None, P, 0, Q, 0, 1, 8, 8, None, 0, None), b'null packed')
    refused(trunk(C.byref(cfg), P, P, 0, Q, 0, 1, 0, 8, None, 0, None), b'bad shape')
    refused(trunk(C.byref(cfg), P, P, 0, Q, 0, 1, 4096, 4096, None, 0, None), b'too large')
    refused(trunk(C.byref(cfg), P, P + 4, 0, Q, 0, 1, 8, 8, None, 0, None), b'aligned')
    refused(trunk(C.byref(cfg), P, P, 4, Q, 0, 1, 8, 8, None, 0, None), b'multiples of 8')
    refused(trunk(C.byref(cfg), P, P, 80 * 64 - 8, Q, 64 * 64, 2, 8, 8, None, 0, None), b'smaller than the image')
    refused(trunk(C.byref(cfg), P, P, 0, Q, 0, 1, 8, 8, None, 0, None), b'workspace', SR_ENOSPACE)
    need = lib.sr_rvsr_trunk_workspace_bytes_bf16(C.byref(cfg), 1, 8, 8)
    refused(trunk(C.byref(cfg), P, P, 0, Q, 0, 1, 8, 8, 1 << 20, need - 1, None), b'workspace', SR_ENOSPACE)
    pack = lib.sr_rvsr_trunk_pack_bf16
    refused(pack(C.byref(cfg), None, Q, None), b'null argument')
    ptrs = (C.c_void_p * 6)(*[P] * 6)
    refused(pack(C.byref(cfg), ptrs, None, None), b'null argument')
    refused(pack(C.byref(cfg), ptrs, Q + 16, None), b'256-byte aligned')
    ptrs[5] = None
    refused(pack(C.byref(cfg), ptrs, Q, None), b'null parameter')
    for bad in ((24, 1, 1), (8, 1, 1), (64, -1, 1), (64, 1, 3), (0, 1, 1)):
        c = H.vsr_trunk_cfg(*bad)
        refused(pack(C.byref(c), ptrs, Q, None), b'bad config')
        refused(trunk(C.byref(c), P, P, 0, Q, 0, 1, 8, 8, None, 0, None), b'multiple of 16')
        assert lib.sr_rvsr_trunk_packed_bytes_bf16(C.byref(c)) == 0 and lib.sr_rvsr_trunk_workspace_bytes_bf16(C.byref(c), 1, 8, 8) == 0
    assert lib.sr_rvsr_trunk_workspace_bytes_bf16(C.byref(cfg), 0, 8, 8) == 0


@pytest.mark.parametrize('num_feat', [64, 48, 16])
def test_restated_blob_and_workspace_sizes(num_feat):
    lib = _lib.load()

    def table(rows):
        return ((rows + 1) * PACK_ENTRY_BYTES + 255) // 256 * 256
    for segs in (1, 2):
        for nb in (0, 1, 3):
            cfg = H.vsr_trunk_cfg(num_feat, nb, segs)
            convs = B.trunk_convs(num_feat, nb, segs)
            assert lib.sr_vsr_trunk_num_params(C.byref(cfg)) == 2 * len(convs) == 2 * (1 + 2 * nb)      # the fp32 header's count, reused
            for co, ci, fs, sg, cp in convs:
                assert lib.sr_conv3x3_cin_pad16(ci, fs, sg) == cp
            assert convs[0][4] == (80, 144)[segs - 1] if num_feat == 64 else convs[0][4] == 16 + segs * num_feat
            want = B.trunk_blob_bytes(num_feat, nb, segs, lib.sr_conv3x3_packed_weight_elems_bf16, lib.sr_conv3x3_packed_bias_floats, table)
            assert lib.sr_rvsr_trunk_packed_bytes_bf16(C.byref(cfg)) == want
            assert lib.sr_rvsr_trunk_workspace_bytes_bf16(C.byref(cfg), 2, 13, 37) == B.trunk_workspace_bytes(num_feat, 2, 13, 37)


def test_profiler_id_167():
    lib = _lib.load()
    assert lib.sr_kernel_name(167).decode() == 'vsr_prop_input_bf16_kernel'
    assert lib.sr_kernel_name(166).decode() == '' and lib.sr_kernel_name(168).decode() == ''
    assert lib.sr_kernel_name(165).decode() == 'bn_lrelu_bwd_kernel' and lib.sr_kernel_name(159).decode() == 'vsr_prop_input_kernel'


def test_prop_input_kernel_uses_no_scratch(tmp_path):
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
                cur = found.setdefault(val, {}) if 'vsr_prop_input_bf16_kernel' in val else None
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count',
                                             'group_segment_fixed_size'):
                cur[key] = int(val)
    assert len(found) == 1, sorted(found)
    md = next(iter(found.values()))
    assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 and md.get('sgpr_spill_count', 0) == 0
    assert md.get('group_segment_fixed_size', 0) == 0                     # no LDS
    assert md['vgpr_count'] <= 72, md                                     # seven waves per SIMD at least


# ---------------------------------------------------------------------------------- set_compute_dtype, network identity
def _checksum(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v.detach().numpy()).tobytes())
    return h.hexdigest()


def test_set_compute_dtype_and_what_it_leaves_alone(golden):
    g = golden('g_ze_basicvsr')
    assert [(k, p.default) for k, p in inspect.signature(BasicVSR.__init__).parameters.items()][1:] == \
        [('num_feat', 64), ('num_block', 15), ('spynet_path', None)]
    assert [(k, p.default) for k, p in inspect.signature(IconVSR.__init__).parameters.items()][1:] == \
        [('num_feat', 64), ('num_block', 15), ('keyframe_stride', 5), ('temporal_padding', 2), ('spynet_path', None), ('edvr_path', None)]
    torch.manual_seed(int(g['init_seed']))
    net = BasicVSR()
    assert net.compute_dtype == 'fp32'
    keys, before = list(net.state_dict()), _checksum(net.state_dict())
    assert net.set_compute_dtype('bf16') is net and net.compute_dtype == 'bf16'
    assert list(net.state_dict()) == keys == [str(k) for k in g['basicvsr_keys']]
    assert _checksum(net.state_dict()) == before == str(g['basicvsr_init_checksum'])
    assert net.set_compute_dtype('fp32') is net and net.compute_dtype == 'fp32'
    for bad in ('fp16', 'BF16', None, 16, 'float32'):
        with pytest.raises(ValueError, match='supported'):
            net.set_compute_dtype(bad)
    assert net.compute_dtype == 'fp32'
    for nf in (8, 24):
        small = BasicVSR(num_feat=nf, num_block=1)
        with pytest.raises(ValueError, match='CB16'):
            small.set_compute_dtype('bf16')
        assert small.compute_dtype == 'fp32' and small.set_compute_dtype('fp32') is small
    gi = golden('g_zf_iconvsr')
    torch.manual_seed(int(gi['init_seed']))
    icon = IconVSR()
    assert icon.set_compute_dtype('bf16') is icon and icon.compute_dtype == 'bf16'
    assert list(icon.state_dict()) == [str(k) for k in gi['iconvsr_keys']] and _checksum(icon.state_dict()) == str(gi['iconvsr_init_checksum'])
    assert BasicVSR(num_feat=16, num_block=0).compute_dtype == 'fp32'     # the class attribute is untouched


def test_bf16_refusals_come_after_the_fp32_ones_and_before_the_device_check():
    net = BasicVSR(num_feat=16, num_block=1).set_compute_dtype('bf16').eval()
    ok = torch.zeros(1, 3, 3, 40, 40)
    flows = torch.zeros(1, 2, 2, 40, 40)
    cases = ((torch.zeros(1, 1, 3, 40, 40), 'reference fails'), (torch.zeros(1, 3, 4, 40, 40), r'\[b, n, 3, h, w\]'),
             (ok.half(), 'supported: fp32'), (ok.bfloat16(), 'supported: fp32'), (torch.zeros(1, 3, 3, 32, 40), 'too small'))
    for mode in (net.eval, net.train):
        mode()
        for x, needle in cases:                                            # every fp32 refusal first, unchanged, in both modes
            for call in (net, net.get_flow):
                with pytest.raises(ValueError, match=needle):
                    call(x)
        with pytest.raises(ValueError, match='flows must be'):
            net.propagate(ok, flows, torch.zeros(1, 2, 2, 40, 41))
        with pytest.raises(ValueError, match='supported: fp32'):
            net.propagate(ok, flows.bfloat16(), flows)
    # train mode with a graph needed: refused on CPU tensors, naming fp32
    net.train()
    for call in (lambda: net(ok), lambda: net.get_flow(ok), lambda: net.propagate(ok, flows, flows)):
        with pytest.raises(NotImplementedError, match="compute_dtype='fp32'"):
            call()
    with torch.no_grad():                                                  # no graph needed: the device check is next
        with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
            net(ok)
    net.eval()
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        net(ok)
    # fp32 keeps its own order: the device check first
    net.set_compute_dtype('fp32').train()
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        net(ok)
    icon = IconVSR(num_block=0).set_compute_dtype('bf16').train()
    with pytest.raises(ValueError, match='at least 5'):
        icon(torch.zeros(1, 4, 3, 40, 40))
    with pytest.raises(ValueError, match='multiples of 4'):
        icon.propagate(torch.zeros(1, 5, 3, 38, 40), torch.zeros(1, 4, 2, 38, 40), torch.zeros(1, 4, 2, 38, 40))
    with pytest.raises(NotImplementedError, match="compute_dtype='fp32'"):
        icon(torch.zeros(1, 5, 3, 40, 40))
    from image_restoration_amd.archs.basicvsr_arch import ConvResidualBlocks
    with pytest.raises(ValueError, match='CB16'):
        ConvResidualBlocks(3 + 24, 24, 1).packed('cpu', bf16=True)


# ------------------------------------------------------------------------------------------------------ option route
def test_option_route_builds_on_the_cpu_and_leaves_the_callers_dict_alone():
    from image_restoration_amd.models import VideoRecurrentModel, build_model
    for net_opt, cls in ((dict(type='BasicVSR', num_feat=16, num_block=1), BasicVSR), (dict(type='IconVSR', num_block=0), IconVSR)):
        for dtype in ('bf16', 'fp32', None):
            given = dict(net_opt) if dtype is None else dict(net_opt, compute_dtype=dtype)
            opt = dict(name='t', model_type='VideoRecurrentModel', scale=4, num_gpu=0, is_train=False, dist=False, rank=0, world_size=1,
                       network_g=dict(given), path=dict(pretrain_network_g=None, strict_load_g=True))
            model = build_model(opt)
            assert isinstance(model, VideoRecurrentModel) and type(model.net_g) is cls
            assert model.net_g.compute_dtype == (dtype or 'fp32')
            assert opt['network_g'] == given                               # the key is taken out of a copy
    bad = dict(name='t', model_type='VideoRecurrentModel', scale=4, num_gpu=0, is_train=False, dist=False, rank=0, world_size=1,
               network_g=dict(type='BasicVSR', num_feat=24, num_block=1, compute_dtype='bf16'), path=dict(pretrain_network_g=None))
    with pytest.raises(ValueError, match='CB16'):
        build_model(bad)
    with pytest.raises(ValueError, match='supported'):
        build_model(dict(bad, network_g=dict(type='BasicVSR', num_feat=16, num_block=1, compute_dtype='fp16')))


def test_shipped_bf16_option_files():
    import yaml
    for name in ('BasicVSR', 'IconVSR'):
        d = os.path.join(ROOT, 'options', 'test', 'BasicVSR')
        opt, plain = yaml.safe_load(open(os.path.join(d, f'test_{name}_REDS_bf16.yml'))), yaml.safe_load(open(os.path.join(d, f'test_{name}_REDS.yml')))
        assert opt['model_type'] == 'VideoRecurrentModel' and opt['network_g'] == dict(plain['network_g'], compute_dtype='bf16')
        assert opt['name'] != plain['name']


# ------------------------------------------------------------------------------------------------- the rounding model
@pytest.fixture(scope='module')
def basicvsr_runs(golden):
    g = golden('g_ze_basicvsr')
    sd = V.basicvsr_weights(int(g['weight_seed']), V.NUM_FEAT, V.NUM_BLOCK, float(g['trunk_scale']))
    runs = {}
    for k, (tag, b, n, h, w) in enumerate(V.CASES):
        x = V.clip_input(int(g['input_seed']) + k, b, n, h, w)
        ff, fb = g[tag + '_flows_forward'], g[tag + '_flows_backward']
        runs[tag] = dict(sd=sd, x=x, ff=ff, fb=fb, y64=V.basicvsr_propagate(sd, x, ff, fb), ym=B.basicvsr_propagate(sd, x, ff, fb))
    return runs


@pytest.mark.parametrize('tag', [c[0] for c in V.CASES])
def test_basicvsr_model_is_exact_without_rounding_and_its_proxy_fits(basicvsr_runs, tag):
    r = basicvsr_runs[tag]
    sd, x, ff, fb, y64, ym = (r[k] for k in ('sd', 'x', 'ff', 'fb', 'y64', 'ym'))
    assert np.array_equal(B.basicvsr_propagate(sd, x, ff, fb, rounding=False), y64)
    bound = B.network_bound(ym, y64)
    d_model, proxy = float(np.abs(ym - y64).max()), float(np.abs(B.basicvsr_propagate(sd, x, ff, fb, acc32=True) - y64).max())
    print(f'{tag}: max|y64| {np.abs(y64).max():.3f}, d_model {d_model:.3e}, proxy {proxy:.3e}, proxy / bound {proxy / bound:.3f}')
    assert 1e-5 < d_model < 1e-3                                            # the roundings are visible and small
    assert proxy / bound <= PROXY_LIMIT


def test_basicvsr_negative_controls_leave_the_bound(basicvsr_runs):
    tag = V.CASES[0][0]                                                     # three frames: both branches warp twice
    r = basicvsr_runs[tag]
    sd, x, ff, fb, y64, ym = (r[k] for k in ('sd', 'x', 'ff', 'fb', 'y64', 'ym'))
    bound = B.network_bound(ym, y64)
    wrong = {'zeroed flows': B.basicvsr_propagate(sd, x, np.zeros_like(ff), np.zeros_like(fb)),
             'swapped flow planes': B.basicvsr_propagate(sd, x, ff[:, :, ::-1], fb[:, :, ::-1]),
             'zeroed backward features': B.basicvsr_propagate(sd, x, ff, fb, zero_backward=True)}
    for what, y in wrong.items():
        d = float(np.abs(y - y64).max())
        print(f'{tag} {what}: {d:.3e} = {d / bound:.1f} x the bound')
        assert d > bound, what


def test_iconvsr_model_is_exact_without_rounding_and_its_proxies_fit(golden):
    g = golden('g_zf_iconvsr')
    tag, b, n, h, w, stride = V.ICON_CASE
    keys, shapes = [str(k) for k in g['iconvsr_keys']], [tuple(int(d) for d in str(s).split(',')) for s in g['iconvsr_shapes']]
    ek = [(k[5:], s) for k, s in zip(keys, shapes) if k.startswith('edvr.')]
    edvr = V.extractor_weights(int(g['edvr_seed']), [k for k, _ in ek], [s for _, s in ek])
    sd = V.iconvsr_weights(int(g['weight_seed']), V.NUM_FEAT, V.NUM_BLOCK, float(g['trunk_scale']))
    x = V.pad_spatial(V.clip_input(int(g['input_seed']), b, n, h, w))
    idx = V.keyframes(n, stride)
    ff, fb = g[tag + '_flows_forward'], g[tag + '_flows_backward']
    kf64 = V.keyframe_features(edvr, x, idx)
    kf_off = B.keyframe_features(edvr, x, idx, rounding=False)
    assert all(np.array_equal(kf_off[i], kf64[i]) for i in idx)
    y64 = V.iconvsr_propagate(sd, x, ff, fb, kf64)
    assert np.array_equal(B.iconvsr_propagate(sd, x, ff, fb, kf64, rounding=False), y64)
    kfm, kfa = B.keyframe_features(edvr, x, idx), B.keyframe_features(edvr, x, idx, acc32=True)
    # whole: the shape the GPU test uses
    ym, ya = B.iconvsr_propagate(sd, x, ff, fb, kfm), B.iconvsr_propagate(sd, x, ff, fb, kfa, acc32=True)
    whole = float(np.abs(ya - y64).max()) / B.network_bound(ym, y64)
    print(f'{tag} whole: d_model {np.abs(ym - y64).max():.3e}, proxy / bound {whole:.3f}')
    assert whole <= PROXY_LIMIT
    # split: propagate on float64 keyframe features
    ym, ya = B.iconvsr_propagate(sd, x, ff, fb, kf64), B.iconvsr_propagate(sd, x, ff, fb, kf64, acc32=True)
    split = float(np.abs(ya - y64).max()) / B.network_bound(ym, y64)
    print(f'{tag} propagate on float64 keyframe features: d_model {np.abs(ym - y64).max():.3e}, proxy / bound {split:.3f}')
    assert split <= PROXY_LIMIT
