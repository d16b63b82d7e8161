"""The recurrent backward of BasicVSR on the host side (no GPU): the ABI of include/sr_hip_vsr_bwd.h (declared, bound, exported,
in no other header, each entry point mapped to the GPU test that pins it, one hip_ops wrapper per stream-ordered entry point),
every refusal of the C functions before any launch (dummy pointers, null stream), the size queries against the header's formulas,
the profiler name at id 178, the compiled resources of the new kernel, the router's rule for shared parameters, the
``set_autograd`` contracts that need no device, and the yardstick of the whole backward: tests/vsr_grad_restate.py against
tests/vsr_restate.py, against its own forced mode and against the reference's own gradients
(tests/golden/g_zh_basicvsr_grad.npz, tools/make_golden_basicvsr_grad.py)."""
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
from image_restoration_amd.archs import hip_generator
from image_restoration_amd.archs.basicvsr_arch import BasicVSR, IconVSR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as FR  # noqa: E402
import vsr_grad_restate as G  # noqa: E402
import vsr_restate as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_vsr_bwd.h')
SR_EINVAL, SR_ENOSPACE = -1, -3
_OPS = 'tests/test_vsr_bwd_ops_gpu.py::'
PINNED = {
    'sr_vsr_prop_input_bwd_f32': _OPS + 'test_prop_input_bwd_matches_float64',
    'sr_vsr_trunk_keep_bytes': _OPS + 'test_trunk_keep_is_the_trunk_bit_for_bit_and_keeps_the_activations',
    'sr_vsr_trunk_keep_f32': _OPS + 'test_trunk_keep_is_the_trunk_bit_for_bit_and_keeps_the_activations',
    'sr_vsr_trunk_packed_dgrad_bytes': _OPS + 'test_trunk_bwd_matches_the_forced_restatement',
    'sr_vsr_trunk_pack_dgrad_f32': _OPS + 'test_trunk_bwd_matches_the_forced_restatement',
    'sr_vsr_trunk_bwd_workspace_bytes': _OPS + 'test_trunk_bwd_matches_the_forced_restatement',
    'sr_vsr_trunk_bwd_f32': _OPS + 'test_trunk_bwd_matches_the_forced_restatement',
}
PACK_ENTRY_BYTES = 120     # sizeof(sr::PackEntry), as tests/test_vsr_host.py


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_every_declared_entry_point_is_bound_exported_and_pinned():
    declared = set(re.findall(r'\b(?:int|size_t)\s+(sr_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(_lib.VSR_BWD_SIGNATURES) == set(PINNED) and len(declared) == 7
    others = set()
    for name in dir(_lib):
        if name.endswith('SIGNATURES') and name != 'VSR_BWD_SIGNATURES':
            others |= set(getattr(_lib, name))
    assert others and not declared & others
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'sr_hip_vsr_bwd.h':
            text = open(os.path.join(ROOT, 'include', other)).read()
            assert not any(s in text for s in declared), other
    for s, target in PINNED.items():
        path, _, func = target.partition('::')
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith('test_')}
        assert func in tests, (s, target)
    # every stream-ordered entry point has one hip_ops wrapper that goes through launch
    src = open(os.path.join(ROOT, 'image_restoration_amd', 'hip_ops.py')).read()
    wrappers = {'sr_vsr_prop_input_bwd_f32': 'vsr_prop_input_bwd', 'sr_vsr_trunk_keep_f32': 'vsr_trunk_keep',
                'sr_vsr_trunk_pack_dgrad_f32': 'vsr_trunk_pack_dgrad', 'sr_vsr_trunk_bwd_f32': 'vsr_trunk_bwd'}
    ordered = {s for s, (res, args) in _lib.VSR_BWD_SIGNATURES.items() if res is C.c_int and args and args[-1] is C.c_void_p}
    assert ordered == set(wrappers)
    for s in ordered:
        assert src.count(f"_launch_arg('{s}'") == 1 and hasattr(H, wrappers[s]), s
    assert C.sizeof(_lib.VsrPropBwdDesc) == 96 and C.sizeof(_lib.VsrTrunkBwdDesc) == 128
    assert 'sr_hip_vsr_bwd.h' in open(os.path.join(ROOT, 'image_restoration_amd', 'csrc', 'Makefile')).read()
    # the forward header is untouched: it still declares its seven functions and none of these
    fwd = open(os.path.join(ROOT, 'include', 'sr_hip_vsr.h')).read()
    assert len(set(re.findall(r'\b(?:int|size_t)\s+(sr_[a-z0-9_]+)\s*\(', fwd))) == 7 and 'bwd' not in fwd and 'keep' not in fwd


def test_profiler_id_178():
    lib = _lib.load()
    assert lib.sr_kernel_name(178).decode() == 'vsr_prop_input_bwd_kernel'
    assert lib.sr_kernel_name(177).decode() == '' and lib.sr_kernel_name(179).decode() == ''
    assert lib.sr_kernel_name(176).decode() == 'resize_bilinear_adjoint_kernel'


# -------------------------------------------------------------------------------------------------------- size queries
@pytest.mark.parametrize('num_feat', [64, 24])
def test_size_queries_follow_the_header(num_feat):
    lib = _lib.load()
    up = lambda v: (v + 255) // 256 * 256   # noqa: E731
    for segs in (1, 2):
        for nb in (0, 1, 3):
            cfg = H.vsr_trunk_cfg(num_feat, nb, segs)
            for n, h, w in ((1, 1, 1), (2, 13, 37), (3, 33, 40)):
                one = up(4 * n * num_feat * h * w)
                assert lib.sr_vsr_trunk_keep_bytes(C.byref(cfg), n, h, w) == 2 * nb * one
                assert lib.sr_vsr_trunk_bwd_workspace_bytes(C.byref(cfg), n, h, w) == 3 * one + up(lib.sr_conv3x3_wgrad_slab_bytes(n, h, w))
            # the data-gradient images: the convs' roles swapped, each rounded up to 256 bytes, then the pack table of one row each
            convs = V.trunk_convs(num_feat, nb, segs)
            images = sum(up(4 * lib.sr_conv3x3_packed_weight_floats(cp, co)) for co, ci, cp in convs)
            table = ((len(convs) + 1) * PACK_ENTRY_BYTES + 255) // 256 * 256
            assert lib.sr_vsr_trunk_packed_dgrad_bytes(C.byref(cfg)) == images + table
    for bad in (H.vsr_trunk_cfg(20, 1, 1), H.vsr_trunk_cfg(64, -1, 1), H.vsr_trunk_cfg(64, 1, 3)):
        assert lib.sr_vsr_trunk_keep_bytes(C.byref(bad), 1, 8, 8) == 0 and lib.sr_vsr_trunk_packed_dgrad_bytes(C.byref(bad)) == 0
        assert lib.sr_vsr_trunk_bwd_workspace_bytes(C.byref(bad), 1, 8, 8) == 0
    cfg = H.vsr_trunk_cfg(64, 1, 1)
    assert lib.sr_vsr_trunk_keep_bytes(C.byref(cfg), 0, 8, 8) == 0 and lib.sr_vsr_trunk_bwd_workspace_bytes(C.byref(cfg), 1, 0, 8) == 0


# ------------------------------------------------------------------------------------------------------------ refusals
def _prop_desc(h=4, w=5, fb=2, n=1):
    d = _lib.VsrPropBwdDesc()
    win = 8 * fb * h * w
    d.g, d.prev, d.flow, d.dprev, d.dflow = 256, 4096, 8192, 12288, 16384
    d.g_img_stride = d.prev_img_stride = d.dprev_img_stride = win
    d.flow_img_stride = d.dflow_img_stride = 2 * h * w
    d.n, d.h, d.w, d.fb = n, h, w, fb
    return d


def _trunk_desc(cfg, n=1, h=8, w=8):
    lib = _lib.load()
    nparams = lib.sr_vsr_trunk_num_params(C.byref(cfg))
    d = _lib.VsrTrunkBwdDesc()
    d.packed_dgrad, d.in_, d.out, d.stack, d.dout, d.din, d.workspace = 256, 4096, 8192, 12288, 16384, 20480, 24576
    d.in_img_stride = d.din_img_stride = (8 + cfg.cin_segs * cfg.num_feat) * h * w
    d.out_img_stride = d.dout_img_stride = cfg.num_feat * h * w
    d.stack_bytes = lib.sr_vsr_trunk_keep_bytes(C.byref(cfg), n, h, w)
    d.workspace_bytes = lib.sr_vsr_trunk_bwd_workspace_bytes(C.byref(cfg), n, h, w)
    d.dparams = (C.c_void_p * nparams)(*[1024 + 64 * i for i in range(nparams)])
    d.n, d.h, d.w = n, h, w
    return d


def test_c_abi_refuses_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.sr_last_error().decode()   # noqa: E731
    # the step-input adjoint
    assert lib.sr_vsr_prop_input_bwd_f32(None, None) == SR_EINVAL and 'null descriptor' in err()
    for field, value, needle in (('g', None, 'null'), ('prev', None, 'null'), ('flow', None, 'null'), ('fb', 0, 'bad shape'),
                                 ('n', 0, 'bad shape'), ('n', 65536, 'bad shape'), ('h', -1, 'bad shape'), ('fb', 65535, 'bad shape'),
                                 ('g', 260, '16-byte aligned'), ('dprev', 12292, '16-byte aligned'), ('flow', 8193, '4-byte aligned'),
                                 ('dflow', 16386, '4-byte aligned'), ('prev_img_stride', 8 * 2 * 20 + 2, 'multiples of 4'),
                                 ('dprev', 256, 'must not be a source'), ('dprev', 4096, 'must not be a source'),
                                 ('dflow', 8192, 'must not be a source')):
        d = _prop_desc()
        setattr(d, field, value)
        assert lib.sr_vsr_prop_input_bwd_f32(C.byref(d), None) == SR_EINVAL and needle in err(), (field, err())
    d = _prop_desc()
    d.dprev = d.dflow = None
    assert lib.sr_vsr_prop_input_bwd_f32(C.byref(d), None) == SR_EINVAL and 'nothing to compute' in err()
    for field in ('g_img_stride', 'prev_img_stride', 'dprev_img_stride', 'flow_img_stride', 'dflow_img_stride'):
        d = _prop_desc(n=2)
        setattr(d, field, getattr(d, field) - 4)
        assert lib.sr_vsr_prop_input_bwd_f32(C.byref(d), None) == SR_EINVAL and 'smaller than the image' in err(), field
    d = _prop_desc(h=16384, w=16384)
    assert lib.sr_vsr_prop_input_bwd_f32(C.byref(d), None) == SR_EINVAL and 'too large' in err()
    # the keeping forward: the forward's checks, and its own word for the stack
    cfg, P, Q = H.vsr_trunk_cfg(64, 1, 1), 256, 4096
    assert lib.sr_vsr_trunk_keep_f32(C.byref(cfg), None, P, 0, Q, 0, 1, 8, 8, None, 0, None) == SR_EINVAL and 'sr_vsr_trunk_keep_f32' in err()
    assert lib.sr_vsr_trunk_keep_f32(C.byref(cfg), P, P, 0, Q, 0, 1, 0, 8, None, 0, None) == SR_EINVAL and 'bad shape' in err()
    assert lib.sr_vsr_trunk_keep_f32(C.byref(cfg), P, P, 0, Q, 0, 1, 8, 8, 8192, 16, None) == SR_ENOSPACE
    assert 'stack of 16 bytes' in err() and 'sr_vsr_trunk_keep_bytes' in err()
    bad = H.vsr_trunk_cfg(20, 1, 1)
    assert lib.sr_vsr_trunk_keep_f32(C.byref(bad), P, P, 0, Q, 0, 1, 8, 8, None, 0, None) == SR_EINVAL and 'bad config' in err()
    # the data-gradient pack
    assert lib.sr_vsr_trunk_pack_dgrad_f32(C.byref(bad), None, Q, None) == SR_EINVAL and 'bad config' in err()
    assert lib.sr_vsr_trunk_pack_dgrad_f32(C.byref(cfg), None, Q, None) == SR_EINVAL and 'null' in err()
    ptrs = (C.c_void_p * 6)(*[1024] * 6)
    assert lib.sr_vsr_trunk_pack_dgrad_f32(C.byref(cfg), ptrs, Q + 16, None) == SR_EINVAL and '256-byte aligned' in err()
    ptrs[2] = None
    assert lib.sr_vsr_trunk_pack_dgrad_f32(C.byref(cfg), ptrs, Q, None) == SR_EINVAL and 'null weight 1' in err()
    # the trunk's backward
    assert lib.sr_vsr_trunk_bwd_f32(C.byref(cfg), None, None) == SR_EINVAL and 'null descriptor' in err()
    assert lib.sr_vsr_trunk_bwd_f32(C.byref(bad), C.byref(_trunk_desc(cfg)), None) == SR_EINVAL and 'bad config' in err()
    for field, value, needle in (('packed_dgrad', None, 'null'), ('in_', None, 'null'), ('dout', None, 'null'), ('workspace', None, 'null'),
                                 ('n', 0, 'bad shape'), ('w', 0, 'bad shape'), ('accumulate', 2, 'accumulate must be'),
                                 ('packed_dgrad', 272, '256-byte aligned'), ('stack', 12304, '256-byte aligned'),
                                 ('dout', 16388, '16-byte aligned'), ('din', 20484, '16-byte aligned'),
                                 ('in_img_stride', 72 * 64 + 2, 'multiples of 4'), ('din', 4096, 'din must not be'),
                                 ('din', 16384, 'din must not be')):
        d = _trunk_desc(cfg)
        setattr(d, field, value)
        assert lib.sr_vsr_trunk_bwd_f32(C.byref(cfg), C.byref(d), None) == SR_EINVAL and needle in err(), (field, err())
    for field in ('in_img_stride', 'dout_img_stride', 'din_img_stride'):
        d = _trunk_desc(cfg, n=2)
        setattr(d, field, getattr(d, field) - 4)
        assert lib.sr_vsr_trunk_bwd_f32(C.byref(cfg), C.byref(d), None) == SR_EINVAL and 'smaller than the image' in err(), field
    d = _trunk_desc(cfg)
    d.dparams = None
    assert lib.sr_vsr_trunk_bwd_f32(C.byref(cfg), C.byref(d), None) == SR_EINVAL and 'null' in err()
    d = _trunk_desc(cfg)
    d.dparams[2] = None                                            # conv1's weight target gone, its bias target left
    assert lib.sr_vsr_trunk_bwd_f32(C.byref(cfg), C.byref(d), None) == SR_EINVAL and 'bias target of conv 1 needs its weight target' in err()
    d = _trunk_desc(cfg)
    d.dparams[1] = 1026
    assert lib.sr_vsr_trunk_bwd_f32(C.byref(cfg), C.byref(d), None) == SR_EINVAL and '4-byte aligned' in err()
    d = _trunk_desc(cfg)
    d.workspace_bytes -= 1
    assert lib.sr_vsr_trunk_bwd_f32(C.byref(cfg), C.byref(d), None) == SR_ENOSPACE and 'sr_vsr_trunk_bwd_workspace_bytes' in err()
    d = _trunk_desc(cfg)
    d.stack_bytes -= 1
    assert lib.sr_vsr_trunk_bwd_f32(C.byref(cfg), C.byref(d), None) == SR_ENOSPACE and 'sr_vsr_trunk_keep_bytes' in err()
    d = _trunk_desc(cfg)
    d.stack = None
    assert lib.sr_vsr_trunk_bwd_f32(C.byref(cfg), C.byref(d), None) == SR_ENOSPACE
    cfg0 = H.vsr_trunk_cfg(64, 0, 1)                              # no block: the mask is `out` itself
    d = _trunk_desc(cfg0)
    d.out = None
    assert lib.sr_vsr_trunk_bwd_f32(C.byref(cfg0), C.byref(d), None) == SR_EINVAL and 'needs out' in err()
    d = _trunk_desc(cfg, h=4096, w=4096)
    assert lib.sr_vsr_trunk_bwd_f32(C.byref(cfg), C.byref(d), None) == SR_EINVAL and 'too large' in err()


def test_wrappers_refuse_before_the_device():
    flow = torch.zeros(1, 2, 4, 5)
    with pytest.raises(ValueError, match='CB8 windows of one shape'):
        H.vsr_prop_input_bwd(None, None, flow)
    cfg = H.vsr_trunk_cfg(64, 1, 1)
    with pytest.raises(ValueError, match='windows do not fit'):
        H.vsr_trunk_keep(cfg, None, None, None)
    with pytest.raises(ValueError, match='3 targets, the config has 6'):
        H.vsr_trunk_bwd(cfg, None, None, None, None, None, None, [None] * 3)
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        H.vsr_trunk_pack_dgrad(cfg, [torch.zeros(1)] * 6)


# --------------------------------------------------------------------------------------------------- compiled kernel
def test_prop_input_bwd_kernel_uses_no_scratch(tmp_path):
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
                cur = found.setdefault(val, {}) if 'vsr_prop_input_bwd_kernel' in val else None
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count',
                                             'group_segment_fixed_size'):
                cur[key] = int(val)
    assert len(found) == 1, sorted(found)
    md = next(iter(found.values()))
    assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 and md.get('sgpr_spill_count', 0) == 0
    assert md.get('group_segment_fixed_size', 0) == 0 and md['vgpr_count'] <= 64, md      # no LDS; eight waves per SIMD


# ------------------------------------------------------------------------------------------------- the generator base
def test_router_adds_later_launches_of_a_shared_parameter(monkeypatch):
    calls = []

    class T:
        def __init__(self, p):
            self.p = p

        def data_ptr(self):
            return self.p
    monkeypatch.setattr(H, 'conv3x3_wgrad', lambda *a, **k: calls.append(k['out']) or (None if k['out'] else (T(11), T(12))))

    class Net:
        _grad_sink = None
    conv = torch.nn.Conv2d(8, 8, 3, 1, 1)
    router = hip_generator.GradRouter(Net(), [conv.weight, conv.bias], [True, True])
    for _ in range(3):
        router.wgrad(conv, 'src', 'd')
    assert calls == [None, (11, 12), (11, 12)]                      # stored once, then added into the first call's tensors
    assert [g.p for g in router.grads] == [11, 12]
    # whole-call targets: fresh tensors for the first call, the same pointers with accumulate for the later ones
    router = hip_generator.GradRouter(Net(), [conv.weight, conv.bias], [True, False])
    first, again = router.shared_targets([conv.weight, conv.bias]), router.shared_targets([conv.weight, conv.bias])
    assert first[1] is False and again[1] is True and first[0] == again[0] and first[0][1] is None
    assert first[0][0] == router.grads[0].data_ptr() and router.grads[1] is None
    # an arena: always its pointers, always added
    class Sink:
        grad_ptrs = [64, 128]
    net = Net()
    net._grad_sink = Sink()
    router = hip_generator.GradRouter(net, [conv.weight, conv.bias], [True, True])
    assert router.shared_targets([conv.weight, conv.bias]) == ((64, 128), True) == router.shared_targets([conv.weight, conv.bias])


# ------------------------------------------------------------------------------------------- the set_autograd contract
class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the device: reaches the checks behind ``is_cuda`` without a GPU."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    is_cuda = property(lambda self: True)


def test_set_autograd_contract_on_cpu_tensors():
    net = BasicVSR(num_feat=8, num_block=1)
    assert net._autograd is False and net.spynet._autograd is False
    x = torch.zeros(1, 3, 3, 40, 40)
    flows = torch.zeros(1, 2, 2, 40, 40)
    net.train()
    for call in (lambda: net(_FakeCuda(x)), lambda: net.get_flow(_FakeCuda(x)), lambda: net.propagate(_FakeCuda(x), _FakeCuda(flows), _FakeCuda(flows))):
        with pytest.raises(NotImplementedError, match='follow-up') as e:        # default off: today's refusal, type and word kept
            call()
        assert 'set_autograd(True)' in str(e.value)
    assert net.set_autograd() is net and net._autograd is True and net.spynet._autograd is True
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):               # CPU tensors are still refused first
        net(x)
    with pytest.raises(NotImplementedError, match='frames are data'):
        net(_FakeCuda(x.clone().requires_grad_()))
    with pytest.raises(NotImplementedError, match='frames are data'):
        net.propagate(_FakeCuda(x.clone().requires_grad_()), _FakeCuda(flows), _FakeCuda(flows))
    with pytest.raises(ValueError, match='too small'):                          # the shape refusals come first in either mode
        net(torch.zeros(1, 3, 3, 32, 40))
    assert net.set_autograd(False) is net and net._autograd is False and net.spynet._autograd is False
    with pytest.raises(NotImplementedError, match='follow-up'):
        net(_FakeCuda(x))
    # bf16 stays refused with its present message, before the device check, whatever the switch says
    net16 = BasicVSR(num_feat=16, num_block=1).set_compute_dtype('bf16').set_autograd(True).train()
    with pytest.raises(NotImplementedError, match="compute_dtype='fp32'"):
        net16(x)
    # IconVSR cannot be switched on, and its refusal keeps its word
    icon = IconVSR(num_feat=64, num_block=1)
    with pytest.raises(NotImplementedError, match='follow-up'):
        icon.set_autograd(True)
    assert icon.set_autograd(False) is icon and icon._autograd is False
    icon.train()
    with pytest.raises(NotImplementedError, match='follow-up'):
        icon(_FakeCuda(torch.zeros(1, 5, 3, 40, 40)))


# -------------------------------------------------------------------------------------------------- the yardstick
def test_restatement_is_propagate_and_forcing_it_with_itself_changes_nothing(golden):
    fix = golden('g_ze_basicvsr')
    tag = G.CASES[0][0]
    _, b, n, h, w, nf, nb = G.case(tag)
    sd, x, ff, fb = G.case_data(fix, tag)
    assert (nf, nb) == (V.NUM_FEAT, V.NUM_BLOCK) and FR.weights_checksum(sd) == FR.weights_checksum(
        V.basicvsr_weights(int(fix['weight_seed']), V.NUM_FEAT, V.NUM_BLOCK, float(fix['trunk_scale'])))
    g = G.grad_output(tag)
    rec = {}
    mine, y = G.gradients(sd, x, ff, fb, g, nb, record=rec)
    want = V.basicvsr_propagate(sd, x, ff, fb)
    assert np.abs(y.numpy() - want).max() <= 1e-12
    assert len(mine) == 32 and list(mine)[-2:] == list(G.FLOW_KEYS) and all(np.abs(v).max() > 0 for v in mine.values())
    assert len(rec['cells']) == 2 * (n - 1) and len(rec['masks']) == 3 * n
    assert all(len(m) == (4 if k[0] == 'head' else 1 + nb) for k, m in rec['masks'].items())
    forced, _ = G.gradients(sd, x, ff, fb, g, nb, forced=rec)
    assert max(G.rel_l2(forced, mine).values()) <= 1e-10
    # forcing one flipped mask moves the gradients: the forced mode does select the piece
    rec['masks'][('forward', 1)][1] = ~rec['masks'][('forward', 1)][1]
    flipped, _ = G.gradients(sd, x, ff, fb, g, nb, forced=rec)
    assert max(G.rel_l2(flipped, mine).values()) > 1e-3


def test_restatement_reproduces_the_reference_gradients(golden):
    """tests/golden/g_zh_basicvsr_grad.npz (tools/make_golden_basicvsr_grad.py): the reference BasicVSR's own float64 autograd
    gradients of the first case, per tensor the L2 norm and a strided sample, stored as float64."""
    fix, f = golden('g_ze_basicvsr'), golden('g_zh_basicvsr_grad')
    tag = str(f['tag'])
    _, b, n, h, w, nf, nb = G.case(tag)
    sd, x, ff, fb = G.case_data(fix, tag)
    assert int(f['weight_seed']) == int(fix['weight_seed']) and int(f['input_seed']) == int(fix['input_seed'])
    assert str(f['weight_checksum']) == FR.weights_checksum(sd) and float(f['fp32_dist']) <= 1e-5
    grads, _ = G.gradients(sd, x, ff, fb, G.grad_output(tag, int(f['grad_seed'])), nb)
    assert [str(k) for k in f['names']] == list(grads)
    for k, v in grads.items():
        norm = float(f[f'{k}/norm'])
        assert norm > 0 and abs(np.linalg.norm(v) - norm) <= 1e-9 * norm, k
        assert np.abs(v.reshape(-1)[G.sample_index(v.shape)] - f[f'{k}/vals']).max() <= 1e-9 * norm, k
