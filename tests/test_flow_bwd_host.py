"""SpyNet's backward kernels on the host side (no GPU): the ABI of include/sr_hip_flow_bwd.h (declared, bound, exported, in no
other header, each entry point mapped to the GPU test that pins it, one hip_ops wrapper per stream-ordered entry point), every
refusal of the C functions before any launch (dummy pointers, null stream), the size queries against the header's plan, the
profiler names at ids 169-176, the compiled resources read from the code object, the routing of 7x7 convs in the generator
base (``packed(conv, mode=1)``, ``GradRouter.wgrad``), SpyNet's ``set_autograd`` contract, and the yardstick of the whole
backward: tests/spynet_grad_restate.py against the numpy restatement, plain torch autograd and the reference's own gradients
(tests/golden/g_zg_spynet_grad.npz, tools/make_golden_spynet_grad.py)."""
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
from image_restoration_amd.archs.spynet_arch import SpyNet

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as R  # noqa: E402
import spynet_grad_restate as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_flow_bwd.h')
SR_EINVAL = -1
_OPS = 'tests/test_flow_bwd_ops_gpu.py::'
PINNED = {
    'sr_conv7x7_dgrad_instance': _OPS + 'test_conv7x7_dgrad_matches_float64',
    'sr_conv7x7_dgrad_packed_floats': _OPS + 'test_conv7x7_dgrad_matches_float64',
    'sr_conv7x7_dgrad_pack_f32': _OPS + 'test_conv7x7_dgrad_matches_float64',
    'sr_conv7x7_dgrad_f32': _OPS + 'test_conv7x7_dgrad_matches_float64',
    'sr_conv7x7_wgrad_slab_bytes': _OPS + 'test_conv7x7_wgrad_matches_float64',
    'sr_conv7x7_wgrad_f32': _OPS + 'test_conv7x7_wgrad_matches_float64',
    'sr_spynet_level_input_bwd_f32': _OPS + 'test_level_input_bwd_is_warp_bwd_then_float64_upT',
    'sr_resize_bilinear_adjoint_f32': _OPS + 'test_resize_adjoint_is_the_transpose',
}
NAMES = ['conv7x7_dgrad_f32_kernelILi1ELi4EE', 'conv7x7_dgrad_f32_kernelILi2ELi2EE', 'conv7x7_dgrad_pack_kernel',
         'conv7x7_wgrad_f32_kernel', 'conv7x7_wgrad_reduce_kernel', 'spynet_level_dup_kernel', 'spynet_level_upT_kernel',
         'resize_bilinear_adjoint_kernel']
KERNELS = ('conv7x7_dgrad_f32_kernel', 'conv7x7_dgrad_pack_kernel', 'conv7x7_wgrad_f32_kernel', 'conv7x7_wgrad_reduce_kernel',
           'spynet_level_dup_kernel', 'spynet_level_upT_kernel', 'resize_bilinear_adjoint_kernel')
PAIRS = ((8, 32), (32, 64), (64, 32), (32, 16), (16, 2))
UNSERVED = ((8, 16), (16, 32), (3, 2), (64, 64), (8, 2), (32, 32))


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_every_declared_entry_point_is_bound_exported_and_pinned():
    declared = set(re.findall(r'\b(?:int|size_t)\s+(sr_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(_lib.FLOW_BWD_SIGNATURES) == set(PINNED) and len(declared) == 8
    others = set()
    for name in dir(_lib):
        if name.endswith('SIGNATURES') and name != 'FLOW_BWD_SIGNATURES':
            others |= set(getattr(_lib, name))
    assert others and not declared & others
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'sr_hip_flow_bwd.h':
            text = open(os.path.join(ROOT, 'include', other)).read()
            assert not any(s in text for s in declared), other
    for s, target in PINNED.items():
        path, _, func = target.partition('::')
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith('test_')}
        assert func in tests, (s, target)
    # every stream-ordered entry point has one hip_ops wrapper that goes through launch
    src = open(os.path.join(ROOT, 'image_restoration_amd', 'hip_ops.py')).read()
    wrappers = {'sr_conv7x7_dgrad_f32': 'conv7x7_dgrad', 'sr_conv7x7_wgrad_f32': 'conv7x7_wgrad',
                'sr_spynet_level_input_bwd_f32': 'spynet_level_input_bwd', 'sr_resize_bilinear_adjoint_f32': 'resize_bilinear_adjoint',
                'sr_conv7x7_dgrad_pack_f32': 'PackedConv7x7'}
    ordered = {s for s, (res, args) in _lib.FLOW_BWD_SIGNATURES.items()
               if res is C.c_int and args and args[-1] is C.c_void_p and s != 'sr_conv7x7_dgrad_instance'}
    assert ordered == set(wrappers)
    for s in ordered:
        assert src.count(f"_launch_arg('{s}'") == 1 and hasattr(H, wrappers[s]), s
    assert C.sizeof(_lib.Conv7x7DgradDesc) == 80 and C.sizeof(_lib.Conv7x7WgradDesc) == 96
    assert 'sr_hip_flow_bwd.h' in open(os.path.join(ROOT, 'image_restoration_amd', 'csrc', 'Makefile')).read()
    # the forward header is untouched: it still declares its nine functions and none of these
    fwd = open(os.path.join(ROOT, 'include', 'sr_hip_flow.h')).read()
    assert len(set(re.findall(r'\b(?:int|size_t)\s+(sr_[a-z0-9_]+)\s*\(', fwd))) == 9 and 'dgrad' not in fwd and 'wgrad' not in fwd


def test_profiler_ids_resolve_from_169():
    lib = _lib.load()
    assert [lib.sr_kernel_name(i).decode() for i in range(169, 177)] == NAMES
    for i in (158, 160, 166, 168, 177):
        assert lib.sr_kernel_name(i).decode() == '', i
    assert lib.sr_kernel_name(167).decode() == 'vsr_prop_input_bf16_kernel'


# ------------------------------------------------------------------------------------------------ dispatch and sizes
def _plan(n, h, w, cout, cin):
    cdiv = lambda a, b: -(-a // b)   # noqa: E731
    ct, it, tx = cdiv(cout, 32), cdiv(cin, 32), cdiv(w, 32)
    chunks = min(max(cdiv(1024, n * tx * ct * it * 7), 1), cdiv(h, 4))
    rw = 4 * cdiv(cdiv(h, chunks), 4)
    return 4 * n * cdiv(h, rw) * tx * (ct * it * 49 * 1024 + ct * 64)


def test_dispatch_and_size_queries():
    lib = _lib.load()
    assert [lib.sr_conv7x7_dgrad_instance(co, ci) for ci, co in PAIRS] == [0, 0, 1, 0, 0]
    reachable = {lib.sr_conv7x7_dgrad_instance(co, ci) for ci in range(0, 72) for co in range(0, 72)} - {-1}
    assert reachable == {0, 1}
    served = {(ci, co) for ci in range(0, 72) for co in range(0, 72) if lib.sr_conv7x7_dgrad_instance(co, ci) >= 0}
    assert served == set(PAIRS) == set(H.CONV7X7_SHAPES)
    # image: [dx group][dy block][49][COT][32][8] + one zero per padded dx channel
    want = {(8, 32): 4 * 49 * 256 + 32, (32, 64): 8 * 49 * 256 + 32, (64, 32): 4 * 49 * 2 * 256 + 64, (32, 16): 2 * 49 * 256 + 32,
            (16, 2): 49 * 256 + 32}
    for ci, co in PAIRS:
        assert lib.sr_conv7x7_dgrad_packed_floats(co, ci) == want[(ci, co)]
        for n, h, w in ((1, 1, 1), (2, 19, 37), (8, 64, 64), (8, 180, 320), (4, 320, 70)):
            assert lib.sr_conv7x7_wgrad_slab_bytes(n, h, w, co, ci) == _plan(n, h, w, co, ci), (ci, co, n, h, w)
    for ci, co in UNSERVED:
        assert lib.sr_conv7x7_dgrad_instance(co, ci) == -1 and lib.sr_conv7x7_dgrad_packed_floats(co, ci) == 0
        assert lib.sr_conv7x7_wgrad_slab_bytes(1, 8, 8, co, ci) == 0
    assert lib.sr_conv7x7_wgrad_slab_bytes(0, 8, 8, 32, 8) == 0
    # 8 pairs of 180x320, the benchmark's shape: 160 strips, 31 MB for a one-tile pair — the shared 9-tap buffers are not involved
    assert lib.sr_conv7x7_wgrad_slab_bytes(8, 180, 320, 32, 8) == 4 * 160 * (49 * 1024 + 64)


# ------------------------------------------------------------------------------------------------------------ refusals
def _dgrad_desc(cin=8, cout=32, h=8, w=8, dy=256, dx=4096, packed=8192):
    d = _lib.Conv7x7DgradDesc()
    d.dy, d.dy_img_stride, d.cin, d.cout, d.n, d.h, d.w = dy, (cout + 7) // 8 * 8 * h * w, cin, cout, 1, h, w
    d.packed, d.dx, d.dx_img_stride = packed, dx, cin * h * w
    return d


def _wgrad_desc(cin=8, cout=32, h=8, w=8):
    d = _lib.Conv7x7WgradDesc()
    d.x, d.x_img_stride, d.dy, d.dy_img_stride = 256, cin * h * w, 4096, (cout + 7) // 8 * 8 * h * w
    d.cin, d.cout, d.n, d.h, d.w, d.scale = cin, cout, 1, h, w, 1.0
    d.dweight, d.dbias, d.slab = 8192, 12288, 16384
    d.slab_bytes = _lib.load().sr_conv7x7_wgrad_slab_bytes(1, h, w, cout, cin)
    return d


def test_c_abi_refuses_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.sr_last_error().decode()   # noqa: E731
    pairs = 'supported: (8, 32), (32, 64), (64, 32), (32, 16), (16, 2)'
    for ci, co in UNSERVED:
        assert lib.sr_conv7x7_dgrad_f32(C.byref(_dgrad_desc(ci, co)), None) == SR_EINVAL
        assert f'(cin, cout) = ({ci}, {co}) is not supported; {pairs}' in err()
        assert lib.sr_conv7x7_dgrad_pack_f32(256, co, ci, 4096, None) == SR_EINVAL and pairs in err()
        assert lib.sr_conv7x7_wgrad_f32(C.byref(_wgrad_desc(ci, co)), None) == SR_EINVAL and pairs in err()
    assert lib.sr_conv7x7_dgrad_f32(None, None) == SR_EINVAL and lib.sr_conv7x7_wgrad_f32(None, None) == SR_EINVAL
    assert lib.sr_conv7x7_dgrad_pack_f32(256, 32, 8, 4100, None) == SR_EINVAL and '16-byte aligned' in err()
    assert lib.sr_conv7x7_dgrad_pack_f32(None, 32, 8, 4096, None) == SR_EINVAL and 'null' in err()
    # data gradient: null, misaligned, strides, overlap, size
    for field, value, needle in (('dx', None, 'null'), ('dy', 260, '16-byte aligned'), ('mask', 260, '16-byte aligned'),
                                 ('dy_img_stride', 32 * 64 + 2, 'multiples of 4'), ('dx_img_stride', 8 * 64 - 4, 'smaller than the image'),
                                 ('n', 0, 'bad shape'), ('h', -1, 'bad shape'), ('dx', 256, 'must not be dy')):
        d = _dgrad_desc()
        setattr(d, field, value)
        assert lib.sr_conv7x7_dgrad_f32(C.byref(d), None) == SR_EINVAL and needle in err(), (field, err())
    d = _dgrad_desc(h=8192, w=8192)
    assert lib.sr_conv7x7_dgrad_f32(C.byref(d), None) == SR_EINVAL and 'too large' in err()
    d = _dgrad_desc()
    d.mask, d.mask_img_stride = 4096 * 4, 8
    assert lib.sr_conv7x7_dgrad_f32(C.byref(d), None) == SR_EINVAL and 'smaller than the image' in err()
    # weight gradient: null, misaligned, a slab that is too small, accumulate, strides
    for field, value, needle in (('slab', None, 'null'), ('dweight', None, 'null'), ('x', 260, '16-byte aligned'), ('slab', 16388, '16-byte aligned'),
                                 ('dweight', 8194, '4-byte aligned'), ('dbias', 12289, '4-byte aligned'), ('accumulate', 2, 'accumulate must be'),
                                 ('x_img_stride', 8 * 64 + 1, 'multiples of 4'), ('dy_img_stride', 32 * 64 - 4, 'smaller than the image'),
                                 ('n', 0, 'bad shape'), ('w', 0, 'bad shape')):
        d = _wgrad_desc()
        setattr(d, field, value)
        assert lib.sr_conv7x7_wgrad_f32(C.byref(d), None) == SR_EINVAL and needle in err(), (field, err())
    d = _wgrad_desc()
    d.slab_bytes -= 1
    assert lib.sr_conv7x7_wgrad_f32(C.byref(d), None) == SR_EINVAL
    assert f'slab of {d.slab_bytes} bytes, sr_conv7x7_wgrad_slab_bytes asks for {d.slab_bytes + 1}' in err()
    # level adjoint: odd H or W, null, misaligned, aliasing
    P, Q, S = 256, 4096, 8192
    assert lib.sr_spynet_level_input_bwd_f32(P, P, P, P, Q, S, 1, 7, 8, None) == SR_EINVAL and 'must be even' in err()
    assert lib.sr_spynet_level_input_bwd_f32(P, P, P, P, Q, S, 1, 8, 7, None) == SR_EINVAL and 'must be even' in err()
    assert lib.sr_spynet_level_input_bwd_f32(P, P, P, None, Q, S, 1, 8, 8, None) == SR_EINVAL and 'null' in err()
    assert lib.sr_spynet_level_input_bwd_f32(P, P + 4, P, P, Q, S, 1, 8, 8, None) == SR_EINVAL and '16-byte aligned' in err()
    assert lib.sr_spynet_level_input_bwd_f32(P, P, P, P, Q + 4, S, 1, 8, 8, None) == SR_EINVAL and '8-byte aligned' in err()
    assert lib.sr_spynet_level_input_bwd_f32(P, P, P, Q, S, Q, 1, 8, 8, None) == SR_EINVAL and 'must not be an input' in err()
    assert lib.sr_spynet_level_input_bwd_f32(P, P, P, P, Q, S, 0, 8, 8, None) == SR_EINVAL and 'bad shape' in err()
    # resize adjoint
    assert lib.sr_resize_bilinear_adjoint_f32(P, None, 1, 4, 4, 8, 8, None) == SR_EINVAL and 'null' in err()
    assert lib.sr_resize_bilinear_adjoint_f32(P, Q, 0, 4, 4, 8, 8, None) == SR_EINVAL and 'bad shape' in err()
    assert lib.sr_resize_bilinear_adjoint_f32(P, Q, 65536, 4, 4, 8, 8, None) == SR_EINVAL and '65535' in err()
    assert lib.sr_resize_bilinear_adjoint_f32(P, Q, 1, 4, 0, 8, 8, None) == SR_EINVAL
    assert lib.sr_resize_bilinear_adjoint_f32(P, P, 1, 4, 4, 8, 8, None) == SR_EINVAL and 'must not be dy' in err()


def test_wrappers_refuse_cpu_tensors():
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        H.PackedConv7x7(torch.zeros(32, 8, 7, 7), None, mode=1)
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        H.resize_bilinear_adjoint(torch.zeros(1, 2, 8, 8), (4, 4))
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        H.spynet_level_input_bwd(torch.zeros(1, 3, 4, 4), None, None, None)


# ------------------------------------------------------------------------------------------------- the generator base
def test_generator_base_routes_7x7_convs(monkeypatch):
    calls = []
    monkeypatch.setattr(H, 'conv7x7_wgrad', lambda *a, **k: calls.append(('7x7', a[2:], k)) or ('dw7', 'db7'))
    monkeypatch.setattr(H, 'conv3x3_wgrad', lambda *a, **k: calls.append(('3x3', a[2:], k)) or ('dw3', 'db3'))
    monkeypatch.setattr(H, 'convd_wgrad', lambda *a, **k: calls.append(('kxk', a[2:], k)) or ('dwk', 'dbk'))

    class Net:
        _grad_sink = None
    convs = [torch.nn.Conv2d(8, 32, 7, 1, 3), torch.nn.Conv2d(8, 8, 3, 1, 1), torch.nn.Conv2d(8, 8, 1), torch.nn.Conv2d(8, 8, 3, 1, 2, 2)]
    params = [p for c in convs for p in (c.weight, c.bias)]
    router = hip_generator.GradRouter(Net(), params, [True] * 8)
    router.wgrad(convs[0], 'src', 'd', scale=0.5)
    router.wgrad(convs[1], 'src', 'd')
    router.wgrad(convs[2], 'src', 'd')
    router.wgrad(convs[3], 'src', 'd', dilation=2)
    assert [c[0] for c in calls] == ['7x7', '3x3', 'kxk', 'kxk']                 # every other kernel size keeps its route
    assert calls[0][1] == (32, 8) and calls[0][2] == dict(scale=0.5, out=None)
    assert router.grads == ['dw7', 'db7', 'dw3', 'db3', 'dwk', 'dbk', 'dwk', 'dbk']
    # packed(conv, mode=1) builds the 7x7 data-gradient image without a bias
    built = []

    class Fake:
        def __init__(self, w, b, mode=0):
            built.append((tuple(w.shape), b is None, mode))
    monkeypatch.setattr(H, 'PackedConv7x7', Fake)
    gen = hip_generator.HipGenerator()
    assert isinstance(gen.packed(convs[0], mode=1), Fake) and isinstance(gen.packed(convs[0], mode=0), Fake)
    assert built == [((32, 8, 7, 7), True, 1), ((32, 8, 7, 7), False, 0)]
    assert gen.packed(convs[0], mode=1) is gen.packed(convs[0], mode=1) and len(built) == 2     # cached per mode


# ------------------------------------------------------------------------------------------- the set_autograd contract
def test_set_autograd_contract_on_cpu_tensors():
    net = SpyNet()
    assert net._autograd is False and net.set_autograd() is net and net._autograd is True
    assert net.set_autograd(False) is net and net._autograd is False
    x = torch.zeros(1, 3, 64, 64)
    net.train()
    with pytest.raises(NotImplementedError, match='backward') as e:             # default off: today's refusal, type and word kept
        net(_FakeCuda(x), _FakeCuda(x))
    assert 'set_autograd(True)' in str(e.value)
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):               # CPU tensors are refused before anything else
        net(x, x)
    net.set_autograd(True)
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        net(x, x)
    with pytest.raises(NotImplementedError, match='image gradients'):
        net(_FakeCuda(x.clone().requires_grad_()), _FakeCuda(x))
    net.eval()
    with pytest.raises(ValueError, match='same size'):                           # the shape refusals come first in either mode
        net(x, torch.zeros(1, 3, 64, 96))


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the device: reaches the checks behind ``is_cuda`` without a GPU."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)

    is_cuda = property(lambda self: True)


# -------------------------------------------------------------------------------------------------- the yardstick
def test_restatement_is_spynet_and_its_gradients_are_autograd():
    """With its own masks and cells the restatement is SpyNet: its forward agrees with the numpy restatement to 1e-10, and its
    gradients with plain torch autograd (F.relu, F.grid_sample, F.interpolate) of the same network."""
    sd = R.spynet_weights(G.WEIGHT_SEED, G.LAST_SCALE)
    for tag in ('70x90',):                                   # the case with the pre-resize and the rescale; the others: the fixture
        ref, supp = G.case_inputs(tag)
        g = G.grad_output(tag)
        rec = []
        mine, flow = G.gradients(G.spynet, G.parameters(), ref, supp, g, record=rec)
        want, _ = R.spynet(sd, ref, supp)
        assert np.abs(flow.numpy() - want).max() <= 1e-10, tag
        theirs, flow_p = G.gradients(G.plain, G.parameters(), ref, supp, g)
        assert float((flow - flow_p).abs().max()) <= 1e-10 and max(G.rel_l2(mine, theirs).values()) <= 1e-10, tag
        assert len(mine) == 60 and len(rec) == 6 and all(len(r['masks']) == 4 for r in rec)
        # forcing it with what it recorded changes nothing; forcing one flipped mask element does
        again, _ = G.gradients(G.spynet, G.parameters(), ref, supp, g, forced=rec)
        assert max(G.rel_l2(again, mine).values()) == 0.0
    rec[5]['masks'][3] = ~rec[5]['masks'][3]
    flipped, _ = G.gradients(G.spynet, G.parameters(), ref, supp, g, forced=rec)
    assert max(G.rel_l2(flipped, mine).values()) > 1e-3


def test_restatement_reproduces_the_reference_gradients(golden):
    """tests/golden/g_zg_spynet_grad.npz (tools/make_golden_spynet_grad.py): the reference's own float64 autograd gradients,
    reduced per parameter tensor to norm, sum and 16 entries; the biases in full."""
    f = golden('g_zg_spynet_grad')
    assert int(f['weight_seed']) == G.WEIGHT_SEED and float(f['last_scale']) == G.LAST_SCALE
    assert str(f['weight_checksum']) == R.weights_checksum(R.spynet_weights(G.WEIGHT_SEED, G.LAST_SCALE))
    for tag, n, h, w in (c for c in G.CASES if c[0] in G.GRAD_CASES):
        assert float(f[f'{tag}_fp32_dist']) <= 2e-5                      # the tool's cases cross no kink
        ref, supp = R.spynet_inputs(int(f[f'{tag}_input_seed']), n, h, w)
        grads, _ = G.gradients(G.spynet, G.parameters(), ref, supp, G.grad_output(tag))
        for k, v in grads.items():
            norm = float(f[f'{tag}/{k}/norm'])
            assert abs(np.linalg.norm(v) - norm) <= 1e-9 * norm and abs(v.sum() - float(f[f'{tag}/{k}/sum'])) <= 1e-9 * norm, (tag, k)
            assert np.abs(v.reshape(-1)[f[f'{tag}/{k}/idx']] - f[f'{tag}/{k}/vals']).max() <= 1e-9 * norm, (tag, k)
            if k.endswith('bias'):
                assert np.abs(v - f[f'{tag}/{k}/full']).max() <= 1e-9 * norm, (tag, k)


# --------------------------------------------------------------------------------------------------- compiled kernels
def test_kernels_use_no_scratch_and_fit_their_launch_bounds(tmp_path):
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
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count',
                                             'group_segment_fixed_size'):
                cur[key] = int(val)
    for k in KERNELS:
        assert any(k in name for name in found), (k, sorted(found))
    assert len(found) == 8, sorted(found)            # two data-gradient instances and one of each other kernel
    for name, md in found.items():
        assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 \
            and md.get('sgpr_spill_count', 0) == 0, (name, md)
        # __launch_bounds__(256, 2): two workgroups of four waves per CU, 256 registers a wave; the data gradient keeps the
        # forward body's 128.  The weight gradient holds 7 x 16 accumulators and the 37 + 16 row registers.
        limit = 128 if 'dgrad_f32_kernel' in name else 256
        assert md['vgpr_count'] <= limit, (name, md)
    wg = next(md for name, md in found.items() if 'conv7x7_wgrad_f32_kernel' in name)
    assert 112 < wg['vgpr_count']
    assert {m.groups() for m in (re.search(r'conv7x7_dgrad_f32_kernelILi(\d)ELi(\d)EE', n) for n in found) if m} == {('1', '4'), ('2', '2')}
