"""TSAFusion, PredeblurModule and EDVR on the GPU.

TSAFusion(16, 3, 1) and PredeblurModule(3, 16, hr_in=True) are checked against a golden recorded from the reference's own
classes in float64 on the CPU (tests/golden/g_z_edvr.npz, tools/make_edvr_golden.py): weights, input, output gradient, the
output and every gradient (the gradients are stored rounded to float32: 2^-25 relative per element).

The whole EDVR has no reference golden: the reference's deformable convolution exists only as a CUDA extension, so its EDVR
cannot run where the goldens are recorded (DESIGN.md §23 says the same of PCDAlignment).  Its yardstick is the float64
restatement tests/edvr_restate.py (plain torch.nn.functional, PCD from tests/dcn_restate.py), which aligns the frames one by one
as the reference does.  Weights come from numpy.random.default_rng with the scales of tests/test_pcd_gpu.py (plain conv and
DCN weights N(0, 1.4^2 / fan_in), conv_offset weights N(0, 1 / fan_in), biases N(0, 0.1^2)); it is asserted on the float64 side
that with them the PCD offsets really deform.

Tolerance: the rule and margin of tests/test_pcd_gpu.py and tests/test_gfpgan_gpu.py.  The same restatement run in float32 on
the CPU is measured against float64 per tensor as relative L2; the HIP modules must stay within 10x that distance.  Both
distances are printed.
"""
import os
import sys

import numpy as np
import pytest
import torch

from image_restoration_amd.archs.edvr_arch import EDVR, PredeblurModule, TSAFusion

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_restate as R  # noqa: E402
import edvr_restate as E  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g_z_edvr.npz')


@pytest.fixture(scope='module')
def cuda():
    return torch.device('cuda:0')


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _compare(names, hip, f32, f64):
    bad = []
    for name, h, a32, a64 in zip(names, hip, f32, f64):
        assert h is not None and tuple(h.shape) == tuple(a64.shape), name
        d32, dhip = _rel(a32, a64), _rel(h.cpu(), a64)
        print(f'{name}: float32 restatement {d32:.3e}, HIP {dhip:.3e} (relative L2 to float64)')
        if not dhip <= 10 * d32:
            bad.append((name, dhip, d32))
    assert not bad, bad


# ------------------------------------------------------------------------------------- the two modules against the golden
def _golden(tag):
    g = np.load(GOLDEN)
    keys = [str(k) for k in g[f'{tag}_keys']]
    sd = {k: torch.from_numpy(g[f'{tag}_w{i}']) for i, k in enumerate(keys)}
    grads = [torch.from_numpy(g[f'{tag}_dx'])] + [torch.from_numpy(g[f'{tag}_dw{i}']) for i in range(len(keys))]
    return sd, torch.from_numpy(g[f'{tag}_x']), torch.from_numpy(g[f'{tag}_gy']), torch.from_numpy(g[f'{tag}_y']), grads


def _restated32(fn, sd, x, gy):
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    y = fn(p, xr)
    return y.detach(), [t.detach() for t in torch.autograd.grad(y, [xr] + list(p.values()), gy)]


def _module_case(cuda, tag, module, fn):
    sd, x, gy, y64, g64 = _golden(tag)
    y32, g32 = _restated32(fn, sd, x, gy)
    module = module.to(cuda).eval()
    module.load_state_dict(sd, strict=True)
    xd = x.to(cuda).requires_grad_(True)
    y = module(xd)
    y.backward(gy.to(cuda))
    torch.cuda.synchronize()
    names = ['output', 'grad input'] + [f'grad {k}' for k in sd]
    _compare(names, [y.detach(), xd.grad] + [p.grad for p in module.parameters()], [y32] + g32, [y64] + g64)


def test_tsa_fusion_against_the_reference_golden(cuda):
    _module_case(cuda, 'tsa', TSAFusion(16, 3, 1), lambda p, x: E.tsa_fusion(p, x, 1))


def test_predeblur_against_the_reference_golden(cuda):
    _module_case(cuda, 'pre', PredeblurModule(3, 16, hr_in=True), lambda p, x: E.predeblur(p, x, True))


# ---------------------------------------------------------------------------------------------------------- whole EDVR
BASE = dict(num_feat=64, deformable_groups=8, num_extract_block=1, num_reconstruct_block=1)
CONFIGS = {
    # (constructor arguments, input shape, input scale, seed of the weights; the input's seed is one more)
    'tsa3': (dict(num_frame=3), (1, 3, 3, 16, 24), 1.0, 20),
    'notsa5': (dict(num_frame=5, with_tsa=False), (1, 5, 3, 8, 12), 1.0, 20),
    # N(0, 0.1^2) frames: the pre-deblur module's 17 convs at gain 1.4 amplify N(0, 1) frames until the offsets reach 14 to 29
    # pixels on the 8 x 12 level-1 map and 93 % or more of the samples fall outside the image.  Even then the biases alone
    # give 2.5 to 5.7 pixels; of the seeds 20 .. 29, 22 is the one whose float64 level-1 offsets lie in the band of
    # tests/test_pcd_gpu.py, [0.5, 3] pixels (2.53, 41 % of the samples outside).  All of this was measured with the float64
    # restatement on the CPU, none of it on the code under test.
    'predeblur_hr3': (dict(with_predeblur=True, hr_in=True, num_frame=3), (1, 3, 3, 32, 48), 0.1, 22),
}


def _state_dict(net, seed):
    rng = np.random.default_rng(seed)
    sd = {}
    for k, v in net.state_dict().items():
        if k.endswith('weight'):
            sc = (1.0 if 'conv_offset' in k else 1.4) / np.sqrt(v.shape[1] * v.shape[2] * v.shape[3])
            sd[k] = torch.from_numpy((rng.standard_normal(tuple(v.shape)) * sc).astype(np.float32))
        else:
            sd[k] = torch.from_numpy((rng.standard_normal(tuple(v.shape)) * 0.1).astype(np.float32))
    return sd


def _restated(sd, x, gy, kw, dtype, offsets_out=None):
    p = {k: v.clone().to(dtype).requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().to(dtype).requires_grad_(True)
    y = E.edvr(p, xr, num_frame=kw['num_frame'], num_extract_block=1, num_reconstruct_block=1, hr_in=kw.get('hr_in', False),
               with_predeblur=kw.get('with_predeblur', False), with_tsa=kw.get('with_tsa', True), offsets_out=offsets_out)
    return y.detach(), [t.detach() for t in torch.autograd.grad(y, [xr] + list(p.values()), gy.to(dtype))]


@pytest.fixture(scope='module', params=list(CONFIGS))
def edvr(request, cuda):
    kw, shape, in_scale, seed = CONFIGS[request.param]
    net = EDVR(**BASE, **kw)
    sd = _state_dict(net, seed)
    rng = np.random.default_rng(seed + 1)
    x = torch.from_numpy((rng.standard_normal(shape) * in_scale).astype(np.float32))
    offs = {}
    scale = 1 if kw.get('hr_in') else 4
    out_shape = (shape[0], 3, scale * shape[3], scale * shape[4])
    gy = torch.from_numpy(rng.standard_normal(tuple(out_shape)).astype(np.float32))
    y64, g64 = _restated(sd, x, gy, kw, torch.float64, offs)
    y32, g32 = _restated(sd, x, gy, kw, torch.float32)
    net = net.to(cuda).eval()   # eval mode without no_grad: no offset warning (a host sync), gradients flow
    net.load_state_dict(sd, strict=True)
    xd = x.to(cuda).requires_grad_(True)
    y = net(xd)
    y.backward(gy.to(cuda))
    torch.cuda.synchronize()
    return dict(name=request.param, kw=kw, sd=sd, x=x, offs=offs, net=net, y=y.detach(),
                hip=[y.detach(), xd.grad] + [p.grad for p in net.parameters()], f32=[y32] + g32, f64=[y64] + g64)


def test_edvr_output_shape_and_the_case_really_deforms(edvr):
    kw, x = edvr['kw'], edvr['x']
    b, t, c, h, w = x.shape
    s = 1 if kw.get('hr_in') else 4
    assert tuple(edvr['y'].shape) == (b, 3, s * h, s * w)
    off = edvr['offs']['l1']          # the first frame's level-1 offsets of the float64 restatement
    mean_l1 = float(off.abs().mean())
    h_im, w_im = R.positions(off, 8)
    outside = float(((h_im <= -1) | (w_im <= -1) | (h_im >= off.shape[2]) | (w_im >= off.shape[3])).double().mean())
    print(f'{edvr["name"]}: mean|offset| at level 1 = {mean_l1:.3f} px, samples outside the image: {100 * outside:.1f} %')
    # the band of tests/test_pcd_gpu.py: the samples leave their taps, and some cross the border
    assert 0.5 <= mean_l1 <= 3.0 and outside >= 0.01
    assert all(float(v.abs().max()) > 0 for k, v in edvr['sd'].items() if 'conv_offset' in k)


def test_edvr_forward_and_every_gradient_within_10x_the_float32_distance(edvr):
    names = ['output', 'grad input'] + [f'grad {k}' for k in edvr['sd']]
    assert len(edvr['hip']) == len(edvr['f64']) == len(names)
    _compare(names, edvr['hip'], edvr['f32'], edvr['f64'])


def test_edvr_state_dict_round_trip_and_reproducibility(edvr, cuda):
    net, kw = edvr['net'], edvr['kw']
    sd = net.state_dict()
    assert list(sd) == list(edvr['sd']) and all(torch.equal(sd[k].cpu(), edvr['sd'][k]) for k in sd)
    net2 = EDVR(**BASE, **kw).to(cuda).eval()
    net2.load_state_dict(sd, strict=True)
    xd = edvr['x'].to(cuda)
    with torch.no_grad():
        y_ng = net2(xd)
    assert not y_ng.requires_grad and y_ng.grad_fn is None
    assert torch.equal(y_ng, edvr['y']), 'a no_grad forward of a reloaded network is the grad-mode forward bit for bit'
    y2 = net2(xd)
    assert torch.equal(y2.detach(), edvr['y']), 'two forwards are bit-identical'


def test_batched_alignment_equals_the_per_frame_loop(edvr, cuda):
    """One PCD call on the b * t batch against t separate forward_cb8 calls, on pyramids of the network's own sizes."""
    net, kw = edvr['net'], edvr['kw']
    b, t = 2, kw['num_frame']
    h, w = 8, 12
    rng = np.random.default_rng(22)
    feats = [torch.from_numpy(rng.standard_normal((b * t, 8, hh, ww, 8)).astype(np.float32)).to(cuda)
             for hh, ww in ((h, w), (h // 2, w // 2), (h // 4, w // 4))]
    c = net.center_frame_idx
    with torch.no_grad():
        batched = net.align_cb8(feats, b, t).view(b, t, 8, h, w, 8)
        v = [f.view(b, t, *f.shape[1:]) for f in feats]
        ref = [f[:, c].contiguous() for f in v]
        for i in range(t):
            one = net.pcd_align.forward_cb8([f[:, i].contiguous() for f in v], ref)
            assert torch.equal(one, batched[:, i]), f'frame {i}'
