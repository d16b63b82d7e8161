"""PCDAlignment(64, 8) and the public DCN surface on the GPU against the float64 restatement (tests/dcn_restate.py).

Weights come from a seeded numpy.random.default_rng (as utils/synth does): plain conv and DCN weights N(0, 1.4^2 / fan_in), the
conv_offset weights N(0, 1 / fan_in), biases N(0, 0.1^2).  The scales were picked on the CPU so that, on the float64
restatement, mean|offset| at level 1 lies in [0.5, 3] pixels and at least 1 % of the level-3 samples fall outside the image
(asserted below): the deformable convs really sample away from their taps, and across the border.

Tolerance: the whole-network margin of tests/test_gfpgan_gpu.py.  The same restatement run in float32 on the CPU is measured
against the float64 one per tensor as relative L2 (a gradient through floor jumps at integer coordinates, and a handful of
samples may change cell between precisions); the HIP path must stay within 10x that distance.  Both distances are printed.
"""
import logging
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from image_restoration_amd import hip_ops as H
from image_restoration_amd.archs.arch_util import DCNv2Pack
from image_restoration_amd.archs.edvr_arch import PCDAlignment
from image_restoration_amd.ops.dcn import modulated_deform_conv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SIZES = ((16, 24), (8, 12), (4, 6))


@pytest.fixture(scope='module')
def cuda():
    return torch.device('cuda:0')


def _state_dict(seed):
    rng = np.random.default_rng(seed)
    sd = {}
    for k, v in PCDAlignment(64, 8).state_dict().items():
        if k.endswith('weight'):
            sc = (1.0 if 'conv_offset' in k else 1.4) / np.sqrt(v.shape[1] * 9)
            sd[k] = torch.from_numpy((rng.standard_normal(tuple(v.shape)) * sc).astype(np.float32))
        else:
            sd[k] = torch.from_numpy((rng.standard_normal(tuple(v.shape)) * 0.1).astype(np.float32))
    return sd


def _pyramids(seed):
    rng = np.random.default_rng(seed)
    return [[torch.from_numpy(rng.standard_normal((2, 64, h, w)).astype(np.float32)) for h, w in SIZES] for _ in range(2)]


def _restated(sd, nbr, ref, gy, dtype, offsets_out=None):
    """Output and every gradient (inputs, then parameters in state_dict order) of the restatement in ``dtype`` on the CPU."""
    p = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in sd.items()}
    a = [t.detach().clone().to(dtype).requires_grad_(True) for t in nbr]
    b = [t.detach().clone().to(dtype).requires_grad_(True) for t in ref]
    out = R.pcd_alignment(p, a, b, 8, offsets_out)
    grads = torch.autograd.grad(out, a + b + list(p.values()), gy.to(dtype))
    return out.detach(), [g.detach() for g in grads]


@pytest.fixture(scope='module')
def pcd(cuda):
    sd, (nbr, ref) = _state_dict(0), _pyramids(1)
    gy = torch.from_numpy(np.random.default_rng(2).standard_normal((2, 64, 16, 24)).astype(np.float32))
    offs = {}
    out64, g64 = _restated(sd, nbr, ref, gy, torch.float64, offs)
    out32, g32 = _restated(sd, nbr, ref, gy, torch.float32)
    net = PCDAlignment(64, 8).to(cuda)
    net.load_state_dict(sd, strict=True)
    net.eval()   # eval mode without torch.no_grad(): the offset warning's reduction and host sync are skipped, gradients flow
    a = [t.detach().to(cuda).requires_grad_(True) for t in nbr]
    b = [t.detach().to(cuda).requires_grad_(True) for t in ref]
    out = net(a, b)
    out.backward(gy.to(cuda))
    torch.cuda.synchronize()
    grads = [t.grad for t in a + b] + [p.grad for p in net.parameters()]
    names = [f'nbr_l{i}' for i in (1, 2, 3)] + [f'ref_l{i}' for i in (1, 2, 3)] + [k for k, _ in net.named_parameters()]
    return dict(sd=sd, offs=offs, out=(out.detach().cpu(), out32, out64), grads=(grads, g32, g64), names=names, net=net)


def test_the_case_really_deforms(pcd):
    offs = pcd['offs']
    mean_l1 = float(offs['l1'].abs().mean())
    h_im, w_im = R.positions(offs['l3'], 8)
    outside = float(((h_im <= -1) | (w_im <= -1) | (h_im >= 4) | (w_im >= 6)).double().mean())
    print(f'mean|offset| at level 1 = {mean_l1:.3f} px, level-3 samples outside the image: {100 * outside:.1f} %')
    assert 0.5 <= mean_l1 <= 3.0 and outside >= 0.01
    assert all(float(v.abs().max()) > 0 for k, v in pcd['sd'].items() if 'conv_offset' in k)


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm().clamp_min(1e-300))


def test_forward_and_every_gradient_within_10x_the_float32_distance(pcd):
    hip, f32, f64 = pcd['out']
    d32, dhip = _rel(f32, f64), _rel(hip, f64)
    print(f'output: float32 restatement {d32:.3e}, HIP {dhip:.3e} (relative L2 to float64)')
    bad = [] if dhip <= 10 * d32 else [('output', dhip, d32)]
    ghip, g32, g64 = pcd['grads']
    assert len(ghip) == len(g64) == len(pcd['names']) == 6 + 40
    for name, gh, a32, a64 in zip(pcd['names'], ghip, g32, g64):
        assert gh is not None and tuple(gh.shape) == tuple(a64.shape), name
        d32, dhip = _rel(a32, a64), _rel(gh.cpu(), a64)
        print(f'grad {name}: float32 restatement {d32:.3e}, HIP {dhip:.3e}')
        if not dhip <= 10 * d32:
            bad.append((name, dhip, d32))
    assert not bad, bad


def test_state_dict_round_trip(pcd, cuda):
    net = pcd['net']
    sd = net.state_dict()
    assert list(sd) == list(pcd['sd']) and all(torch.equal(sd[k].cpu(), pcd['sd'][k]) for k in sd)
    net2 = PCDAlignment(64, 8).to(cuda)
    net2.load_state_dict(sd, strict=True)
    nbr, ref = _pyramids(1)
    with torch.no_grad():
        y = net2.eval()([t.to(cuda) for t in nbr], [t.to(cuda) for t in ref])
    assert torch.equal(y.cpu(), pcd['out'][0])   # every launch of the forward is bit-reproducible


def test_fresh_dcnv2pack_is_half_the_conv_plus_bias(cuda):
    """conv_offset is zero after construction: offsets 0, mask sigmoid(0) = 1/2, so the output is 0.5 * conv3x3(x) + bias.
    Against sr_conv3x3_f32 on the same weights, within the forward bound of tests/test_dcn_ops_gpu.py (k = 2 * 9 * cin + 8 + 2
    + 4 for the DCN, 2 * 9 * cin + 8 for the conv) on A = conv(|x|, |w|) / 2 + |b|."""
    torch.manual_seed(3)
    m = DCNv2Pack(64, 64, 3, padding=1, deformable_groups=8).to(cuda)
    with torch.no_grad():
        m.bias.copy_(torch.randn(64) * 0.5)
    x, feat = torch.randn(2, 64, 13, 35, device=cuda), torch.randn(2, 64, 13, 35, device=cuda)
    with torch.no_grad():
        y = m(x, feat).cpu().double()
        conv = H.cb8_to_nchw(H.conv3x3(H.nchw_to_cb8(x), H.PackedConv(m.weight.detach(), None)), 64).cpu().double()
    b64 = m.bias.detach().cpu().double().view(1, -1, 1, 1)
    Aabs = 0.5 * F.conv2d(x.cpu().double().abs(), m.weight.detach().cpu().double().abs(), padding=1) + b64.abs()
    k = (2 * 9 * 64 + 14) + (2 * 9 * 64 + 8)
    err = (y - (0.5 * conv + b64)).abs()
    print(f'fresh DCNv2Pack vs 0.5 conv + bias: max err / bound = {float((err / (k * EPS * Aabs)).max()):.3f}')
    assert bool((err <= k * EPS * Aabs + EPS * y.abs()).all())


def test_functional_on_nchw_tensors(cuda):
    rng = np.random.default_rng(5)
    n, cin, cout, dg, h, w = 2, 32, 24, 2, 9, 37
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))  # noqa: E731
    x, off, msk = f(n, cin, h, w), f(n, 18 * dg, h, w) * 2, torch.from_numpy(rng.uniform(0, 1, (n, 9 * dg, h, w)).astype(np.float32))
    wt, b = f(cout, cin, 3, 3) / np.sqrt(cin * 9), f(cout)
    xs = x.to(cuda).requires_grad_(True)
    y = modulated_deform_conv(xs, off.to(cuda), msk.to(cuda), wt.to(cuda), b.to(cuda), 1, 1, 1, 1, dg)
    assert tuple(y.shape) == (n, cout, h, w)
    y.sum().backward()
    ref = R.modulated_deform_conv(x.double(), off.double(), msk.double(), wt.double(), b.double(), dg)
    ref32 = R.modulated_deform_conv(x, off, msk, wt, b, dg)
    d32, dhip = _rel(ref32, ref), _rel(y.detach().cpu(), ref)
    print(f'functional: float32 restatement {d32:.3e}, HIP {dhip:.3e}')
    assert dhip <= 10 * d32 and xs.grad is not None and bool(torch.isfinite(xs.grad).all())


def test_offset_warning_fires_in_training_mode_only(cuda, caplog):
    m = DCNv2Pack(64, 64, 3, padding=1, deformable_groups=8).to(cuda)
    with torch.no_grad():
        m.conv_offset.bias[:144] = 60.0   # offsets of 60 pixels
    x = torch.randn(2, 64, 8, 12, device=cuda)
    with caplog.at_level(logging.WARNING, logger='basicsr'):
        m.eval()
        m(x, x)
        assert not [r for r in caplog.records if 'Offset abs mean' in r.getMessage()]
        m.train()
        m(x, x)
    msgs = [r.getMessage() for r in caplog.records if 'Offset abs mean' in r.getMessage()]
    assert len(msgs) == 1 and 'larger than 50' in msgs[0] and '60' in msgs[0]
