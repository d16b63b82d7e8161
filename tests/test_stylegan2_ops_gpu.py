"""The kernels of include/sr_hip_stylegan2.h and their autograd Functions against float64 (tests/upfirdn_restate.py) and against
IEEE arithmetic in numpy, on every instance the dispatch can take.

Bounds are derived, not fitted.  EPS = 2^-24; A is the same operation on absolute values, in float64.

upfirdn2d   |y - y64| <= (T + 1) EPS A, T = ceil(kh / up_y) * ceil(kw / up_x): the kernel adds at most T products with one fmaf
            each into a zero accumulator, so its error is at most gamma_T A = T EPS A / (1 - T EPS) <= (T + 1) EPS A for
            T (T + 1) <= 2^24 (T <= 256 here).  Where A = 0 the output must be exactly zero.
            Integer sources in [-8, 8] with the [1, 3, 3, 1] x [1, 3, 3, 1] / 64 filter (times 4 at up 2) make every product and
            partial sum a multiple of 1/64 below 2^11: fp32 is exact and the result must equal float64 bit for bit.
activation  forward, forward with ref and the backward's gx are one add and two multiplies, each rounded once: they must equal
            the same operations in numpy float32 bit for bit.  gbias sums gx through the tree of the header; a term passes
            through at most d = (4 v - 1) + 6 + 3 + (ceil(P / 64) - 1) + 6 additions, P = N ceil(inner / (1024 v)), v = 4 or 1, so
            |gbias - sum64(gx)| <= d EPS sum |gx| with d the larger of the two v (the device's own gx, read back, is summed in
            float64, so gx's roundings do not enter).
autograd    d upfirdn2d / dx is the same kernel with the factors swapped: the bound above with T' = ceil(kh / down_y) *
            ceil(kw / down_x) on the gradient call of |g|, |k|.  The activation's gx against float64 carries its two multiplies,
            (1 + EPS)^2 - 1 <= 3 EPS relative; its gbias (d + 3) EPS sum |gx64|.  The float64 side uses the fp32 values of the
            slope and the scale.  x + b rounds to zero only when it is zero, so fp32 and float64 take the same branch.
R1 probe    out = act(A x + b) with A = upfirdn2d(k, pad (1, 1)); L = sum(v out); gx = A^T z, gb = S z with z = D v,
            D = diag(scale * (1 or slope)) and S the per-channel sum; P = sum gx^2 + sum gb^2; dP/dv = D (A (2 gx) + 2 gb[c]).
            Counting the device's roundings to first order (T = 16 taps, d as above, |A| = A for the non-negative filter):
              z 2 EPS |z|;  gx (T + 1) EPS A^T|z| + A^T|dz| <= (T + 3) EPS A^T|z|;  gb (d + 2) EPS S|z|;  2 gx, 2 gb exact;
              w = A (2 gx): (T + 1) EPS W + 2 A |dgx| <= (2 T + 4) EPS W with W = 2 A A^T |z|;
              D (w + 2 gb): one add, two multiplies: 3 EPS (W + G) + |dw| + 2 |dgb| with G = 2 S^T S |z|
            so |dP/dv - float64| <= D ((2 T + 7) W + (2 d + 7) G) EPS; the test uses 2 T + 8 and 2 d + 8 to cover the second-order
            terms.  x, k and b sit on dyadic grids (x in 2^-3 Z, k in 2^-6 Z, b an odd multiple of 2^-10), so every pre-activation
            is exact in fp32 and an odd multiple of 2^-10: its sign cannot differ between fp32 and float64.  Both facts are
            asserted on the float64 side.

Operands of the upfirdn2d cases lie in buffers whose slack holds a NaN bit pattern that must come back unchanged; outputs start
as that pattern and must be finite everywhere.  Negative controls show that each bound notices the mistake it is there for."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from image_restoration_amd import hip_ops as H
from image_restoration_amd.ops.fused_act import FusedLeakyReLU, fused_leaky_relu
from image_restoration_amd.ops.upfirdn2d import UpFirDn2d, upfirdn2d

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upfirdn_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
NANBITS = 0x7fc0beef
SLACK = 64
SLOPE, SCALE = 0.2, 2 ** 0.5
SLOPE32, SCALE32 = float(np.float32(SLOPE)), float(np.float32(SCALE))
D64 = torch.float64


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


class _Slack:
    """A tensor on the device as a contiguous view into a buffer whose other words hold NANBITS; lead shifts the view off the
    16-byte grid."""

    def __init__(self, shape, dev, value=None, lead=3):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * SLACK,), NANBITS, dtype=torch.int32, device=dev)
        self.lo, self.hi = SLACK + lead, SLACK + lead + n
        self.t = self.buf.view(torch.float32)[self.lo:self.hi].view(shape)
        self.value = value
        if value is not None:
            self.t.copy_(value)

    def intact(self):
        ok = bool((self.buf[:self.lo] == NANBITS).all()) and bool((self.buf[self.hi:] == NANBITS).all())
        if self.value is not None:
            ok = ok and torch.equal(self.t.cpu().view(torch.int32), self.value.contiguous().view(torch.int32))
        return ok


def _device_ufd(x, k, up, down, pad, dev):
    """sr_upfirdn2d_f32 on operands in NaN slack; asserts the slack, the operands and the finiteness of the output."""
    oh, ow = R.out_size(x.size(2), x.size(3), k.size(0), k.size(1), up, down, pad)
    xs, ks, ys = _Slack(x.shape, dev, x), _Slack(k.shape, dev, k, lead=1), _Slack((x.size(0), x.size(1), oh, ow), dev, lead=2)
    H.upfirdn2d(xs.t, ks.t, up, down, pad, out=ys.t)
    torch.cuda.synchronize()
    assert xs.intact() and ks.intact() and ys.intact(), 'the call wrote outside its output or changed an operand'
    y = ys.t.cpu()
    assert bool(torch.isfinite(y).all())
    return y


def _within(got, y64, bound):
    """False when the shape differs or an element leaves its bound."""
    return tuple(got.shape) == tuple(y64.shape) and bool(((got.double() - y64).abs() <= bound).all())


def _ufd_ref(x, k, up, down, pad):
    y64 = R.upfirdn2d(x.double(), k.double(), up, down, pad)
    bound = (R.taps(k.size(0), k.size(1), up) + 1) * EPS * R.upfirdn2d(x.double().abs(), k.double().abs(), up, down, pad)
    return y64, bound


RESAMPLE = torch.tensor([1., 3., 3., 1.])
K44 = torch.outer(RESAMPLE, RESAMPLE) / 64
# (up, down, instance): the three StyleGAN2 instances
SG2 = {1: ((1, 1), (1, 1)), 2: ((2, 2), (1, 1)), 3: ((1, 1), (2, 2))}
# per instance: (N, C, H, W, pad (x0, x1, y0, y1)); tiles are 64 columns x 32 rows of the output
SG2_CASES = {
    1: [(2, 1, 1, 1, (2, 1, 2, 1)),            # a 1x1 input
        (2, 1, 70, 141, (2, 1, 2, 1)),         # 70 x 141 outputs: two tiles and a ragged tail each way
        (2, 7, 35, 66, (1, 2, 2, 1)),          # 7 planes, one full tile + tails
        (2, 2, 40, 70, (-1, 2, 3, -2)),        # negative pads: crops
        (2, 2, 9, 11, (6, 5, 7, 9))],          # pads larger than the filter
    2: [(2, 1, 1, 1, (2, 1, 2, 1)),
        (2, 1, 35, 70, (2, 1, 2, 1)),          # 70 x 140 outputs
        (2, 7, 17, 35, (2, 1, 2, 1)),
        (2, 2, 20, 37, (-1, 2, 3, -2)),
        (2, 2, 9, 11, (6, 5, 7, 9)),
        (2, 2, 3, 4, (2, 2, 2, 1))],           # the gradient call of the plain down-sampler on a 6x9 input
    3: [(2, 1, 1, 1, (2, 1, 2, 1)),
        (2, 1, 141, 281, (1, 1, 1, 1)),        # 70 x 140 outputs
        (2, 7, 70, 133, (1, 1, 1, 1)),
        (2, 2, 80, 150, (-1, 2, 3, -2)),
        (2, 2, 9, 11, (6, 5, 7, 9))],
}
# the generic instance: (kh, kw, up, down, N, C, H, W, pad)
GENERIC_CASES = [
    (3, 5, (1, 1), (1, 1), 2, 1, 1, 1, (4, 4, 2, 2)),             # a 1x1 input
    (3, 5, (3, 3), (1, 1), 2, 1, 24, 47, (2, 1, 1, 2)),           # factor 3; 72 x 139 outputs: two tiles + tails
    (2, 7, (2, 3), (3, 2), 2, 7, 30, 120, (3, 2, 1, 4)),          # (2, 3) mixed per axis, 7 planes
    (5, 3, (1, 1), (3, 3), 2, 2, 110, 210, (-1, 2, 3, -2)),       # phase planes at down 3, negative pads
    (4, 4, (2, 2), (2, 2), 2, 2, 9, 11, (6, 5, 7, 9)),            # pads larger than the filter
    (4, 4, (3, 3), (1, 1), 2, 2, 2, 4, (2, 0, 2, 2)),             # the gradient call of a down-sampler by 3 (pad 1) on 7x11
    (16, 16, (1, 1), (8, 8), 2, 1, 40, 600, (0, 0, 0, 0)),        # the largest window: 2-row tiles
    (1, 1, (2, 2), (1, 1), 2, 2, 5, 6, (0, 0, 0, 0)),             # outputs that meet no tap at all
    (4, 4, (2, 1), (1, 1), 2, 2, 9, 40, (2, 1, 1, 2)),            # the 4x4 filter with mixed factors is generic too
]


# ------------------------------------------------------------------------------------------------------------ upfirdn2d
@pytest.mark.parametrize('inst', [1, 2, 3])
def test_upfirdn2d_stylegan2_instances_match_float64(cuda, inst):
    up, down = SG2[inst]
    k = _rand((4, 4), 10 + inst)                      # a non-symmetric 4x4 filter
    for i, (n, c, h, w, pad) in enumerate(SG2_CASES[inst]):
        assert H.upfirdn2d_instance(4, 4, *up, *down)[:2] == (inst, 32)
        x = _rand((n, c, h, w), 100 * inst + i)
        y64, bound = _ufd_ref(x, k, up, down, pad)
        y = _device_ufd(x, k, up, down, pad, cuda)
        err = float(((y.double() - y64).abs() - bound).max())
        print(f'instance {inst} case {i}: out {tuple(y.shape)} max(err - bound) {err:.3e} max bound {float(bound.max()):.3e}')
        assert _within(y, y64, bound), (inst, i)


def test_upfirdn2d_generic_instance_matches_float64(cuda):
    tiles = set()
    for i, (kh, kw, up, down, n, c, h, w, pad) in enumerate(GENERIC_CASES):
        inst, th, lds = H.upfirdn2d_instance(kh, kw, *up, *down)
        assert inst == 0 and lds <= 63 * 1024
        tiles.add(th)
        x, k = _rand((n, c, h, w), 500 + i), _rand((kh, kw), 600 + i)
        y64, bound = _ufd_ref(x, k, up, down, pad)
        y = _device_ufd(x, k, up, down, pad, cuda)
        err = float(((y.double() - y64).abs() - bound).max())
        print(f'generic case {i}: out {tuple(y.shape)} tile rows {th} max(err - bound) {err:.3e}')
        assert _within(y, y64, bound), i
        if kh == 1 and up == (2, 2):
            assert float(y[:, :, 1::2].abs().max()) == 0.0 and float(y[:, :, :, 1::2].abs().max()) == 0.0
    assert {32, 16, 2} <= tiles


def test_dispatch_reaches_every_instance():
    reached = {H.upfirdn2d_instance(4, 4, *SG2[i][0], *SG2[i][1])[0] for i in SG2} \
        | {H.upfirdn2d_instance(kh, kw, *up, *down)[0] for kh, kw, up, down, *_ in GENERIC_CASES}
    assert reached == {0, 1, 2, 3}


@pytest.mark.parametrize('inst', [1, 2, 3])
def test_upfirdn2d_exact_cases_equal_float64_bit_for_bit(cuda, inst):
    up, down = SG2[inst]
    k = K44 * (4 if up[0] == 2 else 1)
    n, c, h, w, pad = SG2_CASES[inst][1][0], 3, *SG2_CASES[inst][1][2:]
    x = torch.randint(-8, 9, (n, c, h, w), generator=torch.Generator().manual_seed(40 + inst)).float()
    y64 = R.upfirdn2d(x.double(), k.double(), up, down, pad)
    assert torch.equal(y64, y64.float().double()) and float(y64.abs().max()) > 1
    y = _device_ufd(x, k, up, down, pad, cuda)
    assert torch.equal(y.double(), y64)


@pytest.mark.parametrize('case', [(4, 4, (1, 1), (1, 1)), (4, 4, (2, 2), (1, 1)), (4, 4, (1, 1), (2, 2)), (3, 5, (2, 3), (3, 2))])
def test_upfirdn2d_batch_of_two_is_two_batches_of_one_and_reruns_are_identical(cuda, case):
    kh, kw, up, down = case
    x, k = _rand((2, 3, 45, 77), 70).to(cuda), _rand((kh, kw), 71).to(cuda)
    pad = (2, 1, 1, 2)
    both = H.upfirdn2d(x, k, up, down, pad)
    again = H.upfirdn2d(x, k, up, down, pad)
    singles = torch.cat([H.upfirdn2d(x[i:i + 1].contiguous(), k, up, down, pad) for i in range(2)])
    one_plane = H.upfirdn2d(x[1:2, 2:3].contiguous(), k, up, down, pad)
    assert torch.equal(both.view(torch.int32), again.view(torch.int32))
    assert torch.equal(both.view(torch.int32), singles.view(torch.int32))
    assert torch.equal(both[1:2, 2:3].contiguous().view(torch.int32), one_plane.view(torch.int32))


# ----------------------------------------------------------------------------------------------------------- activation
def _np_act(x, b, slope, scale, ref=None):
    """The definition in IEEE float32: one add, one multiply on the negative side, one multiply by scale."""
    t = x if b is None else x + b.reshape((1, -1) + (1,) * (x.ndim - 2))
    assert t.dtype == np.float32
    t = np.where((t if ref is None else ref) > 0, t, t * np.float32(slope))
    return t * np.float32(scale)


def _depth(n, inner):
    """d of the header's reduction tree, the larger of the 16-byte and the scalar pass."""
    return max((4 * v - 1) + 6 + 3 + (math.ceil(n * math.ceil(inner / (1024 * v)) / 64) - 1) + 6 for v in (1, 4))


# C in {1, 3, 8, 100}; inner 1 (a single element per channel and image), below one chunk, ragged against 1024 and 4096 values
ACT_SHAPES = [(5, 1), (2, 3), (7, 8), (16, 100), (2, 3, 1, 1), (2, 3, 5, 7), (2, 8, 12, 12), (3, 1, 37, 113), (2, 100, 4, 3),
              (2, 3, 64, 68), (70, 8, 33, 32)]


@pytest.mark.parametrize('shape', ACT_SHAPES)
@pytest.mark.parametrize('lead', [0, 3])
def test_activation_forward_backward_and_ref_are_ieee_exact(cuda, shape, lead):
    """lead 0: 16-byte aligned operands (16-byte accesses where inner is a multiple of 4); lead 3: the scalar pass."""
    c = shape[1]
    seed = sum(shape) + lead
    x, g, ref = _rand(shape, seed), _rand(shape, seed + 1), _rand(shape, seed + 2)
    b = _rand((c,), seed + 3)
    xs, gs, rs = (_Slack(shape, cuda, t, lead=lead) for t in (x, g, ref))
    bd = b.to(cuda)
    for bias in (None, bd):
        want = _np_act(x.numpy(), None if bias is None else b.numpy(), SLOPE, SCALE)
        out = H.fused_bias_act(xs.t, bias, None, SLOPE, SCALE)
        assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    want_ref = _np_act(x.numpy(), b.numpy(), SLOPE, SCALE, ref=ref.numpy())
    assert np.array_equal(H.fused_bias_act(xs.t, bd, rs.t, SLOPE, SCALE).cpu().numpy().view(np.int32), want_ref.view(np.int32))
    # backward: ref = out, no bias
    out_s = _Slack(shape, cuda, out.cpu(), lead=lead)
    gx, gb = H.fused_bias_act_bwd(gs.t, out_s.t, SLOPE, SCALE)
    gx2, none = H.fused_bias_act_bwd(gs.t, out_s.t, SLOPE, SCALE, want_bias=False)
    torch.cuda.synchronize()
    want_gx = _np_act(g.numpy(), None, SLOPE, SCALE, ref=out.cpu().numpy())
    assert np.array_equal(gx.cpu().numpy().view(np.int32), want_gx.view(np.int32)) and none is None
    assert torch.equal(gx.view(torch.int32), gx2.view(torch.int32))
    dims = [0] + list(range(2, len(shape)))
    gx64 = gx.cpu().double()
    inner = int(np.prod(shape[2:]))
    bound = _depth(shape[0], inner) * EPS * gx64.abs().sum(dims)
    err = (gb.cpu().double() - gx64.sum(dims)).abs()
    print(f'{shape} lead {lead}: depth {_depth(shape[0], inner)} max gbias err / bound {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all())
    assert xs.intact() and gs.intact() and rs.intact() and out_s.intact()
    # reruns and batch splits are bit-identical
    gx3, gb3 = H.fused_bias_act_bwd(gs.t, out_s.t, SLOPE, SCALE)
    assert torch.equal(gb.view(torch.int32), gb3.view(torch.int32)) and torch.equal(gx.view(torch.int32), gx3.view(torch.int32))
    halves = torch.cat([H.fused_bias_act(xs.t[i:i + 1].contiguous(), bd, None, SLOPE, SCALE) for i in range(shape[0])])
    assert torch.equal(halves.view(torch.int32), out.view(torch.int32))


def test_negative_control_ref_ignored_in_the_backward(cuda):
    shape = (2, 3, 5, 7)
    g, out = _rand(shape, 1), _rand(shape, 2)
    want = _np_act(g.numpy(), None, SLOPE, SCALE, ref=out.numpy())
    gx, _ = H.fused_bias_act_bwd(g.to(cuda), out.to(cuda), SLOPE, SCALE)
    assert np.array_equal(gx.cpu().numpy().view(np.int32), want.view(np.int32))
    ignored = H.fused_bias_act(g.to(cuda), None, None, SLOPE, SCALE)           # the sign taken from g itself
    assert not np.array_equal(ignored.cpu().numpy().view(np.int32), want.view(np.int32))


# ------------------------------------------------------------------------------------------------------------- autograd
GRAD_CASES = [(K44, (1, 1), (1, 1), (2, 1, 2, 1), (2, 3, 40, 70)), (K44 * 4, (2, 2), (1, 1), (2, 1, 2, 1), (2, 3, 20, 37)),
              (K44, (1, 1), (2, 2), (1, 1, 1, 1), (2, 3, 6, 9)), (K44, (1, 1), (2, 2), (1, 1, 1, 1), (2, 3, 70, 133)),
              (None, (2, 3), (3, 2), (3, 2, 1, 4), (2, 2, 30, 50))]


@pytest.mark.parametrize('case', range(len(GRAD_CASES)))
def test_upfirdn2d_first_derivative_matches_float64_autograd(cuda, case):
    k, up, down, pad, shape = GRAD_CASES[case]
    k = _rand((3, 5), 80) if k is None else k
    x = _rand(shape, 81 + case)
    xd = x.to(cuda).requires_grad_(True)
    kd = k.to(cuda).requires_grad_(True)
    y = UpFirDn2d.apply(xd, kd, up, down, pad)
    g = _rand(tuple(y.shape), 90 + case)
    gx, gk = torch.autograd.grad(y, (xd, kd), g.to(cuda), allow_unused=True)
    assert gk is None                                       # the kernel argument gets no gradient
    x64 = x.double().requires_grad_(True)
    y64 = R.upfirdn2d(x64, k.double(), up, down, pad)
    assert _within(y.detach().cpu(), y64.detach(), _ufd_ref(x, k, up, down, pad)[1])
    gx64, = torch.autograd.grad(y64, x64, g.double())
    a, gp = R.grad_call(g.double().abs(), k.double().abs(), shape[2:], up, down, pad)
    bound = (R.taps(k.size(0), k.size(1), down) + 1) * EPS * a
    print(f'case {case}: gradient pads {gp} max(err - bound) {float(((gx.cpu().double() - gx64).abs() - bound).max()):.3e}')
    assert _within(gx.cpu(), gx64, bound)
    if case == 2:
        assert gp == (2, 2, 2, 1)                          # the asymmetric pads of the plain down-sampler on 6x9


@pytest.mark.parametrize('shape', [(4, 8), (2, 3, 5, 7), (2, 8, 33, 32)])
def test_activation_first_derivative_matches_float64_autograd(cuda, shape):
    x, g, b = _rand(shape, 5), _rand(shape, 6), _rand((shape[1],), 7)
    xd, bd = x.to(cuda).requires_grad_(True), b.to(cuda).requires_grad_(True)
    out = fused_leaky_relu(xd, bd, SLOPE, SCALE)
    gx, gb = torch.autograd.grad(out, (xd, bd), g.to(cuda))
    x64, b64 = x.double().requires_grad_(True), b.double().requires_grad_(True)
    out64 = R.bias_act(x64, b64, SLOPE32, SCALE32)
    gx64, gb64 = torch.autograd.grad(out64, (x64, b64), g.double())
    assert _within(out.detach().cpu(), out64.detach(), 3 * EPS * out64.detach().abs())
    assert _within(gx.cpu(), gx64, 3 * EPS * gx64.abs())
    dims = [0] + list(range(2, len(shape)))
    d = _depth(shape[0], int(np.prod(shape[2:])))
    assert _within(gb.cpu(), gb64, (d + 3) * EPS * gx64.abs().sum(dims))
    # without a bias (ScaledLeakyReLU's call) there is no bias gradient to compute
    out2 = fused_leaky_relu(xd, None, SLOPE, SCALE)
    gx2, = torch.autograd.grad(out2, xd, g.to(cuda))
    want = _np_act(g.numpy(), None, SLOPE, SCALE, ref=x.detach().numpy())
    assert np.array_equal(gx2.cpu().numpy().view(np.int32), want.view(np.int32))


def _r1_operands():
    gen = torch.Generator().manual_seed(2024)
    shape = (2, 8, 9, 11)
    x = torch.randint(-32, 33, shape, generator=gen).float() / 8                 # 2^-3 Z, |x| <= 4
    b = (2 * torch.randint(-512, 512, (8,), generator=gen) + 1).float() / 1024    # odd multiples of 2^-10, |b| < 1
    v = torch.randn((2, 8, 8, 10), generator=gen, dtype=torch.float32)
    return x, K44.clone(), b, v


def _r1(x, k, b, v, ufd, act):
    out = act(ufd(x, k), b)
    loss = (v * out).sum()
    gx, gb = torch.autograd.grad(loss, (x, b), create_graph=True)
    p = gx.pow(2).sum() + gb.pow(2).sum()
    dv, = torch.autograd.grad(p, v)
    return out, gx, gb, dv


def test_second_derivative_r1_pattern_matches_float64(cuda):
    x, k, b, v = _r1_operands()
    pad = (1, 1, 1, 1)
    one = (1, 1)
    x64, b64, v64 = (t.double().requires_grad_(True) for t in (x, b, v))
    k64 = k.double()
    pre = R.upfirdn2d(x64, k64, one, one, pad) + b64.view(1, -1, 1, 1)
    assert torch.equal(pre.detach(), pre.detach().float().double()) and float(pre.detach().abs().min()) >= 2.0 ** -10
    out64, gx64, gb64, dv64 = _r1(x64, k64, b64, v64, lambda a, f: R.upfirdn2d(a, f, one, one, pad),
                                  lambda u, c: R.bias_act(u, c, SLOPE32, SCALE32))
    xd, bd, vd = (t.to(cuda).requires_grad_(True) for t in (x, b, v))
    out, gx, gb, dv = _r1(xd, k.to(cuda), bd, vd, lambda a, f: upfirdn2d(a, f, pad=(1, 1)),
                          lambda u, c: fused_leaky_relu(u, c, SLOPE, SCALE))
    rms = float(dv64.pow(2).mean().sqrt())
    assert rms > 1, rms                                                        # far from degenerate
    # the bound of the module docstring
    dmul = torch.where(pre.detach() > 0, 1.0, SLOPE32) * SCALE32
    z = (dmul * v.double()).abs()
    t, d = 16, _depth(2, 80)
    w = 2 * R.upfirdn2d(R.grad_call(z, k64, (9, 11), one, one, pad)[0], k64, one, one, pad)
    gsum = 2 * z.sum((0, 2, 3)).view(1, -1, 1, 1).expand_as(z)
    bound = dmul * ((2 * t + 8) * w + (2 * d + 8) * gsum) * EPS
    err = (dv.cpu().double() - dv64).abs()
    print(f'R1: rms dP/dv {rms:.2f}, max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}, d {d}')
    assert bool((err <= bound).all())
    assert _within(gx.detach().cpu(), gx64.detach(), (t + 3) * EPS * R.grad_call(z, k64, (9, 11), one, one, pad)[0])
    assert _within(gb.detach().cpu(), gb64.detach(), (d + 2) * EPS * z.sum((0, 2, 3)))
    # a mistake in the second-order path is far outside the bound: the activation's double backward without `ref`
    wrong = R.bias_act(R.upfirdn2d(2 * gx64.detach(), k64, one, one, pad), 2 * gb64.detach(), SLOPE32, SCALE32)
    assert not _within(wrong, dv64, bound)


def test_module_bias_receives_its_gradient(cuda):
    m = FusedLeakyReLU(8).to(cuda)
    assert float(m.bias.detach().abs().max()) == 0.0 and m.negative_slope == 0.2 and m.scale == 2 ** 0.5
    x = _rand((2, 8, 5, 6), 3)
    m(x.to(cuda)).sum().backward()
    want = torch.where(x > 0, 1.0, SLOPE32).double().sum((0, 2, 3)) * SCALE32
    assert m.bias.grad is not None and _within(m.bias.grad.cpu(), want, (_depth(2, 30) + 3) * EPS * want.abs())


# ---------------------------------------------------------------------------------------------------- negative controls
def test_negative_control_filter_not_flipped(cuda):
    x, k = _rand((2, 2, 20, 30), 1), _rand((3, 5), 2)
    up, down, pad = (1, 1), (1, 1), (2, 2, 1, 1)
    y64, bound = _ufd_ref(x, k, up, down, pad)
    assert _within(_device_ufd(x, k, up, down, pad, cuda), y64, bound)
    assert not _within(_device_ufd(x, torch.flip(k, [0, 1]).contiguous(), up, down, pad, cuda), y64, bound)


def test_negative_control_x_and_y_pads_swapped(cuda):
    x, k = _rand((2, 2, 20, 20), 3), _rand((4, 4), 4)
    up, down, pad = (2, 2), (1, 1), (2, 1, 1, 2)
    y64, bound = _ufd_ref(x, k, up, down, pad)
    assert _within(_device_ufd(x, k, up, down, pad, cuda), y64, bound)
    assert not _within(_device_ufd(x, k, up, down, (1, 2, 2, 1), cuda), y64, bound)


def test_negative_control_second_gradient_pad_off_by_one(cuda):
    """The down-sampler on 6x9: its gradient is the up-2 call with pads (2, 2, 2, 1); with (2, 2, 2, 2) or (2, 3, 2, 1) it is not."""
    k, up, down, pad, shape = K44, (1, 1), (2, 2), (1, 1, 1, 1), (2, 3, 6, 9)
    x64 = _rand(shape, 5).double().requires_grad_(True)
    y64 = R.upfirdn2d(x64, k.double(), up, down, pad)
    g = _rand(tuple(y64.shape), 6)
    gx64, = torch.autograd.grad(y64, x64, g.double())
    a, gp = R.grad_call(g.double().abs(), k.double(), shape[2:], up, down, pad)
    bound = (4 + 1) * EPS * a
    flipped = torch.flip(k, [0, 1]).contiguous()
    assert gp == (2, 2, 2, 1) and _within(_device_ufd(g, flipped, down, up, gp, cuda), gx64, bound)
    for wrong in ((2, 2, 2, 2), (2, 3, 2, 1), (2, 2, 2, 0)):
        assert not _within(_device_ufd(g, flipped, down, up, wrong, cuda), gx64, bound), wrong
    # a first pad off by one keeps the shape when the second gives the sample back: the values leave the bound
    assert not _within(_device_ufd(g, flipped, down, up, (3, 1, 2, 1), cuda), gx64, bound)
