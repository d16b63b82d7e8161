"""Every kernel of include/sr_hip_edvr_bf16.h against float64, on its production dispatch.

Conventions.  A CB16 operand is a channel-block window of a wider tensor, so its image stride exceeds the image; every slack
element of inputs and outputs holds the NaN pattern 0x7FC1 and must come back bit for bit.  Offsets and masks are channel slices
of one fp32 NCHW tensor with spare planes.  Every launch runs twice and must repeat bit for bit.  Inputs, weights and biases are
bf16-exact, so the float64 reference starts from the same numbers.

Bounds are derived, not fitted.  EPS = 2^-24 (half an fp32 ulp, relative).  Half a bf16 ulp of a value v is
hulp(v) = 2^(floor(log2 |v|) - 8): between 2^-9 |v| (at the top of a binade) and 2^-8 |v| (at its bottom); the tests use hulp
itself, evaluated at |y64| + E where E is the error before the rounding, so the figure is never wider than the format's.
A is the same operation on absolute values in float64.

  deformable conv   E = k EPS A + EPS |y64| + sum |W| dcol,  |y - y64| <= E + hulp(|y64| + E)
      k = 2 * 9 * cin + K_EPI: two roundings per product of the MFMA chain over (block, tap, channel) as in tests/test_conv_ops_gpu.py
          (the products of two bf16 values are exact; the internal order of the MFMA sum is not documented), K_EPI = 2 for the
          bias add and the LeakyReLU product.
      dcol, the error of one masked sample (the column the MFMA reads), by offset family:
        zero offsets, mask 1    the weights are 1, 0, 0, 0 and the mask product is by 1: the sample is x, a bf16 value.  dcol = 0
                                and k = 2 * 9 * cin + 8, the plain bf16 conv's bound.
        exact                   offsets integer + q/4, mask in {1, 1/2, 1/4}, x integers in [-3, 3]: the weights are multiples of
                                1/16, every product and sum is exact in fp32 and the masked sample is m/64 with |m| <= 192: a
                                bf16 value.  dcol = 0.  What is left is the chain, the epilogue and the output's rounding: the
                                sharp test of indexing, tap order, group mapping and swizzle.
        border                  the same with positions in (-1, 0) and (H - 1, H) (W likewise), where only some corners count,
                                and exactly -1 and exactly H (outside: zero).  dcol = 0.
        arbitrary N(0, 2^2), logit mask
                                dcol = E_s + hulp(|c64| + E_s),  E_s = (K_SAMPLE + 1 + K_SIGMOID) EPS C + EPS (|h_im| + |w_im| + 2) S
                                with C the sample of |x| under |mask|, K_SAMPLE = 8 (four products, three adds, the mask product),
                                + 1 because the weight products are no longer exact, K_SIGMOID = 4 (expf 1 ulp = 2 EPS, one
                                add, one division), and the position term of tests/test_dcn_ops_gpu.py: S = |mask| * (sum of |v|
                                over the valid corners) bounds the sample's slope in either coordinate and in 1 - lh, 1 - lw.
        far outside             every sample is zero: the output is bf16(act(bias)) exactly.
  1x1 conv          E = (2 cin + 8) EPS A + EPS |y64|, |y - y64| <= E + hulp(|y64| + E)
  subsample, max    exact
  average           E = 9 EPS avg(|x|): eight adds and a correctly rounded division; + hulp
  correlation       p: 0.25 * 2 c EPS sum |emb| |ref| + K_SIGMOID EPS p (the fp32 kernel's bound; the products are exact here);
                    out against float64 aligned * (the kernel's own p): 3 EPS |v| + hulp
  gate              against float64 (feat * m) * 2 + add with m = sigmoid in float64: 6 EPS (2 |feat| m + |add|) + hulp

Negative controls: the (dy, dx) planes of one tap swapped, the mask planes of two groups swapped, two weight rows of the 1x1
conv swapped; each must break its bound.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from image_restoration_amd import hip_ops as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_restate as R  # noqa: E402
from bf16_opwise import check, hulp  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
K_EPI, K_SAMPLE, K_SIGMOID = 2, 8, 4
NAN16 = 0x7FC1
D = torch.float64


def bf(t):
    return t.float().bfloat16().double()


def to_cb16(x, dev, lead=1, tail=2):
    """NCHW (bf16-exact values) -> a CB16 window with `lead` / `tail` slack blocks of NaN pattern around it."""
    n, c, h, w = x.shape
    cb = (c + 15) // 16
    buf = torch.empty((n, lead + cb + tail, h, w, 16), dtype=torch.bfloat16)
    buf.view(torch.int16).fill_(NAN16)
    xp = torch.zeros((n, cb * 16, h, w), dtype=D)
    xp[:, :c] = x
    buf[:, lead:lead + cb] = xp.view(n, cb, 16, h, w).permute(0, 1, 3, 4, 2).bfloat16()
    return H.CB16(buf.to(dev), lead, cb)


def empty_cb16(n, c, h, w, dev, lead=1, tail=2):
    cb = (c + 15) // 16
    buf = torch.empty((n, lead + cb + tail, h, w, 16), dtype=torch.bfloat16)
    buf.view(torch.int16).fill_(NAN16)
    return H.CB16(buf.to(dev), lead, cb)


def nchw(win, c=None):
    b = win.buf[:, win.cb0:win.cb0 + win.cbn].cpu()
    n, cb, h, w, _ = b.shape
    full = b.permute(0, 1, 4, 2, 3).reshape(n, cb * 16, h, w).double()
    return full if c is None else full[:, :c]


def slack_kept(win, what):
    bits = win.buf.cpu().view(torch.int16)
    keep = torch.ones(bits.shape[1], dtype=torch.bool)
    keep[win.cb0:win.cb0 + win.cbn] = False
    assert bool((bits[:, keep] == NAN16).all()), f'{what}: slack blocks changed'


def bits(win):
    return win.buf.cpu().view(torch.int16).clone()


# ------------------------------------------------------------------------------------------------------ deformable conv
DCN_CASES = [(1, 16, 16, 2, 1, 1), (2, 16, 32, 2, 5, 7), (1, 32, 24, 4, 9, 33), (1, 64, 64, 8, 12, 40), (1, 32, 16, 1, 6, 6)]
FAMILIES = ['zero', 'exact', 'arbitrary', 'border', 'far']


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dcn_inputs(case, family):
    n, cin, cout, dg, h, w = case
    g = _gen(1000 * FAMILIES.index(family) + sum((i + 1) * v for i, v in enumerate(case)))
    wt = bf(torch.randint(-8, 9, (cout, cin, 3, 3), generator=g).double() / 16)
    bias = bf(torch.randint(-8, 9, (cout,), generator=g).double() / 4)
    logit = False
    if family in ('exact', 'border', 'far'):
        x = torch.randint(-3, 4, (n, cin, h, w), generator=g).double()
        mask = torch.tensor([1.0, 0.5, 0.25], dtype=D)[torch.randint(0, 3, (n, 9 * dg, h, w), generator=g)]
        if family == 'exact':
            off = torch.randint(-3, 4, (n, 18 * dg, h, w), generator=g).double() + torch.randint(0, 4, (n, 18 * dg, h, w), generator=g).double() / 4
        elif family == 'far':
            off = torch.where(torch.rand((n, 18 * dg, h, w), generator=g) < 0.5, -1.0, 1.0).double() * (1000.0 + h + w)
        else:
            # positions chosen outright: off = target - (pixel - 1 + tap); targets just inside and exactly on both borders
            th = torch.tensor([-1.0, -0.75, -0.25, h - 0.75, h - 0.25, float(h), 0.0, h - 1.0], dtype=D)
            tw = torch.tensor([-1.0, -0.75, -0.25, w - 0.75, w - 0.25, float(w), 0.0, w - 1.0], dtype=D)
            hi = th[torch.randint(0, 8, (n, dg, 9, h, w), generator=g)]
            wi = tw[torch.randint(0, 8, (n, dg, 9, h, w), generator=g)]
            zero = torch.zeros((n, 18 * dg, h, w), dtype=D)
            bh, bw = R.positions(zero, dg)
            off = torch.stack([hi - bh, wi - bw], dim=3).reshape(n, 18 * dg, h, w)
    else:
        x = bf(torch.randn((n, cin, h, w), generator=g, dtype=D))
        if family == 'zero':
            off, mask = torch.zeros((n, 18 * dg, h, w), dtype=D), torch.ones((n, 9 * dg, h, w), dtype=D)
        else:
            off = (torch.randn((n, 18 * dg, h, w), generator=g, dtype=D) * 2).float().double()
            mask = torch.randn((n, 9 * dg, h, w), generator=g, dtype=D).float().double()
            logit = True
    return x, off, mask, logit, wt, bias


def _dcn_reference(case, family, x, off, mask, logit, wt, bias, slope):
    n, cin, cout, dg, h, w = case
    m = torch.sigmoid(mask) if logit else mask
    cols = R.columns(x, off, m, dg)                                   # [n, cin, 9, h, w]
    absw = wt.abs().reshape(cout, cin, 9)
    pre = torch.einsum('ock,nckhw->nohw', wt.reshape(cout, cin, 9), cols) + bias.view(1, -1, 1, 1)
    y64 = torch.where(pre > 0, pre, slope * pre)
    cabs = R.columns(x.abs(), off, m.abs(), dg)
    A = torch.einsum('ock,nckhw->nohw', absw, cabs) + bias.abs().view(1, -1, 1, 1)
    k = 2 * 9 * cin + (8 if family == 'zero' else K_EPI)
    E = k * EPS * A + EPS * y64.abs()
    if family == 'arbitrary':
        S = R.columns(x.abs(), off, m.abs(), dg, corner_weights='ones')
        h_im, w_im = R.positions(off, dg)
        pos = (h_im.abs() + w_im.abs() + 2).unsqueeze(2).expand(n, dg, cin // dg, 9, h, w).reshape(n, cin, 9, h, w)
        Es = (K_SAMPLE + 1 + K_SIGMOID) * EPS * cabs + EPS * pos * S
        dcol = Es + hulp(cols.abs() + Es)
        E = E + torch.einsum('ock,nckhw->nohw', absw, dcol)
    return y64, E + hulp(y64.abs() + E)


def _run_dcn(case, x, off, mask, logit, wt, bias, slope, cuda):
    n, cin, cout, dg, h, w = case
    xw = to_cb16(x, cuda)
    planes = torch.full((n, 27 * dg + 5, h, w), float('nan'), dtype=torch.float32)
    planes[:, :18 * dg], planes[:, 18 * dg:27 * dg] = off.float(), mask.float()
    planes = planes.to(cuda)
    pc = H.PackedConvBF16(wt.float().to(cuda), bias.float().to(cuda))
    outs = []
    for _ in range(2):
        ow = empty_cb16(n, cout, h, w, cuda)
        H.dcn_fwd_bf16(xw, planes[:, :18 * dg], planes[:, 18 * dg:27 * dg], pc, dg, mask_is_logit=logit, act_slope=slope, out=ow)
        outs.append(ow)
    torch.cuda.synchronize()
    assert torch.equal(bits(outs[0]), bits(outs[1])), 'rerun differs'
    slack_kept(outs[0], 'dcn out')
    slack_kept(xw, 'dcn x')
    full = nchw(outs[0])
    assert float(full[:, cout:].abs().max()) == 0.0 if full.size(1) > cout else True, 'pad channels are not zero'
    return full[:, :cout]


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('case', DCN_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_dcn_fwd(cuda, case, family):
    n, cin, cout, dg, h, w = case
    cot, rows, lds = H.dcn_bf16_instance(cout, n, h, w)
    assert (cot, rows, lds) == ((2, 4, 72 * 1024) if cout == 64 else (1, 4, 54 * 1024))   # both instances are reached below
    slope = 0.1
    x, off, mask, logit, wt, bias = _dcn_inputs(case, family)
    got = _run_dcn(case, x, off, mask, logit, wt, bias, slope, cuda)
    if family == 'far':
        b32 = bias.float()
        want = torch.where(b32 > 0, b32, b32 * slope).bfloat16().double().view(1, -1, 1, 1).expand_as(got)
        assert torch.equal(got, want), 'far outside: the output is not bf16(act(bias))'
        return
    y64, bound = _dcn_reference(case, family, x, off, mask, logit, wt, bias, slope)
    if family in ('exact', 'border'):   # the premise of dcol = 0: every masked sample is a bf16 value
        cols = R.columns(x, off, mask, dg)
        assert torch.equal(bf(cols), cols)
    check(got, y64, bound, f'dcn {family} {case}')


def test_dcn_instances_of_the_default_network(cuda):
    """cout 64 (COT 2) and the 24 / 16 / 32-cout cases (COT 1) are the two instances the dispatch can choose."""
    assert {H.dcn_bf16_instance(c[2], c[0], c[4], c[5])[0] for c in DCN_CASES} == {1, 2}


@pytest.mark.parametrize('control', ['swap_dy_dx', 'swap_mask_groups'])
def test_dcn_negative_controls(cuda, control):
    case = (2, 16, 32, 2, 5, 7)
    n, cin, cout, dg, h, w = case
    x, off, mask, logit, wt, bias = _dcn_inputs(case, 'exact')
    y64, bound = _dcn_reference(case, 'exact', x, off, mask, logit, wt, bias, 0.1)
    off2, mask2 = off.clone(), mask.clone()
    if control == 'swap_dy_dx':
        off2[:, 8], off2[:, 9] = off[:, 9], off[:, 8]            # tap 4 of group 0
    else:
        mask2[:, :9], mask2[:, 9:18] = mask[:, 9:18], mask[:, :9]
    got = _run_dcn(case, x, off2, mask2, logit, wt, bias, 0.1, cuda)
    assert bool(((got - y64).abs() > bound).any()), f'{control} stays inside the bound: the bound cannot see it'


# ------------------------------------------------------------------------------------------------------------- 1x1 conv
PW_CASES = [(1, 16, 1, 1, 1), (2, 320, 64, 5, 7), (1, 32, 24, 3, 70), (1, 128, 64, 33, 33)]


def _pw(case, with_bias, slope, cuda, swap_rows=False):
    n, cin, cout, h, w = case
    g = _gen(sum((i + 1) * v for i, v in enumerate(case)))
    x = bf(torch.randn((n, cin, h, w), generator=g, dtype=D))
    wt = bf(torch.randn((cout, cin, 1, 1), generator=g, dtype=D) * 0.25)
    bias = bf(torch.randn((cout,), generator=g, dtype=D)) if with_bias else None
    pre = F.conv2d(x, wt, bias)
    y64 = torch.where(pre > 0, pre, slope * pre)
    A = F.conv2d(x.abs(), wt.abs(), bias.abs() if with_bias else None)
    E = (2 * cin + 8) * EPS * A + EPS * y64.abs()
    wd = wt.clone()
    if swap_rows:
        wd[0], wd[cout - 1] = wt[cout - 1], wt[0]
    pc = H.PackedConv1x1BF16(wd.float().to(cuda), bias.float().to(cuda) if with_bias else None)
    xw = to_cb16(x, cuda)
    outs = []
    for _ in range(2):
        ow = empty_cb16(n, cout, h, w, cuda)
        H.conv1x1_bf16(xw, pc, out=ow, act_slope=slope)
        outs.append(ow)
    torch.cuda.synchronize()
    assert torch.equal(bits(outs[0]), bits(outs[1])), 'rerun differs'
    slack_kept(outs[0], 'conv1x1 out')
    full = nchw(outs[0])
    if full.size(1) > cout:
        assert float(full[:, cout:].abs().max()) == 0.0, 'pad channels are not zero'
    return full[:, :cout], y64, E + hulp(y64.abs() + E)


@pytest.mark.parametrize('with_bias,slope', [(True, 0.1), (False, 1.0), (True, 1.0)])
@pytest.mark.parametrize('case', PW_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_conv1x1(cuda, case, with_bias, slope):
    got, y64, bound = _pw(case, with_bias, slope, cuda)
    check(got, y64, bound, f'conv1x1 {case} bias={with_bias} slope={slope}')


def test_conv1x1_negative_control(cuda):
    got, y64, bound = _pw((2, 320, 64, 5, 7), True, 0.1, cuda, swap_rows=True)
    assert bool(((got - y64).abs() > bound).any())


# ---------------------------------------------------------------------------------------- subsample, pool, correlation, gate
SIZES = [(1, 16, 1, 1), (1, 16, 2, 2), (2, 32, 5, 7), (1, 16, 8, 12), (2, 48, 13, 35)]


def _rand_cb(shape, seed, cuda, scale=1.0):
    x = bf(torch.randn(shape, generator=_gen(seed), dtype=D) * scale)
    return x, to_cb16(x, cuda)


@pytest.mark.parametrize('shape', SIZES, ids=lambda s: 'x'.join(map(str, s)))
def test_subsample2(cuda, shape):
    n, c, h, w = shape
    x, xw = _rand_cb(shape, 11, cuda)
    ow = empty_cb16(n, c, (h + 1) // 2, (w + 1) // 2, cuda)
    H.subsample2_bf16(xw, out=ow)
    ow2 = empty_cb16(n, c, (h + 1) // 2, (w + 1) // 2, cuda)
    H.subsample2_bf16(xw, out=ow2)
    assert torch.equal(nchw(ow, c), x[:, :, ::2, ::2]) and torch.equal(bits(ow), bits(ow2))
    slack_kept(ow, 'subsample out')


def test_subsample2_after_a_stride1_conv_is_the_stride2_conv(cuda):
    """sr_conv3x3_bf16 then the subsample equals F.conv2d(stride=2) of the same bf16 operands within the plain conv's bound."""
    n, cin, cout, h, w = 1, 16, 16, 9, 14
    g = _gen(5)
    x = bf(torch.randn((n, cin, h, w), generator=g, dtype=D))
    wt = bf(torch.randn((cout, cin, 3, 3), generator=g, dtype=D) * 0.125)
    bias = bf(torch.randn((cout,), generator=g, dtype=D))
    pc = H.PackedConvBF16(wt.float().to(cuda), bias.float().to(cuda))
    got = nchw(H.subsample2_bf16(H.conv3x3_bf16(to_cb16(x, cuda), pc, act_slope=0.1)), cout)
    pre = F.conv2d(x, wt, bias, stride=2, padding=1)
    y64 = torch.where(pre > 0, pre, 0.1 * pre)
    E = (2 * 9 * cin + 8) * EPS * F.conv2d(x.abs(), wt.abs(), bias.abs(), stride=2, padding=1) + EPS * y64.abs()
    check(got, y64, E + hulp(y64.abs() + E), 'stride-2 conv as conv + subsample')


@pytest.mark.parametrize('shape', SIZES, ids=lambda s: 'x'.join(map(str, s)))
def test_pool3x3s2(cuda, shape):
    n, c, h, w = shape
    x, xw = _rand_cb(shape, 12, cuda)
    ho, wo = (h + 1) // 2, (w + 1) // 2
    ow = empty_cb16(n, 2 * c, ho, wo, cuda)
    H.pool3x3s2_bf16(xw, out=ow)
    ow2 = empty_cb16(n, 2 * c, ho, wo, cuda)
    H.pool3x3s2_bf16(xw, out=ow2)
    torch.cuda.synchronize()
    assert torch.equal(bits(ow), bits(ow2))
    got = nchw(ow)
    assert torch.equal(got[:, :c], F.max_pool2d(x, 3, 2, 1)), 'max pool is not exact'
    avg = F.avg_pool2d(x, 3, 2, 1)
    E = 9 * EPS * F.avg_pool2d(x.abs(), 3, 2, 1)
    check(got[:, c:], avg, E + hulp(avg.abs() + E), f'avg pool {shape}')
    slack_kept(ow, 'pool out')


@pytest.mark.parametrize('t', [1, 3, 5])
@pytest.mark.parametrize('c,h,w', [(16, 1, 1), (16, 2, 2), (64, 5, 7), (16, 13, 35)])
def test_tsa_corr(cuda, t, c, h, w):
    b = 2
    emb, ew = _rand_cb((b * t, c, h, w), 21, cuda, 0.5)
    ref, rw = _rand_cb((b, c, h, w), 22, cuda, 0.5)
    al, aw = _rand_cb((b * t, c, h, w), 23, cuda)
    s64 = (emb.view(b, t, c, h, w) * ref.unsqueeze(1)).sum(2)
    As = (emb.abs().view(b, t, c, h, w) * ref.abs().unsqueeze(1)).sum(2)
    p64 = torch.sigmoid(s64)
    runs = []
    for _ in range(2):
        ow = empty_cb16(b * t, c, h, w, cuda)
        prob, _ = H.tsa_corr_bf16(ew, rw, aw, t, out=ow, want_prob=True)
        runs.append((prob.cpu().double(), ow))
    torch.cuda.synchronize()
    pd, ow = runs[0]
    assert torch.equal(pd, runs[1][0]) and torch.equal(bits(ow), bits(runs[1][1]))
    check(pd, p64, 0.25 * 2 * c * EPS * As + K_SIGMOID * EPS * p64, f'tsa_corr p t={t} c={c} {h}x{w}')
    v = (al.view(b, t, c, h, w) * pd.unsqueeze(2)).reshape(b * t, c, h, w)    # float64 from the kernel's own p
    E = 3 * EPS * v.abs()
    check(nchw(ow, c), v, E + hulp(v.abs() + E), 'tsa_corr out')
    slack_kept(ow, 'tsa_corr out')
    ow3 = empty_cb16(b * t, c, h, w, cuda)
    H.tsa_corr_bf16(ew, rw, aw, t, out=ow3)                                    # without the prob pointer
    assert torch.equal(bits(ow3), bits(ow))


@pytest.mark.parametrize('shape', SIZES, ids=lambda s: 'x'.join(map(str, s)))
def test_tsa_gate(cuda, shape):
    n, c, h, w = shape
    feat, fw = _rand_cb(shape, 31, cuda)
    attn, tw = _rand_cb(shape, 32, cuda, 2.0)
    add, dw = _rand_cb(shape, 33, cuda)
    ow, ow2 = empty_cb16(n, c, h, w, cuda), empty_cb16(n, c, h, w, cuda)
    H.tsa_gate_bf16(fw, tw, dw, out=ow)
    H.tsa_gate_bf16(fw, tw, dw, out=ow2)
    torch.cuda.synchronize()
    assert torch.equal(bits(ow), bits(ow2))
    m = torch.sigmoid(attn)
    v = feat * m * 2 + add
    E = 6 * EPS * (2 * feat.abs() * m + add.abs())
    check(nchw(ow, c), v, E + hulp(v.abs() + E), f'tsa_gate {shape}')
    slack_kept(ow, 'tsa_gate out')


# -------------------------------------------------------------------------------------------------- one weight image, two kernels
def test_the_mode0_image_serves_both_kernels(cuda):
    """With zero offsets and unit mask the deformable conv and sr_conv3x3_bf16 read the same weight image and sample the same
    bf16 values in the same (block, tap) order: their outputs agree bit for bit (a packed image that differed between the
    two kernels, or a swizzle that moved a value, could not)."""
    n, cin, cout, dg, h, w = 1, 64, 64, 8, 12, 40
    g = _gen(9)
    x = bf(torch.randn((n, cin, h, w), generator=g, dtype=D))
    wt = bf(torch.randn((cout, cin, 3, 3), generator=g, dtype=D) * 0.1)
    bias = bf(torch.randn((cout,), generator=g, dtype=D))
    pc = H.PackedConvBF16(wt.float().to(cuda), bias.float().to(cuda))
    xw = to_cb16(x, cuda)
    off = torch.zeros((n, 18 * dg, h, w), dtype=torch.float32, device=cuda)
    mask = torch.ones((n, 9 * dg, h, w), dtype=torch.float32, device=cuda)
    a = H.dcn_fwd_bf16(xw, off, mask, pc, dg, act_slope=0.1)
    b = H.conv3x3_bf16(xw, pc, act_slope=0.1)
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(b)), 'the deformable conv at zero offsets is not sr_conv3x3_bf16 bit for bit'
