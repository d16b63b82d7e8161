"""The non-convolution training and metric kernels of csrc/train_ops.hip against float64 references of the same operation, at the
shapes where they go wrong: flat reductions at lengths around the block size and at production size (the grid is capped at 256
blocks, so every thread loops), Adam / EMA, Linear, bilinear x2, max-pool (ties, odd sizes), spectral norm (both row-chunked
branches of the power iteration), the element-wise ops and the PSNR / SSIM validation sums.

Tolerances are bounds, not fits.  EPS = 2^-24 is the unit roundoff of fp32; a chain of k fp32 operations over terms t_i is off by at
most about k * EPS * sum|t_i|.  Each reduction's bound is that product with k = its longest serial chain of additions (per-thread loop
+ 9 levels of the block tree + the sequential finalize); each element-wise bound counts the fp32 roundings of its formula (expf /
log1pf count as 2 ulp, i.e. 4 EPS).  Element-wise ops with no rounding are compared bit for bit.  The last element of every
reduction and the last input of every Linear row is chosen so that its contribution exceeds four times the bound: a kernel that
drops the tail fails (the test checks that it would)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from image_restoration_amd import _lib
from image_restoration_amd import hip_autograd as A

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
NS = [1, 255, 257, 4097, 256 * 4096 + 1, 25165824]  # the last: one 32x3x512x512 batch
f32 = np.float32


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr() if t is not None else None


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(cuda)


def _scal(v, cuda):
    return torch.tensor(v, dtype=torch.float32, device=cuda)


def _ws(lib, cuda):
    nb = lib.sr_reduce_workspace_bytes(8)
    return torch.zeros(nb, dtype=torch.uint8, device=cuda), nb


def _chain(n):
    """Longest serial chain of fp32 additions of flat_reduce over n terms (+2: the fp32 scale and its product)."""
    blocks = min(max((n + 4095) // 4096, 1), 256)
    return -(-n // (256 * blocks)) + 9 + blocks + 2


# ------------------------------------------------------------------------------------------------------ flat reductions / losses
# Every case: terms(x, t, shift) -> (f_i, mag_i) in float64 (mag bounds the per-term rounding: |fl(f_i) - f_i| <= ops * EPS * mag_i),
# tail(T, shift) -> (x_last, t_last) with |f_last| >= T.  `ops` counts the roundings of one term.
def _softplus(z):
    return np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))


def _sigmoid(z):
    return 0.5 * (1 + np.tanh(0.5 * z))


FWD = {
    # name: (call(lib, x, t, shift, n, w, out, dsum, ws, nb) -> rc, scale(w, n), terms, ops, tail)
    'mean': (lambda L, x, t, s, n, w, o, d, ws, nb: L.sr_mean_f32(x, n, o, ws, nb, _st()),
             lambda w, n: 1.0 / n, lambda x, t, s: (x, np.abs(x)), 0, lambda T, s: (T, 0.0)),
    'l1': (lambda L, x, t, s, n, w, o, d, ws, nb: L.sr_l1_loss_fwd_f32(x, t, n, w, o, ws, nb, _st()),
           lambda w, n: w / n, lambda x, t, s: (np.abs(x - t), np.abs(x - t)), 1, lambda T, s: (0.5 + T, 0.5)),
    'pixel_l1': (lambda L, x, t, s, n, w, o, d, ws, nb: L.sr_pixel_loss_fwd_f32(x, t, n, 0, 0.0, w, o, ws, nb, _st()),
                 lambda w, n: w / n, lambda x, t, s: (np.abs(x - t), np.abs(x - t)), 1, lambda T, s: (0.5 - T, 0.5)),
    'mse': (lambda L, x, t, s, n, w, o, d, ws, nb: L.sr_pixel_loss_fwd_f32(x, t, n, 1, 0.0, w, o, ws, nb, _st()),
            lambda w, n: w / n, lambda x, t, s: ((x - t) ** 2, (x - t) ** 2), 3, lambda T, s: (0.25 + math.sqrt(T), 0.25)),
    'charb1e-12': (lambda L, x, t, s, n, w, o, d, ws, nb: L.sr_pixel_loss_fwd_f32(x, t, n, 2, 1e-12, w, o, ws, nb, _st()),
                   lambda w, n: w / n, lambda x, t, s: (np.sqrt((x - t) ** 2 + float(f32(1e-12))),) * 2, 5, lambda T, s: (T, 0.0)),
    'charb1e-6': (lambda L, x, t, s, n, w, o, d, ws, nb: L.sr_pixel_loss_fwd_f32(x, t, n, 2, 1e-6, w, o, ws, nb, _st()),
                  lambda w, n: w / n, lambda x, t, s: (np.sqrt((x - t) ** 2 + float(f32(1e-6))),) * 2, 5, lambda T, s: (-T, 0.0)),
}
for _c in (-1.0, 1.0):
    FWD[f'gan1_{_c:+g}'] = (lambda L, x, t, s, n, w, o, d, ws, nb, c=_c: L.sr_gan_point_loss_fwd_f32(x, n, 1, c, w, o, ws, nb, _st()),
                            lambda w, n: w / n, lambda x, t, s, c=_c: ((x - c) ** 2,) * 2, 3, lambda T, s, c=_c: (c + math.sqrt(T), 0.0))
    FWD[f'gan2_{_c:+g}'] = (lambda L, x, t, s, n, w, o, d, ws, nb, c=_c: L.sr_gan_point_loss_fwd_f32(x, n, 2, c, w, o, ws, nb, _st()),
                            lambda w, n, c=_c: c * w / n, lambda x, t, s: (x, np.abs(x)), 2, lambda T, s: (T, 0.0))
    FWD[f'gan3_{_c:+g}'] = (lambda L, x, t, s, n, w, o, d, ws, nb, c=_c: L.sr_gan_point_loss_fwd_f32(x, n, 3, c, w, o, ws, nb, _st()),
                            lambda w, n: w / n, lambda x, t, s, c=_c: (_softplus(c * x),) * 2, 10, lambda T, s, c=_c: (c * T, 0.0))
    FWD[f'gan4_{_c:+g}'] = (lambda L, x, t, s, n, w, o, d, ws, nb, c=_c: L.sr_gan_point_loss_fwd_f32(x, n, 4, c, w, o, ws, nb, _st()),
                            lambda w, n: w / n, lambda x, t, s, c=_c: (np.maximum(1 + c * x, 0), 1 + np.abs(x)), 2,
                            lambda T, s, c=_c: (c * T, 0.0))
FWD['gan5_0.25'] = (lambda L, x, t, s, n, w, o, d, ws, nb: L.sr_gan_point_loss_fwd_f32(x, n, 5, 0.25, w, o, ws, nb, _st()),
                    lambda w, n: w / n, lambda x, t, s: (_softplus(x) - 0.25 * x, _softplus(x) + 0.25 * np.abs(x)), 12,
                    lambda T, s: (2 * T, 0.0))
for _real in (0, 1):
    _sg = -1.0 if _real else 1.0
    for _shift in (False, True):
        # BCE-with-logits of x - shift; the subtraction's rounding error is amplified by sigmoid(z) * |x| in softplus(z)
        FWD[f'bce_real{_real}_shift{int(_shift)}'] = (
            lambda L, x, t, s, n, w, o, d, ws, nb, r=_real: L.sr_bce_logits_fwd_f32(x, s, n, r, w, o, d, ws, nb, _st()),
            lambda w, n: w / n,
            lambda x, t, s, g=_sg: (_softplus(g * (x - s)), _softplus(g * (x - s)) + _sigmoid(g * (x - s)) * (np.abs(x) + abs(s))), 10,
            lambda T, s, g=_sg: (s + g * T, 0.0))


def _body(n, seed):
    """n - 1 body values (the tail is set per case): N(0, 2) logits / predictions with exact ties (x == t), both hinge kinks
    (x = +-1) and logits of +-100."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 2).astype(f32)
    t = rng.standard_normal(n).astype(f32)
    x[::7] = t[::7]
    x[3::11], x[5::11] = 1.0, -1.0
    x[2::13], x[4::13] = 100.0, -100.0
    return x, t


_DATA = {}


def _data(n):
    if n not in _DATA:
        _DATA[n] = _body(n, n)
    return _DATA[n]


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('name', list(FWD))
def test_flat_reduction_forward(cuda, lib, name, n):
    call, scale_of, terms, ops, tail = FWD[name]
    x, t = (a.copy() for a in _data(n))
    use_shift = 'shift1' in name
    shift = float(f32(0.37)) if use_shift else 0.0
    weight = 0.8
    scale = scale_of(float(f32(weight)), n)
    chain = _chain(n)
    # the tail term must outweigh four bounds on the sum of everything else
    fb, mb = terms(x[:-1].astype(np.float64), t[:-1].astype(np.float64), shift)
    T = 8 * EPS * ((chain + 1) * float(np.abs(fb).sum()) + ops * float(mb.sum())) + 4.0
    x[-1], t[-1] = (f32(v) for v in tail(T, shift))
    f, mag = terms(x.astype(np.float64), t.astype(np.float64), shift)
    ref = scale * float(f.sum())
    tol = EPS * abs(scale) * ((chain + 1) * float(np.abs(f).sum()) + ops * float(mag.sum())) + FLT_MIN
    assert abs(scale * f[-1]) > 4 * tol, 'the tail does not carry the sum: the case would not catch a dropped element'
    xd, td = _dev(x, cuda), _dev(t, cuda)
    sd = _scal(shift, cuda) if use_shift else None
    out = _scal(np.nan, cuda)
    dsum = _scal(np.nan, cuda) if name.startswith('bce') else None
    ws, nb = _ws(lib, cuda)
    _lib.check(call(lib, _p(xd), _p(td), _p(sd), n, weight, _p(out), _p(dsum), _p(ws), nb), name)
    got = float(out.cpu())
    assert abs(got - ref) <= tol, (name, n, got, ref, tol)
    if dsum is not None:
        # dsum = scale * sum sign * sigmoid(sign * (x - shift)): the derivative of the loss w.r.t. the shift, through `other`
        sg = -1.0 if 'real1' in name else 1.0
        z = sg * (x.astype(np.float64) - shift)
        d = sg * _sigmoid(z)
        dref = scale * float(d.sum())
        dtol = EPS * scale * ((chain + 1) * float(np.abs(d).sum()) + 8 * float((np.abs(d) * (1 + np.abs(z))).sum())) + FLT_MIN
        assert abs(float(dsum.cpu()) - dref) <= dtol, (name, n, float(dsum.cpu()), dref, dtol)
    assert np.isfinite(got)


# ------------------------------------------------------------------------------------------------------ element-wise backwards
def _bwd_case(name, x, t, shift):
    """(call(lib, x, t, shift, n, weight, g, dx) -> rc, ref d/dx per element before scale * g, magnitude, roundings)"""
    x64, t64 = x.astype(np.float64), t.astype(np.float64)
    if name in ('l1', 'pixel_l1'):
        k = 0
        fn = (lambda L, x, t, s, n, w, g, o: L.sr_l1_loss_bwd_f32(x, t, n, w, g, o, _st())) if name == 'l1' else \
            (lambda L, x, t, s, n, w, g, o: L.sr_pixel_loss_bwd_f32(x, t, n, 0, 0.0, w, g, o, _st()))
        return fn, np.sign(x64 - t64), np.abs(np.sign(x64 - t64)), 3
    if name == 'mse':
        return (lambda L, x, t, s, n, w, g, o: L.sr_pixel_loss_bwd_f32(x, t, n, 1, 0.0, w, g, o, _st()),
                2 * (x64 - t64), 2 * np.abs(x64 - t64), 4)
    if name.startswith('charb'):
        eps = 1e-12 if name == 'charb1e-12' else 1e-6
        d = x64 - t64
        r = d / np.sqrt(d * d + float(f32(eps)))
        return (lambda L, x, t, s, n, w, g, o, e=eps: L.sr_pixel_loss_bwd_f32(x, t, n, 2, e, w, g, o, _st()), r, np.abs(r), 9)
    if name.startswith('gan'):
        kind = int(name[3])
        c = float(name.split('_')[1])
        call = lambda L, x, t, s, n, w, g, o, k=kind, c=c: L.sr_gan_point_loss_bwd_f32(x, n, k, c, w, g, o, _st())
        if kind == 1:
            return call, 2 * (x64 - c), 2 * np.abs(x64 - c), 5
        if kind == 2:
            return call, np.full_like(x64, c), np.full_like(x64, abs(c)), 3
        if kind == 3:
            r = c * _sigmoid(c * x64)
            return call, r, np.abs(r), 9
        if kind == 4:
            r = np.where(1 + c * x64 > 0, c, 0.0)
            return call, r, np.abs(r), 3
        s = _sigmoid(x64)
        return call, s - c, s + abs(c), 10
    sg = -1.0 if 'real1' in name else 1.0
    z = sg * (x64 - shift)
    r = sg * _sigmoid(z)
    return (lambda L, x, t, s, n, w, g, o, real=int('real1' in name): L.sr_bce_logits_bwd_f32(x, s, n, real, w, g, o, _st()),
            r, np.abs(r) * (1 + np.abs(z)), 10)


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('name', [k for k in FWD if k != 'mean'])
def test_elementwise_backward(cuda, lib, name, n):
    x, t = _data(n)
    use_shift = 'shift1' in name
    shift = float(f32(0.37)) if use_shift else 0.0
    weight, g = 0.8, float(f32(0.7312))
    call, r, mag, ops = _bwd_case(name, x, t, shift)
    scale = weight / n
    xd, td, gd = _dev(x, cuda), _dev(t, cuda), _scal(g, cuda)
    sd = _scal(shift, cuda) if use_shift else None
    dx = torch.full((n,), float('nan'), device=cuda)
    _lib.check(call(lib, _p(xd), _p(td), _p(sd), n, weight, _p(gd), _p(dx)), name)
    got = dx.cpu().numpy().astype(np.float64)
    ref = r * scale * g
    tol = (ops + 2) * EPS * mag * scale * g + FLT_MIN   # + 2: weight / n is formed in fp32
    bad = np.abs(got - ref) > tol
    assert not bad.any(), (name, n, int(bad.sum()), got[bad][:4], ref[bad][:4])
    ties = (x == t)
    if name in ('l1', 'pixel_l1') or name.startswith('charb'):
        assert (got[ties] == 0).all()          # d = 0: L1 sign 0, Charbonnier 0 / sqrt(eps)
    if name.startswith('gan4'):
        c = float(name.split('_')[1])
        kink = (1 + c * x.astype(np.float64) == 0)
        assert kink[:-1].any() or n < 16
        assert (got[kink] == 0).all()          # relu'(0) = 0, as torch
    assert np.isfinite(got).all()


@pytest.mark.parametrize('n', [1, 257, 256 * 4096 + 1])
def test_fill_scaled(cuda, lib, n):
    g, s = _scal(0.7312, cuda), _scal(-3.25, cuda)
    dx = torch.full((n,), float('nan'), device=cuda)
    _lib.check(lib.sr_fill_scaled_f32(_p(g), _p(s), -1.0 / n, _p(dx), n, _st()), 'sr_fill_scaled_f32')
    ref = float(f32(-1.0 / n)) * float(f32(0.7312)) * -3.25
    got = dx.cpu().numpy().astype(np.float64)
    assert (np.abs(got - ref) <= 2 * EPS * abs(ref)).all()


def test_bce_relativistic_through_the_wrapper_matches_torch(cuda):
    """BCELogitsFn(x, other): loss and both gradients against torch float64 autograd of BCEWithLogits(x - mean(other))."""
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(4097, generator=g) * 3)
    x[:3] = torch.tensor([100.0, -100.0, 0.0])
    o = torch.randn(1000, generator=g) * 2
    for real in (True, False):
        xd, od = x.clone().to(cuda).requires_grad_(True), o.clone().to(cuda).requires_grad_(True)
        loss = A.BCELogitsFn.apply(xd, od, real, 0.5)
        loss.backward()
        x64, o64 = x.double().requires_grad_(True), o.double().requires_grad_(True)
        ref = 0.5 * F.binary_cross_entropy_with_logits(x64 - o64.mean(), torch.full_like(x64, float(real)))
        ref.backward()
        assert abs(float(loss) - float(ref)) <= 1e-6 * float(ref)
        assert torch.allclose(xd.grad.cpu().double(), x64.grad, rtol=1e-5, atol=1e-12)
        assert torch.allclose(od.grad.cpu().double(), o64.grad, rtol=1e-5, atol=1e-12)


# ------------------------------------------------------------------------------------------------------ loss wrappers: dtypes
@pytest.mark.parametrize('dtype,tdtype', [(torch.float64, torch.float32), (torch.bfloat16, torch.float32),
                                          (torch.float32, torch.float64), (torch.float64, torch.float64)])
def test_loss_wrappers_accept_any_floating_dtype(cuda, dtype, tdtype):
    """fp32 arithmetic whatever the inputs' dtype; each gradient in its input's dtype (as torch's losses)."""
    g = torch.Generator().manual_seed(9)
    p0, t0 = torch.randn(3, 5, 7, generator=g), torch.randn(3, 5, 7, generator=g)
    pred, target = p0.to(dtype), t0.to(tdtype)
    p32, t32 = pred.float().double(), target.float().double()
    cases = [
        ('l1', lambda p, t: A.L1LossFn.apply(p, t, 0.5), lambda p, t: 0.5 * (p - t).abs().mean()),
        ('mse', lambda p, t: A.PixelLossFn.apply(p, t, 0.5, 1, 0.0), lambda p, t: 0.5 * ((p - t) ** 2).mean()),
        ('charb', lambda p, t: A.PixelLossFn.apply(p, t, 0.5, 2, 1e-6),
         lambda p, t: 0.5 * torch.sqrt((p - t) ** 2 + float(f32(1e-6))).mean()),
        ('bce', lambda p, t: A.BCELogitsFn.apply(p, t, True, 0.5),
         lambda p, t: 0.5 * F.binary_cross_entropy_with_logits(p - t.mean(), torch.ones_like(p))),
        ('gan', lambda p, t: A.GanPointLossFn.apply(p, 1, 1.0, 0.5), lambda p, t: 0.5 * ((p - 1.0) ** 2).mean()),
    ]
    for name, hip, ref in cases:
        pd = pred.to(cuda).requires_grad_(True)
        td = target.to(cuda).requires_grad_(name == 'bce')
        loss = hip(pd, td)
        loss.backward()
        pr, tr = p32.clone().requires_grad_(True), t32.clone().requires_grad_(True)
        lr = ref(pr, tr)
        lr.backward()
        assert abs(float(loss) - float(lr)) <= 1e-5 * abs(float(lr)) + 1e-7, name
        assert pd.grad.dtype == dtype, name
        gtol = 2 ** -7 if dtype == torch.bfloat16 else 1e-5
        assert torch.allclose(pd.grad.cpu().double(), pr.grad, rtol=gtol, atol=1e-9), name
        if name == 'bce':
            assert td.grad.dtype == tdtype
            assert torch.allclose(td.grad.cpu().double(), tr.grad, rtol=1e-5, atol=1e-9)
    m = A.mean(pred.to(cuda))
    assert abs(float(m) - float(p32.mean())) <= 1e-6


# ------------------------------------------------------------------------------------------------------ Adam, EMA
def _adam_ref(p, m, v, g, step, lr, b1, b2, eps, wd, gs, mabs):
    g = g * gs
    if wd:
        g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    mabs = b1 * mabs + (1 - b1) * np.abs(g)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    upd = lr / bc1 * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return p - upd, m, v, mabs, np.abs(upd)


@pytest.mark.parametrize('step0', [1, 10000])
@pytest.mark.parametrize('wd,gs', [(0.0, 1.0), (0.01, 0.37)])
def test_adam_five_steps(cuda, lib, step0, wd, gs):
    n = 100003
    rng = np.random.default_rng(step0 + int(wd * 100))
    lr, b1, b2, eps = 2e-4, 0.9, 0.99, 1e-8
    c = [float(f32(a)) for a in (lr, b1, b2, eps, wd, gs)]
    p = rng.standard_normal(n).astype(f32)
    if step0 == 1:
        m, v = np.zeros(n, f32), np.zeros(n, f32)
    else:   # state of a long run
        m, v = (rng.standard_normal(n) * 1e-2).astype(f32), (rng.random(n) * 1e-4).astype(f32)
    pd, md, vd = _dev(p, cuda), _dev(m, cuda), _dev(v, cuda)
    P, M, V = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    mabs, upd_sum = np.abs(M), np.zeros(n)
    for k in range(5):
        g = (rng.standard_normal(n) * 1e-2).astype(f32)
        gd = _dev(g, cuda)
        _lib.check(lib.sr_adam_step_f32(_p(pd), _p(gd), _p(md), _p(vd), n, step0 + k, lr, b1, b2, eps, wd, gs, None, None,
                                        _st()), 'sr_adam_step_f32')
        P, M, V, mabs, upd = _adam_ref(P, M, V, g.astype(np.float64), step0 + k, *c, mabs)
        upd_sum += upd
    steps = 5
    gm, gv, gp = (a.cpu().numpy().astype(np.float64) for a in (md, vd, pd))
    assert (np.abs(gm - M) <= 4 * steps * EPS * mabs + FLT_MIN).all()
    assert (np.abs(gv - V) <= 6 * steps * EPS * V + FLT_MIN).all()
    # per step: p - upd rounds once (|p| + |upd|); upd carries ~16 roundings (m, v, sqrt, the bias corrections, eps, lr / bc1)
    assert (np.abs(gp - P) <= EPS * (2 * steps * np.abs(P) + 32 * upd_sum) + FLT_MIN).all()


@pytest.mark.parametrize('decay', [0.999, 0.5])
def test_ema_axpby(cuda, lib, decay):
    n = 100003
    rng = np.random.default_rng(3)
    d, s = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    a, b = float(f32(decay)), float(f32(1 - decay))
    dd = _dev(d, cuda)
    sd = _dev(s, cuda)
    _lib.check(lib.sr_axpby_f32(_p(dd), _p(sd), decay, 1 - decay, n, None, _st()), 'sr_axpby_f32')
    ref = a * d.astype(np.float64) + b * s.astype(np.float64)
    got = dd.cpu().numpy().astype(np.float64)
    assert (np.abs(got - ref) <= 2 * EPS * (np.abs(a * d) + np.abs(b * s)) + EPS * np.abs(ref)).all()


# ------------------------------------------------------------------------------------------------------ Linear (+ LeakyReLU)
@pytest.mark.parametrize('nin', [1, 255, 257, 8195])
@pytest.mark.parametrize('nout', [1, 100])
@pytest.mark.parametrize('nb', [1, 33])
def test_linear(cuda, lib, nin, nout, nb):
    slope = 0.2 if (nin + nout + nb) % 2 else 1.0
    with_bias = nin != 257
    rng = np.random.default_rng(nin * 1000 + nout + nb)
    x = rng.standard_normal((nb, nin)).astype(f32)
    w = (rng.standard_normal((nout, nin)) / math.sqrt(nin)).astype(f32)
    b = rng.standard_normal(nout).astype(f32) if with_bias else None
    ch_f = -(-nin // 256) + 9 + 2
    # the last input of every row: its product must outweigh four bounds on the rest of the row
    body = np.abs(x[:, :-1]).astype(np.float64) @ np.abs(w[:, :-1]).T.astype(np.float64) + (np.abs(b) if with_bias else 0)
    big = math.sqrt(8 * EPS * ch_f * float(body.max()) + 1.0) * 2
    x[:, -1] = big * np.where(np.arange(nb) % 2, 1, -1)
    w[:, -1] = big * np.where(np.arange(nout) % 3, 1, -1)
    X, W = x.astype(np.float64), w.astype(np.float64)
    z = X @ W.T + (b.astype(np.float64) if with_bias else 0)
    y_ref = np.where(z > 0, z, z * slope)
    zabs = np.abs(X) @ np.abs(W).T + (np.abs(b) if with_bias else 0)
    tol = EPS * (ch_f * zabs + np.abs(z))
    assert (np.abs(X[:, -1:] * W[:, -1][None, :]) > 4 * tol).all()
    xd, wd = _dev(x, cuda), _dev(w, cuda)
    bd = _dev(b, cuda) if with_bias else None
    y = torch.full((nb, nout), float('nan'), device=cuda)
    _lib.check(lib.sr_linear_fwd_f32(_p(xd), _p(wd), _p(bd), _p(y), nb, nin, nout, slope, _st()), 'sr_linear_fwd_f32')
    Y = y.cpu().numpy().astype(np.float64)
    assert (np.abs(Y - y_ref) <= tol).all(), float(np.abs(Y - y_ref).max())
    # backward; dz = dy * lrelu'(y) from the kernel's own y, so the slope branch is the kernel's
    dy = rng.standard_normal((nb, nout)).astype(f32)
    DZ = np.where(Y > 0, dy, dy * f32(slope)).astype(np.float64)
    dyd = _dev(dy, cuda)
    for want_dx, want_dw in ((True, True), (True, False), (False, True)):
        dz = torch.full((nb, nout), float('nan'), device=cuda)
        dx = torch.full((nb, nin), float('nan'), device=cuda) if want_dx else None
        dw = torch.full((nout, nin), float('nan'), device=cuda) if want_dw else None
        db = torch.full((nout,), float('nan'), device=cuda) if (want_dw and with_bias) else None
        _lib.check(lib.sr_linear_bwd_f32(_p(xd), _p(wd), _p(y), _p(dyd), nb, nin, nout, slope, _p(dz), _p(dx), _p(dw), _p(db), _st()),
                   'sr_linear_bwd_f32')
        assert np.array_equal(dz.cpu().numpy(), DZ.astype(f32))
        if want_dx:
            ref = DZ @ W
            assert (np.abs(dx.cpu().numpy() - ref) <= EPS * (nout + 1) * (np.abs(DZ) @ np.abs(W))).all()
        if want_dw:
            ref = DZ.T @ X
            assert (np.abs(dw.cpu().numpy() - ref) <= EPS * (nb + 1) * (np.abs(DZ).T @ np.abs(X))).all()
        if db is not None:
            assert (np.abs(db.cpu().numpy() - DZ.sum(0)) <= EPS * (nb + 1) * np.abs(DZ).sum(0)).all()


# ------------------------------------------------------------------------------------------------------ bilinear x2 on CB8
def _cb8_to_nchw(a):
    n, cb, h, w, _ = a.shape
    return a.permute(0, 1, 4, 2, 3).reshape(n, cb * 8, h, w)


@pytest.mark.parametrize('h', [1, 2, 3, 17])
@pytest.mark.parametrize('w', [1, 2, 3, 17])
def test_bilinear2x(cuda, lib, h, w):
    n, cb, gap = 3, 2, 40       # images sit `gap` floats apart: the batch stride is larger than the image
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(n, cb, h, w, 8, generator=g)
    gy = torch.randn(n, cb, 2 * h, 2 * w, 8, generator=g)
    si, so = cb * h * w * 8, cb * h * w * 32
    SENT = -12345.5

    def strided(t, stride):
        buf = torch.full((t.shape[0] * stride + gap,), SENT)
        for i in range(t.shape[0]):
            buf[i * stride:i * stride + t[i].numel()] = t[i].reshape(-1)
        return buf

    def unstride(buf, stride, shape):
        return torch.stack([buf[i * stride:i * stride + math.prod(shape[1:])].reshape(shape[1:]) for i in range(shape[0])])

    def gaps_intact(buf, stride, size):
        keep = torch.ones_like(buf, dtype=torch.bool)
        for i in range(n):
            keep[i * stride:i * stride + size] = False
        return bool((buf[keep] == SENT).all())

    src = strided(x, si + gap).to(cuda)
    dst = torch.full((n * (so + gap) + gap,), SENT, device=cuda)
    _lib.check(lib.sr_bilinear2x_fwd_f32(_p(src), si + gap, _p(dst), so + gap, n, cb, h, w, _st()), 'sr_bilinear2x_fwd_f32')
    dst = dst.cpu()
    assert gaps_intact(dst, so + gap, so)
    y = unstride(dst, so + gap, (n, cb, 2 * h, 2 * w, 8))
    xr = _cb8_to_nchw(x).double().requires_grad_(True)
    yr = F.interpolate(xr, scale_factor=2, mode='bilinear', align_corners=False)
    yabs = F.interpolate(_cb8_to_nchw(x).double().abs(), scale_factor=2, mode='bilinear', align_corners=False)
    assert ((_cb8_to_nchw(y).double() - yr.detach()).abs() <= 6 * EPS * yabs).all()
    gsrc_buf = strided(gy, so + gap).to(cuda)
    gx = torch.full((n * (si + gap) + gap,), SENT, device=cuda)
    _lib.check(lib.sr_bilinear2x_bwd_f32(_p(gsrc_buf), so + gap, _p(gx), si + gap, n, cb, h, w, _st()), 'sr_bilinear2x_bwd_f32')
    gx = gx.cpu()
    assert gaps_intact(gx, si + gap, si)
    yr.backward(_cb8_to_nchw(gy).double())
    xa = _cb8_to_nchw(x).double().requires_grad_(True)
    F.interpolate(xa, scale_factor=2, mode='bilinear', align_corners=False).backward(_cb8_to_nchw(gy).double().abs())
    got = _cb8_to_nchw(unstride(gx, si + gap, (n, cb, h, w, 8))).double()
    assert ((got - xr.grad).abs() <= 20 * EPS * xa.grad).all()


# ------------------------------------------------------------------------------------------------------ max-pool 2x2 on CB8
@pytest.mark.parametrize('h,w', [(2, 2), (5, 7), (16, 9), (33, 32)])
@pytest.mark.parametrize('content', ['random', 'relu', 'flat'])
def test_maxpool2x2_bit_exact(cuda, lib, h, w, content):
    n, cb = 2, 3
    g = torch.Generator().manual_seed(h * w)
    x = torch.randn(n, cb, h, w, 8, generator=g)
    if content == 'relu':           # post-ReLU, coarsely quantised: zeros and equal maxima in most windows
        x = torch.round(x * 2).clamp_min(0) / 2 + 0.0   # (+ 0.0: no negative zeros)
    elif content == 'flat':         # every window all-equal
        x = torch.full_like(x, 0.75)
    gy = torch.randn(n, cb, h // 2, w // 2, 8, generator=g)
    xd, gyd = x.to(cuda), gy.to(cuda)
    y = torch.full((n, cb, h // 2, w // 2, 8), float('nan'), device=cuda)
    dx = torch.full_like(xd, float('nan'))
    _lib.check(lib.sr_maxpool2x2_fwd_f32(_p(xd), _p(y), n, cb, h, w, _st()), 'sr_maxpool2x2_fwd_f32')
    _lib.check(lib.sr_maxpool2x2_bwd_f32(_p(xd), _p(gyd), _p(dx), n, cb, h, w, _st()), 'sr_maxpool2x2_bwd_f32')
    xr = _cb8_to_nchw(x).requires_grad_(True)
    yr, idx = F.max_pool2d(xr, 2, 2, return_indices=True)
    yr.backward(_cb8_to_nchw(gy))
    assert torch.equal(_cb8_to_nchw(y.cpu()), yr.detach())
    got = _cb8_to_nchw(dx.cpu())
    assert torch.equal(got, xr.grad)
    if h % 2:
        assert (got[:, :, -1, :] == 0).all()
    if w % 2:
        assert (got[:, :, :, -1] == 0).all()


# ------------------------------------------------------------------------------------------------------ spectral norm
SN_ROWS = [1, 63, 64, 511, 512, 1000]
SN_COLS = [1, 257, 4608]


def _sn_inputs(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(rows, cols, generator=g) / math.sqrt(cols)
    u = F.normalize(torch.randn(rows, generator=g), dim=0, eps=1e-12)
    v = F.normalize(torch.randn(cols, generator=g), dim=0, eps=1e-12)
    return W, u, v


def _sn_ref(W, u, v, update):
    """torch.nn.utils.spectral_norm (one power iteration) on a float64 copy."""
    lin = torch.nn.Linear(W.shape[1], W.shape[0], bias=False).double()
    with torch.no_grad():
        lin.weight.copy_(W.double())
    lin = torch.nn.utils.spectral_norm(lin, n_power_iterations=1, eps=1e-12)
    with torch.no_grad():
        lin.weight_u.copy_(u.double())
        lin.weight_v.copy_(v.double())
    lin.train(update)
    with torch.no_grad():
        lin(torch.zeros(1, W.shape[1], dtype=torch.float64))
    u, v = lin.weight_u.clone(), lin.weight_v.clone()
    return lin.weight.detach(), u, v, float(u @ (W.double() @ v))


def _sn_run(lib, cuda, W, u, v, update):
    rows, cols = W.shape
    Wd, ud, vd = W.to(cuda), u.clone().to(cuda), v.clone().to(cuda)
    w_sn, sigma = torch.full_like(Wd, float('nan')), _scal(np.nan, cuda)
    nb = (rows + 16 * cols) * 4
    ws = torch.zeros(nb, dtype=torch.uint8, device=cuda)
    _lib.check(lib.sr_spectral_norm_fwd_f32(_p(Wd), _p(ud), _p(vd), rows, cols, int(update), 1e-12, _p(w_sn), _p(sigma), _p(ws), nb,
                                            _st()), 'sr_spectral_norm_fwd_f32')
    return w_sn.cpu(), ud.cpu(), vd.cpu(), float(sigma.cpu())


@pytest.mark.parametrize('rows', SN_ROWS)
@pytest.mark.parametrize('cols', SN_COLS)
def test_spectral_norm_forward(cuda, lib, rows, cols):
    W, u, v = _sn_inputs(rows, cols, rows * 7 + cols)
    parts = 16 if rows >= 512 else 8 if rows >= 64 else 1
    chunk = -(-rows // parts)
    # bound of every stage relative to its result's scale: the W^T u column sums (chunk + parts), the two normalisations
    # (cols / 256 + rows / 256 + tree levels) and W v (cols / 256 + tree), times |W|-weighted condition numbers.  These bounds
    # are worst-case and loose for the largest layers; the batch test below pins the arithmetic bit for bit.
    W64, u64, v64 = W.double(), u.double(), v.double()
    t = W64.T @ u64
    kappa_t = float((W64.abs().T @ u64.abs()).max() / t.abs().max())
    for update in (True, False):
        w_sn, ug, vg, sigma = _sn_run(lib, cuda, W, u, v, update)
        rw, ru, rv, rsig = _sn_ref(W, u, v, update)
        if update:
            s = W64 @ rv
            kappa_s = float((W64.abs() @ rv.abs()).max() / s.abs().max())
            Lt = chunk + parts + 2 * (-(-cols // 256)) + 20
            Ls = 2 * (-(-cols // 256)) + 2 * (-(-rows // 256)) + 20
            dv = 4 * EPS * Lt * kappa_t * float(rv.abs().max())
            # u = normalize(W v): its own chain, plus v's error carried through the rows of W
            du = 4 * (EPS * Ls * kappa_s * float(s.abs().max()) + dv * float(W64.abs().sum(1).max())) / float(s.norm())
            assert float((vg.double() - rv).abs().max()) <= dv, 'v'
            assert float((ug.double() - ru).abs().max()) <= du, 'u'
            tsig = 2 * du / float(ru.abs().max())
        else:
            assert torch.equal(ug, u) and torch.equal(vg, v)   # eval: the buffers are left alone
            s = W64 @ v64
            Ls = -(-cols // 256) + -(-rows // 256) + 20
            tsig = 4 * EPS * Ls * float((W64.abs() @ v64.abs()).abs() @ u64.abs()) / abs(rsig)
        assert abs(sigma - rsig) <= tsig * abs(rsig), ('sigma', sigma, rsig)
        assert float(((w_sn.double() - rw).abs() / rw.abs().clamp_min(1e-30)).max()) <= tsig + 4 * EPS


def test_spectral_norm_batch_equals_single_layer_calls(cuda, lib):
    """The batched forward (one launch per stage for all layers) computes what the per-layer call does, bit for bit, for a mix
    of layers on both sides of each row-chunking threshold."""
    shapes = [(1, 257), (63, 4608), (64, 1), (511, 257), (512, 4608), (1000, 257), (512, 1), (64, 4608)]
    layers = [_sn_inputs(r, c, 100 + i) for i, (r, c) in enumerate(shapes)]
    for update in (True, False):
        singles = [_sn_run(lib, cuda, W, u, v, update) for W, u, v in layers]
        Ws = [W.to(cuda) for W, _, _ in layers]
        us = [u.clone().to(cuda) for _, u, _ in layers]
        vs = [v.clone().to(cuda) for _, _, v in layers]
        outs = [torch.full_like(W, float('nan')) for W in Ws]
        sig = torch.full((len(layers),), float('nan'), device=cuda)
        table = (_lib.SnLayer * len(layers))()
        need = 0
        for i, ((r, c), W) in enumerate(zip(shapes, Ws)):
            table[i].w_orig, table[i].u, table[i].v = W.data_ptr(), us[i].data_ptr(), vs[i].data_ptr()
            table[i].rows, table[i].cols = r, c
            table[i].w_sn, table[i].sigma = outs[i].data_ptr(), sig.data_ptr() + 4 * i
            need += ((r + 16 * c) * 4 + 255) // 256 * 256
        ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
        _lib.check(lib.sr_spectral_norm_fwd_batch_f32(table, len(layers), int(update), 1e-12, _p(ws), need, _st()),
                   'sr_spectral_norm_fwd_batch_f32')
        for i, (w_sn, ug, vg, sigma) in enumerate(singles):
            assert torch.equal(outs[i].cpu(), w_sn), (shapes[i], update)
            assert torch.equal(us[i].cpu(), ug) and torch.equal(vs[i].cpu(), vg), (shapes[i], update)
            assert float(sig[i].cpu()) == sigma, (shapes[i], update)


@pytest.mark.parametrize('rows,cols', [(1, 257), (64, 1), (512, 4608), (1000, 257)])
def test_spectral_norm_backward(cuda, lib, rows, cols):
    W, u, v = _sn_inputs(rows, cols, rows + cols)
    w_sn, ug, vg, sigma = _sn_run(lib, cuda, W, u, v, True)
    G = torch.randn(rows, cols, generator=torch.Generator().manual_seed(1))
    gd = torch.full((rows, cols), float('nan'), device=cuda)
    nb = lib.sr_reduce_workspace_bytes(8) + 64
    ws = torch.zeros(nb, dtype=torch.uint8, device=cuda)
    # (every device argument is held by a name until the launch: a temporary's memory could be handed to the next one)
    Gd, wd, ud, vd, sd = G.to(cuda), w_sn.to(cuda), ug.to(cuda), vg.to(cuda), _scal(sigma, cuda)
    _lib.check(lib.sr_spectral_norm_bwd_f32(_p(Gd), _p(wd), _p(ud), _p(vd), _p(sd), rows, cols, _p(gd), _p(ws), nb, _st()), 'sr_spectral_norm_bwd_f32')
    # d/dW of W / (u^T W v) with u, v held constant (torch's spectral_norm backward), from the forward's fp32 outputs
    u64, v64 = ug.double(), vg.double()
    dot = float((G.double() * w_sn.double()).sum())
    ref = (G.double() - dot * torch.outer(u64, v64)) / sigma
    n = rows * cols
    dot_err = EPS * _chain(n) * float((G.double() * w_sn.double()).abs().sum())
    tol = (EPS * (2 * G.double().abs() + 5 * abs(dot) * torch.outer(u64, v64).abs()) + dot_err * torch.outer(u64, v64).abs()) / sigma
    assert ((gd.cpu().double() - ref).abs() <= tol + FLT_MIN).all()
    # and the formula is torch's autograd of weight / sigma with the power-iteration vectors held fixed
    W64 = W.double().requires_grad_(True)
    wt = W64 / (u64 @ W64 @ v64)
    wt.backward(G.double())
    assert torch.allclose(ref, W64.grad, rtol=1e-4, atol=1e-6 * float(W64.grad.abs().max()))


# ------------------------------------------------------------------------------------------------------ bit-exact element-wise ops
@pytest.mark.parametrize('with_b', [True, False])
def test_channel_affine_bit_exact(cuda, lib, with_b):
    n, c, h, w = 3, 5, 7, 9
    g = torch.Generator().manual_seed(2)
    x, a, b = torch.randn(n, c, h, w, generator=g), torch.randn(c, generator=g), torch.randn(c, generator=g)
    y = torch.full_like(x, float('nan')).to(cuda)
    xd, ad, bd = x.to(cuda), a.to(cuda), b.to(cuda)
    _lib.check(lib.sr_channel_affine_f32(_p(xd), _p(y), _p(ad), _p(bd) if with_b else None, n, c, h * w, _st()),
               'sr_channel_affine_f32')
    ref = x * a.view(1, c, 1, 1)
    if with_b:
        ref = ref + b.view(1, c, 1, 1)
    assert torch.equal(y.cpu(), ref)


@pytest.mark.parametrize('slope', [0.2, 0.0])
def test_lrelu_bit_exact(cuda, lib, slope):
    n = 4097
    g = torch.Generator().manual_seed(4)
    x, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
    x[:5] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, float('inf')])
    xd, y, dx = x.to(cuda), torch.full((n,), float('nan'), device=cuda), torch.full((n,), float('nan'), device=cuda)
    _lib.check(lib.sr_lrelu_fwd_f32(_p(xd), _p(y), slope, n, _st()), 'sr_lrelu_fwd_f32')
    dyd = dy.to(cuda)
    _lib.check(lib.sr_lrelu_bwd_f32(_p(dyd), _p(y), _p(dx), slope, n, _st()), 'sr_lrelu_bwd_f32')
    s = torch.tensor(slope, dtype=torch.float32)
    yr = torch.where(x > 0, x, x * s)
    assert torch.equal(y.cpu(), yr)
    assert torch.equal(dx.cpu(), torch.where(yr > 0, dy, dy * s))


def test_add_bit_exact_and_rejects_ragged_length(cuda, lib):
    n = 4096 + 4
    g = torch.Generator().manual_seed(6)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    out = torch.full((n,), float('nan'), device=cuda)
    ad, bd = a.to(cuda), b.to(cuda)
    _lib.check(lib.sr_add_f32(_p(ad), _p(bd), _p(out), n, _st()), 'sr_add_f32')
    assert torch.equal(out.cpu(), a + b)
    out2 = torch.full((8,), -7.0, device=cuda)
    rc = lib.sr_add_f32(_p(ad), _p(bd), _p(out2), 6, _st())
    torch.cuda.synchronize()
    assert rc != 0
    assert (out2.cpu() == -7.0).all()


# ------------------------------------------------------------------------------------------------------ PSNR / SSIM
def _content(kind, shape, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'noise':
        gt = torch.rand(shape, generator=g)
        return (gt + 0.08 * torch.randn(shape, generator=g)).clamp(0, 1), gt
    if kind in ('bright', 'dark'):     # smooth content, one grey level of difference (sky / walls; shadows)
        base, sd = (240.0, 1.0) if kind == 'bright' else (12.0, 2.0)
        gt = (base + sd * torch.randn(shape, generator=g)).round().clamp(0, 255)
        sr = (gt + torch.randint(0, 2, shape, generator=g) * 2 - 1).clamp(0, 255)
        return sr / 255, gt / 255
    if kind == 'outside':              # values outside [0, 1] (clamped by tensor2img)
        return torch.rand(shape, generator=g) * 1.6 - 0.3, torch.rand(shape, generator=g) * 1.6 - 0.3
    if kind == 'halves':               # x * 255 == k + 0.5 exactly in fp32 (round half to even, as np.round)
        k = torch.randint(0, 255, shape, generator=g).float()
        v = ((k + 0.5) / 255).float()
        for _ in range(4):             # walk to an fp32 value whose fp32 product with 255 is exactly k + 0.5
            p = v * 255
            v = torch.where(p > k + 0.5, torch.nextafter(v, torch.zeros_like(v)),
                            torch.where(p < k + 0.5, torch.nextafter(v, torch.ones_like(v)), v))
        assert (v * 255 == k + 0.5).float().mean() > 0.5
        return v, (k + torch.randint(0, 3, shape, generator=g).float() - 1).clamp(0, 255) / 255
    raise ValueError(kind)


def _host_metrics(sr, gt, crop):
    from image_restoration_amd.metrics import calculate_psnr, calculate_ssim
    from image_restoration_amd.utils.img_util import tensor2img
    ps, ss = [], []
    for i in range(sr.shape[0]):
        a, b = tensor2img(sr[i:i + 1], rgb2bgr=True, min_max=(0, 1)), tensor2img(gt[i:i + 1], rgb2bgr=True, min_max=(0, 1))
        ps.append(calculate_psnr(a, b, crop))
        ss.append(calculate_ssim(a, b, crop))
    return ps, ss


@pytest.mark.parametrize('kind', ['noise', 'bright', 'dark', 'outside', 'halves', 'identical'])
@pytest.mark.parametrize('crop', [0, 4])
@pytest.mark.parametrize('side', ['min', 'mid'])
def test_psnr_ssim_device(cuda, kind, crop, side):
    from image_restoration_amd.metrics import psnr_device, ssim_device
    h = w = 2 * crop + 11 if side == 'min' else None
    if side == 'mid':
        h, w = 2 * crop + 61, 2 * crop + 90
    shape = (3, 3, h, w)
    sr, gt = _content('noise' if kind == 'identical' else kind, shape, h * 31 + crop)
    if kind == 'identical':
        sr = gt.clone()
    p_dev, s_dev = psnr_device(sr.to(cuda), gt.to(cuda), crop), ssim_device(sr.to(cuda), gt.to(cuda), crop)
    p_ref, s_ref = _host_metrics(sr, gt, crop)
    count = 3 * (h - 2 * crop) * (w - 2 * crop)
    for i in range(3):
        if kind == 'identical':
            assert p_dev[i] == float('inf') and p_ref[i] == float('inf')
            assert abs(s_dev[i] - 1.0) <= 1e-6
            continue
        # integer squared errors summed in fp32: relative chain bound of the 64-part reduction, in dB
        chain = -(-count // (256 * 64)) + 9 + 64
        assert abs(p_dev[i] - p_ref[i]) <= 10 / math.log(10) * EPS * chain + 1e-9, (kind, i, p_dev[i], p_ref[i])
        assert abs(s_dev[i] - s_ref[i]) <= 1e-6, (kind, i, s_dev[i], s_ref[i])


def test_ssim_device_bright_smooth_large_image(cuda):
    from image_restoration_amd.metrics import ssim_device
    sr, gt = _content('bright', (1, 3, 264, 392), 77)
    _, s_ref = _host_metrics(sr, gt, 4)
    assert abs(ssim_device(sr.to(cuda), gt.to(cuda), 4)[0] - s_ref[0]) <= 1e-6
