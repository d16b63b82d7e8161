"""RIDNet on the MI355X: the new kernels (ridnet_ops.hip, include/sr_hip_ridnet.h) against float64 on the CPU, and the network
(forward, backward, frozen parameters, FlatAdam arena, checkpoint, tiling, inference script, SRModel training) against the
reference's own results in tests/golden/g_w_ridnet.npz (tools/make_golden_ridnet.py)."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_restoration_amd as ira
from image_restoration_amd import _lib, hip_ops
from image_restoration_amd.utils import synth

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24   # unit roundoff of fp32


def _st():
    return torch.cuda.current_stream().cuda_stream


def _profiled(lib, fn, cap=4096):
    _lib.check(lib.sr_profile_start(cap), 'sr_profile_start')
    try:
        fn()
    finally:
        recs = (_lib.LaunchRecord * cap)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, cap, C.byref(cnt)), 'sr_profile_stop')
    return [recs[i] for i in range(min(cnt.value, cap))]


def _to_cb8(x, dev, extra_front=0, extra_back=0):
    """NCHW CPU tensor (channels a multiple of 8) -> a CB8 channel slice of a wider NaN-padded buffer (exercises the strides)."""
    n, c, h, w = x.shape
    cb = c // 8
    buf = torch.full((n, cb + extra_front + extra_back, h, w, 8), float('nan'), dtype=torch.float32)
    buf[:, extra_front:extra_front + cb] = x.float().reshape(n, cb, 8, h, w).permute(0, 1, 3, 4, 2)
    return hip_ops.CB8(buf.to(dev)).slice(8 * extra_front, c)


def _from_cb8(t, c=None):
    b = t.buf[:, t.cb0:t.cb0 + t.cbn]
    return b.permute(0, 1, 4, 2, 3).reshape(t.n, t.channels, t.h, t.w)[:, :c].cpu()


def _within(got, want, bound, what):
    err = (got.double() - want.double()).abs()
    ok = err <= bound + 1e-30
    assert bool(ok.all()), (what, float(err.max()), float((err / (bound + 1e-30)).max()))


# --------------------------------------------------------------------------------------------------------- the convolutions
# (ksize, dilation, cin, cout, n, h, w): H, W in {1, d, 2d+1, 33x65, 97x131}; cin 8 / 64 / 128, cout 8 / 64
CONV_CASES = [(3, 2, 8, 8, 1, 1, 1), (3, 2, 64, 64, 2, 2, 5), (3, 3, 64, 8, 3, 7, 3), (3, 4, 128, 64, 1, 9, 4), (3, 4, 64, 64, 2, 33, 65),
              (3, 3, 128, 64, 1, 97, 131), (3, 2, 64, 8, 2, 97, 131), (3, 1, 64, 64, 2, 33, 65), (1, 1, 64, 64, 2, 33, 65),
              (1, 1, 128, 8, 3, 1, 1), (1, 1, 8, 64, 1, 97, 131)]


def _rand(shape, g, scale=1.0):
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


def _conv64(x, w, b, d):
    k = w.shape[2]
    return F.conv2d(x.double(), w.double(), None if b is None else b.double(), padding=d * (k - 1) // 2, dilation=d)


def _bound(x, w, b, d, extra=0):
    """fp32 bound of a k*k*cin-term dot product summed in one chain (the MFMA accumulator) plus bias and epilogue ops:
    (K + 4 + extra) u * sum |terms|."""
    k = w.shape[2]
    K = k * k * w.shape[1]
    return (K + 4 + extra) * U32 * _conv64(x.abs(), w.abs(), None if b is None else b.abs(), d)


@pytest.mark.parametrize('k,d,cin,cout,n,h,w', CONV_CASES)
def test_convd_forward_matches_float64(cuda, k, d, cin, cout, n, h, w):
    """Forward of the dilated / 1x1 conv against F.conv2d(dilation=d) in float64 on channel slices of NaN-padded buffers, with
    the conv3x3 epilogue (LeakyReLU, alpha, res1, res2), the post-add ReLU (act(conv + b + res1)) and out_pre."""
    g = torch.Generator().manual_seed(k * 1000 + d * 100 + cin + cout + h * 7 + w)
    x = _rand((n, cin, h, w), g)
    wt = _rand((cout, cin, k, k), g, (1.0 / (cin * k * k)) ** 0.5)
    bias = _rand((cout,), g, 0.1)
    cp = (cout + 7) // 8 * 8
    r1, r2 = _rand((n, cp, h, w), g), _rand((n, cp, h, w), g)
    xd = _to_cb8(x, cuda, 1, 1)
    pc = hip_ops.PackedConvK(wt.float().to(cuda), bias.float().to(cuda))
    if k == 3:   # the 3x3 image of sr_conv3x3_pack_f32 is the same
        pc3 = hip_ops.PackedConv(wt.float().to(cuda), bias.float().to(cuda))
        assert torch.equal(pc.w, pc3.w) and torch.equal(pc.b, pc3.b)
    conv = _conv64(x.float(), wt.float(), bias.float(), d)
    base_b = _bound(x, wt, bias, d)
    R1, R2 = _to_cb8(r1, cuda, 0, 1), _to_cb8(r2, cuda, 1, 0)
    r1c, r2c = r1[:, :cout].float().double(), r2[:, :cout].float().double()
    # conv3x3 epilogue: alpha * lrelu(conv + b) + beta1 * res1 + beta2 * res2, and out_pre = alpha * lrelu(conv + b)
    pre = hip_ops.CB8(torch.full((n, cp // 8 + 1, h, w, 8), float('nan'), device=cuda)).slice(8, cp)
    out = hip_ops.convd(xd, pc, d, act_slope=0.2, alpha=0.5, res1=R1, beta1=0.75, res2=R2, beta2=-1.25, out_pre=pre)
    want_pre = 0.5 * F.leaky_relu(conv, 0.2)
    want = want_pre + 0.75 * r1c - 1.25 * r2c
    _within(_from_cb8(pre, cout), want_pre, base_b, 'out_pre')
    _within(_from_cb8(out, cout), want, base_b + 4 * U32 * (want_pre.abs() + r1c.abs() + r2c.abs()), 'epilogue')
    # post-add ReLU: relu(conv + b + res1)
    out = hip_ops.convd(xd, pc, d, post_act=True, act_slope=0.0, res1=R1, beta1=1.0)
    want = torch.relu(conv + r1c)
    _within(_from_cb8(out, cout), want, base_b + 2 * U32 * r1c.abs(), 'post_act')
    torch.cuda.synchronize()


@pytest.mark.parametrize('k,d,cin,cout,n,h,w', CONV_CASES)
def test_convd_data_gradient_matches_float64(cuda, k, d, cin, cout, n, h, w):
    """Data gradient (mode-1 image, flipped taps) against autograd's conv2d input gradient in float64, with accumulate and a
    ReLU mask (mask_src, slope 0)."""
    g = torch.Generator().manual_seed(k * 2000 + d * 100 + cin + cout + h * 3 + w)
    wt = _rand((cout, cin, k, k), g, (1.0 / (cin * k * k)) ** 0.5)
    dy = _rand((n, cout, h, w), g)
    old = _rand((n, cin, h, w), g)
    msk = _rand((n, cin, h, w), g)
    dyp = torch.zeros(n, (cout + 7) // 8 * 8, h, w, dtype=torch.float64)
    dyp[:, :cout] = dy
    pc = hip_ops.PackedConvK(wt.float().to(cuda), None, mode=1)
    if k == 3:
        assert torch.equal(pc.w, hip_ops.PackedConv(wt.float().to(cuda), None, mode=1).w)
    x = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
    _conv64(x, wt.float(), None, d).backward(dy.float().double())
    dx = x.grad
    ad = torch.zeros_like(x)
    ad2 = x.detach().clone().requires_grad_(True)
    _conv64(ad2, wt.float().abs(), None, d).backward(dy.float().double().abs())
    bnd = (k * k * cout + 4) * U32 * ad2.grad
    out_t = _to_cb8(old, cuda, 1, 0)
    got = hip_ops.convd(_to_cb8(dyp, cuda, 0, 1), pc, d, out=out_t, accumulate=True, mask=_to_cb8(msk, cuda), mask_slope=0.0)
    o = old.float().double()
    want = torch.where(msk.float() > 0, dx + o, torch.zeros_like(dx))
    _within(_from_cb8(got, cin), want, bnd + 2 * U32 * (dx.abs() + o.abs()), 'dgrad')
    del ad


@pytest.mark.parametrize('k,d,cin,cout,n,h,w', CONV_CASES)
def test_convd_weight_gradient_matches_float64_and_is_bit_reproducible(cuda, k, d, cin, cout, n, h, w):
    """dW / db against float64 (bound from the slab summation: one fp32 chain over the pixels of a workgroup, then the
    splits in two fixed-order stages), two launches bit-identical, and the arena form adds into existing values."""
    g = torch.Generator().manual_seed(k * 3000 + d * 100 + cin + cout + h * 5 + w)
    x = _rand((n, cin, h, w), g)
    dy = _rand((n, cout, h, w), g)
    dyp = torch.zeros(n, (cout + 7) // 8 * 8, h, w, dtype=torch.float64)
    dyp[:, :cout] = dy
    xd, dyd = _to_cb8(x, cuda, 1, 0), _to_cb8(dyp, cuda, 0, 1)
    dw, db = hip_ops.convd_wgrad(xd, dyd, cout, cin, k, d)
    dw2, db2 = hip_ops.convd_wgrad(xd, dyd, cout, cin, k, d)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    xf, dyf = x.float().double(), dy.float().double()
    wt = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    _conv64(xf, wt, None, d).backward(dyf)
    wa = torch.zeros_like(wt, requires_grad=True)
    _conv64(xf.abs(), wa, None, d).backward(dyf.abs())
    P = n * h * w
    _within(dw.cpu(), wt.grad, (P + 64) * U32 * wa.grad, 'dW')
    _within(db.cpu(), dyf.sum((0, 2, 3)), (P + 64) * U32 * dyf.abs().sum((0, 2, 3)), 'db')
    acc_w, acc_b = torch.ones_like(dw), torch.ones_like(db)
    hip_ops.convd_wgrad(xd, dyd, cout, cin, k, d, out=(acc_w.data_ptr(), acc_b.data_ptr()))
    assert torch.allclose(acc_w, dw + 1, rtol=0, atol=4 * U32 * float((dw.abs() + 1).max()))
    assert torch.allclose(acc_b, db + 1, rtol=0, atol=4 * U32 * float((db.abs() + 1).max()))


@pytest.mark.parametrize('cin,cout,n,h,w', [(64, 64, 2, 33, 65), (128, 64, 1, 97, 131), (8, 8, 3, 9, 40), (64, 8, 1, 1, 1)])
def test_dilation_one_equals_conv3x3_bit_for_bit(cuda, cin, cout, n, h, w):
    """A dilation-1 3x3 call of the new path and sr_conv3x3_f32 run the same MFMA chain per output (chunk by chunk, tap by tap)
    and the same epilogue operations in the same order: bit-identical, forward and data gradient."""
    g = torch.Generator().manual_seed(cin + cout + h + w)
    x = _rand((n, cin, h, w), g)
    wt = _rand((cout, cin, 3, 3), g, (1.0 / (cin * 9)) ** 0.5).float().to(cuda)
    bias = _rand((cout,), g, 0.1).float().to(cuda)
    cp = (cout + 7) // 8 * 8
    r1 = _to_cb8(_rand((n, cp, h, w), g), cuda)
    xd = _to_cb8(x, cuda, 1, 0)
    pc = hip_ops.PackedConv(wt, bias)
    a = hip_ops.conv3x3(xd, pc, act_slope=0.0, res1=r1, beta1=1.0)
    b = hip_ops.convd(xd, pc, 1, act_slope=0.0, res1=r1, beta1=1.0)
    assert torch.equal(_from_cb8(a, cout), _from_cb8(b, cout))
    dy = _to_cb8(_rand((n, cp, h, w), g), cuda)
    pm = hip_ops.PackedConv(wt, None, mode=1)
    msk = _to_cb8(_rand((n, cin, h, w), g), cuda)
    a = hip_ops.conv3x3(dy, pm, mask=msk, mask_slope=0.0)
    b = hip_ops.convd(dy, pm, 1, mask=msk, mask_slope=0.0)
    assert torch.equal(_from_cb8(a), _from_cb8(b))


def test_profiler_counts_the_one_by_one_conv_as_one_tap(cuda):
    lib = _lib.load()
    x = hip_ops.CB8.zeros(2, 64, 16, 40, cuda)
    pc1 = hip_ops.PackedConvK(torch.zeros(64, 64, 1, 1, device=cuda), torch.zeros(64, device=cuda))
    pc3 = hip_ops.PackedConvK(torch.zeros(8, 64, 3, 3, device=cuda), torch.zeros(8, device=cuda))
    recs = _profiled(lib, lambda: (hip_ops.convd(x, pc1, 1), hip_ops.convd(x, pc3, 4)))
    assert [r.kernel_id for r in recs] == [82, 81]
    assert recs[0].flops == 2 * 64 * 64 * 2 * 16 * 40 and recs[1].flops == 2 * 9 * 64 * 8 * 2 * 16 * 40
    assert lib.sr_kernel_name(81) == b'convd_f32_kernel' and lib.sr_kernel_name(84) == b'wgradd_f32_kernel'


def test_convd_argument_errors_are_codes(cuda):
    lib = _lib.load()
    x = hip_ops.CB8.zeros(1, 8, 4, 4, cuda)
    pc = hip_ops.PackedConvK(torch.zeros(8, 8, 3, 3, device=cuda))
    for dil in (0, 5):
        with pytest.raises(_lib.SrHipError):
            hip_ops.convd(x, pc, dil)
    with pytest.raises(_lib.SrHipError):
        hip_ops.convd(x, pc, 2, post_act=True, out_pre=hip_ops.CB8.zeros(1, 8, 4, 4, cuda))
    assert lib.sr_convk_packed_weight_floats(8, 8, 2, 0) == 0
    assert lib.sr_convd_wgrad_slab_bytes(1, 4, 4, 8, 8, 3, 0) == 0
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------- the small passes
@pytest.mark.parametrize('n,h,w', [(1, 1, 1), (2, 5, 13), (3, 70, 97)])
def test_mean_shift_ends_match_float64(cuda, n, h, w):
    """sub_mean / add_mean forward and both adjoints (dW, db, dx with the global residual, dt) against float64; dW / db are
    bit-identical across launches and add into an arena."""
    g = torch.Generator().manual_seed(n * 100 + h + w)
    x = torch.rand(n, 3, h, w, generator=g, dtype=torch.float64).float()
    W = (torch.eye(3, dtype=torch.float64) + 0.05 * _rand((3, 3), g)).float().view(3, 3, 1, 1)
    b = (_rand((3,), g) * 100).float()
    xd, Wd, bd = x.to(cuda), W.to(cuda), b.to(cuda)
    W2 = W.double()[:, :, 0, 0]
    s = hip_ops.ridnet_sub_mean(xd, Wd, bd)
    want = torch.einsum('ck,nkhw->nchw', W2, x.double()) + b.double()[None, :, None, None]
    sb = 4 * U32 * (torch.einsum('ck,nkhw->nchw', W2.abs(), x.double().abs()) + b.double().abs()[None, :, None, None])
    got = _from_cb8(s)
    _within(got[:, :3], want, sb, 'sub_mean')
    assert torch.equal(got[:, 3:], torch.zeros_like(got[:, 3:]))
    t = _rand((n, 8, h, w), g) * 50
    t[:, 3:] = float('nan')            # channels 3..7 of the tail output are never read
    td = _to_cb8(t, cuda, 1, 0)
    y = hip_ops.ridnet_add_mean(xd, td, Wd, bd)
    t3 = t[:, :3].float().double()
    mix = torch.einsum('ck,nkhw->nchw', W2, t3) + b.double()[None, :, None, None]
    _within(y.cpu(), x.double() + mix, 5 * U32 * (x.double().abs() + torch.einsum('ck,nkhw->nchw', W2.abs(), t3.abs())
                                                   + b.double().abs()[None, :, None, None]), 'add_mean')
    gy = _rand((n, 3, h, w), g).float()
    gs = _rand((n, 8, h, w), g)
    dW, db = torch.empty(3, 3, 1, 1, device=cuda), torch.empty(3, device=cuda)
    dt = hip_ops.ridnet_add_mean_bwd(gy.to(cuda), td, Wd, dW.data_ptr(), db.data_ptr())
    g64 = gy.double()
    P = n * h * w
    _within(dW.cpu()[:, :, 0, 0], torch.einsum('nchw,nkhw->ck', g64, t3),
            (P + 80) * U32 * torch.einsum('nchw,nkhw->ck', g64.abs(), t3.abs()), 'add dW')
    _within(db.cpu(), g64.sum((0, 2, 3)), (P + 80) * U32 * g64.abs().sum((0, 2, 3)), 'add db')
    dtw = torch.einsum('ck,nchw->nkhw', W2, g64)
    dtc = _from_cb8(dt)
    _within(dtc[:, :3], dtw, 4 * U32 * torch.einsum('ck,nchw->nkhw', W2.abs(), g64.abs()), 'dt')
    assert torch.equal(dtc[:, 3:], torch.zeros_like(dtc[:, 3:]))
    gsd = _to_cb8(gs, cuda, 0, 1)
    dW2, db2 = torch.empty_like(dW), torch.empty_like(db)
    res = _rand((n, 3, h, w), g).float()
    dx = hip_ops.ridnet_sub_mean_bwd(xd, gsd, Wd, dW2.data_ptr(), db2.data_ptr(), want_dx=True, dx_res=res.to(cuda))
    gs3 = gs[:, :3].float().double()
    _within(dW2.cpu()[:, :, 0, 0], torch.einsum('nchw,nkhw->ck', gs3, x.double()),
            (P + 80) * U32 * torch.einsum('nchw,nkhw->ck', gs3.abs(), x.double().abs()), 'sub dW')
    _within(db2.cpu(), gs3.sum((0, 2, 3)), (P + 80) * U32 * gs3.abs().sum((0, 2, 3)), 'sub db')
    _within(dx.cpu(), torch.einsum('ck,nchw->nkhw', W2, gs3) + res.double(),
            5 * U32 * (torch.einsum('ck,nchw->nkhw', W2.abs(), gs3.abs()) + res.double().abs()), 'dx')
    acc = dW2.clone()
    hip_ops.ridnet_sub_mean_bwd(xd, gsd, Wd, acc.data_ptr(), None, accumulate=True)
    again = torch.empty_like(dW2)
    hip_ops.ridnet_sub_mean_bwd(xd, gsd, Wd, again.data_ptr(), None)
    assert torch.equal(again, dW2) and torch.equal(acc, dW2 + dW2)


def test_attention_scale_and_relu_mask(cuda):
    g = torch.Generator().manual_seed(9)
    u = _rand((2, 64, 9, 11), g)
    s = torch.rand(2, 64, generator=g)
    ud = _to_cb8(u, cuda, 1, 1)
    out = hip_ops.ca_scale(ud, s.to(cuda))
    assert torch.equal(_from_cb8(out), (u.float() * s[:, :, None, None]))
    m = _rand((2, 64, 9, 11), g)
    got = hip_ops.relu_mask(ud, _to_cb8(m, cuda, 0, 1))
    assert torch.equal(_from_cb8(got), torch.where(m.float() > 0, u.float(), torch.zeros_like(u.float())))


# --------------------------------------------------------------------------------------------------------- the network
SMALL_CFG = dict(in_channels=3, mid_channels=16, out_channels=3, num_block=2)


def _load(net, sd, dev):
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return net.to(dev)


def _small(i, dev):
    return _load(ira.build_network(dict(type='RIDNet', **SMALL_CFG)), synth.ridnet_state_dict(400 + i, **SMALL_CFG), dev)


def _gy(g, i):
    x = g[f'fwd{i}_x']
    gy = synth.gaussian(int(g[f'fwd{i}_gy_seed']), x.shape)
    assert hashlib.sha256(gy.tobytes()).hexdigest() == str(g[f'fwd{i}_gy_sha256'])
    return torch.from_numpy(gy)


def _fwd_tol(g, i):
    """Features are in the hundreds (inputs in [0, 1] minus 255 * mean, as in the reference), so the output carries fp32
    rounding of that size: 10x the reference's own float32 distance from float64, and never below 1e-4."""
    return max(1e-4, 10 * float(g[f'fwd{i}_y32_err']))


@pytest.mark.parametrize('i', [0, 1])
def test_forward_matches_the_reference(cuda, golden, i):
    g = golden('g_w_ridnet')
    net = _small(i, cuda).eval()
    with torch.no_grad():
        y = net(torch.from_numpy(g[f'fwd{i}_x']).to(cuda)).cpu().numpy()
    assert y.shape == g[f'fwd{i}_y'].shape
    err = np.abs(y - g[f'fwd{i}_y']).max()
    assert err < _fwd_tol(g, i), (err, float(g[f'fwd{i}_y32_err']))


def test_default_net_forward_matches_the_reference(cuda, golden):
    g = golden('g_w_ridnet')
    cfg = dict(in_channels=3, mid_channels=64, out_channels=3)
    sd = synth.ridnet_state_dict(int(g['big_seed']), **cfg)
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v, np.float32).tobytes())
    assert h.hexdigest() == str(g['big_weights_sha256'])
    net = _load(ira.build_network(dict(type='RIDNet', **cfg)), sd, cuda).eval()
    with torch.no_grad():
        y = net(torch.from_numpy(g['big_x']).to(cuda)).cpu().numpy()
    assert y.shape == (1, 3, 12, 16)
    assert np.abs(y - g['big_y']).max() < 2e-4


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _grad_bound(g, i):
    """1e-4 relative L2; 1e-3 where the fixture's float64 run has a ReLU pre-activation within 1e-4 of zero (inside fp32
    rounding of features in the hundreds, a mask element may flip)."""
    return 1e-4 if g[f'fwd{i}_relu_margin'].min() > 1e-4 else 1e-3


@pytest.mark.parametrize('i', [0, 1])
def test_backward_matches_the_reference(cuda, golden, i):
    """dL/dx and every parameter gradient, the two MeanShift layers' full 3x3 mixes and biases included."""
    g = golden('g_w_ridnet')
    net = _small(i, cuda).train()
    x = torch.from_numpy(g[f'fwd{i}_x']).to(cuda).requires_grad_(True)
    y = net(x)
    y.backward(_gy(g, i).to(cuda))
    tol = _grad_bound(g, i)
    assert np.abs(y.detach().cpu().numpy() - g[f'fwd{i}_y']).max() < _fwd_tol(g, i)
    assert _rel_l2(x.grad.cpu(), g[f'fwd{i}_dx64']) < tol
    names = sorted(k[len(f'fwd{i}_grad64.'):] for k in g if k.startswith(f'fwd{i}_grad64.'))
    assert sorted(k for k, _ in net.named_parameters()) == names
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        assert _rel_l2(p.grad.cpu(), g[f'fwd{i}_grad64.{k}']) < tol, (k, _rel_l2(p.grad.cpu(), g[f'fwd{i}_grad64.{k}']))
    assert np.count_nonzero(g[f'fwd{i}_grad64.sub_mean.weight']) == 9


def test_backward_with_frozen_parameters_and_no_input_grad(cuda, golden):
    g = golden('g_w_ridnet')
    net = _small(0, cuda).train()
    x = torch.from_numpy(g['fwd0_x']).to(cuda)
    gy = _gy(g, 0).to(cuda)
    net(x).backward(gy)
    full = {k: p.grad.clone() for k, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    frozen = ('sub_mean.', 'body.0.merge.dilation2.', 'body.1.block2.body.4.', 'body.1.ca.attention.3.')
    for k, p in net.named_parameters():
        p.requires_grad_(not k.startswith(frozen))
    net(x).backward(gy)
    for k, p in net.named_parameters():
        if k.startswith(frozen):
            assert p.grad is None, k
        else:
            assert torch.equal(p.grad, full[k]), k
    for p in net.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        assert not net(x).requires_grad


def test_flat_adam_arena_receives_the_gradients(cuda, golden):
    from image_restoration_amd import optim
    g = golden('g_w_ridnet')
    x = torch.from_numpy(g['fwd1_x']).to(cuda)
    gy = _gy(g, 1).to(cuda)
    ref = _small(1, cuda).train()
    ref(x).backward(gy)
    net = _small(1, cuda).train()
    adam = optim.FlatAdam(list(net.parameters()), lr=1e-4, betas=(0.9, 0.99), modules=[net])
    assert net._grad_sink is not None
    adam.zero_grad()
    net(x).backward(gy)
    for (k, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    adam.step()
    with torch.no_grad():
        y_after = net(x)
        twin = _small(1, cuda).eval()
        twin.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
        assert torch.equal(y_after, twin(x))


def test_checkpoint_loads_strict_and_reproduces_the_fixture(cuda, golden, tmp_path):
    from image_restoration_amd.utils.checkpoint import load_generator_weights
    g = golden('g_w_ridnet')
    path = tmp_path / 'net_g.pth'
    torch.save({'params': {k: torch.from_numpy(v) for k, v in synth.ridnet_state_dict(401, **SMALL_CFG).items()}}, path)
    net = ira.build_network(dict(type='RIDNet', **SMALL_CFG))
    load_generator_weights(net, str(path), strict=True)
    net = net.to(cuda).eval()
    with torch.no_grad():
        y = net(torch.from_numpy(g['fwd1_x']).to(cuda)).cpu().numpy()
    assert np.abs(y - g['fwd1_y']).max() < _fwd_tol(g, 1)


def test_single_tile_equals_the_whole_image(cuda):
    """Attention statistics are per tile, so only a tile that covers the image reproduces the untiled forward (bit for bit)."""
    from image_restoration_amd.tiling import tiled_forward
    net = _small(0, cuda).eval()
    x = torch.rand(1, 3, 21, 26, generator=torch.Generator().manual_seed(5)).to(cuda)
    with torch.no_grad():
        whole = net(x)
        tiled = tiled_forward(net, x, tile=32, pad=4, scale=1)
        assert tiled.shape == (1, 3, 21, 26) and torch.equal(tiled, whole)
        assert tiled_forward(net, x, tile=12, pad=4, scale=1).shape == (1, 3, 21, 26)


def test_inference_script_ridnet(cuda, tmp_path):
    from image_restoration_amd import inference
    rng = np.random.default_rng(3)
    src = tmp_path / 'noisy.png'
    inference.imwrite_bgr(str(src), rng.integers(0, 256, (20, 28, 3), dtype=np.uint8))
    ck = tmp_path / 'net_g.pth'
    torch.save({'params': {k: torch.from_numpy(v) for k, v in synth.ridnet_state_dict(402, **SMALL_CFG).items()}}, ck)
    common = ['--input', str(src), '--model_path', str(ck), '--arch', 'RIDNet', '--scale', '1', '--num_feat', '16', '--num_block', '2']
    inference.main(common + ['--output', str(tmp_path / 'out.png')])
    out = inference.imread_bgr(str(tmp_path / 'out.png'))
    assert out.shape == (20, 28, 3)
    net = _load(ira.build_network(dict(type='RIDNet', **SMALL_CFG)), synth.ridnet_state_dict(402, **SMALL_CFG), cuda).eval()
    img = inference.imread_bgr(str(src))[:, :, ::-1].astype(np.float32) / 255.
    with torch.no_grad():
        y = net(torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)))[None].to(cuda))[0].clamp_(0, 1).cpu().numpy()
    want = (y.transpose(1, 2, 0)[:, :, ::-1] * 255.0).round().astype(np.uint8)
    assert np.abs(out.astype(int) - want.astype(int)).max() <= 1
    inference.main(common + ['--output', str(tmp_path / 'tiled.png'), '--tile', '16', '--tile_pad', '4'])
    assert inference.imread_bgr(str(tmp_path / 'tiled.png')).shape == (20, 28, 3)


# ------------------------------------------------------------------------------------------------------------------- training
def _train_opt():
    from collections import OrderedDict as OD
    opt = OD(name='golden', model_type='SRModel', scale=1, num_gpu=1, manual_seed=0, is_train=True, dist=False, rank=0, world_size=1)
    opt['network_g'] = OD(type='RIDNet', **SMALL_CFG)
    opt['path'] = OD(pretrain_network_g=None, strict_load_g=True, resume_state=None)
    tr = OD(ema_decay=0.9)
    tr['optim_g'] = OD(type='Adam', lr=1e-4, weight_decay=0, betas=[0.9, 0.99])
    tr['scheduler'] = OD(type='MultiStepLR', milestones=[2, 3], gamma=0.5)
    tr['total_iter'] = 4
    tr['warmup_iter'] = -1
    tr['pixel_opt'] = OD(type='L1Loss', loss_weight=1.0, reduction='mean')
    opt['train'] = tr
    return opt


def _checksums(net):
    return np.array([[float(p.detach().double().sum()), float(p.detach().double().norm())] for _, p in net.named_parameters()])


def _model():
    from image_restoration_amd.models import build_model
    model = build_model(_train_opt())
    model.net_g.load_state_dict({k: torch.from_numpy(v) for k, v in synth.ridnet_state_dict(481, **SMALL_CFG).items()}, strict=True)
    model.net_g.invalidate_packed()
    model.model_ema(0)
    return model


def _step(model, it):
    model.update_learning_rate(it, warmup_iter=-1)
    gt = synth.uniform_input(1950 + it, (4, 3, 24, 24))
    lq = np.clip(gt + 0.1 * synth.gaussian(1900 + it, (4, 3, 24, 24)), 0, 1).astype(np.float32)
    model.feed_data({'lq': torch.from_numpy(lq), 'gt': torch.from_numpy(gt)})
    model.optimize_parameters(it)


def test_optimize_parameters_three_iterations(cuda, golden):
    """Three SRModel iterations against the reference's float32 / float64 trajectories by the G-i rule
    (tests/test_training_gpu.py): |hip - q64| <= 5*|q32 - q64| + floor; iteration 1's loss within 2e-5 of float32.  Floors: 2e-5,
    or 1e-3 from iteration 2 on where the fixture's float64 run has a ReLU pre-activation within 1e-4 of zero."""
    g = golden('g_w_ridnet')
    mt = 'SRModel'
    K = 5.0

    def bound(hip, q32, q64, floor, what):
        hip, q32, q64 = np.asarray(hip, np.float64), np.asarray(q32, np.float64), np.asarray(q64, np.float64)
        err, ref_err = np.abs(hip - q64).max(), np.abs(q32 - q64).max()
        assert err <= K * ref_err + floor, (what, err, ref_err)

    model = _model()
    keys = [str(k) for k in g[f'{mt}_log_keys']]
    kinked = False
    for it in range(1, 4):
        _step(model, it)
        assert abs(model.get_current_learning_rate()[0] - g[f'{mt}_lrs'][it - 1]) < 1e-15
        log = model.get_current_log()
        assert sorted(log) == keys
        l32, l64 = g[f'{mt}_logs'][it - 1], g[f'{mt}64_logs'][it - 1]
        scale = np.maximum(np.abs(l64), 1e-3)
        noise = (np.abs(l32 - l64) / scale).max()
        for j, k in enumerate(keys):
            if it == 1:
                assert abs(log[k] - l32[j]) <= 2e-5 * max(abs(l32[j]), 1e-3), (k, log[k], l32[j])
            assert abs(log[k] - l64[j]) / scale[j] <= K * noise + 2e-5, (it, k, log[k], l64[j], noise)
        kinked = kinked or g[f'{mt}64_relu_margin_it{it}'].min() < 1e-4
        floor = 1e-3 if kinked and it > 1 else 2e-5
        bound(_checksums(model.net_g), g[f'{mt}_g_checksum_it{it}'], g[f'{mt}64_g_checksum_it{it}'], floor, (it, 'g params'))
    floor = 1e-3 if kinked else 2e-5
    bound(_checksums(model.net_g_ema), g[f'{mt}_ema_checksum'], g[f'{mt}64_ema_checksum'], floor, 'ema')
    st = model.optimizer_g.state_dict()['state']
    ea = np.array([float(st[i]['exp_avg'].double().norm()) for i in sorted(st)])
    ea2 = np.array([float(st[i]['exp_avg_sq'].double().norm()) for i in sorted(st)])
    bound(ea, g[f'{mt}_adam_g_exp_avg'], g[f'{mt}64_adam_g_exp_avg'], 1e-3 * g[f'{mt}64_adam_g_exp_avg'].max(), 'exp_avg')
    bound(ea2, g[f'{mt}_adam_g_exp_avg_sq'], g[f'{mt}64_adam_g_exp_avg_sq'], 1e-3 * g[f'{mt}64_adam_g_exp_avg_sq'].max(), 'exp_avg_sq')
    bound(model.net_g.tail.weight.detach().cpu().numpy(), g[f'{mt}_g_tail_weight'], g[f'{mt}64_g_tail_weight'], floor * 0.1, 'tail')


def test_srmodel_steps_are_bit_reproducible(cuda):
    """No atomics on the path: two runs of two seeded SRModel steps end in bit-identical weights and logs."""
    def run():
        model = _model()
        for it in (1, 2):
            _step(model, it)
        return [p.detach().clone() for p in model.net_g.parameters()], dict(model.get_current_log())
    p1, l1 = run()
    p2, l2 = run()
    assert all(torch.equal(a, b) for a, b in zip(p1, p2)) and l1 == l2


def test_small_net_on_the_8_row_path_matches_the_float64_oracle(cuda):
    """The fixture's small net (mid 16, 2 EAMs) at batch 4 of 128^2: at cout 16 that is 4 strips x 16 row tiles x 4 images =
    256 workgroups, so every sr_convd_f32 launch takes the 8-row tiles (asserted through the restated dispatch of
    tests/test_convd_ops_gpu.py on the profiled launches).  Forward, dL/dx and every parameter gradient against autograd
    through oracle/ridnet_ref.py in float64 (pinned to the reference by tests/test_oracle.py).  Bounds: the forward within 10x
    the float32 oracle's own distance from float64 (features are in the hundreds), never below 1e-4; gradients, as
    tests/test_backward_gpu.py states for whole networks, relative-L2 < 2e-3 and max-relative < 2e-2, or 5x the float32
    oracle's own distance from float64 where that is larger (the G-i rule of tests/test_training_gpu.py): a ReLU pre-activation
    within rounding of zero may take the other branch in float32, and at 65536 pixels per image with features in the hundreds
    the float32 oracle itself moves a dilated layer's gradient by ~1e-3; a missed halo row or a wrong tile is O(1) on the
    elements it touches."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_convd_ops_gpu import _convd_instance
    from oracle import ridnet_ref as RR
    sd_np = synth.ridnet_state_dict(400, **SMALL_CFG)
    x_np = synth.uniform_input(430, (4, 3, 128, 128))
    gy_np = synth.gaussian(431, (4, 3, 128, 128))
    net = _load(ira.build_network(dict(type='RIDNet', **SMALL_CFG)), sd_np, cuda).train()
    x = torch.from_numpy(x_np).to(cuda).requires_grad_(True)
    lib = _lib.load()
    out = {}

    def run():
        out['y'] = net(x)
        out['y'].backward(torch.from_numpy(gy_np).to(cuda))
        torch.cuda.synchronize()
    recs = _profiled(lib, run)
    convd = [r for r in recs if r.kernel_id in (81, 82)]
    assert len(convd) >= 2 * 6, len(convd)      # per EAM, forward alone: d = 2, 3, 4, the aggregation, block1's post_act, the 1x1
    for r in convd:
        assert (r.n, r.h, r.w) == (4, 128, 128) and _convd_instance(3, 1, r.cout, r.n, r.h, r.w)[1:] == (2, 16), (r.cout, r.cin)
    sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd_np.items()}
    xr = torch.from_numpy(x_np).double().requires_grad_(True)
    yr = RR.ridnet_forward(xr, sd, num_block=2)
    yr.backward(torch.from_numpy(gy_np).double())
    sd32 = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in sd_np.items()}
    x32 = torch.from_numpy(x_np).clone().requires_grad_(True)
    y32 = RR.ridnet_forward(x32, sd32, num_block=2)
    y32.backward(torch.from_numpy(gy_np))
    y32 = y32.detach()
    tol = max(1e-4, 10 * float((y32.double() - yr.detach()).abs().max()))
    err = float((out['y'].detach().cpu().double() - yr.detach()).abs().max())
    assert err < tol, (err, tol)

    def rel(a, b):
        a, b = a.detach().cpu().double(), b.detach().double()
        return float((a - b).norm() / max(float(b.norm()), 1e-30)), float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))
    def check(got, want, q32, what):
        r2, rm = rel(got, want)
        n2, nm = rel(q32, want)
        assert r2 < max(2e-3, 5 * n2) and rm < max(2e-2, 5 * nm), (what, r2, rm, n2, nm)
    check(x.grad, xr.grad, x32.grad, 'dx')
    params = dict(net.named_parameters())
    assert sorted(params) == sorted(sd)
    for k, p in sd.items():
        check(params[k].grad, p.grad, sd32[k].grad, k)
