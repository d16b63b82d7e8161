"""sr_ca_squeeze_bf16 / sr_ca_excite_bf16 (channel_attention_bf16.hip) against float64 on the CPU.

Every case runs on tensors whose image strides exceed the images, with the slack between and after the images filled with NaN
bit patterns in u, x and out; one excite runs in place (out = x).  bf16 -> fp32 is exact, so p, h and s are held to the bounds
tests/test_rcan_gpu.py derives for the fp32 kernels on the same arithmetic (a lane sums 8 values, a 5-level butterfly, 8 waves,
the bands, one division: inside that test's BAND // 256 + 13 + bands operations), twice the bound allowed as there.  out is
compared with x + res_scale * u * s in float64 from the kernel's own s: half a bf16 ulp of the value plus 3 fp32 eps of
|x| + |res_scale * u * s| (the fp32 evaluation before the single rounding)."""
import ctypes as C

import numpy as np
import pytest
import torch

from image_restoration_amd import _lib

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24    # unit roundoff of fp32
EPS32 = 2.0 ** -23  # fp32 machine epsilon
BAND = 2048         # pixels per partial sum (channel_attention_bf16.hip kBandPixels)
NAN_BITS = (0x7FC1, 0xFFFF, 0x7FA5)   # quiet and signalling NaN patterns, as int16 below
CASES = [(1, 16, 1, 1, 1), (2, 16, 4, 3, 5), (2, 48, 3, 45, 47), (1, 64, 4, 64, 64), (2, 32, 2, 7, 293), (1, 512, 32, 4, 4)]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _profiled(lib, fn, cap=64):
    _lib.check(lib.sr_profile_start(cap), 'sr_profile_start')
    try:
        fn()
    finally:
        recs = (_lib.LaunchRecord * cap)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, cap, C.byref(cnt)), 'sr_profile_stop')
    return [recs[i].kernel_id for i in range(min(cnt.value, cap))]


class Strided:
    """A CB16 tensor [n][nf/16][h][w][16] inside a flat bf16 buffer with an image stride larger than the image; everything
    outside the images holds NaN bit patterns."""

    def __init__(self, n, nf, h, w, dev, extra, tail, values=None):
        self.n, self.nf, self.h, self.w = n, nf, h, w
        self.img = nf * h * w
        self.stride = self.img + extra
        total = n * self.stride + tail
        pat = torch.tensor(np.array(NAN_BITS, dtype=np.uint16).view(np.int16)).repeat(total // 3 + 1)[:total]
        self.mask = torch.ones(total, dtype=torch.bool)
        for i in range(n):
            self.mask[i * self.stride:i * self.stride + self.img] = False
        self.slack = pat[self.mask].clone()
        bits = pat.clone()
        if values is not None:   # NCHW bf16 values
            cb = values.to(torch.bfloat16).reshape(n, nf // 16, 16, h, w).permute(0, 1, 3, 4, 2).contiguous().view(torch.int16)
            for i in range(n):
                bits[i * self.stride:i * self.stride + self.img] = cb[i].reshape(-1)
        self.buf = bits.to(dev)

    ptr = property(lambda s: s.buf.data_ptr())

    def images(self):
        """NCHW float64 of what the buffer holds."""
        b = self.buf.cpu()
        t = torch.stack([b[i * self.stride:i * self.stride + self.img] for i in range(self.n)]).view(torch.bfloat16)
        return t.reshape(self.n, self.nf // 16, self.h, self.w, 16).permute(0, 1, 4, 2, 3).reshape(self.n, self.nf, self.h, self.w).double()

    def slack_untouched(self):
        return torch.equal(self.buf.cpu()[self.mask], self.slack)


def _case(n, nf, hid, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    u = (torch.randn(n, nf, h, w, generator=g, dtype=torch.float64) * 2 + 0.3).to(torch.bfloat16)
    x = torch.randn(n, nf, h, w, generator=g, dtype=torch.float64).to(torch.bfloat16)
    w1 = (torch.rand(hid, nf, 1, 1, generator=g, dtype=torch.float64) * 2 - 1) / nf ** 0.5
    b1 = torch.rand(hid, generator=g, dtype=torch.float64) - 0.5
    w2 = (torch.rand(nf, hid, 1, 1, generator=g, dtype=torch.float64) * 2 - 1) / hid ** 0.5
    b2 = torch.rand(nf, generator=g, dtype=torch.float64) - 0.5
    return u, x, [t.float() for t in (w1, b1, w2, b2)]


def _within(got, want, bound, what, k=2.0):
    err = (got.double() - want.double()).abs()
    ratio = float((err / (bound + 1e-300)).max())
    print(f'{what}: max err {float(err.max()):.3e}  max err / bound {ratio:.3f}')
    assert bool((err <= k * bound + 1e-30).all()), (what, float(err.max()), ratio)


def _out_bound(x, u, s, rs):
    """(x + rs * u * s in float64, the bound of the module docstring): the kernel's fp32 value is within 3 eps of
    |x| + |rs u s| of the exact one, and its rounding to bf16 (8 significant bits) moves it by at most half an ulp."""
    term = rs * u * s[:, :, None, None]
    want = x + term
    e32 = 3 * EPS32 * (x.abs() + term.abs())
    mag = want.abs() + e32
    half_ulp = torch.where(mag > 0, torch.exp2(torch.floor(torch.log2(mag.clamp_min(1e-300))) - 8), torch.zeros_like(mag))
    return want, half_ulp + e32


@pytest.mark.parametrize('n,nf,hid,h,w', CASES)
def test_squeeze_and_excite_match_float64(cuda, n, nf, hid, h, w):
    lib = _lib.load()
    rs = 0.75 if nf == 16 else 1.0
    u, x, W = _case(n, nf, hid, h, w, seed=nf * 1000 + h * 7 + w)
    w1, b1, w2, b2 = W
    ud = Strided(n, nf, h, w, cuda, 48, 80, u)
    xd = Strided(n, nf, h, w, cuda, 16, 32, x)
    od = Strided(n, nf, h, w, cuda, 112, 16)
    Wd = [t.to(cuda) for t in W]
    need = lib.sr_ca_workspace_bytes_bf16(n, nf, hid, h, w)
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)

    def squeeze(p, hb, s):
        _lib.check(lib.sr_ca_squeeze_bf16(ud.ptr, ud.stride, n, nf, h, w, *(t.data_ptr() for t in Wd), hid,
                                          p.data_ptr() if p is not None else None, hb.data_ptr() if hb is not None else None,
                                          s.data_ptr(), ws.data_ptr(), need, _st()), 'sr_ca_squeeze_bf16')

    def excite(src, dst, gates):
        _lib.check(lib.sr_ca_excite_bf16(src.ptr, src.stride, ud.ptr, ud.stride, gates.data_ptr(), dst.ptr, dst.stride, n, nf, h, w,
                                         rs, _st()), 'sr_ca_excite_bf16')
    p, hb, s = (torch.full((n, k), float('nan'), device=cuda) for k in (nf, hid, nf))
    assert _profiled(lib, lambda: squeeze(p, hb, s)) == [102, 103]
    # float64 of the bf16-valued u
    u64, x64 = u.double(), x.double()
    A1, A2 = w1.double()[:, :, 0, 0], w2.double()[:, :, 0, 0]
    p64 = u64.mean((2, 3))
    h64 = torch.relu(p64 @ A1.T + b1.double())
    s64 = torch.sigmoid(h64 @ A2.T + b2.double())
    bands = -(-(h * w) // BAND)
    e_p = (BAND // 256 + 13 + bands) * U32 * u64.abs().mean((2, 3))
    e_z1 = (nf + 2) * U32 * (p64.abs() @ A1.abs().T + b1.double().abs()) + e_p @ A1.abs().T
    e_z2 = (hid + 2) * U32 * (h64.abs() @ A2.abs().T + b2.double().abs()) + e_z1 @ A2.abs().T
    e_s = 0.25 * e_z2 + 4 * U32 * s64
    _within(p.cpu(), p64, e_p, 'p')
    _within(hb.cpu(), h64, e_z1, 'h')
    _within(s.cpu(), s64, e_s, 's')
    # p and hbuf are optional; a second run is bit-identical
    s2 = torch.full_like(s, float('nan'))
    squeeze(None, None, s2)
    assert torch.equal(s2, s)
    p3, h3, s3 = (torch.full_like(t, float('nan')) for t in (p, hb, s))
    squeeze(p3, h3, s3)
    assert torch.equal(p3, p) and torch.equal(h3, hb) and torch.equal(s3, s)
    # excite, from the kernel's own s
    assert _profiled(lib, lambda: excite(xd, od, s)) == [104]
    want, bound = _out_bound(x64, u64, s.cpu().double(), rs)
    got = od.images()
    _within(got, want, bound, 'out', k=1.0)
    # negative control: gates rotated by one channel are outside the bound
    wrong, wbound = _out_bound(x64, u64, torch.roll(s.cpu().double(), 1, dims=1), rs)
    assert not bool(((got - wrong).abs() <= wbound).all())
    # nothing outside the images was read into the result or written
    assert ud.slack_untouched() and xd.slack_untouched() and od.slack_untouched()
    assert torch.equal(ud.images(), u64) and torch.equal(xd.images(), x64)
    # a second run is bit-identical, and so is the run in place
    first = od.buf.clone()
    od2 = Strided(n, nf, h, w, cuda, 112, 16)
    excite(xd, od2, s)
    assert torch.equal(od2.buf, first)
    xa = Strided(n, nf, h, w, cuda, 16, 32, x)
    excite(xa, xa, s)
    assert xa.slack_untouched() and torch.equal(xa.images(), got)
    torch.cuda.synchronize()


def test_refusals_return_their_codes(cuda):
    lib = _lib.load()
    n, nf, hid, h, w = 2, 32, 2, 5, 6
    img = nf * h * w
    u = torch.zeros(n * img, dtype=torch.bfloat16, device=cuda)
    v = [torch.zeros(k, device=cuda) for k in (hid * nf, hid, nf * hid, nf)]
    s = torch.zeros(n, nf, device=cuda)
    need = lib.sr_ca_workspace_bytes_bf16(n, nf, hid, h, w)
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)

    def squeeze(nf_=nf, hid_=hid, stride=img, wsb=need, hh=h, ww=w, up=u.data_ptr(), sp=s.data_ptr()):
        return lib.sr_ca_squeeze_bf16(up, stride, n, nf_, hh, ww, v[0].data_ptr(), v[1].data_ptr(), v[2].data_ptr(), v[3].data_ptr(),
                                      hid_, None, None, sp, ws.data_ptr(), wsb, _st())

    def excite(nf_=nf, hh=h, ww=w, stride=img, op=u.data_ptr(), sp=s.data_ptr()):
        return lib.sr_ca_excite_bf16(u.data_ptr(), stride, u.data_ptr(), stride, sp, op, stride, n, nf_, hh, ww, 1.0, _st())
    assert squeeze() == 0 and excite() == 0
    assert squeeze(nf_=24) == -1 and squeeze(nf_=528) == -1 and squeeze(hid_=0) == -1 and squeeze(hid_=nf + 1) == -1
    assert squeeze(hh=0) == -1 and squeeze(ww=0) == -1 and squeeze(up=None) == -1 and squeeze(sp=None) == -1
    assert squeeze(stride=img - 16) == -1
    assert squeeze(wsb=need - 4) == -3
    assert b'workspace' in lib.sr_last_error()
    assert excite(nf_=24) == -1 and excite(nf_=528) == -1 and excite(hh=0) == -1 and excite(ww=0) == -1
    assert excite(sp=None) == -1 and excite(op=None) == -1 and excite(op=u.data_ptr() + 2) == -1 and excite(stride=img - 16) == -1
    torch.cuda.synchronize()


def test_host_layer_wrappers(cuda):
    """hip_ops.ca_squeeze_bf16 / ca_excite_bf16 on CB16 tensors: the same results as the raw entry points, in place when asked."""
    from image_restoration_amd import hip_ops
    n, nf, hid, h, w = 2, 32, 2, 9, 11
    u, x, W = _case(n, nf, hid, h, w, seed=5)
    Wd = [t.to(cuda) for t in W]

    def cb16(t):
        return hip_ops.CB16(t.reshape(n, nf // 16, 16, h, w).permute(0, 1, 3, 4, 2).contiguous().to(cuda))
    ud, xd = cb16(u), cb16(x)
    s = hip_ops.ca_squeeze_bf16(ud, *Wd)
    assert s.shape == (n, nf) and s.dtype == torch.float32
    out = hip_ops.ca_excite_bf16(xd, ud, s, 0.5)
    want, bound = _out_bound(x.double(), u.double(), s.cpu().double(), 0.5)
    got = out.buf.cpu().permute(0, 1, 4, 2, 3).reshape(n, nf, h, w).double()
    _within(got, want, bound, 'wrapper out', k=1.0)
    same = hip_ops.ca_excite_bf16(xd, ud, s, 0.5, out=xd)
    assert same is xd and torch.equal(xd.buf, out.buf)
