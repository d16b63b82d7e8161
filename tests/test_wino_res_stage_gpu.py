"""Residual 1 of the Winograd fp32 kernel (csrc/conv_wino_f32.hip) through the LDS, at the smallest shapes where it can go wrong;
through the development hooks sr_dev_conv3x3_wino_pack_f32 and sr_dev_conv3x3_wino_f32, which accept any size.

At NW = 2 and 1, with two chunks or more, a workgroup brings its own output tile of residual 1 into the X buffers by LDS-DMA under the
MFMAs of its last chunk, and the epilogue reads it from there; the exchange of the output transform lives in the U buffers.  With one
chunk, at NW = 4, or under sr_dev_set_wino_res_stage(0), the epilogue loads residual 1 from memory as before.  A staged tile's
epilogue also issues its loads of residual 2 in front of its first store.  Every path computes the same expression: all of them
must give the same bits.

  * cin = 8, 16, 24: one chunk (never staged), two (the staging chunk directly behind the peeled one), three (one body iteration);
  * cout = 64 and 96: two and three cout groups; 96 also with res_cbn = 8, so that the third group's planes carry no residual;
  * 6 x 70 and 13 x 37: ragged rows and columns for both tile heights, two column tiles; one case through the x2 source map;
  * no residual, res1, res1 + res2, with distinct betas, alpha != 1 and a slope.

Bound, restated from tests/test_wino_f32_gpu.py.  EPS = 2^-24.  With A the SAME Winograd pipeline on absolute values in float64,

    A0 = |A^T| [ sum_cin (|G| |g| |G|^T) . (|B^T| |d| |B|) ] |A|,    A = |alpha| (A0 + |bias|) + |beta1 r1| + |beta2 r2|,

|y - y64| <= k EPS A + EPS |y64| with k = 2 cin_pad + 8 + 8 (two roundings per product of the MFMA sum, 8 for the transforms, 8 for
the epilogue).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from image_restoration_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_wino_f32_gpu import SENTINEL, WINO_IDS, _from_cb8, _pack, _profiled, _ptr, _st, _stride, _to_cb8  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
TINY = 1e-30
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)

N = 2
ALPHA, SLOPE, BETA1, BETA2 = 0.75, 0.2, 0.3, -1.25
# (stage, mode): modes 2, 3, 4 are NW = 4, 2, 1
PATHS = [(1, 2), (1, 3), (1, 4), (0, 3), (0, 4)]


def _case(cin, cout, res_cbn, h, w, nres, up=False):
    return (cin, cout, res_cbn, h, w, nres, up)


CASES = [_case(cin, cout, cbn, h, w, nres)
         for cin in (8, 16, 24)
         for (h, w) in ((6, 70), (13, 37))
         for nres in (0, 1, 2)
         for (cout, cbn) in ((64, 0), (96, 0), (96, 8))
         if not (nres == 0 and cbn)]
CASES.append(_case(16, 64, 0, 8, 40, 2, up=True))     # the x2 source map: 16 x 80 output


def _id(c):
    cin, cout, cbn, h, w, nres, up = c
    return f'{cin}to{cout}' + (f'cbn{cbn}' if cbn else '') + f'-{h}x{w}-res{nres}' + ('-up' if up else '')


def _f32(a):
    return a.float().double()


def wino_abs(x, wt):
    """|A^T| [sum_cin (|G||g||G|^T) . (|B^T||d||B|)] |A| in float64: x [n][cin][H][W] (already upsampled), wt [cout][cin][3][3];
    patches anchored at even coordinates, zeros beyond the image."""
    n, cin, H, W = x.shape
    ph, pw = (H + 1) // 2, (W + 1) // 2
    xp = torch.zeros((n, cin, 2 * ph + 2, 2 * pw + 2), dtype=torch.float64)
    xp[:, :, 1:H + 1, 1:W + 1] = x.abs()
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)
    v = torch.einsum('ia,ncpqab,jb->ncpqij', BT.abs(), d, BT.abs())
    u = torch.einsum('ia,ocab,jb->ocij', G.abs(), wt.abs(), G.abs())
    m = torch.einsum('ocij,ncpqij->nopqij', u, v)
    y = torch.einsum('ia,nopqab,jb->nopqij', AT.abs(), m, AT.abs())
    return y.permute(0, 1, 2, 4, 3, 5).reshape(n, -1, 2 * ph, 2 * pw)[:, :, :H, :W]


def reference(case):
    """(x, wt, bias, [residuals], y64, bound).  A residual covers the first res_cbn channel blocks (all of them when res_cbn = 0)."""
    cin, cout, cbn, h, w, nres, up = case
    rng = np.random.default_rng(sum(map(ord, _id(case))))
    H, W = (2 * h, 2 * w) if up else (h, w)
    rc = cbn * 8 if cbn else cout
    x = _f32(torch.from_numpy(rng.standard_normal((N, cin, h, w))))
    wt = _f32(torch.from_numpy(rng.standard_normal((cout, cin, 3, 3)))) * 0.125
    bias = _f32(torch.from_numpy(rng.standard_normal((cout,)))) * 0.5
    res = [_f32(torch.from_numpy(rng.standard_normal((N, rc, H, W)))) for _ in range(nres)]
    xu = F.interpolate(x, scale_factor=2, mode='nearest') if up else x
    c = F.conv2d(xu, wt, bias, padding=1)
    y = torch.where(c > 0, c, SLOPE * c) * ALPHA
    A = abs(ALPHA) * (wino_abs(xu, wt) + bias.abs().view(1, -1, 1, 1))
    for beta, r in zip((BETA1, BETA2), res):
        y[:, :rc] += beta * r
        A[:, :rc] += abs(beta) * r.abs()
    k = 2 * cin + 8 + 8   # cin is a multiple of 8: cin_pad = cin
    return x, wt, bias, res, y, k * EPS * A + EPS * y.abs() + TINY


@pytest.fixture(scope='module')
def lib():
    lib = _lib.load()
    lib.sr_dev_set_wino_f32.argtypes = [C.c_int]
    lib.sr_dev_set_wino_res_stage.argtypes = [C.c_int]
    lib.sr_dev_conv3x3_wino_f32.argtypes = [C.POINTER(_lib.ConvDesc), C.c_void_p, C.c_void_p]
    lib.sr_dev_conv3x3_wino_pack_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.sr_dev_conv3x3_wino_pack_bytes.argtypes = [C.c_int, C.c_int]
    lib.sr_dev_conv3x3_wino_pack_bytes.restype = C.c_size_t
    yield lib
    lib.sr_dev_set_wino_f32(1)
    lib.sr_dev_set_wino_res_stage(1)


@pytest.fixture(scope='module')
def refs():
    """case id -> reference(case), computed when first asked for and never changed."""
    cache = {}

    def get(case):
        if _id(case) not in cache:
            cache[_id(case)] = reference(case)
        return cache[_id(case)]
    return get


class Launch:
    """One case on the device: weight image, bias and residual buffers made once; run(stage, mode) launches into a fresh destination."""

    def __init__(self, lib, case, ref, dev):
        self.lib, self.case, self.dev = lib, case, dev
        cin, cout, cbn, h, w, nres, up = case
        self.x, wt, bias, res = ref[0], ref[1], ref[2], ref[3]
        self.image = _pack(lib, wt, dev)
        self.bias = bias.float().to(dev)
        rb = cbn if cbn else cout // 8
        self.res = [_to_cb8(r, 1 + rb + 1, 1, dev) for r in res]     # [sentinel | residual blocks | sentinel]
        self.res_before = [r.cpu() for r in self.res]
        self.src = _to_cb8(self.x, cin // 8 + 2, 1, dev)
        self.src_before = self.src.cpu()

    def desc(self, dst):
        cin, cout, cbn, h, w, nres, up = self.case
        d = _lib.ConvDesc()
        d.in_, d.in_img_stride, d.cin_pad, d.cin_real, d.in_h, d.in_w = _ptr(self.src, 1), _stride(self.src), cin, cin, h, w
        d.upsample = int(up)
        d.wpacked, d.bpacked, d.cout = self.image.data_ptr(), self.bias.data_ptr(), cout
        d.out, d.out_img_stride = _ptr(dst, 1), _stride(dst)
        d.n, d.act_slope, d.alpha = N, SLOPE, ALPHA
        d.res_cbn = cbn
        for k, (rb, beta) in enumerate(zip(self.res, (BETA1, BETA2))):
            setattr(d, f'res{k + 1}', _ptr(rb, 1))
            setattr(d, f'res{k + 1}_img_stride', _stride(rb))
            setattr(d, f'beta{k + 1}', beta)
        return d

    def launch(self, d, stage, mode):
        self.lib.sr_dev_set_wino_res_stage(stage)
        self.lib.sr_dev_set_wino_f32(mode)
        ids = _profiled(self.lib, lambda: _lib.check(self.lib.sr_dev_conv3x3_wino_f32(C.byref(d), self.image.data_ptr(), _st()),
                                                     'wino conv'))
        torch.cuda.synchronize()
        return ids

    def run(self, stage, mode):
        """(whole destination buffer on the CPU, launch ids)"""
        cin, cout, cbn, h, w, nres, up = self.case
        H, W = (2 * h, 2 * w) if up else (h, w)
        dst = torch.full((N, cout // 8 + 2, H, W, 8), SENTINEL, dtype=torch.float32, device=self.dev)
        ids = self.launch(self.desc(dst), stage, mode)
        return dst.cpu(), ids

    def inputs_unchanged(self):
        return torch.equal(self.src.cpu(), self.src_before) and all(torch.equal(r.cpu(), b) for r, b in zip(self.res, self.res_before))


def _reset(lib):
    lib.sr_dev_set_wino_f32(1)
    lib.sr_dev_set_wino_res_stage(1)


@pytest.mark.parametrize('case', CASES, ids=[_id(c) for c in CASES])
def test_every_path_gives_the_same_bits_inside_the_float64_bound(cuda, lib, refs, case):
    cin, cout, cbn, h, w, nres, up = case
    ref = refs(case)
    y64, bound = ref[4], ref[5]
    launch = Launch(lib, case, ref, cuda)
    db = cout // 8
    outs = {}
    try:
        for stage, mode in PATHS:
            out, ids = launch.run(stage, mode)
            assert ids == [WINO_IDS[mode]], (stage, mode, ids)
            err = (_from_cb8(out, 1, cout) - y64).abs()
            print(f'{_id(case)} stage {stage} mode {mode}: max err / bound {float((err / bound).max()):.4f}, max err {float(err.max()):.3e}')
            assert not bool((err > bound).any()), (stage, mode, int((err > bound).sum()), float((err / bound).max()))
            assert bool((out[:, :1] == SENTINEL).all()), f'stage {stage} mode {mode} wrote below its channel slice'
            assert bool((out[:, 1 + db:] == SENTINEL).all()), f'stage {stage} mode {mode} wrote above its channel slice'
            assert launch.inputs_unchanged(), f'stage {stage} mode {mode} changed its source or a residual'
            outs[(stage, mode)] = out
        for path in PATHS[1:]:
            assert torch.equal(outs[path], outs[PATHS[0]]), f'(stage, mode) = {path} differs from {PATHS[0]}'
    finally:
        _reset(lib)


@pytest.mark.parametrize('mode', [3, 4], ids=['nw2', 'nw1'])
@pytest.mark.parametrize('cin', [16, 24], ids=['2chunks', '3chunks'])
def test_reused_lds_regions_do_not_race(cuda, lib, refs, cin, mode):
    """The residual tile in the X buffers and the exchange in the U buffers, 20 launches into fresh buffers: equal bits every time."""
    case = _case(cin, 96, 0, 13, 37, 2)
    launch = Launch(lib, case, refs(case), cuda)
    try:
        first = launch.run(1, mode)[0]
        assert bool(torch.isfinite(first[:, 1:-1]).all())
        for i in range(19):
            assert torch.equal(launch.run(1, mode)[0], first), f'launch {i + 2} differs from the first'
    finally:
        _reset(lib)


@pytest.mark.parametrize('mode', [3, 4], ids=['nw2', 'nw1'])
@pytest.mark.parametrize('which', [1, 2], ids=['res1', 'res2'])
def test_residual_that_is_the_destination(cuda, lib, refs, which, mode):
    """res1 == out (or res2 == out), plane for plane (an in-place residual add): a workgroup stages, and a lane loads ahead of its
    stores, exactly the pixels and planes it stores itself, so stage on equals stage off, and both are the value computed from the
    destination's old contents."""
    case = _case(24, 64, 0, 13, 37, which)
    ref = refs(case)
    y64, bound = ref[4], ref[5]
    launch = Launch(lib, case, ref, cuda)
    outs = []
    try:
        for stage in (1, 0):
            dst = launch.res[which - 1].clone()    # [sentinel | the residual | sentinel]
            d = launch.desc(dst)
            setattr(d, f'res{which}', d.out)
            setattr(d, f'res{which}_img_stride', d.out_img_stride)
            launch.launch(d, stage, mode)
            out = dst.cpu()
            assert bool((out[:, :1] == SENTINEL).all()) and bool((out[:, -1:] == SENTINEL).all())
            err = (_from_cb8(out, 1, 64) - y64).abs()
            assert not bool((err > bound).any()), (stage, float((err / bound).max()))
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), 'stage on differs from stage off'
    finally:
        _reset(lib)
