"""GFPGANv1OCR on the MI355X: every entry point of include/sr_hip_gfpgan.h against float64 on the CPU, the network against the
reference's fixture (g_x_gfpgan, tools/make_golden_gfpgan.py) and against the float64 restatement (tests/gfpgan_restate.py) at the
product configurations at batch 2 and at the benchmark's batch 16, random noise, checkpoints, the inference command line and
determinism.

Bounds of the entry points are derived, in the conventions of tests/test_convd_ops_gpu.py.  EPS = 2^-24.  For every output
element let A be the same operation on absolute values in float64 (|x s|, |W|, |d|, |noise|, |bias|, then sqrt(2) for the
activation, |S| and |T| for the SFT, |s_next|).  Then |y - y64| <= k EPS A + EPS |y64| with k = 2 * taps * cin_pad + 16: two
roundings per product of the MFMA chain over (cin block, tap), plus the tail (demod, noise multiply-add, bias, activation,
alpha, SFT multiply-add, s_next) and, for the upsampling conv, the 16-tap blur.  A slope <= 1 only shrinks an error.  ToRGB sums
C products per channel (k = 2 C + 16); the style kernel nsf and cin products (k = 2 nsf + 8 for s, 2 cin + 8 for d's sum).
The network tests use the rule of tests/test_ridnet_gpu.py: within 10x the reference's own float32 distance from float64.
"""
import math
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_restoration_amd as ira
from image_restoration_amd import _lib, hip_ops
from image_restoration_amd.utils import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gfpgan_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
SQRT2 = math.sqrt(2.0)
CONFIGS = {
    'sq': dict(input_width=32, input_height=32, num_style_feat=64, channel_multiplier=0.5, narrow=0.0625, num_mlp=2,
               input_is_latent=True, different_w=True, sft_half=True),
    'rect': dict(input_width=64, input_height=16, num_style_feat=32, channel_multiplier=0.5, narrow=0.0625, num_mlp=2,
                 input_is_latent=True, different_w=True, sft_half=True),
    'mlp': dict(input_width=16, input_height=16, num_style_feat=32, channel_multiplier=1, narrow=0.0625, num_mlp=3,
                input_is_latent=False, different_w=False, sft_half=False),
}
SEEDS = {'sq': 501, 'rect': 502, 'mlp': 503}
PRODUCT = dict(num_style_feat=256, channel_multiplier=0.5, narrow=1, num_mlp=4, input_is_latent=True, different_w=True,
               sft_half=True)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _check(y, y64, a64, k, what):
    y = y.detach().double().cpu()
    err = (y - y64).abs()
    bound = k * EPS * a64 + EPS * y64.abs() + 1e-30
    bad = ~(err <= bound)
    assert not bool(bad.any()), (what, int(bad.sum()), float((err / bound).nan_to_num(1e30).max()), float(err.nan_to_num(1e30).max()))


def _to_cb8(t, blocks_total, cb0, cuda, fill=float('nan')):
    """NCHW float64 [n, c, h, w] (c multiple of 8) -> a CB8 window at block cb0 of a buffer of blocks_total blocks, NaN around."""
    n, c, h, w = t.shape
    buf = torch.full((n, blocks_total, h, w, 8), fill, dtype=torch.float32)
    buf[:, cb0:cb0 + c // 8] = t.float().view(n, c // 8, 8, h, w).permute(0, 1, 3, 4, 2)
    return hip_ops.CB8(buf.to(cuda), cb0, c // 8)


def _from_cb8(win):
    b = win.buf[:, win.cb0:win.cb0 + win.cbn].double().cpu()
    n, cb, h, w, _ = b.shape
    return b.permute(0, 1, 4, 2, 3).reshape(n, cb * 8, h, w)


def _tail64(raw, araw, d, noise, ns, bias, sft, sft_c0, s_next):
    """The tail in float64 on (value, magnitude)."""
    v = raw * d[:, :, None, None]
    a = araw * d.abs()[:, :, None, None]
    if noise is not None:
        v = v + ns * noise
        a = a + abs(ns) * noise.abs()
    v = F.leaky_relu(v + bias.view(1, -1, 1, 1), 0.2) * SQRT2
    a = (a + bias.abs().view(1, -1, 1, 1)) * SQRT2
    if sft is not None:
        s, t = sft
        v = torch.cat([v[:, :sft_c0], v[:, sft_c0:] * s + t], 1)
        a = torch.cat([a[:, :sft_c0], a[:, sft_c0:] * s.abs() + t.abs()], 1)
    if s_next is not None:
        v = v * s_next[:, :, None, None]
        a = a * s_next.abs()[:, :, None, None]
    return v, a


def _tail_case(g, n, cout, h, w, noise_mode, sft_mode, with_next, cuda):
    d = torch.rand(n, cout, generator=g, dtype=torch.float64) + 0.5
    noise = None
    if noise_mode == 'buffer':
        noise = torch.randn(1, 1, h, w, generator=g, dtype=torch.float64)
    elif noise_mode == 'sample':
        noise = torch.randn(n, 1, h, w, generator=g, dtype=torch.float64)
    bias = torch.randn(cout, generator=g, dtype=torch.float64) * 0.1
    sft_c0 = cout // 16 * 8 if sft_mode == "half" else 0
    sft = None
    if sft_mode != 'none':
        c = cout - sft_c0
        sft = (torch.randn(n, c, h, w, generator=g, dtype=torch.float64) + 1, torch.randn(n, c, h, w, generator=g, dtype=torch.float64))
    s_next = torch.randn(n, cout, generator=g, dtype=torch.float64) if with_next else None
    dev = dict(d=d.float().contiguous().to(cuda), noise=None if noise is None else noise.float().contiguous().to(cuda),
               bias=bias.float().contiguous().to(cuda), s_next=None if s_next is None else s_next.float().contiguous().to(cuda))
    if sft is not None:
        c = sft[0].shape[1]
        dev['sft'] = (_to_cb8(sft[0], c // 8 + 2, 1, cuda), _to_cb8(sft[1], c // 8 + 1, 0, cuda))
    else:
        dev['sft'] = None
    tail = hip_ops.gfpgan_tail(dev['d'], dev['noise'], 0.37, dev['sft'], sft_c0, dev['s_next'])
    return dict(d=d, noise=noise, ns=float(np.float32(0.37)), bias=bias, sft=sft, sft_c0=sft_c0, s_next=s_next), dev, tail


TAIL_OPTS = [('none', 'none', False), ('buffer', 'half', True), ('sample', 'full', False), ('sample', 'half', False),
             ('buffer', 'none', True)]
MOD_SHAPES = [(2, 16, 16, 4, 4), (2, 32, 64, 4, 16), (3, 24, 40, 37, 45), (2, 64, 32, 64, 64), (1, 32, 32, 256, 256)]


@pytest.mark.parametrize('shape', MOD_SHAPES, ids=[f'{s}' for s in MOD_SHAPES])
@pytest.mark.parametrize('opts', TAIL_OPTS, ids=['plain', 'buf-half-next', 'smp-full', 'smp-half', 'buf-next'])
def test_modconv_forward(cuda, shape, opts):
    """sr_gfpgan_modconv_f32 + sr_convk_pack_f32: a 3x3 StyleConv with every tail option, source and output NaN-padded windows."""
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(_seed(shape, opts))
    xs = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    W = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) / math.sqrt(cin * 9)
    ref, dev, tail = _tail_case(g, n, cout, h, w, *opts, cuda)
    src = _to_cb8(xs, cin // 8 + 2, 1, cuda)
    pc = hip_ops.PackedConvK(W.float().to(cuda), dev['bias'])
    out = _to_cb8(torch.zeros(n, cout, h, w, dtype=torch.float64), cout // 8 + 2, 1, cuda)
    hip_ops.gfpgan_modconv(src, pc, tail, out=out)
    torch.cuda.synchronize()
    raw = F.conv2d(xs.float().double(), W.float().double(), padding=1)
    araw = F.conv2d(xs.float().double().abs(), W.float().double().abs(), padding=1)
    y64, a64 = _tail64(raw, araw, ref['d'].float().double(), None if ref['noise'] is None else ref['noise'].float().double(), ref['ns'],
                       ref['bias'].float().double(), None if ref['sft'] is None else tuple(t.float().double() for t in ref['sft']),
                       ref['sft_c0'], None if ref['s_next'] is None else ref['s_next'].float().double())
    _check(_from_cb8(out), y64, a64, 2 * 9 * cin + 16, 'modconv')
    full = out.buf.cpu()
    assert torch.isnan(full[:, 0]).all() and torch.isnan(full[:, -1]).all()


UP_SHAPES = [(2, 16, 16, 4, 4), (2, 32, 64, 4, 16), (3, 40, 24, 13, 21), (2, 64, 32, 32, 32), (1, 64, 32, 128, 128)]


@pytest.mark.parametrize('shape', UP_SHAPES, ids=[f'{s}' for s in UP_SHAPES])
@pytest.mark.parametrize('opts', TAIL_OPTS, ids=['plain', 'buf-half-next', 'smp-full', 'smp-half', 'buf-next'])
def test_upconv_blur_forward(cuda, shape, opts):
    """sr_gfpgan_upconv_f32 (raw transposed conv, every parity) and sr_gfpgan_blur_up_f32 (blur + tail) at 2h x 2w."""
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(_seed(shape, opts, 'up'))
    xs = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    W = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) / math.sqrt(cin * 9)
    ref, dev, tail = _tail_case(g, n, cout, 2 * h, 2 * w, *opts, cuda)
    src = _to_cb8(xs, cin // 8 + 1, 1, cuda)
    pc = hip_ops.PackedConvK(W.float().to(cuda), None)
    t = hip_ops.gfpgan_upconv(src, pc)
    x32, w32 = xs.float().double(), W.float().double()
    raw = F.conv_transpose2d(x32, w32.transpose(0, 1), stride=2)
    araw = F.conv_transpose2d(x32.abs(), w32.abs().transpose(0, 1), stride=2)
    _check(_from_cb8(t), raw, araw, 2 * 9 * cin + 4, 'upconv raw')
    out = _to_cb8(torch.zeros(n, cout, 2 * h, 2 * w, dtype=torch.float64), cout // 8 + 1, 0, cuda)
    hip_ops.gfpgan_blur_up(t, dev['bias'], tail, out=out)
    torch.cuda.synchronize()
    y64, a64 = _tail64(R.fir(raw, 1, 1, 4.0), R.fir(araw, 1, 1, 4.0), ref['d'].float().double(),
                       None if ref['noise'] is None else ref['noise'].float().double(), ref['ns'], ref['bias'].float().double(),
                       None if ref['sft'] is None else tuple(v.float().double() for v in ref['sft']), ref['sft_c0'],
                       None if ref['s_next'] is None else ref['s_next'].float().double())
    _check(_from_cb8(out), y64, a64, 2 * 9 * cin + 16 + 16, 'upconv + blur')
    assert torch.isnan(out.buf[:, -1]).all()


@pytest.mark.parametrize('skip', [False, True])
@pytest.mark.parametrize('nxt', [False, True])
@pytest.mark.parametrize('shape', [(2, 16, 4, 4), (2, 512, 4, 16), (3, 64, 38, 46), (1, 32, 256, 256)])
def test_torgb(cuda, shape, skip, nxt):
    """sr_gfpgan_torgb_f32: modulated 1x1 to RGB + bias + upfirdn2d(skip, up 2), and x * s_next from the same read."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(_seed(shape, skip, nxt))
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64).float().double()
    W = torch.randn(3, c, generator=g, dtype=torch.float64).float().double()
    s = (torch.rand(n, c, generator=g, dtype=torch.float64) + 0.5).float().double()
    b = (torch.randn(3, generator=g, dtype=torch.float64) * 0.1).float().double()
    sk = torch.randn(n, 3, h // 2, w // 2, generator=g, dtype=torch.float64).float().double() if skip else None
    sn = torch.randn(n, c, generator=g, dtype=torch.float64).float().double() if nxt else None
    scale = 1 / math.sqrt(c)
    y, xn = hip_ops.gfpgan_torgb(_to_cb8(x, c // 8 + 1, 1, cuda), W.float().to(cuda), scale, s.float().to(cuda), b.float().to(cuda),
                                 sk.float().contiguous().to(cuda) if skip else None, sn.float().to(cuda) if nxt else None)
    torch.cuda.synchronize()
    wn = float(np.float32(scale)) * W[None] * s[:, None]
    y64 = torch.einsum('noc,nchw->nohw', wn, x) + b.view(1, 3, 1, 1)
    a64 = torch.einsum('noc,nchw->nohw', wn.abs(), x.abs()) + b.abs().view(1, 3, 1, 1)
    if skip:
        y64 = y64 + R.up2_fir(sk)
        a64 = a64 + R.up2_fir(sk.abs())
    _check(y, y64, a64, 2 * c + 16, 'torgb')
    if nxt:
        assert torch.equal(_from_cb8(xn).float(), (x * sn[:, :, None, None]).float())
    else:
        assert xn is None


@pytest.mark.parametrize('row_stride', ['per-layer', 'repeated'])
def test_style_coefficients(cuda, row_stride):
    """sr_gfpgan_style_f32: every layer's s (and d where Q is given) for a batch of distinct latents, in one launch."""
    g = torch.Generator().manual_seed(7 if row_stride == 'repeated' else 8)
    n, nsf = 3, 256
    dims = [(512, 512, True), (512, 3, False), (512, 128, True), (128, 128, True), (64, 3, False), (16, 32, True), (24, 8, True)]
    nl = len(dims)
    lat = torch.randn(n, nl, nsf, generator=g, dtype=torch.float64).float()
    table = (_lib.GfpganStyleLayer * nl)()
    keep, outs = [], []
    for i, (cin, cout, dm) in enumerate(dims):
        A = torch.randn(cin, nsf, generator=g).float().to(cuda)
        b = (torch.rand(cin, generator=g) + 0.5).float().to(cuda)
        Q = (torch.rand(cout, cin, generator=g) * 9).float().to(cuda) if dm else None
        s = torch.full((n, cin), float('nan'), device=cuda)
        d = torch.full((n, cout), float('nan'), device=cuda) if dm else None
        row = table[i]
        row.mod_w, row.mod_b, row.cin, row.cout, row.latent_index, row.s = A.data_ptr(), b.data_ptr(), cin, cout, nl - 1 - i, s.data_ptr()
        row.wscale = 1 / math.sqrt(cin * 9)
        if dm:
            row.q, row.d = Q.data_ptr(), d.data_ptr()
        keep += [A, b, Q]
        outs.append((A, b, Q, s, d, cin, nl - 1 - i))
    latd = lat.to(cuda)
    rs = nsf if row_stride == 'per-layer' else 0
    hip_ops.gfpgan_style(latd, nl * nsf, rs, nsf, table, n)
    torch.cuda.synchronize()
    for A, b, Q, s, d, cin, k in outs:
        lk = lat[:, k if rs else 0].double()
        A64, b64 = A.double().cpu(), b.double().cpu()
        s64 = lk @ A64.t() / math.sqrt(nsf) + b64
        as64 = lk.abs() @ A64.abs().t() / math.sqrt(nsf) + b64.abs()
        _check(s.cpu(), s64, as64, 2 * nsf + 8, 's')
        if Q is not None:
            c = 1 / math.sqrt(cin * 9)
            sg = s.double().cpu()
            d64 = c / torch.sqrt(c * c * (sg ** 2) @ Q.double().cpu().t() + 1e-8)
            # relative error of the sum (2 cin + 8) EPS, halved by the square root, plus the root and the division
            rel = ((d.double().cpu() - d64) / d64).abs().max()
            assert float(rel) <= (cin + 8) * EPS, float(rel)


def test_norm_style(cuda):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 512, generator=g) * 3
    y = hip_ops.gfpgan_norm_style(x.to(cuda)).cpu().double()
    x64 = x.double()
    y64 = x64 * torch.rsqrt(x64.pow(2).mean(1, keepdim=True) + 1e-8)
    assert float(((y - y64).abs() / y64.abs().clamp_min(1e-30)).max()) <= (512 + 8) * EPS
    xi = x.to(cuda)
    hip_ops.gfpgan_norm_style(xi, out=xi)   # in place
    assert torch.equal(xi.cpu(), y.float())


# ---------------------------------------------------------------------------------------------------------------- network
def _net(cfg, sd, cuda):
    net = ira.build_network(dict(type='GFPGANv1OCR', **cfg)).to(cuda).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net


@pytest.mark.parametrize('c', list(CONFIGS))
def test_network_matches_the_reference_fixture(cuda, golden, c):
    """Image and out_rgbs within 10x the reference's own float32 distance from float64; return_rgb=False gives no out_rgbs and
    the same image; the style code and the SFT conditions follow."""
    g = golden('g_x_gfpgan')
    cfg = CONFIGS[c]
    net = _net(cfg, synth.gfpgan_state_dict(SEEDS[c], **cfg), cuda)
    x = torch.from_numpy(g[f'{c}_x']).to(cuda)
    img, rgbs = net(x, randomize_noise=False)
    tol = max(1e-5, 10 * float(g[f'{c}_image32_err']))
    assert float((img.cpu().double() - torch.from_numpy(g[f'{c}_image']).double()).abs().max()) < tol
    assert len(rgbs) == int(math.log2(cfg['input_height'])) - 2
    rtol = max(1e-5, 10 * float(g[f'{c}_rgb32_err']))
    for i, r in enumerate(rgbs):
        assert r.shape == g[f'{c}_rgb{i}'].shape
        assert float((r.cpu().double() - torch.from_numpy(g[f'{c}_rgb{i}']).double()).abs().max()) < rtol, i
    img2, rgbs2 = net(x, return_rgb=False, randomize_noise=False)
    assert rgbs2 == [] and torch.equal(img2, img)
    with torch.no_grad():
        _, _, ex = net.run_forward(x, keep=True, randomize_noise=False)
    sc = torch.from_numpy(g[f'{c}_style_code']).double()
    assert float((ex['style_code'].cpu().double() - sc).abs().max()) < 1e-4 * max(1.0, float(sc.abs().max()))
    for j, (s, t) in enumerate(ex['conditions']):
        for k, v in ((2 * j, s), (2 * j + 1, t)):
            ref = torch.from_numpy(g[f'{c}_cond{k}']).double()
            assert float((_from_cb8(v)[:, :ref.shape[1]] - ref).abs().max()) < 1e-4 * max(1.0, float(ref.abs().max())), k


def _product(cfg_hw, seed, cuda, n=2):
    cfg = dict(PRODUCT, input_width=cfg_hw[0], input_height=cfg_hw[1])
    sd = synth.gfpgan_state_dict(seed, **cfg)
    x = synth.signed_input(seed + 1, (n, 3, cfg['input_height'], cfg['input_width']))
    return cfg, sd, x


_PRODUCT_REF = {}


def _product_ref(hw):
    """(cfg, sd, x, r64, r32) of a product configuration at its two seeded images: the float64 and float32 CPU restatements are
    computed once per module run and shared by the batch-2 and batch-16 tests."""
    if hw not in _PRODUCT_REF:
        cfg, sd, x = _product(hw, 900 + hw[1], None)
        sd64 = {k: torch.from_numpy(v).double() for k, v in sd.items()}
        sd32 = {k: torch.from_numpy(v) for k, v in sd.items()}
        _PRODUCT_REF[hw] = (cfg, sd, x, R.forward(sd64, cfg, torch.from_numpy(x).double()), R.forward(sd32, cfg, torch.from_numpy(x)))
    return _PRODUCT_REF[hw]


@pytest.mark.parametrize('hw', [(256, 256), (256, 64)], ids=['256x256', '256x64'])
def test_product_configs_match_the_float64_restatement(cuda, hw):
    """The product configurations at batch 2 with seeded weights: within 10x the float32 CPU restatement's distance from
    float64."""
    cfg, sd, x, r64, r32 = _product_ref(hw)
    net = _net(cfg, sd, cuda)
    img, rgbs = net(torch.from_numpy(x).to(cuda), randomize_noise=False)
    e32 = float((r32['image'].double() - r64['image']).abs().max())
    err = float((img.cpu().double() - r64['image']).abs().max())
    assert err < max(1e-5, 10 * e32), (err, e32)
    for a, b, c32 in zip(rgbs, r64['out_rgbs'], r32['out_rgbs']):
        assert float((a.cpu().double() - b).abs().max()) < max(1e-5, 10 * float((c32.double() - b).abs().max()))


@pytest.mark.parametrize('hw', [(256, 256), (256, 64)], ids=['256x256', '256x64'])
def test_product_configs_at_the_benchmarks_batch(cuda, hw):
    """The product configurations at batch 16 (what the benchmark and inference.py at throughput run): the two seeded images
    tiled eight times.  Every one of the 16 outputs and every out_rgbs level lies within the rule above of its source image's
    float64 result (max over that image), and the eight replicas of an image are bit-identical.

    Batch 16 runs other kernel instances than batch 2 (tests/test_gfpgan_plan_host.py::test_product_decoder_instances): at 256x256
    nine of the thirteen decoder launches — the upsampling convs at 4, 8, 16, 32 and 64 rows (gfp_upconv_kernel<2,1> -> <2,2>, an
    instance the square network never takes at batch 2) and the 3x3 convs at 16, 32, 64 and 128 rows (gfp_modconv_kernel<2,1> ->
    <2,2>); at 256x64 the upsampling conv at 4 rows and the 3x3 conv at 16 rows.

    Batch 16 equals batch 2 BIT FOR BIT, and this asserts it.  The decoder guarantees it (per output element every instance
    accumulates in the order cin block, tap, MFMA k-slice: tests/test_gfpgan_ops_gpu.py).  So does the U-Net, from its dispatch:
    sr_conv3x3_f32 chooses among tile shapes of one conv_tile_f32 body (8- or 4-row tiles, the 16- and 8-column tiles over the
    stacked batch) whose chain per element is (cin block, tap, k-slice) in each; sr_conv4x4s2_f32 is four accumulating passes of
    that body in a fixed order; sr_convd_f32 as the decoder; sr_linear_fwd_f32 runs one workgroup per (output, sample); the rest
    (bilinear, axpby, pixel unshuffle, layout, channel scale, blur, ToRGB, style) is per element or per sample."""
    cfg, sd, x, r64, r32 = _product_ref(hw)
    net = _net(cfg, sd, cuda)
    xd = torch.from_numpy(x).to(cuda)
    img2, rgbs2 = net(xd, randomize_noise=False)
    img, rgbs = net(xd.repeat(8, 1, 1, 1), randomize_noise=False)
    assert img.shape[0] == 16 and len(rgbs) == len(r64['out_rgbs']) == len(rgbs2)
    pairs = [(img, img2, r64['image'], r32['image'])] + list(zip(rgbs, rgbs2, r64['out_rgbs'], r32['out_rgbs']))
    for lvl, (a, a2, b64, b32) in enumerate(pairs):
        a = a.cpu()
        tol = max(1e-5, 10 * float((b32.double() - b64).abs().max()))     # the rule of the batch-2 test, unchanged
        for i in range(16):
            err = float((a[i].double() - b64[i % 2]).abs().max())
            assert err < tol, (lvl, i, err, tol)
            assert torch.equal(a[i], a[i % 2]), (lvl, i)
        assert torch.equal(a[:2], a2.cpu()), (lvl, float((a[:2] - a2.cpu()).abs().max()))
        bad = a[:2].clone()
        bad.view(-1).view(torch.int32)[-1] ^= 1            # negative controls: one flipped bit, one element off by twice the rule
        assert not torch.equal(bad, a2.cpu())
        bad = a[15].double().clone()
        bad.view(-1)[0] += 2 * tol
        assert not float((bad - b64[1]).abs().max()) < tol


def test_random_noise_follows_the_documented_draws(cuda):
    """randomize_noise=True under torch.manual_seed: the restatement fed the same draws (regenerated in layer order) agrees;
    two unseeded calls differ."""
    c = 'sq'
    cfg = CONFIGS[c]
    sd = synth.gfpgan_state_dict(SEEDS[c], **cfg)
    net = _net(cfg, sd, cuda)
    x = torch.from_numpy(synth.signed_input(77, (2, 3, 32, 32))).to(cuda)
    torch.manual_seed(1234)
    img, _ = net(x, randomize_noise=True)
    torch.manual_seed(1234)
    noises = [torch.empty((2, 1, h, w), device=cuda).normal_() for h, w in R.noise_shapes(cfg)]
    sd64 = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    sd32 = {k: torch.from_numpy(v) for k, v in sd.items()}
    r64 = R.forward(sd64, cfg, x.cpu().double(), noises=[z.cpu().double() for z in noises])
    r32 = R.forward(sd32, cfg, x.cpu(), noises=[z.cpu() for z in noises])
    e32 = float((r32['image'].double() - r64['image']).abs().max())
    assert float((img.cpu().double() - r64['image']).abs().max()) < max(1e-5, 10 * e32)
    stored, _ = net(x, randomize_noise=False)
    assert not torch.equal(stored, img)
    a, _ = net(x)
    b, _ = net(x)
    assert not torch.equal(a, b)


def test_checkpoint_round_trip_and_determinism(cuda, tmp_path):
    """A BasicSR {'params_ema': sd} file loads with strict=True through load_generator_weights and reproduces the output;
    reruns are bit-identical; eval mode without no_grad gives no grad_fn; train mode with grad raises."""
    from image_restoration_amd.utils.checkpoint import load_generator_weights
    c = 'rect'
    cfg = CONFIGS[c]
    sd = synth.gfpgan_state_dict(SEEDS[c], **cfg)
    net = _net(cfg, sd, cuda)
    x = torch.from_numpy(synth.signed_input(5, (3, 3, 16, 64))).to(cuda)
    y1, r1 = net(x, randomize_noise=False)
    y2, r2 = net(x, randomize_noise=False)
    assert torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(r1, r2))
    assert y1.grad_fn is None and not y1.requires_grad
    path = str(tmp_path / 'net_g.pth')
    torch.save({'params_ema': {k: torch.from_numpy(v) for k, v in sd.items()}}, path)
    torch.manual_seed(9)
    net2 = ira.build_network(dict(type='GFPGANv1OCR', **cfg))
    load_generator_weights(net2, path, strict=True)
    net2 = net2.to(cuda).eval()
    y3, _ = net2(x, randomize_noise=False)
    assert torch.equal(y1, y3)
    net2.train()
    with pytest.raises(NotImplementedError):
        net2(x)
    with torch.no_grad():
        y4, _ = net2(x, randomize_noise=False)
    assert torch.equal(y1, y4)


def test_inference_script_end_to_end(cuda, tmp_path):
    """inference.py --arch GFPGANv1OCR on a PNG: output size and uint8 values equal the tensor path's."""
    from PIL import Image
    from image_restoration_amd import inference
    from image_restoration_amd.utils.img_util import tensor2img
    c = 'sq'
    cfg = CONFIGS[c]
    sd = synth.gfpgan_state_dict(SEEDS[c], **cfg)
    path = str(tmp_path / 'g.pth')
    torch.save({'params_ema': {k: torch.from_numpy(v) for k, v in sd.items()}}, path)
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    src, dst = str(tmp_path / 'in.png'), str(tmp_path / 'out.png')
    Image.fromarray(img).save(src)
    argv = ['--arch', 'GFPGANv1OCR', '--input', src, '--output', dst, '--model_path', path, '--input_width', '32', '--input_height',
            '32', '--num_style_feat', '64', '--channel_multiplier', '0.5', '--num_mlp', '2', '--narrow', '0.0625']
    r = subprocess.run([sys.executable, '-m', 'image_restoration_amd.inference'] + argv, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.asarray(Image.open(dst).convert('RGB'))
    assert out.shape == img.shape
    net = _net(cfg, sd, cuda)
    ref = inference.gfpgan_restore(net, np.ascontiguousarray(img[:, :, ::-1]), randomize_noise=False)
    assert np.array_equal(out, ref[:, :, ::-1])
