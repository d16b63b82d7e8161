"""Every kernel instance of include/sr_hip_gfpgan.h against float64, on the path production takes to it.

sr_gfpgan_modconv_f32 and sr_gfpgan_upconv_f32 run gfp_modconv_kernel<COT, PT> / gfp_upconv_kernel<COT, PT> (gfpgan_ops.hip):
COT 32-cout sub-tiles per workgroup, tiles of 4 * PT rows x 32 columns, `groups` workgroup columns over cout (group `cog` reads
its weights at cog * cin_blocks * W_CHUNK).  The choice cannot be observed on the device (every launch has profiler id 92 / 93), so
it is restated here from modconv_common (_modconv_instance) and pinned on the host by tests/test_gfpgan_plan_host.py: the
instance sets the restatement can produce are the ones the code object holds, and the product networks' launches are the
instances DESIGN §16 lists.  Every case below names the instance, group count and tile counts it must reach and asserts them
against the restatement, so that a change of the 256-workgroup threshold fails here instead of silently testing something else;
_assert_coverage (run on the host too) checks the lists reach all eight instances, each with >= 2 groups, each COT with a last
group that is partly past cout, each 8-row instance with >= 3 row and >= 3 column tiles whose last ones are partial, the
upsampling conv at w = 32 and 64 (a last column tile of one column) and h = 1 and 3 (8-row tiles on a 2..4-row grid), and
xcd_tile with fewer than 8 workgroups and with a count that is not a multiple of 8.

Bounds are the ones tests/test_gfpgan_gpu.py derives, unchanged: EPS = 2^-24, A the same operation on absolute values in
float64, |y - y64| <= k EPS A + EPS |y64| with k = 2 * taps * cin_pad + 16 (+ 16 for the blur; + 4 for the raw map), k = 2 C + 16
for ToRGB, 2 nsf + 8 for s, a relative (cin + 8) EPS for d and (nsf + 8) EPS for NormStyleCode.  The float64 side uses the
float32-rounded act_slope, alpha and noise_strength the device receives.

Method.  Source, output, the raw (2h+1) x (2w+1) map, the map sr_gfpgan_blur_up_f32 reads and both SFT tensors are CB8 windows
inside NaN-filled buffers with blocks before and after the window (so every image stride is larger than the dense one).  After a
launch every slack element still has the NaN's bits and every window element is finite: each element of the raw map is written,
by the parity that owns it.  Besides Gaussian data every case runs an input that is zero except for single spikes on the rows
and columns on either side of the tile boundaries (y = 3, 4, 7, 8, x = 31, 32, the first and last row and column), in the first
and last channel of each cin block, against random weights: a wrong halo row, tap-to-parity assignment or group offset shows at
single pixels.  The tail options of test_gfpgan_gpu.TAIL_OPTS are crossed with the instances, with act_slope in {0, 0.1, 0.2, 1},
alpha in {1, 1.3, sqrt 2}, noise_strength in {0, 0.37, -0.5} and sft_c0 in {0, cout / 2, cout - 8}.

Bit-exact links.  Per output element the accumulation order is (cin block, tap, MFMA k-slice) in every instance and the tail
is elementwise, so one sample gives the same bits alone (4-row tiles) and replicated until the launch takes 8-row tiles
(test_instances_agree_bit_for_bit): the link between the batch-2 and the batch-16 network.  noise_strength = 0 with a finite
noise map equals no noise.  With act_slope = 1, alpha = 1, demod = 1, bias = 0 the modulated conv is a plain conv and equals
sr_convd_f32 at dilation 1 on the same packed weights BIT FOR BIT: read side by side, convd_f32_kernel and modconv_body stage the
same tiles, run the same MFMA chain (cin block, dy, dx, k-slice) and convd's epilogue (v + bias, slope, alpha) differs from the
tail (v * 1, + bias, slope, alpha) only by exact operations.

Negative controls: every family of checks is also run on a copy of the device result with one planted error (twice that
element's bound added, or the lowest bit flipped for the bit-exact and slack checks) and must fail.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from image_restoration_amd import _lib, hip_ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gfpgan_restate as R  # noqa: E402
from test_gfpgan_gpu import EPS, TAIL_OPTS, _check, _from_cb8, _seed  # noqa: E402

pytestmark = pytest.mark.gpu

SQRT2 = math.sqrt(2.0)
NAN = float('nan')
TAIL_IDS = ['plain', 'buf-half-next', 'smp-full', 'smp-half', 'buf-next']


def _cdiv(a, b):
    return -(-a // b)


def _f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------------ dispatch, restated
def _modconv_instance(up, n, cout, h, w):
    """(COT, PT, groups, tiles_x, tiles_y) of one sr_gfpgan_modconv_f32 (up = False) or sr_gfpgan_upconv_f32 (up = True) launch,
    restated from modconv_common (gfpgan_ops.hip): the grid is h x w, or (h + 1) x (w + 1) for the upsampling conv; 64-cout
    groups (COT 2) when cout rounded up to 32 is a multiple of 64, else 32-cout groups; 8-row tiles, or 4-row tiles (PT 1) when
    tiles_x * ceil(GH / 8) * n * groups * (4 parities) < 256 and GH > 4."""
    gh, gw = (h + 1, w + 1) if up else (h, w)
    r32 = (cout + 31) // 32 * 32
    gc = 64 if r32 % 64 == 0 else 32
    groups = r32 // gc
    tiles_x, tiles_y = _cdiv(gw, 32), _cdiv(gh, 8)
    small = tiles_x * tiles_y * n * groups * (4 if up else 1) < 256 and gh > 4
    if small:
        tiles_y = _cdiv(gh, 4)
    return (2 if gc == 64 else 1), (1 if small else 2), groups, tiles_x, tiles_y


# shape (n, cin, cout, h, w), the instance it must reach (COT, PT, groups, tiles_x, tiles_y), index into TAIL_OPTS, act_slope,
# alpha, noise_strength, sft_c0 rule ('half': cout // 16 * 8, 'full': 0, 'last8': cout - 8; ignored without an SFT)
MOD_CASES = [
    ((4, 8, 256, 44, 70), (2, 2, 4, 3, 6), 1, 0.2, SQRT2, 0.37, 'half'),
    ((3, 8, 96, 67, 33), (1, 1, 3, 2, 17), 2, 0.0, 1.0, -0.5, 'full'),
    ((5, 24, 192, 8, 32), (2, 1, 3, 1, 2), 3, 0.1, 1.3, 0.37, 'last8'),
    ((2, 16, 72, 21, 40), (1, 1, 3, 2, 6), 4, 1.0, 1.3, -0.5, 'half'),
    ((5, 8, 96, 44, 70), (1, 2, 3, 3, 6), 1, 0.1, 1.0, 0.37, 'last8'),
    ((5, 8, 96, 67, 33), (1, 2, 3, 2, 9), 0, 0.2, SQRT2, 0.37, 'half'),
    ((5, 8, 168, 44, 70), (2, 2, 3, 3, 6), 2, 0.2, SQRT2, 0.0, 'full'),
    ((2, 8, 168, 21, 40), (2, 1, 3, 2, 6), 3, 1.0, 1.0, -0.5, 'half'),
    ((2, 512, 512, 8, 32), (2, 1, 8, 1, 2), 1, 0.2, SQRT2, 0.37, 'half'),      # a product width
]
UP_CASES = [
    ((4, 8, 128, 19, 64), (2, 2, 2, 3, 3), 1, 0.2, SQRT2, 0.37, 'half'),
    ((2, 8, 256, 3, 33), (2, 2, 4, 2, 1), 2, 0.1, 1.0, -0.5, 'full'),          # GH = 4; 4 workgroups per parity and group
    ((3, 8, 96, 33, 32), (1, 2, 3, 2, 5), 3, 0.0, 1.3, 0.37, 'last8'),         # 30 workgroups: not a multiple of 8
    ((16, 8, 128, 4, 4), (2, 1, 2, 1, 2), 4, 1.0, 1.0, -0.5, 'half'),
    ((3, 8, 96, 19, 70), (1, 2, 3, 3, 3), 0, 0.2, SQRT2, 0.37, 'half'),
    ((2, 16, 72, 13, 21), (1, 1, 3, 1, 4), 1, 0.1, 1.3, 0.37, 'last8'),
    ((2, 8, 168, 1, 40), (2, 2, 3, 2, 1), 3, 0.2, SQRT2, 0.0, 'half'),         # GH = 2
    ((2, 8, 168, 9, 20), (2, 1, 3, 1, 3), 2, 1.0, 1.3, 0.37, 'full'),
    ((2, 512, 512, 8, 32), (2, 2, 8, 2, 2), 1, 0.2, SQRT2, 0.37, 'half'),      # a product width
]
# (cin, cout, h, w, replicas): one sample alone takes PT 1, `replicas` copies of it PT 2
MOD_REPLICATED = [(8, 64, 20, 40, 43), (16, 96, 21, 70, 10)]
UP_REPLICATED = [(8, 128, 19, 40, 6), (8, 32, 19, 64, 8)]
PLAIN_CONV = [(4, 8, 256, 44, 70), (2, 16, 72, 21, 40), (5, 8, 96, 44, 70)]


def _case_id(c):
    return '%s-%d%d-%s' % ('x'.join(map(str, c[0])), c[1][0], c[1][1], TAIL_IDS[c[2]])


def _assert_coverage():
    """The case lists reach what the module docstring says, by the restatement (no GPU needed)."""
    for up, cases in ((False, MOD_CASES), (True, UP_CASES)):
        seen, multi, partial_group, big, opts = set(), set(), set(), set(), set()
        for (n, cin, cout, h, w), want, opt, slope, alpha, ns, sft in cases:
            inst = _modconv_instance(up, n, cout, h, w)
            assert inst == want, (up, (n, cin, cout, h, w), inst, want)
            cot, pt, groups, tx, ty = inst
            gh, gw = (h + 1, w + 1) if up else (h, w)
            seen.add((cot, pt))
            if groups >= 2:
                multi.add((cot, pt))
                opts.add(opt)
                if cout % (32 * cot):
                    partial_group.add(cot)
            if pt == 2 and ty >= 3 and gh % 8 and tx >= 3 and gw % 32:
                big.add((cot, pt))
        assert seen == multi == {(1, 1), (1, 2), (2, 1), (2, 2)}, (up, seen, multi)
        assert partial_group == {1, 2}, (up, partial_group)
        assert big == {(1, 2), (2, 2)}, (up, big)
        assert opts == set(range(len(TAIL_OPTS))), (up, opts)
        assert any(c[0][1:] == (512, 512, 8, 32) and c[0][0] == 2 for c in cases)
        assert {c[3] for c in cases} >= {0.0, 0.1, 0.2, 1.0} and {c[4] for c in cases} >= {1.0, 1.3, SQRT2}
        assert {c[5] for c in cases} >= {0.0, 0.37, -0.5}
        assert {c[6] for c in cases if TAIL_OPTS[c[2]][1] != 'none'} == {'half', 'full', 'last8'}
    ws, hs, nwg = set(), set(), set()
    for (n, cin, cout, h, w), want, *_ in UP_CASES:
        ws.add(w)
        hs.add(h)
        nwg.add(want[3] * want[4] * n)
    assert {32, 64} <= ws and {1, 3} <= hs
    assert any(v < 8 for v in nwg) and any(v > 8 and v % 8 for v in nwg), nwg
    for up, reps in ((False, MOD_REPLICATED), (True, UP_REPLICATED)):
        cots = set()
        for cin, cout, h, w, rep in reps:
            one, many = _modconv_instance(up, 1, cout, h, w), _modconv_instance(up, rep, cout, h, w)
            assert one[1] == 1 and many[1] == 2 and one[0] == many[0] and one[2:4] == many[2:4], (up, cout, h, w, one, many)
            cots.add(one[0])
        assert cots == {1, 2}


# ------------------------------------------------------------------------------------------------------------- windows
def _window(t64, cuda, pre=1, post=1):
    """NCHW float64 [n, c, h, w] (c a multiple of 8) -> a CB8 window with `pre` NaN blocks before and `post` after."""
    n, c, h, w = t64.shape
    buf = torch.full((n, pre + c // 8 + post, h, w, 8), NAN, dtype=torch.float32)
    buf[:, pre:pre + c // 8] = t64.float().view(n, c // 8, 8, h, w).permute(0, 1, 3, 4, 2)
    return hip_ops.CB8(buf.to(cuda), pre, c // 8)


def _nan_window(n, c, h, w, cuda, pre=1, post=1):
    """An output window that is NaN itself: a finite element afterwards was written."""
    return hip_ops.CB8(torch.full((n, pre + c // 8 + post, h, w, 8), NAN, dtype=torch.float32, device=cuda), pre, c // 8)


def _nan_bits(dev):
    return torch.full((1,), NAN, dtype=torch.float32, device=dev).view(torch.int32)


def _slack_is_nan(buf, cb0, cbn):
    """Every element of the blocks outside [cb0, cb0 + cbn) has the bits torch.full(NaN) wrote."""
    bits = buf.view(torch.int32)
    nb = _nan_bits(buf.device)
    return bool((bits[:, :cb0] == nb).all()) and bool((bits[:, cb0 + cbn:] == nb).all())


def _window_ok(win, what):
    """Slack untouched, window finite; and the two checks see one flipped bit / one NaN (negative controls)."""
    assert _slack_is_nan(win.buf, win.cb0, win.cbn), what + ': slack written'
    inner = win.buf[:, win.cb0:win.cb0 + win.cbn]
    assert bool(torch.isfinite(inner).all()), (what + ': window elements not written or not finite',
                                               int((~torch.isfinite(inner)).sum()))
    bad = win.buf.clone()
    bad.view(torch.int32)[-1, -1, -1, -1, -1] ^= 1
    assert not _slack_is_nan(bad, win.cb0, win.cbn)
    bad = win.buf.clone()
    bad.view(torch.int32)[0, 0, 0, 0, 0] ^= 1
    assert not _slack_is_nan(bad, win.cb0, win.cbn)


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _check_nc(y, y64, a64, k, what):
    """_check, and its negative control: twice the bound added to one element must fail."""
    y = y.detach().double().cpu()
    _check(y, y64, a64, k, what)
    bound = k * EPS * a64 + EPS * y64.abs() + 1e-30
    i = int(torch.argmax(bound.flatten()))
    for idx in (i, y.numel() - 1):
        bad = y.clone()
        bad.view(-1)[idx] += 2 * bound.reshape(-1)[idx]
        assert _fails(lambda: _check(bad, y64, a64, k, what)), (what, 'negative control', idx)


def _equal_nc(a, b, what):
    """torch.equal, and its negative control: one flipped low bit must be seen."""
    assert a.dtype == torch.float32 and b.dtype == torch.float32
    assert torch.equal(a, b), (what, int((a != b).sum()), float((a.double() - b.double()).abs().max()))
    bad = a.clone().contiguous()
    flat = bad.view(-1).view(torch.int32)
    j = int(torch.nonzero(bad.view(-1) != 0)[0])      # not a zero: -0 and +0 compare equal
    flat[j] ^= 1
    assert not torch.equal(bad, b), (what, 'negative control')


# ---------------------------------------------------------------------------------------------------------------- tail
def _make_tail(g, n, cout, h, w, opts, cuda, slope, alpha, ns, sft_rule, plain=False):
    """-> (float64 reference dict, device tail struct, objects to keep alive, SFT windows).  (h, w): the output's size."""
    noise_mode, sft_mode, with_next = opts
    if plain:
        d = torch.ones(n, cout, dtype=torch.float64)
        bias = torch.zeros(cout, dtype=torch.float64)
    else:
        d = torch.rand(n, cout, generator=g, dtype=torch.float64) + 0.5
        bias = torch.randn(cout, generator=g, dtype=torch.float64) * 0.1
    noise = None
    if noise_mode == 'buffer':
        noise = torch.randn(1, 1, h, w, generator=g, dtype=torch.float64)
    elif noise_mode == 'sample':
        noise = torch.randn(n, 1, h, w, generator=g, dtype=torch.float64)
    sft, sft_c0, wins = None, 0, []
    if sft_mode != 'none':
        sft_c0 = {'half': cout // 16 * 8, 'full': 0, 'last8': cout - 8}[sft_rule]
        c = cout - sft_c0
        sft = (torch.randn(n, c, h, w, generator=g, dtype=torch.float64) + 1, torch.randn(n, c, h, w, generator=g, dtype=torch.float64))
        wins = [_window(sft[0], cuda, 1, 2), _window(sft[1], cuda, 2, 1)]
    s_next = torch.randn(n, cout, generator=g, dtype=torch.float64) if with_next else None
    r32 = lambda t: None if t is None else t.float().double()  # noqa: E731
    dev = dict(d=d.float().contiguous().to(cuda), noise=None if noise is None else noise.float().contiguous().to(cuda),
               bias=bias.float().contiguous().to(cuda), s_next=None if s_next is None else s_next.float().contiguous().to(cuda))
    tail = hip_ops.gfpgan_tail(dev['d'], dev['noise'], ns, tuple(wins) if wins else None, sft_c0, dev['s_next'])
    ref = dict(d=r32(d), noise=r32(noise), ns=_f32(ns), bias=r32(bias), sft=None if sft is None else (r32(sft[0]), r32(sft[1])),
               sft_c0=sft_c0, s_next=r32(s_next), slope=_f32(slope), alpha=_f32(alpha))
    return ref, tail, dev, wins


def _tail64(raw, araw, T):
    """The tail of include/sr_hip_gfpgan.h in float64 on (value, magnitude)."""
    v = raw * T['d'][:, :, None, None]
    a = araw * T['d'].abs()[:, :, None, None]
    if T['noise'] is not None:
        v = v + T['ns'] * T['noise']
        a = a + abs(T['ns']) * T['noise'].abs()
    v = F.leaky_relu(v + T['bias'].view(1, -1, 1, 1), T['slope']) * T['alpha']
    a = (a + T['bias'].abs().view(1, -1, 1, 1)) * abs(T['alpha'])
    if T['sft'] is not None:
        s, t = T['sft']
        c0 = T['sft_c0']
        v = torch.cat([v[:, :c0], v[:, c0:] * s + t], 1)
        a = torch.cat([a[:, :c0], a[:, c0:] * s.abs() + t.abs()], 1)
    if T['s_next'] is not None:
        v = v * T['s_next'][:, :, None, None]
        a = a * T['s_next'].abs()[:, :, None, None]
    return v, a


def _spikes(g, n, cin, h, w):
    """Zero except single spikes on the rows / columns on either side of the tile boundaries and on the borders, cycling over the
    samples and over the first and last channel of each cin block."""
    x = torch.zeros(n, cin, h, w, dtype=torch.float64)
    rows = sorted({0, h - 1} | {r for r in (3, 4, 7, 8) if r < h})
    cols = sorted({0, w - 1} | {c for c in (31, 32) if c < w})
    chans = [cb * 8 + e for cb in range(cin // 8) for e in (0, 7)]
    k = 0
    for r in rows:
        for c in cols:
            v = (1.0 + float(torch.rand((), generator=g))) * (1 if k % 3 else -1)
            x[k % n, chans[(k // n + k) % len(chans)], r, c] = v
            k += 1
    # every sample, and both ends of every cin block, hold a spike at the last pixel (the last tile's last element)
    for i in range(n):
        x[i, chans[i % len(chans)], h - 1, w - 1] = 1.5
    return x


def _inputs(g, shape):
    n, cin, cout, h, w = shape
    W = (torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) / math.sqrt(cin * 9)).float().double()
    gauss = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64).float().double()
    return W, [('gauss', gauss), ('spikes', _spikes(g, n, cin, h, w).float().double())]


# ---------------------------------------------------------------------------------------------- modulated 3x3 convolution
@pytest.mark.parametrize('case', MOD_CASES, ids=_case_id)
def test_modconv_instances(cuda, case):
    """sr_gfpgan_modconv_f32 at the instance, group count and tile counts the case names: Gaussian and spiked sources against
    float64, windows with NaN slack, every tail option."""
    shape, want, opt, slope, alpha, ns, sft_rule = case
    n, cin, cout, h, w = shape
    assert _modconv_instance(False, n, cout, h, w) == want
    g = torch.Generator().manual_seed(_seed('mod', shape, opt))
    W, sources = _inputs(g, shape)
    T, tail, dev, sft_wins = _make_tail(g, n, cout, h, w, TAIL_OPTS[opt], cuda, slope, alpha, ns, sft_rule)
    pc = hip_ops.PackedConvK(W.float().to(cuda), dev['bias'])
    for name, xs in sources:
        src = _window(xs, cuda, 1, 2)
        out = _nan_window(n, cout, h, w, cuda, 2, 1)
        hip_ops.gfpgan_modconv(src, pc, tail, out=out, act_slope=slope, alpha=alpha)
        torch.cuda.synchronize()
        _window_ok(out, f'modconv {name} out')
        y64, a64 = _tail64(F.conv2d(xs, W, padding=1), F.conv2d(xs.abs(), W.abs(), padding=1), T)
        _check_nc(_from_cb8(out), y64, a64, 2 * 9 * cin + 16, f'modconv {name}')
    for win in sft_wins:
        assert _slack_is_nan(win.buf, win.cb0, win.cbn)


@pytest.mark.parametrize('case', UP_CASES, ids=_case_id)
def test_upconv_blur_instances(cuda, case):
    """sr_gfpgan_upconv_f32 into a NaN window (every element of the (2h+1) x (2w+1) map written, nothing else), then
    sr_gfpgan_blur_up_f32 reading that window (t_img_stride larger than dense) with every tail option."""
    shape, want, opt, slope, alpha, ns, sft_rule = case
    n, cin, cout, h, w = shape
    assert _modconv_instance(True, n, cout, h, w) == want
    g = torch.Generator().manual_seed(_seed('up', shape, opt))
    W, sources = _inputs(g, shape)
    T, tail, dev, sft_wins = _make_tail(g, n, cout, 2 * h, 2 * w, TAIL_OPTS[opt], cuda, slope, alpha, ns, sft_rule)
    pc = hip_ops.PackedConvK(W.float().to(cuda), None)
    for name, xs in sources:
        src = _window(xs, cuda, 2, 1)
        t = _nan_window(n, cout, 2 * h + 1, 2 * w + 1, cuda, 1, 2)
        hip_ops.gfpgan_upconv(src, pc, out=t)
        torch.cuda.synchronize()
        _window_ok(t, f'upconv {name} raw map')
        raw = F.conv_transpose2d(xs, W.transpose(0, 1), stride=2)
        araw = F.conv_transpose2d(xs.abs(), W.abs().transpose(0, 1), stride=2)
        _check_nc(_from_cb8(t), raw, araw, 2 * 9 * cin + 4, f'upconv {name} raw')
        out = _nan_window(n, cout, 2 * h, 2 * w, cuda, 1, 1)
        hip_ops.gfpgan_blur_up(t, dev['bias'], tail, out=out, act_slope=slope, alpha=alpha)
        torch.cuda.synchronize()
        _window_ok(out, f'blur_up {name} out')
        assert _slack_is_nan(t.buf, t.cb0, t.cbn)
        y64, a64 = _tail64(R.fir(raw, 1, 1, 4.0), R.fir(araw, 1, 1, 4.0), T)
        _check_nc(_from_cb8(out), y64, a64, 2 * 9 * cin + 16 + 16, f'upconv + blur {name}')
    for win in sft_wins:
        assert _slack_is_nan(win.buf, win.cb0, win.cbn)


def _replicated_tail(g, rep, cout, h, w, cuda):
    """One sample's tail (demod, shared noise map, half SFT, s_next), alone and replicated `rep` times."""
    T1, _, dev1, wins1 = _make_tail(g, 1, cout, h, w, TAIL_OPTS[1], cuda, 0.2, SQRT2, 0.37, 'half')
    c0 = T1['sft_c0']
    winsr = [hip_ops.CB8(wn.buf.repeat(rep, 1, 1, 1, 1).contiguous(), wn.cb0, wn.cbn) for wn in wins1]
    devr = dict(d=dev1['d'].repeat(rep, 1).contiguous(), s_next=dev1['s_next'].repeat(rep, 1).contiguous())
    tail1 = hip_ops.gfpgan_tail(dev1['d'], dev1['noise'], 0.37, tuple(wins1), c0, dev1['s_next'])
    tailr = hip_ops.gfpgan_tail(devr['d'], dev1['noise'], 0.37, tuple(winsr), c0, devr['s_next'])
    return (tail1, tailr, dev1['bias']), (dev1, devr, wins1, winsr)


@pytest.mark.parametrize('shape', MOD_REPLICATED, ids=str)
def test_modconv_instances_agree_bit_for_bit(cuda, shape):
    """One sample alone (4-row tiles) and replicated until the launch takes 8-row tiles: identical bits on every replica."""
    cin, cout, h, w, rep = shape
    assert _modconv_instance(False, 1, cout, h, w)[1] == 1 and _modconv_instance(False, rep, cout, h, w)[1] == 2
    g = torch.Generator().manual_seed(_seed('modrep', shape))
    W, sources = _inputs(g, (1, cin, cout, h, w))
    (tail1, tailr, bias), keep = _replicated_tail(g, rep, cout, h, w, cuda)
    pc = hip_ops.PackedConvK(W.float().to(cuda), bias)
    xs = sources[0][1]
    one = hip_ops.gfpgan_modconv(_window(xs, cuda), pc, tail1)
    many = hip_ops.gfpgan_modconv(_window(xs.repeat(rep, 1, 1, 1), cuda), pc, tailr)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(one.buf).all())
    _equal_nc(many.buf[rep - 1], one.buf[0], 'modconv last replica')
    for i in range(rep):
        assert torch.equal(many.buf[i], one.buf[0]), i


@pytest.mark.parametrize('shape', UP_REPLICATED, ids=str)
def test_upconv_instances_agree_bit_for_bit(cuda, shape):
    """The raw map and the blurred output of one sample, alone (4-row tiles) and replicated (8-row tiles): identical bits."""
    cin, cout, h, w, rep = shape
    assert _modconv_instance(True, 1, cout, h, w)[1] == 1 and _modconv_instance(True, rep, cout, h, w)[1] == 2
    g = torch.Generator().manual_seed(_seed('uprep', shape))
    W, sources = _inputs(g, (1, cin, cout, h, w))
    (tail1, tailr, bias), keep = _replicated_tail(g, rep, cout, 2 * h, 2 * w, cuda)
    pc = hip_ops.PackedConvK(W.float().to(cuda), None)
    xs = sources[0][1]
    t1 = hip_ops.gfpgan_upconv(_window(xs, cuda), pc)
    tr = hip_ops.gfpgan_upconv(_window(xs.repeat(rep, 1, 1, 1), cuda), pc)
    o1 = hip_ops.gfpgan_blur_up(t1, bias, tail1)
    orr = hip_ops.gfpgan_blur_up(tr, bias, tailr)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(t1.buf).all()) and bool(torch.isfinite(o1.buf).all())
    _equal_nc(tr.buf[rep - 1], t1.buf[0], 'upconv last replica')
    for i in range(rep):
        assert torch.equal(tr.buf[i], t1.buf[0]) and torch.equal(orr.buf[i], o1.buf[0]), i


@pytest.mark.parametrize('up', [False, True], ids=['modconv', 'upconv'])
def test_zero_noise_strength_equals_no_noise(cuda, up):
    """noise_strength = 0 with a finite per-sample noise map changes no bit (v + 0 * z == v)."""
    shape = (2, 16, 72, 13, 21)
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(_seed('ns0', up))
    W, sources = _inputs(g, shape)
    xs = sources[0][1]
    oh, ow = (2 * h, 2 * w) if up else (h, w)
    d = (torch.rand(n, cout, generator=g) + 0.5).to(cuda)
    bias = (torch.randn(cout, generator=g) * 0.1).to(cuda)
    noise = torch.randn(n, 1, oh, ow, generator=g).to(cuda)
    res = []
    for tail in (hip_ops.gfpgan_tail(d), hip_ops.gfpgan_tail(d, noise, 0.0)):
        if up:
            t = hip_ops.gfpgan_upconv(_window(xs, cuda), hip_ops.PackedConvK(W.float().to(cuda), None))
            res.append(hip_ops.gfpgan_blur_up(t, bias, tail).buf)
        else:
            res.append(hip_ops.gfpgan_modconv(_window(xs, cuda), hip_ops.PackedConvK(W.float().to(cuda), bias), tail).buf)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(res[0]).all())
    _equal_nc(res[1], res[0], 'zero noise strength')


@pytest.mark.parametrize('shape', PLAIN_CONV, ids=str)
def test_plain_modconv_equals_convd_bit_for_bit(cuda, shape):
    """act_slope = 1, alpha = 1, demod = 1, bias = 0, no other option: sr_gfpgan_modconv_f32 is a plain 3x3 conv and equals
    sr_convd_f32 at dilation 1 on the same packed weights bit for bit — the same staging, MFMA chain (cin block, dy, dx,
    k-slice) and, up to the exact v * 1 and v + 0, epilogue order (ridnet_ops.hip convd_f32_kernel against modconv_body; both
    take the same instance, their dispatch rules being the same function of the same numbers).  Both also match float64."""
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(_seed('plain', shape))
    W, sources = _inputs(g, shape)
    T, tail, dev, _ = _make_tail(g, n, cout, h, w, TAIL_OPTS[0], cuda, 1.0, 1.0, 0.0, 'half', plain=True)
    pc = hip_ops.PackedConvK(W.float().to(cuda), dev['bias'])
    for name, xs in sources:
        a = hip_ops.gfpgan_modconv(_window(xs, cuda), pc, tail, act_slope=1.0, alpha=1.0)
        b = hip_ops.convd(_window(xs, cuda, 2, 1), pc, 1, act_slope=1.0, alpha=1.0)
        torch.cuda.synchronize()
        _equal_nc(a.buf, b.buf, f'plain conv {name}')
        y64, a64 = F.conv2d(xs, W, padding=1), F.conv2d(xs.abs(), W.abs(), padding=1)
        _check_nc(_from_cb8(a), y64, a64, 2 * 9 * cin + 16, f'plain modconv {name}')


def test_case_lists_reach_every_instance():
    _assert_coverage()


# ------------------------------------------------------------------------------------------------------- blur on its own
def _coverage(size_out, size_t):
    k = [0.25, 0.75, 0.75, 0.25]
    return torch.tensor([sum(k[a] for a in range(4) if 0 <= y + a - 1 < size_t) for y in range(size_out)], dtype=torch.float64)


@pytest.mark.parametrize('shape', [(2, 16, 5, 7), (3, 8, 1, 1), (1, 24, 3, 34)], ids=str)
def test_blur_up_on_its_own(cuda, shape):
    """sr_gfpgan_blur_up_f32 on a map this test writes, in a NaN-padded window: t = 1 with an identity tail gives the closed-form
    coverage of the 4x4 kernel (interior 4, edges 3.5, corners 3.0625 — exact in fp32); single integer spikes in the first and
    last row and column of the (2h+1) x (2w+1) map give the float64 FIR exactly."""
    n, cout, h, w = shape
    ht, wt = 2 * h + 1, 2 * w + 1
    one = torch.ones(n, cout, dtype=torch.float32, device=cuda)
    bias = torch.zeros(cout, dtype=torch.float32, device=cuda)
    tail = hip_ops.gfpgan_tail(one)
    ones = torch.ones(n, cout, ht, wt, dtype=torch.float64)
    sp = torch.zeros(n, cout, ht, wt, dtype=torch.float64)
    k = 0
    for r in sorted({0, 1, ht // 2, ht - 2, ht - 1}):
        for c in sorted({0, 1, wt // 2, wt - 2, wt - 1}):
            if r in (0, ht - 1) or c in (0, wt - 1):
                sp[k % n, (k * 5) % cout, r, c] = float(k % 7 + 1) * (-1) ** k
                k += 1
    cov = torch.outer(_coverage(2 * h, ht), _coverage(2 * w, wt))
    if h > 1 and w > 1:
        assert float(cov[1, 1]) == 4.0 and float(cov[0, 1]) == 3.5 and float(cov[0, 0]) == 3.0625
    for name, t64, want in (('ones', ones, cov.expand(n, cout, -1, -1)), ('spikes', sp, R.fir(sp, 1, 1, 4.0))):
        t = _window(t64, cuda, 2, 3)
        out = _nan_window(n, cout, 2 * h, 2 * w, cuda, 1, 2)
        hip_ops.gfpgan_blur_up(t, bias, tail, out=out, act_slope=1.0, alpha=1.0)
        torch.cuda.synchronize()
        _window_ok(out, f'blur_up alone {name}')
        assert _slack_is_nan(t.buf, t.cb0, t.cbn)
        _equal_nc(_from_cb8(out).float(), want.float().contiguous(), f'blur_up alone {name}')


# ------------------------------------------------------------------------------------------------------------------ ToRGB
def _flat_guarded(numel, cuda, guard=64):
    return torch.full((numel + 2 * guard,), NAN, dtype=torch.float32, device=cuda), guard


@pytest.mark.parametrize('data', ['gauss', 'spiked-skip'])
@pytest.mark.parametrize('shape', [(3, 8, 10, 14), (3, 512, 10, 14), (2, 8, 2, 2), (2, 512, 2, 2)], ids=str)
def test_torgb_edges(cuda, shape, data):
    """sr_gfpgan_torgb_f32 through the raw entry point: x and x_next in NaN-slack windows, y between guard bands, h * w not a
    multiple of 256 and 2x2 with a 1x1 skip; 'spiked-skip' has x = 0 and a skip that is zero but for its corners and edge
    midpoints, so the two-tap border form is compared pixel by pixel at a bound of a few EPS."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(_seed('rgb', shape, data))
    r32 = lambda t: t.float().double()  # noqa: E731
    Wt = r32(torch.randn(3, c, generator=g, dtype=torch.float64))
    s = r32(torch.rand(n, c, generator=g, dtype=torch.float64) + 0.5)
    b = r32(torch.randn(3, generator=g, dtype=torch.float64) * 0.1)
    sn = r32(torch.randn(n, c, generator=g, dtype=torch.float64))
    h2, w2 = h // 2, w // 2
    if data == 'gauss':
        x = r32(torch.randn(n, c, h, w, generator=g, dtype=torch.float64))
        sk = r32(torch.randn(n, 3, h2, w2, generator=g, dtype=torch.float64))
    else:
        x = torch.zeros(n, c, h, w, dtype=torch.float64)
        sk = torch.zeros(n, 3, h2, w2, dtype=torch.float64)
        k = 0
        for r in sorted({0, h2 // 2, h2 - 1}):
            for cc in sorted({0, w2 // 2, w2 - 1}):
                if r in (0, h2 - 1) or cc in (0, w2 - 1):
                    sk[k % n, k % 3, r, cc] = r32(torch.tensor(1.0 + 0.37 * k, dtype=torch.float64)) * (-1) ** k
                    k += 1
    scale = 1 / math.sqrt(c)
    xw = _window(x, cuda, 1, 2)
    xn = _nan_window(n, c, h, w, cuda, 2, 1)
    ybuf, guard = _flat_guarded(n * 3 * h * w, cuda)
    dv = lambda t: t.float().contiguous().to(cuda)  # noqa: E731
    Wd, sd, bd, skd, snd = dv(Wt), dv(s), dv(b), dv(sk), dv(sn)
    lib = _lib.load()
    with torch.cuda.device(cuda):
        _lib.check(lib.sr_gfpgan_torgb_f32(xw.ptr, xw.img_stride, Wd.data_ptr(), float(scale), sd.data_ptr(), bd.data_ptr(),
                                           skd.data_ptr(), ybuf.data_ptr() + guard * 4, xn.ptr, xn.img_stride, snd.data_ptr(), n, c, h, w,
                                           hip_ops._stream(cuda)), 'sr_gfpgan_torgb_f32')
    torch.cuda.synchronize()
    nb = _nan_bits(cuda)
    bits = ybuf.view(torch.int32)
    assert bool((bits[:guard] == nb).all()) and bool((bits[-guard:] == nb).all())
    y = ybuf[guard:-guard].view(n, 3, h, w)
    assert bool(torch.isfinite(y).all())
    _window_ok(xn, 'torgb x_next')
    assert _slack_is_nan(xw.buf, xw.cb0, xw.cbn)
    wn = _f32(scale) * Wt[None] * s[:, None]
    y64 = torch.einsum('noc,nchw->nohw', wn, x) + b.view(1, 3, 1, 1) + R.up2_fir(sk)
    a64 = torch.einsum('noc,nchw->nohw', wn.abs(), x.abs()) + b.abs().view(1, 3, 1, 1) + R.up2_fir(sk.abs())
    _check_nc(y, y64, a64, 2 * c + 16, f'torgb {data}')
    if data == 'gauss':
        _equal_nc(_from_cb8(xn).float(), (x * sn[:, :, None, None]).float(), 'torgb x_next')
    assert torch.equal(_from_cb8(xn).float(), (x * sn[:, :, None, None]).float())


# ------------------------------------------------------------------------------------------------------ style coefficients
def _slab(numel, cuda, pad=8):
    """A NaN buffer of numel + 2 * pad floats; the output lives at [pad, pad + numel)."""
    return torch.full((numel + 2 * pad,), NAN, dtype=torch.float32, device=cuda), pad


def _slab_ok(buf, pad, what):
    nb = _nan_bits(buf.device)
    bits = buf.view(torch.int32)
    assert bool((bits[:pad] == nb).all()) and bool((bits[-pad:] == nb).all()), what + ': slack written'
    assert bool(torch.isfinite(buf[pad:-pad]).all()), what + ': not written'


def _run_style(cuda, g, n, nsf, dims, row_stride, lat, A_scale=1.0, b_of=None):
    """One sr_gfpgan_style_f32 launch over `dims` = [(cin, cout, demodulate)]; latent row k of layer i is len(dims) - 1 - i.
    -> per layer (A, b, Q, s, d, cin, cout, k, wscale) with s / d the written parts of NaN slabs, all on the CPU."""
    nl = len(dims)
    table = (_lib.GfpganStyleLayer * nl)()
    keep, outs = [], []
    for i, (cin, cout, dm) in enumerate(dims):
        A = (torch.randn(cin, nsf, generator=g) * A_scale).float()
        b = (torch.rand(cin, generator=g) + 0.5).float() if b_of is None else b_of(i, cin)
        Q = (torch.rand(cout, cin, generator=g) * 9).float() if dm else None
        sb, pad = _slab(n * cin, cuda)
        db = _slab(n * cout, cuda)[0] if dm else None
        Ad, bd, Qd = A.to(cuda), b.to(cuda), (Q.to(cuda) if dm else None)
        row = table[i]
        row.mod_w, row.mod_b, row.cin, row.cout, row.latent_index = Ad.data_ptr(), bd.data_ptr(), cin, cout, nl - 1 - i
        row.s = sb.data_ptr() + pad * 4
        row.wscale = 1 / math.sqrt(cin * 9)
        if dm:
            row.q, row.d = Qd.data_ptr(), db.data_ptr() + pad * 4
        keep += [Ad, bd, Qd]
        outs.append((A, b, Q, sb, db, cin, cout, nl - 1 - i, float(row.wscale)))
    hip_ops.gfpgan_style(lat, lat.stride(0), row_stride, nsf, table, n)
    torch.cuda.synchronize()
    res = []
    for A, b, Q, sb, db, cin, cout, k, ws in outs:
        _slab_ok(sb, 8, 's')
        s = sb[8:-8].view(n, cin).cpu()
        d = None
        if db is not None:
            _slab_ok(db, 8, 'd')
            d = db[8:-8].view(n, cout).cpu()
        res.append((A, b, Q, s, d, cin, cout, k, ws))
    return res


def _check_style(res, lat_rows, nsf, row_stride):
    """s against float64 (k = 2 nsf + 8); d against float64 from the device's own s, relative (cin + 8) EPS; each with its
    negative control."""
    for A, b, Q, s, d, cin, cout, k, ws in res:
        lk = lat_rows[:, k if row_stride else 0].double()
        A64, b64 = A.double(), b.double()
        s64 = lk @ A64.t() / math.sqrt(nsf) + b64
        as64 = lk.abs() @ A64.abs().t() / math.sqrt(nsf) + b64.abs()
        _check_nc(s, s64, as64, 2 * nsf + 8, 's')
        if Q is not None:
            d64 = ws / torch.sqrt(ws * ws * (s.double() ** 2) @ Q.double().t() + 1e-8)
            rel = ((d.double() - d64) / d64).abs()
            assert float(rel.max()) <= (cin + 8) * EPS, (cin, cout, float(rel.max()))
            bad = d.double().clone()
            bad[-1, -1] += 2 * (cin + 8) * EPS * d64[-1, -1]
            assert float(((bad - d64) / d64).abs().max()) > (cin + 8) * EPS


def _latent(g, n, nl, nsf, cuda, scale=1.0, gap=24):
    """[n, nl * nsf + gap] with NaN in the gap: an image stride larger than dense.  -> (device tensor, CPU rows [n, nl, nsf])."""
    rows = (torch.randn(n, nl, nsf, generator=g) * scale).float()
    buf = torch.full((n, nl * nsf + gap), NAN, dtype=torch.float32)
    buf[:, :nl * nsf] = rows.view(n, -1)
    return buf.to(cuda), rows


STYLE_DIMS = ([(512, 512, True), (512, 3, False), (8, 16, True), (24, 10, True), (8, 3, False), (512, 8, True), (16, 510, True),
               (40, 6, True)] + [(8 * (i % 5 + 1), 4 * i + 3, i % 3 != 0) for i in range(24)])


@pytest.mark.parametrize('row_stride', ['per-layer', 'repeated'])
@pytest.mark.parametrize('n', [1, 5])
@pytest.mark.parametrize('nsf', [32, 100, 1024])
def test_style_shapes(cuda, nsf, n, row_stride):
    """sr_gfpgan_style_f32 at its limits: a table of SR_GFPGAN_MAX_LAYERS = 32 layers with cin = cout = 512, cin = 8 and couts
    that are not multiples of 4; nsf 32, 100 (not a multiple of 64) and 1024; n 1 and 5; latent row stride nsf and 0, its image
    stride larger than dense with NaN in the gap (and, at row stride 0, NaN in every row but the first); every s and d in NaN
    slack."""
    assert len(STYLE_DIMS) == 32
    g = torch.Generator().manual_seed(_seed('style', nsf, n, row_stride))
    nl = len(STYLE_DIMS)
    lat, rows = _latent(g, n, nl, nsf, cuda)
    rs = nsf
    if row_stride == 'repeated':
        rs = 0
        lat[:, nsf:] = NAN
    res = _run_style(cuda, g, n, nsf, STYLE_DIMS, rs, lat)
    _check_style(res, rows, nsf, rs)


def test_style_demodulation_eps(cuda):
    """The 1e-8 inside the demodulation root: latents and mod_b scaled so that wscale^2 sum s^2 Q lies in [1e-9, 1e-7], where
    dropping the 1e-8 (or applying it outside the wscale^2 scaling) moves d by more than 5 % against a bound of (cin + 8) EPS."""
    n, nsf = 3, 256
    dims = [(64, 64, True), (128, 24, True), (64, 32, True), (32, 40, True)]
    g = torch.Generator().manual_seed(_seed('style-eps'))
    lat, rows = _latent(g, n, len(dims), nsf, cuda, scale=2e-5)
    res = _run_style(cuda, g, n, nsf, dims, nsf, lat,
                     b_of=lambda i, cin: (1.5e-4 * (0.75 + 0.5 * torch.rand(cin, generator=g))).float())
    _check_style(res, rows, nsf, nsf)
    for A, b, Q, s, d, cin, cout, k, ws in res:
        t = ws * ws * (s.double() ** 2) @ Q.double().t()
        assert 1e-9 <= float(t.min()) and float(t.max()) <= 1e-7, (float(t.min()), float(t.max()))
        d64 = ws / torch.sqrt(t + 1e-8)
        for wrong in (ws / torch.sqrt(t), ws / torch.sqrt(t + 1e-8 * ws * ws), ws / torch.sqrt(t + 1e-8 / (ws * ws))):
            assert float(((wrong - d64) / d64).abs().min()) > 0.05


def test_style_zero_modulation(cuda):
    """A layer with s = 0 exactly (zero latent row, zero mod_b) between ordinary ones: s is 0 and d = wscale * 1e4, finite."""
    n, nsf = 2, 64
    dims = [(16, 24, True), (64, 40, True), (32, 8, True)]
    zero_layer = 1
    zk = len(dims) - 1 - zero_layer
    g = torch.Generator().manual_seed(_seed('style-zero'))
    lat, rows = _latent(g, n, len(dims), nsf, cuda)
    rows[:, zk] = 0
    lat[:, zk * nsf:(zk + 1) * nsf] = 0
    res = _run_style(cuda, g, n, nsf, dims, nsf, lat,
                     b_of=lambda i, cin: torch.zeros(cin) if i == zero_layer else (torch.rand(cin, generator=g) + 0.5).float())
    _check_style(res, rows, nsf, nsf)
    A, b, Q, s, d, cin, cout, k, ws = res[zero_layer]
    assert float(s.abs().max()) == 0.0
    assert float((d.double() / (ws * 1e4) - 1).abs().max()) <= (cin + 8) * EPS


# ------------------------------------------------------------------------------------------------------------ NormStyleCode
@pytest.mark.parametrize('nsf', [1, 100, 512, 1024])
def test_norm_style_edges(cuda, nsf):
    """sr_gfpgan_norm_style_f32: a Gaussian row, a row of zeros (exactly 0, no NaN), a row with mean x^2 ~ 1e-8 (eps visible), rows
    scaled by 1e15 (the relative bound holds) and 1e-15 (eps dominates: y = x * 1e4); output in NaN slack; in place == out of
    place."""
    g = torch.Generator().manual_seed(_seed('norm', nsf))
    base = torch.randn(6, nsf, generator=g)
    base[base.abs() < 0.05] = 0.5
    base.clamp_(-2, 2)
    x = torch.stack([base[0] * 3, torch.zeros(nsf), base[2] * 1e-4, base[3] * 1e15, base[4] * 1e-15, base[5]]).float().contiguous()
    n = x.shape[0]
    xd = x.to(cuda)
    yb, pad = _slab(n * nsf, cuda)
    lib = _lib.load()
    with torch.cuda.device(cuda):
        _lib.check(lib.sr_gfpgan_norm_style_f32(xd.data_ptr(), yb.data_ptr() + pad * 4, n, nsf, hip_ops._stream(cuda)),
                   'sr_gfpgan_norm_style_f32')
    torch.cuda.synchronize()
    _slab_ok(yb, pad, 'norm_style')
    y = yb[pad:-pad].view(n, nsf).cpu()
    x64 = x.double()
    m = x64.pow(2).mean(1, keepdim=True)
    y64 = x64 * torch.rsqrt(m + 1e-8)
    assert float(y[1].abs().max()) == 0.0
    err = (y.double() - y64).abs()
    bound = (nsf + 8) * EPS * y64.abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    bad = y.double().clone()
    bad[0, -1] += 2 * bound[0, -1]
    assert not bool(((bad - y64).abs() <= bound).all())
    # eps is visible in row 2 and dominates in row 4
    assert float((x64[2] * torch.rsqrt(m[2]) / y64[2] - 1).abs().min()) > 0.05
    assert float((y64[4] / (x64[4] * 1e4) - 1).abs().max()) < 1e-9
    assert float((y[4].double() / (x64[4] * 1e4) - 1).abs().max()) <= (nsf + 8) * EPS
    xi = x.to(cuda)
    hip_ops.gfpgan_norm_style(xi, out=xi)
    out = hip_ops.gfpgan_norm_style(x.to(cuda))
    torch.cuda.synchronize()
    _equal_nc(xi.cpu(), y, 'norm_style in place')
    assert torch.equal(out.cpu(), y)
