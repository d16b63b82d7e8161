"""The entry points of include/sr_hip_duf.h on the GPU, each against float64 of that one op on every element.  EPS = 2^-24.

  conv3d  nn.Conv3d(cin, cout, (kt, 3, 3), 1, (pad_t, 1, 1)) in float64 (torch on the CPU) on the operand the kernel sees — the
          prologue max(x * scale + shift, 0) computed in fp32 with those three operations — with the bound the header derives from
          its summation order:  |got - exact| <= (K + 2) * EPS * (sum |w x| + |bias|),  K = 9 * kt * cin_pad.
          The source's channels beyond cin and the destination outside the written slice are NaN beforehand: the output must be
          finite and the rest of the destination must keep its bit pattern.
  pw      the same with K = cin.
  filter  softmax over the 25 taps, the 5x5 window of the centre frame, + res, pixel shuffle.  The device's expf enters, so the
          tolerance is MARGIN = 10 (tests/test_tof_gpu.py) times the distance of torch's fp32 CPU result of the reference's op
          sequence from float64 on the same inputs.
All three: a rerun is bit-equal and a batch of two equals two single runs bit for bit; for the convolutions clip 0 of a batch does
not change by a bit when clip 1 is filled with 1e30 (nothing leaks across the clip boundary).
The largest error / bound of each case is printed (run with -s)."""
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import duf_restate as D  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
TINY = 1e-30
NAN = float('nan')
MARGIN = 10.0


def _bits(t):
    return t.contiguous().view(torch.int32)


def _clip_buffer(x, cuda, after=1):
    """[b, c, t, h, w] numpy -> frame-major CB8 buffer [b, t, cb + after, h, w, 8]; pad channels and slack blocks are NaN."""
    b, c, t, h, w = x.shape
    cb = (c + 7) // 8
    xp = torch.full((b, cb * 8, t, h, w), NAN, dtype=torch.float32)
    xp[:, :c] = torch.from_numpy(np.asarray(x, np.float32))
    buf = torch.full((b, t, cb + after, h, w, 8), NAN, dtype=torch.float32)
    buf[:, :, :cb] = xp.reshape(b, cb, 8, t, h, w).permute(0, 3, 1, 4, 5, 2)
    return H.ClipCB8(buf.to(cuda))


def _read(buf, cb0, cbn):
    """[b, t, CB, h, w, 8] -> [b, 8 cbn, t, h, w] of the blocks [cb0, cb0 + cbn)."""
    v = buf[:, :, cb0:cb0 + cbn].cpu()
    b, t, n, h, w, _ = v.shape
    return v.permute(0, 2, 5, 1, 3, 4).reshape(b, n * 8, t, h, w)


def _prologue_fp32(x, scale, shift):
    """max(x * scale + shift, 0) in fp32: one multiply, one add, one max, each rounded."""
    s, t = (v.astype(np.float32).reshape(1, -1, 1, 1, 1) for v in (scale, shift))
    prod = (x.astype(np.float32) * s).astype(np.float32)
    return np.maximum((prod + t).astype(np.float32), np.float32(0))


def _conv64(x, wt, b, pad_t, pad_s):
    """(float64 conv, sum of |terms|) with torch on the CPU."""
    x64, w64, b64 = torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double()
    out = F.conv3d(x64, w64, b64, 1, (pad_t, pad_s, pad_s))
    mag = F.conv3d(x64.abs(), w64.abs(), b64.abs(), 1, (pad_t, pad_s, pad_s))
    return out.numpy(), mag.numpy()


def _check_conv(cuda, who, run, pc, x, wt, b, kt, pad_t, pad_s, prologue, relu, out_cb0):
    """Runs ``run(src, pc, dst, out_cb0, ...)`` on NaN-surrounded buffers and checks everything the module docstring lists."""
    bsz, cin, t, h, w = x.shape
    cout = wt.shape[0]
    rng = np.random.default_rng(7)
    pro = None
    operand = x
    if prologue:
        scale, shift = rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.uniform(0.1, 0.6, cin).astype(np.float32)   # shift > 0
        operand = _prologue_fp32(x, scale, shift)
        pro = (torch.from_numpy(scale).to(cuda), torch.from_numpy(shift).to(cuda))
    want, mag = _conv64(operand, wt, b, pad_t, pad_s)
    if relu:
        want = np.maximum(want, 0)
    tout = want.shape[2]
    t0 = (t - tout) // 2                                       # the destination window of cat(x[:, :, 1:-1], conv(x))
    cinp = (cin + 7) // 8 * 8
    bound = ((9 * kt * cinp if pad_s else cinp) + 2) * EPS * mag + TINY              # K = 9 kt cin_pad; K = cin for the 1x1x1 conv

    def launch(xs):
        src = _clip_buffer(xs, cuda)
        dst = H.ClipCB8(torch.full((xs.shape[0], t, out_cb0 + cout // 8 + 1, h, w, 8), NAN, dtype=torch.float32, device=cuda))
        run(src, pc, dst.frames(t0, tout), out_cb0, prologue=pro, relu=relu, **({'pad_t': pad_t} if pad_s else {}))
        return dst.buf

    buf = launch(x)
    got = _read(buf[:, t0:t0 + tout], out_cb0, cout // 8).double().numpy()
    err = np.abs(got - want)
    print(f'{who} {cin}->{cout} kt={kt} pad_t={pad_t} prologue={prologue} relu={relu} b={bsz} t={t} {h}x{w}: largest error / bound = '
          f'{float((err / bound).max()):.4f}')
    assert np.isfinite(got).all() and (err <= bound).all(), float((err / bound).max())
    # the rest of the destination keeps its bit pattern: the other channel blocks and the frames outside the window
    rest = buf.clone()
    rest[:, t0:t0 + tout, out_cb0:out_cb0 + cout // 8] = NAN
    assert torch.equal(_bits(rest.cpu()), _bits(torch.full_like(rest, NAN).cpu()))
    # negative control: twice the bound added to one element is caught
    bad = got.copy()
    at = np.unravel_index(np.argmax(mag), mag.shape)
    bad[at] = got[at] + 2 * bound[at]
    assert not (np.abs(bad - want) <= bound).all()
    if prologue and pad_s:
        # at the border the padded positions contribute zero, not max(shift, 0): padding BEFORE the prologue is outside the bound
        padded = np.broadcast_to(np.maximum(shift, 0).reshape(1, -1, 1, 1, 1), (bsz, cin, t + 2 * pad_t, h + 2, w + 2)).astype(np.float32)
        padded[:, :, pad_t:pad_t + t, 1:1 + h, 1:1 + w] = operand
        wrong = F.conv3d(torch.from_numpy(padded).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double()).numpy()
        assert not (np.abs((np.maximum(wrong, 0) if relu else wrong) - got) <= bound).all()
    assert torch.equal(_bits(launch(x)), _bits(buf))                                     # a rerun is bit-equal
    if bsz == 2:
        for i in range(2):                                                               # a batch of two equals two single runs
            assert torch.equal(_bits(launch(x[i:i + 1])[0]), _bits(buf[i]))
        loud = x.copy()
        loud[1] = 1e30                                                                   # nothing of clip 1 reaches clip 0
        assert torch.equal(_bits(launch(loud)[0]), _bits(buf[0]))


# ------------------------------------------------------------------------------------------------------------- conv3d
# (b, T, h, w): 5x7 inside one 8 x 32 tile; 8x33 one tile row, a one-column tail tile; 17x40 three tile rows with a one-row tail
CONV_SHAPES = ((2, 7, 5, 7), (2, 3, 8, 33), (1, 5, 17, 40))
CONV_PAIRS = ((64, 16), (80, 16), (224, 32), (432, 16), (448, 256), (3, 64))
# (kt, pad_t, prologue): the dense blocks, the temporal-reduce blocks, bn3d2 -> conv3d2, and the prologue under temporal padding
CONV_CONFIGS = ((3, 1, False), (3, 0, False), (1, 0, True), (3, 1, True))
_conv_inputs = {}


def _conv_input(cin, cout, kt, shape):
    key = (cin, cout, kt, shape)
    if key not in _conv_inputs:
        b, t, h, w = shape
        rng = np.random.default_rng(1000 * cin + 10 * cout + kt + h)
        x = rng.standard_normal((b, cin, t, h, w)).astype(np.float32)
        wt = (rng.standard_normal((cout, cin, kt, 3, 3)) / np.sqrt(9 * kt * cin)).astype(np.float32)
        bias = rng.standard_normal(cout).astype(np.float32)
        _conv_inputs[key] = (x, wt, bias)
    return _conv_inputs[key]


@pytest.mark.parametrize('config', CONV_CONFIGS, ids=[f'kt{k}_pad{p}{"_prologue" if g else ""}' for k, p, g in CONV_CONFIGS])
@pytest.mark.parametrize('shape', CONV_SHAPES, ids=['x'.join(str(v) for v in s) for s in CONV_SHAPES])
@pytest.mark.parametrize('pair', CONV_PAIRS, ids=[f'{ci}to{co}' for ci, co in CONV_PAIRS])
def test_conv3d_matches_float64(cuda, pair, shape, config):
    cin, cout = pair
    kt, pad_t, prologue = config
    x, wt, bias = _conv_input(cin, cout, kt, shape)
    pc = H.PackedDufConv(torch.from_numpy(wt).to(cuda), torch.from_numpy(bias).to(cuda))
    cinb, gc = (cin + 7) // 8, min(cout, 64)
    assert pc.w.numel() == _lib.load().sr_duf_conv3d_packed_floats(cout, cin, kt) == cinb * kt * 9 * cout * 8 + cout
    # the packed image: [cout group][cin block][frame tap][tap][couts of the group][8 channels], pad channels zero, then the bias
    wp = np.zeros((cout, cinb * 8, kt, 9), np.float32)
    wp[:, :cin] = wt.reshape(cout, cin, kt, 9)
    want_img = wp.reshape(cout // gc, gc, cinb, 8, kt, 9).transpose(0, 2, 4, 5, 1, 3).reshape(-1)
    img = pc.w.cpu().numpy()
    assert np.array_equal(img[:-cout], want_img) and np.array_equal(img[-cout:], bias)
    _check_conv(cuda, 'conv3d', H.duf_conv3d, pc, x, wt, bias, kt, pad_t, 1, prologue, relu=(kt == 1), out_cb0=2)


def test_conv3d_refuses_what_it_does_not_serve(cuda):
    lib = _lib.load()
    for cout, cin, kt in ((16, 12, 3), (48, 64, 3), (16, 456, 3), (16, 64, 2), (16, 4, 1)):
        assert lib.sr_duf_conv3d_packed_floats(cout, cin, kt) == 0
        with pytest.raises(ValueError, match='not supported'):
            H.PackedDufConv(torch.zeros(cout, cin, kt, 3, 3, device=cuda))
    pc = H.PackedDufConv(torch.zeros(16, 64, 3, 3, 3, device=cuda))
    src = H.ClipCB8.empty(1, 3, 64, 4, 4, cuda)
    with pytest.raises(ValueError, match='too few channel blocks'):
        H.duf_conv3d(H.ClipCB8.empty(1, 3, 32, 4, 4, cuda), pc, H.ClipCB8.empty(1, 3, 16, 4, 4, cuda), pad_t=1)
    with pytest.raises(ValueError, match='does not fit'):
        H.duf_conv3d(src, pc, H.ClipCB8.empty(1, 3, 16, 4, 4, cuda), pad_t=0)         # kt = 3 without padding leaves one frame
    with pytest.raises(ValueError, match='does not fit'):
        H.duf_conv3d(src, pc, H.ClipCB8.empty(1, 3, 16, 4, 4, cuda), 1, pad_t=1)      # the slice ends beyond the destination
    with pytest.raises(ValueError, match='1x1x1'):
        H.duf_pw(src, pc, H.ClipCB8.empty(1, 3, 64, 4, 4, cuda))
    with pytest.raises(ValueError, match='prologue'):
        H.duf_conv3d(src, pc, H.ClipCB8.empty(1, 3, 16, 4, 4, cuda), pad_t=1, prologue=(torch.ones(8, device=cuda), torch.ones(8, device=cuda)))


# ----------------------------------------------------------------------------------------------------------------- pw
PW_SHAPES = ((1, 7, 5, 7), (2, 1, 9, 33))


@pytest.mark.parametrize('prologue', [False, True], ids=['plain', 'prologue'])
@pytest.mark.parametrize('shape', PW_SHAPES, ids=['x'.join(str(v) for v in s) for s in PW_SHAPES])
@pytest.mark.parametrize('c', [64, 432])
def test_pw_matches_float64(cuda, c, shape, prologue):
    b, t, h, w = shape
    rng = np.random.default_rng(c + h)
    x = rng.standard_normal((b, c, t, h, w)).astype(np.float32)
    wt = (rng.standard_normal((c, c, 1, 1, 1)) / np.sqrt(c)).astype(np.float32)
    bias = rng.standard_normal(c).astype(np.float32)
    pc = H.PackedDufConv(torch.from_numpy(wt).to(cuda), torch.from_numpy(bias).to(cuda))
    groups = (c + 63) // 64
    assert pc.w.numel() == _lib.load().sr_duf_pw_packed_floats(c) == groups * (c // 8) * 64 * 8 + groups * 64
    _check_conv(cuda, 'pw', H.duf_pw, pc, x, wt, bias, 1, 0, 0, prologue, relu=prologue, out_cb0=1)


# ------------------------------------------------------------------------------------------------------------- filter
def _reference_tail(logits, res, centre, s, softmax, shuffle):
    """The reference's op sequence (duf_arch.py:177-185, 276-281) in the dtype of its inputs, with torch on the CPU."""
    n, _, h, w = centre.shape
    s2 = s * s
    f = logits.view(n, 25, s2, h, w)
    if softmax:
        f = F.softmax(f, dim=1)
    expansion = torch.eye(25, dtype=centre.dtype).view(25, 1, 5, 5).repeat(3, 1, 1, 1)
    expanded = F.conv2d(centre, expansion, padding=2, groups=3).view(n, 3, 25, h, w).permute(0, 3, 4, 1, 2)
    out = torch.matmul(expanded, f.permute(0, 3, 4, 1, 2)).permute(0, 3, 4, 1, 2).reshape(n, 3 * s2, h, w)
    if res is not None:
        out = out + res
    return F.pixel_shuffle(out, s) if shuffle else out


FILTER_MAPS = ((1, 1), (3, 5), (9, 33))


@pytest.mark.parametrize('kind', ['pm80', 'uniform', 'shifted'])
@pytest.mark.parametrize('hw', FILTER_MAPS, ids=[f'{h}x{w}' for h, w in FILTER_MAPS])
@pytest.mark.parametrize('s', [2, 3, 4])
def test_filter_matches_float64(cuda, s, hw, kind):
    h, w = hw
    n, s2 = 2, s * s
    rng = np.random.default_rng(100 * s + h)
    if kind == 'uniform':                                   # every weight 1 / 25: the zero-padded window at the border
        logits = np.full((n, 25 * s2, h, w), 3.0, np.float32)
    else:                                                   # +-80: exp overflows without the maximum subtracted once shifted up
        logits = rng.uniform(-80, 80, (n, 25 * s2, h, w)).astype(np.float32) + np.float32(60.0 if kind == 'shifted' else 0.0)
    res = rng.standard_normal((n, 3 * s2, h, w)).astype(np.float32)
    centre = rng.uniform(0, 1, (n, 7, 3, h, w)).astype(np.float32)        # read in place from a clip: frame 3
    clip = torch.from_numpy(centre).to(cuda)
    lt, rt, ct = torch.from_numpy(logits), torch.from_numpy(res), torch.from_numpy(centre[:, 3])
    lcb, rcb = H.nchw_to_cb8(lt.to(cuda)), H.nchw_to_cb8(rt.to(cuda))
    # the flag combinations in use: the network (softmax, res, shuffle) and the module alone (normalised filters, neither)
    for softmax, with_res, shuffle in ((True, True, True), (False, False, False), (True, False, True), (True, True, False)):
        lin = lt if softmax else F.softmax(lt.view(n, 25, s2, h, w), 1).reshape(n, 25 * s2, h, w)
        want = _reference_tail(lin.double(), rt.double() if with_res else None, ct.double(), s, softmax, shuffle)
        ref32 = _reference_tail(lin, rt if with_res else None, ct, s, softmax, shuffle)
        dist = float((ref32.double() - want).abs().max())
        lin_cb = lcb if softmax else H.nchw_to_cb8(lin.to(cuda))
        got = H.duf_filter(lin_cb, clip[:, 3], s, rcb if with_res else None, softmax=softmax, shuffle=shuffle)
        assert got.shape == want.shape and got.dtype == torch.float32
        err = float((got.cpu().double() - want).abs().max())
        print(f'filter s={s} {h}x{w} {kind} softmax={softmax} res={with_res} shuffle={shuffle}: error {err:.3e} = {err / max(dist, TINY):.2f} x the fp32 '
              f'CPU distance {dist:.3e}')
        assert bool(torch.isfinite(got).all()) and err <= MARGIN * dist, (err, dist)
        again = H.duf_filter(lin_cb, clip[:, 3], s, rcb if with_res else None, softmax=softmax, shuffle=shuffle)
        assert torch.equal(_bits(again), _bits(got))
        for i in range(n):                                   # a batch of two equals two single runs
            li = H.nchw_to_cb8(lin[i:i + 1].to(cuda))
            ri = H.nchw_to_cb8(rt[i:i + 1].to(cuda)) if with_res else None
            one = H.duf_filter(li, clip[i:i + 1, 3], s, ri, softmax=softmax, shuffle=shuffle)
            assert torch.equal(_bits(one[0]), _bits(got[i]))
    if kind == 'uniform':
        # the window itself: with equal weights an output pixel is the zero-padded 5x5 box mean of the centre frame
        box = F.avg_pool2d(ct.double(), 5, 1, 2, count_include_pad=True)
        got = H.duf_filter(lcb, clip[:, 3], s, None, softmax=True, shuffle=True)
        assert float(np.abs(got.cpu().double().numpy() - D.nearest_up(box.numpy(), s)).max()) <= 30 * EPS


def test_filter_refusals(cuda):
    lg = H.CB8.zeros(1, 400, 4, 4, cuda)
    x = torch.zeros(1, 3, 4, 4, device=cuda)
    with pytest.raises(ValueError, match='scale'):
        H.duf_filter(lg, x, 5)
    with pytest.raises(ValueError, match='channels'):
        H.duf_filter(H.CB8.zeros(1, 100, 4, 4, cuda), x, 4)
    with pytest.raises(ValueError, match='centre'):
        H.duf_filter(lg, x[:, :2], 4)
    with pytest.raises(ValueError, match='res does not fit'):
        H.duf_filter(lg, x, 4, H.CB8.zeros(1, 16, 4, 4, cuda))
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        H.duf_filter(lg, x.cpu(), 4)
