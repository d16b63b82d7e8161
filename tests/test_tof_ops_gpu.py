"""The entry points of include/sr_hip_tof.h on the GPU.  EPS = 2^-24.

  conv9x9      against float64 (tests/tof_restate.py) with the bound the header derives from its summation order: K = 81 * cin_pad
               fused multiply-adds from a zero accumulator, + bias, ReLU:  |got - exact| <= (K + 2) * EPS * (sum |w x| + |bias|).
  level input  up_out bit-equal to the level input of the flow header, the warped channels bit-equal to its zeros-padding warp of
               supp by up, the ref and flow channels exact.
  stack        bit-equal to the per-frame zeros-padding warp; finish bit-identical to torch fp32 on the CPU.
The largest error / bound of each convolution case is printed (run with -s)."""
import os
import sys

import numpy as np
import pytest
import torch

from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tof_restate as T  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
TINY = 1e-30
NAN = float('nan')


def _to_cb8(x, cuda, before=0, after=0, fill=NAN):
    """[N, C, H, W] numpy -> CB8 window of a buffer with ``before`` / ``after`` slack blocks and pad channels, all ``fill``."""
    n, c, h, w = x.shape
    cb = (c + 7) // 8
    buf = torch.full((n, before + cb + after, h, w, 8), fill, dtype=torch.float32)
    xp = torch.full((n, cb * 8, h, w), fill, dtype=torch.float32)
    xp[:, :c] = torch.from_numpy(np.asarray(x, np.float32))
    buf[:, before:before + cb] = xp.reshape(n, cb, 8, h, w).permute(0, 1, 3, 4, 2)
    return H.CB8(buf.to(cuda), before, cb)


def _from_cb8(t):
    b = t.buf[:, t.cb0:t.cb0 + t.cbn].cpu()
    n, cb, h, w, _ = b.shape
    return b.permute(0, 1, 4, 2, 3).reshape(n, cb * 8, h, w)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ conv9x9
# 1x1: below the halo; 5x7: inside one 8 x 32 tile; 33x40: five tile rows with a one-row tail, two tile columns with an 8-column tail
CONV_MAPS = ((1, 1), (5, 7), (33, 40))
_conv_cache = {}


def _conv_case(cin, h, w):
    key = (cin, h, w)
    if key not in _conv_cache:
        rng = np.random.default_rng(100 * cin + h)
        x = rng.standard_normal((3, cin, h, w)).astype(np.float32)
        wt = (rng.standard_normal((64, cin, 9, 9)) / np.sqrt(81 * cin)).astype(np.float32)
        b = rng.standard_normal(64).astype(np.float32)
        pre, mag = T.conv(x, wt, b, want_mag=True)            # computed once, shared, never modified
        _conv_cache[key] = (x, wt, b, pre, mag)
    return _conv_cache[key]


@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('hw', CONV_MAPS, ids=[f'{h}x{w}' for h, w in CONV_MAPS])
@pytest.mark.parametrize('pair', H.CONV9X9_SHAPES, ids=[f'{ci}to{co}' for ci, co in H.CONV9X9_SHAPES])
def test_conv9x9_matches_float64(cuda, pair, hw, n, relu):
    cin, cout = pair
    h, w = hw
    x, wt, b, pre, mag = _conv_case(cin, h, w)
    x, pre, mag = x[:n], pre[:n], mag[:n]
    pc = H.PackedConv9x9(torch.from_numpy(wt).to(cuda), torch.from_numpy(b).to(cuda))
    cinb = (cin + 7) // 8
    assert pc.w.numel() == _lib.load().sr_tof_conv9x9_packed_floats(cout, cin) == cinb * 81 * 512 + 64
    # the packed image: [cin block][tap][64 couts][8 channels], pad channels zero, then the bias
    wp = np.zeros((64, cinb * 8, 81), np.float32)
    wp[:, :cin] = wt.reshape(64, cin, 81)
    want_img = wp.reshape(64, cinb, 8, 81).transpose(1, 3, 0, 2).reshape(-1)
    img = pc.w.cpu().numpy()
    assert np.array_equal(img[:-64], want_img) and np.array_equal(img[-64:], b)
    src = _to_cb8(x, cuda, before=1, after=1)                # NaN slack blocks and NaN pad channels 21-23: non-dense image strides
    out = H.CB8(torch.full((n, 8 + 3, h, w, 8), NAN, dtype=torch.float32, device=cuda), 2, 8)
    H.conv9x9(src, pc, out=out, relu=relu)
    got = _from_cb8(out).double().numpy()
    want = np.maximum(pre, 0) if relu else pre
    bound = (81 * cinb * 8 + 2) * EPS * mag + TINY
    err = np.abs(got - want)
    print(f'conv9x9 {cin}->{cout} {h}x{w} n={n} relu={relu}: largest error / bound = {float((err / bound).max()):.4f}')
    assert np.isfinite(got).all() and (err <= bound).all(), (pair, hw, float((err / bound).max()))
    # the slack stays NaN bit for bit
    slack = torch.cat([out.buf[:, :2].flatten(), out.buf[:, 10:].flatten()])
    assert torch.equal(_bits(slack.cpu()), _bits(torch.full_like(slack, NAN).cpu()))
    # negative control: twice the bound added to one element is caught
    bad = got.copy()
    at = np.unravel_index(np.argmax(mag), mag.shape)
    bad[at] = got[at] + 2 * bound[at]
    assert not (np.abs(bad - want) <= bound).all()
    # an image of the batch equals the image alone, bit for bit; so does a rerun
    if n == 3:
        one = H.conv9x9(_to_cb8(x[1:2], cuda), pc, relu=relu)
        assert torch.equal(_bits(one.buf[0]), _bits(out.buf[1, 2:10]))
        again = H.CB8(torch.full_like(out.buf, NAN), 2, 8)
        H.conv9x9(src, pc, out=again, relu=relu)
        assert torch.equal(_bits(again.buf[:, 2:10]), _bits(out.buf[:, 2:10]))


def test_conv9x9_refuses_what_it_does_not_serve(cuda):
    for cout, cin in ((64, 24), (32, 64), (64, 32), (3, 64)):
        with pytest.raises(ValueError, match='not supported'):
            H.PackedConv9x9(torch.zeros(cout, cin, 9, 9, device=cuda))
    pc = H.PackedConv9x9(torch.zeros(64, 21, 9, 9, device=cuda))
    with pytest.raises(ValueError, match='channel blocks'):
        H.conv9x9(H.CB8.zeros(1, 64, 4, 4, cuda), pc)
    with pytest.raises(ValueError, match='does not fit'):
        H.conv9x9(H.CB8.zeros(1, 24, 4, 4, cuda), pc, out=H.CB8.zeros(1, 64, 4, 5, cuda))


# -------------------------------------------------------------------------------------------------------- level input
LEVEL_MAPS = ((2, 2), (6, 10), (34, 40))       # from 1x1, 3x5 and 17x20


def _flow_block(flow, cuda):
    """[N, 2, h, w] numpy -> the one-block CB8 buffer the last conv of a level writes."""
    return H.CB8(_to_cb8(flow, cuda, fill=0.0).buf)


@pytest.mark.parametrize('kind', ['null', 'inside', 'outside_nan'])
@pytest.mark.parametrize('hw', LEVEL_MAPS, ids=[f'{h}x{w}' for h, w in LEVEL_MAPS])
def test_level_input_matches_the_flow_header_bit_for_bit(cuda, hw, kind):
    h, w = hw
    n = 3
    rng = np.random.default_rng(h * 7 + len(kind))
    ref = torch.from_numpy(rng.standard_normal((n, 3, h, w)).astype(np.float32)).to(cuda)
    supp = torch.from_numpy(rng.standard_normal((n, 3, h, w)).astype(np.float32)).to(cuda)
    prev = None
    if kind != 'null':
        scale = 0.4 if kind == 'inside' else 0.6 * max(h, w)       # doubled by the upsampling: the second samples outside
        fl = (rng.standard_normal((n, 2, h // 2, w // 2)) * scale).astype(np.float32)
        if kind == 'outside_nan':
            fl[1, 0, 0, 0] = NAN
        prev = _flow_block(fl, cuda)
    out, up = H.tof_level_input(ref, supp, prev)
    _, up_spy = H.spynet_level_input(ref, supp, prev)
    assert torch.equal(_bits(up.buf), _bits(up_spy.buf))                       # the same upsampling, bit for bit
    o = _from_cb8(out).to(cuda)
    upn = up.buf[:, 0, :, :, :2].contiguous()                                  # [N, H, W, 2]
    warped = H.flow_warp(supp, upn, 'zeros')
    assert torch.equal(_bits(o[:, 3:6]), _bits(warped))                        # the zeros-padding warp of supp by up
    assert torch.equal(_bits(o[:, :3]), _bits(ref))
    assert torch.equal(_bits(o[:, 6:8]), _bits(upn.permute(0, 3, 1, 2)))
    if kind == 'null':
        assert not up.buf.any() and torch.equal(o[:, 3:6], supp)
    else:
        # and against float64: the upsampling is rounded once, the warp follows the rounded position
        want, _ = T.level_input(ref.cpu().numpy(), supp.cpu().numpy(), fl.astype(np.float64))
        fin = np.isfinite(want[:, 6:8]).all(1)
        assert (np.abs(up.buf[:, 0, :, :, :2].cpu().double().numpy().transpose(0, 3, 1, 2) - want[:, 6:8])[np.isfinite(want[:, 6:8])]
                <= EPS * np.abs(want[:, 6:8])[np.isfinite(want[:, 6:8])] + TINY).all()
        exact = T.R.flow_warp(supp.cpu().numpy(), upn.cpu().numpy().astype(np.float32), 'zeros', np.float32)
        sel = np.broadcast_to(fin[:, None], exact.shape)
        assert (np.abs(o[:, 3:6].cpu().double().numpy() - exact)[sel] <= EPS * float(supp.abs().max()) + TINY).all()
        if kind == 'outside_nan':
            assert np.isnan(want[:, 6:8]).any() and (o[:, 3:6].cpu().numpy()[~sel] == 0).all()      # a NaN position samples nothing
            assert (o[:, 3:6] == 0).float().mean() > 0.2                                            # many samples fall outside


def test_level_input_reads_the_pairs_of_a_clip_in_place(cuda):
    rng = np.random.default_rng(5)
    b, h, w = 2, 6, 10
    clip = torch.from_numpy(rng.standard_normal((b, 7, 3, h, w)).astype(np.float32)).to(cuda)
    prev = _flow_block((rng.standard_normal((6 * b, 2, h // 2, w // 2)) * 2).astype(np.float32), cuda)
    for r in (0, 3, 6):
        others = [i for i in range(7) if i != r]
        ref = clip[:, r:r + 1].expand(b, 6, 3, h, w).reshape(6 * b, 3, h, w).contiguous()
        supp = clip[:, others].reshape(6 * b, 3, h, w).contiguous()
        want, want_up = H.tof_level_input(ref, supp, prev)
        got, got_up = H.tof_level_input(None, None, prev, clip=clip, ref_idx=r)
        assert torch.equal(_bits(got.buf), _bits(want.buf)) and torch.equal(_bits(got_up.buf), _bits(want_up.buf)), r


# ------------------------------------------------------------------------------------------------------ aligned stack
@pytest.mark.parametrize('ref_idx', [0, 3])
@pytest.mark.parametrize('b', [1, 2])
def test_aligned_stack_is_the_per_frame_zeros_warp(cuda, b, ref_idx):
    rng = np.random.default_rng(10 * b + ref_idx)
    h, w = 9, 13
    clip = torch.from_numpy(rng.standard_normal((b, 7, 3, h, w)).astype(np.float32)).to(cuda)
    fl = (rng.standard_normal((6 * b, 2, h, w)) * 3).astype(np.float32)
    fl[0, :, 0, 0] = NAN
    flows = H.CB8(_to_cb8(fl, cuda, fill=NAN).buf)            # channels 2-7 of the flow blocks hold NaN: only 0, 1 are read
    out = H.CB8(torch.full((b, 5, h, w, 8), NAN, dtype=torch.float32, device=cuda), 1, 3)
    H.tof_align(clip, flows, ref_idx, out=out)
    got = _from_cb8(out).to(cuda)
    fln = torch.from_numpy(fl).to(cuda).view(b, 6, 2, h, w).permute(0, 1, 3, 4, 2).contiguous()
    k = 0
    for i in range(7):
        if i == ref_idx:
            want = clip[:, i]
        else:
            want = H.flow_warp(clip[:, i].contiguous(), fln[:, k].contiguous(), 'zeros')
            k += 1
        assert torch.equal(_bits(got[:, 3 * i:3 * i + 3]), _bits(want)), i
    assert not got[:, 21:].any()                                               # channels 21-23 are zero
    assert torch.isnan(out.buf[:, 0]).all() and torch.isnan(out.buf[:, 4]).all()
    if b == 2:
        one = H.tof_align(clip[1:2].contiguous(), H.CB8(flows.buf[6:].contiguous()), ref_idx)
        assert torch.equal(_bits(one.buf[0]), _bits(out.buf[1, 1:4]))
    want64 = T.aligned_stack(clip.cpu().numpy(), fl.reshape(b, 6, 2, h, w), ref_idx, np.float32)
    ok = np.isfinite(want64)
    assert (np.abs(got[:, :21].cpu().double().numpy() - want64)[ok] <= EPS * float(clip.abs().max()) + TINY).all()


# -------------------------------------------------------------------------------------------------------------- finish
@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 5, 7), (3, 17, 33)], ids=['1x1', 'b2_5x7', 'b3_17x33'])
def test_finish_is_bit_identical_to_torch(cuda, shape):
    b, h, w = shape
    rng = np.random.default_rng(b + h)
    clip = torch.from_numpy(rng.standard_normal((b, 7, 3, h, w)).astype(np.float32))
    y = rng.standard_normal((b, 3, h, w)).astype(np.float32)
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    for r in (0, 3):
        want = (torch.from_numpy(y) + clip[:, r]) * std + mean                  # tof_arch.py:170-172, fp32 on the CPU
        got = H.tof_finish(_to_cb8(y, cuda, before=1, after=1), clip.to(cuda), r, mean.flatten().tolist(), std.flatten().tolist())
        assert torch.equal(_bits(got.cpu()), _bits(want)), (shape, r)
