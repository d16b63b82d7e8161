"""A numpy model of the integer arithmetic of sr_dcn_bwd_data_det_f32 (include/sr_hip_dcn_det.h), the data of its GPU test and the
header's bound — shared by tests/test_dcn_det_host.py (the model against the float64 definition of tests/dcn_restate.py) and
tests/test_dcn_det_ops_gpu.py (the device against the model, bit for bit).

The model follows the header step by step.  The sampling position is evaluated in fp32 as the device does ((float)(y - 1 + i) +
offset, the `inside` test, floor, the fractions lh = h_im - floor(h_im)); the four weights in float64 from the fp32 fractions
((1 - lh) and (1 - lw) in float64); a term is ((double)dcol * (double)m) * wq; Md and Mm are unsigned maxima of sign-cleared bit
patterns; e = ilogb(Md) + 1 (+ ilogb(Mm) + 1 for a raw mask), L = ceil(log2(9 h w)), k = 61 - e - L; every term becomes
rint(ldexp(term, k)), is summed in int64 per element, and dx = float32(ldexp(float64(acc), -k)).

The mask VALUE m is an input of the model (fp32): for a logit mask it is the device's own fp32 sigmoid, which numpy cannot restate
bit for bit, so the GPU test reads it back from the forward's column kernel; the logits themselves only say whether one is NaN."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixed_sum_model as FS  # noqa: E402
from fixed_sum_model import INF_BITS, U, exp_of, max_bits  # noqa: E402,F401


def level_of(h, w):
    """L = ceil(log2(9 h w))."""
    return FS.level_of(9 * h * w)


def scale_state(md, mm, logit, h, w):
    """('zero' | 'nan' | 'sum', k, e, L) from the two scale words of an image."""
    L = level_of(h, w)
    if md >= INF_BITS or mm >= INF_BITS:
        return 'nan', None, None, L
    if md == 0 or (not logit and mm == 0):
        return 'zero', None, None, L
    e = exp_of(md) + (0 if logit else exp_of(mm))
    return 'sum', 61 - e - L, e, L


def cells(offset, dg):
    """The device's fp32 sampling cells.  offset: fp32 [n, 18 dg, h, w].  Returns dict of [n, dg, 9, h, w] arrays: h_im, w_im (fp32,
    as computed), inside, hl, wl (int64), lh, lw (fp32)."""
    offset = np.asarray(offset, np.float32)
    n, _, h, w = offset.shape
    off = offset.reshape(n, dg, 9, 2, h, w)
    ti = (np.arange(9) // 3).reshape(1, 1, 9, 1, 1)
    tj = (np.arange(9) % 3).reshape(1, 1, 9, 1, 1)
    ys = np.arange(h).reshape(1, 1, 1, h, 1)
    xs = np.arange(w).reshape(1, 1, 1, 1, w)
    with np.errstate(invalid='ignore', over='ignore'):
        h_im = ((ys - 1 + ti).astype(np.float32) + off[:, :, :, 0]).astype(np.float32)
        w_im = ((xs - 1 + tj).astype(np.float32) + off[:, :, :, 1]).astype(np.float32)
        h_im, w_im = np.broadcast_arrays(h_im, w_im)
        inside = (h_im > np.float32(-1)) & (w_im > np.float32(-1)) & (h_im < np.float32(h)) & (w_im < np.float32(w))
    hs, ws = np.where(inside, h_im, np.float32(0)), np.where(inside, w_im, np.float32(0))
    fh, fw = np.floor(hs), np.floor(ws)
    return dict(h_im=h_im, w_im=w_im, inside=inside, hl=fh.astype(np.int64), wl=fw.astype(np.int64),
                lh=(hs - fh).astype(np.float32), lw=(ws - fw).astype(np.float32))


def exact_offsets(offset, dg):
    """float64 offsets [n, 18 dg, h, w] with which a float64 evaluation of y - 1 + i + offset gives exactly the device's cell plus
    its fp32 fraction, hl + lh, so that the float64 definition forms the header's terms.  That is the device's fp32 position
    itself, except in the border cells (-1, 0), where lh = h_im + 1 is rounded to fp32 (the forward's own fraction): there it is
    the position whose exact fraction is that lh.  A position outside the `inside` test (a non-finite one too) is kept."""
    c = cells(offset, dg)
    n, _, h, w = np.asarray(offset).shape
    for pos, low, frac in (('h_im', 'hl', 'lh'), ('w_im', 'wl', 'lw')):
        snapped = c[low].astype(np.float64) + c[frac].astype(np.float64)
        moved = c['inside'] & (snapped != c[pos].astype(np.float64))
        assert not (moved & (c[low] != -1)).any()                       # the fraction is exact in every other cell
        c[pos] = np.where(c['inside'], snapped, c[pos].astype(np.float64))
    ti = (np.arange(9) // 3).reshape(1, 1, 9, 1, 1).astype(np.float64)
    tj = (np.arange(9) % 3).reshape(1, 1, 9, 1, 1).astype(np.float64)
    ys = np.arange(h, dtype=np.float64).reshape(1, 1, 1, h, 1)
    xs = np.arange(w, dtype=np.float64).reshape(1, 1, 1, 1, w)
    with np.errstate(invalid='ignore'):
        oh = c['h_im'].astype(np.float64) - (ys - 1 + ti)
        ow = c['w_im'].astype(np.float64) - (xs - 1 + tj)
    assert np.array_equal((ys - 1 + ti) + oh, c['h_im'].astype(np.float64), equal_nan=True)
    assert np.array_equal((xs - 1 + tj) + ow, c['w_im'].astype(np.float64), equal_nan=True)
    return np.stack([oh, ow], axis=3).reshape(n, 18 * dg, h, w)


def det_dx(dcol, offset, m, dg, logit, logits=None):
    """The model.  dcol: fp32 [n, 9, cin, h, w] (tap-major, as the CB8 column gradient); offset: fp32 [n, 18 dg, h, w]; m: the fp32
    mask VALUES [n, 9 dg, h, w]; ``logits``: with ``logit``, the fp32 logits (only their NaNs matter).  Returns (dx fp32
    [n, cin, h, w], info) with info a list per image of dict(state, md, mm, k, e, L, acc int64 [cin, h, w], count int64, maxabs:
    the largest |integer term|)."""
    dcol, m = np.asarray(dcol, np.float32), np.asarray(m, np.float32)
    n, _, cin, h, w = dcol.shape
    cpg = cin // dg
    c = cells(offset, dg)
    lh, lw = c['lh'].astype(np.float64), c['lw'].astype(np.float64)
    hh, hw = 1.0 - lh, 1.0 - lw
    corners = (((0, 0), hh * hw), ((0, 1), hh * lw), ((1, 0), lh * hw), ((1, 1), lh * lw))
    out, info = np.zeros((n, cin, h, w), np.float32), []
    for i in range(n):
        md = max_bits(dcol[i])
        if logit:
            nan_bits = np.ascontiguousarray(logits[i], np.float32).view(np.uint32) & np.uint32(0x7fffffff)
            mm = int(nan_bits[nan_bits > INF_BITS].max(initial=0))
        else:
            mm = max_bits(m[i])
        state, k, e, L = scale_state(md, mm, logit, h, w)
        rec = dict(state=state, md=md, mm=mm, k=k, e=e, L=L, acc=None, count=None, maxabs=0.0)
        info.append(rec)
        if state == 'nan':
            out[i] = np.float32(np.nan)
        if state != 'sum':
            continue
        acc, count = np.zeros((cin, h, w), np.int64), np.zeros((cin, h, w), np.int64)
        maxabs = 0.0
        for g in range(dg):
            av, cv = acc[g * cpg:(g + 1) * cpg], count[g * cpg:(g + 1) * cpg]
            for tap in range(9):
                dm = dcol[i, tap, g * cpg:(g + 1) * cpg].astype(np.float64) * m[i, 9 * g + tap].astype(np.float64)[None]   # exact
                for (oy, ox), wq in corners:
                    yy, xx, wt = c['hl'][i, g, tap] + oy, c['wl'][i, g, tap] + ox, wq[i, g, tap]
                    sel = c['inside'][i, g, tap] & (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1) & (wt != 0)
                    if not sel.any():
                        continue
                    scaled = FS.quantise(dm[:, sel] * wt[sel][None], k)
                    maxabs = max(maxabs, float(np.abs(scaled).max()))
                    np.add.at(av, (slice(None), yy[sel], xx[sel]), scaled.astype(np.int64))
                    np.add.at(cv, (slice(None), yy[sel], xx[sel]), 1)
        assert maxabs <= 2.0 ** (61 - L)
        rec.update(acc=acc, count=count, maxabs=maxabs)
        with np.errstate(over='ignore'):
            out[i] = FS.scaled_back(acc, k).astype(np.float32)
    return out, info


def det_bound(exact, count, absterms, ks):
    """The header's bound per element: 2^-24 |exact| + d 2^-(k + 1) + 2^-50 sum |terms|; ``ks``: k per image (None for an image
    whose dx is zero or NaN)."""
    return FS.bound(exact, count, absterms, ks)


# ------------------------------------------------------------------------------------------------------------ the cases
SIZES = ((1, 1), (5, 7), (33, 40))
CHANNELS = ((8, 1), (16, 1), (64, 8), (24, 3))        # (cin, deformable groups): one and two blocks a group, the last block of
BATCHES = (1, 3)                                      # the mask whole (72 channels), partly pad (9, 27)
KINDS = ('zero', 'dyadic', 'arbitrary', 'onecell', 'outside')


def offsets_of(kind, rng, n, dg, h, w):
    """fp32 offsets [n, 18 dg, h, w] of one kind."""
    shape = (n, dg, 9, 2, h, w)
    if kind == 'zero':
        off = np.zeros(shape)
    elif kind == 'dyadic':      # an integer in [-3, 3] plus a multiple of 1/16 in [2/16, 14/16]
        off = rng.integers(-3, 4, shape) + rng.integers(2, 15, shape) / 16.0
    elif kind == 'arbitrary':
        off = rng.standard_normal(shape) * 2.0
    elif kind == 'onecell':     # every pixel and tap samples the cell of (h // 2, w // 2) at fractions (1/4, 5/8): d = 9 h w there
        ti = (np.arange(9) // 3).reshape(1, 1, 9, 1, 1)
        tj = (np.arange(9) % 3).reshape(1, 1, 9, 1, 1)
        ys, xs = np.arange(h).reshape(1, 1, 1, h, 1), np.arange(w).reshape(1, 1, 1, 1, w)
        off = np.zeros(shape)
        off[:, :, :, 0] = (h // 2 + 0.25) - (ys - 1 + ti)
        off[:, :, :, 1] = (w // 2 + 0.625) - (xs - 1 + tj)
    elif kind == 'outside':     # far outside, in the half-open border cells (-1, 0) and (H - 1, H), and a NaN and an Inf position
        off = rng.uniform(-1.5, 1.5, shape) * np.array([h + 2, w + 2]).reshape(1, 1, 1, 2, 1, 1)
        flat = off.reshape(-1)
        flat[0], flat[flat.size // 2], flat[-1] = np.nan, np.inf, -1e30
    else:
        raise ValueError(kind)
    return off.reshape(n, 18 * dg, h, w).astype(np.float32)


def case_data(h, w, cin, dg, n, logit):
    """(rng, dcol fp32 [n, 9, cin, h, w], mask input fp32 [n, 9 dg, h, w]) of a case: the mask input is logits in [-4, 4], or raw
    values in [-3, 3] (outside [0, 1] and negative: the scale covers them)."""
    rng = np.random.default_rng(100000 * h + 1000 * w + 10 * cin + 2 * n + int(logit))
    dcol = rng.standard_normal((n, 9, cin, h, w)).astype(np.float32)
    mask_in = (rng.uniform(-4.0, 4.0, (n, 9 * dg, h, w)) if logit else rng.uniform(-3.0, 3.0, (n, 9 * dg, h, w))).astype(np.float32)
    return rng, dcol, mask_in


def dcol_variants(dcol):
    """{name: dcol} of the extra gradient cases: scaled by 2^100 and by 2^-100, all zero, holding one NaN; at n >= 3 the first
    three are three images of one batch."""
    n = dcol.shape[0]
    out = {}
    if n >= 3:
        mixed = dcol.copy()
        mixed[0] *= np.float32(2.0 ** 100)
        mixed[1] *= np.float32(2.0 ** -100)
        mixed[2] = 0.0
        out['mixed'] = mixed
    else:
        out['big'], out['small'], out['zero'] = dcol * np.float32(2.0 ** 100), dcol * np.float32(2.0 ** -100), np.zeros_like(dcol)
    nan = dcol.copy()
    nan[n - 1].reshape(-1)[nan[n - 1].size // 2] = np.nan
    out['nan'] = nan
    return out
