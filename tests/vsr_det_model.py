"""A numpy model of the integer arithmetic of sr_vsr_prop_input_bwd_det_f32 (include/sr_hip_vsr_det.h), the data of its GPU test
and the header's bound — shared by tests/test_vsr_det_host.py (the model against the float64 definition) and
tests/test_vsr_det_ops_gpu.py (the device against the model, bit for bit).

The model follows the header step by step: M as the unsigned maximum of the sign-cleared bit patterns of the image's g,
e = ilogb(M) + 1, L = ceil(log2(4 h w)), k = 61 - e - L, every term (double)g * wq rounded to an integer by rint(ldexp(term, k)),
an int64 sum per element, and dprev = float32(float64(before) + ldexp(float64(acc), -k)).  The coordinates are evaluated in fp32 as
the device does (tests/flow_restate.warp_coords on an fp32 flow), the weights wq in float64 from the fp32 fractions."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixed_sum_model as FS  # noqa: E402
import flow_restate as FR  # noqa: E402
from fixed_sum_model import INF_BITS, U  # noqa: E402,F401

scale_bits = FS.max_bits    # of |g| over one image


def shift_of(mbits, h, w):
    """(k, e, L) for a finite non-zero M given by its bits."""
    e, L = FS.exp_of(mbits), FS.level_of(4 * h * w)
    return 61 - e - L, e, L


def valid_pixels(flow, h, w):
    """(valid [n, h, w], the flow with invalid pixels set to 0, as [n, h, w, 2] fp32): the device's own test of the position."""
    fl = np.ascontiguousarray(np.asarray(flow, np.float32).transpose(0, 2, 3, 1))
    with np.errstate(invalid='ignore'):
        ix = (np.arange(w, dtype=np.float32)[None, None, :] + fl[..., 0]).astype(np.float32) if w > 1 else np.zeros(fl.shape[:3], np.float32)
        iy = (np.arange(h, dtype=np.float32)[None, :, None] + fl[..., 1]).astype(np.float32) if h > 1 else np.zeros(fl.shape[:3], np.float32)
        valid = (ix > -1) & (ix < w) & (iy > -1) & (iy < h)
    return valid, np.where(valid[..., None], fl, np.float32(0))


def det_dprev(before, g, flow):
    """The model.  before, g: fp32 [n, c, h, w]; flow: fp32 [n, 2, h, w].  Returns (dprev fp32 [n, c, h, w], info) with info a list
    per image of dict(bits, k, e, L, acc int64 [c, h, w], absacc: the sum of |integer terms| per element as Python-exact float64
    upper bound, count)."""
    before, g = np.asarray(before, np.float32), np.asarray(g, np.float32)
    n, c, h, w = g.shape
    valid, safe = valid_pixels(flow, h, w)
    x0, y0, fx, fy, _, _ = FR.warp_coords(safe, h, w, 'zeros')
    wts = [(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx]
    offs = [(0, 0), (0, 1), (1, 0), (1, 1)]
    out, info = before.copy(), []
    for i in range(n):
        bits = scale_bits(g[i])
        rec = dict(bits=bits, k=None, acc=None, absacc=None, count=None)
        info.append(rec)
        if bits == 0:
            continue
        if bits >= INF_BITS:
            out[i] = np.float32(np.nan)
            continue
        k, e, L = shift_of(bits, h, w)
        acc, absacc, count = np.zeros((c, h, w), np.int64), np.zeros((c, h, w), np.float64), np.zeros((c, h, w), np.int64)
        gd = g[i].astype(np.float64)
        for (oy, ox), wt in zip(offs, wts):
            yy, xx = y0[i] + oy, x0[i] + ox
            sel = valid[i] & (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w) & (wt[i] != 0)
            ys, xs = yy[sel], xx[sel]
            for ch in range(c):
                term = (gd[ch] * wt[i])[sel]
                scaled = FS.quantise(term, k)
                assert np.abs(scaled).max(initial=0.0) <= 2.0 ** (61 - L)
                np.add.at(acc[ch], (ys, xs), scaled.astype(np.int64))
                np.add.at(absacc[ch], (ys, xs), np.abs(scaled))
                np.add.at(count[ch], (ys, xs), 1)
        rec.update(k=k, e=e, L=L, acc=acc, absacc=absacc, count=count)
        out[i] = (before[i].astype(np.float64) + FS.scaled_back(acc, k)).astype(np.float32)
    return out, info


def det_bound(before, exact, count, absterms, ks):
    """The header's bound per element: 2^-24 |before + exact| + d 2^-(k + 1) + 2^-50 sum |terms|; ``ks``: k per image (None for an
    image that is skipped: the bound is then 0 only where nothing is added)."""
    return FS.bound(before + exact, count, absterms, ks)


def case_data(h, w, fb, n):
    """(rng, prev, g, before) of the GPU test's case: float64 arrays holding fp32 values, [n, 8 fb, h, w]."""
    rng = np.random.default_rng(1000 * h + 10 * fb + n + 7)
    shape = (n, 8 * fb, h, w)
    prev, g, before = (rng.standard_normal(shape).astype(np.float32).astype(np.float64) for _ in range(3))
    return rng, prev, g, before


def g_variants(g, n):
    """{name: g} of the extra gradient cases: an image scaled by 2^100, one by 2^-100, one all zero, one with a NaN."""
    out = {'plain': g}
    if n >= 3:
        mixed = g.copy()
        mixed[0] *= 2.0 ** 100
        mixed[1] *= 2.0 ** -100
        mixed[2] = 0.0
        out['mixed'] = mixed
    else:
        out['big'], out['small'], out['zero'] = g * 2.0 ** 100, g * 2.0 ** -100, np.zeros_like(g)
    nan = g.copy()
    nan[n - 1].reshape(-1)[nan[n - 1].size // 2] = np.nan
    out['nan'] = nan
    return out
