"""sr_adam_step_groups_f32 (csrc/adam_groups.hip) through the C ABI: bit identity with sr_adam_step_f32 when there is one class,
four classes (two learning rates, two step counts, one frozen segment between two live ones) against a float64 Adam per segment
within the bounds of tests/test_train_ops_gpu.py::test_adam_five_steps, the untouched chunks (inactive class, class id out of
range), the abort word and run-to-run bit identity.

Every slot the kernel must not read holds a NaN with its own payload: a read shows as NaN in a live slot or as a changed payload."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from image_restoration_amd import _lib

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
f32 = np.float32
LR, B1, B2, ADAM_EPS = 2e-4, 0.9, 0.99, 1e-8


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr() if t is not None else None


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _nan_pattern(n, tag):
    """n distinct quiet NaNs: payload = tag * 2^16 + index."""
    return (np.uint32(0x7FC00000) | (np.uint32(tag) << np.uint32(16)) | (np.arange(n, dtype=np.uint32) & np.uint32(0xFFFF))).view(f32)


def _classes(rows):
    arr = (_lib.AdamClass * len(rows))()
    for c, (lr, step, active) in enumerate(rows):
        arr[c].lr, arr[c].step, arr[c].active = lr, step, active
    return arr


def _groups(lib, pd, gd, md, vd, n, cls, rows, wd=0.0, gs=1.0, word=None, skipped=None):
    _lib.check(lib.sr_adam_step_groups_f32(_p(pd), _p(gd), _p(md), _p(vd), n, _p(cls), _classes(rows), len(rows), B1, B2, ADAM_EPS, wd,
                                           gs, _p(word), _p(skipped), _st()), 'sr_adam_step_groups_f32')


def _adam_ref(p, m, v, g, step, lr, b1, b2, eps, wd, gs, mabs):
    """The formula of tests/test_train_ops_gpu.py::_adam_ref, restated."""
    g = g * gs
    if wd:
        g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    mabs = b1 * mabs + (1 - b1) * np.abs(g)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    upd = lr / bc1 * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return p - upd, m, v, mabs, np.abs(upd)


# ------------------------------------------------------------------------------------------------------------ 1. one class
@pytest.mark.parametrize('step0', [1, 10000])
@pytest.mark.parametrize('wd,gs', [(0.0, 1.0), (0.01, 0.5)])
def test_one_class_has_the_bits_of_the_plain_step(cuda, lib, step0, wd, gs):
    n = 64 * 1563   # 25008 float4: 97.7 workgroups of 256 threads
    rng = np.random.default_rng(step0 + int(wd * 100))
    p = rng.standard_normal(n).astype(f32)
    if step0 == 1:
        m, v = np.zeros(n, f32), np.zeros(n, f32)
    else:   # state of a long run
        m, v = (rng.standard_normal(n) * 1e-2).astype(f32), (rng.random(n) * 1e-4).astype(f32)
    a = [_dev(x, cuda) for x in (p, m, v)]
    b = [_dev(x, cuda) for x in (p, m, v)]
    cls = torch.zeros(n // 64, dtype=torch.uint8, device=cuda)
    for k in range(5):
        gd = _dev((rng.standard_normal(n) * 1e-2).astype(f32), cuda)
        _lib.check(lib.sr_adam_step_f32(_p(a[0]), _p(gd), _p(a[1]), _p(a[2]), n, step0 + k, LR, B1, B2, ADAM_EPS, wd, gs, None, None,
                                        _st()), 'sr_adam_step_f32')
        _groups(lib, b[0], gd, b[1], b[2], n, cls, [(LR, step0 + k, 1)], wd, gs)
        for x, y, what in zip(a, b, ('param', 'exp_avg', 'exp_avg_sq')):
            assert np.array_equal(_bits(x), _bits(y)), (what, k)
    assert float(a[0].abs().sum()) > 0 and not np.array_equal(_bits(a[0]), p.view(np.int32))


# ---------------------------------------------------------------------------------------------------------- 2. four classes
SEGS = [64, 64 * 3, 64 * 1000, 64]          # floats per segment; segment k is class k
ROWS = [(LR, 1, 1), (LR, 3, 0), (0.25 * LR, 7, 1), (LR, 7, 1)]   # the frozen class sits between two live ones
STEPS = 5
_RUNS = {}


def _four_inputs():
    n = sum(SEGS)
    rng = np.random.default_rng(2024)
    start = np.cumsum([0] + SEGS)
    p = rng.standard_normal(n).astype(f32)
    m = (rng.standard_normal(n) * 1e-2).astype(f32)
    v = (rng.random(n) * 1e-4).astype(f32)
    m[start[0]:start[1]] = 0   # the class at step 1 starts from zero moments
    v[start[0]:start[1]] = 0
    lo, hi = start[1], start[2]
    # the frozen segment: nothing of it may be read, so all four arrays hold NaN there, each slot with its own payload
    p[lo:hi], m[lo:hi], v[lo:hi] = _nan_pattern(hi - lo, 1), _nan_pattern(hi - lo, 2), _nan_pattern(hi - lo, 3)
    grads = []
    for k in range(STEPS):
        g = (rng.standard_normal(n) * 1e-2).astype(f32)
        g[lo:hi] = _nan_pattern(hi - lo, 4 + k)
        grads.append(g)
    cls = np.repeat(np.arange(4, dtype=np.uint8), [s // 64 for s in SEGS])
    return n, start, p, m, v, grads, cls


def _four(cuda, lib, rows_key='plain', fresh=False):
    """Five steps of the four-class case on the device; results are cached per class table so the reference is computed once."""
    if rows_key in _RUNS and not fresh:
        return _RUNS[rows_key]
    n, start, p, m, v, grads, cls = _four_inputs()
    rows = list(ROWS)
    if rows_key == 'swapped':   # classes 0 and 2 trade their learning rates
        rows[0], rows[2] = (ROWS[2][0], ROWS[0][1], 1), (ROWS[0][0], ROWS[2][1], 1)
    pd, md, vd, cd = _dev(p, cuda), _dev(m, cuda), _dev(v, cuda), _dev(cls, cuda)
    for k in range(STEPS):
        gd = _dev(grads[k], cuda)
        _groups(lib, pd, gd, md, vd, n, cd, [(lr, s + k, a) for lr, s, a in rows], wd=0.01, gs=0.5)
    out = tuple(t.cpu().numpy() for t in (pd, md, vd))
    if not fresh:
        _RUNS[rows_key] = out
    return out


def _segment_errors(got, seg):
    """(|m - M|, bound), (|v - V|, bound), (|p - P|, bound) of segment `seg` against float64 Adam with ROWS[seg]."""
    n, start, p, m, v, grads, _ = _four_inputs()
    lo, hi = start[seg], start[seg + 1]
    lr, step0, _ = ROWS[seg]
    c = [float(f32(a)) for a in (lr, B1, B2, ADAM_EPS, 0.01, 0.5)]
    P, M, V = (a[lo:hi].astype(np.float64) for a in (p, m, v))
    mabs, upd_sum = np.abs(M), np.zeros(hi - lo)
    for k in range(STEPS):
        P, M, V, mabs, upd = _adam_ref(P, M, V, grads[k][lo:hi].astype(np.float64), step0 + k, *c, mabs)
        upd_sum += upd
    gp, gm, gv = (a[lo:hi].astype(np.float64) for a in got)
    return ((np.abs(gm - M), 4 * STEPS * EPS * mabs + FLT_MIN), (np.abs(gv - V), 6 * STEPS * EPS * V + FLT_MIN),
            (np.abs(gp - P), EPS * (2 * STEPS * np.abs(P) + 32 * upd_sum) + FLT_MIN))


def test_four_classes_match_float64_adam_per_segment_and_leave_the_frozen_one_alone(cuda, lib):
    got = _four(cuda, lib)
    n, start, p, m, v, grads, _ = _four_inputs()
    for seg in (0, 2, 3):
        for (err, bound), what in zip(_segment_errors(got, seg), ('exp_avg', 'exp_avg_sq', 'param')):
            print(f'segment {seg} {what}: max err / bound = {float((err / bound).max()):.3f}')
            assert np.isfinite(err).all() and (err <= bound).all(), (seg, what)
    lo, hi = start[1], start[2]
    for a, b, what in zip(got, (p, m, v), ('param', 'exp_avg', 'exp_avg_sq')):
        assert np.array_equal(a[lo:hi].view(np.int32), b[lo:hi].view(np.int32)), what   # bit-unchanged, payloads included


def test_swapping_two_learning_rates_leaves_the_bound(cuda, lib):
    """Negative control: were the class table ignored or mis-indexed, the test above could not tell.  Classes 0 and 2 trade their
    rates (a factor 4): both segments must leave the parameter bound, the untouched class 3 must stay inside."""
    got = _four(cuda, lib, 'swapped')
    for seg in (0, 2):
        err, bound = _segment_errors(got, seg)[2]
        assert (err > bound).mean() > 0.9, seg
    err, bound = _segment_errors(got, 3)[2]
    assert (err <= bound).all()


def test_two_runs_are_bit_identical(cuda, lib):
    first, again = _four(cuda, lib), _four(cuda, lib, fresh=True)
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


# --------------------------------------------------------------------------------------------- 3. smallest arena, bad class id
def test_one_chunk_and_a_class_id_out_of_range(cuda, lib):
    rng = np.random.default_rng(5)
    p, g = rng.standard_normal(64).astype(f32), (rng.standard_normal(64) * 1e-2).astype(f32)
    a = [_dev(x, cuda) for x in (p, np.zeros(64, f32), np.zeros(64, f32))]
    b = [_dev(x, cuda) for x in (p, np.zeros(64, f32), np.zeros(64, f32))]
    gd = _dev(g, cuda)
    _lib.check(lib.sr_adam_step_f32(_p(a[0]), _p(gd), _p(a[1]), _p(a[2]), 64, 1, LR, B1, B2, ADAM_EPS, 0.0, 1.0, None, None, _st()),
               'sr_adam_step_f32')
    _groups(lib, b[0], gd, b[1], b[2], 64, torch.zeros(1, dtype=torch.uint8, device=cuda), [(LR, 1, 1)])
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    assert not np.array_equal(_bits(b[0]), p.view(np.int32))
    # two chunks, one class: the second chunk says class 5 (and 255) and must be left alone, NaN gradient and all
    for bad in (1, 5, 255):
        p2 = np.concatenate([p, _nan_pattern(64, 9)])
        g2 = np.concatenate([g, _nan_pattern(64, 10)])
        z2 = np.concatenate([np.zeros(64, f32), _nan_pattern(64, 11)])
        c = [_dev(x, cuda) for x in (p2, z2, z2.copy())]
        _groups(lib, c[0], _dev(g2, cuda), c[1], c[2], 128, _dev(np.array([0, bad], np.uint8), cuda), [(LR, 1, 1)])
        for x, y, src in zip(c, b, (p2, z2, z2)):
            assert np.array_equal(_bits(x)[:64], _bits(y)), bad
            assert np.array_equal(_bits(x)[64:], src[64:].view(np.int32)), bad


# ------------------------------------------------------------------------------------------------------------ 4. abort word
def test_a_raised_abort_word_refuses_the_whole_call_once(cuda, lib):
    n, start, p, m, v, grads, cls = _four_inputs()
    pd, md, vd, cd, gd = _dev(p, cuda), _dev(m, cuda), _dev(v, cuda), _dev(cls, cuda), _dev(grads[0], cuda)
    word = torch.ones(1, dtype=torch.int32, device=cuda)
    skipped = torch.zeros(1, dtype=torch.int32, device=cuda)
    _groups(lib, pd, gd, md, vd, n, cd, ROWS, wd=0.01, gs=0.5, word=word, skipped=skipped)
    for t, src in zip((pd, md, vd), (p, m, v)):
        assert np.array_equal(_bits(t), src.view(np.int32))
    assert int(skipped.item()) == 1
    word.zero_()   # the same call with the word down steps, and does not count
    _groups(lib, pd, gd, md, vd, n, cd, ROWS, wd=0.01, gs=0.5, word=word, skipped=skipped)
    assert int(skipped.item()) == 1 and not np.array_equal(_bits(pd), p.view(np.int32))
