"""A numpy model of the order-free fixed-point sum of csrc/fixed_sum.h, shared by tests/vsr_det_model.py and tests/dcn_det_model.py:
the maximum M as the unsigned maximum of sign-cleared bit patterns, its exponent e = ilogb(M) + 1, the level L = ceil(log2(count)),
a term as rint(ldexp(term, k)), the sum scaled back by ldexp(acc, -k), and the bound the two headers state."""
import numpy as np

U = 2.0 ** -24
INF_BITS = 0x7f800000


def max_bits(a):
    """The unsigned maximum of the bit patterns of |a| (fp32 array); 0 for an empty one."""
    return int((np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0x7fffffff)).max(initial=0))


def exp_of(bits):
    """ilogb(M) + 1 for a finite non-zero M given by its bits, denormals included."""
    return int(np.frexp(float(np.array(bits, np.uint32).view(np.float32)))[1])   # M = f * 2^e, f in [0.5, 1)


def level_of(count):
    """L = ceil(log2(count))."""
    L = 0
    while (1 << L) < count:
        L += 1
    return L


def quantise(term, k):
    """The integer a float64 term is added as (a float64 array of integers; the caller converts it where it sums in int64)."""
    return np.rint(np.ldexp(term, k))


def scaled_back(acc, k):
    """The float64 value of an int64 sum."""
    return np.ldexp(acc.astype(np.float64), -k)


def bound(x, count, absterms, ks):
    """2^-24 |x| + d 2^-(k + 1) + 2^-50 sum |terms| per element; ``x``: the exact result, ``count``: d, the number of terms, ``ks``:
    k per image (None for an image in which nothing is summed)."""
    out = U * np.abs(x) + 2.0 ** -50 * absterms
    for i, k in enumerate(ks):
        if k is not None:
            out[i] += count[i] * 2.0 ** -(k + 1)
    return out
