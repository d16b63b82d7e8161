"""float64 restatement in numpy of DUF (reference: basicsr/archs/duf_arch.py), written from the definition: 3D convolutions as
shifted slices over (time, row, column), explicit eval-mode BatchNorm3d, the softmax over the 25 taps, the 5x5 dynamic filter as 25
shifted slices of the centre frame, and the pixel shuffle.  The yardstick of tests/test_duf_host.py (which checks it against the
reference's own float64 outputs, tests/golden/g_zj_duf.npz), tests/test_duf_ops_gpu.py and tests/test_duf_gpu.py.

Also here, shared with tools/make_golden_duf.py: the cases of the fixture, the 8-bit input clips (tests/tof_restate.clip_u8) and
the closed-form Gaussian kernel and downsampling of the DUF test set.
"""
import numpy as np

from tof_restate import clip_u8, decode  # noqa: F401  (the same seeded clips as the TOFlow fixture's recipe)

# (tag, num_layer, scale, b, h, w, adapt_official_weights)
CASES = (('l16_x4_b2_8x12', 16, 4, 2, 8, 12, False), ('l28_x3_9x17', 28, 3, 1, 9, 17, True),
         ('l52_x4_12x20', 52, 4, 1, 12, 20, True), ('l52_x2_16x16', 52, 2, 1, 16, 16, False))
WEIGHT_SEED, INPUT_SEED = 20262, 57
BLOCKS = {16: (3, 32), 28: (9, 16), 52: (21, 16)}


def eps_of(adapt):
    return 1e-3 if adapt else 1e-5


# -------------------------------------------------------------------------------------------------------------- pieces
def conv3d(x, weight, bias=None, pad_t=0, want_mag=False):
    """nn.Conv3d(cin, cout, (kt, k, k), 1, (pad_t, k // 2, k // 2)) on [n, c, t, h, w].  Returns (out, sum of |terms| or None)."""
    x, weight = np.asarray(x, np.float64), np.asarray(weight, np.float64)
    n, c, t, h, w = x.shape
    kt, k = weight.shape[2], weight.shape[3]
    p = k // 2
    xp = np.zeros((n, c, t + 2 * pad_t, h + 2 * p, w + 2 * p))
    xp[:, :, pad_t:pad_t + t, p:p + h, p:p + w] = x
    to = t + 2 * pad_t - kt + 1
    out = np.zeros((n, weight.shape[0], to, h, w))
    mag = np.zeros_like(out) if want_mag else None
    for dt in range(kt):
        for dy in range(k):
            for dx in range(k):
                s = xp[:, :, dt:dt + to, dy:dy + h, dx:dx + w]
                out += np.tensordot(weight[:, :, dt, dy, dx], s, axes=([1], [1])).transpose(1, 0, 2, 3, 4)
                if want_mag:
                    mag += np.tensordot(np.abs(weight[:, :, dt, dy, dx]), np.abs(s), axes=([1], [1])).transpose(1, 0, 2, 3, 4)
    if bias is not None:
        b = np.asarray(bias, np.float64)[None, :, None, None, None]
        out = out + b
        if want_mag:
            mag = mag + np.abs(b)
    return out, mag


def batchnorm_eval(x, gamma, beta, mean, var, eps):
    g, b, m, v = (np.asarray(t, np.float64).reshape((1, -1) + (1,) * (x.ndim - 2)) for t in (gamma, beta, mean, var))
    return (x - m) / np.sqrt(v + eps) * g + b


def fold(weight, bias, gamma, beta, mean, var, eps):
    """(w', b') of eval-mode BatchNorm behind a conv with a bias, in float64."""
    s = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    w = np.asarray(weight, np.float64)
    return w * s.reshape((-1,) + (1,) * (w.ndim - 1)), (np.asarray(bias, np.float64) - np.asarray(mean, np.float64)) * s + np.asarray(beta, np.float64)


def prologue_arrays(gamma, beta, mean, var, eps):
    """(scale, shift) of eval-mode BatchNorm in front of a conv, in float64."""
    s = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    return s, np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * s


def softmax_taps(logits):
    """softmax over axis 1 of [n, 25, s2, h, w]."""
    e = np.exp(logits - logits.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def dynamic_filter(x, filters):
    """DynamicUpsamplingFilter((5, 5)).forward: x [n, 3, h, w], filters [n, 25, s2, h, w] -> [n, 3 * s2, h, w]."""
    x, filters = np.asarray(x, np.float64), np.asarray(filters, np.float64)
    n, _, h, w = x.shape
    s2 = filters.shape[2]
    xp = np.zeros((n, 3, h + 4, w + 4))
    xp[:, :, 2:2 + h, 2:2 + w] = x
    out = np.zeros((n, 3, s2, h, w))
    for tap in range(25):
        dy, dx = divmod(tap, 5)
        out += xp[:, :, None, dy:dy + h, dx:dx + w] * filters[:, None, tap]
    return out.reshape(n, 3 * s2, h, w)


def pixel_shuffle(x, s):
    n, c, h, w = x.shape
    return x.reshape(n, c // (s * s), s, s, h, w).transpose(0, 1, 4, 2, 5, 3).reshape(n, c // (s * s), h * s, w * s)


def tail(logits, res, centre, s):
    """softmax, filter, + res, shuffle: logits [n, 25 s2, h, w], res [n, 3 s2, h, w] or None, centre [n, 3, h, w]."""
    n, _, h, w = logits.shape
    out = dynamic_filter(centre, softmax_taps(np.asarray(logits, np.float64).reshape(n, 25, s * s, h, w)))
    if res is not None:
        out = out + res
    return pixel_shuffle(out, s)


# ------------------------------------------------------------------------------------------------------------- network
def _bn(sd, name, x, eps):
    return batchnorm_eval(x, *(sd[f'{name}.{p}'] for p in ('weight', 'bias', 'running_mean', 'running_var')), eps)


def _dense(sd, name, x, pad_t, eps, fractions):
    y = _bn(sd, name + '.0', x, eps)
    if fractions is not None:
        fractions.append(float((y > 0).mean()))
    y, _ = conv3d(np.maximum(y, 0), sd[name + '.2.weight'], sd[name + '.2.bias'])
    y = np.maximum(_bn(sd, name + '.3', y, eps), 0)
    y, _ = conv3d(y, sd[name + '.5.weight'], sd[name + '.5.bias'], pad_t)
    return np.concatenate([x if pad_t else x[:, :, 1:-1], y], 1)


def duf(sd, x, num_layer, scale, adapt=False, keep=None):
    """DUF.forward in float64 on x [b, 7, 3, h, w]: the output [b, 3, s h, s w].  ``keep`` (a dict) receives ``logits``
    [b, 25 s2, h, w], ``res`` [b, 3 s2, h, w] and ``fractions``, the share of elements that pass the ReLU behind the first
    BatchNorm of every dense block."""
    x = np.asarray(x, np.float64)
    eps = eps_of(adapt)
    nb, _ = BLOCKS[num_layer]
    fractions = [] if keep is not None else None
    centre = x[:, 3]
    f, _ = conv3d(x.transpose(0, 2, 1, 3, 4), sd['conv3d1.weight'], sd['conv3d1.bias'])
    for i in range(nb):
        f = _dense(sd, f'dense_block1.dense_blocks.{i}', f, 1, eps, fractions)
    for i in range(3):
        f = _dense(sd, f'dense_block2.temporal_reduce{i + 1}', f, 0, eps, fractions)
    f = np.maximum(_bn(sd, 'bn3d2', f, eps), 0)
    f, _ = conv3d(f, sd['conv3d2.weight'], sd['conv3d2.bias'])
    f = np.maximum(f, 0)
    r, _ = conv3d(f, sd['conv3d_r1.weight'], sd['conv3d_r1.bias'])
    res, _ = conv3d(np.maximum(r, 0), sd['conv3d_r2.weight'], sd['conv3d_r2.bias'])
    g, _ = conv3d(f, sd['conv3d_f1.weight'], sd['conv3d_f1.bias'])
    logits, _ = conv3d(np.maximum(g, 0), sd['conv3d_f2.weight'], sd['conv3d_f2.bias'])
    logits, res = logits[:, :, 0], res[:, :, 0]
    if keep is not None:
        keep.update(logits=logits, res=res, fractions=np.array(fractions))
    return tail(logits, res, centre, scale)


def nearest_up(x, s):
    return np.repeat(np.repeat(x, s, axis=-2), s, axis=-1)


# ------------------------------------------------------------------------------------------------ the DUF test set's blur
def gaussian_kernel(kernel_size=13, sigma=1.6):
    """The Gaussian kernel of ``duf_downsample`` in closed form: the outer product of the 1D Gaussian exp(-x^2 / (2 sigma^2)),
    truncated at radius int(4 sigma + 0.5) and normalised to sum 1, placed at the centre of ``kernel_size`` taps.  The radius must
    fit: then smoothing a unit impulse meets no boundary."""
    radius = int(4.0 * sigma + 0.5)
    assert radius <= kernel_size // 2, (kernel_size, sigma)
    xs = np.arange(-radius, radius + 1, dtype=np.float64)
    g = np.exp(-0.5 / (sigma * sigma) * xs ** 2)
    g = g / g.sum()
    k1 = np.zeros(kernel_size)
    k1[kernel_size // 2 - radius:kernel_size // 2 + radius + 1] = g
    return np.outer(k1, k1)


def duf_downsample(x, kernel_size=13, scale=4):
    """``duf_downsample`` of the reference on [b, t, c, h, w] (or [t, c, h, w]) in float64: reflect padding by
    kernel_size // 2 + 2 scale, the Gaussian with sigma 0.4 scale at stride ``scale``, two rows and columns cut from every side."""
    x = np.asarray(x, np.float64)
    squeeze = x.ndim == 4
    if squeeze:
        x = x[None]
    b, t, c, h, w = x.shape
    pad = kernel_size // 2 + scale * 2
    xp = np.pad(x.reshape(-1, h, w), ((0, 0), (pad, pad), (pad, pad)), mode='reflect')
    k = gaussian_kernel(kernel_size, 0.4 * scale)
    ho, wo = (h + 2 * pad - kernel_size) // scale + 1, (w + 2 * pad - kernel_size) // scale + 1
    out = np.zeros((xp.shape[0], ho, wo))
    for dy in range(kernel_size):
        for dx in range(kernel_size):
            out += k[dy, dx] * xp[:, dy:dy + (ho - 1) * scale + 1:scale, dx:dx + (wo - 1) * scale + 1:scale]
    out = out[:, 2:-2, 2:-2].reshape(b, t, c, ho - 4, wo - 4)
    return out[0] if squeeze else out
