"""float64 restatement in numpy of TOFlow (reference: basicsr/archs/tof_arch.py), written from the definition: shifted-slice
convolutions, explicit eval-mode BatchNorm, the corner-sum warp and the upsampling of tests/flow_restate.py.  The yardstick of
tests/test_tof_host.py (which checks it against the reference's own float64 outputs, tests/golden/g_zi_tof.npz),
tests/test_tof_ops_gpu.py and tests/test_tof_gpu.py.

Also here, shared with tools/make_golden_tof.py: the cases of the fixture and the decoding of its 8-bit input clips.
"""
import numpy as np

import flow_restate as R

CHANNELS = R.CHANNELS
MEAN, STD = R.MEAN, R.STD
EPS = 1e-5
OFFICIAL_ORDER = (3, 0, 1, 2, 4, 5, 6)
CASES = (('b2_16x16', 2, 16, 16), ('32x48', 1, 32, 48), ('48x80', 1, 48, 80))     # (tag, b, h, w)
WEIGHT_SEED, INPUT_SEED = 20261, 91


def clip_u8(seed, b, h, w):
    """A seeded 7-frame clip as uint8 [b, 7, 3, h, w]: a few sinusoids that drift by (0.9, -0.6) px per frame, plus noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    f = rng.uniform(0.05, 0.6, (6, b, 3, 2, 1, 1))
    ph = rng.uniform(0, 2 * np.pi, (6, b, 3, 1, 1))
    amp = rng.uniform(0.3, 1.0, (6, b, 3, 1, 1))
    frames = []
    for t in range(7):
        img = np.zeros((b, 3, h, w))
        for k in range(6):
            img += amp[k] * np.sin(f[k][:, :, 0] * (xx + 0.9 * (t - 3)) + f[k][:, :, 1] * (yy - 0.6 * (t - 3)) + ph[k])
        frames.append(img)
    clip = np.stack(frames, 1)
    clip = (clip - clip.min()) / (clip.max() - clip.min()) * 0.9 + 0.08 * rng.uniform(0, 1, clip.shape)
    return np.clip(np.rint(clip * 255.0), 0, 255).astype(np.uint8)


def decode(u8):
    """The fp32 clip in [0, 1] the networks see."""
    return u8.astype(np.float32) / np.float32(255.0)


# -------------------------------------------------------------------------------------------------------------- pieces
def conv(x, weight, bias=None, relu=False, want_mag=False):
    """Conv2d(k, 1, k // 2) as k * k shifted slices.  Returns (out, sum of |terms| or None)."""
    x, weight = np.asarray(x, np.float64), np.asarray(weight, np.float64)
    n, c, h, w = x.shape
    k = weight.shape[2]
    p = k // 2
    xp = np.zeros((n, c, h + 2 * p, w + 2 * p))
    xp[:, :, p:p + h, p:p + w] = x
    out = np.zeros((n, weight.shape[0], h, w))
    mag = np.zeros_like(out) if want_mag else None
    for dy in range(k):
        for dx in range(k):
            s = xp[:, :, dy:dy + h, dx:dx + w]
            out += np.tensordot(weight[:, :, dy, dx], s, axes=([1], [1])).transpose(1, 0, 2, 3)
            if want_mag:
                mag += np.tensordot(np.abs(weight[:, :, dy, dx]), np.abs(s), axes=([1], [1])).transpose(1, 0, 2, 3)
    if bias is not None:
        b = np.asarray(bias, np.float64)[None, :, None, None]
        out = out + b
        if want_mag:
            mag = mag + np.abs(b)
    return (np.maximum(out, 0) if relu else out), mag


def batchnorm_eval(x, gamma, beta, mean, var, eps=EPS):
    g, b, m, v = (np.asarray(t, np.float64)[None, :, None, None] for t in (gamma, beta, mean, var))
    return (x - m) / np.sqrt(v + eps) * g + b


def fold(weight, gamma, beta, mean, var, eps=EPS):
    """(w', b') of the fold, in float64."""
    s = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    return np.asarray(weight, np.float64) * s[:, None, None, None], np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * s


def level_input(ref, supp, flow_prev, coord_dtype=np.float64):
    """(the 8-channel input of a level, up): tof_arch.py:86-89, zeros padding."""
    n, _, h, w = ref.shape
    up = np.zeros((n, 2, h, w)) if flow_prev is None else 2.0 * R.upsample2_align(np.asarray(flow_prev, np.float64))
    warped = R.flow_warp(supp, up.transpose(0, 2, 3, 1), 'zeros', coord_dtype)
    return np.concatenate([np.asarray(ref, np.float64), warped, up], 1), up


def spynet(sd, ref, supp, prefix='spynet.'):
    """SPyNetTOF.forward in float64: the flow [N, 2, h, w]."""
    refs, supps = [np.asarray(ref, np.float64)], [np.asarray(supp, np.float64)]
    for _ in range(3):
        refs.insert(0, R.avgpool2(refs[0]))
        supps.insert(0, R.avgpool2(supps[0]))
    flow = None
    for level in range(4):
        x, up = level_input(refs[level], supps[level], flow)
        base = f'{prefix}basic_module.{level}.basic_module.'
        for i in range(4):
            x, _ = conv(x, sd[f'{base}{3 * i}.weight'])
            x = np.maximum(batchnorm_eval(x, *(sd[f'{base}{3 * i + 1}.{p}'] for p in ('weight', 'bias', 'running_mean', 'running_var'))), 0)
        x, _ = conv(x, sd[base + '12.weight'], sd[base + '12.bias'])
        flow = x + up
    return flow


def aligned_stack(clip, flows, ref_idx, coord_dtype=np.float64):
    """tof_arch.py:154-166: [b, 21, h, w] from the normalised clip and the flows [b, 6, 2, h, w]."""
    out, k = [], 0
    for i in range(7):
        if i == ref_idx:
            out.append(np.asarray(clip[:, i], np.float64))
        else:
            out.append(R.flow_warp(clip[:, i], np.asarray(flows[:, k]).transpose(0, 2, 3, 1), 'zeros', coord_dtype))
            k += 1
    return np.concatenate(out, 1)


def finish(y, lr_ref, mean=MEAN, std=STD):
    return (y + lr_ref) * std[None, :, None, None] + mean[None, :, None, None]


def toflow(sd, lrs, adapt_official_weights=False):
    """(output [b, 3, h, w], flows [6 b, 2, h, w] with image 6 b + k) of TOFlow.forward in float64."""
    lrs = np.asarray(lrs, np.float64)
    if adapt_official_weights:
        lrs = lrs[:, list(OFFICIAL_ORDER)]
    ref_idx = 0 if adapt_official_weights else 3
    b, _, _, h, w = lrs.shape
    mean, std = (np.asarray(sd[k], np.float32).astype(np.float64).reshape(3) for k in ('mean', 'std'))
    clip = (lrs - mean[None, None, :, None, None]) / std[None, None, :, None, None]
    others = [i for i in range(7) if i != ref_idx]
    ref = np.repeat(clip[:, ref_idx:ref_idx + 1], 6, 1).reshape(b * 6, 3, h, w)
    supp = clip[:, others].reshape(b * 6, 3, h, w)
    flows = spynet(sd, ref, supp)
    x = aligned_stack(clip, flows.reshape(b, 6, 2, h, w), ref_idx)
    x, _ = conv(x, sd['conv_1.weight'], sd['conv_1.bias'], relu=True)
    x, _ = conv(x, sd['conv_2.weight'], sd['conv_2.bias'], relu=True)
    x, _ = conv(x, sd['conv_3.weight'], sd['conv_3.bias'], relu=True)
    y, _ = conv(x, sd['conv_4.weight'], sd['conv_4.bias'])
    return finish(y, clip[:, ref_idx], mean, std), flows
