"""float64 restatement in numpy of flow warping and SpyNet (reference: basicsr/archs/arch_util.py:112-143,
basicsr/archs/spynet_arch.py), written from the definition: explicit corner sums and shifted-slice convolutions, no grid_sample
and no conv2d, with analytic dx and dflow.  The yardstick of tests/test_flow_host.py, tests/test_flow_ops_gpu.py and
tests/test_spynet_gpu.py; tests/test_flow_host.py checks it against the reference's own outputs (tests/golden/g_zd_spynet.npz).

Also here, shared by tools/make_golden_spynet.py and the tests: the seeded SpyNet weights (``spynet_weights``) — the fixture
stores the seed and a checksum, not the 1.44 M values.
"""
import hashlib

import numpy as np

CHANNELS = ((8, 32), (32, 64), (64, 32), (32, 16), (16, 2))
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32).astype(np.float64)   # the fp32 buffers of the module
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ weights
def spynet_weights(seed, last_scale=16.0):
    """state_dict (numpy float32) of a SpyNet drawn from one seeded generator: nn.Conv2d's default ranges (U(+-1/sqrt(fan_in))
    for weight and bias), except the last conv of every level, whose weight is scaled by ``last_scale`` and whose bias is
    U(-0.5, 0.5) — default init gives flows below one pixel, which tests no warping."""
    rng = np.random.default_rng(seed)
    sd = {'mean': MEAN.astype(np.float32).reshape(1, 3, 1, 1), 'std': STD.astype(np.float32).reshape(1, 3, 1, 1)}
    for level in range(6):
        for i, (cin, cout) in enumerate(CHANNELS):
            bound = 1.0 / np.sqrt(cin * 49.0)
            w = rng.uniform(-bound, bound, (cout, cin, 7, 7))
            b = rng.uniform(-bound, bound, (cout,))
            if i == 4:
                w = w * last_scale
                b = rng.uniform(-0.5, 0.5, (cout,))
            sd[f'basic_module.{level}.basic_module.{2 * i}.weight'] = w.astype(np.float32)
            sd[f'basic_module.{level}.basic_module.{2 * i}.bias'] = b.astype(np.float32)
    return sd


def spynet_inputs(seed, n, h, w):
    """(ref, supp) float32 [n, 3, h, w] in [0, 1]: a few seeded sinusoids plus noise; supp is the same scene displaced."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')

    def scene(dx, dy):
        img = np.zeros((n, 3, h, w))
        for k in range(6):
            f = r.uniform(0.02, 0.35, (n, 3, 2, 1, 1))
            ph = r.uniform(0, 2 * np.pi, (n, 3, 1, 1))
            img += r.uniform(0.3, 1.0, (n, 3, 1, 1)) * np.sin(f[:, :, 0] * (xx + dx) + f[:, :, 1] * (yy + dy) + ph)
        return img
    r = np.random.default_rng(seed + 1)
    a = scene(0.0, 0.0)
    r = np.random.default_rng(seed + 1)
    b = scene(2.5, -1.75)
    lo, hi = a.min(), a.max()
    ref = (a - lo) / (hi - lo) * 0.9 + 0.05 * rng.uniform(0, 1, a.shape)
    supp = np.clip((b - lo) / (hi - lo), 0, 1) * 0.9 + 0.05 * rng.uniform(0, 1, a.shape)
    return ref.astype(np.float32), supp.astype(np.float32)


def weights_checksum(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------------ warping
def warp_coords(flow, h, w, padding):
    """(x0, y0, fx, fy, gx_on, gy_on) of every output pixel from ``flow`` [N, H, W, 2] in the arithmetic of ``flow``'s dtype
    (float64 for the exact definition; float32 to restate the kernel's coordinate roundings)."""
    dt = flow.dtype
    gy, gx = np.meshgrid(np.arange(h, dtype=dt), np.arange(w, dtype=dt), indexing='ij')
    ix = (gx + flow[..., 0]).astype(dt) if w > 1 else np.zeros(flow.shape[:3], dt)
    iy = (gy + flow[..., 1]).astype(dt) if h > 1 else np.zeros(flow.shape[:3], dt)
    gx_on, gy_on = np.full(ix.shape, w > 1), np.full(iy.shape, h > 1)
    if padding == 'border':
        gx_on &= (ix >= 0) & (ix <= w - 1)
        gy_on &= (iy >= 0) & (iy <= h - 1)
        ix, iy = np.clip(ix, 0, w - 1), np.clip(iy, 0, h - 1)
    x0, y0 = np.floor(ix), np.floor(iy)
    return x0.astype(np.int64), y0.astype(np.int64), (ix - x0).astype(np.float64), (iy - y0).astype(np.float64), gx_on, gy_on


def _corner(x, yy, xx):
    """x[n, :, yy, xx] with zeros outside the image; also the validity mask."""
    n, c, h, w = x.shape
    ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
    yc, xc = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
    v = x[np.arange(n)[:, None, None], :, yc, xc]                 # [N, H, W, C]
    return np.where(ok[..., None], v, 0.0).transpose(0, 3, 1, 2), ok


def flow_warp(x, flow, padding='zeros', coord_dtype=np.float64):
    """out [N, C, H, W] in float64.  ``coord_dtype=np.float32`` rounds the sampling position as the kernel does."""
    x = np.asarray(x, np.float64)
    n, c, h, w = x.shape
    x0, y0, fx, fy, _, _ = warp_coords(np.asarray(flow, coord_dtype), h, w, padding)
    v00, _ = _corner(x, y0, x0)
    v01, _ = _corner(x, y0, x0 + 1)
    v10, _ = _corner(x, y0 + 1, x0)
    v11, _ = _corner(x, y0 + 1, x0 + 1)
    fx, fy = fx[:, None], fy[:, None]
    return (1 - fy) * ((1 - fx) * v00 + fx * v01) + fy * ((1 - fx) * v10 + fx * v11)


def flow_warp_bwd(x, flow, g, padding='zeros', coord_dtype=np.float64):
    """(dx, dflow, count, absterms): the analytic gradients in float64, the number of non-zero contributions each element of
    dx receives, and the sum of their magnitudes."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    n, c, h, w = x.shape
    x0, y0, fx, fy, gx_on, gy_on = warp_coords(np.asarray(flow, coord_dtype), h, w, padding)
    cs = [_corner(x, y0, x0), _corner(x, y0, x0 + 1), _corner(x, y0 + 1, x0), _corner(x, y0 + 1, x0 + 1)]
    (v00, _), (v01, _), (v10, _), (v11, _) = cs
    fxe, fye = fx[:, None], fy[:, None]
    dfx = (g * ((1 - fye) * (v01 - v00) + fye * (v11 - v10))).sum(1) * gx_on
    dfy = (g * ((1 - fxe) * (v10 - v00) + fxe * (v11 - v01))).sum(1) * gy_on
    dx, absterms = np.zeros_like(x), np.zeros_like(x)
    count = np.zeros(x.shape, np.int64)
    wts = [(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx]
    offs = [(0, 0), (0, 1), (1, 0), (1, 1)]
    ni = np.broadcast_to(np.arange(n)[:, None, None], x0.shape)
    for (oy, ox), wt, (_, ok) in zip(offs, wts, cs):
        sel = ok & (wt != 0)
        nn_, yy, xx = ni[sel], (y0 + oy)[sel], (x0 + ox)[sel]
        for ch in range(c):
            term = (g[:, ch] * wt)[sel]
            np.add.at(dx[:, ch], (nn_, yy, xx), term)
            np.add.at(absterms[:, ch], (nn_, yy, xx), np.abs(term))
            np.add.at(count[:, ch], (nn_, yy, xx), 1)
    return dx, np.stack([dfx, dfy], -1), count, absterms


# ------------------------------------------------------------------------------------------------------------- SpyNet
def conv7x7(x, weight, bias, relu=False, want_mag=True):
    """Conv2d(k7, s1, p3) as 49 shifted slices.  Returns (out, sum of |terms|) for the rounding bounds (None when not wanted)."""
    x, weight = np.asarray(x, np.float64), np.asarray(weight, np.float64)
    n, c, h, w = x.shape
    xp = np.zeros((n, c, h + 6, w + 6))
    xp[:, :, 3:3 + h, 3:3 + w] = x
    out = np.zeros((n, weight.shape[0], h, w))
    mag = np.zeros_like(out) if want_mag else None
    for dy in range(7):
        for dx in range(7):
            s = xp[:, :, dy:dy + h, dx:dx + w]
            out += np.tensordot(weight[:, :, dy, dx], s, axes=([1], [1])).transpose(1, 0, 2, 3)
            if want_mag:
                mag += np.tensordot(np.abs(weight[:, :, dy, dx]), np.abs(s), axes=([1], [1])).transpose(1, 0, 2, 3)
    b = np.asarray(bias, np.float64)[None, :, None, None]
    out = out + b
    if want_mag:
        mag = mag + np.abs(b)
    return (np.maximum(out, 0) if relu else out), mag


def resize_half_pixel(x, oh, ow):
    """F.interpolate(bilinear, align_corners=False) in float64."""
    x = np.asarray(x, np.float64)
    h, w = x.shape[2:]

    def axis(n_in, n_out):
        s = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0)
        i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), np.where(i0 >= n_in - 1, 0.0, s - i0)
    y0, y1, fy = axis(h, oh)
    x0, x1, fx = axis(w, ow)
    fy, fx = fy[:, None], fx[None, :]
    top = (1 - fx) * x[:, :, y0][:, :, :, x0] + fx * x[:, :, y0][:, :, :, x1]
    bot = (1 - fx) * x[:, :, y1][:, :, :, x0] + fx * x[:, :, y1][:, :, :, x1]
    return (1 - fy) * top + fy * bot


def upsample2_align(x):
    """F.interpolate(scale_factor=2, bilinear, align_corners=True) in float64."""
    h, w = x.shape[2:]

    def axis(n_in):
        n_out = 2 * n_in
        s = np.arange(n_out) * ((n_in - 1) / (n_out - 1)) if n_out > 1 else np.zeros(n_out)
        i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), s - i0
    y0, y1, fy = axis(h)
    x0, x1, fx = axis(w)
    fy, fx = fy[:, None], fx[None, :]
    top = (1 - fx) * x[:, :, y0][:, :, :, x0] + fx * x[:, :, y0][:, :, :, x1]
    bot = (1 - fx) * x[:, :, y1][:, :, :, x0] + fx * x[:, :, y1][:, :, :, x1]
    return (1 - fy) * top + fy * bot


def avgpool2(x):
    return (x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2] + x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2]) / 4


def level_input(ref, supp, flow_prev):
    """(the 8-channel input of a level, up) from the level's images and the coarser flow (None: zero)."""
    n, _, h, w = ref.shape
    up = np.zeros((n, 2, h, w)) if flow_prev is None else 2.0 * upsample2_align(flow_prev)
    warped = flow_warp(supp, up.transpose(0, 2, 3, 1), 'border')
    return np.concatenate([ref, warped, up], 1), up


def spynet(sd, ref, supp):
    """(flow [N, 2, h, w], [flow after each level]) of SpyNet.forward in float64."""
    ref, supp = np.asarray(ref, np.float64), np.asarray(supp, np.float64)
    h, w = ref.shape[2:]
    hf, wf = -(-h // 32) * 32, -(-w // 32) * 32
    if (hf, wf) != (h, w):
        ref, supp = resize_half_pixel(ref, hf, wf), resize_half_pixel(supp, hf, wf)
    nm = lambda t: (t - MEAN[None, :, None, None]) / STD[None, :, None, None]   # noqa: E731
    refs, supps = [nm(ref)], [nm(supp)]
    for _ in range(5):
        refs.insert(0, avgpool2(refs[0]))
        supps.insert(0, avgpool2(supps[0]))
    flow, levels = None, []
    for level in range(6):
        x, up = level_input(refs[level], supps[level], flow)
        for i in range(5):
            x, _ = conv7x7(x, sd[f'basic_module.{level}.basic_module.{2 * i}.weight'],
                           sd[f'basic_module.{level}.basic_module.{2 * i}.bias'], relu=i < 4, want_mag=False)
        flow = x + up
        levels.append(flow)
    if (hf, wf) != (h, w):
        flow = resize_half_pixel(flow, h, w) * np.array([w / wf, h / hf])[None, :, None, None]
    return flow, levels
