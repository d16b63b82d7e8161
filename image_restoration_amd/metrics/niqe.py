"""NIQE, the no-reference quality metric of the reference (basicsr/metrics/niqe.py:65-189), on the host and on the device.

The reference evaluates NIQE in float32 numpy + scipy: Y of the uint8 BGR image, the MSCN image at two scales
(7x7 Gaussian mean and deviation with replicated edges), per 96x96 (scale 1) / 48x48 (scale 2) block the generalised
Gaussian fits of the MSCN and of its four wrapped neighbour products, and the distance of the blocks' Gaussian model to
a pristine one.  Both forms here share one contract:

- Y and MSCN are the reference's float32 values bit for bit: every float32 operation is the one the reference performs,
  the two 49-tap convolutions sum in float64 (as scipy.ndimage.convolve does) and are rounded to float32 once.
- Per block and field the fit needs five sums only, kept in float64: n_neg, sum b^2 | b<0, n_pos, sum b^2 | b>0 and
  sum |b| ("moments", layout [block][field][5], blocks in the reference's order: block column outer, block row inner).
  The reference takes these as float32 pairwise means, so its rhatnorm carries a float32 rounding error (a few 1e-7
  relative) that the float64 sums here do not; alpha, which is the grid point nearest rhatnorm, can therefore differ
  by one grid step where rhatnorm lies that close to the midpoint of two grid points.
- One float64 host stage turns moments into the 36 features and the score (``_features`` / ``_score``).

``calculate_niqe`` is the numpy form with the reference's signature (uint8 BGR image); ``niqe_device`` reduces an NCHW
network output on the HIP device (sr_niqe_luma_f32 + sr_niqe_moments_f32) and copies back the moments only.

The pristine model (BasicSR's ``niqe_pris_params.npz``: mu_pris_param 1x36, cov_pris_param 36x36, gaussian_window 7x7)
is not shipped with the package; ``pris_params`` names the file.
"""
import math
import os

import numpy as np
import torch

from ..utils.registry import METRIC_REGISTRY
from .psnr import _to_y

BLOCK = 96
_SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))  # np.roll shifts of the four neighbour products (niqe.py:55)
_params_cache = {}


def load_niqe_params(path):
    """The pristine model of an npz in BasicSR's format, cached per path.  A mapping with the three arrays passes through."""
    if path is None:
        raise ValueError('NIQE needs the pristine model niqe_pris_params.npz (BasicSR basicsr/metrics/niqe_pris_params.npz, '
                         'arrays mu_pris_param, cov_pris_param, gaussian_window): pass pris_params=<path to it>')
    if not isinstance(path, (str, os.PathLike)):
        return {k: np.asarray(path[k], np.float64) for k in ('mu_pris_param', 'cov_pris_param', 'gaussian_window')}
    key = os.path.abspath(os.fspath(path))
    if key not in _params_cache:
        if not os.path.isfile(key):
            raise FileNotFoundError(f'NIQE pristine model {key} not found: it is BasicSR\'s basicsr/metrics/niqe_pris_params.npz '
                                    '(not shipped with this package)')
        with np.load(key) as z:
            p = {k: np.ascontiguousarray(z[k], np.float64) for k in ('mu_pris_param', 'cov_pris_param', 'gaussian_window')}
        if p['mu_pris_param'].shape != (1, 36) or p['cov_pris_param'].shape != (36, 36) or p['gaussian_window'].shape != (7, 7):
            raise ValueError(f'{key}: not a NIQE pristine model (shapes {[v.shape for v in p.values()]})')
        _params_cache[key] = p
    return _params_cache[key]


# ------------------------------------------------------------------------------------------------ the alpha grid
def _grid():
    """gam = arange(0.2, 10.001, 0.001) as the reference builds it, r_gam(gam) = G(2/a)^2 / (G(1/a) G(3/a)), and the Gamma
    values the beta and mean factors need, per grid position."""
    gam = np.arange(0.2, 10.001, 0.001)
    g = np.array([[math.gamma(k / a) for k in (1, 2, 3)] for a in gam])
    r_gam = np.square(g[:, 1]) / (g[:, 0] * g[:, 2])
    return gam, r_gam, np.sqrt(g[:, 0] / g[:, 2]), g[:, 1] / g[:, 0]


_GAM, _R_GAM, _BETA_F, _MEAN_F = _grid()


def _alpha_index(rhatnorm):
    """argmin((r_gam - rhatnorm)^2) as a nearest-neighbour search (r_gam is strictly increasing); ties and NaN go to the
    lower index, as np.argmin does (an all-NaN argument gives index 0, alpha 0.2)."""
    rn = np.asarray(rhatnorm, np.float64)
    k = np.clip(np.searchsorted(_R_GAM, np.where(np.isnan(rn), -np.inf, rn)), 1, len(_R_GAM) - 1)
    lo = k - 1
    pick = np.where((_R_GAM[lo] - rn)**2 <= (_R_GAM[k] - rn)**2, lo, k)
    return np.where(np.isnan(rn), 0, pick)


def _rhatnorm(mom, block):
    """rhatnorm and the two one-sided deviations of every [..., 5] moment vector (estimate_aggd_param, niqe.py:10-35)."""
    n_neg, s_neg, n_pos, s_pos, s_abs = np.moveaxis(mom, -1, 0)
    npx = float(block * block)
    with np.errstate(divide='ignore', invalid='ignore'):
        left, right = np.sqrt(s_neg / n_neg), np.sqrt(s_pos / n_pos)
        g = left / right
        rhat = (s_abs / npx)**2 / ((s_neg + s_pos) / npx)
        return rhat * (g**3 + 1) * (g + 1) / ((g**2 + 1)**2), left, right


def _features(mom, block):
    """[nb, 5, 5] moments of one scale -> [nb, 18] features (compute_feature, niqe.py:38-62) and [nb, 5] rhatnorm."""
    rn, left, right = _rhatnorm(mom, block)
    idx = _alpha_index(rn)
    alpha, bf = _GAM[idx], _BETA_F[idx]
    bl, br = left * bf, right * bf
    cols = [alpha[:, 0], (bl[:, 0] + br[:, 0]) / 2]
    for f in range(1, 5):
        cols += [alpha[:, f], (br[:, f] - bl[:, f]) * _MEAN_F[idx[:, f]], bl[:, f], br[:, f]]
    return np.stack(cols, axis=1), rn


def _score(feat, params):
    """Distance of the blocks' Gaussian model to the pristine one (niqe.py:131-146): nanmean over blocks, covariance of
    the blocks with no NaN feature, sqrt(d pinv((S_p + S_d) / 2) d^T)."""
    finite = ~np.isnan(feat).any(axis=1)
    if finite.sum() < 2:
        raise ValueError(f'NIQE needs at least 2 blocks of {BLOCK}x{BLOCK} pixels whose features are all finite (a flat or '
                         f'one-block image has none to fit a covariance to); this image has {int(finite.sum())}')
    mu_d = np.nanmean(feat, axis=0)
    cov_d = np.cov(feat[finite], rowvar=False)
    inv = np.linalg.pinv((params['cov_pris_param'] + cov_d) / 2)
    d = params['mu_pris_param'] - mu_d
    return float(np.sqrt(d @ inv @ d.T).reshape(()))


def _score_moments(mom1, mom2, params):
    feat = np.concatenate([_features(mom1, BLOCK)[0], _features(mom2, BLOCK // 2)[0]], axis=1)
    return _score(feat, params)


# ------------------------------------------------------------------------------------------------ host form
def _mscn(img, window):
    """MSCN of a float32 image, the reference's float32 values (niqe.py:109-112): 49 taps summed in float64 in the order
    the device sums them, the edge replicated, mu and E[x^2] rounded to float32, the rest in float32."""
    h, w = img.shape
    p = np.pad(img, 3, mode='edge')
    p64, q64 = p.astype(np.float64), np.square(p).astype(np.float64)
    mu, ex2 = np.zeros((h, w)), np.zeros((h, w))
    for a in range(7):
        for b in range(7):
            t = window[6 - a, 6 - b]  # convolution: the window is flipped
            mu += t * p64[a:a + h, b:b + w]
            ex2 += t * q64[a:a + h, b:b + w]
    mu, ex2 = mu.astype(np.float32), ex2.astype(np.float32)
    sigma = np.sqrt(np.abs(ex2 - np.square(mu)))
    return (img - mu) / (sigma + np.float32(1))


def _fields(mscn, block):
    """[nb, 5, B, B] float32: the MSCN blocks in the reference's order and their four wrapped neighbour products."""
    h, w = mscn.shape
    blocks = mscn.reshape(h // block, block, w // block, block).transpose(2, 0, 1, 3).reshape(-1, block, block)
    return np.stack([blocks] + [blocks * np.roll(blocks, s, axis=(1, 2)) for s in _SHIFTS], axis=1)


def _moments(fields):
    b = fields.reshape(fields.shape[0], 5, -1).astype(np.float64)
    neg, pos, sq = b < 0, b > 0, b * b
    return np.stack([neg.sum(-1), (sq * neg).sum(-1), pos.sum(-1), (sq * pos).sum(-1), np.abs(b).sum(-1)], axis=-1).astype(np.float64)


def _half(y):
    """Scale-2 image: cv2.resize(y / 255., (w // 2, h // 2), INTER_LINEAR) * 255. of an even-sided image as the mean of each
    2x2 cell (the exact 2x downscale), float32: (((a00 + a01) + a10) + a11) * 0.25."""
    h, w = y.shape
    a = (y / np.float32(255.)).reshape(h // 2, 2, w // 2, 2)
    return ((((a[:, 0, :, 0] + a[:, 0, :, 1]) + a[:, 1, :, 0]) + a[:, 1, :, 1]) * np.float32(0.25)) * np.float32(255.)


def _host_stages(y, window):
    """Y (cut to whole blocks) -> (mscn1, mscn2, moments1, moments2)."""
    m1 = _mscn(y, window)
    m2 = _mscn(_half(y), window)
    return m1, m2, _moments(_fields(m1, BLOCK)), _moments(_fields(m2, BLOCK // 2))


def _luma(img, crop_border, input_order):
    img = np.asarray(img).astype(np.float32)
    if input_order != 'HW':
        if input_order not in ('HWC', 'CHW'):
            raise ValueError(f'Wrong input_order {input_order}. Supported input_orders are "HW", "HWC" and "CHW"')
        if img.ndim == 2:
            img = img[..., None]
        if input_order == 'CHW':
            img = img.transpose(1, 2, 0)
        img = _to_y(img)[..., 0] if img.shape[2] == 3 else (img / 255.) * 255.  # metric_util.to_y_channel
        img = np.squeeze(img)
    if crop_border != 0:
        img = img[crop_border:-crop_border, crop_border:-crop_border]
    yh, yw = img.shape[0] // BLOCK * BLOCK, img.shape[1] // BLOCK * BLOCK
    if yh == 0 or yw == 0:
        raise ValueError(f'NIQE needs at least one {BLOCK}x{BLOCK} block after the border crop; the image is {img.shape}')
    return np.ascontiguousarray(img[:yh, :yw])


def _check_convert(convert_to):
    if convert_to != 'y':
        raise ValueError(f"NIQE convert_to={convert_to!r} is not supported: only 'y' (the Y of MATLAB's YCbCr)")


@METRIC_REGISTRY.register()
def calculate_niqe(img, crop_border, input_order='HWC', convert_to='y', pris_params=None):
    """NIQE of a uint8-range image (BGR for 'HWC' / 'CHW'), the reference's calculate_niqe (niqe.py:149-189) with the
    pristine model named by ``pris_params``."""
    _check_convert(convert_to)
    params = load_niqe_params(pris_params)
    y = _luma(img, crop_border, input_order)
    _, _, mom1, mom2 = _host_stages(y, params['gaussian_window'])
    return _score_moments(mom1, mom2, params)


# ------------------------------------------------------------------------------------------------ device form
def _device_stages(sr, crop_border, window, want_mscn=False):
    """NCHW output in [0, 1] (C = 3 RGB, C = 1 grey) -> (y [n, yh, yw] f32, moments [2, n, nb, 5, 5] f64 and, on request,
    the MSCN images (scale 1, scale 2)), all on the device."""
    from .. import _lib
    from ..hip_ops import scratch
    if sr.dim() != 4 or not sr.is_cuda or sr.shape[1] not in (1, 3):
        raise ValueError(f'niqe_device: expected an NCHW device tensor with 1 or 3 channels, got {tuple(sr.shape)} on {sr.device}')
    lib = _lib.load()
    sr = sr.contiguous().float()
    n, c, h, w = sr.shape
    if crop_border < 0 or h - 2 * crop_border < BLOCK or w - 2 * crop_border < BLOCK:
        raise ValueError(f'NIQE needs at least one {BLOCK}x{BLOCK} block after the border crop; the image is '
                         f'{h}x{w} with crop_border {crop_border}')
    yh, yw = (h - 2 * crop_border) // BLOCK * BLOCK, (w - 2 * crop_border) // BLOCK * BLOCK
    nb = (yh // BLOCK) * (yw // BLOCK)
    win = np.ascontiguousarray(window, np.float64)
    dev = sr.device
    y = torch.empty(n, yh, yw, dtype=torch.float32, device=dev)
    mom = torch.empty(2, n, nb, 5, 5, dtype=torch.float64, device=dev)
    mscn = [torch.empty(n, yh // s, yw // s, dtype=torch.float32, device=dev) for s in (1, 2)] if want_mscn else None
    wsb = lib.sr_niqe_workspace_bytes(n, yh, yw)
    ws = scratch(dev, wsb, tag='niqe')
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.sr_niqe_luma_f32(sr.data_ptr(), n, c, h, w, crop_border, y.data_ptr(), yh, yw, stream), 'sr_niqe_luma_f32')
        for s in (1, 2):
            _lib.check(lib.sr_niqe_moments_f32(y.data_ptr(), n, yh, yw, s, win.ctypes.data, mom[s - 1].data_ptr(),
                                               mscn[s - 1].data_ptr() if want_mscn else None, ws.data_ptr(), wsb, stream),
                       'sr_niqe_moments_f32')
    return y, mom, mscn


def niqe_device(sr, crop_border=0, pris_params=None, convert_to='y'):
    """NIQE per image of an NCHW tensor in [0, 1] on the HIP device (C = 3: RGB as the network produces it, C = 1: grey),
    with tensor2img's quantisation: the kernels produce the per-block moments, the host fits them (float64)."""
    _check_convert(convert_to)
    params = load_niqe_params(pris_params)
    _, mom, _ = _device_stages(sr, crop_border, params['gaussian_window'])
    mom = mom.cpu().numpy()
    return [_score_moments(mom[0, i], mom[1, i], params) for i in range(mom.shape[1])]
