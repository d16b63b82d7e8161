"""NIQE on the host (metrics/niqe.py) against the reference's own run (tests/golden/g_t_niqe.npz, tools/make_golden_niqe.py).

Contract (module docstring of metrics/niqe.py): Y and MSCN bit for bit; alpha identical except where the reference's
float32 rhatnorm and ours straddle the midpoint of two adjacent grid points; the other features and the score within the
bounds derived below.

Feature bound.  The reference forms each side's mean of b^2 and the mean of |b| as float32 pairwise sums of at most 96^2
terms: relative error <= ~log2(9216) * 2^-24 ~ 8e-7 in the worst case, ~1e-7 typically; ours are float64.  beta = sqrt(mean)
* const halves that (<= 4e-7); the mean feature (beta_r - beta_l) * G(2/a)/G(1/a) is a difference and can lose digits
where beta_r ~ beta_l, so it is bounded against the scale of its terms, max(|beta_l|, |beta_r|).  With slack for the
float32 rounding of the reference's squares (2^-24 each): 2e-6 relative to the term scale.

Score bound.  A one-grid-step alpha flip moves one block's feature by 1e-3 out of ~1 (the rest move by <= 2e-6); the
score is a smooth function of the mean and covariance of >= 2 blocks, so its relative change stays within a small multiple
of the feature changes divided by the block count.  We assert 1e-4 relative.  Measured: ~1e-7 on the small cases (no
alpha flip), 1.6e-5 on the large case, where two of its 30 blocks flip alpha by one grid step.
"""
import hashlib
import os

import numpy as np
import pytest

from image_restoration_amd import _lib
from image_restoration_amd.metrics import calculate_niqe, load_niqe_params
from image_restoration_amd.metrics import niqe as N
from image_restoration_amd.utils import synth
from image_restoration_amd.utils.registry import METRIC_REGISTRY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'g_t_niqe.npz')
ALPHA_COLS = [0, 2, 6, 10, 14]
ALPHA_COLS = ALPHA_COLS + [18 + c for c in ALPHA_COLS]
FEATURE_RTOL = 2e-6
SCORE_RTOL = 1e-4


@pytest.fixture(scope='module')
def g():
    return dict(np.load(FIXTURE))


def case_image(g, name):
    """The case's uint8 BGR image: stored, or (large case) regenerated from its seed and checked against the stored SHA-256."""
    if f'{name}/img' in g:
        return g[f'{name}/img']
    h, w = (int(v) for v in g[f'{name}/shape'])
    img = synth.niqe_image(int(g[f'{name}/seed']), h, w)
    assert hashlib.sha256(img.tobytes()).hexdigest() == str(g[f'{name}/sha256']), f'{name}: regenerated image differs from the fixture'
    return img


def check_features(feat, ref, rh_ours, rh_ref):
    """The feature contract of this module's docstring; feat / ref [nb, 36], rh_* [nb, 10] (scale 1 fields, scale 2 fields)."""
    assert feat.shape == ref.shape
    np.testing.assert_array_equal(np.isnan(feat), np.isnan(ref))
    gam_step = 1e-3
    for j, col in enumerate(ALPHA_COLS):
        diff = np.nonzero(feat[:, col] != ref[:, col])[0]
        for b in diff:  # a flip: adjacent grid points, and the midpoint of their r_gam lies between the two rhatnorm values
            ia, ib = (int(round((v - 0.2) / gam_step)) for v in (feat[b, col], ref[b, col]))
            assert abs(ia - ib) == 1, (b, col, feat[b, col], ref[b, col])
            mid = (N._R_GAM[ia] + N._R_GAM[ib]) / 2
            lo, hi = sorted((float(rh_ours[b, j]), float(rh_ref[b, j])))
            assert lo <= mid <= hi, (b, col, lo, mid, hi)
    flipped = np.zeros(feat.shape[0], bool)
    for col in ALPHA_COLS:
        flipped |= feat[:, col] != ref[:, col]
    for s in range(2):
        o = 18 * s
        groups = [[o + 1]] + [[o + 3 + 4 * f, o + 4 + 4 * f, o + 5 + 4 * f] for f in range(4)]
        for grp in groups:  # mean, beta_l, beta_r of one field; scale: the field's betas
            scale = np.nanmax(np.abs(ref[:, grp]), axis=1, keepdims=True)
            ok = ~flipped[:, None] & ~np.isnan(ref[:, grp])
            err = np.abs(feat[:, grp] - ref[:, grp]) / scale
            assert np.all(err[ok] <= FEATURE_RTOL), (grp, float(err[ok].max()))


def test_fixture_window_is_bit_symmetric_and_grid_is_increasing(g):
    w = g['gaussian_window']
    assert w.shape == (7, 7)
    np.testing.assert_array_equal(w, w[::-1, :])
    np.testing.assert_array_equal(w, w[:, ::-1])
    np.testing.assert_array_equal(w, w.T)
    assert len(N._GAM) == 9801 and N._GAM[0] == 0.2 and abs(N._GAM[-1] - 10.0) < 1e-9
    step = np.diff(N._R_GAM)
    assert np.all(step > 0)
    assert step.min() > 1e-6  # ~1.67e-6 at the alpha = 10 end: far above the float64 error of r_gam


def test_alpha_index_is_argmin_of_squared_distance():
    rng = np.random.default_rng(0)
    rn = np.concatenate([rng.uniform(N._R_GAM[0] - 0.05, N._R_GAM[-1] + 0.05, 4000), N._R_GAM[::97],
                         (N._R_GAM[:-1:89] + N._R_GAM[1::89]) / 2, [np.nan]])
    with np.errstate(invalid='ignore'):
        want = np.array([np.argmin((N._R_GAM - v)**2) for v in rn])
    np.testing.assert_array_equal(N._alpha_index(rn), want)
    assert N._alpha_index(np.array([np.nan]))[0] == 0


@pytest.mark.parametrize('name', ['small0', 'small4', 'tall4', 'flat'])
def test_luma_and_mscn_are_bit_exact(g, name):
    y = N._luma(g[f'{name}/img'], int(g[f'{name}/crop']), 'HWC')
    np.testing.assert_array_equal(y, g[f'{name}/y'])
    m1, m2, _, _ = N._host_stages(y, g['gaussian_window'])
    assert m1.dtype == np.float32 and m2.dtype == np.float32
    np.testing.assert_array_equal(m1, g[f'{name}/mscn1'])
    np.testing.assert_array_equal(m2, g[f'{name}/mscn2'])


@pytest.mark.parametrize('name', ['small0', 'small4', 'tall4', 'large'])
def test_features_and_score_match_reference(g, name):
    img, crop = case_image(g, name), int(g[f'{name}/crop'])
    y = N._luma(img, crop, 'HWC')
    _, _, mom1, mom2 = N._host_stages(y, g['gaussian_window'])
    f1, r1 = N._features(mom1, 96)
    f2, r2 = N._features(mom2, 48)
    rh_ref = np.concatenate([g[f'{name}/rhatnorm1'], g[f'{name}/rhatnorm2']], axis=1).astype(np.float64)
    check_features(np.concatenate([f1, f2], axis=1), g[f'{name}/feat'], np.concatenate([r1, r2], axis=1), rh_ref)
    score = calculate_niqe(img, crop, pris_params=FIXTURE)
    ref = float(g[f'{name}/score'])
    assert abs(score - ref) <= SCORE_RTOL * ref, (score, ref)
    # same through the registry, with the image in CHW order
    assert METRIC_REGISTRY.get('calculate_niqe')(img.transpose(2, 0, 1), crop, input_order='CHW', pris_params=FIXTURE) == score


def test_flat_patch_gives_nan_betas_and_alpha_0_2(g):
    """A block with no negative or no positive value has NaN betas and alpha 0.2 (argmin of an all-NaN array is 0); the
    reference then fails in pinv, this module raises ValueError naming the minimum."""
    feat = g['flat/feat']
    want = np.full(18, np.nan)
    want[[0, 2, 6, 10, 14]] = 0.2
    for row in feat:
        np.testing.assert_array_equal(row, np.concatenate([want, want]))
    assert str(g['flat/err']) == 'LinAlgError' and np.isnan(g['flat/score'])
    y = N._luma(g['flat/img'], 0, 'HWC')
    _, _, mom1, mom2 = N._host_stages(y, g['gaussian_window'])
    f1, _ = N._features(mom1, 96)
    f2, _ = N._features(mom2, 48)
    np.testing.assert_array_equal(np.concatenate([f1, f2], axis=1), feat)
    with pytest.raises(ValueError, match='at least 2 blocks'):
        calculate_niqe(g['flat/img'], 0, pris_params=FIXTURE)


def test_nan_quirk_on_one_sided_moments():
    # field with positives only: beta_l NaN, alpha 0.2, beta_r finite; all-zero field: everything but alpha NaN
    mom = np.zeros((1, 5, 5))
    mom[0, :, 2], mom[0, :, 3], mom[0, :, 4] = 10, 4.0, 6.0
    mom[0, 1] = 0
    f, rn = N._features(mom, 96)
    assert np.isnan(rn).all()
    assert f[0, 0] == 0.2 and np.isnan(f[0, 1])
    assert f[0, 2] == 0.2 and np.isnan(f[0, 3:6]).all()
    assert f[0, 6] == 0.2 and np.isnan(f[0, 7]) and np.isnan(f[0, 8]) and np.isfinite(f[0, 9])


def test_errors():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (150, 250, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match='niqe_pris_params.npz'):
        calculate_niqe(img, 0)
    with pytest.raises(FileNotFoundError, match='niqe_pris_params.npz'):
        calculate_niqe(img, 0, pris_params=os.path.join(ROOT, 'no_such_niqe_pris_params.npz'))
    with pytest.raises(ValueError, match="'gray'"):
        calculate_niqe(img, 0, convert_to='gray', pris_params=FIXTURE)
    with pytest.raises(ValueError, match='at least one 96x96 block'):
        calculate_niqe(img[:95], 0, pris_params=FIXTURE)
    with pytest.raises(ValueError, match='at least one 96x96 block'):
        calculate_niqe(img[:100], 4, pris_params=FIXTURE)
    with pytest.raises(ValueError, match='at least 2 blocks'):  # one block: the reference fails in pinv
        calculate_niqe(img[:96, :96], 0, pris_params=FIXTURE)
    # two blocks of noise are enough
    assert np.isfinite(calculate_niqe(img[:96, :192], 0, pris_params=FIXTURE))


def test_params_cache_and_grey_input(g):
    p = load_niqe_params(FIXTURE)
    assert load_niqe_params(FIXTURE) is p
    assert p['mu_pris_param'].shape == (1, 36) and p['cov_pris_param'].shape == (36, 36)
    # a grey image: HW is used as is, HWC with one channel goes through to_y_channel's /255*255 (exact on integers)
    grey = g['small0/img'][..., 1]
    s_hw = calculate_niqe(grey, 0, input_order='HW', pris_params=p)
    assert s_hw == calculate_niqe(grey[..., None], 0, input_order='HWC', pris_params=p)
    assert np.isfinite(s_hw)


def test_device_entry_points_are_exported_and_check_arguments():
    lib = _lib.load()

    def failed(rc, word):
        return rc < 0 and word in lib.sr_last_error().decode()
    assert lib.sr_niqe_workspace_bytes(2, 192, 288) == 2 * 96 * 144 * 4
    assert lib.sr_niqe_workspace_bytes(0, 192, 288) == 0
    assert failed(lib.sr_niqe_luma_f32(None, 1, 3, 200, 300, 0, 256, 192, 288, None), 'bad argument')
    assert failed(lib.sr_niqe_luma_f32(256, 1, 2, 200, 300, 0, 256, 192, 288, None), 'bad argument')
    assert failed(lib.sr_niqe_luma_f32(256, 1, 3, 200, 300, 0, 256, 190, 288, None), 'multiples of 96')
    assert failed(lib.sr_niqe_luma_f32(256, 1, 3, 200, 300, 5, 256, 192, 288, None), 'multiples of 96')
    w = np.zeros(49)
    assert failed(lib.sr_niqe_moments_f32(256, 1, 192, 288, 3, w.ctypes.data, 256, None, 256, 1 << 20, None), 'bad argument')
    assert failed(lib.sr_niqe_moments_f32(256, 1, 192, 288, 1, None, 256, None, 256, 1 << 20, None), 'bad argument')
    assert failed(lib.sr_niqe_moments_f32(256, 1, 200, 288, 1, w.ctypes.data, 256, None, None, 0, None), 'multiples of 96')
    assert failed(lib.sr_niqe_moments_f32(256, 1, 192, 288, 2, w.ctypes.data, 256, None, 256, 100, None), 'workspace')
