"""Host side of the blur: the kernel generators of the reference (basicsr/data/degradations.py:19-351) and ``draw_blur_kernel``,
which draws what ``random_mixed_kernels`` (:419-522) draws but returns the kernel instead of filtering an image with it — the
filtering is sr_filter2d_f32's (include/sr_hip_degrade.h).

The generators are float64 closed forms with the reference's signatures.  ``draw_blur_kernel`` consumes ``random`` and
``numpy.random`` in the reference's order, so a seeded run draws the same kernels.  Only the kinds that are one linear kernel are
supported; the others need cv2, PIL or pyblur on uint8 images and raise ValueError.
"""
import math
import random

import numpy as np

LINEAR_KINDS = ('iso', 'aniso', 'generalized_iso', 'generalized_aniso', 'plateau_iso', 'plateau_aniso', 'motion', 'average')
UNSUPPORTED_KINDS = ('median', 'bilateral', 'pyblur', 'pyblur_motion', 'random_cover', 'bicubic')


def sigma_matrix2(sig_x, sig_y, theta):
    """The rotated covariance matrix U diag(sig_x^2, sig_y^2) U^T."""
    d = np.array([[sig_x ** 2, 0], [0, sig_y ** 2]])
    u = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    return np.dot(u, np.dot(d, u.T))


def mesh_grid(kernel_size):
    """(xy [K, K, 2], xx [K, K], yy [K, K]) centred at zero."""
    ax = np.arange(-kernel_size // 2 + 1., kernel_size // 2 + 1.)
    xx, yy = np.meshgrid(ax, ax)
    xy = np.stack([xx, yy], axis=2)
    return xy, xx, yy


def _quadratic_form(sigma_matrix, grid):
    return np.sum(np.dot(grid, np.linalg.inv(sigma_matrix)) * grid, 2)


def pdf2(sigma_matrix, grid):
    """The un-normalised bivariate Gaussian density on the grid."""
    return np.exp(-0.5 * _quadratic_form(sigma_matrix, grid))


def _sigma(sig_x, sig_y, theta, isotropic):
    return np.array([[sig_x ** 2, 0], [0, sig_x ** 2]]) if isotropic else sigma_matrix2(sig_x, sig_y, theta)


def bivariate_Gaussian(kernel_size, sig_x, sig_y, theta, grid=None, isotropic=True):
    if grid is None:
        grid, _, _ = mesh_grid(kernel_size)
    kernel = pdf2(_sigma(sig_x, sig_y, theta, isotropic), grid)
    return kernel / np.sum(kernel)


def bivariate_generalized_Gaussian(kernel_size, sig_x, sig_y, theta, beta, grid=None, isotropic=True):
    if grid is None:
        grid, _, _ = mesh_grid(kernel_size)
    kernel = np.exp(-0.5 * np.power(_quadratic_form(_sigma(sig_x, sig_y, theta, isotropic), grid), beta))
    return kernel / np.sum(kernel)


def bivariate_plateau(kernel_size, sig_x, sig_y, theta, beta, grid=None, isotropic=True):
    if grid is None:
        grid, _, _ = mesh_grid(kernel_size)
    kernel = np.reciprocal(np.power(_quadratic_form(_sigma(sig_x, sig_y, theta, isotropic), grid), beta) + 1)
    return kernel / np.sum(kernel)


def _draw_sigmas(kernel_size, sigma_x_range, sigma_y_range, rotation_range, isotropic):
    assert kernel_size % 2 == 1, 'Kernel size must be an odd number.'
    assert sigma_x_range[0] < sigma_x_range[1], 'Wrong sigma_x_range.'
    sigma_x = np.random.uniform(sigma_x_range[0], sigma_x_range[1])
    if isotropic is False:
        assert sigma_y_range[0] < sigma_y_range[1], 'Wrong sigma_y_range.'
        assert rotation_range[0] < rotation_range[1], 'Wrong rotation_range.'
        sigma_y = np.random.uniform(sigma_y_range[0], sigma_y_range[1])
        rotation = np.random.uniform(rotation_range[0], rotation_range[1])
    else:
        sigma_y, rotation = sigma_x, 0
    return sigma_x, sigma_y, rotation


def _draw_beta(beta_range):
    if np.random.uniform() < 0.5:
        return np.random.uniform(beta_range[0], 1)
    return np.random.uniform(1, beta_range[1])


def _kernel_noise(kernel, noise_range):
    if noise_range is not None:
        assert noise_range[0] < noise_range[1], 'Wrong noise range.'
        kernel = kernel * np.random.uniform(noise_range[0], noise_range[1], size=kernel.shape)
    return kernel / np.sum(kernel)


def random_bivariate_Gaussian(kernel_size, sigma_x_range, sigma_y_range, rotation_range, noise_range=None, isotropic=True):
    sx, sy, rot = _draw_sigmas(kernel_size, sigma_x_range, sigma_y_range, rotation_range, isotropic)
    return _kernel_noise(bivariate_Gaussian(kernel_size, sx, sy, rot, isotropic=isotropic), noise_range)


def random_bivariate_generalized_Gaussian(kernel_size, sigma_x_range, sigma_y_range, rotation_range, beta_range, noise_range=None,
                                          isotropic=True):
    sx, sy, rot = _draw_sigmas(kernel_size, sigma_x_range, sigma_y_range, rotation_range, isotropic)
    beta = _draw_beta(beta_range)
    return _kernel_noise(bivariate_generalized_Gaussian(kernel_size, sx, sy, rot, beta, isotropic=isotropic), noise_range)


def random_bivariate_plateau(kernel_size, sigma_x_range, sigma_y_range, rotation_range, beta_range, noise_range=None, isotropic=True):
    sx, sy, rot = _draw_sigmas(kernel_size, sigma_x_range, sigma_y_range, rotation_range, isotropic)
    beta = _draw_beta(beta_range)
    return _kernel_noise(bivariate_plateau(kernel_size, sx, sy, rot, beta, isotropic=isotropic), noise_range)


def motion_kernel(kernel_size):
    """A horizontal or vertical line of 1 / kernel_size through the centre (one ``random.random()``)."""
    kernel = np.zeros((kernel_size, kernel_size))
    if random.random() > 0.5:
        kernel[(kernel_size - 1) // 2, :] = 1.0
    else:
        kernel[:, (kernel_size - 1) // 2] = 1.0
    return kernel / kernel_size


def average_kernel(kernel_size):
    return np.ones((kernel_size, kernel_size), np.float32) / (kernel_size * kernel_size)


def pad_kernel_to(kernel, size):
    """Zero border up to ``size`` x ``size``: the same filter."""
    pad = (size - kernel.shape[0]) // 2
    if pad < 0 or (size - kernel.shape[0]) % 2:
        raise ValueError(f'a {kernel.shape[0]}x{kernel.shape[0]} kernel cannot be centred in {size}x{size}')
    return np.pad(kernel, ((pad, pad), (pad, pad)))


def draw_blur_kernel(kernel_list, kernel_prob, kernel_size=21, sigma_x_range=(0.6, 5), sigma_y_range=(0.6, 5),
                     rotation_range=(-math.pi, math.pi), betag_range=(0.5, 8), betap_range=(0.5, 8), noise_range=None,
                     pad_to=None):
    """The kernel ``random_mixed_kernels`` would filter with: float32 [k, k] (k = ``pad_to`` when given, else ``kernel_size``)."""
    kind = random.choices(kernel_list, kernel_prob)[0]
    if kind in ('iso', 'aniso'):
        kernel = random_bivariate_Gaussian(kernel_size, sigma_x_range, sigma_y_range, rotation_range, noise_range=noise_range,
                                           isotropic=kind == 'iso')
    elif kind in ('generalized_iso', 'generalized_aniso'):
        kernel = random_bivariate_generalized_Gaussian(kernel_size, sigma_x_range, sigma_y_range, rotation_range, betag_range,
                                                       noise_range=noise_range, isotropic=kind == 'generalized_iso')
    elif kind in ('plateau_iso', 'plateau_aniso'):
        kernel = random_bivariate_plateau(kernel_size, sigma_x_range, sigma_y_range, rotation_range, betap_range, noise_range=None,
                                          isotropic=kind == 'plateau_iso')
    elif kind == 'motion':
        kernel = motion_kernel(kernel_size)
    elif kind == 'average':
        kernel = average_kernel(kernel_size)
    else:
        raise ValueError(f"blur kind '{kind}' is not one linear kernel (it needs cv2, PIL or pyblur on uint8 images); "
                         f'supported: {", ".join(LINEAR_KINDS)}')
    if pad_to is not None:
        kernel = pad_kernel_to(kernel, pad_to)
    return np.ascontiguousarray(kernel, dtype=np.float32)


def check_kernel_list(kernel_list):
    bad = [k for k in kernel_list if k not in LINEAR_KINDS]
    if bad:
        raise ValueError(f"blur kind '{bad[0]}' is not one linear kernel (it needs cv2, PIL or pyblur on uint8 images); "
                         f'supported: {", ".join(LINEAR_KINDS)}')
