"""Validation metrics of the path: PSNR and SSIM on uint8-rounded images, and the no-reference NIQE;
host (numpy) and device (HIP)."""
from .psnr import calculate_psnr, calculate_ssim, psnr_device, ssim_device  # noqa: F401
from .niqe import calculate_niqe, load_niqe_params, niqe_device  # noqa: F401
