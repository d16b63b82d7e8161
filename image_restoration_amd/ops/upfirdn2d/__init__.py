"""Up-sample, FIR filter, down-sample — the reference's ``basicsr/ops/upfirdn2d`` on libsr_hip.so (include/sr_hip_stylegan2.h)."""
from .upfirdn2d import UpFirDn2d, UpFirDn2dBackward, upfirdn2d, upfirdn2d_native

__all__ = ['UpFirDn2d', 'UpFirDn2dBackward', 'upfirdn2d', 'upfirdn2d_native']
