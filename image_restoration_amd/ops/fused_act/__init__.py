"""Fused bias + LeakyReLU — the reference's ``basicsr/ops/fused_act`` on libsr_hip.so (include/sr_hip_stylegan2.h)."""
from .fused_act import FusedLeakyReLU, FusedLeakyReLUFunction, FusedLeakyReLUFunctionBackward, fused_leaky_relu

__all__ = ['FusedLeakyReLU', 'FusedLeakyReLUFunction', 'FusedLeakyReLUFunctionBackward', 'fused_leaky_relu']
