"""Modulated deformable convolution (DCNv2) — the reference's ``basicsr/ops/dcn`` on libsr_hip.so (include/sr_hip_dcn.h).
Only the modulated (v2) operator is provided: nothing in the reference calls DeformConv / DeformConvPack (v1)."""
from .deform_conv import ModulatedDeformConv, ModulatedDeformConvPack, modulated_deform_conv

__all__ = ['ModulatedDeformConv', 'ModulatedDeformConvPack', 'modulated_deform_conv']
