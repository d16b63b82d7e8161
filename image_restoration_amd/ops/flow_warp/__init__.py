"""Warping by optical flow — the reference's ``flow_warp`` (basicsr/archs/arch_util.py:112-143) on libsr_hip.so
(include/sr_hip_flow.h)."""
from .flow_warp import FlowWarp, flow_warp, flow_warp_native

__all__ = ['FlowWarp', 'flow_warp', 'flow_warp_native']
