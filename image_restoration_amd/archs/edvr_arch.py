"""PCD alignment of EDVR (reference basicsr/archs/edvr_arch.py:9-98) on libsr_hip.so.  EDVR itself is not here yet (it needs a
stride-2 3x3 conv, TSA's pooling and sigmoid kernels and the frame loop); like the reference, PCDAlignment is not registered
in ARCH_REGISTRY."""
import torch
from torch import nn

from .. import hip_autograd as A
from .arch_util import Conv3x3Params, DCNv2Pack


class PCDAlignment(nn.Module):
    """Alignment module using Pyramid, Cascading and Deformable convolution (PCD).

    ``forward(nbr_feat_l, ref_feat_l)`` takes the two three-level pyramids (L1, L2, L3; each [b, c, h, w], NCHW fp32 on the GPU)
    and returns the aligned L1 features as NCHW.  Inside, everything is CB8: the inputs are converted once at entry, the result
    once at exit, and every layer is an autograd Function of hip_autograd (3x3 convs with LeakyReLU 0.1 in their epilogue,
    bilinear x2 with align_corners=False, DCNFn).  Channel concatenation and the ``* 2`` of the upsampled offsets are tensor
    plumbing on the CB8 storage (torch.cat along the block dimension, one scaling).

    Args:
        num_feat (int): Channel number of middle features (a multiple of 8 * deformable_groups). Default: 64.
        deformable_groups (int): Deformable groups. Defaults: 8.
    """

    def __init__(self, num_feat=64, deformable_groups=8):
        super().__init__()
        # Pyramid has three levels: L3 (1/4 size), L2 (1/2 size), L1 (original size)
        self.offset_conv1 = nn.ModuleDict()
        self.offset_conv2 = nn.ModuleDict()
        self.offset_conv3 = nn.ModuleDict()
        self.dcn_pack = nn.ModuleDict()
        self.feat_conv = nn.ModuleDict()
        for i in range(3, 0, -1):
            level = f'l{i}'
            self.offset_conv1[level] = Conv3x3Params(num_feat * 2, num_feat)
            if i == 3:
                self.offset_conv2[level] = Conv3x3Params(num_feat, num_feat)
            else:
                self.offset_conv2[level] = Conv3x3Params(num_feat * 2, num_feat)
                self.offset_conv3[level] = Conv3x3Params(num_feat, num_feat)
            self.dcn_pack[level] = DCNv2Pack(num_feat, num_feat, 3, padding=1, deformable_groups=deformable_groups)
            if i < 3:
                self.feat_conv[level] = Conv3x3Params(num_feat * 2, num_feat)
        # Cascading dcn
        self.cas_offset_conv1 = Conv3x3Params(num_feat * 2, num_feat)
        self.cas_offset_conv2 = Conv3x3Params(num_feat, num_feat)
        self.cas_dcnpack = DCNv2Pack(num_feat, num_feat, 3, padding=1, deformable_groups=deformable_groups)
        self.num_feat = num_feat

    @staticmethod
    def _conv(m, x, slope=0.1):
        return A.ConvFn.apply(x, m.weight, m.bias, slope)

    def forward(self, nbr_feat_l, ref_feat_l):
        for t in list(nbr_feat_l) + list(ref_feat_l):
            if not t.is_cuda:
                raise NotImplementedError
        nbr = [A.ToCB8.apply(t) for t in nbr_feat_l]
        ref = [A.ToCB8.apply(t) for t in ref_feat_l]
        conv = self._conv
        upsampled_offset, upsampled_feat = None, None
        for i in range(3, 0, -1):
            level = f'l{i}'
            offset = conv(self.offset_conv1[level], torch.cat([nbr[i - 1], ref[i - 1]], dim=1))
            if i == 3:
                offset = conv(self.offset_conv2[level], offset)
            else:
                offset = conv(self.offset_conv2[level], torch.cat([offset, upsampled_offset], dim=1))
                offset = conv(self.offset_conv3[level], offset)
            if i < 3:
                feat = self.dcn_pack[level].forward_cb8(nbr[i - 1], offset)
                # LeakyReLU on level 2 only: the level-1 feat_conv output goes on without activation
                feat = conv(self.feat_conv[level], torch.cat([feat, upsampled_feat], dim=1), 0.1 if i > 1 else 1.0)
            else:
                feat = self.dcn_pack[level].forward_cb8(nbr[i - 1], offset, 0.1)
            if i > 1:  # upsample offset and features; x2: an upsampled offset is also twice as long
                upsampled_offset = A.Bilinear2xFn.apply(offset) * 2
                upsampled_feat = A.Bilinear2xFn.apply(feat)
        # Cascading
        offset = conv(self.cas_offset_conv2, conv(self.cas_offset_conv1, torch.cat([feat, ref[0]], dim=1)))
        feat = self.cas_dcnpack.forward_cb8(feat, offset, 0.1)
        return A.FromCB8.apply(feat, self.num_feat)
