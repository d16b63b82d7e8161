"""RIDNet (real image denoising with feature attention) on the MI355X HIP path.

Same constructor, forward contract, state_dict keys, parameter order and initialisation as the reference
``basicsr/archs/ridnet_arch.py`` (PyTorch's default init everywhere, ``ResidualBlockNoBN`` at kaiming_normal * 0.1, the two
MeanShift layers at eye(3) / std and sign * img_range * mean / std), so ``network_g: {type: RIDNet, ...}`` option blocks and
checkpoints converted from the official release (which maps tensors by position) load with strict=True.  As in the reference,
the MeanShift weights and biases are ordinary trainable parameters: they are full 3x3 channel mixes plus a bias, not a fixed
per-channel affine, and they receive gradients.  The modules only hold parameters; the network is a composition of per-layer
launches (include/sr_hip_ridnet.h next to sr_hip.h):

    sub_mean                      sr_ridnet_sub_mean_f32 (NCHW -> CB8, 3x3 mix + bias)
    head, relu                    sr_conv3x3_f32 (act_slope 0)
    per EAM
      merge.dilation1             sr_conv3x3_f32, then sr_convd_f32 (dilation 2) into channels [0, mid) of one 2*mid CB8 buffer
      merge.dilation2             sr_convd_f32 (dilation 3), then sr_convd_f32 (dilation 4) into channels [mid, 2*mid)
      merge.aggregation, + x      sr_convd_f32 (dilation 1) with ReLU and res1 = the EAM input (training: also stores the ReLU
                                  output, whose mask the backward needs)
      block1, relu                sr_conv3x3_f32; sr_convd_f32 with post_act (relu(conv + x))
      block2                      sr_conv3x3_f32 twice; the 1x1 conv with post_act (relu(conv1x1 + x))
      ca                          sr_ca_squeeze_f32 (pool + mid -> mid/16 -> mid MLP), sr_ca_scale_f32 (x * s)
    tail                          sr_conv3x3_f32 (3 channels in one CB8 block)
    add_mean, + x                 sr_ridnet_add_mean_f32 (NCHW)

Training goes through one autograd function for the whole network (ridnet_autograd.py).  fp32 only.
"""
import torch
from torch import nn

from .. import hip_ops
from ..utils.registry import ARCH_REGISTRY
from .arch_util import Conv3x3Params, ResidualBlockNoBN, make_layer
from .hip_generator import HipGenerator
from .rcan_arch import ChannelAttentionParams


class MeanShiftParams(nn.Module):
    """The reference's MeanShift (ridnet_arch.py:8-29): a 3 -> 3 1x1 conv with weight eye(3) / std and bias
    sign * rgb_range * mean / std.  Its ``requires_grad`` attribute is a plain module attribute there, so the parameters train."""

    def __init__(self, rgb_range, rgb_mean, rgb_std, sign=-1):
        super().__init__()
        std = torch.tensor(rgb_std, dtype=torch.float32)
        self.weight = nn.Parameter(torch.eye(3).view(3, 3, 1, 1) / std.view(3, 1, 1, 1))
        self.bias = nn.Parameter(sign * rgb_range * torch.tensor(rgb_mean, dtype=torch.float32) / std)

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('MeanShiftParams is a parameter container; RIDNet launches the HIP kernels')


class MergeRunParams(nn.Module):
    """``dilation1`` (3x3, then 3x3 dilation 2), ``dilation2`` (3x3 dilation 3, then dilation 4), each conv + ReLU, and
    ``aggregation`` (3x3 over the concatenation, + ReLU) — ridnet_arch.py:60-84."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.dilation1 = nn.Sequential(Conv3x3Params(in_channels, out_channels), nn.ReLU(True),
                                       Conv3x3Params(out_channels, out_channels), nn.ReLU(True))
        self.dilation2 = nn.Sequential(Conv3x3Params(in_channels, out_channels), nn.ReLU(True),
                                       Conv3x3Params(out_channels, out_channels), nn.ReLU(True))
        self.aggregation = nn.Sequential(Conv3x3Params(out_channels * 2, out_channels), nn.ReLU(True))

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('MergeRunParams is a parameter container; RIDNet launches the HIP kernels')


class EResidualBlockParams(nn.Module):
    """``relu(body(x) + x)`` with body = 3x3, ReLU, 3x3, ReLU, 1x1 (ridnet_arch.py:32-57): keys ``body.{0,2,4}``."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.body = nn.Sequential(Conv3x3Params(in_channels, out_channels), nn.ReLU(True), Conv3x3Params(out_channels, out_channels),
                                  nn.ReLU(True), Conv3x3Params(out_channels, out_channels, ksize=1))

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('EResidualBlockParams is a parameter container; RIDNet launches the HIP kernels')


class EAMParams(nn.Module):
    """merge, block1 (ResidualBlockNoBN, then ReLU), block2, ca (ridnet_arch.py:108-135)."""

    def __init__(self, in_channels, mid_channels, out_channels):
        super().__init__()
        self.merge = MergeRunParams(in_channels, mid_channels)
        self.block1 = ResidualBlockNoBN(mid_channels)
        self.block2 = EResidualBlockParams(mid_channels, out_channels)
        self.ca = ChannelAttentionParams(out_channels)

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('EAMParams is a parameter container; RIDNet launches the HIP kernels')


@ARCH_REGISTRY.register()
class RIDNet(HipGenerator):
    """RIDNet(in_channels, mid_channels, out_channels, num_block=4, img_range=255., rgb_mean=(0.4488, 0.4371, 0.4040),
    rgb_std=(1.0, 1.0, 1.0)).

    forward(x [N, 3, H, W] fp32 on a HIP device) -> [N, 3, H, W].  As in the reference the input is NOT rescaled: inputs in
    [0, 1] minus 255 * mean give features in the hundreds.  ValueError for: ``in_channels`` or ``out_channels`` other than 3
    (the MeanShift layers are 3-channel); ``mid_channels`` not a positive multiple of 8 (CB8 activations), below 16 (the
    attention squeezes by 16) or above 512; ``num_block`` below 1; ``compute_dtype`` other than fp32.
    """

    def __init__(self, in_channels, mid_channels, out_channels, num_block=4, img_range=255., rgb_mean=(0.4488, 0.4371, 0.4040),
                 rgb_std=(1.0, 1.0, 1.0), compute_dtype='fp32'):
        super().__init__()
        if compute_dtype not in ('fp32', 'float32', None):
            raise ValueError(f'RIDNet runs in fp32 only, got compute_dtype={compute_dtype!r}')
        if in_channels != 3 or out_channels != 3:
            raise ValueError(f'RIDNet\'s MeanShift layers are 3-channel: in_channels and out_channels must be 3, got '
                             f'{in_channels}, {out_channels}')
        if not isinstance(mid_channels, int) or mid_channels < 16 or mid_channels % 8 or mid_channels > 512:
            raise ValueError(f'RIDNet needs mid_channels to be a multiple of 8 in [16, 512] (CB8 activations, attention squeeze 16), '
                             f'got {mid_channels!r}')
        if not isinstance(num_block, int) or num_block < 1:
            raise ValueError(f'RIDNet needs num_block >= 1, got {num_block!r}')
        if len(rgb_mean) != 3 or len(rgb_std) != 3:
            raise ValueError(f'rgb_mean and rgb_std must hold 3 values, got {rgb_mean!r}, {rgb_std!r}')
        self.in_channels, self.mid_channels, self.out_channels, self.num_block = in_channels, mid_channels, out_channels, num_block
        self.img_range = float(img_range)

        self.sub_mean = MeanShiftParams(img_range, rgb_mean, rgb_std, -1)
        self.add_mean = MeanShiftParams(img_range, rgb_mean, rgb_std, 1)
        self.head = Conv3x3Params(in_channels, mid_channels)
        self.body = make_layer(EAMParams, num_block, in_channels=mid_channels, mid_channels=mid_channels, out_channels=mid_channels)
        self.tail = Conv3x3Params(mid_channels, out_channels)

    # ------------------------------------------------------------------ HIP plumbing
    _in_channels = property(lambda self: self.in_channels)

    def _autograd_apply(self, x):
        from .ridnet_autograd import ridnet_apply
        return ridnet_apply(self, x)

    def run_forward(self, x, keep=False):
        """The forward as per-layer launches on the current stream.  ``keep``: also return what the backward reads (the input,
        the sub_mean output, the head output, per EAM its input and every intermediate activation, the tail output)."""
        mid = self.mid_channels
        dev = x.device
        n, _, h, w = x.shape
        with torch.cuda.device(dev):
            s = hip_ops.ridnet_sub_mean(x, self.sub_mean.weight, self.sub_mean.bias)
            feat = hip_ops.conv3x3(s, self.packed(self.head), act_slope=0.0)
            saved = dict(x=x, s=s, head=feat, eams=[]) if keep else None
            for eam in self.body:
                mg, b1p, b2p, ca = eam.merge, eam.block1, eam.block2, eam.ca
                f_in = feat
                cat = hip_ops.CB8.empty(n, 2 * mid, h, w, dev)
                d1a = hip_ops.conv3x3(f_in, self.packed(mg.dilation1[0]), act_slope=0.0)
                hip_ops.convd(d1a, self.packed(mg.dilation1[2]), 2, out=cat.slice(0, mid), act_slope=0.0)
                d2a = hip_ops.convd(f_in, self.packed(mg.dilation2[0]), 3, act_slope=0.0)
                hip_ops.convd(d2a, self.packed(mg.dilation2[2]), 4, out=cat.slice(mid, mid), act_slope=0.0)
                agg = hip_ops.CB8.empty(n, mid, h, w, dev) if keep else None
                m = hip_ops.convd(cat, self.packed(mg.aggregation[0]), 1, act_slope=0.0, res1=f_in, beta1=1.0, out_pre=agg)
                t = hip_ops.conv3x3(m, self.packed(b1p.conv1), act_slope=0.0)
                b1 = hip_ops.convd(t, self.packed(b1p.conv2), 1, post_act=True, act_slope=0.0, res1=m, beta1=1.0)
                u1 = hip_ops.conv3x3(b1, self.packed(b2p.body[0]), act_slope=0.0)
                u2 = hip_ops.conv3x3(u1, self.packed(b2p.body[2]), act_slope=0.0)
                b2 = hip_ops.convd(u2, self.packed(b2p.body[4]), 1, post_act=True, act_slope=0.0, res1=b1, beta1=1.0)
                p, hb, sv = hip_ops.ca_squeeze(b2, ca.fc1.weight, ca.fc1.bias, ca.fc2.weight, ca.fc2.bias)
                feat = hip_ops.ca_scale(b2, sv)
                if keep:
                    saved['eams'].append(dict(f_in=f_in, d1a=d1a, d2a=d2a, cat=cat, agg=agg, m=m, t=t, b1=b1, u1=u1, u2=u2, b2=b2,
                                              p=p, hb=hb, s=sv))
                del cat, d1a, d2a, m, t, u1, u2
            tail = hip_ops.conv3x3(feat, self.packed(self.tail))
            if keep:
                saved['feat'] = feat
                saved['tail'] = tail
            y = hip_ops.ridnet_add_mean(x, tail, self.add_mean.weight, self.add_mean.bias)
        return y, saved
