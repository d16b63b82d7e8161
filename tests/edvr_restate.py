"""A restatement of the reference's TSAFusion, PredeblurModule and EDVR (basicsr/archs/edvr_arch.py:101-383) on plain
torch.nn.functional, differentiable by torch autograd, in the dtype of its inputs: float64 as the yardstick of the whole-network
tests, float32 on the CPU to measure what single precision alone costs.  Written in this project's own words from the
semantics of the reference's modules, on a state dict of tensors with the reference's keys; PCD alignment and the deformable
convolution come from tests/dcn_restate.py.
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_restate as R  # noqa: E402


def _conv(sd, name, t, stride=1, padding=1):
    return F.conv2d(t, sd[name + '.weight'], sd[name + '.bias'], stride=stride, padding=padding)


def _conv1(sd, name, t):
    return _conv(sd, name, t, padding=0)


def _lrelu(t):
    return F.leaky_relu(t, 0.1)


def _up(t):
    return F.interpolate(t, scale_factor=2, mode='bilinear', align_corners=False)


def _resblock(sd, name, t):
    return t + _conv(sd, name + '.conv2', F.relu(_conv(sd, name + '.conv1', t)))


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def _pools(t):
    return torch.cat([F.max_pool2d(t, 3, 2, 1), F.avg_pool2d(t, 3, 2, 1)], dim=1)


def tsa_fusion(sd, aligned, center, corr_out=None):
    """TSAFusion.forward on (b, t, c, h, w).  ``corr_out``: a list that receives the pre-sigmoid correlations (b, t, h, w)."""
    b, t, c, h, w = aligned.shape
    emb_ref = _conv(sd, 'temporal_attn1', aligned[:, center])
    emb = _conv(sd, 'temporal_attn2', aligned.reshape(b * t, c, h, w)).view(b, t, -1, h, w)
    corr = (emb * emb_ref.unsqueeze(1)).sum(2)                       # (b, t, h, w)
    if corr_out is not None:
        corr_out.append(corr.detach())
    fused = (aligned * torch.sigmoid(corr).unsqueeze(2)).reshape(b, t * c, h, w)
    feat = _lrelu(_conv1(sd, 'feat_fusion', fused))
    attn = _lrelu(_conv1(sd, 'spatial_attn1', fused))
    attn = _lrelu(_conv1(sd, 'spatial_attn2', _pools(attn)))
    level = _lrelu(_conv1(sd, 'spatial_attn_l1', attn))
    level = _lrelu(_conv(sd, 'spatial_attn_l2', _pools(level)))
    level = _up(_lrelu(_conv(sd, 'spatial_attn_l3', level)))
    attn = _lrelu(_conv(sd, 'spatial_attn3', attn)) + level
    attn = _up(_lrelu(_conv1(sd, 'spatial_attn4', attn)))
    attn = _conv(sd, 'spatial_attn5', attn)
    attn_add = _conv1(sd, 'spatial_attn_add2', _lrelu(_conv1(sd, 'spatial_attn_add1', attn)))
    return feat * torch.sigmoid(attn) * 2 + attn_add


def predeblur(sd, x, hr_in):
    """PredeblurModule.forward on (n, c, h, w)."""
    l1 = _lrelu(_conv(sd, 'conv_first', x))
    if hr_in:
        l1 = _lrelu(_conv(sd, 'stride_conv_hr1', l1, stride=2))
        l1 = _lrelu(_conv(sd, 'stride_conv_hr2', l1, stride=2))
    l2 = _lrelu(_conv(sd, 'stride_conv_l2', l1, stride=2))
    l3 = _lrelu(_conv(sd, 'stride_conv_l3', l2, stride=2))
    l3 = _up(_resblock(sd, 'resblock_l3', l3))
    l2 = _resblock(sd, 'resblock_l2_1', l2) + l3
    l2 = _up(_resblock(sd, 'resblock_l2_2', l2))
    for i in range(2):
        l1 = _resblock(sd, f'resblock_l1.{i}', l1)
    l1 = l1 + l2
    for i in range(2, 5):
        l1 = _resblock(sd, f'resblock_l1.{i}', l1)
    return l1


def edvr(sd, x, *, num_frame, deformable_groups=8, num_extract_block=5, num_reconstruct_block=10, center=None, hr_in=False,
         with_predeblur=False, with_tsa=True, offsets_out=None):
    """EDVR.forward on (b, t, c, h, w), the frames aligned one by one as the reference does.  ``offsets_out``: a dict that
    receives the PCD offsets of the first frame ('l3', 'l2', 'l1', 'cas')."""
    b, t, c, h, w = x.shape
    center = num_frame // 2 if center is None else center
    x_center = x[:, center]
    flat = x.reshape(b * t, c, h, w)
    if with_predeblur:
        l1 = _conv1(sd, 'conv_1x1', predeblur(_sub(sd, 'predeblur.'), flat, hr_in))
        if hr_in:
            h, w = h // 4, w // 4
    else:
        l1 = _lrelu(_conv(sd, 'conv_first', flat))
    for i in range(num_extract_block):
        l1 = _resblock(sd, f'feature_extraction.{i}', l1)
    l2 = _lrelu(_conv(sd, 'conv_l2_2', _lrelu(_conv(sd, 'conv_l2_1', l1, stride=2))))
    l3 = _lrelu(_conv(sd, 'conv_l3_2', _lrelu(_conv(sd, 'conv_l3_1', l2, stride=2))))
    l1, l2, l3 = l1.view(b, t, -1, h, w), l2.view(b, t, -1, h // 2, w // 2), l3.view(b, t, -1, h // 4, w // 4)
    pcd = _sub(sd, 'pcd_align.')
    ref = [l1[:, center], l2[:, center], l3[:, center]]
    aligned = torch.stack([R.pcd_alignment(pcd, [l1[:, i], l2[:, i], l3[:, i]], ref, deformable_groups,
                                           offsets_out if i == 0 else None) for i in range(t)], dim=1)
    if with_tsa:
        feat = tsa_fusion(_sub(sd, 'fusion.'), aligned, center)
    else:
        feat = _conv1(sd, 'fusion', aligned.reshape(b, -1, h, w))
    out = feat
    for i in range(num_reconstruct_block):
        out = _resblock(sd, f'reconstruction.{i}', out)
    out = _lrelu(F.pixel_shuffle(_conv(sd, 'upconv1', out), 2))
    out = _lrelu(F.pixel_shuffle(_conv(sd, 'upconv2', out), 2))
    out = _conv(sd, 'conv_last', _lrelu(_conv(sd, 'conv_hr', out)))
    base = x_center if hr_in else F.interpolate(x_center, scale_factor=4, mode='bilinear', align_corners=False)
    return out + base
