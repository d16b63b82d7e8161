"""EDVR (reference basicsr/archs/edvr_arch.py) on libsr_hip.so: PCD alignment, TSA fusion, the pre-deblur module and the
network.  Parameter names, shapes and defaults are the reference's, so its checkpoints load key for key; like the reference,
only EDVR is registered in ARCH_REGISTRY.

Between the entry ToCB8 and the exit FromCB8 every activation is CB8 and every layer is an autograd Function of hip_autograd:

    3x3 convs                       ConvFn (sr_conv3x3_f32), LeakyReLU / ReLU in the epilogue
    3x3 stride-2 convs              ConvS2Fn (sr_conv3x3s2_f32; backward on the zero-inserted gradient)
    1x1 convs                       Conv1x1Fn (sr_convd_f32, ksize 1)
    deformable convs                DCNv2Pack.forward_cb8 (sr_dcn_fwd_f32)
    bilinear x2                     Bilinear2xFn
    max + average pooling           Pool3x3s2Fn, one launch writing the concatenation
    temporal attention              TSACorrFn, whose output already is the (b, t*c, h, w) tensor of the fusion convs
    feat * sigmoid(attn) * 2 + add  TSAGateFn
    pixel shuffle                   PixelShuffleFn; the LeakyReLU after it runs in the upconv's epilogue (it commutes)
    bilinear x4 base                BilinearUpFn, added into the NCHW output in place

The frames are a batch: PCD alignment runs ONCE on the b*t images with the centre frame's pyramid expanded over t (the
reference calls it t times); every image is processed independently, so the result is the per-frame loop's bit for bit, and the
expand's autograd sums the reference pyramid's gradients over t.  Channel concatenation, frame selection and the expand are
tensor plumbing on the CB8 storage.

``EDVR(..., compute_dtype='bf16')`` (forward only) runs the same layer list on hip_ops.CB16 windows between
sr_nchw_to_cb16_bf16 and conv_last's fp32 NCHW store: sr_conv3x3_bf16 (the stride-2 convs followed by sr_cb16_subsample2_bf16),
sr_dcn_fwd_bf16 on fp32 offset / mask planes, sr_conv1x1_bf16, sr_pool3x3s2_fwd_bf16, sr_tsa_corr_fwd_bf16, sr_tsa_gate_fwd_bf16,
sr_bilinear2x_fwd_bf16, sr_cb16_pixel_shuffle_bf16; the x4 base is still sr_bilinear_up_f32 of the fp32 centre frame.  Each
module's ``forward_cb16`` is its ``forward_cb8`` on those launches.
"""
import torch
from torch import nn

from .. import hip_autograd as A
from .. import hip_ops as H
from ..utils.registry import ARCH_REGISTRY
from .arch_util import Conv3x3Params, DCNv2Pack, ResidualBlockNoBN, make_layer


def _conv(m, x, slope=0.1):
    return A.ConvFn.apply(x, m.weight, m.bias, slope)


def _conv_s2(m, x, slope=0.1):
    return A.ConvS2Fn.apply(x, m.weight, m.bias, slope)


def _conv1x1(m, x, slope=0.1):
    return A.Conv1x1Fn.apply(x, m.weight, m.bias, slope)


def _resblock(m, x):
    """ResidualBlockNoBN: x + conv2(relu(conv1(x)))."""
    return A.AddFn.apply(x, _conv(m.conv2, _conv(m.conv1, x, 0.0), 1.0))


# ---- the bf16 inference path: hip_ops.CB16 windows between sr_nchw_to_cb16_bf16 and conv_last's fp32 NCHW store ----

def _conv16(m, x, slope=0.1, **kw):
    return H.conv3x3_bf16(x, H.packed_conv_bf16(m), act_slope=slope, **kw)


def _conv_s2_16(m, x, slope=0.1):
    """3x3 / stride 2 / pad 1: the stride-1 conv sampled at the even positions (4x the MACs of a native stride-2 kernel)."""
    return H.subsample2_bf16(_conv16(m, x, slope))


def _conv1x1_16(m, x, slope=0.1):
    return H.conv1x1_bf16(x, H.packed_conv_bf16(m), act_slope=slope)


def _resblock16(m, x, extra=None):
    """ResidualBlockNoBN (+ ``extra``): both additions in conv2's epilogue, one rounding."""
    kw = dict(res2=extra, beta2=1.0) if extra is not None else {}
    return _conv16(m.conv2, _conv16(m.conv1, x, 0.0), 1.0, res1=x, beta1=1.0, **kw)


def _cat16(*ts):
    """torch.cat along the channel-block dimension of whole CB16 tensors."""
    assert all(t.cb0 == 0 and t.cbn == t.buf.size(1) for t in ts)
    return H.CB16(torch.cat([t.buf for t in ts], dim=1))


def _check_input(x, what, dims):
    if x.dim() != dims:
        raise ValueError(f'{what}: expected a {dims}-dimensional input, got {tuple(x.shape)}')
    if x.dtype != torch.float32:
        raise ValueError(f'{what}: {x.dtype} input is not supported; supported: fp32')


def _need_gpu(x):
    """After the shape refusals, so that they do not depend on where the tensor lives."""
    if not x.is_cuda:
        raise NotImplementedError


class PCDAlignment(nn.Module):
    """EDVR's alignment of one frame's features to the centre frame's: deformable convs on a three-level pyramid, coarse to
    fine, and one more deformable conv on the result (the reference's PCDAlignment, edvr_arch.py:9-98).

    ``forward(nbr_feat_l, ref_feat_l)`` takes the two three-level pyramids (L1, L2, L3; each [b, c, h, w], NCHW fp32 on the GPU)
    and returns the aligned L1 features as NCHW; ``forward_cb8`` is the same on CB8 tensors, CB8 out.  Inside, everything is
    CB8: every layer is an autograd Function of hip_autograd (3x3 convs with LeakyReLU 0.1 in their epilogue, bilinear x2 with
    align_corners=False, DCNFn).  Channel concatenation and the ``* 2`` of the upsampled offsets are tensor plumbing on the CB8
    storage (torch.cat along the block dimension, one scaling).

    Args:
        num_feat (int): channels of every feature map; a multiple of 8 * deformable_groups.  Default: 64.
        deformable_groups (int): offset / mask groups of the deformable convs.  Default: 8.
    """

    def __init__(self, num_feat=64, deformable_groups=8):
        super().__init__()
        # per level l3 (quarter size), l2 (half size), l1 (full size), in the reference's registration order
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
        # the deformable conv applied to the aligned level-1 features
        self.cas_offset_conv1 = Conv3x3Params(num_feat * 2, num_feat)
        self.cas_offset_conv2 = Conv3x3Params(num_feat, num_feat)
        self.cas_dcnpack = DCNv2Pack(num_feat, num_feat, 3, padding=1, deformable_groups=deformable_groups)
        self.num_feat = num_feat

    _conv = staticmethod(_conv)

    def forward_cb8(self, nbr, ref):
        """The two pyramids as lists of CB8 tensors (L1, L2, L3) -> the aligned L1 features, CB8."""
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
            if i > 1:  # hand offsets and features to the next finer level; offsets count pixels, so they double as well
                upsampled_offset = A.Bilinear2xFn.apply(offset) * 2
                upsampled_feat = A.Bilinear2xFn.apply(feat)
        # the last deformable conv, its offsets from the aligned features and the centre frame
        offset = conv(self.cas_offset_conv2, conv(self.cas_offset_conv1, torch.cat([feat, ref[0]], dim=1)))
        return self.cas_dcnpack.forward_cb8(feat, offset, 0.1)

    def forward_cb16(self, nbr, ref):
        """forward_cb8's layer list on hip_ops.CB16 windows (bf16 inference): the pyramids as lists of CB16 -> aligned L1, CB16."""
        upsampled_offset, upsampled_feat = None, None
        for i in range(3, 0, -1):
            level = f'l{i}'
            offset = _conv16(self.offset_conv1[level], _cat16(nbr[i - 1], ref[i - 1]))
            if i == 3:
                offset = _conv16(self.offset_conv2[level], offset)
            else:
                offset = _conv16(self.offset_conv2[level], _cat16(offset, upsampled_offset))
                offset = _conv16(self.offset_conv3[level], offset)
            if i < 3:
                feat = self.dcn_pack[level].forward_cb16(nbr[i - 1], offset)
                feat = _conv16(self.feat_conv[level], _cat16(feat, upsampled_feat), 0.1 if i > 1 else 1.0)
            else:
                feat = self.dcn_pack[level].forward_cb16(nbr[i - 1], offset, 0.1)
            if i > 1:
                upsampled_offset = H.cb16_scale(H.bilinear2x_bf16(offset), 2.0)   # exact: a power of two
                upsampled_feat = H.bilinear2x_bf16(feat)
        offset = _conv16(self.cas_offset_conv2, _conv16(self.cas_offset_conv1, _cat16(feat, ref[0])))
        return self.cas_dcnpack.forward_cb16(feat, offset, 0.1)

    def forward(self, nbr_feat_l, ref_feat_l):
        for t in list(nbr_feat_l) + list(ref_feat_l):
            if not t.is_cuda:
                raise NotImplementedError
        nbr = [A.ToCB8.apply(t) for t in nbr_feat_l]
        ref = [A.ToCB8.apply(t) for t in ref_feat_l]
        return A.FromCB8.apply(self.forward_cb8(nbr, ref), self.num_feat)


class TSAFusion(nn.Module):
    """EDVR's fusion of the aligned frames into one feature map (the reference's TSAFusion, edvr_arch.py:101-190).

    First every frame is weighted, per pixel, by the sigmoid of its embedding's correlation with the centre frame's; the
    weighted frames are fused by a 1x1 conv.  Then an attention map computed on two coarser levels (max + average pooling down,
    bilinear up) scales the fused features, and a second map from the same branch is added.

    ``forward(aligned_feat)`` takes (b, t, c, h, w) NCHW fp32 on the GPU with h and w multiples of 4 (on other sizes the reference
    fails with a shape error after its two poolings and upsamplings; here it is a ValueError) and returns (b, c, h, w);
    ``forward_cb8(aligned, b, t)`` takes the frames as a CB8 batch of b * t images and returns CB8.

    Args:
        num_feat (int): channels per frame and of the result; a multiple of 8.  Default: 64.
        num_frame (int): frames per clip.  Default: 5.
        center_frame_idx (int): which frame the others are correlated with.  Default: 2.
    """

    def __init__(self, num_feat=64, num_frame=5, center_frame_idx=2):
        super().__init__()
        if num_feat % 8:
            raise ValueError(f'TSAFusion: num_feat={num_feat} must be a multiple of 8 (frames are concatenated by CB8 block)')
        self.center_frame_idx = center_frame_idx
        self.num_feat, self.num_frame = num_feat, num_frame
        # frame weighting: embeddings of the centre frame and of every frame, then the 1x1 fusion over t * num_feat channels
        self.temporal_attn1 = Conv3x3Params(num_feat, num_feat)
        self.temporal_attn2 = Conv3x3Params(num_feat, num_feat)
        self.feat_fusion = Conv3x3Params(num_frame * num_feat, num_feat, ksize=1)
        # attention branch on the weighted frames: half and quarter resolution, back up, scale and shift of the fused features
        self.spatial_attn1 = Conv3x3Params(num_frame * num_feat, num_feat, ksize=1)
        self.spatial_attn2 = Conv3x3Params(num_feat * 2, num_feat, ksize=1)
        self.spatial_attn3 = Conv3x3Params(num_feat, num_feat)
        self.spatial_attn4 = Conv3x3Params(num_feat, num_feat, ksize=1)
        self.spatial_attn5 = Conv3x3Params(num_feat, num_feat)
        self.spatial_attn_l1 = Conv3x3Params(num_feat, num_feat, ksize=1)
        self.spatial_attn_l2 = Conv3x3Params(num_feat * 2, num_feat)
        self.spatial_attn_l3 = Conv3x3Params(num_feat, num_feat)
        self.spatial_attn_add1 = Conv3x3Params(num_feat, num_feat, ksize=1)
        self.spatial_attn_add2 = Conv3x3Params(num_feat, num_feat, ksize=1)

    def forward_cb8(self, aligned, b, t):
        bt, cb, h, w, _ = aligned.shape
        if bt != b * t or t != self.num_frame:
            raise ValueError(f'TSAFusion: {bt} images are not {b} x num_frame={self.num_frame}')
        if h % 4 or w % 4:
            raise ValueError(f'TSAFusion: the height and width must be multiples of 4 (got {h}x{w})')
        # per-frame weights from the correlation with the centre frame
        center = aligned.view(b, t, cb, h, w, 8)[:, self.center_frame_idx].contiguous()
        embedding_ref = _conv(self.temporal_attn1, center, 1.0)
        embedding = _conv(self.temporal_attn2, aligned, 1.0)
        fused = A.TSACorrFn.apply(embedding, embedding_ref, aligned, t)   # (b, t*c): aligned * sigmoid(correlation)
        feat = _conv1x1(self.feat_fusion, fused)
        # attention branch, half resolution
        attn = _conv1x1(self.spatial_attn1, fused)
        attn = _conv1x1(self.spatial_attn2, A.Pool3x3s2Fn.apply(attn))
        # quarter resolution and back
        attn_level = _conv1x1(self.spatial_attn_l1, attn)
        attn_level = _conv(self.spatial_attn_l2, A.Pool3x3s2Fn.apply(attn_level))
        attn_level = A.Bilinear2xFn.apply(_conv(self.spatial_attn_l3, attn_level))
        attn = A.AddFn.apply(_conv(self.spatial_attn3, attn), attn_level)
        attn = A.Bilinear2xFn.apply(_conv1x1(self.spatial_attn4, attn))
        attn = _conv(self.spatial_attn5, attn, 1.0)
        attn_add = _conv1x1(self.spatial_attn_add2, _conv1x1(self.spatial_attn_add1, attn), 1.0)
        # sigmoid(attn) * 2 is about 1 for a freshly initialised branch (attn near 0), so the gate starts as the identity
        return A.TSAGateFn.apply(feat, attn, attn_add)

    def forward_cb16(self, aligned, b, t):
        """forward_cb8's layer list on hip_ops.CB16 windows (bf16 inference); ``aligned``: a whole CB16 tensor of b * t images."""
        bt, cb, h, w = aligned.n, aligned.cbn, aligned.h, aligned.w
        if bt != b * t or t != self.num_frame:
            raise ValueError(f'TSAFusion: {bt} images are not {b} x num_frame={self.num_frame}')
        if h % 4 or w % 4:
            raise ValueError(f'TSAFusion: the height and width must be multiples of 4 (got {h}x{w})')
        center = H.CB16(aligned.buf.view(b, t, cb, h, w, 16)[:, self.center_frame_idx].contiguous())
        embedding_ref = _conv16(self.temporal_attn1, center, 1.0)
        embedding = _conv16(self.temporal_attn2, aligned, 1.0)
        fused = H.tsa_corr_bf16(embedding, embedding_ref, aligned, t)
        fused = H.CB16(fused.buf.view(b, t * cb, h, w, 16))                 # (b, t*c): what the fusion convs read
        feat = _conv1x1_16(self.feat_fusion, fused)
        attn = _conv1x1_16(self.spatial_attn1, fused)
        attn = _conv1x1_16(self.spatial_attn2, H.pool3x3s2_bf16(attn))
        attn_level = _conv1x1_16(self.spatial_attn_l1, attn)
        attn_level = _conv16(self.spatial_attn_l2, H.pool3x3s2_bf16(attn_level))
        attn_level = H.bilinear2x_bf16(_conv16(self.spatial_attn_l3, attn_level))
        attn = _conv16(self.spatial_attn3, attn, res1=attn_level, beta1=1.0)   # the addition in the conv's epilogue
        attn = H.bilinear2x_bf16(_conv1x1_16(self.spatial_attn4, attn))
        attn = _conv16(self.spatial_attn5, attn, 1.0)
        attn_add = _conv1x1_16(self.spatial_attn_add2, _conv1x1_16(self.spatial_attn_add1, attn), 1.0)
        return H.tsa_gate_bf16(feat, attn, attn_add)

    def forward(self, aligned_feat):
        _check_input(aligned_feat, 'TSAFusion', 5)
        b, t, c, h, w = aligned_feat.shape
        if c != self.num_feat:
            raise ValueError(f'TSAFusion: {c} channels, expected num_feat={self.num_feat}')
        if h % 4 or w % 4:
            raise ValueError(f'TSAFusion: the height and width must be multiples of 4 (got {h}x{w})')
        _need_gpu(aligned_feat)
        out = self.forward_cb8(A.ToCB8.apply(aligned_feat.reshape(b * t, c, h, w)), b, t)
        return A.FromCB8.apply(out, self.num_feat)


class PredeblurModule(nn.Module):
    """EDVR's optional front end for blurred input (the reference's PredeblurModule, edvr_arch.py:193-243): features of each
    frame refined by residual blocks on three resolutions, the coarser results upsampled and added to the finer ones.

    Args:
        num_in_ch (int): image channels.  Default: 3.
        num_feat (int): feature channels.  Default: 64.
        hr_in (bool): the input already has the output's size; two more stride-2 convs bring it down by 4 first.
            Default: False.
    """

    def __init__(self, num_in_ch=3, num_feat=64, hr_in=False):
        super().__init__()
        self.hr_in = hr_in
        self.num_feat = num_feat

        self.conv_first = Conv3x3Params(num_in_ch, num_feat)
        if self.hr_in:
            # two stride-2 convs: a quarter of the input's size
            self.stride_conv_hr1 = Conv3x3Params(num_feat, num_feat)
            self.stride_conv_hr2 = Conv3x3Params(num_feat, num_feat)

        # half and quarter size of that
        self.stride_conv_l2 = Conv3x3Params(num_feat, num_feat)
        self.stride_conv_l3 = Conv3x3Params(num_feat, num_feat)

        self.resblock_l3 = ResidualBlockNoBN(num_feat=num_feat)
        self.resblock_l2_1 = ResidualBlockNoBN(num_feat=num_feat)
        self.resblock_l2_2 = ResidualBlockNoBN(num_feat=num_feat)
        self.resblock_l1 = nn.ModuleList([ResidualBlockNoBN(num_feat=num_feat) for i in range(5)])

    def _check_size(self, h, w):
        m = 16 if self.hr_in else 4
        if h % m or w % m:
            raise ValueError(f'PredeblurModule: the height and width must be multiples of {m} (got {h}x{w})')

    def forward_cb8(self, x):
        self._check_size(x.size(2), x.size(3))
        feat_l1 = _conv(self.conv_first, x)
        if self.hr_in:
            feat_l1 = _conv_s2(self.stride_conv_hr1, feat_l1)
            feat_l1 = _conv_s2(self.stride_conv_hr2, feat_l1)
        feat_l2 = _conv_s2(self.stride_conv_l2, feat_l1)
        feat_l3 = _conv_s2(self.stride_conv_l3, feat_l2)

        feat_l3 = A.Bilinear2xFn.apply(_resblock(self.resblock_l3, feat_l3))
        feat_l2 = A.AddFn.apply(_resblock(self.resblock_l2_1, feat_l2), feat_l3)
        feat_l2 = A.Bilinear2xFn.apply(_resblock(self.resblock_l2_2, feat_l2))

        for i in range(2):
            feat_l1 = _resblock(self.resblock_l1[i], feat_l1)
        feat_l1 = A.AddFn.apply(feat_l1, feat_l2)
        for i in range(2, 5):
            feat_l1 = _resblock(self.resblock_l1[i], feat_l1)
        return feat_l1

    def forward_cb16(self, x):
        """forward_cb8's layer list on hip_ops.CB16 windows (bf16 inference); the two additions run in the epilogue of the
        preceding residual block's second conv."""
        self._check_size(x.h, x.w)
        feat_l1 = _conv16(self.conv_first, x)
        if self.hr_in:
            feat_l1 = _conv_s2_16(self.stride_conv_hr1, feat_l1)
            feat_l1 = _conv_s2_16(self.stride_conv_hr2, feat_l1)
        feat_l2 = _conv_s2_16(self.stride_conv_l2, feat_l1)
        feat_l3 = _conv_s2_16(self.stride_conv_l3, feat_l2)

        feat_l3 = H.bilinear2x_bf16(_resblock16(self.resblock_l3, feat_l3))
        feat_l2 = _resblock16(self.resblock_l2_1, feat_l2, feat_l3)
        feat_l2 = H.bilinear2x_bf16(_resblock16(self.resblock_l2_2, feat_l2))

        feat_l1 = _resblock16(self.resblock_l1[0], feat_l1)
        feat_l1 = _resblock16(self.resblock_l1[1], feat_l1, feat_l2)
        for i in range(2, 5):
            feat_l1 = _resblock16(self.resblock_l1[i], feat_l1)
        return feat_l1

    def forward(self, x):
        _check_input(x, 'PredeblurModule', 4)
        self._check_size(x.size(2), x.size(3))
        _need_gpu(x)
        return A.FromCB8.apply(self.forward_cb8(A.ToCB8.apply(x)), self.num_feat)


@ARCH_REGISTRY.register()
class EDVR(nn.Module):
    """EDVR (Wang et al., "EDVR: Video Restoration with Enhanced Deformable Convolutional Networks"; the reference's
    edvr_arch.py:246-383): restores the centre frame of a clip, x4 like the reference.

    ``forward(x)`` takes (b, t, c, h, w) fp32 on the GPU, h and w multiples of 4, and returns (b, 3, 4h, 4w).  With ``hr_in``
    (which needs ``with_predeblur``: the pre-deblur module is what brings the input down by 4) h and w are multiples of 16
    and the result is (b, 3, h, w).  ``hr_in`` without ``with_predeblur`` is refused at construction; the reference builds
    that network and fails in its forward when it adds the x4 output to the centre frame.

    Args:
        num_in_ch (int): image channels of the input frames.  Default: 3.
        num_out_ch (int): accepted for the reference's signature; the last conv always has 3 outputs, as there.  Default: 3.
        num_feat (int): feature channels; a multiple of 8 * deformable_groups.  Default: 64.
        num_frame (int): frames per clip.  Default: 5.
        deformable_groups (int): offset / mask groups of the deformable convs.  Default: 8.
        num_extract_block (int): residual blocks before the pyramid.  Default: 5.
        num_reconstruct_block (int): residual blocks after the fusion.  Default: 10.
        center_frame_idx (int): the frame to restore, from 0.  Default: num_frame // 2.
        hr_in (bool): the input already has the output's size (needs with_predeblur).  Default: False.
        with_predeblur (bool): run PredeblurModule and a 1x1 conv instead of the first conv.  Default: False.
        with_tsa (bool): fuse with TSAFusion; otherwise with one 1x1 conv over the t * num_feat channels.  Default: True.
        compute_dtype (str): this project's own key, 'fp32' or 'bf16' (anything else is a ValueError).  'bf16' needs num_feat to
            be a multiple of 16 (CB16 activations) and is forward only (eval mode or no_grad): bf16 activations and weight
            images rounded from the fp32 parameters, fp32 accumulation, offsets and mask logits of the deformable convs in
            fp32, conv_last and the x4 base of the fp32 centre frame in fp32.  The parameters, their names and their
            initialisation do not depend on it.  Default: 'fp32'.
    """

    def __init__(self,
                 num_in_ch=3,
                 num_out_ch=3,
                 num_feat=64,
                 num_frame=5,
                 deformable_groups=8,
                 num_extract_block=5,
                 num_reconstruct_block=10,
                 center_frame_idx=None,
                 hr_in=False,
                 with_predeblur=False,
                 with_tsa=True,
                 compute_dtype='fp32'):
        super().__init__()
        if compute_dtype not in ('fp32', 'bf16'):
            raise ValueError(f"compute dtype must be 'fp32' or 'bf16', got {compute_dtype!r}")
        if deformable_groups <= 0 or num_feat % (8 * deformable_groups):
            raise ValueError(f'EDVR: num_feat={num_feat} must be a multiple of 8 * deformable_groups={deformable_groups} '
                             '(a CB8 block never straddles two deformable groups)')
        if compute_dtype == 'bf16' and num_feat % 16:
            raise ValueError(f'EDVR in bf16 needs num_feat to be a multiple of 16 (CB16 activations), got {num_feat!r}')
        self.compute_dtype = compute_dtype
        if hr_in and not with_predeblur:
            raise ValueError('EDVR: hr_in needs with_predeblur=True (only the pre-deblur module brings a high-resolution input '
                             'down by 4; without it the x4 output cannot be added to the centre frame)')
        if center_frame_idx is None:
            self.center_frame_idx = num_frame // 2
        else:
            self.center_frame_idx = center_frame_idx
        self.hr_in = hr_in
        self.with_predeblur = with_predeblur
        self.with_tsa = with_tsa
        self.num_feat, self.num_frame = num_feat, num_frame

        # first layer(s), per frame
        if self.with_predeblur:
            self.predeblur = PredeblurModule(num_feat=num_feat, hr_in=self.hr_in)
            self.conv_1x1 = Conv3x3Params(num_feat, num_feat, ksize=1)
        else:
            self.conv_first = Conv3x3Params(num_in_ch, num_feat)

        # residual blocks at full size, then the half- and quarter-size levels of the pyramid
        self.feature_extraction = make_layer(ResidualBlockNoBN, num_extract_block, num_feat=num_feat)
        self.conv_l2_1 = Conv3x3Params(num_feat, num_feat)
        self.conv_l2_2 = Conv3x3Params(num_feat, num_feat)
        self.conv_l3_1 = Conv3x3Params(num_feat, num_feat)
        self.conv_l3_2 = Conv3x3Params(num_feat, num_feat)

        # alignment and fusion
        self.pcd_align = PCDAlignment(num_feat=num_feat, deformable_groups=deformable_groups)
        if self.with_tsa:
            self.fusion = TSAFusion(num_feat=num_feat, num_frame=num_frame, center_frame_idx=self.center_frame_idx)
        else:
            self.fusion = Conv3x3Params(num_frame * num_feat, num_feat, ksize=1)

        # residual blocks on the fused features, then two conv + pixel-shuffle stages and the two output convs
        self.reconstruction = make_layer(ResidualBlockNoBN, num_reconstruct_block, num_feat=num_feat)
        self.upconv1 = Conv3x3Params(num_feat, num_feat * 4)
        self.upconv2 = Conv3x3Params(num_feat, 64 * 4)
        self.conv_hr = Conv3x3Params(64, 64)
        self.conv_last = Conv3x3Params(64, 3)

    def align_cb8(self, feat_l, b, t):
        """PCD alignment of every frame to the centre frame in one batched call: ``feat_l`` = the pyramid (L1, L2, L3) of the
        b * t frames, CB8; the centre frame's pyramid is expanded over t."""
        ref_l = []
        for f in feat_l:
            _, cb, h, w, _ = f.shape
            c = f.view(b, t, cb, h, w, 8)[:, self.center_frame_idx:self.center_frame_idx + 1]
            ref_l.append(c.expand(b, t, cb, h, w, 8).reshape(b * t, cb, h, w, 8))
        return self.pcd_align.forward_cb8(feat_l, ref_l)

    def forward_bf16(self, x):
        """The layer list of ``forward`` on CB16 bf16 activations; fp32 NCHW in and out."""
        b, t, c, h, w = x.shape
        ci = self.center_frame_idx
        x_center = x[:, ci].contiguous()
        frames = H.nchw_to_cb16(x.reshape(b * t, c, h, w))
        if self.with_predeblur:
            feat_l1 = _conv1x1_16(self.conv_1x1, self.predeblur.forward_cb16(frames), 1.0)
        else:
            feat_l1 = _conv16(self.conv_first, frames)
        for blk in self.feature_extraction:
            feat_l1 = _resblock16(blk, feat_l1)
        feat_l2 = _conv16(self.conv_l2_2, _conv_s2_16(self.conv_l2_1, feat_l1))
        feat_l3 = _conv16(self.conv_l3_2, _conv_s2_16(self.conv_l3_1, feat_l2))

        feat_l = [feat_l1, feat_l2, feat_l3]
        ref_l = []
        for f in feat_l:   # the centre frame's pyramid expanded over t
            v = f.buf.view(b, t, f.cbn, f.h, f.w, 16)[:, ci:ci + 1]
            ref_l.append(H.CB16(v.expand(b, t, f.cbn, f.h, f.w, 16).reshape(b * t, f.cbn, f.h, f.w, 16).contiguous()))
        aligned = self.pcd_align.forward_cb16(feat_l, ref_l)

        if self.with_tsa:
            out = self.fusion.forward_cb16(aligned, b, t)
        else:
            fused = H.CB16(aligned.buf.view(b, t * aligned.cbn, aligned.h, aligned.w, 16))
            out = _conv1x1_16(self.fusion, fused, 1.0)
        for blk in self.reconstruction:
            out = _resblock16(blk, out)
        out = H.pixel_shuffle_bf16(_conv16(self.upconv1, out), self.num_feat, 2)
        out = H.pixel_shuffle_bf16(_conv16(self.upconv2, out), 64, 2)
        out = _conv16(self.conv_hr, out)
        y = torch.empty((b, 3, out.h, out.w), dtype=torch.float32, device=x.device)
        _conv16(self.conv_last, out, 1.0, out_nchw=y)
        if self.hr_in:
            return A.AddFn.apply(y, x_center)
        return H.bilinear_up(x_center, 4, out=y)

    def forward(self, x):
        _check_input(x, 'EDVR', 5)
        b, t, c, h, w = x.shape
        if t != self.num_frame:
            raise ValueError(f'EDVR: {t} frames, expected num_frame={self.num_frame}')
        m = 16 if self.hr_in else 4
        if h % m or w % m:
            raise ValueError(f'EDVR: the height and width must be multiples of {m} (got {h}x{w})')
        _need_gpu(x)
        if self.compute_dtype == 'bf16':
            needs_graph = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
            if needs_graph and self.training:
                raise NotImplementedError("EDVR with compute_dtype='bf16' is forward only (eval mode or torch.no_grad()); train "
                                          "with compute_dtype='fp32'")
            with torch.no_grad():
                return self.forward_bf16(x)

        x_center = x[:, self.center_frame_idx].contiguous()
        frames = A.ToCB8.apply(x.reshape(b * t, c, h, w))

        # level-1 features of every frame
        if self.with_predeblur:
            feat_l1 = _conv1x1(self.conv_1x1, self.predeblur.forward_cb8(frames), 1.0)
        else:
            feat_l1 = _conv(self.conv_first, frames)
        for blk in self.feature_extraction:
            feat_l1 = _resblock(blk, feat_l1)
        feat_l2 = _conv(self.conv_l2_2, _conv_s2(self.conv_l2_1, feat_l1))
        feat_l3 = _conv(self.conv_l3_2, _conv_s2(self.conv_l3_1, feat_l2))

        # PCD alignment, all frames at once
        aligned = self.align_cb8([feat_l1, feat_l2, feat_l3], b, t)

        if self.with_tsa:
            feat = self.fusion.forward_cb8(aligned, b, t)
        else:
            bt, cb, fh, fw, _ = aligned.shape
            feat = _conv1x1(self.fusion, aligned.view(b, t * cb, fh, fw, 8), 1.0)

        out = feat
        for blk in self.reconstruction:
            out = _resblock(blk, out)
        # the LeakyReLU after each pixel shuffle commutes with it: it runs in the upconv's epilogue
        out = A.PixelShuffleFn.apply(_conv(self.upconv1, out), self.num_feat, 2)
        out = A.PixelShuffleFn.apply(_conv(self.upconv2, out), 64, 2)
        out = _conv(self.conv_hr, out)
        out = A.FromCB8.apply(_conv(self.conv_last, out, 1.0), 3)
        if self.hr_in:
            return A.AddFn.apply(out, x_center)
        return A.BilinearUpFn.apply(x_center, 4, out)
