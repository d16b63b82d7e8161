"""EDVR (reference basicsr/archs/edvr_arch.py) on libsr_hip.so: PCD alignment, TSA fusion, the pre-deblur module and the
network.  Parameter names, shapes and defaults are the reference's, so its checkpoints load key for key; like the reference,
only EDVR is registered in ARCH_REGISTRY.

Every module states its layer list ONCE (``_layers(ops, ...)``; ``EDVR._run(x, ops)``) against a table of operations, and there
are two tables: ``_CB8Ops`` (fp32, with gradients) and ``_CB16Ops`` (bf16, forward only).  A table says how a layer is launched
and which neighbouring additions it fuses; which layers there are, their parameters, slopes and skips is said by the list alone.
``forward_cb8`` / ``forward_cb16`` of a module are its list on the one table or the other.

``_CB8Ops``: between the entry ToCB8 and the exit FromCB8 every activation is a raw CB8 tensor [n, cb, h, w, 8] and every layer is
an autograd Function of hip_autograd:

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

``_CB16Ops`` (``EDVR(..., compute_dtype='bf16')``): hip_ops.CB16 windows between sr_nchw_to_cb16_bf16 and the last
conv's fp32 NCHW store: sr_conv3x3_bf16 (the stride-2 convs followed by sr_cb16_subsample2_bf16; a skip addition after a conv runs
in its epilogue), sr_dcn_fwd_bf16 on fp32 offset / mask planes (DCNv2Pack.forward_cb16), sr_conv1x1_bf16, sr_pool3x3s2_fwd_bf16,
sr_tsa_corr_fwd_bf16, sr_tsa_gate_fwd_bf16, sr_bilinear2x_fwd_bf16, sr_cb16_pixel_shuffle_bf16; the x4 base is still
sr_bilinear_up_f32 of the fp32 centre frame.

The frames are a batch: PCD alignment runs ONCE on the b*t images with the centre frame's pyramid expanded over t (the
reference calls it t times); every image is processed independently, so the result is the per-frame loop's bit for bit, and the
expand's autograd sums the reference pyramid's gradients over t.  Channel concatenation, frame selection and the expand are
tensor plumbing on the channel-blocked storage, written once for both tables (``_Ops``).
"""
import torch
from torch import nn

from .. import hip_autograd as A
from .. import hip_ops as H
from ..utils.registry import ARCH_REGISTRY
from .arch_util import Conv3x3Params, DCNv2Pack, ResidualBlockNoBN, make_layer


class _Ops:
    """What the two tables share: the frame plumbing, on the storage [n, cb, h, w, lanes] of a whole activation (``raw``; ``wrap``
    makes an activation of a view of one, with a copy only where the table's layers need contiguous storage)."""

    def dims(self, x):
        return tuple(self.raw(x).shape[:4])

    def _clips(self, x, b, t):
        return self.raw(x).view(b, t, *self.raw(x).shape[1:])

    def center(self, x, b, t, idx):
        """Frame ``idx`` of every clip of a b * t batch: b images."""
        return self.wrap(self._clips(x, b, t)[:, idx].contiguous())

    def center_over_t(self, x, b, t, idx):
        """The same frame expanded over t: b * t images (in fp32 the expand's autograd sums the gradients over t).  For b == 1
        the result is still a view, stride 0 over t: no copy unless ``wrap`` makes one."""
        v = self._clips(x, b, t)[:, idx:idx + 1]
        return self.wrap(v.expand(b, t, *v.shape[2:]).reshape(self.raw(x).shape))

    def frames_to_channels(self, x, b, t):
        """(b * t, cb) read as (b, t * cb): a clip's frames concatenated by channel, the same memory."""
        _, cb, *rest = self.raw(x).shape
        return self.wrap(self.raw(x).view(b, t * cb, *rest))


class _CB8Ops(_Ops):
    """fp32: autograd Functions of hip_autograd on raw CB8 tensors [n, cb, h, w, 8]."""
    raw = wrap = staticmethod(lambda x: x)
    enter = A.ToCB8.apply
    pool = A.Pool3x3s2Fn.apply
    tsa_corr = A.TSACorrFn.apply        # its output already is (b, t*c)
    tsa_gate = A.TSAGateFn.apply
    pixel_shuffle = A.PixelShuffleFn.apply
    dcn = staticmethod(DCNv2Pack.forward_cb8)

    def conv(self, m, x, slope=0.1):
        return A.ConvFn.apply(x, m.weight, m.bias, slope)

    def conv_s2(self, m, x, slope=0.1):
        return A.ConvS2Fn.apply(x, m.weight, m.bias, slope)

    def conv1x1(self, m, x, slope=0.1):
        return A.Conv1x1Fn.apply(x, m.weight, m.bias, slope)

    def conv_add(self, m, x, other, slope=0.1):
        return A.AddFn.apply(self.conv(m, x, slope), other)

    def conv_nchw(self, m, x):
        return A.FromCB8.apply(self.conv(m, x, 1.0), m.out_channels)

    def resblock(self, m, x, extra=None):
        """ResidualBlockNoBN: x + conv2(relu(conv1(x))) (+ ``extra``)."""
        y = A.AddFn.apply(x, self.conv(m.conv2, self.conv(m.conv1, x, 0.0), 1.0))
        return y if extra is None else A.AddFn.apply(y, extra)

    def cat(self, *ts):
        return torch.cat(ts, dim=1)

    def up2(self, x, scale=1.0):
        y = A.Bilinear2xFn.apply(x)
        return y if scale == 1.0 else y * scale


class _CB16Ops(_Ops):
    """bf16, forward only: hip_ops launches on whole hip_ops.CB16 windows; the weight images are hip_ops.packed_conv_bf16's."""
    raw, wrap = staticmethod(lambda x: x.buf), staticmethod(lambda buf: H.CB16(buf.contiguous()))
    enter = staticmethod(H.nchw_to_cb16)
    pool = staticmethod(H.pool3x3s2_bf16)
    tsa_gate = staticmethod(H.tsa_gate_bf16)
    pixel_shuffle = staticmethod(H.pixel_shuffle_bf16)
    dcn = staticmethod(DCNv2Pack.forward_cb16)

    def conv(self, m, x, slope=0.1, **kw):
        return H.conv3x3_bf16(x, H.packed_conv_bf16(m), act_slope=slope, **kw)

    def conv_s2(self, m, x, slope=0.1):
        """3x3 / stride 2 / pad 1: the stride-1 conv sampled at the even positions (4x the MACs of a native stride-2 kernel)."""
        return H.subsample2_bf16(self.conv(m, x, slope))

    def conv1x1(self, m, x, slope=0.1):
        return H.conv1x1_bf16(x, H.packed_conv_bf16(m), act_slope=slope)

    def conv_add(self, m, x, other, slope=0.1):
        return self.conv(m, x, slope, res1=other, beta1=1.0)   # the addition in the conv's epilogue

    def conv_nchw(self, m, x):
        y = torch.empty((x.n, m.out_channels, x.h, x.w), dtype=torch.float32, device=x.device)
        self.conv(m, x, 1.0, out_nchw=y)
        return y

    def resblock(self, m, x, extra=None):
        """ResidualBlockNoBN (+ ``extra``): both additions in conv2's epilogue, one rounding."""
        kw = dict(res2=extra, beta2=1.0) if extra is not None else {}
        return self.conv(m.conv2, self.conv(m.conv1, x, 0.0), 1.0, res1=x, beta1=1.0, **kw)

    def cat(self, *ts):
        """torch.cat along the channel-block dimension of whole CB16 tensors."""
        assert all(t.cb0 == 0 and t.cbn == t.buf.size(1) for t in ts)
        return H.CB16(torch.cat([t.buf for t in ts], dim=1))

    def up2(self, x, scale=1.0):
        y = H.bilinear2x_bf16(x)
        return y if scale == 1.0 else H.cb16_scale(y, scale)   # exact for a power of two

    def tsa_corr(self, emb, emb_ref, aligned, t):
        return self.frames_to_channels(H.tsa_corr_bf16(emb, emb_ref, aligned, t), emb_ref.n, t)


_FP32, _BF16 = _CB8Ops(), _CB16Ops()


def _check_input(x, what, dims):
    if x.dim() != dims:
        raise ValueError(f'{what}: expected a {dims}-dimensional input, got {tuple(x.shape)}')
    if x.dtype != torch.float32:
        raise ValueError(f'{what}: {x.dtype} input is not supported; supported: fp32')


def _need_gpu(x):
    """After the shape refusals, so that they do not depend on where the tensor lives."""
    if not x.is_cuda:
        raise NotImplementedError


def _set_deterministic(module, flag):
    for m in module.modules():
        if isinstance(m, DCNv2Pack):
            m.deterministic = bool(flag)
    return module


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

    def set_deterministic(self, flag=True):
        """This project's own switch: every deformable conv below takes the bit-reproducible input gradient
        (include/sr_hip_dcn_det.h) in its backward.  Off by default; the forward is the same.  Returns self."""
        return _set_deterministic(self, flag)

    def _layers(self, ops, nbr, ref):
        conv, cat = ops.conv, ops.cat
        upsampled_offset, upsampled_feat = None, None
        for i in range(3, 0, -1):
            level = f'l{i}'
            offset = conv(self.offset_conv1[level], cat(nbr[i - 1], ref[i - 1]))
            if i == 3:
                offset = conv(self.offset_conv2[level], offset)
            else:
                offset = conv(self.offset_conv2[level], cat(offset, upsampled_offset))
                offset = conv(self.offset_conv3[level], offset)
            # LeakyReLU after the level-3 deformable conv; on the finer levels it follows feat_conv, and on level 2 only: the
            # level-1 feat_conv output goes on without activation
            feat = ops.dcn(self.dcn_pack[level], nbr[i - 1], offset, 0.1 if i == 3 else 1.0)
            if i < 3:
                feat = conv(self.feat_conv[level], cat(feat, upsampled_feat), 0.1 if i > 1 else 1.0)
            if i > 1:  # hand offsets and features to the next finer level; offsets count pixels, so they double as well
                upsampled_offset = ops.up2(offset, 2.0)
                upsampled_feat = ops.up2(feat)
        # the last deformable conv, its offsets from the aligned features and the centre frame
        offset = conv(self.cas_offset_conv2, conv(self.cas_offset_conv1, cat(feat, ref[0])))
        return ops.dcn(self.cas_dcnpack, feat, offset, 0.1)

    def forward_cb8(self, nbr, ref):
        """The two pyramids as lists of CB8 tensors (L1, L2, L3) -> the aligned L1 features, CB8."""
        return self._layers(_FP32, nbr, ref)

    def forward_cb16(self, nbr, ref):
        """The same on hip_ops.CB16 windows (bf16 inference): the pyramids as lists of CB16 -> aligned L1, CB16."""
        return self._layers(_BF16, nbr, ref)

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

    def _layers(self, ops, aligned, b, t):
        conv, conv1x1 = ops.conv, ops.conv1x1
        bt, _, h, w = ops.dims(aligned)
        if bt != b * t or t != self.num_frame:
            raise ValueError(f'TSAFusion: {bt} images are not {b} x num_frame={self.num_frame}')
        if h % 4 or w % 4:
            raise ValueError(f'TSAFusion: the height and width must be multiples of 4 (got {h}x{w})')
        # per-frame weights from the correlation with the centre frame
        center = ops.center(aligned, b, t, self.center_frame_idx)
        embedding_ref = conv(self.temporal_attn1, center, 1.0)
        embedding = conv(self.temporal_attn2, aligned, 1.0)
        fused = ops.tsa_corr(embedding, embedding_ref, aligned, t)   # (b, t*c): aligned * sigmoid(correlation)
        feat = conv1x1(self.feat_fusion, fused)
        # attention branch, half resolution
        attn = conv1x1(self.spatial_attn1, fused)
        attn = conv1x1(self.spatial_attn2, ops.pool(attn))
        # quarter resolution and back
        attn_level = conv1x1(self.spatial_attn_l1, attn)
        attn_level = conv(self.spatial_attn_l2, ops.pool(attn_level))
        attn_level = ops.up2(conv(self.spatial_attn_l3, attn_level))
        attn = ops.conv_add(self.spatial_attn3, attn, attn_level)
        attn = ops.up2(conv1x1(self.spatial_attn4, attn))
        attn = conv(self.spatial_attn5, attn, 1.0)
        attn_add = conv1x1(self.spatial_attn_add2, conv1x1(self.spatial_attn_add1, attn), 1.0)
        # sigmoid(attn) * 2 is about 1 for a freshly initialised branch (attn near 0), so the gate starts as the identity
        return ops.tsa_gate(feat, attn, attn_add)

    def forward_cb8(self, aligned, b, t):
        return self._layers(_FP32, aligned, b, t)

    def forward_cb16(self, aligned, b, t):
        """The same on hip_ops.CB16 windows (bf16 inference); ``aligned``: a whole CB16 tensor of b * t images."""
        return self._layers(_BF16, aligned, b, t)

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

    def _layers(self, ops, x):
        conv_s2, resblock = ops.conv_s2, ops.resblock
        self._check_size(*ops.dims(x)[2:])
        feat_l1 = ops.conv(self.conv_first, x)
        if self.hr_in:
            feat_l1 = conv_s2(self.stride_conv_hr1, feat_l1)
            feat_l1 = conv_s2(self.stride_conv_hr2, feat_l1)
        feat_l2 = conv_s2(self.stride_conv_l2, feat_l1)
        feat_l3 = conv_s2(self.stride_conv_l3, feat_l2)

        # each coarser level is upsampled and added to the next finer one after that level's first block(s)
        feat_l3 = ops.up2(resblock(self.resblock_l3, feat_l3))
        feat_l2 = resblock(self.resblock_l2_1, feat_l2, feat_l3)
        feat_l2 = ops.up2(resblock(self.resblock_l2_2, feat_l2))

        for i, blk in enumerate(self.resblock_l1):
            feat_l1 = resblock(blk, feat_l1, feat_l2 if i == 1 else None)
        return feat_l1

    def forward_cb8(self, x):
        return self._layers(_FP32, x)

    def forward_cb16(self, x):
        """The same on hip_ops.CB16 windows (bf16 inference); the two additions run in the epilogue of the preceding residual
        block's second conv."""
        return self._layers(_BF16, x)

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

    def set_deterministic(self, flag=True):
        """This project's own switch: every deformable conv of the network takes the bit-reproducible input gradient
        (include/sr_hip_dcn_det.h), after which two backward passes of the fp32 network agree bit for bit.  Off by default.  With
        compute_dtype='bf16' the flag is accepted and does nothing: that path is forward only.  Returns self."""
        return _set_deterministic(self, flag)

    def _align(self, ops, feat_l, b, t):
        ref_l = [ops.center_over_t(f, b, t, self.center_frame_idx) for f in feat_l]
        return self.pcd_align._layers(ops, feat_l, ref_l)

    def align_cb8(self, feat_l, b, t):
        """PCD alignment of every frame to the centre frame in one batched call: ``feat_l`` = the pyramid (L1, L2, L3) of the
        b * t frames, CB8; the centre frame's pyramid is expanded over t."""
        return self._align(_FP32, feat_l, b, t)

    def _run(self, x, ops):
        """The layer list; fp32 NCHW in and out, ``ops`` activations in between."""
        conv, resblock = ops.conv, ops.resblock
        b, t, c, h, w = x.shape
        x_center = x[:, self.center_frame_idx].contiguous()
        frames = ops.enter(x.reshape(b * t, c, h, w))

        # level-1 features of every frame
        if self.with_predeblur:
            feat_l1 = ops.conv1x1(self.conv_1x1, self.predeblur._layers(ops, frames), 1.0)
        else:
            feat_l1 = conv(self.conv_first, frames)
        for blk in self.feature_extraction:
            feat_l1 = resblock(blk, feat_l1)
        feat_l2 = conv(self.conv_l2_2, ops.conv_s2(self.conv_l2_1, feat_l1))
        feat_l3 = conv(self.conv_l3_2, ops.conv_s2(self.conv_l3_1, feat_l2))

        # PCD alignment, all frames at once
        aligned = self._align(ops, [feat_l1, feat_l2, feat_l3], b, t)

        if self.with_tsa:
            out = self.fusion._layers(ops, aligned, b, t)
        else:
            out = ops.conv1x1(self.fusion, ops.frames_to_channels(aligned, b, t), 1.0)
        for blk in self.reconstruction:
            out = resblock(blk, out)
        # the LeakyReLU after each pixel shuffle commutes with it: it runs in the upconv's epilogue
        out = ops.pixel_shuffle(conv(self.upconv1, out), self.num_feat, 2)
        out = ops.pixel_shuffle(conv(self.upconv2, out), 64, 2)
        out = conv(self.conv_hr, out)
        out = ops.conv_nchw(self.conv_last, out)
        if self.hr_in:
            return A.AddFn.apply(out, x_center)
        return A.BilinearUpFn.apply(x_center, 4, out)

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
                return self._run(x, _BF16)
        return self._run(x, _FP32)
