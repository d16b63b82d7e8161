"""DUF, the dynamic-upsampling-filter video super-resolver of the reference (``basicsr/archs/duf_arch.py``), on libsr_hip.so.
Inference only, fp32, eval mode.

Same constructors, state_dict keys, order and shapes as the reference (real ``nn.Conv3d`` / ``nn.BatchNorm3d`` modules at the
reference's ``Sequential`` indices, every ``num_batches_tracked`` included) and PyTorch's default initialisation, so a reference
checkpoint loads with ``strict=True`` and a seeded fresh network has the reference's draws.  The modules only hold parameters; a
forward is a composition of launches (include/sr_hip_duf.h, include/sr_hip_ridnet.h) on frame-major CB8 clips
``[b][T][C/8][h][w][8]``:

    conv3d1 (1,3,3) 3 -> 64              sr_duf_conv3d_f32 on the clip as one 3-channel block per frame, into the concat buffer
    per dense block (C -> C -> g)        sr_duf_pw_f32 on the channel prefix of the concat buffer: BatchNorm -> ReLU in front as
                                         the prologue, the BatchNorm behind folded into weight and bias, ReLU in the epilogue;
                                         sr_duf_conv3d_f32 (3,3,3) writes its g couts at channel C of the same buffer
    the three temporal-reduce blocks     the same two launches without temporal padding: the destination is the same buffer
                                         one frame further on, which is cat(x[:, :, 1:-1], conv(x))
    bn3d2 -> ReLU -> conv3d2 -> ReLU     sr_duf_conv3d_f32 (1,3,3) on the centre frame with the prologue
    conv3d_r1 / r2, conv3d_f1 / f2       sr_convd_f32, ksize 1
    softmax, 5x5 filter, + res, shuffle  sr_duf_filter_f32

The concat buffer is allocated once at the final channel count, so no concatenation copies anything.  BatchNorm runs in eval
mode only: the one in front of a convolution becomes ``scale = gamma / sqrt(var + eps)``, ``shift = beta - mean * scale``
(float64 on the host, rounded once: ``arch_util.bn_prologue``), the one behind the 1x1x1 convolution is folded
(``arch_util.fold_batchnorm`` with the bias).  Packed weights, folds and prologue arrays are cached by ``HipGenerator.derived`` on
storage pointer, version and FlatAdam epoch of every tensor they are made from, so an in-place edit of ``running_var`` is seen by
the next forward.

ValueError for a clip that is not ``[b, 7, 3, h, w]`` fp32 (the temporal arithmetic 7 -> 7 -> 5 -> 3 -> 1 fixes 7 frames);
NotImplementedError in training mode (even under ``torch.no_grad()``) and when a graph would be needed; ``_lib.SrHipError`` for
CPU tensors.  Training, bf16 and a Vimeo90K dataset are not built.
"""
import numpy as np
import torch
from torch import nn

from .. import hip_ops
from ..utils.registry import ARCH_REGISTRY
from .arch_util import bn_prologue, fold_batchnorm, refuse_inference_only  # noqa: F401  (bn_prologue: its old home)
from .hip_generator import HipGenerator


def _bn_args(adapt_official_weights):
    return dict(eps=1e-3, momentum=1e-3) if adapt_official_weights else dict(eps=1e-05, momentum=0.1)


def _dense_layers(cin, num_grow_ch, pad_t, bn):
    """[BN, ReLU, conv 1x1x1 (cin -> cin), BN, ReLU, conv (3,3,3) (cin -> num_grow_ch)]: indices 0, 2, 3, 5 hold parameters."""
    return nn.Sequential(
        nn.BatchNorm3d(cin, **bn), nn.ReLU(inplace=True),
        nn.Conv3d(cin, cin, (1, 1, 1), stride=(1, 1, 1), padding=(0, 0, 0), bias=True),
        nn.BatchNorm3d(cin, **bn), nn.ReLU(inplace=True),
        nn.Conv3d(cin, num_grow_ch, (3, 3, 3), stride=(1, 1, 1), padding=(pad_t, 1, 1), bias=True))


class DenseBlocksTemporalReduce(nn.Module):
    """Parameters of the three dense blocks that take two frames off each (7 -> 1).  No forward: DUF issues the launches."""

    def __init__(self, num_feat=64, num_grow_ch=32, adapt_official_weights=False):
        super().__init__()
        bn = _bn_args(adapt_official_weights)
        self.temporal_reduce1 = _dense_layers(num_feat, num_grow_ch, 0, bn)
        self.temporal_reduce2 = _dense_layers(num_feat + num_grow_ch, num_grow_ch, 0, bn)
        self.temporal_reduce3 = _dense_layers(num_feat + 2 * num_grow_ch, num_grow_ch, 0, bn)

    def blocks(self):
        return [self.temporal_reduce1, self.temporal_reduce2, self.temporal_reduce3]

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('DenseBlocksTemporalReduce is a parameter container; DUF launches the HIP kernels')


class DenseBlocks(nn.Module):
    """Parameters of ``num_block`` dense blocks (DUF-16: 3, DUF-28: 9, DUF-52: 21).  No forward: DUF issues the launches."""

    def __init__(self, num_block, num_feat=64, num_grow_ch=16, adapt_official_weights=False):
        super().__init__()
        bn = _bn_args(adapt_official_weights)
        self.dense_blocks = nn.ModuleList()
        for i in range(0, num_block):
            self.dense_blocks.append(_dense_layers(num_feat + i * num_grow_ch, num_grow_ch, 1, bn))

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('DenseBlocks is a parameter container; DUF launches the HIP kernels')


class DynamicUpsamplingFilter(nn.Module):
    """The dynamic upsampling filter: ``forward(x, filters)`` with x [n, 3, h, w] and already-normalised filters
    [n, 25, s*s, h, w] (s in 2, 3, 4) -> [n, 3*s*s, h, w], the same filters on the three colours — one sr_duf_filter_f32 launch
    without softmax, residual or shuffle.  Only (5, 5) is built."""

    def __init__(self, filter_size=(5, 5)):
        super().__init__()
        if not isinstance(filter_size, tuple):
            raise TypeError('The type of filter_size must be tuple, ' f'but got type{filter_size}')
        if len(filter_size) != 2:
            raise ValueError('The length of filter size must be 2, ' f'but got {len(filter_size)}.')
        if filter_size != (5, 5):
            raise NotImplementedError(f'DynamicUpsamplingFilter: only the (5, 5) filter of DUF is built, got {filter_size}')
        self.filter_size = filter_size

    def forward(self, x, filters):
        if x.dim() != 4 or x.size(1) != 3 or x.dtype != torch.float32 or x.numel() == 0:
            raise ValueError(f'DynamicUpsamplingFilter: expected an fp32 [n, 3, h, w] image, got {x.dtype} {tuple(x.shape)}')
        n, _, h, w = x.shape
        if filters.dim() != 5 or filters.dtype != torch.float32 or tuple(filters.shape[:2]) != (n, 25) \
                or filters.size(2) not in (4, 9, 16) or tuple(filters.shape[3:]) != (h, w):
            raise ValueError(f'DynamicUpsamplingFilter: expected fp32 [{n}, 25, 4 | 9 | 16, {h}, {w}] filters, got {filters.dtype} '
                             f'{tuple(filters.shape)}')
        refuse_inference_only('DynamicUpsamplingFilter', False, (x, filters), (), 'applied from')
        with torch.no_grad():
            s2 = filters.size(2)
            logits = hip_ops.nchw_to_cb8(filters.reshape(n, 25 * s2, h, w))
            return hip_ops.duf_filter(logits, x.contiguous(), int(round(s2 ** 0.5)), softmax=False, shuffle=False)


@ARCH_REGISTRY.register()
class DUF(HipGenerator):
    """DUF: [b, 7, 3, h, w] LR frames -> the super-resolved centre frame [b, 3, s*h, s*w].  ``num_layer`` 16, 28 or 52;
    ``adapt_official_weights``: BatchNorm eps = momentum = 1e-3, for weights translated from the official implementation."""

    def __init__(self, scale=4, num_layer=52, adapt_official_weights=False):
        super().__init__()
        self.scale = scale
        bn = _bn_args(adapt_official_weights)
        self.conv3d1 = nn.Conv3d(3, 64, (1, 3, 3), stride=(1, 1, 1), padding=(0, 1, 1), bias=True)
        self.dynamic_filter = DynamicUpsamplingFilter((5, 5))
        if num_layer == 16:
            num_block, num_grow_ch = 3, 32
        elif num_layer == 28:
            num_block, num_grow_ch = 9, 16
        elif num_layer == 52:
            num_block, num_grow_ch = 21, 16
        else:
            raise ValueError(f'Only supported (16, 28, 52) layers, but got {num_layer}.')
        self.num_layer, self.num_block, self.num_grow_ch = num_layer, num_block, num_grow_ch
        self.dense_block1 = DenseBlocks(num_block=num_block, num_feat=64, num_grow_ch=num_grow_ch,
                                        adapt_official_weights=adapt_official_weights)
        self.dense_block2 = DenseBlocksTemporalReduce(64 + num_grow_ch * num_block, num_grow_ch,
                                                      adapt_official_weights=adapt_official_weights)
        channels = 64 + num_grow_ch * num_block + num_grow_ch * 3
        self.channels = channels
        self.bn3d2 = nn.BatchNorm3d(channels, **bn)
        self.conv3d2 = nn.Conv3d(channels, 256, (1, 3, 3), stride=(1, 1, 1), padding=(0, 1, 1), bias=True)
        self.conv3d_r1 = nn.Conv3d(256, 256, (1, 1, 1), stride=(1, 1, 1), padding=(0, 0, 0), bias=True)
        self.conv3d_r2 = nn.Conv3d(256, 3 * (scale ** 2), (1, 1, 1), stride=(1, 1, 1), padding=(0, 0, 0), bias=True)
        self.conv3d_f1 = nn.Conv3d(256, 512, (1, 1, 1), stride=(1, 1, 1), padding=(0, 0, 0), bias=True)
        self.conv3d_f2 = nn.Conv3d(512, 1 * 5 * 5 * (scale ** 2), (1, 1, 1), stride=(1, 1, 1), padding=(0, 0, 0), bias=True)

    # ---- device images, cached by HipGenerator.derived: rebuilt when a tensor they are made from changed
    def packed_conv(self, conv, bn=None):
        """The weight image of a Conv3d (hip_ops.PackedDufConv), with eval-mode ``bn`` behind it folded in."""
        tensors = (conv.weight, conv.bias) + (() if bn is None else (bn.weight, bn.bias, bn.running_mean, bn.running_var))

        def build():
            if bn is None:
                return hip_ops.PackedDufConv(conv.weight, conv.bias)
            w, b = fold_batchnorm(conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bias=conv.bias)
            dev = conv.weight.device
            return hip_ops.PackedDufConv(w.to(dev), b.to(dev))
        return self.derived((id(conv), 'conv'), tensors, None if bn is None else float(bn.eps), build)

    def packed_head(self, conv):
        """The sr_convd_f32 (ksize 1) image of one of the four 1x1x1 head convolutions."""
        w = conv.weight
        return self.derived((id(conv), 'head'), (w, conv.bias), None,
                            lambda: hip_ops.PackedConvK(w.detach().view(w.size(0), w.size(1), 1, 1), conv.bias.detach()))

    def prologue(self, bn):
        """(scale, shift) of eval-mode ``bn`` on the device."""
        dev = bn.weight.device
        return self.derived((id(bn), 'prologue'), (bn.weight, bn.bias, bn.running_mean, bn.running_var), float(bn.eps),
                            lambda: tuple(t.to(dev) for t in bn_prologue(bn)))

    def _dense(self, seq, cat, tmp, cin, pad_t):
        """One dense block on the frame windows ``cat`` / ``tmp``: channels [0, cin) of cat -> channels [cin, cin + g) of cat."""
        hip_ops.duf_pw(cat, self.packed_conv(seq[2], seq[3]), tmp, 0, relu=True, prologue=self.prologue(seq[0]))
        dst = cat if pad_t else cat.frames(1, cat.tn - 2)
        hip_ops.duf_conv3d(tmp, self.packed_conv(seq[5]), dst, cin // 8, pad_t=pad_t)
        return dst

    def run_forward(self, x, keep=None):
        """The whole forward on a contiguous fp32 device clip [b, 7, 3, h, w].  ``keep`` (a dict) receives ``logits`` and
        ``res`` as NCHW tensors."""
        b, t, _, h, w = x.shape
        dev, g, s = x.device, self.num_grow_ch, self.scale
        frames = hip_ops.ClipCB8(hip_ops.nchw_to_cb8(x.view(b * t, 3, h, w)).buf.view(b, t, 1, h, w, 8))
        cat = hip_ops.ClipCB8.empty(b, t, self.channels, h, w, dev)
        tmp = hip_ops.ClipCB8.empty(b, t, self.channels - g, h, w, dev)
        hip_ops.duf_conv3d(frames, self.packed_conv(self.conv3d1), cat, 0)
        cin = 64
        for seq in self.dense_block1.dense_blocks:
            self._dense(seq, cat, tmp, cin, 1)
            cin += g
        win, twin = cat, tmp
        for seq in self.dense_block2.blocks():
            win = self._dense(seq, win, twin, cin, 0)
            twin = twin.frames(1, twin.tn - 2)
            cin += g
        feat = hip_ops.ClipCB8.empty(b, 1, 256, h, w, dev)
        hip_ops.duf_conv3d(win, self.packed_conv(self.conv3d2), feat, 0, relu=True, prologue=self.prologue(self.bn3d2))
        feat = feat.images()
        r = hip_ops.convd(feat, self.packed_head(self.conv3d_r1), act_slope=0.0)
        res = hip_ops.convd(r, self.packed_head(self.conv3d_r2))
        f = hip_ops.convd(feat, self.packed_head(self.conv3d_f1), act_slope=0.0)
        logits = hip_ops.convd(f, self.packed_head(self.conv3d_f2))
        if keep is not None:
            keep['logits'] = hip_ops.cb_to_nchw(logits, 25 * s * s)
            keep['res'] = hip_ops.cb_to_nchw(res, 3 * s * s)
        return hip_ops.duf_filter(logits, x[:, t // 2], s, res)

    def forward(self, x, keep=None):
        if x.dim() != 5 or x.size(1) != 7 or x.size(2) != 3 or x.dtype != torch.float32 or x.numel() == 0:
            raise ValueError(f'DUF: expected an fp32 [b, 7, 3, h, w] clip (the temporal reduction 7 -> 5 -> 3 -> 1 fixes 7 frames), '
                             f'got {x.dtype} {tuple(x.shape)}')
        refuse_inference_only('DUF', self.training, (x,), self.parameters(), 'applied from')
        with torch.no_grad():
            return self.run_forward(x.contiguous(), keep)


def num_parameters(num_layer, scale):
    """Parameter count of DUF(scale, num_layer), from the layer list (a check for the tests and the docs)."""
    nb, g = {16: (3, 32), 28: (9, 16), 52: (21, 16)}[num_layer]
    n = 3 * 64 * 9 + 64
    c = 64
    for i in range(nb + 3):
        n += 2 * c + c * c + c + 2 * c + c * g * 27 + g
        c += g
    n += 2 * c + c * 256 * 9 + 256
    s2 = scale * scale
    n += 256 * 256 + 256 + 256 * 3 * s2 + 3 * s2 + 256 * 512 + 512 + 512 * 25 * s2 + 25 * s2
    return int(np.int64(n))
