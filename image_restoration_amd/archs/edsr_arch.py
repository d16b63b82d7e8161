"""EDSR (x2^n / x3) on the MI355X HIP path: fp32 training and inference, bf16 inference.

Same constructor, forward contract, state_dict keys and initialisation as the reference ``basicsr/archs/edsr_arch.py:9-61``, so
``network_g: {type: EDSR, ...}`` option blocks and BasicSR checkpoints drop in; ``compute_dtype`` is this project's own key.
The modules only hold parameters; the network is a composition of per-layer launches:

    (x - mean) * img_range   sr_edsr_shift_in_f32 / _bf16 (NCHW -> one channel block; before conv_first's zero padding)
    conv_first               sr_conv3x3_f32 / sr_conv3x3_bf16, no activation
    body.{i}                 conv1 with ReLU (act_slope 0); conv2 with the residual x + res_scale*conv in the epilogue
    conv_after_body          the conv_first output added in the epilogue (res1)
    upsample.0[, .2, ...]    conv, then sr_cb8_pixel_shuffle_f32 / sr_cb16_pixel_shuffle_bf16 (no activation)
    conv_last                storing NCHW fp32, then sr_edsr_shift_out_f32 (y / img_range + mean) in place

Training (fp32) goes through one autograd function for the whole network (edsr_autograd.py).
"""
import math

import torch
from torch import nn

from .. import _lib, hip_ops
from ..utils.registry import ARCH_REGISTRY
from .arch_util import Conv3x3Params, ResidualBlockNoBN, make_layer


class Upsample(nn.Sequential):
    """Parameters of the reference's Upsample (arch_util.py:90-109): conv nf -> 4nf + PixelShuffle(2), log2(scale) times, or
    conv nf -> 9nf + PixelShuffle(3).  The PixelShuffle entries only keep the reference's ``upsample.{0,2,..}`` numbering."""

    def __init__(self, scale, num_feat):
        m = []
        if isinstance(scale, int) and scale >= 1 and (scale & (scale - 1)) == 0:
            for _ in range(int(math.log2(scale))):
                m += [Conv3x3Params(num_feat, 4 * num_feat), nn.PixelShuffle(2)]
        elif scale == 3:
            m += [Conv3x3Params(num_feat, 9 * num_feat), nn.PixelShuffle(3)]
        else:
            raise ValueError(f'scale {scale} is not supported. Supported scales: 2^n and 3.')
        super().__init__(*m)

    def stages(self):
        """(conv, r) of the stages in forward order."""
        mods = list(self)
        return [(mods[i], mods[i + 1].upscale_factor) for i in range(0, len(mods), 2)]

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('Upsample is a parameter container; EDSR launches the HIP kernels')


@ARCH_REGISTRY.register()
class EDSR(nn.Module):
    """EDSR(num_in_ch, num_out_ch, num_feat=64, num_block=16, upscale=4, res_scale=1, img_range=255.,
    rgb_mean=(0.4488, 0.4371, 0.4040)[, compute_dtype='fp32']).

    forward(x [N, 3, H, W] fp32 on a HIP device) -> [N, 3, upscale*H, upscale*W] fp32.  ``upscale``: 2^n or 3 (ValueError
    otherwise, as the reference).  num_in_ch and num_out_ch must be 3 (the reference's ``mean.view(1, 3, 1, 1)``).  ``num_feat``
    must be a positive multiple of 8 (fp32, CB8 activations) or of 16 (bf16, CB16), so that no pad channel sits between layers.
    ``compute_dtype='bf16'``: forward only (eval mode or no_grad): bf16 activations and weight images rounded from the fp32
    parameters, fp32 accumulation and epilogues, fp32 output."""

    def __init__(self, num_in_ch, num_out_ch, num_feat=64, num_block=16, upscale=4, res_scale=1, img_range=255.,
                 rgb_mean=(0.4488, 0.4371, 0.4040), compute_dtype='fp32'):
        super().__init__()
        if num_in_ch != 3 or num_out_ch != 3:
            raise ValueError(f'EDSR shifts by a 3-channel mean: num_in_ch and num_out_ch must be 3, got {num_in_ch!r}, {num_out_ch!r}')
        if len(rgb_mean) != 3:
            raise ValueError(f'rgb_mean must have 3 entries, got {len(rgb_mean)}')
        if compute_dtype not in ('fp32', 'bf16'):
            raise ValueError(f"compute dtype must be 'fp32' or 'bf16', got {compute_dtype!r}")
        grid = 16 if compute_dtype == 'bf16' else 8
        if not isinstance(num_feat, int) or num_feat <= 0 or num_feat % grid:
            raise ValueError(f'EDSR in {compute_dtype} needs num_feat to be a positive multiple of {grid}, got {num_feat!r}')
        if num_block < 0:
            raise ValueError(f'num_block must be >= 0, got {num_block!r}')
        if float(img_range) == 0.0:
            raise ValueError('img_range must not be 0')
        self.upscale, self.num_feat, self.num_block = upscale, num_feat, num_block
        self.num_in_ch, self.num_out_ch = num_in_ch, num_out_ch
        self.compute_dtype = compute_dtype
        self.img_range = img_range
        self.mean = torch.Tensor(rgb_mean).view(1, 3, 1, 1)   # a plain attribute, as in the reference (not in the state dict)
        self._mean3 = tuple(float(v) for v in torch.tensor(rgb_mean, dtype=torch.float32))

        self.conv_first = Conv3x3Params(num_in_ch, num_feat)
        self.body = make_layer(ResidualBlockNoBN, num_block, num_feat=num_feat, res_scale=res_scale, pytorch_init=True)
        self.conv_after_body = Conv3x3Params(num_feat, num_feat)
        self.upsample = Upsample(upscale, num_feat)
        self.conv_last = Conv3x3Params(num_feat, num_out_ch)
        self._packs = {}
        self._pack_gen = 0
        self._grad_sink = None  # set by optim.FlatAdam: weight gradients are added straight into its arena

    # ------------------------------------------------------------------ HIP plumbing
    def ups(self):
        """(conv, r) of the upsampling stages, in forward order."""
        return self.upsample.stages()

    def convs(self):
        """Every conv in state_dict order."""
        out = [self.conv_first]
        for blk in self.body:
            out += [blk.conv1, blk.conv2]
        return out + [self.conv_after_body] + [c for c, _ in self.ups()] + [self.conv_last]

    def _param_list(self):
        """Parameters in state_dict order (weight, bias per conv)."""
        return [t for c in self.convs() for t in (c.weight, c.bias)]

    def invalidate_packed(self):
        """Call after parameter memory was written behind torch's version counters (fused Adam, EMA, a broadcast)."""
        self._pack_gen += 1

    def packed(self, conv, mode=0, bf16=False):
        """Weight image of ``conv`` (mode 0: forward, 1: data gradient; bf16: the CB16 image rounded from the fp32 parameter),
        rebuilt when the parameter storage, its version, the FlatAdam epoch of the parameter or this net's generation
        (invalidate_packed) changed."""
        w, b = conv.weight, conv.bias
        sig = (w.data_ptr(), w._version, getattr(w, '_sr_epoch', (0,))[0], b.data_ptr(), b._version, self._pack_gen)
        key = (id(conv), mode, bf16)
        hit = self._packs.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1]
        if w.dtype != torch.float32 or b.dtype != torch.float32:
            raise _lib.SrHipError('EDSR parameters must be fp32')
        cls = hip_ops.PackedConvBF16 if bf16 else hip_ops.PackedConv
        pc = cls(w, b if mode == 0 else None, mode=mode)
        self._packs[key] = (sig, pc)
        return pc

    def _apply(self, fn, *args, **kwargs):
        self._packs = {}
        return super()._apply(fn, *args, **kwargs)

    def run_forward(self, x, keep=False):
        """The fp32 forward as per-layer launches on the current stream.  ``keep``: also return what the backward reads (CB8
        activations: the shifted input, conv_first output, per block the ReLU output and the block output, the trunk output,
        per upsampling stage the shuffled output)."""
        n, _, h, w = x.shape
        s, nf = self.upscale, self.num_feat
        with torch.cuda.device(x.device):
            xc = hip_ops.edsr_shift_in(x, self._mean3, self.img_range)
            feat0 = feat = hip_ops.conv3x3(xc, self.packed(self.conv_first))
            saved = dict(x=xc, feat0=feat0, blocks=[], ups=[]) if keep else None
            for blk in self.body:
                t = hip_ops.conv3x3(feat, self.packed(blk.conv1), act_slope=0.0)
                feat = hip_ops.conv3x3(t, self.packed(blk.conv2), alpha=float(blk.res_scale), res1=feat, beta1=1.0)
                if keep:
                    saved['blocks'].append((t, feat))
            feat = hip_ops.conv3x3(feat, self.packed(self.conv_after_body), res1=feat0, beta1=1.0)
            if keep:
                saved['trunk'] = feat
            for conv, r in self.ups():
                u = hip_ops.conv3x3(feat, self.packed(conv))
                feat = hip_ops.pixel_shuffle(u, nf, r)
                del u
                if keep:
                    saved['ups'].append(feat)
            y = torch.empty((n, 3, h * s, w * s), dtype=torch.float32, device=x.device)
            hip_ops.conv3x3(feat, self.packed(self.conv_last), out_nchw=y)
            hip_ops.edsr_shift_out(y, self._mean3, self.img_range)
        return y, saved

    def run_forward_bf16(self, x):
        """The bf16 forward: CB16 activations on sr_conv3x3_bf16, every epilogue in fp32; conv_last stores fp32 NCHW."""
        n, _, h, w = x.shape
        s, nf = self.upscale, self.num_feat

        def pk(conv):
            return self.packed(conv, 0, True)

        with torch.cuda.device(x.device):
            xc = hip_ops.edsr_shift_in(x, self._mean3, self.img_range, bf16=True)
            feat0 = feat = hip_ops.conv3x3_bf16(xc, pk(self.conv_first))
            for blk in self.body:
                t = hip_ops.conv3x3_bf16(feat, pk(blk.conv1), act_slope=0.0)
                feat = hip_ops.conv3x3_bf16(t, pk(blk.conv2), alpha=float(blk.res_scale), res1=feat, beta1=1.0)
            feat = hip_ops.conv3x3_bf16(feat, pk(self.conv_after_body), res1=feat0, beta1=1.0)
            for conv, r in self.ups():
                u = hip_ops.conv3x3_bf16(feat, pk(conv))
                feat = hip_ops.pixel_shuffle_bf16(u, nf, r)
                del u
            y = torch.empty((n, 3, h * s, w * s), dtype=torch.float32, device=x.device)
            hip_ops.conv3x3_bf16(feat, pk(self.conv_last), out_nchw=y)
            hip_ops.edsr_shift_out(y, self._mean3, self.img_range)
        return y

    def forward(self, x):
        if not x.is_cuda:
            raise _lib.SrHipError('EDSR.forward runs only on a HIP device (no CPU fallback): move the module and input '
                                  'with .to("cuda")')
        if x.dim() != 4 or x.size(1) != 3:
            raise ValueError(f'expected [N, 3, H, W], got {tuple(x.shape)}')
        x = x.contiguous().float()
        needs_graph = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self._param_list()))
        if self.compute_dtype == 'bf16':
            if needs_graph and self.training:
                raise NotImplementedError("EDSR with compute_dtype='bf16' is forward only (eval mode or torch.no_grad()); "
                                          "train with compute_dtype='fp32'")
            return self.run_forward_bf16(x)
        if needs_graph:
            from .edsr_autograd import edsr_apply
            return edsr_apply(self, x)
        return self.run_forward(x)[0]
