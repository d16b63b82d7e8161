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
import torch
from torch import nn

from .. import hip_ops
from ..utils.registry import ARCH_REGISTRY
from .arch_util import Conv3x3Params, ResidualBlockNoBN, make_layer, upscale_stages
from .hip_generator import F32, HipGenerator, residual_block, upsample_stage


class Upsample(nn.Sequential):
    """Parameters of the reference's Upsample (arch_util.py:90-109): conv nf -> 4nf + PixelShuffle(2), log2(scale) times, or
    conv nf -> 9nf + PixelShuffle(3).  The PixelShuffle entries only keep the reference's ``upsample.{0,2,..}`` numbering."""

    def __init__(self, scale, num_feat):
        factors = upscale_stages(scale)
        if factors is None:
            raise ValueError(f'scale {scale} is not supported. Supported scales: 2^n and 3.')
        m = []
        for r in factors:
            m += [Conv3x3Params(num_feat, r * r * num_feat), nn.PixelShuffle(r)]
        super().__init__(*m)

    def stages(self):
        """(conv, r) of the stages in forward order."""
        mods = list(self)
        return [(mods[i], mods[i + 1].upscale_factor) for i in range(0, len(mods), 2)]

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('Upsample is a parameter container; EDSR launches the HIP kernels')


@ARCH_REGISTRY.register()
class EDSR(HipGenerator):
    """EDSR(num_in_ch, num_out_ch, num_feat=64, num_block=16, upscale=4, res_scale=1, img_range=255.,
    rgb_mean=(0.4488, 0.4371, 0.4040)[, compute_dtype='fp32']).

    forward(x [N, 3, H, W] fp32 on a HIP device) -> [N, 3, upscale*H, upscale*W] fp32.  ``upscale``: 2^n or 3 (ValueError
    otherwise, as the reference).  num_in_ch and num_out_ch must be 3 (the reference's ``mean.view(1, 3, 1, 1)``).  ``num_feat``
    must be a positive multiple of 8 (fp32, CB8 activations) or of 16 (bf16, CB16), so that no pad channel sits between layers.
    ``compute_dtype='bf16'``: forward only (eval mode or no_grad): bf16 activations and weight images rounded from the fp32
    parameters, fp32 accumulation and epilogues, fp32 output."""

    _in_channels = 3

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

    # ------------------------------------------------------------------ HIP plumbing
    def ups(self):
        """(conv, r) of the upsampling stages, in forward order."""
        return self.upsample.stages()

    def _autograd_apply(self, x):
        from .edsr_autograd import edsr_apply
        return edsr_apply(self, x)

    def run_forward(self, x, keep=False, ops=F32):
        """The forward as per-layer launches on the current stream, on CB8 fp32 (``F32``) or CB16 bf16 (``BF16``) activations
        with every epilogue in fp32; conv_last stores fp32 NCHW.  ``keep`` (fp32 only): also return what the backward reads (CB8
        activations: the shifted input, conv_first output, per block the ReLU output and the block output, the trunk output,
        per upsampling stage the shuffled output)."""
        assert not (keep and ops.bf16), 'the backward reads fp32 activations'
        n, _, h, w = x.shape
        s = self.upscale

        def pk(conv):
            return self.packed(conv, 0, ops.bf16)

        with torch.cuda.device(x.device):
            xc = hip_ops.edsr_shift_in(x, self._mean3, self.img_range, bf16=ops.bf16)
            feat0 = feat = ops.conv3x3(xc, pk(self.conv_first))
            saved = dict(x=xc, feat0=feat0, blocks=[], ups=[]) if keep else None
            for blk in self.body:
                t, feat = residual_block(self, feat, blk, ops)
                if keep:
                    saved['blocks'].append((t, feat))
            feat = ops.conv3x3(feat, pk(self.conv_after_body), res1=feat0, beta1=1.0)
            if keep:
                saved['trunk'] = feat
            for conv, r in self.ups():
                feat = upsample_stage(self, feat, conv, r, ops)
                if keep:
                    saved['ups'].append(feat)
            y = torch.empty((n, 3, h * s, w * s), dtype=torch.float32, device=x.device)
            ops.conv3x3(feat, pk(self.conv_last), out_nchw=y)
            hip_ops.edsr_shift_out(y, self._mean3, self.img_range)
        return y, saved
