"""MSRResNet (modified SRResNet, x2 / x3 / x4) on the MI355X HIP path.

Same constructor, forward contract, state_dict keys and initialisation as the reference
``basicsr/archs/srresnet_arch.py:9-68``, so ``network_g: {type: MSRResNet, ...}`` option blocks and BasicSR
checkpoints drop in.  The modules only hold parameters; the network is a composition of per-layer launches:

    conv_first          sr_conv3x3_f32, LeakyReLU(0.1) in the epilogue
    body.{i}            conv1: sr_conv3x3_f32 with ReLU (act_slope 0); conv2: the residual x + res_scale*conv in the epilogue
    upconv1[, upconv2]  sr_conv3x3_f32 with LeakyReLU(0.1), then sr_cb8_pixel_shuffle_f32 (the activation commutes with it)
    conv_hr             sr_conv3x3_f32, LeakyReLU(0.1)
    conv_last           sr_conv3x3_f32 storing NCHW, then sr_bilinear_up_f32 adds the bilinear base into that output

Training goes through one autograd function for the whole network (srresnet_autograd.py).

``compute_dtype='bf16'`` (forward only): sr_nchw_to_cb16_bf16 on the input, the same layer list on sr_conv3x3_bf16 and
sr_cb16_pixel_shuffle_bf16 (CB16 bf16 activations), conv_last storing fp32 NCHW, and the same sr_bilinear_up_f32 adding the
bilinear base of the fp32 input.
"""
import torch

from .. import hip_ops
from ..utils.registry import ARCH_REGISTRY
from .arch_util import Conv3x3Params, ResidualBlockNoBN, default_init_weights, make_layer
from .hip_generator import F32, HipGenerator, residual_block, upsample_stage

LRELU = 0.1


@ARCH_REGISTRY.register()
class MSRResNet(HipGenerator):
    """MSRResNet(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=16, upscale=4[, compute_dtype='fp32']).

    forward(x [N, num_in_ch, H, W] fp32 on a HIP device) -> [N, num_out_ch, upscale*H, upscale*W].
    ``upscale`` must be 2, 3 or 4 (ValueError otherwise; the reference silently builds a net without upsampling).
    ``num_feat`` must be a positive multiple of 8: every activation lives in whole 8-channel CB8 blocks, so no pad
    channel ever sits between two layers.  num_in_ch == num_out_ch (the bilinear base is added to the output).
    ``compute_dtype='bf16'`` (this project's own key; ValueError for anything but 'fp32' / 'bf16') needs ``num_feat`` to be a
    multiple of 16 (CB16 activations) and ``num_out_ch`` >= 1 (sr_conv3x3_bf16's fp32 NCHW store guards every output channel,
    so it takes any positive count), and is forward only (eval mode or no_grad): bf16 activations and weight images rounded
    from the fp32 parameters, fp32 accumulation, epilogues and output.
    """

    def __init__(self, num_in_ch=3, num_out_ch=3, num_feat=64, num_block=16, upscale=4, compute_dtype='fp32'):
        super().__init__()
        if compute_dtype not in ('fp32', 'bf16'):
            raise ValueError(f"compute dtype must be 'fp32' or 'bf16', got {compute_dtype!r}")
        if upscale not in (2, 3, 4):
            raise ValueError(f'MSRResNet supports upscale 2, 3 and 4, got {upscale!r}')
        if not isinstance(num_feat, int) or num_feat <= 0 or num_feat % 8:
            raise ValueError(f'MSRResNet needs num_feat to be a positive multiple of 8 (CB8 activations), got {num_feat!r}')
        if num_block < 0:
            raise ValueError(f'num_block must be >= 0, got {num_block!r}')
        if compute_dtype == 'bf16':
            if num_feat % 16:
                raise ValueError(f'MSRResNet in bf16 needs num_feat to be a multiple of 16 (CB16 activations), got {num_feat!r}')
            if not isinstance(num_out_ch, int) or num_out_ch < 1 or not isinstance(num_in_ch, int) or num_in_ch < 1:
                raise ValueError(f'MSRResNet in bf16 needs num_in_ch >= 1 and num_out_ch >= 1, got {num_in_ch!r}, {num_out_ch!r}')
        self.upscale = upscale
        self.compute_dtype = compute_dtype
        self.num_in_ch, self.num_out_ch, self.num_feat, self.num_block = num_in_ch, num_out_ch, num_feat, num_block

        self.conv_first = Conv3x3Params(num_in_ch, num_feat)
        self.body = make_layer(ResidualBlockNoBN, num_block, num_feat=num_feat)
        if upscale in (2, 3):
            self.upconv1 = Conv3x3Params(num_feat, num_feat * upscale * upscale)
        else:
            self.upconv1 = Conv3x3Params(num_feat, num_feat * 4)
            self.upconv2 = Conv3x3Params(num_feat, num_feat * 4)
        self.conv_hr = Conv3x3Params(num_feat, num_feat)
        self.conv_last = Conv3x3Params(num_feat, num_out_ch)

        default_init_weights([self.conv_first, self.upconv1, self.conv_hr, self.conv_last], 0.1)
        if upscale == 4:
            default_init_weights(self.upconv2, 0.1)

    # ------------------------------------------------------------------ HIP plumbing
    def ups(self):
        """(conv, r) of the upsampling stages, in forward order."""
        return [(self.upconv1, 2), (self.upconv2, 2)] if self.upscale == 4 else [(self.upconv1, self.upscale)]

    _in_channels = property(lambda self: self.num_in_ch)

    def _check_input(self, x):
        if self.num_in_ch != self.num_out_ch:
            raise ValueError('MSRResNet adds the bilinear upsampled input to its output: num_in_ch must equal num_out_ch')

    def _autograd_apply(self, x):
        from .srresnet_autograd import msrresnet_apply
        return msrresnet_apply(self, x)

    def run_forward(self, x, keep=False, ops=F32):
        """The forward as per-layer launches on the current stream, on CB8 fp32 (``F32``) or CB16 bf16 (``BF16``) activations
        with every epilogue in fp32.  ``keep`` (fp32 only): also return what the backward reads (CB8 activations: input,
        conv_first output, per block the ReLU output and the block output, per upsampling stage the shuffled output, conv_hr
        output)."""
        assert not (keep and ops.bf16), 'the backward reads fp32 activations'
        n, _, h, w = x.shape
        s = self.upscale

        def pk(conv):
            return self.packed(conv, 0, ops.bf16)

        with torch.cuda.device(x.device):
            xc = ops.to_cb(x)
            feat = ops.conv3x3(xc, pk(self.conv_first), act_slope=LRELU)
            saved = dict(x=xc, feat0=feat, blocks=[], ups=[]) if keep else None
            for blk in self.body:
                t, feat = residual_block(self, feat, blk, ops)
                if keep:
                    saved['blocks'].append((t, feat))
            for conv, r in self.ups():
                feat = upsample_stage(self, feat, conv, r, ops, LRELU)
                if keep:
                    saved['ups'].append(feat)
            hr = ops.conv3x3(feat, pk(self.conv_hr), act_slope=LRELU)
            if keep:
                saved['hr'] = hr
            if ops.bf16 or self.num_out_ch <= 4:   # sr_conv3x3_bf16's fp32 NCHW store takes any channel count
                y = torch.empty((n, self.num_out_ch, h * s, w * s), dtype=torch.float32, device=x.device)
                ops.conv3x3(hr, pk(self.conv_last), out_nchw=y)
            else:
                y = hip_ops.cb8_to_nchw(ops.conv3x3(hr, pk(self.conv_last)), self.num_out_ch)
            hip_ops.bilinear_up(x, s, out=y)   # out += F.interpolate(x, scale_factor=s, mode='bilinear') of the fp32 input
        return y, saved
