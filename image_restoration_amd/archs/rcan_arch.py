"""RCAN (residual channel attention network, x2^n / x3) on the MI355X HIP path.

Same constructor, forward contract, state_dict keys and initialisation as the reference ``basicsr/archs/rcan_arch.py:8-135``
(PyTorch's default init everywhere; ``mean`` is a plain attribute, not a buffer), so ``network_g: {type: RCAN, ...}`` option
blocks and the official checkpoints load with strict=True.  The modules only hold parameters; the network is a composition of
per-layer launches:

    (x - mean) * img_range          sr_channel_affine_f32 (NCHW), then the CB8 conversion
    conv_first                      sr_conv3x3_f32
    per RCAB                        conv 0: sr_conv3x3_f32 with ReLU (act_slope 0); conv 2: sr_conv3x3_f32;
                                    channel attention: sr_ca_squeeze_f32 (pool + 64->4->64 MLP), sr_ca_excite_f32
                                    (x + res_scale * u * s)
    body.{g}.conv                   sr_conv3x3_f32 with res1 = the group input
    conv_after_body                 sr_conv3x3_f32 with res1 = conv_first's output
    upsample                        per stage sr_conv3x3_f32, then sr_cb8_pixel_shuffle_f32
    conv_last, / img_range + mean   sr_conv3x3_f32 storing NCHW, then sr_channel_affine_f32

Training goes through one autograd function for the whole network (rcan_autograd.py).

``compute_dtype='bf16'`` (forward only) keeps every activation in CB16 bf16 between the input shift and conv_last:

    (x - mean) * img_range          sr_edsr_shift_in_bf16 (the same arithmetic; NCHW fp32 -> one CB16 block)
    conv_first, rcab.0, rcab.2      sr_conv3x3_bf16 (act_slope 0 for the ReLU)
    channel attention               sr_ca_squeeze_bf16 (fp32 pool + MLP on the fp32 parameters), sr_ca_excite_bf16
    body.{g}.conv, conv_after_body  sr_conv3x3_bf16 with res1, beta1 = 1
    upsample                        per stage sr_conv3x3_bf16, then sr_cb16_pixel_shuffle_bf16
    conv_last, / img_range + mean   sr_conv3x3_bf16 storing fp32 NCHW, then sr_edsr_shift_out_f32 in place
"""
import torch
from torch import nn

from .. import hip_ops
from ..utils.registry import ARCH_REGISTRY
from .arch_util import Conv3x3Params, make_layer, upscale_stages
from .hip_generator import F32, HipGenerator, upsample_stage


class ChannelAttentionParams(nn.Module):
    """Parameters of the reference's ChannelAttention (rcan_arch.py:8-24): ``attention.1`` = Conv2d(nf, nf // sf, 1) and
    ``attention.3`` = Conv2d(nf // sf, nf, 1), both with bias and PyTorch's default init; indices 0, 2 and 4 (pool, ReLU,
    sigmoid) hold nothing.  The kernels read the [hid][nf][1][1] / [nf][hid][1][1] tensors as they are, so an optimiser step
    needs no repacking."""

    def __init__(self, num_feat, squeeze_factor=16):
        super().__init__()
        hid = num_feat // squeeze_factor
        self.attention = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(num_feat, hid, 1), nn.ReLU(inplace=True),
                                       nn.Conv2d(hid, num_feat, 1), nn.Sigmoid())

    @property
    def fc1(self):
        return self.attention[1]

    @property
    def fc2(self):
        return self.attention[3]

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('ChannelAttentionParams is a parameter container; RCAN launches the HIP kernels')


class RCABParams(nn.Module):
    """Parameters of ``x + res_scale * CA(conv(relu(conv(x))))`` (rcan_arch.py:27-46): keys ``rcab.{0,2}`` (3x3 convs) and
    ``rcab.3.attention.{1,3}``."""

    def __init__(self, num_feat, squeeze_factor=16, res_scale=1):
        super().__init__()
        self.res_scale = res_scale
        self.rcab = nn.Sequential(Conv3x3Params(num_feat, num_feat), nn.ReLU(True), Conv3x3Params(num_feat, num_feat),
                                  ChannelAttentionParams(num_feat, squeeze_factor))

    conv1 = property(lambda s: s.rcab[0])
    conv2 = property(lambda s: s.rcab[2])
    ca = property(lambda s: s.rcab[3])

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('RCABParams is a parameter container; RCAN launches the HIP kernels')


class ResidualGroupParams(nn.Module):
    """``num_block`` RCABs (``residual_group.{b}``), then a 3x3 conv (``conv``), plus the group input (rcan_arch.py:49-68)."""

    def __init__(self, num_feat, num_block, squeeze_factor=16, res_scale=1):
        super().__init__()
        self.residual_group = make_layer(RCABParams, num_block, num_feat=num_feat, squeeze_factor=squeeze_factor,
                                         res_scale=res_scale)
        self.conv = Conv3x3Params(num_feat, num_feat)

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('ResidualGroupParams is a parameter container; RCAN launches the HIP kernels')


@ARCH_REGISTRY.register()
class RCAN(HipGenerator):
    """RCAN(num_in_ch, num_out_ch, num_feat=64, num_group=10, num_block=16, squeeze_factor=16, upscale=4, res_scale=1,
    img_range=255., rgb_mean=(0.4488, 0.4371, 0.4040)[, compute_dtype='fp32']).

    forward(x [N, 3, H, W] fp32 on a HIP device) -> [N, 3, upscale*H, upscale*W].  ValueError for: ``upscale`` not 2^n (n >= 1)
    or 3; ``num_feat`` not a positive multiple of 8 (CB8 activations) or above 512; ``num_feat // squeeze_factor < 1``;
    ``num_in_ch`` or ``num_out_ch`` other than 3 (the reference's mean only broadcasts over 3 channels); ``num_group`` or
    ``num_block`` below 1; a ``compute_dtype`` other than 'fp32' / 'bf16'.  ``compute_dtype='bf16'`` (this project's own key) needs
    ``num_feat`` to be a multiple of 16 (CB16 activations) and is forward only (eval mode or no_grad): bf16 activations and
    weight images rounded from the fp32 parameters, fp32 accumulation, epilogues, attention MLP and output.
    """

    _in_channels = property(lambda self: self.num_in_ch)

    def __init__(self, num_in_ch, num_out_ch, num_feat=64, num_group=10, num_block=16, squeeze_factor=16, upscale=4,
                 res_scale=1, img_range=255., rgb_mean=(0.4488, 0.4371, 0.4040), compute_dtype='fp32'):
        super().__init__()
        if compute_dtype not in ('fp32', 'bf16'):
            raise ValueError(f"compute dtype must be 'fp32' or 'bf16', got {compute_dtype!r}")
        self.stages = upscale_stages(upscale) if isinstance(upscale, int) and not isinstance(upscale, bool) else None
        if not self.stages:   # None, or no stage at all (upscale 1)
            raise ValueError(f'RCAN supports upscale 2^n (n >= 1) and 3, got {upscale!r}')
        if not isinstance(num_feat, int) or num_feat <= 0 or num_feat % 8 or num_feat > 512:
            raise ValueError(f'RCAN needs num_feat to be a positive multiple of 8 up to 512 (CB8 activations), got {num_feat!r}')
        if compute_dtype == 'bf16' and num_feat % 16:
            raise ValueError(f'RCAN in bf16 needs num_feat to be a multiple of 16 (CB16 activations), got {num_feat!r}')
        if not isinstance(squeeze_factor, int) or squeeze_factor <= 0 or num_feat // squeeze_factor < 1:
            raise ValueError(f'RCAN needs num_feat // squeeze_factor >= 1, got {num_feat!r} // {squeeze_factor!r}')
        if num_in_ch != 3 or num_out_ch != 3:
            raise ValueError(f'RCAN subtracts a 3-channel RGB mean: num_in_ch and num_out_ch must be 3, got {num_in_ch}, {num_out_ch}')
        if num_group < 1 or num_block < 1:
            raise ValueError(f'RCAN needs num_group >= 1 and num_block >= 1, got {num_group!r}, {num_block!r}')
        if len(rgb_mean) != 3:
            raise ValueError(f'rgb_mean must hold 3 values, got {rgb_mean!r}')
        self.upscale, self.img_range = upscale, float(img_range)
        self.num_in_ch, self.num_out_ch, self.num_feat = num_in_ch, num_out_ch, num_feat
        self.num_group, self.num_block, self.squeeze_factor = num_group, num_block, squeeze_factor
        self.res_scale = res_scale
        self.compute_dtype = compute_dtype
        self.rgb_mean = tuple(float(v) for v in rgb_mean)
        self.mean = torch.Tensor(rgb_mean).view(1, 3, 1, 1)   # a plain attribute, as in the reference: not in the state_dict

        self.conv_first = Conv3x3Params(num_in_ch, num_feat)
        self.body = make_layer(ResidualGroupParams, num_group, num_feat=num_feat, num_block=num_block,
                               squeeze_factor=squeeze_factor, res_scale=res_scale)
        self.conv_after_body = Conv3x3Params(num_feat, num_feat)
        ups = []
        for r in self.stages:
            ups += [Conv3x3Params(num_feat, r * r * num_feat), nn.PixelShuffle(r)]
        self.upsample = nn.Sequential(*ups)
        self.conv_last = Conv3x3Params(num_feat, num_out_ch)
        self._affine = {}

    # ------------------------------------------------------------------ HIP plumbing
    def blocks(self):
        """[(group, [RCABParams])] in forward order."""
        return [(grp, list(grp.residual_group)) for grp in self.body]

    def ups(self):
        """(conv, r) of the upsampling stages, in forward order."""
        return [(self.upsample[2 * i], r) for i, r in enumerate(self.stages)]

    def _drop_device_caches(self):
        self._affine = {}

    def _autograd_apply(self, x):
        from .rcan_autograd import rcan_apply
        return rcan_apply(self, x)

    def affine(self, dev):
        """Per-channel (a, b) device constants of the mean shift: in (x * R - R*mean), out (y * (1/R) + mean), and their
        adjoints' scales (R, 1/R)."""
        hit = self._affine.get(str(dev))
        if hit is None:
            R = self.img_range
            m = torch.tensor(self.rgb_mean, dtype=torch.float64)
            hit = dict(in_a=torch.full((3,), R, dtype=torch.float32), in_b=(-m * R).float(),
                       out_a=torch.full((3,), 1.0 / R, dtype=torch.float32), out_b=m.float())
            hit = {k: v.to(dev) for k, v in hit.items()}
            self._affine[str(dev)] = hit
        return hit

    def _channel_affine(self, x, a, b):
        n, c, h, w = x.shape
        y = torch.empty_like(x)
        hip_ops.launch('sr_channel_affine_f32', x.device, x.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr() if b is not None else None,
                       n, c, h * w)
        return y

    def run_forward(self, x, keep=False, ops=F32):
        """The forward as per-layer launches on the current stream, on CB8 fp32 (``F32``) or CB16 bf16 (``BF16``) activations:
        in bf16 every conv epilogue is fp32, the attention pools and gates in fp32 from the fp32 parameters and rounds
        x + res_scale * u * s once, and conv_last stores fp32 NCHW.  ``keep`` (fp32 only): also return what the backward reads
        (the CB8 input, conv_first's output, per RCAB (conv 0 output t, conv 2 output u, p, h, s, block output), per group its
        input, the body's output, the conv_after_body output and each shuffled upsampling output)."""
        assert not (keep and ops.bf16), 'the backward reads fp32 activations'
        n, _, h, w = x.shape
        s = self.upscale

        def pk(conv):
            return self.packed(conv, 0, ops.bf16)

        with torch.cuda.device(x.device):
            if ops.bf16:
                xc = hip_ops.edsr_shift_in(x, self.rgb_mean, self.img_range, bf16=True)
            else:   # x*R - R*mean: not the shift kernels' (x - mean)*R, whose rounding differs
                af = self.affine(x.device)
                xc = hip_ops.nchw_to_cb8(self._channel_affine(x, af['in_a'], af['in_b']))
            x0 = feat = ops.conv3x3(xc, pk(self.conv_first))
            saved = dict(x=xc, x0=x0, groups=[], ups=[]) if keep else None
            for grp, rcabs in self.blocks():
                g_in = feat
                blocks = []
                for blk in rcabs:
                    ca = blk.ca
                    mlp = (ca.fc1.weight, ca.fc1.bias, ca.fc2.weight, ca.fc2.bias)
                    t = ops.conv3x3(feat, pk(blk.conv1), act_slope=0.0)
                    u = ops.conv3x3(t, pk(blk.conv2))
                    if ops.bf16:
                        sv = hip_ops.ca_squeeze_bf16(u, *mlp)
                        # in place except where feat is still the group's input, which body.{g}.conv adds back
                        feat = hip_ops.ca_excite_bf16(feat, u, sv, float(blk.res_scale), out=None if feat is g_in else feat)
                    else:
                        p, hb, sv = hip_ops.ca_squeeze(u, *mlp)
                        feat = hip_ops.ca_excite(feat, u, sv, float(blk.res_scale))
                    if keep:
                        blocks.append((t, u, p, hb, sv, feat))
                    else:
                        del t, u
                feat = ops.conv3x3(feat, pk(grp.conv), res1=g_in, beta1=1.0)
                if keep:
                    saved['groups'].append((g_in, blocks))
            if keep:
                saved['body'] = feat
            feat = ops.conv3x3(feat, pk(self.conv_after_body), res1=x0, beta1=1.0)
            if keep:
                saved['res'] = feat
            for conv, r in self.ups():
                feat = upsample_stage(self, feat, conv, r, ops)
                if keep:
                    saved['ups'].append(feat)
            y = torch.empty((n, self.num_out_ch, h * s, w * s), dtype=torch.float32, device=x.device)
            ops.conv3x3(feat, pk(self.conv_last), out_nchw=y)
            if ops.bf16:
                hip_ops.edsr_shift_out(y, self.rgb_mean, self.img_range)
            else:
                y = self._channel_affine(y, af['out_a'], af['out_b'])
        return y, saved
