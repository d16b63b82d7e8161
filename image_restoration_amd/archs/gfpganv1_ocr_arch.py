"""GFPGANv1OCR (the U-Net + StyleGAN2-with-SFT licence-plate restorer) on the MI355X HIP path, fp32 inference.

Same constructor, defaults, ``state_dict`` keys, shapes and order (the ``noises.noise{k}`` buffers and the unused style MLP
included) and initialisation as the reference ``basicsr/archs/gfpganv1_ocr_arch.py`` with the StyleGAN2 modules of
``stylegan2_ocr_arch.py``, so ``network_g: {type: GFPGANv1OCR, ...}`` option blocks and BasicSR checkpoints load with
strict=True.  The modules only hold parameters; the forward is a composition of launches (include/sr_hip_gfpgan.h next to
sr_hip.h and sr_hip_ridnet.h):

    U-Net encoder
      conv_body_first (1x1)             sr_convd_f32 (ksize 1, FusedLeakyReLU as act 0.2 / alpha sqrt(2))
      ResBlock conv1                    sr_conv3x3_f32
      ResBlock skip (blur + 1x1 / s2)   sr_conv4x4s2_f32 on the composite weight W (x) blur, alpha 1/sqrt(2)
      ResBlock conv2 (blur + 3x3 / s2)  sr_cb8_pixel_unshuffle_f32, then sr_conv3x3_f32 on the 4*cin-channel composite of the
                                        6x6 / s2 conv W * blur, res1 = the skip: (conv2 + skip) / sqrt(2) in its epilogue
      final_conv                        sr_conv3x3_f32
      final_linear                      sr_linear_fwd_f32 on the CB8 features (its columns permuted at pack time)
    U-Net decoder, per level
      feat + unet skip                  sr_cb8_axpby_f32
      ResUpBlock                        sr_conv3x3_f32, sr_bilinear2x_fwd_f32, sr_conv3x3_f32; skip: sr_bilinear2x_fwd_f32 and
                                        sr_convd_f32 (1x1) with res1 = conv2: (conv2 + skip) / sqrt(2)
      condition_scale / _shift          their first convs as ONE sr_conv3x3_f32 of 2C outputs, then two sr_conv3x3_f32
      toRGB (return_rgb)                sr_convd_f32 (1x1 -> 3), sr_cb8_to_nchw_f32
    StyleGAN2 decoder
      style MLP (input_is_latent off)   sr_gfpgan_norm_style_f32, num_mlp x sr_linear_fwd_f32 (sqrt(2) folded into W and b)
      every modulation s / demod d      sr_gfpgan_style_f32: ONE launch for all layers and samples
      constant input * s                sr_ca_scale_f32 (image stride 0)
      style_conv1                       sr_gfpgan_modconv_f32
      to_rgb1 / to_rgbs                 sr_gfpgan_torgb_f32, which also writes out * s of the next level's conv1
      StyleConv (upsample)              sr_gfpgan_upconv_f32 (polyphase transposed conv), sr_gfpgan_blur_up_f32 (blur, demod,
                                        noise, FusedLeakyReLU, SFT, * s of conv2)
      StyleConv                         sr_gfpgan_modconv_f32

Noise: ``randomize_noise=False`` reads the ``noises.noise{k}`` buffers (one map for the batch); ``randomize_noise=True`` (the
reference's default) draws ``torch.empty(N, 1, h, w).normal_()`` on the input's device with torch's default generator, one map
per StyleConv in layer order (style_conv1, then per level conv1, conv2) before any kernel runs: the draws the reference makes
lazily in the same order.  Inference only: a forward in train mode with grad enabled raises NotImplementedError; outputs never
carry a grad_fn.  fp32 only.
"""
import math

import torch
from torch import nn

from .. import _lib, hip_ops
from ..utils.registry import ARCH_REGISTRY

SQRT2 = math.sqrt(2.0)
BLUR_1D = (1.0, 3.0, 3.0, 1.0)


def _channels(narrow, channel_multiplier, unet):
    f = narrow * (0.5 if unet else 1.0)
    return {'4': int(512 * f), '8': int(512 * f), '16': int(512 * f), '32': int(512 * f), '64': int(256 * channel_multiplier * f),
            '128': int(128 * channel_multiplier * f), '256': int(64 * channel_multiplier * f), '512': int(32 * channel_multiplier * f),
            '1024': int(16 * channel_multiplier * f)}


class _ParamsOnly(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError(f'{type(self).__name__} is a parameter container; GFPGANv1OCR launches the HIP kernels')


class Blur(_ParamsOnly):
    """The reference's UpFirDnSmooth / UpFirDnUpsample: a fixed FIR, no parameters (holds a Sequential index)."""


class ScaledLeakyReLU(_ParamsOnly):
    pass


class NormStyleCode(_ParamsOnly):
    pass


class FusedLeakyReLU(_ParamsOnly):
    def __init__(self, channel):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(channel))


class EqualConv2d(_ParamsOnly):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, bias_init_val=0):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.scale = 1 / math.sqrt(in_channels * kernel_size ** 2)
        self.weight = nn.Parameter(torch.randn(out_channels, in_channels, kernel_size, kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels).fill_(bias_init_val))
        else:
            self.register_parameter('bias', None)


class EqualLinear(_ParamsOnly):
    def __init__(self, in_channels, out_channels, bias=True, bias_init_val=0, lr_mul=1, activation=None):
        super().__init__()
        if activation not in ('fused_lrelu', None):
            raise ValueError(f'EqualLinear activation must be fused_lrelu or None, got {activation!r}')
        self.in_channels, self.out_channels, self.lr_mul, self.activation = in_channels, out_channels, lr_mul, activation
        self.scale = (1 / math.sqrt(in_channels)) * lr_mul
        self.weight = nn.Parameter(torch.randn(out_channels, in_channels).div_(lr_mul))
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels).fill_(bias_init_val))
        else:
            self.register_parameter('bias', None)


class ConvLayer(nn.Sequential):
    """[Blur,] EqualConv2d (bias only without activation), FusedLeakyReLU / ScaledLeakyReLU — the reference's ConvLayer."""

    def __init__(self, in_channels, out_channels, kernel_size, downsample=False, bias=True, activate=True):
        layers = [Blur()] if downsample else []
        layers.append(EqualConv2d(in_channels, out_channels, kernel_size, bias=bias and not activate))
        if activate:
            layers.append(FusedLeakyReLU(out_channels) if bias else ScaledLeakyReLU())
        super().__init__(*layers)


class ResBlock(_ParamsOnly):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = ConvLayer(in_channels, in_channels, 3)
        self.conv2 = ConvLayer(in_channels, out_channels, 3, downsample=True)
        self.skip = ConvLayer(in_channels, out_channels, 1, downsample=True, bias=False, activate=False)


class ConvUpLayer(_ParamsOnly):
    def __init__(self, in_channels, out_channels, kernel_size, bias=True, bias_init_val=0, activate=True):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.scale = 1 / math.sqrt(in_channels * kernel_size ** 2)
        self.weight = nn.Parameter(torch.randn(out_channels, in_channels, kernel_size, kernel_size))
        if bias and not activate:
            self.bias = nn.Parameter(torch.zeros(out_channels).fill_(bias_init_val))
        else:
            self.register_parameter('bias', None)
        if activate:
            self.activation = FusedLeakyReLU(out_channels) if bias else ScaledLeakyReLU()
        else:
            self.activation = None


class ResUpBlock(_ParamsOnly):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = ConvLayer(in_channels, in_channels, 3)
        self.conv2 = ConvUpLayer(in_channels, out_channels, 3)
        self.skip = ConvUpLayer(in_channels, out_channels, 1, bias=False, activate=False)


class ModulatedConv2d(_ParamsOnly):
    def __init__(self, in_channels, out_channels, kernel_size, num_style_feat, demodulate=True, sample_mode=None):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.demodulate, self.sample_mode = demodulate, sample_mode
        if sample_mode == 'upsample':
            self.smooth = Blur()
        self.scale = 1 / math.sqrt(in_channels * kernel_size ** 2)
        self.modulation = EqualLinear(num_style_feat, in_channels, bias=True, bias_init_val=1, lr_mul=1, activation=None)
        self.weight = nn.Parameter(torch.randn(1, out_channels, in_channels, kernel_size, kernel_size))


class StyleConv(_ParamsOnly):
    def __init__(self, in_channels, out_channels, kernel_size, num_style_feat, sample_mode=None):
        super().__init__()
        self.modulated_conv = ModulatedConv2d(in_channels, out_channels, kernel_size, num_style_feat, sample_mode=sample_mode)
        self.weight = nn.Parameter(torch.zeros(1))  # noise strength
        self.activate = FusedLeakyReLU(out_channels)


class ToRGB(_ParamsOnly):
    def __init__(self, in_channels, num_style_feat, upsample=True):
        super().__init__()
        self.upsample = Blur() if upsample else None
        self.modulated_conv = ModulatedConv2d(in_channels, 3, 1, num_style_feat, demodulate=False)
        self.bias = nn.Parameter(torch.zeros(1, 3, 1, 1))


class ConstantInput(_ParamsOnly):
    def __init__(self, num_channel, size_width, size_height):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(1, num_channel, size_height, size_width))


class StyleGAN2OCRGeneratorSFT(_ParamsOnly):
    """The decoder's parameters in the reference's layout (StyleGAN2OCRGenerator + sft_half)."""

    def __init__(self, input_width=256, input_height=256, num_style_feat=512, num_mlp=8, channel_multiplier=2, lr_mlp=0.01, narrow=1,
                 sft_half=False):
        super().__init__()
        self.num_style_feat, self.sft_half = num_style_feat, sft_half
        self.style_mlp = nn.Sequential(NormStyleCode(), *[
            EqualLinear(num_style_feat, num_style_feat, bias=True, bias_init_val=0, lr_mul=lr_mlp, activation='fused_lrelu')
            for _ in range(num_mlp)])
        ch = _channels(narrow, channel_multiplier, unet=False)
        self.channels = ch
        ratio = int(input_width / input_height)
        self.constant_input = ConstantInput(ch['4'], size_height=4, size_width=4 * ratio)
        self.style_conv1 = StyleConv(ch['4'], ch['4'], 3, num_style_feat)
        self.to_rgb1 = ToRGB(ch['4'], num_style_feat, upsample=False)
        self.log_size = int(math.log(min(input_width, input_height), 2))
        self.num_layers = (self.log_size - 2) * 2 + 1
        self.num_latent = self.log_size * 2 - 2
        self.style_convs = nn.ModuleList()
        self.to_rgbs = nn.ModuleList()
        self.noises = nn.Module()
        for k in range(self.num_layers):
            rh = 2 ** ((k + 5) // 2)
            self.noises.register_buffer(f'noise{k}', torch.randn(1, 1, rh, rh * ratio))
        cin = ch['4']
        for i in range(3, self.log_size + 1):
            cout = ch[f'{2 ** i}']
            self.style_convs.append(StyleConv(cin, cout, 3, num_style_feat, sample_mode='upsample'))
            self.style_convs.append(StyleConv(cout, cout, 3, num_style_feat))
            self.to_rgbs.append(ToRGB(cout, num_style_feat))
            cin = cout


def _blur_kernel(dtype=torch.float64):
    k = torch.tensor(BLUR_1D, dtype=dtype)
    k = torch.outer(k, k)
    return k / k.sum()


@ARCH_REGISTRY.register()
class GFPGANv1OCR(nn.Module):
    """GFPGANv1OCR(input_width=768, input_height=32, num_style_feat=512, channel_multiplier=1, resample_kernel=(1, 3, 3, 1),
    decoder_load_path=None, fix_decoder=True, num_mlp=8, lr_mlp=0.01, input_is_latent=False, different_w=False, narrow=1,
    sft_half=False).

    forward(x [N, 3, input_height, input_width] in [-1, 1], fp32 on a HIP device, return_latents=False, save_feat_path=None,
    load_feat_path=None, return_rgb=True, randomize_noise=True) -> (image [N, 3, H, W], out_rgbs).  ValueError for:
    ``input_height`` not a power of two >= 8; ``input_width`` not a multiple of it; ``input_is_latent=False`` with
    ``different_w=True`` (the reference's style MLP is ill-defined on a 3-D style code); a resample kernel other than
    (1, 3, 3, 1); channel counts that are not multiples of 8 in [8, 512]; ``num_style_feat`` above 1024; ``compute_dtype`` other
    than fp32; an input of another size.  ``save_feat_path`` / ``load_feat_path`` raise NotImplementedError.
    """

    def __init__(self, input_width=768, input_height=32, num_style_feat=512, channel_multiplier=1, resample_kernel=(1, 3, 3, 1),
                 decoder_load_path=None, fix_decoder=True, num_mlp=8, lr_mlp=0.01, input_is_latent=False, different_w=False,
                 narrow=1, sft_half=False, compute_dtype='fp32'):
        super().__init__()
        if compute_dtype not in ('fp32', 'float32', None):
            raise ValueError(f'GFPGANv1OCR runs in fp32 only, got compute_dtype={compute_dtype!r}')
        if not isinstance(input_height, int) or input_height < 8 or input_height & (input_height - 1):
            raise ValueError(f'GFPGANv1OCR needs input_height to be a power of two >= 8, got {input_height!r}')
        if not isinstance(input_width, int) or input_width < input_height or input_width % input_height:
            raise ValueError(f'GFPGANv1OCR needs input_width to be a multiple of input_height, got {input_width!r} x {input_height}')
        if not input_is_latent and different_w:
            raise ValueError('GFPGANv1OCR: input_is_latent=False with different_w=True is ill-defined in the reference (the style '
                             'MLP normalises a 3-D style code over its layer axis); refused')
        if tuple(resample_kernel) != BLUR_1D:
            raise ValueError(f'GFPGANv1OCR runs the (1, 3, 3, 1) resample kernel only, got {resample_kernel!r}')
        if not 0 < num_style_feat <= 1024:
            raise ValueError(f'GFPGANv1OCR needs num_style_feat in [1, 1024], got {num_style_feat!r}')
        self.input_width, self.input_height = input_width, input_height
        self.input_is_latent, self.different_w, self.num_style_feat = input_is_latent, different_w, num_style_feat
        self.sft_half = sft_half
        self.log_size = int(math.log(input_height, 2))
        self.ratio = input_width // input_height
        unet = _channels(narrow, channel_multiplier, unet=True)
        dec = _channels(narrow, channel_multiplier, unet=False)
        used = [f'{2 ** i}' for i in range(2, self.log_size + 1)]
        for key in used:
            for c in (unet[key], dec[key]):
                if c < 8 or c > 512 or c % 8:
                    raise ValueError(f'GFPGANv1OCR needs every channel count to be a multiple of 8 in [8, 512] (CB8 activations); '
                                     f'narrow={narrow}, channel_multiplier={channel_multiplier} give {c} at {key}')
            if dec[key] != 2 * unet[key]:
                raise ValueError(f'GFPGANv1OCR needs the decoder to have twice the U-Net channels (SFT), got {dec[key]} and '
                                 f'{unet[key]} at {key}')
        self.unet_channels, self.dec_channels = unet, dec

        first = unet[f'{input_height}']
        self.conv_body_first = ConvLayer(3, first, 1)
        cin = first
        self.conv_body_down = nn.ModuleList()
        for i in range(self.log_size, 2, -1):
            cout = unet[f'{2 ** (i - 1)}']
            self.conv_body_down.append(ResBlock(cin, cout))
            cin = cout
        self.final_conv = ConvLayer(cin, unet['4'], 3)
        cin = unet['4']
        self.conv_body_up = nn.ModuleList()
        for i in range(3, self.log_size + 1):
            cout = unet[f'{2 ** i}']
            self.conv_body_up.append(ResUpBlock(cin, cout))
            cin = cout
        self.toRGB = nn.ModuleList(
            [EqualConv2d(unet[f'{2 ** i}'], 3, 1, bias=True, bias_init_val=0) for i in range(3, self.log_size + 1)])
        lin_out = (self.log_size * 2 - 2) * num_style_feat if different_w else num_style_feat
        self.final_linear = EqualLinear(unet['4'] * 4 * 4 * self.ratio, lin_out, bias=True, bias_init_val=0, lr_mul=1, activation=None)
        self.stylegan_decoder = StyleGAN2OCRGeneratorSFT(input_width, input_height, num_style_feat, num_mlp, channel_multiplier,
                                                         lr_mlp, narrow, sft_half)
        if decoder_load_path:
            self.stylegan_decoder.load_state_dict(
                torch.load(decoder_load_path, map_location=lambda storage, loc: storage, weights_only=False)['params_ema'])
        if fix_decoder:
            for _, p in self.stylegan_decoder.named_parameters():
                p.requires_grad = False
        self.condition_scale = nn.ModuleList()
        self.condition_shift = nn.ModuleList()
        for i in range(3, self.log_size + 1):
            c = unet[f'{2 ** i}']
            sft_c = c if sft_half else 2 * c
            self.condition_scale.append(nn.Sequential(EqualConv2d(c, c, 3, padding=1), ScaledLeakyReLU(),
                                                      EqualConv2d(c, sft_c, 3, padding=1, bias_init_val=1)))
            self.condition_shift.append(nn.Sequential(EqualConv2d(c, c, 3, padding=1), ScaledLeakyReLU(),
                                                      EqualConv2d(c, sft_c, 3, padding=1, bias_init_val=0)))
        self._pack = None
        self._pack_gen = 0
        self._style_tables = {}

    # ------------------------------------------------------------------ HIP plumbing
    def invalidate_packed(self):
        """Call after parameter memory was written behind torch's version counters."""
        self._pack_gen += 1

    def _apply(self, fn, *args, **kwargs):
        self._pack = None
        self._style_tables = {}
        return super()._apply(fn, *args, **kwargs)

    def _signature(self):
        return (self._pack_gen,) + tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _packed(self):
        sig = self._signature()
        if self._pack is not None and self._pack[0] == sig:
            return self._pack[1]
        for p in self.parameters():
            if p.dtype != torch.float32:
                raise _lib.SrHipError('GFPGANv1OCR parameters must be fp32')
        with torch.no_grad():
            pk = self._build_pack()
        self._pack = (sig, pk)
        self._style_tables = {}
        return pk

    def _build_pack(self):
        """Weight images and folded constants, built once per parameter change (host plumbing, no forward compute)."""
        dev = self.final_linear.weight.device
        kb = _blur_kernel().to(dev)
        pk = {}

        def conv3(ec, bias):
            w = ec.weight * ec.scale
            return hip_ops.PackedConv(w.float().contiguous(), None if bias is None else bias.float().contiguous())

        def convk(w, bias):
            return hip_ops.PackedConvK(w.float().contiguous(), None if bias is None else bias.float().contiguous())

        pk['first'] = convk(self.conv_body_first[0].weight * self.conv_body_first[0].scale, self.conv_body_first[1].bias)
        pk['down'] = []
        for blk in self.conv_body_down:
            c1 = conv3(blk.conv1[0], blk.conv1[1].bias)
            # blur (pad 1) + 1x1 / s2 == 4x4 / s2 / pad 1 with W (x) K
            ws = blk.skip[1].weight.double() * blk.skip[1].scale
            w4 = ws * kb.view(1, 1, 4, 4)
            sk = hip_ops.PackedConv4x4s2(w4.float().contiguous())
            # blur (pad 2) + 3x3 / s2 == 6x6 / s2 / pad 2 with W * K == 3x3 / pad 1 on the 2x pixel-unshuffled source
            w3 = blk.conv2[1].weight.double() * blk.conv2[1].scale
            co, ci = w3.shape[:2]
            w6 = torch.zeros(co, ci, 6, 6, dtype=torch.float64, device=dev)
            for a in range(3):
                for b in range(3):
                    w6[:, :, a:a + 4, b:b + 4] += w3[:, :, a, b, None, None] * kb
            wu = w6.view(co, ci, 3, 2, 3, 2).permute(0, 1, 3, 5, 2, 4).reshape(co, ci * 4, 3, 3)
            c2 = hip_ops.PackedConv(wu.float().contiguous(), blk.conv2[2].bias.float().contiguous())
            pk['down'].append((c1, sk, c2))
        pk['final'] = conv3(self.final_conv[0], self.final_conv[1].bias)
        # final_linear on the CB8-flattened [C/8][4][4r][8] features: its columns permuted from the NCHW flattening
        c4, hh, ww = self.unet_channels['4'], 4, 4 * self.ratio
        perm = torch.arange(c4 * hh * ww, device=dev).view(c4 // 8, 8, hh, ww).permute(0, 2, 3, 1).reshape(-1)
        fl = self.final_linear
        pk['lin_w'] = (fl.weight * fl.scale)[:, perm].float().contiguous()
        pk['lin_b'] = (fl.bias * fl.lr_mul).float().contiguous()
        dec = self.stylegan_decoder
        pk['mlp'] = [((m.weight * (m.scale * SQRT2)).float().contiguous(), (m.bias * (m.lr_mul * SQRT2)).float().contiguous())
                     for m in list(dec.style_mlp)[1:]]
        pk['up'] = []
        for j, blk in enumerate(self.conv_body_up):
            c1 = conv3(blk.conv1[0], blk.conv1[1].bias)
            c2 = hip_ops.PackedConv((blk.conv2.weight * blk.conv2.scale).float().contiguous(),
                                    blk.conv2.activation.bias.float().contiguous())
            sk = convk(blk.skip.weight * blk.skip.scale, None)
            cs, ct = self.condition_scale[j], self.condition_shift[j]
            h1 = hip_ops.PackedConv(torch.cat([cs[0].weight * cs[0].scale, ct[0].weight * ct[0].scale]).float().contiguous(),
                                    torch.cat([cs[0].bias, ct[0].bias]).float().contiguous())
            s2 = conv3(cs[2], cs[2].bias)
            t2 = conv3(ct[2], ct[2].bias)
            rgb = convk(self.toRGB[j].weight * self.toRGB[j].scale, self.toRGB[j].bias)
            pk['up'].append((c1, c2, sk, h1, s2, t2, rgb))
        # decoder: constant input in CB8, per StyleConv the shared 3x3 image, Q = sum_taps W^2 and the noise strength (read
        # once here, so the forward needs no host sync), per ToRGB its 3 x C weight
        ci = dec.constant_input.weight
        cst = hip_ops.CB8.empty(1, ci.shape[1], ci.shape[2], ci.shape[3], dev)
        cst.buf.copy_(ci.detach().float().view(1, ci.shape[1] // 8, 8, ci.shape[2], ci.shape[3]).permute(0, 1, 3, 4, 2))
        pk['const'] = cst
        convs = [dec.style_conv1] + list(dec.style_convs)
        pk['sconv'] = []
        for sc in convs:
            mc = sc.modulated_conv
            w = mc.weight[0].float().contiguous()
            pk['sconv'].append(dict(pc=convk(w, sc.activate.bias), q=(w.double() ** 2).sum((2, 3)).float().contiguous(),
                                    bias=sc.activate.bias.float().contiguous(), ns=float(sc.weight.detach().cpu()[0]),
                                    mod=mc.modulation, scale=mc.scale, cin=mc.in_channels, cout=mc.out_channels))
        rgbs = [dec.to_rgb1] + list(dec.to_rgbs)
        pk['rgb'] = [dict(w=t.modulated_conv.weight.view(3, -1).float().contiguous(), bias=t.bias.view(3).float().contiguous(),
                          mod=t.modulated_conv.modulation, scale=t.modulated_conv.scale, cin=t.modulated_conv.in_channels)
                     for t in rgbs]
        return pk

    def _style_table(self, pk, n, dev):
        """The layer table of sr_gfpgan_style_f32 and its s / d outputs for a batch of n: style_conv1, to_rgb1, then per level
        conv1, conv2, to_rgb (latent indices 0, 1, then i, i + 1, i + 2 for i = 1, 3, ...)."""
        key = (n, str(dev))
        hit = self._style_tables.get(key)
        if hit is not None:
            return hit
        L = self.log_size - 2
        order = [('c', 0, 0), ('r', 0, 1)]
        for j in range(L):
            i = 1 + 2 * j
            order += [('c', 1 + 2 * j, i), ('c', 2 + 2 * j, i + 1), ('r', 1 + j, i + 2)]
        table = (_lib.GfpganStyleLayer * len(order))()
        outs, keep = [], []
        for t, (kind, idx, lat) in enumerate(order):
            e = pk['sconv'][idx] if kind == 'c' else pk['rgb'][idx]
            mod = e['mod']
            mw, mb = mod.weight.detach().float().contiguous(), (mod.bias * mod.lr_mul).detach().float().contiguous()
            s = torch.empty((n, e['cin']), dtype=torch.float32, device=dev)
            d = torch.empty((n, e['cout']), dtype=torch.float32, device=dev) if kind == 'c' else None
            keep += [mw, mb]
            row = table[t]
            row.mod_w, row.mod_b, row.cin, row.latent_index = mw.data_ptr(), mb.data_ptr(), e['cin'], lat
            row.s = s.data_ptr()
            if kind == 'c':
                row.q, row.cout, row.wscale, row.d = e['q'].data_ptr(), e['cout'], e['scale'], d.data_ptr()
            outs.append((s, d))
        hit = (table, outs, keep)
        self._style_tables[key] = hit
        return hit

    def run_forward(self, x, return_rgb=True, randomize_noise=True, keep=False):
        """The forward as launches on the current stream.  Returns (image, out_rgbs, extras); ``keep``: extras holds the style
        code / latent and the SFT conditions (CB8), for the tests."""
        pk = self._packed()
        dev = x.device
        n = x.shape[0]
        L = self.log_size - 2
        dec = self.stylegan_decoder
        nsf = self.num_style_feat
        # noises first (the reference's lazy draws, in layer order)
        shapes = [(4, 4 * self.ratio)] + [(2 ** (3 + j), 2 ** (3 + j) * self.ratio) for j in range(L) for _ in range(2)]
        if randomize_noise:
            noises = [torch.empty((n, 1, h, w), dtype=torch.float32, device=dev).normal_() for h, w in shapes]
        else:
            noises = [getattr(dec.noises, f'noise{k}') for k in range(len(shapes))]
            noises = [z if z.dtype == torch.float32 and z.is_contiguous() else z.float().contiguous() for z in noises]
        extras = {}
        with torch.cuda.device(dev):
            # U-Net encoder
            feat = hip_ops.convd(hip_ops.nchw_to_cb8(x), pk['first'], 1, act_slope=0.2, alpha=SQRT2)
            skips = []
            for c1, sk, c2 in pk['down']:
                a = hip_ops.conv3x3(feat, c1, act_slope=0.2, alpha=SQRT2)
                s = hip_ops.conv4x4s2(feat, sk, act_slope=1.0, alpha=1 / SQRT2)
                feat = hip_ops.conv3x3(hip_ops.pixel_unshuffle(a, a.channels, 2), c2, act_slope=0.2, alpha=1.0, res1=s, beta1=1.0)
                skips.insert(0, feat)
            feat = hip_ops.conv3x3(feat, pk['final'], act_slope=0.2, alpha=SQRT2)
            style = hip_ops.linear(feat.buf.view(n, -1), pk['lin_w'], pk['lin_b'])
            if keep:
                extras['style_code'] = style
            # style code -> latent rows
            if self.input_is_latent:
                latent, lat_rs = style, (nsf if self.different_w else 0)
            else:
                latent = hip_ops.gfpgan_norm_style(style)
                for w, b in pk['mlp']:
                    latent = hip_ops.linear(latent, w, b, act_slope=0.2)
                lat_rs = 0
            if keep:
                extras['latent'] = latent
            # U-Net decoder: features, SFT conditions, the U-Net's own RGB outputs
            conds, out_rgbs = [], []
            for j, (c1, c2, sk, h1, s2, t2, rgb) in enumerate(pk['up']):
                hip_ops.cb8_axpby(feat, skips[j])
                a = hip_ops.conv3x3(feat, c1, act_slope=0.2, alpha=SQRT2)
                b = hip_ops.conv3x3(hip_ops.bilinear2x(a), c2, act_slope=0.2, alpha=SQRT2)
                feat = hip_ops.convd(hip_ops.bilinear2x(feat), sk, 1, act_slope=1.0, alpha=1 / SQRT2, res1=b, beta1=1 / SQRT2)
                c = feat.channels
                hh = hip_ops.conv3x3(feat, h1, act_slope=0.2, alpha=SQRT2)
                conds.append((hip_ops.conv3x3(hh.slice(0, c), s2), hip_ops.conv3x3(hh.slice(c, c), t2)))
                if return_rgb:
                    out_rgbs.append(hip_ops.cb8_to_nchw(hip_ops.convd(feat, rgb, 1), 3))
            if keep:
                extras['conditions'] = conds
            # StyleGAN2 decoder
            table, sd, _ = self._style_table(pk, n, dev)
            hip_ops.gfpgan_style(latent, latent.stride(0), lat_rs, nsf, table, n)
            sc, rg = pk['sconv'], pk['rgb']
            s_c = [sd[0]] + [sd[2 + 3 * j + k] for j in range(L) for k in range(2)]   # (s, d) of the StyleConvs in layer order
            s_r = [sd[1]] + [sd[4 + 3 * j] for j in range(L)]
            x0 = hip_ops.cb8_channel_scale(pk['const'], s_c[0][0], n)
            out = hip_ops.gfpgan_modconv(x0, sc[0]['pc'], hip_ops.gfpgan_tail(s_c[0][1], noises[0], sc[0]['ns']))
            img, xm = hip_ops.gfpgan_torgb(out, rg[0]['w'], rg[0]['scale'], s_r[0][0], rg[0]['bias'], None,
                                           s_c[1][0] if L else None)
            for j in range(L):
                k1, k2 = 1 + 2 * j, 2 + 2 * j
                t = hip_ops.gfpgan_upconv(xm, sc[k1]['pc'])
                sft_c0 = sc[k1]['cout'] // 2 if self.sft_half else 0
                o1 = hip_ops.gfpgan_blur_up(t, sc[k1]['bias'], hip_ops.gfpgan_tail(s_c[k1][1], noises[k1], sc[k1]['ns'], conds[j], sft_c0,
                                                                                   s_next=s_c[k2][0]))
                del t
                o2 = hip_ops.gfpgan_modconv(o1, sc[k2]['pc'], hip_ops.gfpgan_tail(s_c[k2][1], noises[k2], sc[k2]['ns']))
                nxt = s_c[k2 + 1][0] if j + 1 < L else None
                img, xm = hip_ops.gfpgan_torgb(o2, rg[1 + j]['w'], rg[1 + j]['scale'], s_r[1 + j][0], rg[1 + j]['bias'], img, nxt)
        if keep:
            extras['noises'] = noises
        return img, out_rgbs, extras

    def forward(self, x, return_latents=False, save_feat_path=None, load_feat_path=None, return_rgb=True, randomize_noise=True):
        if save_feat_path is not None or load_feat_path is not None:
            raise NotImplementedError('GFPGANv1OCR: save_feat_path / load_feat_path are not supported')
        if not x.is_cuda:
            raise _lib.SrHipError('GFPGANv1OCR.forward runs only on a HIP device (no CPU fallback): move the module and input with '
                                  '.to("cuda")')
        if self.training and torch.is_grad_enabled():
            raise NotImplementedError('GFPGANv1OCR runs inference only: call .eval() (or run under torch.no_grad())')
        if x.dim() != 4 or x.size(1) != 3 or tuple(x.shape[2:]) != (self.input_height, self.input_width):
            raise ValueError(f'expected [N, 3, {self.input_height}, {self.input_width}], got {tuple(x.shape)}')
        with torch.no_grad():
            image, out_rgbs, _ = self.run_forward(x.contiguous().float(), return_rgb, randomize_noise)
        return image, out_rgbs
