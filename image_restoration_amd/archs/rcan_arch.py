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

from .. import _lib, hip_ops
from ..utils.registry import ARCH_REGISTRY
from .arch_util import Conv3x3Params, make_layer


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


def _upscale_stages(upscale):
    """Pixel-shuffle factors of the reference's Upsample (arch_util.py Upsample): 2^n -> n stages of 2, 3 -> one of 3."""
    if isinstance(upscale, int) and not isinstance(upscale, bool):
        if upscale == 3:
            return [3]
        if upscale >= 2 and upscale & (upscale - 1) == 0:
            return [2] * (upscale.bit_length() - 1)
    raise ValueError(f'RCAN supports upscale 2^n (n >= 1) and 3, got {upscale!r}')


@ARCH_REGISTRY.register()
class RCAN(nn.Module):
    """RCAN(num_in_ch, num_out_ch, num_feat=64, num_group=10, num_block=16, squeeze_factor=16, upscale=4, res_scale=1,
    img_range=255., rgb_mean=(0.4488, 0.4371, 0.4040)[, compute_dtype='fp32']).

    forward(x [N, 3, H, W] fp32 on a HIP device) -> [N, 3, upscale*H, upscale*W].  ValueError for: ``upscale`` not 2^n (n >= 1)
    or 3; ``num_feat`` not a positive multiple of 8 (CB8 activations) or above 512; ``num_feat // squeeze_factor < 1``;
    ``num_in_ch`` or ``num_out_ch`` other than 3 (the reference's mean only broadcasts over 3 channels); ``num_group`` or
    ``num_block`` below 1; a ``compute_dtype`` other than 'fp32' / 'bf16'.  ``compute_dtype='bf16'`` (this project's own key) needs
    ``num_feat`` to be a multiple of 16 (CB16 activations) and is forward only (eval mode or no_grad): bf16 activations and
    weight images rounded from the fp32 parameters, fp32 accumulation, epilogues, attention MLP and output.
    """

    def __init__(self, num_in_ch, num_out_ch, num_feat=64, num_group=10, num_block=16, squeeze_factor=16, upscale=4,
                 res_scale=1, img_range=255., rgb_mean=(0.4488, 0.4371, 0.4040), compute_dtype='fp32'):
        super().__init__()
        if compute_dtype not in ('fp32', 'bf16'):
            raise ValueError(f"compute dtype must be 'fp32' or 'bf16', got {compute_dtype!r}")
        self.stages = _upscale_stages(upscale)
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
        self._packs = {}
        self._pack_gen = 0
        self._affine = {}
        self._grad_sink = None  # set by optim.FlatAdam: weight gradients are added straight into its arena

    # ------------------------------------------------------------------ HIP plumbing
    def blocks(self):
        """[(group, [RCABParams])] in forward order."""
        return [(grp, list(grp.residual_group)) for grp in self.body]

    def ups(self):
        """(conv, r) of the upsampling stages, in forward order."""
        return [(self.upsample[2 * i], r) for i, r in enumerate(self.stages)]

    def _param_list(self):
        """Parameters in state_dict (= named_parameters) order."""
        return list(self.parameters())

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
            raise _lib.SrHipError('RCAN parameters must be fp32')
        cls = hip_ops.PackedConvBF16 if bf16 else hip_ops.PackedConv
        pc = cls(w, b if mode == 0 else None, mode=mode)
        self._packs[key] = (sig, pc)
        return pc

    def _apply(self, fn, *args, **kwargs):
        self._packs = {}
        self._affine = {}
        return super()._apply(fn, *args, **kwargs)

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
        lib = _lib.load()
        n, c, h, w = x.shape
        y = torch.empty_like(x)
        _lib.check(lib.sr_channel_affine_f32(x.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr() if b is not None else None, n, c,
                                             h * w, hip_ops._stream(x.device)), 'sr_channel_affine_f32')
        return y

    def run_forward(self, x, keep=False):
        """The forward as per-layer launches on the current stream.  ``keep``: also return what the backward reads (the CB8
        input, conv_first's output, per RCAB (conv 0 output t, conv 2 output u, p, h, s, block output), per group its input,
        the body's output, the conv_after_body output and each shuffled upsampling output)."""
        n, _, h, w = x.shape
        s, nf = self.upscale, self.num_feat
        with torch.cuda.device(x.device):
            af = self.affine(x.device)
            xc = hip_ops.nchw_to_cb8(self._channel_affine(x, af['in_a'], af['in_b']))
            x0 = hip_ops.conv3x3(xc, self.packed(self.conv_first))
            saved = dict(x=xc, x0=x0, groups=[], ups=[]) if keep else None
            feat = x0
            for grp, rcabs in self.blocks():
                g_in = feat
                blocks = []
                for blk in rcabs:
                    ca = blk.ca
                    t = hip_ops.conv3x3(feat, self.packed(blk.conv1), act_slope=0.0)
                    u = hip_ops.conv3x3(t, self.packed(blk.conv2))
                    p, hb, sv = hip_ops.ca_squeeze(u, ca.fc1.weight, ca.fc1.bias, ca.fc2.weight, ca.fc2.bias)
                    feat = hip_ops.ca_excite(feat, u, sv, float(blk.res_scale))
                    if keep:
                        blocks.append((t, u, p, hb, sv, feat))
                    else:
                        del t, u
                feat = hip_ops.conv3x3(feat, self.packed(grp.conv), res1=g_in, beta1=1.0)
                if keep:
                    saved['groups'].append((g_in, blocks))
            if keep:
                saved['body'] = feat
            feat = hip_ops.conv3x3(feat, self.packed(self.conv_after_body), res1=x0, beta1=1.0)
            if keep:
                saved['res'] = feat
            for conv, r in self.ups():
                u = hip_ops.conv3x3(feat, self.packed(conv))
                feat = hip_ops.pixel_shuffle(u, nf, r)
                del u
                if keep:
                    saved['ups'].append(feat)
            y = torch.empty((n, self.num_out_ch, h * s, w * s), dtype=torch.float32, device=x.device)
            hip_ops.conv3x3(feat, self.packed(self.conv_last), out_nchw=y)
            y = self._channel_affine(y, af['out_a'], af['out_b'])
        return y, saved

    def run_forward_bf16(self, x):
        """The bf16 forward: CB16 activations on sr_conv3x3_bf16 with fp32 epilogues; the attention pools and gates in fp32
        from the fp32 parameters and rounds x + res_scale * u * s once; conv_last stores fp32 NCHW."""
        n, _, h, w = x.shape
        s, nf = self.upscale, self.num_feat

        def pk(conv):
            return self.packed(conv, 0, True)

        with torch.cuda.device(x.device):
            xc = hip_ops.edsr_shift_in(x, self.rgb_mean, self.img_range, bf16=True)
            x0 = feat = hip_ops.conv3x3_bf16(xc, pk(self.conv_first))
            for grp, rcabs in self.blocks():
                g_in = feat
                for blk in rcabs:
                    ca = blk.ca
                    t = hip_ops.conv3x3_bf16(feat, pk(blk.conv1), act_slope=0.0)
                    u = hip_ops.conv3x3_bf16(t, pk(blk.conv2))
                    sv = hip_ops.ca_squeeze_bf16(u, ca.fc1.weight, ca.fc1.bias, ca.fc2.weight, ca.fc2.bias)
                    # in place except where feat is still the group's input, which body.{g}.conv adds back
                    feat = hip_ops.ca_excite_bf16(feat, u, sv, float(blk.res_scale), out=None if feat is g_in else feat)
                    del t, u
                feat = hip_ops.conv3x3_bf16(feat, pk(grp.conv), res1=g_in, beta1=1.0)
            feat = hip_ops.conv3x3_bf16(feat, pk(self.conv_after_body), res1=x0, beta1=1.0)
            for conv, r in self.ups():
                u = hip_ops.conv3x3_bf16(feat, pk(conv))
                feat = hip_ops.pixel_shuffle_bf16(u, nf, r)
                del u
            y = torch.empty((n, self.num_out_ch, h * s, w * s), dtype=torch.float32, device=x.device)
            hip_ops.conv3x3_bf16(feat, pk(self.conv_last), out_nchw=y)
            hip_ops.edsr_shift_out(y, self.rgb_mean, self.img_range)
        return y

    def forward(self, x):
        if not x.is_cuda:
            raise _lib.SrHipError('RCAN.forward runs only on a HIP device (no CPU fallback): move the module '
                                  'and input with .to("cuda")')
        if x.dim() != 4 or x.size(1) != self.num_in_ch:
            raise ValueError(f'expected [N, {self.num_in_ch}, H, W], got {tuple(x.shape)}')
        x = x.contiguous().float()
        needs_graph = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self._param_list()))
        if self.compute_dtype == 'bf16':
            if needs_graph and self.training:
                raise NotImplementedError("RCAN with compute_dtype='bf16' is forward only (eval mode or torch.no_grad()); "
                                          "train with compute_dtype='fp32'")
            return self.run_forward_bf16(x)
        if needs_graph:
            from .rcan_autograd import rcan_apply
            return rcan_apply(self, x)
        return self.run_forward(x)[0]
