"""A float64 restatement of GFPGANv1OCR's forward on plain torch ops (CPU or GPU), written from the layer definitions of
image_restoration_amd/archs/gfpganv1_ocr_arch.py's docstring and the issue's contract — not from the reference's program text.
It is the yardstick the GFPGAN tests measure the HIP forward against; tests/test_gfpgan_host.py pins it to the reference's
own outputs (fixture g_x_gfpgan).

Everything takes a state dict of tensors (keys as the reference's) and a config dict with the constructor's keys."""
import math

import torch
import torch.nn.functional as F

SQRT2 = math.sqrt(2.0)


def channels(cfg, unet):
    f = cfg.get('narrow', 1) * (0.5 if unet else 1.0)
    cm = cfg.get('channel_multiplier', 1)
    base = {4: 512, 8: 512, 16: 512, 32: 512, 64: 256 * cm, 128: 128 * cm, 256: 64 * cm, 512: 32 * cm, 1024: 16 * cm}
    return {k: int(v * f) for k, v in base.items()}


def blur_kernel(ref):
    k = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=ref.dtype, device=ref.device)
    k = torch.outer(k, k)
    return k / k.sum()


def fir(x, pad0, pad1, gain=1.0):
    """Depthwise 4x4 FIR ([1,3,3,1] (x) [1,3,3,1] / 64 * gain) after zero padding pad0 before / pad1 after on both axes."""
    c = x.shape[1]
    k = (blur_kernel(x) * gain).flip((0, 1))[None, None].repeat(c, 1, 1, 1)
    return F.conv2d(F.pad(x, (pad0, pad1, pad0, pad1)), k, groups=c)


def up2_fir(x):
    """Zero-insertion upsampling by 2, then the FIR with gain 4 and pad (2, 1)."""
    n, c, h, w = x.shape
    u = x.new_zeros(n, c, 2 * h, 2 * w)
    u[:, :, ::2, ::2] = x
    return fir(u, 2, 1, 4.0)


def flrelu(x, b):
    return F.leaky_relu(x + b.view(1, -1, *([1] * (x.dim() - 2))), 0.2) * SQRT2


def eq_conv(x, w, b=None, stride=1, padding=0):
    return F.conv2d(x, w * (1 / math.sqrt(w.shape[1] * w.shape[2] * w.shape[3])), b, stride, padding)


def conv_layer(x, sd, pre, k, down=False, act=True):
    if down:
        x = fir(x, 2, 2) if k == 3 else fir(x, 1, 1)
        w = sd[f'{pre}.1.weight']
        y = eq_conv(x, w, stride=2)
        return flrelu(y, sd[f'{pre}.2.bias']) if act else y
    y = eq_conv(x, sd[f'{pre}.0.weight'], padding=k // 2)
    return flrelu(y, sd[f'{pre}.1.bias']) if act else y


def res_block(x, sd, pre):
    out = conv_layer(conv_layer(x, sd, f'{pre}.conv1', 3), sd, f'{pre}.conv2', 3, down=True)
    return (out + conv_layer(x, sd, f'{pre}.skip', 1, down=True, act=False)) / SQRT2


def bilinear2(x):
    return F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)


def res_up_block(x, sd, pre):
    out = conv_layer(x, sd, f'{pre}.conv1', 3)
    out = flrelu(eq_conv(bilinear2(out), sd[f'{pre}.conv2.weight'], padding=1), sd[f'{pre}.conv2.activation.bias'])
    skip = eq_conv(bilinear2(x), sd[f'{pre}.skip.weight'])
    return (out + skip) / SQRT2


def modulated(x, style, sd, pre, demod=True, up=False):
    """ModulatedConv2d: per-sample weights scale * W * s (demodulated), then conv (pad k//2) or transposed conv (stride 2) + FIR."""
    w = sd[f'{pre}.weight']
    mw, mb = sd[f'{pre}.modulation.weight'], sd[f'{pre}.modulation.bias']
    s = F.linear(style, mw * (1 / math.sqrt(mw.shape[1])), mb)
    _, co, ci, k, _ = w.shape
    wn = (1 / math.sqrt(ci * k * k)) * w * s.view(-1, 1, ci, 1, 1)
    if demod:
        wn = wn * torch.rsqrt(wn.pow(2).sum((2, 3, 4)) + 1e-8).view(-1, co, 1, 1, 1)
    outs = []
    for i in range(x.shape[0]):
        if up:
            y = F.conv_transpose2d(x[i:i + 1], wn[i].transpose(0, 1), stride=2)
            outs.append(fir(y, 1, 1, 4.0))
        else:
            outs.append(F.conv2d(x[i:i + 1], wn[i], padding=k // 2))
    return torch.cat(outs)


def style_conv(x, style, noise, sd, pre, up=False):
    y = modulated(x, style, sd, f'{pre}.modulated_conv', up=up)
    return flrelu(y + sd[f'{pre}.weight'] * noise, sd[f'{pre}.activate.bias'])


def to_rgb(x, style, skip, sd, pre):
    y = modulated(x, style, sd, f'{pre}.modulated_conv', demod=False) + sd[f'{pre}.bias']
    return y if skip is None else y + up2_fir(skip)


def noise_shapes(cfg):
    log = int(math.log2(cfg['input_height']))
    r = cfg['input_width'] // cfg['input_height']
    return [(4, 4 * r)] + [(2 ** (3 + j), 2 ** (3 + j) * r) for j in range(log - 2) for _ in range(2)]


def forward(sd, cfg, x, noises=None, return_rgb=True):
    """-> dict(image, out_rgbs, style_code, latent, conditions).  ``noises``: per StyleConv a [1 or N, 1, h, w] map in layer order
    (default: the state dict's noise buffers)."""
    log = int(math.log2(cfg['input_height']))
    nsf = cfg.get('num_style_feat', 512)
    L = log - 2
    feat = conv_layer(x, sd, 'conv_body_first', 1)
    skips = []
    for i in range(L):
        feat = res_block(feat, sd, f'conv_body_down.{i}')
        skips.insert(0, feat)
    feat = conv_layer(feat, sd, 'final_conv', 3)
    lw = sd['final_linear.weight']
    style = F.linear(feat.reshape(feat.shape[0], -1), lw * (1 / math.sqrt(lw.shape[1])), sd['final_linear.bias'])
    out = dict(style_code=style)
    conds, rgbs = [], []
    for i in range(L):
        feat = res_up_block(feat + skips[i], sd, f'conv_body_up.{i}')
        sc = [sd[f'condition_scale.{i}.{k}.{t}'] for k in (0, 2) for t in ('weight', 'bias')]
        sh = [sd[f'condition_shift.{i}.{k}.{t}'] for k in (0, 2) for t in ('weight', 'bias')]
        for p in (sc, sh):
            h = F.leaky_relu(eq_conv(feat, p[0], p[1], padding=1), 0.2) * SQRT2
            conds.append(eq_conv(h, p[2], p[3], padding=1))
        if return_rgb:
            rgbs.append(eq_conv(feat, sd[f'toRGB.{i}.weight'], sd[f'toRGB.{i}.bias']))
    out['conditions'], out['out_rgbs'] = conds, rgbs
    pre = 'stylegan_decoder'
    if cfg.get('input_is_latent', False):
        latent = style.view(style.shape[0], -1, nsf) if cfg.get('different_w', False) else style[:, None].expand(-1, 2 * log - 2, -1)
    else:
        z = style * torch.rsqrt(style.pow(2).mean(1, keepdim=True) + 1e-8)
        lr = cfg.get('lr_mlp', 0.01)
        for k in range(1, cfg.get('num_mlp', 8) + 1):
            w, b = sd[f'{pre}.style_mlp.{k}.weight'], sd[f'{pre}.style_mlp.{k}.bias']
            z = flrelu(F.linear(z, w * (lr / math.sqrt(w.shape[1]))), b * lr)
        latent = z[:, None].expand(-1, 2 * log - 2, -1)
    out['latent'] = latent
    if noises is None:
        noises = [sd[f'{pre}.noises.noise{k}'] for k in range(2 * L + 1)]
    n = x.shape[0]
    h = sd[f'{pre}.constant_input.weight'].expand(n, -1, -1, -1)
    h = style_conv(h, latent[:, 0], noises[0], sd, f'{pre}.style_conv1')
    skip = to_rgb(h, latent[:, 1], None, sd, f'{pre}.to_rgb1')
    for j in range(L):
        i = 1 + 2 * j
        h = style_conv(h, latent[:, i], noises[1 + 2 * j], sd, f'{pre}.style_convs.{2 * j}', up=True)
        s, t = conds[2 * j], conds[2 * j + 1]
        if cfg.get('sft_half', False):
            c = h.shape[1] // 2
            h = torch.cat([h[:, :c], h[:, c:] * s + t], 1)
        else:
            h = h * s + t
        h = style_conv(h, latent[:, i + 1], noises[2 + 2 * j], sd, f'{pre}.style_convs.{2 * j + 1}')
        skip = to_rgb(h, latent[:, i + 2], skip, sd, f'{pre}.to_rgbs.{j}')
    out['image'] = skip
    return out
