"""Deterministic synthetic parameters and inputs (numpy PCG64: stable across versions).

Never relies on torch's RNG streams, so the same seed gives the same network here, in the
golden generator (which loads them into the REFERENCE modules) and on the GPU box.
RDB conv weights ~ N(0, (0.1*sqrt(2/fan_in))^2) like the reference initialisation
(arch_util.py:12-40 with scale 0.1), other convs ~ U(+-1/sqrt(fan_in)); biases are small and
NON-zero so bias paths are exercised.
"""
import math
from collections import OrderedDict

import numpy as np


def rrdbnet_param_shapes(num_in_ch, num_out_ch, scale=4, num_feat=64, num_block=23, num_grow_ch=32):
    """(name, shape) in state_dict order of RRDBNet (rrdbnet_arch.py:94-101)."""
    cin = num_in_ch * {4: 1, 2: 4, 1: 16}.get(scale, 1)
    out = []

    def conv(name, ci, co):
        out.append((f'{name}.weight', (co, ci, 3, 3)))
        out.append((f'{name}.bias', (co,)))

    conv('conv_first', cin, num_feat)
    for b in range(num_block):
        for r in (1, 2, 3):
            for k in range(1, 5):
                conv(f'body.{b}.rdb{r}.conv{k}', num_feat + (k - 1) * num_grow_ch, num_grow_ch)
            conv(f'body.{b}.rdb{r}.conv5', num_feat + 4 * num_grow_ch, num_feat)
    for name in ('conv_body', 'conv_up1', 'conv_up2', 'conv_hr'):
        conv(name, num_feat, num_feat)
    conv('conv_last', num_feat, num_out_ch)
    return out


def conv_params(rng, shape_w, rdb_style, bias_scale=0.05):
    co, ci, kh, kw = shape_w
    fan_in = ci * kh * kw
    if rdb_style:
        w = rng.standard_normal(shape_w, dtype=np.float32) * np.float32(0.1 * math.sqrt(2.0 / fan_in))
    else:
        bound = 1.0 / math.sqrt(fan_in)
        w = (rng.random(shape_w, dtype=np.float32) * 2 - 1) * np.float32(bound)
    b = (rng.random((co,), dtype=np.float32) * 2 - 1) * np.float32(bias_scale)
    return w.astype(np.float32), b.astype(np.float32)


def rrdbnet_state_dict(seed=0, **cfg):
    """OrderedDict name -> np.float32 array for RRDBNet(**cfg)."""
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    shapes = rrdbnet_param_shapes(**cfg)
    for i in range(0, len(shapes), 2):
        (wn, ws), (bn, _) = shapes[i], shapes[i + 1]
        w, b = conv_params(rng, ws, rdb_style='.rdb' in wn)
        sd[wn], sd[bn] = w, b
    return sd


def msrresnet_param_shapes(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=16, upscale=4):
    """(name, shape) in state_dict order of MSRResNet (srresnet_arch.py:30-44)."""
    out = []

    def conv(name, ci, co):
        out.append((f'{name}.weight', (co, ci, 3, 3)))
        out.append((f'{name}.bias', (co,)))

    conv('conv_first', num_in_ch, num_feat)
    for b in range(num_block):
        conv(f'body.{b}.conv1', num_feat, num_feat)
        conv(f'body.{b}.conv2', num_feat, num_feat)
    if upscale == 4:
        conv('upconv1', num_feat, num_feat * 4)
        conv('upconv2', num_feat, num_feat * 4)
    else:
        conv('upconv1', num_feat, num_feat * upscale * upscale)
    conv('conv_hr', num_feat, num_feat)
    conv('conv_last', num_feat, num_out_ch)
    return out


def msrresnet_state_dict(seed=0, **cfg):
    """OrderedDict name -> np.float32 array for MSRResNet(**cfg): residual-block convs ~ kaiming_normal * 0.1 (the
    reference's init), the others ~ U(+-1/sqrt(fan_in)) so that the head and tail carry signal; small non-zero biases."""
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    shapes = msrresnet_param_shapes(**cfg)
    for i in range(0, len(shapes), 2):
        (wn, ws), (bn, _) = shapes[i], shapes[i + 1]
        w, b = conv_params(rng, ws, rdb_style=wn.startswith('body.'))
        sd[wn], sd[bn] = w, b
    return sd


def rdb_state_dict(seed, num_feat=64, num_grow_ch=32, prefix=''):
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    for k in range(1, 6):
        ci = num_feat + (k - 1) * num_grow_ch
        co = num_grow_ch if k < 5 else num_feat
        w, b = conv_params(rng, (co, ci, 3, 3), rdb_style=True)
        sd[f'{prefix}conv{k}.weight'], sd[f'{prefix}conv{k}.bias'] = w, b
    return sd


def rrdb_state_dict(seed, num_feat=64, num_grow_ch=32):
    sd = OrderedDict()
    for r in (1, 2, 3):
        sd.update(rdb_state_dict(seed * 10 + r, num_feat, num_grow_ch, prefix=f'rdb{r}.'))
    return sd


def uniform_input(seed, shape):
    """U[0,1) fp32 images, the benchmark's synthetic input."""
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def gaussian(seed, shape):
    """N(0, 1) draws in float64 rounded to fp32: upstream gradients of the golden backward runs."""
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def signed_input(seed, shape, scale=1.0):
    """Zero-mean features for block-level tests."""
    return ((np.random.default_rng(seed).random(shape, dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)


def vgg128_param_shapes(num_in_ch, num_feat, input_size=128):
    """(name, shape, kind) in state_dict order of VGGStyleDiscriminator128 (discriminator_arch.py:21-46) or, with
    input_size=256, VGGStyleDiscriminator256 (:75-120: one more 8nf -> 8nf stage)."""
    nf = num_feat
    out = []

    def conv(name, ci, co, k, bias):
        out.append((f'{name}.weight', (co, ci, k, k), 'conv'))
        if bias:
            out.append((f'{name}.bias', (co,), 'bias'))

    def bn(name, c):
        out.extend([(f'{name}.weight', (c,), 'bn_w'), (f'{name}.bias', (c,), 'bias'), (f'{name}.running_mean', (c,), 'rm'),
                    (f'{name}.running_var', (c,), 'rv'), (f'{name}.num_batches_tracked', (), 'nbt')])

    conv('conv0_0', num_in_ch, nf, 3, True)
    conv('conv0_1', nf, nf, 4, False)
    bn('bn0_1', nf)
    widths = [(nf, nf * 2), (nf * 2, nf * 4), (nf * 4, nf * 8), (nf * 8, nf * 8)] + ([(nf * 8, nf * 8)] if input_size == 256 else [])
    for i, (ci, co) in enumerate(widths, start=1):
        conv(f'conv{i}_0', ci, co, 3, False)
        bn(f'bn{i}_0', co)
        conv(f'conv{i}_1', co, co, 4, False)
        bn(f'bn{i}_1', co)
    out.extend([('linear1.weight', (100, nf * 8 * 16), 'lin'), ('linear1.bias', (100,), 'bias'),
                ('linear2.weight', (1, 100), 'lin'), ('linear2.bias', (1,), 'bias')])
    return out


def vgg128_state_dict(seed, num_in_ch=3, num_feat=64, input_size=128):
    """Deterministic VGGStyleDiscriminator128 / 256 state (non-trivial BN affine and running statistics)."""
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    for name, shape, kind in vgg128_param_shapes(num_in_ch, num_feat, input_size):
        if kind == 'conv':
            fan_in = shape[1] * shape[2] * shape[3]
            sd[name] = (rng.standard_normal(shape, dtype=np.float32) * np.float32(math.sqrt(2.0 / fan_in) * 0.7)).astype(np.float32)
        elif kind == 'lin':
            sd[name] = ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(1.0 / math.sqrt(shape[1]))).astype(np.float32)
        elif kind == 'bias':
            sd[name] = ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(0.1)).astype(np.float32)
        elif kind == 'bn_w':
            sd[name] = (1.0 + (rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(0.2)).astype(np.float32)
        elif kind == 'rm':
            sd[name] = ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(0.1)).astype(np.float32)
        elif kind == 'rv':
            sd[name] = (0.5 + rng.random(shape, dtype=np.float32)).astype(np.float32)
        else:
            sd[name] = np.array(0, dtype=np.int64)
    return sd


def smooth_pairs(seed, n, size, scale=4):
    """(lq, gt) batches with learnable structure for end-to-end training checks: gt = bicubic x8 enlargement of uniform
    noise (smooth colour fields in [0, 1], [n, 3, size, size]), lq = its scale x scale box average."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(n, 3, size // 8 + 2, size // 8 + 2, generator=g)
    gt = F.interpolate(low, scale_factor=8, mode='bicubic', align_corners=False)[:, :, 8:8 + size, 8:8 + size].clamp(0, 1)
    return F.avg_pool2d(gt, scale), gt.contiguous()


def niqe_image(seed, h, w, c=3):
    """Seeded uint8 HWC image with some spatial structure for the NIQE fixtures: box-smoothed noise plus a gradient plus fine
    noise (float64 elementwise arithmetic only, so the bytes are the same on every machine)."""
    rng = np.random.default_rng(seed)
    x = rng.random((h, w, c))
    for _ in range(3):
        x = (x + np.roll(x, 1, 0) + np.roll(x, -1, 0) + np.roll(x, 1, 1) + np.roll(x, -1, 1)) / 5
    x = (x - x.min()) / (x.max() - x.min())
    g = np.linspace(0, 1, w)[None, :, None] * np.linspace(0.3, 1, h)[:, None, None]
    x = 0.6 * x + 0.3 * g + 0.1 * rng.random((h, w, c))
    return np.clip(np.round(x * 255), 0, 255).astype(np.uint8)


def rcan_param_shapes(num_in_ch=3, num_out_ch=3, num_feat=64, num_group=10, num_block=16, squeeze_factor=16, upscale=4, **_):
    """(name, shape) in state_dict order of RCAN (rcan_arch.py:27-135; Upsample of arch_util.py)."""
    out = []
    hid = num_feat // squeeze_factor

    def conv(name, ci, co, k=3):
        out.append((f'{name}.weight', (co, ci, k, k)))
        out.append((f'{name}.bias', (co,)))

    conv('conv_first', num_in_ch, num_feat)
    for g in range(num_group):
        for b in range(num_block):
            pre = f'body.{g}.residual_group.{b}.rcab'
            conv(f'{pre}.0', num_feat, num_feat)
            conv(f'{pre}.2', num_feat, num_feat)
            conv(f'{pre}.3.attention.1', num_feat, hid, 1)
            conv(f'{pre}.3.attention.3', hid, num_feat, 1)
        conv(f'body.{g}.conv', num_feat, num_feat)
    conv('conv_after_body', num_feat, num_feat)
    stages = [3] if upscale == 3 else [2] * (int(upscale).bit_length() - 1)
    for i, r in enumerate(stages):
        conv(f'upsample.{2 * i}', num_feat, r * r * num_feat)
    conv('conv_last', num_feat, num_out_ch)
    return out


def rcan_state_dict(seed=0, **cfg):
    """OrderedDict name -> np.float32 array for RCAN(**cfg): the 3x3 convs inside the body ~ kaiming_normal * 0.1 (so that
    the residual chain stays of the input's size over many blocks), the others and the attention's 1x1 convs
    ~ U(+-1/sqrt(fan_in)); small non-zero biases, larger (+-0.5) on the attention so its ReLU and sigmoid see both signs."""
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    shapes = rcan_param_shapes(**cfg)
    for i in range(0, len(shapes), 2):
        (wn, ws), (bn, _) = shapes[i], shapes[i + 1]
        ca = '.attention.' in wn
        w, b = conv_params(rng, ws, rdb_style=wn.startswith('body.') and not ca, bias_scale=0.5 if ca else 0.05)
        sd[wn], sd[bn] = w, b
    return sd


def ridnet_param_shapes(in_channels=3, mid_channels=64, out_channels=3, num_block=4, **_):
    """(name, shape) in state_dict (= named_parameters) order of RIDNet (ridnet_arch.py:138-180)."""
    out = []
    mid, hid = mid_channels, mid_channels // 16

    def conv(name, ci, co, k=3):
        out.append((f'{name}.weight', (co, ci, k, k)))
        out.append((f'{name}.bias', (co,)))

    conv('sub_mean', in_channels, in_channels, 1)
    conv('add_mean', out_channels, out_channels, 1)
    conv('head', in_channels, mid)
    for b in range(num_block):
        pre = f'body.{b}'
        conv(f'{pre}.merge.dilation1.0', mid, mid)
        conv(f'{pre}.merge.dilation1.2', mid, mid)
        conv(f'{pre}.merge.dilation2.0', mid, mid)
        conv(f'{pre}.merge.dilation2.2', mid, mid)
        conv(f'{pre}.merge.aggregation.0', 2 * mid, mid)
        conv(f'{pre}.block1.conv1', mid, mid)
        conv(f'{pre}.block1.conv2', mid, mid)
        conv(f'{pre}.block2.body.0', mid, mid)
        conv(f'{pre}.block2.body.2', mid, mid)
        conv(f'{pre}.block2.body.4', mid, mid, 1)
        conv(f'{pre}.ca.attention.1', mid, hid, 1)
        conv(f'{pre}.ca.attention.3', hid, mid, 1)
    conv('tail', mid, out_channels)
    return out


def ridnet_state_dict(seed=0, img_range=255., rgb_mean=(0.4488, 0.4371, 0.4040), **cfg):
    """OrderedDict name -> np.float32 array for RIDNet(**cfg): the MeanShift layers near their initial eye(3) and
    -/+ img_range * mean, perturbed (+-0.05 on the mix, +-1 on the bias) so that both act as full 3x3 mixes; ResidualBlockNoBN's
    convs ~ kaiming_normal * 0.1 as initialised there; every other conv ~ U(+-1/sqrt(fan_in)) with small non-zero biases, larger
    (+-0.5) on the attention so its ReLU and sigmoid see both signs."""
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    shapes = ridnet_param_shapes(**cfg)
    mean = np.asarray(rgb_mean, np.float64)
    for i in range(0, len(shapes), 2):
        (wn, ws), (bn, _) = shapes[i], shapes[i + 1]
        if wn in ('sub_mean.weight', 'add_mean.weight'):
            sign = -1.0 if wn.startswith('sub') else 1.0
            w = np.eye(3, dtype=np.float32).reshape(3, 3, 1, 1) + (rng.random(ws, dtype=np.float32) * 2 - 1) * np.float32(0.05)
            b = (sign * img_range * mean + (rng.random(3) * 2 - 1)).astype(np.float32)
        else:
            ca = '.attention.' in wn
            w, b = conv_params(rng, ws, rdb_style='.block1.' in wn, bias_scale=0.5 if ca else 0.05)
        sd[wn], sd[bn] = w.astype(np.float32), b
    return sd


def gfpgan_param_shapes(**cfg):
    """(name, shape) of every state_dict entry (parameters and the noise buffers, in state_dict order) of GFPGANv1OCR(**cfg),
    read from the module built on the meta device (no memory, no kernels)."""
    import torch
    from ..archs.gfpganv1_ocr_arch import GFPGANv1OCR
    with torch.device('meta'):
        net = GFPGANv1OCR(**cfg)
    return [(k, tuple(v.shape)) for k, v in net.state_dict().items()]


def gfpgan_state_dict(seed=0, lr_mlp=0.01, **cfg):
    """OrderedDict name -> np.float32 array for GFPGANv1OCR(**cfg): weights ~ N(0, 1) as initialised (the style MLP's / lr_mlp), the
    noise buffers ~ N(0, 1), and — unlike the default initialisation, which zeroes the noise path and leaves the SFT scale at 1 —
    noise strengths ~ U(0.05, 0.25), modulation and SFT-scale biases ~ 1 + U(+-0.2), every other bias ~ U(+-0.1)."""
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    for name, shape in gfpgan_param_shapes(lr_mlp=lr_mlp, **cfg):
        leaf = name.rsplit('.', 1)[-1]
        if '.noises.noise' in name:
            v = rng.standard_normal(shape)
        elif leaf == 'weight' and shape == (1,):
            v = rng.uniform(0.05, 0.25, shape)
        elif leaf == 'bias' and ('.modulation.' in name or (name.startswith('condition_scale.') and '.2.' in name)):
            v = 1 + rng.uniform(-0.2, 0.2, shape)
        elif leaf == 'bias':
            v = rng.uniform(-0.1, 0.1, shape)
        elif '.style_mlp.' in name:
            v = rng.standard_normal(shape) / lr_mlp
        else:
            v = rng.standard_normal(shape)
        sd[name] = np.asarray(v, np.float32)
    return sd


def edsr_param_shapes(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=16, upscale=4, **_):
    """(name, shape) in state_dict order of EDSR (edsr_arch.py:44-48): upscale 2^n or 3."""
    out = []

    def conv(name, ci, co):
        out.append((f'{name}.weight', (co, ci, 3, 3)))
        out.append((f'{name}.bias', (co,)))

    conv('conv_first', num_in_ch, num_feat)
    for b in range(num_block):
        conv(f'body.{b}.conv1', num_feat, num_feat)
        conv(f'body.{b}.conv2', num_feat, num_feat)
    conv('conv_after_body', num_feat, num_feat)
    if upscale == 3:
        conv('upsample.0', num_feat, 9 * num_feat)
    else:
        for k in range(int(round(math.log2(upscale)))):
            conv(f'upsample.{2 * k}', num_feat, 4 * num_feat)
    conv('conv_last', num_feat, num_out_ch)
    return out


def edsr_state_dict(seed=0, **cfg):
    """OrderedDict name -> np.float32 array for EDSR(**cfg): every conv ~ U(+-1/sqrt(fan_in)) (the reference builds its blocks
    with pytorch_init=True, so no conv is scaled down), small non-zero biases."""
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    shapes = edsr_param_shapes(**cfg)
    for i in range(0, len(shapes), 2):
        (wn, ws), (bn, _) = shapes[i], shapes[i + 1]
        w, b = conv_params(rng, ws, rdb_style=False)
        sd[wn], sd[bn] = w, b
    return sd


def tof_param_shapes():
    """(name, shape) in state_dict order of TOFlow (tof_arch.py:111-126): 114 entries, the ``mean`` / ``std`` buffers and every
    BatchNorm ``num_batches_tracked`` (shape ()) included."""
    out = [('mean', (1, 3, 1, 1)), ('std', (1, 3, 1, 1))]
    for level in range(4):
        for i, (cin, cout) in enumerate(((8, 32), (32, 64), (64, 32), (32, 16), (16, 2))):
            base = f'spynet.basic_module.{level}.basic_module'
            out.append((f'{base}.{3 * i}.weight', (cout, cin, 7, 7)))
            if i == 4:
                out.append((f'{base}.{3 * i}.bias', (cout,)))
                continue
            for p in ('weight', 'bias', 'running_mean', 'running_var'):
                out.append((f'{base}.{3 * i + 1}.{p}', (cout,)))
            out.append((f'{base}.{3 * i + 1}.num_batches_tracked', ()))
    for name, cin, cout, k in (('conv_1', 21, 64, 9), ('conv_2', 64, 64, 9), ('conv_3', 64, 64, 1), ('conv_4', 64, 3, 1)):
        out.append((f'{name}.weight', (cout, cin, k, k)))
        out.append((f'{name}.bias', (cout,)))
    return out


def tof_state_dict(seed=0, flow_gain=4.0, flow_bias=0.2, recon_gain=2.0):
    """OrderedDict name -> numpy array for TOFlow, drawn in state_dict order from one seeded generator.  Convs ~ U(+-1/sqrt(fan_in))
    (nn.Conv2d's default range) with these departures, without which the flows stay far below a pixel, BatchNorm is the identity
    and the 9x9 path barely moves the output: BatchNorm gamma ~ U(0.5, 1.5), beta and running_mean ~ U(-0.3, 0.3), running_var ~
    U(0.5, 2) and num_batches_tracked = 100; the last conv of every level has its weight scaled by ``flow_gain`` and its bias ~
    U(+-flow_bias); the four reconstruction convs are scaled by ``recon_gain``."""
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    for name, shape in tof_param_shapes():
        leaf = name.rsplit('.', 1)[-1]
        if name == 'mean':
            v = np.array([0.485, 0.456, 0.406]).reshape(shape)
        elif name == 'std':
            v = np.array([0.229, 0.224, 0.225]).reshape(shape)
        elif leaf == 'num_batches_tracked':
            sd[name] = np.array(100, np.int64)
            continue
        elif len(shape) == 4:
            bound = 1.0 / math.sqrt(shape[1] * shape[2] * shape[3])
            v = rng.uniform(-bound, bound, shape)
            if name.startswith('conv_'):
                v = v * recon_gain
            elif shape[0] == 2:
                v = v * flow_gain
            fan_bound = bound
        elif leaf == 'running_var':
            v = rng.uniform(0.5, 2.0, shape)
        elif leaf == 'running_mean':
            v = rng.uniform(-0.3, 0.3, shape)
        elif '.basic_module.' in name and shape[0] != 2:       # BatchNorm gamma / beta
            v = rng.uniform(0.5, 1.5, shape) if leaf == 'weight' else rng.uniform(-0.3, 0.3, shape)
        elif shape[0] == 2:                                     # bias of a level's last conv
            v = rng.uniform(-flow_bias, flow_bias, shape)
        else:                                                   # bias of a reconstruction conv
            v = rng.uniform(-fan_bound, fan_bound, shape)
        sd[name] = np.asarray(v, np.float32)
    return sd


_DUF_BLOCKS = {16: (3, 32), 28: (9, 16), 52: (21, 16)}   # num_layer -> (num_block, num_grow_ch)


def duf_param_shapes(num_layer=52, scale=4):
    """[(name, shape)] of DUF's state_dict, in the reference's order (BatchNorm3d: weight, bias, running_mean, running_var,
    num_batches_tracked)."""
    nb, g = _DUF_BLOCKS[num_layer]
    out = []

    def bn(name, c):
        out.extend([(f'{name}.weight', (c,)), (f'{name}.bias', (c,)), (f'{name}.running_mean', (c,)), (f'{name}.running_var', (c,)),
                    (f'{name}.num_batches_tracked', ())])

    def conv(name, cout, cin, kt, k):
        out.extend([(f'{name}.weight', (cout, cin, kt, k, k)), (f'{name}.bias', (cout,))])

    def dense(name, c):
        bn(f'{name}.0', c)
        conv(f'{name}.2', c, c, 1, 1)
        bn(f'{name}.3', c)
        conv(f'{name}.5', g, c, 3, 3)

    conv('conv3d1', 64, 3, 1, 3)
    c = 64
    for i in range(nb):
        dense(f'dense_block1.dense_blocks.{i}', c)
        c += g
    for i in range(3):
        dense(f'dense_block2.temporal_reduce{i + 1}', c)
        c += g
    bn('bn3d2', c)
    conv('conv3d2', 256, c, 1, 3)
    s2 = scale * scale
    conv('conv3d_r1', 256, 256, 1, 1)
    conv('conv3d_r2', 3 * s2, 256, 1, 1)
    conv('conv3d_f1', 512, 256, 1, 1)
    conv('conv3d_f2', 25 * s2, 512, 1, 1)
    return out


def duf_state_dict(seed=0, num_layer=52, scale=4, conv_gain=2.0, filter_gain=12.0, res_gain=3.0):
    """OrderedDict name -> numpy array for DUF, drawn in state_dict order from one seeded generator.  With the default
    initialisation every BatchNorm is the identity, the 25 filter weights are near uniform and the residual is invisible, which
    tests nothing.  So: convs ~ U(+-1/sqrt(fan_in)) scaled by ``conv_gain`` (a ReLU halves the energy, the uniform range thirds it),
    biases ~ U(+-1/sqrt(fan_in)); BatchNorm gamma ~ U(0.5, 1.5), beta and running_mean ~ U(-0.3, 0.3), running_var ~ U(0.5, 2),
    num_batches_tracked = 100; ``conv3d_f2`` is scaled by ``filter_gain`` (a peaked softmax) and ``conv3d_r2`` by ``res_gain`` (a
    visible residual)."""
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    fan_bound = 1.0
    for name, shape in duf_param_shapes(num_layer, scale):
        leaf = name.rsplit('.', 1)[-1]
        if leaf == 'num_batches_tracked':
            sd[name] = np.array(100, np.int64)
            continue
        if len(shape) == 5:
            fan_bound = 1.0 / math.sqrt(shape[1] * shape[2] * shape[3] * shape[4])
            gain = filter_gain if name.startswith('conv3d_f2') else res_gain if name.startswith('conv3d_r2') else conv_gain
            v = rng.uniform(-fan_bound, fan_bound, shape) * gain
        elif leaf == 'running_var':
            v = rng.uniform(0.5, 2.0, shape)
        elif leaf == 'running_mean':
            v = rng.uniform(-0.3, 0.3, shape)
        elif name.rsplit('.', 2)[-2] in ('0', '3', 'bn3d2'):   # BatchNorm gamma / beta
            v = rng.uniform(0.5, 1.5, shape) if leaf == 'weight' else rng.uniform(-0.3, 0.3, shape)
        else:                                                   # bias of a conv
            v = rng.uniform(-fan_bound, fan_bound, shape)
        sd[name] = np.asarray(v, np.float32)
    return sd
