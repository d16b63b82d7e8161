"""The recurrent video networks BasicVSR and IconVSR (basicsr/archs/basicvsr_arch.py) restated in numpy float64, with the seeded
weight and input generators the fixtures tests/golden/g_ze_basicvsr.npz and g_zf_iconvsr.npz were recorded with
(tools/make_golden_basicvsr.py, tools/make_golden_iconvsr.py).  IconVSR's keyframe branch comes from tests/edvr_restate.py and
tests/dcn_restate.py (torch float64), on windows of the mirrored clip built here from the definition.

The restatement is ``propagate``: it takes the flows as inputs and does not restate SpyNet (tests/flow_restate.py does).  The warp
is flow_restate's; added here are a shifted-slice 3x3 convolution, the pixel shuffle and the half-pixel x4 bilinear upsampling.
No torch, no GPU: the GPU tests compare the device results against this, the host tests compare this against the reference's own
recorded outputs.
"""
import numpy as np

import flow_restate as FR

CASES = (('basicvsr_b1_n3_33x40', 1, 3, 33, 40), ('basicvsr_b2_n2_34x33', 2, 2, 34, 33))
NUM_FEAT, NUM_BLOCK = 64, 2


# ------------------------------------------------------------------------------------------------------------ weights
def trunk_keys(prefix, num_block):
    keys = [f'{prefix}.main.0.weight', f'{prefix}.main.0.bias']
    for i in range(num_block):
        for c in ('conv1', 'conv2'):
            keys += [f'{prefix}.main.2.{i}.{c}.weight', f'{prefix}.main.2.{i}.{c}.bias']
    return keys


def trunk_weights(rng, prefix, cin, num_feat, num_block, scale):
    """One ConvResidualBlocks: the first conv in nn.Conv2d's default range, the block convs N(0, 2 / fan_in) * ``scale`` with a small
    uniform bias (the reference's own initialisation, * 0.1 and bias 0, leaves the residual branches invisible at fp32 resolution)."""
    sd = {}
    bound = 1.0 / np.sqrt(cin * 9.0)
    sd[f'{prefix}.main.0.weight'] = rng.uniform(-bound, bound, (num_feat, cin, 3, 3)).astype(np.float32)
    sd[f'{prefix}.main.0.bias'] = rng.uniform(-bound, bound, (num_feat,)).astype(np.float32)
    for i in range(num_block):
        for c in ('conv1', 'conv2'):
            std = np.sqrt(2.0 / (num_feat * 9.0)) * scale
            sd[f'{prefix}.main.2.{i}.{c}.weight'] = (rng.standard_normal((num_feat, num_feat, 3, 3)) * std).astype(np.float32)
            sd[f'{prefix}.main.2.{i}.{c}.bias'] = rng.uniform(-0.05, 0.05, (num_feat,)).astype(np.float32)
    return sd


def _conv_default(rng, sd, name, cout, cin, k):
    bound = 1.0 / np.sqrt(cin * k * k)
    sd[name + '.weight'] = rng.uniform(-bound, bound, (cout, cin, k, k)).astype(np.float32)
    sd[name + '.bias'] = rng.uniform(-bound, bound, (cout,)).astype(np.float32)


def basicvsr_weights(seed, num_feat=NUM_FEAT, num_block=NUM_BLOCK, scale=0.5):
    """state_dict (numpy float32) of BasicVSR WITHOUT the ``spynet.*`` entries, in the reference's key order."""
    rng = np.random.default_rng(seed)
    sd = {}
    sd.update(trunk_weights(rng, 'backward_trunk', num_feat + 3, num_feat, num_block, scale))
    sd.update(trunk_weights(rng, 'forward_trunk', num_feat + 3, num_feat, num_block, scale))
    _conv_default(rng, sd, 'fusion', num_feat, 2 * num_feat, 1)
    _conv_default(rng, sd, 'upconv1', 4 * num_feat, num_feat, 3)
    _conv_default(rng, sd, 'upconv2', 256, num_feat, 3)
    _conv_default(rng, sd, 'conv_hr', 64, 64, 3)
    _conv_default(rng, sd, 'conv_last', 3, 64, 3)
    return sd


def basicvsr_keys(num_block):
    spy = ['spynet.mean', 'spynet.std'] + [f'spynet.basic_module.{lv}.basic_module.{i}.{p}' for lv in range(6) for i in (0, 2, 4, 6, 8)
                                           for p in ('weight', 'bias')]
    rest = trunk_keys('backward_trunk', num_block) + trunk_keys('forward_trunk', num_block)
    for name in ('fusion', 'upconv1', 'upconv2', 'conv_hr', 'conv_last'):
        rest += [name + '.weight', name + '.bias']
    return spy + rest


def clip_input(seed, b, n, h, w):
    """float32 [b, n, 3, h, w] in [0, 1]: flow_restate's scene, every frame the scene displaced a little further."""
    frames = []
    for i in range(n):
        ref, supp = FR.spynet_inputs(seed + 10 * i, b, h, w)
        frames.append(ref if i % 2 == 0 else supp)
    return np.stack(frames, 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- ops
def conv3x3(x, weight, bias):
    """nn.Conv2d(cin, cout, 3, 1, 1) on [N, C, H, W] in float64: nine shifted slices of the zero-padded input."""
    x, weight = np.asarray(x, np.float64), np.asarray(weight, np.float64)
    n, c, h, w = x.shape
    xp = np.zeros((n, c, h + 2, w + 2))
    xp[:, :, 1:-1, 1:-1] = x
    out = np.zeros((n, weight.shape[0], h, w))
    taps = np.ascontiguousarray(weight.transpose(2, 3, 0, 1))       # [3][3][cout][cin]: dense operands for the matrix product
    for dy in range(3):
        for dx in range(3):
            out += np.matmul(taps[dy, dx], xp[:, :, dy:dy + h, dx:dx + w].reshape(n, c, h * w)).reshape(n, -1, h, w)
    return out + np.asarray(bias, np.float64)[None, :, None, None]


def conv1x1(x, weight, bias):
    x = np.asarray(x, np.float64)
    n, c, h, w = x.shape
    return np.matmul(np.asarray(weight, np.float64)[:, :, 0, 0], x.reshape(n, c, h * w)).reshape(n, -1, h, w) + \
        np.asarray(bias, np.float64)[None, :, None, None]


def lrelu(x, slope=0.1):
    return np.where(x > 0, x, x * slope)


def pixel_shuffle(x, r=2):
    n, c, h, w = x.shape
    return x.reshape(n, c // (r * r), r, r, h, w).transpose(0, 1, 4, 2, 5, 3).reshape(n, c // (r * r), h * r, w * r)


def bilinear_x4(x):
    """F.interpolate(x, scale_factor=4, mode='bilinear', align_corners=False): half-pixel centres, source clamped at 0."""
    n, c, h, w = x.shape
    return FR.resize_half_pixel(np.asarray(x, np.float64), 4 * h, 4 * w)


def trunk(sd, prefix, x, num_block):
    """ConvResidualBlocks: conv + LeakyReLU(0.1), then num_block times x + conv2(relu(conv1(x)))."""
    x = lrelu(conv3x3(x, sd[f'{prefix}.main.0.weight'], sd[f'{prefix}.main.0.bias']))
    for i in range(num_block):
        p = f'{prefix}.main.2.{i}'
        t = np.maximum(conv3x3(x, sd[p + '.conv1.weight'], sd[p + '.conv1.bias']), 0.0)
        x = x + conv3x3(t, sd[p + '.conv2.weight'], sd[p + '.conv2.bias'])
    return x


def basicvsr_propagate(sd, x, flows_forward, flows_backward, num_block=NUM_BLOCK, zero_backward=False):
    """BasicVSR.forward after get_flow: x [b, n, 3, h, w], flows [b, n - 1, 2, h, w] -> [b, n, 3, 4h, 4w], float64.
    ``zero_backward``: the backward branch's features replaced by zeros (the fixture tool's sensitivity check)."""
    x = np.asarray(x, np.float64)
    b, n, _, h, w = x.shape
    num_feat = sd['fusion.weight'].shape[0]
    out_l = [None] * n
    feat = np.zeros((b, num_feat, h, w))
    for i in range(n - 1, -1, -1):
        if i < n - 1:
            feat = FR.flow_warp(feat, np.asarray(flows_backward[:, i], np.float64).transpose(0, 2, 3, 1), 'zeros')
        feat = trunk(sd, 'backward_trunk', np.concatenate([x[:, i], feat], 1), num_block)
        out_l[i] = np.zeros_like(feat) if zero_backward else feat
    feat = np.zeros((b, num_feat, h, w))
    outs = []
    for i in range(n):
        if i > 0:
            feat = FR.flow_warp(feat, np.asarray(flows_forward[:, i - 1], np.float64).transpose(0, 2, 3, 1), 'zeros')
        feat = trunk(sd, 'forward_trunk', np.concatenate([x[:, i], feat], 1), num_block)
        out = lrelu(conv1x1(np.concatenate([out_l[i], feat], 1), sd['fusion.weight'], sd['fusion.bias']))
        out = lrelu(pixel_shuffle(conv3x3(out, sd['upconv1.weight'], sd['upconv1.bias'])))
        out = lrelu(pixel_shuffle(conv3x3(out, sd['upconv2.weight'], sd['upconv2.bias'])))
        out = lrelu(conv3x3(out, sd['conv_hr.weight'], sd['conv_hr.bias']))
        out = conv3x3(out, sd['conv_last.weight'], sd['conv_last.bias'])
        outs.append(out + bilinear_x4(x[:, i]))
    return np.stack(outs, 1)


# --------------------------------------------------------------------------------------------- dispatch, restated
def wino_eligible(cout, cin):
    """conv_wino_f32.hip: a conv has a Winograd image iff cout % 32 == 0 and cin >= 8."""
    return cout % 32 == 0 and cin >= 8


def trunk_convs(num_feat, num_block, cin_segs):
    """(cout, cin, cin_pad) of every conv of a trunk in launch order."""
    convs = [(num_feat, 3 + cin_segs * num_feat, 8 + cin_segs * num_feat)]
    return convs + [(num_feat, num_feat, num_feat)] * (2 * num_block)


def trunk_wino_launches(num_feat, num_block, cin_segs, h, w, mode):
    """Winograd launches of one sr_vsr_trunk_f32 call: mode 0 none; mode 1 the eligible convs when H * W >= 128 * 128; a forced
    tile variant (mode >= 2) every eligible conv."""
    if mode == 0 or (mode == 1 and h * w < 128 * 128):
        return 0
    return sum(wino_eligible(co, ci) for co, ci, _ in trunk_convs(num_feat, num_block, cin_segs))


def _align(v, a):
    return (v + a - 1) // a * a


def trunk_blob_bytes(num_feat, num_block, cin_segs, weight_floats, bias_floats, table_bytes):
    """sr_vsr_trunk_packed_bytes restated: per conv the direct weight and bias images (sizes from the library's own queries,
    ``weight_floats(cout, cin_pad)`` / ``bias_floats(cout)``), each rounded up to 64 floats; behind them 16 * cout * cin_pad
    floats per eligible conv; then the pack table of one row per image."""
    floats, rows = 0, 0
    convs = trunk_convs(num_feat, num_block, cin_segs)
    for co, ci, cp in convs:
        floats += _align(weight_floats(co, cp), 64) + _align(bias_floats(co), 64)
        rows += 1
    for co, ci, cp in convs:
        if wino_eligible(co, ci):
            floats += _align(16 * co * cp, 64)
            rows += 1
    return 4 * floats + table_bytes(rows)


# ------------------------------------------------------------------------------------------------------------ IconVSR
ICON_CASE = ('iconvsr_b1_n6_34x38', 1, 6, 34, 38, 4)     # padded to 36x40; keyframe_stride 4: keyframes 0, 4, 5


def iconvsr_weights(seed, num_feat=NUM_FEAT, num_block=NUM_BLOCK, scale=0.5):
    """state_dict (numpy float32) of IconVSR WITHOUT the ``edvr.*`` and ``spynet.*`` entries, in the reference's key order."""
    rng = np.random.default_rng(seed)
    sd = {}
    _conv_default(rng, sd, 'backward_fusion', num_feat, 2 * num_feat, 3)
    sd.update(trunk_weights(rng, 'backward_trunk', num_feat + 3, num_feat, num_block, scale))
    _conv_default(rng, sd, 'forward_fusion', num_feat, 2 * num_feat, 3)
    sd.update(trunk_weights(rng, 'forward_trunk', 2 * num_feat + 3, num_feat, num_block, scale))
    _conv_default(rng, sd, 'upconv1', 4 * num_feat, num_feat, 3)
    _conv_default(rng, sd, 'upconv2', 256, num_feat, 3)
    _conv_default(rng, sd, 'conv_hr', 64, 64, 3)
    _conv_default(rng, sd, 'conv_last', 3, 64, 3)
    return sd


def keyframes(n, stride):
    idx = list(range(0, n, stride))
    return idx if idx[-1] == n - 1 else idx + [n - 1]


def pad_spatial(x):
    """Reflect padding at the bottom and the right to multiples of 4."""
    h, w = x.shape[-2:]
    return np.pad(x, [(0, 0)] * (x.ndim - 2) + [(0, (4 - h % 4) % 4), (0, (4 - w % 4) % 4)], mode='reflect')


def iconvsr_propagate(sd, x, flows_forward, flows_backward, feats_keyframe, num_block=NUM_BLOCK):
    """IconVSR.forward after pad_spatial, get_flow and get_keyframe_feature (basicvsr_arch.py:210-248, before the crop): x
    [b, n, 3, h, w], flows [b, n - 1, 2, h, w], feats_keyframe {i: [b, num_feat, h, w]} -> [b, n, 3, 4h, 4w], float64."""
    x = np.asarray(x, np.float64)
    b, n, _, h, w = x.shape
    num_feat = sd['backward_fusion.weight'].shape[0]
    out_l = [None] * n
    feat = np.zeros((b, num_feat, h, w))
    for i in range(n - 1, -1, -1):
        if i < n - 1:
            feat = FR.flow_warp(feat, np.asarray(flows_backward[:, i], np.float64).transpose(0, 2, 3, 1), 'zeros')
        if i in feats_keyframe:
            feat = conv3x3(np.concatenate([feat, feats_keyframe[i]], 1), sd['backward_fusion.weight'], sd['backward_fusion.bias'])
        feat = trunk(sd, 'backward_trunk', np.concatenate([x[:, i], feat], 1), num_block)
        out_l[i] = feat
    feat = np.zeros((b, num_feat, h, w))
    outs = []
    for i in range(n):
        if i > 0:
            feat = FR.flow_warp(feat, np.asarray(flows_forward[:, i - 1], np.float64).transpose(0, 2, 3, 1), 'zeros')
        if i in feats_keyframe:
            feat = conv3x3(np.concatenate([feat, feats_keyframe[i]], 1), sd['forward_fusion.weight'], sd['forward_fusion.bias'])
        feat = trunk(sd, 'forward_trunk', np.concatenate([x[:, i], out_l[i], feat], 1), num_block)
        out = lrelu(pixel_shuffle(conv3x3(feat, sd['upconv1.weight'], sd['upconv1.bias'])))
        out = lrelu(pixel_shuffle(conv3x3(out, sd['upconv2.weight'], sd['upconv2.bias'])))
        out = lrelu(conv3x3(out, sd['conv_hr.weight'], sd['conv_hr.bias']))
        out = conv3x3(out, sd['conv_last.weight'], sd['conv_last.bias'])
        outs.append(out + bilinear_x4(x[:, i]))
    return np.stack(outs, 1)


# ------------------------------------------------------------------------------- IconVSR's keyframe branch, restated
def extractor_weights(seed, keys, shapes):
    """state_dict (numpy float32) of the EDVR feature extractor for the given (key, shape) list — the ``edvr.*`` entries of the
    reference's IconVSR with the prefix removed: weights N(0, 1.4^2 / fan_in), biases N(0, 0.1^2), the scales of
    tools/make_edvr_golden.py.  (The reference's own initialisation zeroes the offset convs: no deformation to test.)"""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shape in zip(keys, shapes):
        shape = tuple(int(d) for d in shape)
        if k.endswith('weight'):
            sd[k] = (rng.standard_normal(shape) * (1.4 / np.sqrt(shape[1] * shape[2] * shape[3]))).astype(np.float32)
        else:
            sd[k] = (rng.standard_normal(shape) * 0.1).astype(np.float32)
    return sd


def mirrored_windows(n, keyframe_idx, temporal_padding):
    """Per keyframe the frame indices of its EDVR window, from the definition (basicvsr_arch.py:183-194): the clip is extended by
    ``temporal_padding`` reflected frames at either end — [4, 3] + clip + [-4, -5] for 2, [6, 5, 4] + clip + [-5, -6, -7] for 3 —
    and keyframe i takes 2 * temporal_padding + 1 frames of the extended clip from position i."""
    lead, tail = ([4, 3], [n - 4, n - 5]) if temporal_padding == 2 else ([6, 5, 4], [n - 5, n - 6, n - 7])
    ext = lead + list(range(n)) + tail
    return {i: ext[i:i + 2 * temporal_padding + 1] for i in keyframe_idx}


def extractor(sd, x, deformable_groups=8):
    """EDVRFeatureExtractor.forward (basicvsr_arch.py:277-309) on a torch clip [b, t, 3, h, w] in its dtype, from the pieces of
    tests/edvr_restate.py and tests/dcn_restate.py: frames aligned one by one to the centre frame, then the TSA fusion."""
    import torch
    import edvr_restate as E
    import dcn_restate as D
    b, t, c, h, w = x.shape
    center = t // 2
    l1 = E._lrelu(E._conv(sd, 'conv_first', x.reshape(b * t, c, h, w)))
    for i in range(5):
        l1 = E._resblock(sd, f'feature_extraction.{i}', l1)
    l2 = E._lrelu(E._conv(sd, 'conv_l2_2', E._lrelu(E._conv(sd, 'conv_l2_1', l1, stride=2))))
    l3 = E._lrelu(E._conv(sd, 'conv_l3_2', E._lrelu(E._conv(sd, 'conv_l3_1', l2, stride=2))))
    l1, l2, l3 = l1.view(b, t, -1, h, w), l2.view(b, t, -1, h // 2, w // 2), l3.view(b, t, -1, h // 4, w // 4)
    pcd = E._sub(sd, 'pcd_align.')
    ref = [l1[:, center], l2[:, center], l3[:, center]]
    aligned = torch.stack([D.pcd_alignment(pcd, [l1[:, i], l2[:, i], l3[:, i]], ref, deformable_groups) for i in range(t)], dim=1)
    return E.tsa_fusion(E._sub(sd, 'fusion.'), aligned, center)


def keyframe_features(sd_edvr, x, keyframe_idx, temporal_padding=2):
    """{i: float64 [b, 64, h, w]} of the padded clip x (numpy [b, n, 3, h, w]) for an extractor state dict of numpy arrays."""
    import torch
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd_edvr.items()}
    xt = torch.from_numpy(np.asarray(x, np.float64))
    with torch.no_grad():
        return {i: extractor(sd, xt[:, idx]).numpy() for i, idx in mirrored_windows(x.shape[1], keyframe_idx, temporal_padding).items()}
