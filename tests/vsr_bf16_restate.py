"""A float64 model of the bf16 inference forward of BasicVSR and IconVSR: tests/vsr_restate.py with a bf16 round trip wherever the
HIP path stores or rounds a tensor, and nowhere else.

Rounded (``rt``, through fp32 as the kernels do): the frame block of a trunk's input; the warped feature; every conv output after
its epilogue (bias, activation, and ``x + conv2``: one rounding); the keyframe features as the
fusion conv reads them and the keyframe fusion conv's output; the packed weights; the head's
activations (the 1x1 fusion, upconv1 / upconv2 with their LeakyReLU, conv_hr).
Not rounded: the flows, the biases, conv_last's output (fp32 NCHW) and the x4 bilinear base of the fp32 frames.
IconVSR's keyframe extractor is built from the pieces of tests/edvr_bf16_restate.py (``Model``), which rounds where EDVR's bf16 ops
table does.

``rounding=False`` switches every round trip off; the model then performs vsr_restate's operations in its order and reproduces it
exactly (tests/test_vsr_bf16_host.py asserts that).  ``acc32=True`` evaluates every convolution's sum in float32: the CPU proxy of
what the HIP path's fp32 accumulation adds to the roundings.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edvr_bf16_restate as EB  # noqa: E402
import flow_restate as FR  # noqa: E402
import vsr_restate as V  # noqa: E402


class Model:
    def __init__(self, sd, rounding=True, acc32=False):
        self.rounding, self.acc32 = rounding, acc32
        self.sd = {k: (self.rt(v) if k.endswith('weight') else np.asarray(v, np.float64)) for k, v in sd.items()}

    def rt(self, a):
        a = np.asarray(a, np.float64)
        if not self.rounding:
            return a
        return torch.from_numpy(np.ascontiguousarray(a)).float().bfloat16().double().numpy()

    def conv(self, x, name):
        w, b = self.sd[name + '.weight'], self.sd[name + '.bias']
        if self.acc32:
            y = F.conv2d(torch.from_numpy(np.ascontiguousarray(x)).float(), torch.from_numpy(w).float(), torch.from_numpy(b).float(),
                         padding=w.shape[2] // 2)
            return y.double().numpy()
        return V.conv3x3(x, w, b) if w.shape[2] == 3 else V.conv1x1(x, w, b)

    def trunk(self, prefix, x, num_block):
        x = self.rt(V.lrelu(self.conv(x, f'{prefix}.main.0')))
        for i in range(num_block):
            p = f'{prefix}.main.2.{i}'
            t = self.rt(np.maximum(self.conv(x, p + '.conv1'), 0.0))
            x = self.rt(x + self.conv(t, p + '.conv2'))
        return x

    def warp(self, feat, flow):
        return self.rt(FR.flow_warp(feat, np.asarray(flow, np.float64).transpose(0, 2, 3, 1), 'zeros'))

    def head(self, out, frame):
        out = self.rt(V.lrelu(V.pixel_shuffle(self.conv(out, 'upconv1'))))
        out = self.rt(V.lrelu(V.pixel_shuffle(self.conv(out, 'upconv2'))))
        out = self.rt(V.lrelu(self.conv(out, 'conv_hr')))
        return self.conv(out, 'conv_last') + V.bilinear_x4(frame)

    def basicvsr_propagate(self, x, flows_forward, flows_backward, num_block=V.NUM_BLOCK, zero_backward=False):
        x = np.asarray(x, np.float64)
        b, n, _, h, w = x.shape
        num_feat = self.sd['fusion.weight'].shape[0]
        out_l = [None] * n
        feat = np.zeros((b, num_feat, h, w))
        for i in range(n - 1, -1, -1):
            if i < n - 1:
                feat = self.warp(feat, flows_backward[:, i])
            feat = self.trunk('backward_trunk', np.concatenate([self.rt(x[:, i]), feat], 1), num_block)
            out_l[i] = np.zeros_like(feat) if zero_backward else feat
        feat = np.zeros((b, num_feat, h, w))
        outs = []
        for i in range(n):
            if i > 0:
                feat = self.warp(feat, flows_forward[:, i - 1])
            feat = self.trunk('forward_trunk', np.concatenate([self.rt(x[:, i]), feat], 1), num_block)
            out = self.rt(V.lrelu(self.conv(np.concatenate([out_l[i], feat], 1), 'fusion')))
            outs.append(self.head(out, x[:, i]))
        return np.stack(outs, 1)

    def iconvsr_propagate(self, x, flows_forward, flows_backward, feats_keyframe, num_block=V.NUM_BLOCK):
        x = np.asarray(x, np.float64)
        b, n, _, h, w = x.shape
        num_feat = self.sd['backward_fusion.weight'].shape[0]
        kf = {i: self.rt(f) for i, f in feats_keyframe.items()}          # stored as CB16 (already bf16 from the bf16 extractor)
        out_l = [None] * n
        feat = np.zeros((b, num_feat, h, w))
        for i in range(n - 1, -1, -1):
            if i < n - 1:
                feat = self.warp(feat, flows_backward[:, i])
            if i in feats_keyframe:
                feat = self.rt(self.conv(np.concatenate([feat, kf[i]], 1), 'backward_fusion'))
            feat = self.trunk('backward_trunk', np.concatenate([self.rt(x[:, i]), feat], 1), num_block)
            out_l[i] = feat
        feat = np.zeros((b, num_feat, h, w))
        outs = []
        for i in range(n):
            if i > 0:
                feat = self.warp(feat, flows_forward[:, i - 1])
            if i in feats_keyframe:
                feat = self.rt(self.conv(np.concatenate([feat, kf[i]], 1), 'forward_fusion'))
            feat = self.trunk('forward_trunk', np.concatenate([self.rt(x[:, i]), out_l[i], feat], 1), num_block)
            outs.append(self.head(feat, x[:, i]))
        return np.stack(outs, 1)


def basicvsr_propagate(sd, x, flows_forward, flows_backward, rounding=True, acc32=False, **kw):
    return Model(sd, rounding, acc32).basicvsr_propagate(x, flows_forward, flows_backward, **kw)


def iconvsr_propagate(sd, x, flows_forward, flows_backward, feats_keyframe, rounding=True, acc32=False, **kw):
    return Model(sd, rounding, acc32).iconvsr_propagate(x, flows_forward, flows_backward, feats_keyframe, **kw)


# ------------------------------------------------------------------------------- IconVSR's keyframe branch in bf16
def extractor(sd, x, rounding=True, acc32=False, deformable_groups=8):
    """vsr_restate.extractor on edvr_bf16_restate.Model's layers: a torch clip [b, t, 3, h, w] (float64) -> [b, 64, h, w]."""
    m = EB.Model(sd, rounding, acc32)
    b, t, c, h, w = x.shape
    center = t // 2
    l1 = m.conv('conv_first', m.rt(x.reshape(b * t, c, h, w)))
    for i in range(5):
        l1 = m.resblock(f'feature_extraction.{i}', l1)
    l2 = m.conv('conv_l2_2', m.conv('conv_l2_1', l1, stride=2))
    l3 = m.conv('conv_l3_2', m.conv('conv_l3_1', l2, stride=2))
    l1, l2, l3 = l1.view(b, t, -1, h, w), l2.view(b, t, -1, h // 2, w // 2), l3.view(b, t, -1, h // 4, w // 4)
    pcd = m.sub('pcd_align.')
    ref = [l1[:, center], l2[:, center], l3[:, center]]
    aligned = torch.stack([pcd.pcd_alignment([l1[:, i], l2[:, i], l3[:, i]], ref, deformable_groups) for i in range(t)], dim=1)
    return m.sub('fusion.').tsa_fusion(aligned, center)


def keyframe_features(sd_edvr, x, keyframe_idx, temporal_padding=2, rounding=True, acc32=False):
    """{i: float64 [b, 64, h, w]} of the padded clip x (numpy [b, n, 3, h, w]) for an extractor state dict of numpy arrays."""
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd_edvr.items()}
    xt = torch.from_numpy(np.asarray(x, np.float64))
    with torch.no_grad():
        return {i: extractor(sd, xt[:, idx], rounding, acc32).numpy()
                for i, idx in V.mirrored_windows(x.shape[1], keyframe_idx, temporal_padding).items()}


# ------------------------------------------------------------------------------------------ bound and sizes, restated
def network_bound(y_model, y64):
    """The project's bf16 network bound: 2 max|y_model - y64| + 4 fp32 ulp of max|y64|."""
    ymax = float(np.abs(y64).max())
    return 2.0 * float(np.abs(y_model - y64).max()) + 4.0 * 2.0 ** (np.floor(np.log2(ymax)) - 23)


def _align(v, a):
    return (v + a - 1) // a * a


def trunk_convs(num_feat, num_block, cin_segs):
    """(cout, cin, first_seg, seg, cin_pad) of every conv of a bf16 trunk in launch order."""
    convs = [(num_feat, 3 + cin_segs * num_feat, 3, num_feat, 16 + cin_segs * num_feat)]
    return convs + [(num_feat, num_feat, num_feat, 0, num_feat)] * (2 * num_block)


def trunk_blob_bytes(num_feat, num_block, cin_segs, weight_elems, bias_floats, table_bytes):
    """sr_rvsr_trunk_packed_bytes_bf16 restated: per conv the bf16 image (``weight_elems(cout, cin, first_seg, seg, 0)`` elements of
    2 bytes) and the fp32 packed bias, each rounded up to 256 bytes; then the pack table of one row per conv."""
    convs = trunk_convs(num_feat, num_block, cin_segs)
    nbytes = sum(_align(2 * weight_elems(co, ci, fs, sg, 0), 256) + _align(4 * bias_floats(co), 256) for co, ci, fs, sg, _ in convs)
    return nbytes + table_bytes(len(convs))


def trunk_workspace_bytes(num_feat, n, h, w):
    return 3 * _align(2 * n * num_feat * h * w, 256)
