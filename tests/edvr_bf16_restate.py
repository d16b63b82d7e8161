"""A float64 model of EDVR's bf16 inference forward (EDVR in bf16): tests/edvr_restate.py and tests/dcn_restate.py with a
bf16 round trip wherever the HIP path stores or rounds a tensor, and nowhere else.

Rounded (``rt``): the converted frames; every conv, deformable-conv and 1x1 output after its epilogue (bias, activation and the
residuals the epilogue adds: one rounding); the masked samples of the deformable conv; the average pool, the correlation's
output, the gate, bilinear x2 and addition outputs; the packed weights.
Not rounded: offsets and mask logits (conv_offset stores fp32), the correlation's p, biases, conv_last's output, the bilinear x4
base of the fp32 centre frame.

``rounding=False`` switches every round trip off; the model then performs edvr_restate.edvr's operations in its order and
reproduces it exactly (tests/test_edvr_bf16_gpu.py checks that on the CPU).  ``acc32=True`` evaluates every convolution's sum
in float32: the CPU proxy of what the HIP path's fp32 accumulation adds to the roundings.
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_restate as R  # noqa: E402
import edvr_restate as E  # noqa: E402


class Model:
    def __init__(self, sd, rounding=True, acc32=False):
        self.rounding, self.acc32 = rounding, acc32
        self.sd = {k: (self.rt(v) if k.endswith('weight') else v) for k, v in sd.items()}

    def rt(self, t):
        return t.float().bfloat16().to(t.dtype) if self.rounding else t

    def sub(self, prefix):
        m = Model({}, self.rounding, self.acc32)
        m.sd = E._sub(self.sd, prefix)
        return m

    # ---- layers: F.conv2d -> activation -> residuals -> one rounding
    def conv(self, name, t, act='lrelu', stride=1, padding=1, res=(), store=True):
        w, b = self.sd[name + '.weight'], self.sd[name + '.bias']
        if self.acc32:
            y = F.conv2d(t.float(), w.float(), b.float(), stride=stride, padding=padding).to(t.dtype)
        else:
            y = F.conv2d(t, w, b, stride=stride, padding=padding)
        if act == 'lrelu':
            y = F.leaky_relu(y, 0.1)
        elif act == 'relu':
            y = F.relu(y)
        for r in res:
            y = r + y if r is res[0] else y + r
        return self.rt(y) if store else y

    def conv1(self, name, t, act='lrelu'):
        return self.conv(name, t, act, padding=0)

    def up(self, t):
        return self.rt(E._up(t))

    def resblock(self, name, t, extra=None):
        mid = self.conv(name + '.conv1', t, 'relu')
        return self.conv(name + '.conv2', mid, None, res=(t,) if extra is None else (t, extra))

    def pools(self, t):
        return torch.cat([F.max_pool2d(t, 3, 2, 1), self.rt(F.avg_pool2d(t, 3, 2, 1))], dim=1)

    def dcn_pack(self, prefix, x, feat, dg, lrelu):
        sd = self.sd
        out = self.conv(prefix + 'conv_offset', feat, None, store=False)          # fp32 NCHW: not rounded
        o1, o2, logit = torch.chunk(out, 3, dim=1)
        offset = torch.cat((o1, o2), dim=1)
        cols = self.rt(R.columns(x, offset, torch.sigmoid(logit), dg))            # the masked samples
        weight, bias = sd[prefix + 'weight'], sd.get(prefix + 'bias')
        cout, cin = weight.shape[:2]
        if self.acc32:
            y = torch.einsum('ock,nckhw->nohw', weight.reshape(cout, cin, 9).float(), cols.float()).to(x.dtype)
        else:
            y = torch.einsum('ock,nckhw->nohw', weight.reshape(cout, cin, 9), cols)
        if bias is not None:
            y = y + bias.view(1, -1, 1, 1)
        if lrelu:
            y = F.leaky_relu(y, 0.1)
        return self.rt(y), offset

    def pcd_alignment(self, nbr, ref, dg, offsets_out=None):
        upsampled_offset = upsampled_feat = None
        for i in range(3, 0, -1):
            level = f'l{i}'
            offset = self.conv(f'offset_conv1.{level}', torch.cat([nbr[i - 1], ref[i - 1]], dim=1))
            if i == 3:
                offset = self.conv(f'offset_conv2.{level}', offset)
            else:
                offset = self.conv(f'offset_conv2.{level}', torch.cat([offset, upsampled_offset], dim=1))
                offset = self.conv(f'offset_conv3.{level}', offset)
            feat, off = self.dcn_pack(f'dcn_pack.{level}.', nbr[i - 1], offset, dg, lrelu=(i == 3))
            if offsets_out is not None:
                offsets_out[level] = off
            if i < 3:
                feat = self.conv(f'feat_conv.{level}', torch.cat([feat, upsampled_feat], dim=1), 'lrelu' if i > 1 else None)
            if i > 1:
                upsampled_offset = self.up(offset) * 2
                upsampled_feat = self.up(feat)
        offset = self.conv('cas_offset_conv2', self.conv('cas_offset_conv1', torch.cat([feat, ref[0]], dim=1)))
        feat, off = self.dcn_pack('cas_dcnpack.', feat, offset, dg, lrelu=True)
        if offsets_out is not None:
            offsets_out['cas'] = off
        return feat

    def tsa_fusion(self, aligned, center):
        b, t, c, h, w = aligned.shape
        emb_ref = self.conv('temporal_attn1', aligned[:, center], None)
        emb = self.conv('temporal_attn2', aligned.reshape(b * t, c, h, w), None).view(b, t, -1, h, w)
        corr = (emb * emb_ref.unsqueeze(1)).sum(2)
        fused = self.rt((aligned * torch.sigmoid(corr).unsqueeze(2)).reshape(b, t * c, h, w))
        feat = self.conv1('feat_fusion', fused)
        attn = self.conv1('spatial_attn1', fused)
        attn = self.conv1('spatial_attn2', self.pools(attn))
        level = self.conv1('spatial_attn_l1', attn)
        level = self.conv('spatial_attn_l2', self.pools(level))
        level = self.up(self.conv('spatial_attn_l3', level))
        attn = self.conv('spatial_attn3', attn, res=(level,))
        attn = self.up(self.conv1('spatial_attn4', attn))
        attn = self.conv('spatial_attn5', attn, None)
        attn_add = self.conv1('spatial_attn_add2', self.conv1('spatial_attn_add1', attn), None)
        return self.rt(feat * torch.sigmoid(attn) * 2 + attn_add)

    def predeblur(self, x, hr_in):
        l1 = self.conv('conv_first', x)
        if hr_in:
            l1 = self.conv('stride_conv_hr1', l1, stride=2)
            l1 = self.conv('stride_conv_hr2', l1, stride=2)
        l2 = self.conv('stride_conv_l2', l1, stride=2)
        l3 = self.conv('stride_conv_l3', l2, stride=2)
        l3 = self.up(self.resblock('resblock_l3', l3))
        l2 = self.resblock('resblock_l2_1', l2, l3)
        l2 = self.up(self.resblock('resblock_l2_2', l2))
        l1 = self.resblock('resblock_l1.0', l1)
        l1 = self.resblock('resblock_l1.1', l1, l2)
        for i in range(2, 5):
            l1 = self.resblock(f'resblock_l1.{i}', l1)
        return l1

    def edvr(self, x, *, num_frame, deformable_groups=8, num_extract_block=5, num_reconstruct_block=10, center=None, hr_in=False,
             with_predeblur=False, with_tsa=True, offsets_out=None):
        b, t, c, h, w = x.shape
        center = num_frame // 2 if center is None else center
        x_center = x[:, center]                                                    # fp32: the base is not rounded
        flat = self.rt(x.reshape(b * t, c, h, w))
        if with_predeblur:
            l1 = self.conv1('conv_1x1', self.sub('predeblur.').predeblur(flat, hr_in), None)
            if hr_in:
                h, w = h // 4, w // 4
        else:
            l1 = self.conv('conv_first', flat)
        for i in range(num_extract_block):
            l1 = self.resblock(f'feature_extraction.{i}', l1)
        l2 = self.conv('conv_l2_2', self.conv('conv_l2_1', l1, stride=2))
        l3 = self.conv('conv_l3_2', self.conv('conv_l3_1', l2, stride=2))
        l1, l2, l3 = l1.view(b, t, -1, h, w), l2.view(b, t, -1, h // 2, w // 2), l3.view(b, t, -1, h // 4, w // 4)
        pcd = self.sub('pcd_align.')
        ref = [l1[:, center], l2[:, center], l3[:, center]]
        aligned = torch.stack([pcd.pcd_alignment([l1[:, i], l2[:, i], l3[:, i]], ref, deformable_groups,
                                                 offsets_out if i == 0 else None) for i in range(t)], dim=1)
        if with_tsa:
            feat = self.sub('fusion.').tsa_fusion(aligned, center)
        else:
            feat = self.conv1('fusion', aligned.reshape(b, -1, h, w), None)
        out = feat
        for i in range(num_reconstruct_block):
            out = self.resblock(f'reconstruction.{i}', out)
        out = self.rt(F.leaky_relu(F.pixel_shuffle(self.conv('upconv1', out, None, store=False), 2), 0.1))
        out = self.rt(F.leaky_relu(F.pixel_shuffle(self.conv('upconv2', out, None, store=False), 2), 0.1))
        out = self.conv('conv_last', self.conv('conv_hr', out), None, store=False)
        base = x_center if hr_in else F.interpolate(x_center, scale_factor=4, mode='bilinear', align_corners=False)
        return out + base


def edvr(sd, x, rounding=True, acc32=False, **kw):
    return Model(sd, rounding, acc32).edvr(x, **kw)
