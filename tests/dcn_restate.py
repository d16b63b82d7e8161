"""A restatement of the reference's modulated deformable convolution (DCNv2) and of PCDAlignment on plain torch ops,
differentiable by torch autograd, in the dtype of its inputs (float64 as the yardstick of the DCN tests; float32 on the CPU to
measure what single precision alone costs).  Written in this project's own words from the semantics of the reference's kernel
source, which it cites by file and line — not from its program text:

  basicsr/ops/dcn/src/deform_conv_cuda_kernel.cu
    :571-633  modulated_deformable_im2col_gpu_kernel   sampling position, the `inside` test (:618), value * mask (:627)
    :466-497  dmcn_im2col_bilinear                      corners floor / floor + 1, per-corner validity, the four weights
  basicsr/ops/dcn/deform_conv.py:121-186               ModulatedDeformConvFunction: y = W * columns + bias
  basicsr/archs/arch_util.py:204-227                   DCNv2Pack: conv_offset, chunk into (o1, o2, mask), sigmoid
  basicsr/archs/edvr_arch.py:56-98                     PCDAlignment.forward

Supported configuration only: 3x3, stride 1, padding 1, dilation 1, groups 1.  With dg deformable groups, cpg = cin / dg and
tap k = 3i + j, input channel ci belongs to group g = ci // cpg and samples at
  h_im = y - 1 + i + offset[n, 18g + 2k, y, x],   w_im = x - 1 + j + offset[n, 18g + 2k + 1, y, x]
with mask[n, 9g + k, y, x].  The gradients of the reference's backward kernels (:636-767) are the partial derivatives of this
expression wherever it is differentiable (floor is treated as locally constant), so autograd through it is their yardstick.
"""
import torch
import torch.nn.functional as F


def positions(offset, dg):
    """(h_im, w_im), each [n, dg, 9, H, W]: where tap k of group g samples for every output pixel."""
    n, _, H, W = offset.shape
    dt = offset.dtype
    tap_i = torch.arange(9).div(3, rounding_mode='floor').to(dt).view(1, 1, 9, 1, 1)
    tap_j = (torch.arange(9) % 3).to(dt).view(1, 1, 9, 1, 1)
    ys = torch.arange(H, dtype=dt).view(1, 1, 1, H, 1)
    xs = torch.arange(W, dtype=dt).view(1, 1, 1, 1, W)
    off = offset.reshape(n, dg, 9, 2, H, W)                     # channel 18g + 2k + (0: h, 1: w)
    return ys - 1 + tap_i + off[:, :, :, 0], xs - 1 + tap_j + off[:, :, :, 1]


def columns(x, offset, mask, dg, corner_weights='bilinear'):
    """[n, cin, 9, H, W]: mask * bilinear sample of x for every input channel and tap.  ``corner_weights='ones'`` replaces the
    four bilinear weights by 1 (with |x| and |mask| as inputs: the sample's slope bound, the sum of |v| over its valid corners)."""
    n, cin, H, W = x.shape
    cpg = cin // dg
    dt = x.dtype
    h_im, w_im = positions(offset, dg)
    inside = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
    h_low, w_low = torch.floor(h_im.detach()), torch.floor(w_im.detach())
    lh, lw = h_im - h_low, w_im - w_low
    flat = x.reshape(n, dg, cpg, H * W)
    val = torch.zeros((n, dg, cpg, 9, H, W), dtype=dt)
    for dh, dw, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
        hc, wc = (h_low + dh).long(), (w_low + dw).long()
        valid = inside & (hc >= 0) & (hc <= H - 1) & (wc >= 0) & (wc <= W - 1)
        idx = (hc.clamp(0, H - 1) * W + wc.clamp(0, W - 1)).view(n, dg, 1, 9 * H * W).expand(n, dg, cpg, 9 * H * W)
        v = torch.gather(flat, 3, idx).view(n, dg, cpg, 9, H, W)
        if corner_weights == 'ones':
            wt = torch.ones_like(wt)
        val = val + (wt * valid.to(dt)).unsqueeze(2) * v
    val = val * mask.reshape(n, dg, 1, 9, H, W)                 # channel 9g + k
    return val.reshape(n, cin, 9, H, W)


def modulated_deform_conv(x, offset, mask, weight, bias, dg):
    """y[n, co] = bias[co] + sum_{ci, k} W[co, ci, i, j] * mask * sample  (NCHW)."""
    cout, cin = weight.shape[:2]
    y = torch.einsum('ock,nckhw->nohw', weight.reshape(cout, cin, 9), columns(x, offset, mask, dg))
    return y if bias is None else y + bias.view(1, -1, 1, 1)


def dcn_pack(sd, prefix, x, feat, dg):
    """DCNv2Pack.forward(x, feat) (arch_util.py:215-227); returns (output, offset)."""
    out = F.conv2d(feat, sd[prefix + 'conv_offset.weight'], sd[prefix + 'conv_offset.bias'], padding=1)
    o1, o2, logit = torch.chunk(out, 3, dim=1)
    offset = torch.cat((o1, o2), dim=1)
    y = modulated_deform_conv(x, offset, torch.sigmoid(logit), sd[prefix + 'weight'], sd.get(prefix + 'bias'), dg)
    return y, offset


def pcd_alignment(sd, nbr_feat_l, ref_feat_l, dg, offsets_out=None):
    """PCDAlignment.forward (edvr_arch.py:56-98) on a state dict of tensors with the reference's keys.  ``offsets_out``: a dict
    that receives each level's DCN offsets ('l3', 'l2', 'l1', 'cas')."""
    def conv(name, t):
        return F.conv2d(t, sd[name + '.weight'], sd[name + '.bias'], padding=1)

    def lrelu(t):
        return F.leaky_relu(t, 0.1)

    def up(t):
        return F.interpolate(t, scale_factor=2, mode='bilinear', align_corners=False)

    upsampled_offset = upsampled_feat = None
    for i in range(3, 0, -1):
        level = f'l{i}'
        offset = lrelu(conv(f'offset_conv1.{level}', torch.cat([nbr_feat_l[i - 1], ref_feat_l[i - 1]], dim=1)))
        if i == 3:
            offset = lrelu(conv(f'offset_conv2.{level}', offset))
        else:
            offset = lrelu(conv(f'offset_conv2.{level}', torch.cat([offset, upsampled_offset], dim=1)))
            offset = lrelu(conv(f'offset_conv3.{level}', offset))
        feat, off = dcn_pack(sd, f'dcn_pack.{level}.', nbr_feat_l[i - 1], offset, dg)
        if offsets_out is not None:
            offsets_out[level] = off
        if i < 3:
            feat = conv(f'feat_conv.{level}', torch.cat([feat, upsampled_feat], dim=1))
        if i > 1:
            feat = lrelu(feat)
            upsampled_offset = up(offset) * 2
            upsampled_feat = up(feat)
    offset = lrelu(conv('cas_offset_conv2', lrelu(conv('cas_offset_conv1', torch.cat([feat, ref_feat_l[0]], dim=1)))))
    feat, off = dcn_pack(sd, 'cas_dcnpack.', feat, offset, dg)
    if offsets_out is not None:
        offsets_out['cas'] = off
    return lrelu(feat)
