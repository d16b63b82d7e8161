"""torch.autograd.Function wrappers of the single-op C ABI (discriminators, losses).

Activations travel between these Functions as plain fp32 tensors shaped [N, C/8, H, W, 8]
(the CB8 layout of include/sr_hip.h); every forward/backward below is libsr_hip.so launches
only, each made through hip_ops.launch.  The generator does not use this file: it is one fused Function
(archs/rrdbnet_autograd.py).

BNLReLUFn, MaxPool2x2Fn and LReLUFn also serve bf16 CB16 tensors [N, C/16, H, W, 16] (hip_autograd_bf16 exports them under
their ...Fn16 names): the body takes the entry point's suffix from the tensor's dtype and the block width from x.size(4).
"""
import torch

from . import _lib
from . import hip_ops as H


def _cb8(t):
    return H.CB8(t)


def _window(t):
    """The whole-tensor window of a channel-blocked activation, CB8 or CB16 by its block width."""
    return (H.CB16 if t.size(4) == 16 else H.CB8)(t)


def _sfx(t):
    """Entry-point suffix of an activation's dtype."""
    return '_bf16' if t.dtype == torch.bfloat16 else '_f32'


def _lrelu_bwd(gy, y, slope):
    """dz = gy * LeakyReLU'(slope) by the sign of the saved output ``y`` (contiguous, one dtype) — sr_lrelu_bwd_f32 / _bf16."""
    dz = torch.empty_like(gy)
    H.launch('sr_lrelu_bwd' + _sfx(gy), gy.device, gy.data_ptr(), y.data_ptr(), dz.data_ptr(), slope, gy.numel())
    return dz


class ToCB8(torch.autograd.Function):
    """NCHW -> CB8 (sr_nchw_to_cb8_f32); backward CB8 -> NCHW."""

    @staticmethod
    def forward(ctx, x):
        ctx.c = x.size(1)
        return H.nchw_to_cb8(x).buf

    @staticmethod
    def backward(ctx, g):
        return H.cb_to_nchw(_window(g.contiguous()), ctx.c)


class FromCB8(torch.autograd.Function):
    """CB8 -> NCHW with `channels` real channels; backward NCHW -> CB8 (pad channels zero)."""

    @staticmethod
    def forward(ctx, t, channels):
        ctx.cb = t.size(1)
        return H.cb8_to_nchw(_cb8(t), channels)

    @staticmethod
    def backward(ctx, g):
        out = H.CB8.empty(g.size(0), ctx.cb * 8, g.size(2), g.size(3), g.device)
        return H.nchw_to_cb8(g.contiguous(), out=out).buf, None


class ConvFn(torch.autograd.Function):
    """3x3/s1/p1 or 4x4/s2/p1 convolution (+bias, +LeakyReLU(act_slope)) on CB8.

    forward  : sr_conv3x3_f32 / sr_conv4x4s2_f32
    backward : LeakyReLU mask + data gradient fused in sr_conv3x3_f32 (mode-1 weights) / sr_conv4x4s2_dgrad_f32,
               weight gradient sr_conv3x3_wgrad_f32 / sr_conv4x4s2_wgrad_f32.
    """

    @staticmethod
    def forward(ctx, x, weight, bias, act_slope):
        k = weight.size(2)
        src = _cb8(x)
        if k == 3:
            out = H.conv3x3(src, H.cached_pack('f32 fwd', weight, bias, lambda: H.PackedConv(weight, bias)), act_slope=act_slope)
        elif k == 4:
            out = H.conv4x4s2(src, H.cached_pack('f32 fwd', weight, bias, lambda: H.PackedConv4x4s2(weight, bias)), act_slope=act_slope)
        else:
            raise NotImplementedError(f'kernel size {k}')
        ctx.save_for_backward(x, weight, out.buf if act_slope != 1.0 else None)
        ctx.act_slope, ctx.has_bias, ctx.k = act_slope, bias is not None, k
        ctx.param = weight if isinstance(weight, torch.nn.Parameter) else None   # key of the transposed image's cache entry
        return out.buf

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        k = ctx.k
        cout, cin = weight.shape[:2]
        gy = gy.contiguous()
        # dL/d(pre-activation): LeakyReLU backward against the saved output
        dz = _lrelu_bwd(gy, y, ctx.act_slope) if y is not None else gy
        dzc, src = _cb8(dz), _cb8(x)
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dx = dw = db = None
        if need_x:
            if k == 3:
                dx = H.conv3x3(dzc, H.cached_pack('f32 dgrad', ctx.param, None, lambda: H.PackedConv(weight, None, mode=1))).buf
            else:
                dx = H.conv4x4s2_dgrad(dzc, H.cached_pack('f32 dgrad', ctx.param, None, lambda: H.PackedConv4x4s2(weight, None, mode=1)),
                                       src.h, src.w).buf
            if dx.size(1) != x.size(1):  # dgrad writes roundup8(cin) channels == x's blocks
                dx = dx[:, :x.size(1)].contiguous()
        if need_w or (need_b and ctx.has_bias):
            if k == 3:
                dw, db = H.conv3x3_wgrad(src, dzc, cout, cin, want_bias=ctx.has_bias)
            else:
                dw, db = H.conv4x4s2_wgrad(src, dzc, cout, cin, want_bias=ctx.has_bias)
        return dx, dw, (db if ctx.has_bias else None), None


class DCNFn(torch.autograd.Function):
    """Modulated deformable 3x3/s1/p1 convolution (+bias, +LeakyReLU(act_slope)) on CB8 (include/sr_hip_dcn.h).

    forward(x, offset, mask_or_logits, weight, bias, act_slope, deformable_groups, mask_is_logit[, windows[, deterministic]]): ``offset`` /
    ``mask`` are CB8 tensors of 18 * dg / 9 * dg channels (pad channels ignored).  With ``windows`` = ((first block, blocks) of
    the offsets, (first block, blocks) of the mask) both arguments are the SAME tensor (DCNv2Pack: the conv_offset output, whose
    two thirds are block-aligned when dg % 4 == 0); its gradient is then one tensor the kernel writes both windows of, returned
    as the offset argument's gradient (the mask argument's is None, autograd adds the two).
    forward  : sr_dcn_fwd_f32
    backward : LeakyReLU mask against the saved output; columns (sr_dcn_cols_f32) -> sr_convd_wgrad_f32 ksize 1 ->
               sr_dcn_weight_unpack_f32 for dweight / dbias; dcol = Wt dz (sr_convd_f32 ksize 1 on sr_dcn_pack_t_f32's image);
               sr_dcn_bwd_data_f32 for doffset / dmask (bit-reproducible) and dx (atomicAdd: last bits depend on arrival order).
               With ``deterministic`` (behind ``windows``, which may be None) sr_dcn_bwd_data_det_f32 instead: the same doffset /
               dmask, and a dx summed in 64-bit integers (include/sr_hip_dcn_det.h), so that two backward passes agree bit for bit.
    """

    @staticmethod
    def forward(ctx, x, offset, mask, weight, bias, act_slope, deformable_groups, mask_is_logit, *extra):
        dg = deformable_groups
        windows = extra[0] if extra else None
        ctx.deterministic = bool(extra[1]) if len(extra) > 1 else False
        ctx.nextra = len(extra)
        src = _cb8(x)
        ctx.windows = windows   # ((off cb0, off cbn), (mask cb0, mask cbn)) when offset and mask are one tensor
        off_w, mask_w = DCNFn._windows(offset, mask, windows)
        out = H.dcn_fwd(src, off_w, mask_w, H.cached_pack('f32 fwd', weight, bias, lambda: H.PackedConvK(weight, bias)), dg,
                        mask_is_logit=mask_is_logit, act_slope=act_slope)
        ctx.save_for_backward(x, offset, mask if windows is None else None, weight, out.buf if act_slope != 1.0 else None)
        ctx.act_slope, ctx.has_bias, ctx.dg, ctx.logit = act_slope, bias is not None, dg, bool(mask_is_logit)
        ctx.param = weight if isinstance(weight, torch.nn.Parameter) else None
        return out.buf

    @staticmethod
    def _windows(offset, mask, windows):
        if windows is None:
            return _cb8(offset), _cb8(mask)
        (o0, on), (m0, mn) = windows
        return H.CB8(offset, o0, on), H.CB8(offset, m0, mn)

    @staticmethod
    def backward(ctx, gy):
        x, offset, mask, weight, y = ctx.saved_tensors
        cout, cin = weight.shape[:2]
        gy = gy.contiguous()
        dz = _lrelu_bwd(gy, y, ctx.act_slope) if y is not None else gy
        dzc, src = _cb8(dz), _cb8(x)
        off_w, mask_w = DCNFn._windows(offset, mask, ctx.windows)
        need_x, need_o, need_m, need_w, need_b = ctx.needs_input_grad[:5]
        need_b = need_b and ctx.has_bias
        if ctx.windows is not None:
            need_o = need_m = need_o or need_m
        dx = doff = dmsk = dw = db = None
        if need_w or need_b:
            cols = H.dcn_cols(src, off_w, mask_w, ctx.dg, mask_is_logit=ctx.logit)
            dw, db = H.dcn_wgrad(cols, dzc, cout, cin, want_bias=ctx.has_bias)
            del cols
        if need_x or need_o or need_m:
            dcol = H.convd(dzc, H.cached_pack('f32 dcn t', ctx.param, None, lambda: H.PackedDcnT(weight)))
            do_w = dm_w = None
            if need_o or need_m:
                if ctx.windows is not None:   # one gradient tensor, two windows; blocks outside both stay zero
                    doff = torch.zeros_like(offset)
                    (o0, on), (m0, mn) = ctx.windows
                    do_w, dm_w = H.CB8(doff, o0, on), H.CB8(doff, m0, mn)
                else:                          # pad channels are not written by the kernel
                    doff, dmsk = torch.zeros_like(offset), torch.zeros_like(mask)
                    do_w, dm_w = _cb8(doff), _cb8(dmsk)
            bwd_data = H.dcn_bwd_data_det if ctx.deterministic else H.dcn_bwd_data
            dxw = bwd_data(dcol, src, off_w, mask_w, ctx.dg, mask_is_logit=ctx.logit, want_dx=need_x, doffset=do_w, dmask=dm_w)
            dx = dxw.buf if dxw is not None else None
        return (dx, doff if need_o else None, dmsk if need_m else None, dw if need_w else None, db if need_b else None,
                None, None, None) + (None,) * ctx.nextra


class BNLReLUFn(torch.autograd.Function):
    """nn.BatchNorm2d + LeakyReLU on CB8 or CB16 (sr_bn_lrelu_fwd_f32 / sr_bn_lrelu_bwd_f32, or their _bf16 twins); parameters,
    statistics and running buffers fp32."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, train, momentum, eps, slope):
        x = x.contiguous()
        n, cb, h, w, blk = x.shape
        c = gamma.numel()
        dev = x.device
        y = torch.empty_like(x)
        mean = torch.empty(c, dtype=torch.float32, device=dev)
        invstd = torch.empty(c, dtype=torch.float32, device=dev)
        ws, wsb = H.reduce_ws(dev, c)
        ns = cb * h * w * blk
        H.launch('sr_bn_lrelu_fwd' + _sfx(x), dev, x.data_ptr(), ns, y.data_ptr(), ns, n, c, h, w, gamma.data_ptr(),
                 beta.data_ptr(), running_mean.data_ptr() if running_mean is not None else None,
                 running_var.data_ptr() if running_var is not None else None, int(train), momentum, eps, slope, mean.data_ptr(),
                 invstd.data_ptr(), ws.data_ptr(), wsb)
        ctx.save_for_backward(x, y, gamma, mean, invstd)
        ctx.train, ctx.slope = bool(train), slope
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, gamma, mean, invstd = ctx.saved_tensors
        n, cb, h, w, blk = x.shape
        c = gamma.numel()
        dev = x.device
        gy = gy.contiguous()
        dx = torch.empty_like(x)
        dgamma = torch.empty_like(gamma)
        dbeta = torch.empty_like(gamma)
        ws, wsb = H.reduce_ws(dev, c)
        ns = cb * h * w * blk
        H.launch('sr_bn_lrelu_bwd' + _sfx(x), dev, x.data_ptr(), ns, gy.data_ptr(), ns, y.data_ptr(), ns, dx.data_ptr(), ns, n, c,
                 h, w, gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(), int(ctx.train), ctx.slope, dgamma.data_ptr(),
                 dbeta.data_ptr(), ws.data_ptr(), wsb)
        return dx, dgamma, dbeta, None, None, None, None, None, None


class LinearFn(torch.autograd.Function):
    """nn.Linear + LeakyReLU(act_slope) (sr_linear_fwd_f32 / sr_linear_bwd_f32)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act_slope):
        x = x.contiguous()
        n, nin = x.shape
        nout = weight.size(0)
        y = torch.empty((n, nout), dtype=torch.float32, device=x.device)
        H.launch('sr_linear_fwd_f32', x.device, x.data_ptr(), weight.data_ptr(), bias.data_ptr() if bias is not None else None,
                 y.data_ptr(), n, nin, nout, act_slope)
        ctx.save_for_backward(x, weight, y)
        ctx.act_slope, ctx.has_bias = act_slope, bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        n, nin = x.shape
        nout = weight.size(0)
        gy = gy.contiguous()
        dev = x.device
        dz = torch.empty_like(gy)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(weight) if ctx.needs_input_grad[1] else None
        db = torch.empty(nout, dtype=torch.float32, device=dev) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        if db is not None and dw is None:
            dw = torch.empty_like(weight)
        H.launch('sr_linear_bwd_f32', dev, x.data_ptr(), weight.data_ptr(), y.data_ptr(), gy.data_ptr(), n, nin, nout,
                 ctx.act_slope, dz.data_ptr(), dx.data_ptr() if dx is not None else None,
                 dw.data_ptr() if dw is not None else None, db.data_ptr() if db is not None else None)
        return dx, (dw if ctx.needs_input_grad[1] else None), db, None


class L1LossFn(torch.autograd.Function):
    """loss_weight * mean|pred - target| (sr_l1_loss_fwd_f32 / sr_l1_loss_bwd_f32).  Inputs of any floating dtype are computed
    in fp32; the gradient comes back in pred's dtype (as torch's losses do)."""

    @staticmethod
    def forward(ctx, pred, target, weight):
        ctx.dtype = pred.dtype
        pred, target = pred.contiguous().float(), target.contiguous().float()
        dev = pred.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws, wsb = H.reduce_ws(dev)
        H.launch('sr_l1_loss_fwd_f32', dev, pred.data_ptr(), target.data_ptr(), pred.numel(), weight, loss.data_ptr(),
                 ws.data_ptr(), wsb)
        ctx.save_for_backward(pred, target)
        ctx.weight = weight
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        dev = pred.device
        g = g.contiguous().float()
        dp = torch.empty_like(pred)
        H.launch('sr_l1_loss_bwd_f32', dev, pred.data_ptr(), target.data_ptr(), pred.numel(), ctx.weight, g.data_ptr(),
                 dp.data_ptr())
        return dp.to(ctx.dtype), None, None


class GramFn(torch.autograd.Function):
    """[n, c, h, w] -> [n, c, c] = F F^T / (c h w), F = the feature map as [c, h w] (PerceptualLoss._gram_mat, losses.py:342-356):
    sr_gram_fwd_f32 / sr_gram_bwd_f32."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous().float()
        n, c, h, w = x.shape
        dev = x.device
        g = torch.empty((n, c, c), dtype=torch.float32, device=dev)
        H.launch('sr_gram_fwd_f32', dev, x.data_ptr(), n, c, h * w, 1.0 / (c * h * w), g.data_ptr())
        ctx.save_for_backward(x)
        return g

    @staticmethod
    def backward(ctx, dg):
        x, = ctx.saved_tensors
        n, c, h, w = x.shape
        dev = x.device
        dx = torch.empty_like(x)
        H.launch('sr_gram_bwd_f32', dev, x.data_ptr(), dg.contiguous().float().data_ptr(), n, c, h * w, 1.0 / (c * h * w),
                 dx.data_ptr())
        return dx


class PixelLossFn(torch.autograd.Function):
    """weight * mean(criterion(pred - target)), criterion kind 1 = squared error, 2 = Charbonnier(eps)
    (sr_pixel_loss_fwd_f32 / sr_pixel_loss_bwd_f32); fp32 arithmetic, the gradient in pred's dtype (as L1LossFn)."""

    @staticmethod
    def forward(ctx, pred, target, weight, kind, eps):
        ctx.dtype = pred.dtype
        pred, target = pred.contiguous().float(), target.contiguous().float()
        dev = pred.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws, wsb = H.reduce_ws(dev)
        H.launch('sr_pixel_loss_fwd_f32', dev, pred.data_ptr(), target.data_ptr(), pred.numel(), kind, eps, weight,
                 loss.data_ptr(), ws.data_ptr(), wsb)
        ctx.save_for_backward(pred, target)
        ctx.args = (weight, kind, eps)
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        weight, kind, eps = ctx.args
        dev = pred.device
        dp = torch.empty_like(pred)
        H.launch('sr_pixel_loss_bwd_f32', dev, pred.data_ptr(), target.data_ptr(), pred.numel(), kind, eps, weight,
                 g.contiguous().float().data_ptr(), dp.data_ptr())
        return dp.to(ctx.dtype), None, None, None, None


class GanPointLossFn(torch.autograd.Function):
    """weight * mean f(x) for the point-wise GAN criteria (sr_gan_point_loss_{fwd,bwd}_f32; kinds in include/sr_hip.h)."""

    @staticmethod
    def forward(ctx, x, kind, c, weight):
        ctx.dtype = x.dtype
        x = x.contiguous().float()
        dev = x.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws, wsb = H.reduce_ws(dev)
        H.launch('sr_gan_point_loss_fwd_f32', dev, x.data_ptr(), x.numel(), kind, c, weight, loss.data_ptr(), ws.data_ptr(), wsb)
        ctx.save_for_backward(x)
        ctx.args = (kind, c, weight)
        return loss

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        kind, c, weight = ctx.args
        dx = torch.empty_like(x)
        H.launch('sr_gan_point_loss_bwd_f32', x.device, x.data_ptr(), x.numel(), kind, c, weight,
                 g.contiguous().float().data_ptr(), dx.data_ptr())
        return dx.to(ctx.dtype), None, None, None


class BCELogitsFn(torch.autograd.Function):
    """weight * BCEWithLogits(x - mean(other), target) with `other` optional (plain GAN loss when None).

    The relativistic-average form of esrgan_model.py:40-41,67,71; gradients reach both x and other.  fp32 arithmetic; each
    gradient comes back in its input's dtype."""

    @staticmethod
    def forward(ctx, x, other, target_is_real, weight):
        ctx.dtypes = (x.dtype, other.dtype if other is not None else None)
        x = x.contiguous().float()
        dev = x.device
        ws, wsb = H.reduce_ws(dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        shift = dsum = None
        if other is not None:
            other = other.contiguous().float()
            shift = torch.empty((), dtype=torch.float32, device=dev)
            dsum = torch.empty((), dtype=torch.float32, device=dev)
            H.launch('sr_mean_f32', dev, other.data_ptr(), other.numel(), shift.data_ptr(), ws.data_ptr(), wsb)
        H.launch('sr_bce_logits_fwd_f32', dev, x.data_ptr(), shift.data_ptr() if shift is not None else None, x.numel(),
                 int(target_is_real), weight, loss.data_ptr(), dsum.data_ptr() if dsum is not None else None, ws.data_ptr(), wsb)
        ctx.save_for_backward(x, shift, dsum)
        ctx.target_is_real, ctx.weight = bool(target_is_real), weight
        ctx.other_shape = tuple(other.shape) if other is not None else None
        return loss

    @staticmethod
    def backward(ctx, g):
        x, shift, dsum = ctx.saved_tensors
        dev = x.device
        g = g.contiguous().float()
        dx = dother = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            H.launch('sr_bce_logits_bwd_f32', dev, x.data_ptr(), shift.data_ptr() if shift is not None else None, x.numel(),
                     int(ctx.target_is_real), ctx.weight, g.data_ptr(), dx.data_ptr())
        if ctx.other_shape is not None and ctx.needs_input_grad[1]:
            dother = torch.empty(ctx.other_shape, dtype=torch.float32, device=dev)
            H.launch('sr_fill_scaled_f32', dev, g.data_ptr(), dsum.data_ptr(), -1.0 / dother.numel(), dother.data_ptr(),
                     dother.numel())
        if dx is not None:
            dx = dx.to(ctx.dtypes[0])
        if dother is not None:
            dother = dother.to(ctx.dtypes[1])
        return dx, dother, None, None


def mean(x):
    """torch.mean(x.detach()) as one HIP reduction (logging of out_d_real / out_d_fake, esrgan_model.py:77-78); fp32 result for
    any floating input."""
    x = x.detach().contiguous().float()
    dev = x.device
    out = torch.empty((), dtype=torch.float32, device=dev)
    ws, wsb = H.reduce_ws(dev)
    H.launch('sr_mean_f32', dev, x.data_ptr(), x.numel(), out.data_ptr(), ws.data_ptr(), wsb)
    return out


class Bilinear2xFn(torch.autograd.Function):
    """F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) on CB8 (sr_bilinear2x_{fwd,bwd}_f32)."""

    @staticmethod
    def forward(ctx, x):
        n, cb, h, w, _ = x.shape
        y = torch.empty((n, cb, 2 * h, 2 * w, 8), dtype=torch.float32, device=x.device)
        H.launch('sr_bilinear2x_fwd_f32', x.device, x.data_ptr(), cb * h * w * 8, y.data_ptr(), cb * h * w * 32, n, cb, h, w)
        ctx.shape = (n, cb, h, w)
        return y

    @staticmethod
    def backward(ctx, g):
        n, cb, h, w = ctx.shape
        g = g.contiguous()
        gx = torch.empty((n, cb, h, w, 8), dtype=torch.float32, device=g.device)
        H.launch('sr_bilinear2x_bwd_f32', g.device, g.data_ptr(), cb * h * w * 32, gx.data_ptr(), cb * h * w * 8, n, cb, h, w)
        return gx


class AddFn(torch.autograd.Function):
    """a + b of two CB8 activations (sr_add_f32); both inputs receive the incoming gradient."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        out = torch.empty_like(a)
        H.launch('sr_add_f32', a.device, a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel())
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g


def _sn_bwd(g, w_sn, u, v, sigma_ptr, rows, cols):
    """Gradient of one spectrally normalised weight w.r.t. weight_orig, given this forward's u, v and sigma —
    sr_spectral_norm_bwd_f32."""
    dev = g.device
    g = g.contiguous()
    gw = torch.empty_like(g)
    wsb = max((rows + cols) * 4, _lib.load().sr_reduce_workspace_bytes(8) + 64)
    ws = H.scratch(dev, wsb)
    H.launch('sr_spectral_norm_bwd_f32', dev, g.data_ptr(), w_sn.data_ptr(), u.data_ptr(), v.data_ptr(), sigma_ptr, rows, cols,
             gw.data_ptr(), ws.data_ptr(), wsb)
    return gw


class SpectralNormFn(torch.autograd.Function):
    """weight = weight_orig / sigma with one power iteration on (u, v) in train mode
    (sr_spectral_norm_{fwd,bwd}_f32); u and v are buffers updated in place, as torch.nn.utils.spectral_norm does."""

    @staticmethod
    def forward(ctx, weight_orig, u, v, update, eps):
        lib = _lib.load()
        w = weight_orig.contiguous()
        rows = w.size(0)
        cols = w.numel() // rows
        dev = w.device
        w_sn = torch.empty_like(w)
        sigma = torch.empty((), dtype=torch.float32, device=dev)
        wsb = max((rows + 16 * cols) * 4, lib.sr_reduce_workspace_bytes(8) + 64)
        ws = H.scratch(dev, wsb)
        H.launch('sr_spectral_norm_fwd_f32', dev, w.data_ptr(), u.data_ptr(), v.data_ptr(), rows, cols, int(update), eps,
                 w_sn.data_ptr(), sigma.data_ptr(), ws.data_ptr(), wsb)
        ctx.save_for_backward(w_sn, u.clone(), v.clone(), sigma)
        ctx.dims = (rows, cols)
        return w_sn

    @staticmethod
    def backward(ctx, g):
        w_sn, u, v, sigma = ctx.saved_tensors
        return _sn_bwd(g, w_sn, u, v, sigma.data_ptr(), *ctx.dims), None, None, None, None


class SpectralNormBatchFn(torch.autograd.Function):
    """SpectralNormFn for all spectral-norm layers of a network in one call (sr_spectral_norm_fwd_batch_f32: one launch per stage
    of the power iteration for all layers): forward(update, eps, w0, u0, v0, w1, u1, v1, ...) -> (w_sn0, w_sn1, ...); per layer the
    same values as SpectralNormFn.  The backward stays per layer (one launch each)."""

    @staticmethod
    def forward(ctx, update, eps, *wuv):
        nl = len(wuv) // 3
        ws_, us, vs = [w.contiguous() for w in wuv[0::3]], wuv[1::3], wuv[2::3]
        dev = ws_[0].device
        outs = [torch.empty_like(w) for w in ws_]
        sigmas = torch.empty(nl, dtype=torch.float32, device=dev)
        table = (_lib.SnLayer * nl)()
        need = 0
        dims = []
        for i, (w, u, v) in enumerate(zip(ws_, us, vs)):
            rows = w.size(0)
            cols = w.numel() // rows
            dims.append((rows, cols))
            table[i].w_orig, table[i].u, table[i].v = w.data_ptr(), u.data_ptr(), v.data_ptr()
            table[i].rows, table[i].cols = rows, cols
            table[i].w_sn, table[i].sigma = outs[i].data_ptr(), sigmas.data_ptr() + 4 * i
            need += ((rows + 16 * cols) * 4 + 255) // 256 * 256
        ws = H.scratch(dev, need + 256)
        H.launch('sr_spectral_norm_fwd_batch_f32', dev, table, nl, int(update), eps, ws.data_ptr(), need + 256)
        if any(ctx.needs_input_grad[2::3]):   # u, v are updated in place by the next forward: the backward needs this forward's
            ctx.save_for_backward(sigmas, *outs, *[u.clone() for u in us], *[v.clone() for v in vs])
        ctx.dims = dims
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        saved = ctx.saved_tensors
        nl = len(ctx.dims)
        sigmas, outs, us, vs = saved[0], saved[1:1 + nl], saved[1 + nl:1 + 2 * nl], saved[1 + 2 * nl:1 + 3 * nl]
        grads = [None, None]
        for i, g in enumerate(gs):
            if g is None:
                grads += [None, None, None]
                continue
            gw = _sn_bwd(g, outs[i], us[i], vs[i], sigmas.data_ptr() + 4 * i, *ctx.dims[i])
            grads += [gw, None, None]
        return tuple(grads)


class MaxPool2x2Fn(torch.autograd.Function):
    """nn.MaxPool2d(kernel_size=2, stride=2) on CB8 or CB16 (sr_maxpool2x2_fwd_f32 / sr_maxpool2x2_bwd_f32, or their _bf16 twins)."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        n, cb, h, w, blk = x.shape
        y = torch.empty((n, cb, h // 2, w // 2, blk), dtype=x.dtype, device=x.device)
        H.launch('sr_maxpool2x2_fwd' + _sfx(x), x.device, x.data_ptr(), y.data_ptr(), n, cb, h, w)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        n, cb, h, w, _ = x.shape
        dx = torch.empty_like(x)
        gy = gy.contiguous()
        H.launch('sr_maxpool2x2_bwd' + _sfx(x), x.device, x.data_ptr(), gy.data_ptr(), dx.data_ptr(), n, cb, h, w)
        return dx


class ChannelAffineFn(torch.autograd.Function):
    """y[n][c] = x[n][c] * a[c] + b[c] on NCHW fp32 (constants a, b: the VGG input normalisation) — sr_channel_affine_f32."""

    @staticmethod
    def forward(ctx, x, a, b):
        x = x.contiguous().float()
        n, c, h, w = x.shape
        y = torch.empty_like(x)
        H.launch('sr_channel_affine_f32', x.device, x.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr(), n, c, h * w)
        ctx.save_for_backward(a)
        return y

    @staticmethod
    def backward(ctx, gy):
        a, = ctx.saved_tensors
        gy = gy.contiguous()
        n, c, h, w = gy.shape
        dx = torch.empty_like(gy)
        H.launch('sr_channel_affine_f32', gy.device, gy.data_ptr(), dx.data_ptr(), a.data_ptr(), None, n, c, h * w)
        return dx, None, None


class LReLUFn(torch.autograd.Function):
    """Stand-alone LeakyReLU(slope) / ReLU (slope 0) on any contiguous fp32 or bf16 tensor (sr_lrelu_fwd_f32 / sr_lrelu_bwd_f32, or
    their _bf16 twins)."""

    @staticmethod
    def forward(ctx, x, slope):
        x = x.contiguous()
        y = torch.empty_like(x)
        H.launch('sr_lrelu_fwd' + _sfx(x), x.device, x.data_ptr(), y.data_ptr(), slope, x.numel())
        ctx.save_for_backward(y)
        ctx.slope = slope
        return y

    @staticmethod
    def backward(ctx, gy):
        y, = ctx.saved_tensors
        return _lrelu_bwd(gy.contiguous(), y, ctx.slope), None


# ---- EDVR (include/sr_hip_edvr.h) ----

class ConvS2Fn(torch.autograd.Function):
    """3x3 / stride 2 / pad 1 convolution (+bias, +LeakyReLU(act_slope)) on CB8: (H + 1) // 2 x (W + 1) // 2.

    forward  : sr_conv3x3s2_f32
    backward : LeakyReLU mask against the saved output, sr_cb8_zero_insert2_f32, then the stride-1 operators on the zero-inserted
               gradient: sr_conv3x3_f32 (mode-1 weights) for dx, sr_conv3x3_wgrad_f32 for dweight / dbias.  Both are exact (the
               added products are zeros) and each costs one full-resolution conv.
    """

    @staticmethod
    def forward(ctx, x, weight, bias, act_slope):
        out = H.conv3x3s2(_cb8(x), H.cached_pack('f32 fwd', weight, bias, lambda: H.PackedConv(weight, bias)), act_slope=act_slope)
        ctx.save_for_backward(x, weight, out.buf if act_slope != 1.0 else None)
        ctx.act_slope, ctx.has_bias = act_slope, bias is not None
        ctx.param = weight if isinstance(weight, torch.nn.Parameter) else None
        return out.buf

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        cout, cin = weight.shape[:2]
        gy = gy.contiguous()
        dz = _lrelu_bwd(gy, y, ctx.act_slope) if y is not None else gy
        src = _cb8(x)
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and ctx.has_bias
        dx = dw = db = None
        if need_x or need_w or need_b:
            full = H.zero_insert2(_cb8(dz), src.h, src.w)
            if need_x:
                dx = H.conv3x3(full, H.cached_pack('f32 dgrad', ctx.param, None, lambda: H.PackedConv(weight, None, mode=1))).buf
                if dx.size(1) != x.size(1):
                    dx = dx[:, :x.size(1)].contiguous()
            if need_w or need_b:
                dw, db = H.conv3x3_wgrad(src, full, cout, cin, want_bias=ctx.has_bias)
        return dx, dw, (db if ctx.has_bias else None), None


class Conv1x1Fn(torch.autograd.Function):
    """1x1 convolution (+bias, +LeakyReLU(act_slope)) on CB8.

    forward  : sr_convd_f32 with ksize 1
    backward : LeakyReLU mask against the saved output; sr_convd_f32 with ksize 1 on the mode-1 image for dx;
               sr_convd_wgrad_f32 with ksize 1 for dweight / dbias.
    """

    @staticmethod
    def forward(ctx, x, weight, bias, act_slope):
        out = H.convd(_cb8(x), H.cached_pack('f32 fwd 1x1', weight, bias, lambda: H.PackedConvK(weight, bias)), act_slope=act_slope)
        ctx.save_for_backward(x, weight, out.buf if act_slope != 1.0 else None)
        ctx.act_slope, ctx.has_bias = act_slope, bias is not None
        ctx.param = weight if isinstance(weight, torch.nn.Parameter) else None
        return out.buf

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        cout, cin = weight.shape[:2]
        gy = gy.contiguous()
        dz = _lrelu_bwd(gy, y, ctx.act_slope) if y is not None else gy
        dzc, src = _cb8(dz), _cb8(x)
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and ctx.has_bias
        dx = dw = db = None
        if need_x:
            dx = H.convd(dzc, H.cached_pack('f32 dgrad 1x1', ctx.param, None, lambda: H.PackedConvK(weight, None, mode=1))).buf
            if dx.size(1) != x.size(1):
                dx = dx[:, :x.size(1)].contiguous()
        if need_w or need_b:
            dw, db = H.convd_wgrad(src, dzc, cout, cin, ksize=1, want_bias=ctx.has_bias)
        return dx, dw, (db if ctx.has_bias else None), None


class Pool3x3s2Fn(torch.autograd.Function):
    """torch.cat([MaxPool2d(3, 2, 1)(x), AvgPool2d(3, 2, 1)(x)], 1) on CB8 (sr_pool3x3s2_fwd_f32 / sr_pool3x3s2_bwd_f32)."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return H.pool3x3s2(_cb8(x)).buf

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return H.pool3x3s2_bwd(_cb8(x), _cb8(g.contiguous())).buf


class TSACorrFn(torch.autograd.Function):
    """TSA's temporal attention on CB8: forward(emb [b*t], emb_ref [b], aligned [b*t], t) -> aligned * sigmoid(sum_c emb *
    emb_ref) as [b, t * C/8, h, w, 8], the channel concatenation over the frames (the same memory as [b*t, C/8, h, w, 8]) —
    sr_tsa_corr_fwd_f32 / sr_tsa_corr_bwd_f32."""

    @staticmethod
    def forward(ctx, emb, emb_ref, aligned, t):
        emb, emb_ref, aligned = emb.contiguous(), emb_ref.contiguous(), aligned.contiguous()
        prob, out = H.tsa_corr(_cb8(emb), _cb8(emb_ref), _cb8(aligned), t)
        ctx.save_for_backward(emb, emb_ref, aligned, prob)
        bt, cb, h, w, _ = out.buf.shape
        return out.buf.view(bt // t, t * cb, h, w, 8)

    @staticmethod
    def backward(ctx, g):
        emb, emb_ref, aligned, prob = ctx.saved_tensors
        g = g.contiguous().view(emb.shape)
        dal, demb, dref = H.tsa_corr_bwd(_cb8(g), _cb8(emb), _cb8(emb_ref), _cb8(aligned), prob)
        return demb.buf, dref.buf, dal.buf, None


class TSAGateFn(torch.autograd.Function):
    """feat * sigmoid(attn) * 2 + attn_add on CB8 (sr_tsa_gate_fwd_f32 / sr_tsa_gate_bwd_f32)."""

    @staticmethod
    def forward(ctx, feat, attn, attn_add):
        feat, attn, attn_add = feat.contiguous(), attn.contiguous(), attn_add.contiguous()
        ctx.save_for_backward(feat, attn)
        return H.tsa_gate(_cb8(feat), _cb8(attn), _cb8(attn_add)).buf

    @staticmethod
    def backward(ctx, g):
        feat, attn = ctx.saved_tensors
        g = g.contiguous()
        df, da = H.tsa_gate_bwd(_cb8(g), _cb8(feat), _cb8(attn))
        return df.buf, da.buf, g


class PixelShuffleFn(torch.autograd.Function):
    """nn.PixelShuffle(r) on CB8, ``channels`` real output channels (sr_cb8_pixel_shuffle_f32 / sr_cb8_pixel_unshuffle_f32)."""

    @staticmethod
    def forward(ctx, x, channels, r):
        ctx.args = (channels, r)
        return H.pixel_shuffle(_cb8(x.contiguous()), channels, r).buf

    @staticmethod
    def backward(ctx, g):
        channels, r = ctx.args
        return H.pixel_unshuffle(_cb8(g.contiguous()), channels, r).buf, None, None


class BilinearUpFn(torch.autograd.Function):
    """F.interpolate(x, scale_factor=s, mode='bilinear', align_corners=False) on NCHW fp32, added into ``acc`` [N, C, s*H, s*W]
    in place when given (sr_bilinear_up_f32 / sr_bilinear_up_bwd_f32); both inputs receive gradients."""

    @staticmethod
    def forward(ctx, x, s, acc=None):
        ctx.s, ctx.has_acc = s, acc is not None
        if acc is None:
            return H.bilinear_up(x, s)
        ctx.mark_dirty(acc)
        H.bilinear_up(x, s, out=acc)
        return acc

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        return (H.bilinear_up_bwd(g, ctx.s) if ctx.needs_input_grad[0] else None), None, (g if ctx.has_acc else None)
