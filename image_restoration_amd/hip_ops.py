"""Thin torch-tensor wrappers over the C ABI (include/sr_hip.h and its per-network companions).

Tensors only provide device memory and the current HIP stream; every op below is one libsr_hip.so call, made through
``launch`` (device guard, the device's current stream as the last argument, the status check that names the symbol).
Activations between ops are channel-blocked: fp32 ``[N][C/8][H][W][8]`` (class ``CB8``) or bf16 ``[N][C/16][H][W][16]``
(class ``CB16``); channel slices are views (pointer + parent stride).  What the conv wrappers share is written once:
``_PackedWeights`` (the four weight-image classes), ``_conv_desc`` (struct sr_conv3x3_desc for both dtypes) and
``_wgrad_targets`` / ``_wgrad_desc`` (struct sr_conv3x3_wgrad_desc).  A wrapper is its assertions, its allocations and one
``launch`` line.
"""
import ctypes as C
import weakref

import torch

from . import _lib


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def launch(name, dev, *args):
    """The one way a stream-ordered entry point is called: ``lib.<name>(*args, stream)`` under ``dev``'s device guard, with
    ``dev``'s current stream looked up inside the guard, and a non-zero status raised as SrHipError naming ``name``.  ``args``
    are what ctypes takes: device pointers as ints (``t.data_ptr()``, a CB window's ``.ptr``), None for NULL, scalars, byref."""
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(getattr(lib, name)(*args, _stream(dev)), name)


_scratch = {}

# ---- weight images of long-lived parameters are packed once per change, not once per call ----
# The discriminators and the perceptual extractor run their convs one autograd function at a time; every call packed its weight
# (and, in the backward, the transposed image) again: the ESRGAN step runs the discriminator five times on the same weights.
# A cached image is valid while the parameter object, its storage address, its torch version counter and its write epoch are the
# same.  The epoch covers writers torch cannot see: the fused Adam / EMA kernels write through raw pointers (optim.FlatAdam tags
# its parameters with its epoch cell and bumps it per step); invalidate_packs() is the global form.  Only nn.Parameter weights
# are cached: temporaries (a spectrally normalised weight is a new tensor every forward) would pin memory and can alias addresses.
# (An in-place write through ``param.data`` is invisible to all of these: call invalidate_packs() after one.)
_pack_epoch = [0]
_pack_cache = {}


def invalidate_packs():
    _pack_epoch[0] += 1


def cached_pack(kind, weight, bias, build):
    if not isinstance(weight, torch.nn.Parameter):
        return build()
    sig = (weight.data_ptr(), weight._version, getattr(weight, '_sr_epoch', _pack_epoch)[0], _pack_epoch[0],
           None if bias is None else (bias.data_ptr(), bias._version))
    wid = id(weight)
    slot = _pack_cache.get(wid)
    if slot is None or slot[0]() is not weight:
        # the entry (and the device memory of its images) goes when the parameter does
        slot = (weakref.ref(weight, lambda _, wid=wid: _pack_cache.pop(wid, None)), {})
        _pack_cache[wid] = slot
    hit = slot[1].get(kind)
    if hit is not None and hit[0] == sig:
        return hit[1]
    val = build()
    slot[1][kind] = (sig, val)
    return val


def scratch(dev, nbytes, tag='ws'):
    """Grow-only per-device scratch buffer (reduction workspaces, wgrad slabs).  Launches that share it are
    ordered on the current stream."""
    key = (str(dev), tag)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        _scratch[key] = buf
    return buf


def reduce_ws(dev, c=8):
    """(workspace, its size in bytes) of the two-stage reductions over ``c`` channels (sr_reduce_workspace_bytes)."""
    nbytes = _lib.load().sr_reduce_workspace_bytes(c)
    return scratch(dev, nbytes), nbytes


def _need_cuda(t, what):
    if not t.is_cuda:
        raise _lib.SrHipError(f'{what}: tensor is on {t.device}; the HIP path has no CPU fallback')


class _CBWindow:
    """A channel-blocked activation: storage ``buf`` [N, CB, H, W, block] plus a channel-block window [cb0, cb0 + cbn)."""
    block = dtype = esize = None   # channels per block, element type, bytes per element

    def __init__(self, buf, cb0=0, cbn=None):
        assert buf.dim() == 5 and buf.size(4) == self.block and buf.dtype == self.dtype and buf.is_contiguous()
        self.buf, self.cb0 = buf, cb0
        self.cbn = buf.size(1) - cb0 if cbn is None else cbn
        assert 0 <= cb0 and cb0 + self.cbn <= buf.size(1)

    @classmethod
    def empty(cls, n, channels, h, w, device):
        return cls(torch.empty((n, (channels + cls.block - 1) // cls.block, h, w, cls.block), dtype=cls.dtype, device=device))

    @classmethod
    def zeros(cls, n, channels, h, w, device):
        return cls(torch.zeros((n, (channels + cls.block - 1) // cls.block, h, w, cls.block), dtype=cls.dtype, device=device))

    n = property(lambda s: s.buf.size(0))
    h = property(lambda s: s.buf.size(2))
    w = property(lambda s: s.buf.size(3))
    channels = property(lambda s: s.cbn * s.block)
    img_stride = property(lambda s: s.buf.size(1) * s.buf.size(2) * s.buf.size(3) * s.block)
    device = property(lambda s: s.buf.device)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.cb0 * self.h * self.w * self.block * self.esize

    def slice(self, c0, c):
        assert c0 % self.block == 0 and c % self.block == 0
        return type(self)(self.buf, self.cb0 + c0 // self.block, c // self.block)


class CB8(_CBWindow):
    """A channel-blocked fp32 activation: storage ``buf`` [N, CB, H, W, 8] plus a channel-block window."""
    block, dtype, esize = 8, torch.float32, 4


class CB16(_CBWindow):
    """A channel-blocked bf16 activation: storage ``buf`` [N, CB, H, W, 16] plus a channel-block window."""
    block, dtype, esize = 16, torch.bfloat16, 2


def nchw_to_cb8(x, unshuffle=1, out=None):
    _need_cuda(x, 'nchw_to_cb8')
    x = x.contiguous().float()
    n, c, hh, ww = x.shape
    h, w = hh // unshuffle, ww // unshuffle
    cu = c * unshuffle * unshuffle
    if out is None:
        out = CB8.empty(n, cu, h, w, x.device)
    launch('sr_nchw_to_cb8_f32', x.device, x.data_ptr(), out.ptr, n, c, h, w, unshuffle, out.cbn, out.img_stride)
    return out


def cb_to_nchw(t, channels):
    """CB8 or CB16 window -> NCHW fp32 with ``channels`` real channels — sr_cb8_to_nchw_f32 / sr_cb16_to_nchw_f32."""
    y = torch.empty((t.n, channels, t.h, t.w), dtype=torch.float32, device=t.device)
    launch(f'sr_cb{t.block}_to_nchw_f32', t.device, t.ptr, t.img_stride, y.data_ptr(), t.n, channels, t.h, t.w, 1)
    return y


cb8_to_nchw = cb16_to_nchw = cb_to_nchw


class _PackedWeights:
    """What the weight-image classes share: the device check, the fp32 copy of the weight, cout / src_channels by ``mode``
    (0 = forward, 1 = data gradient: the image consumes dY and produces the padded source channels), the weight image, the bias
    image (mode 0 with a bias only) and the one pack call.  A subclass states its kernel-size assertion and padding rule
    (``_cin_pad``) and its size query and pack entry point (``_image``); every pack entry point takes (weight, bias,
    *geometry, weight image, bias image, stream)."""
    block, wdtype = 8, torch.float32   # channel block of the activations, element type of the weight image

    def __init__(self, weight, bias, mode, first_seg=None, seg=0):
        _need_cuda(weight, type(self).__name__)
        lib = _lib.load()
        weight = weight.detach().contiguous().float()
        cout, cin = weight.shape[:2]
        first_seg = cin if first_seg is None else first_seg
        cin_pad = self._cin_pad(lib, weight, first_seg, seg)
        self.mode = mode
        if mode == 0:
            self.cout, self.src_channels = cout, cin_pad
        else:
            self.cout, self.src_channels = cin_pad, (cout + self.block - 1) // self.block * self.block
        nw, name, geometry = self._image(lib, cout, cin, first_seg, seg, mode)
        dev = weight.device
        self.w = torch.empty(nw, dtype=self.wdtype, device=dev)
        self.b = None
        if mode == 0 and bias is not None:
            bias = bias.detach().contiguous().float()
            self.b = torch.empty(lib.sr_conv3x3_packed_bias_floats(cout), dtype=torch.float32, device=dev)
        launch(name, dev, weight.data_ptr(), bias.data_ptr() if self.b is not None else None, *geometry, self.w.data_ptr(),
               self.b.data_ptr() if self.b is not None else None)


class PackedConv(_PackedWeights):
    """MFMA operand image of one 3x3 conv (sr_conv3x3_pack_f32)."""

    def __init__(self, weight, bias=None, first_seg=None, seg=0, mode=0):
        super().__init__(weight, bias, mode, first_seg, seg)

    def _cin_pad(self, lib, weight, first_seg, seg):
        cin = weight.shape[1]
        assert weight.shape[2:] == (3, 3)
        self.cin_pad = lib.sr_conv3x3_cin_pad(cin, first_seg, seg)
        if self.cin_pad <= 0:
            raise ValueError(f'cin={cin} is not first_seg={first_seg} + k*seg={seg}')
        return self.cin_pad

    def _image(self, lib, cout, cin, first_seg, seg, mode):
        return (lib.sr_conv3x3_packed_weight_floats(self.cout, self.src_channels), 'sr_conv3x3_pack_f32',
                (cout, cin, first_seg, seg, mode))


def _conv_operands(d, src, pc, bias=True):
    """The source and weight fields of a struct sr_conv3x3_desc."""
    d.in_, d.in_img_stride, d.cin_pad, d.in_h, d.in_w = src.ptr, src.img_stride, pc.src_channels, src.h, src.w
    d.wpacked, d.cout = pc.w.data_ptr(), pc.cout
    if bias and pc.b is not None:
        d.bpacked = pc.b.data_ptr()


def _conv_desc(src, pc, out, upsample, act_slope, alpha, res1, beta1, res2, beta2, out_nchw, mask, mask_cb0, mask_slope,
               out_unshuffle2=False):
    """What sr_conv3x3_f32 and sr_conv3x3_bf16 (and the descriptors that embed theirs) share of a struct sr_conv3x3_desc:
    operands, destination, epilogue scalars, residuals and mask; the windows are ``type(src)`` (CB8 or CB16).  Returns
    (descriptor, what the conv returns)."""
    assert src.channels == pc.src_channels, (src.channels, pc.src_channels)
    CB = type(src)
    H, W = (2 * src.h, 2 * src.w) if upsample else (src.h, src.w)
    d = _lib.ConvDesc()
    _conv_operands(d, src, pc)
    d.upsample = int(upsample)
    if out_nchw is not None:
        assert out_nchw.is_contiguous() and out_nchw.shape == (src.n, pc.cout, H, W)
        d.out, d.out_img_stride, d.out_nchw = out_nchw.data_ptr(), pc.cout * H * W, 1
        ret = out_nchw
    elif out_unshuffle2:   # (bf16 only)
        # the destination only exists pixel-unshuffled: [n][4 cout / 16][H / 2][W / 2][16] (sr_conv3x3_desc.out_unshuffle2)
        assert out is None and pc.cout % 16 == 0 and H % 2 == 0 and W % 2 == 0
        ret = CB.empty(src.n, 4 * pc.cout, H // 2, W // 2, src.device)
        d.out, d.out_img_stride, d.out_nchw, d.out_unshuffle2 = ret.ptr, ret.img_stride, 0, 1
    else:
        if out is None:
            out = CB.empty(src.n, pc.cout, H, W, src.device)  # every valid block is written (pad couts: zero weights)
        assert (out.n, out.h, out.w) == (src.n, H, W) and out.channels >= (pc.cout + CB.block - 1) // CB.block * CB.block
        d.out, d.out_img_stride, d.out_nchw = out.ptr, out.img_stride, 0
        ret = out
    d.n, d.act_slope, d.alpha = src.n, act_slope, alpha
    if res1 is not None:
        d.res1, d.res1_img_stride, d.beta1 = res1.ptr, res1.img_stride, beta1
    if res2 is not None:
        d.res2, d.res2_img_stride, d.beta2 = res2.ptr, res2.img_stride, beta2
    if mask is not None:
        _conv_mask(d, mask, mask_cb0, mask_slope)
    return d, ret


def _conv_mask(d, mask, mask_cb0, mask_slope):
    d.mask_src, d.mask_img_stride, d.mask_cb0, d.mask_cbn, d.mask_slope = mask.ptr, mask.img_stride, mask_cb0, mask.cbn, mask_slope


def _conv_desc_f32(src, pc, out=None, *, upsample=False, act_slope=1.0, alpha=1.0, res1=None, beta1=0.0, res2=None,
                   beta2=0.0, accumulate=False, mask=None, mask_cb0=0, mask_slope=0.2, out_nchw=None):
    d, ret = _conv_desc(src, pc, out, upsample, act_slope, alpha, res1, beta1, res2, beta2, out_nchw, mask, mask_cb0, mask_slope)
    d.accumulate = int(accumulate)
    return d, ret


def conv3x3(src, pc, out=None, **kw):
    """out = alpha*lrelu(conv(src)+bias) + beta1*res1 + beta2*res2  (one sr_conv3x3_f32 launch).

    src: CB8 window of pc.src_channels channels.  out: CB8 window (allocated if None) or, with
    ``out_nchw`` = an NCHW tensor [N, cout<=4, H, W], a plain tensor.  Keywords: upsample, act_slope, alpha, res1/beta1,
    res2/beta2, accumulate, mask/mask_cb0/mask_slope, out_nchw."""
    d, ret = _conv_desc_f32(src, pc, out, **kw)
    launch('sr_conv3x3_f32', src.device, C.byref(d))
    return ret


def _conv_chain(name, conv_desc, steps, sync, call_index):
    src0 = steps[0][0]
    if sync is None:
        sync = torch.zeros(_lib.load().sr_conv3x3_chain_sync_ints(src0.n, src0.h, src0.w), dtype=torch.int32, device=src0.device)
    descs = (_lib.ConvDesc * len(steps))()
    outs = []
    for i, (src, pc, out, kw) in enumerate(steps):
        descs[i], ret = conv_desc(src, pc, out, **kw)
        outs.append(ret)
    launch(name, src0.device, descs, len(steps), sync.data_ptr(), call_index)
    return outs, sync


def conv3x3_chain(steps, sync=None, call_index=0):
    """fp32 twin of conv3x3_chain_bf16 — sr_conv3x3_chain_f32.  ``steps`` = [(src CB8, PackedConv, out CB8, kwargs of conv3x3)]."""
    return _conv_chain('sr_conv3x3_chain_f32', _conv_desc_f32, steps, sync, call_index)


def _wgrad_targets(out, shape, want_bias, dev, zeros=False):
    """Where a weight gradient goes: (dw, db, (dweight pointer, dbias pointer, accumulate)).  ``out`` = the caller's
    (dweight, dbias or None) device pointers the gradients are ADDED into (dw = db = None), else fresh fp32 tensors."""
    if out is not None:
        return None, None, (out[0], out[1], 1)
    dw = (torch.zeros if zeros else torch.empty)(shape, dtype=torch.float32, device=dev)
    db = torch.empty((shape[0],), dtype=torch.float32, device=dev) if want_bias else None
    return dw, db, (dw.data_ptr(), db.data_ptr() if db is not None else None, 0)


def _wgrad_desc(d, src, dy, cin_pad, upsample, cout, cin, first_seg, seg, scale, target, nbytes, tag='slab'):
    """Fills a struct sr_conv3x3_wgrad_desc; the slab of ``nbytes`` is the per-device scratch buffer ``tag``."""
    slab = scratch(src.device, nbytes, tag)
    d.x, d.x_img_stride, d.cin_pad, d.in_h, d.in_w, d.upsample = src.ptr, src.img_stride, cin_pad, src.h, src.w, int(upsample)
    d.dy, d.dy_img_stride = dy.ptr, dy.img_stride
    d.cout, d.cin, d.first_seg, d.seg, d.n, d.scale = cout, cin, first_seg, seg, src.n, scale
    d.dweight, d.dbias, d.accumulate = target
    d.slab, d.slab_bytes = slab.data_ptr(), nbytes
    return d


def conv3x3_wgrad(src, dy, cout, cin, first_seg=None, seg=0, *, upsample=False, scale=1.0, want_bias=True, out=None):
    """(dweight [cout,cin,3,3], dbias [cout]) of a 3x3 conv whose source was ``src`` (CB8) and whose
    pre-activation output gradient is ``dy`` (CB8) — one sr_conv3x3_wgrad_f32 call.  ``out`` = (dweight, dbias or None):
    device pointers (ints) the gradients are ADDED into (accumulate = 1, e.g. a FlatAdam gradient arena) instead."""
    lib = _lib.load()
    first_seg = cin if first_seg is None else first_seg
    cin_pad = lib.sr_conv3x3_cin_pad(cin, first_seg, seg)
    assert src.channels == cin_pad, (src.channels, cin_pad)
    H, W = (2 * src.h, 2 * src.w) if upsample else (src.h, src.w)
    assert (dy.n, dy.h, dy.w) == (src.n, H, W) and dy.channels >= (cout + 7) // 8 * 8
    dw, db, target = _wgrad_targets(out, (cout, cin, 3, 3), want_bias, src.device)
    d = _wgrad_desc(_lib.WgradDesc(), src, dy, cin_pad, upsample, cout, cin, first_seg, seg, scale, target,
                    lib.sr_conv3x3_wgrad_slab_bytes(src.n, H, W))
    launch('sr_conv3x3_wgrad_f32', src.device, C.byref(d))
    return None if out is not None else (dw, db)


def upsample2x_bwd(g, mask=None, mask_slope=0.2):
    """2x2-sum backward of the nearest upsample (+ optional LeakyReLU backward) — sr_upsample2x_bwd_f32."""
    assert g.h % 2 == 0 and g.w % 2 == 0
    out = CB8.empty(g.n, g.channels, g.h // 2, g.w // 2, g.device)
    launch('sr_upsample2x_bwd_f32', g.device, g.ptr, g.img_stride, out.ptr, out.img_stride,
           mask.ptr if mask is not None else None, mask.img_stride if mask is not None else 0, mask_slope, g.n, g.cbn, out.h,
           out.w)
    return out


def cb8_axpby(dst, src, a=1.0, b=1.0):
    """dst = a*dst + b*src on CB8 windows — sr_cb8_axpby_f32."""
    assert (dst.n, dst.cbn, dst.h, dst.w) == (src.n, src.cbn, src.h, src.w)
    launch('sr_cb8_axpby_f32', dst.device, dst.ptr, dst.img_stride, src.ptr, src.img_stride, a, b, dst.n, dst.cbn, dst.h, dst.w)
    return dst


def pixel_shuffle(src, channels, r):
    """nn.PixelShuffle(r) on CB8 (r in {2, 3}): ``src`` holds r*r*channels real channels -> CB8 of ``channels`` at r x the
    size — sr_cb8_pixel_shuffle_f32."""
    assert src.channels >= channels * r * r
    out = CB8.empty(src.n, channels, src.h * r, src.w * r, src.device)
    launch('sr_cb8_pixel_shuffle_f32', src.device, src.ptr, src.img_stride, out.ptr, out.img_stride, src.n, channels, src.h,
           src.w, r)
    return out


def pixel_unshuffle(src, channels, r):
    """nn.PixelUnshuffle(r) on CB8, the shuffle's backward: ``channels`` real channels of ``src`` -> CB8 of r*r*channels at
    1/r of the size — sr_cb8_pixel_unshuffle_f32."""
    assert src.channels >= channels and src.h % r == 0 and src.w % r == 0
    out = CB8.empty(src.n, channels * r * r, src.h // r, src.w // r, src.device)
    launch('sr_cb8_pixel_unshuffle_f32', src.device, src.ptr, src.img_stride, out.ptr, out.img_stride, src.n, channels, out.h,
           out.w, r)
    return out


def bilinear_up(x, s, out=None):
    """F.interpolate(x, scale_factor=s, mode='bilinear', align_corners=False) on NCHW fp32, s in {2, 3, 4} —
    sr_bilinear_up_f32.  ``out``: an NCHW tensor [N, C, s*H, s*W] the result is ADDED into (returned)."""
    _need_cuda(x, 'bilinear_up')
    x = x.contiguous().float()
    n, c, h, w = x.shape
    acc = out is not None
    if out is None:
        out = torch.empty((n, c, h * s, w * s), dtype=torch.float32, device=x.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (n, c, h * s, w * s)
    launch('sr_bilinear_up_f32', x.device, x.data_ptr(), out.data_ptr(), n, c, h, w, s, int(acc))
    return out


def bilinear_up_bwd(g, s, out=None):
    """Adjoint of bilinear_up (gather form, bit-reproducible): g [N, C, s*H, s*W] -> [N, C, H, W] — sr_bilinear_up_bwd_f32.
    ``out``: an NCHW tensor the result is ADDED into (returned)."""
    _need_cuda(g, 'bilinear_up_bwd')
    g = g.contiguous().float()
    n, c, hh, ww = g.shape
    assert hh % s == 0 and ww % s == 0
    h, w = hh // s, ww // s
    acc = out is not None
    if out is None:
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=g.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (n, c, h, w)
    launch('sr_bilinear_up_bwd_f32', g.device, g.data_ptr(), out.data_ptr(), n, c, h, w, s, int(acc))
    return out


def _ca_workspace(lib, dev, n, nf, hid, h, w):
    nbytes = lib.sr_ca_workspace_bytes(n, nf, hid, h, w)
    return scratch(dev, nbytes, 'ca'), nbytes


def ca_squeeze(u, w1, b1, w2, b2):
    """RCAN channel attention, the squeeze: p = mean_hw u, h = relu(W1 p + b1), s = sigmoid(W2 h + b2) for the CB8 tensor ``u``
    (all its channels).  W1 [hid, nf, 1, 1], W2 [nf, hid, 1, 1] as stored.  Returns (p [N, nf], h [N, hid], s [N, nf]) —
    sr_ca_squeeze_f32."""
    lib = _lib.load()
    n, nf, hid = u.n, u.channels, w1.shape[0]
    assert tuple(w1.shape[:2]) == (hid, nf) and tuple(w2.shape[:2]) == (nf, hid)
    dev = u.device
    p = torch.empty((n, nf), dtype=torch.float32, device=dev)
    hb = torch.empty((n, hid), dtype=torch.float32, device=dev)
    s = torch.empty((n, nf), dtype=torch.float32, device=dev)
    ws, nbytes = _ca_workspace(lib, dev, n, nf, hid, u.h, u.w)
    launch('sr_ca_squeeze_f32', dev, u.ptr, u.img_stride, n, nf, u.h, u.w, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
           b2.data_ptr(), hid, p.data_ptr(), hb.data_ptr(), s.data_ptr(), ws.data_ptr(), nbytes)
    return p, hb, s


def ca_excite(x, u, s, res_scale=1.0, out=None):
    """out = x + res_scale * (u * s[n][c]) on CB8 (out allocated if None; may be x) — sr_ca_excite_f32."""
    if out is None:
        out = CB8.empty(u.n, u.channels, u.h, u.w, u.device)
    assert x.channels == u.channels == out.channels and s.is_contiguous()
    launch('sr_ca_excite_f32', u.device, x.ptr, x.img_stride, u.ptr, u.img_stride, s.data_ptr(), out.ptr, out.img_stride, u.n,
           u.channels, u.h, u.w, float(res_scale))
    return out


def ca_bwd(g, u, res_scale, w1, w2, p, hb, s, grads=None, accumulate=False):
    """Adjoint of the squeeze given g = dL/d(excite output): returns q [N, nf] = dL/dp / (H*W), the pooled part of dL/du.
    ``grads`` = (dW1, db1, dW2, db2) device pointers (ints or None) the weight gradients are written (or, accumulate, added)
    into — sr_ca_bwd_f32."""
    lib = _lib.load()
    n, nf, hid = u.n, u.channels, w1.shape[0]
    assert g.channels == nf and (g.n, g.h, g.w) == (n, u.h, u.w)
    dev = u.device
    q = torch.empty((n, nf), dtype=torch.float32, device=dev)
    ws, nbytes = _ca_workspace(lib, dev, n, nf, hid, u.h, u.w)
    d = tuple(grads) if grads is not None else (None, None, None, None)
    launch('sr_ca_bwd_f32', dev, g.ptr, g.img_stride, u.ptr, u.img_stride, n, nf, u.h, u.w, float(res_scale), w1.data_ptr(),
           w2.data_ptr(), hid, p.data_ptr(), hb.data_ptr(), s.data_ptr(), d[0], d[1], d[2], d[3], int(accumulate), q.data_ptr(),
           ws.data_ptr(), nbytes)
    return q


def ca_bwd_apply(g, s, q, res_scale=1.0, out=None):
    """du = (res_scale * g) * s[n][c] + q[n][c] on CB8 (out allocated if None; may be g) — sr_ca_bwd_apply_f32."""
    if out is None:
        out = CB8.empty(g.n, g.channels, g.h, g.w, g.device)
    assert out.channels == g.channels
    launch('sr_ca_bwd_apply_f32', g.device, g.ptr, g.img_stride, s.data_ptr(), q.data_ptr(), out.ptr, out.img_stride, g.n,
           g.channels, g.h, g.w, float(res_scale))
    return out


# ---- RIDNet: dilated 3x3 / 1x1 convolutions, the MeanShift ends, attention scale (include/sr_hip_ridnet.h) ----

class PackedConvK(_PackedWeights):
    """MFMA operand image of a k x k conv, k in {1, 3}, dense cin (sr_convk_pack_f32); mode 1 = data gradient.  A 3x3 image
    serves every dilation."""

    def __init__(self, weight, bias=None, mode=0):
        super().__init__(weight, bias, mode)

    def _cin_pad(self, lib, weight, first_seg, seg):
        assert weight.shape[2:] in ((1, 1), (3, 3)), weight.shape
        self.ksize = weight.shape[2]
        return (weight.shape[1] + 7) // 8 * 8

    def _image(self, lib, cout, cin, first_seg, seg, mode):
        return lib.sr_convk_packed_weight_floats(cout, cin, self.ksize, mode), 'sr_convk_pack_f32', (cout, cin, self.ksize, mode)


def convd(src, pc, dilation=1, out=None, *, post_act=False, out_pre=None, **kw):
    """Stride-1 "same" k x k conv (k = pc.ksize; dilation 1..4 for k = 3) — one sr_convd_f32 launch.
    post_act False: out = alpha*act(conv+bias) + beta1*res1 + beta2*res2 (conv3x3's epilogue); True: out = act(alpha*(conv+bias) +
    beta1*res1 + beta2*res2).  ``out_pre``: a CB8 window that also receives alpha*act(conv+bias) (post_act False).  Other keywords
    as conv3x3 (act_slope, alpha, res1/beta1, res2/beta2, accumulate, mask/mask_cb0/mask_slope)."""
    base, ret = _conv_desc_f32(src, pc, out, **kw)
    d = _lib.ConvdDesc()
    d.base, d.ksize, d.dilation, d.post_act = base, getattr(pc, 'ksize', 3), int(dilation), int(post_act)
    if out_pre is not None:
        assert (out_pre.n, out_pre.h, out_pre.w) == (ret.n, ret.h, ret.w) and out_pre.channels >= ret.channels
        d.out_pre, d.out_pre_img_stride = out_pre.ptr, out_pre.img_stride
    launch('sr_convd_f32', src.device, C.byref(d))
    return ret


def convd_wgrad(src, dy, cout, cin, ksize=3, dilation=1, *, scale=1.0, want_bias=True, out=None):
    """(dweight [cout, cin, k, k], dbias [cout]) of a convd conv from its source ``src`` and its pre-activation output gradient
    ``dy`` (CB8) — one sr_convd_wgrad_f32 call.  ``out`` = (dweight, dbias or None) device pointers the gradients are ADDED into."""
    lib = _lib.load()
    cin_pad = (cin + 7) // 8 * 8
    assert src.channels == cin_pad, (src.channels, cin_pad)
    assert (dy.n, dy.h, dy.w) == (src.n, src.h, src.w) and dy.channels >= (cout + 7) // 8 * 8
    dw, db, target = _wgrad_targets(out, (cout, cin, ksize, ksize), want_bias, src.device)
    d = _lib.ConvdWgradDesc()
    _wgrad_desc(d.base, src, dy, cin_pad, False, cout, cin, cin, 0, scale, target,
                lib.sr_convd_wgrad_slab_bytes(src.n, src.h, src.w, cout, cin, ksize, dilation))
    d.ksize, d.dilation = ksize, dilation
    launch('sr_convd_wgrad_f32', src.device, C.byref(d))
    return dw, db


def ridnet_sub_mean(x, w, b):
    """s = W x + b (RIDNet's sub_mean, a trainable 3-channel 1x1 conv) from NCHW fp32 ``x`` [N, 3, H, W] into a one-block CB8
    tensor (channels 3..7 zero) — sr_ridnet_sub_mean_f32."""
    _need_cuda(x, 'ridnet_sub_mean')
    n, c, h, ww = x.shape
    assert c == 3 and x.is_contiguous()
    out = CB8.empty(n, 8, h, ww, x.device)
    launch('sr_ridnet_sub_mean_f32', x.device, x.data_ptr(), w.data_ptr(), b.data_ptr(), out.ptr, out.img_stride, n, h, ww)
    return out


def ridnet_add_mean(x, t, w, b):
    """y = x + W t + b (add_mean plus RIDNet's global residual): ``x`` NCHW [N, 3, H, W], ``t`` the tail conv's CB8 output —
    sr_ridnet_add_mean_f32."""
    n, _, h, ww = x.shape
    y = torch.empty_like(x)
    launch('sr_ridnet_add_mean_f32', x.device, x.data_ptr(), t.ptr, t.img_stride, w.data_ptr(), b.data_ptr(), y.data_ptr(), n, h,
           ww)
    return y


def _mean_ws(lib, dev, n, h, w):
    nbytes = lib.sr_ridnet_mean_workspace_bytes(n, h, w)
    return scratch(dev, nbytes, 'ridnet_mean'), nbytes


def ridnet_sub_mean_bwd(x, g, w, dw=None, db=None, accumulate=False, want_dx=False, dx_res=None):
    """Adjoint of ridnet_sub_mean given g = dL/ds (CB8): dW, db written (accumulate: added) through the device pointers ``dw`` /
    ``db`` (ints or None); returns dx = W^T g (+ dx_res, NCHW) when ``want_dx`` — sr_ridnet_sub_mean_bwd_f32."""
    lib = _lib.load()
    n, _, h, ww = x.shape
    dev = x.device
    dx = torch.empty_like(x) if want_dx else None
    ws, nbytes = _mean_ws(lib, dev, n, h, ww)
    if dx_res is not None:
        assert dx_res.is_contiguous() and dx_res.shape == x.shape
    launch('sr_ridnet_sub_mean_bwd_f32', dev, x.data_ptr(), g.ptr, g.img_stride, w.data_ptr(), dw, db, int(accumulate),
           dx.data_ptr() if dx is not None else None, dx_res.data_ptr() if dx_res is not None else None, n, h, ww, ws.data_ptr(),
           nbytes)
    return dx


def ridnet_add_mean_bwd(g, t, w, dw=None, db=None, accumulate=False):
    """Adjoint of ridnet_add_mean's mix given g = dL/dy (NCHW): dW, db through device pointers (as ridnet_sub_mean_bwd); returns
    dt = W^T g as a one-block CB8 tensor (channels 3..7 zero) — sr_ridnet_add_mean_bwd_f32."""
    lib = _lib.load()
    g = g.contiguous()
    n, _, h, ww = g.shape
    dev = g.device
    dt = CB8.empty(n, 8, h, ww, dev)
    ws, nbytes = _mean_ws(lib, dev, n, h, ww)
    launch('sr_ridnet_add_mean_bwd_f32', dev, g.data_ptr(), t.ptr, t.img_stride, w.data_ptr(), dw, db, int(accumulate), dt.ptr,
           dt.img_stride, n, h, ww, ws.data_ptr(), nbytes)
    return dt


def ca_scale(u, s, out=None):
    """out = u * s[n][c] on CB8 (RIDNet's channel attention, no identity) — sr_ca_scale_f32."""
    if out is None:
        out = CB8.empty(u.n, u.channels, u.h, u.w, u.device)
    assert out.channels == u.channels and s.is_contiguous() and tuple(s.shape) == (u.n, u.channels)
    launch('sr_ca_scale_f32', u.device, u.ptr, u.img_stride, s.data_ptr(), out.ptr, out.img_stride, u.n, u.channels, u.h, u.w)
    return out


def relu_mask(g, mask, slope=0.0, out=None):
    """out = mask > 0 ? g : slope * g on CB8 windows of equal shape — sr_cb8_relu_mask_f32."""
    if out is None:
        out = CB8.empty(g.n, g.channels, g.h, g.w, g.device)
    assert (mask.n, mask.cbn, mask.h, mask.w) == (g.n, g.cbn, g.h, g.w) and out.cbn == g.cbn
    launch('sr_cb8_relu_mask_f32', g.device, g.ptr, g.img_stride, mask.ptr, mask.img_stride, float(slope), out.ptr,
           out.img_stride, g.n, g.cbn, g.h, g.w)
    return out


class PackedConv4x4s2(_PackedWeights):
    """Parity-pass weight images of a 4x4 / stride 2 / pad 1 conv (sr_conv4x4s2_pack_f32); mode 1 = data gradient."""

    def __init__(self, weight, bias=None, mode=0):
        super().__init__(weight, bias, mode)

    def _cin_pad(self, lib, weight, first_seg, seg):
        assert weight.shape[2:] == (4, 4)
        self.conv_cout, self.conv_cin = weight.shape[:2]
        return (self.conv_cin + 7) // 8 * 8

    def _image(self, lib, cout, cin, first_seg, seg, mode):
        return lib.sr_conv4x4s2_packed_weight_floats(cout, cin, mode), 'sr_conv4x4s2_pack_f32', (cout, cin, mode)


def conv4x4s2(src, pc, out=None, *, act_slope=1.0, alpha=1.0):
    """Forward 4x4/s2/p1 conv (+bias, LeakyReLU): four accumulating parity passes of sr_conv4x4s2_f32."""
    assert pc.mode == 0 and src.channels == pc.src_channels
    H, W = (src.h - 2) // 2 + 1, (src.w - 2) // 2 + 1
    if out is None:
        out = CB8.empty(src.n, pc.cout, H, W, src.device)
    d = _lib.ConvDesc()
    _conv_operands(d, src, pc)
    d.out, d.out_img_stride, d.n, d.act_slope, d.alpha = out.ptr, out.img_stride, src.n, act_slope, alpha
    launch('sr_conv4x4s2_f32', src.device, C.byref(d))
    return out


def conv4x4s2_dgrad(dy, pc, out_h, out_w, out=None, *, alpha=1.0, accumulate=False, mask=None, mask_cb0=0,
                    mask_slope=0.2):
    """dX of the 4x4/s2 conv from dY (sr_conv4x4s2_dgrad_f32)."""
    assert pc.mode == 1 and dy.channels == pc.src_channels
    if out is None:
        out = CB8.empty(dy.n, pc.cout, out_h, out_w, dy.device)
    d = _lib.ConvDesc()
    _conv_operands(d, dy, pc, bias=False)
    d.out, d.out_img_stride, d.out_h, d.out_w = out.ptr, out.img_stride, out_h, out_w
    d.n, d.act_slope, d.alpha, d.accumulate = dy.n, 1.0, alpha, int(accumulate)
    if mask is not None:
        _conv_mask(d, mask, mask_cb0, mask_slope)
    launch('sr_conv4x4s2_dgrad_f32', dy.device, C.byref(d))
    return out


def conv4x4s2_wgrad(src, dy, cout, cin, *, scale=1.0, want_bias=False):
    """(dweight [cout,cin,4,4], dbias) of the 4x4/s2 conv (sr_conv4x4s2_wgrad_f32)."""
    lib = _lib.load()
    cin_pad = (cin + 7) // 8 * 8
    assert src.channels == cin_pad
    H, W = (src.h - 2) // 2 + 1, (src.w - 2) // 2 + 1
    assert (dy.n, dy.h, dy.w) == (src.n, H, W)
    dw, db, target = _wgrad_targets(None, (cout, cin, 4, 4), want_bias, src.device, zeros=True)  # the passes add into dw
    d = _wgrad_desc(_lib.WgradDesc(), src, dy, cin_pad, False, cout, cin, cin, 0, scale, target,
                    lib.sr_conv3x3_wgrad_slab_bytes(src.n, H, W))
    launch('sr_conv4x4s2_wgrad_f32', src.device, C.byref(d))
    return dw, db


# ------------------------------------------------------------------ bf16 (CB16) inference ops
def nchw_to_cb16(x, unshuffle=1):
    """fp32 NCHW -> CB16 bf16 (round-to-nearest-even), pixel_unshuffle fused — sr_nchw_to_cb16_bf16."""
    _need_cuda(x, 'nchw_to_cb16')
    x = x.contiguous().float()
    n, c, sh, sw = x.shape
    h, w = sh // unshuffle, sw // unshuffle
    out = CB16.empty(n, c * unshuffle * unshuffle, h, w, x.device)  # the kernel writes every block, pad channels as zero
    launch('sr_nchw_to_cb16_bf16', x.device, x.data_ptr(), out.ptr, n, c, h, w, unshuffle, out.cbn, out.img_stride)
    return out


class PackedConvBF16(_PackedWeights):
    """bf16 MFMA weight image (+ fp32 bias) of one 3x3 conv — sr_conv3x3_pack_bf16."""
    block, wdtype = 16, torch.bfloat16

    def __init__(self, weight, bias=None, first_seg=None, seg=0, mode=0):
        super().__init__(weight, bias, mode, first_seg, seg)

    def _cin_pad(self, lib, weight, first_seg, seg):
        cin = weight.shape[1]
        self.cin_pad = lib.sr_conv3x3_cin_pad16(cin, first_seg, seg)
        if self.cin_pad <= 0:
            raise ValueError(f'cin={cin} is not first_seg={first_seg} + k*seg={seg}')
        return self.cin_pad

    def _image(self, lib, cout, cin, first_seg, seg, mode):
        return (lib.sr_conv3x3_packed_weight_elems_bf16(cout, cin, first_seg, seg, mode), 'sr_conv3x3_pack_bf16',
                (cout, cin, first_seg, seg, mode))


def _conv_desc_bf16(src, pc, out=None, *, upsample=False, act_slope=1.0, alpha=1.0, res1=None, beta1=0.0, res2=None,
                    beta2=0.0, out_nchw=None, mask=None, mask_slope=0.2, s2_channels=0, s2_side=0, out_unshuffle2=False,
                    res1_u2=False, res1_keep_sign=False):
    assert out_nchw is None or out_nchw.dtype == torch.float32
    d, ret = _conv_desc(src, pc, out, upsample, act_slope, alpha, res1, beta1, res2, beta2, out_nchw, mask, 0, mask_slope,
                        out_unshuffle2)
    d.s2_channels, d.s2_side = s2_channels, s2_side
    if res1 is not None:
        d.res1_u2, d.res1_keep_sign = int(res1_u2), int(res1_keep_sign)
    return d, ret


def conv3x3_bf16(src, pc, out=None, **kw):
    """bf16 twin of conv3x3 (fp32 accumulation and epilogue, bf16 CB16 or fp32 NCHW output) — sr_conv3x3_bf16.
    Keywords: upsample, act_slope, alpha, res1/beta1, res2/beta2, out_nchw, mask/mask_slope, s2_channels/s2_side
    (s2_channels = C marks a 4x4/s2 conv carried on a pixel-unshuffled operand of 4C channels: zero taps are skipped),
    out_unshuffle2 (the result is stored pixel-unshuffled only: [n][4 cout / 16][H / 2][W / 2][16])."""
    d, ret = _conv_desc_bf16(src, pc, out, **kw)
    launch('sr_conv3x3_bf16', src.device, C.byref(d))
    return ret


def conv3x3_chain_bf16(steps, sync=None, call_index=0):
    """A dependency chain of convs as one persistent launch — sr_conv3x3_chain_bf16.  ``steps`` = [(src, pc, out, kwargs), ...] in
    execution order (conv k reads what earlier convs wrote); ``sync`` = int32 tensor of sr_conv3x3_chain_sync_ints(n, h, w) zeros
    (created when None).  Returns (outputs, sync); sync[0] != 0 after a synchronisation means a dependency wait timed out."""
    return _conv_chain('sr_conv3x3_chain_bf16', _conv_desc_bf16, steps, sync, call_index)


def conv3x3_wgrad_bf16(src, dy, cout, cin, first_seg=None, seg=0, *, upsample=False, scale=1.0, want_bias=True):
    """(dweight, dbias) in fp32 from bf16 CB16 source and output gradient — one sr_conv3x3_wgrad_bf16 call."""
    lib = _lib.load()
    first_seg = cin if first_seg is None else first_seg
    cin_pad = lib.sr_conv3x3_cin_pad16(cin, first_seg, seg)
    assert src.channels == cin_pad, (src.channels, cin_pad)
    H, W = (2 * src.h, 2 * src.w) if upsample else (src.h, src.w)
    assert (dy.n, dy.h, dy.w) == (src.n, H, W) and dy.channels >= (cout + 15) // 16 * 16
    dw, db, target = _wgrad_targets(None, (cout, cin, 3, 3), want_bias, src.device)
    d = _wgrad_desc(_lib.WgradDesc(), src, dy, cin_pad, upsample, cout, cin, first_seg, seg, scale, target,
                    lib.sr_conv3x3_wgrad_slab_bytes_bf16(src.n, H, W), 'slab16')
    launch('sr_conv3x3_wgrad_bf16', src.device, C.byref(d))
    return dw, db


# ---- EDSR: the bf16 pixel shuffle and the image shifts at both ends (include/sr_hip_edsr.h) ----

def pixel_shuffle_bf16(src, channels, r, out=None):
    """nn.PixelShuffle(r) on CB16 (r in {2, 3}): ``src`` holds r*r*channels real channels -> CB16 of ``channels`` at r x the
    size — sr_cb16_pixel_shuffle_bf16."""
    assert src.channels >= channels * r * r
    if out is None:
        out = CB16.empty(src.n, channels, src.h * r, src.w * r, src.device)
    assert (out.n, out.h, out.w) == (src.n, src.h * r, src.w * r) and out.channels >= channels
    launch('sr_cb16_pixel_shuffle_bf16', src.device, src.ptr, src.img_stride, out.ptr, out.img_stride, src.n, channels, src.h,
           src.w, r)
    return out


def edsr_shift_in(x, mean, img_range, bf16=False):
    """(x - mean[c]) * img_range of an NCHW fp32 image [N, 3, H, W] into a one-block CB8 (fp32) or CB16 (bf16) tensor, pad
    channels zero — sr_edsr_shift_in_f32 / sr_edsr_shift_in_bf16.  ``mean``: three Python floats."""
    _need_cuda(x, 'edsr_shift_in')
    n, c, h, w = x.shape
    assert c == 3 and x.is_contiguous() and x.dtype == torch.float32 and len(mean) == 3
    out = (CB16 if bf16 else CB8).empty(n, 3, h, w, x.device)
    m = (C.c_float * 3)(*mean)
    launch('sr_edsr_shift_in_bf16' if bf16 else 'sr_edsr_shift_in_f32', x.device, x.data_ptr(), out.ptr, out.img_stride, m,
           float(img_range), n, h, w)
    return out


def edsr_shift_out(y, mean, img_range):
    """y = y / img_range + mean[c] in place on an NCHW fp32 image [N, 3, H, W] — sr_edsr_shift_out_f32."""
    _need_cuda(y, 'edsr_shift_out')
    n, c, h, w = y.shape
    assert c == 3 and y.is_contiguous() and y.dtype == torch.float32 and len(mean) == 3
    m = (C.c_float * 3)(*mean)
    launch('sr_edsr_shift_out_f32', y.device, y.data_ptr(), m, float(img_range), n, h, w)
    return y


# ---- RCAN in bf16: channel attention on CB16 tensors (include/sr_hip_ca_bf16.h) ----

def ca_squeeze_bf16(u, w1, b1, w2, b2):
    """RCAN channel attention, the squeeze, on the CB16 tensor ``u`` (all its channels): s = sigmoid(W2 relu(W1 mean_hw u + b1)
    + b2) in fp32 on the fp32 parameters as stored (W1 [hid, nf, 1, 1], W2 [nf, hid, 1, 1]).  Returns s [N, nf] fp32 —
    sr_ca_squeeze_bf16."""
    lib = _lib.load()
    n, nf, hid = u.n, u.channels, w1.shape[0]
    assert tuple(w1.shape[:2]) == (hid, nf) and tuple(w2.shape[:2]) == (nf, hid)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (w1, b1, w2, b2))
    dev = u.device
    s = torch.empty((n, nf), dtype=torch.float32, device=dev)
    nbytes = lib.sr_ca_workspace_bytes_bf16(n, nf, hid, u.h, u.w)
    ws = scratch(dev, nbytes, 'ca16')
    launch('sr_ca_squeeze_bf16', dev, u.ptr, u.img_stride, n, nf, u.h, u.w, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
           b2.data_ptr(), hid, None, None, s.data_ptr(), ws.data_ptr(), nbytes)
    return s


def ca_excite_bf16(x, u, s, res_scale=1.0, out=None):
    """out = bf16(x + res_scale * (u * s[n][c])) on CB16, evaluated in fp32 and rounded once (out allocated if None; may be x)
    — sr_ca_excite_bf16."""
    if out is None:
        out = CB16.empty(u.n, u.channels, u.h, u.w, u.device)
    assert x.channels == u.channels == out.channels and s.is_contiguous() and s.dtype == torch.float32
    launch('sr_ca_excite_bf16', u.device, x.ptr, x.img_stride, u.ptr, u.img_stride, s.data_ptr(), out.ptr, out.img_stride, u.n,
           u.channels, u.h, u.w, float(res_scale))
    return out


# ---- GFPGANv1OCR: style coefficients, modulated and upsampling convs, ToRGB (include/sr_hip_gfpgan.h) ----

def bilinear2x(src, out=None):
    """F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) on a CB8 window — sr_bilinear2x_fwd_f32."""
    if out is None:
        out = CB8.empty(src.n, src.channels, 2 * src.h, 2 * src.w, src.device)
    assert (out.n, out.cbn, out.h, out.w) == (src.n, src.cbn, 2 * src.h, 2 * src.w)
    launch('sr_bilinear2x_fwd_f32', src.device, src.ptr, src.img_stride, out.ptr, out.img_stride, src.n, src.cbn, src.h, src.w)
    return out


def cb8_channel_scale(u, s, n, out=None):
    """out[n] = u[n or 0] * s[n][c] (sr_ca_scale_f32): ``u`` with one image is repeated over the batch of ``n`` (image stride 0),
    as the decoder's constant input."""
    assert u.n in (1, n) and s.is_contiguous() and tuple(s.shape) == (n, u.channels)
    if out is None:
        out = CB8.empty(n, u.channels, u.h, u.w, u.device)
    launch('sr_ca_scale_f32', u.device, u.ptr, 0 if u.n == 1 else u.img_stride, s.data_ptr(), out.ptr, out.img_stride, n,
           u.channels, u.h, u.w)
    return out


def gfpgan_tail(demod, noise=None, noise_strength=0.0, sft=None, sft_c0=0, s_next=None):
    """struct sr_gfpgan_tail: ``demod`` [N, cout]; ``noise`` [1 or N, 1, H, W] (one map for the batch when its first dim is 1);
    ``sft`` = (scale, shift) CB8 windows applied to channels >= ``sft_c0``; ``s_next`` [N, cout]."""
    t = _lib.GfpganTail()
    assert demod.is_contiguous() and demod.dtype == torch.float32
    t.demod = demod.data_ptr()
    if noise is not None:
        assert noise.is_contiguous() and noise.dtype == torch.float32 and noise.dim() == 4 and noise.size(1) == 1
        t.noise, t.noise_img_stride = noise.data_ptr(), (0 if noise.size(0) == 1 else noise[0].numel())
        t.noise_strength = float(noise_strength)
    if sft is not None:
        sc, sh = sft
        t.sft_scale, t.sft_scale_img_stride = sc.ptr, sc.img_stride
        t.sft_shift, t.sft_shift_img_stride = sh.ptr, sh.img_stride
        t.sft_c0 = int(sft_c0)
    if s_next is not None:
        assert s_next.is_contiguous() and tuple(s_next.shape) == tuple(demod.shape)
        t.s_next = s_next.data_ptr()
    return t


def gfpgan_modconv(src, pc, tail, out=None, act_slope=0.2, alpha=2 ** 0.5):
    """One StyleConv at the source's size — sr_gfpgan_modconv_f32.  ``src``: CB8 x * s[n]; ``pc``: PackedConvK (3x3) of the
    shared weight with the StyleConv's activation bias; ``tail``: gfpgan_tail(...)."""
    base, ret = _conv_desc_f32(src, pc, out, act_slope=act_slope, alpha=alpha)
    d = _lib.GfpganModconvDesc()
    d.base, d.tail = base, tail
    launch('sr_gfpgan_modconv_f32', src.device, C.byref(d))
    return ret


def gfpgan_upconv(src, pc, out=None):
    """conv_transpose2d(src, W^T, stride 2) as four output parities -> the raw CB8 map of (2h+1) x (2w+1) —
    sr_gfpgan_upconv_f32."""
    assert src.channels == pc.src_channels and pc.ksize == 3
    if out is None:
        out = CB8.empty(src.n, pc.cout, 2 * src.h + 1, 2 * src.w + 1, src.device)
    assert (out.n, out.h, out.w) == (src.n, 2 * src.h + 1, 2 * src.w + 1) and out.channels >= pc.cout
    d = _lib.GfpganModconvDesc()
    _conv_operands(d.base, src, pc, bias=False)
    d.base.out, d.base.out_img_stride, d.base.n = out.ptr, out.img_stride, src.n
    launch('sr_gfpgan_upconv_f32', src.device, C.byref(d))
    return out


def gfpgan_blur_up(t, bias, tail, out=None, act_slope=0.2, alpha=2 ** 0.5):
    """The upsampling StyleConv's blur ([1,3,3,1]^2 / 64 * 4, pad 1) and tail: t (2h+1) x (2w+1) -> CB8 2h x 2w —
    sr_gfpgan_blur_up_f32.  ``bias``: the activation bias [cout] (contiguous fp32)."""
    h, w = (t.h - 1) // 2, (t.w - 1) // 2
    assert t.h == 2 * h + 1 and t.w == 2 * w + 1 and bias.is_contiguous()
    cout = bias.numel()
    if out is None:
        out = CB8.empty(t.n, cout, 2 * h, 2 * w, t.device)
    assert (out.n, out.h, out.w) == (t.n, 2 * h, 2 * w) and out.channels == cout == t.channels
    launch('sr_gfpgan_blur_up_f32', t.device, t.ptr, t.img_stride, out.ptr, out.img_stride, bias.data_ptr(), act_slope, alpha,
           C.byref(tail), t.n, cout, h, w)
    return out


def gfpgan_torgb(x, w, wscale, s, bias, skip=None, s_next=None):
    """ToRGB of the decoder: y [N, 3, H, W] (NCHW) = modulated 1x1 (no demodulation) + bias + upfirdn2d(skip, up 2); with
    ``s_next`` also x * s_next[n] (CB8), the next level's modulated input — sr_gfpgan_torgb_f32.  Returns (y, x_next or None)."""
    n, c = x.n, x.channels
    assert w.is_contiguous() and tuple(w.shape) == (3, c) and s.is_contiguous() and tuple(s.shape) == (n, c)
    y = torch.empty((n, 3, x.h, x.w), dtype=torch.float32, device=x.device)
    if skip is not None:
        assert skip.is_contiguous() and tuple(skip.shape) == (n, 3, x.h // 2, x.w // 2)
    xn = CB8.empty(n, c, x.h, x.w, x.device) if s_next is not None else None
    launch('sr_gfpgan_torgb_f32', x.device, x.ptr, x.img_stride, w.data_ptr(), float(wscale), s.data_ptr(), bias.data_ptr(),
           skip.data_ptr() if skip is not None else None, y.data_ptr(), xn.ptr if xn is not None else None,
           xn.img_stride if xn is not None else 0, s_next.data_ptr() if s_next is not None else None, n, c, x.h, x.w)
    return y, xn


def gfpgan_style(latent, img_stride, row_stride, nsf, layers, n):
    """Every layer's modulation s and demodulation d in one sr_gfpgan_style_f32 launch.  ``layers``: a ctypes array of
    _lib.GfpganStyleLayer whose s / d pointers name the outputs."""
    launch('sr_gfpgan_style_f32', latent.device, latent.data_ptr(), img_stride, row_stride, nsf, layers, len(layers), n)


def gfpgan_norm_style(x, out=None):
    """NormStyleCode on rows of a contiguous [N, nsf] tensor — sr_gfpgan_norm_style_f32."""
    _need_cuda(x, 'gfpgan_norm_style')
    assert x.is_contiguous() and x.dim() == 2 and x.dtype == torch.float32
    out = torch.empty_like(x) if out is None else out
    launch('sr_gfpgan_norm_style_f32', x.device, x.data_ptr(), out.data_ptr(), x.size(0), x.size(1))
    return out


def linear(x, w, b, act_slope=1.0, out=None):
    """y = lrelu(x w^T + b, act_slope) on contiguous fp32 rows — sr_linear_fwd_f32."""
    n, k = x.shape
    assert x.is_contiguous() and w.is_contiguous() and w.shape[1] == k
    y = torch.empty((n, w.shape[0]), dtype=torch.float32, device=x.device) if out is None else out
    launch('sr_linear_fwd_f32', x.device, x.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None, y.data_ptr(), n, k,
           w.shape[0], float(act_slope))
    return y


# ---- modulated deformable convolution (DCNv2): forward, columns, scatter / coordinate gradients (include/sr_hip_dcn.h) ----

class PackedDcnT:
    """ksize-1 forward image of Wt[tap * cin + ci][co] of a 3x3 weight (sr_dcn_pack_t_f32): sr_convd_f32 with it turns dY into
    the column gradient dcol of 9 * cin channels.  Quacks like a PackedConvK for ``convd``."""
    ksize, mode, b = 1, 0, None

    def __init__(self, weight):
        _need_cuda(weight, 'PackedDcnT')
        weight = weight.detach().contiguous().float()
        cout, cin = weight.shape[:2]
        assert weight.shape[2:] == (3, 3) and cin % 8 == 0
        self.cout, self.src_channels = 9 * cin, (cout + 7) // 8 * 8
        self.w = torch.empty(_lib.load().sr_dcn_packed_t_weight_floats(cout, cin), dtype=torch.float32, device=weight.device)
        launch('sr_dcn_pack_t_f32', weight.device, weight.data_ptr(), cout, cin, self.w.data_ptr())


def _dcn_desc(d, x, offset, mask, dg, mask_is_logit, cout):
    """The operand and geometry fields of a struct sr_dcn_desc: ``x`` / ``offset`` / ``mask`` are CB8 windows."""
    assert (offset.n, offset.h, offset.w) == (mask.n, mask.h, mask.w) == (x.n, x.h, x.w)
    assert offset.channels >= 18 * dg and mask.channels >= 9 * dg
    d.x, d.x_img_stride = x.ptr, x.img_stride
    d.offset, d.offset_img_stride = offset.ptr, offset.img_stride
    d.mask, d.mask_img_stride, d.mask_is_logit = mask.ptr, mask.img_stride, int(mask_is_logit)
    d.n, d.cin, d.cout, d.h, d.w, d.deformable_groups = x.n, x.channels, cout, x.h, x.w, dg
    d.ksize, d.stride, d.padding, d.dilation, d.groups, d.act_slope = 3, 1, 1, 1, 1, 1.0
    return d


def dcn_fwd(x, offset, mask, pc, dg, *, mask_is_logit=False, act_slope=1.0, out=None):
    """out = lrelu(bias + sum W * mask * bilinear sample of x at the offset positions) — one sr_dcn_fwd_f32 launch.  ``x``: CB8
    window of cin channels (cin / dg a multiple of 8); ``offset`` / ``mask``: CB8 windows of 18 * dg / 9 * dg channels in the
    reference's order; ``pc``: PackedConvK or PackedConv (mode 0) of the 3x3 weight."""
    assert pc.mode == 0 and x.channels == pc.src_channels
    if out is None:
        out = CB8.empty(x.n, pc.cout, x.h, x.w, x.device)
    assert (out.n, out.h, out.w) == (x.n, x.h, x.w) and out.channels >= (pc.cout + 7) // 8 * 8
    d = _dcn_desc(_lib.DcnDesc(), x, offset, mask, dg, mask_is_logit, pc.cout)
    d.wpacked, d.bpacked = pc.w.data_ptr(), pc.b.data_ptr() if pc.b is not None else None
    d.out, d.out_img_stride, d.act_slope = out.ptr, out.img_stride, act_slope
    launch('sr_dcn_fwd_f32', x.device, C.byref(d))
    return out


def dcn_cols(x, offset, mask, dg, *, mask_is_logit=False):
    """The masked columns as a CB8 tensor of 9 * cin channels, tap-major — sr_dcn_cols_f32."""
    cols = CB8.empty(x.n, 9 * x.channels, x.h, x.w, x.device)
    d = _dcn_desc(_lib.DcnDesc(), x, offset, mask, dg, mask_is_logit, 1)
    launch('sr_dcn_cols_f32', x.device, C.byref(d), cols.ptr, cols.buf.numel() * 4)
    return cols


def dcn_wgrad(cols, dy, cout, cin, want_bias=True):
    """(dweight [cout, cin, 3, 3], dbias [cout]) from the columns and the pre-activation output gradient: sr_convd_wgrad_f32
    with ksize 1 over 9 * cin channels, then sr_dcn_weight_unpack_f32."""
    dwc, db = convd_wgrad(cols, dy, cout, 9 * cin, ksize=1, want_bias=want_bias)
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=dwc.device)
    launch('sr_dcn_weight_unpack_f32', dwc.device, dwc.data_ptr(), cout, cin, dw.data_ptr(), 0)
    return dw, db


def _dcn_bwd_desc(d, dcol, x, offset, mask, dg, mask_is_logit, dx, doffset, dmask):
    """The fields of a struct sr_dcn_bwd_desc; ``dx`` and ``doffset`` / ``dmask`` may be None.  The callers check that they fit."""
    _dcn_desc(d.fwd, x, offset, mask, dg, mask_is_logit, 1)
    d.dcol = dcol.ptr
    if dx is not None:
        d.dx, d.dx_img_stride = dx.ptr, dx.img_stride
    if doffset is not None:
        d.doffset, d.doffset_img_stride, d.dmask, d.dmask_img_stride = doffset.ptr, doffset.img_stride, dmask.ptr, dmask.img_stride
    return d


def _det_workspace(who, dd, device, nbytes, workspace):
    """The workspace fields of a deterministic descriptor: ``workspace`` (uint8, at least ``nbytes`` on ``device``), or the
    grow-only scratch when None."""
    if workspace is None:
        workspace = scratch(device, nbytes, who)
    _arg(workspace.dtype == torch.uint8 and workspace.numel() >= nbytes and workspace.device == device,
         f'{who}: the workspace is too small')
    dd.workspace, dd.workspace_bytes = workspace.data_ptr(), nbytes


def dcn_bwd_data(dcol, x, offset, mask, dg, *, mask_is_logit=False, want_dx=True, dx=None, doffset=None, dmask=None):
    """dx (atomicAdd scatter into a zeroed CB8 tensor, or ADDED into the CB8 window ``dx`` when given; returned, or None) and,
    into the CB8 windows ``doffset`` / ``dmask`` (given together or not at all), the offset and mask (or logit) gradients — one
    sr_dcn_bwd_data_f32 launch."""
    assert dcol.channels == 9 * x.channels and dcol.cb0 == 0 and dcol.cbn == dcol.buf.size(1)
    if dx is None and want_dx:
        dx = CB8.zeros(x.n, x.channels, x.h, x.w, x.device)
    assert dx is None or (dx.n, dx.cbn, dx.h, dx.w) == (x.n, x.cbn, x.h, x.w)
    assert doffset is None or (doffset.channels >= 18 * dg and dmask.channels >= 9 * dg)
    d = _dcn_bwd_desc(_lib.DcnBwdDesc(), dcol, x, offset, mask, dg, mask_is_logit, dx, doffset, dmask)
    launch('sr_dcn_bwd_data_f32', x.device, C.byref(d))
    return dx


def dcn_bwd_data_det_workspace_bytes(n, cin, h, w):
    """Bytes of the workspace of dcn_bwd_data_det — sr_dcn_bwd_data_det_workspace_bytes."""
    return _lib.load().sr_dcn_bwd_data_det_workspace_bytes(n, cin, h, w)


def dcn_bwd_data_det(dcol, x, offset, mask, dg, *, mask_is_logit=False, want_dx=True, dx=None, doffset=None, dmask=None, workspace=None):
    """dcn_bwd_data with a bit-reproducible ``dx`` (include/sr_hip_dcn_det.h) — one sr_dcn_bwd_data_det_f32 call: the terms are
    summed as 64-bit integers in ``workspace`` (uint8, dcn_bwd_data_det_workspace_bytes; the grow-only scratch when None) and
    STORED into ``dx`` with one rounding (a new CB8 tensor, or the CB8 window ``dx`` when given, which need not be zeroed;
    returned, or None); ``doffset`` / ``dmask`` are dcn_bwd_data's bit for bit."""
    who = 'dcn_bwd_data_det'
    _arg(isinstance(dcol, CB8) and isinstance(x, CB8) and dcol.channels == 9 * x.channels and dcol.cb0 == 0
         and dcol.cbn == dcol.buf.size(1), f'{who}: dcol must be a whole CB8 tensor of 9 * cin channels')
    _arg((doffset is None) == (dmask is None), f'{who}: doffset and dmask go together')
    if dx is None and want_dx:
        dx = CB8.empty(x.n, x.channels, x.h, x.w, x.device)
    _arg(dx is None or (isinstance(dx, CB8) and (dx.n, dx.cbn, dx.h, dx.w) == (x.n, x.cbn, x.h, x.w)), f'{who}: dx does not fit')
    dd = _lib.DcnBwdDetDesc()
    _dcn_bwd_desc(dd.d, dcol, x, offset, mask, dg, mask_is_logit, dx, doffset, dmask)
    if dx is not None:
        nbytes = dcn_bwd_data_det_workspace_bytes(x.n, x.channels, x.h, x.w)
        _arg(nbytes > 0, f'{who}: bad shape n={x.n} cin={x.channels} h={x.h} w={x.w}')
        _det_workspace(who, dd, x.device, nbytes, workspace)
    _arg(doffset is None or (doffset.channels >= 18 * dg and dmask.channels >= 9 * dg), f'{who}: doffset / dmask do not fit')
    _launch_arg('sr_dcn_bwd_data_det_f32', x.device, C.byref(dd))
    return dx


# ---- EDVR: stride-2 conv and its zero insertion, TSA's pooling, correlation and gate (include/sr_hip_edvr.h) ----

def _arg(cond, msg):
    """Bad arguments of the EDVR wrappers are ValueErrors (the C ABI's SR_EINVAL)."""
    if not cond:
        raise ValueError(msg)


def _same(a, *others):
    return all((o.n, o.cbn, o.h, o.w) == (a.n, a.cbn, a.h, a.w) for o in others)


def conv3x3s2(src, pc, out=None, *, act_slope=1.0):
    """out = lrelu(conv(src) + bias) for a 3x3 / stride 2 / pad 1 conv: (H + 1) // 2 x (W + 1) // 2 — one sr_conv3x3s2_f32
    launch.  ``pc``: PackedConvK or PackedConv (mode 0) of the 3x3 weight."""
    _arg(pc.mode == 0 and getattr(pc, 'ksize', 3) == 3, 'conv3x3s2: needs the forward image of a 3x3 weight')
    _arg(src.channels == pc.src_channels, f'conv3x3s2: source has {src.channels} channels, the weight image {pc.src_channels}')
    ho, wo = (src.h + 1) // 2, (src.w + 1) // 2
    if out is None:
        out = CB8.empty(src.n, pc.cout, ho, wo, src.device)
    _arg((out.n, out.h, out.w) == (src.n, ho, wo) and out.channels >= (pc.cout + 7) // 8 * 8, 'conv3x3s2: output window does not fit')
    d = _lib.ConvS2Desc()
    d.in_, d.in_img_stride, d.cin_pad, d.in_h, d.in_w = src.ptr, src.img_stride, pc.src_channels, src.h, src.w
    d.wpacked, d.bpacked, d.cout = pc.w.data_ptr(), pc.b.data_ptr() if pc.b is not None else None, pc.cout
    d.out, d.out_img_stride, d.n, d.act_slope = out.ptr, out.img_stride, src.n, act_slope
    launch('sr_conv3x3s2_f32', src.device, C.byref(d))
    return out


def zero_insert2(dy, h, w, out=None):
    """``dy`` ((h + 1) // 2 x (w + 1) // 2) at the even positions of a zero-filled h x w tensor — sr_cb8_zero_insert2_f32."""
    _arg((dy.h, dy.w) == ((h + 1) // 2, (w + 1) // 2), f'zero_insert2: {dy.h}x{dy.w} is not the stride-2 size of {h}x{w}')
    if out is None:
        out = CB8.empty(dy.n, dy.channels, h, w, dy.device)
    _arg((out.n, out.cbn, out.h, out.w) == (dy.n, dy.cbn, h, w), 'zero_insert2: output window does not fit')
    launch('sr_cb8_zero_insert2_f32', dy.device, dy.ptr, dy.img_stride, out.ptr, out.img_stride, dy.n, dy.cbn, h, w)
    return out


def pool3x3s2(src, out=None):
    """torch.cat([MaxPool2d(3, 2, 1)(x), AvgPool2d(3, 2, 1)(x)], 1) as one CB8 tensor of 2 * channels — one sr_pool3x3s2_fwd_f32
    launch writing both windows.  ``out``: a CB8 window of 2 * src.cbn blocks."""
    ho, wo = (src.h + 1) // 2, (src.w + 1) // 2
    if out is None:
        out = CB8.empty(src.n, 2 * src.channels, ho, wo, src.device)
    _arg((out.n, out.cbn, out.h, out.w) == (src.n, 2 * src.cbn, ho, wo), 'pool3x3s2: output window does not fit')
    mx, av = CB8(out.buf, out.cb0, src.cbn), CB8(out.buf, out.cb0 + src.cbn, src.cbn)
    launch('sr_pool3x3s2_fwd_f32', src.device, src.ptr, src.img_stride, mx.ptr, mx.img_stride, av.ptr, av.img_stride, src.n,
           src.cbn, src.h, src.w)
    return out


def pool3x3s2_bwd(src, g, out=None):
    """dx of pool3x3s2 from its source and ``g``, the gradient of the [max, avg] tensor — sr_pool3x3s2_bwd_f32."""
    ho, wo = (src.h + 1) // 2, (src.w + 1) // 2
    _arg((g.n, g.cbn, g.h, g.w) == (src.n, 2 * src.cbn, ho, wo), 'pool3x3s2_bwd: gradient does not fit the source')
    if out is None:
        out = CB8.empty(src.n, src.channels, src.h, src.w, src.device)
    _arg(_same(src, out), 'pool3x3s2_bwd: output window does not fit')
    gm, ga = CB8(g.buf, g.cb0, src.cbn), CB8(g.buf, g.cb0 + src.cbn, src.cbn)
    launch('sr_pool3x3s2_bwd_f32', src.device, src.ptr, src.img_stride, gm.ptr, gm.img_stride, ga.ptr, ga.img_stride, out.ptr,
           out.img_stride, src.n, src.cbn, src.h, src.w)
    return out


def tsa_corr(emb, emb_ref, aligned, t, out=None):
    """TSA's temporal attention: (prob [b, t, h, w], aligned * prob as CB8 [b * t, c]) with prob = sigmoid(sum_c emb * emb_ref) —
    one sr_tsa_corr_fwd_f32 launch.  ``emb`` / ``aligned``: CB8 windows of b * t images, ``emb_ref``: of b images."""
    _arg(t >= 1 and emb.n == emb_ref.n * t, f'tsa_corr: {emb.n} frames are not {emb_ref.n} x {t}')
    _arg(_same(emb, aligned) and (emb_ref.cbn, emb_ref.h, emb_ref.w) == (emb.cbn, emb.h, emb.w), 'tsa_corr: shapes differ')
    if out is None:
        out = CB8.empty(emb.n, emb.channels, emb.h, emb.w, emb.device)
    _arg(_same(emb, out), 'tsa_corr: output window does not fit')
    prob = torch.empty((emb_ref.n, t, emb.h, emb.w), dtype=torch.float32, device=emb.device)
    launch('sr_tsa_corr_fwd_f32', emb.device, emb.ptr, emb.img_stride, emb_ref.ptr, emb_ref.img_stride, aligned.ptr,
           aligned.img_stride, prob.data_ptr(), out.ptr, out.img_stride, emb_ref.n, t, emb.channels, emb.h, emb.w)
    return prob, out


def tsa_corr_bwd(g, emb, emb_ref, aligned, prob):
    """(d aligned, d emb, d emb_ref) of tsa_corr from ``g``, the gradient of its CB8 output — sr_tsa_corr_bwd_f32."""
    b, t = prob.shape[:2]
    _arg(prob.is_contiguous() and prob.dtype == torch.float32 and tuple(prob.shape) == (emb_ref.n, t, emb.h, emb.w) and emb.n == b * t,
         'tsa_corr_bwd: prob does not fit')
    _arg(_same(emb, aligned, g) and (emb_ref.cbn, emb_ref.h, emb_ref.w) == (emb.cbn, emb.h, emb.w), 'tsa_corr_bwd: shapes differ')
    dal = CB8.empty(emb.n, emb.channels, emb.h, emb.w, emb.device)
    demb = CB8.empty(emb.n, emb.channels, emb.h, emb.w, emb.device)
    dref = CB8.empty(b, emb.channels, emb.h, emb.w, emb.device)
    dcorr = torch.empty_like(prob)
    launch('sr_tsa_corr_bwd_f32', emb.device, g.ptr, g.img_stride, emb.ptr, emb.img_stride, emb_ref.ptr, emb_ref.img_stride,
           aligned.ptr, aligned.img_stride, prob.data_ptr(), dcorr.data_ptr(), dal.ptr, dal.img_stride, demb.ptr, demb.img_stride,
           dref.ptr, dref.img_stride, b, t, emb.channels, emb.h, emb.w)
    return dal, demb, dref


def tsa_gate(feat, attn, attn_add, out=None):
    """out = feat * sigmoid(attn) * 2 + attn_add on CB8 windows of equal shape — sr_tsa_gate_fwd_f32."""
    _arg(_same(feat, attn, attn_add), 'tsa_gate: shapes differ')
    if out is None:
        out = CB8.empty(feat.n, feat.channels, feat.h, feat.w, feat.device)
    _arg(_same(feat, out), 'tsa_gate: output window does not fit')
    launch('sr_tsa_gate_fwd_f32', feat.device, feat.ptr, feat.img_stride, attn.ptr, attn.img_stride, attn_add.ptr,
           attn_add.img_stride, out.ptr, out.img_stride, feat.n, feat.cbn, feat.h, feat.w)
    return out


def tsa_gate_bwd(g, feat, attn):
    """(d feat, d attn) of tsa_gate from ``g``, the gradient of its output (d attn_add is ``g``) — sr_tsa_gate_bwd_f32."""
    _arg(_same(feat, attn, g), 'tsa_gate_bwd: shapes differ')
    df = CB8.empty(feat.n, feat.channels, feat.h, feat.w, feat.device)
    da = CB8.empty(feat.n, feat.channels, feat.h, feat.w, feat.device)
    launch('sr_tsa_gate_bwd_f32', feat.device, g.ptr, g.img_stride, feat.ptr, feat.img_stride, attn.ptr, attn.img_stride, df.ptr,
           df.img_stride, da.ptr, da.img_stride, feat.n, feat.cbn, feat.h, feat.w)
    return df, da


# ---- EDVR in bf16: deformable conv, 1x1 conv, subsample, pooling, correlation and gate on CB16 (include/sr_hip_edvr_bf16.h) ----

def _launch_arg(name, dev, *args):
    """``launch`` for the entry points of sr_hip_edvr_bf16.h: their SR_EINVAL is a ValueError, as the wrappers' own checks."""
    try:
        launch(name, dev, *args)
    except _lib.SrHipError as e:
        if '(status -1)' in str(e):
            raise ValueError(str(e)) from None
        raise


def _bias_image(bias, cout, dev):
    return None if bias is None else torch.empty(_lib.load().sr_conv3x3_packed_bias_floats(cout), dtype=torch.float32, device=dev)


class PackedConv1x1BF16:
    """bf16 MFMA weight image (+ fp32 bias) of one 1x1 conv over CB16 — sr_conv1x1_pack_bf16."""
    mode, ksize = 0, 1

    def __init__(self, weight, bias=None):
        _need_cuda(weight, 'PackedConv1x1BF16')
        weight = weight.detach().contiguous().float()
        cout, cin = weight.shape[:2]
        _arg(weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1), 'PackedConv1x1BF16: needs a [cout, cin, 1, 1] weight')
        _arg(cin % 16 == 0, f'PackedConv1x1BF16: cin={cin} must be a multiple of 16 (CB16)')
        self.cout, self.src_channels = cout, cin
        dev = weight.device
        self.w = torch.empty(_lib.load().sr_conv1x1_packed_weight_elems_bf16(cout, cin), dtype=torch.bfloat16, device=dev)
        self.b = _bias_image(bias, cout, dev)
        if bias is not None:
            bias = bias.detach().contiguous().float()
        _launch_arg('sr_conv1x1_pack_bf16', dev, weight.data_ptr(), bias.data_ptr() if bias is not None else None, cout, cin,
                    self.w.data_ptr(), self.b.data_ptr() if self.b is not None else None)


def packed_conv_bf16(conv):
    """The bf16 forward image of a parameter container (3x3: PackedConvBF16, 1x1: PackedConv1x1BF16), cached per parameter
    version under a bf16 key."""
    w, b = conv.weight, conv.bias
    if w.shape[2] == 3:
        return cached_pack('bf16 image', w, b, lambda: PackedConvBF16(w, b))
    return cached_pack('bf16 image 1x1', w, b, lambda: PackedConv1x1BF16(w, b))


def conv1x1_bf16(src, pc, out=None, *, act_slope=1.0):
    """out = bf16(lrelu(W x + bias)) for a 1x1 conv on CB16 — one sr_conv1x1_bf16 launch.  ``pc``: PackedConv1x1BF16."""
    _arg(getattr(pc, 'ksize', 3) == 1 and pc.mode == 0, 'conv1x1_bf16: needs the forward image of a 1x1 weight')
    _arg(src.channels == pc.src_channels, f'conv1x1_bf16: source has {src.channels} channels, the weight image {pc.src_channels}')
    if out is None:
        out = CB16.empty(src.n, pc.cout, src.h, src.w, src.device)
    _arg((out.n, out.h, out.w) == (src.n, src.h, src.w) and out.channels >= (pc.cout + 15) // 16 * 16,
         'conv1x1_bf16: output window does not fit')
    _launch_arg('sr_conv1x1_bf16', src.device, src.ptr, src.img_stride, pc.w.data_ptr(), pc.b.data_ptr() if pc.b is not None else None,
                out.ptr, out.img_stride, src.n, pc.src_channels, pc.cout, src.h, src.w, float(act_slope))
    return out


def _planes(t, channels, like, what):
    """(pointer, image stride in floats) of an fp32 NCHW tensor or channel slice whose images are dense planes."""
    _arg(t.dtype == torch.float32 and t.dim() == 4 and tuple(t.shape) == (like.n, channels, like.h, like.w)
         and tuple(t.stride()[1:]) == (like.h * like.w, like.w, 1), f'{what}: needs dense fp32 planes [{like.n}, {channels}, {like.h}, {like.w}]')
    return t.data_ptr(), t.stride(0) if like.n > 1 else max(t.stride(0), channels * like.h * like.w)


def dcn_fwd_bf16(x, offset, mask, pc, dg, *, mask_is_logit=False, act_slope=1.0, out=None):
    """Modulated deformable 3x3 conv on CB16 — one sr_dcn_fwd_bf16 launch.  ``x``: CB16 window of cin channels (cin / dg a
    multiple of 8); ``offset`` / ``mask``: fp32 NCHW tensors (or channel slices of one) of 18 * dg / 9 * dg planes in the
    reference's order; ``pc``: PackedConvBF16 (mode 0) of the 3x3 weight."""
    _arg(pc.mode == 0 and getattr(pc, 'ksize', 3) == 3, 'dcn_fwd_bf16: needs the forward image of a 3x3 weight')
    _arg(x.channels == pc.src_channels, f'dcn_fwd_bf16: source has {x.channels} channels, the weight image {pc.src_channels}')
    _arg(dg > 0 and x.channels % dg == 0 and (x.channels // dg) % 8 == 0,
         f'dcn_fwd_bf16: cin {x.channels} / deformable_groups {dg} must be a multiple of 8')
    if out is None:
        out = CB16.empty(x.n, pc.cout, x.h, x.w, x.device)
    _arg((out.n, out.h, out.w) == (x.n, x.h, x.w) and out.channels >= (pc.cout + 15) // 16 * 16, 'dcn_fwd_bf16: output window does not fit')
    d = _lib.DcnBf16Desc()
    d.x, d.x_img_stride = x.ptr, x.img_stride
    d.offset, d.offset_img_stride = _planes(offset, 18 * dg, x, 'dcn_fwd_bf16 offset')
    d.mask, d.mask_img_stride = _planes(mask, 9 * dg, x, 'dcn_fwd_bf16 mask')
    d.mask_is_logit = int(mask_is_logit)
    d.wpacked, d.bpacked = pc.w.data_ptr(), pc.b.data_ptr() if pc.b is not None else None
    d.out, d.out_img_stride = out.ptr, out.img_stride
    d.n, d.cin, d.cout, d.h, d.w, d.deformable_groups = x.n, x.channels, pc.cout, x.h, x.w, dg
    d.ksize, d.stride, d.padding, d.dilation, d.groups, d.act_slope = 3, 1, 1, 1, 1, float(act_slope)
    _launch_arg('sr_dcn_fwd_bf16', x.device, C.byref(d))
    return out


def dcn_bf16_instance(cout, n, h, w):
    """(COT, tile rows, dynamic LDS bytes) of the sr_dcn_fwd_bf16 launch for this shape — sr_dcn_bf16_lds_bytes."""
    cot, rows = C.c_int(0), C.c_int(0)
    lds = _lib.load().sr_dcn_bf16_lds_bytes(cout, n, h, w, C.byref(cot), C.byref(rows))
    return cot.value, rows.value, lds


def subsample2_bf16(src, out=None):
    """The even rows and columns of a CB16 window: (H + 1) // 2 x (W + 1) // 2 — sr_cb16_subsample2_bf16."""
    ho, wo = (src.h + 1) // 2, (src.w + 1) // 2
    if out is None:
        out = CB16.empty(src.n, src.channels, ho, wo, src.device)
    _arg((out.n, out.cbn, out.h, out.w) == (src.n, src.cbn, ho, wo), 'subsample2_bf16: output window does not fit')
    _launch_arg('sr_cb16_subsample2_bf16', src.device, src.ptr, src.img_stride, out.ptr, out.img_stride, src.n, src.cbn, src.h, src.w)
    return out


def pool3x3s2_bf16(src, out=None):
    """torch.cat([MaxPool2d(3, 2, 1)(x), AvgPool2d(3, 2, 1)(x)], 1) as one CB16 tensor of 2 * channels — one
    sr_pool3x3s2_fwd_bf16 launch writing both windows.  ``out``: a CB16 window of 2 * src.cbn blocks."""
    ho, wo = (src.h + 1) // 2, (src.w + 1) // 2
    if out is None:
        out = CB16.empty(src.n, 2 * src.channels, ho, wo, src.device)
    _arg((out.n, out.cbn, out.h, out.w) == (src.n, 2 * src.cbn, ho, wo), 'pool3x3s2_bf16: output window does not fit')
    mx, av = CB16(out.buf, out.cb0, src.cbn), CB16(out.buf, out.cb0 + src.cbn, src.cbn)
    _launch_arg('sr_pool3x3s2_fwd_bf16', src.device, src.ptr, src.img_stride, mx.ptr, mx.img_stride, av.ptr, av.img_stride, src.n,
                src.cbn, src.h, src.w)
    return out


def tsa_corr_bf16(emb, emb_ref, aligned, t, out=None, want_prob=False):
    """TSA's temporal attention on CB16: aligned * sigmoid(sum_c emb * emb_ref) as CB16 [b * t, c] (and prob [b, t, h, w] fp32
    with ``want_prob``) — one sr_tsa_corr_fwd_bf16 launch.  ``emb`` / ``aligned``: windows of b * t images, ``emb_ref``: of b."""
    _arg(t >= 1 and emb.n == emb_ref.n * t, f'tsa_corr_bf16: {emb.n} frames are not {emb_ref.n} x {t}')
    _arg(_same(emb, aligned) and (emb_ref.cbn, emb_ref.h, emb_ref.w) == (emb.cbn, emb.h, emb.w), 'tsa_corr_bf16: shapes differ')
    if out is None:
        out = CB16.empty(emb.n, emb.channels, emb.h, emb.w, emb.device)
    _arg(_same(emb, out), 'tsa_corr_bf16: output window does not fit')
    prob = torch.empty((emb_ref.n, t, emb.h, emb.w), dtype=torch.float32, device=emb.device) if want_prob else None
    _launch_arg('sr_tsa_corr_fwd_bf16', emb.device, emb.ptr, emb.img_stride, emb_ref.ptr, emb_ref.img_stride, aligned.ptr,
                aligned.img_stride, prob.data_ptr() if want_prob else None, out.ptr, out.img_stride, emb_ref.n, t, emb.channels,
                emb.h, emb.w)
    return (prob, out) if want_prob else out


def tsa_gate_bf16(feat, attn, attn_add, out=None):
    """out = bf16(feat * sigmoid(attn) * 2 + attn_add) on CB16 windows of equal shape — sr_tsa_gate_fwd_bf16."""
    _arg(_same(feat, attn, attn_add), 'tsa_gate_bf16: shapes differ')
    if out is None:
        out = CB16.empty(feat.n, feat.channels, feat.h, feat.w, feat.device)
    _arg(_same(feat, out), 'tsa_gate_bf16: output window does not fit')
    _launch_arg('sr_tsa_gate_fwd_bf16', feat.device, feat.ptr, feat.img_stride, attn.ptr, attn.img_stride, attn_add.ptr,
                attn_add.img_stride, out.ptr, out.img_stride, feat.n, feat.cbn, feat.h, feat.w)
    return out


def bilinear2x_bf16(src, skip=None):
    """F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) of ``src`` (of bf16(src + skip) when given) on CB16 —
    sr_bilinear2x_fwd_bf16."""
    _arg(skip is None or _same(src, skip), 'bilinear2x_bf16: shapes differ')
    out = CB16.empty(src.n, src.channels, 2 * src.h, 2 * src.w, src.device)
    launch('sr_bilinear2x_fwd_bf16', src.device, src.ptr, src.img_stride, skip.ptr if skip is not None else None,
           skip.img_stride if skip is not None else 0, out.ptr, out.img_stride, src.n, src.cbn, src.h, src.w)
    return out


def cb16_scale(t, a):
    """t = bf16(a * t) in place on a CB16 window (exact for a power of two) — sr_cb16_axpby_bf16 with b = 0."""
    launch('sr_cb16_axpby_bf16', t.device, t.ptr, t.img_stride, t.ptr, t.img_stride, float(a), 0.0, t.n, t.cbn, t.h, t.w)
    return t


# ---- StyleGAN2 building blocks: upfirdn2d and the fused bias + LeakyReLU on NCHW tensors (include/sr_hip_stylegan2.h) ----

def upfirdn2d_instance(kh, kw, up_x, up_y, down_x, down_y):
    """(instance, tile rows, LDS bytes) of an sr_upfirdn2d_f32 call with this filter size and these factors
    (sr_upfirdn2d_instance): 0 generic, 1 / 2 / 3 the 4x4 filter at (up, down) = (1, 1) / (2, 1) / (1, 2); tiles are 64 columns
    wide.  ValueError when the filter or the factors are not supported."""
    th, lds = C.c_int(0), C.c_size_t(0)
    inst = _lib.load().sr_upfirdn2d_instance(kh, kw, up_x, up_y, down_x, down_y, C.byref(th), C.byref(lds))
    _arg(inst >= 0, f'upfirdn2d: filter {kh}x{kw}, up ({up_x}, {up_y}), down ({down_x}, {down_y}) is not supported; supported: '
                    'fp32, filter sides 1..16, factors 1..8')
    return inst, th.value, lds.value


def upfirdn2d_out_size(in_h, in_w, kh, kw, up, down, pad):
    """(out_h, out_w) of upfirdn2d: (in * up + pad0 + pad1 - k) // down + 1 per axis; up, down = (x, y), pad = (x0, x1, y0, y1)."""
    return ((in_h * up[1] + pad[2] + pad[3] - kh) // down[1] + 1, (in_w * up[0] + pad[0] + pad[1] - kw) // down[0] + 1)


def upfirdn2d(x, kernel, up, down, pad, out=None):
    """Up-sample by ``up`` = (x, y), pad by ``pad`` = (x0, x1, y0, y1), convolve with the [kh, kw] ``kernel``, keep every
    ``down``-th sample, on every plane of the contiguous fp32 NCHW tensor ``x`` — one sr_upfirdn2d_f32 launch."""
    _need_cuda(x, 'upfirdn2d')
    _arg(x.dim() == 4 and x.is_contiguous() and x.dtype == torch.float32, 'upfirdn2d: needs a contiguous fp32 NCHW tensor')
    _arg(kernel.dim() == 2 and kernel.is_contiguous() and kernel.dtype == torch.float32 and kernel.device == x.device,
         'upfirdn2d: needs a contiguous fp32 [kh, kw] kernel on the device of the input')
    n, c, h, w = x.shape
    kh, kw = kernel.shape
    upfirdn2d_instance(kh, kw, up[0], up[1], down[0], down[1])
    oh, ow = upfirdn2d_out_size(h, w, kh, kw, up, down, pad)
    _arg(oh > 0 and ow > 0, f'upfirdn2d: output size {oh}x{ow} is not positive (input {h}x{w}, kernel {kh}x{kw}, up {tuple(up)}, '
                            f'down {tuple(down)}, pad {tuple(pad)})')
    if out is None:
        out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    _arg(tuple(out.shape) == (n, c, oh, ow) and out.is_contiguous() and out.dtype == torch.float32, 'upfirdn2d: output does not fit')
    if n * c:
        _launch_arg('sr_upfirdn2d_f32', x.device, x.data_ptr(), c * h * w, out.data_ptr(), c * oh * ow, kernel.data_ptr(), n, c, h, w, 1,
                    kh, kw, up[0], up[1], down[0], down[1], *pad)
    return out


def _act_shape(x, what):
    _need_cuda(x, what)
    _arg(x.dim() >= 2 and x.is_contiguous() and x.dtype == torch.float32, f'{what}: needs a contiguous fp32 tensor of rank >= 2')
    inner = 1
    for s in x.shape[2:]:
        inner *= s
    return x.size(0), x.size(1), inner


def fused_bias_act(x, bias=None, ref=None, slope=0.2, scale=2 ** 0.5):
    """lrelu(x + bias[c], slope) * scale with the channel on dimension 1; the sign comes from ``ref`` where one is given — one
    sr_fused_bias_act_f32 launch."""
    n, c, inner = _act_shape(x, 'fused_bias_act')
    _arg(bias is None or (bias.dim() == 1 and bias.numel() == c and bias.is_contiguous() and bias.dtype == torch.float32),
         f'fused_bias_act: needs a contiguous fp32 bias of {c} values')
    _arg(ref is None or (ref.shape == x.shape and ref.is_contiguous() and ref.dtype == torch.float32), 'fused_bias_act: ref does not fit')
    out = torch.empty_like(x)
    if x.numel():
        _launch_arg('sr_fused_bias_act_f32', x.device, x.data_ptr(), None if bias is None else bias.data_ptr(),
                    None if ref is None else ref.data_ptr(), out.data_ptr(), n, c, inner, float(slope), float(scale))
    return out


def fused_bias_act_bwd(g, out, slope=0.2, scale=2 ** 0.5, want_bias=True):
    """(gx, gbias) of fused_bias_act from the gradient ``g`` of its output ``out``: gx = lrelu_by(out)(g) * scale, gbias[c] its sum
    over every other dimension, from the same pass — sr_fused_bias_act_bwd_f32."""
    n, c, inner = _act_shape(g, 'fused_bias_act_bwd')
    _arg(out.shape == g.shape and out.is_contiguous() and out.dtype == torch.float32, 'fused_bias_act_bwd: out does not fit')
    gx = torch.empty_like(g)
    gbias = torch.zeros(c, dtype=torch.float32, device=g.device) if want_bias else None
    if g.numel():
        nbytes = _lib.load().sr_fused_bias_act_workspace_bytes(n, c, inner) if want_bias else 0
        ws = scratch(g.device, nbytes, 'act') if want_bias else None
        _launch_arg('sr_fused_bias_act_bwd_f32', g.device, g.data_ptr(), out.data_ptr(), gx.data_ptr(),
                    gbias.data_ptr() if want_bias else None, n, c, inner, float(slope), float(scale),
                    ws.data_ptr() if want_bias else None, nbytes)
    return gx, gbias


# ---- the degradation chain of the plate training set on NCHW tensors (include/sr_hip_degrade.h) ----

def _image_batch(t, what, channels=None):
    _need_cuda(t, what)
    _arg(t.dim() == 4 and t.is_contiguous() and t.dtype == torch.float32 and t.numel() > 0
         and (channels is None or t.size(1) == channels),
         f'{what}: needs a non-empty contiguous fp32 [B, {channels or "C"}, H, W] tensor, got {t.dtype} {tuple(t.shape)}')
    return t.shape


def _per_sample(v, b, like, what, width=None):
    """A per-sample fp32 device array [B] (or [B, width]) from a tensor, a sequence or a number; None stays None."""
    if v is None:
        return None
    if not torch.is_tensor(v):
        v = torch.tensor(v, dtype=torch.float32)
        if v.dim() == 0:
            v = v.expand(b)
    v = v.to(device=like.device, dtype=torch.float32).contiguous()
    _arg(tuple(v.shape) == ((b,) if width is None else (b, width)), f'{what}: expected {b} per-sample values, got {tuple(v.shape)}')
    return v


def ragged_sizes(sizes, b, hmax, wmax, dev, what='sizes'):
    """The int32 device array [B, 2] of (h_i, w_i) a ragged batch travels with.  A sequence or a CPU tensor is checked here (every
    entry in 1..Hmax x 1..Wmax: the C ABI cannot refuse what lies on the device, its kernels clamp); a device tensor passes as is."""
    if sizes is None:
        return None
    if torch.is_tensor(sizes) and sizes.is_cuda:
        _arg(sizes.dtype == torch.int32 and tuple(sizes.shape) == (b, 2) and sizes.is_contiguous(),
             f'{what}: a device size array is int32 [{b}, 2]')
        return sizes
    host = torch.as_tensor(sizes).to(torch.int64).reshape(-1, 2)
    _arg(host.size(0) == b, f'{what}: {host.size(0)} sizes for a batch of {b}')
    _arg(bool((host >= 1).all()) and int(host[:, 0].max()) <= hmax and int(host[:, 1].max()) <= wmax,
         f'{what}: every (h, w) must lie in 1..{hmax} x 1..{wmax}, got {host.tolist()}')
    return host.to(torch.int32).to(dev)


def _p(t):
    return None if t is None else t.data_ptr()


def filter2d(img, kernel, out=None):
    """Correlation of every plane of ``img`` [B, C, H, W] with ``kernel`` [1 or B, k, k] under the reflect border — one
    sr_filter2d_f32 launch."""
    b, c, h, w = _image_batch(img, 'filter2d')
    _arg(kernel.dim() == 3 and kernel.size(1) == kernel.size(2) and kernel.dtype == torch.float32 and kernel.device == img.device,
         f'filter2d: needs an fp32 [1 or B, k, k] kernel on the device of the image, got {kernel.dtype} {tuple(kernel.shape)}')
    kernel = kernel.contiguous()
    k, kb = kernel.size(1), kernel.size(0)
    _arg(k % 2 == 1 and k <= 21, f'filter2d: kernel size {k} is not supported: odd, 1..21')
    _arg(h > k // 2 and w > k // 2, f'filter2d: a {h}x{w} image is too small to reflect by {k // 2}')
    _arg(kb in (1, b), f'filter2d: {kb} kernels for a batch of {b}')
    if out is None:
        out = torch.empty_like(img)
    _arg(out.shape == img.shape and out.is_contiguous() and out.dtype == torch.float32 and out.data_ptr() != img.data_ptr(),
         'filter2d: output does not fit (and cannot be the input)')
    _launch_arg('sr_filter2d_f32', img.device, img.data_ptr(), kernel.data_ptr(), out.data_ptr(), b, c, h, w, k, kb)
    return out


def resize_bilinear(x, size, src_sizes=None, dst_sizes=None, out=None):
    """``x`` [B, C, Hs, Ws] to [B, C, *size], bilinear, half-pixel centres, no antialiasing; with size arrays each sample is
    resized from / to its own rectangle and the rest of the output is zero — one sr_resize_bilinear_f32 launch."""
    b, c, hs, ws = _image_batch(x, 'resize_bilinear')
    hd, wd = int(size[0]), int(size[1])
    _arg(hd > 0 and wd > 0, f'resize_bilinear: output size {hd}x{wd} is not positive')
    ss = ragged_sizes(src_sizes, b, hs, ws, x.device, 'resize_bilinear: src_sizes')
    ds = ragged_sizes(dst_sizes, b, hd, wd, x.device, 'resize_bilinear: dst_sizes')
    if out is None:
        out = torch.empty((b, c, hd, wd), dtype=torch.float32, device=x.device)
    _arg(tuple(out.shape) == (b, c, hd, wd) and out.is_contiguous() and out.dtype == torch.float32 and out.data_ptr() != x.data_ptr(),
         'resize_bilinear: output does not fit (and cannot be the input)')
    _launch_arg('sr_resize_bilinear_f32', x.device, x.data_ptr(), _p(ss), out.data_ptr(), _p(ds), b, c, hs, ws, hd, wd)
    return out


def add_gaussian_noise(x, noise, sigma, noise_gray=None, gray=None, clip=True, rounds=False, out=None):
    """x + noise * sigma[b] / 255 (the gray plane for every channel where gray[b] is set), then the reference's clip / round cases
    — one sr_add_gaussian_noise_f32 launch."""
    b, c, h, w = _image_batch(x, 'add_gaussian_noise')
    _arg(noise.shape == x.shape and noise.is_contiguous() and noise.dtype == torch.float32 and noise.device == x.device,
         'add_gaussian_noise: noise does not fit the image')
    sigma = _per_sample(sigma, b, x, 'add_gaussian_noise: sigma')
    gray = _per_sample(gray, b, x, 'add_gaussian_noise: gray')
    _arg(gray is None or noise_gray is not None, 'add_gaussian_noise: gray needs noise_gray')
    _arg(noise_gray is None or (tuple(noise_gray.shape) == (b, 1, h, w) and noise_gray.is_contiguous() and noise_gray.dtype == torch.float32
                                and noise_gray.device == x.device), f'add_gaussian_noise: noise_gray must be fp32 [{b}, 1, {h}, {w}]')
    if out is None:
        out = torch.empty_like(x)
    _arg(out.shape == x.shape and out.is_contiguous() and out.dtype == torch.float32, 'add_gaussian_noise: output does not fit')
    _launch_arg('sr_add_gaussian_noise_f32', x.device, x.data_ptr(), noise.data_ptr(), _p(noise_gray), sigma.data_ptr(), _p(gray),
                out.data_ptr(), b, c, h, w, int(bool(clip)), int(bool(rounds)))
    return out


def diffjpeg(x, factor, sizes=None, differentiable=False, out=None):
    """DiffJPEG's round trip of the RGB batch ``x`` [B, 3, H, W] in [0, 1] with the quantisation factors ``factor`` [B] — one
    sr_diffjpeg_f32 launch."""
    b, _, h, w = _image_batch(x, 'diffjpeg', 3)
    factor = _per_sample(factor, b, x, 'diffjpeg: factor')
    sz = ragged_sizes(sizes, b, h, w, x.device, 'diffjpeg: sizes')
    if out is None:
        out = torch.empty_like(x)
    _arg(out.shape == x.shape and out.is_contiguous() and out.dtype == torch.float32, 'diffjpeg: output does not fit')
    _launch_arg('sr_diffjpeg_f32', x.device, x.data_ptr(), _p(sz), factor.data_ptr(), out.data_ptr(), b, h, w, int(bool(differentiable)))
    return out


def diffjpeg_bwd(x, factor, grad_out, sizes=None):
    """The gradient of diffjpeg(differentiable=True) with respect to ``x`` — one sr_diffjpeg_bwd_f32 launch; nothing but ``x`` was
    saved."""
    b, _, h, w = _image_batch(x, 'diffjpeg_bwd', 3)
    _need_cuda(grad_out, 'diffjpeg_bwd')
    grad_out = grad_out.contiguous()
    _arg(grad_out.shape == x.shape and grad_out.dtype == torch.float32, 'diffjpeg_bwd: grad_out does not fit')
    factor = _per_sample(factor, b, x, 'diffjpeg_bwd: factor')
    sz = ragged_sizes(sizes, b, h, w, x.device, 'diffjpeg_bwd: sizes')
    gx = torch.empty_like(x)
    _launch_arg('sr_diffjpeg_bwd_f32', x.device, x.data_ptr(), _p(sz), factor.data_ptr(), grad_out.data_ptr(), gx.data_ptr(), b, h, w)
    return gx


def degrade_finish(x, jitter=None, gray=None, mean=None, std=None, out=None):
    """The tail of the degradation: per-sample jitter shift + clip, gray where set, round to 8 bits, normalise — one
    sr_degrade_finish_f32 launch on the RGB batch ``x`` [B, 3, H, W]."""
    b, _, h, w = _image_batch(x, 'degrade_finish', 3)
    jitter = _per_sample(jitter, b, x, 'degrade_finish: jitter', 3)
    gray = _per_sample(gray, b, x, 'degrade_finish: gray')
    f3 = [None if v is None else (C.c_float * 3)(*[float(t) for t in v]) for v in (mean, std)]
    if out is None:
        out = torch.empty_like(x)
    _arg(out.shape == x.shape and out.is_contiguous() and out.dtype == torch.float32, 'degrade_finish: output does not fit')
    _launch_arg('sr_degrade_finish_f32', x.device, x.data_ptr(), _p(jitter), _p(gray), out.data_ptr(), b, h, w, f3[0], f3[1])
    return out


# ---- optical flow: the 7x7 conv, flow warping and SpyNet's pieces (include/sr_hip_flow.h) ----

CONV7X7_SHAPES = ((8, 32), (32, 64), (64, 32), (32, 16), (16, 2))   # (cin, cout) of SpyNet's BasicModule
FLOW_PADDING = {'zeros': 0, 'border': 1}


def conv7x7_instance(cout, cin):
    """The kernel instance sr_conv7x7_f32 runs a (cin, cout) pair on (sr_conv7x7_instance): 0 = 32 couts x 16 rows, 1 = 64 couts
    x 8 rows, 2 = the few-cout form.  ValueError for a pair that is not served."""
    inst = _lib.load().sr_conv7x7_instance(cout, cin)
    _arg(inst >= 0, f'conv7x7: (cin, cout) = ({cin}, {cout}) is not supported; supported: {CONV7X7_SHAPES}')
    return inst


class _PackedConvTaps:
    """What PackedConv7x7 and PackedConv9x9 share: the device, mode, shape and bias checks, ``cout`` / ``cin`` / ``mode`` and the
    one image ``w`` (weights in operand order, then the bias).  A subclass states ``ksize``, the ``modes`` it serves, its size
    query (``_packed_floats``, which refuses a (cin, cout) pair that is not served) and its pack launch (``_pack``)."""
    ksize, modes = None, ()

    def __init__(self, weight, bias=None, mode=0):
        name, k = type(self).__name__, self.ksize
        _need_cuda(weight, name)
        _arg(mode in range(len(self.modes)),
             f'{name}: mode {mode} is not supported; supported: ' + ', '.join(f'{i} ({m})' for i, m in enumerate(self.modes)))
        _arg(mode == 0 or bias is None, f'{name}: the data-gradient image has no bias')
        _arg(weight.dim() == 4 and tuple(weight.shape[2:]) == (k, k) and weight.dtype == torch.float32,
             f'{name}: needs an fp32 [cout, cin, {k}, {k}] weight, got {weight.dtype} {tuple(weight.shape)}')
        _arg(bias is None or (bias.dtype == torch.float32 and tuple(bias.shape) == (weight.size(0),)), f'{name}: bias does not fit')
        weight = weight.detach().contiguous()
        bias = None if bias is None else bias.detach().contiguous()
        self.mode = mode
        self.cout, self.cin = weight.shape[:2]
        self.w = torch.empty(self._packed_floats(_lib.load()), dtype=torch.float32, device=weight.device)
        self._pack(weight.device, weight.data_ptr(), _p(bias))


class PackedConv7x7(_PackedConvTaps):
    """MFMA operand image of one 7x7 conv of SpyNet: mode 0 the forward image (weights, then bias) — sr_conv7x7_pack_f32;
    mode 1 the data-gradient image (the weights flipped and transposed, no bias) — sr_conv7x7_dgrad_pack_f32."""
    ksize, modes = 7, ('forward', 'data gradient')

    def _packed_floats(self, lib):
        self.instance = conv7x7_instance(self.cout, self.cin)     # refuses a pair that is not served
        if self.mode == 0:
            return lib.sr_conv7x7_packed_floats(self.cout, self.cin)
        self.instance = lib.sr_conv7x7_dgrad_instance(self.cout, self.cin)
        return lib.sr_conv7x7_dgrad_packed_floats(self.cout, self.cin)

    def _pack(self, dev, weight, bias):
        if self.mode == 0:
            _launch_arg('sr_conv7x7_pack_f32', dev, weight, bias, self.cout, self.cin, self.w.data_ptr())
        else:
            _launch_arg('sr_conv7x7_dgrad_pack_f32', dev, weight, self.cout, self.cin, self.w.data_ptr())


def _conv_taps_desc(d, src, pc, out, relu):
    """The fields a struct sr_conv7x7_desc and a struct sr_tof_conv9x9_desc have in common."""
    d.in_, d.in_img_stride, d.cin, d.cout, d.n, d.h, d.w = src.ptr, src.img_stride, pc.cin, pc.cout, src.n, src.h, src.w
    d.packed, d.out, d.out_img_stride, d.relu = pc.w.data_ptr(), out.ptr, out.img_stride, int(bool(relu))
    return d


def conv7x7(src, pc, out=None, *, relu=False, res1=None):
    """out = [relu](conv7x7(src) + bias) [+ res1] on CB8, stride 1, pad 3 — one sr_conv7x7_f32 launch.  ``pc``: PackedConv7x7."""
    _arg(getattr(pc, 'mode', 0) == 0, 'conv7x7: needs the forward image (mode 0)')
    _arg(src.channels == pc.cin, f'conv7x7: source has {src.channels} channels, the weight image {pc.cin}')
    if out is None:
        out = CB8.empty(src.n, pc.cout, src.h, src.w, src.device)
    cob = (pc.cout + 7) // 8
    _arg((out.n, out.h, out.w) == (src.n, src.h, src.w) and out.cbn >= cob, 'conv7x7: output window does not fit')
    _arg(res1 is None or ((res1.n, res1.h, res1.w) == (src.n, src.h, src.w) and res1.cbn >= cob), 'conv7x7: res1 does not fit')
    d = _conv_taps_desc(_lib.Conv7x7Desc(), src, pc, out, relu)
    if res1 is not None:
        d.res1, d.res1_img_stride = res1.ptr, res1.img_stride
    _launch_arg('sr_conv7x7_f32', src.device, C.byref(d))
    return out


def _warp_operands(x, flow, channels, padding, what):
    """(pointer source, n, c, h, w, layout) of a warp call: ``x`` an fp32 NCHW tensor, or a CB8 window that is its whole buffer
    with ``channels`` real channels."""
    _arg(padding in FLOW_PADDING, f"{what}: padding_mode '{padding}' is not supported; supported: 'zeros', 'border'")
    if isinstance(x, CB8):
        c = x.channels if channels is None else channels
        _arg(x.cb0 == 0 and x.cbn == x.buf.size(1) == (c + 7) // 8, f'{what}: a CB8 source is a whole buffer of ceil({c} / 8) blocks')
        n, h, w, layout, dev = x.n, x.h, x.w, 1, x.device
    else:
        _need_cuda(x, what)
        _arg(x.dim() == 4 and x.is_contiguous() and x.dtype == torch.float32 and x.numel() > 0,
             f'{what}: needs a non-empty contiguous fp32 [N, C, H, W] tensor, got {x.dtype} {tuple(x.shape)}')
        (n, c, h, w), layout, dev = x.shape, 0, x.device
    _arg(flow.dtype == torch.float32 and flow.is_contiguous() and flow.device == dev and tuple(flow.shape) == (n, h, w, 2),
         f'{what}: flow must be a contiguous fp32 [{n}, {h}, {w}, 2] tensor on the device of x, got {flow.dtype} {tuple(flow.shape)}')
    return n, c, h, w, layout


def _like(x):
    return CB8(torch.empty_like(x.buf)) if isinstance(x, CB8) else torch.empty_like(x)


def _tp(t):
    return t.ptr if isinstance(t, CB8) else t.data_ptr()


def flow_warp(x, flow, padding='zeros', channels=None, out=None):
    """grid_sample(x, pixel grid + flow, bilinear, ``padding``, align_corners=True) — one sr_flow_warp_f32 launch.  ``x``: NCHW
    tensor or CB8 buffer (``channels`` real channels), ``flow`` [N, H, W, 2] in pixels; the result is laid out like ``x``."""
    n, c, h, w, layout = _warp_operands(x, flow, channels, padding, 'flow_warp')
    if out is None:
        out = _like(x)
    _arg(isinstance(out, CB8) == bool(layout) and (out.buf.shape == x.buf.shape if layout else (out.shape == x.shape and out.is_contiguous()
                                                                                 and out.dtype == torch.float32)),
         'flow_warp: output does not fit')
    _launch_arg('sr_flow_warp_f32', flow.device, _tp(x), flow.data_ptr(), _tp(out), n, c, h, w, layout, FLOW_PADDING[padding])
    return out


def flow_warp_bwd(x, flow, g, padding='zeros', channels=None, want_dx=True, want_dflow=True):
    """(dx, dflow) of flow_warp from ``g``, the gradient of its output (laid out like ``x``) — sr_flow_warp_bwd_f32.  dx is
    accumulated with float atomics into a zeroed tensor; dflow is a gather."""
    n, c, h, w, layout = _warp_operands(x, flow, channels, padding, 'flow_warp_bwd')
    _arg(isinstance(g, CB8) == bool(layout) and (g.buf.shape == x.buf.shape if layout else (g.shape == x.shape and g.is_contiguous()
                                                                           and g.dtype == torch.float32)),
         'flow_warp_bwd: the output gradient does not fit')
    dx = dflow = None
    if want_dx:
        dx = CB8(torch.zeros_like(x.buf)) if layout else torch.zeros_like(x)
    if want_dflow:
        dflow = torch.empty_like(flow)
    if want_dx or want_dflow:
        _launch_arg('sr_flow_warp_bwd_f32', flow.device, _tp(x), flow.data_ptr(), _tp(g), None if dx is None else _tp(dx), _p(dflow),
                    n, c, h, w, layout, FLOW_PADDING[padding])
    return dx, dflow


def spynet_level_input(ref, supp, flow_prev=None):
    """(the level's 8-channel CB8 input block [ref, warp(supp, up), up], up as a CB8 block) from the level's images [N, 3, H, W]
    and the coarser level's flow (a one-block CB8 window at H / 2 x W / 2, None at the coarsest level: up = 0) — one
    sr_spynet_level_input_f32 launch."""
    n, _, h, w = _image_batch(ref, 'spynet_level_input', 3)
    _arg(supp.shape == ref.shape and supp.is_contiguous() and supp.dtype == torch.float32 and supp.device == ref.device,
         'spynet_level_input: supp does not fit ref')
    _arg(flow_prev is None or (h % 2 == 0 and w % 2 == 0 and flow_prev.cb0 == 0 and tuple(flow_prev.buf.shape) == (n, 1, h // 2, w // 2, 8)),
         f'spynet_level_input: flow_prev must be one CB8 block at {h // 2}x{w // 2}')
    out, up = CB8.empty(n, 8, h, w, ref.device), CB8.empty(n, 8, h, w, ref.device)
    _launch_arg('sr_spynet_level_input_f32', ref.device, ref.data_ptr(), supp.data_ptr(), None if flow_prev is None else flow_prev.ptr,
                out.ptr, up.ptr, n, h, w)
    return out, up


def spynet_preprocess(x, mean, std, out=None):
    """(x - mean[c]) / std[c] on an RGB batch [N, 3, H, W] — one sr_spynet_preprocess_f32 launch."""
    n, _, h, w = _image_batch(x, 'spynet_preprocess', 3)
    f3 = [(C.c_float * 3)(*[float(t) for t in v]) for v in (mean, std)]
    if out is None:
        out = torch.empty_like(x)
    _arg(out.shape == x.shape and out.is_contiguous() and out.dtype == torch.float32, 'spynet_preprocess: output does not fit')
    _launch_arg('sr_spynet_preprocess_f32', x.device, x.data_ptr(), out.data_ptr(), n, h, w, f3[0], f3[1])
    return out


def avgpool2x2(x):
    """F.avg_pool2d(x, 2, 2) of a contiguous fp32 [N, C, H, W] tensor with even H and W — one sr_avgpool2x2_f32 launch."""
    n, c, h, w = _image_batch(x, 'avgpool2x2')
    _arg(h % 2 == 0 and w % 2 == 0, f'avgpool2x2: {h}x{w} is not even')
    out = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    _launch_arg('sr_avgpool2x2_f32', x.device, x.data_ptr(), out.data_ptr(), n * c, h, w)
    return out


# ---- SpyNet's backward: 7x7 data and weight gradients, level-input and resize adjoints (include/sr_hip_flow_bwd.h) ----

def conv7x7_dgrad(dy, pc, out=None, *, mask=None):
    """dx = (7x7 data gradient of ``dy``) * (mask > 0) on CB8 — one sr_conv7x7_dgrad_f32 launch.  ``pc``: PackedConv7x7(mode=1);
    ``dy`` holds the conv's output gradient (ceil(cout / 8) blocks), ``mask`` the post-ReLU activation that fed the conv."""
    _arg(getattr(pc, 'mode', 0) == 1, 'conv7x7_dgrad: needs the data-gradient image (mode 1)')
    dyb = (pc.cout + 7) // 8
    _arg(dy.cbn == dyb, f'conv7x7_dgrad: dy has {dy.cbn} channel blocks, the weight image {dyb}')
    if out is None:
        out = CB8.empty(dy.n, pc.cin, dy.h, dy.w, dy.device)
    _arg((out.n, out.h, out.w) == (dy.n, dy.h, dy.w) and out.cbn == pc.cin // 8, 'conv7x7_dgrad: output window does not fit')
    _arg(mask is None or ((mask.n, mask.h, mask.w) == (dy.n, dy.h, dy.w) and mask.cbn == pc.cin // 8), 'conv7x7_dgrad: mask does not fit')
    d = _lib.Conv7x7DgradDesc()
    d.dy, d.dy_img_stride, d.cin, d.cout, d.n, d.h, d.w = dy.ptr, dy.img_stride, pc.cin, pc.cout, dy.n, dy.h, dy.w
    d.packed, d.dx, d.dx_img_stride = pc.w.data_ptr(), out.ptr, out.img_stride
    if mask is not None:
        d.mask, d.mask_img_stride = mask.ptr, mask.img_stride
    _launch_arg('sr_conv7x7_dgrad_f32', dy.device, C.byref(d))
    return out


def conv7x7_wgrad(src, dy, cout, cin, *, scale=1.0, want_bias=True, out=None):
    """(dweight [cout, cin, 7, 7], dbias [cout]) of a 7x7 conv of SpyNet whose source was ``src`` (CB8) and whose pre-activation
    output gradient is ``dy`` (CB8) — one sr_conv7x7_wgrad_f32 call (tiles + fixed-order reduction).  ``out`` = (dweight, dbias
    or None): device pointers (ints) the gradients are ADDED into (accumulate = 1, e.g. a FlatAdam gradient arena) instead."""
    _arg((cin, cout) in CONV7X7_SHAPES, f'conv7x7_wgrad: (cin, cout) = ({cin}, {cout}) is not supported; supported: {CONV7X7_SHAPES}')
    _arg(src.cbn == cin // 8 and dy.cbn == (cout + 7) // 8 and (dy.n, dy.h, dy.w) == (src.n, src.h, src.w),
         'conv7x7_wgrad: src / dy do not fit the pair')
    nbytes = _lib.load().sr_conv7x7_wgrad_slab_bytes(src.n, src.h, src.w, cout, cin)
    slab = scratch(src.device, nbytes, 'slab7')
    dw, db, target = _wgrad_targets(out, (cout, cin, 7, 7), want_bias, src.device)
    d = _lib.Conv7x7WgradDesc()
    d.x, d.x_img_stride, d.dy, d.dy_img_stride = src.ptr, src.img_stride, dy.ptr, dy.img_stride
    d.cin, d.cout, d.n, d.h, d.w, d.scale = cin, cout, src.n, src.h, src.w, scale
    d.dweight, d.dbias, d.accumulate = target
    d.slab, d.slab_bytes = slab.data_ptr(), nbytes
    _launch_arg('sr_conv7x7_wgrad_f32', src.device, C.byref(d))
    return None if out is not None else (dw, db)


def spynet_level_input_bwd(supp, up, g_in, g_res):
    """The gradient of the coarser level's flow (a one-block CB8 tensor at H / 2 x W / 2) from a level's ``supp`` [N, 3, H, W],
    its saved ``up`` block, the gradient ``g_in`` of its input block and the gradient ``g_res`` of its output flow (one-block CB8
    windows at H x W) — one sr_spynet_level_input_bwd_f32 call (two launches)."""
    n, _, h, w = _image_batch(supp, 'spynet_level_input_bwd', 3)
    _arg(h % 2 == 0 and w % 2 == 0, f'spynet_level_input_bwd: {h}x{w} is not even')
    for t, name in ((up, 'up'), (g_in, 'g_in'), (g_res, 'g_res')):
        _arg(isinstance(t, CB8) and t.cb0 == 0 and tuple(t.buf.shape) == (n, 1, h, w, 8) and t.device == supp.device,
             f'spynet_level_input_bwd: {name} must be one CB8 block at {h}x{w}')
    d_up = torch.empty((n, h, w, 2), dtype=torch.float32, device=supp.device)
    g_prev = CB8.empty(n, 8, h // 2, w // 2, supp.device)
    _launch_arg('sr_spynet_level_input_bwd_f32', supp.device, supp.data_ptr(), up.ptr, g_in.ptr, g_res.ptr, d_up.data_ptr(),
                g_prev.ptr, n, h, w)
    return g_prev


def resize_bilinear_adjoint(dy, size):
    """The transpose of F.interpolate(size=dy.shape[2:], mode='bilinear', align_corners=False) applied to ``dy`` [N, C, Hd, Wd]:
    the gradient [N, C, *size] of the resize's input — one sr_resize_bilinear_adjoint_f32 launch."""
    n, c, hd, wd = _image_batch(dy, 'resize_bilinear_adjoint')
    hs, ws = int(size[0]), int(size[1])
    _arg(hs > 0 and ws > 0, f'resize_bilinear_adjoint: bad size {size}')
    dx = torch.empty((n, c, hs, ws), dtype=torch.float32, device=dy.device)
    _launch_arg('sr_resize_bilinear_adjoint_f32', dy.device, dy.data_ptr(), dx.data_ptr(), n * c, hs, ws, hd, wd)
    return dx


# ---- the recurrent video networks: propagation step input and trunk driver, fp32 on CB8 (include/sr_hip_vsr.h) and bf16 on
# CB16 (include/sr_hip_vsr_bf16.h).  One implementation each, told the window class and the symbols; the public wrappers keep the
# literal _launch_arg call of their entry point ----

def _vsr_prop_desc(who, CB, Desc, frame, prev, flow, warp_out, frame_out):
    """The checked and filled descriptor of a step-input launch on windows of class ``CB``."""
    _need_cuda(frame, who)
    _arg(frame.dim() == 4 and frame.size(1) == 3 and frame.dtype == torch.float32 and frame.numel() > 0 and frame[0].is_contiguous(),
         f'{who}: needs an fp32 [N, 3, H, W] frame batch with dense images, got {frame.dtype} {tuple(frame.shape)}')
    n, _, h, w = frame.shape
    _arg((prev is None) == (flow is None), f'{who}: prev and flow come together')
    _arg(isinstance(warp_out, CB) and (warp_out.n, warp_out.h, warp_out.w) == (n, h, w), f'{who}: warp_out does not fit')
    d = Desc()
    d.frame, d.frame_img_stride = frame.data_ptr(), frame.stride(0)
    if prev is not None:
        _arg(isinstance(prev, CB) and (prev.n, prev.h, prev.w, prev.cbn) == (n, h, w, warp_out.cbn), f'{who}: prev does not fit')
        _arg(flow.dtype == torch.float32 and tuple(flow.shape) == (n, 2, h, w) and flow[0].is_contiguous() and flow.device == frame.device,
             f'{who}: flow must be an fp32 [{n}, 2, {h}, {w}] view with dense images, got {flow.dtype} {tuple(flow.shape)}')
        d.prev, d.prev_img_stride, d.flow, d.flow_img_stride = prev.ptr, prev.img_stride, flow.data_ptr(), flow.stride(0)
    if frame_out is not None:
        _arg(isinstance(frame_out, CB) and (frame_out.n, frame_out.h, frame_out.w, frame_out.cbn) == (n, h, w, 1),
             f'{who}: frame_out must be a one-block window')
        d.frame_out, d.frame_out_img_stride = frame_out.ptr, frame_out.img_stride
    d.warp_out, d.warp_out_img_stride = warp_out.ptr, warp_out.img_stride
    d.n, d.h, d.w, d.fb = n, h, w, warp_out.cbn
    return d


def vsr_prop_input(frame, prev, flow, warp_out, frame_out=None):
    """What one propagation step feeds its trunk — one sr_vsr_prop_input_f32 launch.  ``frame``: fp32 [N, 3, H, W] view whose
    images are dense (``x[:, i]`` of a clip is read in place); ``prev``: CB8 window of the previous propagated feature or None;
    ``flow``: fp32 [N, 2, H, W] view with dense images (what SpyNet returns), None iff ``prev`` is None.  Writes
    flow_warp(prev, flow) (zeros for None) into the CB8 window ``warp_out`` and, when given, the frame into the one-block
    window ``frame_out``."""
    d = _vsr_prop_desc('vsr_prop_input', CB8, _lib.VsrPropDesc, frame, prev, flow, warp_out, frame_out)
    _launch_arg('sr_vsr_prop_input_f32', frame.device, C.byref(d))
    return warp_out


def vsr_prop_input_bf16(frame, prev, flow, warp_out, frame_out=None):
    """The CB16 twin of vsr_prop_input — one sr_rvsr_prop_input_bf16 launch.  ``frame`` and ``flow`` stay fp32 views with dense
    images ([N, 3, H, W], [N, 2, H, W]); ``prev``, ``warp_out`` and the one-block ``frame_out`` are CB16 windows.  Writes
    bf16(flow_warp(widened prev, flow)) (zeros for None) into ``warp_out`` and bf16(frame) with 13 zero channels into ``frame_out``."""
    d = _vsr_prop_desc('vsr_prop_input_bf16', CB16, _lib.RvsrPropDesc, frame, prev, flow, warp_out, frame_out)
    _launch_arg('sr_rvsr_prop_input_bf16', frame.device, C.byref(d))
    return warp_out


def vsr_trunk_cfg(num_feat, num_block, cin_segs=1):
    return _lib.VsrTrunkCfg(int(num_feat), int(num_block), int(cin_segs))


def vsr_trunk_wino_convs(cfg):
    """Per conv of a trunk (the first conv, then conv1, conv2 of each block): whether the blob holds a Winograd image for it."""
    lib = _lib.load()
    n = lib.sr_vsr_trunk_num_params(C.byref(cfg))
    _arg(n > 0, f'vsr_trunk: bad config num_feat={cfg.num_feat} num_block={cfg.num_block} cin_segs={cfg.cin_segs}')
    return [bool(lib.sr_vsr_trunk_conv_wino(C.byref(cfg), i)) for i in range(n // 2)]


def _vsr_trunk_pack_args(who, bytes_query, cfg, params, blob):
    """(blob, parameter pointer array) of a trunk pack call; the parameter count is sr_vsr_trunk_num_params for both kinds."""
    lib = _lib.load()
    n = lib.sr_vsr_trunk_num_params(C.byref(cfg))
    _arg(n > 0 and n == len(params), f'{who}: {len(params)} parameters, the config has {n}')
    for p in params:
        _need_cuda(p, who)
        _arg(p.dtype == torch.float32 and p.is_contiguous(), f'{who}: parameters must be contiguous fp32')
    nbytes = getattr(lib, bytes_query)(C.byref(cfg))
    if blob is None:
        blob = torch.empty(nbytes, dtype=torch.uint8, device=params[0].device)
    _arg(blob.numel() >= nbytes and blob.dtype == torch.uint8, f'{who}: blob too small')
    return blob, (C.c_void_p * n)(*[p.data_ptr() for p in params])


def vsr_trunk_pack(cfg, params, blob=None):
    """The packed blob of a trunk from its parameters in state_dict order (device fp32, contiguous) — sr_vsr_trunk_pack_f32."""
    blob, ptrs = _vsr_trunk_pack_args('vsr_trunk_pack', 'sr_vsr_trunk_packed_bytes', cfg, params, blob)
    _launch_arg('sr_vsr_trunk_pack_f32', blob.device, C.byref(cfg), ptrs, blob.data_ptr())
    return blob


def vsr_trunk_pack_bf16(cfg, params, blob=None):
    """The bf16 blob of a trunk (bf16 weight images, fp32 biases) from its fp32 parameters in state_dict order —
    sr_rvsr_trunk_pack_bf16."""
    _arg(_lib.load().sr_rvsr_trunk_packed_bytes_bf16(C.byref(cfg)) > 0,
         f'vsr_trunk_pack_bf16: bad config num_feat={cfg.num_feat} (a multiple of 16, CB16) num_block={cfg.num_block} '
         f'cin_segs={cfg.cin_segs}')
    blob, ptrs = _vsr_trunk_pack_args('vsr_trunk_pack_bf16', 'sr_rvsr_trunk_packed_bytes_bf16', cfg, params, blob)
    _launch_arg('sr_rvsr_trunk_pack_bf16', blob.device, C.byref(cfg), ptrs, blob.data_ptr())
    return blob


def _vsr_trunk_args(who, CB, lanes, ws_query, cfg, blob, src, out):
    """The checked arguments of a trunk call on windows of class ``CB`` (``lanes`` channels a block), after the device."""
    _arg(isinstance(src, CB) and isinstance(out, CB) and src.cbn == 1 + cfg.cin_segs * cfg.num_feat // lanes
         and out.cbn == cfg.num_feat // lanes and (out.n, out.h, out.w) == (src.n, src.h, src.w), f'{who}: windows do not fit the config')
    nbytes = getattr(_lib.load(), ws_query)(C.byref(cfg), src.n, src.h, src.w)
    ws = scratch(src.device, nbytes, who)
    return (C.byref(cfg), blob.data_ptr(), src.ptr, src.img_stride, out.ptr, out.img_stride, src.n, src.h, src.w, ws.data_ptr(), nbytes)


def vsr_trunk(cfg, blob, src, out):
    """ConvResidualBlocks on the CB8 window ``src`` (frame block + cin_segs feature windows) into the CB8 window ``out`` — one
    sr_vsr_trunk_f32 call: 1 + 2 * num_block conv launches, no allocation beyond the grow-only scratch."""
    _launch_arg('sr_vsr_trunk_f32', src.device, *_vsr_trunk_args('vsr_trunk', CB8, 8, 'sr_vsr_trunk_workspace_bytes', cfg, blob, src, out))
    return out


def vsr_trunk_bf16(cfg, blob, src, out):
    """ConvResidualBlocks on the CB16 window ``src`` (frame block + cin_segs feature windows) into the CB16 window ``out`` — one
    sr_rvsr_trunk_bf16 call: 1 + 2 * num_block sr_conv3x3_bf16 launches, no allocation beyond the grow-only scratch."""
    _arg(cfg.num_feat % 16 == 0, 'vsr_trunk_bf16: windows do not fit the config')     # a valid fp32 config may not be one here
    _launch_arg('sr_rvsr_trunk_bf16', src.device,
                *_vsr_trunk_args('vsr_trunk_bf16', CB16, 16, 'sr_rvsr_trunk_workspace_bytes_bf16', cfg, blob, src, out))
    return out


# ---- the recurrent backward of BasicVSR: the step-input adjoint, the trunk call that keeps its activations and the trunk's
# backward (include/sr_hip_vsr_bwd.h) ----

def _vsr_prop_bwd_desc(who, d, g, prev, flow, dprev, dflow):
    """Checks the operands of the step-input adjoint and fills a struct sr_vsr_prop_bwd_desc from them."""
    _arg(isinstance(g, CB8) and isinstance(prev, CB8) and (prev.n, prev.h, prev.w, prev.cbn) == (g.n, g.h, g.w, g.cbn),
         f'{who}: g and prev must be CB8 windows of one shape')
    n, h, w = g.n, g.h, g.w
    _need_cuda(flow, who)
    _arg(dprev is not None or dflow is not None, f'{who}: nothing to compute')
    for name, t in (('flow', flow), ('dflow', dflow)):
        if t is None:
            continue
        _arg(t.dtype == torch.float32 and tuple(t.shape) == (n, 2, h, w) and t[0].is_contiguous() and t.device == g.device,
             f'{who}: {name} must be an fp32 [{n}, 2, {h}, {w}] view with dense images, got {t.dtype} {tuple(t.shape)}')
        setattr(d, name, t.data_ptr())
        setattr(d, name + '_img_stride', t.stride(0))
    if dprev is not None:
        _arg(isinstance(dprev, CB8) and (dprev.n, dprev.h, dprev.w, dprev.cbn) == (n, h, w, g.cbn), f'{who}: dprev does not fit')
        d.dprev, d.dprev_img_stride = dprev.ptr, dprev.img_stride
    d.g, d.g_img_stride, d.prev, d.prev_img_stride = g.ptr, g.img_stride, prev.ptr, prev.img_stride
    d.n, d.h, d.w, d.fb = n, h, w, g.cbn
    return d


def vsr_prop_input_bwd(g, prev, flow, dprev=None, dflow=None):
    """The adjoint of vsr_prop_input with respect to ``prev`` and ``flow`` — one sr_vsr_prop_input_bwd_f32 launch.  ``g``: CB8
    window, the gradient of warp_out; ``prev``: the CB8 window that was warped; ``flow``: the fp32 [N, 2, H, W] view the forward
    read.  ``dprev``: CB8 window the gradient is ADDED into with float atomics (never zeroed here), or None; ``dflow``: fp32
    [N, 2, H, W] view with dense images the flow gradient is stored into (a float64 gather, bit-reproducible), or None."""
    d = _vsr_prop_bwd_desc('vsr_prop_input_bwd', _lib.VsrPropBwdDesc(), g, prev, flow, dprev, dflow)
    _launch_arg('sr_vsr_prop_input_bwd_f32', g.device, C.byref(d))
    return dprev, dflow


def vsr_prop_input_bwd_det_workspace_bytes(n, h, w, fb):
    """Bytes of the workspace of vsr_prop_input_bwd_det — sr_vsr_prop_input_bwd_det_workspace_bytes."""
    return _lib.load().sr_vsr_prop_input_bwd_det_workspace_bytes(n, h, w, fb)


def vsr_prop_input_bwd_det(g, prev, flow, dprev=None, dflow=None, workspace=None):
    """vsr_prop_input_bwd with a bit-reproducible ``dprev`` (include/sr_hip_vsr_det.h) — one sr_vsr_prop_input_bwd_det_f32 call:
    the terms are summed as 64-bit integers in ``workspace`` (uint8, vsr_prop_input_bwd_det_workspace_bytes; the grow-only scratch
    when None) and added into ``dprev`` with one rounding; ``dflow`` is vsr_prop_input_bwd's bit for bit.  Three launches with
    ``dprev``, one without."""
    who = 'vsr_prop_input_bwd_det'
    dd = _lib.VsrPropBwdDetDesc()
    _vsr_prop_bwd_desc(who, dd.d, g, prev, flow, dprev, dflow)
    if dprev is not None:
        _det_workspace(who, dd, g.device, vsr_prop_input_bwd_det_workspace_bytes(g.n, g.h, g.w, g.cbn), workspace)
    _launch_arg('sr_vsr_prop_input_bwd_det_f32', g.device, C.byref(dd))
    return dprev, dflow


def vsr_trunk_keep_bytes(cfg, n, h, w):
    """Bytes of the activation stack of vsr_trunk_keep — sr_vsr_trunk_keep_bytes."""
    return _lib.load().sr_vsr_trunk_keep_bytes(C.byref(cfg), n, h, w)


def vsr_trunk_keep(cfg, blob, src, out, stack=None):
    """vsr_trunk with every activation its backward reads written to ``stack`` (uint8, sr_vsr_trunk_keep_bytes; allocated when
    None) — one sr_vsr_trunk_keep_f32 call, the launches of vsr_trunk.  Returns (out, stack)."""
    who = 'vsr_trunk_keep'
    _arg(isinstance(src, CB8) and isinstance(out, CB8) and src.cbn == 1 + cfg.cin_segs * cfg.num_feat // 8
         and out.cbn == cfg.num_feat // 8 and (out.n, out.h, out.w) == (src.n, src.h, src.w), f'{who}: windows do not fit the config')
    nbytes = vsr_trunk_keep_bytes(cfg, src.n, src.h, src.w)
    if stack is None:
        stack = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=src.device)
    _arg(stack.dtype == torch.uint8 and stack.numel() >= nbytes and stack.device == src.device, f'{who}: the stack is too small')
    _launch_arg('sr_vsr_trunk_keep_f32', src.device, C.byref(cfg), blob.data_ptr(), src.ptr, src.img_stride, out.ptr, out.img_stride,
                src.n, src.h, src.w, stack.data_ptr(), nbytes)
    return out, stack


def vsr_trunk_stack_views(cfg, stack, n, h, w):
    """The activations of a vsr_trunk_keep stack as CB8 tensors, in the order of the header: the first conv's output, then per
    block the ReLU output and (but for the last block) the block output."""
    one = -(-(4 * n * cfg.num_feat * h * w) // 256) * 256
    return [CB8(stack[i * one:i * one + 4 * n * cfg.num_feat * h * w].view(torch.float32).view(n, cfg.num_feat // 8, h, w, 8))
            for i in range(2 * cfg.num_block)]


def vsr_trunk_pack_dgrad(cfg, params, blob=None):
    """The blob of data-gradient images of a trunk from its parameters in state_dict order — sr_vsr_trunk_pack_dgrad_f32."""
    blob, ptrs = _vsr_trunk_pack_args('vsr_trunk_pack_dgrad', 'sr_vsr_trunk_packed_dgrad_bytes', cfg, params, blob)
    _launch_arg('sr_vsr_trunk_pack_dgrad_f32', blob.device, C.byref(cfg), ptrs, blob.data_ptr())
    return blob


def vsr_trunk_bwd(cfg, dblob, src, out, stack, dout, din, targets, accumulate=False):
    """The adjoint of vsr_trunk_keep — one sr_vsr_trunk_bwd_f32 call.  ``dblob``: vsr_trunk_pack_dgrad of the forward's parameters;
    ``src`` / ``out`` / ``stack``: the forward's input window, output window and stack; ``dout``: CB8 window, the gradient of
    ``out``; ``din``: CB8 window laid out like ``src`` (block 0 receives the frame block's gradient) or None; ``targets``: one
    device pointer (int) or None per parameter in state_dict order — a None target's launch is skipped; a bias target whose
    weight target is None gets a scratch weight target.  ``accumulate``: the gradients are ADDED into the targets."""
    who = 'vsr_trunk_bwd'
    lib = _lib.load()
    fb, nparams = cfg.num_feat // 8, lib.sr_vsr_trunk_num_params(C.byref(cfg))
    _arg(nparams > 0 and len(targets) == nparams, f'{who}: {len(targets)} targets, the config has {nparams} parameters')
    _arg(isinstance(src, CB8) and isinstance(out, CB8) and isinstance(dout, CB8) and src.cbn == 1 + cfg.cin_segs * fb
         and out.cbn == dout.cbn == fb and _same(dout, out) and (out.n, out.h, out.w) == (src.n, src.h, src.w)
         and (din is None or (isinstance(din, CB8) and _same(din, src))), f'{who}: windows do not fit the config')
    n, h, w, dev = src.n, src.h, src.w, src.device
    targets = list(targets)
    for i in range(0, nparams, 2):
        if targets[i] is None and targets[i + 1] is not None:
            nw = cfg.num_feat * (3 + cfg.cin_segs * cfg.num_feat if i == 0 else cfg.num_feat) * 9
            targets[i] = scratch(dev, 4 * nw, 'vsr_trunk_bwd_dw').data_ptr()
    nstack, nws = vsr_trunk_keep_bytes(cfg, n, h, w), lib.sr_vsr_trunk_bwd_workspace_bytes(C.byref(cfg), n, h, w)
    _arg(nstack == 0 or (stack is not None and stack.numel() >= nstack), f'{who}: the stack is too small')
    ws = scratch(dev, nws, who)
    d = _lib.VsrTrunkBwdDesc()
    d.packed_dgrad, d.in_, d.in_img_stride, d.out, d.out_img_stride = dblob.data_ptr(), src.ptr, src.img_stride, out.ptr, out.img_stride
    d.stack, d.stack_bytes = (stack.data_ptr() if nstack else None), nstack
    d.dout, d.dout_img_stride = dout.ptr, dout.img_stride
    if din is not None:
        d.din, d.din_img_stride = din.ptr, din.img_stride
    d.dparams = (C.c_void_p * nparams)(*targets)
    d.accumulate, d.n, d.h, d.w, d.workspace, d.workspace_bytes = int(accumulate), n, h, w, ws.data_ptr(), nws
    _launch_arg('sr_vsr_trunk_bwd_f32', dev, C.byref(cfg), C.byref(d))
    return din


# ---- TOFlow: the 9x9 conv, SPyNetTOF's level input, the aligned stack and the finish (include/sr_hip_tof.h) ----

CONV9X9_SHAPES = ((21, 64), (64, 64))   # (cin, cout) of TOFlow's conv_1 and conv_2


class PackedConv9x9(_PackedConvTaps):
    """MFMA operand image of one 9x9 conv of TOFlow (weights in operand order, then the bias) — sr_tof_conv9x9_pack_f32.
    ``mode`` exists for HipGenerator.packed: only 0 (forward) is served."""
    ksize, modes = 9, ('forward',)

    def _packed_floats(self, lib):
        nfloats = lib.sr_tof_conv9x9_packed_floats(self.cout, self.cin)
        _arg(nfloats > 0, f'conv9x9: (cin, cout) = ({self.cin}, {self.cout}) is not supported; supported: {CONV9X9_SHAPES}')
        return nfloats

    def _pack(self, dev, weight, bias):
        _launch_arg('sr_tof_conv9x9_pack_f32', dev, weight, bias, self.cout, self.cin, self.w.data_ptr())


def conv9x9(src, pc, out=None, *, relu=False):
    """out = [relu](conv9x9(src) + bias) on CB8, stride 1, pad 4 — one sr_tof_conv9x9_f32 launch.  ``pc``: PackedConv9x9; the
    21-channel source is a 3-block window whose channels 21-23 are ignored."""
    _arg(src.cbn == (pc.cin + 7) // 8, f'conv9x9: source has {src.cbn} channel blocks, the weight image needs {(pc.cin + 7) // 8}')
    if out is None:
        out = CB8.empty(src.n, pc.cout, src.h, src.w, src.device)
    _arg((out.n, out.h, out.w) == (src.n, src.h, src.w) and out.cbn >= pc.cout // 8, 'conv9x9: output window does not fit')
    _launch_arg('sr_tof_conv9x9_f32', src.device, C.byref(_conv_taps_desc(_lib.TofConv9x9Desc(), src, pc, out, relu)))
    return out


def _frames(t, what, lead):
    _need_cuda(t, what)
    _arg(t.dim() == len(lead) + 3 and t.is_contiguous() and t.dtype == torch.float32 and t.numel() > 0
         and all(want is None or got == want for got, want in zip(t.shape, lead + (3,))),
         f'{what}: needs a non-empty contiguous fp32 [{", ".join("B" if v is None else str(v) for v in lead)}, 3, H, W] tensor, got '
         f'{t.dtype} {tuple(t.shape)}')
    return t.shape


def tof_level_input(ref, supp, flow_prev=None, *, clip=None, ref_idx=None):
    """(the level's CB8 input block [ref, warp(supp, up, zeros), up], up as a CB8 block) of SPyNetTOF — one
    sr_tof_level_input_f32 launch.  Either ``ref`` and ``supp`` [N, 3, H, W], or ``clip`` [B, 7, 3, H, W] with ``ref_idx``: the
    N = 6 B pairs (frame ref_idx, every other frame in order) of the clips, image n = 6 b + k, read in place.  ``flow_prev``: the
    coarser level's flow (a one-block CB8 window at H / 2 x W / 2), None at the coarsest level."""
    if clip is not None:
        b, _, _, h, w = _frames(clip, 'tof_level_input', (None, 7))
        _arg(ref is None and supp is None and ref_idx in range(7), 'tof_level_input: a clip comes with ref_idx in 0..6 and no ref / supp')
        n, group, skip, stride = 6 * b, 6, ref_idx, 21 * h * w
        ref_ptr, supp_ptr, dev = clip.data_ptr() + ref_idx * 3 * h * w * 4, clip.data_ptr(), clip.device
    else:
        n, _, h, w = _frames(ref, 'tof_level_input', (None,))
        _arg(supp.shape == ref.shape and supp.is_contiguous() and supp.dtype == torch.float32 and supp.device == ref.device,
             'tof_level_input: supp does not fit ref')
        group, skip, stride, ref_ptr, supp_ptr, dev = 1, 1, 3 * h * w, ref.data_ptr(), supp.data_ptr(), ref.device
    _arg(flow_prev is None or (h % 2 == 0 and w % 2 == 0 and flow_prev.cb0 == 0 and tuple(flow_prev.buf.shape) == (n, 1, h // 2, w // 2, 8)),
         f'tof_level_input: flow_prev must be one CB8 block at {h // 2}x{w // 2}')
    out, up = CB8.empty(n, 8, h, w, dev), CB8.empty(n, 8, h, w, dev)
    _launch_arg('sr_tof_level_input_f32', dev, ref_ptr, stride, supp_ptr, stride, group, skip, None if flow_prev is None else flow_prev.ptr,
                out.ptr, up.ptr, n, h, w)
    return out, up


def tof_align(clip, flows, ref_idx, out=None):
    """The 21-channel aligned stack of TOFlow as a 3-block CB8 tensor: frame i of ``clip`` [B, 7, 3, H, W] warped (zeros padding) by
    its flow, frame ``ref_idx`` copied, channels 21-23 zero — one sr_tof_align_f32 launch.  ``flows``: the one-block CB8 buffer
    [6 B, 1, H, W, 8] of the six flows of each clip, image 6 b + k."""
    b, _, _, h, w = _frames(clip, 'tof_align', (None, 7))
    _arg(ref_idx in range(7), f'tof_align: ref_idx {ref_idx} is not one of the 7 frames')
    _arg(isinstance(flows, CB8) and flows.cb0 == 0 and tuple(flows.buf.shape) == (6 * b, 1, h, w, 8) and flows.device == clip.device,
         f'tof_align: flows must be one CB8 block per pair, [{6 * b}, 1, {h}, {w}, 8]')
    if out is None:
        out = CB8.empty(b, 24, h, w, clip.device)
    _arg((out.n, out.cbn, out.h, out.w) == (b, 3, h, w), 'tof_align: output window does not fit')
    _launch_arg('sr_tof_align_f32', clip.device, clip.data_ptr(), flows.ptr, flows.img_stride, out.ptr, out.img_stride, b, ref_idx, h, w)
    return out


def tof_finish(y, clip, ref_idx, mean, std, out=None):
    """(y + clip[:, ref_idx]) * std[c] + mean[c] as an NCHW tensor [B, 3, H, W]: ``y`` the one-block CB8 output of conv_4, ``clip``
    the normalised [B, 7, 3, H, W] frames — one sr_tof_finish_f32 launch."""
    b, t, _, h, w = _frames(clip, 'tof_finish', (None, None))
    _arg(0 <= ref_idx < t, f'tof_finish: ref_idx {ref_idx} is not one of the {t} frames')
    _arg(isinstance(y, CB8) and (y.n, y.h, y.w) == (b, h, w) and y.cbn >= 1 and y.device == clip.device, 'tof_finish: y does not fit the clip')
    f3 = [(C.c_float * 3)(*[float(v) for v in vals]) for vals in (mean, std)]
    if out is None:
        out = torch.empty((b, 3, h, w), dtype=torch.float32, device=clip.device)
    _arg(tuple(out.shape) == (b, 3, h, w) and out.is_contiguous() and out.dtype == torch.float32, 'tof_finish: output does not fit')
    _launch_arg('sr_tof_finish_f32', clip.device, y.ptr, y.img_stride, clip.data_ptr() + ref_idx * 3 * h * w * 4, t * 3 * h * w,
                out.data_ptr(), b, h, w, f3[0], f3[1])
    return out


# ---- DUF: 3D convolutions on frame-major CB8 clips, the 1x1x1 conv, the dynamic-filter tail (include/sr_hip_duf.h) ----

DUF_CONV3D_COUTS = (16, 32, 64, 256)


class ClipCB8:
    """A frame-major channel-blocked clip: storage ``buf`` [B, T, C/8, H, W, 8] fp32 plus a frame window [t0, t0 + tn).  Frame t
    of clip i is a CB8 image; a dense concatenation is one such buffer at its final channel count."""

    def __init__(self, buf, t0=0, tn=None):
        assert buf.dim() == 6 and buf.size(5) == 8 and buf.dtype == torch.float32 and buf.is_contiguous()
        self.buf, self.t0 = buf, t0
        self.tn = buf.size(1) - t0 if tn is None else tn
        assert 0 <= t0 and self.tn > 0 and t0 + self.tn <= buf.size(1)

    @classmethod
    def empty(cls, b, t, channels, h, w, device):
        return cls(torch.empty((b, t, (channels + 7) // 8, h, w, 8), dtype=torch.float32, device=device))

    b = property(lambda s: s.buf.size(0))
    cbn = property(lambda s: s.buf.size(2))
    h = property(lambda s: s.buf.size(3))
    w = property(lambda s: s.buf.size(4))
    device = property(lambda s: s.buf.device)
    frame_stride = property(lambda s: s.buf.size(2) * s.buf.size(3) * s.buf.size(4) * 8)
    clip_stride = property(lambda s: s.buf.size(1) * s.frame_stride)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.t0 * self.frame_stride * 4

    def frames(self, t0, tn):
        """The window of frames [t0, t0 + tn) of this window."""
        return ClipCB8(self.buf, self.t0 + t0, tn)

    def images(self):
        """The clips of a one-frame window as a plain CB8 batch (a view; needs T == 1 in storage)."""
        assert self.buf.size(1) == 1
        return CB8(self.buf.view(self.b, self.cbn, self.h, self.w, 8))


class PackedDufConv:
    """MFMA operand image (weights in operand order, then the bias) of one DUF convolution: an OIDHW weight [cout, cin, kt, 3, 3]
    -> sr_duf_conv3d_pack_f32, [c, c, 1, 1, 1] -> sr_duf_pw_pack_f32."""

    def __init__(self, weight, bias=None):
        _need_cuda(weight, 'PackedDufConv')
        _arg(weight.dim() == 5 and weight.dtype == torch.float32 and tuple(weight.shape[3:]) in ((3, 3), (1, 1)),
             f'PackedDufConv: needs an fp32 [cout, cin, kt, 3, 3] or [c, c, 1, 1, 1] weight, got {weight.dtype} {tuple(weight.shape)}')
        _arg(bias is None or (bias.dtype == torch.float32 and tuple(bias.shape) == (weight.size(0),)), 'PackedDufConv: bias does not fit')
        weight = weight.detach().contiguous()
        bias = None if bias is None else bias.detach().contiguous()
        self.cout, self.cin, self.kt = weight.shape[:3]
        self.pw = weight.size(3) == 1
        lib = _lib.load()
        if self.pw:
            _arg(self.kt == 1 and self.cout == self.cin, f'PackedDufConv: a 1x1x1 weight must be [c, c, 1, 1, 1], got {tuple(weight.shape)}')
            nfloats = lib.sr_duf_pw_packed_floats(self.cout)
            _arg(nfloats > 0, f'duf_pw: c = {self.cout} is not supported; supported: a multiple of 8 up to 432')
            self.w = torch.empty(nfloats, dtype=torch.float32, device=weight.device)
            _launch_arg('sr_duf_pw_pack_f32', weight.device, weight.data_ptr(), _p(bias), self.cout, self.w.data_ptr())
        else:
            nfloats = lib.sr_duf_conv3d_packed_floats(self.cout, self.cin, self.kt)
            _arg(nfloats > 0, f'duf_conv3d: (cin, cout, kt) = ({self.cin}, {self.cout}, {self.kt}) is not supported; supported: cin 3 or a '
                 f'multiple of 8 up to 448, cout in {DUF_CONV3D_COUTS}, kt 1 or 3')
            self.w = torch.empty(nfloats, dtype=torch.float32, device=weight.device)
            _launch_arg('sr_duf_conv3d_pack_f32', weight.device, weight.data_ptr(), _p(bias), self.cout, self.cin, self.kt, self.w.data_ptr())


def _duf_conv_desc(who, src, pc, dst, out_cb0, pad_t, relu, prologue):
    _arg(isinstance(src, ClipCB8) and isinstance(dst, ClipCB8), f'{who}: source and destination must be ClipCB8 windows')
    cinb = (pc.cin + 7) // 8
    tout = src.tn - 2 * (1 - pad_t) if pc.kt == 3 else src.tn
    _arg(src.cbn >= cinb, f'{who}: the source has too few channel blocks')
    _arg((dst.b, dst.h, dst.w) == (src.b, src.h, src.w) and dst.tn == tout and dst.device == src.device
         and out_cb0 >= 0 and dst.cbn >= out_cb0 + pc.cout // 8, f'{who}: the destination window does not fit')
    d = _lib.DufConvDesc()
    d.in_, d.in_frame_stride, d.in_clip_stride = src.ptr, src.frame_stride, src.clip_stride
    d.cin, d.cout, d.kt, d.pad_t, d.b, d.t, d.h, d.w = pc.cin, pc.cout, pc.kt, pad_t, src.b, src.tn, src.h, src.w
    d.packed, d.out, d.out_frame_stride, d.out_clip_stride = pc.w.data_ptr(), dst.ptr, dst.frame_stride, dst.clip_stride
    d.out_cb0, d.relu = out_cb0, int(bool(relu))
    if prologue is not None:
        scale, shift = prologue
        _arg(all(t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (pc.cin,) and t.device == src.device
                 for t in (scale, shift)), f'{who}: the prologue needs two fp32 [{pc.cin}] arrays on the device of the source')
        d.scale, d.shift = scale.data_ptr(), shift.data_ptr()
    return d


def duf_conv3d(src, pc, dst, out_cb0=0, *, pad_t=0, relu=False, prologue=None):
    """nn.Conv3d(cin, cout, (kt, 3, 3), 1, (pad_t, 1, 1)) [+ ReLU] from the channel prefix of the frames of ``src`` into channel
    block ``out_cb0`` onward of the frames of ``dst`` (ClipCB8 windows; dst has src.tn - 2 frames for kt = 3 without temporal
    padding) — one sr_duf_conv3d_f32 launch.  ``prologue``: (scale, shift), the operand becomes max(x * scale + shift, 0)."""
    _arg(not pc.pw, 'duf_conv3d: the weight image is a 1x1x1 one')
    d = _duf_conv_desc('duf_conv3d', src, pc, dst, out_cb0, pad_t, relu, prologue)
    _launch_arg('sr_duf_conv3d_f32', src.device, C.byref(d))
    return dst


def duf_pw(src, pc, dst, out_cb0=0, *, relu=False, prologue=None):
    """nn.Conv3d(c, c, 1) [+ ReLU] with the same optional prologue — one sr_duf_pw_f32 launch."""
    _arg(pc.pw, 'duf_pw: the weight image is not a 1x1x1 one')
    d = _duf_conv_desc('duf_pw', src, pc, dst, out_cb0, 0, relu, prologue)
    _launch_arg('sr_duf_pw_f32', src.device, C.byref(d))
    return dst


def duf_filter(logits, centre, scale, res=None, *, softmax=True, shuffle=True):
    """The tail of DUF: [softmax over the 25 taps of] ``logits`` (CB8, 25 s^2 channels, channel = tap * s^2 + sub) applied as a
    5x5 filter to ``centre`` ([N, 3, H, W] fp32, a view whose images are contiguous: the centre frames of the clip, read in
    place), plus ``res`` (CB8, 3 s^2 channels), pixel-shuffled to [N, 3, s H, s W] — or [N, 3 s^2, H, W] without ``shuffle`` —
    one sr_duf_filter_f32 launch."""
    _need_cuda(centre, 'duf_filter')
    n, h, w = logits.n, logits.h, logits.w
    s2 = scale * scale
    _arg(scale in (2, 3, 4), f'duf_filter: scale {scale} is not supported; supported: 2, 3, 4')
    _arg(isinstance(logits, CB8) and logits.cbn >= (25 * s2 + 7) // 8, f'duf_filter: logits need {25 * s2} channels')
    _arg(centre.dtype == torch.float32 and tuple(centre.shape) == (n, 3, h, w) and tuple(centre.stride()[1:]) == (h * w, w, 1)
         and centre.device == logits.device, f'duf_filter: centre must be fp32 [{n}, 3, {h}, {w}] with contiguous images')
    _arg(res is None or (isinstance(res, CB8) and (res.n, res.h, res.w) == (n, h, w) and res.cbn >= (3 * s2 + 7) // 8),
         'duf_filter: res does not fit')
    shape = (n, 3, scale * h, scale * w) if shuffle else (n, 3 * s2, h, w)
    out = torch.empty(shape, dtype=torch.float32, device=logits.device)
    _launch_arg('sr_duf_filter_f32', logits.device, logits.ptr, logits.img_stride, None if res is None else res.ptr,
                0 if res is None else res.img_stride, centre.data_ptr(), centre.stride(0) if n > 1 else 3 * h * w, out.data_ptr(), n,
                scale, h, w, int(bool(softmax)), int(bool(shuffle)))
    return out
