"""What the per-layer HIP generators (MSRResNet, EDSR, RCAN, RIDNet, SpyNet, TOFlow, DUF) share: the forward dispatch and ONE
cache of everything a net derives from its tensors (``HipGenerator.derived``: weight images, BatchNorm folds and prologues, the
host copy of ``mean`` / ``std``; the eval-mode BatchNorm arithmetic itself is arch_util.fold_batchnorm / bn_prologue), the
fp32 / bf16 ops table one layer list is written against (``F32``, ``BF16``) with the residual block and upsampling stage the
networks have in common, and the autograd scaffold (``WholeNetFunction``, ``GradRouter``).

A network built on this writes its parameters, ``run_forward(x, keep, ops)`` and the ``run_backward`` of its Function.  RRDBNet
and the discriminators (whole-network C entry points) have their own base, hip_driver.py; GFPGANv1OCR (one Python-built pack for
the net) uses neither.
"""
from types import SimpleNamespace

import torch
from torch import nn

from .. import _lib, hip_ops

# The per-dtype launches a layer list is written against; ``bf16`` is handed on to packed() and hip_ops.edsr_shift_in.
# The functions are bound here, at import: a wrapper put on hip_ops.conv3x3 later reaches the backward and packed(), which look
# hip_ops up per call, but not the three forwards; wrap F32.conv3x3 / BF16.conv3x3 as well.
F32 = SimpleNamespace(conv3x3=hip_ops.conv3x3, pixel_shuffle=hip_ops.pixel_shuffle, to_cb=hip_ops.nchw_to_cb8, bf16=False)
BF16 = SimpleNamespace(conv3x3=hip_ops.conv3x3_bf16, pixel_shuffle=hip_ops.pixel_shuffle_bf16, to_cb=hip_ops.nchw_to_cb16,
                       bf16=True)


class HipGenerator(nn.Module):
    """Base of the generators that are a composition of per-layer launches.  A subclass provides ``_in_channels``,
    ``_autograd_apply(x)`` (its whole-network Function), ``run_forward(x, keep=False[, ops=F32])`` -> (y, saved) and, where it
    has a bf16 forward, ``compute_dtype``."""

    compute_dtype = 'fp32'

    def __init__(self):
        super().__init__()
        self._packs = {}
        self._pack_gen = 0
        self._grad_sink = None  # set by optim.FlatAdam: weight gradients are added straight into its arena

    def _param_list(self):
        """Parameters in state_dict (= named_parameters) order."""
        return list(self.parameters())

    def invalidate_packed(self):
        """Call after parameter memory was written behind torch's version counters (fused Adam, EMA, a broadcast)."""
        self._pack_gen += 1

    def derived(self, key, tensors, extra, build):
        """``build()``, cached in ``_packs`` under ``key``: a weight image, a BatchNorm fold, host floats — anything made from
        ``tensors``.  Rebuilt when the storage, the version or the FlatAdam epoch (``_sr_epoch``: a write behind torch's version
        counter) of one of them, ``extra`` (a scalar the result depends on, e.g. a BatchNorm eps) or this net's generation
        (invalidate_packed) changed; ``_apply`` empties the cache.  Refuses tensors that are not fp32."""
        sig = tuple((t.data_ptr(), t._version, getattr(t, '_sr_epoch', (0,))[0]) for t in tensors) + (extra, self._pack_gen)
        hit = self._packs.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1]
        if any(t.dtype != torch.float32 for t in tensors):
            raise _lib.SrHipError(f'{type(self).__name__} parameters must be fp32')
        val = build()
        self._packs[key] = (sig, val)
        return val

    def packed(self, conv, mode=0, bf16=False):
        """Weight image of ``conv`` (mode 0: forward, 1: data gradient; bf16: the CB16 image rounded from the fp32 parameter):
        sr_conv3x3_pack_f32 for 3x3 convs (every dilation), sr_conv7x7_pack_f32 / sr_conv7x7_dgrad_pack_f32 for SpyNet's 7x7 convs,
        sr_tof_conv9x9_pack_f32 for TOFlow's 9x9 convs, sr_convk_pack_f32 for any other kernel size; cached by ``derived``.
        Not hip_ops.cached_pack: that cache is keyed on the process-global epoch, so one net's invalidate_packed() would repack
        every other network's images (the discriminator's after each generator step)."""
        w, b = conv.weight, conv.bias
        cls = hip_ops.PackedConvBF16 if bf16 else hip_ops.PackedConv if w.shape[2] == 3 else \
            hip_ops.PackedConv7x7 if w.shape[2] == 7 else hip_ops.PackedConv9x9 if w.shape[2] == 9 else hip_ops.PackedConvK
        return self.derived((id(conv), mode, bf16), (w, b), None, lambda: cls(w, b if mode == 0 else None, mode=mode))

    def _norm_host(self):
        """The ``mean`` and ``std`` buffers of a network that has them as host floats, read back once per value of the buffers."""
        return self.derived('norm', (self.mean, self.std), None, lambda: (self.mean.flatten().tolist(), self.std.flatten().tolist()))

    def _drop_device_caches(self):
        """Whatever else a subclass keeps per device; cleared with the weight images when the module is moved or cast."""

    def _apply(self, fn, *args, **kwargs):
        self._packs = {}
        self._drop_device_caches()
        return super()._apply(fn, *args, **kwargs)

    def _check_input(self, x):
        """A subclass's own refusals of an input of the right shape."""

    def forward(self, x):
        if not x.is_cuda:
            raise _lib.SrHipError(f'{type(self).__name__}.forward runs only on a HIP device (no CPU fallback): move the module '
                                  'and input with .to("cuda")')
        if x.dim() != 4 or x.size(1) != self._in_channels:
            raise ValueError(f'expected [N, {self._in_channels}, H, W], got {tuple(x.shape)}')
        self._check_input(x)
        x = x.contiguous().float()
        needs_graph = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self._param_list()))
        if self.compute_dtype == 'bf16':
            if needs_graph and self.training:
                raise NotImplementedError(f"{type(self).__name__} with compute_dtype='bf16' is forward only (eval mode or "
                                          "torch.no_grad()); train with compute_dtype='fp32'")
            return self.run_forward(x, ops=BF16)[0]
        if needs_graph:
            return self._autograd_apply(x)
        return self.run_forward(x)[0]


def residual_block(net, feat, blk, ops):
    """One ResidualBlockNoBN: conv1 with ReLU (act_slope 0), conv2 with the residual x + res_scale*conv in the epilogue.
    Returns (the ReLU output, the block output).  One block, not the loop: the caller's loop variable is then the only
    reference to the block's input, as it must be for the input to be freed when the next block has read it."""
    t = ops.conv3x3(feat, net.packed(blk.conv1, 0, ops.bf16), act_slope=0.0)
    return t, ops.conv3x3(t, net.packed(blk.conv2, 0, ops.bf16), alpha=float(blk.res_scale), res1=feat, beta1=1.0)


def upsample_stage(net, feat, conv, r, ops, act_slope=1.0):
    """One upsampling stage: the conv (with LeakyReLU(act_slope), which commutes with the shuffle), then the pixel shuffle; the
    unshuffled conv output is freed on return.  One stage, not the loop, for the reason given at residual_block."""
    u = ops.conv3x3(feat, net.packed(conv, 0, ops.bf16), act_slope=act_slope)
    return ops.pixel_shuffle(u, net.num_feat, r)


def residual_block_backward(net, sv, b, g, router, **extra):
    """Adjoint of block ``b`` of residual_block, f' = f + rs*conv2(relu(conv1(f))): ``g`` = dL/df' -> dL/df.  ``extra``: further
    epilogue terms of the conv1 data gradient (block 0, where the body input's other consumers and its activation are folded
    in)."""
    blk = net.body[b]
    t, _ = sv['blocks'][b]
    f_in = sv['blocks'][b - 1][1] if b > 0 else sv['feat0']
    rs = float(blk.res_scale)
    router.wgrad(blk.conv2, t, g, scale=rs)
    dt = hip_ops.conv3x3(g, net.packed(blk.conv2, 1), alpha=rs, mask=t, mask_slope=0.0)   # d(conv1 pre-act)
    router.wgrad(blk.conv1, f_in, dt)
    # d(block input) = conv1 data gradient + the identity path (res1)
    return hip_ops.conv3x3(dt, net.packed(blk.conv1, 1), res1=g, beta1=1.0, **extra)


class GradRouter:
    """Where the parameter gradients of one backward go: into the tuple returned to autograd (``grads``, None for a frozen
    parameter), or, with an optim.FlatAdam arena attached (``net._grad_sink``), added straight into the arena.  A parameter that
    several launches of one backward contribute to (a head run in chunks, a trunk shared by the steps of a recurrent branch) is
    stored by the first of them and ADDED into by the later ones, in call order, by the kernels' accumulate mode: ``wgrad`` does so
    by itself, whole-call targets through ``shared_targets``."""

    def __init__(self, net, params, need_p):
        self.need_p = need_p
        self.grads = [None] * len(params)
        self.index = {id(p): i for i, p in enumerate(params)}
        self.sink = getattr(net, '_grad_sink', None)
        self.to_sink = self.sink is not None and any(need_p)
        if self.to_sink and not all(need_p):
            raise _lib.SrHipError('flat-arena mode needs every generator parameter to require grad')
        self._first = {}     # index of a conv's weight -> what its first wgrad call returned
        self._shared = {}    # id of the first parameter of a shared_targets call -> its pointers

    def wgrad(self, conv, src, d, scale=1.0, dilation=None):
        """weight / bias gradient of ``conv`` from its source and its pre-activation output gradient: the dense 3x3 path of
        sr_conv3x3_wgrad_f32, sr_conv7x7_wgrad_f32 for SpyNet's 7x7 convs, or sr_convd_wgrad_f32 for a dilated or 1x1 conv.  No
        launch when neither is wanted."""
        iw, ib = self.index[id(conv.weight)], self.index[id(conv.bias)]
        if not (self.to_sink or self.need_p[iw] or self.need_p[ib]):
            return
        out = (self.sink.grad_ptrs[iw], self.sink.grad_ptrs[ib]) if self.to_sink else None   # arena: added in place
        first = None if self.to_sink else self._first.get(iw)
        if first is not None:                                  # a later launch of the same conv adds into the first one's tensors
            out = (first[0].data_ptr(), first[1].data_ptr())
        k = conv.weight.shape[2]
        if dilation is None and k == 3:
            res = hip_ops.conv3x3_wgrad(src, d, conv.out_channels, conv.in_channels, scale=scale, out=out)
        elif dilation is None and k == 7:
            res = hip_ops.conv7x7_wgrad(src, d, conv.out_channels, conv.in_channels, scale=scale, out=out)
        else:
            res = hip_ops.convd_wgrad(src, d, conv.out_channels, conv.in_channels, k, dilation or 1, scale=scale, out=out)
        if not self.to_sink and first is None:
            self._first[iw] = res
            self.grads[iw] = res[0] if self.need_p[iw] else None
            self.grads[ib] = res[1] if self.need_p[ib] else None

    def shared_targets(self, params):
        """``targets`` for parameters that several calls of one backward write: the first call gets fresh tensors to store into,
        every later call the same pointers with accumulate set."""
        key = id(params[0])
        if not self.to_sink and key in self._shared:
            return self._shared[key], True
        ptrs, accumulate = self.targets(params)
        self._shared[key] = ptrs
        return ptrs, accumulate

    def targets(self, params):
        """Device pointers (or None) the gradients of ``params`` go to, and whether they accumulate (arena)."""
        idx = [self.index[id(p)] for p in params]
        if self.to_sink:
            return tuple(self.sink.grad_ptrs[i] for i in idx), True
        out = []
        for p, i in zip(params, idx):
            if self.need_p[i]:
                self.grads[i] = torch.empty_like(p)
                out.append(self.grads[i].data_ptr())
            else:
                out.append(None)
        return tuple(out), False


class WholeNetFunction(torch.autograd.Function):
    """ONE autograd Function for a whole HipGenerator: forward keeps what ``net.run_forward(x, keep=True)`` saved; a subclass
    writes the network's adjoint, ``run_backward(net, saved, dy, router, need_x)`` -> dx (or None), issuing per layer the
    weight gradient through ``router`` and then the data gradient."""

    @staticmethod
    def forward(ctx, net, x, *params):
        y, saved = net.run_forward(x, keep=True)
        ctx.net, ctx.saved, ctx.params = net, saved, params
        return y

    @classmethod   # not the usual staticmethod: it has to reach the subclass's run_backward, and autograd calls it on that class
    def backward(cls, ctx, dy):
        dy = dy.contiguous().float()
        router = GradRouter(ctx.net, ctx.params, ctx.needs_input_grad[2:])
        with torch.cuda.device(dy.device):
            dx = cls.run_backward(ctx.net, ctx.saved, dy, router, ctx.needs_input_grad[1])
        ctx.saved = None
        return (None, dx) + tuple(router.grads)

    @classmethod
    def net_apply(cls, net, x):
        """The module-level ``<net>_apply(net, x)`` of each autograd file."""
        return cls.apply(net, x, *net._param_list())
