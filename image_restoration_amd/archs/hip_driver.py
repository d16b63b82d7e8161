"""What the whole-network drivers (RRDBNet, VGGStyleDiscriminator128/256, UNetDiscriminatorSN) share: one C entry point per
pass, so what is left to Python is the weights' identity, the cache of packed weight images, the scratch buffers, the entry
point of a dtype and where a backward writes the parameter gradients.  The counterpart of hip_generator.py, whose networks
are compositions of per-layer launches.

A network built on this writes its parameters, ``_cfg()``, ``_param_ends()``, the ``_blob`` call of each image it packs and
the autograd Function around its forward and backward entry points.
"""
import ctypes as C
import os

import torch
from torch import nn

from .. import _lib, hip_ops

_DEBUG_PARAM_LIST = os.environ.get('SR_DEBUG_PACKS') == '1'


def symbol(lib, stem, bf16, query=False, short=False):
    """(entry point, the name error texts use for it) of ``stem`` for a dtype.  Launches are sr_x_f32 / sr_x_bf16, size queries
    (``query``) sr_x / sr_x_bf16; ``short``: the text names the bare stem, as the discriminator drivers and the data-gradient
    pack always have."""
    name = stem + ('_bf16' if bf16 else '' if query else '_f32')
    return getattr(lib, name), stem if short else name


def device_input(x, who):
    """The refusal of a CPU input and the dense fp32 copy every driver Function starts with."""
    if not x.is_cuda:
        raise _lib.SrHipError(f'{who} runs only on a HIP device (no CPU fallback)')
    return x.contiguous().float()


def grow_workspace(net, tag, nbytes, dev):
    """Grow-only scratch ``net._grown[tag]``: kept while it is large enough and on ``dev``."""
    ws = net._grown.get(tag)
    if ws is None or ws.numel() < nbytes or ws.device != dev:
        ws = net._grown[tag] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def grad_targets(items, need_p, sink, refusal, pairs=False, dev=None):
    """Where one whole-network backward writes its parameter gradients -> (what autograd gets back, the C pointer array or
    None, ``accumulate``).  ``items``: the parameters, or their shapes with ``dev`` (the U-Net's weights are temporaries).
    ``sink``: the optim.FlatAdam arena (``net._grad_sink``) or None; with one the gradients are ADDED straight into the arena
    that is all-reduced and consumed by the fused Adam kernel, and autograd sees none.  Some but not all of ``need_p`` is
    refused with ``refusal``, except (``pairs``, RRDBNet without an arena) that weight and bias of one conv may be frozen
    together: a conv is skipped only when its weight needs no gradient; that route hands C an array even when it is all NULL."""
    n = len(items)
    wanted = any(need_p)
    if wanted and not all(need_p) and (sink is not None or not pairs):
        raise _lib.SrHipError(refusal)
    if wanted and sink is not None:
        return [None] * n, (C.c_void_p * n)(*sink.grad_ptrs), 1
    if not (wanted or pairs):
        return [None] * n, None, 0
    if dev is None:
        grads = [torch.empty_like(p) if need else None for p, need in zip(items, need_p)]
    else:
        grads = [torch.empty(s, dtype=torch.float32, device=dev) if need else None for s, need in zip(items, need_p)]
    ptrs = (C.c_void_p * n)(*[g.data_ptr() if g is not None else None for g in grads])
    if pairs:
        for i in range(0, n, 2):
            if grads[i] is None and grads[i + 1] is not None:
                raise _lib.SrHipError('bias.requires_grad without weight.requires_grad is not supported')
    return grads, ptrs, 0


class HipDriverNet(nn.Module):
    """Base of the networks whose long-lived parameters are packed into device blobs for whole-network entry points.  A
    subclass states ``_num_params`` (the sr_*_num_params query), ``_params_name`` (how the parameter refusal calls them) and
    ``_param_ends()``."""

    _num_params = _params_name = None

    def __init__(self):
        super().__init__()
        self._plist = None       # the cached parameter walk
        self._blobs = {}         # kind, e.g. ('fwd', bf16) -> (weights key, device blob of weight images)
        self._pack_epoch = 0
        self._grown = {}         # grow_workspace
        self._grad_sink = None   # set by optim.FlatAdam: gradients accumulate straight into its arena

    def invalidate_packed(self):
        """Call after parameter memory was written behind torch's version counters (fused Adam / EMA kernels write the arena
        through raw pointers)."""
        self._pack_epoch += 1

    def _param_ends(self):
        """(first, last) parameter of the network: what the cached walk is revalidated by."""
        raise NotImplementedError

    def _param_list(self):
        """Parameters in state_dict order (what the pack entry points expect).  The walk over the module tree (RRDBNet: 702
        parameters, twice per training step, 2.6 ms of host time) is cached; the cache is dropped when the first or the last
        parameter object is no longer the module's (``load_state_dict(assign=True)``, a re-registered parameter) and by
        ``_apply`` (``.to()``, ``.cuda()``)."""
        cached = self._plist
        if cached is not None:
            first, last = self._param_ends()
            if cached[0] is first and cached[-1] is last:
                if _DEBUG_PARAM_LIST:   # SR_DEBUG_PACKS=1: the full walk every time, and say so if the shortcut would have lied
                    fresh = [p for _, p in self.named_parameters()]
                    assert len(fresh) == len(cached) and all(a is b for a, b in zip(fresh, cached)), \
                        'a parameter in the middle of the network was re-registered: call net._apply(lambda t: t) or invalidate the list'
                return cached
        self._drop_device_caches()
        self._plist = [p for _, p in self.named_parameters()]
        return self._plist

    def _drop_device_caches(self):
        """Whatever else a subclass derives from the walk; dropped with it."""

    def _apply(self, fn, *args, **kwargs):
        self._plist = None
        self._drop_device_caches()
        return super()._apply(fn, *args, **kwargs)

    def _weights_key(self, stride=1):
        """Identity of the current weights: parameter storage + torch version counters + the epochs of writers torch cannot
        see (FlatAdam's fused step, invalidate_packed, hip_ops.invalidate_packs).  ``stride`` 2: of the conv weights alone."""
        params = self._param_list()
        return (self._pack_epoch, hip_ops._pack_epoch[0], getattr(params[0], '_sr_epoch', (0,))[0],
                tuple((p.data_ptr(), p._version) for p in (params if stride == 1 else params[0::stride])))

    def _blob(self, kind, lib, cfg, stream, size_stem, pack_stem, stride=1, count=True, layout=True, short=False):
        """The device blob ``kind`` = (what, bf16) of weight images, packed again when ``_weights_key(stride)`` moved; the old
        allocation is kept when size and device still fit.  ``count`` / ``layout``: the parameter checks this image has
        always had."""
        key = self._weights_key(stride)
        hit = self._blobs.get(kind)
        if hit is not None and hit[0] == key:
            return hit[1]
        params = self._param_list()
        if count:
            n = getattr(lib, self._num_params)(C.byref(cfg))
            if n != len(params):
                raise _lib.SrHipError(f'parameter count {len(params)} != {n} expected by libsr_hip.so')
        dev = params[0].device
        if layout:
            for p in params:
                if p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                    raise _lib.SrHipError(f'{self._params_name} parameters must be contiguous fp32 on one HIP device')
        nbytes = symbol(lib, size_stem, kind[1], query=True)[0](C.byref(cfg))
        blob = hit[1] if hit is not None and hit[1].numel() == nbytes and hit[1].device == dev else \
            torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ptrs = (C.c_void_p * len(params))(*[p.data_ptr() for p in params])
        pack, name = symbol(lib, pack_stem, kind[1], short=short)
        _lib.check(pack(C.byref(cfg), ptrs, blob.data_ptr(), stream), name)
        self._blobs[kind] = (key, blob)
        return blob
