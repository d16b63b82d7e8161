"""Flat-arena Adam: the optimiser / gradient-exchange side of the MI355X training path.

All parameters of a network live in ONE contiguous fp32 arena and their gradients in another
(``param.data`` / ``param.grad`` are views).  Consequences:

* the generator's backward writes weight gradients straight into the gradient arena
  (``net._grad_sink``, sr_rrdbnet_backward_f32 accumulate=1) — no per-parameter tensors;
* data-parallel exchange is ONE RCCL all-reduce of the arena (66.8 MB for the 23-block generator)
  instead of DDP's per-bucket traffic — sized for point-to-point xGMI links, where few large
  ring steps beat many small ones;
* the update is one fused kernel (sr_adam_step_f32) with torch.optim.Adam semantics
  (reference: base_model.py:78-83, lr 1e-4, betas (0.9, 0.99) from train_ESRGAN_x4.yml:64-73),
  the 1/world_size of DDP's gradient mean folded in as ``grad_scale``.

Parameter groups, frozen parameters and per-parameter step counts (the EDVR recipe: edvr_model.py:20-67) go through
sr_adam_step_groups_f32, still one launch over the arena: every 64-float chunk carries a class (group, step count) or is
inactive.  One group with every parameter taking part and all step counts equal stays on sr_adam_step_f32.

state_dict()/load_state_dict() use torch.optim.Adam's format, so ``*.state`` files written by the
reference (base_model.py:279-311) resume here and vice versa.
"""
import collections
import ctypes as C

import torch

from . import _lib

_ALIGN = 64  # floats
MAX_CLASSES = 16  # SR_ADAM_MAX_CLASSES


class _GradSink:
    def __init__(self, ptrs):
        self.grad_ptrs = ptrs


def partition_classes(group_of, steps, active):
    """The class scheme of sr_adam_step_groups_f32, on the host alone.  ``group_of[i]``, ``steps[i]`` (steps taken so far) and
    ``active[i]`` describe parameter i.  Parameters that take part share a class when they share group and step count; all
    others fall into one inactive class.  Returns (class id per parameter, [(group, steps so far, active)] per class); ids are
    numbered by first appearance, so they do not change while the same parameters keep stepping together."""
    ids, seen = [], {}
    for g, s, a in zip(group_of, steps, active):
        key = (g, s) if a else None
        if key not in seen:
            seen[key] = len(seen)
        ids.append(seen[key])
    classes = [(key[0], key[1], True) if key is not None else (None, 0, False) for key in seen]
    return ids, classes


class FlatAdam:
    """torch.optim.Adam (amsgrad False) over one arena.

    ``params`` is a flat list of parameters or torch's list of group dicts (``[{'params': [...], 'lr': ...}, ...]``; a group's
    ``lr`` overrides the default).  The arena holds the parameters in group order.  betas, eps and weight_decay are one set
    for the whole optimiser.

    Which parameters a step updates.  A parameter takes part in ``step()`` if and only if its ``requires_grad`` is true at
    that call; its own step count (bias correction) advances only then, and a parameter that never took part has no entry in
    ``state_dict()``.  torch.optim.Adam instead skips a parameter whose ``.grad`` is None.  The two rules agree for the
    schedule this exists for (EDVRModel: the optimiser is built while everything is trainable, parameters are frozen before
    they have received any gradient, and un-frozen once): there a parameter has ``requires_grad`` false exactly while torch's
    ``.grad`` would still be None.  They differ when a parameter is frozen AFTER it has trained: torch, under
    ``zero_grad(set_to_none=False)``, keeps stepping it on a zero gradient (its moments decay and keep moving it), here it
    stands still.  Gradients live in the arena and are zeroed, never None, so the rule cannot be restated on ``.grad``."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, modules=()):
        params = list(params)
        if not params:
            raise ValueError('optimizer got an empty parameter list')
        groups = [dict(g) for g in params] if isinstance(params[0], dict) else [dict(params=params)]
        self.params, self.group_of = [], []
        self.param_groups = []
        for gi, g in enumerate(groups):
            members = list(g.pop('params'))
            if not members:
                raise ValueError(f'optimizer got an empty parameter group ({gi})')
            unknown = set(g) - {'lr'}
            if unknown:
                raise ValueError(f'FlatAdam groups override lr only, not {sorted(unknown)}')
            self.params += members
            self.group_of += [gi] * len(members)
            self.param_groups.append(dict(params=members, lr=g.get('lr', lr), betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                          amsgrad=False))
        if len({id(p) for p in self.params}) != len(self.params):
            raise ValueError('some parameters appear in more than one parameter group')
        dev = self.params[0].device
        for p in self.params:
            if p.device != dev or p.dtype != torch.float32:
                raise ValueError('FlatAdam needs fp32 parameters on one device')
        self.device = dev
        self.offsets = []
        off = 0
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.numel = off
        self._epoch = [0]
        self.flat_p = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(off, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(off, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(off, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                view = self.flat_p[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p.grad = self.flat_g[o:o + p.numel()].view(p.shape)
                p._sr_epoch = self._epoch   # hip_ops.cached_pack: this optimiser rewrites the parameter behind torch's version counter
        self.steps = [0] * len(self.params)   # per parameter: the steps it took part in
        # who took part in the latest steps (newest last), for take_back_skipped: None = everybody
        self._took_part = collections.deque(maxlen=1024)
        self._class_ids = None          # class id per parameter the device array below was written for
        self.class_of_chunk = None      # uint8 [numel / 64] on the device, rewritten only when the partition changes
        self.partition_writes = 0
        # steps the fused kernel refused on the device because a launch behind their gradients had timed out (sr_abort_latch):
        # parameters and moments are untouched by those, take_back_skipped() takes them out of the step counts again
        self.skipped = torch.zeros(1, dtype=torch.int32, device=dev) if dev.type == 'cuda' else None
        self.modules = list(modules)
        for m in self.modules:
            # generator: let the fused backward accumulate straight into the arena
            if hasattr(m, '_param_list') and [id(p) for p in m._param_list()] == [id(p) for p in self.params]:
                m._grad_sink = _GradSink([self.flat_g.data_ptr() + 4 * o for o in self.offsets])
        self._invalidate()

    @property
    def step_count(self):
        """The largest per-parameter step count (with one group and nothing frozen: the step count)."""
        return max(self.steps)

    # ------------------------------------------------------------------ torch.optim-like surface
    def zero_grad(self, set_to_none=False):
        self.flat_g.zero_()
        for p, o in zip(self.params, self.offsets):
            if p.grad is None or p.grad.data_ptr() != self.flat_g.data_ptr() + 4 * o:
                p.grad = self.flat_g[o:o + p.numel()].view(p.shape)

    def all_reduce_grads(self, group=None):
        """SUM all-reduce of the whole gradient arena (RCCL on GPUs, gloo in CPU tests).  Returns the factor the
        update must scale gradients by (DDP averages: 1/world_size)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return 1.0
        world = dist.get_world_size(group)
        if world == 1:
            return 1.0
        dist.all_reduce(self.flat_g, op=dist.ReduceOp.SUM, group=group)
        return 1.0 / world

    def plan_step(self):
        """What the next ``step()`` launches, from host state alone: ``('single', None, None)`` for sr_adam_step_f32 (one group,
        every parameter takes part, all step counts equal), else ``('groups', class id per parameter, classes)`` with
        ``classes`` as ``partition_classes`` returns them."""
        active = [bool(p.requires_grad) for p in self.params]
        if len(self.param_groups) == 1 and all(active) and len(set(self.steps)) == 1:
            return 'single', None, None
        ids, classes = partition_classes(self.group_of, self.steps, active)
        if len(classes) > MAX_CLASSES:
            raise ValueError(f'{len(classes)} distinct (group, step count) classes, the kernel takes {MAX_CLASSES}')
        return 'groups', ids, classes

    def chunk_classes(self, ids):
        """uint8 [numel / 64] on the host: the class of every 64-float chunk of the arena for the per-parameter ids."""
        out = torch.zeros(self.numel // _ALIGN, dtype=torch.uint8)
        ends = self.offsets[1:] + [self.numel]
        for c, o, e in zip(ids, self.offsets, ends):
            out[o // _ALIGN:e // _ALIGN] = c
        return out

    def _shared(self, key):
        vals = {repr(g[key]) for g in self.param_groups}
        if len(vals) != 1:
            raise ValueError(f'FlatAdam: parameter groups differ in {key}; only lr may differ')
        return self.param_groups[0][key]

    def step(self, grad_scale=1.0):
        if not self.flat_p.is_cuda:
            raise _lib.SrHipError('FlatAdam.step runs only on a HIP device (no CPU fallback)')
        lib = _lib.load()
        route, ids, classes = self.plan_step()
        betas, eps, wd = self._shared('betas'), self._shared('eps'), self._shared('weight_decay')
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if route == 'single':
            g = self.param_groups[0]
            self.steps = [self.steps[0] + 1] * len(self.steps)
            self._took_part.append(None)
            with torch.cuda.device(self.device):
                _lib.check(lib.sr_adam_step_f32(self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.exp_avg.data_ptr(),
                                                self.exp_avg_sq.data_ptr(), self.numel, self.steps[0], g['lr'], betas[0],
                                                betas[1], eps, wd, grad_scale, lib.sr_abort_latch(),
                                                self.skipped.data_ptr(), stream),
                           'sr_adam_step_f32')
            self._invalidate()
            return
        if ids != self._class_ids:   # a freeze, an un-freeze, or parameters whose step counts came apart: twice in an EDVR run
            self.class_of_chunk = self.chunk_classes(ids).to(self.device)
            self._class_ids = ids
            self.partition_writes += 1
        table = (_lib.AdamClass * len(classes))()
        for c, (gi, taken, on) in enumerate(classes):
            table[c].lr = self.param_groups[gi]['lr'] if on else 0.0
            table[c].step = taken + 1 if on else 0
            table[c].active = 1 if on else 0
        took = tuple(classes[c][2] for c in ids)
        if self._took_part and self._took_part[-1] == took:
            took = self._took_part[-1]   # one tuple shared by the steps of a phase
        self._took_part.append(took)
        self.steps = [s + 1 if a else s for s, a in zip(self.steps, took)]
        with torch.cuda.device(self.device):
            _lib.check(lib.sr_adam_step_groups_f32(self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.exp_avg.data_ptr(),
                                                   self.exp_avg_sq.data_ptr(), self.numel, self.class_of_chunk.data_ptr(), table,
                                                   len(classes), betas[0], betas[1], eps, wd, grad_scale, lib.sr_abort_latch(),
                                                   self.skipped.data_ptr(), stream),
                       'sr_adam_step_groups_f32')
        self._invalidate()

    def take_back_skipped(self):
        """After a time-out was reported: how many of the steps issued since were refused on the device (their bias-correction
        counts are taken back from the parameters that took part in them, so the next real step continues the sequence).
        Synchronises."""
        if self.skipped is None:
            return 0
        n = int(self.skipped.item())
        if n:
            for _ in range(n):
                took = self._took_part.pop() if self._took_part else None
                self.steps = [s - 1 if (took is None or took[i]) else s for i, s in enumerate(self.steps)]
            self.skipped.zero_()
        return n

    def _invalidate(self):
        self._epoch[0] += 1
        for m in self.modules:
            if hasattr(m, 'invalidate_packed'):
                m.invalidate_packed()

    # ------------------------------------------------------------------ checkpoint format of torch.optim.Adam
    def state_dict(self):
        state = {}
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            if self.steps[i] > 0:   # as torch: a parameter that never took part has no state
                state[i] = dict(step=torch.tensor(float(self.steps[i])),
                                exp_avg=self.exp_avg[o:o + p.numel()].view(p.shape).clone(),
                                exp_avg_sq=self.exp_avg_sq[o:o + p.numel()].view(p.shape).clone())
        out, at = [], 0
        for g in self.param_groups:
            group = {k: v for k, v in g.items() if k != 'params'}
            group['params'] = list(range(at, at + len(g['params'])))
            at += len(g['params'])
            out.append(group)
        return dict(state=state, param_groups=out)

    def load_state_dict(self, sd):
        if len(sd['param_groups']) != len(self.param_groups):
            raise ValueError('loaded state dict has a different number of parameter groups')
        for mine, group in zip(self.param_groups, sd['param_groups']):
            if len(group['params']) != len(mine['params']):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
            for k, v in group.items():
                if k != 'params':
                    mine[k] = tuple(v) if k == 'betas' else v
        steps = [0] * len(self.params)
        with torch.no_grad():
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            for i, st in sd['state'].items():
                i = int(i)
                p, o = self.params[i], self.offsets[i]
                self.exp_avg[o:o + p.numel()].view(p.shape).copy_(st['exp_avg'])
                self.exp_avg_sq[o:o + p.numel()].view(p.shape).copy_(st['exp_avg_sq'])
                steps[i] = int(float(st['step']))
        self.steps = steps
        self._took_part.clear()


def ema_update(ema_opt_or_flat, src_flat, decay, modules=()):
    """flat_ema = decay*flat_ema + (1-decay)*flat_src  (model_ema, base_model.py:50-57) as one HIP launch."""
    lib = _lib.load()
    dst = ema_opt_or_flat
    assert dst.numel() == src_flat.numel()
    with torch.cuda.device(dst.device):
        _lib.check(lib.sr_axpby_f32(dst.data_ptr(), src_flat.data_ptr(), float(decay), float(1.0 - decay), dst.numel(),
                                    lib.sr_abort_latch(), torch.cuda.current_stream(dst.device).cuda_stream), 'sr_axpby_f32')
    for m in modules:
        if hasattr(m, 'invalidate_packed'):
            m.invalidate_packed()


def flatten_parameters(net, order=None):
    """Moves a network's parameters into one arena (no optimiser) and returns it — used for the EMA copy.  ``order``: the
    parameters in the order the arena shall hold them (default: the module's own), e.g. a grouped optimiser's."""
    params = [p for p in net.parameters()] if order is None else list(order)
    dev = params[0].device
    offsets, off = [], 0
    for p in params:
        offsets.append(off)
        off += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
    flat = torch.zeros(off, dtype=torch.float32, device=dev)
    with torch.no_grad():
        for p, o in zip(params, offsets):
            view = flat[o:o + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view
    if hasattr(net, 'invalidate_packed'):
        net.invalidate_packed()
    return flat
