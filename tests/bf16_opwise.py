"""Shared pieces of the per-op bf16 tests (tests/test_edvr_bf16_ops_gpu.py, tests/test_vgg_bf16_opwise_gpu.py): half a bf16 ulp, the
bf16 round trip, CB16 <-> NCHW views on the host, the checker that reports the worst got / bound, and a recorder / replayer of the
autograd Functions a per-layer bf16 route calls.

The recorder stands in for the Functions the routes look up through module attributes at call time (hip_autograd_bf16.ConvFn16, ...,
hip_autograd.LinearFn): every ``apply`` goes to the real Function; the proxy keeps the arguments (detached clones of the tensors), the
output, and asks autograd to keep the output's gradient.  After one backward every op's inputs, output and upstream gradient are known
from the production forward itself.  ``replay`` then runs one recorded op alone on fresh leaf copies.
"""
import torch

EPS = 2.0 ** -24
D = torch.float64


def hulp(v):
    """Half a bf16 ulp of |v| (0 at 0)."""
    v = v.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(v)) - 8)


def bf(t):
    """Rounds to bf16 (nearest even) and back to float64."""
    return t.float().bfloat16().double()


def check(got, want, bound, what):
    err = (got - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f'{what}: max err {float(err.max()):.3e}, largest err / bound {ratio:.3f}')
    assert bool((err <= bound).all()), f'{what}: err / bound = {ratio:.3f}'
    return ratio


def worst(got, want, bound):
    """Largest err / bound without asserting (negative controls: the kernel's output against a mutated reference)."""
    err = (got - want).abs()
    return float((err / bound.clamp_min(1e-300)).max())


def cb16_to_nchw(t, c=None):
    """[N, C/16, H, W, 16] -> [N, C, H, W] (float64 on the host); ``c`` keeps the first c channels."""
    t = t.detach().cpu()
    n, cb, h, w, blk = t.shape
    full = t.permute(0, 1, 4, 2, 3).reshape(n, cb * blk, h, w).double()
    return full if c is None else full[:, :c]


def nchw_to_cb16(x, dtype=torch.bfloat16):
    """[N, C, H, W] -> [N, ceil(C/16), H, W, 16] of ``dtype`` on the host, pad channels zero."""
    x = x.detach().cpu()
    n, c, h, w = x.shape
    cb = (c + 15) // 16
    xp = torch.zeros((n, cb * 16, h, w), dtype=x.dtype)
    xp[:, :c] = x
    return xp.reshape(n, cb, 16, h, w).permute(0, 1, 3, 4, 2).contiguous().to(dtype)


# ------------------------------------------------------------------------------------------------------ recorder / replayer
class Record:
    """One ``apply``: ``args`` are the objects the route passed (kept alive: their identity tells producers from consumers and
    their ``.grad`` is the recorded input gradient), ``vals`` detached clones taken before the call, ``post`` clones taken after it
    (buffers a Function updates in place), ``out`` the output tensor itself, ``out_val`` its detached clone, ``gy`` its gradient."""

    def __init__(self, name, cls, args):
        self.name, self.cls, self.args = name, cls, args
        self.vals = tuple(a.detach().clone() if torch.is_tensor(a) else a for a in args)
        self.post = self.out = self.out_val = self.gy = None
        self.tag = ''

    def __repr__(self):
        return f'{self.name}[{self.tag}]'


class _Proxy:
    def __init__(self, recorder, name, cls):
        self.recorder, self.name, self.cls = recorder, name, cls

    def apply(self, *args):
        for a in args:
            if torch.is_tensor(a) and a.requires_grad and not a.is_leaf:
                a.retain_grad()
        rec = Record(self.name, self.cls, args)
        out = self.cls.apply(*args)
        rec.post = tuple(a.detach().clone() if torch.is_tensor(a) else a for a in args)
        rec.out, rec.out_val = out, out.detach().clone()
        if out.requires_grad:
            out.retain_grad()
        self.recorder.records.append(rec)
        return out


class Recorder:
    """``install(monkeypatch, {module: names})`` puts a proxy in the place of every named Function; ``finish()`` after the backward
    collects the upstream gradients and counts the consumers of every tensor."""

    def __init__(self):
        self.records = []
        self.uses = {}

    def install(self, monkeypatch, table):
        for mod, names in table.items():
            for name in names:
                monkeypatch.setattr(mod, name, _Proxy(self, name, getattr(mod, name)))

    def finish(self):
        self.uses = {}
        for rec in self.records:
            rec.gy = rec.out.grad.detach().clone() if rec.out.grad is not None else None
            for a in rec.args:
                if torch.is_tensor(a) and a.requires_grad:
                    self.uses[id(a)] = self.uses.get(id(a), 0) + 1
        return self

    def single_consumer(self, tensor):
        return self.uses.get(id(tensor), 0) == 1


class Replay:
    """One recorded op run alone: ``fresh`` its arguments (leaf copies; buffers are clones, so an in-place update lands in the copy),
    ``out`` the output, ``grads`` {argument index: gradient} for the recorded upstream gradient."""

    def __init__(self, rec):
        self.fresh = []
        for a, v in zip(rec.args, rec.vals):
            if torch.is_tensor(a):
                t = v.clone()
                if a.requires_grad:
                    t.requires_grad_(True)
                self.fresh.append(t)
            else:
                self.fresh.append(a)
        out = rec.cls.apply(*self.fresh)
        self.out = out.detach()
        idx = [i for i, t in enumerate(self.fresh) if torch.is_tensor(t) and t.requires_grad]
        self.grads = {}
        if idx and rec.gy is not None:
            gs = torch.autograd.grad(out, [self.fresh[i] for i in idx], rec.gy, allow_unused=True)
            self.grads = {i: g for i, g in zip(idx, gs) if g is not None}


def assert_replay_reproduces(recorder, rec, rep):
    """The replayed output equals the recorded one bit for bit; tensors the Function updated in place end as recorded; where an input
    has a single consumer, the replayed input gradient equals the recorded ``.grad`` of that tensor.  Returns the number of gradients
    compared."""
    assert torch.equal(rep.out, rec.out_val), f'{rec}: the replayed output differs from the recorded one'
    for i, (a, p) in enumerate(zip(rec.args, rec.post)):
        if torch.is_tensor(a) and not a.requires_grad:
            assert torch.equal(rep.fresh[i], p), f'{rec}: argument {i} after the replay differs from the recorded run'
    compared = 0
    for i, g in rep.grads.items():
        a = rec.args[i]
        if recorder.single_consumer(a) and a.grad is not None:
            assert torch.equal(g, a.grad), f'{rec}: the replayed gradient of argument {i} differs from the recorded one'
            compared += 1
    return compared
