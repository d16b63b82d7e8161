"""What the per-op fp32 tests (tests/test_f32_nets_opwise_gpu.py) add to the recorder of tests/bf16_opwise.py, which holds nothing that
is bf16: CB8 <-> NCHW views on the host, and a recorder / replayer that also takes a Function with several outputs
(hip_autograd.SpectralNormBatchFn returns one normalised weight per layer).  For such a Function ``out``, ``out_val`` and ``gy`` of the
record are tuples, one entry per output (a ``gy`` entry is None where no gradient arrived)."""
import torch

import bf16_opwise as W
from bf16_opwise import EPS, D, Record, check, worst  # noqa: F401


def cb8_to_nchw(t, c=None):
    """[N, C/8, H, W, 8] -> [N, C, H, W] (float64 on the host); ``c`` keeps the first c channels."""
    t = t.detach().cpu()
    n, cb, h, w, blk = t.shape
    full = t.permute(0, 1, 4, 2, 3).reshape(n, cb * blk, h, w).double()
    return full if c is None else full[:, :c]


def nchw_to_cb8(x):
    """[N, C, H, W] -> [N, ceil(C/8), H, W, 8] on the host in x's dtype, pad channels zero."""
    x = x.detach().cpu()
    n, c, h, w = x.shape
    cb = (c + 7) // 8
    xp = torch.zeros((n, cb * 8, h, w), dtype=x.dtype)
    xp[:, :c] = x
    return xp.reshape(n, cb, 8, h, w).permute(0, 1, 3, 4, 2).contiguous()


def _clones(args):
    return tuple(a.detach().clone() if torch.is_tensor(a) else a for a in args)


class _Proxy:
    def __init__(self, recorder, name, cls):
        self.recorder, self.name, self.cls = recorder, name, cls

    def apply(self, *args):
        for a in args:
            if torch.is_tensor(a) and a.requires_grad and not a.is_leaf:
                a.retain_grad()
        rec = Record(self.name, self.cls, args)
        out = self.cls.apply(*args)
        rec.post = _clones(args)
        rec.out = out
        rec.out_val = _clones(out) if isinstance(out, tuple) else out.detach().clone()
        for o in (out if isinstance(out, tuple) else (out,)):
            if o.requires_grad:
                o.retain_grad()
        self.recorder.records.append(rec)
        return out


class Recorder(W.Recorder):
    def install(self, monkeypatch, table):
        for mod, names in table.items():
            for name in names:
                monkeypatch.setattr(mod, name, _Proxy(self, name, getattr(mod, name)))

    def finish(self):
        self.uses = {}
        for rec in self.records:
            if isinstance(rec.out, tuple):
                rec.gy = tuple(o.grad.detach().clone() if o.grad is not None else None for o in rec.out)
                if all(g is None for g in rec.gy):
                    rec.gy = None
            else:
                rec.gy = rec.out.grad.detach().clone() if rec.out.grad is not None else None
            for a in rec.args:
                if torch.is_tensor(a) and a.requires_grad:
                    self.uses[id(a)] = self.uses.get(id(a), 0) + 1
        return self

    def consumers(self, tensor):
        """[(record index, argument index)] of every recorded use of ``tensor`` as an input, in forward order."""
        return [(i, j) for i, rec in enumerate(self.records) for j, a in enumerate(rec.args) if a is tensor]


class Replay:
    """bf16_opwise.Replay for one or several outputs."""

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
        self.out = _clones(out) if isinstance(out, tuple) else out.detach()
        idx = [i for i, t in enumerate(self.fresh) if torch.is_tensor(t) and t.requires_grad]
        self.grads = {}
        if idx and rec.gy is not None:
            if isinstance(out, tuple):
                pairs = [(o, g) for o, g in zip(out, rec.gy) if g is not None]
                outs, gys = [p[0] for p in pairs], [p[1] for p in pairs]
            else:
                outs, gys = [out], [rec.gy]
            gs = torch.autograd.grad(outs, [self.fresh[i] for i in idx], gys, allow_unused=True)
            self.grads = {i: g for i, g in zip(idx, gs) if g is not None}


def assert_replay_reproduces(recorder, rec, rep):
    """bf16_opwise.assert_replay_reproduces for one or several outputs.  Returns (gradients compared, argument indices whose
    tensor has several consumers: their recorded ``.grad`` is a sum, checked by the caller)."""
    if isinstance(rec.out_val, tuple):
        assert len(rep.out) == len(rec.out_val)
        for k, (a, b) in enumerate(zip(rep.out, rec.out_val)):
            assert torch.equal(a, b), f'{rec}: replayed output {k} differs from the recorded one'
    else:
        assert torch.equal(rep.out, rec.out_val), f'{rec}: the replayed output differs from the recorded one'
    for i, (a, p) in enumerate(zip(rec.args, rec.post)):
        if torch.is_tensor(a) and not a.requires_grad:
            assert torch.equal(rep.fresh[i], p), f'{rec}: argument {i} after the replay differs from the recorded run'
    compared, shared = 0, []
    for i, g in rep.grads.items():
        a = rec.args[i]
        assert a.grad is not None, f'{rec}: argument {i} has no recorded gradient'
        if recorder.single_consumer(a):
            assert torch.equal(g, a.grad), f'{rec}: the replayed gradient of argument {i} differs from the recorded one'
            compared += 1
        else:
            shared.append(i)
    return compared, shared


# ------------------------------------------------------------------------------------ train-mode BatchNorm + LeakyReLU in float64
def bn_tree_depth(M, general):
    """L: the additions a term passes on its way to the root of the kernels' fixed reduction trees, restated from the code.
    bn_small.h (one launch, n h w <= 32768): a thread walks ceil(M / 1024) pixels, then 6 shuffle steps, then the 16 wave results
    in order.  train_ops.hip / disc_bf16.hip (two-stage): the thread stride is 128 * RED_SPLITS = 8192 pixels, 6 shuffle steps, 3
    adds over the four waves (block_sum), then the 64 partial sums in order (bn_finalize_kernel)."""
    return -(-M // 8192) + 6 + 3 + 64 if general else -(-M // 1024) + 6 + 16


def bn_train_reference(z, g64, b64, rm64, rv64, eps32, slope32, K, a, gy, mutate=None, store=0.0):
    """float64 BatchNorm (batch statistics) + LeakyReLU of ``z`` [n, c, h, w], written out, with the bounds of the derivation in
    tests/test_vgg_bf16_opwise_gpu.py's docstring for K = L + 6.  ``a`` is the kernel's own output (the backward's LeakyReLU mask), ``gy``
    the upstream gradient.  ``store`` is the relative rounding of the activation stores (0 for fp32: the store rounds nothing that is
    not already counted; 2^-8 for bf16).  The momentum is 0.1.  M = 1 follows the kernels' own rule: unbiased = biased variance.
    Returns {what: (want, bound)}.  ``mutate`` builds a wrong reference (negative controls)."""
    n, c, h, w = z.shape
    M = n * h * w
    v4 = lambda t: t.view(1, c, 1, 1)  # noqa: E731
    if mutate == 'eps':
        eps32 = 1e-3
    mu = z.mean((0, 2, 3))
    var = ((z - v4(mu)) ** 2).mean((0, 2, 3))
    if mutate == 'one_pass':     # E[x^2] - E[x]^2 evaluated in float32, clamped at 0: what a one-pass kernel would normalise with
        zf = z.float()
        var = ((zf * zf).mean((0, 2, 3)) - zf.mean((0, 2, 3)) ** 2).clamp_min(0).double()
    dmu = K * EPS * z.abs().sum((0, 2, 3)) / M
    dvar = K * EPS * var + dmu ** 2
    inv = 1.0 / torch.sqrt(var + eps32)
    ris = 0.5 * dvar / (var + eps32) + 3 * EPS
    d = z - v4(mu)
    xhat = d * v4(inv)
    pre = v4(g64) * xhat + v4(b64)
    y64 = torch.where(pre > 0, pre, slope32 * pre)
    dxhat = v4(inv) * (d.abs() * v4(ris) + v4(dmu))
    E = v4(g64.abs()) * dxhat + 5 * EPS * ((v4(g64) * xhat).abs() + v4(b64.abs()))
    res = {'fwd': (y64, E + store * (y64.abs() + E)), 'mean': (mu, dmu), 'invstd': (inv, inv * ris)}
    f = M / (M - 1) if M > 1 else 1.0
    unb = var if mutate == 'biased_var' else var * f
    res['running_mean'] = (0.9 * rm64 + 0.1 * mu, 4 * EPS * (0.9 * rm64.abs() + 0.1 * mu.abs()) + 0.1 * dmu)
    res['running_var'] = (0.9 * rv64 + 0.1 * unb, 4 * EPS * (0.9 * rv64.abs() + 0.1 * unb) + 0.1 * dvar * f)
    dz = torch.where((gy if mutate == 'mask_from_gy' else a) > 0, gy, gy * slope32)
    dbeta, dgamma = dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3))
    e_db = K * EPS * dz.abs().sum((0, 2, 3))
    e_dg = K * EPS * (dz * xhat).abs().sum((0, 2, 3)) + (dz.abs() * dxhat).sum((0, 2, 3))
    t = dz if mutate == 'no_1_over_M' else dz - (v4(dbeta) + xhat * v4(dgamma)) / M
    dx64 = v4(g64 * inv) * t
    e_t = ((v4(e_db) + xhat.abs() * v4(e_dg) + v4(dgamma.abs()) * (dxhat + 2 * EPS * xhat.abs())) / M
           + 6 * EPS * (dz.abs() + (v4(dbeta.abs()) + (xhat * v4(dgamma)).abs()) / M))
    E = v4(g64.abs() * inv) * e_t + dx64.abs() * (v4(ris) + 2 * EPS)
    res['dx'] = (dx64, E + store * (dx64.abs() + E))
    res['dgamma'] = (dgamma, e_dg)
    res['dbeta'] = (dbeta, e_db)
    return res
