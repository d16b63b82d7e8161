"""What the per-op fp32 EDVR tests (tests/test_edvr_opwise_gpu.py, tests/test_edvr_opwise_host.py) share; nothing here needs a GPU.

  the three configurations, their weights, inputs and seeds;
  the float64 reference of every operation the fp32 EDVR launches, on NCHW tensors, and ``Ref64Ops``: the same references as an ops
      table, so that the network's own layer list (``EDVR._run``) composes them in the network's order;
  the deformable convolution's backward with the bilinear cell FORCED to the one float32 arithmetic takes (``cells32``,
      ``columns_forced``, ``dcn_backward``) and its bounds at arbitrary offsets (``dcn_backward_bounds``);
  a recorder on top of tests/f32_opwise.py's that also replaces the five Functions ``edvr_arch._CB8Ops`` binds when the class is
      created, counts a tensor passed twice to one call (DCNFn with windows) as one use, keeps the strides of a non-contiguous
      argument in the replay and replays BilinearUpFn's in-place addition from the pre-call value;
  the gradient that must arrive at a Function's output, rebuilt from the replayed gradients of its consumers through the torch
      plumbing between the Functions (``contributions``, ``sum_rule``).

The plumbing (torch.cat, view, reshape, contiguous, expand, ``* 2.0``, slicing, frame selection) is never restated: a second forward
(``Recorder(detach=True)``) hands every Function's output on as a fresh leaf, so the autograd graph of every argument holds the
plumbing between it and those leaves and nothing else, and torch.autograd.grad through it is the plumbing's own adjoint.  Movements
and ``* 2`` are exact in float32.  The only adjoint that adds is the expand over t; the upstream gradient is therefore pushed through
one image at a time (one channel block at a time where two elements of an image meet in one leaf element), each push is exact, and
every contribution to an element is known on its own.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_restate as R  # noqa: E402
import edvr_restate as E  # noqa: E402
import f32_opwise as W  # noqa: E402
from f32_opwise import EPS  # noqa: E402

K_SAMPLE, K_EPI, K_SIGMOID = 8, 2, 4
BLOCKS = dict(num_extract_block=1, num_reconstruct_block=1)
# name: (constructor arguments, input (b, t, c, h, w), input scale, seed of the weights; the input's seed is one more).  The seed is
# the first of 20 .. 29 whose float64 restatement meets both conditions of tests/test_edvr_gpu.py (test_edvr_opwise_gpu.py's docstring).
CONFIGS = {
    'tsa-b2': (dict(num_feat=64, deformable_groups=8, num_frame=3), (2, 3, 3, 12, 36), 1.0, 20),
    'predeblur-hr-b1': (dict(num_feat=64, deformable_groups=8, num_frame=3, with_predeblur=True, hr_in=True), (1, 3, 3, 32, 48), 0.1, 22),
    'nf16-dg2-notsa': (dict(num_feat=16, deformable_groups=2, num_frame=5, with_tsa=False), (2, 5, 3, 8, 12), 1.0, 20),
}
FUNCTIONS = ('ConvFn', 'ConvS2Fn', 'Conv1x1Fn', 'AddFn', 'Bilinear2xFn', 'FromCB8', 'BilinearUpFn', 'DCNFn', 'ToCB8', 'Pool3x3s2Fn',
             'TSACorrFn', 'TSAGateFn', 'PixelShuffleFn')
CLASS_ATTRS = {'enter': 'ToCB8', 'pool': 'Pool3x3s2Fn', 'tsa_corr': 'TSACorrFn', 'tsa_gate': 'TSAGateFn', 'pixel_shuffle': 'PixelShuffleFn'}
DIRTY = {'BilinearUpFn': (2,)}     # arguments a Function updates in place


def f32(v):
    return float(np.float32(v))


def r8(c):
    return (c + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------------------------ the cases
def state_dict(net, seed):
    """tests/test_edvr_gpu.py::_state_dict: plain conv and DCN weights N(0, 1.4^2 / fan_in), conv_offset weights N(0, 1 / fan_in),
    biases N(0, 0.1^2), drawn in the order of the state dict."""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, v in net.state_dict().items():
        if k.endswith('weight'):
            sc = (1.0 if 'conv_offset' in k else 1.4) / np.sqrt(v.shape[1] * v.shape[2] * v.shape[3])
            sd[k] = torch.from_numpy((rng.standard_normal(tuple(v.shape)) * sc).astype(np.float32))
        else:
            sd[k] = torch.from_numpy((rng.standard_normal(tuple(v.shape)) * 0.1).astype(np.float32))
    return sd


def make_case(name, seed=None):
    """(network on the CPU with the case's weights loaded, state dict, input, upstream gradient of the output)."""
    from image_restoration_amd.archs.edvr_arch import EDVR
    kw, shape, scale, seed0 = CONFIGS[name]
    seed = seed0 if seed is None else seed
    net = EDVR(**BLOCKS, **kw)
    sd = state_dict(net, seed)
    net.load_state_dict(sd, strict=True)
    net.eval()
    rng = np.random.default_rng(seed + 1)
    x = torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))
    s = 1 if kw.get('hr_in') else 4
    gy = torch.from_numpy(rng.standard_normal((shape[0], 3, s * shape[3], s * shape[4])).astype(np.float32))
    return net, sd, x, gy


def restated(sd, x, gy, kw, dtype, offsets_out=None):
    """tests/edvr_restate.py in ``dtype``: (output, [input gradient, parameter gradients in the state dict's order]); without ``gy``
    the output alone."""
    p = {k: v.clone().to(dtype).requires_grad_(gy is not None) for k, v in sd.items()}
    xr = x.clone().to(dtype).requires_grad_(gy is not None)
    y = E.edvr(p, xr, num_frame=kw['num_frame'], deformable_groups=kw['deformable_groups'], **BLOCKS, hr_in=kw.get('hr_in', False),
               with_predeblur=kw.get('with_predeblur', False), with_tsa=kw.get('with_tsa', True), offsets_out=offsets_out)
    if gy is None:
        return y.detach()
    return y.detach(), [t.detach() for t in torch.autograd.grad(y, [xr] + list(p.values()), gy.to(dtype))]


def deforms(off, dg):
    """(mean |offset|, share of the samples outside the image) of one level's offsets: the two conditions of tests/test_edvr_gpu.py."""
    h_im, w_im = R.positions(off, dg)
    outside = ((h_im <= -1) | (w_im <= -1) | (h_im >= off.shape[2]) | (w_im >= off.shape[3])).double().mean()
    return float(off.detach().abs().mean()), float(outside)


# -------------------------------------------------------------------------------------------------- float64 references, NCHW
def lrelu(pre, slope):
    return torch.where(pre > 0, pre, slope * pre)


def conv_ref(x, w, b, slope, stride=1, mutate=None):
    """act(conv(x, w) + b) for a k x k kernel with padding k // 2.  ``mutate='odd'``: the stride-2 conv sampled at the odd positions."""
    pad = w.size(2) // 2
    if mutate == 'odd':
        return lrelu(F.conv2d(x, w, b, 1, pad)[:, :, 1::2, 1::2], slope)
    return lrelu(F.conv2d(x, w, b, stride, pad), slope)


def dcn_ref(x, off, logit, w, b, slope, dg, mutate=None):
    """act(modulated deformable conv) with the sigmoid of the mask logits (tests/dcn_restate.py).  ``mutate``: 'swap' exchanges dy
    and dx of every offset pair, 'mask_group' takes every group's mask from the group before it."""
    if mutate == 'swap':
        n, _, h, wd = off.shape
        off = off.reshape(n, -1, 2, h, wd).flip(2).reshape(off.shape)
    if mutate == 'mask_group':
        logit = torch.roll(logit, 9, dims=1)
    return lrelu(R.modulated_deform_conv(x, off, torch.sigmoid(logit), w, b, dg), slope)


def pool_ref(x, mutate=None):
    """``mutate='valid_count'``: the average divides by the number of taps inside the image instead of 9."""
    return torch.cat([F.max_pool2d(x, 3, 2, 1), F.avg_pool2d(x, 3, 2, 1, count_include_pad=mutate != 'valid_count')], dim=1)


def up2_ref(x, mutate=None):
    return F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=mutate == 'align_corners')


def corr_ref(emb, ref, al, t, mutate=None):
    """(correlation (b, t, h, w), its sigmoid, aligned * sigmoid as (b, t * c, h, w)).  ``mutate='other_clip'``: every clip is correlated
    with the centre frame of the next clip."""
    bt, c, h, w = emb.shape
    b = bt // t
    if mutate == 'other_clip':
        ref = torch.roll(ref, 1, dims=0)
    s = (emb.view(b, t, c, h, w) * ref.unsqueeze(1)).sum(2)
    p = torch.sigmoid(s)
    return s, p, (al.view(b, t, c, h, w) * p.unsqueeze(2)).reshape(b, t * c, h, w)


def gate_ref(feat, attn, add):
    return feat * torch.sigmoid(attn) * 2 + add


def up4_add_ref(x, acc):
    return acc + F.interpolate(x, scale_factor=4, mode='bilinear', align_corners=False)


class Ref64Ops:
    """The references above as an ops table of image_restoration_amd.archs.edvr_arch: activations are NCHW tensors in the dtype of the
    input, parameters are read from the network's modules and converted to it.  ``log`` receives (operation, inputs) of every call.
    ``slope32``: LeakyReLU slopes as the kernels hold them (float32(0.1)); False: as tests/edvr_restate.py writes them (0.1)."""

    def __init__(self, slope32=False):
        from image_restoration_amd.archs import edvr_arch
        self.log = []
        self.slope32 = slope32
        for name in ('dims', '_clips', 'center', 'center_over_t', 'frames_to_channels'):   # the frame plumbing is the production code's
            setattr(self, name, getattr(edvr_arch._Ops, name).__get__(self))

    raw = wrap = enter = staticmethod(lambda x: x)

    def _s(self, slope):
        return f32(slope) if self.slope32 else slope

    def _p(self, m, x):
        return m.weight.detach().to(x.dtype), m.bias.detach().to(x.dtype)

    def conv(self, m, x, slope=0.1):
        self.log.append(('conv', (x, m, slope)))
        return conv_ref(x, *self._p(m, x), self._s(slope))

    def conv_s2(self, m, x, slope=0.1):
        self.log.append(('conv_s2', (x, m, slope)))
        return conv_ref(x, *self._p(m, x), self._s(slope), stride=2)

    def conv1x1(self, m, x, slope=0.1):
        self.log.append(('conv1x1', (x, m, slope)))
        return conv_ref(x, *self._p(m, x), self._s(slope))

    def conv_add(self, m, x, other, slope=0.1):
        return self.conv(m, x, slope) + other

    def conv_nchw(self, m, x):
        return self.conv(m, x, 1.0)

    def resblock(self, m, x, extra=None):
        y = x + self.conv(m.conv2, self.conv(m.conv1, x, 0.0), 1.0)
        return y if extra is None else y + extra

    def cat(self, *ts):
        return torch.cat(ts, dim=1)

    def up2(self, x, scale=1.0):
        self.log.append(('up2', (x,)))
        y = up2_ref(x)
        return y if scale == 1.0 else y * scale

    def pool(self, x):
        self.log.append(('pool', (x,)))
        return pool_ref(x)

    def tsa_corr(self, emb, emb_ref, aligned, t):
        self.log.append(('tsa_corr', (emb, emb_ref, aligned, t)))
        return corr_ref(emb, emb_ref, aligned, t)[2]

    def tsa_gate(self, feat, attn, add):
        return gate_ref(feat, attn, add)

    def pixel_shuffle(self, x, channels, r):
        return F.pixel_shuffle(x, r)

    def dcn(self, pack, x, feat, slope=1.0):
        dg = pack.deformable_groups
        co = conv_ref(feat, *self._p(pack.conv_offset, feat), 1.0)
        self.log.append(('dcn', (x, co[:, :18 * dg], co[:, 18 * dg:], pack, slope, dg)))
        return dcn_ref(x, co[:, :18 * dg], co[:, 18 * dg:], *self._p(pack, x), self._s(slope), dg).contiguous()   # einsum's strides


class _Exit:
    """Stand-ins for the two Functions ``EDVR._run`` calls by name after the last conv."""
    class AddFn:
        apply = staticmethod(lambda a, b: a + b)

    class BilinearUpFn:
        apply = staticmethod(lambda x, s, acc: up4_add_ref(x, acc))


def composed(net, x, monkeypatch, slope32=False):
    """The network's own layer list on the float64 references: (output, the ops table with its log)."""
    from image_restoration_amd import hip_autograd as A
    ops = Ref64Ops(slope32)
    monkeypatch.setattr(A, 'AddFn', _Exit.AddFn)
    monkeypatch.setattr(A, 'BilinearUpFn', _Exit.BilinearUpFn)
    return net._run(x, ops), ops


# ------------------------------------------------------------------------------- deformable conv backward on the float32 cell
def cells32(off, dg):
    """(inside, h_low, w_low) as float32 arithmetic in the kernel's operation order gives them (dcn_ops.hip, bilinear_at): h_im =
    float(y - 1 + i) + offset is ONE rounding (tests/dcn_restate.py::positions adds in that order), the `inside` test and the floor
    are taken of that float32 number, and outside the image the cell is (0, 0) with no valid corner."""
    h_im, w_im = R.positions(off.float(), dg)
    H, Wd = off.shape[2:]
    inside = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < Wd)
    zero = torch.zeros_like(h_im)
    return inside, torch.floor(torch.where(inside, h_im, zero)).double(), torch.floor(torch.where(inside, w_im, zero)).double()


def cells64(off, dg):
    """The same in float64: where it equals cells32, the forced-cell reference is tests/dcn_restate.py's."""
    h_im, w_im = R.positions(off, dg)
    H, Wd = off.shape[2:]
    inside = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < Wd)
    zero = torch.zeros_like(h_im)
    return inside, torch.floor(torch.where(inside, h_im, zero)), torch.floor(torch.where(inside, w_im, zero))


def columns_forced(x, offset, mask, dg, cell, corner_weights='bilinear'):
    """tests/dcn_restate.py::columns with the `inside` test and the bilinear cell given instead of taken from the float64 position:
    lh = h_im - h_low may then lie a rounding outside [0, 1], and the sample is the cell's bilinear polynomial continued.
    ``corner_weights``: 'bilinear', 'abs' (their magnitudes) or 'ones'."""
    n, cin, H, Wd = x.shape
    cpg = cin // dg
    dt = x.dtype
    inside, h_low, w_low = cell
    h_im, w_im = R.positions(offset, dg)
    lh, lw = h_im - h_low, w_im - w_low
    flat = x.reshape(n, dg, cpg, H * Wd)
    val = torch.zeros((n, dg, cpg, 9, H, Wd), dtype=dt)
    for dh, dw, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
        hc, wc = (h_low + dh).long(), (w_low + dw).long()
        valid = inside & (hc >= 0) & (hc <= H - 1) & (wc >= 0) & (wc <= Wd - 1)
        idx = (hc.clamp(0, H - 1) * Wd + wc.clamp(0, Wd - 1)).view(n, dg, 1, 9 * H * Wd).expand(n, dg, cpg, 9 * H * Wd)
        v = torch.gather(flat, 3, idx).view(n, dg, cpg, 9, H, Wd)
        if corner_weights == 'ones':
            wt = torch.ones_like(wt)
        elif corner_weights == 'abs':
            wt = wt.abs()
        val = val + (wt * valid.to(dt)).unsqueeze(2) * v
    val = val * mask.reshape(n, dg, 1, 9, H, Wd)
    return val.reshape(n, cin, 9, H, Wd)


def dcn_backward(x, off, logit, wt, bias, dg, dz, cell, mutate=None):
    """float64 gradients (dx, doffset, dlogit, dweight, dbias) of sum(dz * (W * columns + bias)) on the given cell.  ``mutate='swap'``:
    the dy and dx gradients of every offset pair exchanged."""
    leaves = [t.clone().requires_grad_(True) for t in (x, off, logit, wt, bias)]
    xs, os_, ls, ws, bs = leaves
    cout, cin = wt.shape[:2]
    z = torch.einsum('ock,nckhw->nohw', ws.reshape(cout, cin, 9), columns_forced(xs, os_, torch.sigmoid(ls), dg, cell))
    z = z + bs.view(1, -1, 1, 1)
    g = list(torch.autograd.grad(z, leaves, dz))
    if mutate == 'swap':
        n, _, h, w = off.shape
        g[1] = g[1].reshape(n, -1, 2, h, w).flip(2).reshape(off.shape)
    return g


def dcn_backward_bounds(x, off, logit, wt, dg, dz, cell, chain):
    """{gradient: bound} of DCNFn's backward at arbitrary offsets against ``dcn_backward`` on the float32 cell (the
    docstring of tests/test_edvr_opwise_gpu.py), without the EPS |reference| term.  ``chain``: the chain count of sr_convd_wgrad_f32
    with ksize 1 over 9 cin channels (tests/test_convd_ops_gpu.py::_wgradd_chain).  Also returns J, the largest number of atomicAdds
    that reach one element of dx."""
    n, cin, H, Wd = x.shape
    cout = wt.size(0)
    cpg = cin // dg
    m = torch.sigmoid(logit)
    m5 = m.reshape(n, dg, 9, H, Wd)
    ones = torch.ones_like(m)
    adz = dz.abs()
    h_im, w_im = R.positions(off, dg)
    mag = h_im.abs() + w_im.abs() + 2                                                        # [n, dg, 9, H, W]

    def per_c(t):
        return t.reshape(n, dg, cpg, 9, H, Wd)

    cols_abs = columns_forced(x.abs(), off, m, dg, cell, 'abs')                              # m sum |w| |v|
    samp_abs = columns_forced(x.abs(), off, ones, dg, cell, 'abs')                           # sum |w| |v|
    S1 = columns_forced(x.abs(), off, ones, dg, cell, 'ones')                                # sum |v| over the valid corners
    Acol = torch.einsum('ock,nohw->nckhw', wt.abs().reshape(cout, cin, 9), adz)
    K_COL = 2 * r8(cout) + 8
    coordS = (per_c(S1) * (m5 * mag).unsqueeze(2)).reshape(n, cin, 9, H, Wd)                 # (|h_im| + |w_im| + 2) m sum |v|
    out = {}
    Aw = torch.einsum('nohw,nckhw->ock', adz, cols_abs)
    Cw = torch.einsum('nohw,nckhw->ock', adz, coordS)
    out['dweight'] = ((chain + K_SAMPLE + 1 + K_SIGMOID + 1) * EPS * Aw + EPS * Cw).reshape(cout, cin, 3, 3)
    out['dbias'] = (chain + 1) * EPS * adz.sum(dim=(0, 2, 3))
    Am = per_c(Acol * samp_abs).sum(dim=2)
    Cm = (per_c(Acol * S1) * mag.unsqueeze(2)).sum(dim=2)
    km = 2 * cpg + 7 + 1 + K_COL
    kdsig = 7 + 4 * torch.exp(logit.reshape(n, dg, 9, H, Wd))
    out['dmask'] = (EPS * m5 * (1 - m5) * ((km + kdsig) * Am + Cm)).reshape(n, 9 * dg, H, Wd)
    Ao = per_c(Acol * S1).sum(dim=2) * m5
    bo = EPS * Ao * (2 * cpg + 8 + K_COL + K_SIGMOID + mag)
    out['doffset'] = bo.unsqueeze(3).expand(n, dg, 9, 2, H, Wd).reshape(n, 18 * dg, H, Wd)
    xa = x.abs().clone().requires_grad_(True)
    Ax, = torch.autograd.grad(columns_forced(xa, off, m, dg, cell, 'abs'), xa, Acol)
    xo = torch.ones_like(x).requires_grad_(True)
    col1 = columns_forced(xo, off, ones, dg, cell, 'ones')
    J, = torch.autograd.grad(col1, xo, torch.ones_like(col1), retain_graph=True)
    Cx, =torch.autograd.grad(col1, xo, (per_c(Acol) * (m5 * mag).unsqueeze(2)).reshape(n, cin, 9, H, Wd))
    jmax = int(J.max())
    out['dx'] = (jmax + 2 + 1 + K_COL + K_SIGMOID) * EPS * Ax + EPS * Cx
    out['dx order'] = 2 * jmax * EPS * Ax * (1 + 64 * EPS)       # two arrival orders of the same J terms (sum_rule's slack)
    return out, jmax


# ----------------------------------------------------------------------------------------------------------- recorder, replayer
class _Proxy:
    def __init__(self, recorder, name, cls):
        self.recorder, self.name, self.cls = recorder, name, cls

    def __getattr__(self, attr):     # a Function that names itself (DCNFn._windows) finds the class's own helpers
        return getattr(self.cls, attr)

    def apply(self, *args):
        rec = W.Record(self.name, self.cls, args)
        rec.strides = tuple((a.stride(), a.is_contiguous()) if torch.is_tensor(a) else None for a in args)
        if self.recorder.detach:     # forward only, every output handed on as a fresh leaf: what follows is plumbing on leaves
            with torch.no_grad():
                out = self.cls.apply(*[a.detach() if torch.is_tensor(a) else a for a in args])
            rec.out_val = out.detach().clone()
            rec.out = out.detach().requires_grad_(True)
            self.recorder.records.append(rec)
            return rec.out
        for a in args:
            if torch.is_tensor(a) and a.requires_grad and not a.is_leaf:
                a.retain_grad()
        out = self.cls.apply(*args)
        rec.post = W._clones(args)
        rec.out, rec.out_val = out, out.detach().clone()
        if out.requires_grad:
            out.retain_grad()
        self.recorder.records.append(rec)
        return out


class Recorder(W.Recorder):
    """``install`` stands in for the Functions looked up in hip_autograd at call time AND for the five ``_CB8Ops`` bound when the class
    was created.  A tensor that one call receives twice (DCNFn with windows: offsets and mask logits are windows of one tensor, whose
    gradient comes back under the offset argument only) is one use."""

    def __init__(self, detach=False):
        super().__init__()
        self.detach = detach

    def install(self, monkeypatch):
        from image_restoration_amd import hip_autograd as A
        from image_restoration_amd.archs import edvr_arch
        proxies = {name: _Proxy(self, name, getattr(A, name)) for name in FUNCTIONS}
        for name, p in proxies.items():
            monkeypatch.setattr(A, name, p)
        for attr, name in CLASS_ATTRS.items():
            assert getattr(edvr_arch._CB8Ops, attr) == proxies[name].cls.apply, attr
            monkeypatch.setattr(edvr_arch._CB8Ops, attr, proxies[name].apply)

    def finish(self):
        self.uses = {}
        for rec in self.records:
            rec.gy = rec.out.grad.detach().clone() if rec.out.grad is not None else None
            for i in {id(a) for a in rec.args if torch.is_tensor(a) and a.requires_grad}:
                self.uses[i] = self.uses.get(i, 0) + 1
        return self


def grad_args(rec):
    """Indices of the tensor arguments that take a gradient, a tensor passed twice under its first index only."""
    seen, idx = set(), []
    for i, a in enumerate(rec.args):
        if torch.is_tensor(a) and a.requires_grad and id(a) not in seen:
            seen.add(id(a))
            idx.append(i)
    return idx


def _as_recorded(v, strides):
    """A copy of ``v`` with the strides the production call saw (a non-contiguous NCHW slice stays one)."""
    stride, contiguous = strides
    if contiguous or 0 in stride:
        return v.clone()
    need = sum((s - 1) * st for s, st in zip(v.shape, stride)) + 1
    t = torch.zeros(need, dtype=v.dtype, device=v.device).as_strided(tuple(v.shape), stride)
    t.copy_(v)
    return t


class Replay:
    """One recorded op alone on fresh leaf copies of the values its arguments had BEFORE the call, in the strides they had; a
    tensor passed twice is one leaf; an argument the Function updates in place (BilinearUpFn's ``acc``) goes in as a differentiable
    copy of its leaf, so the update lands in the copy."""

    def __init__(self, rec):
        self.fresh, seen = [], {}
        for a, v, st in zip(rec.args, rec.vals, rec.strides):
            if not torch.is_tensor(a):
                self.fresh.append(a)
            elif id(a) in seen:
                self.fresh.append(seen[id(a)])
            else:
                t = _as_recorded(v, st)
                if a.requires_grad:
                    t.requires_grad_(True)
                seen[id(a)] = t
                self.fresh.append(t)
        call = list(self.fresh)
        for j in DIRTY.get(rec.name, ()):
            if len(call) > j and torch.is_tensor(call[j]):
                call[j] = call[j].clone()
        out = rec.cls.apply(*call)
        self.out = out.detach().clone()
        idx = grad_args(rec)
        self.grads = {}
        if idx and rec.gy is not None:
            gs = torch.autograd.grad(out, [self.fresh[i] for i in idx], rec.gy, allow_unused=True)
            self.grads = {i: g for i, g in zip(idx, gs) if g is not None}


def assert_replay_reproduces(rec, rep, single):
    """Bit for bit: the output; every argument that takes no gradient is left as the recorded call left it; the recorded ``.grad`` of
    every argument with a single consumer (``single(j)``: argument j is a Function's output, the input or a parameter itself, and
    nothing else consumes that tensor, not even through plumbing).  Returns the number of gradients compared."""
    assert torch.equal(rep.out, rec.out_val), f'{rec}: the replayed output differs from the recorded one'
    for i, (a, p) in enumerate(zip(rec.args, rec.post)):
        if torch.is_tensor(a) and not a.requires_grad:
            assert torch.equal(rep.fresh[i], p), f'{rec}: argument {i} after the replay differs from the recorded run'
    compared = 0
    for i, g in rep.grads.items():
        a = rec.args[i]
        assert a.grad is not None, f'{rec}: argument {i} has no recorded gradient'
        if single(i):
            assert torch.equal(g, a.grad), f'{rec}: the replayed gradient of argument {i} differs from the recorded one'
            compared += 1
    return compared


# ------------------------------------------------------------------------------------------ gradients through the torch plumbing
def contributions(records, leaves, grads_of, slack_of=None, one_frame=False):
    """{id(leaf): [(contribution, which elements it reaches, slack)]} for the records of a ``detach=True`` run.  ``grads_of(i)`` gives
    {argument index: gradient} of record i (the replayed gradients of the recorded run), ``slack_of(i, j)`` a tensor like that
    gradient by which it is only known (DCNFn's dx: the arrival order of its atomicAdds), or None.  An argument that IS a leaf
    contributes its gradient as it stands.  Any other argument is plumbing of leaves: its gradient goes through torch.autograd.grad one
    image at a time (one channel block at a time where two elements of an image meet in a leaf), so that an adjoint that adds (expand
    over frames) adds one number and zeros: every push is exact.
    ``one_frame`` (negative control): of the pushes of one argument that land on the same elements of a leaf only the first is kept."""
    by_id = {id(t): t for t in leaves}
    out = {i: [] for i in by_id}
    for i, rec in enumerate(records):
        for j, g in grads_of(i).items():
            a = rec.args[j]
            slack = slack_of(i, j) if slack_of is not None else None
            if id(a) in by_id:
                out[id(a)].append((g, torch.ones_like(g, dtype=torch.bool), slack))
                continue
            assert a.grad_fn is not None, f'{rec}: argument {j} is neither a leaf nor plumbing of leaves'
            first = torch.autograd.grad(a, leaves, torch.ones_like(g), retain_graph=True, allow_unused=True)
            hit = [t for t, c in zip(leaves, first) if c is not None and bool((c != 0).any())]
            if not hit:
                continue
            kept = {id(t): None for t in hit}

            def push(sel):
                one = torch.zeros_like(g)
                one[sel] = 1.0
                os_ = torch.autograd.grad(a, hit, one, retain_graph=True, allow_unused=True)
                return one, os_

            for p in range(g.size(0)):
                sels = [(p,)]
                one, os_ = push(sels[0])
                if any(o is not None and float(o.max()) > 1 for o in os_):
                    # two elements of this image land on one element of a leaf (cat of a frame with the expanded centre frame), or
                    # the path scales (* 2): push one channel block at a time; within one the plumbing only moves and scales
                    sels = [(p, c) for c in range(g.size(1))]
                for sel in sels:
                    if len(sels) > 1:
                        one, os_ = push(sel)
                    piece = g * one
                    cs = torch.autograd.grad(a, hit, piece, retain_graph=True, allow_unused=True)
                    ss = torch.autograd.grad(a, hit, slack * one, retain_graph=True, allow_unused=True) if slack is not None \
                        else [None] * len(hit)
                    for t, c, o, sk in zip(hit, cs, os_, ss):
                        if c is None or not bool((o != 0).any()):
                            continue
                        ind = o != 0
                        if one_frame and kept[id(t)] is not None and bool((kept[id(t)] & ind).any()):
                            continue
                        kept[id(t)] = ind if kept[id(t)] is None else kept[id(t)] | ind
                        out[id(t)].append((c, ind, sk))
    return out


def sum_rule(contribs, got):
    """The recorded gradient ``got`` against its contributions, element by element (m contributions reach an element):
    m <= 2   the float32 sum, in either order: a + b = b + a, and with one contribution the number itself;
    m > 2    within (m - 1) EPS sum |g_i| of the float64 sum: m - 1 float32 additions in whatever order autograd took;
    where a contribution is only known within a slack, every rule is the second with the slacks added.
    Returns (all elements pass, largest error / bound over the bounded elements, largest m)."""
    dev = got.device
    S = torch.zeros(got.shape, dtype=torch.float64, device=dev)
    Aabs, slack = torch.zeros_like(S), torch.zeros_like(S)
    m = torch.zeros(got.shape, dtype=torch.long, device=dev)
    for c, ind, s in contribs:
        S += c.double()
        Aabs += c.double().abs()
        m += ind.long()
        if s is not None:
            slack += s.double()
    err = (got.double() - S).abs()
    bound = (m - 1).clamp_min(0).double() * EPS * Aabs * (1 + 16 * EPS) + slack
    bounded = (m > 2) | (slack > 0)
    ok = torch.where(bounded, err <= bound, got == S.float())
    ratio = float((err / bound.clamp_min(1e-300))[bounded].max()) if bool(bounded.any()) else 0.0
    return bool(ok.all()), ratio, int(m.max())


# ------------------------------------------------------------------------- reference and bound of every op (NCHW float64 inputs)
# Each returns {quantity: (reference, bound)}; the derivations are cited in the docstring of tests/test_edvr_opwise_gpu.py.  ``y`` is the
# op's own output (the LeakyReLU / ReLU mask of its backward), ``gy`` the upstream gradient; without ``gy`` only the forward is returned.
def _dz(y, gy, slope):
    """dL/d(pre-activation) exactly as sr_lrelu_bwd_f32 forms it: gy where y > 0, else the float32 product gy * slope."""
    if slope == 1.0:
        return gy
    return torch.where(y > 0, gy, (gy.float() * torch.tensor(slope, dtype=torch.float32)).double())


def conv_spec(x, w, b, slope, stride=1, y=None, gy=None, k_w=None, k_dx_extra=0, mutate=None):
    """k x k conv, padding k // 2, stride 1 or 2: k = 2 taps cin_pad + 8 forward, 2 taps roundup8(cout) + 8 (+ ``k_dx_extra``) for the
    data gradient, ``k_w`` for the weight and bias gradients.  ``mutate``: 'odd' (conv_ref), 'slope' (LeakyReLU 0.2 in the forward),
    'unmasked' (the backward without the activation's mask)."""
    cout, cin, k, _ = w.shape
    pad, taps = k // 2, k * k
    s32 = f32(0.2 if mutate == 'slope' else slope)
    want = conv_ref(x, w, b, s32, stride, mutate)
    A = F.conv2d(x.abs(), w.abs(), b.abs(), stride, pad)
    res = {'fwd': (want, (2 * taps * r8(cin) + 8) * EPS * A + EPS * want.abs())}
    if gy is None:
        return res
    dz = gy if mutate == 'unmasked' else _dz(y, gy, slope)
    dx = torch.nn.grad.conv2d_input(x.shape, w, dz, stride, pad)
    Ad = torch.nn.grad.conv2d_input(x.shape, w.abs(), dz.abs(), stride, pad)
    res['dx'] = (dx, (2 * taps * r8(cout) + 8 + k_dx_extra) * EPS * Ad + EPS * dx.abs())
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dz, stride, pad)
    Aw = torch.nn.grad.conv2d_weight(x.abs(), w.shape, dz.abs(), stride, pad)
    res['dw'] = (dw, k_w * EPS * Aw + EPS * dw.abs())
    db = dz.sum((0, 2, 3))
    res['db'] = (db, k_w * EPS * dz.abs().sum((0, 2, 3)) + EPS * db.abs())
    return res


def pool_spec(x, gy=None, mutate=None):
    """[max, avg] pooling 3x3 / s2 / p1: the maximum bit-exact (torch's CPU float32 max_pool2d), the average k = 9; backward k = 12 on
    the same adjoint of |g| (tests/test_edvr_ops_gpu.py)."""
    c = x.size(1)
    want = pool_ref(x, mutate)
    assert torch.equal(want[:, :c], F.max_pool2d(x.float(), 3, 2, 1).double())
    A = F.avg_pool2d(x.abs(), 3, 2, 1)
    res = {'fwd': (want, torch.cat([torch.zeros_like(A), 9 * EPS * A + EPS * want[:, c:].abs()], dim=1))}
    if gy is not None:
        xr = x.clone().requires_grad_(True)
        dx, = torch.autograd.grad(pool_ref(xr), xr, gy, retain_graph=True)
        Aabs, = torch.autograd.grad(pool_ref(xr), xr, gy.abs())
        res['dx'] = (dx, 12 * EPS * Aabs + EPS * dx.abs())
    return res


def up2_spec(x, gy=None, mutate=None):
    """Bilinear x2, align_corners=False: 6 EPS interp(|x|) forward, 20 EPS adjoint(|g|) backward (tests/test_train_ops_gpu.py)."""
    xr = x.clone().requires_grad_(True)
    yr = up2_ref(xr, mutate)
    res = {'fwd': (yr.detach(), 6 * EPS * up2_ref(x.abs(), mutate))}
    if gy is not None:
        dx, = torch.autograd.grad(yr, xr, gy)
        xa = x.clone().requires_grad_(True)
        Aabs, = torch.autograd.grad(up2_ref(xa, mutate), xa, gy.abs())
        res['dx'] = (dx, 20 * EPS * Aabs)
    return res


def corr_spec(emb, ref, al, t, gy=None, mutate=None):
    """TSA correlation (tests/test_edvr_ops_gpu.py): p within bound_p = 2 c EPS A / 4 + 4 EPS p of sigmoid(sum_c emb emb_ref), A = sum
    |emb| |emb_ref|.  The Function does not return p; its output is one rounding from aligned * (the kernel's p):
    |out - aligned p64| <= |aligned| bound_p (1 + EPS) + EPS |aligned| p64.  Backward as derived there, on the kernel's own p."""
    bt, c, h, w = emb.shape
    b = bt // t
    s, p, want = corr_ref(emb, ref, al, t, mutate)
    e5, a5 = emb.view(b, t, c, h, w), al.view(b, t, c, h, w)
    As = (e5.abs() * ref.abs().unsqueeze(1)).sum(2)
    bound_p = 0.25 * 2 * c * EPS * As + K_SIGMOID * EPS * p
    bp = bound_p.unsqueeze(2)
    res = {'fwd': (want, (a5.abs() * bp * (1 + EPS) + EPS * a5.abs() * p.unsqueeze(2)).reshape(want.shape))}
    if gy is not None:
        e_, r_, a_ = (v.clone().requires_grad_(True) for v in (emb, ref, al))
        de, dr, da = torch.autograd.grad(corr_ref(e_, r_, a_, t)[2], (e_, r_, a_), gy)
        g5 = gy.reshape(b, t, c, h, w)
        res['d_aligned'] = (da, (g5.abs() * bp).reshape(da.shape) + EPS * da.abs())
        S, AS = (g5 * a5).sum(2), (g5.abs() * a5.abs()).sum(2)
        q = p * (1 - p)
        bound_ds = q * 2 * c * EPS * AS + S.abs() * bound_p + 3 * EPS * S.abs() * q
        ds = S * q
        res['d_emb'] = (de, (ref.abs().unsqueeze(1) * bound_ds.unsqueeze(2)).reshape(de.shape) + EPS * de.abs())
        res['d_emb_ref'] = (dr, (e5.abs() * bound_ds.unsqueeze(2)).sum(1) + 2 * t * EPS * (e5 * ds.unsqueeze(2)).abs().sum(1) + EPS * dr.abs())
    return res


def gate_spec(feat, attn, add, gy=None):
    """feat * sigmoid(attn) * 2 + add: k = 6; d_feat k = 5; d_attn (8 + 4 e^attn) relative; d_add = g (tests/test_edvr_ops_gpu.py)."""
    m = torch.sigmoid(attn)
    want = gate_ref(feat, attn, add)
    res = {'fwd': (want, 6 * EPS * (2 * feat.abs() * m + add.abs()) + EPS * want.abs())}
    if gy is not None:
        df = gy * 2 * m
        res['d_feat'] = (df, 5 * EPS * df.abs() + EPS * df.abs())
        da = gy * feat * 2 * m * (1 - m)
        res['d_attn'] = (da, (8 + 4 * torch.exp(attn)) * EPS * da.abs() + EPS * da.abs())
        res['d_add'] = (gy, torch.zeros_like(gy))
    return res


def up4_spec(x, acc, gy=None):
    """acc + bilinear x4 of x (tests/test_msrresnet_gpu.py): (7 + 12 max(h, w)) EPS max |x| for the interpolation and one rounding
    for the addition into acc; the adjoint within ((2 s)^2 + 2 + 12 max(h, w)) EPS adjoint(|g|); acc's gradient is g."""
    h, w = x.shape[2:]
    want = up4_add_ref(x, acc)
    res = {'fwd': (want, torch.full_like(want, (7 + 12 * max(h, w)) * EPS * float(x.abs().max())) + EPS * want.abs())}
    if gy is not None:
        xr = x.clone().requires_grad_(True)
        up = F.interpolate(xr, scale_factor=4, mode='bilinear', align_corners=False)
        dx, = torch.autograd.grad(up, xr, gy, retain_graph=True)
        S, = torch.autograd.grad(up, xr, gy.abs())
        res['dx'] = (dx, (64 + 2 + 12 * max(h, w)) * EPS * S)
        res['d_acc'] = (gy, torch.zeros_like(gy))
    return res


def dcn_coord_term(x, off, m, wt, dg):
    """tests/test_dcn_ops_gpu.py::_coord_term: sum |W| EPS (|h_im| + |w_im| + 2) |mask| sum of |v| over the valid corners."""
    n, cin, h, w = x.shape
    h_im, w_im = R.positions(off, dg)
    mag = h_im.abs() + w_im.abs() + 2
    S = R.columns(x.abs(), off, m.abs(), dg, corner_weights='ones').reshape(n, dg, cin // dg, 9, h, w)
    T = (S * mag.unsqueeze(2)).reshape(n, cin, 9, h, w)
    cout = wt.shape[0]
    return EPS * torch.einsum('ock,nckhw->nohw', wt.abs().reshape(cout, cin, 9), T)


def dcn_spec(x, off, logit, wt, b, slope, dg, y=None, gy=None, chain=None, mutate=None):
    """DCNFn with logit masks at arbitrary offsets.  Forward: tests/test_dcn_ops_gpu.py, k = 2 * 9 cin + K_SAMPLE + 1 + K_EPI +
    K_SIGMOID and the coordinate term.  Backward: on the float32 cell, ``dcn_backward_bounds``.  Also returns J under 'J'."""
    cin = x.size(1)
    m = torch.sigmoid(logit)
    want = dcn_ref(x, off, logit, wt, b, f32(slope), dg, mutate)
    Aabs = R.modulated_deform_conv(x.abs(), off, m, wt.abs(), b.abs(), dg)
    k = 2 * 9 * cin + K_SAMPLE + 1 + K_EPI + K_SIGMOID
    res = {'fwd': (want, k * EPS * Aabs + dcn_coord_term(x, off, m, wt, dg) + EPS * want.abs())}
    if gy is None:
        return res
    dz = _dz(y, gy, slope)
    cell = cells32(off, dg)
    refs = dcn_backward(x, off, logit, wt, b, dg, dz, cell, mutate)
    bounds, jmax = dcn_backward_bounds(x, off, logit, wt, dg, dz, cell, chain)
    for name, ref in zip(('dx', 'doffset', 'dmask', 'dweight', 'dbias'), refs):
        res[name] = (ref, bounds[name] + EPS * ref.abs())
    res['dx order'] = bounds['dx order']
    res['J'] = jmax
    return res
