"""sr_dcn_bwd_data_det_f32 (include/sr_hip_dcn_det.h) on the GPU: the deterministic input gradient of the deformable convolution.

dx against the numpy model of the integer arithmetic (tests/dcn_det_model.py) bit for bit — the model is held to the float64
definition under the header's bound on the host, tests/test_dcn_det_host.py — and doffset / dmask against sr_dcn_bwd_data_f32 bit
for bit, on every image size, channel split, batch, mask kind and offset kind of the model's case list.  The fp32 mask VALUE of a
logit mask is the device's own sigmoid, read back through sr_dcn_cols_f32 (x = 1 and offsets that make every tap sample its own
pixel: the column is then exactly m).

Conventions (tests/test_dcn_ops_gpu.py): dx, doffset and dmask are windows between SENTINEL blocks that must come back unchanged;
dx's window is PREFILLED with SENTINEL (the entry point stores, the caller need not zero); the pad channels of the offset and mask
tensors hold values that must not matter — for the mask 3e38 (raw) or NaN (logit), which would wreck the image's scale if the scale
kernel read them."""
import os
import sys

import numpy as np
import pytest
import torch

from image_restoration_amd import hip_ops as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_det_model as M  # noqa: E402
import dcn_restate as R  # noqa: E402
from test_dcn_ops_gpu import EPS, K_SIGMOID, SENTINEL, _cb8_buf, _check, _nchw, _sentinel_kept  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cuda():
    return torch.device('cuda:0')


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float32)).double()


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


class Operands:
    """The device operands of one case: x (only doffset / dmask read it), the offsets, the mask input, dcol."""

    def __init__(self, cuda, dcol, offset, mask_in, dg, logit, seed=0):
        n, _, cin, h, w = dcol.shape
        self.shape, self.dg, self.logit, self.cuda = (n, cin, h, w), dg, logit, cuda
        x = np.random.default_rng(seed).standard_normal((n, cin, h, w)).astype(np.float32)
        _, self.x = _cb8_buf(_t(x), cuda)
        _, self.off = _cb8_buf(_t(offset), cuda, pad_fill=7.5)
        _, self.mask = _cb8_buf(_t(mask_in), cuda, pad_fill=float('nan') if logit else 3e38)
        self.dcol = H.CB8(torch.from_numpy(dcol.reshape(n, 9 * cin // 8, 8, h, w).transpose(0, 1, 3, 4, 2).copy()).to(cuda))

    def outputs(self):
        n, cin, h, w = self.shape
        _, dx = _cb8_buf(torch.full((n, cin, h, w), SENTINEL, dtype=torch.float64), self.cuda)
        _, do = _cb8_buf(torch.zeros((n, 18 * self.dg, h, w), dtype=torch.float64), self.cuda, pad_fill=SENTINEL)
        _, dm = _cb8_buf(torch.zeros((n, 9 * self.dg, h, w), dtype=torch.float64), self.cuda, pad_fill=SENTINEL)
        return dx, do, dm

    def det(self, **kw):
        dx, do, dm = self.outputs()
        H.dcn_bwd_data_det(self.dcol, self.x, self.off, self.mask, self.dg, mask_is_logit=self.logit, dx=dx, doffset=do, dmask=dm, **kw)
        torch.cuda.synchronize()
        return dx, do, dm

    def atomic(self):
        dx, do, dm = self.outputs()
        dx.buf[:, dx.cb0:dx.cb0 + dx.cbn] = 0
        H.dcn_bwd_data(self.dcol, self.x, self.off, self.mask, self.dg, mask_is_logit=self.logit, dx=dx, doffset=do, dmask=dm)
        torch.cuda.synchronize()
        return dx, do, dm

    def mask_values(self, mask_in):
        """The fp32 mask values as the device forms them: the input itself, or its sigmoid read back through the column kernel."""
        if not self.logit:
            return mask_in
        n, cin, h, w = self.shape
        own = np.zeros((n, self.dg, 9, 2, h, w), np.float32)            # tap (i, j) samples (y - 1 + i - (i - 1), x - 1 + j - (j - 1))
        own[:, :, :, 0] = -(np.arange(9) // 3 - 1).reshape(1, 1, 9, 1, 1)
        own[:, :, :, 1] = -(np.arange(9) % 3 - 1).reshape(1, 1, 9, 1, 1)
        ones = H.CB8(torch.ones((n, cin // 8, h, w, 8), dtype=torch.float32, device=self.cuda))
        _, ow = _cb8_buf(_t(own.reshape(n, 18 * self.dg, h, w)), self.cuda)
        cols = _nchw(H.dcn_cols(ones, ow, self.mask, self.dg, mask_is_logit=True), 9 * cin).float().numpy().reshape(n, 9, self.dg, cin // self.dg, h, w)
        assert (cols == cols[:, :, :, :1]).all()
        return np.ascontiguousarray(cols[:, :, :, 0].transpose(0, 2, 1, 3, 4)).reshape(n, 9 * self.dg, h, w)


def _same(a, b):
    """Two windows' buffers hold the same bits (a NaN equals itself)."""
    return torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32))


def _f32(win, c):
    return _nchw(win, c).float().numpy()


def _kept(dx, do, dm, dg, what):
    for win, ch, name in ((dx, None, 'dx'), (do, 18 * dg, 'doffset'), (dm, 9 * dg, 'dmask')):
        _sentinel_kept(win, f'{what} {name}')
        if ch is not None and win.cbn * 8 != ch:
            assert bool((_nchw(win, win.cbn * 8)[:, ch:] == SENTINEL).all()), (what, name, 'wrote pad channels')


CASES = [(h, w, cin, dg, n, logit) for (h, w) in M.SIZES for (cin, dg) in M.CHANNELS for n in M.BATCHES for logit in (True, False)]


def _cid(c):
    return '{}x{}-c{}g{}-n{}-{}'.format(*c[:5], 'logit' if c[5] else 'raw')


@pytest.mark.parametrize('case', CASES, ids=_cid)
def test_dx_is_the_model_bit_for_bit(cuda, case):
    h, w, cin, dg, n, logit = case
    rng, dcol, mask_in = M.case_data(h, w, cin, dg, n, logit)
    assert H.dcn_bwd_data_det_workspace_bytes(n, cin, h, w) == (8 * n * cin * h * w + 255) // 256 * 256 + (8 * n + 255) // 256 * 256
    m = None
    for kind in M.KINDS:
        offset = M.offsets_of(kind, rng, n, dg, h, w)
        ops = Operands(cuda, dcol, offset, mask_in, dg, logit)
        if m is None:
            m = ops.mask_values(mask_in)
            if logit:                                                   # the device's sigmoid, within its documented 4 EPS
                ref = 1.0 / (1.0 + np.exp(-mask_in.astype(np.float64)))
                assert float(np.abs(m - ref).max()) <= 4 * EPS
        dx, do, dm = ops.det()
        _kept(dx, do, dm, dg, f'{_cid(case)} {kind}')
        model, info = M.det_dx(dcol, offset, m, dg, logit, mask_in)
        assert all(r['state'] == 'sum' for r in info)
        got = _f32(dx, cin)
        assert _bits_equal(got, model), (kind, int((got != model).sum()), float(np.abs(got.astype(np.float64) - model).max()))
        if kind == 'onecell':
            assert max(int(r['count'].max()) for r in info) == 9 * h * w
        adx, ado, adm = ops.atomic()
        assert _same(do, ado) and _same(dm, adm), kind
        if kind == 'arbitrary':                                         # two runs are bit-identical, in its own workspace too
            ws = torch.empty(H.dcn_bwd_data_det_workspace_bytes(n, cin, h, w) + 64, dtype=torch.uint8, device=cuda).fill_(0xa5)
            dx2, do2, dm2 = ops.det(workspace=ws)
            assert torch.equal(dx.buf, dx2.buf) and torch.equal(do.buf, do2.buf) and torch.equal(dm.buf, dm2.buf)
            assert bool((ws[-64:] == 0xa5).all())


@pytest.mark.parametrize('case', [(5, 7, 16, 1, 3, False), (33, 40, 64, 8, 3, True), (33, 40, 24, 3, 3, False)], ids=_cid)
def test_an_image_of_a_batch_equals_the_image_alone(cuda, case):
    h, w, cin, dg, n, logit = case
    rng, dcol, mask_in = M.case_data(h, w, cin, dg, n, logit)
    dcol = dcol.copy()
    dcol[0] *= np.float32(2.0 ** 20)                                    # the neighbours' scales differ: they must not matter
    dcol[2] *= np.float32(2.0 ** -20)
    offset = M.offsets_of('arbitrary', rng, n, dg, h, w)
    whole = _f32(Operands(cuda, dcol, offset, mask_in, dg, logit).det()[0], cin)
    for i in range(n):
        alone = _f32(Operands(cuda, dcol[i:i + 1], offset[i:i + 1], mask_in[i:i + 1], dg, logit).det()[0], cin)
        assert _bits_equal(whole[i:i + 1], alone), i


@pytest.mark.parametrize('case', [(5, 7, 16, 1, 3, True), (5, 7, 24, 3, 1, False), (33, 40, 64, 8, 3, False), (33, 40, 8, 1, 1, True)],
                         ids=_cid)
def test_scaled_zero_and_nan_gradients(cuda, case):
    """dcol scaled by 2^100 and by 2^-100, all zero (dx == 0 over the SENTINEL prefill) and holding one NaN (that image's dx is NaN,
    the others are unaffected) — the model bit for bit; doffset / dmask stay the atomic entry point's."""
    h, w, cin, dg, n, logit = case
    rng, dcol0, mask_in = M.case_data(h, w, cin, dg, n, logit)
    m = None
    for kind in ('dyadic', 'onecell'):
        offset = M.offsets_of(kind, rng, n, dg, h, w)
        for name, dcol in M.dcol_variants(dcol0).items():
            ops = Operands(cuda, dcol, offset, mask_in, dg, logit)
            m = ops.mask_values(mask_in) if m is None else m
            dx, do, dm = ops.det()
            _kept(dx, do, dm, dg, f'{_cid(case)} {kind} {name}')
            model, info = M.det_dx(dcol, offset, m, dg, logit, mask_in)
            got = _f32(dx, cin)
            assert _bits_equal(np.nan_to_num(got, nan=7.0), np.nan_to_num(model, nan=7.0)) and np.array_equal(np.isnan(got), np.isnan(model)), \
                (kind, name)
            states = [r['state'] for r in info]
            if name in ('zero', 'mixed'):
                assert states[-1 if name == 'zero' else 2] == 'zero' and not got[-1 if name == 'zero' else 2].any()
            if name == 'nan':
                assert states[n - 1] == 'nan' and np.isnan(got[n - 1]).all() and np.isfinite(got[:n - 1]).all()
            if name in ('big', 'mixed'):
                assert float(np.abs(got[0]).max()) > 2.0 ** 90
            _, ado, adm = ops.atomic()
            assert _same(do, ado) and _same(dm, adm), (kind, name)


def test_a_nan_logit_or_a_zero_raw_mask(cuda):
    h, w, cin, dg, n = 5, 7, 16, 1, 3
    rng, dcol, logits = M.case_data(h, w, cin, dg, n, True)
    offset = M.offsets_of('dyadic', rng, n, dg, h, w)
    logits = logits.copy()
    logits[1, 3, 2, 2] = np.nan
    got = _f32(Operands(cuda, dcol, offset, logits, dg, True).det()[0], cin)
    assert np.isnan(got[1]).all() and np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    raw = logits.copy()
    raw[1] = 0.0
    raw[2, 4, 1, 1] = np.inf
    got = _f32(Operands(cuda, dcol, offset, raw, dg, False).det()[0], cin)
    assert np.isfinite(got[0]).all() and got[0].any() and not got[1].any() and np.isnan(got[2]).all()


def test_dx_alone_and_gradients_alone(cuda):
    """dx without doffset / dmask, and doffset / dmask without dx (no workspace needed): the same bits as together."""
    h, w, cin, dg, n, logit = 33, 40, 24, 3, 3, True
    rng, dcol, mask_in = M.case_data(h, w, cin, dg, n, logit)
    ops = Operands(cuda, dcol, M.offsets_of('arbitrary', rng, n, dg, h, w), mask_in, dg, logit)
    dx, do, dm = ops.det()
    dx1, do1, dm1 = ops.outputs()
    H.dcn_bwd_data_det(ops.dcol, ops.x, ops.off, ops.mask, dg, mask_is_logit=logit, dx=dx1)
    assert H.dcn_bwd_data_det(ops.dcol, ops.x, ops.off, ops.mask, dg, mask_is_logit=logit, want_dx=False, doffset=do1, dmask=dm1) is None
    torch.cuda.synchronize()
    assert torch.equal(dx.buf, dx1.buf) and torch.equal(do.buf, do1.buf) and torch.equal(dm.buf, dm1.buf)
    fresh = H.dcn_bwd_data_det(ops.dcol, ops.x, ops.off, ops.mask, dg, mask_is_logit=logit)     # a new tensor: torch.empty, stored
    assert torch.equal(fresh.buf, dx.buf[:, dx.cb0:dx.cb0 + dx.cbn])


@pytest.mark.parametrize('case', [(5, 7, 16, 1, 3, False), (33, 40, 64, 8, 1, True), (33, 40, 24, 3, 3, True), (1, 1, 8, 1, 3, False)],
                         ids=_cid)
def test_the_atomic_dx_is_within_its_own_bound_of_the_deterministic_one(cuda, case):
    """sr_dcn_bwd_data_f32's dx against the deterministic dx under the bound tests/test_dcn_ops_gpu.py holds it to against float64:
    (J + 2 (+ K_SIGMOID)) EPS on the scatter of absolute values + EPS |ref|, J the largest number of adds to one element."""
    h, w, cin, dg, n, logit = case
    rng, dcol, mask_in = M.case_data(h, w, cin, dg, n, logit)
    for kind in ('dyadic', 'arbitrary', 'onecell'):
        offset = M.offsets_of(kind, rng, n, dg, h, w)
        ops = Operands(cuda, dcol, offset, mask_in, dg, logit)
        det, atomic = _nchw(ops.det()[0], cin), _nchw(ops.atomic()[0], cin)
        off64 = torch.from_numpy(M.exact_offsets(offset, dg))
        mval = torch.sigmoid(_t(mask_in)) if logit else _t(mask_in)
        g = _t(dcol).permute(0, 2, 1, 3, 4).contiguous()
        xa = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)
        Ax, = torch.autograd.grad(R.columns(xa, off64, mval.abs(), dg), xa, g.abs())
        J, = torch.autograd.grad(R.columns(xa, off64, torch.ones_like(mval), dg, corner_weights='ones'), xa, torch.ones_like(g))
        k = int(J.max()) + 2 + (K_SIGMOID if logit else 0)
        _check(atomic, det, k * EPS * Ax, f'atomic dx against the deterministic one {_cid(case)} {kind}')
