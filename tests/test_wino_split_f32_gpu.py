"""The split of the Winograd fp32 kernel (csrc/conv_wino_f32.hip) over two waves per patch row, at the smallest shapes where it can
go wrong, through the development hooks sr_dev_conv3x3_wino_pack_f32 and sr_dev_conv3x3_wino_f32.

A patch row's 16 transform points are split by transform row: the "low" wave holds rows 0, 1 and stores output row dy = 0, the "high"
wave holds rows 2, 3 and stores dy = 1; the row step of the output transform exchanges one transform row each way through LDS behind a
barrier.  The bound, the float64 reference and the spike are those of tests/test_wino_f32_gpu.py (imported, not restated), whose
cases start at 8 chunks of 8 input channels; here:

  * 1, 2 and 3 chunks: the peeled prologue and tail of the chunk loop (no steady-state chunk at all below 3);
  * odd H and W: a tile's last patch row is half outside the image, so the low wave stores and its high partner must not; the
    17 x 64 case ends on a patch row whose raw rows d2, d3 (all the high half adds to its first transform row) lie outside;
  * 96 couts: three 32-cout groups, both residuals;
  * the nearest x2 source map with one chunk;
  * every tile variant (sr_dev_set_wino_f32(2 | 3 | 4): 8, 4, 2 waves per workgroup) and the default choice: inside the bound,
    sentinels around the destination slice intact, source unchanged, all four bit-equal;
  * the same launch 20 times into fresh buffers (NW = 4 and 2): bit-equal, which a missing barrier around the exchange would break.
"""
import ctypes as C
import os
import sys

import pytest
import torch

from image_restoration_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_wino_f32_gpu import (SENTINEL, WINO_IDS, _case_id, _from_cb8, _pack, _profiled, _ptr, _st, _stride, _to_cb8,  # noqa: E402
                               lib, reference)  # noqa: F401  (lib is a fixture)

pytestmark = pytest.mark.gpu

CASES = [
    (1, 8, 32, 5, 67, dict(slope=0.2)),                            # 1 chunk, two column tiles, odd H and W
    (2, 16, 32, 3, 65, dict(concat=True)),                         # 2 chunks, channel slices of one buffer
    (1, 24, 96, 17, 64, dict(alpha=0.04, res1=0.2, res2=1.0)),     # 3 chunks, three cout groups, both residuals, three row tiles
    (1, 8, 32, 3, 35, dict(slope=0.2, upsample=True)),             # nearest x2 source map: 6 x 70 output
]
REPEAT_CASE = CASES[2]


@pytest.fixture(scope='module')
def refs():
    """case id -> reference(case), computed once for the module and never changed."""
    return {_case_id(c): reference(c) for c in CASES}


class Launch:
    """One case on the device: weight image, bias and residual buffers made once; run(mode) launches into fresh buffers."""

    def __init__(self, lib, case, ref, dev):
        self.lib, self.case, self.dev = lib, case, dev
        n, cin, cout, h, w, o = case
        self.x, wt, bias, res = ref[0], ref[1], ref[2], ref[3]
        self.image = _pack(lib, wt, dev)
        self.bias = bias.float().to(dev)
        self.res = {name: _to_cb8(r, cout // 8 + 1, 1, dev) for name, r in res.items()}

    def run(self, mode):
        """(whole destination buffer, its first destination block, whole source buffer after the launch, source before, ids)."""
        n, cin, cout, h, w, o = self.case
        up = o.get('upsample', False)
        H, W = (2 * h, 2 * w) if up else (h, w)
        sb, db = cin // 8, cout // 8
        d = _lib.ConvDesc()
        if o.get('concat', False):   # [sentinel | source | destination | sentinel] blocks of one buffer
            buf = _to_cb8(self.x, 1 + sb + db + 1, 1, self.dev)
            src, src_cb, dst, dst_cb = buf, 1, buf, 1 + sb
        else:
            src, src_cb = _to_cb8(self.x, sb + 2, 1, self.dev), 1
            dst, dst_cb = torch.full((n, db + 2, H, W, 8), SENTINEL, dtype=torch.float32, device=self.dev), 1
        before = src.cpu()
        d.in_, d.in_img_stride, d.cin_pad, d.cin_real, d.in_h, d.in_w = _ptr(src, src_cb), _stride(src), cin, cin, h, w
        d.upsample = int(up)
        d.wpacked, d.bpacked, d.cout = self.image.data_ptr(), self.bias.data_ptr(), cout
        d.out, d.out_img_stride = _ptr(dst, dst_cb), _stride(dst)
        d.n, d.act_slope, d.alpha = n, o.get('slope', 1.0), o.get('alpha', 1.0)
        for name, rb in self.res.items():
            setattr(d, name, _ptr(rb, 1))
            setattr(d, name + '_img_stride', _stride(rb))
            setattr(d, 'beta' + name[-1], o[name])
        self.lib.sr_dev_set_wino_f32(mode)
        ids = _profiled(self.lib, lambda: _lib.check(self.lib.sr_dev_conv3x3_wino_f32(C.byref(d), self.image.data_ptr(), _st()),
                                                     'wino conv'))
        torch.cuda.synchronize()
        return dst.cpu(), dst_cb, src.cpu(), before, ids


@pytest.mark.parametrize('case', CASES, ids=[_case_id(c) for c in CASES])
def test_split_against_float64_on_every_variant(cuda, lib, refs, case):
    n, cin, cout, h, w, o = case
    ref = refs[_case_id(case)]
    y64, bound, y_ns = ref[4], ref[5], ref[6]
    ratio = ((y64 - y_ns)[-1:].abs() / bound[-1:])
    assert float(ratio.max()) > 4.0, ('the spike does not reach four bounds', float(ratio.max()))
    sb, db = cin // 8, cout // 8
    concat = o.get('concat', False)
    launch = Launch(lib, case, ref, cuda)
    outs = {}
    try:
        for mode in (1, 2, 3, 4):
            out, dst_cb, src_after, src_before, ids = launch.run(mode)
            if mode == 1:
                assert len(ids) == 1 and ids[0] in WINO_IDS.values(), ids
            else:
                assert ids == [WINO_IDS[mode]], (mode, ids)
            got = _from_cb8(out, dst_cb, cout)
            err = (got - y64).abs()
            bad = err > bound
            print(f'{_case_id(case)} mode {mode}: max err / bound {float((err / bound).max()):.4f}, max err {float(err.max()):.3e}')
            assert not bool(bad.any()), (mode, int(bad.sum()), float((err / bound).max()), float(err.max()))
            assert bool((out[:, :dst_cb - sb if concat else dst_cb] == SENTINEL).all()), f'mode {mode} wrote below its channel slice'
            assert bool((out[:, dst_cb + db:] == SENTINEL).all()), f'mode {mode} wrote above its channel slice'
            if concat:   # source and destination share the buffer: compare the source blocks and the sentinel in front of them
                assert torch.equal(src_after[:, :1 + sb], src_before[:, :1 + sb]), f'mode {mode} changed its source'
            else:
                assert torch.equal(src_after, src_before), f'mode {mode} changed its source'
            outs[mode] = out
        for mode in (2, 3, 4):
            assert torch.equal(outs[mode], outs[1]), f'variant {mode} differs from the default choice'
    finally:
        lib.sr_dev_set_wino_f32(1)


@pytest.mark.parametrize('mode', [2, 3], ids=['nw4', 'nw2'])
def test_split_is_repeatable(cuda, lib, refs, mode):
    """20 launches of the three-row-tile, three-cout-group case into fresh buffers: equal bits every time."""
    launch = Launch(lib, REPEAT_CASE, refs[_case_id(REPEAT_CASE)], cuda)
    try:
        first = launch.run(mode)[0]
        assert bool(torch.isfinite(first[:, 1:-1]).all())
        for i in range(19):
            assert torch.equal(launch.run(mode)[0], first), f'launch {i + 2} differs from the first'
    finally:
        lib.sr_dev_set_wino_f32(1)
