"""sr_vsr_prop_input_bwd_det_f32 (include/sr_hip_vsr_det.h) on the GPU: the deterministic step-input adjoint.

dprev against the numpy model of the integer arithmetic (tests/vsr_det_model.py) bit for bit, against the float64 definition under
the header's bound
    |dprev - (before + exact)| <= 2^-24 |before + exact| + d 2^-(k + 1) + 2^-50 sum |terms|
and against the atomic entry point's result within the sum of the two kernels' bounds (each lies within its own bound of the same
float64 value); dflow against the atomic entry point's bit for bit.  Windows sit at a non-zero block offset of wider sentinel
tensors, the flow is a step slice with an image stride, the workspace has a guard behind it.  The flows are the five kinds of
tests/test_vsr_bwd_ops_gpu.py; the gradient also comes with an image scaled by 2^100, one by 2^-100, one all zero and one holding
a NaN."""
import os
import sys

import numpy as np
import pytest
import torch

from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vsr_bwd_ops_gpu as B  # noqa: E402
import vsr_det_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float('nan')
DET_IDS = [180, 181, 182]
GUARD = 0xAB


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('fb', [1, 8, 9])
@pytest.mark.parametrize('shape', [(1, 1), (5, 7), (33, 40)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_prop_input_bwd_det(cuda, lib, shape, fb, n):
    h, w = shape
    rng, prev, g0, before = M.case_data(h, w, fb, n)
    prev_wide = torch.full((n, fb + 2, h, w, 8), NAN, device=cuda)
    prev_wide[:, 1:1 + fb] = B._to_cb8(prev, cuda)
    nbytes = H.vsr_prop_input_bwd_det_workspace_bytes(n, h, w, fb)
    assert nbytes == (64 * n * fb * h * w + 255) // 256 * 256 + (4 * n + 255) // 256 * 256
    before_cb8 = B._to_cb8(before, cuda)
    worst = 0.0
    for kind in B.FLOWS:
        flow = B._flow(kind, rng, n, h, w)
        flows = torch.full((n, 2, 2, h, w), NAN, device=cuda)           # the flow is step 1 of 2: an image stride of 4 h w
        flows[:, 1] = torch.from_numpy(flow).to(cuda)
        for name, g in M.g_variants(g0, n).items():
            if name != 'plain' and kind not in ('smooth', 'samecell'):
                continue                                               # the extra gradients: on a smooth flow and on the one-cell flow
            g_wide = torch.full((n, fb + 3, h, w, 8), NAN, device=cuda)
            g_wide[:, 2:2 + fb] = B._to_cb8(g, cuda)

            def run(want_dprev=True, want_dflow=True, images=slice(0, n), det=True):
                k = images.stop - images.start
                dprev_wide = torch.full((k, fb + 2, h, w, 8), 777.0, device=cuda)
                dprev_wide[:, 1:1 + fb] = before_cb8[images]
                dflows = torch.full((k, 3, 2, h, w), NAN, device=cuda)
                args = (H.CB8(g_wide[images].contiguous(), 2, fb), H.CB8(prev_wide[images].contiguous(), 1, fb), flows[images][:, 1],
                        H.CB8(dprev_wide, 1, fb) if want_dprev else None, dflows[:, 2] if want_dflow else None)
                if det:
                    need = H.vsr_prop_input_bwd_det_workspace_bytes(k, h, w, fb)
                    ws = torch.full((need + 256,), GUARD, dtype=torch.uint8, device=cuda)
                    H.vsr_prop_input_bwd_det(*args, workspace=ws[:need])
                    assert bool((ws[need:] == GUARD).all()), (kind, name)                # nothing behind the workspace
                    if not want_dprev:
                        assert bool((ws == GUARD).all()), (kind, name)                   # and none of it without dprev
                else:
                    H.vsr_prop_input_bwd(*args)
                # nothing outside the destinations; a destination that was not asked for is untouched
                assert bool((dprev_wide[:, 0] == 777.0).all()) and bool((dprev_wide[:, 1 + fb] == 777.0).all()), (kind, name)
                assert bool(torch.isnan(dflows[:, :2]).all()), (kind, name)
                if not want_dprev:
                    assert B._same(dprev_wide[:, 1:1 + fb], before_cb8[images]), (kind, name)
                if not want_dflow:
                    assert bool(torch.isnan(dflows[:, 2]).all()), (kind, name)
                return dprev_wide[:, 1:1 + fb], dflows[:, 2]

            dprev, dflow = run()
            got = B._nchw(dprev)
            # ---- the numpy model, bit for bit
            model, info = M.det_dprev(before, g, flow)
            assert np.array_equal(got.astype(np.float32).view(np.uint32), model.view(np.uint32)), (kind, name)
            # ---- the atomic entry point: dflow bit for bit
            dprev_a, dflow_a = run(det=False)
            assert B._same(dflow, dflow_a), (kind, name)
            # ---- the float64 definition under the header's bound; images that are skipped or poisoned by their own rule
            finite = [i for i in range(n) if 0 < info[i]['bits'] < M.INF_BITS]
            for i in range(n):
                if info[i]['bits'] == 0:
                    assert B._same(dprev[i], before_cb8[i]), (kind, name, i)             # M == 0: untouched
                elif info[i]['bits'] >= M.INF_BITS:
                    assert bool(torch.isnan(dprev[i]).all()), (kind, name, i)            # a non-finite g: NaN everywhere
            if finite:
                gf = np.where(np.isfinite(g), g, 0.0)
                want_dx, _, count, absterms, _ = B._prop_reference(prev, flow, gf)
                bound = M.det_bound(before, want_dx, count, absterms, [info[i]['k'] for i in range(n)])
                err = np.abs(got - (before + want_dx))
                assert (err[finite] <= bound[finite]).all(), (kind, name, float((err[finite] / bound[finite]).max()))
                worst = max(worst, float((err[finite] / bound[finite]).max()))
                # the atomic result lies within its own bound of the same float64 value
                bound_a = (count + 1) * M.U * (np.abs(before) + absterms)
                assert (np.abs(got - B._nchw(dprev_a))[finite] <= (bound + bound_a)[finite]).all(), (kind, name)
                if kind == 'samecell':
                    assert int(count.max()) == h * w
                    assert max(float(info[i]['absacc'].max()) for i in finite) < 2.0 ** 62   # and the integer sum stays in range
            if name != 'plain':
                continue
            # ---- exactly the three launches, in order; one without dprev
            assert B._profiled(lib, lambda: run()) == DET_IDS
            assert B._profiled(lib, lambda: run(want_dprev=False)) == [181]
            # ---- two runs are bit-identical
            dprev2, dflow2 = run()
            assert B._same(dprev2, dprev) and B._same(dflow2, dflow), kind
            # ---- a batch is its images one by one, bit for bit
            if n > 1:
                for i in range(n):
                    dp1, df1 = run(images=slice(i, i + 1))
                    assert B._same(dp1, dprev[i:i + 1]) and B._same(df1, dflow[i:i + 1]), (kind, i)
            # ---- a NULL dprev or a NULL dflow leaves the other result as it was
            _, dflow3 = run(want_dprev=False)
            assert B._same(dflow3, dflow), kind
            dprev3, _ = run(want_dflow=False)
            assert B._same(dprev3, dprev), kind
    print(f'{h}x{w} fb={fb} n={n}: worst dprev error / bound {worst:.3f}')


def test_wrapper_refuses_misfits(cuda):
    g, prev = H.CB8.zeros(1, 16, 4, 5, cuda), H.CB8.zeros(1, 16, 4, 5, cuda)
    flow = torch.zeros((1, 2, 4, 5), device=cuda)
    with pytest.raises(ValueError, match='nothing to compute'):
        H.vsr_prop_input_bwd_det(g, prev, flow)
    with pytest.raises(ValueError, match='dprev does not fit'):
        H.vsr_prop_input_bwd_det(g, prev, flow, dprev=H.CB8.zeros(1, 8, 4, 5, cuda))
    with pytest.raises(ValueError, match='must not be a source'):
        H.vsr_prop_input_bwd_det(g, prev, flow, dprev=prev)
    with pytest.raises(ValueError, match='workspace is too small'):
        H.vsr_prop_input_bwd_det(g, prev, flow, dprev=H.CB8.zeros(1, 16, 4, 5, cuda), workspace=torch.zeros(16, dtype=torch.uint8, device=cuda))
