"""The Winograd F(2x2,3x3) fp32 convolution (csrc/conv_wino_f32.hip) through its development hooks, and the inference forward with
the switch on against the switch off.

Kernel bound, in the style of tests/test_conv_ops_gpu.py.  EPS = 2^-24.  For every output element let A be the SAME Winograd
pipeline on absolute values in float64,

    A0 = |A^T| [ sum_cin (|G| |g| |G|^T) . (|B^T| |d| |B|) ] |A|,    A = |alpha| (A0 + |bias|) + |beta1 r1| + |beta2 r2|.

Then |y - y64| <= k EPS A + EPS |y64| with k = 2 cin_pad + 8 + 8: two roundings per product of the MFMA sum over cin_pad channels
(one sum per transform point); 8 = three roundings in the input transform (two levels of adds and the operand itself), one for
U = G g G^T (float64, rounded once) and four in the output transform (two levels of two adds); 8 for the epilogue (bias,
activation, alpha, two residual multiply-adds), as in the direct kernels' bound.  A is about seven times the direct convolution's A
(the absolute transforms do not cancel), so this is a bound with room, not a fit.

Sensitivity is asserted: every case plants the existing suite's spike at the border pixel (0, 0) of the last input channel of the
last image, weighted by a corner tap of +-1/2; its contribution must exceed four bounds at an output it reaches.

Every forced tile variant (sr_dev_set_wino_f32(2 | 3 | 4): 4, 2, 1 patch rows per workgroup) runs every case and gives the bits of
the default choice.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_restoration_amd as ira
from image_restoration_amd import _lib
from image_restoration_amd.utils import synth

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
TINY = 1e-30
SENTINEL = 12345.0
NOT_ELIGIBLE = 1
WINO_IDS = {2: 106, 3: 107, 4: 108}

BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


@pytest.fixture(scope='module')
def lib():
    lib = _lib.load()
    lib.sr_dev_set_wino_f32.argtypes = [C.c_int]
    lib.sr_dev_set_wino_f32.restype = C.c_int
    lib.sr_dev_conv3x3_wino_f32.argtypes = [C.POINTER(_lib.ConvDesc), C.c_void_p, C.c_void_p]
    lib.sr_dev_conv3x3_wino_f32.restype = C.c_int
    lib.sr_dev_conv3x3_wino_pack_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.sr_dev_conv3x3_wino_pack_f32.restype = C.c_int
    lib.sr_dev_conv3x3_wino_pack_bytes.argtypes = [C.c_int, C.c_int]
    lib.sr_dev_conv3x3_wino_pack_bytes.restype = C.c_size_t
    yield lib
    lib.sr_dev_set_wino_f32(1)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _profiled(lib, fn):
    _lib.check(lib.sr_profile_start(1024), 'sr_profile_start')
    try:
        fn()
    finally:
        recs = (_lib.LaunchRecord * 1024)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, 1024, C.byref(cnt)), 'sr_profile_stop')
    return [recs[i].kernel_id for i in range(min(cnt.value, 1024))]


def _f32(a):
    return a.float().double()


def _rand(rng, shape):
    return _f32(torch.from_numpy(rng.standard_normal(shape)))


def _to_cb8(x, blocks, cb0, dev, fill=SENTINEL):
    n, c, h, w = x.shape
    nb = (c + 7) // 8
    buf = torch.full((n, blocks, h, w, 8), fill, dtype=torch.float32)
    xp = torch.zeros((n, nb * 8, h, w), dtype=torch.float64)
    xp[:, :c] = x
    buf[:, cb0:cb0 + nb] = xp.reshape(n, nb, 8, h, w).permute(0, 1, 3, 4, 2).float()
    return buf.to(dev)


def _from_cb8(buf, cb0, c):
    n, _, h, w, _ = buf.shape
    nb = (c + 7) // 8
    return buf[:, cb0:cb0 + nb].cpu().double().permute(0, 1, 4, 2, 3).reshape(n, nb * 8, h, w)[:, :c]


def _ptr(buf, cb0):
    return buf.data_ptr() + cb0 * buf.shape[2] * buf.shape[3] * 8 * 4


def _stride(buf):
    return buf.shape[1] * buf.shape[2] * buf.shape[3] * 8


def wino_abs(x, wt):
    """|A^T| [sum_cin (|G||g||G|^T) . (|B^T||d||B|)] |A| in float64: x [n][cin][H][W] (already upsampled), wt [cout][cin][3][3];
    patches anchored at even coordinates, zeros beyond the image."""
    n, cin, H, W = x.shape
    ph, pw = (H + 1) // 2, (W + 1) // 2
    xp = torch.zeros((n, cin, 2 * ph + 2, 2 * pw + 2), dtype=torch.float64)
    xp[:, :, 1:H + 1, 1:W + 1] = x.abs()
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                     # [n][cin][ph][pw][4][4]
    v = torch.einsum('ia,ncpqab,jb->ncpqij', BT.abs(), d, BT.abs())
    u = torch.einsum('ia,ocab,jb->ocij', G.abs(), wt.abs(), G.abs())            # [cout][cin][4][4]
    m = torch.einsum('ocij,ncpqij->nopqij', u, v)
    y = torch.einsum('ia,nopqab,jb->nopqij', AT.abs(), m, AT.abs())             # [n][cout][ph][pw][2][2]
    return y.permute(0, 1, 2, 4, 3, 5).reshape(n, -1, 2 * ph, 2 * pw)[:, :, :H, :W]


# (n, cin, cout, h, w, options): odd sizes both ways with channel slices of one concat buffer; two tiles each way for every tile
# shape (tiles are 8 | 4 | 2 rows x 64 columns) with both residuals; the nearest x2 source map; images smaller than a patch row
CASES = [
    (2, 96, 32, 13, 37, dict(slope=0.2, concat=True)),
    (2, 192, 64, 20, 70, dict(alpha=0.04, res1=0.2, res2=1.0)),
    (1, 64, 64, 9, 7, dict(slope=0.2, upsample=True)),
    (3, 64, 32, 2, 2, dict()),
    (1, 64, 32, 1, 5, dict()),
]


def _case_id(c):
    return f'n{c[0]}-{c[1]}to{c[2]}-{c[3]}x{c[4]}' + ''.join('-' + k for k in sorted(c[5]))


def reference(case):
    """(x with the spike, wt, bias, residuals, y64, bound, y64 without the spike): everything the device run is compared with."""
    n, cin, cout, h, w, o = case
    rng = np.random.default_rng(sum(map(ord, _case_id(case))))
    up = o.get('upsample', False)
    slope, alpha = o.get('slope', 1.0), o.get('alpha', 1.0)
    H, W = (2 * h, 2 * w) if up else (h, w)
    wt = _rand(rng, (cout, cin, 3, 3)) * 0.125
    wt[:, -1, 0, 0] = torch.from_numpy(np.where(rng.random(cout) < 0.5, -0.5, 0.5))
    bias = _rand(rng, (cout,)) * 0.5
    res = {name: _rand(rng, (n, cout, H, W)) for name in ('res1', 'res2') if name in o}
    k = 2 * cin + 8 + 8  # cin is a multiple of 8 in every case: cin_pad = cin

    def y_of(x):
        xu = F.interpolate(x, scale_factor=2, mode='nearest') if up else x
        c = F.conv2d(xu, wt, bias, padding=1)
        v = torch.where(c > 0, c, slope * c) * alpha
        A = abs(alpha) * (wino_abs(xu, wt) + bias.abs().view(1, -1, 1, 1))
        for name, r in res.items():
            v = v + o[name] * r
            A = A + abs(o[name]) * r.abs()
        return v, A

    x = _rand(rng, (n, cin, h, w))
    y0, A0 = y_of(x)
    # the spike reaches output (1 - ty, 1 - tx) through tap (ty, tx) of the last channel, where that output exists
    taps = [(ty, tx) for ty in range(3) for tx in range(3) if 0 <= 1 - ty < H and 0 <= 1 - tx < W]
    wmax = max(float(wt[:, -1, ty, tx].abs().max()) for ty, tx in taps)
    gain = wmax * abs(alpha) * (slope if 0 < slope < 1 else 1.0)
    spike = 8 * (k * EPS * float(A0.max()) + EPS * float(y0.abs().max())) / gain + 4.0
    x[-1, -1, 0, 0] = spike
    y64, A = y_of(x)
    bound = k * EPS * A + EPS * y64.abs() + TINY
    xq = x.clone()
    xq[-1, -1, 0, 0] = 0.0
    return x, wt, bias, res, y64, bound, y_of(xq)[0]


def _pack(lib, wt, dev):
    cout, cin = wt.shape[:2]
    nbytes = lib.sr_dev_conv3x3_wino_pack_bytes(cout, cin)
    assert nbytes > 0
    image = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    wdev = wt.float().contiguous().to(dev)
    _lib.check(lib.sr_dev_conv3x3_wino_pack_f32(wdev.data_ptr(), cout, cin, cin, 0, image.data_ptr(), _st()), 'wino pack')
    torch.cuda.synchronize()
    return image


@pytest.mark.parametrize('case', CASES, ids=[_case_id(c) for c in CASES])
def test_wino_conv_against_float64(cuda, lib, case):
    n, cin, cout, h, w, o = case
    up = o.get('upsample', False)
    H, W = (2 * h, 2 * w) if up else (h, w)
    x, wt, bias, res, y64, bound, y_ns = reference(case)
    ratio = ((y64 - y_ns)[-1:].abs() / bound[-1:])
    assert float(ratio.max()) > 4.0, ('the spike does not reach four bounds', float(ratio.max()))

    image = _pack(lib, wt, cuda)
    bdev = bias.float().to(cuda)
    sb, db = cin // 8, cout // 8
    concat = o.get('concat', False)
    keep = []

    def run(mode):
        """One launch under sr_dev_set_wino_f32(mode) into fresh buffers; returns (whole destination buffer on the CPU, ids)."""
        d = _lib.ConvDesc()
        if concat:  # [sentinel | source | destination | sentinel] blocks of one buffer
            buf = _to_cb8(x, 1 + sb + db + 1, 1, cuda)
            src, src_cb, dst, dst_cb = buf, 1, buf, 1 + sb
        else:
            src, src_cb = _to_cb8(x, sb, 0, cuda), 0
            dst, dst_cb = torch.full((n, db + 2, H, W, 8), SENTINEL, dtype=torch.float32, device=cuda), 1
        d.in_, d.in_img_stride, d.cin_pad, d.cin_real, d.in_h, d.in_w = _ptr(src, src_cb), _stride(src), cin, cin, h, w
        d.upsample = int(up)
        d.wpacked, d.bpacked, d.cout = image.data_ptr(), bdev.data_ptr(), cout
        d.out, d.out_img_stride = _ptr(dst, dst_cb), _stride(dst)
        d.n, d.act_slope, d.alpha = n, o.get('slope', 1.0), o.get('alpha', 1.0)
        for name, r in res.items():
            rb = _to_cb8(r, db + 1, 1, cuda)
            keep.append(rb)
            setattr(d, name, _ptr(rb, 1))
            setattr(d, name + '_img_stride', _stride(rb))
            setattr(d, 'beta' + name[-1], o[name])
        lib.sr_dev_set_wino_f32(mode)
        ids = _profiled(lib, lambda: _lib.check(lib.sr_dev_conv3x3_wino_f32(C.byref(d), image.data_ptr(), _st()), 'wino conv'))
        torch.cuda.synchronize()
        return dst.cpu(), dst_cb, ids

    try:
        out, dst_cb, ids = run(1)
        assert len(ids) == 1 and ids[0] in WINO_IDS.values(), ids
        got = _from_cb8(out, dst_cb, cout)
        err = (got - y64).abs()
        bad = err > bound
        print(f'{_case_id(case)}: max err / bound {float((err / bound).max()):.4f}, max err {float(err.max()):.3e}')
        assert not bool(bad.any()), (int(bad.sum()), float((err / bound).max()), float(err.max()))
        assert bool((out[:, :dst_cb - sb if concat else dst_cb] == SENTINEL).all()), 'wrote below its channel slice'
        assert bool((out[:, dst_cb + db:] == SENTINEL).all()), 'wrote above its channel slice'
        if concat:
            assert torch.equal(out[:, 1:1 + sb], _to_cb8(x, sb, 0, 'cpu')), 'changed its source'
        for mode, kid in WINO_IDS.items():
            out_v, _, ids_v = run(mode)
            assert ids_v == [kid], (mode, ids_v)
            assert torch.equal(out_v, out), f'variant {mode} differs from the default choice'
    finally:
        lib.sr_dev_set_wino_f32(1)


def test_not_eligible_descriptors_launch_nothing(cuda, lib):
    x = torch.zeros((1, 8, 6, 6, 8), dtype=torch.float32, device=cuda)
    out = torch.full((1, 8, 6, 6, 8), SENTINEL, dtype=torch.float32, device=cuda)
    image = torch.zeros(64 * 64 * 16, dtype=torch.float32, device=cuda)

    def desc(cin_pad, cin_real, cout, **kw):
        d = _lib.ConvDesc()
        d.in_, d.in_img_stride, d.cin_pad, d.cin_real, d.in_h, d.in_w = x.data_ptr(), _stride(x), cin_pad, cin_real, 6, 6
        d.wpacked, d.cout, d.out, d.out_img_stride = image.data_ptr(), cout, out.data_ptr(), _stride(out)
        d.n, d.act_slope, d.alpha = 1, 1.0, 1.0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    cases = {'cin 3': desc(8, 3, 32), 'cout 3': desc(64, 64, 3), 'cout 20': desc(64, 64, 20),
             'accumulate': desc(64, 64, 32, accumulate=1),
             'mask': desc(64, 64, 32, mask_src=x.data_ptr(), mask_img_stride=_stride(x), mask_cbn=4, mask_slope=0.2),
             'nchw': desc(64, 64, 32, out_nchw=1)}
    for name, d in cases.items():
        rcs = []
        ids = _profiled(lib, lambda: rcs.append(lib.sr_dev_conv3x3_wino_f32(C.byref(d), image.data_ptr(), _st())))
        assert rcs == [NOT_ELIGIBLE] and ids == [], (name, rcs, ids)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    ok = desc(64, 64, 32)  # the same descriptor without the excluded option is taken
    assert lib.sr_dev_conv3x3_wino_f32(C.byref(ok), image.data_ptr(), _st()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ network
CFG = dict(num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=2, num_grow_ch=32)


def _net(dev):
    net = ira.build_network(dict(type='RRDBNet', **CFG)).to(dev).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.rrdbnet_state_dict(0, **CFG).items()}, strict=True)
    return net


@pytest.fixture(scope='module')
def net(cuda):
    return _net(cuda)


@pytest.fixture(scope='module')
def oracle64():
    """float64 reference of the two network shapes, computed once."""
    from oracle import rrdbnet_ref as R
    sd = {k: torch.from_numpy(v).double() for k, v in synth.rrdbnet_state_dict(0, **CFG).items()}
    out = {}
    for shape in ((2, 3, 24, 40), (1, 3, 13, 37)):
        x = synth.uniform_input(1234, shape)
        with torch.no_grad():
            out[shape] = (x, R.rrdbnet_forward(torch.from_numpy(x).double(), sd, 4, CFG['num_block']).numpy())
    return out


@pytest.mark.parametrize('shape', [(2, 3, 24, 40), (1, 3, 13, 37)], ids=['2x24x40', '1x13x37'])
def test_network_switch_on_against_switch_off(cuda, lib, net, oracle64, shape):
    """err_on < 1e-4 (the tolerance the project holds) and err_on <= 4 err_off + 2^-20: the worst-case amplification A_wino / A_direct
    is about 7, a simulated fp32 pipeline measured 0.76-0.87.  Maps of this size are below the size at which the forward takes the
    Winograd kernel on its own (128 x 128 output pixels), so the switch is on with a forced tile variant: every eligible conv then
    runs it, which the launch profiler proves."""
    x, ref = oracle64[shape]
    xd = torch.from_numpy(x).to(cuda)

    def run(mode):
        lib.sr_dev_set_wino_f32(mode)
        with torch.no_grad():
            net(xd)  # packs the weights outside the profiled call
            ids = _profiled(lib, lambda: net(xd))
            y = net(xd)
        torch.cuda.synchronize()
        return y.cpu().numpy().astype(np.float64), ids

    try:
        y_off, ids_off = run(0)
        assert not set(ids_off) & set(WINO_IDS.values()), ids_off
        err_off = float(np.abs(y_off - ref).max())
        for mode in (2, 4):
            y_on, ids_on = run(mode)
            assert ids_on.count(WINO_IDS[mode]) == 5 * 3 * CFG['num_block'] + 4, ids_on  # dense blocks, conv_body, up1, up2, hr
            err_on = float(np.abs(y_on - ref).max())
            print(f'{shape} mode {mode}: err_off {err_off:.3e} err_on {err_on:.3e} ratio {err_on / err_off:.3f}')
            assert err_on < 1e-4, (err_on, err_off)
            assert err_on <= 4 * err_off + 2.0 ** -20, (err_on, err_off)
    finally:
        lib.sr_dev_set_wino_f32(1)


def test_network_default_switch_takes_winograd_at_size(cuda, lib, net):
    """The default setting on one 128 x 128 image: the forward's own choice, by the size of one image, is the Winograd kernel for all
    34 eligible convs, whatever the batch; batch and single image give the same bits."""
    xd = torch.from_numpy(synth.uniform_input(7, (3, 3, 128, 128))).to(cuda)
    lib.sr_dev_set_wino_f32(1)
    with torch.no_grad():
        y = net(xd)
        ids = _profiled(lib, lambda: net(xd[1:2]))
        y1 = net(xd[1:2])
    assert sum(ids.count(k) for k in WINO_IDS.values()) == 5 * 3 * CFG['num_block'] + 4, ids
    assert torch.equal(y[1:2], y1)


def test_independence_of_batch_run_and_profiling(cuda, lib, net):
    """Batch 5 of 24 x 70 against image 3 alone, two runs, and a run under the launch profiler: equal bits (forced variant, so that
    the Winograd kernel runs at this size; the batch of 5 and the single image still get different grids)."""
    xd = torch.from_numpy(synth.uniform_input(99, (5, 3, 24, 70))).to(cuda)
    try:
        for mode in (2, 3):
            lib.sr_dev_set_wino_f32(mode)
            with torch.no_grad():
                y = net(xd)
                y2 = net(xd)
                y3 = net(xd[3:4])
                box = []
                ids = _profiled(lib, lambda: box.append(net(xd)))
            assert WINO_IDS[mode] in ids
            assert torch.equal(y, y2)
            assert torch.equal(y[3:4], y3)
            assert torch.equal(y, box[0])
            assert bool(torch.isfinite(y).all())
        lib.sr_dev_set_wino_f32(1)  # the default choice takes its variant by launch size: same bits as any forced variant
        with torch.no_grad():
            big = torch.from_numpy(synth.uniform_input(5, (2, 3, 128, 128))).to(cuda)
            y_auto = net(big)
            lib.sr_dev_set_wino_f32(4)
            assert torch.equal(y_auto, net(big))
    finally:
        lib.sr_dev_set_wino_f32(1)
