"""MSRResNet on the MI355X: the two new kernels (CB8 pixel shuffle / unshuffle, NCHW bilinear upsampling and its adjoint)
against torch on the CPU, and the network (forward, backward, SRModel / SRGANModel training, checkpoint, tiling, inference
script) against the reference's own results in tests/golden/g_u_msrresnet.npz (tools/make_golden_msrresnet.py)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_restoration_amd as ira
from image_restoration_amd import _lib, hip_ops
from image_restoration_amd.utils import synth

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24   # unit roundoff of fp32


def _st():
    return torch.cuda.current_stream().cuda_stream


def _profiled(lib, fn, cap=512):
    """Runs fn() under the launch profiler; returns the launch records (kernel id, bytes) in order."""
    _lib.check(lib.sr_profile_start(cap), 'sr_profile_start')
    try:
        fn()
    finally:
        recs = (_lib.LaunchRecord * cap)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, cap, C.byref(cnt)), 'sr_profile_stop')
    return [(recs[i].kernel_id, recs[i].bytes) for i in range(min(cnt.value, cap))]


def _cb8_nan(n, c, h, w, dev):
    return hip_ops.CB8(torch.full((n, (c + 7) // 8, h, w, 8), float('nan'), dtype=torch.float32, device=dev))


# ------------------------------------------------------------------------------------------------------------- shuffle kernels
@pytest.mark.parametrize('r', [2, 3])
@pytest.mark.parametrize('c,n,h,w', [(8, 1, 1, 1), (64, 2, 7, 5), (16, 3, 9, 13), (3, 2, 5, 3), (13, 1, 11, 6)])
def test_pixel_shuffle_and_unshuffle_are_bit_exact_permutations(cuda, r, c, n, h, w):
    """Pure moves: bit for bit against torch's pixel_shuffle / pixel_unshuffle on the CPU.  The destinations start as NaN,
    so every destination value, pad channels included (c % 8 != 0 in two cases), is written by the kernel; pads are 0."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(100 * r + c)
    x = torch.randn(n, c * r * r, h, w, generator=g)
    src = hip_ops.nchw_to_cb8(x.to(cuda))
    dst = _cb8_nan(n, c, h * r, w * r, cuda)
    ids = _profiled(lib, lambda: _lib.check(lib.sr_cb8_pixel_shuffle_f32(src.ptr, src.img_stride, dst.ptr, dst.img_stride, n, c, h, w,
                                                                          r, _st()), 'shuffle'))
    assert [i for i, _ in ids] == [70]
    y = dst.buf.permute(0, 1, 4, 2, 3).reshape(n, -1, h * r, w * r)
    assert torch.equal(y[:, :c].cpu(), F.pixel_shuffle(x, r))
    assert torch.count_nonzero(y[:, c:]) == 0 and not torch.isnan(y).any()
    # inverse: back to the source layout, against pixel_unshuffle
    back = _cb8_nan(n, c * r * r, h, w, cuda)
    ids = _profiled(lib, lambda: _lib.check(lib.sr_cb8_pixel_unshuffle_f32(dst.ptr, dst.img_stride, back.ptr, back.img_stride, n, c, h, w,
                                                                            r, _st()), 'unshuffle'))
    assert [i for i, _ in ids] == [71]
    z = back.buf.permute(0, 1, 4, 2, 3).reshape(n, -1, h, w)
    assert torch.equal(z[:, :c * r * r].cpu(), F.pixel_unshuffle(F.pixel_shuffle(x, r), r))
    assert torch.equal(z[:, :c * r * r].cpu(), x)
    assert torch.count_nonzero(z[:, c * r * r:]) == 0 and not torch.isnan(z).any()


def test_shuffle_rejects_bad_arguments(cuda):
    lib = _lib.load()
    a = hip_ops.CB8.zeros(1, 32, 4, 4, cuda)
    b = hip_ops.CB8.zeros(1, 8, 8, 8, cuda)
    assert lib.sr_cb8_pixel_shuffle_f32(a.ptr, a.img_stride, b.ptr, b.img_stride, 1, 8, 4, 4, 4, _st()) == -1
    assert lib.sr_cb8_pixel_shuffle_f32(a.ptr, a.img_stride - 8, b.ptr, b.img_stride, 1, 8, 4, 4, 2, _st()) == -1
    assert lib.sr_bilinear_up_f32(a.ptr, b.ptr, 1, 1, 4, 4, 5, 0, _st()) == -1


# ------------------------------------------------------------------------------------------------------------ bilinear kernels
BILINEAR_CASES = [(2, 2, 3, 7, 9), (3, 1, 3, 9, 11), (4, 2, 3, 13, 17), (2, 1, 2, 1, 5), (3, 2, 1, 4, 1), (4, 1, 3, 1, 1),
                  (3, 1, 3, 40, 36)]


def _bilinear_bound(x, s, h, w):
    """Each output is l0y*(l0x*a + l1x*b) + l1y*(l0x*c + l1x*d) with l0 = 1 - l1 in fp32.  The 7 roundings of the products
    and sums cost <= 7u * max|x|.  The weights carry the error of the source index: inv_s*(o + 0.5) - 0.5 is formed with
    inv_s = fl(1/s) (exact for s = 2, 4; relative error u for s = 3) and two roundings of a value < max(h, w), so
    |lambda - lambda_exact| <= 3u*max(h, w), and each weight error moves the result by at most that times the spread of the
    two neighbours (<= 2 max|x|), in both directions.  Bound: (7 + 12 max(h, w)) u max|x|."""
    return (7 + 12 * max(h, w)) * U32 * float(x.abs().max())


@pytest.mark.parametrize('s,n,c,h,w', BILINEAR_CASES)
def test_bilinear_up_matches_float64_interpolate(cuda, s, n, c, h, w):
    lib = _lib.load()
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(s * 1000 + h * 10 + w))
    ref = F.interpolate(x.double(), scale_factor=s, mode='bilinear', align_corners=False)
    out = torch.full((n, c, h * s, w * s), float('nan'), device=cuda)
    ids = _profiled(lib, lambda: hip_ops.bilinear_up(x.to(cuda), s, out=out.zero_()))
    assert [i for i, _ in ids] == [72]
    y = hip_ops.bilinear_up(x.to(cuda), s)
    err = float((y.cpu().double() - ref).abs().max())
    assert err <= _bilinear_bound(x, s, h, w), (err, _bilinear_bound(x, s, h, w))
    assert torch.equal(out, y)   # accumulate into zeros == plain store
    # accumulate: y + up(x) in one more rounding
    base = torch.randn(n, c, h * s, w * s, generator=torch.Generator().manual_seed(7)).to(cuda)
    acc = hip_ops.bilinear_up(x.to(cuda), s, out=base.clone())
    assert torch.equal(acc, base + y)


@pytest.mark.parametrize('s,n,c,h,w', BILINEAR_CASES)
def test_bilinear_adjoint_matches_autograd_and_is_reproducible(cuda, s, n, c, h, w):
    """dx[i] = sum over the output window of w(o, i) * g[o] with at most (2s)^2 terms, summed in fp32 in a fixed order: the
    sum's rounding is <= (2s)^2 u * S with S = sum |w g| (the float64 adjoint applied to |g|); the weights carry the index
    error of _bilinear_bound (3u max(h, w) per factor, a product of two factors) times S.  Bound: ((2s)^2 + 2 + 12 max(h, w)) u S.
    The same bound covers <up(x), g> = <x, up^T(g)> from the two fp32 results (accumulated in float64)."""
    lib = _lib.load()
    gen = torch.Generator().manual_seed(s * 77 + h)
    x = torch.randn(n, c, h, w, generator=gen, dtype=torch.float64, requires_grad=True)
    g = torch.randn(n, c, h * s, w * s, generator=gen)
    F.interpolate(x, scale_factor=s, mode='bilinear', align_corners=False).backward(g.double())
    xa = torch.ones_like(x, requires_grad=True)
    F.interpolate(xa, scale_factor=s, mode='bilinear', align_corners=False).backward(g.double().abs())
    S = xa.grad
    gd = g.to(cuda)
    ids = _profiled(lib, lambda: hip_ops.bilinear_up_bwd(gd, s))
    assert [i for i, _ in ids] == [73]
    dx = hip_ops.bilinear_up_bwd(gd, s)
    k = ((2 * s) ** 2 + 2 + 12 * max(h, w)) * U32
    err = (dx.cpu().double() - x.grad).abs()
    assert bool((err <= k * S + 1e-30).all()), float((err / (S + 1e-30)).max() / U32)
    assert torch.equal(hip_ops.bilinear_up_bwd(gd, s), dx)   # bit-reproducible
    # adjoint identity
    xs = x.detach().float().to(cuda)
    up = hip_ops.bilinear_up(xs, s)
    lhs = float((up.double() * gd.double()).sum())
    rhs = float((xs.double() * dx.double()).sum())
    scale = float((up.double().abs() * gd.double().abs()).sum())
    assert abs(lhs - rhs) <= 2 * k * scale
    # accumulate form
    base = torch.randn(n, c, h, w, generator=gen).to(cuda)
    assert torch.equal(hip_ops.bilinear_up_bwd(gd, s, out=base.clone()), base + dx)


# ----------------------------------------------------------------------------------------------------------------- the network
def _load(net, sd, dev):
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return net.to(dev)


def _small(s, dev):
    cfg = dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=2, upscale=s)
    return _load(ira.build_network(dict(type='MSRResNet', **cfg)), synth.msrresnet_state_dict(100 + s, **cfg), dev)


def _big_weights(g):
    import hashlib
    cfg = dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=16, upscale=4)
    sd = synth.msrresnet_state_dict(int(g['big_seed']), **cfg)
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v, np.float32).tobytes())
    assert h.hexdigest() == str(g['big_weights_sha256'])
    return cfg, sd


@pytest.mark.parametrize('s', [2, 3, 4])
def test_forward_matches_the_reference(cuda, golden, s):
    """The RRDBNet forward bar of DESIGN.md section 2, 1e-4 max-abs against the reference's float32 output; the float64 output
    shows how far the reference itself is from exact (stated in the failure message)."""
    g = golden('g_u_msrresnet')
    net = _small(s, cuda).eval()
    with torch.no_grad():
        y = net(torch.from_numpy(g[f'fwd_x{s}_x']).to(cuda)).cpu().numpy()
    assert y.shape == g[f'fwd_x{s}_y'].shape
    err = np.abs(y - g[f'fwd_x{s}_y']).max()
    assert err < 1e-4, (err, np.abs(g[f'fwd_x{s}_y'] - g[f'fwd_x{s}_y64']).max())


def test_default_net_forward_matches_the_reference(cuda, golden):
    g = golden('g_u_msrresnet')
    cfg, sd = _big_weights(g)
    net = _load(ira.build_network(dict(type='MSRResNet', **cfg)), sd, cuda).eval()
    with torch.no_grad():
        y = net(torch.from_numpy(g['big_x']).to(cuda)).cpu().numpy()
    assert y.shape == (1, 3, 128, 128)
    assert np.abs(y - g['big_y']).max() < 1e-4


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize('s', [2, 3, 4])
def test_backward_matches_the_reference(cuda, golden, s):
    """dL/dx and every parameter gradient against autograd through the reference in float64, relative L2.  The bound allows
    for ReLU / LeakyReLU kinks: a pre-activation within fp32 rounding of 0 may take
    the other branch of the mask than in float64, which moves a gradient by a whole term rather than by rounding.  Without
    kinks the fp32 chain is ~1e-6 relative; 1e-4 leaves room for a handful of flipped mask elements and catches any
    structural error (a missing identity path, a wrong mask, a transposed shuffle: all O(1))."""
    g = golden('g_u_msrresnet')
    net = _small(s, cuda).train()
    x = torch.from_numpy(g[f'fwd_x{s}_x']).to(cuda).requires_grad_(True)
    y = net(x)
    y.backward(torch.from_numpy(g[f'fwd_x{s}_gy']).to(cuda))
    assert np.abs(y.detach().cpu().numpy() - g[f'fwd_x{s}_y']).max() < 1e-4
    assert _rel_l2(x.grad.cpu(), g[f'fwd_x{s}_dx64']) < 1e-4
    assert sorted(k for k, _ in net.named_parameters()) == sorted(k[len(f'fwd_x{s}_grad64.'):] for k in g
                                                                    if k.startswith(f'fwd_x{s}_grad64.'))
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        assert _rel_l2(p.grad.cpu(), g[f'fwd_x{s}_grad64.{k}']) < 1e-4, (k, _rel_l2(p.grad.cpu(), g[f'fwd_x{s}_grad64.{k}']))


def test_backward_with_frozen_parameters_and_no_input_grad(cuda, golden):
    """requires_grad_(False) toggling (SRGANModel freezes networks this way): frozen parameters get no gradient, the others
    the same values as with everything trainable; dL/dx is skipped when x needs none."""
    g = golden('g_u_msrresnet')
    net = _small(4, cuda).train()
    x = torch.from_numpy(g['fwd_x4_x']).to(cuda)
    gy = torch.from_numpy(g['fwd_x4_gy']).to(cuda)
    net(x).backward(gy)
    full = {k: p.grad.clone() for k, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    for k, p in net.named_parameters():
        p.requires_grad_(not k.startswith('body.0.'))
    net(x).backward(gy)
    for k, p in net.named_parameters():
        if k.startswith('body.0.'):
            assert p.grad is None
        else:
            assert torch.equal(p.grad, full[k]), k
    for p in net.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        assert not net(x).requires_grad


def test_flat_adam_arena_receives_the_gradients(cuda, golden):
    """With optim.FlatAdam the gradients are added straight into its arena (p.grad are views of it): same values as the
    autograd route, and the packed weight images follow the fused Adam update."""
    from image_restoration_amd import optim
    g = golden('g_u_msrresnet')
    x = torch.from_numpy(g['fwd_x3_x']).to(cuda)
    gy = torch.from_numpy(g['fwd_x3_gy']).to(cuda)
    ref = _small(3, cuda).train()
    ref(x).backward(gy)
    net = _small(3, cuda).train()
    adam = optim.FlatAdam(list(net.parameters()), lr=1e-3, betas=(0.9, 0.99), modules=[net])
    assert net._grad_sink is not None
    adam.zero_grad()
    net(x).backward(gy)
    for (k, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    adam.step()
    with torch.no_grad():
        y_after = net(x)
        twin = _small(3, cuda).eval()
        twin.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
        assert torch.equal(y_after, twin(x))


def test_x4_forward_launch_sequence(cuda):
    """Under the launch profiler an x4 forward is 2*num_block + 5 convs, two shuffles of ~168 MB per 128x128 image at the
    default width (each reads and writes 64 channels at its output size, 256^2 and 512^2), and the bilinear base."""
    lib = _lib.load()
    conv_ids = set(range(0, 16)) | {41, 44, 45, 46, 47}
    for nb, nf, hw in ((2, 16, (9, 11)), (16, 64, (128, 128))):
        net = ira.build_network(dict(type='MSRResNet', num_feat=nf, num_block=nb)).to(cuda).eval()
        x = torch.rand(1, 3, *hw, device=cuda)
        with torch.no_grad():
            net(x)   # packs the weights (not profiled below)
            recs = _profiled(lib, lambda: net(x))
        ids = [i for i, _ in recs]
        assert ids[-1] == 72 and ids.count(70) == 2 and len(ids) == 2 * nb + 5 + 3, ids
        assert all(i in conv_ids for i in ids if i not in (70, 72)), ids
        shuffles = [i for i, k in enumerate(ids) if k == 70]
        assert shuffles == [2 * nb + 2, 2 * nb + 4]
        if nf == 64:
            mb = sum(b for i, b in recs if i == 70) / 1e6
            assert abs(mb - 4 * 2 * 64 * (256 ** 2 + 512 ** 2) / 1e6) < 1e-6 and 165 < mb < 170


def test_checkpoint_loads_strict_and_reproduces_the_fixture(cuda, golden, tmp_path):
    from image_restoration_amd.utils.checkpoint import load_generator_weights
    g = golden('g_u_msrresnet')
    cfg = dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=2, upscale=3)
    sd = synth.msrresnet_state_dict(103, **cfg)
    path = tmp_path / 'net_g.pth'
    torch.save({'params': {k: torch.from_numpy(v) for k, v in sd.items()}}, path)
    net = ira.build_network(dict(type='MSRResNet', **cfg))
    load_generator_weights(net, str(path), strict=True)
    net = net.to(cuda).eval()
    with torch.no_grad():
        y = net(torch.from_numpy(g['fwd_x3_x']).to(cuda)).cpu().numpy()
    assert np.abs(y - g['fwd_x3_y']).max() < 1e-4


def test_tiled_forward_at_scale_3_equals_the_whole_image(cuda):
    from image_restoration_amd.tiling import tiled_forward
    net = _small(3, cuda).eval()
    x = torch.rand(1, 3, 21, 26, generator=torch.Generator().manual_seed(5)).to(cuda)
    with torch.no_grad():
        whole = net(x)
        tiled = tiled_forward(net, x, tile=32, pad=4, scale=3)
    assert tiled.shape == (1, 3, 63, 78) and torch.equal(tiled, whole)
    with torch.no_grad():   # and a real split runs at every scale
        for s in (2, 3, 4):
            n2 = _small(s, cuda).eval()
            xs = torch.rand(1, 3, 20, 24, device=cuda)
            assert tiled_forward(n2, xs, tile=12, pad=2, scale=s).shape == (1, 3, 20 * s, 24 * s)


def test_inference_script_msrresnet_scale_3(cuda, tmp_path):
    from image_restoration_amd import inference
    rng = np.random.default_rng(3)
    src = tmp_path / 'crop.png'
    inference.imwrite_bgr(str(src), rng.integers(0, 256, (20, 28, 3), dtype=np.uint8))
    cfg = dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=2, upscale=3)
    ck = tmp_path / 'net_g.pth'
    torch.save({'params': {k: torch.from_numpy(v) for k, v in synth.msrresnet_state_dict(103, **cfg).items()}}, ck)
    inference.main(['--input', str(src), '--output', str(tmp_path / 'out.png'), '--model_path', str(ck), '--arch', 'MSRResNet',
                    '--scale', '3', '--num_feat', '16', '--num_block', '2'])
    assert inference.imread_bgr(str(tmp_path / 'out.png')).shape == (60, 84, 3)
    inference.main(['--input', str(src), '--output', str(tmp_path / 'tiled.png'), '--model_path', str(ck), '--arch', 'MSRResNet',
                    '--scale', '3', '--num_feat', '16', '--num_block', '2', '--tile', '16', '--tile_pad', '4'])
    assert inference.imread_bgr(str(tmp_path / 'tiled.png')).shape == (60, 84, 3)


# ------------------------------------------------------------------------------------------------------------------- training
def _train_opt(model_type):
    from collections import OrderedDict as OD
    opt = OD(name='golden', model_type=model_type, scale=4, num_gpu=1, manual_seed=0, is_train=True, dist=False, rank=0,
             world_size=1)
    opt['network_g'] = OD(type='MSRResNet', num_in_ch=3, num_out_ch=3, num_feat=16, num_block=2, upscale=4)
    opt['network_d'] = OD(type='VGGStyleDiscriminator128', num_in_ch=3, num_feat=8)
    opt['path'] = OD(pretrain_network_g=None, strict_load_g=True, resume_state=None)
    tr = OD(ema_decay=0.9)
    tr['optim_g'] = OD(type='Adam', lr=1e-3, weight_decay=0, betas=[0.9, 0.99])
    tr['optim_d'] = OD(type='Adam', lr=1e-3, weight_decay=0, betas=[0.9, 0.99])
    tr['scheduler'] = OD(type='MultiStepLR', milestones=[2, 3], gamma=0.5)
    tr['total_iter'] = 4
    tr['warmup_iter'] = -1
    tr['pixel_opt'] = OD(type='L1Loss', loss_weight=1e-2, reduction='mean')
    tr['gan_opt'] = OD(type='GANLoss', gan_type='vanilla', real_label_val=1.0, fake_label_val=0.0, loss_weight=5e-3)
    tr['net_d_iters'] = 1
    tr['net_d_init_iters'] = 0
    opt['train'] = tr
    if model_type == 'SRModel':
        opt['train'].pop('gan_opt')
        opt.pop('network_d')
        opt['train'].pop('optim_d')
    return opt


def _checksums(net):
    return np.array([[float(p.detach().double().sum()), float(p.detach().double().norm())] for _, p in net.named_parameters()])


def _model(mt):
    from image_restoration_amd.models import build_model
    model = build_model(_train_opt(mt))
    cfg = dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=2, upscale=4)
    model.net_g.load_state_dict({k: torch.from_numpy(v) for k, v in synth.msrresnet_state_dict(81, **cfg).items()}, strict=True)
    model.net_g.invalidate_packed()
    model.model_ema(0)
    if hasattr(model, 'net_d'):
        model.net_d.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.vgg128_state_dict(82, 3, 8).items()},
                                    strict=True)
    return model


def _step(model, it):
    model.update_learning_rate(it, warmup_iter=-1)
    model.feed_data({'lq': torch.from_numpy(synth.uniform_input(900 + it, (4, 3, 32, 32))),
                     'gt': torch.from_numpy(synth.uniform_input(950 + it, (4, 3, 128, 128)))})
    model.optimize_parameters(it)


@pytest.mark.parametrize('mt', ['SRModel', 'SRGANModel'])
def test_optimize_parameters_three_iterations(cuda, golden, mt):
    """Three optimize_parameters iterations against the reference's trajectories, by the rule of the G-i test
    (tests/test_training_gpu.py): the fixture holds each trajectory in float32 and float64, both from the reference, and
    every quantity q satisfies |hip - q64| <= 5*|q32 - q64| + floor, i.e. the HIP path is no further from the exact recipe
    than a small multiple of the reference's own float32 arithmetic.  Learning rates and log keys are exact; iteration 1
    starts from identical weights and is also held to 2e-5 on every loss against the float32 reference.

    The floor after iteration 1 carries the ReLU-kink caveat of DESIGN.md section 13.  At iteration 2 of this recipe one
    upconv2 pre-activation lies 4.7e-9 from zero (and one conv_hr pre-activation 2.8e-9 at iteration 3): inside fp32
    rounding, so whether its LeakyReLU mask is 1 or 0.1 is a coin toss for any fp32 evaluation, the reference's included
    (its float32 run happened to agree with float64 there).  A flip moves the gradient of every tensor upstream by
    ~1e-4 relative (measured: 0.7-1.4e-4 relative L2 on all 14 tensors before conv_hr, < 1e-5 at iterations 1 and 3), and
    Adam turns that into per-element update changes of up to ~lr * 1e-4 * |g|/|g_j| on the small elements: parameter
    sums moved by 3.7e-5 at iteration 2 and 2.0e-4 at iteration 3.  KINK = 1e-3 bounds that with 5x room; a structural
    error (a wrong mask, a dropped identity path, a transposed shuffle) moves these sums by O(lr * sqrt(n)) ~ 5e-2."""
    g = golden('g_u_msrresnet')
    K = 5.0
    KINK = 1e-3

    def bound(hip, q32, q64, floor, what):
        hip, q32, q64 = np.asarray(hip, np.float64), np.asarray(q32, np.float64), np.asarray(q64, np.float64)
        err, ref_err = np.abs(hip - q64).max(), np.abs(q32 - q64).max()
        assert err <= K * ref_err + floor, (what, err, ref_err)

    model = _model(mt)
    keys = [str(k) for k in g[f'{mt}_log_keys']]
    for it in range(1, 4):
        _step(model, it)
        assert abs(model.get_current_learning_rate()[0] - g[f'{mt}_lrs'][it - 1]) < 1e-15
        log = model.get_current_log()
        assert sorted(log) == keys
        l32, l64 = g[f'{mt}_logs'][it - 1], g[f'{mt}64_logs'][it - 1]
        scale = np.maximum(np.abs(l64), 1e-3)
        noise = (np.abs(l32 - l64) / scale).max()
        for j, k in enumerate(keys):
            if it == 1:
                assert abs(log[k] - l32[j]) <= 2e-5 * max(abs(l32[j]), 1e-3), (k, log[k], l32[j])
            assert abs(log[k] - l64[j]) / scale[j] <= K * noise + 2e-6, (it, k, log[k], l64[j], noise)
        floor = 2e-5 if it == 1 else KINK
        bound(_checksums(model.net_g), g[f'{mt}_g_checksum_it{it}'], g[f'{mt}64_g_checksum_it{it}'], floor, (it, 'g params'))
        if hasattr(model, 'net_d'):
            bound(_checksums(model.net_d), g[f'{mt}_d_checksum_it{it}'], g[f'{mt}64_d_checksum_it{it}'], floor, (it, 'd params'))
    bound(_checksums(model.net_g_ema), g[f'{mt}_ema_checksum'], g[f'{mt}64_ema_checksum'], KINK, 'ema')
    st = model.optimizer_g.state_dict()['state']
    ea = np.array([float(st[i]['exp_avg'].double().norm()) for i in sorted(st)])
    ea2 = np.array([float(st[i]['exp_avg_sq'].double().norm()) for i in sorted(st)])
    # moments: a flipped mask moves a gradient by ~1e-4 relative (above), so its moment norms move by about that much
    bound(ea, g[f'{mt}_adam_g_exp_avg'], g[f'{mt}64_adam_g_exp_avg'], 1e-3 * g[f'{mt}64_adam_g_exp_avg'].max(), 'exp_avg')
    bound(ea2, g[f'{mt}_adam_g_exp_avg_sq'], g[f'{mt}64_adam_g_exp_avg_sq'], 1e-3 * g[f'{mt}64_adam_g_exp_avg_sq'].max(), 'exp_avg_sq')
    bound(model.net_g.conv_last.weight.detach().cpu().numpy(), g[f'{mt}_g_conv_last_weight'], g[f'{mt}64_g_conv_last_weight'], KINK * 0.1,
          'conv_last')


def test_srmodel_steps_are_bit_reproducible(cuda):
    """No atomics on the path (gather-form bilinear adjoint, fixed-order weight-gradient slabs): two runs of two seeded
    SRModel steps end in bit-identical weights and logs."""
    def run():
        model = _model('SRModel')
        for it in (1, 2):
            _step(model, it)
        return [p.detach().clone() for p in model.net_g.parameters()], dict(model.get_current_log())
    p1, l1 = run()
    p2, l2 = run()
    assert all(torch.equal(a, b) for a, b in zip(p1, p2)) and l1 == l2
