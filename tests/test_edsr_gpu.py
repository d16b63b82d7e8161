"""EDSR on the MI355X: fp32 forward, backward and SRModel training against the reference's own results in
tests/golden/g_y_edsr.npz (tools/make_golden_edsr.py); EDSR-L at its real width against a float64 restatement; the bf16 forward
against a float64 model of bf16 storage; tiling, checkpoints and the test entry point.

The yardstick of every fp32 comparison is the reference's own float32 distance from its float64 run, stored in the fixture:
|hip - q64| <= 10 * |q32 - q64| + floor.  10x because the summation order differs (MFMA tiles, slab reductions) and the network
is deep; floor = 4 ulp of the tensor's magnitude (4 * 2^-23 * max|q64|) for a tensor on which the reference's float32 run
happens to land closer to float64 than rounding the result itself allows (the float64 values are stored as float32, which
alone costs half an ulp)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import image_restoration_amd as ira
from image_restoration_amd.utils import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23
# upscale -> (network, weight seed): the networks of tools/make_golden_edsr.py
SMALL = {
    2: (dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=2, upscale=2, res_scale=1), 202),
    3: (dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=2, upscale=3, res_scale=0.1, img_range=1.0,
             rgb_mean=(0.5, 0.25, 0.125)), 203),
    4: (dict(num_in_ch=3, num_out_ch=3, num_feat=32, num_block=3, upscale=4, res_scale=0.1), 204),
}
TRAIN_G = dict(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=2, upscale=4, res_scale=0.1)
L4 = dict(num_in_ch=3, num_out_ch=3, num_feat=256, num_block=32, upscale=4, res_scale=0.1, img_range=255.,
          rgb_mean=(0.4488, 0.4371, 0.4040))


def _load(net, sd, dev):
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return net.to(dev)


def _small(s, dev, **kw):
    cfg, seed = SMALL[s]
    return _load(ira.build_network(dict(type='EDSR', **cfg, **kw)), synth.edsr_state_dict(seed, **cfg), dev)


def _within(hip, q64, e32, what, k=10.0):
    """|hip - q64| <= k * e32 + 4 ulp of max|q64|; prints the measured ratio to the reference's own float32 distance."""
    hip, q64 = np.asarray(hip, np.float64), np.asarray(q64, np.float64)
    assert hip.shape == q64.shape, what
    err = float(np.abs(hip - q64).max())
    floor = 4 * ULP * float(np.abs(q64).max())
    print(f'{what}: err {err:.3e}  ref32 {float(e32):.3e}  ratio {err / max(float(e32), 1e-300):.2f}  floor {floor:.1e}')
    assert err <= k * float(e32) + floor, (what, err, float(e32), floor)
    return err


# ----------------------------------------------------------------------------------------------------- float64 restatement
def restate(x, sd, cfg, r=lambda t: t, rw=lambda t: t):
    """EDSR.forward from the layer list (edsr_arch.py:50-61, arch_util.py:84-87, 98-109) in the dtype of ``x`` and ``sd``, in
    plain torch ops.  ``r`` is applied wherever the bf16 path stores an activation (the shifted input, every conv output after
    its epilogue; not conv_last's fp32 output; the shuffle is a permutation), ``rw`` to every weight: identity functions give
    the exact network, bf16 round trips the model of bf16 storage (in the manner of oracle/bf16_sim.py)."""
    def cv(t, name):
        return F.conv2d(t, rw(sd[name + '.weight']), sd[name + '.bias'], padding=1)
    mean = torch.tensor(cfg.get('rgb_mean', (0.4488, 0.4371, 0.4040)), dtype=torch.float32).to(x.dtype).view(1, 3, 1, 1)
    rng, rs, s = cfg.get('img_range', 255.), cfg.get('res_scale', 1), cfg['upscale']
    t = r((x - mean) * rng)
    first = feat = r(cv(t, 'conv_first'))
    for b in range(cfg['num_block']):
        u = r(torch.relu(cv(feat, f'body.{b}.conv1')))
        feat = r(feat + rs * cv(u, f'body.{b}.conv2'))
    feat = r(cv(feat, 'conv_after_body') + first)
    stages = [(0, 3)] if s == 3 else [(2 * k, 2) for k in range(int(round(np.log2(s))))]
    for idx, f in stages:
        feat = F.pixel_shuffle(r(cv(feat, f'upsample.{idx}')), f)
    return cv(feat, 'conv_last') / rng + mean


def _bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _sd_t(sd, dt):
    return {k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in sd.items()}


def test_the_restatement_reproduces_the_reference(golden):
    """The float64 restatement against the reference's float64 outputs (stored as float32): within the storage rounding."""
    g = golden('g_y_edsr')
    for s, (cfg, seed) in SMALL.items():
        y = restate(torch.from_numpy(g[f'x{s}_x']).double(), _sd_t(synth.edsr_state_dict(seed, **cfg), torch.float64), cfg)
        ref = torch.from_numpy(g[f'x{s}_y64']).double()
        assert float((y - ref).abs().max()) <= ULP * float(ref.abs().max())


# ----------------------------------------------------------------------------------------------------------- fp32 forward
@pytest.mark.parametrize('s', [2, 3, 4])
def test_forward_matches_the_reference(cuda, golden, s):
    g = golden('g_y_edsr')
    net = _small(s, cuda).eval()
    with torch.no_grad():
        y = net(torch.from_numpy(g[f'x{s}_x']).to(cuda))
        again = net(torch.from_numpy(g[f'x{s}_x']).to(cuda))
    assert y.dtype == torch.float32 and torch.equal(y, again)
    _within(y.cpu().numpy(), g[f'x{s}_y64'], g[f'x{s}_y32_err'], f'forward x{s}')


def test_any_batch_and_size(cuda):
    """Batch 1 and 5, 1x1 and a 70-wide input: the output has the reference's shape and agrees with the float64 restatement
    within 10x the restatement's own float32 distance."""
    cfg, seed = SMALL[3]
    sd = synth.edsr_state_dict(seed, **cfg)
    net = _small(3, cuda).eval()
    for shape in ((1, 3, 1, 1), (5, 3, 3, 70), (1, 3, 33, 2)):
        x = torch.rand(*shape, generator=torch.Generator().manual_seed(shape[3]))
        y64 = restate(x.double(), _sd_t(sd, torch.float64), cfg)
        y32 = restate(x, _sd_t(sd, torch.float32), cfg)
        with torch.no_grad():
            y = net(x.to(cuda)).cpu()
        assert y.shape == y64.shape == (shape[0], 3, 3 * shape[2], 3 * shape[3])
        _within(y.numpy(), y64.numpy(), float((y32.double() - y64).abs().max()), f'shape {shape}')


def test_x4_forward_launch_sequence(cuda):
    """Under the launch profiler an x4 forward is the input shift, 2*num_block + 5 convs with a shuffle after each of the two
    upsampling convs (the CB8 one in fp32, the CB16 one in bf16), and the output shift: nothing else records itself."""
    import ctypes as C
    from image_restoration_amd import _lib
    lib = _lib.load()
    nb = SMALL[4][0]['num_block']
    for dt, shuffle_id in (('fp32', 70), ('bf16', 98)):
        net = _small(4, cuda, compute_dtype=dt).eval()
        x = torch.rand(2, 3, 9, 11, device=cuda)
        with torch.no_grad():
            net(x)   # packs the weights (not profiled below)
            _lib.check(lib.sr_profile_start(256), 'sr_profile_start')
            try:
                net(x)
            finally:
                recs = (_lib.LaunchRecord * 256)()
                cnt = C.c_int(0)
                _lib.check(lib.sr_profile_stop(recs, 256, C.byref(cnt)), 'sr_profile_stop')
        ids = [recs[i].kernel_id for i in range(cnt.value)]
        assert len(ids) == 2 * nb + 5 + 4 and ids[0] == 99 and ids[-1] == 100, (dt, ids)
        assert [i for i, k in enumerate(ids) if k == shuffle_id] == [2 * nb + 4, 2 * nb + 6], (dt, ids)
        assert not any(k in (70, 98, 99, 100) for k in ids[1:2 * nb + 4]), (dt, ids)


# ---------------------------------------------------------------------------------------------------------- fp32 backward
def _backward(net, g, s, dev, need_x=True):
    x = torch.from_numpy(g[f'x{s}_x']).to(dev).requires_grad_(need_x)
    y = net(x)
    (y * torch.from_numpy(g[f'x{s}_R']).to(dev)).sum().backward()
    return x, y


@pytest.mark.parametrize('s', [2, 3, 4])
def test_backward_matches_the_reference(cuda, golden, s):
    """dL/dx and every parameter gradient of sum(out * R) against autograd through the reference in float64, per tensor, by the
    rule of the module docstring with the float32 run's own gradient distance; a second run is bit-identical."""
    g = golden('g_y_edsr')
    net = _small(s, cuda).train()
    x, y = _backward(net, g, s, cuda)
    _within(y.detach().cpu().numpy(), g[f'x{s}_y64'], g[f'x{s}_y32_err'], f'train forward x{s}')
    _within(x.grad.cpu().numpy(), g[f'x{s}_dx64'], g[f'x{s}_dx32_err'], f'x{s} dx')
    names = [k for k, _ in net.named_parameters()]
    assert sorted(names) == sorted(k[len(f'x{s}_grad64.'):] for k in g if k.startswith(f'x{s}_grad64.'))
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        _within(p.grad.cpu().numpy(), g[f'x{s}_grad64.{k}'], g[f'x{s}_grad32_err.{k}'], f'x{s} {k}')
    first = [x.grad.clone()] + [p.grad.clone() for p in net.parameters()]
    net.zero_grad(set_to_none=True)
    x2, _ = _backward(net, g, s, cuda)
    assert all(torch.equal(a, b) for a, b in zip(first, [x2.grad] + [p.grad for p in net.parameters()]))


def test_backward_with_frozen_parameters_and_no_input_grad(cuda, golden):
    g = golden('g_y_edsr')
    net = _small(4, cuda).train()
    _backward(net, g, 4, cuda, need_x=False)
    full = {k: p.grad.clone() for k, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    frozen = ('body.0.', 'upsample.0.', 'conv_last.bias')
    for k, p in net.named_parameters():
        p.requires_grad_(not k.startswith(frozen))
    x, _ = _backward(net, g, 4, cuda, need_x=False)
    assert x.grad is None
    for k, p in net.named_parameters():
        if k.startswith(frozen):
            assert p.grad is None, k
        else:
            assert torch.equal(p.grad, full[k]), k
    for p in net.parameters():
        p.requires_grad_(False)
    x = torch.from_numpy(g['x4_x']).to(cuda).requires_grad_(True)
    (net(x) * torch.from_numpy(g['x4_R']).to(cuda)).sum().backward()     # only the input needs a gradient
    _within(x.grad.cpu().numpy(), g['x4_dx64'], g['x4_dx32_err'], 'dx with frozen parameters')
    with torch.no_grad():
        assert not net(x).requires_grad


def test_flat_adam_arena_receives_the_gradients(cuda, golden):
    from image_restoration_amd import optim
    g = golden('g_y_edsr')
    ref = _small(3, cuda).train()
    _backward(ref, g, 3, cuda, need_x=False)
    net = _small(3, cuda).train()
    adam = optim.FlatAdam(list(net.parameters()), lr=1e-3, betas=(0.9, 0.99), modules=[net])
    assert net._grad_sink is not None
    adam.zero_grad()
    _backward(net, g, 3, cuda, need_x=False)
    for (k, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    adam.step()
    x = torch.from_numpy(g['x3_x']).to(cuda)
    with torch.no_grad():
        y_after = net(x)
        twin = _small(3, cuda).eval()
        twin.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
        assert torch.equal(y_after, twin(x))
        assert not torch.equal(y_after, ref(x))


# ------------------------------------------------------------------------------------------------------------------- training
def _train_opt():
    from collections import OrderedDict as OD
    opt = OD(name='golden', model_type='SRModel', scale=4, num_gpu=1, manual_seed=0, is_train=True, dist=False, rank=0,
             world_size=1)
    opt['network_g'] = OD(type='EDSR', **TRAIN_G)
    opt['path'] = OD(pretrain_network_g=None, strict_load_g=True, resume_state=None)
    tr = OD(ema_decay=0.9)
    tr['optim_g'] = OD(type='Adam', lr=1e-3, weight_decay=0, betas=[0.9, 0.99])
    tr['scheduler'] = OD(type='MultiStepLR', milestones=[2, 3], gamma=0.5)
    tr['total_iter'] = 4
    tr['warmup_iter'] = -1
    tr['pixel_opt'] = OD(type='L1Loss', loss_weight=1.0, reduction='mean')
    opt['train'] = tr
    return opt


def _checksums(net):
    return np.array([[float(p.detach().double().sum()), float(p.detach().double().norm())] for _, p in net.named_parameters()])


def _model():
    from image_restoration_amd.models import build_model
    model = build_model(_train_opt())
    model.net_g.load_state_dict({k: torch.from_numpy(v) for k, v in synth.edsr_state_dict(281, **TRAIN_G).items()}, strict=True)
    model.net_g.invalidate_packed()
    model.model_ema(0)
    return model


def _step(model, it):
    model.update_learning_rate(it, warmup_iter=-1)
    model.feed_data({'lq': torch.from_numpy(synth.uniform_input(900 + it, (4, 3, 32, 32))),
                     'gt': torch.from_numpy(synth.uniform_input(950 + it, (4, 3, 128, 128)))})
    model.optimize_parameters(it)


def test_optimize_parameters_three_iterations(cuda, golden):
    """Three SRModel.optimize_parameters iterations (L1, Adam) against the reference's trajectories by the rule of
    test_optimize_parameters_three_iterations in tests/test_msrresnet_gpu.py: every quantity q satisfies
    |hip - q64| <= 5*|q32 - q64| + floor.  Learning rates and log keys are exact; iteration 1 starts from identical weights and
    is also held to 2e-5 on the loss against the float32 reference.  EDSR has the same ReLU masks as MSRResNet's blocks, so
    the floor after iteration 1 is that test's KINK = 1e-3 with its reasoning (a pre-activation inside fp32 rounding of zero
    takes either branch in any fp32 evaluation; a flip moves upstream gradients by ~1e-4 relative and, through Adam, parameter
    sums by up to a few 1e-4; a structural error moves them by O(lr * sqrt(n)) ~ 5e-2)."""
    g = golden('g_y_edsr')
    K, KINK, mt = 5.0, 1e-3, 'SRModel'

    def bound(hip, q32, q64, floor, what):
        hip, q32, q64 = np.asarray(hip, np.float64), np.asarray(q32, np.float64), np.asarray(q64, np.float64)
        err, ref_err = np.abs(hip - q64).max(), np.abs(q32 - q64).max()
        print(f'{what}: err {err:.3e}  ref32 {ref_err:.3e}  floor {floor:.1e}')
        assert err <= K * ref_err + floor, (what, err, ref_err)

    model = _model()
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
    bound(_checksums(model.net_g_ema), g[f'{mt}_ema_checksum'], g[f'{mt}64_ema_checksum'], KINK, 'ema')
    st = model.optimizer_g.state_dict()['state']
    ea = np.array([float(st[i]['exp_avg'].double().norm()) for i in sorted(st)])
    ea2 = np.array([float(st[i]['exp_avg_sq'].double().norm()) for i in sorted(st)])
    bound(ea, g[f'{mt}_adam_g_exp_avg'], g[f'{mt}64_adam_g_exp_avg'], 1e-3 * g[f'{mt}64_adam_g_exp_avg'].max(), 'exp_avg')
    bound(ea2, g[f'{mt}_adam_g_exp_avg_sq'], g[f'{mt}64_adam_g_exp_avg_sq'], 1e-3 * g[f'{mt}64_adam_g_exp_avg_sq'].max(), 'exp_avg_sq')
    bound(model.net_g.conv_last.weight.detach().cpu().numpy(), g[f'{mt}_g_conv_last_weight'], g[f'{mt}64_g_conv_last_weight'],
          KINK * 0.1, 'conv_last')


def test_srmodel_steps_are_bit_reproducible(cuda):
    def run():
        model = _model()
        for it in (1, 2):
            _step(model, it)
        return [p.detach().clone() for p in model.net_g.parameters()], dict(model.get_current_log())
    p1, l1 = run()
    p2, l2 = run()
    assert all(torch.equal(a, b) for a, b in zip(p1, p2)) and l1 == l2


# ------------------------------------------------------------------------------------------------ EDSR-L at its real width
@pytest.fixture(scope='module')
def lx4():
    """EDSR-Lx4 (256 features, 32 blocks) on a batch of 2 ragged 6x7 tiles: weights, input, the float64 restatement, the same
    restatement in float32 on the CPU, and the float64 model of bf16 storage."""
    sd = synth.edsr_state_dict(301, **L4)
    x = torch.from_numpy(synth.uniform_input(302, (2, 3, 6, 7)))
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.no_grad():
        sd64 = _sd_t(sd, torch.float64)
        y64 = restate(x.double(), sd64, L4)
        y32 = restate(x, _sd_t(sd, torch.float32), L4)
        ybf = restate(x.double(), sd64, L4, r=_bf16_round, rw=_bf16_round)
    return dict(sd=sd, x=x, y64=y64, y32=y32, ybf=ybf)


def test_lx4_forward_at_its_real_width(cuda, lx4):
    """The only test with 256-wide convs and the 1024-channel shuffle: against the float64 restatement, bounded by 10x the
    distance of the same restatement run in float32 on the CPU (no floor)."""
    net = _load(ira.build_network(dict(type='EDSR', **L4)), lx4['sd'], cuda).eval()
    with torch.no_grad():
        y = net(lx4['x'].to(cuda)).cpu()
    assert y.shape == (2, 3, 24, 28)
    err = float((y.double() - lx4['y64']).abs().max())
    e32 = float((lx4['y32'].double() - lx4['y64']).abs().max())
    print(f'Lx4 fp32: err {err:.3e}  cpu float32 {e32:.3e}  ratio {err / e32:.2f}  max|y| {float(lx4["y64"].abs().max()):.3f}')
    assert err <= 10 * e32, (err, e32)


# --------------------------------------------------------------------------------------------------------------- bf16 forward
def _bf16_check(y_hip, y_model, y64, what):
    """max|y_bf16 - y64| <= 2 * max|y_model - y64| + floor (4 ulp of fp32 at the output's magnitude).  The model accumulates
    exactly and the kernels in fp32; what separates them is values that round the other way at a bf16 tie."""
    y_hip, y_model, y64 = (np.asarray(t, np.float64) for t in (y_hip, y_model, y64))
    err, model = float(np.abs(y_hip - y64).max()), float(np.abs(y_model - y64).max())
    floor = 4 * ULP * float(np.abs(y64).max())
    print(f'{what}: |bf16 - y64| {err:.3e}  |model - y64| {model:.3e}  ratio {err / model:.3f}  '
          f'|bf16 - model| {float(np.abs(y_hip - y_model).max()):.3e}')
    assert err <= 2 * model + floor, (what, err, model)


@pytest.mark.parametrize('s', [2, 3, 4])
def test_bf16_forward_matches_the_model_of_bf16_storage(cuda, golden, s):
    g = golden('g_y_edsr')
    cfg, seed = SMALL[s]
    sd = synth.edsr_state_dict(seed, **cfg)
    x = torch.from_numpy(g[f'x{s}_x'])
    with torch.no_grad():
        y_model = restate(x.double(), _sd_t(sd, torch.float64), cfg, r=_bf16_round, rw=_bf16_round)
    net = _small(s, cuda, compute_dtype='bf16').eval()
    with torch.no_grad():
        y = net(x.to(cuda))
        y_fp32 = _small(s, cuda).eval()(x.to(cuda))
    assert y.dtype == torch.float32 and y.shape == y_model.shape
    _bf16_check(y.cpu().numpy(), y_model.numpy(), g[f'x{s}_y64'], f'bf16 x{s}')
    print(f'bf16 x{s}: distance from the HIP fp32 output (information only) {float((y - y_fp32).abs().max()):.3e}')
    # eval mode with grad enabled: still the forward-only path, no graph; reruns are bit-identical
    y2 = net(x.to(cuda))
    assert y2.grad_fn is None and not y2.requires_grad and torch.equal(y2, y)


def test_bf16_lx4_forward(cuda, lx4):
    net = _load(ira.build_network(dict(type='EDSR', compute_dtype='bf16', **L4)), lx4['sd'], cuda).eval()
    with torch.no_grad():
        y = net(lx4['x'].to(cuda))
        assert torch.equal(net(lx4['x'].to(cuda)), y)
    _bf16_check(y.cpu().numpy(), lx4['ybf'].numpy(), lx4['y64'].numpy(), 'bf16 Lx4')


def test_bf16_refuses_a_forward_that_needs_a_graph(cuda):
    net = _small(2, cuda, compute_dtype='bf16').train()
    x = torch.rand(1, 3, 8, 8, device=cuda)
    with pytest.raises(NotImplementedError, match='fp32'):
        net(x)
    for p in net.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match='fp32'):
        net(x.clone().requires_grad_(True))
    with torch.no_grad():     # train mode under no_grad is a plain forward
        y = net(x)
    assert y.grad_fn is None and y.shape == (1, 3, 16, 16)
    with pytest.raises(ValueError):
        net(torch.rand(1, 4, 8, 8, device=cuda))


def test_bf16_images_follow_a_parameter_update(cuda):
    """The bf16 weight images are rounded from the fp32 parameters at pack time and repacked when a parameter changes."""
    net = _small(2, cuda, compute_dtype='bf16').eval()
    x = torch.rand(1, 3, 9, 7, device=cuda)
    with torch.no_grad():
        y0 = net(x)
        net.conv_last.weight.mul_(2.0)
        y1 = net(x)
        twin = _small(2, cuda, compute_dtype='bf16').eval()
        twin.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
        assert not torch.equal(y0, y1) and torch.equal(y1, twin(x))


# ------------------------------------------------------------------------------------------------ tiling, files, entry point
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


def test_checkpoint_round_trip_reproduces_the_fixture(cuda, golden, tmp_path):
    from image_restoration_amd.utils.checkpoint import load_generator_weights
    g = golden('g_y_edsr')
    cfg, seed = SMALL[3]
    path = tmp_path / 'net_g.pth'
    torch.save({'params_ema': {k: torch.from_numpy(v) for k, v in synth.edsr_state_dict(seed, **cfg).items()}}, path)
    net = ira.build_network(dict(type='EDSR', **cfg))
    load_generator_weights(net, str(path), strict=True)
    net = net.to(cuda).eval()
    with torch.no_grad():
        y = net(torch.from_numpy(g['x3_x']).to(cuda))
    _within(y.cpu().numpy(), g['x3_y64'], g['x3_y32_err'], 'checkpoint x3')
    torch.save({'params_ema': net.state_dict()}, tmp_path / 'again.pth')
    twin = ira.build_network(dict(type='EDSR', **cfg))
    load_generator_weights(twin, str(tmp_path / 'again.pth'), strict=True)
    with torch.no_grad():
        assert torch.equal(twin.to(cuda).eval()(torch.from_numpy(g['x3_x']).to(cuda)), y)


def test_the_test_entry_point_runs_the_mx4_option_file(cuda, tmp_path):
    """python -m image_restoration_amd.test -opt options/test/EDSR/test_EDSR_Mx4.yml with its dataset and checkpoint pointed at a
    temporary folder: images are written and PSNR is reported; the saved PNG is the network's output."""
    from PIL import Image
    from image_restoration_amd.test import test_pipeline
    from image_restoration_amd.utils.img_util import tensor2img
    rng = np.random.default_rng(1)
    (tmp_path / 'gt').mkdir(), (tmp_path / 'lq').mkdir()
    for i in range(2):
        gt = rng.integers(0, 256, (64, 80, 3), dtype=np.uint8)
        Image.fromarray(gt).save(tmp_path / 'gt' / f'p{i}.png')
        Image.fromarray(gt.reshape(16, 4, 20, 4, 3).mean((1, 3)).astype(np.uint8)).save(tmp_path / 'lq' / f'p{i}.png')
    opt = yaml.safe_load(open(os.path.join(ROOT, 'options', 'test', 'EDSR', 'test_EDSR_Mx4.yml')))
    cfg = {k: v for k, v in opt['network_g'].items() if k != 'type'}
    sd = synth.edsr_state_dict(5, **cfg)
    ck = tmp_path / 'net_g.pth'
    torch.save({'params': {k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
    opt['name'] = 'edsr_mx4_tiny'
    opt['datasets'] = dict(test_1=dict(name='pairs', type='PairedImageDataset', dataroot_gt=str(tmp_path / 'gt'),
                                       dataroot_lq=str(tmp_path / 'lq'), io_backend=dict(type='disk')))
    opt['path'].update(pretrain_network_g=str(ck))
    opt['val']['suffix'] = 'x4'
    p = tmp_path / 'test.yml'
    yaml.safe_dump(opt, open(p, 'w'))
    model = test_pipeline(str(tmp_path), ['-opt', str(p)])
    vis = tmp_path / 'results' / 'edsr_mx4_tiny' / 'visualization' / 'pairs'
    assert sorted(os.listdir(vis)) == ['p0_x4.png', 'p1_x4.png']
    assert set(model.metric_results) == {'psnr', 'ssim'} and np.isfinite(model.metric_results['psnr'])
    net = _load(ira.build_network(dict(opt['network_g'])), sd, cuda).eval()
    lq = torch.from_numpy(np.asarray(Image.open(tmp_path / 'lq' / 'p1.png')).transpose(2, 0, 1).astype(np.float32) / 255.)[None]
    with torch.no_grad():
        want = tensor2img([net(lq.to(cuda)).cpu()], rgb2bgr=False)
    assert np.array_equal(np.asarray(Image.open(vis / 'p1_x4.png')), want)
