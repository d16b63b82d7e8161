"""The deterministic deformable-convolution backward through the layers above it, on the GPU: ``DCNFn`` with the flag, ``EDVR``
after ``set_deterministic(True)``, and ``EDVRModel`` with ``train.deterministic_backward: true`` — two backward passes agree bit for
bit, two fresh models take bit-identical steps, and a resumed run continues the uninterrupted one bit for bit (the form of
tests/test_basicvsr_train_gpu.py).

The network is the smallest configuration of tests/test_edvr_gpu.py ('notsa5': five frames of 8 x 12, EDVR-M's 64 features in 8
deformable groups) at b = 2, so that ``center_over_t`` copies; with the flag off its gradients must agree with the deterministic
ones within that file's bound: relative L2 per tensor at most 10x the distance of the float32 restatement from the float64 one.
The model is the one of tests/test_edvr_model_gpu.py (16 features, 2 groups: the split offset / mask path of DCNv2Pack), with
``tsa_iter: 2`` so that from the second step on every parameter, and with it the deformable convolutions' input gradient, trains."""
import os
import sys

import numpy as np
import pytest
import torch

from image_restoration_amd import hip_autograd as A
from image_restoration_amd.archs.arch_util import DCNv2Pack
from image_restoration_amd.archs.edvr_arch import EDVR
from image_restoration_amd.models import build_model

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_edvr_gpu as G  # noqa: E402
import test_edvr_model_gpu as T  # noqa: E402

pytestmark = pytest.mark.gpu

DET_IDS, GATHER_ID = (184, 185, 186), 112
ITERS, SAVE_AT, TSA_ITER, DCN_MUL = 6, 4, 2, 0.25


@pytest.fixture(scope='module')
def cuda():
    return torch.device('cuda:0')


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ the Function
@pytest.mark.parametrize('dg,windows', [(8, True), (2, False)], ids=['windows-dg8', 'split-dg2'])
def test_dcnfn_with_the_flag_gives_the_same_dx_twice(cuda, dg, windows):
    cin, cout, n, h, w = 8 * dg * (1 if windows else 2), 16, 2, 13, 19
    g = torch.Generator().manual_seed(3)
    x = torch.randn((n, cin // 8, h, w, 8), generator=g).to(cuda).requires_grad_(True)
    wt = (torch.randn((cout, cin, 3, 3), generator=g) / (3 * cin ** 0.5)).to(cuda).requires_grad_(True)
    co = (torch.randn((n, (27 * dg + 7) // 8, h, w, 8), generator=g) * 1.5).to(cuda).requires_grad_(True)
    gy = torch.randn((n, cout // 8, h, w, 8), generator=g).to(cuda)
    if windows:
        args = lambda det: (x, co, co, wt, None, 0.1, dg, True, ((0, 18 * dg // 8), (18 * dg // 8, 9 * dg // 8))) + ((det,) if det else ())  # noqa: E731
        leaves = [x, co, wt]
    else:
        off = co[:, :(18 * dg + 7) // 8].detach().clone().requires_grad_(True)
        msk = co[:, :(9 * dg + 7) // 8].detach().clone().requires_grad_(True)
        args = lambda det: (x, off, msk, wt, None, 0.1, dg, True) + ((None, True) if det else ())  # noqa: E731
        leaves = [x, off, msk, wt]
    y = A.DCNFn.apply(*args(True))
    ids = T._profile(lambda: torch.autograd.grad(y, leaves, gy, retain_graph=True))
    assert all(ids.count(i) == 1 for i in DET_IDS) and ids.count(GATHER_ID) == 1
    first, second = (torch.autograd.grad(y, leaves, gy, retain_graph=True) for _ in range(2))
    assert all(_same_bits(a, b) for a, b in zip(first, second)) and bool(first[0].abs().max() > 0)
    # without the flag: the same forward, the same gradients but dx, which is the atomic scatter's
    y0 = A.DCNFn.apply(*args(False))
    assert torch.equal(y0, y)
    ids = T._profile(lambda: torch.autograd.grad(y0, leaves, gy, retain_graph=True))
    assert not set(DET_IDS) & set(ids) and ids.count(GATHER_ID) == 1
    plain = torch.autograd.grad(y0, leaves, gy)
    assert all(_same_bits(a, b) for a, b in zip(plain[1:], first[1:]))
    assert float((plain[0] - first[0]).norm() / first[0].norm()) < 1e-5


# ------------------------------------------------------------------------------------------------------------- the network
@pytest.fixture(scope='module')
def edvr(cuda):
    kw, shape, in_scale, seed = G.CONFIGS['notsa5']
    shape = (2,) + tuple(shape[1:])
    net = EDVR(**G.BASE, **kw)
    sd = G._state_dict(net, seed)
    rng = np.random.default_rng(seed + 1)
    x = torch.from_numpy((rng.standard_normal(shape) * in_scale).astype(np.float32))
    gy = torch.from_numpy(rng.standard_normal((shape[0], 3, 4 * shape[3], 4 * shape[4])).astype(np.float32))
    net = net.to(cuda).eval()          # as tests/test_edvr_gpu.py: eval mode without no_grad, gradients flow
    net.load_state_dict(sd, strict=True)
    return dict(kw=kw, sd=sd, x=x, gy=gy, net=net)


def _pass(edvr, cuda):
    net = edvr['net']
    net.zero_grad(set_to_none=True)
    xd = edvr['x'].to(cuda).requires_grad_(True)
    y = net(xd)
    y.backward(edvr['gy'].to(cuda))
    torch.cuda.synchronize()
    return [y.detach(), xd.grad] + [p.grad.clone() for p in net.parameters()]


def test_edvr_with_the_flag_gives_every_gradient_twice_bit_for_bit(edvr, cuda):
    net = edvr['net']
    packs = [m for m in net.modules() if isinstance(m, DCNv2Pack)]
    assert len(packs) == 4 and not any(m.deterministic for m in packs)
    assert net.set_deterministic(True) is net and all(m.deterministic for m in packs)
    try:
        ids = T._profile(lambda: _pass(edvr, cuda))
        assert all(ids.count(i) == 4 for i in DET_IDS) and ids.count(GATHER_ID) == 4       # one call per deformable conv
        a, b = _pass(edvr, cuda), _pass(edvr, cuda)
        names = ['output', 'grad input'] + [f'grad {k}' for k in edvr['sd']]
        assert len(a) == len(names)
        differ = [n for n, u, v in zip(names, a, b) if not _same_bits(u, v)]
        assert not differ, differ
        assert all(bool(u.abs().max() > 0) for n, u in zip(names, a) if n == 'grad input' or n.endswith('weight'))
        edvr['det'] = a
    finally:
        net.set_deterministic(False)


def test_edvr_without_the_flag_agrees_within_the_float32_distance(edvr, cuda):
    if 'det' not in edvr:
        edvr['net'].set_deterministic(True)
        edvr['det'] = _pass(edvr, cuda)
        edvr['net'].set_deterministic(False)
    ids = T._profile(lambda: _pass(edvr, cuda))
    assert not set(DET_IDS) & set(ids) and ids.count(GATHER_ID) == 4
    atomic = _pass(edvr, cuda)
    y64, g64 = G._restated(edvr['sd'], edvr['x'], edvr['gy'], edvr['kw'], torch.float64)
    y32, g32 = G._restated(edvr['sd'], edvr['x'], edvr['gy'], edvr['kw'], torch.float32)
    names = ['output', 'grad input'] + [f'grad {k}' for k in edvr['sd']]
    bad = []
    for name, u, v, a32, a64 in zip(names, atomic, edvr['det'], [y32] + g32, [y64] + g64):
        d32, d = G._rel(a32, a64), G._rel(u.cpu(), v.cpu())
        if not d <= 10 * d32:
            bad.append((name, d, d32))
    print('atomic against deterministic gradients, largest relative L2: '
          f'{max(G._rel(u.cpu(), v.cpu()) for u, v in zip(atomic, edvr["det"])):.3e}')
    assert not bad, bad
    assert _same_bits(atomic[0], edvr['det'][0])                       # the forward does not know the flag


# --------------------------------------------------------------------------------------------------------------- the model
def _batches():
    rng = np.random.default_rng(79)
    return [(torch.from_numpy(rng.random((2, 3, 3, 8, 12), dtype=np.float32)), torch.from_numpy(rng.random((2, 3, 32, 48), dtype=np.float32)))
            for _ in range(ITERS)]


@pytest.fixture(scope='module')
def base(tmp_path_factory):
    work = str(tmp_path_factory.mktemp('edvr_det'))
    sd = T._state_dict(EDVR(**{k: v for k, v in T.NET.items() if k != 'type'}), 20)
    init = os.path.join(work, 'init.pth')
    torch.save(dict(params=sd), init)
    return dict(work=work, sd=sd, init=init, batches=_batches())


def _model(base, sub, init=None, **train_kw):
    kw = dict(tsa_iter=TSA_ITER, dcn_lr_mul=DCN_MUL, deterministic_backward=True, total_iter=ITERS)
    kw.update(train_kw)
    return build_model(T._opt(os.path.join(base['work'], sub), init or base['init'], **kw))


def _arena(model):
    a = model.optimizer_g
    torch.cuda.synchronize()
    return dict(flat_p=a.flat_p.cpu().clone(), exp_avg=a.exp_avg.cpu().clone(), exp_avg_sq=a.exp_avg_sq.cpu().clone(), steps=list(a.steps),
                lrs=[g['lr'] for g in a.param_groups])


@pytest.fixture(scope='module')
def twins(cuda, base):
    """Two fresh models with one seed: four steps each; the first then saves and goes on to six."""
    out = []
    for sub in ('twin_a', 'twin_b'):
        torch.manual_seed(0)
        model = _model(base, sub)
        T._iterate(model, base['batches'], 1, SAVE_AT, cuda)
        out.append(dict(model=model, at4=T._snapshot(model), arena4=_arena(model)))
    a = out[0]
    a['model'].save(0, SAVE_AT)
    a['launches'] = T._profile(lambda: T._iterate(a['model'], base['batches'], SAVE_AT + 1, SAVE_AT + 1, cuda))
    T._iterate(a['model'], base['batches'], SAVE_AT + 2, ITERS, cuda)
    a['at6'], a['arena6'] = T._snapshot(a['model']), _arena(a['model'])
    return out


def test_two_fresh_models_take_bit_identical_steps(twins, base):
    a, b = twins
    assert all(m.deterministic for m in a['model'].net_g.modules() if isinstance(m, DCNv2Pack))
    assert all(a['launches'].count(i) == 4 for i in DET_IDS)                # a training step runs the deterministic scatter
    for k, v in a['at4'].items():
        assert _same_bits(v, b['at4'][k]), k
    assert all(not torch.equal(v, base['sd'][k]) for k, v in a['at4'].items() if k.endswith('weight'))   # every weight trained
    for key in ('flat_p', 'exp_avg', 'exp_avg_sq'):
        assert _same_bits(a['arena4'][key], b['arena4'][key]), key


def test_save_and_resume_continue_the_same_trajectory_bit_for_bit(twins, cuda, base):
    a = twins[0]
    work = os.path.join(base['work'], 'twin_a')
    state = torch.load(os.path.join(work, 'training_states', f'{SAVE_AT}.state'), map_location='cpu', weights_only=False)
    assert state['iter'] == SAVE_AT and len(state['optimizers'][0]['param_groups']) == 2
    model = _model(base, 'twin_a', init=os.path.join(work, 'models', f'net_g_{SAVE_AT}.pth'))
    model.resume_training(state)
    got = _arena(model)
    for key in ('flat_p', 'exp_avg', 'exp_avg_sq'):
        assert _same_bits(got[key], a['arena4'][key]), key
    assert got['steps'] == a['arena4']['steps'] and got['lrs'] == a['arena4']['lrs']
    T._iterate(model, base['batches'], SAVE_AT + 1, ITERS, cuda)
    for k, v in T._snapshot(model).items():
        assert _same_bits(v, a['at6'][k]), k                                  # the uninterrupted run's parameters
    got = _arena(model)
    for key in ('flat_p', 'exp_avg', 'exp_avg_sq'):
        assert _same_bits(got[key], a['arena6'][key]), key                    # and its optimiser state
    assert got['steps'] == a['arena6']['steps'] and got['lrs'] == a['arena6']['lrs']


def test_the_model_without_the_key_keeps_the_atomic_scatter(cuda, base):
    opt = T._opt(os.path.join(base['work'], 'plain'), base['init'], tsa_iter=TSA_ITER, dcn_lr_mul=DCN_MUL, total_iter=ITERS)
    assert 'deterministic_backward' not in opt['train']
    model = build_model(opt)
    assert not any(m.deterministic for m in model.net_g.modules() if isinstance(m, DCNv2Pack))
    T._iterate(model, base['batches'], 1, TSA_ITER - 1, cuda)
    ids = T._profile(lambda: T._iterate(model, base['batches'], TSA_ITER, TSA_ITER, cuda))
    assert not set(DET_IDS) & set(ids) and ids.count(GATHER_ID) == 4
