"""Training BasicVSR from option files on the GPU: the deterministic backward (``set_autograd(True, deterministic=True)``) at the
network, then VideoRecurrentModel — bit-reproducible steps, save / resume on the same trajectory, the optimiser wiring against
torch.optim.Adam, the frozen flow network, the two learning-rate groups, validation inside training and the command line.

num_feat 8, num_block 2, clips of 3 frames of 36x40 LQ pixels, batch 2: three frames put a scatter upstream of the flow gradients.

Optimiser wiring (the margin and form of tests/test_edvr_model_gpu.py): per iteration the gradients the model produced are read
from its arena; torch.optim.Adam is driven on the CPU in float64 and in float32 with the reference's two groups
(video_recurrent_model.py:17-41), its requires_grad schedule (:43-62) and those same gradients; per tensor and per iteration
||p_hip - p_64|| <= 10 ||p_32 - p_64|| in L2.  Adam's eps is 1e-2 of the rms of the gradient of all parameters at the initial
weights on the first batch, that test's choice and for its reason: with the default 1e-8 one element whose moment ratio rounds
differently moves by 2 lr and decides an L2 comparison by lottery.

The default (atomic) backward against the deterministic one: relative L2 per tensor at most 1e-4, the figure
tests/test_basicvsr_backward_gpu.py::test_contracts allows two atomic passes; printed next to what two atomic passes show."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import image_restoration_amd as ira
from image_restoration_amd import _lib, optim
from image_restoration_amd.data import SyntheticClipDataset
from image_restoration_amd.losses import build_loss
from image_restoration_amd.models import build_model, lr_scheduler

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_restate as FR  # noqa: E402
import vsr_restate as V  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = dict(type='BasicVSR', num_feat=8, num_block=2, spynet_path=None)
BATCH, FRAMES, LQ_H, LQ_W = 2, 3, 36, 40
LR, BETAS, ITERS, FIX_FLOW, FLOW_MUL, PERIOD, SAVE_AT = 4e-4, (0.9, 0.99), 6, 3, 0.125, 8, 4
SPYNET_BWD_IDS = set(range(169, 177))
ATOMIC_ID, DET_IDS, ADAM_GROUPS_ID = 178, (180, 181, 182), 139


def _state_dict():
    sd = {'spynet.' + k: v for k, v in FR.spynet_weights(11, 4.0).items()}
    sd.update(V.basicvsr_weights(12, NET['num_feat'], NET['num_block'], 0.5))
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def _batches():
    rng = np.random.default_rng(78)
    return [(torch.from_numpy(rng.random((BATCH, FRAMES, 3, LQ_H, LQ_W), dtype=np.float32)),
             torch.from_numpy(rng.random((BATCH, FRAMES, 3, 4 * LQ_H, 4 * LQ_W), dtype=np.float32))) for _ in range(ITERS)]


def _network(sd, cuda, deterministic):
    net = ira.build_network(dict(NET)).to(cuda)
    net.load_state_dict(sd, strict=True)
    return net.train().set_autograd(True, deterministic=deterministic)


def _opt(workdir, init, **train_kw):
    train = dict(optim_g=dict(type='Adam', lr=LR, weight_decay=0, betas=list(BETAS)),
                 scheduler=dict(type='CosineAnnealingRestartLR', periods=[PERIOD], restart_weights=[1], eta_min=0), total_iter=ITERS,
                 warmup_iter=-1, pixel_opt=dict(type='CharbonnierLoss', loss_weight=1.0, reduction='mean'))
    train.update(train_kw)
    for leaf in ('models', 'training_states', 'visualization'):
        os.makedirs(os.path.join(workdir, leaf), exist_ok=True)
    return dict(name='basicvsr_t', model_type='VideoRecurrentModel', scale=4, num_gpu=1, manual_seed=0, is_train=True, dist=False, rank=0,
                world_size=1, network_g=dict(NET), train=train,
                path=dict(pretrain_network_g=init, strict_load_g=True, resume_state=None, models=os.path.join(workdir, 'models'),
                          training_states=os.path.join(workdir, 'training_states'), visualization=os.path.join(workdir, 'visualization')))


def _profile(fn, cap=16384):
    lib = _lib.load()
    _lib.check(lib.sr_profile_start(cap), 'sr_profile_start')
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        recs = (_lib.LaunchRecord * cap)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, cap, C.byref(cnt)), 'sr_profile_stop')
    assert cnt.value < cap
    return [recs[i].kernel_id for i in range(cnt.value)]


def _iterate(model, batches, first, last, cuda, on_iter=None):
    for it in range(first, last + 1):
        model.update_learning_rate(it)
        lq, gt = batches[it - 1]
        model.feed_data(dict(lq=lq.to(cuda), gt=gt.to(cuda)))
        model.optimize_parameters(it)
        if on_iter:
            on_iter(it)


def _snapshot(model):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in model.net_g.state_dict().items()}


def _names(model):
    by_id = {id(p): n for n, p in model.net_g.named_parameters()}
    return [by_id[id(p)] for p in model.optimizer_g.params]


def _arena(model):
    a = model.optimizer_g
    torch.cuda.synchronize()
    return dict(flat_p=a.flat_p.cpu().clone(), exp_avg=a.exp_avg.cpu().clone(), exp_avg_sq=a.exp_avg_sq.cpu().clone(), steps=list(a.steps),
                lrs=[g['lr'] for g in a.param_groups])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope='module')
def base(cuda, tmp_path_factory):
    """The weights, the batches and Adam's eps (from one probe backward at the initial weights on the first batch), once."""
    work = str(tmp_path_factory.mktemp('basicvsr_train'))
    sd = _state_dict()
    init = os.path.join(work, 'init.pth')
    torch.save(dict(params=sd), init)
    batches = _batches()
    net = _network(sd, cuda, True)
    cri = build_loss(dict(type='CharbonnierLoss', loss_weight=1.0, reduction='mean')).to(cuda)
    lq, gt = batches[0]
    cri(net(lq.to(cuda)), gt.to(cuda)).backward()
    grads = [p.grad for p in net.parameters()]
    assert all(g is not None for g in grads)
    rms = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads) / sum(g.numel() for g in grads))
    return dict(work=work, sd=sd, init=init, batches=batches, adam_eps=1e-2 * rms)


def _model(base, sub, **train_kw):
    kw = dict(fix_flow=FIX_FLOW, flow_lr_mul=FLOW_MUL)
    kw.update(train_kw)
    opt = _opt(os.path.join(base['work'], sub), base['init'], **kw)
    opt['train']['optim_g']['eps'] = base['adam_eps']
    return build_model(opt), opt


# ------------------------------------------------------------------------------------------- the deterministic backward
def _grads_twice(net, x, gd, leaves):
    """Two backward passes of ONE graph -> two lists of gradients (the parameters ``net`` reaches, then the leaves)."""
    params = [p for n, p in net.named_parameters() if leaves is None or not n.startswith('spynet.')]
    if leaves is None:
        y, extra = net(x), []
    else:
        y, extra = net.propagate(x, *leaves), list(leaves)
    assert y.grad_fn is not None
    loss = (y * gd).sum()
    return [torch.autograd.grad(loss, params + extra, retain_graph=True) for _ in range(2)]


def test_two_backward_passes_of_one_graph_are_bit_identical(cuda, base):
    lq = base['batches'][0][0].to(cuda)
    gd = torch.from_numpy(np.random.default_rng(5).standard_normal((BATCH, FRAMES, 3, 4 * LQ_H, 4 * LQ_W)).astype(np.float32)).to(cuda)
    det, atomic = _network(base['sd'], cuda, True), _network(base['sd'], cuda, False)
    with torch.no_grad():
        ff, fb = (f.clone() for f in det.get_flow(lq))
    assert float(ff.abs().max()) > 0.5                                    # the flows do warp
    leaves = lambda: (ff.clone().requires_grad_(), fb.clone().requires_grad_())   # noqa: E731
    # the flows as leaves: every parameter propagate reaches and both flow tensors
    ids = _profile(lambda: _grads_twice(det, lq, gd, leaves()))
    assert ATOMIC_ID not in ids and all(ids.count(i) == 2 * 2 * (FRAMES - 1) for i in DET_IDS)
    a, b = _grads_twice(det, lq, gd, leaves())
    assert all(_same_bits(u, v) for u, v in zip(a, b)) and all(bool(u.abs().max() > 0) for u in a)
    # the whole network: SpyNet's parameters receive the flow gradients, which lie downstream of a scatter
    wa, wb = _grads_twice(det, lq, gd, None)
    assert len(wa) == len(list(det.parameters())) and all(_same_bits(u, v) for u, v in zip(wa, wb))
    assert all(bool(u.abs().max() > 0) for u in wa)
    # the default mode: the atomic scatter, within the figure two of its own passes are allowed of the deterministic result
    ids = _profile(lambda: _grads_twice(atomic, lq, gd, None))
    assert ids.count(ATOMIC_ID) == 2 * 2 * (FRAMES - 1) and not set(DET_IDS) & set(ids)
    ta, tb = _grads_twice(atomic, lq, gd, None)
    rel = lambda u, v: float((u.double() - v.double()).norm() / v.double().norm())   # noqa: E731
    again = max(rel(u, v) for u, v in zip(ta, tb))
    dist = max(rel(u, v) for u, v in zip(ta, wa))
    print(f'atomic vs deterministic gradients: {dist:.3e}; two atomic passes: {again:.3e}; bound 1e-4')
    assert dist <= 1e-4


def test_flat_adam_arena_route_equals_the_autograd_route_bit_for_bit(cuda, base):
    lq, gt = (t.to(cuda) for t in base['batches'][1])
    ref, net = _network(base['sd'], cuda, True), _network(base['sd'], cuda, True)
    ((ref(lq) - gt) ** 2).sum().backward()
    adam = optim.FlatAdam(list(net.parameters()), lr=1e-4, betas=BETAS, modules=[net])
    assert net._grad_sink is not None
    adam.zero_grad()
    ((net(lq) - gt) ** 2).sum().backward()
    want = dict(ref.named_parameters())
    for k, p in net.named_parameters():
        assert torch.equal(p.grad, want[k].grad) and bool(p.grad.abs().max() > 0), k


# ---------------------------------------------------------------------------------------------------------- model steps
@pytest.fixture(scope='module')
def twins(cuda, base):
    """Two fresh models with one seed: four steps each; the first then saves and goes on to six."""
    out = []
    for sub in ('twin_a', 'twin_b'):
        torch.manual_seed(0)
        model, opt = _model(base, sub)
        _iterate(model, base['batches'], 1, SAVE_AT, cuda)
        out.append(dict(model=model, opt=opt, at4=_snapshot(model), arena4=_arena(model)))
    a = out[0]
    a['model'].save(0, SAVE_AT)
    _iterate(a['model'], base['batches'], SAVE_AT + 1, ITERS, cuda)
    a['at6'], a['arena6'] = _snapshot(a['model']), _arena(a['model'])
    return out


def test_two_fresh_models_take_bit_identical_steps(twins, base):
    a, b = twins
    assert a['model'].net_g._deterministic is True                          # deterministic_backward defaults to true
    for k, v in a['at4'].items():
        assert _same_bits(v, b['at4'][k]), k
    assert any(not torch.equal(v, base['sd'][k]) for k, v in a['at4'].items() if k.startswith('spynet.') and 'weight' in k)
    for key in ('flat_p', 'exp_avg', 'exp_avg_sq'):
        assert _same_bits(a['arena4'][key], b['arena4'][key]), key


def test_save_and_resume_continue_the_same_trajectory_bit_for_bit(twins, cuda, base):
    a = twins[0]
    work = os.path.join(base['work'], 'twin_a')
    state = torch.load(os.path.join(work, 'training_states', f'{SAVE_AT}.state'), map_location='cpu', weights_only=False)
    assert state['iter'] == SAVE_AT and len(state['optimizers'][0]['param_groups']) == 2
    opt = _opt(work, os.path.join(work, 'models', f'net_g_{SAVE_AT}.pth'), fix_flow=FIX_FLOW, flow_lr_mul=FLOW_MUL)
    opt['train']['optim_g']['eps'] = base['adam_eps']
    model = build_model(opt)
    model.resume_training(state)
    got = _arena(model)
    for key in ('flat_p', 'exp_avg', 'exp_avg_sq'):
        assert _same_bits(got[key], a['arena4'][key]), key
    assert got['steps'] == a['arena4']['steps'] and got['lrs'] == a['arena4']['lrs']
    _iterate(model, base['batches'], SAVE_AT + 1, ITERS, cuda)
    for k, v in _snapshot(model).items():
        assert _same_bits(v, a['at6'][k]), k                                  # the uninterrupted run's parameters
    got = _arena(model)
    for key in ('flat_p', 'exp_avg', 'exp_avg_sq'):
        assert _same_bits(got[key], a['arena6'][key]), key                    # and its optimiser state
    assert got['steps'] == a['arena6']['steps'] and got['lrs'] == a['arena6']['lrs']


# ---------------------------------------------------------------------------------------------------- optimiser wiring
@pytest.fixture(scope='module')
def run(cuda, base):
    """Six iterations of one model, every one profiled, with the gradients it produced and what the tests look at recorded."""
    model, opt = _model(base, 'wiring')
    rec = dict(snaps=[], grads=[], lrs=[], state_keys=[], steps=[], launches=[])

    def after(it):
        torch.cuda.synchronize()
        rec['grads'].append({n: p.grad.detach().cpu().clone() for n, p in model.net_g.named_parameters() if p.requires_grad})
        rec['snaps'].append(_snapshot(model))
        rec['lrs'].append(list(model.get_current_learning_rate()))
        rec['state_keys'].append(sorted(model.optimizer_g.state_dict()['state']))
        rec['steps'].append(list(model.optimizer_g.steps))
    for it in range(1, ITERS + 1):
        rec['launches'].append(_profile(lambda: _iterate(model, base['batches'], it, it, cuda, after)))
    return dict(model=model, opt=opt, names=_names(model), **rec)


def _reference_run(sd, grads, dtype, adam_eps):
    """torch.optim.Adam with the reference's two groups and its requires_grad schedule, fed the gradients the model produced."""
    p = {k: v.clone().to(dtype).requires_grad_(True) for k, v in sd.items() if k not in ('spynet.mean', 'spynet.std')}
    groups = [dict(params=[v for k, v in p.items() if 'spynet' not in k], lr=LR),
              dict(params=[v for k, v in p.items() if 'spynet' in k], lr=LR * FLOW_MUL)]
    opt = torch.optim.Adam(groups, LR, betas=BETAS, eps=adam_eps, weight_decay=0)
    sched = lr_scheduler.CosineAnnealingRestartLR(opt, periods=[PERIOD], restart_weights=[1], eta_min=0)
    snaps = []
    for it in range(1, ITERS + 1):
        if it > 1:
            sched.step()
        if it == 1:
            for k, v in p.items():
                if 'spynet' in k or 'edvr' in k:
                    v.requires_grad_(False)
        elif it == FIX_FLOW:
            for v in p.values():
                v.requires_grad_(True)
        opt.zero_grad(set_to_none=True)
        for k, v in p.items():
            if v.requires_grad:
                v.grad = grads[it - 1][k].to(dtype)
        opt.step()
        snaps.append({k: v.detach().clone() for k, v in p.items()})
    index = {id(v): k for k, v in p.items()}
    return snaps, {index[id(q)]: int(float(st['step'])) for q, st in opt.state.items()}


def test_optimiser_wiring_stays_within_ten_times_the_float32_distance(run, base):
    print(f"Adam eps = {base['adam_eps']:.4e} (1e-2 of the rms gradient)")
    ref64, steps64 = _reference_run(base['sd'], run['grads'], torch.float64, base['adam_eps'])
    ref32, _ = _reference_run(base['sd'], run['grads'], torch.float32, base['adam_eps'])
    bad, worst = [], 0.0
    for it in range(1, ITERS + 1):
        for k, p64 in ref64[it - 1].items():
            d32 = float((ref32[it - 1][k].double() - p64).norm())
            dhip = float((run['snaps'][it - 1][k].double() - p64).norm())
            worst = max(worst, dhip / d32 if d32 > 0 else (0.0 if dhip == 0 else float('inf')))
            if not dhip <= 10 * d32:
                bad.append((it, k, dhip, d32))
        print(f'iteration {it}: largest ||p_hip - p_64|| / ||p_32 - p_64|| so far {worst:.3f}')
    assert not bad, bad[:8]
    assert steps64 == {n: (ITERS - FIX_FLOW + 1 if 'spynet' in n else ITERS) for n in run['names']}    # torch counts the same
    assert run['steps'][-1] == [steps64[n] for n in run['names']]


def test_frozen_flow_network_does_not_move_has_no_state_and_runs_no_backward(run, base):
    names = run['names']
    flow = [n for n in names if 'spynet' in n]
    assert names == [n for n in names if 'spynet' not in n] + flow and flow       # arena order: normal parameters first
    flow_idx = {i for i, n in enumerate(names) if 'spynet' in n}
    for it in range(1, FIX_FLOW):
        snap = run['snaps'][it - 1]
        for k, v in base['sd'].items():
            if k.startswith('spynet.'):
                assert torch.equal(snap[k], v), (it, k)                           # bit-identical to the initial value
            else:
                assert not torch.equal(snap[k], v), (it, k)
        assert set(run['state_keys'][it - 1]) == set(range(len(names))) - flow_idx
        assert run['steps'][it - 1] == [0 if i in flow_idx else it for i in range(len(names))]
        ids = run['launches'][it - 1]
        assert not SPYNET_BWD_IDS & set(ids) and ATOMIC_ID not in ids             # no SpyNet backward, no flow gradient
        assert all(ids.count(i) == 2 * (FRAMES - 1) for i in DET_IDS)
        assert not any('spynet' in n for n in run['grads'][it - 1])
    for it in range(FIX_FLOW, ITERS + 1):
        ids, before = run['launches'][it - 1], run['snaps'][it - 2]
        assert SPYNET_BWD_IDS & set(ids)
        for k, v in run['snaps'][it - 1].items():
            if k not in ('spynet.mean', 'spynet.std'):
                assert not torch.equal(v, before[k]), (it, k)                     # from fix_flow on every parameter moves
    assert set(run['state_keys'][-1]) == set(range(len(names)))
    # the frozen set IS the second group: the class array written at the first step serves the whole run, only the table changes
    assert run['model'].optimizer_g.partition_writes == 1


def test_group_learning_rates_follow_the_cosine_schedule_and_the_step_is_one_launch(run):
    for it, lrs in enumerate(run['lrs'], start=1):
        want = 0.5 * LR * (1 + math.cos(math.pi * (it - 1) / PERIOD))
        assert len(lrs) == 2 and lrs[0] == pytest.approx(want, rel=1e-12) and lrs[1] == pytest.approx(FLOW_MUL * lrs[0], rel=1e-12), (it, lrs)
    for ids in run['launches']:
        assert ids.count(ADAM_GROUPS_ID) == 1                                     # one segmented launch for the whole arena


def test_plain_model_has_one_group_and_the_atomic_switch_is_honoured(cuda, base):
    plain, _ = _model(base, 'plain', fix_flow=None, flow_lr_mul=1, deterministic_backward=False)
    assert len(plain.optimizer_g.param_groups) == 1 and plain.net_g._autograd is True and plain.net_g._deterministic is False
    ids = _profile(lambda: _iterate(plain, base['batches'], 1, 1, cuda))
    assert ids.count(ATOMIC_ID) == 2 * (FRAMES - 1) and not set(DET_IDS) & set(ids) and ids.count(ADAM_GROUPS_ID) == 0
    assert SPYNET_BWD_IDS & set(ids) and plain.optimizer_g.steps == [1] * len(plain.optimizer_g.params)


# ------------------------------------------------------------------------------------------- validation inside training
def test_validation_inside_training_reports_per_folder_and_keeps_the_switch(cuda, base):
    from torch.utils.data import DataLoader
    model, _ = _model(base, 'val', ema_decay=0.999)
    assert model.net_g_ema._autograd is False and model.net_g_ema._deterministic is False     # the shadow never builds a graph
    _iterate(model, base['batches'], 1, 1, cuda)
    ds = SyntheticClipDataset(dict(name='synthetic_val', recurrent=True, num_samples=2, num_frame=FRAMES, gt_size=160, scale=4, seed=1))
    model.opt['val'] = dict(metrics=dict(psnr=dict(type='calculate_psnr', crop_border=0, test_y_channel=False)))
    try:
        model.validation(DataLoader(ds, batch_size=1), 1, None, False)
        assert list(model.metric_results) == ['00000000', '00000001']
        assert all(tuple(t.shape) == (FRAMES, 1) and bool(torch.isfinite(t).all()) for t in model.metric_results.values())
        assert set(model.validation_summary['folders']) == {'00000000', '00000001'} and set(model.validation_summary['total']) == {'psnr'}
        net = model.net_g
        assert net.training and net._autograd is True and net._deterministic is True and net.spynet._autograd is True
        with pytest.raises(NotImplementedError, match='not supported during training'):
            model.validation(DataLoader(ds, batch_size=1), 1, None, True)
        _iterate(model, base['batches'], 2, 2, cuda)                                          # and training goes on
        assert np.isfinite(model.get_current_log()['l_pix'])
    finally:
        model.opt.pop('val', None)


# ---------------------------------------------------------------------------------------------------------- command line
def test_train_entry_point_runs_saves_and_resumes(cuda, tmp_path):
    opt = yaml.safe_load(open(os.path.join(ROOT, 'options', 'train', 'BasicVSR', 'train_BasicVSR_x4_synthetic.yml')))
    assert opt['model_type'] == 'VideoRecurrentModel' and opt['train']['fix_flow'] and opt['train']['flow_lr_mul'] != 1
    opt['name'] = 'tiny_basicvsr'
    opt['datasets']['train'].update(num_samples=8, num_frame=3, gt_size=160, batch_size_per_gpu=2, num_worker_per_gpu=0, dataset_enlarge_ratio=1)
    opt['datasets']['val'].update(num_samples=2, num_frame=3, gt_size=160)
    opt['network_g'].update(num_feat=8, num_block=1)
    opt['train'].update(total_iter=4, fix_flow=3)
    opt['train']['scheduler'].update(periods=[8], restart_weights=[1])
    opt['val']['val_freq'] = 2
    opt['logger'].update(print_freq=2, save_checkpoint_freq=2)
    p = tmp_path / 'opt.yml'
    yaml.safe_dump(opt, open(p, 'w'))
    code = 'import sys; from image_restoration_amd.train import train_pipeline; train_pipeline(sys.argv[1], sys.argv[2:])'
    r = subprocess.run([sys.executable, '-c', code, str(tmp_path), '-opt', str(p)], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    exp = tmp_path / 'experiments' / 'tiny_basicvsr'
    assert (exp / 'models' / 'net_g_latest.pth').exists() and (exp / 'models' / 'net_g_4.pth').exists()
    assert (exp / 'training_states' / '2.state').exists() and (exp / 'training_states' / '4.state').exists()
    assert 'Fix flow network and feature extractor for 3 iters.' in r.stderr and 'Train all the parameters.' in r.stderr
    assert 'Multiple the learning rate for flow network with 0.125.' in r.stderr
    assert 'Validation synthetic_val' in r.stderr and '# psnr:' in r.stderr
    # --auto_resume picks 4.state up and goes on to iteration 6
    opt['train']['total_iter'] = 6
    yaml.safe_dump(opt, open(p, 'w'))
    from image_restoration_amd.train import train_pipeline
    model = train_pipeline(str(tmp_path), ['-opt', str(p), '--auto_resume'])
    names = _names(model)
    assert model.optimizer_g.steps == [4 if 'spynet' in n else 6 for n in names] and (exp / 'training_states' / '6.state').exists()
    assert np.isfinite(model.get_current_log()['l_pix'])
