"""EDVRModel on the GPU: six training iterations with ``tsa_iter: 3`` and ``dcn_lr_mul: 0.25`` against torch.optim.Adam driving the
float64 restatement tests/edvr_restate.py on the CPU (the reference's two parameter groups and its requires_grad schedule), the
exact properties of the frozen warm-up, save / resume, the per-folder video validation and the command line.

Trajectory bound (the margin of tests/test_edvr_gpu.py): the same trajectory is run on the CPU in float32; per tensor and per
iteration ||p_hip - p_64|| <= 10 ||p_32 - p_64|| in L2.  Adam's eps for this test is 1e-2 of the rms of the float64 gradient of all
parameters at the initial weights on the first batch (computed from the float64 side alone): with the default 1e-8 one element whose
gradient sign differs between two runs moves by 2 lr, and a single such element in either run decides an L2 comparison by lottery;
the sharp-eps regime is pinned in tests/test_adam_groups_gpu.py, where both sides see identical gradients.  The deformable conv's
data gradient uses float atomics, so nothing here assumes that two backward passes agree bit for bit.

Ratios measured on an MI355X are in DESIGN.md §28."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from image_restoration_amd import _lib
from image_restoration_amd.models import build_model, lr_scheduler

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edvr_restate as E  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24
NET = dict(type='EDVR', num_in_ch=3, num_out_ch=3, num_feat=16, num_frame=3, deformable_groups=2, num_extract_block=1,
           num_reconstruct_block=1, center_frame_idx=None, hr_in=False, with_predeblur=False, with_tsa=True)
LR, BETAS, ITERS, TSA_ITER, DCN_MUL, PERIOD, SAVE_AT = 4e-4, (0.9, 0.99), 6, 3, 0.25, 8, 4
CHARB_EPS = 1e-12


def _state_dict(net, seed):
    """The weights of tests/test_edvr_gpu.py::_state_dict, restated."""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, v in net.state_dict().items():
        if k.endswith('weight'):
            sc = (1.0 if 'conv_offset' in k else 1.4) / np.sqrt(v.shape[1] * v.shape[2] * v.shape[3])
            sd[k] = torch.from_numpy((rng.standard_normal(tuple(v.shape)) * sc).astype(np.float32))
        else:
            sd[k] = torch.from_numpy((rng.standard_normal(tuple(v.shape)) * 0.1).astype(np.float32))
    return sd


def _batches():
    rng = np.random.default_rng(77)
    return [(torch.from_numpy(rng.random((2, 3, 3, 8, 12), dtype=np.float32)), torch.from_numpy(rng.random((2, 3, 32, 48), dtype=np.float32)))
            for _ in range(ITERS)]


def _restated_loss(p, lq, gt, dtype):
    y = E.edvr(p, lq.to(dtype), num_frame=3, deformable_groups=2, num_extract_block=1, num_reconstruct_block=1)
    return torch.sqrt((y - gt.to(dtype)) ** 2 + CHARB_EPS).sum()


def _adam_eps(sd, batches):
    p = {k: v.clone().double().requires_grad_(True) for k, v in sd.items()}
    grads = torch.autograd.grad(_restated_loss(p, *batches[0], torch.float64), list(p.values()))
    rms = math.sqrt(sum(float((g ** 2).sum()) for g in grads) / sum(g.numel() for g in grads))
    return 1e-2 * rms


def _reference_run(sd, batches, dtype, adam_eps):
    """torch.optim.Adam with the reference's two groups (edvr_model.py:20-48) and its requires_grad schedule (:50-67)."""
    p = {k: v.clone().to(dtype).requires_grad_(True) for k, v in sd.items()}
    groups = [dict(params=[v for k, v in p.items() if 'dcn' not in k], lr=LR), dict(params=[v for k, v in p.items() if 'dcn' in k], lr=LR * DCN_MUL)]
    opt = torch.optim.Adam(groups, LR, betas=BETAS, eps=adam_eps, weight_decay=0)
    sched = lr_scheduler.CosineAnnealingRestartLR(opt, periods=[PERIOD], restart_weights=[1], eta_min=0)
    snaps = []
    for it in range(1, ITERS + 1):
        if it > 1:
            sched.step()
        if it == 1:
            for k, v in p.items():
                if 'fusion' not in k:
                    v.requires_grad = False
        elif it == TSA_ITER:
            for v in p.values():
                v.requires_grad = True
        opt.zero_grad(set_to_none=True)
        _restated_loss(p, *batches[it - 1], dtype).backward()
        opt.step()
        snaps.append({k: v.detach().clone() for k, v in p.items()})
    index = {id(v): k for k, v in p.items()}
    steps = {index[id(q)]: int(float(st['step'])) for q, st in opt.state.items()}
    return snaps, steps


def _opt(workdir, init, **train_kw):
    train = dict(optim_g=dict(type='Adam', lr=LR, weight_decay=0, betas=list(BETAS)),
                 scheduler=dict(type='CosineAnnealingRestartLR', periods=[PERIOD], restart_weights=[1], eta_min=0), total_iter=ITERS,
                 warmup_iter=-1, pixel_opt=dict(type='CharbonnierLoss', loss_weight=1.0, reduction='sum'))
    train.update(train_kw)
    for leaf in ('models', 'training_states', 'visualization'):
        os.makedirs(os.path.join(workdir, leaf), exist_ok=True)
    return dict(name='edvr_t', model_type='EDVRModel', scale=4, num_gpu=1, manual_seed=0, is_train=True, dist=False, rank=0, world_size=1,
                network_g=dict(NET), train=train,
                path=dict(pretrain_network_g=init, strict_load_g=True, resume_state=None, models=os.path.join(workdir, 'models'),
                          training_states=os.path.join(workdir, 'training_states'), visualization=os.path.join(workdir, 'visualization')))


def _profile(fn, cap=8192):
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


@pytest.fixture(scope='module')
def run(cuda, tmp_path_factory):
    """Everything expensive, once: the weights, the float64 and float32 trajectories on the CPU, and the HIP model's six iterations
    with what the tests look at recorded after each."""
    work = str(tmp_path_factory.mktemp('edvr_model'))
    from image_restoration_amd.archs.edvr_arch import EDVR
    sd = _state_dict(EDVR(**{k: v for k, v in NET.items() if k != 'type'}), 20)
    init = os.path.join(work, 'init.pth')
    torch.save(dict(params=sd), init)
    batches = _batches()
    adam_eps = _adam_eps(sd, batches)
    ref64, steps64 = _reference_run(sd, batches, torch.float64, adam_eps)
    ref32, _ = _reference_run(sd, batches, torch.float32, adam_eps)
    opt = _opt(work, init, tsa_iter=TSA_ITER, dcn_lr_mul=DCN_MUL)
    opt['train']['optim_g']['eps'] = adam_eps
    model = build_model(opt)
    rec = dict(snaps=[], lrs=[], state_keys=[], steps=[], launches={}, saved=None)

    def after(it):
        rec['snaps'].append(_snapshot(model))
        rec['lrs'].append(list(model.get_current_learning_rate()))
        rec['state_keys'].append(sorted(model.optimizer_g.state_dict()['state']))
        rec['steps'].append(list(model.optimizer_g.steps))
        if it == SAVE_AT:
            model.save(0, it)
            a = model.optimizer_g
            rec['saved'] = dict(flat_p=a.flat_p.cpu().clone(), exp_avg=a.exp_avg.cpu().clone(), exp_avg_sq=a.exp_avg_sq.cpu().clone(),
                                steps=list(a.steps), lrs=[g['lr'] for g in a.param_groups])
    _iterate(model, batches, 1, ITERS - 1, cuda, after)
    rec['launches'] = _profile(lambda: _iterate(model, batches, ITERS, ITERS, cuda, after))
    return dict(work=work, init=init, sd=sd, batches=batches, adam_eps=adam_eps, ref64=ref64, ref32=ref32, steps64=steps64, model=model,
                opt=opt, names=_names(model), **rec)


def _check_bound(hip_snaps, run, its):
    bad, worst = [], 0.0
    for it, snap in zip(its, hip_snaps):
        for k in run['sd']:
            p64 = run['ref64'][it - 1][k]
            d32 = float((run['ref32'][it - 1][k].double() - p64).norm())
            dhip = float((snap[k].double() - p64).norm())
            ratio = dhip / d32 if d32 > 0 else (0.0 if dhip == 0 else float('inf'))
            worst = max(worst, ratio)
            if not dhip <= 10 * d32:
                bad.append((it, k, dhip, d32))
        print(f'iteration {it}: largest ||p_hip - p_64|| / ||p_32 - p_64|| so far {worst:.3f}')
    return bad


# ------------------------------------------------------------------------------------------------------------ trajectory
def test_trajectory_stays_within_ten_times_the_float32_distance(run):
    assert run['adam_eps'] > 0
    print(f"Adam eps = {run['adam_eps']:.4e} (1e-2 of the rms float64 gradient)")
    bad = _check_bound(run['snaps'], run, range(1, ITERS + 1))
    assert not bad, bad[:8]
    moved = [k for k in run['names'] if not torch.equal(run['snaps'][-1][k], run['sd'][k])]
    assert moved == run['names']                                            # after the warm-up everything trained


def test_frozen_parameters_do_not_move_and_have_no_state(run):
    names = run['names']
    dcn = [n for n in names if 'dcn' in n]
    assert names == [n for n in names if 'dcn' not in n] + dcn and dcn       # arena order: normal parameters first, then dcn
    fusion = {i for i, n in enumerate(names) if 'fusion' in n}
    assert fusion and len(fusion) < len(names)
    for it in (1, 2):
        snap = run['snaps'][it - 1]
        for k, v in run['sd'].items():
            if 'fusion' not in k:
                assert torch.equal(snap[k], v), (it, k)                      # bit-identical to the initial value
        assert any(not torch.equal(snap[k], v) for k, v in run['sd'].items() if 'fusion' in k)
        assert set(run['state_keys'][it - 1]) == fusion                      # no optimiser state for what never took part
        assert run['steps'][it - 1] == [it if i in fusion else 0 for i in range(len(names))]
    assert run['steps'][-1] == [6 if i in fusion else 4 for i in range(len(names))]
    assert set(run['state_keys'][-1]) == set(range(len(names)))
    assert run['steps64'] == {n: (6 if 'fusion' in n else 4) for n in names}   # and torch.optim.Adam counts the same
    assert run['model'].optimizer_g.partition_writes == 2                    # the class array was written at the freeze and the un-freeze


def test_group_learning_rates_follow_the_cosine_schedule(run):
    for it, lrs in enumerate(run['lrs'], start=1):
        want = 0.5 * LR * (1 + math.cos(math.pi * (it - 1) / PERIOD))
        assert len(lrs) == 2 and lrs[0] == pytest.approx(want, rel=1e-12) and lrs[1] == pytest.approx(DCN_MUL * lrs[0], rel=1e-12), (it, lrs)


def test_grouped_step_is_one_launch_and_plain_models_are_not_rerouted(run, cuda):
    assert run['launches'].count(139) == 1                                  # iteration 6: one segmented launch for the whole arena
    plain = build_model(_opt(os.path.join(run['work'], 'plain'), run['init']))
    assert len(plain.optimizer_g.param_groups) == 1 and plain.optimizer_g.plan_step()[0] == 'single'
    ids = _profile(lambda: _iterate(plain, run['batches'], 1, 2, cuda))
    assert ids.count(139) == 0 and len(ids) > 0                              # dcn_lr_mul 1, no tsa_iter: the new entry point is never called
    assert plain.optimizer_g.steps == [2] * len(plain.optimizer_g.params) and plain.optimizer_g.class_of_chunk is None
    # dcn_lr_mul alone: two groups from the first step, every parameter stepping
    two = build_model(_opt(os.path.join(run['work'], 'two'), run['init'], dcn_lr_mul=DCN_MUL))
    ids = _profile(lambda: _iterate(two, run['batches'], 1, 1, cuda))
    assert ids.count(139) == 1 and two.optimizer_g.steps == [1] * len(two.optimizer_g.params)
    with pytest.raises(ValueError, match='with_tsa'):
        bad = _opt(os.path.join(run['work'], 'bad'), None, tsa_iter=3)
        bad['network_g']['with_tsa'] = False
        build_model(bad)


def test_save_and_resume_restore_the_optimiser_bit_for_bit(run, cuda):
    work = run['work']
    state = torch.load(os.path.join(work, 'training_states', f'{SAVE_AT}.state'), map_location='cpu', weights_only=False)
    assert state['iter'] == SAVE_AT and len(state['optimizers']) == 1 and len(state['optimizers'][0]['param_groups']) == 2
    steps = {i: int(float(s['step'])) for i, s in state['optimizers'][0]['state'].items()}
    assert steps == {i: (4 if 'fusion' in n else 2) for i, n in enumerate(run['names'])}
    opt = _opt(work, os.path.join(work, 'models', f'net_g_{SAVE_AT}.pth'), tsa_iter=TSA_ITER, dcn_lr_mul=DCN_MUL)
    opt['train']['optim_g']['eps'] = run['adam_eps']
    model = build_model(opt)
    model.resume_training(state)
    a, saved = model.optimizer_g, run['saved']
    for key in ('flat_p', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(getattr(a, key).cpu(), saved[key]), key
    assert a.steps == saved['steps'] and [g['lr'] for g in a.param_groups] == saved['lrs'] and a.param_groups[0]['eps'] == run['adam_eps']
    snaps = []
    _iterate(model, run['batches'], SAVE_AT + 1, ITERS, cuda, lambda it: snaps.append(_snapshot(model)))
    assert a.steps == run['steps'][-1] and model.get_current_learning_rate() == run['lrs'][-1]
    bad = _check_bound(snaps, run, range(SAVE_AT + 1, ITERS + 1))
    assert not bad, bad[:8]


def test_refused_steps_are_taken_back_from_the_parameters_that_took_part(cuda):
    """FlatAdam with two groups and one frozen parameter: a step issued while the device latch is up changes nothing, counts once,
    and take_back_skipped() lowers the step counts of the parameters that took part in it only."""
    from image_restoration_amd import optim
    lib = _lib.load()
    lib.sr_dev_abort_latch_from.argtypes = [C.c_void_p, C.c_void_p]
    lib.sr_dev_abort_latch_from.restype = None
    gen = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(n, generator=gen).to(cuda)) for n in (70, 64, 130)]
    adam = optim.FlatAdam([dict(params=ps[:2]), dict(params=ps[2:], lr=1e-4)], 4e-4, betas=(0.9, 0.99))
    ps[1].requires_grad = False
    adam.flat_g.normal_()
    adam.step()
    adam.step()
    assert adam.steps == [2, 0, 2]
    ps[1].requires_grad = True
    adam.step()
    assert adam.steps == [3, 1, 3] and adam.partition_writes == 1         # the same chunks in the same classes: only the table changed
    torch.cuda.synchronize()
    before = [t.clone() for t in (adam.flat_p, adam.exp_avg, adam.exp_avg_sq)]
    try:
        word = torch.ones(4, dtype=torch.int32, device=cuda)
        lib.sr_dev_abort_latch_from(word.data_ptr(), torch.cuda.current_stream().cuda_stream)
        ps[0].requires_grad = False
        adam.step()                                                           # took part: parameters 1 and 2
        ps[0].requires_grad = True
        adam.step()                                                           # took part: all three
        torch.cuda.synchronize()
        assert adam.steps == [4, 3, 5] and int(adam.skipped.item()) == 2
        for a, b in zip(before, (adam.flat_p, adam.exp_avg, adam.exp_avg_sq)):
            assert torch.equal(a, b)
        assert adam.take_back_skipped() == 2 and adam.steps == [3, 1, 3] and int(adam.skipped.item()) == 0
    finally:
        _lib.check(lib.sr_abort_latch_clear(torch.cuda.current_stream().cuda_stream), 'sr_abort_latch_clear')
        torch.cuda.synchronize()
    adam.step()
    torch.cuda.synchronize()
    assert adam.steps == [4, 2, 4] and not torch.equal(before[0], adam.flat_p) and adam.take_back_skipped() == 0


def test_ema_shadow_follows_the_grouped_arena_and_is_what_test_runs(run, cuda):
    """With two parameter groups the live arena is in group order; the shadow's arena has to have the same layout, or the blend
    mixes different tensors.  decay 0.5 makes the blend exact to restate: s <- 0.5 s + 0.5 p, two roundings, no contraction.  The
    shadow's weight images must follow the blend, which writes behind torch's version counters."""
    from image_restoration_amd.archs.edvr_arch import EDVR
    model = build_model(_opt(os.path.join(run['work'], 'ema'), run['init'], tsa_iter=TSA_ITER, dcn_lr_mul=DCN_MUL, ema_decay=0.5))
    want = {k: v.clone() for k, v in run['sd'].items()}
    lq = run['batches'][0][0].to(cuda)
    for it in (1, 2, 3):
        _iterate(model, run['batches'], it, it, cuda)
        live = _snapshot(model)
        want = {k: 0.5 * want[k] + 0.5 * live[k] for k in want}
        got = {k: v.detach().cpu() for k, v in model.net_g_ema.state_dict().items()}
        for k in want:
            assert torch.equal(got[k], want[k]), (it, k)
        model.feed_data(dict(lq=lq))
        model.test()
        twin = EDVR(**{k: v for k, v in NET.items() if k != 'type'}).to(cuda).eval()
        twin.load_state_dict(want)
        with torch.no_grad():
            assert torch.equal(model.output, twin(lq)), it


# ------------------------------------------------------------------------------------------------------------ validation
def _video_set(root):
    rng = np.random.default_rng(5)
    for folder in ('000', '011'):
        for kind, (h, w) in (('gt', (32, 48)), ('lq', (8, 12))):
            d = os.path.join(root, kind, folder)
            os.makedirs(d)
            for f in range(5):
                Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(d, f'{f:08d}.png'))
    return dict(name='REDS4', type='VideoTestDataset', dataroot_gt=os.path.join(root, 'gt'), dataroot_lq=os.path.join(root, 'lq'),
                io_backend=dict(type='disk'), cache_data=False, num_frame=3, padding='reflection_circle', scale=4, phase='val')


def test_validation_reports_per_folder_and_matches_the_host_metric(run, cuda, tmp_path):
    from torch.utils.data import DataLoader
    from image_restoration_amd.data import VideoTestDataset
    from image_restoration_amd.metrics import calculate_psnr
    from image_restoration_amd.utils.img_util import tensor2img
    model = run['model']
    dopt = _video_set(str(tmp_path))
    model.opt['val'] = dict(save_img=False, metrics=dict(psnr=dict(type='calculate_psnr', crop_border=0, test_y_channel=False),
                                                         ssim=dict(type='calculate_ssim', crop_border=0, test_y_channel=False)))
    try:
        results = {}
        for cache in (False, True):
            ds = VideoTestDataset(dict(dopt, cache_data=cache))
            model.validation(DataLoader(ds, batch_size=1, shuffle=False, num_workers=0), 6, None, False)
            results[cache] = {f: t.clone() for f, t in model.metric_results.items()}
            assert list(results[cache]) == ['000', '011']
            for t in results[cache].values():
                assert tuple(t.shape) == (5, 2) and t.is_cuda and t.dtype == torch.float32
        for f in results[False]:
            assert torch.equal(results[False][f], results[True][f])          # cached and uncached frames: the same bits
        # frame by frame against the host metric on tensor2img of test()'s output
        chain = -(-3 * 32 * 48 // (256 * 64)) + 9 + 64                        # tests/test_train_ops_gpu.py::test_psnr_ssim_device
        for index in range(len(ds)):
            item = ds[index]
            model.feed_data(dict(lq=item['lq'].unsqueeze(0), gt=item['gt'].unsqueeze(0)))
            model.test()
            host = calculate_psnr(tensor2img([model.output.detach().cpu()]), tensor2img([item['gt'].unsqueeze(0)]), 0)
            got = float(results[False][item['folder']][int(item['idx'].split('/')[0]), 0])
            # the device reduction's bound, plus the value's rounding into the float32 result tensor
            assert abs(got - host) <= 10 / math.log(10) * EPS32 * chain + 1e-9 + abs(host) * EPS32, (index, got, host)
        summary = model.validation_summary
        for i, m in enumerate(('psnr', 'ssim')):
            means = [float(t[:, i].double().mean()) for t in results[False].values()]
            assert summary['total'][m] == pytest.approx(sum(means) / 2, abs=1e-5)
            assert [summary['folders'][f][m] for f in ('000', '011')] == pytest.approx(means, abs=1e-5)
        assert 0 < summary['total']['ssim'] <= 1 and np.isfinite(summary['total']['psnr'])
        with pytest.raises(NotImplementedError, match='not supported during training'):
            model.validation(DataLoader(ds, batch_size=1), 6, None, True)
        assert model.image_name('REDS4', 'a/b/000/00000003.png') == '00000003' and model.image_name('Vimeo90K', 'x/00001/0266/im4.png') == '00001_0266_im4'
    finally:
        model.opt.pop('val', None)


# ---------------------------------------------------------------------------------------------------------- command line
def test_test_entry_point_reaches_the_video_validation_and_saves_per_folder(run, cuda, tmp_path):
    from image_restoration_amd.test import test_pipeline
    opt = yaml.safe_load(open(os.path.join(ROOT, 'options', 'test', 'EDVR', 'test_EDVR_M_x4_SR_REDS.yml')))
    assert opt['model_type'] == 'EDVRModel' and opt['datasets']['test']['type'] == 'VideoTestDataset' and opt['val']['save_img']
    dopt = _video_set(str(tmp_path / 'data'))
    opt['name'] = 'edvr_test'
    opt['datasets']['test'].update(dataroot_gt=dopt['dataroot_gt'], dataroot_lq=dopt['dataroot_lq'], num_frame=3)
    del opt['datasets']['test']['meta_info_file']                              # folder scan
    opt['network_g'] = dict(NET)
    opt['path']['pretrain_network_g'] = run['init']
    p = tmp_path / 'opt.yml'
    yaml.safe_dump(opt, open(p, 'w'))
    model = test_pipeline(str(tmp_path), ['-opt', str(p)])
    assert type(model).__name__ == 'EDVRModel' and list(model.metric_results) == ['000', '011']
    assert all(tuple(t.shape) == (5, 1) and bool(torch.isfinite(t).all()) for t in model.metric_results.values())
    vis = tmp_path / 'results' / 'edvr_test' / 'visualization' / 'REDS4'
    for folder in ('000', '011'):
        assert sorted(os.listdir(vis / folder)) == [f'{f:08d}_edvr_test.png' for f in range(5)]
    assert Image.open(vis / '011' / '00000004_edvr_test.png').size == (48, 32)
    assert set(model.validation_summary['total']) == {'psnr'}


def test_train_entry_point_runs_saves_and_resumes(cuda, tmp_path):
    opt = yaml.safe_load(open(os.path.join(ROOT, 'options', 'train', 'EDVR', 'train_EDVR_M_x4_synthetic.yml')))
    assert opt['model_type'] == 'EDVRModel' and opt['train']['tsa_iter'] and opt['train']['dcn_lr_mul'] != 1
    opt['name'] = 'tiny_edvr'
    opt['datasets']['train'].update(num_samples=8, num_frame=3, gt_size=32, batch_size_per_gpu=2, num_worker_per_gpu=0, dataset_enlarge_ratio=1)
    opt['network_g'].update(num_feat=16, num_frame=3, deformable_groups=2, num_extract_block=1, num_reconstruct_block=1)
    opt['train'].update(total_iter=4, tsa_iter=3)
    opt['train']['scheduler'].update(periods=[8], restart_weights=[1])
    opt['logger'].update(print_freq=2, save_checkpoint_freq=2)
    p = tmp_path / 'opt.yml'
    yaml.safe_dump(opt, open(p, 'w'))
    code = 'import sys; from image_restoration_amd.train import train_pipeline; train_pipeline(sys.argv[1], sys.argv[2:])'
    r = subprocess.run([sys.executable, '-c', code, str(tmp_path), '-opt', str(p)], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    exp = tmp_path / 'experiments' / 'tiny_edvr'
    assert (exp / 'models' / 'net_g_latest.pth').exists() and (exp / 'models' / 'net_g_4.pth').exists()
    assert (exp / 'training_states' / '2.state').exists() and (exp / 'training_states' / '4.state').exists()
    assert 'Only train TSA module for 3 iters.' in r.stderr and 'Train all the parameters.' in r.stderr
    assert 'Multiple the learning rate for dcn with 0.25.' in r.stderr
    assert set(torch.load(exp / 'models' / 'net_g_latest.pth', weights_only=False)) == {'params', 'params_ema'}
    # --auto_resume picks 4.state up and goes on to iteration 6
    opt['train']['total_iter'] = 6
    yaml.safe_dump(opt, open(p, 'w'))
    from image_restoration_amd.train import train_pipeline
    model = train_pipeline(str(tmp_path), ['-opt', str(p), '--auto_resume'])
    names = _names(model)
    assert model.optimizer_g.steps == [6 if 'fusion' in n else 4 for n in names] and (exp / 'training_states' / '6.state').exists()
    assert np.isfinite(model.get_current_log()['l_pix'])
