#!/usr/bin/env python3
"""EDVR training on one MI355X: the measurements of DESIGN.md §28.  Prints one JSON line.

* ``adam``: sr_adam_step_groups_f32 next to sr_adam_step_f32 on the arena of the default EDVR (FlatAdam's layout), HIP events around
  single calls, the two entry points interleaved in one process, median of ``--calls`` after ``--warmup``; GB/s counts 28 bytes per
  arena float (16 read, 12 written).  ``groups_1`` has one class, ``groups_3`` the partition of an EDVRModel run after its warm-up
  (normal / fusion / dcn parameters), ``groups_frozen`` the warm-up itself (only the fusion module's chunks are touched: its GB/s
  counts the touched floats).
* ``step``: one EDVRModel iteration at the M recipe's shape (batch 4 of 5 x 64 x 64 LQ frames, gt_size 256) with and without
  ``dcn_lr_mul`` / ``tsa_iter``, split into forward, loss + backward, optimiser and EMA by HIP events around the phases of
  SRModel.optimize_parameters, median of ``--steps``; and the launch profiler's count of launches and sum of kernel time for one step.

* ``--deterministic``: only the ``step`` row, with and without ``train.deterministic_backward``, two models
  alternating in one process over ``--steps`` rounds, median [min, max]; and the kernels of the deformable convolutions' data
  gradient from one profiled step of each.

    python tools/edvr_train_bench.py [--calls 30 --warmup 5 --steps 7] [--deterministic]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
from collections import OrderedDict as OD

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import image_restoration_amd as ira  # noqa: E402
from image_restoration_amd import _lib, optim  # noqa: E402
from image_restoration_amd.models import build_model  # noqa: E402
from image_restoration_amd.models.sr_model import LossBook  # noqa: E402

NET = OD(type='EDVR', num_in_ch=3, num_out_ch=3, num_feat=64, num_frame=5, deformable_groups=8, num_extract_block=5,
         num_reconstruct_block=10, center_frame_idx=None, hr_in=False, with_predeblur=False, with_tsa=True)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench_adam(calls, warmup, dev):
    lib = _lib.load()
    net = ira.build_network(dict(NET)).to(dev)
    names = [n for n, _ in net.named_parameters()]
    adam = optim.FlatAdam([dict(params=[p for n, p in net.named_parameters() if 'dcn' not in n]),
                           dict(params=[p for n, p in net.named_parameters() if 'dcn' in n], lr=1e-4)], 4e-4, betas=(0.9, 0.99))
    by_id = {id(p): n for n, p in net.named_parameters()}
    order = [by_id[id(p)] for p in adam.params]
    n = adam.numel
    adam.flat_g.normal_().mul_(1e-2)
    st = torch.cuda.current_stream().cuda_stream
    ptrs = (adam.flat_p.data_ptr(), adam.flat_g.data_ptr(), adam.exp_avg.data_ptr(), adam.exp_avg_sq.data_ptr())

    def classes(rows):
        arr = (_lib.AdamClass * len(rows))()
        for c, (lr, step, active) in enumerate(rows):
            arr[c].lr, arr[c].step, arr[c].active = lr, step, active
        return arr
    parts = OD()
    parts['groups_1'] = ([0] * len(order), classes([(4e-4, 7, 1)]), n)
    ids3 = [2 if 'dcn' in k else (1 if 'fusion' in k else 0) for k in order]
    parts['groups_3'] = (ids3, classes([(4e-4, 7, 1), (4e-4, 9, 1), (1e-4, 7, 1)]), n)
    idsf = [1 if 'fusion' in k else 0 for k in order]
    ends = adam.offsets[1:] + [n]
    touched = sum(e - o for k, o, e in zip(order, adam.offsets, ends) if 'fusion' in k)
    parts['groups_frozen'] = (idsf, classes([(0.0, 0, 0), (4e-4, 2, 1)]), touched)
    cls = {k: adam.chunk_classes(v[0]).to(dev) for k, v in parts.items()}

    def plain():
        _lib.check(lib.sr_adam_step_f32(*ptrs, n, 7, 4e-4, 0.9, 0.99, 1e-8, 0.0, 1.0, None, None, st), 'sr_adam_step_f32')

    def grouped(key):
        arr = parts[key][1]
        _lib.check(lib.sr_adam_step_groups_f32(*ptrs, n, cls[key].data_ptr(), arr, len(arr), 0.9, 0.99, 1e-8, 0.0, 1.0, None, None, st),
                   'sr_adam_step_groups_f32')
    runs = OD(plain=plain, **{k: (lambda k=k: grouped(k)) for k in parts})
    times = {k: [] for k in runs}
    for i in range(warmup + calls):
        for k, fn in runs.items():     # interleaved: every entry point sees the same clocks and the same cache history
            ms = event_ms(fn)
            if i >= warmup:
                times[k].append(ms)
    out = OD(arena_floats=n, arena_mb=round(4 * n / 1e6, 2), parameters=len(names), fusion_floats=touched)
    for k, v in times.items():
        med = statistics.median(v)
        floats = n if k == 'plain' else parts[k][2]
        out[k] = OD(median_us=round(med * 1e3, 2), min_us=round(min(v) * 1e3, 2), max_us=round(max(v) * 1e3, 2),
                    gb_per_s=round(28.0 * floats / med / 1e6, 1))
    return out


def model_opt(**train_kw):
    train = OD(optim_g=OD(type='Adam', lr=4e-4, weight_decay=0, betas=[0.9, 0.99]), ema_decay=0.999,
               scheduler=OD(type='CosineAnnealingRestartLR', periods=[100000], restart_weights=[1], eta_min=1e-7), total_iter=100000,
               warmup_iter=-1, pixel_opt=OD(type='CharbonnierLoss', loss_weight=1.0, reduction='sum'))
    train.update(train_kw)
    return OD(name='bench', model_type='EDVRModel', scale=4, num_gpu=1, manual_seed=0, is_train=True, dist=False, rank=0, world_size=1,
              network_g=OD(NET), train=train, path=OD(pretrain_network_g=None, strict_load_g=True, resume_state=None))


def profile(fn, cap=16384):
    lib = _lib.load()
    _lib.check(lib.sr_profile_start(cap), 'sr_profile_start')
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        recs = (_lib.LaunchRecord * cap)()
        cnt = C.c_int(0)
        _lib.check(lib.sr_profile_stop(recs, cap, C.byref(cnt)), 'sr_profile_stop')
    return [recs[i] for i in range(min(cnt.value, cap))]


def bench_step(steps, dev, **train_kw):
    import logging
    logging.getLogger('basicsr').setLevel(logging.ERROR)
    model = build_model(model_opt(**train_kw))
    lq, gt = torch.rand(4, 5, 3, 64, 64, device=dev), torch.rand(4, 3, 256, 256, device=dev)
    model.feed_data(dict(lq=lq, gt=gt))
    phases = OD(forward=[], backward=[], optimiser=[], ema=[], total=[])
    book = [None]

    def fwd():
        model.gen.clear_grads()
        model.output = model.net_g(model.lq)

    def bwd():
        book[0] = LossBook()
        model.content_terms(book[0])
        book[0].objective.backward()
    for it in range(1, steps + 3):
        model.update_learning_rate(it)
        if it == 1:
            model.optimize_parameters(it)      # the model's own step once: freezes for the warm-up when tsa_iter is set
            continue
        t = [event_ms(fwd), event_ms(bwd), event_ms(lambda: model.gen.update(False)), event_ms(lambda: model.gen.blend_shadow(model.ema_decay))]
        if it > 2:
            for k, v in zip(phases, t + [sum(t)]):
                phases[k].append(v)
    recs = profile(lambda: model.optimize_parameters(steps + 3))
    lib = _lib.load()
    grouped = [r.ms for r in recs if r.kernel_id == 139]
    out = OD((k, round(statistics.median(v), 3)) for k, v in phases.items())
    out['profiled_launches'] = len(recs)
    out['profiled_kernel_ms'] = round(sum(r.ms for r in recs), 3)
    out['grouped_adam_launches'] = len(grouped)
    out['grouped_adam_ms'] = round(sum(grouped), 4)
    out['route'] = model.optimizer_g.plan_step()[0]
    out['kernel_139'] = lib.sr_kernel_name(139).decode()
    return out


def bench_deterministic(rounds, dev):
    """The ``step`` row with and without ``train.deterministic_backward``: two models of one seed in one process, one step of each
    per round, alternating, so both see the same clocks; median [min, max] over the rounds after two warm-up rounds.  Then one
    profiled step of each: launches and kernel time of the deformable convolutions' data gradient (ids 112; 184, 185, 186)."""
    import logging
    logging.getLogger('basicsr').setLevel(logging.ERROR)
    lq, gt = torch.rand(4, 5, 3, 64, 64, device=dev), torch.rand(4, 3, 256, 256, device=dev)
    models, phases = OD(), OD()
    for key, flag in (('atomic', False), ('deterministic', True)):
        torch.manual_seed(0)
        models[key] = build_model(model_opt(deterministic_backward=flag))
        models[key].feed_data(dict(lq=lq, gt=gt))
        phases[key] = OD(forward=[], backward=[], total=[])

    def step(model):
        def fwd():
            model.gen.clear_grads()
            model.output = model.net_g(model.lq)

        def bwd():
            book = LossBook()
            model.content_terms(book)
            book.objective.backward()
        t = [event_ms(fwd), event_ms(bwd), event_ms(lambda: model.gen.update(False)), event_ms(lambda: model.gen.blend_shadow(model.ema_decay))]
        return t[0], t[1], sum(t)
    for r in range(rounds + 2):
        for key, model in models.items():
            model.update_learning_rate(r + 1)
            t = step(model)
            if r >= 2:
                for k, v in zip(phases[key], t):
                    phases[key][k].append(v)
    lib = _lib.load()
    out = OD()
    for key, model in models.items():
        row = OD((k, OD(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))) for k, v in phases[key].items())
        recs = profile(lambda: model.optimize_parameters(rounds + 3))
        row['profiled_launches'] = len(recs)
        row['profiled_kernel_ms'] = round(sum(r.ms for r in recs), 3)
        row['dcn_data_gradient'] = OD((f'{i} {lib.sr_kernel_name(i).decode()}', OD(launches=sum(r.kernel_id == i for r in recs),
                                                                                   ms=round(sum(r.ms for r in recs if r.kernel_id == i), 4)))
                                      for i in (112, 184, 185, 186))
        out[key] = row
    out['rounds'] = rounds
    out['total_ratio_of_medians'] = round(out['deterministic']['total']['median_ms'] / out['atomic']['total']['median_ms'], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--deterministic', action='store_true',
                    help='only the step row, with and without train.deterministic_backward, alternating in one process (--steps rounds)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    if args.deterministic:
        print(json.dumps(OD(step_deterministic=bench_deterministic(args.steps, dev))))
        return
    out = OD(adam=bench_adam(args.calls, args.warmup, dev))
    out['step_plain'] = bench_step(args.steps, dev)
    out['step_dcn_lr_mul'] = bench_step(args.steps, dev, dcn_lr_mul=0.25)
    out['step_tsa_warmup'] = bench_step(args.steps, dev, dcn_lr_mul=0.25, tsa_iter=1000)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
