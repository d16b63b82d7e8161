"""The segmented Adam step on the host side (no GPU): the ABI of include/sr_hip_train_groups.h (declared, bound, exported, the compute
entry point mapped to the GPU test that pins it), its profiler name, the compiled resources read from the code object, every
refusal, the class table the kernel receives, and FlatAdam's parameter groups on CPU tensors: arena order, the class partition
after a freeze and an un-freeze, torch's state_dict format and the choice between the two entry points.

The host side of adam_groups.hip is also run under the host sanitizers by the stand-alone program
tests/helpers/adam_groups_host_checks.cpp; its result is reported in DESIGN.md."""
import ast
import copy
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from image_restoration_amd import _lib, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_train_groups.h')
SR_EINVAL = -1
PINNED = {'sr_adam_step_groups_f32': 'tests/test_adam_groups_gpu.py::test_four_classes_match_float64_adam_per_segment_and_leave_the_frozen_one_alone'}
EXEMPT = {'sr_adam_class_table': 'host-only: the table the step hands to its kernel, test_class_table_is_the_plain_step_arithmetic'}


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_every_declared_entry_point_is_bound_exported_and_pinned():
    declared = set(re.findall(r'\bint\s+(sr_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(_lib.TRAIN_GROUPS_SIGNATURES) == set(PINNED) | set(EXEMPT) and len(declared) == 2
    others = set(_lib.SIGNATURES) | set(_lib.RIDNET_SIGNATURES) | set(_lib.GFPGAN_SIGNATURES) | set(_lib.EDSR_SIGNATURES) \
        | set(_lib.CA_BF16_SIGNATURES) | set(_lib.DCN_SIGNATURES) | set(_lib.EDVR_SIGNATURES) | set(_lib.EDVR_BF16_SIGNATURES) \
        | set(_lib.STYLEGAN2_SIGNATURES)
    assert not declared & others
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    base = open(os.path.join(ROOT, 'include', 'sr_hip.h')).read()
    assert not any(re.search(r'\b' + s + r'\s*\(', base) for s in declared)      # declared apart from the ledgered header
    for s, target in PINNED.items():
        path, _, func = target.partition('::')
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        assert func in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, (s, target)
    assert C.sizeof(_lib.AdamClass) == 12 and [f[0] for f in _lib.AdamClass._fields_] == ['lr', 'step', 'active']
    assert optim.MAX_CLASSES == int(re.search(r'#define SR_ADAM_MAX_CLASSES (\d+)', open(HEADER).read()).group(1)) == 16
    assert optim._ALIGN == int(re.search(r'#define SR_ADAM_CHUNK (\d+)', open(HEADER).read()).group(1)) == 64


def test_profiler_id_139_is_named_and_138_stays_empty():
    lib = _lib.load()
    assert lib.sr_kernel_name(139).decode() == 'adam_groups_kernel'
    assert lib.sr_kernel_name(138).decode() == '' and lib.sr_kernel_name(140).decode() == ''
    assert lib.sr_kernel_name(137).decode() == 'fused_bias_act_finish_kernel'


def test_code_object_has_no_scratch_no_spills_and_no_lds(tmp_path):
    llvm = '/opt/rocm/lib/llvm/bin'
    for tool in ('llvm-objdump', 'llvm-readelf'):
        if not os.path.exists(os.path.join(llvm, tool)):
            pytest.fail(f'{tool} is missing from {llvm}')
    lib = shutil.copy(os.path.join(ROOT, 'image_restoration_amd', 'lib', 'libsr_hip.so'), tmp_path / 'libsr_hip.so')
    subprocess.run([os.path.join(llvm, 'llvm-objdump'), '--offloading', lib], check=True, capture_output=True, cwd=tmp_path)
    found = {}
    for f in sorted(os.listdir(tmp_path)):
        if 'gfx950' not in f:
            continue
        notes = subprocess.run([os.path.join(llvm, 'llvm-readelf'), '--notes', str(tmp_path / f)], check=True, capture_output=True,
                               text=True).stdout
        cur, lds, kernarg = None, 0, 0
        for line in notes.splitlines():
            m = re.match(r'\s+(?:- )?\.(\w+):\s+(\S+)', line)
            if not m:
                continue
            key, val = m.groups()
            if key == 'group_segment_fixed_size':   # the keys of a kernel's entry are sorted: these two precede its name
                lds = int(val)
            elif key == 'kernarg_segment_size':
                kernarg = int(val)
            elif key == 'name' and val.startswith('_Z'):
                cur = found.setdefault(val, {}) if 'adam_groups_kernel' in val else None
                if cur is not None:
                    cur.update(group_segment_fixed_size=lds, kernarg_segment_size=kernarg)
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count'):
                cur[key] = int(val)
    assert len(found) == 1, sorted(found)
    (name, md), = found.items()
    assert md['private_segment_fixed_size'] == 0 and md['vgpr_spill_count'] == 0 and md['sgpr_spill_count'] == 0, md
    assert md['group_segment_fixed_size'] == 0 and md['vgpr_count'] <= 64, md
    assert 'ClassTable' in name and md['kernarg_segment_size'] >= 4 * 16 * 4      # the table travels by value in the arguments


# ------------------------------------------------------------------------------------------------------------ refusals
def _call(lib, **kw):
    rows = kw.pop('rows', [(1e-4, 1, 1)])
    arr = (_lib.AdamClass * max(len(rows), 1))()
    for c, (lr, step, active) in enumerate(rows):
        arr[c].lr, arr[c].step, arr[c].active = lr, step, active
    a = dict(p=256, g=512, m=768, v=1024, n=128, cls=2048, classes=arr, nc=len(rows))
    a.update(kw)
    return lib.sr_adam_step_groups_f32(a['p'], a['g'], a['m'], a['v'], a['n'], a['cls'], a['classes'], a['nc'], 0.9, 0.99, 1e-8, 0.0, 1.0,
                                       None, None, None)


def test_every_refusal_comes_before_the_launch():
    lib = _lib.load()
    seventeen = [(1e-4, 1, 1)] * 17
    for kw, needle in ((dict(p=None), b'null'), (dict(g=None), b'null'), (dict(m=None), b'null'), (dict(v=None), b'null'),
                       (dict(cls=None), b'null'), (dict(classes=None), b'null classes'),
                       (dict(p=260), b'aligned'), (dict(g=516), b'aligned'), (dict(m=8 + 768), b'aligned'), (dict(v=1028), b'aligned'),
                       (dict(n=0), b'multiple of 64'), (dict(n=-64), b'multiple of 64'), (dict(n=96), b'multiple of 64'),
                       (dict(n=1), b'multiple of 64'), (dict(n=1 << 50), b'grid'),
                       (dict(nc=0), b'outside 1..16'), (dict(rows=seventeen), b'outside 1..16'), (dict(nc=-1), b'outside 1..16'),
                       (dict(rows=[(1e-4, -1, 1)]), b'step -1 < 1'), (dict(rows=[(1e-4, 1, 1), (1e-4, -3, 1)]), b'class 1 has step -3'),
                       (dict(rows=[(1e-4, 0, 1)]), b'step 0 < 1')):
        assert _call(lib, **kw) == SR_EINVAL, kw
        err = lib.sr_last_error()
        assert b'sr_adam_step_groups_f32' in err and needle in err, (kw, err)


def _table(lib, rows, b1=0.9, b2=0.99):
    arr = (_lib.AdamClass * len(rows))()
    for c, (lr, step, active) in enumerate(rows):
        arr[c].lr, arr[c].step, arr[c].active = lr, step, active
    n = len(rows)
    lr, bc1, bc2, act = (C.c_float * n)(), (C.c_float * n)(), (C.c_float * n)(), (C.c_int * n)()
    rc = lib.sr_adam_class_table(arr, n, b1, b2, lr, bc1, bc2, act)
    return rc, list(lr), list(bc1), list(bc2), list(act)


def test_class_table_is_the_plain_step_arithmetic():
    """1 - beta1^t and sqrt(1 - beta2^t) in double from the fp32 betas, rounded once: what sr_adam_step_f32 passes to its kernel.
    A negative step is only refused in an active class."""
    lib = _lib.load()
    import numpy as np
    rows = [(2e-4, 1, 1), (5e-5, 7, 1), (1.0, -5, 0), (2e-4, 600000, 2)]
    rc, lr, bc1, bc2, act = _table(lib, rows)
    assert rc == 0 and act == [1, 1, 0, 1]
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.99))
    for c in (0, 1, 3):
        assert lr[c] == float(np.float32(rows[c][0]))
        assert bc1[c] == float(np.float32(1.0 - b1 ** rows[c][1])) and bc2[c] == float(np.float32(np.sqrt(1.0 - b2 ** rows[c][1])))
    assert (lr[2], bc1[2], bc2[2]) == (0.0, 1.0, 1.0) and bc1[3] == 1.0
    assert _table(lib, [(1e-4, -1, 1)])[0] == SR_EINVAL and b'sr_adam_class_table' in lib.sr_last_error()
    arr = (_lib.AdamClass * 1)()
    assert lib.sr_adam_class_table(arr, 1, 0.9, 0.99, None, None, None, None) == SR_EINVAL and b'null output' in lib.sr_last_error()
    assert lib.sr_adam_class_table(None, 1, 0.9, 0.99, (C.c_float * 1)(), (C.c_float * 1)(), (C.c_float * 1)(), (C.c_int * 1)()) == SR_EINVAL


# ------------------------------------------------------------------------------------------------- FlatAdam on CPU tensors
def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = dict(a=(3, 5), dcn_w=(70,), fusion_w=(2, 64), b=(1,), dcn_b=(130,))
    return {k: torch.nn.Parameter(torch.randn(s, generator=g)) for k, s in shapes.items()}


def _two_groups(ps, lr=1e-3, mul=0.25):
    normal = [p for k, p in ps.items() if 'dcn' not in k]
    dcn = [p for k, p in ps.items() if 'dcn' in k]
    return [dict(params=normal, lr=lr), dict(params=dcn, lr=lr * mul)]


def test_group_list_construction_arena_order_and_param_groups():
    ps = _params()
    before = {k: p.detach().clone() for k, p in ps.items()}
    opt = optim.FlatAdam(_two_groups(ps), 5e-4, betas=(0.9, 0.99))
    order = ['a', 'fusion_w', 'b', 'dcn_w', 'dcn_b']                      # group order, not module order
    assert [id(p) for p in opt.params] == [id(ps[k]) for k in order] and opt.group_of == [0, 0, 0, 1, 1]
    assert opt.offsets == [0, 64, 192, 256, 384] and opt.numel == 384 + 192
    for k, o in zip(order, opt.offsets):
        assert ps[k].data_ptr() == opt.flat_p.data_ptr() + 4 * o and ps[k].grad.data_ptr() == opt.flat_g.data_ptr() + 4 * o
        assert torch.equal(ps[k].detach(), before[k])
    assert len(opt.param_groups) == 2 and [g['lr'] for g in opt.param_groups] == [1e-3, 2.5e-4]
    assert [len(g['params']) for g in opt.param_groups] == [3, 2]
    for g in opt.param_groups:
        assert g['betas'] == (0.9, 0.99) and g['eps'] == 1e-8 and g['weight_decay'] == 0 and g['amsgrad'] is False
    # a group without lr takes the default; the flat form is one group, as before
    opt2 = optim.FlatAdam([dict(params=[torch.nn.Parameter(torch.zeros(3))]), dict(params=[torch.nn.Parameter(torch.zeros(3))], lr=1.0)], 5e-4)
    assert [g['lr'] for g in opt2.param_groups] == [5e-4, 1.0]
    flat = optim.FlatAdam(list(_params().values()), 5e-4)
    assert len(flat.param_groups) == 1 and flat.group_of == [0] * 5 and flat.param_groups[0]['lr'] == 5e-4
    p = torch.nn.Parameter(torch.zeros(3))
    for bad in (lambda: optim.FlatAdam([dict(params=[p]), dict(params=[p])], 1e-3), lambda: optim.FlatAdam([dict(params=[])], 1e-3),
                lambda: optim.FlatAdam([], 1e-3), lambda: optim.FlatAdam([dict(params=[p], betas=(0.5, 0.9))], 1e-3)):
        with pytest.raises(ValueError):
            bad()
    # the schedulers see one entry per group
    from image_restoration_amd.models import lr_scheduler
    s = lr_scheduler.CosineAnnealingRestartLR(opt, periods=[10], restart_weights=[1], eta_min=0)
    for _ in range(5):
        s.step()
    lrs = [g['lr'] for g in opt.param_groups]
    assert lrs[1] == pytest.approx(0.25 * lrs[0], rel=1e-15) and lrs[0] == pytest.approx(5e-4, rel=1e-12) and len(s.base_lrs) == 2


def test_class_partition_after_freeze_and_unfreeze():
    assert optim.partition_classes([0, 0, 1], [0, 0, 0], [True, True, True]) == ([0, 0, 1], [(0, 0, True), (1, 0, True)])
    assert optim.partition_classes([0, 0, 1], [4, 6, 4], [True, True, False]) == ([0, 1, 2], [(0, 4, True), (0, 6, True), (None, 0, False)])
    assert optim.partition_classes([0, 1, 1, 0], [1, 2, 3, 4], [False] * 4) == ([0, 0, 0, 0], [(None, 0, False)])
    ps = _params()
    opt = optim.FlatAdam(_two_groups(ps), 1e-3)
    assert opt.plan_step() == ('groups', [0, 0, 0, 1, 1], [(0, 0, True), (1, 0, True)])
    for k, p in ps.items():
        p.requires_grad = 'fusion' in k                                     # the warm-up: only the fusion module trains
    route, ids, classes = opt.plan_step()
    assert (route, ids, classes) == ('groups', [0, 1, 0, 0, 0], [(None, 0, False), (0, 0, True)])
    chunks = opt.chunk_classes(ids)
    assert chunks.dtype == torch.uint8 and chunks.tolist() == [0, 1, 1, 0, 0, 0, 0, 0, 0]
    opt.steps = [0, 2, 0, 0, 0]                                             # two warm-up steps later ...
    assert opt.plan_step()[1] == ids                                        # ... the ids stand: nothing to rewrite on the device
    for p in ps.values():
        p.requires_grad = True
    route, ids, classes = opt.plan_step()
    assert ids == [0, 1, 0, 2, 2] and classes == [(0, 0, True), (0, 2, True), (1, 0, True)]
    assert opt.chunk_classes(ids).tolist() == [0, 1, 1, 0, 2, 2, 2, 2, 2]
    opt.steps = [3, 5, 3, 3, 3]
    assert opt.plan_step()[1] == ids and opt.plan_step()[2] == [(0, 3, True), (0, 5, True), (1, 3, True)]
    assert opt.step_count == 5
    many = [torch.nn.Parameter(torch.zeros(1)) for _ in range(17)]
    crowded = optim.FlatAdam(many, 1e-3)
    crowded.steps = list(range(17))
    with pytest.raises(ValueError, match='17 distinct'):
        crowded.plan_step()
    with pytest.raises(_lib.SrHipError, match='no CPU fallback'):
        opt.step()


def test_single_group_all_active_equal_steps_selects_the_old_entry_point():
    ps = _params()
    opt = optim.FlatAdam(list(ps.values()), 1e-3)
    assert opt.plan_step() == ('single', None, None)
    opt.steps = [9] * 5
    assert opt.plan_step() == ('single', None, None) and opt.step_count == 9
    ps['b'].requires_grad = False
    assert opt.plan_step()[0] == 'groups'
    ps['b'].requires_grad = True
    opt.steps = [9, 9, 9, 9, 8]
    assert opt.plan_step()[0] == 'groups'
    assert optim.FlatAdam([dict(params=list(_params().values()), lr=2e-3)], 1e-3).plan_step() == ('single', None, None)
    assert optim.FlatAdam(_two_groups(_params()), 1e-3).plan_step()[0] == 'groups'


def test_state_dict_is_torch_format_and_round_trips_through_torch_adam():
    ps = _params()
    opt = optim.FlatAdam(_two_groups(ps), 1e-3, betas=(0.9, 0.99))
    fresh = opt.state_dict()
    assert fresh['state'] == {} and [g['params'] for g in fresh['param_groups']] == [[0, 1, 2], [3, 4]]
    # a torch.optim.Adam over twins with the same groups, where only the fusion parameter has trained twice and the rest once or never
    twins = {k: torch.nn.Parameter(p.detach().clone()) for k, p in ps.items()}
    ref = torch.optim.Adam(_two_groups(twins), 1e-3, betas=(0.9, 0.99))
    for rounds, names in ((2, ['fusion_w']), (1, ['fusion_w', 'a', 'dcn_b'])):
        for _ in range(rounds):
            ref.zero_grad(set_to_none=True)
            for k in names:
                twins[k].grad = torch.full_like(twins[k], 0.5)
            ref.step()
    sd = ref.state_dict()
    assert sorted(sd['state']) == [0, 1, 4]                                  # torch keeps no state for 'b' (2) and 'dcn_w' (3)
    opt.load_state_dict(copy.deepcopy(sd))
    assert opt.steps == [1, 3, 0, 0, 1] and opt.step_count == 3
    out = opt.state_dict()
    assert sorted(out['state']) == [0, 1, 4] and len(out['param_groups']) == 2
    for i in sd['state']:
        assert float(out['state'][i]['step']) == float(sd['state'][i]['step'])
        assert torch.equal(out['state'][i]['exp_avg'], sd['state'][i]['exp_avg'])
        assert torch.equal(out['state'][i]['exp_avg_sq'], sd['state'][i]['exp_avg_sq'])
    for mine, theirs in zip(out['param_groups'], sd['param_groups']):
        assert mine['params'] == theirs['params'] and mine['lr'] == theirs['lr'] and tuple(mine['betas']) == tuple(theirs['betas'])
    assert float(opt.exp_avg[192:256].abs().sum()) == 0.0                   # 'b' never took part: zero moments, no entry
    # and back: torch loads what FlatAdam wrote, on a second set of twins, and steps on
    again = {k: torch.nn.Parameter(p.detach().clone()) for k, p in ps.items()}
    ref2 = torch.optim.Adam(_two_groups(again), 1e-3, betas=(0.9, 0.99))
    ref2.load_state_dict(copy.deepcopy(out))
    back = ref2.state_dict()
    assert sorted(back['state']) == [0, 1, 4] and float(back['state'][1]['step']) == 3.0
    assert torch.equal(back['state'][4]['exp_avg_sq'], sd['state'][4]['exp_avg_sq'])
    for g in ref2.param_groups:   # torch replaces its groups by the loaded ones: give back the switches a reference file never had
        for k, v in ref2.defaults.items():
            g.setdefault(k, v)
    for p in again.values():
        p.grad = torch.ones_like(p)
    ref2.step()
    assert float(ref2.state_dict()['state'][1]['step']) == 4.0 and float(ref2.state_dict()['state'][2]['step']) == 1.0
    # a state with fewer groups is refused; differing step counts are legal (they were an assertion before)
    with pytest.raises(ValueError, match='number of parameter groups'):
        opt.load_state_dict(dict(state={}, param_groups=sd['param_groups'][:1]))
