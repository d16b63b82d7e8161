"""The dispatch restatements of tests/test_convd_ops_gpu.py pinned on the host (no GPU): _wgradd_plan reproduces
sr_convd_wgrad_slab_bytes over a grid of shapes that reaches every plan, and the instance sets _convd_instance and _wgradd_plan
can produce are the template instances the code object holds (parsed from the mangled kernel names)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from image_restoration_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_convd_ops_gpu import _convd_instance, _wgradd_plan, _wgradd_slab_bytes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD = [(1, 1), (3, 1), (3, 2), (3, 3), (3, 4)]
CHANNELS = [3, 8, 24, 40, 64, 96, 128]
SHAPES = [(1, 1, 1), (2, 5, 33), (1, 19, 45), (3, 43, 700), (16, 128, 128)]
# compiled but never chosen by wgradd_plan: 2x1 pairs on the narrow rings (ksize 1, d 1 and 2: the 2x2 pair fits there), 2x2
# pairs on the wide rings (d 3 and 4: two workgroups per CU no longer fit)
WGRADD_UNREACHABLE = {(2, 1, 1, 1), (2, 1, 3, 1), (2, 1, 3, 2), (2, 2, 3, 3), (2, 2, 3, 4)}


def test_wgradd_plan_reproduces_the_slab_size():
    lib = _lib.load()
    plans = set()
    for ks, d in KD:
        for n, h, w in SHAPES:
            for cout in CHANNELS:
                for cin in CHANNELS:
                    got = lib.sr_convd_wgrad_slab_bytes(n, h, w, cout, cin, ks, d)
                    assert got == _wgradd_slab_bytes(n, h, w, cout, cin, ks, d), (ks, d, n, h, w, cout, cin)
                    ct, it = _wgradd_plan(n, h, w, cout, cin, ks, d)[:2]
                    plans.add((ct, it, ks, d))
    assert len(plans) == 10, sorted(plans)


def _instances(tmp_path):
    llvm = '/opt/rocm/lib/llvm/bin'
    for tool in ('llvm-objdump', 'llvm-readelf'):
        if not os.path.exists(os.path.join(llvm, tool)):
            pytest.fail(f'{tool} is missing from {llvm}')
    lib = shutil.copy(os.path.join(ROOT, 'image_restoration_amd', 'lib', 'libsr_hip.so'), tmp_path / 'libsr_hip.so')
    subprocess.run([os.path.join(llvm, 'llvm-objdump'), '--offloading', lib], check=True, capture_output=True, cwd=tmp_path)
    fwd, wg = set(), set()
    for f in sorted(os.listdir(tmp_path)):
        if 'gfx950' not in f:
            continue
        notes = subprocess.run([os.path.join(llvm, 'llvm-readelf'), '--notes', str(tmp_path / f)], check=True, capture_output=True,
                               text=True).stdout
        for kind, a, b, c, d in re.findall(r'(convd_f32_kernel|wgradd_f32_kernel)ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE', notes):
            (fwd if kind == 'convd_f32_kernel' else wg).add((int(a), int(b), int(c), int(d)))
    return fwd, wg


def test_code_object_instances_are_the_restated_ones(tmp_path):
    fwd, wg = _instances(tmp_path)
    restated_fwd = set()
    for ks, d in KD:
        for n, h, w in SHAPES:
            for cout in CHANNELS:
                cot, pt, _ = _convd_instance(ks, d, cout, n, h, w)
                restated_fwd.add((cot, pt, ks, d))
    assert len(fwd) == 20 and fwd == restated_fwd, (sorted(fwd ^ restated_fwd))
    restated_wg = set()
    for ks, d in KD:
        for n, h, w in SHAPES:
            for cout in CHANNELS:
                for cin in CHANNELS:
                    ct, it = _wgradd_plan(n, h, w, cout, cin, ks, d)[:2]
                    restated_wg.add((ct, it, ks, d))
    assert len(wg) == 15 and len(restated_wg) == 10
    assert restated_wg | WGRADD_UNREACHABLE == wg and not restated_wg & WGRADD_UNREACHABLE, sorted(wg ^ restated_wg)
