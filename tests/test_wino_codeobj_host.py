"""What the compiler made of the Winograd fp32 kernels (csrc/conv_wino_f32.hip); runs without a GPU: reads libsr_hip.so's gfx950
code objects the way tests/test_codeobj_host.py does.

``conv_wino_f32_kernel<4 | 2 | 1>`` keeps 16 points x 16 = 256 accumulator registers per lane plus the raw patch, its transform and
the weight operands: one wave per SIMD on the whole 512-entry register file.  A spill would put scratch traffic into every chunk of
every inference conv, so: no scratch, no spills."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'image_restoration_amd', 'lib', 'libsr_hip.so')
LLVM = '/opt/rocm/lib/llvm/bin'


@pytest.fixture(scope='module')
def wino_kernels(tmp_path_factory):
    """kernel name -> metadata of every conv_wino_f32_kernel instance in the library's gfx950 code objects."""
    for tool in ('llvm-objdump', 'llvm-readelf'):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.fail(f'{tool} is missing from {LLVM}')
    work = tmp_path_factory.mktemp('wino_codeobj')
    lib = shutil.copy(LIB, work / 'libsr_hip.so')     # llvm-objdump --offloading extracts next to its input
    subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '--offloading', lib], check=True, capture_output=True, cwd=work)
    kernels = {}
    for f in sorted(os.listdir(work)):
        if 'gfx950' not in f:
            continue
        notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', str(work / f)], check=True, capture_output=True,
                               text=True).stdout
        cur = None
        for line in notes.splitlines():
            m = re.match(r'\s+(?:- )?\.(\w+):\s+(\S+)', line)
            if not m:
                continue
            key, val = m.groups()
            if key == 'name' and val.startswith('_Z'):
                cur = kernels.setdefault(val, {}) if 'conv_wino_f32_kernel' in val else None
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count'):
                cur[key] = int(val)
    return kernels


def test_wino_kernels_have_no_scratch_and_no_spills(wino_kernels):
    assert len(wino_kernels) == 3, sorted(wino_kernels)   # NW = 4, 2, 1
    for name, md in wino_kernels.items():
        assert md['private_segment_fixed_size'] == 0, (name, md)
        assert md['vgpr_spill_count'] == 0, (name, md)
        assert md['sgpr_spill_count'] == 0, (name, md)
