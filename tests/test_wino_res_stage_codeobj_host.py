"""The budget of the Winograd fp32 kernels (csrc/conv_wino_f32.hip) with residual 1 staged through the LDS; runs without a GPU: reads
libsr_hip.so's gfx950 code-object metadata the way tests/test_wino_split_codeobj_host.py does.

The residual tile (NW x 16 KiB) lives in the X buffers and the exchange of the output transform in the U buffers (NW = 2, 1), so the
LDS of a workgroup stays what it was, 104 / 74 / 59 KiB for NW = 4 / 2 / 1: two NW = 2 workgroups still share a CU.  The staging adds
a buffer descriptor and two offsets to the last chunk of a 256-register wave: it must not cost scratch or a spill."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'image_restoration_amd', 'lib', 'libsr_hip.so')
LLVM = '/opt/rocm/lib/llvm/bin'
KEYS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count',
        'max_flat_workgroup_size', 'group_segment_fixed_size')
XROW = 66
LDS_KIB = {4: 104, 2: 74, 1: 59}


def wino_lds_bytes(nw):
    """csrc/conv_wino_f32.hip's wino_lds_bytes<NW>(), restated: the dynamic LDS of a launch (three X images of whole 1 KiB pieces, a
    multiple of NW of them, and two 16 KiB U chunks)."""
    unit = nw * 1024
    x_bytes = ((2 * nw + 2) * XROW * 32 + unit - 1) // unit * unit
    return 3 * x_bytes, 2 * 16 * 1024


@pytest.fixture(scope='module')
def wino_kernels(tmp_path_factory):
    """NW -> metadata of conv_wino_f32_kernel<NW> in the library's gfx950 code objects."""
    for tool in ('llvm-objdump', 'llvm-readelf'):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.fail(f'{tool} is missing from {LLVM}')
    work = tmp_path_factory.mktemp('wino_res_stage_codeobj')
    lib = shutil.copy(LIB, work / 'libsr_hip.so')     # llvm-objdump --offloading extracts next to its input
    subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '--offloading', lib], check=True, capture_output=True, cwd=work)
    kernels = {}
    for f in sorted(os.listdir(work)):
        if 'gfx950' not in f:
            continue
        notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', str(work / f)], check=True, capture_output=True,
                               text=True).stdout
        items, cur = [], None
        for line in notes.splitlines():
            m = re.match(r'  (- |  )\.(\w+):\s+(\S+)', line)   # a kernel's own keys; the keys of its .args are indented deeper
            if not m:
                continue
            if m.group(1) == '- ':
                cur = {}
                items.append(cur)
            if cur is not None:
                cur[m.group(2)] = m.group(3)
        for item in items:
            k = re.search(r'conv_wino_f32_kernelILi(\d+)E', item.get('name', ''))   # Itanium mangling of the <int NW> argument
            if k:
                kernels[int(k.group(1))] = {key: int(item[key]) for key in KEYS if key in item}
    return kernels


def test_the_three_instances_are_found(wino_kernels):
    assert sorted(wino_kernels) == [1, 2, 4], wino_kernels
    for nw, md in wino_kernels.items():
        assert set(KEYS) <= set(md), (nw, md)


def test_no_scratch_no_spills_at_most_256_registers(wino_kernels):
    for nw, md in wino_kernels.items():
        print(f'NW={nw}: vgpr_count {md["vgpr_count"]} (agpr {md["agpr_count"]}), sgpr_count {md["sgpr_count"]}')
        assert md['vgpr_count'] <= 256, (nw, md)
        assert md['agpr_count'] <= md['vgpr_count'], (nw, md)   # the AGPRs are part of the unified count on gfx950
        assert md['private_segment_fixed_size'] == 0, (nw, md)
        assert md['vgpr_spill_count'] == 0, (nw, md)
        assert md['sgpr_spill_count'] == 0, (nw, md)


def test_lds_is_unchanged_and_holds_the_residual_tile_and_the_exchange(wino_kernels):
    for nw, md in wino_kernels.items():
        x_region, u_region = wino_lds_bytes(nw)
        assert md['group_segment_fixed_size'] == 0, (nw, md)          # all of it is the launch's dynamic LDS
        assert x_region + u_region == LDS_KIB[nw] * 1024, (nw, x_region, u_region)
        exchange = 2 * nw * 8192
        if nw <= 2:
            assert nw * 16384 <= x_region, (nw, x_region)             # residual tile: 2 NW rows x 4 channel blocks x 2 KiB
            assert exchange <= u_region, (nw, u_region)
        else:
            assert exchange <= x_region, (nw, x_region)
    assert 2 * LDS_KIB[2] <= 160


def test_workgroup_size(wino_kernels):
    for nw, md in wino_kernels.items():
        assert md['max_flat_workgroup_size'] == 128 * nw, (nw, md)
