"""The register, workgroup and LDS budget of the split Winograd fp32 kernels (csrc/conv_wino_f32.hip); runs without a GPU: reads
libsr_hip.so's gfx950 code objects the way tests/test_wino_codeobj_host.py does.

``conv_wino_f32_kernel<NW>`` splits the 16 transform points of a patch row over two waves (8 points = 128 accumulator registers
each), so that two waves share a SIMD: that holds only while a wave takes at most 256 of the SIMD's 512 registers per lane (VGPR and
AGPR together: ``.vgpr_count`` is the unified count on gfx950), without scratch.  A workgroup is 2 NW waves, and the NW = 2 variant
has to stay at 80 KiB of LDS or less so that two of its workgroups fit on a CU's 160 KiB."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'image_restoration_amd', 'lib', 'libsr_hip.so')
LLVM = '/opt/rocm/lib/llvm/bin'
KEYS = ('vgpr_count', 'agpr_count', 'private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'max_flat_workgroup_size',
        'group_segment_fixed_size')
XROW = 66


def wino_lds_bytes(nw):
    """csrc/conv_wino_f32.hip's wino_lds_bytes<NW>(), restated: three X images of whole 1 KiB pieces (a multiple of NW of them) and
    two 16 KiB U chunks."""
    unit = nw * 1024
    x_bytes = ((2 * nw + 2) * XROW * 32 + unit - 1) // unit * unit
    return 3 * x_bytes + 2 * 16 * 1024


@pytest.fixture(scope='module')
def wino_kernels(tmp_path_factory):
    """NW -> metadata of conv_wino_f32_kernel<NW> in the library's gfx950 code objects."""
    for tool in ('llvm-objdump', 'llvm-readelf'):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.fail(f'{tool} is missing from {LLVM}')
    work = tmp_path_factory.mktemp('wino_split_codeobj')
    lib = shutil.copy(LIB, work / 'libsr_hip.so')     # llvm-objdump --offloading extracts next to its input
    subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '--offloading', lib], check=True, capture_output=True, cwd=work)
    kernels = {}
    for f in sorted(os.listdir(work)):
        if 'gfx950' not in f:
            continue
        notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', str(work / f)], check=True, capture_output=True,
                               text=True).stdout
        # one list item of amdhsa.kernels per kernel, its keys in alphabetical order (.agpr_count first, .name in the middle): collect
        # a whole item, then file it under its name
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


def test_every_instance_is_found_with_all_its_metadata(wino_kernels):
    assert sorted(wino_kernels) == [1, 2, 4], wino_kernels
    for nw, md in wino_kernels.items():
        assert set(KEYS) <= set(md), (nw, md)


def test_two_waves_per_simd_without_scratch(wino_kernels):
    for nw, md in wino_kernels.items():
        print(f'NW={nw}: vgpr_count {md["vgpr_count"]} (agpr {md["agpr_count"]})')
        assert md['vgpr_count'] <= 256, (nw, md)
        assert md['agpr_count'] <= md['vgpr_count'], (nw, md)   # the AGPRs are part of the unified count
        assert md['private_segment_fixed_size'] == 0, (nw, md)
        assert md['vgpr_spill_count'] == 0, (nw, md)
        assert md['sgpr_spill_count'] == 0, (nw, md)


def test_workgroup_is_two_waves_per_patch_row(wino_kernels):
    for nw, md in wino_kernels.items():
        assert md['max_flat_workgroup_size'] == 128 * nw, (nw, md)


def test_two_nw2_workgroups_fit_on_a_cu(wino_kernels):
    assert wino_kernels[2]['group_segment_fixed_size'] + wino_lds_bytes(2) <= 80 * 1024, (wino_kernels[2], wino_lds_bytes(2))
    for nw, md in wino_kernels.items():   # and every variant launches at all: 160 KiB per CU
        assert md['group_segment_fixed_size'] + wino_lds_bytes(nw) <= 160 * 1024, (nw, md)
