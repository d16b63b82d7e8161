"""RCAN on the host side (no GPU): state_dict layout against the reference's own keys (fixture g_v_rcan, written by
tools/make_golden_rcan.py), initialisation, argument rules, the option files, the inference command line and the compiled
channel-attention kernels' resource use."""
import glob
import math
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import image_restoration_amd as ira
from image_restoration_amd import _lib, inference
from image_restoration_amd.utils import synth
from image_restoration_amd.utils.options import load_yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_FILES = sorted(glob.glob(os.path.join(ROOT, 'options', '*', 'RCAN', '*.yml')))


def _net(**kw):
    return ira.build_network(dict(dict(type='RCAN', num_in_ch=3, num_out_ch=3), **kw))


@pytest.mark.parametrize('s', [2, 3, 4, 8])
def test_state_dict_keys_and_shapes_are_the_references(golden, s):
    g = golden('g_v_rcan')
    sd = _net(upscale=s).state_dict()
    assert list(sd) == [str(k) for k in g[f'keys_x{s}']]
    shapes = [list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()]
    assert np.array_equal(np.array(shapes), g[f'shapes_x{s}'])
    assert 'mean' not in sd
    # and the synthetic weights of the fixture have exactly these keys and shapes
    syn = synth.rcan_state_dict(0, upscale=s)
    assert list(syn) == list(sd) and all(syn[k].shape == tuple(sd[k].shape) for k in sd)


def test_option_file_net_has_the_released_checkpoint_size():
    net = _net(num_group=10, num_block=20, squeeze_factor=16, upscale=4)
    sd = net.state_dict()
    assert len(sd) == 1630 and sum(v.numel() for v in sd.values()) == 15592355
    assert [k for k, _ in net.named_parameters()] == list(sd)
    assert [id(p) for p in net._param_list()] == [id(p) for p in net.parameters()]


def test_init_is_pytorchs_default():
    """nn.Conv2d's default everywhere: weight ~ U(+-1/sqrt(fan_in)) (kaiming_uniform with a = sqrt(5)), bias ~ U(+-1/sqrt(fan_in)).
    The sample std of U(+-b) is b/sqrt(3); over the 40 body convs of 64x64x3x3 (1.47M samples) it is within 0.5 %."""
    torch.manual_seed(0)
    net = _net(num_group=2, num_block=20)
    body = torch.cat([p.detach().reshape(-1) for n, p in net.named_parameters() if n.endswith('rcab.0.weight')])
    b = 1 / math.sqrt(576)
    assert float(body.abs().max()) <= b and abs(float(body.std()) / (b / math.sqrt(3)) - 1) < 0.005
    fc1 = net.body[0].residual_group[0].ca.fc1
    w1, b1 = fc1.weight.detach(), fc1.bias.detach()
    assert float(w1.abs().max()) <= 1 / 8 and float(b1.abs().max()) <= 1 / 8 and torch.count_nonzero(b1) > 0
    w2 = net.body[0].residual_group[0].ca.fc2.weight.detach()   # fan_in 4
    assert 0.4 < float(w2.abs().max()) <= 0.5
    biases = torch.cat([p.detach() for n, p in net.named_parameters() if n.endswith('rcab.0.bias')])
    assert torch.count_nonzero(biases) == biases.numel() and float(biases.abs().max()) <= b


@pytest.mark.parametrize('kw', [dict(upscale=1), dict(upscale=5), dict(upscale=6), dict(upscale=12), dict(num_feat=12),
                                dict(num_feat=0), dict(num_feat=8), dict(num_feat=32, squeeze_factor=64), dict(num_in_ch=1),
                                dict(num_out_ch=4), dict(num_group=0), dict(num_block=0)])
def test_bad_configurations_are_refused(kw):
    with pytest.raises(ValueError):
        _net(**kw)


@pytest.mark.parametrize('s', [2, 3, 4, 8, 16])
def test_supported_upscales_build(s):
    net = _net(num_feat=16, num_group=1, num_block=1, squeeze_factor=4, upscale=s)
    assert net.upscale == s and [r for _, r in net.ups()] == ([3] if s == 3 else [2] * int(math.log2(s)))


def test_cpu_input_raises():
    net = _net(num_feat=16, num_group=1, num_block=1, squeeze_factor=4, upscale=2)
    with pytest.raises(_lib.SrHipError):
        net(torch.zeros(1, 3, 8, 8))
    with pytest.raises(_lib.SrHipError):
        net(torch.zeros(1, 3, 8, 8, requires_grad=True))


@pytest.mark.parametrize('path', OPTION_FILES, ids=[os.path.basename(p) for p in OPTION_FILES])
def test_option_files_parse_and_build(golden, path):
    opt = load_yaml(path)
    assert opt['network_g']['type'] == 'RCAN' and opt['network_g']['upscale'] == opt['scale']
    net = ira.build_network(dict(opt['network_g']))
    sd = net.state_dict()
    up4 = 64 * 256 * 9 + 256   # a x2 stage
    assert len(sd) == (1630 if opt['scale'] == 4 else 1628)
    assert sum(v.numel() for v in sd.values()) == (15592355 if opt['scale'] == 4 else 15592355 - up4)
    if opt['scale'] in (2, 4):
        # the fixture's default-width keys are those of num_block 16; the option files' 20 blocks add blocks 16..19 per group
        g = golden('g_v_rcan')
        ref = [str(k) for k in g[f'keys_x{opt["scale"]}']]
        assert [k for k in sd if not re.search(r'residual_group\.(1[6-9])\.', k)] == ref


def test_required_option_files_exist():
    names = {os.path.relpath(p, os.path.join(ROOT, 'options')) for p in OPTION_FILES}
    assert {'train/RCAN/train_RCAN_x2_synthetic.yml', 'train/RCAN/train_RCAN_x4_synthetic.yml', 'test/RCAN/test_RCAN_x4.yml'} <= names


def _args(**kw):
    base = dict(arch='RRDBNet', scale=4, num_feat=64, num_block=None, num_grow_ch=32, compute_dtype='fp32')
    base.update(kw)
    return SimpleNamespace(**base)


def test_inference_generator_options():
    for s in (2, 3, 4, 8):
        o = inference.generator_options(_args(arch='RCAN', scale=s))
        assert o == dict(type='RCAN', num_in_ch=3, num_out_ch=3, num_feat=64, num_group=10, num_block=20, squeeze_factor=16, upscale=s)
        ira.build_network(dict(o))
    o = inference.generator_options(_args(arch='RCAN', num_block=4, num_group=3, squeeze_factor=8))
    assert (o['num_block'], o['num_group'], o['squeeze_factor']) == (4, 3, 8)
    with pytest.raises(ValueError):
        inference.generator_options(_args(arch='RCAN', scale=1))
    with pytest.raises(ValueError):
        inference.generator_options(_args(arch='RCAN', compute_dtype='bf16'))


@pytest.mark.parametrize('argv', [['--arch', 'RCAN', '--scale', '1'], ['--arch', 'RCAN', '--scale', '6'],
                                  ['--arch', 'RCAN', '--compute_dtype', 'bf16']])
def test_inference_command_line_refuses(argv, tmp_path):
    with pytest.raises(SystemExit) as e:
        inference.main(['--input', str(tmp_path / 'none.png'), '--output', str(tmp_path / 'o.png')] + argv)
    assert e.value.code == 2


def test_channel_attention_abi_is_declared():
    lib = _lib.load()
    for name in ('sr_ca_workspace_bytes', 'sr_ca_squeeze_f32', 'sr_ca_excite_f32', 'sr_ca_bwd_f32', 'sr_ca_bwd_apply_f32'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # partials: n * nf/8 * ceil(hw / 2048) * 8 floats, then n*nf and n*hid, each rounded up to 64 floats
    assert lib.sr_ca_workspace_bytes(16, 64, 4, 128, 128) == 4 * (16 * 8 * 8 * 8 + 1024 + 64)
    assert lib.sr_ca_workspace_bytes(1, 8, 1, 1, 1) == 4 * 3 * 64
    assert lib.sr_ca_workspace_bytes(1, 12, 1, 1, 1) == 0 and lib.sr_ca_workspace_bytes(1, 8, 0, 1, 1) == 0
    names = [lib.sr_kernel_name(i).decode() for i in range(74, 81)]
    assert names == ['ca_partial_kernelILb0E', 'ca_squeeze_finish_kernel', 'ca_excite_kernel', 'ca_partial_kernelILb1E',
                     'ca_bwd_finish_kernel', 'ca_wgrad_kernel', 'ca_bwd_apply_kernel']


def test_channel_attention_kernels_use_no_scratch(tmp_path):
    """The seven channel-attention kernels in libsr_hip.so's gfx950 code object: no private segment, no spills."""
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
        cur = None
        for line in notes.splitlines():
            m = re.match(r'\s+(?:- )?\.(\w+):\s+(\S+)', line)
            if not m:
                continue
            key, val = m.groups()
            if key == 'name' and val.startswith('_Z'):
                cur = found.setdefault(val, {}) if re.search(r'ca_(partial|squeeze_finish|excite|bwd_finish|wgrad|bwd_apply)_kernel', val) \
                    else None
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count'):
                cur[key] = int(val)
    assert len(found) == 7, sorted(found)
    for name, md in found.items():
        assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 \
            and md.get('sgpr_spill_count', 0) == 0, (name, md)
