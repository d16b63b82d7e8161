"""RIDNet on the host side (no GPU): state_dict layout and order against the reference's own (fixture g_w_ridnet, written by
tools/make_golden_ridnet.py), initialisation, argument rules, the option files and the scale-1 paired pipeline, the inference
command line, the ledger of include/sr_hip_ridnet.h and the compiled kernels' resource use."""
import ast
import glob
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
HEADER = os.path.join(ROOT, 'include', 'sr_hip_ridnet.h')
OPTION_FILES = sorted(glob.glob(os.path.join(ROOT, 'options', '*', 'RIDNet', '*.yml')))
_GPU = 'tests/test_convd_ops_gpu.py::'


def _net(**kw):
    return ira.build_network(dict(dict(type='RIDNet', in_channels=3, mid_channels=64, out_channels=3), **kw))


def test_state_dict_keys_shapes_and_order_are_the_references(golden):
    """The official-weight converter maps tensors by position over named_parameters(): keys, shapes and ORDER must match."""
    g = golden('g_w_ridnet')
    net = _net()
    named = list(net.named_parameters())
    assert [k for k, _ in named] == [str(k) for k in g['keys']] == list(net.state_dict())
    assert np.array_equal(np.array([list(p.shape) + [0] * (4 - p.dim()) for _, p in named]), g['shapes'])
    assert len(named) == 104 and sum(p.numel() for _, p in named) == 1499371
    assert [k for k, _ in named[:4]] == ['sub_mean.weight', 'sub_mean.bias', 'add_mean.weight', 'add_mean.bias']
    assert [k for k, _ in named[-4:]] == ['body.3.ca.attention.3.weight', 'body.3.ca.attention.3.bias', 'tail.weight', 'tail.bias']
    syn = synth.ridnet_state_dict(0, in_channels=3, mid_channels=64, out_channels=3)
    assert list(syn) == [k for k, _ in named] and all(syn[k].shape == tuple(p.shape) for k, p in named)


def test_init_statistics_match_the_references(golden):
    """MeanShift exactly (eye(3) / std, -/+ 255 * mean / std); every other tensor's mean and spread like the reference's own
    initialisation (PyTorch's default; ResidualBlockNoBN at kaiming_normal * 0.1 with zero bias); every parameter trains."""
    g = golden('g_w_ridnet')
    torch.manual_seed(1)
    net = _net()
    named = list(net.named_parameters())
    for i, (k, p) in enumerate(named):
        assert p.requires_grad == bool(g['init_requires_grad'][i]) is True, k
        v = p.detach().double()
        if k.startswith(('sub_mean.', 'add_mean.')):
            assert abs(float(v.mean()) - g['init_mean'][i]) < 1e-9 and abs(float(v.std()) - g['init_std'][i]) < 1e-9, k
            continue
        ref_std = g['init_std'][i]
        if ref_std == 0:
            assert torch.count_nonzero(v) == 0, k
        elif p.numel() >= 1000:
            assert abs(float(v.std()) / ref_std - 1) < 0.1, (k, float(v.std()), ref_std)
            assert abs(float(v.mean()) - g['init_mean'][i]) < 0.1 * ref_std, k
        else:
            assert 0.3 < float(v.std()) / ref_std < 3, (k, float(v.std()), ref_std)
    w = net.sub_mean.weight.detach()[:, :, 0, 0]
    assert torch.equal(w, torch.eye(3))
    assert torch.allclose(net.sub_mean.bias.detach(), -255 * torch.tensor([0.4488, 0.4371, 0.4040]))
    assert torch.allclose(net.add_mean.bias.detach(), 255 * torch.tensor([0.4488, 0.4371, 0.4040]))


@pytest.mark.parametrize('kw', [dict(mid_channels=12), dict(mid_channels=8), dict(mid_channels=0), dict(mid_channels=520),
                                dict(in_channels=1), dict(out_channels=4), dict(num_block=0), dict(compute_dtype='bf16'),
                                dict(rgb_mean=(0.5, 0.5))])
def test_bad_configurations_are_refused(kw):
    with pytest.raises(ValueError):
        _net(**kw)


def test_cpu_input_raises():
    net = _net(mid_channels=16, num_block=1)
    with pytest.raises(_lib.SrHipError):
        net(torch.zeros(1, 3, 8, 8))
    with pytest.raises(_lib.SrHipError):
        net(torch.zeros(1, 3, 8, 8, requires_grad=True))


@pytest.mark.parametrize('path', OPTION_FILES, ids=[os.path.basename(p) for p in OPTION_FILES])
def test_option_files_parse_and_build(golden, path):
    opt = load_yaml(path)
    assert opt['network_g']['type'] == 'RIDNet' and opt['scale'] == 1
    net = ira.build_network(dict(opt['network_g']))
    assert [k for k, _ in net.named_parameters()] == [str(k) for k in golden('g_w_ridnet')['keys']]
    if 'train' in opt:
        assert opt['model_type'] == 'SRModel' and opt['train']['pixel_opt']['type'] == 'L1Loss'
        assert opt['train']['optim_g']['type'] == 'Adam' and opt['datasets']['train']['type'] == 'SyntheticPairedDataset'
        assert opt['datasets']['train']['scale'] == 1
    else:
        assert {m['crop_border'] for m in opt['val']['metrics'].values()} == {0}
        assert set(opt['val']['metrics']) == {'psnr', 'ssim'}


def test_required_option_files_exist():
    names = {os.path.relpath(p, os.path.join(ROOT, 'options')) for p in OPTION_FILES}
    assert {'train/RIDNet/train_RIDNet_synthetic.yml', 'test/RIDNet/test_RIDNet.yml'} <= names


def test_scale_one_pipelines_give_same_size_pairs(tmp_path):
    """The synthetic set of the train options and the paired-folder training crop at scale 1: LQ and GT of one size."""
    from image_restoration_amd.data import SyntheticPairedDataset
    from image_restoration_amd.data.transforms import paired_random_crop
    opt = load_yaml(os.path.join(ROOT, 'options', 'train', 'RIDNet', 'train_RIDNet_synthetic.yml'))
    ds_opt = dict(opt['datasets']['train'], phase='train', num_samples=2)
    ds = SyntheticPairedDataset(ds_opt)
    item = ds[0]
    assert item['lq'].shape == item['gt'].shape == (3, 128, 128)
    rng = np.random.default_rng(0)
    gt = rng.random((40, 52, 3), dtype=np.float32)
    lq = rng.random((40, 52, 3), dtype=np.float32)
    g2, l2 = paired_random_crop(gt, lq, 24, 1, 'x.png')
    assert g2.shape == l2.shape == (24, 24, 3)


def _args(**kw):
    base = dict(arch='RIDNet', scale=1, num_feat=64, num_block=None, num_grow_ch=32, compute_dtype='fp32')
    base.update(kw)
    return SimpleNamespace(**base)


def test_inference_generator_options():
    o = inference.generator_options(_args())
    assert o == dict(type='RIDNet', in_channels=3, mid_channels=64, out_channels=3, num_block=4)
    ira.build_network(dict(o))
    assert inference.generator_options(_args(num_feat=32, num_block=2))['mid_channels'] == 32
    for bad in (dict(scale=2), dict(scale=4), dict(compute_dtype='bf16')):
        with pytest.raises(ValueError):
            inference.generator_options(_args(**bad))


@pytest.mark.parametrize('argv', [['--arch', 'RIDNet', '--scale', '2'], ['--arch', 'RIDNet', '--scale', '4'],
                                  ['--arch', 'RIDNet', '--compute_dtype', 'bf16']])
def test_inference_command_line_refuses(argv, tmp_path):
    with pytest.raises(SystemExit) as e:
        inference.main(['--input', str(tmp_path / 'none.png'), '--output', str(tmp_path / 'o.png')] + argv)
    assert e.value.code == 2


def test_inference_help_warns_that_attention_pools_per_tile(capsys):
    with pytest.raises(SystemExit):
        inference.main(['--help'])
    out = ' '.join(capsys.readouterr().out.split())
    assert 'RIDNet' in out and 'pools over each tile' in out and '50 pixels' in out


# ------------------------------------------------------------------------------------------ ledger of sr_hip_ridnet.h
PINNED = {
    'sr_convk_pack_f32': _GPU + 'test_convd_forward',
    'sr_convd_f32': _GPU + 'test_convd_forward',
    'sr_convd_wgrad_f32': _GPU + 'test_convd_weight_gradient',
    'sr_ridnet_sub_mean_f32': _GPU + 'test_mean_shift_bands',
    'sr_ridnet_add_mean_f32': _GPU + 'test_mean_shift_bands',
    'sr_ridnet_sub_mean_bwd_f32': _GPU + 'test_mean_shift_bands',
    'sr_ridnet_add_mean_bwd_f32': _GPU + 'test_mean_shift_bands',
    'sr_ca_scale_f32': _GPU + 'test_ca_scale_bit_for_bit',
    'sr_cb8_relu_mask_f32': _GPU + 'test_relu_mask_bit_for_bit',
}
_SIZE = 'size / workspace query: host arithmetic, no kernel'
EXEMPT = {
    'sr_convk_packed_weight_floats': _SIZE,
    'sr_convd_wgrad_slab_bytes': _SIZE,
    'sr_ridnet_mean_workspace_bytes': _SIZE,
}


def _declared():
    text = open(HEADER).read()
    return set(re.findall(r'\b(sr_[a-z0-9_]+)\s*\(', text))


def test_every_declared_entry_point_is_pinned_or_exempt_and_exported():
    declared = _declared()
    assert len(declared) == 12, sorted(declared)
    assert declared == set(PINNED) | set(EXEMPT) and not set(PINNED) & set(EXEMPT)
    for s in EXEMPT:
        assert re.search(r'(_bytes|_floats)$', s), s
    assert declared == set(_lib.RIDNET_SIGNATURES) and not declared & set(_lib.SIGNATURES)
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    for s, target in PINNED.items():
        path, _, func = target.partition('::')
        assert re.fullmatch(r'tests/test_\w+_gpu\.py', path) and os.path.exists(os.path.join(ROOT, path)), (s, target)
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith('test_')}
        assert func in tests, (s, target)


def test_size_queries():
    lib = _lib.load()
    assert lib.sr_convk_packed_weight_floats(64, 64, 1, 0) == 64 * 64
    assert lib.sr_convk_packed_weight_floats(3, 64, 3, 0) == 32 * 64 * 9
    assert lib.sr_convk_packed_weight_floats(3, 64, 3, 1) == 64 * 8 * 9
    assert lib.sr_convk_packed_weight_floats(3, 64, 2, 0) == 0
    assert lib.sr_ridnet_mean_workspace_bytes(2, 64, 64) == 256 and lib.sr_ridnet_mean_workspace_bytes(0, 1, 1) == 0
    assert lib.sr_convd_wgrad_slab_bytes(16, 128, 128, 64, 64, 3, 4) > 0 and lib.sr_convd_wgrad_slab_bytes(1, 8, 8, 8, 8, 3, 5) == 0
    names = [lib.sr_kernel_name(i).decode() for i in range(81, 91)]
    assert names[0] == names[1] == 'convd_f32_kernel' and names[2] == names[3] == 'wgradd_f32_kernel'


def test_new_kernels_use_no_scratch_no_spills_and_at_most_256_vgprs(tmp_path):
    llvm = '/opt/rocm/lib/llvm/bin'
    for tool in ('llvm-objdump', 'llvm-readelf'):
        if not os.path.exists(os.path.join(llvm, tool)):
            pytest.fail(f'{tool} is missing from {llvm}')
    lib = shutil.copy(os.path.join(ROOT, 'image_restoration_amd', 'lib', 'libsr_hip.so'), tmp_path / 'libsr_hip.so')
    subprocess.run([os.path.join(llvm, 'llvm-objdump'), '--offloading', lib], check=True, capture_output=True, cwd=tmp_path)
    found = {}
    pat = r'(convd_f32_kernel|wgradd_f32_kernel|convk_pack|sub_mean_kernel|add_mean_kernel|mean_bwd_(partial|finish)_kernel|cb8_stream_kernel)'
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
                cur = found.setdefault(val, {}) if re.search(pat, val) else None
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count'):
                cur[key] = int(val)
    assert sum('convd_f32_kernel' in k for k in found) == 20 and sum('wgradd_f32_kernel' in k for k in found) == 15, sorted(found)
    for name, md in found.items():
        assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 \
            and md.get('sgpr_spill_count', 0) == 0 and md['vgpr_count'] <= 256, (name, md)
