"""GFPGANv1OCR on the host side (no GPU): the reference's network_g blocks, state_dict layout and order against the reference's
own (fixture g_x_gfpgan, written by tools/make_golden_gfpgan.py), initialisation, the refusals, the float64 restatement
(tests/gfpgan_restate.py) against the reference's outputs, the exact decompositions the kernels rely on, the inference command
line, and the ledger and compiled resources of include/sr_hip_gfpgan.h."""
import ast
import math
import os
import re
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_restoration_amd as ira
from image_restoration_amd import _lib, inference
from image_restoration_amd.utils import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gfpgan_restate as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sr_hip_gfpgan.h')
_OPS = 'tests/test_gfpgan_ops_gpu.py::'

# network_g of the reference's training_config/train_gfpgan_v4_*.yml (values copied; decoder_load_path is ~ in all four)
_SQ = dict(type='GFPGANv1OCR', input_width=256, input_height=256, num_style_feat=256, channel_multiplier=0.5,
           resample_kernel=[1, 3, 3, 1], decoder_load_path=None, fix_decoder=False, lr_mlp=0.01, input_is_latent=True,
           different_w=True, narrow=1, sft_half=True)
REFERENCE_BLOCKS = {
    'square_license_basic': dict(_SQ, num_mlp=4),
    'square_license_mix_pyblur': dict(_SQ, num_mlp=4),
    'square_license_affine_component': dict(_SQ, num_mlp=8),
    'rec_license_affine_component': dict(_SQ, input_height=64, num_mlp=4),
}
FIXTURE_OF = {'square_license_basic': 'sq256_mlp4', 'square_license_mix_pyblur': 'sq256_mlp4',
              'square_license_affine_component': 'sq256_mlp8', 'rec_license_affine_component': 'rect256x64'}
CONFIGS = {
    'sq': dict(input_width=32, input_height=32, num_style_feat=64, channel_multiplier=0.5, narrow=0.0625, num_mlp=2,
               input_is_latent=True, different_w=True, sft_half=True),
    'rect': dict(input_width=64, input_height=16, num_style_feat=32, channel_multiplier=0.5, narrow=0.0625, num_mlp=2,
                 input_is_latent=True, different_w=True, sft_half=True),
    'mlp': dict(input_width=16, input_height=16, num_style_feat=32, channel_multiplier=1, narrow=0.0625, num_mlp=3,
                input_is_latent=False, different_w=False, sft_half=False),
}
SEEDS = {'sq': 501, 'rect': 502, 'mlp': 503}


@pytest.mark.parametrize('name', list(REFERENCE_BLOCKS))
def test_reference_option_blocks_build_with_the_references_layout(golden, name):
    """Keys, shapes and order (noise buffers included) equal the reference's; parameter counts as measured there."""
    g = golden('g_x_gfpgan')
    net = ira.build_network(dict(REFERENCE_BLOCKS[name]))
    sd = net.state_dict()
    fx = FIXTURE_OF[name]
    assert list(sd) == [str(k) for k in g[f'keys_{fx}']]
    assert np.array_equal(np.array([list(v.shape) + [0] * (5 - v.dim()) for v in sd.values()]), g[f'shapes_{fx}'])
    counts = {'sq256_mlp4': (50505988, 241), 'rect256x64': (77399780, 169)}
    if fx in counts:
        assert (sum(p.numel() for p in net.parameters()), len(sd)) == counts[fx]
    syn = synth.gfpgan_param_shapes(**{k: v for k, v in REFERENCE_BLOCKS[name].items() if k != 'type'})
    assert [k for k, _ in syn] == list(sd) and all(s == tuple(sd[k].shape) for k, s in syn)


def test_init_statistics_match_the_references(golden):
    """randn weights (the style MLP's / lr_mlp), bias fills (modulation 1, SFT scale 1, else 0), zero noise strengths, randn noise
    buffers; with fix_decoder the decoder's parameters do not train."""
    g = golden('g_x_gfpgan')
    torch.manual_seed(0)
    net = ira.build_network(dict(REFERENCE_BLOCKS['square_license_basic'], fix_decoder=True))
    sd = net.state_dict()
    req = {k: p.requires_grad for k, p in net.named_parameters()}
    for i, (k, v) in enumerate(sd.items()):
        assert req.get(k, False) == bool(g['init_requires_grad'][i]), k
        v = v.double()
        ref_std, ref_mean = float(g['init_std'][i]), float(g['init_mean'][i])
        if ref_std == 0:
            assert float(v.std() if v.numel() > 1 else 0) == 0 and abs(float(v.mean()) - ref_mean) < 1e-12, k
        elif v.numel() >= 1000:
            assert abs(float(v.std()) / ref_std - 1) < 0.1 and abs(float(v.mean()) - ref_mean) < 0.1 * ref_std, k
        else:
            assert 0.3 < float(v.std()) / ref_std < 3, k


@pytest.mark.parametrize('kw', [dict(input_height=48), dict(input_height=4), dict(input_width=100), dict(input_width=128),
                                dict(input_is_latent=False, different_w=True), dict(compute_dtype='bf16'),
                                dict(resample_kernel=(1, 2, 1)), dict(narrow=0.01), dict(num_style_feat=2048)])
def test_bad_configurations_are_refused(kw):
    with pytest.raises(ValueError):
        ira.build_network(dict(REFERENCE_BLOCKS['square_license_basic'], **kw))


def test_forward_refusals():
    net = ira.build_network(dict(type='GFPGANv1OCR', **CONFIGS['rect'])).eval()
    with pytest.raises(_lib.SrHipError):
        net(torch.zeros(1, 3, 16, 64))
    with pytest.raises(NotImplementedError):
        net(torch.zeros(1, 3, 16, 64), save_feat_path='f.pth')
    with pytest.raises(NotImplementedError):
        net(torch.zeros(1, 3, 16, 64), load_feat_path='f.pth')


def test_the_restatement_reproduces_the_reference(golden):
    """tests/gfpgan_restate.py in float64 against the reference's float64 run (stored as float32): image, out_rgbs, style code and
    every SFT condition within the float32 storage rounding."""
    g = golden('g_x_gfpgan')
    for c, cfg in CONFIGS.items():
        sd = {k: torch.from_numpy(v).double() for k, v in synth.gfpgan_state_dict(SEEDS[c], **cfg).items()}
        out = R.forward(sd, cfg, torch.from_numpy(g[f'{c}_x']).double())
        pairs = [(out['image'], g[f'{c}_image']), (out['style_code'], g[f'{c}_style_code'])]
        pairs += [(r, g[f'{c}_rgb{i}']) for i, r in enumerate(out['out_rgbs'])]
        pairs += [(t, g[f'{c}_cond{k}']) for k, t in enumerate(out['conditions'])]
        assert len(out['conditions']) == 2 * (int(math.log2(cfg['input_height'])) - 2)
        for a, b in pairs:
            b = torch.from_numpy(b).double()
            assert a.shape == b.shape
            assert float((a - b).abs().max()) <= 4 * 2.0 ** -24 * max(1.0, float(b.abs().max())), c


def test_polyphase_upsampling_matches_the_transposed_conv_and_blur():
    """The upsampling StyleConv as the kernels compute it — parity (py, px) of the (2h+1) x (2w+1) map from taps ky = 1 (py = 1)
    or ky in {2 at row i-1, 0 at row i} (py = 0), likewise kx; then the 4x4 blur with gain 4, pad 1 — equals conv_transpose2d
    (stride 2) followed by the reference's smoothing, in float64."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 5, 6, 7, generator=g, dtype=torch.float64)
    w = torch.randn(4, 5, 3, 3, generator=g, dtype=torch.float64)
    ref = R.fir(F.conv_transpose2d(x, w.transpose(0, 1), stride=2), 1, 1, 4.0)
    n, _, h, ww = x.shape
    t = x.new_zeros(n, 4, 2 * h + 1, 2 * ww + 1)
    xp = F.pad(x, (1, 1, 1, 1))   # source index i - 1 at padded index i
    taps = {0: [(2, 0), (0, 1)], 1: [(1, 1)]}   # parity -> [(k, padded row offset of grid point i)]
    for py in (0, 1):
        for px in (0, 1):
            gh, gw = h + 1 - py, ww + 1 - px
            acc = x.new_zeros(n, 4, gh, gw)
            for ky, oy in taps[py]:
                for kx, ox in taps[px]:
                    acc += torch.einsum('oc,nchw->nohw', w[:, :, ky, kx], xp[:, :, oy:oy + gh, ox:ox + gw])
            t[:, :, py::2, px::2] = acc
    k = torch.tensor([0.25, 0.75, 0.75, 0.25], dtype=torch.float64)
    tp = F.pad(t, (1, 1, 1, 1))
    out = sum(k[a] * k[b] * tp[:, :, a:a + 2 * h, b:b + 2 * ww] for a in range(4) for b in range(4))
    assert float((out - ref).abs().max()) < 1e-12


def test_strided_blur_composites_match_the_reference_op_sequence():
    """ResBlock's downsampling: blur (pad 1) + 1x1 / s2 == the 4x4 / s2 / pad-1 conv with W (x) K (sr_conv4x4s2_f32), and blur
    (pad 2) + 3x3 / s2 == a 3x3 / pad-1 conv of the 2x pixel-unshuffled source with the composite 6x6 weight (the pack of
    GFPGANv1OCR._build_pack), in float64."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 6, 12, 16, generator=g, dtype=torch.float64)
    kb = R.blur_kernel(x)
    w1 = torch.randn(5, 6, 1, 1, generator=g, dtype=torch.float64)
    ref1 = F.conv2d(R.fir(x, 1, 1), w1, stride=2)
    assert float((F.conv2d(x, w1 * kb, stride=2, padding=1) - ref1).abs().max()) < 1e-12
    w3 = torch.randn(5, 6, 3, 3, generator=g, dtype=torch.float64)
    ref3 = F.conv2d(R.fir(x, 2, 2), w3, stride=2)
    w6 = torch.zeros(5, 6, 6, 6, dtype=torch.float64)
    for a in range(3):
        for b in range(3):
            w6[:, :, a:a + 4, b:b + 4] += w3[:, :, a, b, None, None] * kb
    wu = w6.view(5, 6, 3, 2, 3, 2).permute(0, 1, 3, 5, 2, 4).reshape(5, 24, 3, 3)
    out = F.conv2d(F.pixel_unshuffle(x, 2), wu, padding=1)
    assert float((out - ref3).abs().max()) < 1e-12


def test_to_rgb_skip_upsampling_is_the_two_tap_form():
    """upfirdn2d(skip, up 2, pad (2, 1), [1,3,3,1]^2 / 64 * 4) == per axis out[2t] = skip[t-1]/4 + 3 skip[t]/4,
    out[2t+1] = 3 skip[t]/4 + skip[t+1]/4 (zero outside): the form sr_gfpgan_torgb_f32 computes."""
    g = torch.Generator().manual_seed(2)
    s = torch.randn(2, 3, 5, 7, generator=g, dtype=torch.float64)
    ref = R.up2_fir(s)
    sp = F.pad(s, (1, 1, 1, 1))

    def axis(t, dim):  # t zero-padded by 1 on `dim` -> that axis upsampled by 2
        n = t.shape[dim] - 2
        a, b, c = t.narrow(dim, 0, n), t.narrow(dim, 1, n), t.narrow(dim, 2, n)
        ev, od = a / 4 + 3 * b / 4, 3 * b / 4 + c / 4
        return torch.stack([ev, od], dim + 1).flatten(dim, dim + 1)

    out = axis(axis(sp, 2), 3)
    assert out.shape == ref.shape
    assert float((out - ref).abs().max()) < 1e-12


def _args(**kw):
    base = dict(arch='GFPGANv1OCR', scale=1, compute_dtype='fp32', tile=0, input_width=256, input_height=256, num_style_feat=256,
                channel_multiplier=0.5, narrow=1.0, num_mlp=8)
    base.update(kw)
    return SimpleNamespace(**base)


def test_inference_generator_options():
    o = inference.generator_options(_args())
    assert o == dict(type='GFPGANv1OCR', input_width=256, input_height=256, num_style_feat=256, channel_multiplier=0.5, narrow=1.0,
                     num_mlp=8, input_is_latent=True, different_w=True, sft_half=True)
    net = ira.build_network(dict(o))
    assert len(net.state_dict()) == 249
    for bad in (dict(scale=2), dict(compute_dtype='bf16'), dict(tile=128)):
        with pytest.raises(ValueError):
            inference.generator_options(_args(**bad))


@pytest.mark.parametrize('argv', [['--scale', '2'], ['--compute_dtype', 'bf16'], ['--tile', '128'], ['--input_height', '48']])
def test_inference_command_line_refuses(argv, tmp_path):
    with pytest.raises(SystemExit) as e:
        inference.main(['--arch', 'GFPGANv1OCR', '--input', str(tmp_path / 'none.png'), '--output', str(tmp_path / 'o.png')] + argv)
    assert e.value.code == 2


def test_inference_defaults_are_the_square_product_config():
    with pytest.raises(SystemExit):
        inference.main(['--help'])
    ap_defaults = inference.generator_options(_args())
    assert (ap_defaults['input_width'], ap_defaults['input_height'], ap_defaults['num_style_feat'], ap_defaults['channel_multiplier'],
            ap_defaults['num_mlp']) == (256, 256, 256, 0.5, 8)


# ------------------------------------------------------------------------------------------ ledger of sr_hip_gfpgan.h
# the strongest pin of each entry point: every kernel instance on its production dispatch path, at the edges of its contract
PINNED = {
    'sr_gfpgan_style_f32': _OPS + 'test_style_shapes',
    'sr_gfpgan_norm_style_f32': _OPS + 'test_norm_style_edges',
    'sr_gfpgan_modconv_f32': _OPS + 'test_modconv_instances',
    'sr_gfpgan_upconv_f32': _OPS + 'test_upconv_blur_instances',
    'sr_gfpgan_blur_up_f32': _OPS + 'test_upconv_blur_instances',
    'sr_gfpgan_torgb_f32': _OPS + 'test_torgb_edges',
}


def test_every_declared_entry_point_is_pinned_and_exported():
    declared = set(re.findall(r'\b(sr_[a-z0-9_]+)\s*\(', open(HEADER).read()))
    assert declared == set(PINNED) == set(_lib.GFPGAN_SIGNATURES)
    assert not declared & (set(_lib.SIGNATURES) | set(_lib.RIDNET_SIGNATURES))
    lib = _lib.load()
    for s in declared:
        assert hasattr(lib, s), s
    for s, target in PINNED.items():
        path, _, func = target.partition('::')
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith('test_')}
        assert func in tests, (s, target)


def test_profiler_ids_resolve_to_the_new_kernels():
    lib = _lib.load()
    names = [lib.sr_kernel_name(i).decode() for i in range(91, 97)]
    assert names == ['gfp_style_kernel', 'gfp_modconv_kernel', 'gfp_upconv_kernel', 'gfp_blur_up_kernel', 'gfp_torgb_kernel',
                     'gfp_norm_kernel']
    assert lib.sr_kernel_name(97).decode() == ''


def test_new_kernels_use_no_scratch_no_spills_and_at_most_256_vgprs(tmp_path):
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
                cur = found.setdefault(val, {}) if 'gfp_' in val else None
            elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'sgpr_spill_count', 'vgpr_count'):
                cur[key] = int(val)
    assert sum('gfp_modconv_kernel' in k for k in found) == 4 and sum('gfp_upconv_kernel' in k for k in found) == 4, sorted(found)
    assert len(found) == 12, sorted(found)
    for name, md in found.items():
        assert md.get('private_segment_fixed_size', 0) == 0 and md.get('vgpr_spill_count', 0) == 0 \
            and md.get('sgpr_spill_count', 0) == 0 and md['vgpr_count'] <= 256, (name, md)
