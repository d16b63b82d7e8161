"""MSRResNet on the host side (no GPU): state_dict layout against the reference's own keys (fixture g_u_msrresnet, written by
tools/make_golden_msrresnet.py), initialisation, argument rules, the option files and the inference command line."""
import glob
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import image_restoration_amd as ira
from image_restoration_amd import _lib, inference
from image_restoration_amd.archs.arch_util import ResidualBlockNoBN
from image_restoration_amd.utils import synth
from image_restoration_amd.utils.options import load_yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_FILES = sorted(glob.glob(os.path.join(ROOT, 'options', '*', 'SRResNet_SRGAN', '*.yml')))


def _net(**kw):
    return ira.build_network(dict(type='MSRResNet', **kw))


@pytest.mark.parametrize('s', [2, 3, 4])
def test_state_dict_keys_and_shapes_are_the_references(golden, s):
    g = golden('g_u_msrresnet')
    sd = _net(upscale=s).state_dict()
    assert list(sd) == [str(k) for k in g[f'keys_x{s}']]
    assert len(sd) == (74 if s == 4 else 72)
    shapes = [list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()]
    assert np.array_equal(np.array(shapes), g[f'shapes_x{s}'])
    # and the synthetic weights of the fixture have exactly these keys and shapes
    syn = synth.msrresnet_state_dict(0, upscale=s)
    assert list(syn) == list(sd) and all(syn[k].shape == tuple(sd[k].shape) for k in sd)


def test_init_is_kaiming_normal_times_0_1_with_zero_biases():
    """default_init_weights(scale 0.1) on every conv: weight ~ N(0, (0.1*sqrt(2/fan_in))^2), bias 0.  Over the 16 body convs
    (589,824 samples of 64x64x3x3) the sample std is within 1 % of 0.1*sqrt(2/576) with overwhelming probability
    (relative std error of a sample std ~ 1/sqrt(2N) = 0.09 %); the mean is ~0 to 5 standard errors."""
    torch.manual_seed(0)
    net = _net()
    for name, p in net.named_parameters():
        if name.endswith('.bias'):
            assert torch.count_nonzero(p) == 0, name
    body = torch.cat([p.detach().reshape(-1) for n, p in net.named_parameters() if n.startswith('body.') and n.endswith('.weight')])
    want = 0.1 * math.sqrt(2.0 / 576)
    assert abs(float(body.std()) / want - 1) < 0.01
    assert abs(float(body.mean())) < 5 * want / math.sqrt(body.numel())
    w = net.upconv1.weight.detach()
    assert abs(float(w.std()) / want - 1) < 0.02
    w = net.conv_first.weight.detach()   # fan_in 27
    assert abs(float(w.std()) / (0.1 * math.sqrt(2.0 / 27)) - 1) < 0.1


def test_residual_block_pytorch_init_keeps_conv2d_defaults():
    torch.manual_seed(0)
    blk = ResidualBlockNoBN(num_feat=64, res_scale=0.5, pytorch_init=True)
    assert blk.res_scale == 0.5
    assert torch.count_nonzero(blk.conv1.bias) > 0   # nn.Conv2d's U(+-1/sqrt(fan_in)) bias
    assert float(blk.conv1.weight.detach().abs().max()) <= 1 / math.sqrt(576) + 1e-7


@pytest.mark.parametrize('kw', [dict(upscale=1), dict(upscale=8), dict(num_feat=12), dict(num_feat=0), dict(num_block=-1)])
def test_bad_configurations_are_refused(kw):
    with pytest.raises(ValueError):
        _net(**kw)


def test_cpu_input_raises():
    net = _net(num_feat=16, num_block=1, upscale=3)
    with pytest.raises(_lib.SrHipError):
        net(torch.zeros(1, 3, 8, 8))
    with pytest.raises(_lib.SrHipError):
        net(torch.zeros(1, 3, 8, 8, requires_grad=True))


@pytest.mark.parametrize('path', OPTION_FILES, ids=[os.path.basename(p) for p in OPTION_FILES])
def test_option_files_parse_and_build(golden, path):
    opt = load_yaml(path)
    g = golden('g_u_msrresnet')
    assert opt['network_g']['type'] == 'MSRResNet' and opt['network_g']['upscale'] == opt['scale']
    net = ira.build_network(dict(opt['network_g']))
    assert list(net.state_dict()) == [str(k) for k in g[f'keys_x{opt["scale"]}']]
    if 'network_d' in opt:
        ira.build_network(dict(opt['network_d']))
    if opt['model_type'] == 'SRGANModel':
        assert opt['train']['gan_opt']['gan_type'] == 'vanilla' and 'perceptual_opt' in opt['train']


def test_required_option_files_exist():
    names = {os.path.relpath(p, os.path.join(ROOT, 'options')) for p in OPTION_FILES}
    assert {'train/SRResNet_SRGAN/train_MSRResNet_x4_synthetic.yml', 'train/SRResNet_SRGAN/train_MSRGAN_x4_synthetic.yml',
            'test/SRResNet_SRGAN/test_MSRResNet_x4.yml'} <= names
    assert any('x3' in n for n in names)


def _args(**kw):
    base = dict(arch='RRDBNet', scale=4, num_feat=64, num_block=None, num_grow_ch=32, compute_dtype='fp32')
    base.update(kw)
    return SimpleNamespace(**base)


def test_inference_generator_options():
    # the default stays RRDBNet with today's defaults
    assert inference.generator_options(_args()) == dict(type='RRDBNet', num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=23,
                                                        num_grow_ch=32, compute_dtype='fp32')
    assert inference.generator_options(_args(compute_dtype='bf16', num_block=2))['num_block'] == 2
    for s in (2, 3, 4):
        o = inference.generator_options(_args(arch='MSRResNet', scale=s))
        assert o == dict(type='MSRResNet', num_in_ch=3, num_out_ch=3, num_feat=64, num_block=16, upscale=s)
    assert inference.generator_options(_args(arch='MSRResNet', num_block=4))['num_block'] == 4
    with pytest.raises(ValueError):
        inference.generator_options(_args(arch='MSRResNet', scale=1))
    with pytest.raises(ValueError):
        inference.generator_options(_args(arch='MSRResNet', compute_dtype='bf16'))


@pytest.mark.parametrize('argv', [['--arch', 'MSRResNet', '--scale', '1'], ['--arch', 'MSRResNet', '--compute_dtype', 'bf16'],
                                  ['--arch', 'EDSR']])
def test_inference_command_line_refuses(argv, tmp_path):
    with pytest.raises(SystemExit) as e:
        inference.main(['--input', str(tmp_path / 'none.png'), '--output', str(tmp_path / 'o.png')] + argv)
    assert e.value.code == 2
