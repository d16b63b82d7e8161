"""EDVR's bf16 inference forward on the GPU, by the yardstick of the EDSR / RCAN / MSRResNet bf16 forwards.

y64 is tests/edvr_restate.py in float64 (no rounding anywhere); y_model is tests/edvr_bf16_restate.py, the same float64
computation with a bf16 round trip wherever the HIP path stores or rounds a tensor.  The HIP forward must stay within
    max |y_hip - y64| <= 2 max |y_model - y64| + 4 fp32 ulp of max |y64|.
With its round trips switched off the model reproduces edvr_restate.py exactly (asserted below; both run on the CPU).

The offsets are conditioned so that the test cannot pass on zero offsets: conv_offset is zero-initialised, so every parameter is
drawn as in tests/test_edvr_gpu.py (weights N(0, 1.4^2 / fan_in), conv_offset weights N(0, 1 / fan_in), biases N(0, 0.1^2)) and the
seed is chosen from the float64 side only: seed 20 is the first of 20 .. 35 for which, in every configuration, the float64 level-1
offsets of the first frame have a mean magnitude in [0.5, 3] pixels and some level-3 samples fall outside the image.  Both
conditions are asserted.  CPU proxy (the model with its convolutions accumulated in float32, measured before any GPU run): ratio
to the bound 0.56 (nf16), 0.50 (predeblur + hr_in), 0.52 (no TSA), 0.41 (nf64, 5 frames); every seed of 20 .. 35 that meets the
offset conditions lies between 0.37 and 0.70, below the 1.5 a seed must not exceed.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from image_restoration_amd import _lib
from image_restoration_amd import inference_video as V
from image_restoration_amd.archs.edvr_arch import EDVR
from image_restoration_amd.data.data_util import generate_frame_indices

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_restate as R  # noqa: E402
import edvr_bf16_restate as M  # noqa: E402
import edvr_restate as E  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = dict(num_feat=16, num_frame=3, deformable_groups=2, num_extract_block=1, num_reconstruct_block=1)
BIG = dict(num_feat=64, num_frame=5, deformable_groups=8, num_extract_block=2, num_reconstruct_block=2)
CONFIGS = {
    # (constructor arguments, input shape, input scale (0.1 with the pre-deblur module, as tests/test_edvr_gpu.py), seed)
    'nf16': (SMALL, (2, 3, 3, 8, 12), 1.0, 20),
    'nf16_predeblur_hr': (dict(SMALL, with_predeblur=True, hr_in=True), (1, 3, 3, 16, 32), 0.1, 20),
    'nf16_notsa': (dict(SMALL, with_tsa=False), (2, 3, 3, 8, 12), 1.0, 20),
    'nf64_t5': (BIG, (1, 5, 3, 16, 16), 1.0, 20),
}
BF16_IDS = set(range(16, 32)) | {42, 43, 50, 64} | {98} | set(range(124, 130))   # sr_conv3x3_bf16's instances, the shuffle, the new kernels


def _state_dict(net, seed):
    rng = np.random.default_rng(seed)
    sd = {}
    for k, v in net.state_dict().items():
        if k.endswith('weight'):
            sc = (1.0 if 'conv_offset' in k else 1.4) / np.sqrt(v.shape[1] * v.shape[2] * v.shape[3])
            sd[k] = torch.from_numpy((rng.standard_normal(tuple(v.shape)) * sc).astype(np.float32))
        else:
            sd[k] = torch.from_numpy((rng.standard_normal(tuple(v.shape)) * 0.1).astype(np.float32))
    return sd


def _restate_kw(kw):
    return dict(num_frame=kw['num_frame'], deformable_groups=kw['deformable_groups'], num_extract_block=kw['num_extract_block'],
                num_reconstruct_block=kw['num_reconstruct_block'], hr_in=kw.get('hr_in', False),
                with_predeblur=kw.get('with_predeblur', False), with_tsa=kw.get('with_tsa', True))


@pytest.fixture(scope='module', params=list(CONFIGS))
def case(request, cuda):
    kw, shape, in_scale, seed = CONFIGS[request.param]
    net = EDVR(**kw, compute_dtype='bf16')
    sd = _state_dict(net, seed)
    x = torch.from_numpy((np.random.default_rng(seed + 1).standard_normal(shape) * in_scale).astype(np.float32))
    sd64, offs = {k: v.double() for k, v in sd.items()}, {}
    y64 = E.edvr(sd64, x.double(), offsets_out=offs, **_restate_kw(kw))
    y_off = M.edvr(sd64, x.double(), rounding=False, **_restate_kw(kw))
    y_model = M.edvr(sd64, x.double(), **_restate_kw(kw))
    net = net.to(cuda).eval()
    net.load_state_dict(sd, strict=True)
    with torch.no_grad():
        y = net(x.to(cuda))
    torch.cuda.synchronize()
    return dict(name=request.param, kw=kw, sd=sd, x=x, offs=offs, net=net, y=y, y64=y64, y_off=y_off, y_model=y_model)


def test_the_model_without_rounding_is_the_restatement(case):
    assert torch.equal(case['y_off'], case['y64'])


def test_the_case_really_deforms(case):
    dg = case['kw']['deformable_groups']
    mean_l1 = float(case['offs']['l1'].abs().mean())
    off3 = case['offs']['l3']
    h_im, w_im = R.positions(off3, dg)
    outside = float(((h_im <= -1) | (w_im <= -1) | (h_im >= off3.shape[2]) | (w_im >= off3.shape[3])).double().mean())
    print(f'{case["name"]}: mean|offset| at level 1 = {mean_l1:.3f} px, level-3 samples outside the image: {100 * outside:.1f} %')
    assert 0.5 <= mean_l1 <= 3.0 and outside > 0
    assert all(float(v.abs().max()) > 0 for k, v in case['sd'].items() if 'conv_offset' in k)


def test_forward_within_twice_the_model_distance(case):
    y, y64, ym = case['y'].cpu().double(), case['y64'], case['y_model']
    b, t, c, h, w = case['x'].shape
    s = 1 if case['kw'].get('hr_in') else 4
    assert tuple(y.shape) == (b, 3, s * h, s * w) and case['y'].dtype == torch.float32 and case['y'].grad_fn is None
    ymax = float(y64.abs().max())
    ulp = 2.0 ** (np.floor(np.log2(ymax)) - 23)
    d_model, d_hip = float((ym - y64).abs().max()), float((y - y64).abs().max())
    bound = 2 * d_model + 4 * ulp
    print(f'{case["name"]}: max|y64| {ymax:.3f}, model {d_model:.4e}, HIP {d_hip:.4e}, HIP / bound {d_hip / bound:.3f}, '
          f'HIP vs model {float((y - ym).abs().max()):.4e}')
    assert d_hip <= bound


def test_rerun_and_batch_split_are_bit_identical(case, cuda):
    net, x = case['net'], case['x'].to(cuda)
    with torch.no_grad():
        again = net(x)
        assert torch.equal(again, case['y'])
        if x.size(0) == 2:
            parts = torch.cat([net(x[:1]), net(x[1:])])
            assert torch.equal(parts, case['y'])


def test_eval_with_grad_enabled_has_no_grad_fn_and_train_mode_refuses(case, cuda):
    net, x = case['net'], case['x'].to(cuda)
    y = net(x)                                       # eval mode, grad enabled
    assert y.grad_fn is None and not y.requires_grad and torch.equal(y, case['y'])
    net.train()
    try:
        with pytest.raises(NotImplementedError, match='fp32'):
            net(x)
        with torch.no_grad():
            assert torch.equal(net(x), case['y'])    # train mode under no_grad is a forward
    finally:
        net.eval()


def test_weight_images_follow_a_parameter_update(cuda):
    kw, shape, in_scale, seed = CONFIGS['nf16']
    x = torch.from_numpy((np.random.default_rng(seed + 1).standard_normal(shape) * in_scale).astype(np.float32)).to(cuda)
    net, twin = EDVR(**kw, compute_dtype='bf16').to(cuda).eval(), EDVR(**kw, compute_dtype='bf16').to(cuda).eval()
    sd = _state_dict(net, seed)
    net.load_state_dict(sd)
    with torch.no_grad():
        y0 = net(x)
        for name, p in net.named_parameters():       # 3x3, 1x1, deformable and conv_offset weights and a bias
            if name in ('conv_first.weight', 'fusion.feat_fusion.weight', 'pcd_align.dcn_pack.l1.weight',
                        'pcd_align.cas_dcnpack.conv_offset.weight', 'conv_hr.bias'):
                p.mul_(1.25)
        twin.load_state_dict(net.state_dict())
        y1, yt = net(x), twin(x)
    assert torch.equal(y1, yt) and not torch.equal(y1, y0)


def test_only_bf16_kernels_run_between_the_conversion_and_conv_last(cuda):
    kw, shape, in_scale, seed = CONFIGS['nf16']
    lib = _lib.load()
    net = EDVR(**kw, compute_dtype='bf16').to(cuda).eval()
    net.load_state_dict(_state_dict(net, seed))
    x = torch.from_numpy((np.random.default_rng(seed + 1).standard_normal(shape) * in_scale).astype(np.float32)).to(cuda)
    with torch.no_grad():
        net(x)   # packs the weights (not profiled below)
        _lib.check(lib.sr_profile_start(512), 'sr_profile_start')
        try:
            net(x)
        finally:
            recs = (_lib.LaunchRecord * 512)()
            cnt = C.c_int(0)
            _lib.check(lib.sr_profile_stop(recs, 512, C.byref(cnt)), 'sr_profile_stop')
    ids = [recs[i].kernel_id for i in range(cnt.value)]
    print(len(ids), 'profiled launches:', sorted({lib.sr_kernel_name(i).decode() for i in ids}))
    last = len(ids) - 1 - ids[::-1].index(50)                     # conv_last: the few-cout kernel storing fp32 NCHW
    assert set(ids[:last + 1]) <= BF16_IDS, sorted(set(ids[:last + 1]) - BF16_IDS)
    assert ids[last + 1:] == [72], ids[last + 1:]                 # the x4 base of the fp32 centre frame
    assert ids.count(124) == 4                                    # three pyramid levels and the cascade, all frames in one batch
    assert ids.count(125) == 7 and ids.count(126) == 2 and ids.count(127) == 2 and ids.count(128) == 1 and ids.count(129) == 1


# ------------------------------------------------------------------------------------------------------- the clip runner
def _write_frames(folder, n=7, size=16):
    from PIL import Image
    rng = np.random.default_rng(5)
    os.makedirs(folder, exist_ok=True)
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)).save(os.path.join(folder, f'f{i:03d}.png'))


def test_clip_runner_writes_every_frame_and_the_first_is_the_reflected_clip(cuda, tmp_path):
    from PIL import Image
    src, dst, ckpt = str(tmp_path / 'in'), str(tmp_path / 'out'), str(tmp_path / 'net_g.pth')
    _write_frames(src)
    kw = dict(SMALL, num_frame=5)
    ref = EDVR(**kw, compute_dtype='bf16')
    torch.save(dict(params=_state_dict(ref, 20)), ckpt)
    V.main(['--input', src, '--output', dst, '--model_path', ckpt, '--num_frame', '5', '--compute_dtype', 'bf16', '--num_feat', '16',
            '--deformable_groups', '2', '--num_extract_block', '1', '--num_reconstruct_block', '1'])
    outs = sorted(os.listdir(dst))
    assert outs == [f'f{i:03d}.png' for i in range(7)]
    assert all(Image.open(os.path.join(dst, o)).size == (64, 64) for o in outs)
    # the first output is a direct forward on the reflected clip [2, 1, 0, 1, 2]
    net = ref.to(cuda).eval()
    net.load_state_dict(torch.load(ckpt)['params'])
    frames = V.load_frames(V.frame_paths(src)).to(cuda)
    idx = generate_frame_indices(0, 7, 5, padding='reflection')
    assert idx == [2, 1, 0, 1, 2]
    with torch.no_grad():
        y = net(frames[idx].unsqueeze(0))
    want = V.tensor2img(y, rgb2bgr=True, min_max=(0, 1))[:, :, ::-1]
    assert np.array_equal(np.asarray(Image.open(os.path.join(dst, 'f000.png')).convert('RGB')), want)
