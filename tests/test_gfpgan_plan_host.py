"""The dispatch restatement of tests/test_gfpgan_ops_gpu.py pinned on the host (no GPU): the instances _modconv_instance can
produce are the template instances of gfp_modconv_kernel / gfp_upconv_kernel the code object holds (parsed from the mangled
kernel names); the case lists of the GPU module reach what its docstring says; every decoder launch of the two product
configurations takes the instance listed here at batch 1, 2 and 16 (shapes from the network object's own decoder); and every
SR_CHECK_ARG of the six entry points of include/sr_hip_gfpgan.h is a status code with a message naming the entry point, returned
before anything is launched (fake aligned addresses, as tests/test_boundary.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

import image_restoration_amd as ira
from image_restoration_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gfpgan_ops_gpu import _assert_coverage, _modconv_instance  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = {(1, 1), (1, 2), (2, 1), (2, 2)}
# compiled but never chosen by modconv_common: none (every instance of both kernels is reachable)
MODCONV_UNREACHABLE = {'gfp_modconv_kernel': set(), 'gfp_upconv_kernel': set()}
PRODUCT = dict(type='GFPGANv1OCR', num_style_feat=256, channel_multiplier=0.5, narrow=1, num_mlp=4, input_is_latent=True,
               different_w=True, sft_half=True)


def _instances(tmp_path):
    llvm = '/opt/rocm/lib/llvm/bin'
    for tool in ('llvm-objdump', 'llvm-readelf'):
        if not os.path.exists(os.path.join(llvm, tool)):
            pytest.fail(f'{tool} is missing from {llvm}')
    lib = shutil.copy(os.path.join(ROOT, 'image_restoration_amd', 'lib', 'libsr_hip.so'), tmp_path / 'libsr_hip.so')
    subprocess.run([os.path.join(llvm, 'llvm-objdump'), '--offloading', lib], check=True, capture_output=True, cwd=tmp_path)
    found = {'gfp_modconv_kernel': set(), 'gfp_upconv_kernel': set()}
    for f in sorted(os.listdir(tmp_path)):
        if 'gfx950' not in f:
            continue
        notes = subprocess.run([os.path.join(llvm, 'llvm-readelf'), '--notes', str(tmp_path / f)], check=True, capture_output=True,
                               text=True).stdout
        for kind, a, b in re.findall(r'(gfp_modconv_kernel|gfp_upconv_kernel)ILi(\d+)ELi(\d+)EE', notes):
            found[kind].add((int(a), int(b)))
    return found


def test_code_object_instances_are_the_restated_ones(tmp_path):
    found = _instances(tmp_path)
    for up, kind in ((False, 'gfp_modconv_kernel'), (True, 'gfp_upconv_kernel')):
        restated = set()
        for n in (1, 2, 16, 64):
            for cout in (8, 32, 40, 64, 72, 96, 128, 168, 512):
                for h, w in ((1, 1), (3, 33), (4, 4), (4, 16), (5, 5), (19, 64), (67, 33), (128, 128), (256, 256)):
                    restated.add(_modconv_instance(up, n, cout, h, w)[:2])
        assert found[kind] == ALL, (kind, sorted(found[kind]))
        assert restated | MODCONV_UNREACHABLE[kind] == found[kind] and not restated & MODCONV_UNREACHABLE[kind], \
            (kind, sorted(found[kind] ^ restated))


def test_restatement_at_the_switch():
    """Both sides of the 256-workgroup switch and of GH > 4, for both kernels."""
    assert _modconv_instance(False, 255, 32, 8, 32) == (1, 1, 1, 1, 2) and _modconv_instance(False, 256, 32, 8, 32) == (1, 2, 1, 1, 1)
    assert _modconv_instance(False, 1, 64, 4, 32) == (2, 2, 1, 1, 1) and _modconv_instance(False, 1, 64, 5, 32) == (2, 1, 1, 1, 2)
    assert _modconv_instance(True, 63, 64, 7, 31) == (2, 1, 1, 1, 2) and _modconv_instance(True, 64, 64, 7, 31) == (2, 2, 1, 1, 1)
    assert _modconv_instance(True, 1, 32, 3, 32) == (1, 2, 1, 2, 1) and _modconv_instance(True, 1, 32, 4, 32) == (1, 1, 1, 2, 2)
    assert _modconv_instance(False, 1, 40, 9, 9)[:3] == (2, 1, 1) and _modconv_instance(False, 1, 72, 9, 9)[:3] == (1, 1, 3)
    assert _modconv_instance(False, 1, 168, 9, 9)[:3] == (2, 1, 3)


def test_gpu_case_lists_reach_every_instance():
    _assert_coverage()


def _decoder_launches(net):
    """[(up, cin, cout, h, w)] of the decoder's modulated convs in launch order, from the network's own modules: the constant
    input's size, each StyleConv's channels and sample mode."""
    dec = net.stylegan_decoder
    _, c0, h, w = dec.constant_input.weight.shape
    out = []
    for sc in [dec.style_conv1] + list(dec.style_convs):
        mc = sc.modulated_conv
        up = mc.sample_mode == 'upsample'
        assert mc.in_channels == (out[-1][2] if out else c0)
        out.append((up, mc.in_channels, mc.out_channels, h, w))   # (h, w): the source's size
        if up:
            h, w = 2 * h, 2 * w
    return out


# (COT, PT) per decoder launch in order: style_conv1, then per level the upsampling conv and the 3x3 conv
_SQ_SMALL = [(2, 2)] + [(2, 1)] * 10 + [(1, 2)] * 2
PRODUCT_INSTANCES = {
    (256, 256): {1: _SQ_SMALL, 2: _SQ_SMALL,
                 16: [(2, 2), (2, 2), (2, 1)] + [(2, 2)] * 8 + [(1, 2)] * 2},
    (256, 64): {1: [(2, 2), (2, 1), (2, 1), (2, 1), (2, 1), (2, 2), (2, 1), (2, 1), (2, 1)],
                2: [(2, 2), (2, 1), (2, 1), (2, 2), (2, 1), (2, 2), (2, 2), (2, 2), (2, 2)],
                16: [(2, 2), (2, 2), (2, 1)] + [(2, 2)] * 6},
}


@pytest.mark.parametrize('wh', list(PRODUCT_INSTANCES), ids=['256x256', '256x64'])
def test_product_decoder_instances(wh):
    """Every decoder launch of the product configurations at batch 1, 2 and 16.  Batch 16 (the benchmark's, and inference.py's at
    throughput) is another set of instances than batch 2: of the ten square launches on 4-row tiles at batch 2 nine take 8-row
    tiles at batch 16, gfp_upconv_kernel<2,2> among them, which the square network never runs at batch 2."""
    net = ira.build_network(dict(PRODUCT, input_width=wh[0], input_height=wh[1]))
    launches = _decoder_launches(net)
    ch = net.dec_channels
    assert launches[0] == (False, ch['4'], ch['4'], 4, 4 * wh[0] // wh[1])
    assert launches[-1][2] == ch[str(wh[1])] and (launches[-1][3], launches[-1][4]) == (wh[1], wh[0])
    assert [u for u, *_ in launches] == [False] + [True, False] * ((len(launches) - 1) // 2)
    got = {n: [_modconv_instance(up, n, cout, h, w)[:2] for up, cin, cout, h, w in launches] for n in (1, 2, 16)}
    assert got == PRODUCT_INSTANCES[wh], got
    changed = [i for i, (a, b) in enumerate(zip(got[2], got[16])) if a != b]
    ups = lambda n: {inst for (up, *_), inst in zip(launches, got[n]) if up}  # noqa: E731
    if wh == (256, 256):
        assert got[2].count((2, 1)) == 10 and len(changed) == 9 and all(got[16][i] == (2, 2) for i in changed)
        assert (2, 2) not in ups(2) and (2, 2) in ups(16)
    else:
        assert changed == [1, 4] and all(got[2][i] == (2, 1) and got[16][i] == (2, 2) for i in changed)


# ---------------------------------------------------------------------------------------------------------- the refusals
A, M = 1 << 20, (1 << 20) + 8     # aligned / 8-byte-misaligned placeholders: never dereferenced
SR_EINVAL = -1


def _refused(rc, who, word):
    msg = _lib.load().sr_last_error().decode()
    assert rc == SR_EINVAL and who in msg and word in msg, (rc, msg, who, word)


def _desc(**kw):
    d = _lib.GfpganModconvDesc()
    b = d.base
    b.in_, b.wpacked, b.bpacked, b.out = A, A, A, A
    b.in_img_stride, b.out_img_stride = 1 << 16, 1 << 16
    b.cin_pad, b.cout, b.n, b.in_h, b.in_w = 16, 32, 2, 8, 8
    b.act_slope, b.alpha = 0.2, 1.0
    d.tail.demod = A
    for k, v in kw.items():
        tgt = d.tail if k.startswith('tail_') else b
        setattr(tgt, k[5:] if k.startswith('tail_') else k, v)
    return d


BASE_REFUSALS = [
    (dict(in_=None), 'null in/wpacked/out'), (dict(wpacked=None), 'null in/wpacked/out'), (dict(out=None), 'null in/wpacked/out'),
    (dict(cin_pad=12), 'cin_pad=12'), (dict(cin_pad=0), 'cin_pad=0'), (dict(cout=12), 'bad shape'), (dict(cout=0), 'bad shape'),
    (dict(n=0), 'bad shape'), (dict(in_h=0), 'bad shape'), (dict(in_w=0), 'bad shape'),
    (dict(upsample=1), 'only in /'), (dict(out_nchw=1), 'only in /'), (dict(out_h=8), 'only in /'), (dict(out_w=8), 'only in /'),
    (dict(res1=A), 'only in /'), (dict(res2=A), 'only in /'), (dict(accumulate=1), 'only in /'), (dict(mask_src=A), 'only in /'),
    (dict(s2_channels=8), 'only in /'), (dict(out_unshuffle2=1), 'only in /'), (dict(res1_u2=1), 'only in /'),
    (dict(res1_keep_sign=1), 'only in /'),
    (dict(in_=M), 'aligned'), (dict(out=M), 'aligned'), (dict(wpacked=M), 'aligned'), (dict(bpacked=M), 'aligned'),
    (dict(in_img_stride=(1 << 16) + 2), 'aligned'), (dict(out_img_stride=(1 << 16) + 2), 'aligned'),
    (dict(in_h=16384, in_w=16384, cin_pad=8), 'too large'),           # source >= 2^32 bytes
    (dict(in_h=8192, in_w=8192, cin_pad=8, cout=64), 'too large'),    # source fits, output >= 2^31 floats
    (dict(n=(1 << 31) - 1), 'grid too large'),
]
TAIL_REFUSALS = [
    (dict(tail_demod=None), 'needs demod'),
    (dict(tail_sft_scale=A), 'go together'), (dict(tail_sft_shift=A), 'go together'),
    (dict(tail_sft_scale=A, tail_sft_shift=A, tail_sft_c0=4), 'sft_c0=4'),
    (dict(tail_sft_scale=A, tail_sft_shift=A, tail_sft_c0=32), 'sft_c0=32'),
    (dict(tail_sft_scale=A, tail_sft_shift=A, tail_sft_c0=-8), 'sft_c0=-8'),
    (dict(tail_demod=M), 'tail tensors'), (dict(tail_s_next=M), 'tail tensors'),
    (dict(tail_sft_scale=M, tail_sft_shift=A), 'tail tensors'), (dict(tail_sft_scale=A, tail_sft_shift=M), 'tail tensors'),
    (dict(tail_sft_scale=A, tail_sft_shift=A, tail_sft_scale_img_stride=6), 'tail tensors'),
    (dict(tail_sft_scale=A, tail_sft_shift=A, tail_sft_shift_img_stride=6), 'tail tensors'),
]


def test_modconv_and_upconv_refusals():
    lib = _lib.load()
    for fn, who, up in ((lib.sr_gfpgan_modconv_f32, 'sr_gfpgan_modconv_f32', False), (lib.sr_gfpgan_upconv_f32, 'sr_gfpgan_upconv_f32', True)):
        _refused(fn(None, None), who, 'null descriptor')
        for kw, word in BASE_REFUSALS:
            _refused(fn(C.byref(_desc(**kw)), None), who, word)
        if not up:   # the upsampling conv ignores bpacked and the tail
            _refused(fn(C.byref(_desc(bpacked=None)), None), who, 'null in/wpacked/out/bpacked')
            for kw, word in TAIL_REFUSALS:
                _refused(fn(C.byref(_desc(**kw)), None), who, word)


def test_blur_up_refusals():
    lib = _lib.load()
    who = 'sr_gfpgan_blur_up_f32'

    def call(t=A, ts=1 << 16, out=A, os_=1 << 16, bias=A, tail='ok', n=2, cout=32, h=8, w=8, **tk):
        tl = _lib.GfpganTail()
        tl.demod = A
        for k, v in tk.items():
            setattr(tl, k, v)
        return lib.sr_gfpgan_blur_up_f32(t, ts, out, os_, bias, 0.2, 1.0, None if tail is None else C.byref(tl), n, cout, h, w, None)
    for kw in (dict(t=None), dict(out=None), dict(bias=None), dict(n=0), dict(cout=0), dict(cout=12), dict(h=0), dict(w=0)):
        _refused(call(**kw), who, 'bad argument')
    for kw in (dict(t=M), dict(out=M), dict(bias=M), dict(ts=(1 << 16) + 2), dict(os_=(1 << 16) + 2)):
        _refused(call(**kw), who, 'aligned')
    _refused(call(tail=None), who, 'needs demod')
    for kw, word in TAIL_REFUSALS:
        _refused(call(**{k[5:]: v for k, v in kw.items()}), who, word)
    _refused(call(h=20000, w=20000, cout=8), who, 'too large')


def test_torgb_refusals():
    lib = _lib.load()
    who = 'sr_gfpgan_torgb_f32'

    def call(x=A, xs=1 << 16, w=A, s=A, bias=A, skip=None, y=A, xn=None, xns=0, sn=None, n=2, c=32, h=8, w_=8):
        return lib.sr_gfpgan_torgb_f32(x, xs, w, 1.0, s, bias, skip, y, xn, xns, sn, n, c, h, w_, None)
    for kw in (dict(x=None), dict(w=None), dict(s=None), dict(bias=None), dict(y=None), dict(n=0), dict(c=0), dict(c=12),
               dict(c=520), dict(h=0), dict(w_=0)):
        _refused(call(**kw), who, 'bad argument')
    _refused(call(xn=A), who, 'go together')
    _refused(call(sn=A), who, 'go together')
    _refused(call(skip=A, h=7), who, 'even')
    _refused(call(skip=A, w_=7), who, 'even')
    for kw in (dict(x=M), dict(xn=M, sn=A), dict(xs=(1 << 16) + 2), dict(xn=A, sn=A, xns=6)):
        _refused(call(**kw), who, 'aligned')
    _refused(call(h=16384, w_=16384, c=8), who, 'too large')
    _refused(call(n=65536), who, 'too large')


def test_style_and_norm_style_refusals():
    lib = _lib.load()
    who = 'sr_gfpgan_style_f32'

    def table(count=2, **kw):
        t = (_lib.GfpganStyleLayer * max(count, 1))()
        for row in t:
            row.mod_w, row.mod_b, row.q, row.s, row.d = A, A, A, A, A
            row.cin, row.cout, row.latent_index, row.wscale = 64, 32, 0, 0.1
        for k, v in kw.items():
            setattr(t[count - 1], k, v)
        return t

    def call(latent=A, nsf=256, layers='t', n_layers=2, n=2, **kw):
        t = table(n_layers, **kw)
        return lib.sr_gfpgan_style_f32(latent, 4096, 256, nsf, None if layers is None else t, n_layers, n, None)
    for kw in (dict(latent=None), dict(layers=None), dict(nsf=0), dict(nsf=1025), dict(n=0), dict(n=65536)):
        _refused(call(**kw), who, 'bad argument')
    _refused(call(n_layers=0), who, 'n_layers=0')
    _refused(call(n_layers=33), who, 'n_layers=33')
    for kw in (dict(mod_w=None), dict(mod_b=None), dict(s=None), dict(cin=0), dict(cin=520), dict(latent_index=-1)):
        _refused(call(**kw), who, 'bad layer 1')
    for kw in (dict(d=None), dict(q=None), dict(cout=0)):
        _refused(call(**kw), who, 'layer 1: q and d go together')
    who = 'sr_gfpgan_norm_style_f32'
    for args in ((None, A, 2, 256), (A, None, 2, 256), (A, A, 0, 256), (A, A, 65536, 256), (A, A, 2, 0), (A, A, 2, 1025)):
        _refused(lib.sr_gfpgan_norm_style_f32(*args, None), who, 'bad argument')
