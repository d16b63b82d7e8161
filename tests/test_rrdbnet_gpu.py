"""Parity of the HIP path (through the C ABI) against the golden vectors of the reference and
against the oracle on seeded inputs.  Tolerance: BASELINE.json north_star = 1e-3 max abs (fp32);
the fp32-MFMA path is expected ~1e-5, asserted at 1e-4 so a regression in summation shows early."""
import numpy as np
import pytest
import torch

import image_restoration_amd as ira
from image_restoration_amd import hip_ops as H
from image_restoration_amd.utils import synth

pytestmark = pytest.mark.gpu

TOL_SPEC = 1e-3  # north_star
TOL = 1e-4       # what we actually hold


def _net(cfg, seed, dev):
    net = ira.build_network(dict(type='RRDBNet', **cfg)).to(dev).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.rrdbnet_state_dict(seed, **cfg).items()}, strict=True)
    return net


def _err(a, b):
    return float(np.abs(a.detach().cpu().numpy() - b).max())


def test_layout_roundtrip(cuda):
    x = torch.from_numpy(synth.signed_input(1, (2, 19, 7, 11))).to(cuda)
    t = H.nchw_to_cb8(x)
    assert t.cbn == 3
    torch.cuda.synchronize()
    assert torch.equal(H.cb8_to_nchw(t, 19), x)
    assert float(t.buf[:, 2, :, :, 3:].abs().max()) == 0.0  # pad channels are zero


def test_single_conv_variants(cuda):
    """One fused conv against F.conv2d (CPU) for the shapes the network uses, incl. ragged edges,
    upsample, residual epilogue and the NCHW store."""
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    for (cin, cout, h, w, ups, nchw) in [(64, 32, 12, 12, False, False), (96, 32, 9, 33, False, False),
                                         (192, 64, 8, 40, False, False), (64, 64, 5, 7, True, False),
                                         (64, 3, 17, 35, False, True), (8, 64, 6, 6, False, False),
                                         (16, 16, 10, 10, False, False)]:
        wt = torch.from_numpy((rng.standard_normal((cout, cin, 3, 3)) * 0.05).astype(np.float32))
        bs = torch.from_numpy((rng.standard_normal((cout,)) * 0.1).astype(np.float32))
        x = torch.from_numpy(synth.signed_input(cin + h, (2, cin, h, w)))
        xin = F.interpolate(x, scale_factor=2, mode='nearest') if ups else x
        ref = F.leaky_relu(F.conv2d(xin, wt, bs, padding=1), 0.2)
        pc = H.PackedConv(wt.to(cuda), bs.to(cuda))
        src = H.nchw_to_cb8(x.to(cuda))
        if nchw:
            out = torch.empty((2, cout, h, w), device=cuda)
            H.conv3x3(src, pc, act_slope=0.2, out_nchw=out)
            got = out
        else:
            res = torch.from_numpy(synth.signed_input(99, tuple(ref.shape)))
            ref = ref * 0.2 + res * 0.5
            got = H.cb8_to_nchw(H.conv3x3(src, pc, upsample=ups, act_slope=0.2, alpha=0.2,
                                           res1=H.nchw_to_cb8(res.to(cuda)), beta1=0.5), cout)
        e = _err(got, ref.numpy())
        assert e < TOL, f'conv cin={cin} cout={cout} {h}x{w} ups={ups} nchw={nchw}: {e}'


def test_rdb_block_intermediates(cuda, golden):
    """G-a: per-conv pin of one residual dense block, concat buffer never materialised."""
    g = golden('g_a_rdb')
    sd = {k: torch.from_numpy(v).to(cuda) for k, v in synth.rdb_state_dict(11, 64, 32).items()}
    cat = H.CB8.empty(1, 192, 12, 12, cuda)
    H.nchw_to_cb8(torch.from_numpy(g['x']).to(cuda), out=cat.slice(0, 64))
    for k in range(1, 5):
        pc = H.PackedConv(sd[f'conv{k}.weight'], sd[f'conv{k}.bias'], first_seg=64, seg=32)
        H.conv3x3(cat.slice(0, 64 + 32 * (k - 1)), pc, out=cat.slice(64 + 32 * (k - 1), 32), act_slope=0.2)
        e = _err(H.cb8_to_nchw(cat.slice(64 + 32 * (k - 1), 32), 32), g[f'x{k}'])
        assert e < TOL, f'x{k}: {e}'
    pc = H.PackedConv(sd['conv5.weight'], sd['conv5.bias'], first_seg=64, seg=32)
    out = H.conv3x3(cat, pc, alpha=0.2, res1=cat.slice(0, 64), beta1=1.0)
    assert _err(H.cb8_to_nchw(out, 64), g['out']) < TOL


@pytest.mark.parametrize('name,cfg,seed,xk,yk', [
    ('g_d_c1', dict(num_in_ch=3, num_out_ch=3, scale=4, num_feat=32, num_block=1, num_grow_ch=32), 0, 'x', 'y'),
    ('g_e_full23', dict(num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32), 0, 'x', 'y'),
    ('g_f_head', dict(num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=0, num_grow_ch=32), 3, 'x', 'y'),
    ('g_l_scale', dict(num_in_ch=3, num_out_ch=3, scale=2, num_feat=16, num_block=1, num_grow_ch=8), 42, 'x_s2', 'y_s2'),
    ('g_l_scale', dict(num_in_ch=3, num_out_ch=3, scale=1, num_feat=16, num_block=1, num_grow_ch=8), 41, 'x_s1', 'y_s1'),
])
def test_network_vs_reference_goldens(cuda, golden, name, cfg, seed, xk, yk):
    g = golden(name)
    net = _net(cfg, seed, cuda)
    with torch.no_grad():
        y = net(torch.from_numpy(g[xk]).to(cuda))
    assert tuple(y.shape) == g[yk].shape
    e = _err(y, g[yk])
    assert e < TOL, f'{name} scale={cfg["scale"]}: max abs err {e} (spec {TOL_SPEC})'


def test_uint8_pre_post_convention(cuda, golden):
    """a9: uint8 BGR HWC -> net -> uint8 BGR HWC; at most 1 LSB off on <0.1% of pixels (rounding ties)."""
    from image_restoration_amd.utils.img_util import img2tensor, tensor2img
    g = golden('g_d_c1')
    net = _net(dict(num_in_ch=3, num_out_ch=3, scale=4, num_feat=32, num_block=1, num_grow_ch=32), 0, cuda)
    x = img2tensor(g['img_u8'].astype(np.float32) / 255., bgr2rgb=True, float32=True).unsqueeze(0).to(cuda)
    with torch.no_grad():
        out = tensor2img(net(x), rgb2bgr=True, min_max=(0, 1))
    diff = np.abs(out.astype(np.int32) - g['out_u8'].astype(np.int32))
    assert diff.max() <= 1 and (diff > 0).mean() < 1e-3


def test_batch_config2_shape_vs_oracle(cuda):
    """BASELINE config 2 network at a reduced batch (2 x 128x128 tiles) against the oracle run here."""
    from oracle import rrdbnet_ref as R
    cfg = dict(num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32)
    x = synth.uniform_input(1234, (2, 3, 128, 128))
    sd = synth.rrdbnet_state_dict(0, **cfg)
    with torch.no_grad():
        ref = R.rrdbnet_forward(x, sd, 4, 23).numpy()
        y = _net(cfg, 0, cuda)(torch.from_numpy(x).to(cuda))
    e = _err(y, ref)
    assert e < TOL, e


def test_batch_independence_and_determinism(cuda):
    """Size-independent properties at full config-2 size: each image of a batch of 16 equals the same image
    run alone (tiles independent), and two runs are bit-identical."""
    cfg = dict(num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32)
    net = _net(cfg, 0, cuda)
    x = torch.from_numpy(synth.uniform_input(1234, (16, 3, 128, 128))).to(cuda)
    with torch.no_grad():
        y = net(x)
        y2 = net(x)
        y5 = net(x[5:6])
    assert torch.equal(y, y2)
    assert torch.equal(y[5:6], y5)
    assert bool(torch.isfinite(y).all())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_forward_is_graph_capturable(cuda, dtype):
    """include/sr_hip.h promises that the whole-network forward neither allocates nor synchronises: capture it in a HIP graph
    (torch.cuda.graph; the bf16 forward forks / joins its image-group streams inside the capture) and replay on new input."""
    net = ira.build_network(dict(type='RRDBNet', num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=2, num_grow_ch=32,
                                 compute_dtype=dtype)).to(cuda).eval()
    x = torch.rand(16, 3, 64, 64, device=cuda)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                net(x)  # packs the weights, sizes the workspace
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = net(x)
        x.copy_(torch.rand_like(x))
        graph.replay()
        torch.cuda.synchronize()
        got = y.clone()
        assert torch.equal(got, net(x))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_invalidate_packs_reaches_the_generators_weight_images(cuda, dtype):
    """hip_ops.py promises that after a write through ``param.data``, which moves no version counter, a call of
    invalidate_packs() is enough: the next forward runs on the new weights (the bits of a fresh network loaded with them)."""
    cfg = dict(num_in_ch=3, num_out_ch=3, scale=4, num_feat=16, num_block=1, num_grow_ch=8, compute_dtype=dtype)
    net = ira.build_network(dict(type='RRDBNet', **cfg)).to(cuda).eval()
    x = torch.from_numpy(synth.uniform_input(7, (1, 3, 16, 16))).to(cuda)
    bias = net.conv_last.bias
    with torch.no_grad():
        y0 = net(x)
        version, ptr = bias._version, bias.data_ptr()
        bias.data.view(-1).copy_(torch.tensor([0.5, -0.25, 0.125], device=cuda))
        assert (bias._version, bias.data_ptr()) == (version, ptr)      # nothing torch keeps count of has moved
        H.invalidate_packs()
        y1 = net(x)
        fresh = ira.build_network(dict(type='RRDBNet', **cfg)).to(cuda).eval()
        fresh.load_state_dict(net.state_dict(), strict=True)
        want = fresh(x)
    assert torch.equal(y1, want)
    assert not torch.equal(y1, y0)
