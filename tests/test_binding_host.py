"""The call discipline of the C-ABI bindings, on the host (no GPU): hip_ops.launch and what is built on it.

The loaded library is wrapped in a recorder: size queries go through to the real libsr_hip.so (host arithmetic), every
stream-ordered entry point is recorded instead of called and returns a status the test chooses.  The device guard and the
stream lookup are replaced by fakes that note their order, so CPU tensors can stand in for device memory."""
import ctypes as C
import re

import pytest
import torch

from image_restoration_amd import _lib
from image_restoration_amd import hip_ops as H

TABLES = (_lib.SIGNATURES, _lib.RIDNET_SIGNATURES, _lib.GFPGAN_SIGNATURES, _lib.EDSR_SIGNATURES, _lib.CA_BF16_SIGNATURES)
STREAMS = {}


def _takes_stream(name):
    for tab in TABLES:
        if name in tab:
            res, args = tab[name]
            return res is C.c_int and bool(args) and args[-1] is C.c_void_p
    return False


class Recorder:
    def __init__(self, real, log):
        self.real, self.log, self.status = real, log, {}

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not _takes_stream(name):
            return fn

        def stub(*args):
            self.log.append(('call', name, args))
            return self.status.get(name, 0)
        return stub


@pytest.fixture
def rec(monkeypatch):
    log = []
    r = Recorder(_lib.load(), log)
    monkeypatch.setattr(_lib, '_lib', r)

    class Guard:
        def __init__(self, dev):
            self.dev = dev

        def __enter__(self):
            log.append(('enter', self.dev))

        def __exit__(self, *a):
            log.append(('exit', self.dev))

    class Stream:
        def __init__(self, dev):
            log.append(('stream', dev))
            self.cuda_stream = STREAMS.setdefault(str(dev), 0x1000 + 0x10 * len(STREAMS))

    monkeypatch.setattr(torch.cuda, 'device', Guard)
    monkeypatch.setattr(torch.cuda, 'current_stream', Stream)
    monkeypatch.setattr(H, '_need_cuda', lambda t, what: None)
    monkeypatch.setattr(H, '_scratch', {})
    return r


def _calls(rec):
    return [(e[1], e[2]) for e in rec.log if e[0] == 'call']


def test_launch_guards_the_device_and_passes_its_stream_last(rec):
    H.launch('sr_cb8_axpby_f32', 'dev B', 11, 22, None, 44, 0.5, 2.0, 1, 2, 3, 4)
    kinds = [(e[0], e[1]) for e in rec.log]
    # the stream of that device, looked up inside its guard, before the call; nothing after the guard is left
    assert kinds == [('enter', 'dev B'), ('stream', 'dev B'), ('call', 'sr_cb8_axpby_f32'), ('exit', 'dev B')]
    (name, args), = _calls(rec)
    assert args == (11, 22, None, 44, 0.5, 2.0, 1, 2, 3, 4, STREAMS['dev B'])
    assert args[2] is None          # None is handed to ctypes as it is: a NULL pointer
    H.launch('sr_cb8_axpby_f32', 'dev A', 1, 2, 3, 4, 1.0, 1.0, 1, 1, 1, 1)
    assert _calls(rec)[1][1][-1] == STREAMS['dev A'] != STREAMS['dev B']


def test_a_wrapper_launches_on_its_tensors_device(rec):
    dst, src = H.CB8.zeros(1, 8, 2, 2, 'cpu'), H.CB8.zeros(1, 8, 2, 2, 'cpu')
    H.cb8_axpby(dst, src, 0.5, 2.0)
    assert [e for e in rec.log if e[0] != 'call'] == [('enter', dst.device), ('stream', dst.device), ('exit', dst.device)]
    (name, args), = _calls(rec)
    assert name == 'sr_cb8_axpby_f32' and args[-1] == STREAMS[str(dst.device)]
    assert args[:-1] == (dst.ptr, dst.img_stride, src.ptr, src.img_stride, 0.5, 2.0, 1, 1, 2, 2)


def test_optional_tensors_arrive_as_null(rec):
    g = H.CB8.zeros(1, 8, 2, 2, 'cpu')
    H.upsample2x_bwd(g)
    H.linear(torch.zeros(2, 3), torch.zeros(4, 3), None)
    (n0, a0), (n1, a1) = _calls(rec)
    assert (n0, a0[4], a0[5]) == ('sr_upsample2x_bwd_f32', None, 0)
    assert (n1, a1[2]) == ('sr_linear_fwd_f32', None)


@pytest.mark.parametrize('call, symbol', [
    (lambda: H.cb8_axpby(H.CB8.zeros(1, 8, 2, 2, 'cpu'), H.CB8.zeros(1, 8, 2, 2, 'cpu')), 'sr_cb8_axpby_f32'),
    (lambda: H.conv3x3_bf16(H.CB16.zeros(1, 16, 2, 2, 'cpu'), H.PackedConvBF16(torch.zeros(16, 16, 3, 3))), 'sr_conv3x3_bf16'),
    (lambda: H.edsr_shift_in(torch.zeros(1, 3, 2, 2), (0.1, 0.2, 0.3), 255.0, bf16=True), 'sr_edsr_shift_in_bf16'),
    (lambda: H.PackedConvK(torch.zeros(8, 8, 1, 1)), 'sr_convk_pack_f32'),
])
def test_a_failing_call_names_the_symbol_that_was_called(rec, call, symbol):
    rec.status[symbol] = 7
    with pytest.raises(_lib.SrHipError) as e:
        call()
    assert re.match(re.escape(symbol) + r' failed \(status 7\): ', str(e.value))
    assert _calls(rec)[-1][0] == symbol
    assert rec.log[-1][0] == 'exit'     # the guard is left on the error path too


def test_conv3x3_and_its_bf16_twin_refuse_each_others_keywords(rec):
    s8, p8 = H.CB8.zeros(1, 8, 2, 2, 'cpu'), H.PackedConv(torch.zeros(8, 8, 3, 3))
    s16, p16 = H.CB16.zeros(1, 16, 2, 2, 'cpu'), H.PackedConvBF16(torch.zeros(16, 16, 3, 3))
    for kw in ({'s2_channels': 8}, {'s2_side': 1}, {'out_unshuffle2': True}, {'res1_u2': True}, {'res1_keep_sign': True}):
        with pytest.raises(TypeError):
            H.conv3x3(s8, p8, **kw)
        H.conv3x3_bf16(s16, p16, **({'res1': s16, **kw} if 'res1' in next(iter(kw)) else kw))
    for kw in ({'accumulate': True}, {'mask_cb0': 1}):
        with pytest.raises(TypeError):
            H.conv3x3_bf16(s16, p16, **kw)
        H.conv3x3(s8, p8, **kw)
    # fp32 takes mask_cb0 from its keyword; bf16 always passes 0
    H.conv3x3(s8, p8, mask=s8, mask_cb0=3)
    H.conv3x3_bf16(s16, p16, mask=s16)
    d8, d16 = (a[0]._obj for _, a in _calls(rec)[-2:])
    assert (d8.mask_cb0, d8.mask_cbn, d16.mask_cb0, d16.mask_cbn) == (3, 1, 0, 1)
    assert (d8.mask_src, d16.mask_src) == (s8.ptr, s16.ptr)


@pytest.mark.parametrize('cls, block, dtype, esize', [(H.CB8, 8, torch.float32, 4), (H.CB16, 16, torch.bfloat16, 2)])
def test_window_arithmetic_is_the_layouts(cls, block, dtype, esize):
    """Layout [N][CB][H][W][block]: block cb of image 0 starts cb * H * W * block elements into the storage, an image is
    CB * H * W * block elements whatever the window."""
    n, cb, h, w = 2, 5, 3, 4
    buf = torch.zeros((n, cb, h, w, block), dtype=dtype)
    win = cls(buf, 2, 2)
    assert (win.n, win.h, win.w, win.channels, win.device) == (n, h, w, 2 * block, buf.device)
    assert win.img_stride == cb * h * w * block
    assert win.ptr == buf.data_ptr() + 2 * h * w * block * esize == buf[0, 2].data_ptr()
    sub = win.slice(block, block)
    assert type(sub) is cls and sub.buf is buf and (sub.cb0, sub.cbn, sub.channels) == (3, 1, block)
    assert sub.ptr == buf[0, 3].data_ptr() and sub.img_stride == win.img_stride
    whole = cls(buf)
    assert (whole.cb0, whole.cbn, whole.ptr) == (0, cb, buf.data_ptr())
    for bad in (lambda: win.slice(block // 2, block), lambda: win.slice(0, block + 1), lambda: cls(buf, 4, 2), lambda: cls(buf, -1),
                lambda: cls(buf.float() if dtype is torch.bfloat16 else buf.bfloat16()), lambda: cls(buf[:, :, :, :, :block // 2]),
                lambda: cls(buf[:, ::2])):
        with pytest.raises(AssertionError):
            bad()
    e, z = cls.empty(3, block + 1, 2, 5, 'cpu'), cls.zeros(3, block + 1, 2, 5, 'cpu')
    assert type(e) is cls and type(z) is cls and e.buf.shape == z.buf.shape == (3, 2, 2, 5, block) and e.buf.dtype == dtype
    assert not z.buf.any()


PACKED = [(H.PackedConv, 3, 'sr_conv3x3_pack_f32', 8), (H.PackedConvK, 3, 'sr_convk_pack_f32', 8), (H.PackedConvK, 1, 'sr_convk_pack_f32', 8),
          (H.PackedConv4x4s2, 4, 'sr_conv4x4s2_pack_f32', 8), (H.PackedConvBF16, 3, 'sr_conv3x3_pack_bf16', 16)]


@pytest.mark.parametrize('cls, k, symbol, block', PACKED)
def test_packed_weights_allocate_a_bias_image_only_for_a_forward_image_with_bias(rec, cls, k, symbol, block):
    cout, cin = 20, 24
    w, b = torch.zeros(cout, cin, k, k), torch.zeros(cout)
    rup = lambda c: (c + block - 1) // block * block   # noqa: E731
    for bias, mode, has_b in ((b, 0, True), (None, 0, False), (b, 1, False), (None, 1, False)):
        del rec.log[:]
        pc = cls(w, bias, mode=mode)
        (name, args), = _calls(rec)
        assert name == symbol and pc.mode == mode
        assert (pc.cout, pc.src_channels) == ((cout, rup(cin)) if mode == 0 else (rup(cin), rup(cout)))
        assert (pc.b is not None) == has_b
        assert args[0] == w.data_ptr() and args[-3] == pc.w.data_ptr()
        if has_b:
            assert args[1] == b.data_ptr() and args[-2] == pc.b.data_ptr() and pc.b.dtype == torch.float32
        else:
            assert args[1] is None and args[-2] is None
        assert args[2:4] == (cout, cin) and args[-4] == mode
    assert pc.w.dtype == (torch.bfloat16 if block == 16 else torch.float32)


def test_packed_weights_keep_their_attributes_and_errors(rec):
    w3 = torch.zeros(8, 48, 3, 3)
    pc = H.PackedConv(w3, None, 16, 16)
    assert pc.cin_pad == 48 and not hasattr(pc, 'ksize')     # convd reads getattr(pc, 'ksize', 3)
    assert _calls(rec)[-1][1][2:7] == (8, 48, 16, 16, 0)
    assert H.PackedConvBF16(w3, None, first_seg=16, seg=32).cin_pad == 48
    assert H.PackedConvK(torch.zeros(8, 8, 1, 1)).ksize == 1 and H.PackedConvK(w3).ksize == 3
    p4 = H.PackedConv4x4s2(torch.zeros(8, 12, 4, 4))
    assert (p4.conv_cout, p4.conv_cin) == (8, 12)
    for cls in (H.PackedConv, H.PackedConvBF16):
        with pytest.raises(ValueError, match=re.escape('cin=48 is not first_seg=16 + k*seg=5')):
            cls(w3, None, 16, 5)
    for cls, bad in ((H.PackedConv, 5), (H.PackedConvK, 5), (H.PackedConv4x4s2, 3)):
        with pytest.raises(AssertionError):
            cls(torch.zeros(8, 8, bad, bad))


def test_conv4x4s2_wgrad_adds_into_a_zero_filled_dweight(rec):
    src, dy = H.CB8.zeros(2, 16, 6, 8, 'cpu'), H.CB8.zeros(2, 16, 3, 4, 'cpu')
    real_empty = torch.empty
    try:    # a fresh ``empty`` tensor that happens to be zero must not pass for a zero-filled one
        torch.empty = lambda *a, **k: real_empty(*a, **k).fill_(1)
        dw, db = H.conv4x4s2_wgrad(src, dy, 12, 16, want_bias=True)
    finally:
        torch.empty = real_empty
    assert dw.shape == (12, 16, 4, 4) and not dw.any() and db.shape == (12,)
    (name, args), = _calls(rec)
    d = args[0]._obj
    assert name == 'sr_conv4x4s2_wgrad_f32' and (d.dweight, d.dbias, d.accumulate) == (dw.data_ptr(), db.data_ptr(), 0)
    assert d.slab_bytes == _lib.load().sr_conv3x3_wgrad_slab_bytes(2, 3, 4) and d.slab == H.scratch(src.device, 1, 'slab').data_ptr()


def test_wgrad_targets_are_fresh_tensors_or_the_callers_arena(rec):
    src, dy = H.CB8.zeros(2, 16, 4, 6, 'cpu'), H.CB8.zeros(2, 16, 4, 6, 'cpu')
    dw, db = H.conv3x3_wgrad(src, dy, 12, 16, want_bias=False)
    assert dw.shape == (12, 16, 3, 3) and db is None
    assert H.conv3x3_wgrad(src, dy, 12, 16, out=(0x7000, 0x7100)) is None
    assert H.convd_wgrad(src, dy, 12, 16, 3, 2, out=(0x7000, None)) == (None, None)
    d0, d1, d2 = (a[0]._obj for _, a in _calls(rec))
    assert (d0.dweight, d0.dbias, d0.accumulate) == (dw.data_ptr(), None, 0)
    assert (d1.dweight, d1.dbias, d1.accumulate) == (0x7000, 0x7100, 1)
    assert (d2.base.dweight, d2.base.dbias, d2.base.accumulate, d2.ksize, d2.dilation) == (0x7000, None, 1, 3, 2)
    for d in (d0, d1, d2.base):
        assert (d.x, d.x_img_stride, d.cin_pad, d.in_h, d.in_w, d.upsample) == (src.ptr, src.img_stride, 16, 4, 6, 0)
        assert (d.dy, d.dy_img_stride, d.cout, d.cin, d.first_seg, d.seg, d.n, d.scale) == (dy.ptr, dy.img_stride, 12, 16, 16, 0, 2, 1.0)


def test_reduce_ws_is_the_query_and_the_shared_scratch(rec):
    ws, nbytes = H.reduce_ws('cpu', 24)
    assert nbytes == _lib.load().sr_reduce_workspace_bytes(24) and ws.numel() >= nbytes and ws.dtype == torch.uint8
    ws8, nbytes8 = H.reduce_ws('cpu')
    assert nbytes8 == _lib.load().sr_reduce_workspace_bytes(8) and ws8 is H.scratch('cpu', 1)
