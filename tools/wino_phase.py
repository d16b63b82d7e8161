"""Development aid: where a workgroup of the Winograd fp32 kernel spends its tile, per conv shape of the benchmark's forward (batch 16
of 128x128).  Clock ticks of s_memtime: compare phases with one another, not with microseconds.

Needs the diagnostic twin of the library (`make -C image_restoration_amd/csrc stamp`), selected with SR_HIP_LIB_PATH: the product
library has no stamp and no sr_dev_set_wino_stamps.  One lane per workgroup stamps at entry (0), behind the first barrier (1), behind
the last chunk's barrier (2), behind the exchange (3) and behind the last store (4), and at the head of the last chunk (5):

  prologue = 1 - 0   tile decoding, address work, the first chunks' DMAs land
  loop     = 2 - 1   all chunks
  exchange = 3 - 2   output transform and the exchange between the two halves
  epilogue = 4 - 3   bias, activation, residual reads, stores (issue only)
  last chunk = 2 - 5 part of the loop: the chunk under whose MFMAs residual 1 is brought into the LDS
The clocks of different XCDs are not aligned, and grouping the workgroups by blockIdx.x & 7 did not give groups with one clock
each, so the spread between the first and the last workgroup's exit (the launch's drain) is NOT measured by this tool: what a launch
costs beyond its workgroups' own timelines is the launch profiler's duration minus rounds x (the four phases).

usage: SR_HIP_LIB_PATH=image_restoration_amd/lib/libsr_hip_stamp.so python tools/wino_phase.py
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from image_restoration_amd import _lib  # noqa: E402


def _ptr(buf, cb0):
    return buf.data_ptr() + cb0 * buf.shape[2] * buf.shape[3] * 8 * 4


def _stride(buf):
    return buf.shape[1] * buf.shape[2] * buf.shape[3] * 8


N = 16
SHAPES = [  # name, cin, cout, h, w (source), upsample, residuals
    ('conv1 64->32', 64, 32, 128, 128, 0, 0),
    ('conv2 96->32', 96, 32, 128, 128, 0, 0),
    ('conv3 128->32', 128, 32, 128, 128, 0, 0),
    ('conv4 160->32', 160, 32, 128, 128, 0, 0),
    ('conv5 192->64 +res', 192, 64, 128, 128, 0, 2),
    ('conv_body 64->64 +res', 64, 64, 128, 128, 0, 1),
    ('conv_up1 64->64 x2', 64, 64, 128, 128, 1, 0),
    ('conv_hr 64->64 512', 64, 64, 512, 512, 0, 0),
]


def main():
    lib = _lib.load()
    if not hasattr(lib, 'sr_dev_set_wino_stamps'):
        sys.exit('this library has no stamps: build `make stamp` and select it with SR_HIP_LIB_PATH')
    lib.sr_dev_set_wino_stamps.argtypes = [C.c_void_p]
    lib.sr_dev_set_wino_f32.argtypes = [C.c_int]
    lib.sr_dev_set_wino_f32(3)   # NW = 2 at every size: the grid below is that variant's (4 rows x 64 columns x 32 couts per workgroup)
    lib.sr_dev_conv3x3_wino_f32.argtypes = [C.POINTER(_lib.ConvDesc), C.c_void_p, C.c_void_p]
    lib.sr_dev_conv3x3_wino_pack_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.sr_dev_conv3x3_wino_pack_bytes.argtypes = [C.c_int, C.c_int]
    lib.sr_dev_conv3x3_wino_pack_bytes.restype = C.c_size_t
    dev = torch.device('cuda')
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(7)
    print(f'batch {N}, {cus} CUs, NW = 2 (forced; it is the default variant at these sizes); s_memtime ticks; median over workgroups [min..max]')
    for name, cin, cout, h, w, up, nres in SHAPES:
        H, W = (2 * h, 2 * w) if up else (h, w)
        wt = (torch.rand(cout, cin, 3, 3, generator=g, device=dev) - 0.5).mul_(0.1)
        image = torch.empty(lib.sr_dev_conv3x3_wino_pack_bytes(cout, cin), dtype=torch.uint8, device=dev)
        _lib.check(lib.sr_dev_conv3x3_wino_pack_f32(wt.data_ptr(), cout, cin, cin, 0, image.data_ptr(), st), 'pack')
        bias = torch.zeros(cout, device=dev)
        src = torch.rand(N, cin // 8, h, w, 8, generator=g, device=dev)
        dst = torch.empty(N, cout // 8, H, W, 8, device=dev)
        res = [torch.rand(N, cout // 8, H, W, 8, generator=g, device=dev) for _ in range(nres)]
        d = _lib.ConvDesc()
        d.in_, d.in_img_stride, d.cin_pad, d.cin_real, d.in_h, d.in_w, d.upsample = _ptr(src, 0), _stride(src), cin, cin, h, w, up
        d.wpacked, d.bpacked, d.cout = image.data_ptr(), bias.data_ptr(), cout
        d.out, d.out_img_stride, d.n, d.act_slope, d.alpha = _ptr(dst, 0), _stride(dst), N, 0.2, 1.0
        for k, r in enumerate(res):
            setattr(d, f'res{k + 1}', _ptr(r, 0))
            setattr(d, f'res{k + 1}_img_stride', _stride(r))
            setattr(d, f'beta{k + 1}', 0.2)
        gx, gy = N * ((H + 3) // 4) * ((W + 63) // 64), cout // 32   # the launch's grid: tiles x 32-cout groups
        buf = torch.zeros(gx * gy * 8, dtype=torch.int64, device=dev)
        for rep in range(3):   # the third launch is stamped
            lib.sr_dev_set_wino_stamps(buf.data_ptr() if rep == 2 else None)
            _lib.check(lib.sr_dev_conv3x3_wino_f32(C.byref(d), image.data_ptr(), st), 'wino conv')
        lib.sr_dev_set_wino_stamps(None)
        torch.cuda.synchronize()
        t = buf.cpu().view(gy * gx, 8).double()
        ok = (t[:, 0] > 0) & (t[:, 4] > 0)
        line = f'{name:22s}: {gx * gy:5d} workgroups = {gx * gy / (2 * cus):.0f} rounds, {int((~ok).sum())} without stamps'
        line += '\n    ' + ' | '.join(f'{nm} {float(x.median()):6.0f} [{float(x.min()):5.0f}..{float(x.max()):6.0f}]' for nm, x in zip(
            ('prologue', 'loop', 'exchange', 'epilogue'), [(t[:, k + 1] - t[:, k])[ok] for k in range(4)]))
        if bool((t[:, 5] > 0)[ok].all()):   # stamp 5: head of the last chunk, whose barrier drains the residual pieces
            x = (t[:, 2] - t[:, 5])[ok]
            line += f' | last chunk {float(x.median()):6.0f} [{float(x.min()):5.0f}..{float(x.max()):6.0f}]'
        print(line, flush=True)
    lib.sr_dev_set_wino_f32(1)


if __name__ == '__main__':
    main()
