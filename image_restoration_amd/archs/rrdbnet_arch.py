"""RRDBNet (ESRGAN generator) on the MI355X HIP path.

Same constructor, forward contract and state_dict keys as the reference
``basicsr/archs/rrdbnet_arch.py`` (ResidualDenseBlock :9-39, RRDB :42-63, RRDBNet :66-119),
so ``network_g: {type: RRDBNet, ...}`` option blocks and ESRGAN checkpoints drop in.  The
modules below only hold parameters; ``RRDBNet.forward`` hands the whole network to
``sr_rrdbnet_forward_f32`` (include/sr_hip.h), which runs it as fused MFMA conv launches on
the current HIP stream.
"""
import ctypes as C

import torch
from torch import nn

from .. import _lib
from ..utils.registry import ARCH_REGISTRY
from .arch_util import Conv3x3Params, default_init_weights, make_layer
from .hip_driver import HipDriverNet, symbol


class ResidualDenseBlock(nn.Module):
    """Parameters of one residual dense block: conv1..conv5 with growing input width
    (reference :19-30); RDB convs are initialised kaiming_normal * 0.1, bias 0."""

    def __init__(self, num_feat=64, num_grow_ch=32):
        super().__init__()
        self.conv1 = Conv3x3Params(num_feat, num_grow_ch)
        self.conv2 = Conv3x3Params(num_feat + num_grow_ch, num_grow_ch)
        self.conv3 = Conv3x3Params(num_feat + 2 * num_grow_ch, num_grow_ch)
        self.conv4 = Conv3x3Params(num_feat + 3 * num_grow_ch, num_grow_ch)
        self.conv5 = Conv3x3Params(num_feat + 4 * num_grow_ch, num_feat)
        default_init_weights([self.conv1, self.conv2, self.conv3, self.conv4, self.conv5], 0.1)


class RRDB(nn.Module):
    """Three residual dense blocks (reference :52-56)."""

    def __init__(self, num_feat, num_grow_ch=32):
        super().__init__()
        self.rdb1 = ResidualDenseBlock(num_feat, num_grow_ch)
        self.rdb2 = ResidualDenseBlock(num_feat, num_grow_ch)
        self.rdb3 = ResidualDenseBlock(num_feat, num_grow_ch)


@ARCH_REGISTRY.register()
class RRDBNet(HipDriverNet):
    """RRDBNet(num_in_ch, num_out_ch, scale=4, num_feat=64, num_block=23, num_grow_ch=32[, compute_dtype='fp32']).

    forward(x[N, num_in_ch, H, W] fp32 on a HIP device) -> [N, num_out_ch, 4H/s', 4W/s']
    with s' = 1, 2, 4 for scale 4, 2, 1 (pixel_unshuffle at the input, reference :90-93,106-109).
    """

    _num_params, _params_name = 'sr_rrdbnet_num_params', 'RRDBNet'

    def __init__(self, num_in_ch, num_out_ch, scale=4, num_feat=64, num_block=23, num_grow_ch=32, compute_dtype='fp32'):
        super().__init__()
        self.scale = scale
        self.num_in_ch, self.num_out_ch = num_in_ch, num_out_ch
        self.num_feat, self.num_block, self.num_grow_ch = num_feat, num_block, num_grow_ch
        if scale == 2:
            num_in_ch = num_in_ch * 4
        elif scale == 1:
            num_in_ch = num_in_ch * 16
        self.conv_first = Conv3x3Params(num_in_ch, num_feat)
        self.body = make_layer(RRDB, num_block, num_feat=num_feat, num_grow_ch=num_grow_ch)
        self.conv_body = Conv3x3Params(num_feat, num_feat)
        self.conv_up1 = Conv3x3Params(num_feat, num_feat)
        self.conv_up2 = Conv3x3Params(num_feat, num_feat)
        self.conv_hr = Conv3x3Params(num_feat, num_feat)
        self.conv_last = Conv3x3Params(num_feat, num_out_ch)
        self._workspaces = {}     # the inference forward's workspace: (bf16, n, h, w, device) -> buffer, one entry at a time
        self.compute_dtype = 'fp32'
        self.set_compute_dtype(compute_dtype)  # option key beyond the reference's: 'bf16' = reduced-precision kernels

    # ------------------------------------------------------------------ HIP plumbing (the caches: archs/hip_driver.py)
    def set_compute_dtype(self, dtype):
        """'fp32' (reference numerics, default) or 'bf16' (bf16 activations, activation gradients and weight images on
        v_mfma_f32_32x32x16_bf16; fp32 master weights, accumulation, parameter gradients and optimiser)."""
        if dtype not in ('fp32', 'bf16'):
            raise ValueError(f"compute dtype must be 'fp32' or 'bf16', got {dtype!r}")
        self.compute_dtype = dtype
        return self

    def _cfg(self):
        # scale other than 1/2/4 behaves like 4 in the reference (no unshuffle, :106-111)
        s = self.scale if self.scale in (1, 2) else 4
        return _lib.RRDBNetCfg(self.num_in_ch, self.num_out_ch, s, self.num_feat, self.num_block, self.num_grow_ch)

    def _param_ends(self):
        return self.conv_first.weight, self.conv_last.bias

    def _packed(self, lib, cfg, stream, bf16, dgrad=False):
        """The MFMA-ready weight images of the forward (bf16: rounded from the fp32 master parameters), or ``dgrad``: the
        transposed / flipped images of the data-gradient convs, which hold no bias and are keyed on the weights alone."""
        if dgrad:
            return self._blob(('dgrad', bf16), lib, cfg, stream, 'sr_rrdbnet_packed_dgrad_bytes', 'sr_rrdbnet_pack_dgrad',
                              stride=2, count=False, layout=False, short=True)
        return self._blob(('fwd', bf16), lib, cfg, stream, 'sr_rrdbnet_packed_bytes', 'sr_rrdbnet_pack', count=not bf16)

    def _workspace(self, lib, cfg, n, h, w, dev, bf16):
        """The inference forward's workspace: exactly sized, ONE live shape at a time (any other shape or dtype drops it), which
        keeps HBM use bounded when images of many sizes pass through."""
        query, name = symbol(lib, 'sr_rrdbnet_workspace_bytes', bf16, query=True)
        nbytes = query(C.byref(cfg), n, h, w)
        if nbytes == 0:
            if bf16:
                raise _lib.SrHipError(f'{name} returned 0 for input {h}x{w}')
            u = {4: 1, 2: 2, 1: 4}[cfg.scale]
            # the reference asserts divisibility inside pixel_unshuffle (arch_util.py:197)
            assert h % u == 0 and w % u == 0, f'input {h}x{w} is not divisible by the pixel_unshuffle factor {u}'
            raise _lib.SrHipError(f'{name} returned 0')
        key = (bf16, n, h, w, str(dev))
        ws = self._workspaces.get(key)
        if ws is None or ws.numel() < nbytes:
            self._workspaces.clear()
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self._workspaces[key] = ws
        return ws, nbytes

    def forward(self, x):
        if not x.is_cuda:
            raise _lib.SrHipError('RRDBNet.forward runs only on a HIP device (no CPU fallback): move the module '
                                  'and input with .to("cuda")')
        if x.dim() != 4 or x.size(1) != self.num_in_ch:
            raise ValueError(f'expected [N, {self.num_in_ch}, H, W], got {tuple(x.shape)}')
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self._param_list())):
            from .rrdbnet_autograd import rrdbnet_apply
            return rrdbnet_apply(self, x)
        return self._forward_inference(x)

    def _forward_inference(self, x):
        lib = _lib.load()
        x = x.contiguous().float()
        n, _, h, w = x.shape
        cfg = self._cfg()
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream().cuda_stream
            return self._launch(lib, cfg, x, n, h, w, stream)

    def _launch(self, lib, cfg, x, n, h, w, stream):
        bf16 = self.compute_dtype == 'bf16'
        packed = self._packed(lib, cfg, stream, bf16)
        ws, nbytes = self._workspace(lib, cfg, n, h, w, x.device, bf16)
        up = {4: 4, 2: 2, 1: 1}[cfg.scale]
        y = torch.empty((n, self.num_out_ch, h * up, w * up), dtype=torch.float32, device=x.device)
        fwd, name = symbol(lib, 'sr_rrdbnet_forward', bf16)
        _lib.check(fwd(C.byref(cfg), packed.data_ptr(), x.data_ptr(), y.data_ptr(), n, h, w, ws.data_ptr(), nbytes, stream), name)
        return y
