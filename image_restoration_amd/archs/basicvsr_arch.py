"""BasicVSR, the recurrent video super-resolution network of the reference (``basicsr/archs/basicvsr_arch.py``), on libsr_hip.so.

Same constructor, state_dict keys, order and shapes (``spynet.*``, ``backward_trunk.main.0.weight``,
``backward_trunk.main.2.{i}.conv1.weight``, ``fusion.weight`` ...) and the same initialisation draws in the same order as the
reference, so a checkpoint loads key for key and a seeded fresh network has the reference's parameters.  The modules only hold
parameters; ``forward`` is a composition of launches:

    flows               one batched SpyNet call for both directions (SpyNet is batch-independent bit for bit), chunked over pairs
    per step of a branch    sr_vsr_prop_input_f32: the frame block and flow_warp(previous feature, flow) written where the trunk's
                            first conv reads them; sr_vsr_trunk_f32: the 1 + 2 * num_block convs of ConvResidualBlocks in one C call,
                            the last one writing into the step's window of the per-clip feature tensor
    reconstruction      once, batched over frames: fusion 1x1, upconv1 / upconv2 + pixel shuffle (the LeakyReLU after a shuffle
                        commutes with it and runs in the conv's epilogue), conv_hr, conv_last to NCHW, the x4 bilinear base added
                        in place; chunked over frames by a byte budget

The per-clip feature tensor is [n * b, 2 * num_feat / 8, h, w, 8], frame-major: blocks [0, fb) of image (i, batch) hold the
backward branch's feature of frame i, blocks [fb, 2 fb) the forward branch's, so ``cat([out_l[i], feat_prop])`` is the image itself
and is never copied.  The backward branch runs first, then the forward branch.

``set_compute_dtype('bf16')`` (or ``network_g.compute_dtype: bf16`` in an option file) runs propagation and reconstruction on
CB16 bf16 activations: the clip tensor is [n * b, 2 * num_feat / 16, h, w, 16], a step is one
sr_rvsr_prop_input_bf16 and one sr_rvsr_trunk_bf16, the head runs on the bf16 convs and ``conv_last`` stores fp32 NCHW.  The input
clip, SpyNet and the flows stay fp32, so ``get_flow`` is the same bits in both modes; ``num_feat % 16 == 0`` is required.

x4 only.  By default the networks run inference: outputs carry no grad_fn, and a forward that would need a graph (train mode, grad
enabled, something requiring grad) raises NotImplementedError.  ``BasicVSR.set_autograd(True)`` enables fp32 training, as
``SpyNet.set_autograd`` does for the flow estimator (and it switches ``self.spynet`` too): ``get_flow`` then goes through
SpyNet's Function when a ``spynet.*`` parameter requires grad, and ``propagate`` is ONE autograd Function over (x, the two flow
tensors, the parameters) whose backward is archs/basicvsr_autograd.py — the head batched over the frames, then the two branches
walked against their direction, per step one sr_vsr_trunk_bwd_f32 and one sr_vsr_prop_input_bwd_f32 (with
``set_autograd(True, deterministic=True)``: sr_vsr_prop_input_bwd_det_f32, which makes the backward bit-reproducible).  Autograd
itself joins the two Functions.  The training forward issues the inference forward's launches (sr_vsr_trunk_keep_f32 is the same
driver) and its output is the inference output bit for bit.  The frames are data: a clip that requires grad is refused.  bf16
and IconVSR stay forward only (IconVSR's keyframe branch and fusion convs are the follow-up).  Training from an option file is
models/video_recurrent_model.py.  What a training forward keeps, and the one step of the default backward that is not
bit-reproducible, are stated in archs/basicvsr_autograd.py.
ValueError, before anything is launched, for: fewer than two frames (the reference's ``get_flow`` cannot reshape an empty batch),
channels other than 3, a dtype other than fp32, a side of 32 pixels or fewer (SpyNet's rule), ``num_feat % 8 != 0``.
"""
import torch
from torch import nn
from torch.nn import functional as F

from .. import _lib, hip_ops
from ..utils.registry import ARCH_REGISTRY
from .arch_util import Conv3x3Params, ResidualBlockNoBN, make_layer
from .edvr_arch import _BF16, _FP32, PCDAlignment, TSAFusion
from .hip_driver import HipDriverNet
from .hip_generator import HipGenerator
from .spynet_arch import SpyNet

_FLOW_BUDGET = 1 << 30      # bytes of SpyNet activations alive at once
_RECON_BUDGET = 2 << 30     # bytes of high-resolution activations alive at once


class _Layout:
    """What the compute dtype decides, in one record: whether it is bf16, the window class, its channels per block and element
    type, the step-input launch, the trunk call and the stem of its pack symbols, the convs and the pixel shuffle of the head, and
    ``packed(net, conv)``, the weight image of a head or fusion conv."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


_LAYOUTS = {
    'fp32': _Layout(bf16=False, CB=hip_ops.CB8, lanes=8, dtype=torch.float32, prop_input=hip_ops.vsr_prop_input, trunk=hip_ops.vsr_trunk,
                    trunk_stem='sr_vsr_trunk', conv3x3=hip_ops.conv3x3, conv1x1=hip_ops.convd, pixel_shuffle=hip_ops.pixel_shuffle,
                    packed=lambda net, conv: net.packed(conv)),
    # bf16 images: 3x3 from the network's cache, the 1x1 fusion from hip_ops' (both keyed on the parameter's version, so an in-place
    # update is seen)
    'bf16': _Layout(bf16=True, CB=hip_ops.CB16, lanes=16, dtype=torch.bfloat16, prop_input=hip_ops.vsr_prop_input_bf16,
                    trunk=hip_ops.vsr_trunk_bf16, trunk_stem='sr_rvsr_trunk', conv3x3=hip_ops.conv3x3_bf16,
                    conv1x1=hip_ops.conv1x1_bf16, pixel_shuffle=hip_ops.pixel_shuffle_bf16,
                    packed=lambda net, conv: net.packed(conv, 0, True) if conv.weight.shape[2] == 3 else hip_ops.packed_conv_bf16(conv)),
}


class ConvResidualBlocks(HipDriverNet):
    """Parameters of the reference's ConvResidualBlocks: ``main`` = conv 3x3 (num_in_ch -> num_out_ch), LeakyReLU(0.1),
    ``num_block`` ResidualBlockNoBN.  ``num_in_ch`` is 3 + k * num_out_ch (k = 1, 2): the frame, then k feature maps.  No forward:
    ``run`` is one sr_vsr_trunk_f32 call on a prepared CB8 window."""

    _num_params, _params_name = 'sr_vsr_trunk_num_params', 'ConvResidualBlocks'

    def __init__(self, num_in_ch=3, num_out_ch=64, num_block=15):
        super().__init__()
        self.num_in_ch, self.num_out_ch, self.num_block = num_in_ch, num_out_ch, num_block
        self.main = nn.Sequential(Conv3x3Params(num_in_ch, num_out_ch), nn.LeakyReLU(negative_slope=0.1, inplace=True),
                                  make_layer(ResidualBlockNoBN, num_block, num_feat=num_out_ch))

    def _param_ends(self):
        last = self.main[2][-1].conv2.bias if self.num_block > 0 else self.main[0].bias
        return self.main[0].weight, last

    def cfg(self):
        segs, rest = divmod(self.num_in_ch - 3, self.num_out_ch)
        if rest or segs not in (1, 2) or self.num_out_ch % 8:
            raise ValueError(f'ConvResidualBlocks: the HIP trunk needs num_in_ch = 3 + k * num_out_ch (k = 1, 2) and num_out_ch % 8 == 0, '
                             f'got {self.num_in_ch} -> {self.num_out_ch}')
        return _lib.VsrTrunkCfg(self.num_out_ch, self.num_block, segs)

    def packed(self, dev, bf16=False):
        """(config, blob of weight images) for the current parameters: looked up once per branch, not per step — the weights key
        walks every parameter of the trunk.  ``bf16``: the blob of bf16 images and fp32 biases, kept as a second kind beside the
        fp32 one under the same weights key."""
        lib, cfg = _lib.load(), self.cfg()
        if bf16 and self.num_out_ch % 16:
            raise ValueError(f'ConvResidualBlocks: the bf16 trunk needs num_out_ch % 16 == 0 (CB16), got {self.num_out_ch}')
        stem = _LAYOUTS['bf16' if bf16 else 'fp32'].trunk_stem
        with torch.cuda.device(dev):
            blob = self._blob(('fwd', bool(bf16)), lib, cfg, torch.cuda.current_stream(dev).cuda_stream, stem + '_packed_bytes',
                              stem + '_pack')
        return cfg, blob

    def packed_dgrad(self, dev):
        """The blob of fp32 data-gradient images (sr_vsr_trunk_pack_dgrad_f32) for the current parameters: a second kind beside
        the forward blob, under the same weights key."""
        lib, cfg = _lib.load(), self.cfg()
        with torch.cuda.device(dev):
            return self._blob(('dgrad', False), lib, cfg, torch.cuda.current_stream(dev).cuda_stream, 'sr_vsr_trunk_packed_dgrad_bytes',
                              'sr_vsr_trunk_pack_dgrad')

    def run_keep(self, src, out, packed=None):
        """``run`` on fp32 windows with every activation the backward reads kept: (out, the activation stack) — one
        sr_vsr_trunk_keep_f32 call, the launches of ``run``."""
        cfg, blob = packed or self.packed(src.device)
        return hip_ops.vsr_trunk_keep(cfg, blob, src, out)

    def run(self, src, out, packed=None):
        """``src``: CB8 (fp32) or CB16 (bf16) window [frame block, feature windows]; ``out``: window of num_out_ch channels of the
        same kind; ``packed``: what ``packed(device, bf16)`` returned for the current parameters (looked up here when None)."""
        bf16 = isinstance(src, hip_ops.CB16)
        cfg, blob = packed or self.packed(src.device, bf16)
        return _LAYOUTS['bf16' if bf16 else 'fp32'].trunk(cfg, blob, src, out)

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('ConvResidualBlocks is a parameter container; the video network launches the HIP kernels')


@ARCH_REGISTRY.register()
class BasicVSR(HipGenerator):
    """A recurrent network for video SR, x4 only.

    Args:
        num_feat (int): Number of channels (a multiple of 8). Default: 64.
        num_block (int): Number of residual blocks for each branch. Default: 15.
        spynet_path (str): Path to the pretrained weights of SpyNet. Default: None.
    """

    _fuses = True
    _autograd = False
    _deterministic = False

    def __init__(self, num_feat=64, num_block=15, spynet_path=None):
        super().__init__()
        if num_feat <= 0 or num_feat % 8 != 0:
            raise ValueError(f'BasicVSR: num_feat={num_feat} is not supported; supported: positive multiples of 8 (CB8 activations)')
        self.num_feat = num_feat
        # alignment
        self.spynet = SpyNet(spynet_path)
        # propagation
        self.backward_trunk = ConvResidualBlocks(num_feat + 3, num_feat, num_block)
        self.forward_trunk = ConvResidualBlocks(num_feat + 3, num_feat, num_block)
        # reconstruction
        self.fusion = Conv3x3Params(num_feat * 2, num_feat, ksize=1)
        self.upconv1 = Conv3x3Params(num_feat, num_feat * 4)
        self.upconv2 = Conv3x3Params(num_feat, 64 * 4)
        self.conv_hr = Conv3x3Params(64, 64)
        self.conv_last = Conv3x3Params(64, 3)

    # ------------------------------------------------------------------------------------------------- compute dtype
    def set_compute_dtype(self, compute_dtype):
        """'fp32' or 'bf16' for propagation and reconstruction (SpyNet and the flows stay fp32); returns ``self``.  Set after
        construction: the constructor keeps the reference's signature."""
        if compute_dtype not in ('fp32', 'bf16'):
            raise ValueError(f"{type(self).__name__}: compute_dtype={compute_dtype!r} is not supported; supported: 'fp32', 'bf16'")
        if compute_dtype == 'bf16' and self.num_feat % 16 != 0:
            raise ValueError(f"{type(self).__name__}: compute_dtype='bf16' needs num_feat % 16 == 0 (CB16 activations), got "
                             f'num_feat={self.num_feat}')
        self.compute_dtype = compute_dtype
        return self

    def _layout(self):
        """The _Layout record of the compute dtype."""
        return _LAYOUTS[self.compute_dtype]

    # ------------------------------------------------------------------------------------------------------ training
    def set_autograd(self, enabled=True, deterministic=False):
        """Whether an fp32 forward that needs a graph (train mode, grad enabled, a parameter or a flow requiring grad) builds one
        (archs/basicvsr_autograd.py) instead of being refused; also switches ``self.spynet``.  Off by default; set after
        construction, like set_compute_dtype.  ``deterministic``: the step-input adjoint of the backward sums in 64-bit integers
        (sr_vsr_prop_input_bwd_det_f32) instead of with float atomics, which makes the whole backward bit-reproducible; off by
        default, so a caller that does not ask keeps the atomic scatter and its bits.  Returns self."""
        self._autograd = bool(enabled)
        self._deterministic = bool(enabled) and bool(deterministic)
        self.spynet.set_autograd(enabled)
        return self

    # ------------------------------------------------------------------------------------------------------ refusals
    def _check(self, x, flows=()):
        if x.dim() != 5 or x.size(2) != 3:
            raise ValueError(f'{type(self).__name__}: expected a [b, n, 3, h, w] clip, got {tuple(x.shape)}')
        if x.dtype != torch.float32 or any(f.dtype != torch.float32 for f in flows):
            raise ValueError(f'{type(self).__name__}: {x.dtype} input is not supported; supported: fp32')
        b, n, _, h, w = x.shape
        if n < 2:
            raise ValueError(f'{type(self).__name__}: a clip of {n} frame(s) is not supported; at least 2 are needed (the reference fails '
                             'there too: its get_flow cannot reshape an empty batch)')
        self._check_frames(n)
        if b < 1 or min(h, w) <= 32:
            raise ValueError(f'{type(self).__name__}: a {h}x{w} frame is too small; both sides must exceed 32 pixels (SpyNet)')
        for f in flows:
            if tuple(f.shape) != (b, n - 1, 2, h, w):
                raise ValueError(f'{type(self).__name__}: flows must be [{b}, {n - 1}, 2, {h}, {w}], got {tuple(f.shape)}')
        needs_graph = self.training and torch.is_grad_enabled() and (x.requires_grad or any(f.requires_grad for f in flows)
                                                                     or any(p.requires_grad for p in self.parameters()))
        if needs_graph and self.compute_dtype == 'bf16':
            raise NotImplementedError(f"{type(self).__name__} with compute_dtype='bf16' is forward only (eval mode or "
                                      "torch.no_grad()); train with compute_dtype='fp32'")
        if not (x.is_cuda and all(f.is_cuda for f in flows)):
            raise _lib.SrHipError(f'{type(self).__name__}.forward runs only on a HIP device (no CPU fallback): move the module and '
                                  'inputs with .to("cuda")')
        if needs_graph and not self._autograd:
            raise NotImplementedError(self._refusal())
        if needs_graph and x.requires_grad:
            raise NotImplementedError(f'{type(self).__name__} computes no gradient of the input clip: x must not require grad (the '
                                      'frames are data; the parameters and flows passed to propagate are differentiated)')
        return needs_graph

    def _refusal(self):
        """What a forward that needs a graph is told while set_autograd is off."""
        return (f'{type(self).__name__} runs inference only by default: call .eval() (or run under torch.no_grad()), or enable the '
                'recurrent backward (on top of SpyNet\'s) with set_autograd(True), as VideoRecurrentModel does when it trains '
                'from an option file; IconVSR and bf16 training are the follow-up')

    def _check_frames(self, n):
        """A subclass's own rule on the number of frames."""

    # --------------------------------------------------------------------------------------------------------- flows
    def get_flow(self, x):
        """(flows_forward, flows_backward), each [b, n - 1, 2, h, w]: flows_backward[:, i] is SpyNet(x_i, x_{i+1}),
        flows_forward[:, i] is SpyNet(x_{i+1}, x_i)."""
        needs_graph = self._check(x)
        # a graph through SpyNet only when one of its parameters wants a gradient: the flows then carry a grad_fn (spynet_apply,
        # per chunk) that autograd joins to propagate's; otherwise as in inference
        flow_graph = bool(needs_graph) and any(p.requires_grad for p in self.spynet.parameters())
        with torch.set_grad_enabled(flow_graph):
            x = x.contiguous()
            b, n, c, h, w = x.shape
            x_1 = x[:, :-1].reshape(-1, c, h, w)
            x_2 = x[:, 1:].reshape(-1, c, h, w)
            ref, supp = torch.cat([x_1, x_2]), torch.cat([x_2, x_1])
            # per pair: the six levels' inputs and the widest activations of a level at 32-aligned size, about 1 KiB per pixel
            hp, wp = -(-h // 32) * 32, -(-w // 32) * 32
            chunk = max(1, _FLOW_BUDGET // (1024 * hp * wp))
            flows = torch.cat([self.spynet(ref[s:s + chunk], supp[s:s + chunk]) for s in range(0, ref.size(0), chunk)])
            pairs = b * (n - 1)
            return flows[pairs:].view(b, n - 1, 2, h, w), flows[:pairs].view(b, n - 1, 2, h, w)

    # --------------------------------------------------------------------------------------------------- propagation
    def _branch(self, trunk, x, flows, feats, cb0, order, tin, keep=None):
        """One propagation branch over the frames in ``order``: per step one step-input launch (sr_vsr_prop_input_f32 /
        sr_rvsr_prop_input_bf16) and one trunk call (sr_vsr_trunk_f32 / sr_rvsr_trunk_bf16).  ``flows[:, j]`` warps the feature of
        the previous step onto frame ``order[k]``: j = i for the backward branch, i - 1 for the forward branch.  ``keep`` (a
        dict, fp32): the trunk call is sr_vsr_trunk_keep_f32, every step gets a trunk input of its own and ``keep[i]`` =
        (that input, the activation stack) of frame i."""
        L = self._layout()
        CB, b, fb = L.CB, x.size(0), self.num_feat // L.lanes
        prev, packed = None, trunk.packed(x.device, L.bf16)
        for k, i in enumerate(order):
            if keep is not None and k > 0:
                tin = torch.empty_like(tin)
            flow = None if prev is None else flows[:, min(i, order[k - 1])]
            L.prop_input(x[:, i], prev, flow, CB(tin, 1, fb), CB(tin, 0, 1))
            out = CB(feats[i * b:(i + 1) * b], cb0, fb)
            if keep is None:
                prev = trunk.run(CB(tin), out, packed)
            else:
                prev, stack = trunk.run_keep(CB(tin), out, packed)
                keep[i] = (tin, stack)

    def _reconstruct(self, feats, frames, y, keep=None):
        """The upsampling head on images [s, e) of the frame-major clip tensors, into y[s:e].  In bf16 every activation is stored
        as bf16 once, after its epilogue; conv_last writes fp32 NCHW and the x4 bilinear base of the fp32 frames is added in fp32
        in both modes.  ``keep`` (a list): receives the four activations the head's backward reads — the fused feature, the two
        shuffled maps and conv_hr's output, each after its LeakyReLU."""
        L = self._layout()
        out = L.CB(feats)
        if self._fuses:     # BasicVSR: fusion 1x1 of [backward, forward]; IconVSR reconstructs from the forward feature alone
            out = L.conv1x1(out, L.packed(self, self.fusion), act_slope=0.1)
        up1 = L.pixel_shuffle(L.conv3x3(out, L.packed(self, self.upconv1), act_slope=0.1), self.num_feat, 2)
        up2 = L.pixel_shuffle(L.conv3x3(up1, L.packed(self, self.upconv2), act_slope=0.1), 64, 2)
        hr = L.conv3x3(up2, L.packed(self, self.conv_hr), act_slope=0.1)
        L.conv3x3(hr, L.packed(self, self.conv_last), out_nchw=y)
        hip_ops.bilinear_up(frames, 4, out=y)
        if keep is not None:
            keep.extend((out, up1, up2, hr))

    def run_forward(self, x, flows_forward, flows_backward, keep=None):
        """The launches of ``propagate`` on contiguous device tensors, under no_grad.  ``keep`` (a dict, fp32 only) makes it the
        training forward — the same launches, with sr_vsr_trunk_keep_f32 as the trunk call — and receives what the backward
        reads (archs/basicvsr_autograd.py):
            x, flows_forward, flows_backward    the inputs
            feats                               the per-clip feature tensor
            backward, forward                   per branch {frame i: (the trunk input of the step, its activation stack)}
            head                                [(s, e, [fused, up1, up2, hr])] per chunk of frames [s, e)"""
        with torch.no_grad():
            b, n, _, h, w = x.shape
            L = self._layout()
            blk, dtype, fb, dev = L.lanes, L.dtype, self.num_feat // L.lanes, x.device
            feats = torch.empty((n * b, 2 * fb, h, w, blk), dtype=dtype, device=dev)
            tin = torch.empty((b, 1 + fb, h, w, blk), dtype=dtype, device=dev)
            steps = (None, None) if keep is None else ({}, {})
            self._branch(self.backward_trunk, x, flows_backward, feats, 0, list(range(n - 1, -1, -1)), tin, steps[0])
            self._branch(self.forward_trunk, x, flows_forward, feats, fb, list(range(n)), torch.empty_like(tin) if keep is not None else tin,
                         steps[1])
            # reconstruction, frame-major: image i * b + k is frame i of clip k
            frames = x.transpose(0, 1).reshape(n * b, 3, h, w)
            y = torch.empty((n * b, 3, 4 * h, 4 * w), dtype=torch.float32, device=dev)
            # per image: the 4 * num_feat / 256 / 64-channel maps at 2x / 4x size alive around a conv, about 4 maps of 64 x 16 h w floats
            chunk = max(1, _RECON_BUDGET // (4 * 4 * 64 * 16 * h * w))
            head = []
            for s in range(0, n * b, chunk):
                acts = None if keep is None else []
                self._reconstruct(feats[s:s + chunk], frames[s:s + chunk], y[s:s + chunk], acts)
                head.append((s, min(s + chunk, n * b), acts))
            if keep is not None:
                keep.update(x=x, flows_forward=flows_forward, flows_backward=flows_backward, feats=feats, backward=steps[0],
                            forward=steps[1], head=head)
            return y.view(n, b, 3, 4 * h, 4 * w).transpose(0, 1).contiguous()

    def propagate(self, x, flows_forward, flows_backward):
        """The network after ``get_flow``: x [b, n, 3, h, w], flows [b, n - 1, 2, h, w] -> [b, n, 3, 4h, 4w].  With
        ``set_autograd(True)``, in train mode with something requiring grad, the result carries a grad_fn whose backward fills the
        gradients of the parameters and of the two flow tensors (archs/basicvsr_autograd.py)."""
        if self._check(x, (flows_forward, flows_backward)):
            from .basicvsr_autograd import basicvsr_apply
            return basicvsr_apply(self, x.contiguous(), flows_forward, flows_backward)
        return self.run_forward(x.contiguous(), flows_forward.contiguous(), flows_backward.contiguous())

    def forward(self, x):
        return self.propagate(x, *self.get_flow(x))


class EDVRFeatureExtractor(nn.Module):
    """The keyframe branch of IconVSR (the reference's EDVRFeatureExtractor, basicvsr_arch.py:251-309): EDVR up to and including
    the TSA fusion, on EDVR's fp32 ops table and modules (edvr_arch.py).  ``run(x)`` takes [b, t, 3, h, w] (h, w multiples of 4)
    and returns the fused features as a raw CB8 tensor [b, num_feat / 8, h, w, 8]; on the bf16 table (``ops=_BF16``) as a CB16
    window.  The reference hard-codes 64 channels in its residual blocks, so ``num_feat`` is 64."""

    def __init__(self, num_input_frame, num_feat, load_path):
        super().__init__()
        self.center_frame_idx = num_input_frame // 2
        self.conv_first = Conv3x3Params(3, num_feat)
        self.feature_extraction = make_layer(ResidualBlockNoBN, 5, num_feat=64)
        self.conv_l2_1 = Conv3x3Params(num_feat, num_feat)
        self.conv_l2_2 = Conv3x3Params(num_feat, num_feat)
        self.conv_l3_1 = Conv3x3Params(num_feat, num_feat)
        self.conv_l3_2 = Conv3x3Params(num_feat, num_feat)
        self.pcd_align = PCDAlignment(num_feat=num_feat, deformable_groups=8)
        self.fusion = TSAFusion(num_feat=num_feat, num_frame=num_input_frame, center_frame_idx=self.center_frame_idx)
        if load_path:
            self.load_state_dict(torch.load(load_path, map_location='cpu')['params'])

    def run(self, x, ops=_FP32):
        b, t, c, h, w = x.shape
        feat_l1 = ops.conv(self.conv_first, ops.enter(x.reshape(b * t, c, h, w)))
        for blk in self.feature_extraction:
            feat_l1 = ops.resblock(blk, feat_l1)
        feat_l2 = ops.conv(self.conv_l2_2, ops.conv_s2(self.conv_l2_1, feat_l1))
        feat_l3 = ops.conv(self.conv_l3_2, ops.conv_s2(self.conv_l3_1, feat_l2))
        feat_l = [feat_l1, feat_l2, feat_l3]
        ref_l = [ops.center_over_t(f, b, t, self.center_frame_idx) for f in feat_l]
        return self.fusion._layers(ops, self.pcd_align._layers(ops, feat_l, ref_l), b, t)

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('EDVRFeatureExtractor is run by IconVSR (run(x) on device clips)')


@ARCH_REGISTRY.register()
class IconVSR(BasicVSR):
    """IconVSR (basicvsr_arch.py:108-248): BasicVSR's propagation with keyframe features from an EDVR extractor fused into both
    branches at the frames ``range(0, n, keyframe_stride)`` plus the last one, and a forward trunk that also reads the backward
    branch's feature.  Same constructor, state_dict keys and initialisation order as the reference.

    The per-clip tensor is [n * b, 1 + 2 fb, h, w, 8], frame-major: block 0 the frame, blocks [1, 1 + fb) the backward branch's
    feature, blocks [1 + fb, 1 + 2 fb) the forward branch's propagated (warped, at keyframes fused) feature — the image IS
    ``cat([x_i, out_l[i], feat_prop])``, the 136-channel input of the forward trunk.  At a keyframe the step-input launch writes
    the warped feature in front of the keyframe feature in that keyframe's own two-window buffer, which the fusion conv reads
    whole.  The input is reflect-padded to multiples of 4 and the output cropped, as the reference.

    ValueError: ``temporal_padding`` not in (2, 3), ``num_feat != 64`` (the reference hard-codes 64 in its extractor), fewer than
    2 * temporal_padding + 1 frames, and BasicVSR's refusals."""

    _fuses = False

    def set_autograd(self, enabled=True, deterministic=False):
        if enabled:
            raise NotImplementedError('IconVSR.set_autograd(True): IconVSR runs inference only; its training (the backward of the EDVR '
                                      'keyframe branch and of the fusion convs, on top of BasicVSR\'s recurrent backward) is the '
                                      'follow-up')
        return super().set_autograd(False)

    def _refusal(self):
        return ('IconVSR runs inference only: call .eval() (or run under torch.no_grad()); training (the backward of its keyframe '
                'branch and fusion convs, on top of BasicVSR\'s recurrent backward) is the follow-up')

    def __init__(self, num_feat=64, num_block=15, keyframe_stride=5, temporal_padding=2, spynet_path=None, edvr_path=None):
        HipGenerator.__init__(self)
        if temporal_padding not in (2, 3):
            raise ValueError(f'IconVSR: temporal_padding={temporal_padding} is not supported; supported: 2, 3 (the reference builds its '
                             'mirrored clip for these two only)')
        if num_feat != 64:
            raise ValueError(f'IconVSR: num_feat={num_feat} is not supported; supported: 64 (the reference hard-codes 64 channels in '
                             'its EDVR feature extractor)')
        if keyframe_stride < 1:
            raise ValueError(f'IconVSR: keyframe_stride={keyframe_stride} must be at least 1')
        self.num_feat, self.temporal_padding, self.keyframe_stride = num_feat, temporal_padding, keyframe_stride
        self.edvr = EDVRFeatureExtractor(temporal_padding * 2 + 1, num_feat, edvr_path)
        self.spynet = SpyNet(spynet_path)
        self.backward_fusion = Conv3x3Params(2 * num_feat, num_feat)
        self.backward_trunk = ConvResidualBlocks(num_feat + 3, num_feat, num_block)
        self.forward_fusion = Conv3x3Params(2 * num_feat, num_feat)
        self.forward_trunk = ConvResidualBlocks(2 * num_feat + 3, num_feat, num_block)
        self.upconv1 = Conv3x3Params(num_feat, num_feat * 4)
        self.upconv2 = Conv3x3Params(num_feat, 64 * 4)
        self.conv_hr = Conv3x3Params(64, 64)
        self.conv_last = Conv3x3Params(64, 3)

    def _check_frames(self, n):
        need = 2 * self.temporal_padding + 1
        if n < need:
            raise ValueError(f'IconVSR: a clip of {n} frames is not supported; temporal_padding={self.temporal_padding} needs at '
                             f'least {need} (the reference fails there too: its mirrored clip indexes frame {need - 1})')

    def pad_spatial(self, x):
        """Reflect padding at the bottom and the right to multiples of 4 (PCD alignment needs them)."""
        b, n, c, h, w = x.shape
        pad_h, pad_w = (4 - h % 4) % 4, (4 - w % 4) % 4
        if not (pad_h or pad_w):
            return x
        return F.pad(x.reshape(-1, c, h, w), [0, pad_w, 0, pad_h], mode='reflect').view(b, n, c, h + pad_h, w + pad_w)

    def keyframes(self, n):
        idx = list(range(0, n, self.keyframe_stride))
        if idx[-1] != n - 1:
            idx.append(n - 1)
        return idx

    def get_keyframe_feature(self, x, keyframe_idx):
        """{i: fused EDVR features of the window around keyframe i} on the (padded) clip x, each a raw CB8 tensor
        [b, fb, h, w, 8] (bf16: a raw CB16 tensor [b, fb, h, w, 16] from EDVR's bf16 ops table); the windows come from the
        reference's mirrored clip."""
        self._check(x)
        with torch.no_grad():
            tp = self.temporal_padding
            lead, tail = ([4, 3], [-4, -5]) if tp == 2 else ([6, 5, 4], [-5, -6, -7])
            xm = torch.cat([x[:, lead], x, x[:, tail]], dim=1)
            ops = _BF16 if self.compute_dtype == 'bf16' else _FP32
            return {i: ops.raw(self.edvr.run(xm[:, i:i + 2 * tp + 1].contiguous(), ops)) for i in keyframe_idx}

    def propagate(self, x, flows_forward, flows_backward, feats_keyframe=None, crop=None):
        """The network after ``get_flow`` and ``get_keyframe_feature`` on a clip whose sides are multiples of 4; ``crop`` = (h, w)
        of the unpadded input."""
        if x.dim() == 5 and (x.size(3) % 4 or x.size(4) % 4):
            raise ValueError(f'IconVSR.propagate: the sides must be multiples of 4 (pad_spatial), got {x.size(3)}x{x.size(4)}')
        self._check(x, (flows_forward, flows_backward))
        b, n, _, h, w = x.shape
        with torch.no_grad():
            x, flows_forward, flows_backward = x.contiguous(), flows_forward.contiguous(), flows_backward.contiguous()
            keys = self.keyframes(n)
            if feats_keyframe is None:
                feats_keyframe = self.get_keyframe_feature(x, keys)
            L = self._layout()
            CB, blk, dtype, bf16 = L.CB, L.lanes, L.dtype, L.bf16
            fb, dev = self.num_feat // blk, x.device
            clip = torch.empty((n * b, 1 + 2 * fb, h, w, blk), dtype=dtype, device=dev)
            fwd = torch.empty((n * b, fb, h, w, blk), dtype=dtype, device=dev)
            tin = torch.empty((b, 1 + fb, h, w, blk), dtype=dtype, device=dev)
            pair = {}
            for i in keys:      # [warped feature | keyframe feature]: what a fusion conv reads
                pair[i] = torch.empty((b, 2 * fb, h, w, blk), dtype=dtype, device=dev)
                pair[i][:, fb:].copy_(feats_keyframe[i])

            def step(i, prev, flow, fusion, warp_out, frame_out):
                if i in pair:
                    L.prop_input(x[:, i], prev, flow, CB(pair[i], 0, fb), frame_out)
                    L.conv3x3(CB(pair[i]), L.packed(self, fusion), warp_out)
                else:
                    L.prop_input(x[:, i], prev, flow, warp_out, frame_out)

            prev, packed = None, self.backward_trunk.packed(dev, bf16)
            for i in range(n - 1, -1, -1):
                step(i, prev, None if prev is None else flows_backward[:, i], self.backward_fusion, CB(tin, 1, fb), CB(tin, 0, 1))
                prev = self.backward_trunk.run(CB(tin), CB(clip[i * b:(i + 1) * b], 1, fb), packed)
            prev, packed = None, self.forward_trunk.packed(dev, bf16)
            for i in range(n):
                img = clip[i * b:(i + 1) * b]
                step(i, prev, None if prev is None else flows_forward[:, i - 1], self.forward_fusion, CB(img, 1 + fb, fb), CB(img, 0, 1))
                prev = self.forward_trunk.run(CB(img), CB(fwd[i * b:(i + 1) * b]), packed)
            frames = x.transpose(0, 1).reshape(n * b, 3, h, w)
            y = torch.empty((n * b, 3, 4 * h, 4 * w), dtype=torch.float32, device=dev)
            chunk = max(1, _RECON_BUDGET // (4 * 4 * 64 * 16 * h * w))
            for s in range(0, n * b, chunk):
                self._reconstruct(fwd[s:s + chunk], frames[s:s + chunk], y[s:s + chunk])
            y = y.view(n, b, 3, 4 * h, 4 * w).transpose(0, 1)
            if crop is not None:
                y = y[..., :4 * crop[0], :4 * crop[1]]
            return y.contiguous()

    def forward(self, x):
        self._check(x)
        h_in, w_in = x.shape[3:]
        with torch.no_grad():
            xp = self.pad_spatial(x.contiguous())
        return self.propagate(xp, *self.get_flow(xp), crop=(h_in, w_in))
