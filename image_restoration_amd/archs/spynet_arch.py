"""SpyNet, the optical-flow estimator of the reference's video family (``basicsr/archs/spynet_arch.py``), on libsr_hip.so.

Same constructor, state_dict keys, order and shapes (62 entries: the ``mean`` and ``std`` buffers, then
``basic_module.{0..5}.basic_module.{0,2,4,6,8}.{weight,bias}``, 1,440,300 parameters), PyTorch's default initialisation and the
``{'params': ...}`` checkpoint of ``load_path`` as the reference.  The modules only hold parameters; ``forward(ref, supp)`` takes N
frame pairs at once and is a composition of launches (include/sr_hip_flow.h, include/sr_hip_degrade.h):

    resize to multiples of 32        sr_resize_bilinear_f32 (half-pixel centres = align_corners=False); skipped when nothing changes
    (x - mean) / std                 sr_spynet_preprocess_f32 — after the resize, as the reference
    five 2x2 average pools           sr_avgpool2x2_f32, ref and supp of a level in one launch
    per level                        sr_spynet_level_input_f32: [ref, warp(supp, up), up] as one CB8 block, and up
                                     five sr_conv7x7_f32 (8 -> 32 -> 64 -> 32 -> 16 -> 2), ReLU in the epilogue of the first four,
                                     the level's ``+ up`` as res1 of the fifth
    flow back to (h, w)              sr_cb8_to_nchw_f32, sr_resize_bilinear_f32, sr_channel_affine_f32 (w / w_floor, h / h_floor)

The coarsest level's incoming flow is zero by construction, and the reference's replicate pad (spynet_arch.py:67-70) only ever
pads that zero flow (every finer level is exactly twice the size of the one before): level 0 is ``up = 0``, ``warp = supp``, and
there is no pad kernel.

Inference is the default: outputs carry no grad_fn, and a forward that would need a graph (train mode, grad enabled, a parameter
requiring grad) raises NotImplementedError naming ``set_autograd(True)``.  After ``net.set_autograd(True)`` such a forward goes
through ``archs/spynet_autograd.py`` and returns a flow with a grad_fn: the backward walks the levels from fine to coarse with the
7x7 weight and data gradients, the level-input adjoint and the resize adjoint of include/sr_hip_flow_bwd.h.
Gradients with respect to the frames are not computed: ``ref`` or ``supp`` requiring grad raises NotImplementedError.  fp32 only.
ValueError for ``ref`` and ``supp`` of different sizes, channels other than 3, and a side of 32 pixels or fewer (the reference
fails there: its level-0 flow is empty).
"""
import math

import torch
from torch import nn

from .. import _lib, hip_ops
from ..utils.registry import ARCH_REGISTRY
from .arch_util import Conv3x3Params
from .hip_generator import HipGenerator

_CHANNELS = ((8, 32), (32, 64), (64, 32), (32, 16), (16, 2))
_LEVELS = 6
_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class BasicModule(nn.Module):
    """Parameters of SpyNet's basic module: five 7x7 convs at indices 0, 2, 4, 6, 8 of ``basic_module`` (the ReLUs between them
    run in the conv epilogues).  No forward: SpyNet issues the launches."""

    def __init__(self):
        super().__init__()
        layers = []
        for i, (cin, cout) in enumerate(_CHANNELS):
            layers.append(Conv3x3Params(cin, cout, ksize=7))
            if i + 1 < len(_CHANNELS):
                layers.append(nn.ReLU(inplace=False))
        self.basic_module = nn.Sequential(*layers)

    def convs(self):
        return [self.basic_module[i] for i in range(0, 9, 2)]

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('BasicModule is a parameter container; SpyNet launches the HIP kernels')


@ARCH_REGISTRY.register()
class SpyNet(HipGenerator):
    """The six-level flow estimator.  ``load_path``: a checkpoint whose ``'params'`` entry holds the convolution parameters
    (the pretrained SpyNet the reference's video networks load); None keeps the default initialisation."""

    def __init__(self, load_path=None):
        super().__init__()
        self.basic_module = nn.ModuleList(BasicModule() for _ in range(_LEVELS))
        if load_path:   # before the buffers exist, as the reference: the checkpoint holds the convolutions only
            checkpoint = torch.load(load_path, map_location='cpu')
            self.load_state_dict(checkpoint['params'])
        for name, values in (('mean', _MEAN), ('std', _STD)):
            self.register_buffer(name, torch.tensor(values, dtype=torch.float32).view(1, 3, 1, 1))
        self._autograd = False

    def set_autograd(self, enabled=True):
        """Whether a forward that needs a graph (train mode, grad enabled, a parameter requiring grad) builds one
        (archs/spynet_autograd.py) instead of being refused.  Off by default; set after construction, like set_compute_dtype.
        Returns self."""
        self._autograd = bool(enabled)
        return self

    def process(self, ref, supp, levels=None, keep=None):
        """The pyramid on a batch whose sides are multiples of 32: the flow [N, 2, H, W]; ``levels`` (a list) receives the flow
        after each level; ``keep`` (a list) receives per level what the backward reads: the level's ``supp``, its input block
        ``x0``, the four post-ReLU activations ``acts`` and ``up``."""
        n = ref.size(0)
        mean, std = self._norm_host()
        both = hip_ops.spynet_preprocess(torch.cat([ref, supp], 0), mean, std)
        pyramid = [both]
        for _ in range(5):
            pyramid.insert(0, hip_ops.avgpool2x2(pyramid[0]))
        flow = None
        for level, imgs in enumerate(pyramid):
            x, up = hip_ops.spynet_level_input(imgs[:n], imgs[n:], flow)
            convs = self.basic_module[level].convs()
            if keep is not None:   # without it an activation is freed as soon as the next conv has read it
                keep.append(dict(supp=imgs[n:], x0=x, acts=[], up=up))
            for conv in convs[:-1]:
                x = hip_ops.conv7x7(x, self.packed(conv), relu=True)
                if keep is not None:
                    keep[-1]['acts'].append(x)
            flow = hip_ops.conv7x7(x, self.packed(convs[-1]), res1=up)
            if levels is not None:
                levels.append(hip_ops.cb_to_nchw(flow, 2))
        return hip_ops.cb_to_nchw(flow, 2)

    def run_forward(self, ref, supp, levels=None, keep=None):
        """The whole forward on device tensors.  ``keep``: a dict that receives ``size`` = (h, w, h_floor, w_floor) and ``levels``,
        the per-level tensors ``process`` saves for the backward."""
        h, w = ref.size(2), ref.size(3)
        h_floor, w_floor = 32 * math.ceil(h / 32), 32 * math.ceil(w / 32)
        if (h_floor, w_floor) != (h, w):
            both = hip_ops.resize_bilinear(torch.cat([ref, supp], 0), (h_floor, w_floor))
            ref, supp = both[:ref.size(0)], both[ref.size(0):]
        if keep is not None:
            keep['size'], keep['levels'] = (h, w, h_floor, w_floor), []
        flow = self.process(ref, supp, levels, None if keep is None else keep['levels'])
        if (h_floor, w_floor) != (h, w):
            flow = hip_ops.resize_bilinear(flow, (h, w))
            ratio = torch.tensor([float(w) / float(w_floor), float(h) / float(h_floor)], dtype=torch.float32, device=flow.device)
            hip_ops.launch('sr_channel_affine_f32', flow.device, flow.data_ptr(), flow.data_ptr(), ratio.data_ptr(), None, flow.size(0), 2,
                           h * w)
        return flow

    def forward(self, ref, supp):
        if ref.size() != supp.size():
            raise ValueError(f'SpyNet: ref {tuple(ref.shape)} and supp {tuple(supp.shape)} must have the same size')
        if ref.dim() != 4 or ref.size(1) != 3:
            raise ValueError(f'SpyNet: expected [N, 3, H, W] frames, got {tuple(ref.shape)}')
        if min(ref.size(2), ref.size(3)) <= 32:
            raise ValueError(f'SpyNet: a {ref.size(2)}x{ref.size(3)} frame is too small; both sides must exceed 32 pixels')
        if ref.dtype != torch.float32 or supp.dtype != torch.float32:
            raise ValueError(f'SpyNet: {ref.dtype} / {supp.dtype} input is not supported; supported: fp32')
        if not (ref.is_cuda and supp.is_cuda):
            raise _lib.SrHipError('SpyNet.forward runs only on a HIP device (no CPU fallback): move the module and inputs with '
                                  '.to("cuda")')
        if self.training and torch.is_grad_enabled() and (ref.requires_grad or supp.requires_grad
                                                          or any(p.requires_grad for p in self.parameters())):
            if not self._autograd:
                raise NotImplementedError('SpyNet runs inference only by default: call .eval() (or run under torch.no_grad()), or '
                                          'enable its backward (the 7x7 weight and data gradients through the pyramid levels) with '
                                          'set_autograd(True)')
            if ref.requires_grad or supp.requires_grad:
                raise NotImplementedError('SpyNet computes no image gradients: ref and supp must not require grad (the frames are '
                                          'data; only the parameters are differentiated)')
            from .spynet_autograd import spynet_apply
            return spynet_apply(self, ref.contiguous(), supp.contiguous())
        with torch.no_grad():
            return self.run_forward(ref.contiguous(), supp.contiguous())
