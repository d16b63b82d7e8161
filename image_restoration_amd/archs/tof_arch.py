"""TOFlow, the task-oriented-flow video restorer of the reference (``basicsr/archs/tof_arch.py``), on libsr_hip.so.  Inference
only, fp32.

Same constructors, state_dict keys, order and shapes as the reference (114 entries, 1,405,899 parameters: the ``mean`` / ``std``
buffers, ``spynet.basic_module.{0..3}.basic_module.{0,3,6,9}.weight`` with the BatchNorm entries of ``{1,4,7,10}`` — every
``num_batches_tracked`` included — and ``.12.{weight,bias}``, then ``conv_1`` .. ``conv_4``) and PyTorch's default
initialisation, so a reference checkpoint loads with ``strict=True``.  The modules only hold parameters; a forward is a
composition of launches (include/sr_hip_tof.h, include/sr_hip_flow.h, include/sr_hip_ridnet.h):

    (x - mean) / std                 sr_spynet_preprocess_f32 on the 7 b frames, once
    three 2x2 average pools          sr_avgpool2x2_f32 on the whole clip: the six (ref, supp) pairs of a clip share its frames
    per level, ONE batch of 6 b      sr_tof_level_input_f32 reads the pairs in place from the clip's pyramid (image 6 b + k):
                                     [ref, warp(supp, up, zeros), up] as one CB8 block, and up
                                     five sr_conv7x7_f32 (8 -> 32 -> 64 -> 32 -> 16 -> 2), ReLU in the epilogue of the first
                                     four, the level's ``+ up`` as res1 of the fifth
    aligned stack                    sr_tof_align_f32: the 21 channels of conv_1 (3 CB8 blocks) from the clip and the six flows
    conv_1, conv_2                   sr_tof_conv9x9_f32 with ReLU
    conv_3, conv_4                   sr_convd_f32, ksize 1 (slope 0, then none)
    (y + lr_ref) * std + mean        sr_tof_finish_f32

BatchNorm runs in eval mode only and costs no launch: it is folded into the bias-free 7x7 conv in front of it,
``w' = w * gamma / sqrt(var + eps)``, ``b' = beta - mean * gamma / sqrt(var + eps)``, computed in float64 on the host and rounded
once to fp32 (``arch_util.fold_batchnorm``).  The folded image is cached by ``HipGenerator.derived`` on the storage, version and
FlatAdam epoch of the conv weight and of the four BatchNorm tensors, so an in-place change of ``running_var`` is seen by the next
forward.  A module in training mode raises NotImplementedError (batch statistics are not built), even under ``torch.no_grad()``
(``arch_util.refuse_inference_only``).

ValueError for a clip that is not ``[b, 7, 3, h, w]`` fp32 and for h or w that is not a multiple of 16 (the reference's
``torch.cat`` fails there); NotImplementedError when a graph would be needed; ``_lib.SrHipError`` for CPU tensors.
"""
import torch
from torch import nn

from .. import hip_ops
from ..utils.registry import ARCH_REGISTRY
from .arch_util import Conv3x3Params, fold_batchnorm, refuse_inference_only  # noqa: F401  (fold_batchnorm: its old home)
from .hip_generator import HipGenerator

_CHANNELS = ((8, 32), (32, 64), (64, 32), (32, 16), (16, 2))
_LEVELS = 4
_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_OFFICIAL_ORDER = (3, 0, 1, 2, 4, 5, 6)
_BN = 'folded into the 7x7 convs from'   # what refuse_inference_only says of the BatchNorm layers


class BasicModule(nn.Module):
    """Parameters of SPyNetTOF's basic module: 7x7 convs at indices 0, 3, 6, 9 (no bias) and 12 of ``basic_module``, a
    BatchNorm2d after each of the first four (indices 1, 4, 7, 10); the ReLUs (2, 5, 8, 11) run in the conv epilogues.  No
    forward: SPyNetTOF issues the launches."""

    def __init__(self):
        super().__init__()
        layers = []
        for i, (cin, cout) in enumerate(_CHANNELS):
            last = i + 1 == len(_CHANNELS)
            layers.append(Conv3x3Params(cin, cout, bias=last, ksize=7))
            if not last:
                layers += [nn.BatchNorm2d(cout), nn.ReLU(inplace=True)]
        self.basic_module = nn.Sequential(*layers)

    def conv_bn(self):
        """[(conv, its BatchNorm)] of the first four layers."""
        return [(self.basic_module[i], self.basic_module[i + 1]) for i in range(0, 12, 3)]

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('BasicModule is a parameter container; SPyNetTOF launches the HIP kernels')


class SPyNetTOF(HipGenerator):
    """The four-level flow estimator of TOFlow.  ``load_path``: a checkpoint whose ``'params'`` entry holds the state_dict; None
    keeps the default initialisation.  Normalisation is the caller's, as in the reference."""

    def __init__(self, load_path=None):
        super().__init__()
        self.basic_module = nn.ModuleList([BasicModule() for _ in range(_LEVELS)])
        if load_path:
            self.load_state_dict(torch.load(load_path, map_location=lambda storage, loc: storage)['params'])

    def packed_bn(self, conv, bn):
        """The 7x7 weight image of ``conv`` with eval-mode ``bn`` folded in (hip_ops.PackedConv7x7), rebuilt when the conv
        weight or a BatchNorm parameter or buffer changed."""
        tensors = (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)
        dev = conv.weight.device
        return self.derived((id(conv), 'bn'), tensors, float(bn.eps),
                            lambda: hip_ops.PackedConv7x7(*(t.to(dev) for t in fold_batchnorm(*tensors, bn.eps))))

    def flows(self, level_input):
        """The pyramid: ``level_input(level, flow_prev)`` -> (the level's CB8 input block, up).  Returns the finest flow as a
        one-block CB8 buffer (channels 0, 1)."""
        flow = None
        for level in range(_LEVELS):
            module = self.basic_module[level]
            x, up = level_input(level, flow)
            for conv, bn in module.conv_bn():
                x = hip_ops.conv7x7(x, self.packed_bn(conv, bn), relu=True)
            flow = hip_ops.conv7x7(x, self.packed(module.basic_module[12]), res1=up)
        return flow

    def forward(self, ref, supp):
        if ref.size() != supp.size():
            raise ValueError(f'SPyNetTOF: ref {tuple(ref.shape)} and supp {tuple(supp.shape)} must have the same size')
        if ref.dim() != 4 or ref.size(1) != 3 or ref.dtype != torch.float32 or supp.dtype != torch.float32:
            raise ValueError(f'SPyNetTOF: expected fp32 [N, 3, H, W] frames, got {ref.dtype} {tuple(ref.shape)}')
        if ref.size(2) % 16 or ref.size(3) % 16 or ref.numel() == 0:
            raise ValueError(f'SPyNetTOF: h and w must be positive multiples of 16, got {ref.size(2)}x{ref.size(3)}')
        refuse_inference_only('SPyNetTOF', self.training, (ref, supp), self.parameters(), _BN)
        with torch.no_grad():
            n = ref.size(0)
            pyramid = [torch.cat([ref, supp], 0).contiguous()]
            for _ in range(_LEVELS - 1):
                pyramid.insert(0, hip_ops.avgpool2x2(pyramid[0]))
            flow = self.flows(lambda level, prev: hip_ops.tof_level_input(pyramid[level][:n], pyramid[level][n:], prev))
            return hip_ops.cb_to_nchw(flow, 2)


@ARCH_REGISTRY.register()
class TOFlow(HipGenerator):
    """TOFlow: [b, 7, 3, h, w] pre-upsampled LR frames -> the restored centre frame [b, 3, h, w].  ``adapt_official_weights``:
    reorder the frames to [3, 0, 1, 2, 4, 5, 6] and take frame 0 as the reference, for weights translated from the official
    implementation."""

    def __init__(self, adapt_official_weights=False):
        super().__init__()
        self.adapt_official_weights = adapt_official_weights
        self.ref_idx = 0 if adapt_official_weights else 3
        for name, values in (('mean', _MEAN), ('std', _STD)):
            self.register_buffer(name, torch.Tensor(values).view(1, 3, 1, 1))
        self.spynet = SPyNetTOF()
        self.conv_1 = Conv3x3Params(3 * 7, 64, ksize=9)
        self.conv_2 = Conv3x3Params(64, 64, ksize=9)
        self.conv_3 = Conv3x3Params(64, 64, ksize=1)
        self.conv_4 = Conv3x3Params(64, 3, ksize=1)

    def invalidate_packed(self):
        super().invalidate_packed()
        self.spynet.invalidate_packed()

    def run_forward(self, lrs, keep=None):
        """The whole forward on a contiguous fp32 device clip.  ``keep`` (a dict) receives ``flows``, the six flows of each clip
        as [6 b, 2, h, w] (image 6 b + k, k counting the frames other than the reference in order)."""
        b, _, _, h, w = lrs.shape
        if self.adapt_official_weights:
            lrs = lrs[:, list(_OFFICIAL_ORDER)].contiguous()
        mean, std = self._norm_host()
        r = self.ref_idx
        clip = hip_ops.spynet_preprocess(lrs.view(b * 7, 3, h, w), mean, std).view(b, 7, 3, h, w)
        pyramid = [clip]
        for _ in range(_LEVELS - 1):
            top = pyramid[0]
            pyramid.insert(0, hip_ops.avgpool2x2(top.view(b * 7, 3, top.size(3), top.size(4))).view(b, 7, 3, top.size(3) // 2,
                                                                                                   top.size(4) // 2))
        flows = self.spynet.flows(lambda level, prev: hip_ops.tof_level_input(None, None, prev, clip=pyramid[level], ref_idx=r))
        if keep is not None:
            keep['flows'] = hip_ops.cb_to_nchw(flows, 2)
        x = hip_ops.tof_align(clip, flows, r)
        x = hip_ops.conv9x9(x, self.packed(self.conv_1), relu=True)
        x = hip_ops.conv9x9(x, self.packed(self.conv_2), relu=True)
        x = hip_ops.convd(x, self.packed(self.conv_3), act_slope=0.0)
        y = hip_ops.convd(x, self.packed(self.conv_4))
        return hip_ops.tof_finish(y, clip, r, mean, std)

    def forward(self, lrs, keep=None):
        if lrs.dim() != 5 or lrs.size(1) != 7 or lrs.size(2) != 3 or lrs.dtype != torch.float32 or lrs.numel() == 0:
            raise ValueError(f'TOFlow: expected an fp32 [b, 7, 3, h, w] clip, got {lrs.dtype} {tuple(lrs.shape)}')
        if lrs.size(3) % 16 or lrs.size(4) % 16:
            raise ValueError(f'TOFlow: h and w must be multiples of 16 (four pyramid levels), got {lrs.size(3)}x{lrs.size(4)}')
        refuse_inference_only('TOFlow', self.training, (lrs,), self.parameters(), _BN)
        with torch.no_grad():
            return self.run_forward(lrs.contiguous(), keep)
