"""EDVRModel: VideoBaseModel with EDVR's two training options (behaviour of basicsr/models/edvr_model.py:8-67).

``train.dcn_lr_mul``  the parameters whose name contains ``dcn`` form a second Adam parameter group at ``lr * dcn_lr_mul``
    (normal parameters first, as in the reference).  1 (the default) is one group.
``train.tsa_iter``    below iteration ``tsa_iter`` only the parameters whose name contains ``fusion`` train; from iteration
    ``tsa_iter`` on all of them.  torch.optim.Adam skips a parameter without a gradient, so the others keep no optimiser state
    and their bias-correction count starts at ``tsa_iter``; ``optim.FlatAdam`` does the same from ``requires_grad`` (its
    docstring has the equivalence and its limit).

``train.deterministic_backward``  (an extension, default false) ``EDVR.set_deterministic(True)``: the input gradient of every
    deformable convolution sums in 64-bit integers (include/sr_hip_dcn_det.h) instead of float atomics, so two runs from one seed
    take bit-identical steps and a resumed run continues the uninterrupted one's trajectory bit for bit.  Off by default
    only because the float-atomic scatter is what this model has always run; DESIGN.md §39 has the measurements (the deterministic
    step is the faster one) and the argument for flipping the default later.

``dcn_lr_mul`` and ``tsa_iter`` go through ONE launch per step (sr_adam_step_groups_f32).  With neither option set the optimiser is the plain single-group
FlatAdam on sr_adam_step_f32, like every other model.

Deviations.  The reference freezes at ``current_iter == 1`` only, so a run resumed inside the warm-up trains everything from
there; here the freeze holds for every iteration below ``tsa_iter``, resumed or not.  ``tsa_iter`` with a network built with
``with_tsa: false`` is a ValueError at construction: there is no TSA module to warm up, and the reference's recipes never
combine the two."""
from ..utils.registry import MODEL_REGISTRY
from .video_base_model import VideoBaseModel


@MODEL_REGISTRY.register()
class EDVRModel(VideoBaseModel):

    def __init__(self, opt):
        self.train_tsa_iter = None
        if opt['is_train']:
            self.train_tsa_iter = opt['train'].get('tsa_iter')
            if self.train_tsa_iter and not opt['network_g'].get('with_tsa', True):
                raise ValueError('train.tsa_iter trains the TSA fusion module alone first, but network_g.with_tsa is false: '
                                 'there is no TSA module to train')
        self._tsa_frozen = False
        super().__init__(opt)
        if opt['is_train'] and opt['train'].get('deterministic_backward', False):
            self.get_bare_model(self.net_g).set_deterministic(True)

    def setup_optimizers(self):
        train_opt = self.opt['train']
        dcn_lr_mul = train_opt.get('dcn_lr_mul', 1)
        self.logger.info(f'Multiple the learning rate for dcn with {dcn_lr_mul}.')
        block = dict(train_opt['optim_g'])
        kind = block.pop('type')
        if kind != 'Adam':
            raise NotImplementedError(f'optimizer {kind} is not supperted yet.')
        if dcn_lr_mul == 1:
            self.optimizer_g = self.gen.attach_adam(block, self.logger)
        else:   # normal parameters first, then the deformable convolutions at their own rate
            self.optimizer_g = self.gen.attach_adam(block, self.logger, group_of=lambda name: 1 if 'dcn' in name else 0,
                                                    group_lrs=[block['lr'], block['lr'] * dcn_lr_mul])

    def optimize_parameters(self, current_iter):
        if self.train_tsa_iter:
            if current_iter < self.train_tsa_iter and not self._tsa_frozen:
                self.logger.info(f'Only train TSA module for {self.train_tsa_iter} iters.')
                for name, param in self.net_g.named_parameters():
                    if 'fusion' not in name:
                        param.requires_grad = False
                self._tsa_frozen = True
            elif current_iter >= self.train_tsa_iter and self._tsa_frozen:
                self.logger.warning('Train all the parameters.')
                for param in self.net_g.parameters():
                    param.requires_grad = True
                self._tsa_frozen = False
        super().optimize_parameters(current_iter)
