"""BaseEncoder: the reference encoders' two freezing switches (unidistill/models/multisensor_fusion/base.py:50-67).

frozen_bn=True keeps every BatchNorm under the encoder on its running statistics while its convolutions go on training;
frozen_encoder=True stops the encoder's parameter gradients while gradient still flows THROUGH it (the camera branch of a fusion
student whose LiDAR half is frozen).  Both leave the state_dict untouched.  An eval-mode BatchNorm inside a training graph runs
on the frozen-statistics backward of csrc/bn_act.hip (ud_bn_act_bwd_frozen_ld*).
"""
from torch import nn
from torch.nn.modules.batchnorm import _BatchNorm


class BaseEncoder(nn.Module):
    def __init__(self, frozen_encoder=False, frozen_bn=False):
        super().__init__()
        self.frozen_encoder = bool(frozen_encoder)
        self.frozen_bn = bool(frozen_bn)

    def _freeze_stages(self):
        if self.frozen_encoder:
            for p in self.parameters():
                p.requires_grad = False

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        if mode and self.frozen_bn:
            for m in self.modules():
                if isinstance(m, _BatchNorm):
                    m.eval()
        return self
