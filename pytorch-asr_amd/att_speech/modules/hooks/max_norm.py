"""reference modules/hooks/max_norm.py:10-33 — after backward, scale every weight of the
`tgt_modules` whose largest row norm exceeds `magnitude` down to it (prints included).  No recipe
uses it; it is here so that every hook name of the reference resolves."""
import torch

from att_speech.modules.hooks.hook import TrainingLoopHook


class MaxNorm(TrainingLoopHook):
    def __init__(self, magnitude, tgt_modules, **kwargs):
        self.magnitude = magnitude
        self.tgt_modules = tgt_modules
        super(MaxNorm, self).__init__(**kwargs)

    def _requires_norm(self, weight_name):
        if not weight_name.endswith('weight') or 'batch_norm' in weight_name:
            return False
        for mod in self.tgt_modules:
            if weight_name.startswith(mod):
                return True
        return False

    def post_backward(self, model, optimizer, current_iteration, loss):
        for name, weight in model.named_parameters():
            if self._requires_norm(name):
                print(name)
                scale = self.magnitude / torch.max(torch.norm(weight, dim=1), dim=0)[0]
                if scale < 1.0:
                    print("Applying scale %f to %s" % (scale.item(), name))
                    weight.data.mul_(scale)
