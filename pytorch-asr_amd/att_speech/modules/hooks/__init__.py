"""reference modules/hooks/__init__.py — the training-loop hooks the recipes name in
`Trainer.hooks`, plus ConstantGradientNoise."""
from att_speech.modules.hooks.gradient_clipping import GradientClipping
from att_speech.modules.hooks.gradient_noise import ConstantGradientNoise
from att_speech.modules.hooks.hook import TrainingLoopHook
from att_speech.modules.hooks.kill_on_nan import KillOnNan
from att_speech.modules.hooks.max_norm import MaxNorm
from att_speech.modules.hooks.polyak import PolyakDecay
from att_speech.modules.hooks.weight_noise import (ConstantWeightNoise, LinearIncreaseWeightNoise,
                                                   WeightNoise)

__all__ = ['ConstantGradientNoise', 'ConstantWeightNoise', 'GradientClipping', 'KillOnNan',
           'LinearIncreaseWeightNoise', 'MaxNorm', 'PolyakDecay', 'TrainingLoopHook', 'WeightNoise']
