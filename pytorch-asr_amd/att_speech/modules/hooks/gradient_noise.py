"""reference modules/hooks/gradient_noise.py:5-16 — Gaussian noise on the gradients after
backward.  The standard deviation is kept bug-compatible: the reference squares its own
`gradient_noise / (1 + it)^0.55` before using it as the factor of `randn_like`.

With a flat gradient bucket (att_speech.dp: `bucket` is set by `dp.train_step`), or gradients that
are contiguous fp32 GPU tensors, the noise is one launch of csrc/noise.hip (tag 1, global index =
position among the optimizer's parameters, which is the offset in the bucket); the hook runs after
the all-reduce, and the draw depends only on (seed, iteration, index), so every rank adds the
same noise.  Otherwise (CPU, ASR_NATIVE_NOISE=0) a torch generator seeded from (seed, iteration)."""
import torch

from att_speech import noise
from att_speech.modules.hooks.hook import TrainingLoopHook


class ConstantGradientNoise(TrainingLoopHook):
    def __init__(self, gradient_noise, seed=None, **kwargs):
        self.gradient_noise = gradient_noise
        self.seed = seed
        self.bucket = None
        self._table = noise.SegmentTable()
        super(ConstantGradientNoise, self).__init__(**kwargs)

    def sigma(self, current_iteration):
        var = self.gradient_noise / (1 + current_iteration) ** 0.55
        return var ** 2

    def pre_run(self, model, optimizer):
        if self.seed is None:
            self.seed = noise.draw_seed()

    @torch.no_grad()
    def post_backward(self, model, optimizer, current_iteration, loss):
        if self.seed is None:
            self.pre_run(model, optimizer)
        var = self.sigma(current_iteration)
        params = [p for g in optimizer.param_groups for p in g['params']]
        flat = None if self.bucket is None else self.bucket.flat
        if flat is not None and noise.native_ok([flat]):
            self.bucket.check_views()
            table, nsegs = self._table.get([flat], [0], [var])
            noise.launch(table, nsegs, self.seed, noise.TAG_GRADIENT, current_iteration)
            return
        grads = [p.grad for p in params]
        starts, s = [], 0
        for p in params:
            starts.append(s)
            s += p.numel()
        if all(g is not None for g in grads) and noise.native_ok(grads):
            table, nsegs = self._table.get(grads, starts, [var] * len(grads))
            noise.launch(table, nsegs, self.seed, noise.TAG_GRADIENT, current_iteration)
            return
        gens = {}
        for p in params:
            g = gens.get(p.grad.device)
            if g is None:
                g = gens[p.grad.device] = noise.torch_generator(
                    p.grad.device, self.seed, noise.TAG_GRADIENT, current_iteration)
            p.grad += torch.randn(p.grad.shape, generator=g, device=p.grad.device,
                                  dtype=p.grad.dtype) * var
