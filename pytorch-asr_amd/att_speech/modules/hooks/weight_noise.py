"""reference modules/hooks/weight_noise.py:10-99 — Gaussian noise on the weights for the forward
and backward pass of a training step: `pre_train_forward` adds sigma * N(0, 1) to every
parameter whose name contains 'weight' (not 'batch_norm', not under `modules_supporting_noise`,
whose modules draw their own noise from their `weight_noise` attribute), `post_backward` takes
it off again before the optimizer step.  sigma is the first `weight_noise` dict entry whose key
is a prefix of the name (or the one float given).

  LinearIncreaseWeightNoise: sigma = min(1, it / start_iteration) * base, every iteration;
  ConstantWeightNoise:       sigma = base, only when it > start_iteration.

When every noised parameter is a contiguous fp32 GPU tensor the noise is one launch of
csrc/noise.hip each way over a cached segment table (att_speech.noise): z depends only on (seed,
iteration, the element's index among the noised parameters in named_parameters() order), so the
removal regenerates it instead of keeping the reference's per-parameter noise tensors, and all
ranks of a data-parallel run noise identically (the seed is broadcast from rank 0 in `pre_run`).
Anything else (CPU tensors, other dtypes, ASR_NATIVE_NOISE=0) takes a torch path with the same
rules that draws from a generator seeded from (seed, iteration) and keeps its noise tensors.

Deviation: the reference trainer stops calling post_backward hooks once one asked to skip
(trainer.py:257-261), which leaves that step's noise in the weights for good; here noise still
pending is taken off at the start of the next `pre_train_forward` (or by `remove_pending`)."""
import torch

from att_speech import noise
from att_speech.modules.hooks.hook import TrainingLoopHook


class WeightNoise(TrainingLoopHook):
    def __init__(self, weight_noise, start_iteration, modules_supporting_noise=None, seed=None,
                 **kwargs):
        self.weight_noise = weight_noise
        self.start_iteration = start_iteration
        self.modules_supporting_noise = modules_supporting_noise or []
        self.seed = seed
        self.rand_values = {}           # torch path: name -> the noise tensor added
        self._pending = None            # (iteration, native) of the noise now in the weights
        self._table = noise.SegmentTable()
        super(WeightNoise, self).__init__(**kwargs)

    def get_rand_val(self, name, current_iteration):
        raise NotImplementedError

    def _noise_now(self, current_iteration):
        raise NotImplementedError

    def get_base_weight_noise(self, name):
        if isinstance(self.weight_noise, dict):
            for k, v in self.weight_noise.items():
                if name.startswith(k):
                    return v
            raise ValueError("No weight noise information for {}".format(name))
        return self.weight_noise

    def _requires_noise(self, weight_name):
        if 'weight' not in weight_name or 'batch_norm' in weight_name:
            return False
        for mod in self.modules_supporting_noise:
            if weight_name.startswith(mod):
                return False
        return True

    def _apply_module_attrs(self, model, current_iteration, reset=False):
        for mod_name in self.modules_supporting_noise:
            obj = model
            for field in mod_name.split('.'):
                obj = getattr(obj, field)
            assert hasattr(obj, 'weight_noise')
            obj.weight_noise = 0.0 if reset else self.get_rand_val(mod_name, current_iteration)

    def pre_run(self, model, optimizer):
        if self.seed is None:
            self.seed = noise.draw_seed()

    def _noised(self, model):
        """(name, parameter, global index of its first element) in named_parameters() order."""
        out, start = [], 0
        for name, w in model.named_parameters():
            if self._requires_noise(name):
                out.append((name, w, start))
                start += w.numel()
        return out

    @torch.no_grad()
    def _add(self, model, current_iteration, sign):
        params = self._noised(model)
        if not params:
            return False
        ws = [w for _, w, _ in params]
        if noise.native_ok(ws):
            sig = [float(self.get_rand_val(n, current_iteration)) for n, _, _ in params]
            table, nsegs = self._table.get(ws, [s for _, _, s in params], sig)
            noise.launch(table, nsegs, self.seed, noise.TAG_WEIGHT, current_iteration, sign=sign)
            return True
        if sign > 0:
            gens = {}
            self.rand_values = {}
            for name, w, _ in params:
                sigma = self.get_rand_val(name, current_iteration)
                if sigma == 0:
                    continue
                g = gens.get(w.device)
                if g is None:
                    g = gens[w.device] = noise.torch_generator(w.device, self.seed, noise.TAG_WEIGHT,
                                                               current_iteration)
                rand = torch.randn(w.shape, generator=g, device=w.device, dtype=w.dtype)
                rand *= sigma
                self.rand_values[name] = rand
                w.data.add_(rand)
        else:
            for name, w, _ in params:
                rand = self.rand_values.get(name)
                if rand is not None:
                    w.data.add_(-rand)
            self.rand_values = {}
        return False

    def remove_pending(self, model):
        """Take off the noise still in the weights (and reset the modules' noise attribute)."""
        if self._pending is None:
            return
        it = self._pending
        self._pending = None
        self._apply_module_attrs(model, it, reset=True)
        self._add(model, it, -1)

    def pre_train_forward(self, model, optimizer, current_iteration):
        self.remove_pending(model)
        if not self._noise_now(current_iteration):
            return
        if self.seed is None:
            self.pre_run(model, optimizer)
        self._apply_module_attrs(model, current_iteration)
        self._add(model, current_iteration, +1)
        self._pending = current_iteration

    def post_backward(self, model, optimizer, current_iteration, loss):
        self.remove_pending(model)


class ConstantWeightNoise(WeightNoise):
    def get_rand_val(self, name, current_iteration):
        return self.get_base_weight_noise(name)

    def _noise_now(self, current_iteration):
        return current_iteration > self.start_iteration


class LinearIncreaseWeightNoise(WeightNoise):
    def get_rand_val(self, name, current_iteration):
        incr = min(1.0, float(current_iteration) / float(self.start_iteration))
        return incr * self.get_base_weight_noise(name)

    def _noise_now(self, current_iteration):
        return True
