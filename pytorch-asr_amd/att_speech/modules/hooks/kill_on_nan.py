"""reference modules/hooks/kill_on_nan.py:8-27 — skip the optimizer step when the loss is NaN or
+-inf, and end the run (exit status 1) when that has happened `grace_init_val` = 10 times.

Host mode (the default, and what `dp.train_step` uses without `fused=`): the reference's rule,
messages included, with its `loss.item()` read-back between forward and backward.

Device mode (the hook handed to `att_speech.fused_step.FusedClipAdam(kill_on_nan=...)`): no
read-back in the step.  `pre_backward` writes a device flag (csrc/noise.hip:
asr_nonfinite_flag_f32) and returns False; `post_backward` MAX-reduces it over the ranks when
world > 1 — after the backward pass, like the persistent LSTM's error word, so no collective
runs next to the recurrence — so every rank skips exactly when the global loss is not finite;
the update kernel reads the flag (asr_adam_clip_step_ex_f32) and skips the step on the device.
The counter and the messages follow when `FusedClipAdam.poll()` delivers the step's record, a
few steps late: `SystemExit(1)` surfaces from `poll()` / `drain()` (or `dp.train_step`, which
polls) up to the statistics ring's depth after the 10th non-finite step, as the LSTM time-out
already does.  The device flag does not say NaN from inf: the message names both."""
import torch
import torch.distributed as dist

from att_speech.modules.hooks.hook import TrainingLoopHook

INF = float('inf')
MINF = float('-inf')


class KillOnNan(TrainingLoopHook):
    def __init__(self, *args, **kwargs):
        super(KillOnNan, self).__init__(*args, **kwargs)
        self.grace_init_val = 10
        self.grace_counter = self.grace_init_val
        self.flag = None            # device mode: int32[1] on the GPU (set by attach_device)
        self.group = None           # process group of the flag's all-reduce

    @property
    def device_mode(self):
        return self.flag is not None

    def attach_device(self, device):
        """Switch to device mode (FusedClipAdam does this); returns the flag word."""
        if self.flag is None or self.flag.device != torch.device(device):
            self.flag = torch.zeros(1, dtype=torch.int32, device=device)
        return self.flag

    def _count(self, skip_step):
        self.grace_counter -= skip_step
        if self.grace_counter <= 0:
            print('Loss was nan/inf too many times. Killing.')
            raise SystemExit(1)

    def pre_backward(self, model, optimizer, current_iteration, loss):
        if self.device_mode:
            from att_speech import _native
            x = loss.detach()
            if x.device != self.flag.device:
                raise _native.NativeLibraryError('KillOnNan: the loss is not on the flag\'s device')
            x = x.to(torch.float32).contiguous().reshape(-1)
            _native.check(_native.lib().asr_nonfinite_flag_f32(
                _native._p(x), x.numel(), _native._p(self.flag), _native._stream()),
                'asr_nonfinite_flag_f32')
            return False
        skip_step = 0
        if torch.isnan(loss).item():
            print('Loss is nan. Killing soon...')
            skip_step = 1
        elif loss.item() == INF or loss.item() == MINF:
            print('Loss is inf. Killing soon...')
            skip_step = 1
        self._count(skip_step)
        return skip_step == 1

    def post_backward(self, model, optimizer, current_iteration, loss):
        if self.device_mode and dist.is_available() and dist.is_initialized() \
                and dist.get_world_size(self.group) > 1:
            dist.all_reduce(self.flag, op=dist.ReduceOp.MAX, group=self.group)
        return False

    def device_record(self, flagged):
        """FusedClipAdam.poll(): one completed step whose flag was `flagged`."""
        if flagged:
            print('Loss is nan or inf. Killing soon...')
        self._count(int(bool(flagged)))
