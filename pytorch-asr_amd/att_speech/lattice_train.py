"""Training against lattices that stay on the device: the differentiable lattice objective.

`lattice_objective(log_probs, batch, ...)` is DeviceLatticeBatch.seq_objective as one autograd node: the
forward runs the launch of asr_lattice_seqtrain_f64 (csrc/lattice_train.hip) on the live log_probs and
keeps the occupancies, the backward hands them to the encoder as a [T, B, C] tensor.  'mmi' gives the log
partition function of every lattice (the denominator of lattice MMI, of boosted MMI with boost > 0 and a
frame alignment as `ref`), 'smbr' the expected frame accuracy.  DESIGN.md section 4.26;
att_speech.modules.sequence_losses holds the loss modules built on it."""
import numpy as np
import torch

from att_speech.lattice_dp import DeviceLatticeBatch


class _LatticeObjective(torch.autograd.Function):
    """objective [B] of a DeviceLatticeBatch as a function of log_probs [T, B, C]"""

    @staticmethod
    def forward(ctx, log_probs, batch, ref, criterion, acoustic_scale, lm_scale, boost, workspace_bytes):
        objective, _, occ = batch.seq_objective(log_probs.detach(), ref, criterion, acoustic_scale, lm_scale,
                                                boost, workspace_bytes=workspace_bytes)
        sc = batch.acoustic_scale if acoustic_scale is None else np.full(batch.num_utterances,
                                                                         float(acoustic_scale))
        ctx.scale = torch.from_numpy(np.asarray(sc, np.float64)).to(log_probs.device, torch.float32)
        ctx.save_for_backward(occ)
        ctx.dtype = log_probs.dtype
        path = torch.isfinite(objective)
        if criterion == 'smbr':                 # 0 without a path: told apart by the lattice itself
            path = path & torch.from_numpy(np.diff(batch.node_off) > 0).to(path.device)
        ctx.mark_non_differentiable(path)
        return torch.where(path, objective, torch.zeros_like(objective)).float(), path

    @staticmethod
    def backward(ctx, grad_out, _):
        (occ,) = ctx.saved_tensors              # zero for utterances without a path
        grad = occ * (grad_out.float() * ctx.scale)[None, :, None]
        return (grad.to(ctx.dtype),) + (None,) * 7


def lattice_objective(log_probs, batch, ref=None, criterion='mmi', acoustic_scale=None, lm_scale=1.0, boost=0.0,
                      workspace_bytes=None):
    """objective [B] float32 of `batch` (a DeviceLatticeBatch) under the live log_probs [T, B, C], with
    d objective[b] / d log_probs = acoustic_scale occ (DeviceLatticeBatch.seq_objective).  An utterance
    without a complete path contributes 0 and a zero gradient; the result's .skipped counts them and
    .has_path [B] bool names the others ('smbr', whose objective is 0 there anyway: the utterances whose
    lattice has no nodes).  A batch of CPU tensors runs the numpy twin."""
    if not isinstance(batch, DeviceLatticeBatch):
        raise TypeError("lattice_objective needs a DeviceLatticeBatch (DeviceLatticeBatch.from_lattices uploads "
                        "host lattices)")
    out, path = _LatticeObjective.apply(log_probs, batch, ref, criterion, acoustic_scale, lm_scale, float(boost),
                                        workspace_bytes)
    out.has_path = path
    out.skipped = int(path.numel() - int(path.sum()))
    return out
