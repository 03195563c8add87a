"""Sequence-discriminative losses against a word-level or large-LM decoding graph, with the denominator
taken from pruned lattices that stay on the device:

  LatticeMMILoss    -(sc log p(labels | acts) - log Z(lattice)), boosted MMI with boost > 0
  LatticeSMBRLoss   -(expected frame accuracy of the lattice's paths against the forced alignment)

Both take normalised log_probs [T, B, C], decode their own lattices from log_probs.detach() with
decode_lattice_device unless a DeviceLatticeBatch is passed in (lattices made once by a stale model can be
reused: the objective reads the live scores), and differentiate through
att_speech.lattice_train.lattice_objective, one launch of asr_lattice_seqtrain_f64.  The numerator of MMI is
the project's native CTC log-likelihood (fst_utils.path_reduction over the mono CTC lattice), the frame
reference of boosted MMI and sMBR ctc_viterbi_align_batch(...).frames.  CPU tensors run the numpy twins
(and torch's CTC for the numerator)."""
import numpy as np
import torch
from torch import nn

from att_speech.lattice_dp import DeviceLatticeBatch, decode_lattice_device
from att_speech.lattice_train import lattice_objective
from att_speech.modules import ctc_losses
from att_speech.wfst_decode import DEFAULT_WORKSPACE_BYTES


def _int_list(v):
    return [int(x) for x in torch.as_tensor(v).reshape(-1).tolist()]


def ctc_feasible(labels, act_lens, label_lens):
    """[B] bool: the transcript is not empty and fits its frames (one frame per label and one blank
    between equal neighbours)"""
    flat = _int_list(labels)
    out, o = [], 0
    for n, l in zip(_int_list(act_lens), _int_list(label_lens)):
        seq = flat[o:o + l]
        o += l
        out.append(l > 0 and n >= l + sum(1 for i in range(1, l) if seq[i] == seq[i - 1]))
    return np.array(out, bool)


def ctc_loglik(log_probs, labels, act_lens, label_lens):
    """log p(labels | log_probs) [B] of the mono CTC lattice (blank 0) on already normalised scores,
    differentiable: the native lattice kernel on a GPU (act_lens sorted, longest first, as for the other
    lattice losses), torch's CTC on CPU tensors.  Infeasible utterances hold an arbitrary finite value."""
    lens, lls = _int_list(act_lens), _int_list(label_lens)
    if log_probs.is_cuda:
        gg = ctc_losses._graph_gen(log_probs.size(2), 1)
        mats = gg.get_training_matrices_batch(ctc_losses._labels_to_batch(labels, lls), torch.as_tensor(lls))
        return -ctc_losses.path_reduction(log_probs, torch.as_tensor(lens), mats, negate=True)
    flat = torch.as_tensor(labels).reshape(-1).long()[:sum(lls)]
    return -nn.functional.ctc_loss(log_probs, flat, torch.as_tensor(lens), torch.as_tensor(lls), blank=0,
                                   reduction='none', zero_infinity=True)


class _LatticeLoss(nn.Module):
    """What the two losses share: the graph, the search and the scales.

    graph: a DecodingGraph; beam, lattice_beam: of decode_lattice_device; acoustic_scale: of the search and
    of the objective (the scores enter a path's cost as -acoustic_scale s); lm_scale: on the graph weights in
    the objective; boost >= 0: boost per correct frame added to a path's cost; workspace_bytes: of the search
    and of the objective's launch."""
    criterion = None

    def __init__(self, graph, beam=16.0, lattice_beam=8.0, acoustic_scale=1.0, lm_scale=1.0, boost=0.0,
                 workspace_bytes=DEFAULT_WORKSPACE_BYTES):
        super(_LatticeLoss, self).__init__()
        if not float(boost) >= 0.0 or not np.isfinite(float(boost)):
            raise ValueError("boost must be finite and >= 0")
        self.graph, self.beam, self.lattice_beam = graph, float(beam), float(lattice_beam)
        self.acoustic_scale, self.lm_scale, self.boost = float(acoustic_scale), float(lm_scale), float(boost)
        self.workspace_bytes = int(workspace_bytes)
        self.skipped = 0

    def decode(self, log_probs, act_lens):
        """the DeviceLatticeBatch of log_probs.detach() under the module's search settings"""
        with torch.no_grad():
            return decode_lattice_device(log_probs.detach(), _int_list(act_lens), self.graph, beam=self.beam,
                                         lattice_beam=self.lattice_beam, acoustic_scale=self.acoustic_scale,
                                         workspace_bytes=self.workspace_bytes)[0]

    def _prepare(self, log_probs, act_lens, labels, label_lens, lattices, want_ref):
        if log_probs.dim() != 3:
            raise ValueError("log_probs must be [T, B, C]")
        if lattices is None:
            lattices = self.decode(log_probs, act_lens)
        elif not isinstance(lattices, DeviceLatticeBatch):
            raise TypeError("lattices must be a DeviceLatticeBatch")
        feasible = ctc_feasible(labels, act_lens, label_lens)
        ref = None
        if want_ref:
            ali = ctc_losses.ctc_viterbi_align_batch(log_probs.detach().float(), labels, act_lens, label_lens,
                                                     num_symbols=log_probs.size(2))
            ref = ali.frames
            feasible = feasible & ali.feasible.cpu().numpy()
        return lattices, ref, torch.from_numpy(feasible).to(log_probs.device)

    def _objective(self, log_probs, lattices, ref):
        return lattice_objective(log_probs, lattices, ref, self.criterion, self.acoustic_scale, self.lm_scale,
                                 self.boost, workspace_bytes=self.workspace_bytes)

    def _finish(self, terms, keep):
        loss = torch.where(keep, terms, torch.zeros_like(terms)).sum()
        self.skipped = loss.skipped = int(keep.numel() - int(keep.sum()))
        return loss


class LatticeMMILoss(_LatticeLoss):
    """Lattice MMI: loss = -sum over the batch of (acoustic_scale log p(labels | log_probs) - log Z), log Z
    over the lattice's paths under the live scores; with boost > 0 boosted MMI (a denominator path is
    down-weighted by exp(-boost x its frames that agree with the forced alignment)).  Utterances whose
    transcript has no alignment or whose lattice has no path are left out; .skipped (on the module and on
    the result) counts them."""
    criterion = 'mmi'

    def forward(self, log_probs, act_lens, labels, label_lens, lattices=None):
        lattices, ref, feasible = self._prepare(log_probs, act_lens, labels, label_lens, lattices, self.boost > 0)
        den = self._objective(log_probs, lattices, ref)
        num = ctc_loglik(log_probs, labels, act_lens, label_lens).float()
        return self._finish(-(self.acoustic_scale * num - den), feasible & den.has_path)


class LatticeSMBRLoss(_LatticeLoss):
    """State-level minimum Bayes risk: loss = -sum over the batch of the expected number of frames on which
    a lattice path reads the class of the forced alignment (ctc_viterbi_align_batch(...).frames).  A
    nonzero boost reshapes the path distribution as in boosted MMI.  Skipped utterances as for
    LatticeMMILoss."""
    criterion = 'smbr'

    def forward(self, log_probs, act_lens, labels, label_lens, lattices=None):
        lattices, ref, feasible = self._prepare(log_probs, act_lens, labels, label_lens, lattices, True)
        obj = self._objective(log_probs, lattices, ref)
        return self._finish(-obj, feasible & obj.has_path)
