#!/usr/bin/env python
"""tests/golden/make_golden_tcn_ff.py — regenerates tests/golden/tcn_beam_ff.npz.

Runs ONLY where the reference checkout exists (/root/reference): it imports the reference's own
att_speech.modules.tcn under the installed Python with empty stub modules for the absent
third-party packages and the `beam_search.py[:182]` shim of make_golden.py::golden_tcn_beam
(the file's later classes are Python 2), builds `AttentionDecoderTCN` with
`att_force_forward = (-2, 6)` and `learnable_initial_attention = False`, runs `decode` for
beam 1 and beam 3 on seeded inputs and stores inputs + the reference's outputs.  Data only;
nothing of the reference's source travels.

Records: state_dict (every parameter perturbed, a raised EOS bias), encoder output, lengths,
the window; per beam (`b1_`, `b3_`): decoded labels (flat + lengths), acoustic scores, finished
counts, final estimations and beam scores, the step logits, the alignment of every step
[steps + 1, T', hyp], the smallest decision margin and the smallest peak of an alignment that
a window was computed from.

The first alignment is a one-hot and the window is 8 frames wide, so every later alignment has
at least 1/8 of its mass on one frame: the window is active on every row of every step
(asserted here from the recorded alignments).  A record is stored only if, at every step of the
reference's search, the last kept and the first dropped candidate score, and EOS and the best
other class of every live hypothesis, are more than 1e-3 apart (the floor of
make_golden_attention_rnn.py); otherwise the seed is advanced.

Usage:  python tests/golden/make_golden_tcn_ff.py
"""
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'

for name in ['pywrapfst', 'torchtext', 'torchtext.vocab', 'kaldi_io', 'tensorboardX']:
    sys.modules[name] = types.ModuleType(name)
sys.modules['torchtext'].vocab = sys.modules['torchtext.vocab']
sys.modules['torchtext.vocab'].Vocab = object
sys.modules['tensorboardX'].SummaryWriter = object
sys.path.insert(0, REF)

import numpy as np          # noqa: E402
import torch                # noqa: E402

warnings.filterwarnings('ignore')
torch.set_num_threads(4)

MARGIN = 1e-3
E, HH, A, S, T, B = 16, 24, 8, 7, 40, 3
LENS = [40, 23, 9]
WINDOW = (-2, 6)
GUARD = 12
EOS_BIAS = 1.0
KW = dict(tcn_hidden_size=HH, att_hidden_size=A, dropout_p=0.0, kernel_size=3,
          dilation_sizes=[1, 2], beam_size=3, length_normalization=0.6,
          attention_temperature=1.25, tcn_layers_per_block=2,
          learnable_initial_attention=False, att_force_forward=WINDOW)


def reference_module():
    from att_speech.configuration import Globals
    Globals.cuda = False
    src = open(os.path.join(REF, 'att_speech/modules/beam_search.py')).read().split('\n')
    ns = {}
    exec(compile('\n'.join(src[:182]), 'beam_search.py[:182]', 'exec'), ns)
    margins = []

    class WatchedBeamSearch(ns['BeamSearch']):
        """the reference's search; records the decision margins of every step"""

        def step(self, logits, *args, **kwargs):
            C, beam, bs = self.num_classes, self.beam_size, self.batch_size
            gs = torch.log_softmax(logits.squeeze(0), 1) + self.scores[:, None]
            live = torch.isfinite(self.scores)
            if self.estimations is not None and bool(live.any()):
                other = gs[:, :-1].max(1)[0]
                margins.append(float((gs[:, -1] - other).abs()[live].min()))
            cand = gs[:, :-1].contiguous().view(bs, -1)
            if self.estimations is None:
                cand = cand[:, :C - 1]
            if cand.size(1) > beam:
                top = torch.sort(cand, 1, descending=True)[0]
                gap = top[:, beam - 1] - top[:, beam]
                gap = gap[torch.isfinite(gap)]
                if gap.numel():
                    margins.append(float(gap.min()))
            return super(WatchedBeamSearch, self).step(logits, *args, **kwargs)

    shim = types.ModuleType('att_speech.modules.beam_search')
    shim.BeamSearch = WatchedBeamSearch
    shim.BeamSearchLM = shim.GraphSearch = shim.RescoreSearchLM = object
    sys.modules['att_speech.modules.beam_search'] = shim
    from att_speech.modules import tcn as ref_tcn
    return ref_tcn, margins


def make_decoder(ref_tcn, seed):
    torch.manual_seed(seed)
    dec = ref_tcn.AttentionDecoderTCN({'features': torch.zeros(T, B, E)}, S, **KW)
    dec.eval()
    with torch.no_grad():
        for prm in dec.parameters():            # make the decoder non-trivial
            prm.add_(torch.randn_like(prm) * 0.1)
        dec.output_to_logits.bias[S] += EOS_BIAS     # EOS competitive -> hypotheses finish
    return dec


def decode_record(dec, enc, lens, beam, margins, out):
    dec.beam_size = beam
    dec.TRANSCRIPTION_LEN_GUARD = GUARD
    del margins[:]
    with torch.no_grad():
        res = dec.decode(enc, lens, return_attention=True)
    key = 'b%d_' % beam
    att = torch.stack(res['attweights']).numpy()                    # [steps + 1, T', hyp]
    out[key + 'flat'] = np.array([int(c) for d in res['decoded'] for c in
                                  (d.tolist() if hasattr(d, 'tolist') else d)], np.int64)
    out[key + 'lens'] = np.array([len(d) for d in res['decoded']], np.int64)
    out[key + 'scores'] = np.array([float(v) for v in res['decoded_scores']['acoustic']],
                                   np.float64)
    out[key + 'finished_count'] = np.array(res['beam_search'].finished_count, np.int64)
    out[key + 'final_estimations'] = res['beam_search'].estimations.numpy()
    out[key + 'final_beam_scores'] = res['beam_search'].scores.numpy()
    out[key + 'step_logits'] = torch.cat(res['logits']).numpy()
    out[key + 'att'] = att
    out[key + 'margin'] = np.float64(min(margins))
    # every alignment but the last is one a window was computed from
    out[key + 'min_peak'] = np.float64(att[:-1].max(1).min())
    return float(out[key + 'margin']), float(out[key + 'min_peak'])


def main():
    ref_tcn, margins = reference_module()
    for seed in range(1010, 1200):
        dec = make_decoder(ref_tcn, seed)
        g = torch.Generator().manual_seed(seed + 1000)
        enc = torch.randn(T, B, E, generator=g)
        lens = torch.tensor(LENS)
        out = {'S': np.int32(S), 'guard': np.int32(GUARD), 'seed': np.int32(seed),
               'enc': enc.numpy(), 'lens': lens.numpy(), 'window': np.array(WINDOW, np.int64)}
        for k, v in dec.state_dict().items():
            out['sd_' + k] = v.detach().numpy().copy()
        stats = [decode_record(dec, enc, lens, beam, margins, out) for beam in (1, 3)]
        worst, peak = min(s[0] for s in stats), min(s[1] for s in stats)
        if (worst > MARGIN and peak >= 0.125
                and all(out['b%d_lens' % b].min() > 0 for b in (1, 3))):
            break
        print('seed %d: decision margin %.2e, smallest peak %.3f, reseeding' % (seed, worst, peak))
    else:
        raise SystemExit('no seed with clear decode margins')
    path = os.path.join(HERE, 'tcn_beam_ff.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d arrays, %d bytes), seed %d, margin %.3g, smallest peak %.3f, steps %s' % (
        path, len(out), os.path.getsize(path), seed, worst, peak,
        [out['b%d_att' % b].shape[0] - 1 for b in (1, 3)]))


if __name__ == '__main__':
    main()
