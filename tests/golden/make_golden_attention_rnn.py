#!/usr/bin/env python
"""tests/golden/make_golden_attention_rnn.py — regenerates tests/golden/attention_rnn.npz.

Runs ONLY where the reference checkout exists (/root/reference): it imports the reference's own
att_speech.modules.decoders.attention_decoder under the installed Python with empty stub
modules for the absent third-party packages and the `beam_search.py[:182]` shim that
make_golden.py::golden_tcn_beam uses (the file's later classes are Python 2), runs
`AttentionDecoderRNN` on seeded inputs and stores inputs + the reference's outputs.  Data
only; nothing of the reference's source travels.

Records:
  main (n_layers = 1): state_dict (every parameter perturbed — the zero score vector would make
      every alignment uniform — and a raised EOS bias), loss, the L alignments, the L states,
      the gradient of every parameter and of `encoded`, `decode` for beam 1 and beam 3 with a
      shortened length guard;
  ff_  (att_force_forward set) and l2_ (n_layers = 2): state_dict, loss, alignments, states.

The decode results are only stored if, at every step of the reference's search and for every
utterance, the last kept and the first dropped candidate score, and EOS and the best other
class of every live hypothesis, are more than 1e-3 apart: a label comparison must not hang on
an fp32 tie.  Otherwise the seed is advanced.

Usage:  python tests/golden/make_golden_attention_rnn.py
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
E, H, S, T, B, L = 16, 24, 7, 14, 3, 5
GUARD = 12


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
    from att_speech.modules.decoders import attention_decoder as ref
    return ref, margins


def make_decoder(ref, seed, **kw):
    torch.manual_seed(seed)
    args = dict(n_layers=1, hidden_size=H, dropout_p=0.0, beam_size=3, length_normalization=0.6)
    args.update(kw)
    dec = ref.AttentionDecoderRNN({'features': torch.zeros(T, B, E)}, S, **args)
    with torch.no_grad():
        for prm in dec.parameters():
            prm.add_(torch.randn_like(prm) * 0.3)
        dec.output_to_logits.bias[S] += 1.5          # EOS competitive -> hypotheses finish
    return dec


def inputs(seed):
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(T, B, E, generator=g)
    texts = torch.randint(1, S, (B, L), generator=g, dtype=torch.int32)
    return enc, torch.tensor([14, 11, 8]), texts, torch.tensor([5, 4, 2])


def forward_record(dec, enc, lens, texts, tl, prefix, out, with_grads):
    for k, v in dec.state_dict().items():
        out[prefix + 'sd_' + k] = v.detach().numpy().copy()
    x = enc.clone().requires_grad_()
    fw = dec(x, lens, texts.clone(), tl, return_att_weights=True, return_rnn_states=True)
    out[prefix + 'loss'] = fw['loss'].detach().numpy()
    out[prefix + 'att'] = torch.stack(fw['attweights']).detach().numpy()       # [L, T, B]
    out[prefix + 'states'] = torch.stack(fw['rnnstates']).detach().numpy()     # [L, layers, B, H]
    if with_grads:
        fw['loss'].backward()
        for k, prm in dec.named_parameters():
            out[prefix + 'grad_' + k] = prm.grad.detach().numpy().copy()
        out[prefix + 'grad_encoded'] = x.grad.detach().numpy().copy()


def decode_record(dec, enc, lens, beam, margins, out):
    dec.eval()
    dec.beam_size = beam
    dec.TRANSCRIPTION_LEN_GUARD = GUARD
    del margins[:]
    with torch.no_grad():
        res = dec.decode(enc, lens)
    worst = min(margins)
    key = 'dec%d_' % beam
    out[key + 'flat'] = np.array([int(c) for d in res['decoded'] for c in
                                  (d.tolist() if hasattr(d, 'tolist') else d)], np.int64)
    out[key + 'lens'] = np.array([len(d) for d in res['decoded']], np.int64)
    out[key + 'scores'] = np.array([float(v) for v in res['decoded_scores']['acoustic']],
                                   np.float64)
    out[key + 'loss'] = np.float64(float(res['loss']))
    out[key + 'margin'] = np.float64(worst)
    return worst


def main():
    ref, margins = reference_module()
    for seed in range(7, 200):
        out = {'S': np.int32(S), 'guard': np.int32(GUARD), 'seed': np.int32(seed),
               'length_normalization': np.float64(0.6)}
        enc, lens, texts, tl = inputs(seed + 1000)
        out.update(enc=enc.numpy(), lens=lens.numpy(), texts=texts.numpy(),
                   text_lens=tl.numpy())
        dec = make_decoder(ref, seed)
        forward_record(dec, enc, lens, texts, tl, '', out, with_grads=True)
        worst = min(decode_record(dec, enc, lens, beam, margins, out) for beam in (1, 3))
        if worst > MARGIN and all(out['dec%d_lens' % b].min() > 0 for b in (1, 3)):
            break
        print('seed %d: decision margin %.2e, reseeding' % (seed, worst))
    else:
        raise SystemExit('no seed with clear decode margins')
    assert min(out['dec1_margin'], out['dec3_margin']) > MARGIN
    out['ff_window'] = np.array([-1, 4], np.int64)
    ff = make_decoder(ref, seed + 1, att_force_forward=(-1, 4))
    forward_record(ff, enc, lens, texts, tl, 'ff_', out, with_grads=False)
    two = make_decoder(ref, seed + 2, n_layers=2)
    forward_record(two, enc, lens, texts, tl, 'l2_', out, with_grads=False)
    path = os.path.join(HERE, 'attention_rnn.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d arrays, %d bytes), seed %d, margins %.3g / %.3g' % (
        path, len(out), os.path.getsize(path), seed, out['dec1_margin'], out['dec3_margin']))


if __name__ == '__main__':
    main()
