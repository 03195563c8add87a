"""Decode-side measurements (development tool; bench.py is the contract benchmark):
config 1-3 greedy / Viterbi decode through FSTDecoder.decode and config 4, the TCN
attention decoder with plain BeamSearch (egs/wsj/yamls/lattice_decoding/tcn.yaml
shapes: tcn_hidden_size 384, dilations [1, 2], 2 layers per block, beam_size from
--beam).  Synthetic 40-dim x 1000-frame features, random weights; prints utterances/s
and input frames/s.

--decoder-only times AttentionDecoderTCN.decode alone on a random encoder output of --enc-frames
frames for every batch size of --batches (median, min and max of --iters timed calls; --out
writes them as JSON), with --force-forward LO HI and --no-learnable-init for the readme's
`att_force_forward` decode.  The score vector of LocalAttention starts at zero, which makes
every alignment uniform and, under a window, diffuse from the second step on (the window is
then inactive); --score-scale X draws it from N(0, X^2 / A) instead, and the fraction of
(step, hypothesis) rows with an active window is printed beside the times.  The A/B switches
(ASR_TCN_NATIVE, ASR_TCN_FF_NATIVE) are read from the environment as everywhere."""
import argparse
import datetime
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault('MIOPEN_USER_DB_PATH', os.path.join(ROOT, 'pytorch-asr_amd', 'miopen_db'))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-asr_amd'))
sys.path.insert(0, ROOT)

import bench                                   # noqa: E402  (model_config, synthetic_batch)
from att_speech.models import SpeechModel       # noqa: E402

S = 49


def timeit(fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.time() - t0) / n


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return sorted(out)


def decoder_only(a, dev):
    from att_speech.modules.tcn import AttentionDecoderTCN
    torch.manual_seed(0)
    E, A = 320, 64
    window = tuple(a.force_forward) if a.force_forward else None
    dec = AttentionDecoderTCN(
        {'features': torch.zeros(a.enc_frames, 2, E)}, S, tcn_hidden_size=384, att_hidden_size=A,
        dropout_p=0.3, kernel_size=3, dilation_sizes=[1, 2], tcn_layers_per_block=2,
        beam_size=a.beam, length_normalization=0.6, att_force_forward=window,
        learnable_initial_attention=not a.no_learnable_init).eval()
    if a.score_scale > 0:
        with torch.no_grad():
            dec.attn.hidden_to_score.weight.normal_(0.0, a.score_scale / A ** 0.5)
    dec = dec.to(dev)
    dec.TRANSCRIPTION_LEN_GUARD = a.steps
    batches = a.batches or [a.batch]
    enc = torch.randn(a.enc_frames, max(batches), E, generator=torch.Generator().manual_seed(1)).to(dev)
    res = {'date': datetime.date.today().isoformat(), 'device': torch.cuda.get_device_name(0),
           'enc_frames': a.enc_frames, 'steps': a.steps, 'beam': a.beam, 'force_forward': window,
           'learnable_initial_attention': not a.no_learnable_init, 'score_scale': a.score_scale,
           'switches': {k: os.environ.get(k) for k in ('ASR_TCN_NATIVE', 'ASR_TCN_FF_NATIVE')},
           'batches': {}}
    with torch.no_grad():
        for B in batches:
            e, lens = enc[:, :B].contiguous(), torch.full((B,), a.enc_frames)
            out = dec.decode(e, lens, return_attention=True)
            peaks = torch.stack(out['attweights'][:-1]).max(1)[0]
            active = float((peaks >= 0.1).float().mean()) if window else 0.0
            ts = timed(lambda: dec.decode(e, lens), a.iters)
            st = dict(ms_median=ts[len(ts) // 2] * 1e3, ms_min=ts[0] * 1e3, ms_max=ts[-1] * 1e3,
                      calls=len(ts), search=type(out['beam_search']).__name__,
                      label_steps=len(out['logits']), window_active=active)
            res['batches'][str(B)] = st
            print('TCN decode only  B=%-3d %-16s %8.1f ms (min %.1f max %.1f over %d calls)  %d steps, '
                  'window active on %.0f %% of the rows' % (
                      B, st['search'], st['ms_median'], st['ms_min'], st['ms_max'], st['calls'],
                      st['label_steps'], 100 * active), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--beam', type=int, default=10)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--force-forward', type=int, nargs=2, metavar=('LO', 'HI'), default=None)
    ap.add_argument('--no-learnable-init', action='store_true')
    ap.add_argument('--score-scale', type=float, default=0.0)
    ap.add_argument('--decoder-only', action='store_true')
    ap.add_argument('--batches', type=int, nargs='+', default=None)
    ap.add_argument('--enc-frames', type=int, default=334)
    ap.add_argument('--steps', type=int, default=120)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    if a.decoder_only:
        return decoder_only(a, dev)
    B, T = a.batch, a.frames
    feats, lens, texts, llens = bench.synthetic_batch(B, T, 0, 1)

    def sample():      # SpeechModel replaces sample_batch['features'] by the encoded probe (models.py:29-30)
        return {'features': feats[:2].clone(), 'features_lengths': lens[:2].clone(), 'spkids': None}
    enc_cfg, dec_cfg = bench.model_config(1, None)
    torch.manual_seed(0)
    with torch.no_grad():
        # ---- FSTDecoder: encoder + logits + Viterbi read-out (advanced_decoder.py:519-593)
        model = SpeechModel(enc_cfg, dec_cfg, sample(), S, [str(i) for i in range(S)]).to(dev).eval()
        f = feats.to(dev)
        dt = timeit(lambda: model.decode(f, lens, None, texts, llens), a.iters)
        print('FSTDecoder Viterbi decode  B=%d: %.1f ms/batch  %.0f utt/s  %.2f M frames/s'
              % (B, dt * 1e3, B / dt, B * T / dt / 1e6))
        # ---- TCN attention decoder + BeamSearch on the same encoder
        tcn_cfg = dict(class_name='att_speech.modules.tcn.AttentionDecoderTCN',
                       att_hidden_size=64, beam_size=a.beam, dilation_sizes=[1, 2], dropout_p=0.3,
                       kernel_size=3, length_normalization=0.6, tcn_hidden_size=384,
                       tcn_layers_per_block=2, learnable_initial_attention=not a.no_learnable_init,
                       att_force_forward=tuple(a.force_forward) if a.force_forward else None)
        enc_cfg2, _ = bench.model_config(1, None)
        model2 = SpeechModel(enc_cfg2, tcn_cfg, sample(), S, [str(i) for i in range(S)]).to(dev).eval()
        model2.decoder.TRANSCRIPTION_LEN_GUARD = a.steps
        dt = timeit(lambda: model2.decode(f, lens, None, texts, llens), max(1, a.iters - 1))
        print('TCN + BeamSearch(beam=%d) decode B=%d: %.1f ms/batch  %.1f utt/s  %.3f M frames/s'
              % (a.beam, B, dt * 1e3, B / dt, B * T / dt / 1e6))


if __name__ == '__main__':
    main()
