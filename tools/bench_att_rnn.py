"""RNN attention decoder measurement (development tool; bench.py is the contract benchmark):
the DeepSpeech2 encoder + AttentionDecoderRNN (hidden 256, one GRU layer, 49 symbols + EOS) on
bench.synthetic_batch inputs (1000 frames -> T' = 334, E = 320, L = 101), forward + backward +
Adam.  The label recurrence runs through the native scan (ASR_ATT_RNN_NATIVE=1) and through
the per-position loop on torch ops (=0), alternating in one process; per batch the medians over
the rounds are reported: ms/step, the decoder's forward + backward ms (device events around a
synchronised region), the two scan launches timed on their own, and the floor they are
compared with.  --decode adds the beam-10 decode throughput at B = 16, native against the torch
ops + host BeamSearch.  --json writes the same as one JSON document."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault('MIOPEN_USER_DB_PATH', os.path.join(ROOT, 'pytorch-asr_amd', 'miopen_db'))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-asr_amd'))
sys.path.insert(0, ROOT)

import bench                                   # noqa: E402  (model_config, synthetic_batch)
from att_speech import _native                  # noqa: E402
from att_speech.models import SpeechModel       # noqa: E402

S = 49
SWITCH = 'ASR_ATT_RNN_NATIVE'
CU, CLOCK = 256, 2.4e9                         # MI355X: CUs, clock
L2_PER_CU = 70e9                               # bytes/s one CU streams from its XCD's L2
TRANS_PER_CLK = 16                             # transcendental lanes per clock and CU (quarter rate)
RNN_DEC = dict(class_name='att_speech.modules.decoders.attention_decoder.AttentionDecoderRNN',
               n_layers=1, hidden_size=256, dropout_p=0.3, beam_size=1, length_normalization=0.6)


def scan_floor_ms(B, Tp, L, A, E, H):
    """What one workgroup (one CU) per utterance cannot beat, per launch: the fp32 weights of
    the three matrix-vector products streamed from L2 once per position, and T' * A tanh per
    position (exp + reciprocal) at the transcendental rate; the backward pass streams the
    transposed weights and recomputes the tanh.  ceil(B / CUs) utterances per CU in turn."""
    waves = -(-B // CU)
    weights = 4.0 * (A * H + 3 * H * E + 3 * H * H)
    stream = L * weights / L2_PER_CU * 1e3 * waves
    tanh = L * Tp * A * 2.0 / TRANS_PER_CLK / CLOCK * 1e3 * waves
    return {'weights_ms': round(stream, 4), 'tanh_ms': round(tanh, 4),
            'floor_ms': round(max(stream, tanh), 4)}


def median(xs):
    return statistics.median(xs)


def event_ms(fn, iters):
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        out.append(ev0.elapsed_time(ev1))
    return median(out)


def kernel_times(dec, encoded, enc_lens, L, iters):
    """the two scan launches alone, on the decoder's own weights"""
    H, dev = dec.hidden_size, encoded.device
    T, B, E = encoded.shape
    with torch.no_grad():
        eproj = dec.attn.encoded_to_hidden(encoded).contiguous()
        gx = torch.randn(L, B, 3 * H, device=dev) * 0.1
        w_ic = dec.rnn.weight_ih_l0[:, H:].contiguous()
        w_hh, b_hh = dec.rnn.weight_hh_l0.detach(), dec.rnn.bias_hh_l0.detach()
        w_rec = dec.attn.rec_state_to_hidden.weight.detach()
        v = dec.attn.hidden_to_score.weight.detach().reshape(-1).contiguous()
        bsc = dec.attn.hidden_to_score.bias.detach()
        h0 = torch.zeros(B, H, device=dev)
        lens = torch.as_tensor(enc_lens).to(dev, torch.int32)
        args = (eproj, encoded.contiguous(), lens, gx, w_ic, w_hh, b_hh, w_rec, v, bsc, h0)
        att, states, ctxs, gates, rec = _native.att_gru_scan_fwd(*args)
        fwd = event_ms(lambda: _native.att_gru_scan_fwd(*args), iters)
        wt = (w_ic.t().contiguous(), w_hh.t().contiguous(), w_rec.t().contiguous())
        d_states = torch.randn_like(states) * 1e-3
        bwd = event_ms(lambda: _native.att_gru_scan_bwd(
            eproj, args[1], lens, wt[0], wt[1], wt[2], v, h0, att, states, gates, rec, None,
            d_states), iters)
    return fwd, bwd


def decode_rate(dec, B, beam, rounds):
    g = torch.Generator().manual_seed(5)
    dev = next(dec.parameters()).device
    enc = torch.randn(334, B, dec.encoded_size, generator=g).to(dev)
    lens = torch.tensor([334 - 8 * b for b in range(B)], dtype=torch.int32)
    was = dec.beam_size, dec.training, dec.TRANSCRIPTION_LEN_GUARD
    dec.beam_size, dec.TRANSCRIPTION_LEN_GUARD = beam, 100
    dec.eval()
    rates = {'native': [], 'host': []}
    for _ in range(rounds):
        for path in ('native', 'host'):
            os.environ[SWITCH] = '1' if path == 'native' else '0'
            torch.cuda.synchronize()
            t0 = time.time()
            with torch.no_grad():
                dec.decode(enc, lens)
            torch.cuda.synchronize()
            rates[path].append(B / (time.time() - t0))
    os.environ.pop(SWITCH, None)
    dec.beam_size, _, dec.TRANSCRIPTION_LEN_GUARD = was
    dec.train(was[1])
    return {k: round(median(v), 2) for k, v in rates.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='20,256')
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=5, help='native / loop alternations')
    ap.add_argument('--only', choices=['native', 'loop'], default=None,
                    help='one path, one round (for a kernel trace)')
    ap.add_argument('--decode', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    T = a.frames
    enc_cfg, _ = bench.model_config(1, None)
    result = {'frames': T, 'iters': a.iters, 'rounds': a.rounds, 'rows': [], 'summary': []}
    for B in [int(x) for x in a.batches.split(',')]:
        feats, lens, texts, llens = bench.synthetic_batch(B, T, 0, 1)
        sample = {'features': feats[:2].clone(), 'features_lengths': lens[:2].clone(),
                  'spkids': None}
        torch.manual_seed(0)
        model = SpeechModel(enc_cfg, dict(RNN_DEC), sample, S,
                            [str(i) for i in range(S)]).to(dev).train()
        with torch.no_grad():      # a trained decoder's score vector is not zero
            model.decoder.attn.hidden_to_score.weight.normal_(0.0, 0.5)
        opt = torch.optim.Adam(model.parameters(), lr=4e-4)
        f = feats.to(dev)

        def step():
            opt.zero_grad(set_to_none=True)
            model(f, lens, None, texts, llens)['loss'].backward()
            opt.step()

        with torch.no_grad():
            encoded, enc_lens = model.encoder(f, lens, None, None)
        encoded = encoded.detach()
        Tp, L = encoded.size(0), texts.size(1) + 1

        def dec_only():
            x = encoded.clone().requires_grad_()
            model.decoder(x, enc_lens, texts, llens)['loss'].backward()

        paths = [a.only] if a.only else ['native', 'loop'] * a.rounds
        seen = {}
        for path in paths:
            os.environ[SWITCH] = '1' if path == 'native' else '0'
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(a.iters):
                step()
            torch.cuda.synchronize()
            ms_step = (time.time() - t0) / a.iters * 1e3
            dec_ms = event_ms(dec_only, a.iters)
            row = {'B': B, 'path': path, 'T_enc': Tp, 'L': L, 'ms_per_step': round(ms_step, 3),
                   'decoder_fwd_bwd_ms': round(dec_ms, 3)}
            result['rows'].append(row)
            seen.setdefault(path, []).append((ms_step, dec_ms))
            print('B=%-4d %-6s  %.1f ms/step  decoder fwd+bwd %.2f ms  (T\'=%d, L=%d)'
                  % (B, path, ms_step, dec_ms, Tp, L), flush=True)
        os.environ.pop(SWITCH, None)
        dec = model.decoder
        summary = {'B': B, 'T_enc': Tp, 'L': L}
        for path, vals in seen.items():
            summary[path + '_ms_per_step'] = round(median([v[0] for v in vals]), 3)
            summary[path + '_decoder_fwd_bwd_ms'] = round(median([v[1] for v in vals]), 3)
        if a.only != 'loop':
            fwd, bwd = kernel_times(dec, encoded, enc_lens, L, a.iters)
            floor = scan_floor_ms(B, Tp, L, dec.attn.hidden_size, dec.encoded_size,
                                  dec.hidden_size)
            summary.update(scan_fwd_ms=round(fwd, 3), scan_bwd_ms=round(bwd, 3), floor=floor,
                           fwd_fraction_of_floor=round(floor['floor_ms'] / fwd, 3),
                           bwd_fraction_of_floor=round(floor['floor_ms'] / bwd, 3))
        result['summary'].append(summary)
        print(json.dumps(summary), flush=True)
        if a.decode and B == int(a.batches.split(',')[0]):
            result['decode_B16_beam10_utt_per_s'] = decode_rate(dec, 16, 10, 3)
            print('decode', result['decode_B16_beam10_utt_per_s'], flush=True)
        del model, opt
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(result, fh, indent=1)


if __name__ == '__main__':
    main()
