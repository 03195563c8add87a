"""Stage-2 training-step measurement (development tool; bench.py is the contract benchmark):
the DeepSpeech2 encoder + AttentionDecoderTCN at the egs/wsj/yamls/lattice_decoding/tcn.yaml
dimensions (TCN 384, attention 64, dilations [1, 2], 2 layers per block, temperature 1.25,
dropout 0.3, 49 symbols + EOS), forward + backward + Adam on bench.synthetic_batch inputs.
The attention recurrence runs through the native scan (ASR_TCN_TRAIN_NATIVE=1) and through
the per-position loop (=0), alternating in one process.  Prints ms/step, the decoder's
forward + backward ms (device events around a synchronised region) and the scan kernels'
fp32 arithmetic floor; --json writes the same as one JSON document."""
import argparse
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
CU, CLOCK, FLOP_PER_CLK = 256, 2.4e9, 256      # MI355X: CUs, clock, fp32 FLOP/clk per CU
TCN_DEC = dict(class_name='att_speech.modules.tcn.AttentionDecoderTCN', att_hidden_size=64,
               attention_temperature=1.25, beam_size=1, branching_threshold=0.0,
               dilation_sizes=[1, 2], dropout_p=0.3, kernel_size=3, length_normalization=0.6,
               tcn_hidden_size=384, tcn_layers_per_block=2)


def scan_floor_ms(B, Tp, L, A, K=32):
    """fp32 floor of the two scan launches: one workgroup (one CU) per utterance, so the
    launch lasts at least one utterance's arithmetic (B <= CUs) or ceil(B / CUs) of them.
    Forward: the location filter (T'*A*K multiply-adds) per step; backward: the filter again
    (recomputed h), its gradient d_filt and the carry through it (3x)."""
    waves = -(-B // CU)
    fwd = 2.0 * L * Tp * A * K * waves / (FLOP_PER_CLK * CLOCK) * 1e3
    return fwd, 3 * fwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='20,256')
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=2, help='native / loop alternations')
    ap.add_argument('--only', choices=['native', 'loop'], default=None,
                    help='one path, one round (for a kernel trace)')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    T = a.frames
    enc_cfg, _ = bench.model_config(1, None)
    result = {'frames': T, 'iters': a.iters, 'rows': []}
    for B in [int(x) for x in a.batches.split(',')]:
        feats, lens, texts, llens = bench.synthetic_batch(B, T, 0, 1)
        sample = {'features': feats[:2].clone(), 'features_lengths': lens[:2].clone(),
                  'spkids': None}
        torch.manual_seed(0)
        model = SpeechModel(enc_cfg, dict(TCN_DEC), sample, S,
                            [str(i) for i in range(S)]).to(dev).train()
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
        for path in paths:
            os.environ['ASR_TCN_TRAIN_NATIVE'] = '1' if path == 'native' else '0'
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(a.iters):
                step()
            torch.cuda.synchronize()
            ms_step = (time.time() - t0) / a.iters * 1e3
            dec_ms = []
            for _ in range(a.iters):
                torch.cuda.synchronize()
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                dec_only()
                ev1.record()
                torch.cuda.synchronize()
                dec_ms.append(ev0.elapsed_time(ev1))
            row = {'B': B, 'path': path, 'T_enc': Tp, 'L': L, 'ms_per_step': round(ms_step, 3),
                   'decoder_fwd_bwd_ms': round(sorted(dec_ms)[len(dec_ms) // 2], 3)}
            result['rows'].append(row)
            print('B=%-4d %-6s  %.1f ms/step  decoder fwd+bwd %.2f ms  (T\'=%d, L=%d)'
                  % (B, path, row['ms_per_step'], row['decoder_fwd_bwd_ms'], Tp, L), flush=True)
        fwd, bwd = scan_floor_ms(B, Tp, L, TCN_DEC['att_hidden_size'])
        result.setdefault('scan_floor_ms', {})[str(B)] = {'fwd': round(fwd, 4), 'bwd': round(bwd, 4)}
        print('B=%-4d scan fp32 floor: fwd %.3f ms, bwd %.3f ms' % (B, fwd, bwd), flush=True)
        os.environ.pop('ASR_TCN_TRAIN_NATIVE', None)
        del model, opt
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(result, fh, indent=1)


if __name__ == '__main__':
    main()
