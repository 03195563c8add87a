"""The DeepSpeech2 recurrent stack with rnn_type=GRU: 4 bidirectional layers (first-layer input
F = 352 behind the conv front-end, H = 320, directions summed between layers), forward +
backward, timed with device events, the variants alternated round by round in one run:
  gru_native     native_gru.bigru per layer (persistent kernels)
  gru_per_step   the same with ASR_LSTM_PERSIST=0 (one launch per time step)
  gru_miopen     torch nn.GRU on packed input, the path BatchRNN took for GRU layers before
  lstm_native    the native BiLSTM stack (native_lstm.bilstm_stack) at the same shape
plus the recurrence kernels alone (forward + backward of one F == H layer, GRU against LSTM)
and one full SpeechModel training step (mono CTC, rnn_type='GRU') in frames/s.
  python tools/bench_gru.py [--batches 768,16] [--T 334] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'pytorch-asr_amd'))
from att_speech import _native                                    # noqa: E402
from att_speech.modules.encoders.native_gru import bigru          # noqa: E402
from att_speech.modules.encoders.native_lstm import bilstm_stack  # noqa: E402

dev = torch.device('cuda:0')
F0, H, NL = 352, 320, 4


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def stack_case(B, T, rounds, reps):
    torch.manual_seed(0)
    lens = torch.full((B,), T, dtype=torch.int64)
    x = torch.randn(T, B, F0, device=dev)
    dy = torch.randn(T, B, H, device=dev)
    grus = [nn.GRU(F0 if l == 0 else H, H, bidirectional=True, bias=False).to(dev) for l in range(NL)]
    lstms = [nn.LSTM(F0 if l == 0 else H, H, bidirectional=True, bias=False).to(dev) for l in range(NL)]

    def native():
        y = x.requires_grad_()
        for r in grus:
            y = bigru(y, lens, r, sum_dirs=True)
        y.backward(dy)

    def per_step():
        os.environ['ASR_LSTM_PERSIST'] = '0'
        try:
            native()
        finally:
            os.environ.pop('ASR_LSTM_PERSIST', None)

    def miopen():
        y = x.requires_grad_()
        for r in grus:
            packed = nn.utils.rnn.pack_padded_sequence(y, lens)
            out, _ = r(packed)
            out, _ = nn.utils.rnn.pad_packed_sequence(out, total_length=T)
            y = out.view(T, B, 2, H).sum(2)
        y.backward(dy)

    def lstm():
        y = bilstm_stack(x.requires_grad_(), lens, lstms)
        y.backward(dy)

    variants = {'gru_native': native, 'gru_per_step': per_step, 'gru_miopen': miopen,
                'lstm_native': lstm}
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, reps))
    _native.lstm_check_errors()
    return {k: {'median_ms': statistics.median(v), 'all_ms': v} for k, v in ms.items()}


def recurrence_case(B, T, rounds, reps):
    """the recurrence kernels of one F == H layer alone: GRU fwd + bwd against LSTM fwd + bwd"""
    g = torch.Generator().manual_seed(1)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    dy = torch.randn(T, B, H, generator=g).to(dev)
    gx3 = (torch.randn(T, B, 2, 3 * H, generator=g)).to(dev, torch.bfloat16)
    gx4 = (torch.randn(T, B, 2, 4 * H, generator=g)).to(dev, torch.bfloat16)
    w3 = (torch.randn(2, 3 * H, H, generator=g) / H ** 0.5).to(dev, torch.bfloat16)
    w4 = (torch.randn(2, 4 * H, H, generator=g) / H ** 0.5).to(dev, torch.bfloat16)
    w3T, w4T = w3.transpose(1, 2).contiguous(), w4.transpose(1, 2).contiguous()
    yg, _, gg = _native.gru_bidir_fwd(gx3, w3, lens)
    _, _, gl, cl = _native.lstm_bidir_fwd(gx4, w4, lens)
    cases = {
        'gru_fwd': lambda: _native.gru_bidir_fwd(gx3, w3, lens),
        'gru_bwd': lambda: _native.gru_bidir_bwd(dy, w3T, lens, gg, yg),
        'lstm_fwd': lambda: _native.lstm_bidir_fwd(gx4, w4, lens, want_y=False),
        'lstm_bwd': lambda: _native.lstm_bidir_bwd(dy, w4T, lens, gl, cl),
    }
    ms = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            ms[k].append(timed(fn, reps))
    _native.lstm_check_errors()
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {'median_ms': med, 'gru_over_lstm': (med['gru_fwd'] + med['gru_bwd']) / (med['lstm_fwd'] + med['lstm_bwd'])}


def train_step_case(B, T_raw, rounds):
    import bench
    from att_speech.models import SpeechModel
    feats, lens, texts, llens = bench.synthetic_batch(B, T_raw, 0, 1)
    enc_cfg, dec_cfg = bench.model_config(1)
    enc_cfg = dict(enc_cfg, rnn_type='GRU')
    torch.manual_seed(7)
    sb = {'features': feats[:2].clone(), 'features_lengths': lens[:2].clone(), 'spkids': None}
    model = SpeechModel(enc_cfg, dec_cfg, sb, 49, [str(i) for i in range(49)]).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    fd = feats.to(dev)

    def step():
        opt.zero_grad(set_to_none=True)
        out = model(fd, lens, None, texts, llens)
        out['loss'].backward()
        opt.step()
    ms = [timed(step, 3) for _ in range(rounds)]
    _native.lstm_check_errors()
    med = statistics.median(ms)
    return {'B': B, 'T_raw': T_raw, 'median_ms': med, 'all_ms': ms,
            'frames_per_s': float(lens.sum()) / (med / 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='768,16')
    ap.add_argument('--T', type=int, default=334)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-train', action='store_true')
    a = ap.parse_args()
    res = {'T': a.T, 'F': F0, 'H': H, 'layers': NL, 'stack': {}, 'recurrence': {}}
    for B in [int(b) for b in a.batches.split(',')]:
        reps = 2 if B >= 256 else 5
        res['stack'][str(B)] = stack_case(B, a.T, a.rounds, reps)
        res['recurrence'][str(B)] = recurrence_case(B, a.T, a.rounds, reps)
        print(json.dumps({'B': B, 'stack_median_ms': {k: round(v['median_ms'], 3) for k, v in res['stack'][str(B)].items()},
                          'recurrence': res['recurrence'][str(B)]}), flush=True)
    if not a.skip_train:
        res['train_step'] = train_step_case(16, 3 * a.T, a.rounds)
        print(json.dumps({'train_step': res['train_step']}), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
