"""CTC forced-alignment measurement (development tool; bench.py is the contract benchmark):
ctc_viterbi_align_batch on the benchmark's encoded shape (T' = 334 frames, 100 labels) with the
mono alphabet (C = 49) and the bi-character one (C = 2401, contextual blanks), at B = 1, 16, 64.
Per size, medians over the rounds of
  device_ms   the batch entry on device tensors, wall time with the host packing, the one launch
              of asr_ctc_align_f64 and the synchronisation,
  kernel_ms   the launch alone between two stream events (device inputs already packed),
  host_ms     the same call with ASR_ALIGN_NATIVE=0 (device log-probs copied to the host, the numpy
              band recurrence, results copied back),
  viterbi_reduction_ms   path_reduction(..., 'viterbi') on the numerator graphs of the same
              transcripts, graph matrices already built: the fp32 best-path SCORE alone, no
              traceback, for scale,
and whether device and host agree bit for bit.  --json writes the result as one JSON document."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'pytorch-asr_amd'))
sys.path.insert(0, ROOT)

from att_speech import _native, fst_utils             # noqa: E402
from att_speech.modules import ctc_losses              # noqa: E402

S = 49
SWITCH = 'ASR_ALIGN_NATIVE'


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    fn()
    torch.cuda.synchronize()
    return (time.time() - t0) * 1e3


def median_ms(fn, rounds):
    return round(statistics.median(timed(fn) for _ in range(rounds)), 4)


def kernel_ms(lp, act, padded, lls, order, flags, rounds):
    dev = lp.device
    act_d = torch.tensor(act, dtype=torch.int32, device=dev)
    lls_d = torch.tensor(lls, dtype=torch.int32, device=dev)
    lab_d = padded.to(device=dev, dtype=torch.int32)
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _native.ctc_align(lp, act_d, lab_d, lls_d, S, order, flags.get('allow_nonblank_selfloops', True),
                          flags.get('eval_repeats_in_context', False))
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return round(statistics.median(out), 4)


def measure(order, B, T, L, rounds, host_rounds, dev):
    g = torch.Generator().manual_seed(100 * order + B)
    C = S ** order
    lp = torch.log_softmax(torch.randn(T, B, C, generator=g), -1).to(dev)
    padded = torch.randint(1, S, (B, L), generator=g)
    act = [T - (3 * b) % 40 for b in range(B)]
    act.sort(reverse=True)                                  # path_reduction wants them sorted
    lls = [L - b % 7 for b in range(B)]
    flat = torch.cat([padded[b, :lls[b]] for b in range(B)])
    flags = {} if order == 1 else dict(allow_nonblank_selfloops=True, eval_repeats_in_context=True)

    def align():
        return ctc_losses.ctc_viterbi_align_batch(lp, flat, act, lls, num_symbols=S, context_order=order, **flags)

    os.environ[SWITCH] = '1'
    on = align()
    res = {'order': order, 'B': B, 'T': T, 'L': L, 'C': C,
           'device_ms': median_ms(align, rounds),
           'kernel_ms': kernel_ms(lp, act, padded, lls, order, flags, rounds)}
    os.environ[SWITCH] = '0'
    off = align()
    res['host_ms'] = median_ms(align, host_rounds)
    os.environ.pop(SWITCH, None)
    res['bit_equal'] = all(bool((x == y).all()) for x, y in zip(on, off))
    res['feasible'] = int(on.feasible.sum())
    res['host_over_device'] = round(res['host_ms'] / res['device_ms'], 2)

    gg_args = {} if order == 1 else dict(graph_build_args=dict(use_contextual_blanks=True))
    gg = fst_utils.CTCGraphGen(context_order=order, num_symbols=S, **gg_args)
    mats = gg.get_training_matrices_batch(padded, torch.tensor(lls))
    lens = torch.tensor(act, dtype=torch.int32)
    with torch.no_grad():
        score = fst_utils.path_reduction(lp, lens, mats, red_kind='viterbi')
        res['viterbi_reduction_ms'] = median_ms(
            lambda: fst_utils.path_reduction(lp, lens, mats, red_kind='viterbi'), rounds)
    # the same lattice: the fp32 best-path score is the fp64 cost up to fp32 rounding
    res['max_score_gap'] = float((score.double().cpu() + on.cost.cpu()).abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=334)
    ap.add_argument('--chars', type=int, default=100)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 16, 64])
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--host-rounds', type=int, default=3)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    result = {'frames': a.frames, 'chars': a.chars, 'rounds': a.rounds, 'host_rounds': a.host_rounds, 'sizes': []}
    for order in (1, 2):
        for B in a.batches:
            r = measure(order, B, a.frames, a.chars, a.rounds, a.host_rounds, dev)
            print(json.dumps(r), flush=True)
            result['sizes'].append(r)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(result, fh, indent=1)


if __name__ == '__main__':
    main()
