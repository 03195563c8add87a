#!/usr/bin/env python
"""Decode a log-prob archive over a decoding graph with a beam: the `decode-faster` stage of the
reference's scoring recipe (egs/wsj/ctc_kaldi_decode.sh:141-147) without Kaldi.

    python tools/decode_graph.py LOGPROBS.ark GRAPH.fst [--words words.txt] [--beam 16]
        [--acoustic-scale 1.0] [--batch 64] [--device cuda:0|cpu] [--out FILE]

LOGPROBS.ark: the float-matrix archive att_speech.ctc_forward writes (one [frames, classes] matrix
per utterance).  GRAPH.fst: an OpenFst binary (vector/standard, plain or gzip) or an AT&T text
file whose input label i > 0 reads class i - 1.  One line `uttid w1 w2 ...` per utterance, in
archive order: the integer transcript decode-faster writes to `ark,t:`, or symbols with --words
(what int2sym.pl makes of it).  An utterance without a path is written with no words."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'pytorch-asr_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np      # noqa: E402
import torch            # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('logprobs')
    ap.add_argument('graph')
    ap.add_argument('--words', default=None, help='symbol table text file (symbol id per line)')
    ap.add_argument('--beam', type=float, default=16.0)
    ap.add_argument('--acoustic-scale', type=float, default=1.0)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--device', default=None, help='default: cuda:0 when there is one, else cpu')
    ap.add_argument('--no-allow-partial', action='store_true')
    ap.add_argument('--out', default=None, help='default: standard output')
    a = ap.parse_args(argv)
    from att_speech import wfst_decode
    from att_speech.ctc_forward import read_kaldi_float_matrices
    from att_speech.lm_fst import SymbolTable
    device = torch.device(a.device or ('cuda:0' if torch.cuda.is_available() else 'cpu'))
    graph = wfst_decode.DecodingGraph.read(a.graph)
    table = SymbolTable.read_text(a.words) if a.words else None
    mats = read_kaldi_float_matrices(a.logprobs)
    keys = list(mats)
    out = open(a.out, 'w') if a.out else sys.stdout
    try:
        for i in range(0, len(keys), max(1, a.batch)):
            part = keys[i:i + max(1, a.batch)]
            lens = np.array([mats[k].shape[0] for k in part], np.int32)
            if lens.min() < 1:
                raise ValueError("empty matrix in the archive")
            C = mats[part[0]].shape[1]
            lp = np.zeros((int(lens.max()), len(part), C), np.float32)
            for j, k in enumerate(part):
                lp[:lens[j], j] = mats[k]
            res = wfst_decode.decode_graph(torch.from_numpy(lp).to(device), lens, graph, beam=a.beam,
                                           acoustic_scale=a.acoustic_scale,
                                           allow_partial=not a.no_allow_partial)
            for k, words in zip(part, res['words']):
                toks = [table.find(int(w)) or str(w) for w in words] if table else [str(w) for w in words]
                out.write(' '.join([k] + toks) + '\n')
    finally:
        if a.out:
            out.close()


if __name__ == '__main__':
    main()
