#!/usr/bin/env python
"""Decode a log-prob archive over a decoding graph with a beam: the `decode-faster` stage of the
reference's scoring recipe (egs/wsj/ctc_kaldi_decode.sh:141-147) without Kaldi.

    python tools/decode_graph.py LOGPROBS.ark GRAPH.fst [--words words.txt] [--beam 16]
        [--acoustic-scale 1.0] [--batch 64] [--device cuda:0|cpu] [--out FILE]
        [--lattice-beam X --nbest N [--device-nbest] [--acwt-sweep LO:HI:STEP] [--post OUT.npz] [--mbr OUT]
         [--rescore-lm NEW.fst [--old-lm OLD.fst] [--rescore-beam X]] [--oracle REF --oracle-out OUT]]

LOGPROBS.ark: the float-matrix archive att_speech.ctc_forward writes (one [frames, classes] matrix
per utterance).  GRAPH.fst: an OpenFst binary (vector/standard, plain or gzip) or an AT&T text
file whose input label i > 0 reads class i - 1.  One line `uttid w1 w2 ...` per utterance, in
archive order: the integer transcript decode-faster writes to `ark,t:`, or symbols with --words
(what int2sym.pl makes of it).  An utterance without a path is written with no words.

With --lattice-beam the search keeps a lattice (att_speech.wfst_lattice.decode_lattice:
latgen-faster) and the output is its n-best list, `uttid-k cost w1 w2 ...` for k = 1..N, cheapest
first.  With --device-nbest the lists come from the lattices where the search left them
(DeviceLatticeBatch.nbest: one launch per batch; the same costs, ties at the last place may fall to
other sequences).  With --acwt-sweep as well, the one search (at --acoustic-scale) is re-ranked for every scale
LO, LO + STEP, ..., HI, which the recipe does with one decode-faster run per scale
(egs/wsj/ctc_kaldi_decode.sh:160-163): lines `scale uttid cost w1 w2 ...`, scale by scale.  The
lattices stay on the device and all scales are one call (att_speech.lattice_dp).  With --post the
frame-level class posteriors of every lattice (lattice-to-post) go to OUT.npz, one
[frames, classes] float32 matrix per utterance key, and nothing else is written.  With --mbr OUT
every lattice is decoded by minimum Bayes risk (DeviceLatticeBatch.mbr: lattice-mbr-decode, one launch
per batch): `uttid w1 w2 ...` lines go to OUT and `uttid word frame confidence` rows to OUT.conf, and
nothing else is written.  With --rescore-lm NEW.fst every lattice is first rescored with that back-off n-gram
LM where the search left it (DeviceLatticeBatch.rescore_lm: lattice-lmrescore under the back-off reading), after
--old-lm OLD.fst, the LM compiled into the graph, was taken out at scale -1; --rescore-beam prunes against the
new best.  The graph's output symbols are matched to the LM's input symbols by name when both files carry
tables, else by number.  Every lattice output above then reads the rescored lattices.  With --oracle REF
--oracle-out OUT (REF: `uttid w1 w2 ...` lines, symbols of --words or integers without it) every lattice, after
--rescore-lm when given, is searched for the path nearest to its reference in word edit distance
(DeviceLatticeBatch.oracle: lattice-oracle, one launch per batch): OUT gets `uttid errors sub ins del ref_len
depth w1 w2 ...` rows (errors -1: the lattice has no complete path; depth: emitting arcs per frame,
lattice-depth) and a last row `TOTAL errors ref_len rate mean_depth`, and nothing else is written."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'pytorch-asr_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np      # noqa: E402
import torch            # noqa: E402


def parse_sweep(text):
    """'LO:HI:STEP' -> the scales LO, LO + STEP, ... up to HI (inclusive, to 1e-9)"""
    lo, hi, step = (float(x) for x in text.split(':'))
    if not (step > 0 and hi >= lo):
        raise ValueError("--acwt-sweep wants LO:HI:STEP with STEP > 0 and HI >= LO")
    return [round(lo + i * step, 9) for i in range(int((hi - lo) / step + 1e-9) + 1)]


def _batches(utts, batch):
    """utts: [(key, [frames, classes] matrix)] -> (keys, lp [T,B,C] zero-padded, lens) per batch"""
    for i in range(0, len(utts), max(1, batch)):
        part = utts[i:i + max(1, batch)]
        lens = np.array([m.shape[0] for _, m in part], np.int32)
        if lens.min() < 1:
            raise ValueError("empty matrix in the archive")
        lp = np.zeros((int(lens.max()), len(part), part[0][1].shape[1]), np.float32)
        for j, (_, m) in enumerate(part):
            lp[:lens[j], j] = m
        yield [k for k, _ in part], lp, lens


def _lattices(graph, utts, device, batch, **kw):
    from att_speech import wfst_lattice
    for keys, lp, lens in _batches(utts, batch):
        lats, _ = wfst_lattice.decode_lattice(torch.from_numpy(lp).to(device), lens, graph, **kw)
        for k, lat in zip(keys, lats):
            yield k, lat


def make_rescorer(new_lm, old_lm=None, beam=None):
    """DeviceLatticeBatch -> DeviceLatticeBatch: old_lm out at scale -1 (when given), new_lm in"""
    from att_speech.lattice_lm import BackoffLm
    new = BackoffLm.from_fst(new_lm)
    old = BackoffLm.from_fst(old_lm) if old_lm is not None else None

    def rescore(batch):
        if old is not None:
            batch = batch.rescore_lm(old, scale=-1.0)
        return batch.rescore_lm(new, lattice_beam=beam)
    return rescore


def _tokens(table, words):
    return [table.find(int(w)) or str(w) for w in words] if table else [str(w) for w in words]


def write_nbest(graph, utts, path, beam, lattice_beam, nbest, acoustic_scale=1.0, allow_partial=True,
                device='cpu', batch=64, table=None, device_nbest=False, rescore=None):
    """`uttid-k cost w1 w2 ...`: the nbest cheapest distinct word sequences of every utterance;
    device_nbest: listed by DeviceLatticeBatch.nbest, a batch at a time"""
    kw = dict(beam=beam, lattice_beam=lattice_beam, acoustic_scale=acoustic_scale, allow_partial=allow_partial)

    def lists():
        if not device_nbest and rescore is None:
            for key, lat in _lattices(graph, utts, device, batch, **kw):
                yield key, lat.nbest(nbest)
            return
        from att_speech.lattice_dp import decode_lattice_device
        for keys, lp, lens in _batches(utts, batch):
            every, _ = decode_lattice_device(torch.from_numpy(lp).to(device), lens, graph, **kw)
            every = rescore(every) if rescore else every
            rows = every.nbest(nbest) if device_nbest else [lat.nbest(nbest) for lat in every.lattices()]
            for key, row in zip(keys, rows):
                yield key, row
    out = open(path, 'w') if path else sys.stdout
    try:
        for key, row in lists():
            for k, (words, cost) in enumerate(row):
                out.write(' '.join(['%s-%d' % (key, k + 1), '%.6f' % cost] + _tokens(table, words)) + '\n')
    finally:
        if path:
            out.close()


def write_sweep(graph, utts, path, beam, lattice_beam, scales, acoustic_scale=1.0, allow_partial=True,
                device='cpu', batch=64, table=None, rescore=None):
    """`scale uttid cost w1 w2 ...`: the best path of every utterance at every scale, from one search"""
    from att_speech.lattice_dp import decode_lattice_device
    rows = [[] for _ in scales]
    for keys, lp, lens in _batches(utts, batch):
        every, _ = decode_lattice_device(torch.from_numpy(lp).to(device), lens, graph, beam=beam,
                                         lattice_beam=lattice_beam, acoustic_scale=acoustic_scale,
                                         allow_partial=allow_partial)
        every = rescore(every) if rescore else every
        for row, best in zip(rows, every.best_paths(scales)):
            row.extend(zip(keys, best))
    out = open(path, 'w') if path else sys.stdout
    try:
        for scale, row in zip(scales, rows):
            for key, (words, cost, _, _) in row:
                out.write(' '.join(['%g' % scale, key, '%.6f' % cost] + _tokens(table, words)) + '\n')
    finally:
        if path:
            out.close()


def write_post(graph, utts, path, beam, lattice_beam, acoustic_scale=1.0, allow_partial=True, device='cpu',
               batch=64, table=None, rescore=None):
    """OUT.npz: per utterance key the [frames, classes] posteriors of its lattice at the search's scales"""
    from att_speech.lattice_dp import decode_lattice_device
    mats = {}
    for keys, lp, lens in _batches(utts, batch):
        every, _ = decode_lattice_device(torch.from_numpy(lp).to(device), lens, graph, beam=beam,
                                         lattice_beam=lattice_beam, acoustic_scale=acoustic_scale,
                                         allow_partial=allow_partial)
        every = rescore(every) if rescore else every
        post = every.posteriors().frame_posteriors().cpu().numpy()
        for j, key in enumerate(keys):
            mats[key] = post[:lens[j], j]
    np.savez(path, **mats)


def write_mbr(graph, utts, path, beam, lattice_beam, acoustic_scale=1.0, allow_partial=True, device='cpu',
              batch=64, table=None, rescore=None):
    """OUT: `uttid w1 w2 ...`, the minimum-Bayes-risk word sequence of every lattice at the search's
    scales; OUT.conf: `uttid word frame confidence`, a row per word"""
    from att_speech.lattice_dp import decode_lattice_device
    with open(path, 'w') as out, open(path + '.conf', 'w') as conf:
        for keys, lp, lens in _batches(utts, batch):
            every, _ = decode_lattice_device(torch.from_numpy(lp).to(device), lens, graph, beam=beam,
                                             lattice_beam=lattice_beam, acoustic_scale=acoustic_scale,
                                             allow_partial=allow_partial)
            every = rescore(every) if rescore else every
            for key, res in zip(keys, every.mbr()):
                tokens = _tokens(table, res.words)
                out.write(' '.join([key] + tokens) + '\n')
                for tok, frame, c in zip(tokens, res.frames, res.confidence):
                    conf.write('%s %s %d %.6f\n' % (key, tok, frame, c))


def read_references(path, table=None):
    """{uttid: [labels]} of `uttid w1 w2 ...` lines: symbols of `table`, or integers without one"""
    refs = {}
    with open(path) as f:
        for line in f:
            parts = line.split()
            if not parts:
                continue
            if table is not None:
                labels = [table.find(tok) for tok in parts[1:]]
                if any(l <= 0 for l in labels):
                    raise ValueError("%s: a word of %s is not in the symbol table" % (path, parts[0]))
            else:
                labels = [int(tok) for tok in parts[1:]]
            refs[parts[0]] = labels
    return refs


def write_oracle(graph, utts, path, references, beam, lattice_beam, acoustic_scale=1.0, allow_partial=True,
                 device='cpu', batch=64, table=None, rescore=None):
    """OUT: `uttid errors sub ins del ref_len depth w1 w2 ...`, the lattice oracle of every utterance against
    references[uttid], then `TOTAL errors ref_len rate mean_depth` over the utterances that have a path"""
    from att_speech.lattice_dp import decode_lattice_device
    from att_speech.wfst_lattice import oracle_error_rate
    missing = [k for k, _ in utts if k not in references]
    if missing:
        raise ValueError("no reference for %d utterances, the first: %s" % (len(missing), missing[0]))
    results, given, depths = [], [], []
    with open(path, 'w') as out:
        for keys, lp, lens in _batches(utts, batch):
            every, _ = decode_lattice_device(torch.from_numpy(lp).to(device), lens, graph, beam=beam,
                                             lattice_beam=lattice_beam, acoustic_scale=acoustic_scale,
                                             allow_partial=allow_partial)
            every = rescore(every) if rescore else every
            refs = [references[k] for k in keys]
            for key, ref, res, depth in zip(keys, refs, every.oracle(refs), every.depth()):
                out.write(' '.join([key] + [str(v) for v in (res.errors, res.substitutions, res.insertions,
                                                               res.deletions, len(ref))] + ['%.6f' % depth]
                                   + _tokens(table, res.words)) + '\n')
                results.append(res), given.append(ref), depths.append(depth)
        total = oracle_error_rate(results, given)
        out.write('TOTAL %d %d %.6f %.6f\n' % (total.errors, total.reference_words, total.rate,
                                               float(np.mean(depths)) if depths else 0.0))


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
    ap.add_argument('--lattice-beam', type=float, default=None, help='keep a lattice this wide; write its n-best')
    ap.add_argument('--nbest', type=int, default=1)
    ap.add_argument('--device-nbest', action='store_true',
                    help='list the n-best on the device, a batch per launch (DeviceLatticeBatch.nbest)')
    ap.add_argument('--acwt-sweep', default=None, help='LO:HI:STEP: the 1-best per acoustic scale from one search')
    ap.add_argument('--post', default=None, help='OUT.npz: frame-level class posteriors of every lattice')
    ap.add_argument('--mbr', default=None, help='OUT: minimum-Bayes-risk transcripts; OUT.conf: word confidences')
    ap.add_argument('--rescore-lm', default=None, help='NEW.fst: rescore every lattice with this back-off n-gram LM')
    ap.add_argument('--old-lm', default=None, help='OLD.fst: the LM compiled into the graph, taken out first')
    ap.add_argument('--rescore-beam', type=float, default=None, help='prune the rescored lattices against their best')
    ap.add_argument('--oracle', default=None, help='REF: `uttid w1 w2 ...` reference transcripts')
    ap.add_argument('--oracle-out', default=None, help='OUT: the lattice oracle of every utterance against REF')
    a = ap.parse_args(argv)
    if a.lattice_beam is None and (a.acwt_sweep or a.nbest != 1 or a.post or a.device_nbest or a.mbr or a.rescore_lm
                                   or a.oracle):
        ap.error('--nbest, --device-nbest, --acwt-sweep, --post, --mbr, --rescore-lm and --oracle need --lattice-beam')
    if (a.oracle is None) != (a.oracle_out is None):
        ap.error('--oracle REF and --oracle-out OUT go together')
    if a.rescore_lm is None and (a.old_lm or a.rescore_beam is not None):
        ap.error('--old-lm and --rescore-beam need --rescore-lm')
    from att_speech import wfst_decode
    from att_speech.ctc_forward import read_kaldi_float_matrices
    from att_speech.lm_fst import SymbolTable
    device = torch.device(a.device or ('cuda:0' if torch.cuda.is_available() else 'cpu'))
    graph = wfst_decode.DecodingGraph.read(a.graph)
    table = SymbolTable.read_text(a.words) if a.words else None
    mats = read_kaldi_float_matrices(a.logprobs)
    keys = list(mats)
    if a.lattice_beam is not None:
        utts = [(k, mats[k]) for k in keys]
        kw = dict(beam=a.beam, lattice_beam=a.lattice_beam, acoustic_scale=a.acoustic_scale,
                  allow_partial=not a.no_allow_partial, device=device, batch=a.batch, table=table)
        if a.rescore_lm:
            kw['rescore'] = make_rescorer(a.rescore_lm, a.old_lm, a.rescore_beam)
        if a.oracle:
            write_oracle(graph, utts, a.oracle_out, read_references(a.oracle, table), **kw)
        elif a.mbr:
            write_mbr(graph, utts, a.mbr, **kw)
        elif a.post:
            write_post(graph, utts, a.post, **kw)
        elif a.acwt_sweep:
            write_sweep(graph, utts, a.out, scales=parse_sweep(a.acwt_sweep), **kw)
        else:
            write_nbest(graph, utts, a.out, nbest=a.nbest, device_nbest=a.device_nbest, **kw)
        return
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
