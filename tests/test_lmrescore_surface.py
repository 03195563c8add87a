"""The surface around DeviceLatticeBatch.rescore_lm on the CPU: FSTDecoder(decode_rescore_lm=...) and
tools/decode_graph.py --rescore-lm, against the calls they stand for."""
import os
import sys

import numpy as np
import pytest
import torch

import lm_rescore_cases as RC
import nbest_cases as NC

from att_speech.lattice_dp import decode_lattice_device
from att_speech.lattice_lm import lm_label_map
from att_speech.lm_fst import LmFst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIGRAM_LM = NC.BIGRAM_LM.replace('_bg_', '_tg_')


def test_fst_decoder_rescores_with_the_shipped_trigram():
    from att_speech.modules.decoders.advanced_decoder import FSTDecoder
    vocab = [l.rstrip('\n') for l in open(NC.WSJ_VOCAB)][:49]
    B, T, D = 2, 16, 24
    gg = dict(class_name='CTCGraphGen', context_order=1, grammar_fst=NC.BIGRAM_LM, vocabulary=NC.WSJ_VOCAB)
    kw = dict(normalize_by_dim=None, denominator_red='logsumexp', vocabulary=vocab, decode_beam=16.0,
              decode_lattice_beam=4.0, decode_nbest=5)
    sample = {'features': torch.zeros(B, T, D)}
    torch.manual_seed(0)
    plain = FSTDecoder(sample, 49, dict(gg), **kw)
    assert plain.decode_rescore_lm is None
    new = FSTDecoder(sample, 49, dict(gg), decode_rescore_lm=TRIGRAM_LM, decode_rescore_old_lm=NC.BIGRAM_LM,
                     decode_rescore_beam=3.0, decode_confidence=True, decode_mbr=True, **kw)
    new.load_state_dict(plain.state_dict())
    enc = torch.randn(T, B, D) * 3
    elens = torch.tensor([16, 11], dtype=torch.int32)
    with torch.no_grad():
        got = new.decode(enc, elens)
        logits = plain.logits(enc, elens)
    g = NC.bigram_graph()
    tg, bg = LmFst.read(TRIGRAM_LM), LmFst.read(NC.BIGRAM_LM)
    batch, _ = decode_lattice_device(logits.float(), elens, g, beam=16.0, lattice_beam=4.0)
    want = batch.rescore_lm(bg, label_map=lm_label_map(bg, NC.WSJ_VOCAB, 49), scale=-1.0) \
        .rescore_lm(tg, label_map=lm_label_map(tg, NC.WSJ_VOCAB, 49), lattice_beam=3.0)
    assert got['decoded'] == [w for w, _, _, _ in want.best_paths()[0]]
    assert got['nbest'] == [lat.nbest(5) for lat in want.lattices()]
    assert [len(c) for c in got['word_confidence']] == [len(w) for w in got['decoded']]
    assert [r[0] for r in got['mbr']] == [r.words for r in want.mbr()]
    for args in (dict(decode_rescore_old_lm=NC.BIGRAM_LM), dict(decode_rescore_beam=2.0)):
        with pytest.raises(ValueError, match='decode_rescore_lm'):
            FSTDecoder(sample, 49, dict(gg), **dict(kw, **args))
    with pytest.raises(ValueError, match='decode_lattice_beam'):
        FSTDecoder(sample, 49, dict(gg), normalize_by_dim=None, denominator_red='logsumexp', vocabulary=vocab,
                   decode_beam=16.0, decode_rescore_lm=TRIGRAM_LM)


def test_tool_rescore_options(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import decode_graph as tool
    finally:
        sys.path.pop(0)
    g, lats, lm = RC.brute_case(0)
    seed, N, T, lens, beam, lb, fs = RC.BRUTE[0]
    rng = np.random.default_rng(seed)
    import wfst_cases as WC
    WC.random_graph(rng, N, 3, final_share=fs, n_words=RC.N_WORDS)              # the draws of brute_case, in its order
    lp = WC.grid_scores(rng, T, len(lens), 3, lens, low=-4.0)
    utts = [('utt%d' % b, lp[:n, b]) for b, n in enumerate(lens)]
    old = RC.random_backoff_lm(np.random.default_rng(9), no_unigram=())
    rescore = tool.make_rescorer(lm, old, beam=2.0)
    out = tmp_path / 'nbest.txt'
    kw = dict(beam=beam, lattice_beam=lb, batch=3, rescore=rescore)
    tool.write_nbest(g, utts, str(out), nbest=3, **kw)
    batch, _ = decode_lattice_device(torch.from_numpy(np.nan_to_num(lp)), lens, g, beam=beam, lattice_beam=lb)
    want = batch.rescore_lm(old, scale=-1.0).rescore_lm(lm, lattice_beam=2.0)
    lines = []
    for b, lat in enumerate(want.lattices()):
        for k, (words, cost) in enumerate(lat.nbest(3)):
            lines.append(' '.join(['utt%d-%d' % (b, k + 1), '%.6f' % cost] + [str(w) for w in words]))
    assert out.read_text().splitlines() == lines and lines
    dev = tmp_path / 'nbest_dev.txt'
    tool.write_nbest(g, utts, str(dev), nbest=3, device_nbest=True, **kw)
    assert [l.split()[1] for l in dev.read_text().splitlines()] == [l.split()[1] for l in lines]
    sweep = tmp_path / 'sweep.txt'
    tool.write_sweep(g, utts, str(sweep), scales=[0.5, 1.0], **kw)
    rows = []
    for scale, best in zip((0.5, 1.0), want.best_paths([0.5, 1.0])):
        for b, (words, cost, _, _) in enumerate(best):
            rows.append(' '.join(['%g' % scale, 'utt%d' % b, '%.6f' % cost] + [str(w) for w in words]))
    assert sweep.read_text().splitlines() == rows
    tool.write_mbr(g, utts, str(tmp_path / 'mbr.txt'), **kw)
    assert (tmp_path / 'mbr.txt').read_text().splitlines() == \
        [' '.join(['utt%d' % b] + [str(w) for w in r.words]) for b, r in enumerate(want.mbr())]
    with pytest.raises(SystemExit):
        tool.main(['a.ark', 'g.fst', '--lattice-beam', '2', '--old-lm', 'x.fst'])
    with pytest.raises(SystemExit):
        tool.main(['a.ark', 'g.fst', '--rescore-lm', 'x.fst'])
