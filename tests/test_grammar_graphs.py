"""Grammar-FST decoding graphs (CTC token transducer composed with a character n-gram LM,
reference att_speech/fst_utils.py:546-640) built without OpenFst: the weighted language of the
builder's graphs against its definition, on the CPU."""
import itertools

import numpy as np
import pytest
import torch

from grammar_cases import (BIGRAM_LM, TRIGRAM_LM, WSJ_VOCAB, lm_log_score, lm_matrices, toy_lm,
                           torch_path_reduction)

RTOL = 1e-5           # tests/test_beam_lm.py's score tolerance


def _gen(kind, order=1, **kw):
    from att_speech import fst_utils as P
    lm, vocab = toy_lm(kind)
    return P.CTCGraphGen(context_order=order, num_symbols=len(vocab), grammar_fst=lm,
                         vocabulary=vocab, **kw), lm, vocab


def _collapse(hc, labeling):
    """Output string of a frame labeling by the HC rule, or None when HC has no such path: walked
    over the transducer's own arc tables (context order 2), written out for order 1 (drop
    repeats, then blanks)."""
    if hc.context_order == 1:
        out, prev = [], 0
        for l in labeling:
            if l != prev and l != 0:
                out.append(l)
            prev = l
        return out
    nxt, ol = hc.transition_tables()
    s, out = 0, []
    for l in labeling:
        if nxt[s, l] < 0:
            return None
        if ol[s, l] > 0:
            out.append(int(ol[s, l]))
        s = nxt[s, l]
    return out


def _enumerate_logz(hc, lm, glabel, lp):
    """log sum over ALL C^T frame labelings of exp(sum_t lp[t, l_t]) G(collapse(l)), fp64"""
    T, C = lp.shape
    mats = lm_matrices(lm, glabel)
    cache, terms = {}, []
    for labeling in itertools.product(range(C), repeat=T):
        y = _collapse(hc, labeling)
        if y is None:
            continue
        key = tuple(y)
        if key not in cache:
            cache[key] = lm_log_score(lm, glabel, y, mats)
        if np.isfinite(cache[key]):
            terms.append(sum(lp[t, l] for t, l in enumerate(labeling)) + cache[key])
    return np.logaddexp.reduce(np.array(terms, np.float64))


DEF_CASES = [('s3', 1, 5), ('s4', 1, 5), ('s3', 2, 4)]


@pytest.mark.parametrize('kind,order,T', DEF_CASES, ids=['%s_o%d' % c[:2] for c in DEF_CASES])
def test_denominator_is_the_sum_over_all_labelings(oracle_lib, kind, order, T):
    from att_speech import fst_utils as P
    gg, lm, vocab = _gen(kind, order)
    glabel = P.grammar_labels(lm, vocab, len(vocab))
    C = len(vocab) ** order
    rng = np.random.default_rng(T * 10 + order)
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, 2, C))), -1).numpy()
    lens = np.array([T, T - 2], np.int32)
    want = np.array([_enumerate_logz(gg.decoding_fst, lm, glabel, lp[:n, b]) for b, n in enumerate(lens)])
    tagged = gg.get_decoding_matrices()
    assert len(tagged) == 8 and tagged[0].shape[0] == 1 and tagged.shared is not None
    assert tagged[:4].shared is tagged.shared
    # the unreachable LM state and the dead end are trimmed away; the start state is 0
    pairs = gg.grammar.state_pairs
    assert tuple(pairs[0]) == (0, lm.start())
    dead = {'s3': {4, 5}, 's4': {5}}[kind]
    assert not dead & set(pairs[:, 1].tolist())
    mats = [m.numpy() for m in tagged]
    f64 = oracle_lib.path_logsumexp_f64(lp.astype(np.float32), lens, mats)
    np.testing.assert_allclose(f64['logZ'], want, rtol=RTOL)
    f32 = oracle_lib.path_logsumexp(lp.astype(np.float32), lens, mats)
    np.testing.assert_allclose(f32['logZ'], want, rtol=RTOL)
    z = torch_path_reduction(torch.from_numpy(lp), lens, tagged)
    np.testing.assert_allclose(z.numpy(), want, rtol=RTOL)
    # the max-plus scan over the same graph bounds the path sum from below
    v = torch_path_reduction(torch.from_numpy(lp), lens, tagged, red_kind='viterbi')
    assert (v.numpy() <= want + 1e-9).all()


@pytest.mark.parametrize('kind', ['s3', 's4'])
def test_numerator_is_the_chain_times_the_grammar_score(oracle_lib, kind):
    from att_speech import fst_utils as P
    gg, lm, vocab = _gen(kind)
    plain = P.CTCGraphGen(context_order=1, num_symbols=len(vocab))
    glabel = P.grammar_labels(lm, vocab, len(vocab))
    S = len(vocab)
    # accepted transcripts, an empty one, and one G rejects ('a b b': the dead end / 'a' + ' ')
    labels = {'s3': [[2, 1, 1], [1, 1, 0], [0, 0, 0], [1, 2, 2]],
              's4': [[2, 3, 1], [3, 3, 0], [0, 0, 0], [2, 1, 0]]}[kind]
    llens = np.array([3, 2, 0, {'s3': 3, 's4': 2}[kind]])
    rng = np.random.default_rng(3)
    T = 7
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, 4, S))), -1).numpy().astype(np.float32)
    lens = np.array([7, 7, 6, 5], np.int32)
    logg = np.array([lm_log_score(lm, glabel, row[:n]) for row, n in zip(labels, llens)])
    assert np.isfinite(logg[:3]).all() and not np.isfinite(logg[3])
    np.testing.assert_allclose(gg._grammar_scores(np.array(labels), llens)[:3], logg[:3], rtol=1e-12)
    chain = oracle_lib.path_logsumexp_f64(lp, lens, [m.numpy() for m in plain.get_training_matrices_batch(
        np.array(labels), llens)])['logZ']
    mats = gg.get_training_matrices_batch(np.array(labels), llens)
    assert len(mats) == 8
    got = oracle_lib.path_logsumexp_f64(lp, lens, [m.numpy() for m in mats])['logZ']
    np.testing.assert_allclose(got[:3], (chain + logg)[:3], rtol=RTOL)
    z = torch_path_reduction(torch.from_numpy(lp).double(), lens, mats)
    np.testing.assert_allclose(z.numpy()[:3], (chain + logg)[:3], rtol=RTOL)
    assert got[3] < -1e19 and z[3] < -1e19             # nc_weight: G does not accept it


def test_shipped_bigram_lm_loads_and_composes(oracle_lib):
    from att_speech import fst_utils as P
    from att_speech.lm_fst import LmFst
    lm = LmFst.read(BIGRAM_LM)
    assert lm.num_states() == 52 and len(lm.src) == 1057 and int((lm.ilabel == 0).sum()) == 80
    assert int(np.isfinite(lm.final_w).sum()) == 1
    vocab = P._read_vocabulary(WSJ_VOCAB)
    assert len(vocab) == 49 and vocab[2] == ' '
    glabel = P.grammar_labels(lm, vocab, 49)
    assert sorted(set(glabel[glabel > 0].tolist())) == list(range(1, 49))   # all 48 symbols
    assert glabel[lm.input_symbols().find('<spc>')] == 2
    assert glabel[lm.input_symbols().find('<s>')] == -1

    gg = P.CTCGraphGen(context_order=1, num_symbols=49, grammar_fst=BIGRAM_LM, vocabulary=WSJ_VOCAB)
    rng = np.random.default_rng(5)
    T, B, S = 6, 2, 49
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, B, S))), -1).numpy()
    # dense fp64 recursion over the UNTRIMMED (HC state x G state) product, probability domain;
    # the epsilon closure is a matrix inverse, applied at the start and after every move of G
    K, by, fin = lm_matrices(lm, glabel)
    want = []
    for b in range(B):
        A = np.zeros((S, lm.num_states()))
        A[0, lm.start()] = 1.0
        A = A @ K
        for t in range(T):
            p = np.exp(lp[t, b])
            tot = A.sum(0)
            new = np.zeros_like(A)
            new[0] = tot * p[0]                                  # into blank: no output
            for d in range(1, S):
                new[d] = A[d] * p[d]                             # repeat: no output
                if d in by:
                    new[d] += ((tot - A[d]) @ by[d] @ K) * p[d]  # d is emitted: G moves
            A = new
        want.append(np.log((A @ fin).sum()))
    tagged = gg.get_decoding_matrices()
    lens = np.array([T, T], np.int32)
    got = oracle_lib.path_logsumexp_f64(lp.astype(np.float32), lens, [m.numpy() for m in tagged])
    np.testing.assert_allclose(got['logZ'], want, rtol=RTOL)
    assert 100 <= gg.grammar.num_states <= 400


def test_trigram_lm_fixture_reads():
    from att_speech.lm_fst import LmFst
    lm = LmFst.read(open(TRIGRAM_LM, 'rb'))
    assert lm.num_states() == 981 and len(lm.src) == 9743 and int((lm.ilabel == 0).sum()) == 1253


def test_failure_modes():
    from att_speech import fst_utils as P
    lm, vocab = toy_lm('s3')
    with pytest.raises(ValueError, match="'b'"):
        P.CTCGraphGen(context_order=1, num_symbols=3, grammar_fst=lm, vocabulary=['<pad>', 'a', 'c'])
    with pytest.raises(NotImplementedError, match='ngram_to_class_file'):
        P.CTCGraphGen(context_order=1, num_symbols=3, ngram_to_class_file='classes.txt')
    # without a grammar nothing changes: the closed-form graph, tagged for the grouped kernels
    tagged = P.CTCGraphGen(context_order=1, num_symbols=3).get_decoding_matrices()
    assert tagged.grouped is not None and tagged.shared is None
