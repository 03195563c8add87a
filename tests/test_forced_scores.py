"""AttentionDecoderTCN.score_sentences (the teacher-forced rescoring pass of the reference's
egs/wsj/local/lattice_search scripts) without a GPU: the host path against the golden record made
from the reference's own decoder and LM functions, the argument checks, the prefix trie, the
sentence walk over a decode graph, and the argument checks of asr_forced_level_f32."""
import ctypes

import numpy as np
import pytest
import torch

import forced_cases as fc
from conftest import golden

EOS = 7


# ---------------------------------------------------------------- 1. host path vs the reference

@pytest.mark.parametrize('tag', ['plain', 'ff'])
def test_host_path_reproduces_the_reference(tag):
    dec = fc.golden_decoder(tag)
    enc, lens, sentences, want = fc.golden_inputs(tag)
    by_log = dec.score_sentences(enc, lens, sentences)
    by_count = dec.score_sentences(enc, lens, sentences, coverage='count')
    assert len(by_log) == len(by_count) == 3
    for u in range(3):
        for res in (by_log[u], by_count[u]):
            assert all(res[k].dtype == np.float64 and res[k].shape == (len(sentences[u]),)
                       for k in ('acoustic', 'coverage', 'lm', 'loss'))
            np.testing.assert_array_equal(res['covered'], want['covered'][u])
            np.testing.assert_allclose(res['lm'], want['lm'][u], rtol=1e-9)
            np.testing.assert_allclose(res['acoustic'], want['acoustic'][u], rtol=1e-5, atol=1e-5)
        # the reference's coverage terms are fp32 values
        np.testing.assert_allclose(by_log[u]['coverage'], want['cov_log'][u], rtol=1e-6)
        np.testing.assert_allclose(by_count[u]['coverage'], want['cov_count'][u], rtol=1e-6)
        np.testing.assert_allclose(by_log[u]['loss'], want['loss_log'][u], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(by_count[u]['loss'], want['loss_count'][u], rtol=1e-5, atol=1e-5)
        # duplicates come back twice, in the given order
        dup = [i for i, s in enumerate(sentences[u]) if sentences[u].count(s) > 1]
        assert len(dup) >= 2
        for i in dup:
            j = sentences[u].index(sentences[u][i])
            assert all(by_log[u][k][i] == by_log[u][k][j] for k in ('acoustic', 'lm', 'loss'))


def test_the_golden_sentences_hold_the_cases_the_trie_must_handle():
    for tag in ('plain', 'ff'):
        _, _, sentences, _ = fc.golden_inputs(tag)
        for sents in sentences:
            tup = [tuple(s) for s in sents]
            assert len(set(tup)) < len(tup)                                  # a duplicate
            assert any(len(s) == 1 for s in tup)                             # one label
            assert any(a != b and b[:len(a)] == a for a in tup for b in tup)  # a proper prefix
            assert any(a != b and len(a) == len(b) and a[:-1] == b[:-1] for a in tup for b in tup)


def test_model_without_lm_scores_zero_lm():
    dec = fc.golden_decoder('plain')
    enc, lens, sentences, want = fc.golden_inputs('plain')
    dec.lm, dec.alphabet_mapping = None, None
    res = dec.score_sentences(enc[:, :1], lens[:1], sentences[:1])
    assert len(res) == 1 and (res[0]['lm'] == 0.0).all()
    np.testing.assert_allclose(res[0]['acoustic'], want['acoustic'][0], rtol=1e-5, atol=1e-5)


def test_argument_errors():
    dec = fc.golden_decoder('plain')
    enc, lens, sentences, _ = fc.golden_inputs('plain')
    ok = [[[1, 2]], [[3]], [[4, 5, 6]]]
    dec.score_sentences(enc, lens, ok)
    for bad in ([[[1, 2]], [[3]]],                       # one list per utterance
                [[[1, 2]], [[]], [[4]]],                 # an empty sentence
                [[[1, EOS]], [[3]], [[4]]],              # EOS is appended here
                [[[1, 8]], [[3]], [[4]]],
                [[[1, -1]], [[3]], [[4]]],
                [[[1, 2.0]], [[3]], [[4]]],
                [[[1, True]], [[3]], [[4]]]):
        with pytest.raises(ValueError):
            dec.score_sentences(enc, lens, bad)
    with pytest.raises(ValueError):
        dec.score_sentences(enc, lens, ok, coverage='fraction')
    dec.train()
    with pytest.raises(RuntimeError):
        dec.score_sentences(enc, lens, ok)
    dec.eval()
    # an utterance may come without sentences
    res = dec.score_sentences(enc, lens, [[[1, 2]], [], [[4]]])
    assert res[1]['acoustic'].shape == (0,) and res[0]['loss'].shape == (1,)
    x = enc.clone().requires_grad_()
    assert isinstance(dec.score_sentences(x, lens, ok)[0]['loss'], np.ndarray)   # no_grad inside


# ---------------------------------------------------------------- 2. the trie

def test_trie_crafted_sets():
    # one sentence
    t = fc.check_trie([[3, 1, 4]], EOS)
    assert [lv['n_units'] for lv in t['levels']] == [1, 1, 1, 1]
    # duplicates share one EOS edge
    t = fc.check_trie([[2, 2], [5], [2, 2], [2, 2]], EOS)
    assert t['count'] == 2 and len(set(t['inverse'][[0, 2, 3]].tolist())) == 1
    assert sum(int((lv['edge_dst'] < 0).sum()) for lv in t['levels']) == 2
    # a sentence that is a prefix of another: its last unit has an EOS edge and a label edge
    t = fc.check_trie([[1, 2, 3], [1, 2], [1, 2, 4]], EOS)
    lv = t['levels'][2]
    assert lv['n_units'] == 1 and sorted(lv['edge_label'].tolist()) == [3, 4, EOS]
    assert sorted((lv['edge_dst'] < 0).tolist()) == [False, False, True]
    # sentences that differ only in the last label share every unit but the last
    t = fc.check_trie([[6, 0, 1], [6, 0, 2]], EOS)
    assert [lv['n_units'] for lv in t['levels']] == [1, 1, 1, 2]
    # label 0 and the largest label, different lengths, nothing shared
    t = fc.check_trie([[0], [6, 6, 6, 6, 6], [0, 0]], EOS)
    assert [lv['n_units'] for lv in t['levels']] == [1, 2, 2, 1, 1, 1]
    # no sentences
    from att_speech.modules.beam_search import sentence_trie
    assert sentence_trie([], EOS)['levels'] == []


def test_trie_random_sets():
    rng = np.random.default_rng(5)
    for _ in range(200):
        nsym = int(rng.integers(1, 5))                        # few symbols: many shared prefixes
        sents = [[int(c) for c in rng.integers(0, nsym, size=int(rng.integers(1, 7)))]
                 for _ in range(int(rng.integers(1, 13)))]
        fc.check_trie(sents, EOS)


def test_batch_levels_pad_with_dead_slots():
    from att_speech.modules.beam_search import batch_trie_levels, sentence_trie
    sets = [[[1, 2, 3], [1, 2], [1, 4, 4, 4]], [[5]], [], [[2], [3], [4, 4]]]
    tries = [sentence_trie(s, EOS) for s in sets]
    levels, offsets = batch_trie_levels(tries)
    assert offsets.tolist() == [0, 3, 4, 4, 7] and len(levels) == 5
    B = len(sets)
    seen = set()
    for l, lv in enumerate(levels):
        W = lv['width']
        assert W == max([t['levels'][l]['n_units'] for t in tries if l < len(t['levels'])] + [1])
        n_edges = np.diff(lv['edge_ptr'])
        for u, t in enumerate(tries):
            k = t['levels'][l]['n_units'] if l < len(t['levels']) else 0
            sl = slice(u * W, (u + 1) * W)
            # live slots carry the utterance's own edges; dead slots have none and continue slot 0
            assert (n_edges[sl][:k] >= 1).all() and (n_edges[sl][k:] == 0).all()
            prev_w = levels[l - 1]['width'] if l else 1
            assert (lv['parent'][sl][k:] == u * prev_w).all()
            assert (lv['parent'][sl] // prev_w == u).all()
        assert (lv['edge_src'] == np.repeat(np.arange(B * W), n_edges)).all()
        dst = lv['edge_dst']
        nxt = levels[l + 1]['width'] if l + 1 < len(levels) else 1
        # an edge stays inside its utterance; sentence ids are global and unique
        assert (dst[dst >= 0] // nxt == lv['edge_src'][dst >= 0] // W).all()
        for s, src in zip(-1 - dst[dst < 0], lv['edge_src'][dst < 0]):
            assert offsets[src // W] <= s < offsets[src // W + 1] and s not in seen
            seen.add(int(s))
    assert seen == set(range(7))


def test_trie_of_a_lattice_sized_set_is_array_work():
    """5000 sentences of 100 labels: the construction is one sort and array passes per level"""
    import time
    from att_speech.modules.beam_search import sentence_trie
    rng = np.random.default_rng(0)
    base = rng.integers(0, 49, size=100)
    sents = np.repeat(base[None], 5000, 0)
    for col in rng.integers(0, 100, size=12):
        sents[:, col] = np.where(rng.random(5000) < 0.5, sents[:, col], rng.integers(0, 49, 5000))
    lists = sents.tolist()
    t0 = time.perf_counter()
    trie = sentence_trie(lists, 49)
    took = time.perf_counter() - t0
    units = sum(lv['n_units'] for lv in trie['levels'])
    assert len(trie['levels']) == 101 and units < 5000 * 101
    assert trie['levels'][-1]['n_units'] == trie['count'] == len({tuple(s) for s in lists})
    assert took < 5.0, took          # a Python loop over the 500000 tokens per level would not be


# ---------------------------------------------------------------- 3. sentences of a graph

def _graph(nodes, edges):
    """nodes: (name, label, finished); hashes are the names' hashes"""
    V = [(hash(n), lab, 0.0, None, fin) for n, lab, fin in nodes]
    return {'V': V, 'E': [(hash(a), hash(b), kind) for a, b, kind in edges]}


def test_graph_sentences_hand_built():
    from att_speech.modules.beam_search import graph_sentences
    #            root
    #        a(3)    b(4, finished)
    #     c(5, fin)    \-- merged --> c
    #     d(6)  e(2, fin)            (d: an unfinished leaf)
    g = _graph([('root', '<sos>', False), ('a', 3, False), ('b', 4, True), ('c', 5, True),
                ('d', 6, False), ('e', 2, True)],
               [('root', 'a', 'normal'), ('root', 'b', 'normal'), ('a', 'c', 'normal'),
                ('b', 'c', 'merged'), ('c', 'd', 'normal'), ('c', 'e', 'normal')])
    want = [[3, 5], [3, 5, 2], [4], [4, 5], [4, 5, 2]]
    assert graph_sentences(g) == want
    assert graph_sentences(g, limit=3) == want[:3]
    assert graph_sentences(g, limit=1) == want[:1] and graph_sentences(g, limit=0) == []
    assert graph_sentences(g, limit=99) == want
    # an edge back to the current path is not followed
    g['E'].append((hash('e'), hash('a'), 'merged'))
    assert graph_sentences(g) == want
    assert graph_sentences({'V': [(0, '<sos>', 0.0, 0., False)], 'E': []}) == []


def _recursive(graph, limit):
    """the script's dfs over label ids; stops a path at a node it already holds"""
    V = {v[0]: v for v in graph['V']}
    E = {v[0]: [] for v in graph['V']}
    for a, b, _ in graph['E']:
        E[a].append(b)
    out = []

    def walk(node, cur, held):
        if V[node][4]:
            out.append(cur)
        for nxt in E[node]:
            if nxt not in held:
                walk(nxt, cur + [int(V[nxt][1])], held | {nxt})
    walk(graph['V'][0][0], [], {graph['V'][0][0]})
    return out if limit is None else out[:limit]


def test_graph_sentences_recorded_graph():
    from att_speech.modules.beam_search import graph_sentences
    g = golden('beam_lm.npz')
    V = [(int(h), '<sos>' if lab < 0 else int(lab), float(sc), None, bool(fin))
         for (h, lab, fin), sc in zip(g['gs_V'].tolist(), g['gs_V_scores'].tolist())]
    graph = {'V': V, 'E': [(int(a), int(b), 'merged' if m else 'normal') for a, b, m in g['gs_E'].tolist()]}
    want = _recursive(graph, None)
    got = graph_sentences(graph)
    assert len(want) >= 5 and got == want
    assert all(len(s) >= 1 and all(0 <= c < 6 for c in s) for s in got)
    for limit in (1, 4, len(want), len(want) + 3):
        assert graph_sentences(graph, limit=limit) == want[:limit]


# ---------------------------------------------------------------- 4. the entry point

def test_forced_level_argument_checks_need_no_gpu():
    from att_speech import _native
    L = _native.lib()
    buf = [ctypes.c_void_p(4096 * (i + 1)) for i in range(13)]       # never dereferenced

    def call(ptrs=None, B=2, width=3, C=7, T=40, rows=2, n_edges=5, n_out=6, n_sent=4):
        p = list(buf) if ptrs is None else ptrs
        return L.asr_forced_level_f32(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9],
                                      p[10], B, width, C, T, rows, n_edges, n_out, n_sent, 0.1,
                                      p[11], p[12], None)
    for i in range(13):                                               # every buffer is needed
        p = list(buf)
        p[i] = None
        assert call(p) == _native.ASR_EINVAL, i
    for a, b in ((2, 3), (1, 3), (8, 9), (11, 9), (11, 8)):           # aliased in / out buffers
        p = list(buf)
        p[b] = p[a]
        assert call(p) == _native.ASR_EINVAL, (a, b)
    for kw in (dict(B=0), dict(width=0), dict(T=0), dict(C=0), dict(rows=0), dict(n_edges=-1),
               dict(n_out=-1), dict(n_sent=-1)):
        assert call(**kw) == _native.ASR_EINVAL, kw
    for kw in (dict(C=1), dict(C=2049), dict(T=8161)):
        assert call(**kw) == _native.ASR_EUNSUPPORTED, kw
    # the limits hold before the pointers are looked at, as for the neighbouring entries
    assert call([None] * 13, C=2049) == _native.ASR_EUNSUPPORTED
