"""The shared-graph lattice kernels (csrc/lattice_shared.hip: asr_lattice_shared_*) on HC o G
decoding graphs, against the generic kernel on the padded matrices of the same graph and the CPU
oracle.  Bounds: those tests/test_lattice_gpu.py applies to the grouped denominator kernel."""
import copy
import os
import warnings

import numpy as np
import pytest
import torch

from grammar_cases import BIGRAM_LM, TRIGRAM_LM, WSJ_VOCAB, toy_lm, torch_path_reduction
from test_lattice_gpu import ATOL_GRAD, RTOL_LOSS, assert_posteriors, dev

pytestmark = pytest.mark.gpu

_GENS = {}


def graph_gen(name):
    """one generator (and its composed graph) per LM for the whole module"""
    from att_speech import fst_utils as P
    if name not in _GENS:
        if name == 'toy':
            lm, vocab = toy_lm('s4')
            _GENS[name] = P.CTCGraphGen(context_order=1, num_symbols=4, grammar_fst=lm, vocabulary=vocab)
        else:
            path = {'bigram': BIGRAM_LM, 'trigram': TRIGRAM_LM}[name]
            _GENS[name] = P.CTCGraphGen(context_order=1, num_symbols=49, grammar_fst=path,
                                        vocabulary=WSJ_VOCAB)
    return _GENS[name]


CASES = [('toy', 5, [5, 4, 2]), ('bigram', 12, [12, 9, 1, 0]), ('trigram', 8, [8, 5])]


def _inputs(name, T, lens):
    gg = graph_gen(name)
    rng = np.random.default_rng(len(name) + T)
    x = rng.standard_normal((T, len(lens), gg.num_classes)).astype(np.float32) * 2
    lp = x - x.max(-1, keepdims=True)               # what get_fst_loss feeds (:479-484)
    return gg, lp, np.array(lens, np.int32)


@pytest.mark.parametrize('name,T,lens', CASES, ids=[c[0] for c in CASES])
def test_shared_kernels_match_generic_kernel_and_oracle(oracle_lib, name, T, lens):
    from att_speech import _native, fst_utils as P
    gg, lp, lens = _inputs(name, T, lens)
    tagged = gg.get_decoding_matrices()
    mats = [m.numpy() for m in tagged]
    N = mats[0].shape[1]
    assert {'toy': N < 64, 'bigram': 100 <= N <= 400, 'trigram': 1500 <= N <= 3000}[name]
    d = dev()
    sg = _native.SharedGraph(tagged.shared, d)
    assert sg.supported(gg.num_classes)
    if name == 'trigram':                           # both reductions: lane groups and whole waves
        assert 0 < sg.n_light_in < sg.N
    lpt, tl = torch.from_numpy(lp).to(d), torch.from_numpy(lens).to(d)
    want = oracle_lib.path_logsumexp(lp, lens, mats)
    generic = _native.Graph(list(tagged), d)
    gz, ggrad, gzb = _native.lattice_fwbw(lpt, tl, generic, -1e20, want_bwd_total=True)
    logZ, grad, zb = _native.shared_fwbw(lpt, tl, sg, -1e20, want_bwd_total=True)
    torch.cuda.synchronize()
    logZ, grad, zb = logZ.cpu().numpy(), grad.cpu().numpy(), zb.cpu().numpy()
    assert np.isfinite(grad).all() and np.isfinite(logZ).all()
    for ref_z, ref_zb in ((want['logZ'], want['logZ_bwd']), (gz.cpu().numpy(), gzb.cpu().numpy())):
        np.testing.assert_allclose(logZ, ref_z, rtol=RTOL_LOSS, atol=1e-5)
        np.testing.assert_allclose(zb, ref_zb, rtol=RTOL_LOSS, atol=1e-4)
    assert_posteriors(grad, want['grad'], lp, lens, mats, oracle_lib)
    assert_posteriors(grad, ggrad.cpu().numpy(), lp, lens, mats, oracle_lib)
    mask = np.arange(T)[:, None] >= lens[None, :]
    assert (grad[mask] == 0).all()                  # rows past the utterance end (:448)

    # the occupancies of -logZ, and added onto a buffer that holds something already
    base = torch.from_numpy(np.random.default_rng(1).standard_normal(lp.shape).astype(np.float32)).to(d)
    z2, neg, _ = _native.shared_fwbw(lpt, tl, sg, -1e20, grad_sign=-1.0)
    # (the row sums are LDS atomics: their order, hence the last bits, differ from launch to launch)
    np.testing.assert_allclose(neg.cpu().numpy(), -grad, rtol=0, atol=ATOL_GRAD)
    assert (neg.cpu().numpy() <= 0).all()
    z3, acc, _ = _native.shared_fwbw(lpt, tl, sg, -1e20, add_to=base.clone())
    np.testing.assert_array_equal(z3.cpu().numpy(), logZ)
    np.testing.assert_allclose(acc.cpu().numpy(), base.cpu().numpy() + grad, rtol=0, atol=ATOL_GRAD)
    assert (acc.cpu().numpy()[mask] == base.cpu().numpy()[mask]).all()

    # alpha-only scan, logsumexp and viterbi
    s, _ = _native.shared_forward(lpt, tl, sg, -1e20)
    np.testing.assert_allclose(s.cpu().numpy(), want['logZ'], rtol=RTOL_LOSS, atol=1e-5)
    vs, vil = oracle_lib.path_forward(lp, lens, mats, viterbi=True)
    gv, gbest = _native.lattice_forward(lpt, tl, generic, -1e20, viterbi=True, want_path=True)
    v, best = _native.shared_forward(lpt, tl, sg, -1e20, viterbi=True, want_path=True)
    v, best = v.cpu().numpy(), best.cpu().numpy()
    np.testing.assert_allclose(v, vs, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(v, gv.cpu().numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_array_equal(best, gbest.cpu().numpy())     # every frame, every utterance
    np.testing.assert_array_equal(best, vil)
    assert (best[mask] == 0).all()
    # the labels really are a path with that score (a tie would show here, not hide)
    g = gg.grammar
    arc_w = {}
    for a, b_, l, w in zip(g.src, g.dst, g.ilabel, g.weight):
        arc_w.setdefault((int(a), int(l)), []).append((int(b_), float(w)))
    for b, n in enumerate(lens):
        front = {0: 0.0}                            # state -> best score over the label sequence
        for t in range(n):
            nxt = {}
            for st, sc in front.items():
                for to, w in arc_w.get((st, int(best[t, b])), ()):
                    val = sc + w + float(lp[t, b, best[t, b]])
                    if val > nxt.get(to, -np.inf):
                        nxt[to] = val
            front = nxt
        assert front, 'the returned labels are not a path of the graph'
        score = max(sc + float(g.final[st]) for st, sc in front.items())
        np.testing.assert_allclose(score, v[b], rtol=1e-5, atol=1e-5)


def test_path_reduction_dispatches_on_the_shared_tag(oracle_lib, monkeypatch):
    """tagged matrices reach the shared kernel through the reference-shaped surface, with
    ASR_SHARED_NATIVE=0 (read per call) the generic kernel runs the same graph"""
    from att_speech import _native, fst_utils as P
    gg, lp, lens = _inputs('bigram', 12, [12, 9, 1, 0])
    tagged = gg.get_decoding_matrices()
    mats = [m.numpy() for m in tagged]
    want = oracle_lib.path_logsumexp(lp, lens, mats)
    calls = []
    real = _native.shared_fwbw
    monkeypatch.setattr(_native, 'shared_fwbw', lambda *a, **k: calls.append(1) or real(*a, **k))
    out = {}
    for flag in ('1', '0'):
        monkeypatch.setenv('ASR_SHARED_NATIVE', flag)
        x = torch.from_numpy(lp).to(dev()).requires_grad_()
        z = P.path_reduction(x, torch.from_numpy(lens), tagged, red_kind='logsumexp')
        z.sum().backward()
        out[flag] = (z.detach().cpu().numpy(), x.grad.cpu().numpy())
        np.testing.assert_allclose(out[flag][0], want['logZ'], rtol=RTOL_LOSS, atol=1e-5)
        assert_posteriors(out[flag][1], want['grad'], lp, lens, mats, oracle_lib)
        assert len(calls) == 1                      # native once, then never
        v = P.path_reduction(x.detach(), torch.from_numpy(lens), tagged, red_kind='viterbi')
        out[flag] += (v.cpu().numpy(),)
    np.testing.assert_allclose(out['1'][2], out['0'][2], rtol=1e-6, atol=1e-6)


def test_unsupported_graph_falls_back_with_one_warning(oracle_lib, monkeypatch):
    """bigram-context HC o G consumes S^2 classes; beyond the kernel's limit (forced here on a toy
    graph) the generic kernel runs the padded matrices, says so once, and gives the same values"""
    from att_speech import _native, fst_utils as P
    lm, vocab = toy_lm('s3')
    gg = P.CTCGraphGen(context_order=2, num_symbols=3, grammar_fst=lm, vocabulary=vocab)
    tagged = gg.get_decoding_matrices()
    rng = np.random.default_rng(9)
    T, lens = 6, np.array([6, 4], np.int32)
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, 2, 9)).astype(np.float32)), -1)
    x = lp.to(dev())
    z_native = P.path_reduction(x, torch.from_numpy(lens), tagged, red_kind='logsumexp_fwb').cpu().numpy()
    want = oracle_lib.path_logsumexp(lp.numpy(), lens, [m.numpy() for m in tagged])
    np.testing.assert_allclose(z_native, want['logZ'], rtol=RTOL_LOSS, atol=1e-5)
    assert not _native.lib().asr_lattice_shared_supported(8000, 10, 9)
    assert not _native.lib().asr_lattice_shared_supported(100, 10, 2401)
    monkeypatch.setattr(_native.SharedGraph, 'supported', lambda self, C: False)
    _native._WARNED.pop('shared_unsupported', None)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        z1 = P.path_reduction(x, torch.from_numpy(lens), tagged, red_kind='logsumexp_fwb').cpu().numpy()
        z2 = P.path_reduction(x, torch.from_numpy(lens), tagged, red_kind='logsumexp_fwb').cpu().numpy()
    assert len([w for w in rec if 'generic' in str(w.message)]) == 1
    np.testing.assert_allclose(z1, z_native, rtol=RTOL_LOSS, atol=1e-5)
    np.testing.assert_array_equal(z1, z2)


def test_fst_decoder_with_grammar_loss_gradient_and_decode(monkeypatch):
    """FSTDecoder with grammar_fst, globally normalised: loss and d loss / d encoded against a CPU
    evaluation of the reference's path_reduction on the padded matrices (identical encoder output:
    the 1e-4 bound of tests/test_model_gpu.py); decode gives the same labels on both kernels."""
    from att_speech.modules.decoders.advanced_decoder import FSTDecoder
    torch.manual_seed(3)
    vocab = [l.rstrip('\n') for l in open(WSJ_VOCAB)][:49]
    B, T, D, L = 3, 14, 24, 4
    enc = torch.randn(T, B, D)
    elens = torch.tensor([14, 11, 7], dtype=torch.int32)
    texts = torch.tensor([[5, 3, 2, 9], [4, 4, 7, 0], [11, 2, 0, 0]], dtype=torch.int32)
    tlens = torch.tensor([4, 3, 2], dtype=torch.int32)
    dec = FSTDecoder({'features': torch.zeros(B, T, D)}, 49,
                     dict(class_name='CTCGraphGen', context_order=1, grammar_fst=BIGRAM_LM,
                          vocabulary=WSJ_VOCAB),
                     normalize_by_dim=None, denominator_red='logsumexp', vocabulary=vocab)
    gg = dec.graph_generator
    ref = copy.deepcopy(dec).double()
    e64 = enc.double().requires_grad_()
    logits = ref.fc(e64)
    shifted = logits - logits.max(-1, keepdim=True)[0].detach()
    num = torch_path_reduction(shifted, elens, gg.get_training_matrices_batch(texts, tlens))
    den = torch_path_reduction(shifted, elens, gg.get_decoding_matrices('cpu'))
    want = (den - num).sum()
    want.backward()

    dec.to(dev())
    eg = enc.to(dev()).requires_grad_()
    out = dec(eg, elens, texts, tlens)
    out['loss'].backward()
    got = float(out['loss'])
    assert abs(got - float(want)) <= 1e-4 * abs(float(want)), (got, float(want))
    torch.testing.assert_close(eg.grad.cpu().double(), e64.grad, rtol=1e-4, atol=1e-3)
    decoded = {}
    for flag in ('1', '0'):
        monkeypatch.setenv('ASR_SHARED_NATIVE', flag)
        with torch.no_grad():
            decoded[flag] = dec.decode(eg.detach(), elens)['decoded']
    assert decoded['1'] == decoded['0'] and len(decoded['1']) == B
    # and the two-node loss on the generic kernel agrees with the fused node on the new one
    monkeypatch.setenv('ASR_SHARED_NATIVE', '0')
    out0 = dec(eg.detach(), elens, texts, tlens)
    assert abs(float(out0['loss']) - got) <= 1e-4 * abs(got)
