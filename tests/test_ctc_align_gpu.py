"""CTC forced alignment on the MI355X: asr_ctc_align_f64 (csrc/ctc_align.hip) against the
reference's recorded outputs (tests/golden/ctc_align.npz), bit for bit on cost, frames, states
and segments: the kernel does the reference's fp64 additions and takes its first maximum, so no
tolerance appears here.  Then the host fall-back, the ASR_ALIGN_NATIVE switch and the align
methods of the decoders and of SpeechModel."""
import numpy as np
import pytest
import torch

import align_cases

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def _ctc():
    from att_speech.modules import ctc_losses
    return ctc_losses


def _native_batch(cases, act_override=None):
    """the kernel through _native on one assembled batch -> numpy (cost, frames, states, segments)"""
    from att_speech import _native
    lp, labels, act, lls = align_cases.assemble(cases, act_override)
    Lmax = max(lls)
    padded = np.zeros((len(cases), Lmax), np.int32)
    for b, c in enumerate(cases):
        padded[b, :c['L']] = c['labels']
    f = align_cases.flags(cases[0])
    got = _native.ctc_align(
        torch.from_numpy(lp).to(DEV), torch.tensor(act, dtype=torch.int32, device=DEV),
        torch.from_numpy(padded).to(DEV), torch.tensor(lls, dtype=torch.int32, device=DEV),
        f['num_symbols'], f['context_order'], f.get('allow_nonblank_selfloops', True),
        f.get('eval_repeats_in_context', False))
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in got], lp.shape[0], Lmax


def _assert_equal(got, want, what):
    for g, w, field in zip(got, want, ('cost', 'frames', 'states', 'segments')):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, field)
        assert (g == w).all(), (what, field)                    # inf == inf counts


def _small_groups():
    by = {}
    for name in align_cases.names():
        if not name.startswith('edge_'):
            c = align_cases.case(name)
            by.setdefault(align_cases.group_key(c), []).append(c)
    return by


def test_every_small_case_alone_is_bit_equal():
    """B = 1: mono, bicontext under the four flag settings (S = 5, 7), the S = 49 case, ties by
    quantised and constant frames, and the infeasible ones (cost inf, -1 everywhere)"""
    groups = _small_groups()
    assert len(groups) == 10                                    # mono, 2 x 4 bicontext, S = 49
    for key, cases in groups.items():
        for c in cases:
            got, T, Lmax = _native_batch([c])
            _assert_equal(got, align_cases.want([c], T, Lmax), c['name'])


def test_batches_of_five_with_unsorted_lengths_are_bit_equal():
    for key, cases in _small_groups().items():
        cases = cases[::-1]
        for i in range(0, len(cases) - 4, 5):
            batch = cases[i:i + 5]
            if i % 2:
                batch = batch[2:] + batch[:2]
            got, T, Lmax = _native_batch(batch)
            _assert_equal(got, align_cases.want(batch, T, Lmax), (key, i))


def test_mixed_batches_with_infeasible_and_empty_utterances():
    """whole groups as one batch: feasible next to infeasible utterances, one cut to zero frames
    (act_lens[b] == 0); padding rows and labels are -1"""
    for key, cases in _small_groups().items():
        if len(cases) < 3:
            continue
        feasible = [b for b, c in enumerate(cases) if c['feasible']]
        cut = {feasible[len(feasible) // 2]}
        got, T, Lmax = _native_batch(cases, {b: 0 for b in cut})
        want = align_cases.want(cases, T, Lmax, infeasible=cut)
        assert np.isinf(want[0]).sum() > len(cut) and np.isfinite(want[0]).sum() > 1
        _assert_equal(got, want, key)
        for b, c in enumerate(cases):
            if np.isfinite(want[0][b]):
                assert (got[1][b, c['T']:] == -1).all() and (got[2][b, c['T']:] == -1).all()
                assert (got[3][b, c['L']:] == -1).all() and (got[3][b, :c['L']] >= 0).all()
            else:
                assert (got[1][b] == -1).all() and (got[2][b] == -1).all() and (got[3][b] == -1).all()


@pytest.mark.parametrize('name', [
    'edge_mono_L31', 'edge_mono_L32', 'edge_mono_L33',          # N = 63, 65, 67: across 16 lanes
    'edge_mono_L127',                                           # N = 255: the last single-wave size
    'edge_mono_L128', 'edge_mono_L129',                         # N = 257, 259: four waves, LDS exchange
    'edge_mono_L127_T768',                                      # back-pointers: exactly 48 KiB of LDS
    'edge_mono_L127_T769',                                      # one frame more: the global workspace
    'edge_mono_L511_T1100',                                     # the largest lattice, global workspace
    'edge_bi2_10_L33', 'edge_bi2_11_L34', 'edge_bi2_00_L35', 'edge_bi2_01_L36'])
def test_kernel_boundary_shapes_are_bit_equal(name):
    from att_speech import _native
    c = align_cases.case(name)
    assert c['feasible']
    in_lds = _native.lib().asr_ctc_align_workspace_bytes(c['T'], 1, c['L']) == 0
    assert in_lds == (name not in ('edge_mono_L127_T769', 'edge_mono_L511_T1100'))
    got, T, Lmax = _native_batch([c])
    _assert_equal(got, align_cases.want([c], T, Lmax), name)


def test_boundary_shapes_in_one_batch_with_shorter_neighbours():
    """a multi-wave batch: Lmax = 129 sizes the launch, the shorter lattices run in it"""
    cases = [align_cases.case(n) for n in ('edge_mono_L33', 'edge_mono_L129', 'edge_mono_L31', 'edge_mono_L128',
                                           align_cases.names(kind='mono', L=3, T=7, feasible=True)[0])]
    got, T, Lmax = _native_batch(cases)
    _assert_equal(got, align_cases.want(cases, T, Lmax), 'mixed')


def _random_batch(L, T, B=2, C=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(torch.randn(T, B, C, generator=g), -1)
    lp = torch.round(lp * 2) / 2
    labels = torch.randint(1, C, (B * L,), generator=g)
    return lp, labels, [T, T - 3][:B], [L] * B


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and bool((x.cpu() == y.cpu()).all())


def test_transcripts_longer_than_the_kernel_take_the_host_path():
    ctc = _ctc()
    from att_speech import _native
    lp, labels, act, lls = _random_batch(512, 700)
    assert not _native.ctc_align_supported(700, 512, 7)
    with pytest.raises(NotImplementedError):
        _native.ctc_align(lp.to(DEV), torch.tensor(act, dtype=torch.int32, device=DEV),
                          labels.view(2, 512).int().to(DEV), torch.tensor(lls, dtype=torch.int32, device=DEV), 7)
    got = ctc.ctc_viterbi_align_batch(lp.to(DEV), labels, act, lls)
    want = ctc.ctc_viterbi_align_batch(lp, labels, act, lls)
    assert got.cost.is_cuda and bool(got.feasible.all())
    _same(got, want)


def test_native_switch_gives_the_same_bits(monkeypatch):
    ctc = _ctc()
    lp, labels, act, lls = _random_batch(40, 90)
    on = ctc.ctc_viterbi_align_batch(lp.to(DEV), labels, act, lls)
    monkeypatch.setenv('ASR_ALIGN_NATIVE', '0')
    calls = []
    from att_speech import _native
    monkeypatch.setattr(_native, 'ctc_align', lambda *a, **k: calls.append(1))
    off = ctc.ctc_viterbi_align_batch(lp.to(DEV), labels, act, lls)
    assert not calls and off.cost.is_cuda
    _same(on, off)


def test_single_utterance_functions_route_device_tensors_through_the_kernel(monkeypatch):
    ctc = _ctc()
    from att_speech import _native
    calls = []
    real = _native.ctc_align
    monkeypatch.setattr(_native, 'ctc_align', lambda *a, **k: calls.append(1) or real(*a, **k))
    c = align_cases.case(align_cases.names(kind='mono', L=4, T=30, feasible=True)[0])
    cost, sol = ctc.mono_CTC_viterbi_align(torch.from_numpy(np.array(c['lp'])).to(DEV),
                                           torch.from_numpy(np.array(c['labels'])).long())
    assert np.float64(cost) == c['cost'] and (sol.numpy() == c['sol']).all()
    c = align_cases.case('bi5_01_triple')
    cost, sol = ctc.bi_CTC_viterbi_align(torch.from_numpy(np.array(c['lp'])).to(DEV),
                                         torch.from_numpy(np.array(c['labels'])).long(),
                                         allow_nonblank_selfloops=False, eval_repeats_in_context=True)
    assert np.float64(cost) == c['cost'] and (sol.numpy() == c['sol']).all()
    assert len(calls) == 2


# ---------------------------------------------------------------------------- model surface
VOCAB7 = [str(i) for i in range(7)]


def _texts(B, L, S, seed):
    g = torch.Generator().manual_seed(seed)
    texts = torch.randint(1, S, (B, L), generator=g, dtype=torch.int32)
    texts[0, 1] = texts[0, 0]                                   # a repeat
    return texts, torch.tensor([L, L - 2, 1][:B], dtype=torch.int32)


def _check_decoder(dec, order, flags):
    ctc = _ctc()
    torch.manual_seed(1)
    T, B, S = 20, 3, 7
    enc = torch.randn(T, B, 16).to(DEV)
    elens = torch.tensor([20, 13, 17], dtype=torch.int32)
    texts, llens = _texts(B, 5, S, 2)
    out = dec.align(enc, elens, texts, llens)
    with torch.no_grad():
        logits = dec.logits(enc, elens)
    flat = torch.cat([texts[b, :llens[b]] for b in range(B)]).long()
    want = ctc.ctc_viterbi_align_batch(logits, flat, elens, llens, num_symbols=S, context_order=order, **flags)
    assert set(out) == {'cost', 'frames', 'states', 'segments', 'feasible', 'alignment'}
    _same([out[k] for k in want._fields], want)
    assert bool(out['feasible'].all()) and out['cost'].is_cuda
    seg = out['segments'].cpu().tolist()
    assert out['alignment'] == [[(int(texts[b, i]), seg[b][i][0], seg[b][i][1]) for i in range(int(llens[b]))]
                                for b in range(B)]
    # the kernel scored these logits: the host path gives the same bits
    host = ctc.ctc_viterbi_align_batch(logits.cpu(), flat, elens, llens, num_symbols=S, context_order=order,
                                       **flags)
    _same([out[k].cpu() for k in host._fields], host)


@pytest.mark.parametrize('order', [1, 2])
def test_ctc_decoder_advanced_align(order):
    from att_speech.modules.decoders import CTCDecoderAdvanced
    torch.manual_seed(0)
    kw = {} if order == 1 else dict(normalize_by_dim=1, ctc_loss_fn='ctc_raw_loss_batch',
                                    ctc_allow_nonblank_selfloops=False)
    dec = CTCDecoderAdvanced({'features': torch.zeros(20, 2, 16)}, 7 ** order, context_order=order,
                             vocabulary=VOCAB7, **kw).to(DEV).eval()
    flags = {} if order == 1 else dict(allow_nonblank_selfloops=False, eval_repeats_in_context=False)
    _check_decoder(dec, order, flags)


def _fst_decoder(order, **gg):
    from att_speech.modules.decoders.advanced_decoder import FSTDecoder
    return FSTDecoder({'features': torch.zeros(20, 2, 16)}, 7 ** order,
                      graph_generator=dict(class_name='CTCGraphGen', context_order=order, **gg),
                      vocabulary=VOCAB7)


@pytest.mark.parametrize('order', [1, 2])
def test_fst_decoder_align(order):
    torch.manual_seed(0)
    gg = {} if order == 1 else dict(graph_build_args=dict(use_contextual_blanks=True))
    dec = _fst_decoder(order, **gg).to(DEV).eval()
    flags = {} if order == 1 else dict(allow_nonblank_selfloops=True, eval_repeats_in_context=True)
    _check_decoder(dec, order, flags)


def test_fst_decoder_align_refuses_grammars_and_global_blanks():
    from att_speech.modules.decoders.advanced_decoder import FSTDecoder
    from grammar_cases import toy_lm
    lm, vocab = toy_lm('s3')
    dec = FSTDecoder({'features': torch.zeros(20, 2, 16)}, 3,
                     graph_generator=dict(class_name='CTCGraphGen', context_order=1, grammar_fst=lm,
                                          vocabulary=vocab), vocabulary=vocab)
    enc, elens = torch.randn(6, 1, 16), torch.tensor([6], dtype=torch.int32)
    texts, llens = torch.tensor([[1, 1]], dtype=torch.int32), torch.tensor([2], dtype=torch.int32)
    with pytest.raises(ValueError, match='grammar'):
        dec.align(enc, elens, texts, llens)
    with pytest.raises(ValueError, match='global blank'):
        _fst_decoder(2).align(enc, elens, texts, llens)


def test_speech_model_align():
    from att_speech.models import SpeechModel
    from test_modules import DEC_MONO, ENC, VOCAB, sample_batch
    from test_model_gpu import make_batch
    torch.manual_seed(3)
    B, T, S = 3, 100, 49
    feats, lens, texts, llens = make_batch(B, T, S, 6, 1, 5)
    model = SpeechModel(ENC, DEC_MONO, sample_batch(B=2, T=T), S, VOCAB).to(DEV).eval()
    out = model.align(feats.to(DEV), lens, None, texts, llens)
    with torch.no_grad():
        enc, elens = model.encoder(feats.to(DEV), lens, None)
    want = model.decoder.align(enc, elens, texts, llens)
    assert set(out) == set(want)
    for k in ('cost', 'frames', 'states', 'segments', 'feasible'):
        assert bool((out[k] == want[k]).all()) and not out[k].requires_grad
    assert out['alignment'] == want['alignment'] and bool(out['feasible'].all())
    assert out['frames'].shape == (B, enc.size(0))
    for b in range(B):
        spans = out['alignment'][b]
        assert [s[0] for s in spans] == texts[b, :llens[b]].tolist()
        assert all(0 <= s[1] < s[2] <= int(elens[b]) for s in spans)
        assert all(p[2] <= n[1] for p, n in zip(spans, spans[1:]))
