"""AttentionDecoderTCN.score_sentences on the MI355X: asr_forced_level_f32 one launch at a time
against the fp64 restatement of forced_cases.forced_level_ref, the device path (prefix trie, one
label step per level) against the per-sentence host loop on the same device (ASR_FORCED_NATIVE=0)
and against the golden record of the reference, the work the trie saves, and the fallbacks."""
import copy
import os
import warnings

import numpy as np
import pytest
import torch

import forced_cases as fc
import lm_beam_referee as lr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SWITCH = 'ASR_FORCED_NATIVE'
TAU = 0.1


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(DEV)


def with_switch(value, fn):
    old = os.environ.get(SWITCH)
    if value is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = value
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = old


# ---------------------------------------------------------------- 1. the kernel, one launch

def level_case(C, T, seed):
    """two utterances of lengths (T, ceil(T / 2)), six slots each over four rows of the previous
    level: 0 a unit with EOS and two label edges, 1 a dead slot, 2 a unit with only its EOS edge,
    3 and 4 two units sharing a parent, 5 a unit with one label edge"""
    rng = np.random.default_rng(seed)
    B, W, rows, W_next = 2, 6, 4, 5
    lens = np.array([T, (T + 1) // 2], np.int32)
    parent = np.concatenate([u * rows + np.array([1, 0, 3, 2, 2, 0]) for u in range(B)]).astype(np.int32)
    counts, lab, dst, sent = [], [], [], 0
    for u in range(B):
        picks = rng.permutation(C - 1)[:4]
        per_slot = [[(C - 1, None), (picks[0], 0), (picks[1], 1)], [], [(C - 1, None)],
                    [(picks[2], 2)], [(picks[2], 3)], [(picks[3], 4)]]
        for edges in per_slot:
            counts.append(len(edges))
            for label, nxt in edges:
                lab.append(int(label))
                if nxt is None:
                    dst.append(-1 - sent)
                    sent += 1
                else:
                    dst.append(u * W_next + nxt)
    logits = rng.standard_normal((B * W, C))
    logits = (logits * (30.0 / np.abs(logits).max())).astype(np.float32)

    def alignments(n):
        a = np.zeros((n, T), np.float32)
        for r in range(n):
            ln = int(lens[r * B // n])
            a[r, :ln] = torch.softmax(torch.from_numpy(rng.standard_normal(ln) * 3.0), 0).float().numpy()
        return a
    att, cov_in = alignments(B * W), alignments(B * rows) + alignments(B * rows)
    for _ in range(50):                      # every |coverage - tau| clear of the threshold
        close = np.abs((cov_in[parent] + att).astype(np.float32).astype(np.float64) - TAU) <= 1e-3
        if not close.any():
            break
        att[close] += np.float32(0.01)
    else:
        raise AssertionError('no clear coverage margins')
    return dict(B=B, W=W, C=C, T=T, lens=lens, parent=parent, logits=logits, att=att, cov_in=cov_in,
                edge_ptr=np.concatenate(([0], np.cumsum(counts))).astype(np.int32),
                edge_label=np.array(lab, np.int32), edge_dst=np.array(dst, np.int32),
                acoustic_in=-rng.uniform(0.0, 40.0, B * W), n_out=B * W_next + 1, n_sent=sent + 1)


def launch(c):
    from att_speech import _native
    out = dict(cov_out=torch.full((c['B'] * c['W'], c['T']), -7.0, device=DEV),
               acoustic_out=torch.full((c['n_out'],), -7.0, dtype=torch.float64, device=DEV),
               sent_acoustic=torch.full((c['n_sent'],), -7.0, dtype=torch.float64, device=DEV),
               sent_covered=torch.full((c['n_sent'],), -7, dtype=torch.int32, device=DEV))
    _native.forced_level(t(c['logits']), t(c['att']), t(c['cov_in']), out['cov_out'], t(c['parent']),
                         t(c['edge_ptr']), t(c['edge_label']), t(c['edge_dst']), t(c['acoustic_in']),
                         out['acoustic_out'], t(c['lens']), c['B'], c['W'], TAU, out['sent_acoustic'],
                         out['sent_covered'])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('C', [7, 50])
@pytest.mark.parametrize('T', [1, 40, 334])
def test_forced_level_against_fp64(C, T):
    """The error of a log-probability term against fp64, |logit| up to 30, is printed per case for
    the kernel and for torch's fp32 log_softmax + gather.  Measured on the MI355X: the two were
    equal in every case, between 6.7e-7 (C 7, T 1) and 3.5e-6 (C 50, T 40)."""
    c = level_case(C, T, seed=100 * C + T)
    want = fc.forced_level_ref(c['logits'], c['att'], c['cov_in'], c['parent'], c['edge_ptr'],
                               c['edge_label'], c['edge_dst'], c['acoustic_in'], c['lens'], c['B'],
                               c['W'], TAU, c['n_out'], c['n_sent'])
    assert want['cov_margin'] > 1e-3
    got = launch(c)
    # coverage rows: one fp32 add, bit for bit, dead slots included
    assert got['cov_out'].tobytes() == want['cov_out'].tobytes()
    # every owned output is written, nothing else is touched
    assert (got['acoustic_out'][~want['out_written']] == -7.0).all()
    assert (got['sent_acoustic'][~want['sent_written']] == -7.0).all()
    assert (got['sent_covered'][~want['sent_written']] == -7).all()
    assert want['out_written'].sum() == 10 and want['sent_written'].sum() == 4
    np.testing.assert_array_equal(got['sent_covered'][want['sent_written']],
                                  want['sent_covered'][want['sent_written']])
    # the log-probability terms: no worse than twice torch's fp32 log_softmax on the same device
    src = np.repeat(np.arange(c['B'] * c['W']), np.diff(c['edge_ptr']))
    d = c['edge_dst']
    got_v = np.where(d >= 0, got['acoustic_out'][np.maximum(d, 0)], got['sent_acoustic'][np.maximum(-1 - d, 0)])
    kernel_err = np.abs(got_v - (c['acoustic_in'][src] + want['terms'])).max()
    lp = torch.log_softmax(t(c['logits']), 1).double().cpu().numpy()
    torch_err = np.abs(lp[src, c['edge_label']] - want['terms']).max()
    print('C %d T %d: kernel error %.3g, torch log_softmax error %.3g' % (C, T, kernel_err, torch_err))
    assert kernel_err <= 2 * torch_err + 1e-6
    # a second launch on the same inputs agrees bit for bit
    again = launch(c)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k


# ---------------------------------------------------------------- 2. end to end

def assert_scores_agree(native, host, dec, enc, lens, sentences, coverage):
    """counts equal, lm to 1e-9, acoustic / loss to 1e-4; where a value misses that, an fp64
    evaluation of the host path on the CPU arbitrates (native no farther than twice the torch path
    is, plus 1e-6)"""
    ref = None
    for u in range(len(native)):
        np.testing.assert_array_equal(native[u]['covered'], host[u]['covered'])
        np.testing.assert_array_equal(native[u]['coverage'], host[u]['coverage'])
        np.testing.assert_allclose(native[u]['lm'], host[u]['lm'], rtol=1e-9)
        for k in ('acoustic', 'loss'):
            if np.allclose(native[u][k], host[u][k], rtol=1e-4, atol=1e-4):
                continue
            if ref is None:
                ref = copy.deepcopy(dec).double().cpu().score_sentences(
                    enc.double().cpu(), lens, sentences, coverage=coverage)
            err_n, err_h = np.abs(native[u][k] - ref[u][k]), np.abs(host[u][k] - ref[u][k])
            print('utterance %d %s: native error %.3g, torch path error %.3g' % (u, k, err_n.max(), err_h.max()))
            assert (err_n <= 2 * err_h + 1e-6).all()


def scored(dec, enc, lens, sentences, coverage='log_fraction'):
    native = with_switch('1', lambda: dec.score_sentences(enc, lens, sentences, coverage=coverage))
    host = with_switch('0', lambda: dec.score_sentences(enc, lens, sentences, coverage=coverage))
    return native, host


@pytest.mark.parametrize('tag', ['plain', 'ff'])
def test_golden_record_native_against_host_and_reference(tag):
    from att_speech import _native
    dec = fc.golden_decoder(tag).to(DEV)
    enc, lens, sentences, want = fc.golden_inputs(tag)
    enc = enc.to(DEV)
    calls = []
    real = _native.forced_level
    _native.forced_level = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        native, host = scored(dec, enc, lens, sentences)
        by_count = with_switch('1', lambda: dec.score_sentences(enc, lens, sentences, coverage='count'))
    finally:
        _native.forced_level = real
    # one launch per trie level, none from the host path
    assert len(calls) == 2 * (max(len(s) for per in sentences for s in per) + 1)
    assert_scores_agree(native, host, dec, enc, lens, sentences, 'log_fraction')
    for u in range(3):
        np.testing.assert_array_equal(native[u]['covered'], want['covered'][u])
        np.testing.assert_allclose(native[u]['lm'], want['lm'][u], rtol=1e-9)
        np.testing.assert_allclose(native[u]['acoustic'], want['acoustic'][u], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(native[u]['coverage'], want['cov_log'][u], rtol=1e-6)
        np.testing.assert_allclose(native[u]['loss'], want['loss_log'][u], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(by_count[u]['coverage'], want['cov_count'][u], rtol=1e-6)
        np.testing.assert_allclose(by_count[u]['loss'], want['loss_count'][u], rtol=1e-5, atol=1e-5)
    # a single utterance, cut to its own frames, gives the batch's values for it
    alone = with_switch('1', lambda: dec.score_sentences(enc[:23, 1:2].contiguous(), lens[1:2], sentences[1:2]))
    np.testing.assert_array_equal(alone[0]['covered'], native[1]['covered'])
    np.testing.assert_allclose(alone[0]['loss'], native[1]['loss'], rtol=1e-5, atol=1e-5)


YAML_SENTENCES = [
    [[5, 9, 2], [5, 9, 2, 30], [5, 9, 2, 31], [5, 9], [5, 9, 2, 30, 7, 7], [12], [5, 9, 2],
     [5, 10, 2, 30], [48, 0, 5]],
    [[3, 3, 3, 3, 3, 3], [3, 3, 3], [3], [4], [3, 3, 4], [3, 3, 3, 3, 3, 4], [20, 21, 22, 23],
     [20, 21, 22, 24], [3, 3, 3]]]


def yaml_decoder(with_lm):
    """tcn.yaml dimensions as tests/test_tcn_train_gpu.py makes them, the scripts' score settings"""
    from test_tcn_train_gpu import make_decoder
    dec = make_decoder(seed=6).eval()
    dec.coverage_tau, dec.coverage_weight = 0.1, 0.5
    dec.lm_weight, dec.length_normalization = 0.8, 1.2
    if with_lm:
        dec.vocabulary = [' ', 'a', 'b', 'c'] + ['x%d' % i for i in range(45)]
        dec.lm = lr.toy_lm()
        dec.alphabet_mapping = dec.create_alphabet_mapping()
    return dec.to(DEV)


@pytest.mark.parametrize('with_lm', [False, True])
def test_yaml_dimensions_native_against_host(with_lm):
    # model seed 6 / encoder seed 13: picked on the CPU (the host path, fp32) for a smallest
    # |coverage - tau| of 3.3e-3 over every frame of every sentence, above the 1e-3 floor of the
    # golden records, so the counts of the two paths cannot differ
    dec = yaml_decoder(with_lm)
    enc = torch.randn(40, 2, 320, generator=torch.Generator().manual_seed(13)).to(DEV)
    lens = torch.tensor([40, 27])
    for coverage in ('log_fraction', 'count'):
        native, host = scored(dec, enc, lens, YAML_SENTENCES, coverage)
        assert_scores_agree(native, host, dec, enc, lens, YAML_SENTENCES, coverage)
        for u in range(2):
            assert (native[u]['lm'] != 0.0).all() == with_lm
    assert native[0]['acoustic'][0] == native[0]['acoustic'][6]              # duplicates
    assert native[1]['acoustic'][1] == native[1]['acoustic'][8]


def test_trie_saving_counts_distinct_prefixes():
    from att_speech import _native
    dec = yaml_decoder(False)
    enc = torch.randn(40, 1, 320, generator=torch.Generator().manual_seed(2)).to(DEV)
    rng = np.random.default_rng(9)
    shared = [7, 8, 9, 10, 11]
    sentences = [shared + [int(c) for c in rng.integers(0, 4, size=int(rng.integers(1, 4)))]
                 for _ in range(32)]
    prefixes = {tuple(s[:l]) for s in sentences for l in range(len(s) + 1)}
    positions = sum(len(s) + 1 for s in sentences)
    launched = []
    real = _native.tcn_attention_step

    def counting(eproj, *args, **kw):
        beam = args[9] if len(args) > 9 else kw['beam']
        launched.append(eproj.shape[1] * beam)
        return real(eproj, *args, **kw)
    _native.tcn_attention_step = counting
    try:
        res = with_switch('1', lambda: dec.score_sentences(enc, torch.tensor([40]), [sentences]))
    finally:
        _native.tcn_attention_step = real
    print('step-kernel hypotheses %d, sentences x positions %d' % (sum(launched), positions))
    assert sum(launched) == len(prefixes) < positions
    assert launched[:6] == [1] * 6 and len(launched) == max(len(s) for s in sentences) + 1
    assert np.isfinite(res[0]['loss']).all() and res[0]['loss'].shape == (32,)


# ---------------------------------------------------------------- 3. fallbacks

def no_native_calls():
    from att_speech import _native
    saved = _native.forced_level, _native.tcn_attention_step

    def refuse(*a, **k):
        raise AssertionError('a native launch on the host path')
    _native.forced_level = _native.tcn_attention_step = refuse
    return saved


def test_switch_and_refused_window_take_the_host_path():
    from att_speech import _native
    dec = fc.golden_decoder('ff').to(DEV)
    enc, lens, sentences, want = fc.golden_inputs('ff')
    enc = enc.to(DEV)
    native = with_switch('1', lambda: dec.score_sentences(enc, lens, sentences))
    saved = no_native_calls()
    try:
        host = with_switch('0', lambda: dec.score_sentences(enc, lens, sentences))
        dec.attn.force_forward = (-2.0, 6.0)             # not integers: the step refuses it
        refused = with_switch('1', lambda: dec.score_sentences(enc, lens, sentences))
        cpu = with_switch('1', lambda: copy.deepcopy(dec).cpu().score_sentences(enc.cpu(), lens, sentences))
    finally:
        _native.forced_level, _native.tcn_attention_step = saved
    for u in range(3):
        for k in ('acoustic', 'coverage', 'lm', 'loss'):
            assert refused[u][k].tobytes() == host[u][k].tobytes()
            np.testing.assert_allclose(cpu[u][k], host[u][k], rtol=1e-4, atol=1e-4)
        np.testing.assert_array_equal(native[u]['covered'], host[u]['covered'])


def test_bag_overflow_falls_back_with_one_warning():
    from att_speech import _native
    from att_speech.lm_fst import LmFst, SymbolTable
    from att_speech.modules.tcn import AttentionDecoderTCN
    # the overflow LM of tests/test_lm_beam_gpu.py: 33 arcs of every label out of state 0
    syms = SymbolTable([(0, '<eps>'), (1, '<spc>'), (2, 'a'), (3, 'b'), (4, 'c')])
    n = 33
    src = [0] * (4 * n) + [s for s in range(1, n + 1) for _ in range(4)]
    dst = [1 + i for _ in range(4) for i in range(n)] + [0] * (4 * n)
    il = [l for l in (1, 2, 3, 4) for _ in range(n)] + [1, 2, 3, 4] * n
    w = list(np.linspace(0.5, 2.0, len(src)))
    lm = LmFst(n + 1, 0, src, dst, il, il, w, np.zeros(n + 1), syms, syms)
    torch.manual_seed(0)
    dec = AttentionDecoderTCN({'features': torch.zeros(14, 1, 16)}, 6, tcn_hidden_size=32,
                              att_hidden_size=8, dropout_p=0.0, kernel_size=3, dilation_sizes=[1, 2],
                              vocabulary=['<pad>', '<unk>', ' ', 'a', 'b', 'c'], lm_file=lm, lm_weight=0.5,
                              coverage_weight=0.1, coverage_tau=0.1).eval().to(DEV)
    enc = torch.randn(14, 1, 16, generator=torch.Generator().manual_seed(1)).to(DEV)
    sentences = [[[3, 4], [3, 5, 2], [4]]]
    _native._WARNED.pop('forced_lm_bag_overflow', None)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        first = with_switch('1', lambda: dec.score_sentences(enc, torch.tensor([14]), sentences))
        again = with_switch('1', lambda: dec.score_sentences(enc, torch.tensor([14]), sentences))
    msgs = [str(r.message) for r in rec if 'LM bag' in str(r.message)]
    assert len(msgs) == 1 and '33' in msgs[0]
    host = with_switch('0', lambda: dec.score_sentences(enc, torch.tensor([14]), sentences))
    for k in ('acoustic', 'coverage', 'lm', 'loss'):
        assert first[0][k].tobytes() == host[0][k].tobytes() == again[0][k].tobytes()
    assert np.isfinite(host[0]['lm']).all()
