"""CTC forced alignment on the host (att_speech.modules.ctc_losses: the dense builders,
raw_generic_viterbi, the mono / bi align and decode functions, ctc_viterbi_align_batch) against
the reference's recorded outputs, tests/golden/ctc_align.npz.  Everything is compared with ==:
the accumulator is fp64 and every step is one IEEE addition of a float32 value, so no tolerance
applies anywhere."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import align_cases
from conftest import ROOT


def _ctc():
    from att_speech.modules import ctc_losses
    return ctc_losses


def _align(c):
    ctc = _ctc()
    lp, lab = torch.from_numpy(np.array(c['lp'])), torch.from_numpy(np.array(c['labels'])).long()
    if c['kind'] == 'mono':
        return ctc.mono_CTC_viterbi_align(lp, lab)
    return ctc.bi_CTC_viterbi_align(lp, lab, allow_nonblank_selfloops=c['allow'],
                                    eval_repeats_in_context=c['evalrep'])


def _small():
    return [n for n in align_cases.names() if not n.startswith('edge_')]


def test_golden_covers_what_it_should():
    _, index, _ = align_cases.data()
    small = [c for c in index if not c['name'].startswith('edge_')]
    assert {c['T'] for c in small} >= {1, 2, 30} and {c['L'] for c in small} == set(range(1, 7))
    assert {(c['S'], c['allow'], c['evalrep']) for c in index if c['kind'] == 'bi'} >= {
        (S, a, e) for S in (5, 7) for a in (True, False) for e in (True, False)}
    assert any(not c['feasible'] for c in index) and any(c['S'] == 49 for c in index)
    assert {c['L'] for c in index} >= {31, 32, 33, 127, 128, 129, 511}


def test_every_small_case_equals_the_reference():
    for name in _small():
        c = align_cases.case(name)
        cost, sol = _align(c)
        assert np.float64(cost) == c['cost'], name            # inf == inf counts
        if c['feasible']:
            assert sol.dtype == torch.int32 and (sol.numpy() == c['sol']).all(), name


@pytest.mark.parametrize('name', ['edge_mono_L33', 'edge_mono_L129', 'edge_bi2_11_L34', 'edge_bi2_00_L35'])
def test_boundary_cases_equal_the_reference_through_the_dense_path(name):
    c = align_cases.case(name)
    cost, sol = _align(c)
    assert c['feasible'] and np.float64(cost) == c['cost'] and (sol.numpy() == c['sol']).all()


def test_decode_raw_and_looprepeats_equal_the_reference():
    ctc = _ctc()
    z = align_cases.data()[0]
    cost, sol = ctc.mono_CTC_viterbi_decode(torch.from_numpy(z['dec_mono_lp']))
    assert cost == z['dec_mono_cost'] and (sol.numpy() == z['dec_mono_sol']).all()
    for ev in (0, 1):
        cost, sol = ctc.bi_CTC_viterbi_decode(torch.from_numpy(z['dec_bi%d_lp' % ev]),
                                              eval_repeats_in_context=bool(ev))
        assert cost == z['dec_bi%d_cost' % ev] and (sol.numpy() == z['dec_bi%d_sol' % ev]).all()
    A, B = ctc.get_CTC_matrices_mono(torch.from_numpy(z['raw_labels']), 7)
    cost, sol = ctc.raw_generic_viterbi(torch.from_numpy(z['raw_lp']), A, B)
    assert cost == z['raw_cost'] and (sol.numpy() == z['raw_sol']).all()
    cost, sol = ctc.bi_CTC_viterbi_align(torch.from_numpy(z['loop_lp']), torch.from_numpy(z['loop_labels']),
                                         loop_using_symbol_repetitions=True)
    assert cost == z['loop_cost'] and (sol.numpy() == z['loop_sol']).all()


def test_dense_builders_equal_the_reference():
    ctc = _ctc()
    z, _, mats = align_cases.data()
    seen = set()
    for k, m in enumerate(mats):
        lab = torch.tensor(m['labels']) if 'labels' in m else None
        if m['what'] == 'mono':
            A, B = ctc.get_CTC_matrices_mono(lab, m['S'])
        elif m['what'] == 'bi':
            A, B = ctc.get_CTC_matrices_bicontext(lab, m['S'], eval_repeats_in_context=m['evalrep'],
                                                  allow_nonblank_selfloops=m['allow'])
        elif m['what'] == 'bi_loop':
            A, B = ctc.get_CTC_matrices_bicontext(lab, m['S'], loop_using_symbol_repetitions=True)
        elif m['what'] == 'bi_looprepeats':
            A, B = ctc.get_CTC_matrices_bicontext_looprepeats(lab, m['S'])
        elif m['what'] == 'dec_mono':
            A, B = ctc.get_CTC_decoding_matrices_mono(m['S'])
        else:
            assert m['what'] == 'dec_bi'
            A, B = ctc.get_CTC_decoding_matrices_bicontext(m['S'], eval_repeats_in_context=m['evalrep'])
        seen.add(m['what'])
        assert A.dtype == torch.float32 and B.dtype == torch.float32
        assert (A.numpy() == z['mats_%d_A' % k]).all() and (B.numpy() == z['mats_%d_B' % k]).all(), m
    assert seen == {'mono', 'bi', 'bi_loop', 'bi_looprepeats', 'dec_mono', 'dec_bi'}


def _groups():
    by = {}
    for name in _small():
        c = align_cases.case(name)
        by.setdefault(align_cases.group_key(c), []).append(c)
    return by


def test_batch_entry_on_cpu_equals_the_per_utterance_calls_and_the_reference():
    """mixed batches (feasible and infeasible, unsorted lengths, one utterance cut to zero frames):
    the band recurrence of the batch entry against the dense per-utterance functions"""
    ctc = _ctc()
    for key, cases in sorted(_groups().items(), key=str):
        cases = cases[::-1]                                     # lengths in no order
        cut = {1} if len(cases) > 1 else set()
        lp, labels, act, lls = align_cases.assemble(cases, act_override={b: 0 for b in cut})
        res = ctc.ctc_viterbi_align_batch(torch.from_numpy(lp), torch.from_numpy(labels), act, lls,
                                          **align_cases.flags(cases[0]))
        cost, frames, states, segments = align_cases.want(cases, lp.shape[0], max(lls), infeasible=cut)
        assert res.cost.dtype == torch.float64 and res.frames.dtype == torch.int32
        assert (res.cost.numpy() == cost).all(), key
        assert (res.feasible.numpy() == np.isfinite(cost)).all()
        assert (res.frames.numpy() == frames).all() and (res.states.numpy() == states).all(), key
        assert (res.segments.numpy() == segments).all(), key
        for b, c in enumerate(cases):
            if b in cut:
                continue
            one_cost, one_sol = _align(c)
            assert np.float64(one_cost) == res.cost[b].item()
            if c['feasible']:
                assert (one_sol.numpy() == res.frames[b, :c['T']].numpy()).all()


def test_batch_entry_large_boundary_cases_on_cpu():
    ctc = _ctc()
    for name in ('edge_mono_L511_T1100', 'edge_mono_L127_T769', 'edge_mono_L128'):
        c = align_cases.case(name)
        lp, labels, act, lls = align_cases.assemble([c])
        res = ctc.ctc_viterbi_align_batch(torch.from_numpy(lp), torch.from_numpy(labels), act, lls,
                                          **align_cases.flags(c))
        cost, frames, states, segments = align_cases.want([c], c['T'], c['L'])
        assert (res.cost.numpy() == cost).all() and (res.frames.numpy() == frames).all()
        assert (res.states.numpy() == states).all() and (res.segments.numpy() == segments).all()


def test_alignment_properties_of_every_feasible_case():
    ctc = _ctc()
    checked = 0
    for key, cases in _groups().items():
        lp, labels, act, lls = align_cases.assemble(cases)
        res = ctc.ctc_viterbi_align_batch(torch.from_numpy(lp), torch.from_numpy(labels), act, lls,
                                          **align_cases.flags(cases[0]))
        for b, c in enumerate(cases):
            if not c['feasible']:
                assert not res.feasible[b] and (res.states[b] == -1).all()
                continue
            checked += 1
            T, L = c['T'], c['L']
            states = res.states[b, :T].tolist()
            frames = res.frames[b, :T].tolist()
            # dropping blanks and merged repeats from the state path gives back the transcript
            visited = [s for s, _ in itertools.groupby(states) if s % 2 == 1]
            assert visited == [2 * i + 1 for i in range(L)]
            assert [int(c['labels'][s // 2]) for s in visited] == c['labels'].tolist()
            # the segments partition the label frames, in order
            seg = res.segments[b, :L].tolist()
            label_frames = [t for t, s in enumerate(states) if s % 2 == 1]
            assert [t for s0, s1 in seg for t in range(s0, s1)] == label_frames
            assert all(s0 < s1 for s0, s1 in seg)
            assert all(states[t] == 2 * i + 1 for i, (s0, s1) in enumerate(seg) for t in range(s0, s1))
            # cost = minus the fp64 sum of lp along the path, added in time order
            total = np.float64(0.0)
            for t, k in enumerate(frames):
                total = total + np.float64(c['lp'][t, k])
            assert res.cost[b].item() == -total
            spans = ctc.alignment_spans(res, labels, lls)[b]
            assert [s[0] for s in spans] == c['labels'].tolist() and [list(s[1:]) for s in spans] == seg
    assert checked > 150


def test_native_switch_is_read_per_call(monkeypatch):
    ctc = _ctc()
    monkeypatch.setenv('ASR_ALIGN_NATIVE', '0')
    assert not ctc._align_native_enabled()
    monkeypatch.setenv('ASR_ALIGN_NATIVE', '1')
    assert ctc._align_native_enabled()
    monkeypatch.delenv('ASR_ALIGN_NATIVE')
    assert ctc._align_native_enabled()


def test_align_entry_points_are_declared_bound_and_check_their_arguments():
    from att_speech import _native
    text = open(os.path.join(ROOT, 'include', 'asr_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('asr_ctc_align_supported', 'asr_ctc_align_workspace_bytes', 'asr_ctc_align_f64'):
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _native._SIGNATURES
    L = _native.lib()
    assert L.asr_ctc_align_supported(334, 100, 49) == 1 and L.asr_ctc_align_supported(1100, 511, 7) == 1
    assert L.asr_ctc_align_supported(600, 512, 7) == 0 and L.asr_ctc_align_supported(0, 4, 7) == 0
    # back-pointers: one byte per four states and frame, in LDS up to 48 KiB per utterance
    assert L.asr_ctc_align_workspace_bytes(768, 3, 127) == 0
    assert L.asr_ctc_align_workspace_bytes(769, 3, 127) == 3 * 769 * 64
    assert L.asr_ctc_align_workspace_bytes(1100, 2, 511) == 2 * 1100 * 256
    args = (None, None, None, None, 2, 10, 7, 3, 7, 1, 1, 0, None, None, None, None, None, 0, None)
    assert L.asr_ctc_align_f64(*args) == _native.ASR_EINVAL                      # null pointers
    bad_order = args[:9] + (3,) + args[10:]
    assert L.asr_ctc_align_f64(*bad_order) == _native.ASR_EINVAL
    too_long = args[:7] + (512,) + args[8:]
    assert L.asr_ctc_align_f64(*too_long) == _native.ASR_EUNSUPPORTED
    empty = args[:4] + (0,) + args[5:]
    assert L.asr_ctc_align_f64(*empty) == _native.ASR_OK
    narrow = args[:6] + (24, 3, 5, 2) + args[10:]                                # S * S > C
    assert L.asr_ctc_align_f64(*narrow) == _native.ASR_EINVAL
