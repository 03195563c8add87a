"""The evaluation surface of att_speech.utils without a GPU: the host edit distance with operation
counts, RunningStatistics, uniq, LogitsDumper and do_evaluate against what the reference's own
functions recorded (tests/golden/scoring.npz, written by tests/golden/make_golden_scoring.py),
and the argument checks of the native scorer's entry points."""
import ctypes
import json
import os
import random
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden


def stored_pairs():
    g = golden('scoring.npz')
    xo, yo = g['pairs_x_off'], g['pairs_y_off']
    x, y = g['pairs_x'], g['pairs_y']
    pairs = [(x[xo[p]:xo[p + 1]].tolist(), y[yo[p]:yo[p + 1]].tolist()) for p in range(len(xo) - 1)]
    return pairs, g['pairs_want']


def wsj_dataset():
    """the tokeniser contract of do_evaluate: `loader.dataset.ids_to_chars_words_sentence` of
    the WSJ recipes (drops '~' with ignore_noise, words = the sentence split at white space)"""
    symbols = open(os.path.join(GOLDEN, 'wsj_vocabulary.txt')).read().split('\n')[:-1]
    assert len(symbols) == 49 and symbols[2] == ' '

    class Dataset(object):
        def ids_to_chars_words_sentence(self, text_ids, ignore_noise=False):
            shown = [symbols[int(i)] for i in text_ids]
            if ignore_noise:
                shown = [c for c in shown if c != '~']
            text = ''.join(shown)
            return shown, text.split(), text
    return Dataset()


class Loader(list):
    dataset = None


def recorded_run():
    ev = json.loads(str(golden('scoring.npz')['eval_json']))
    batches = []
    for rec in ev['batches']:
        nb = len(rec['uttids'])
        batches.append({
            'uttids': rec['uttids'], 'spkids': ['spk%d' % i for i in range(nb)],
            'features': (torch.zeros(nb, 40, 2, 1), torch.tensor(rec['feature_lens'], dtype=torch.int32)),
            'texts': (torch.tensor(rec['texts'], dtype=torch.int32),
                      torch.tensor(rec['text_lens'], dtype=torch.int32)),
            'ivectors': None, 'graph_matrices': ['stub']})
    loader = Loader(batches)
    loader.dataset = wsj_dataset()
    return ev, loader


class StubModel(torch.nn.Module):
    """`decode` returns the recorded label lists and losses, batch after batch"""

    def __init__(self, recorded):
        super(StubModel, self).__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.recorded, self.calls, self.seen = recorded, 0, []

    def decode(self, features, feature_lens, speakers, texts=None, text_lens=None,
               encoder_args=None, decoder_args=None, ivectors=None, **kwargs):
        self.seen.append((sorted(kwargs), encoder_args, decoder_args, self.training,
                          features.device.type))
        rec = self.recorded[self.calls % len(self.recorded)]
        self.calls += 1
        loss = rec['loss']
        dev = self.w.device
        loss = ({k: torch.tensor(v, dtype=torch.float32, device=dev) for k, v in loss.items()}
                if isinstance(loss, dict) else torch.tensor(loss, dtype=torch.float32, device=dev))
        ret = {'decoded': rec['decoded'], 'loss': loss}
        if 'decoded_scores' in rec:
            ret['decoded_scores'] = rec['decoded_scores']
        if decoder_args:
            nb = len(rec['decoded'])
            ret.update(text_loss=[1.5 + i for i in range(nb)], generated_loss=[2.5 + i for i in range(nb)],
                       logits_text_diff=[7 - i for i in range(nb)])
        return ret


def check_against_recorded(ev, summary, rows):
    assert set(summary) == set(ev['summary']) == {'ctc_loss', 'loss', 'WER', 'CER', 'len_ratio'}
    for k, want in ev['summary'].items():
        assert abs(float(summary[k]) - want) <= 1e-12 * abs(want), (k, summary[k], want)
    assert len(rows) == len(ev['rows']) == sum(len(b['uttids']) for b in ev['batches'])
    for got, want in zip(rows, ev['rows']):
        assert set(got) == {'uttid', 'recognized', 'original', 'wer', 'cer', 'wer_stat', 'cer_stat',
                            'text_loss', 'other', 'generated_loss', 'logits_text_diff'}
        for k in ('uttid', 'recognized', 'original', 'wer_stat', 'cer_stat', 'other', 'text_loss',
                  'generated_loss', 'logits_text_diff'):
            assert got[k] == want[k], (got['uttid'], k, got[k], want[k])
        for k in ('wer', 'cer'):
            assert float(got[k]) == want[k], (got['uttid'], k)


def test_host_edit_distance_equals_the_reference_on_every_stored_pair():
    from att_speech import utils
    pairs, want = stored_pairs()
    assert len(pairs) >= 300
    assert max(max(len(x), len(y)) for x, y in pairs) >= 300
    for p, (x, y) in enumerate(pairs):
        dist, ops = utils.edit_distance_with_stats(x, y)
        assert (dist, ops['ins'], ops['del'], ops['sub']) == tuple(want[p].tolist()), (p, x, y)
        assert set(ops) == {'ins', 'del', 'sub'}


def test_counts_add_up_and_the_distance_is_the_plain_one():
    from att_speech import utils
    pairs, _ = stored_pairs()
    for x, y in pairs:
        dist, ops = utils.edit_distance_with_stats(x, y)
        assert dist == ops['ins'] + ops['del'] + ops['sub']
        assert dist == utils.edit_distance(x, y)
    got = utils.score_pairs([x for x, _ in pairs], [y for _, y in pairs])
    assert got.shape == (len(pairs), 4) and (got[:, 0] == got[:, 1:].sum(1)).all()


def traceback_stats(x, y):
    """the straightforward form: full distance and operation matrices, first minimum in the order
    up / left / diagonal, then the walk back from the corner counting the moves that cost"""
    n, m = len(x), len(y)
    dp = [[0] * (m + 1) for _ in range(n + 1)]
    op = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        dp[i][0], op[i][0] = i, 0
    for j in range(m + 1):
        dp[0][j], op[0][j] = j, 1
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            cands = (dp[i - 1][j] + 1, dp[i][j - 1] + 1, dp[i - 1][j - 1] + (x[i - 1] != y[j - 1]))
            op[i][j] = min(range(3), key=lambda k: (cands[k], k))
            dp[i][j] = cands[op[i][j]]
    counts = [0, 0, 0]
    i, j = n, m
    while i > 0 or j > 0:
        k = 0 if j == 0 else 1 if i == 0 else op[i][j]
        ni, nj = (i if k == 1 else i - 1), (j if k == 0 else j - 1)
        if dp[i][j] > dp[ni][nj]:
            counts[k] += 1
        i, j = ni, nj
    return dp[n][m], {'ins': counts[0], 'del': counts[1], 'sub': counts[2]}


def test_carry_forward_equals_the_trace_back_on_two_symbol_alphabets():
    from att_speech import utils
    rnd = random.Random(5)
    for _ in range(300):
        x = [rnd.randrange(2) for _ in range(rnd.randint(0, 40))]
        y = [rnd.randrange(2) for _ in range(rnd.randint(0, 40))]
        assert utils.edit_distance_with_stats(x, y) == traceback_stats(x, y), (x, y)


def test_any_hashables_and_word_error_rate():
    from att_speech import utils
    hyp, ref = 'the cat sat on mat'.split(), 'the cat sat on the mat'.split()
    assert utils.edit_distance_with_stats(hyp, ref) == (1, {'ins': 0, 'del': 1, 'sub': 0})
    assert utils.edit_distance_with_stats([(1, 2), 'a', None], [(1, 2), 'b', None, 4.5]) == (
        2, {'ins': 0, 'del': 1, 'sub': 1})
    assert utils.word_error_rate(ref, hyp) == 1.0 / 6
    got = utils.score_pairs([hyp, [], 'abc'], [ref, ['x'], 'abc'])
    assert got.dtype == np.int64 and got.tolist() == [[1, 0, 1, 0], [1, 0, 1, 0], [0, 0, 0, 0]]
    with pytest.raises(ValueError):
        utils.score_pairs([hyp], [])


def test_running_statistics_and_uniq_match_the_reference():
    from att_speech import utils
    g = golden('scoring.npz')
    rs = utils.RunningStatistics()
    assert rs.variance() == float(g['rs_empty_variance']) == 0.0
    pos = 0
    for c, mean, var in zip(g['rs_chunks'], g['rs_means'], g['rs_variances']):
        rs.add(g['rs_series'][pos:pos + c])
        pos += c
        assert float(rs.mean()) == mean and float(rs.variance()) == var
    assert g['rs_variances'][0] == 0.0          # one sample
    assert utils.uniq(g['uniq_in'].tolist()) == [tuple(r) for r in g['uniq_out'].tolist()]
    assert utils.uniq([]) == [] and utils.uniq([4, 4]) == [(0, 2)] and utils.uniq([7]) == [(0, 1)]


def test_do_evaluate_reproduces_the_recorded_run():
    from att_speech import utils
    ev, loader = recorded_run()
    model, rows = StubModel(ev['batches']), []
    progress = []
    summary = utils.do_evaluate(loader, model, output_callback=lambda **kw: rows.append(kw),
                                progress_callback=lambda *a: progress.append(a))
    check_against_recorded(ev, summary, rows)
    assert progress == [(j, 3, len(b['uttids'])) for j, b in enumerate(ev['batches'])]
    # every batch key but features / texts / spkids / uttids / ivectors goes to decode
    assert [s[:3] for s in model.seen] == [(['graph_matrices'], None, None)] * 3
    # without a callback: the same summary
    again = utils.do_evaluate(loader, StubModel(ev['batches']))
    assert {k: float(v) for k, v in again.items()} == {k: float(v) for k, v in summary.items()}


def test_do_evaluate_generate_data_losses_call_form():
    from att_speech import utils
    ev, loader = recorded_run()
    model, rows = StubModel(ev['batches']), []
    utils.do_evaluate(loader, model, output_callback=lambda **kw: rows.append(kw),
                      generate_data_losses=True)
    assert model.seen[0][1] == {} and model.seen[0][2] == {
        'return_texts_and_generated_loss': True, 'return_logits_text_diff': True}
    assert [r['text_loss'] for r in rows[:4]] == [1.5, 2.5, 3.5, 4.5]
    assert rows[1]['generated_loss'] == 3.5 and rows[1]['logits_text_diff'] == 6


def test_do_evaluate_does_not_hide_an_empty_reference():
    from att_speech import utils
    ev, loader = recorded_run()
    loader[0]['texts'][1][1] = 0
    with pytest.raises(ZeroDivisionError):
        utils.do_evaluate(loader, StubModel(ev['batches']))


def test_print_num_samples_prints_reference_and_frames(capsys):
    from att_speech import utils
    ev, loader = recorded_run()

    class WithFrames(StubModel):
        def decode(self, *a, **kw):
            ret = StubModel.decode(self, *a, **kw)
            ret['decoded_frames'] = [[0, 0, 5, 5, 0, 4], [0, 9, 0, 0, 0, 0], [6, 0, 0, 0, 0, 0]]
            return ret
    utils.do_evaluate(loader, WithFrames(ev['batches']), print_num_samples=2)
    out = capsys.readouterr().out.splitlines()
    assert out == ['Ref:     THE QUICK BROWN FOX', 'Decode:  ' + chr(176) * 2 + 'AA' + chr(176) + 'T',
                   'Ref:     A ~ NOISY LINE ~', 'Decode:  ' + chr(176) + 'S' + chr(176) * 4]


def test_evaluate_greedy_sets_the_module_mode():
    from att_speech import utils
    ev, loader = recorded_run()
    model = StubModel(ev['batches'])
    model.train()
    a = utils.evaluate_greedy(loader, model)
    assert not model.training and [s[3] for s in model.seen] == [False] * 3
    b = utils.evaluate_greedy_in_train_mode(loader, model)
    assert model.training and [s[3] for s in model.seen[3:]] == [True] * 3
    assert a == b and set(a) == set(ev['summary'])


def test_polyak_post_dev_eval_takes_evaluate_greedy():
    from att_speech import utils
    from att_speech.modules.hooks.polyak import PolyakDecay
    ev, loader = recorded_run()
    model = StubModel(ev['batches'])
    hook = PolyakDecay([0.5])
    hook.pre_run(model, None)
    logged = {}
    logger = types.SimpleNamespace(make_step_log=lambda *a: None, end_log=lambda: None,
                                   log_scalar=lambda k, v: logged.__setitem__(k, float(v)))
    hook.post_dev_eval(model, 1, logger, 'dir', loader, evaluate=utils.evaluate_greedy)
    assert abs(logged['_CER'] - ev['summary']['CER']) <= 1e-12 and '_WER' in logged


def test_logits_dumper_round_trip(tmp_path):
    from att_speech import ctc_forward, utils
    rng = np.random.default_rng(0)
    dumper = utils.LogitsDumper(str(tmp_path / 'logits'), 1200)
    dumper.start()
    a = torch.from_numpy(rng.standard_normal((5, 3, 4)).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal((6, 2, 4)).astype(np.float32))
    dumper.add_batch(['u3', 'u1', 'u2'], a)
    assert os.path.exists(str(tmp_path / 'logits' / '1200.ark.temp'))
    dumper.add_batch(['u5', 'u4'], b)
    dumper.end()
    assert sorted(os.listdir(str(tmp_path / 'logits'))) == ['1200.ark']
    got = ctc_forward.read_kaldi_float_matrices(str(tmp_path / 'logits' / '1200.ark'))
    assert list(got) == ['u1', 'u2', 'u3', 'u4', 'u5']          # sorted ids within each batch
    np.testing.assert_array_equal(got['u3'], a[:, 0].numpy())
    np.testing.assert_array_equal(got['u1'], a[:, 1].numpy())
    np.testing.assert_array_equal(got['u4'], b[:, 1].numpy())


def test_do_evaluate_feeds_the_logits_dumper(tmp_path):
    from att_speech import ctc_forward, utils
    ev, loader = recorded_run()

    class WithLogits(StubModel):
        def decode(self, features, *a, **kw):
            ret = StubModel.decode(self, features, *a, **kw)
            ret['logits'] = torch.full((3, features.size(0), 2), float(self.calls))
            return ret
    utils.do_evaluate(loader, WithLogits(ev['batches']),
                      logits_dumper=utils.LogitsDumper(str(tmp_path), 7))
    got = ctc_forward.read_kaldi_float_matrices(str(tmp_path / '7.ark'))
    assert len(got) == len(ev['rows']) and got['utt2_0'].shape == (3, 2) and got['utt2_0'][0, 0] == 3.0


def test_host_scoring_on_the_cpu_and_with_the_switch(monkeypatch):
    """a model on the CPU never reaches the library; ASR_NATIVE_SCORING is read per call"""
    from att_speech import utils
    assert not utils._native_scoring(torch.device('cpu')) and not utils._native_scoring(None)
    monkeypatch.setenv('ASR_NATIVE_SCORING', '0')
    assert not utils._native_scoring(torch.device('cuda:0'))


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from att_speech import _native
    L = _native.lib()
    limit = L.asr_edit_distance_max_len()
    assert limit >= 4096 and _native.edit_distance_max_len() == limit
    buf = ctypes.create_string_buffer(256)
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    call = L.asr_edit_distance_stats_i32
    assert call(ptr, ptr, ptr, ptr, -1, 4, 4, ptr, None) == _native.ASR_EINVAL
    assert call(ptr, ptr, ptr, ptr, 2, -1, 4, ptr, None) == _native.ASR_EINVAL
    assert call(ptr, ptr, ptr, ptr, 2, 4, -1, ptr, None) == _native.ASR_EINVAL
    assert call(ptr, ptr, ptr, ptr, 2, limit + 1, 4, ptr, None) == _native.ASR_EINVAL
    assert call(ptr, ptr, ptr, ptr, 2, 4, limit + 1, ptr, None) == _native.ASR_EINVAL
    for null in (0, 1, 2, 3, 7):
        a = [ptr, ptr, ptr, ptr, 2, 4, 4, ptr, None]
        a[null] = None
        assert call(*a) == _native.ASR_EINVAL, null
    assert call(None, None, None, None, 0, 0, 0, None, None) == _native.ASR_OK     # nothing to do
    with pytest.raises(_native.NativeLibraryError):
        z = torch.zeros(2, dtype=torch.int32)
        _native.edit_distance_stats(z, z, z, z, 0, 0)
    assert 'asr_edit_distance_stats_i32' in _native._SIGNATURES
    assert b'invalid' in L.asr_strerror(call(ptr, ptr, ptr, ptr, 1, limit + 1, 0, ptr, None))
