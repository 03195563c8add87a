"""The native scorer on the MI355X: asr_edit_distance_stats_i32 (csrc/edit_distance.hip) against
the reference's recorded results and against the host implementation, and do_evaluate on real
models with the native scorer and with ASR_NATIVE_SCORING=0.  Everything compared here is an
integer, or a float computed from the same integers in the same order: all comparisons are
exact."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_modules import ENC, VOCAB, sample_batch  # noqa: E402
from test_scoring import Loader, stored_pairs, wsj_dataset  # noqa: E402


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def launch(pairs, max_x=None, max_y=None):
    """the kernel through _native.edit_distance_stats -> int64 numpy [n, 4]"""
    from att_speech import _native
    lx, ly = [len(x) for x, _ in pairs], [len(y) for _, y in pairs]

    def i32(a):
        return torch.tensor(np.asarray(a, np.int32), dtype=torch.int32, device=dev())
    out = _native.edit_distance_stats(
        i32([t for x, _ in pairs for t in x]), i32(np.concatenate([[0], np.cumsum(lx)])),
        i32([t for _, y in pairs for t in y]), i32(np.concatenate([[0], np.cumsum(ly)])),
        max(lx) if max_x is None else max_x, max(ly) if max_y is None else max_y)
    return out.cpu().numpy().astype(np.int64)


def host(pairs):
    from att_speech import utils
    out = np.zeros((len(pairs), 4), np.int64)
    for p, (x, y) in enumerate(pairs):
        dist, ops = utils.edit_distance_with_stats(x, y)
        out[p] = (dist, ops['ins'], ops['del'], ops['sub'])
    return out


def seeded_batch():
    from att_speech import _native
    limit = _native.edit_distance_max_len()
    rng = np.random.RandomState(4242)

    def seq(n, a):
        return rng.randint(0, a, size=n).tolist()
    pairs = []
    for p in range(512 - 12):
        a = (2, 3, 5, 47)[p % 4]
        pairs.append((seq(rng.randint(0, 601), a), seq(rng.randint(0, 601), a)))
    pairs += [([], []), ([], seq(300, 3)), (seq(300, 3), []),
              (seq(100, 2), seq(64, 2)), (seq(100, 2), seq(65, 2)), (seq(100, 2), seq(128, 2)),
              (seq(64, 3), seq(64, 3)), (seq(65, 3), seq(129, 3)), (seq(600, 2), seq(600, 2)),
              (seq(limit, 5), seq(limit, 5)), (seq(limit, 2), seq(7, 2)), (seq(3, 2), seq(limit, 2))]
    assert len(pairs) == 512
    return pairs, limit


def test_kernel_equals_the_reference_on_every_stored_pair():
    pairs, want = stored_pairs()
    got = launch(pairs)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, [(int(p), got[p].tolist(), want[p].tolist()) for p in bad[:5]]


def test_kernel_equals_the_host_on_a_seeded_batch_up_to_the_limit():
    pairs, limit = seeded_batch()
    got = launch(pairs)
    want = host(pairs)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, [(int(p), len(pairs[p][0]), len(pairs[p][1]), got[p].tolist(),
                            want[p].tolist()) for p in bad[:5]]
    assert (got[:, 0] == got[:, 1:].sum(1)).all()
    assert max(len(x) for x, _ in pairs) == limit == max(len(y) for _, y in pairs)


def test_repeated_launches_are_bit_identical():
    pairs, _ = stored_pairs()
    first = launch(pairs)
    for _ in range(3):
        assert (launch(pairs) == first).all()


def test_a_pair_longer_than_the_launch_bounds_is_flagged_not_computed():
    pairs = [([1, 2, 3], [1, 3]), ([1] * 9, [1] * 2), ([1], [2] * 9)]
    got = launch(pairs, max_x=4, max_y=4)
    assert got.tolist() == [[1, 1, 0, 0], [-1] * 4, [-1] * 4]


def test_over_the_limit_the_entry_refuses_and_the_wrapper_takes_the_host():
    from att_speech import _native, utils
    limit = _native.edit_distance_max_len()
    z = torch.zeros(4, dtype=torch.int32, device=dev())
    code = _native.lib().asr_edit_distance_stats_i32(
        _native._p(z), _native._p(z), _native._p(z), _native._p(z), 1, limit + 1, 1,
        _native._p(z), _native._stream())
    assert code == _native.ASR_EINVAL
    with pytest.raises(AssertionError):
        _native.edit_distance_stats(z, z[:2], z, z[:2], limit + 1, 1)
    rng = np.random.RandomState(1)
    hyps = [rng.randint(0, 3, size=limit + 1).tolist(), [1, 2]]
    refs = [rng.randint(0, 3, size=40).tolist(), [2, 2]]
    utils._SCORING_WARNED.clear()
    with pytest.warns(UserWarning, match='scored on the host'):
        got = utils.score_pairs(hyps, refs, device=dev())
    with warnings.catch_warnings():           # one warning only
        warnings.simplefilter('error')
        again = utils.score_pairs(hyps, refs, device=dev())
    assert (got == host(list(zip(hyps, refs)))).all() and (got == again).all()
    assert (utils.score_pairs(hyps[1:], refs[1:], device=dev()) == got[1:]).all()


def test_score_pairs_on_the_device_equals_the_host_for_words():
    from att_speech import utils
    hyps = ['the cat sat on mat'.split(), [], 'a b c'.split(), list('kitten')]
    refs = ['the cat sat on the mat'.split(), ['x'], 'a b c'.split(), list('sitting')]
    got = utils.score_pairs(hyps, refs, device=dev())
    assert got.dtype == np.int64 and (got == utils.score_pairs(hyps, refs)).all()
    assert got.tolist()[0] == [1, 0, 1, 0] and got.tolist()[3][0] == 3


class EvalDataset(object):
    """ids -> characters through the WSJ symbols; ids past the table (an EOS class) print as '>'"""

    def __init__(self):
        self.inner = wsj_dataset()

    def ids_to_chars_words_sentence(self, text_ids, ignore_noise=False):
        return self.inner.ids_to_chars_words_sentence(
            [min(int(i), 47) for i in text_ids], ignore_noise=ignore_noise)


def eval_loader(batches=2, B=6, T=120, L=14, seed=3):
    g = torch.Generator().manual_seed(seed)
    out = []
    for j in range(batches):
        lens = torch.tensor([T - 9 * b for b in range(B)], dtype=torch.int32)
        llens = torch.tensor([max(2, L - 2 * b) for b in range(B)], dtype=torch.int32)
        texts = torch.randint(2, 49, (B, L), generator=g, dtype=torch.int32)
        texts[:, 3::4] = 2                     # spaces: several words per utterance
        out.append({'uttids': ['u%d_%d' % (j, b) for b in range(B)], 'spkids': None,
                    'features': (torch.randn(B, T, 40, 1, generator=g), lens),
                    'texts': (texts, llens), 'ivectors': None})
    loader = Loader(out)
    loader.dataset = EvalDataset()
    return loader


def run_both_ways(model, loader, monkeypatch):
    """do_evaluate with the native scorer and on the host, with and without a callback"""
    from att_speech import _native, utils
    results = {}
    launches = []
    real = _native.edit_distance_stats
    monkeypatch.setattr(_native, 'edit_distance_stats',
                        lambda *a, **kw: (launches.append(1), real(*a, **kw))[1])
    for path in ('native', 'host'):
        monkeypatch.setenv('ASR_NATIVE_SCORING', '1' if path == 'native' else '0')
        rows = []
        with_cb = utils.do_evaluate(loader, model, output_callback=lambda **kw: rows.append(kw))
        results[path] = (with_cb, rows, utils.do_evaluate(loader, model))
    assert len(launches) == 2 * len(loader)           # one launch per batch, none on the host path
    (sn, rn, sn2), (sh, rh, sh2) = results['native'], results['host']
    assert set(sn) == set(sh) and {'WER', 'CER', 'len_ratio', 'loss'} <= set(sn)
    for k in sn:
        assert float(sn[k]) == float(sh[k]) == float(sn2[k]) == float(sh2[k]), k
    assert len(rn) == len(rh) == sum(len(b['uttids']) for b in loader)
    for a, b in zip(rn, rh):
        assert set(a) == set(b)
        for k in a:
            if k == 'other':
                assert set(a[k]) == set(b[k])
                for kk in a[k]:
                    assert np.array_equal(np.asarray(a[k][kk]), np.asarray(b[k][kk])), (a['uttid'], kk)
            else:
                assert a[k] == b[k], (a['uttid'], k, a[k], b[k])
    return sn, rn


def test_do_evaluate_ctc_model_native_scoring_equals_the_host(monkeypatch):
    from att_speech.models import SpeechModel
    torch.manual_seed(2)
    dec = dict(class_name='att_speech.modules.decoders.advanced_decoder.CTCDecoderAdvanced')
    model = SpeechModel(ENC, dec, sample_batch(B=2, T=120), 49, VOCAB).to(dev())
    summary, rows = run_both_ways(model, eval_loader(), monkeypatch)
    assert not model.training and set(summary) == {'ctc_loss', 'loss', 'WER', 'CER', 'len_ratio'}
    assert all(r['other'] == {} and r['text_loss'] is None for r in rows)
    assert all(r['wer_stat'].keys() == {'ins', 'del', 'sub'} for r in rows)


def test_do_evaluate_attention_rnn_decode_carries_decoded_scores(monkeypatch):
    from att_speech.models import SpeechModel
    torch.manual_seed(4)
    dec = dict(class_name='att_speech.modules.decoders.attention_decoder.AttentionDecoderRNN',
               n_layers=1, hidden_size=64, dropout_p=0.0, beam_size=1, length_normalization=0.6)
    model = SpeechModel(ENC, dec, sample_batch(B=2, T=120), 49, VOCAB).to(dev())
    with torch.no_grad():
        model.decoder.attn.hidden_to_score.weight.normal_(0.0, 0.5)
        model.decoder.embedding.weight.mul_(2.0)
        model.decoder.output_to_logits.weight.mul_(5.0)
        model.decoder.output_to_logits.bias[49] += 3.0       # EOS early: hypotheses finish
    model.decoder.TRANSCRIPTION_LEN_GUARD = 30
    summary, rows = run_both_ways(model, eval_loader(batches=1, B=4), monkeypatch)
    assert rows[0]['other'] and set(summary) == {'loss', 'WER', 'CER', 'len_ratio'}
