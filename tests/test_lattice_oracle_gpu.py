"""asr_lattice_oracle_i32 (csrc/lattice_oracle.hip) through DeviceLatticeBatch.oracle: everything the device
returns (errors, the four counts, words, ref_frames, cost) equals LatticeBatch.oracle with ==: the distances
are int32 and the cost is summed in the twin's order, so no schedule can change them.  Every device case asserts
that the kernel was launched (batch.launches)."""
import warnings
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import mbr_cases as MC
import nbest_cases as NC
from wfst_cases import INF, TOYS, grid_scores, toy_graph

from att_speech import lattice_dp
from att_speech.lattice_dp import DeviceLatticeBatch, decode_lattice_device
from att_speech.wfst_lattice import ORACLE_NONE, LatticeBatch, oracle_error_rate

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device('cuda:0')


@contextmanager
def quiet():
    """no warning from the package inside"""
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        yield
    ours = [str(w.message) for w in rec if 'att_speech' in (w.filename or '') or 'oracle' in str(w.message)]
    assert ours == [], ours


def device_oracle(batch, refs, *args, launches=1, **kw):
    assert batch.device.type == 'cuda'
    batch.launches = 0
    with quiet():
        got = batch.oracle(refs, *args, **kw)
    assert batch.launches > 0 and (launches is None or batch.launches == launches), batch.launches
    return got


def check(batch, refs, *args, host=None, launches=1, **kw):
    """the device against the twin: every field, =="""
    host = LatticeBatch(batch.lattices()) if host is None else host
    want = host.oracle(refs, *args)
    got = device_oracle(batch, refs, *args, launches=launches, **kw)
    assert len(got) == len(want) == batch.num_utterances
    for b, (x, y) in enumerate(zip(got, want)):
        assert x == y, (args, b, refs[b], x, y)
        assert type(x.errors) is int and type(x.cost) is float and all(type(w) is int for w in x.words)
    return got


def reference_sets(host, seed, top=8):
    """per utterance: its best sentence, that sentence damaged, random labels, nothing"""
    rng = np.random.default_rng(seed)
    best = [list(w) for w, _, _, _ in host.best_paths()]
    damaged = [s[1:] + rng.integers(1, top, 2).tolist() for s in best]
    random = [rng.integers(1, top, int(rng.integers(0, 7))).tolist() for _ in best]
    return [best, damaged, random, [[] for _ in best]]


def sized(sentence, R, filler=5):
    """the sentence padded with itself (or a filler) or cut to exactly R labels"""
    out = list(sentence)
    while len(out) < R:
        out += list(sentence) if sentence else [filler]
    return out[:R]


@pytest.mark.parametrize('name', sorted(TOYS))
def test_toy_sweep(name):
    """from the device search and from uploaded host lattices; utterance 1 of toys b and c is partial"""
    g, lp = NC.toy_inputs(name)
    x = torch.from_numpy(lp).to(dev())
    for _, scale, lb in [c for c in MC.toy_sweep() if c[0] == name]:
        lats, _ = NC.toy_lattices(name, scale, lb)
        host = LatticeBatch(lats)
        with quiet():
            made, redone = decode_lattice_device(x, NC.LENS, g, beam=INF, lattice_beam=lb, acoustic_scale=scale)
            uploaded = DeviceLatticeBatch.from_lattices(lats, dev())
        assert redone == []
        for refs in reference_sets(host, len(name)):
            got = check(made, refs, host=host)
            assert check(uploaded, refs, host=host) == got
        rescaled = check(made, reference_sets(host, 1)[0], 0.5, 2.0, host=host)
        assert all(r.errors == 0 for r in rescaled)     # the best sentence is in the lattice at any scale
        assert made.depth() == host.depth() == uploaded.depth()


def test_empty_and_partial_utterances_inside_a_batch():
    g = toy_graph('c')
    lens = [1, 5, 2]
    lp = torch.from_numpy(grid_scores(np.random.default_rng(4), 5, 3, 3, lens, low=-4.0)).to(dev())
    with quiet():
        gone, _ = decode_lattice_device(lp, lens, g, beam=INF, lattice_beam=2.0, allow_partial=False)
        partial, _ = decode_lattice_device(lp, lens, g, beam=INF, lattice_beam=2.0, allow_partial=True)
        mixed = DeviceLatticeBatch.from_lattices([gone.lattices()[0], gone.lattices()[1], partial.lattices()[2]],
                                                 dev())
        silent = DeviceLatticeBatch.from_lattices([NC.without_words(gone.lattices()[1])], dev())
        nothing = DeviceLatticeBatch.from_lattices([gone.lattices()[0]], dev())
    refs = [[1, 2], [2, 1, 3, 1], [3]]
    for batch, empty in ((gone, [0, 2]), (mixed, [0]), (partial, [])):
        got = check(batch, refs)
        assert [b for b, r in enumerate(got) if r == ORACLE_NONE] == empty
        assert oracle_error_rate(got, refs).skipped == len(empty)
        assert batch.depth() == LatticeBatch(batch.lattices()).depth()
        assert [d == 0.0 for d in batch.depth()] == [b in empty for b in range(3)]
    res = check(silent, [[4, 4]])[0]
    assert res.words == [] and res.errors == res.deletions == 2 and res.ref_frames == [-1, -1]
    assert nothing.oracle([[1]]) == [ORACLE_NONE] and nothing.launches == 0


@pytest.mark.parametrize('R', [0, 1, 63, 64, 65, 130])
def test_slot_round_boundaries(R):
    """R + 1 = 64 columns is one round of a wave, 65 two with a carry, 131 three"""
    lats = MC.long_lattices()
    with quiet():
        batch = DeviceLatticeBatch.from_lattices(lats, dev())
    host = LatticeBatch(lats)
    sents = batch.sentences(3)
    for i in range(3):
        refs = [sized(s[min(i, len(s) - 1)], R) for s in sents]
        assert all(len(r) == R for r in refs)
        got = check(batch, refs, host=host)
        whole = sents[0][min(i, len(sents[0]) - 1)]
        if R <= len(whole):
            assert got[0].errors <= len(whole) - R      # a prefix of a sentence of the lattice
    refs = [sized(s[0][::-1], R) for s in sents]
    check(batch, refs, 0.5, 2.0, host=host)


def test_fan_lattice():
    """3000 in-arcs at one node: taken in turn by one wave forwards, 64 at a time by ballot backwards"""
    lat = NC.fan_lattice()
    with quiet():
        batch = DeviceLatticeBatch.from_lattices([lat, lat], dev())
    assert int((batch.in_ptr[1:] - batch.in_ptr[:-1]).max()) >= 3000
    host = LatticeBatch([lat, lat])
    sents = lat.sentences(4)
    for refs in ([sents[0], sents[3]], [sents[1][::-1], []], [[7, 8, 7, 8, 7], sents[2] + [99]]):
        check(batch, refs, host=host)
    got = check(batch, [sents[2], sents[2]], 0.0, 1.0, host=host)
    assert got[0] == got[1] and got[0].errors == 0


def test_large():
    """the shape of tests/test_lattice_dp_gpu.py: more than 65536 arcs in one lattice"""
    import test_lattice_dp_gpu as D
    g, lp, lens, batch = D.large()
    assert np.diff(batch.arc_off).max() > 65536
    host = LatticeBatch(batch.lattices())
    for refs in reference_sets(host, 9, top=int(g.olabel.max()) + 1)[:3]:
        got = check(batch, refs, host=host)
        assert all(r.errors >= 0 for r in got)


def test_run_to_run_and_workgroup_sizes(monkeypatch):
    lat = NC.fan_lattice()
    cases = [[lat], NC.unquantised_lattices(6.0), MC.long_lattices()]
    for lats in cases:
        with quiet():
            batch = DeviceLatticeBatch.from_lattices(lats, dev())
        host = LatticeBatch(lats)
        refs = reference_sets(host, 5, top=40)[1]
        first = check(batch, refs, host=host)
        assert device_oracle(batch, refs) == first
        for threads in (64, 128, 256):
            monkeypatch.setattr(lattice_dp, 'THREADS_PER_WORKGROUP', threads)
            assert device_oracle(batch, refs) == first, threads
        monkeypatch.setattr(lattice_dp, 'THREADS_PER_WORKGROUP', 0)


def test_chunking():
    """a workspace that does not hold all utterances: several launches, the same results"""
    lats = NC.unquantised_lattices(4.0)
    with quiet():
        batch = DeviceLatticeBatch.from_lattices(lats, dev())
    refs = reference_sets(LatticeBatch(lats), 6, top=40)[1]
    whole = check(batch, refs)
    nodes = np.diff(batch.node_off)
    per_node = 4 * (max(len(r) for r in refs) + 1)
    one_each = check(batch, refs, workspace_bytes=per_node * int(nodes.max()) + 128, launches=None)
    assert batch.launches >= 3
    pairs = check(batch, refs, workspace_bytes=per_node * int(nodes[:2].sum()) + 128, launches=None)
    assert batch.launches == 2
    assert whole == one_each == pairs
    with pytest.raises(ValueError, match='workspace_bytes'):
        batch.oracle(refs, workspace_bytes=per_node * int(nodes.max()))


def test_fallbacks(monkeypatch):
    """a reference above the device's words: the twin for that utterance, one warning"""
    lats = NC.unquantised_lattices(4.0)
    with quiet():
        batch = DeviceLatticeBatch.from_lattices(lats, dev())
    host = LatticeBatch(lats)
    refs = reference_sets(host, 8, top=40)[1]
    want = host.oracle(refs)
    assert check(batch, refs, host=host) == want
    longest = max(len(r) for r in refs)
    assert sum(len(r) == longest for r in refs) < len(refs)            # some utterances stay on the device
    cases = [(longest - 1, refs), (None, [refs[0], [3] * 1100] + refs[2:])]
    for limit, given in cases:
        if limit is not None:
            monkeypatch.setattr(lattice_dp, 'ORACLE_DEVICE_MAX_WORDS', limit)
        batch.launches = 0
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            got = batch.oracle(given)
        assert batch.launches == 1 and got == host.oracle(given)
        assert len([w for w in rec if 'redone on the host' in str(w.message)]) == 1
        monkeypatch.undo()
    assert lattice_dp.ORACLE_DEVICE_MAX_WORDS == 1023


def test_env_switch(monkeypatch):
    g, lp = NC.toy_inputs('b')
    with quiet():
        batch, _ = decode_lattice_device(torch.from_numpy(lp).to(dev()), NC.LENS, g, beam=INF, lattice_beam=INF)
    refs = reference_sets(LatticeBatch(batch.lattices()), 2)[1]
    native = device_oracle(batch, refs)
    calls = []
    real = LatticeBatch.oracle
    monkeypatch.setattr(LatticeBatch, 'oracle', lambda self, *a, **k: calls.append(a) or real(self, *a, **k))
    monkeypatch.setenv('ASR_LATTICE_ORACLE_NATIVE', '0')
    batch.launches = 0
    assert batch.oracle(refs) == native and batch.launches == 0 and len(calls) == 1
    monkeypatch.delenv('ASR_LATTICE_ORACLE_NATIVE')
    assert device_oracle(batch, refs) == native and len(calls) == 1


def test_a_malformed_batch_is_refused():
    """tensors changed behind the constructor's checks: the kernel's own range checks answer"""
    lats, _ = NC.toy_lattices('a', 1.0, 2.0)
    refs = [[1, 2, 3]] * len(lats)
    for field, index, value in (('dst', 3, 10 ** 6), ('arc', 1, 10 ** 6), ('node_level', 0, 10 ** 6),
                                ('in_ptr', 2, 10 ** 6), ('level_node', 1, 10 ** 6), ('in_arc', 1, 10 ** 6)):
        with quiet():
            batch = DeviceLatticeBatch.from_lattices(lats, dev())
        getattr(batch, field)[index] = value
        with pytest.raises(ValueError, match='inconsistent'):
            batch.oracle(refs)
        assert batch.launches == 1
    with quiet():                                       # an arc turned round: the level does not rise
        batch = DeviceLatticeBatch.from_lattices(lats, dev())
    j = int(np.nonzero(lats[0].src != lats[0].dst)[0][0])
    batch.dst[j] = batch.src[j]
    with pytest.raises(ValueError, match='inconsistent'):
        batch.oracle(refs)
    assert batch.launches == 1


def test_fst_decoder_on_the_device_against_its_cpu_copy(monkeypatch):
    import copy
    from grammar_cases import BIGRAM_LM, WSJ_VOCAB
    from att_speech.modules.decoders.advanced_decoder import FSTDecoder
    vocab = [l.rstrip('\n') for l in open(WSJ_VOCAB)][:49]
    B, T, D = 2, 16, 24
    gg = dict(class_name='CTCGraphGen', context_order=1, grammar_fst=BIGRAM_LM, vocabulary=WSJ_VOCAB)
    torch.manual_seed(0)
    kw = dict(normalize_by_dim=None, denominator_red='logsumexp', vocabulary=vocab, decode_beam=16.0,
              decode_lattice_beam=4.0)
    with pytest.raises(ValueError, match='decode_lattice_beam'):
        FSTDecoder({'features': torch.zeros(B, T, D)}, 49, gg, decode_oracle=True,
                   **dict(kw, decode_lattice_beam=None))
    cpu = FSTDecoder({'features': torch.zeros(B, T, D)}, 49, gg, decode_oracle=True, **kw)
    plain = copy.deepcopy(cpu)
    plain.decode_oracle = False
    gpu = copy.deepcopy(cpu).to(dev())
    cpu._utterance_losses = lambda *a, **k: torch.zeros(B)      # the loss of the transcripts has no CPU path
    enc = torch.randn(T, B, D) * 3
    elens = torch.tensor([16, 11], dtype=torch.int32)
    texts = torch.tensor([[5, 9, 12, 7, 3, 0], [20, 4, 4, 8, 0, 0]], dtype=torch.int32)
    tlens = torch.tensor([5, 4], dtype=torch.int32)
    launched = []
    real = DeviceLatticeBatch.oracle

    def counted(self, *a, **k):
        out = real(self, *a, **k)
        launched.append((self.device.type, self.launches))
        return out
    monkeypatch.setattr(DeviceLatticeBatch, 'oracle', counted)
    with torch.no_grad():
        want = cpu.decode(enc, elens, texts, tlens)
        got = gpu.decode(enc.to(dev()), elens, texts, tlens)
        silent = gpu.decode(enc.to(dev()), elens)
        bare = plain.to(dev()).decode(enc.to(dev()), elens, texts, tlens)
    assert launched == [('cpu', 0), ('cuda', 1)]        # one launch for the batch; none without texts or the flag
    assert 'oracle' not in bare and 'oracle' not in silent
    assert got['decoded'] == want['decoded'] == bare['decoded'] == silent['decoded']
    assert len(got['oracle']) == B
    for b in range(B):
        # the projection runs in fp32 on either device: the lattices agree to its rounding, the counts are equal
        assert got['oracle'][b][0] == want['oracle'][b][0] >= 0
        ref = texts[b, :int(tlens[b])].tolist()
        assert got['oracle'][b][0] <= edit_distance(got['decoded'][b], ref)
        assert edit_distance(got['oracle'][b][1], ref) == got['oracle'][b][0]


def edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[len(b)]
