"""asr_lattice_nbest_f64 (csrc/lattice_dp.hip) through DeviceLatticeBatch.nbest: everything the device
returns, words and costs, equals LatticeBatch.nbest (the numpy twin, itself held to Lattice.nbest and
the enumerator in tests/test_lattice_nbest.py) with ==.  Every device case asserts that the kernel was
launched (batch.launches), so none passes on the host path."""
import warnings
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import nbest_cases as NC
from wfst_cases import INF, TOYS, grid_scores, toy_graph

from att_speech import lattice_dp
from att_speech._native import lib
from att_speech.lattice_dp import DeviceLatticeBatch, decode_lattice_device
from att_speech.wfst_lattice import LatticeBatch

pytestmark = pytest.mark.gpu

CAP = lattice_dp.NBEST_DEVICE_MAX


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device('cuda:0')


@contextmanager
def quiet():
    """no warning from the package inside"""
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        yield
    ours = [str(w.message) for w in rec if 'att_speech' in (w.filename or '') or 'lattice' in str(w.message)]
    assert ours == [], ours


def device_nbest(batch, n, *args, launches=1, **kw):
    """the kernel's lists; launches None: any number above 0"""
    assert batch.device.type == 'cuda'
    batch.launches = 0
    with quiet():
        got = batch.nbest(n, *args, **kw)
    assert batch.launches > 0 and (launches is None or batch.launches == launches), batch.launches
    return got


def check(batch, n, *args, host=None, **kw):
    got = device_nbest(batch, n, *args, **kw)
    host = LatticeBatch(batch.lattices()) if host is None else host
    with np.errstate(invalid='ignore'):
        want = host.nbest(n, *args[:2])
    assert len(got) == len(want) == batch.num_utterances
    for b, (x, y) in enumerate(zip(got, want)):
        assert x == y, (n, args, b, x[:3], y[:3])       # == on words and costs
    return got


@pytest.mark.parametrize('name', sorted(TOYS))
def test_toy_sweep(name):
    """from the device search and from uploaded host lattices; utterance 1 of toys b and c is partial"""
    g, lp = NC.toy_inputs(name)
    x = torch.from_numpy(lp).to(dev())
    for scale in NC.SCALES:
        for lb in NC.LATTICE_BEAMS:
            lats, every = NC.toy_lattices(name, scale, lb)
            host = LatticeBatch(lats)
            with quiet():
                made, redone = decode_lattice_device(x, NC.LENS, g, beam=INF, lattice_beam=lb, acoustic_scale=scale)
                uploaded = DeviceLatticeBatch.from_lattices(lats, dev())
            assert redone == []
            for n in NC.sweep_ns(every):
                if n > CAP:                             # the twin takes over, on a copy
                    made.launches = 0
                    assert made.nbest(n) == host.nbest(n) and made.launches == 0
                    continue
                got = check(made, n, host=host)
                assert check(uploaded, n, host=host) == got
                for b, lat in enumerate(lats):
                    NC.check_against_host(got[b], lat, every[b], n, (name, scale, lb, n, b))


def test_unquantised_scores():
    """bit equality off the 2^-8 grid: fl(x + c) on the device is numpy's, uncontracted"""
    x = NC.unquantised_scores().to(dev())
    for lb in NC.UNQUANTISED_BEAMS:
        with quiet():
            batch, redone = decode_lattice_device(x, NC.UNQUANTISED_LENS, NC.bigram_graph(), beam=16.0,
                                                  lattice_beam=lb)
        assert redone == []
        for n in (5, 20):
            got = check(batch, n)
            assert all(len(row) == n for row in got[:3])
        check(batch, 5, 0.5, 2.0)
    assert any(c != round(c * 256) / 256 for _, c in got[0])            # costs off the grid indeed


def test_fan_lattice():
    """6000 arcs out of one node (94 rounds of a wave) and 3000 into one, cost ties, repeated labels"""
    lat = NC.fan_lattice()
    with quiet():
        batch = DeviceLatticeBatch.from_lattices([lat, lat], dev())
    assert int((batch.out_ptr[1:] - batch.out_ptr[:-1]).max()) >= 3000
    assert int((batch.in_ptr[1:] - batch.in_ptr[:-1]).max()) >= 3000
    host = LatticeBatch([lat, lat])
    for n in (1, 10, CAP):
        got = check(batch, n, host=host)
        assert len(got[0]) == n and got[0] == got[1]
    assert len({c for _, c in got[0]}) < CAP // 2       # ties indeed
    check(batch, 10, 0.0, 1.0, host=host)               # no acoustic cost: every tie is real


def test_large_and_many_levels():
    """the shapes of tests/test_lattice_dp_gpu.py: 79 436 arcs in one lattice; 246 levels beside 5"""
    import test_lattice_dp_gpu as D
    g, lp, lens, batch = D.large()
    assert np.diff(batch.arc_off).max() > 65536
    got = check(batch, 10)
    assert all(len(row) == 10 for row in got)
    g = toy_graph('c')
    lens = [64, 1]
    lp = grid_scores(np.random.default_rng(64), 64, 2, 3, lens, low=-4.0)
    batch = D.device_batch(g, lp, lens, beam=INF, lattice_beam=INF)
    levels = np.diff(batch.level_off)
    assert levels[0] > 3 * 64 and levels[1] <= 6, levels
    got = check(batch, 10)
    assert len(got[0]) == 10 and len(got[0][0][0]) > 10 and 1 <= len(got[1]) <= 10
    check(batch, CAP)


def test_n_1_equals_best_paths():
    for name in sorted(TOYS):
        g, lp = NC.toy_inputs(name)
        with quiet():
            batch, _ = decode_lattice_device(torch.from_numpy(lp).to(dev()), NC.LENS, g, beam=INF, lattice_beam=2.0)
        for sc, lm in ((None, 1.0), (0.5, 1.0), (0.5, 2.0), (1.0, 0.0)):
            got = check(batch, 1, sc, lm)
            if lm:
                best = batch.best_paths(sc, lm)[0]
                assert [row[0][1] for row in got] == [c for _, c, _, _ in best]


def test_the_cap_and_beyond():
    """n = the device cap runs the kernel, cap + 1 the twin on a copy: the same lists where the
    lattice holds no more than cap sequences, and a prefix relation otherwise"""
    g, lp = NC.toy_inputs('a')
    with quiet():
        batch, _ = decode_lattice_device(torch.from_numpy(lp).to(dev()), NC.LENS, g, beam=INF, lattice_beam=INF)
    host = LatticeBatch(batch.lattices())
    at_cap = check(batch, CAP, host=host)
    batch.launches = 0
    with quiet():
        beyond = batch.nbest(CAP + 1)
    assert batch.launches == 0 and beyond == host.nbest(CAP + 1)
    assert max(len(row) for row in beyond) == CAP + 1
    for a, b in zip(at_cap, beyond):
        assert [c for _, c in a] == [c for _, c in b[:CAP]]
        assert len(b) > CAP or a == b
    with quiet():
        small, _ = decode_lattice_device(torch.from_numpy(lp).to(dev()), NC.LENS, g, beam=INF, lattice_beam=1.0)
    few = check(small, CAP)                             # n above the number of sequences
    assert all(0 < len(row) < CAP for row in few)
    small.launches = 0
    assert small.nbest(CAP + 1) == few and small.launches == 0
    assert small.sentences(3) == [[w for w, _ in row] for row in check(small, 3)]


def test_empty_and_partial_utterances_inside_a_batch():
    g = toy_graph('c')                                  # its final state is at least three frames away
    lens = [1, 5, 2]
    lp = torch.from_numpy(grid_scores(np.random.default_rng(4), 5, 3, 3, lens, low=-4.0)).to(dev())
    with quiet():
        gone, _ = decode_lattice_device(lp, lens, g, beam=INF, lattice_beam=2.0, allow_partial=False)
        partial, _ = decode_lattice_device(lp, lens, g, beam=INF, lattice_beam=2.0, allow_partial=True)
        mixed = DeviceLatticeBatch.from_lattices([gone.lattices()[0], gone.lattices()[1], partial.lattices()[2]],
                                                 dev())
        silent = DeviceLatticeBatch.from_lattices([NC.without_words(gone.lattices()[1])], dev())
    assert not partial.reached_final[0]
    for batch, empty in ((gone, [0, 2]), (mixed, [0]), (partial, [])):
        got = check(batch, 4)
        assert [b for b, row in enumerate(got) if not row] == empty
    assert check(silent, 4) == [[([], check(mixed, 1)[1][0][1])]]       # every output label 0: one entry, no words
    with quiet():
        nothing = DeviceLatticeBatch.from_lattices([gone.lattices()[0]], dev())
    assert nothing.nbest(3) == [[]]


def test_chunking():
    """a workspace that does not hold all utterances: several launches, the same bits"""
    x = NC.unquantised_scores().to(dev())
    with quiet():
        batch, _ = decode_lattice_device(x, NC.UNQUANTISED_LENS, NC.bigram_graph(), beam=16.0, lattice_beam=4.0)
    n = 7
    whole = check(batch, n)
    nodes = np.diff(batch.node_off)
    per_node = 28 * n + 4
    one_each = check(batch, n, workspace_bytes=per_node * int(nodes.max()) + 192, launches=None)
    groups, room = 0, 0
    for k in nodes.tolist():                            # utterances in order, as many as fit a launch
        groups, room = (groups, room - k) if k <= room else (groups + 1, int(nodes.max()) - k)
    assert batch.launches == groups >= 3                # [163, 132, 90, 5] nodes: 0; 1; 2 and 3 together
    pairs = check(batch, n, workspace_bytes=per_node * int(nodes[:2].sum()) + 192, launches=None)
    assert batch.launches == 2                          # utterances 0 and 1; then 2 and 3, which are smaller
    assert whole == one_each == pairs
    with pytest.raises(ValueError, match='workspace_bytes'):
        batch.nbest(n, workspace_bytes=per_node * int(nodes.max()))


def test_run_to_run_bits_and_workgroup_sizes(monkeypatch):
    lat = NC.fan_lattice()
    with quiet():
        batches = [DeviceLatticeBatch.from_lattices([lat], dev()),
                   DeviceLatticeBatch.from_lattices(NC.unquantised_lattices(6.0), dev())]
    for batch in batches:
        first = device_nbest(batch, 20)
        assert device_nbest(batch, 20) == first
        for threads in (64, 128, 256):
            monkeypatch.setattr(lattice_dp, 'THREADS_PER_WORKGROUP', threads)
            assert device_nbest(batch, 20) == first, threads
        monkeypatch.setattr(lattice_dp, 'THREADS_PER_WORKGROUP', 0)


def test_env_switch(monkeypatch):
    g, lp = NC.toy_inputs('b')
    with quiet():
        batch, _ = decode_lattice_device(torch.from_numpy(lp).to(dev()), NC.LENS, g, beam=INF, lattice_beam=INF)
    native = check(batch, 6)
    calls = []
    real = LatticeBatch.nbest
    monkeypatch.setattr(LatticeBatch, 'nbest', lambda self, *a, **k: calls.append(a) or real(self, *a, **k))
    monkeypatch.setenv('ASR_LATTICE_NBEST_NATIVE', '0')
    batch.launches = 0
    assert batch.nbest(6) == native and batch.launches == 0 and len(calls) == 1
    monkeypatch.delenv('ASR_LATTICE_NBEST_NATIVE')
    assert device_nbest(batch, 6) == native and len(calls) == 1


def test_a_malformed_batch_is_refused():
    """tensors changed behind the constructor's checks: the kernel's own range checks answer"""
    lats, _ = NC.toy_lattices('a', 1.0, 2.0)
    for field, index, value in (('dst', 3, 10 ** 6), ('arc', 1, 10 ** 6), ('node_level', 0, 10 ** 6),
                                ('out_ptr', 2, 10 ** 6), ('level_node', 1, 10 ** 6)):
        with quiet():
            batch = DeviceLatticeBatch.from_lattices(lats, dev())
        getattr(batch, field)[index] = value
        with pytest.raises(ValueError, match='inconsistent'):
            batch.nbest(3)
        assert batch.launches == 1
    with quiet():                                       # an arc turned round: the level does not rise
        batch = DeviceLatticeBatch.from_lattices(lats, dev())
    j = int(np.nonzero(lats[0].src != lats[0].dst)[0][0])
    batch.dst[j] = batch.src[j]
    with pytest.raises(ValueError, match='inconsistent'):
        batch.nbest(3)


def test_fst_decoder_on_the_device_against_its_cpu_copy(monkeypatch):
    import copy
    from grammar_cases import BIGRAM_LM, WSJ_VOCAB
    from att_speech.modules.decoders.advanced_decoder import FSTDecoder
    vocab = [l.rstrip('\n') for l in open(WSJ_VOCAB)][:49]
    B, T, D = 2, 16, 24
    gg = dict(class_name='CTCGraphGen', context_order=1, grammar_fst=BIGRAM_LM, vocabulary=WSJ_VOCAB)
    torch.manual_seed(0)
    cpu = FSTDecoder({'features': torch.zeros(B, T, D)}, 49, gg, normalize_by_dim=None, denominator_red='logsumexp',
                     vocabulary=vocab, decode_beam=16.0, decode_lattice_beam=4.0, decode_nbest=5,
                     decode_nbest_device=True)
    gpu = copy.deepcopy(cpu).to(dev())
    enc = torch.randn(T, B, D) * 3
    elens = torch.tensor([16, 11], dtype=torch.int32)
    launched = []
    real = DeviceLatticeBatch.nbest

    def counted(self, *a, **k):
        out = real(self, *a, **k)
        launched.append((self.device.type, getattr(self, 'launches', 0)))
        return out
    monkeypatch.setattr(DeviceLatticeBatch, 'nbest', counted)
    with torch.no_grad():
        want = cpu.decode(enc, elens)
        got = gpu.decode(enc.to(dev()), elens)
    assert launched == [('cpu', 0), ('cuda', 1)]        # one launch for the batch
    assert got['decoded'] == want['decoded']
    for b in range(B):
        # the projection runs in fp32 on either device: the lattices agree to its rounding, not in bits
        assert got['nbest'][b][0][0] == want['nbest'][b][0][0] == want['decoded'][b]
        assert len(got['nbest'][b]) == len(want['nbest'][b])
        assert [c for _, c in got['nbest'][b]] == pytest.approx([c for _, c in want['nbest'][b]], abs=1e-3)


def test_the_entry_points_are_exported():
    L = lib()
    assert L.asr_lattice_nbest_supported(1000, 5000, 300, CAP) == 1
    assert L.asr_lattice_nbest_supported(1000, 5000, 300, CAP + 1) == 0
    assert L.asr_lattice_nbest_workspace_bytes(1000, 10) >= 1000 * 284
    assert L.asr_abi_version() == 24 and CAP >= 64
