"""asr_lattice_mbr_f64 (csrc/lattice_dp.hip) through DeviceLatticeBatch.mbr.  With the twin's conditional
posteriors passed in, everything the device returns (words, confidences, frames, risk, iterations,
sausage) equals LatticeBatch.mbr with ==: the arithmetic is integer, so no schedule can change it.  End
to end (the device computes its own posteriors) the risk is held to the twin's within RISK_TOL.  Every
device case asserts that the kernel was launched (batch.launches)."""
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
from att_speech.wfst_lattice import MBR_NONE, LatticeBatch

pytestmark = pytest.mark.gpu

# End to end the device's own log-semiring forward pass (max then sum in the stored order) and numpy's
# pairwise logaddexp differ in the last bits of the conditionals.  The largest |risk - twin's risk| over
# the cases of test_end_to_end, measured once on an MI355X, is 6.37e-12; the
# bound is ten times that.  It must be no looser than 1e-6, a decade under delta = 1e-5.
RISK_TOL = 10 * 6.37e-12


def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device('cuda:0')


@contextmanager
def quiet():
    """no warning from the package inside"""
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        yield
    ours = [str(w.message) for w in rec if 'att_speech' in (w.filename or '') or 'mbr' in str(w.message)]
    assert ours == [], ours


def device_mbr(batch, *args, launches=1, **kw):
    assert batch.device.type == 'cuda'
    batch.launches = 0
    with quiet():
        got = batch.mbr(*args, **kw)
    assert batch.launches > 0 and (launches is None or batch.launches == launches), batch.launches
    return got


def check(batch, *args, host=None, launches=1, **kw):
    """the device against the twin on the twin's conditionals: =="""
    host = LatticeBatch(batch.lattices()) if host is None else host
    arc, end = host.conditionals(*args[:2])
    twin_kw = {k: v for k, v in kw.items() if k in ('max_iterations', 'hypotheses')}
    want = host.mbr(*args, arc_cond=arc, end_cond=end, **twin_kw)
    got = device_mbr(batch, *args, arc_cond=arc, end_cond=end, launches=launches, **kw)
    assert len(got) == len(want) == batch.num_utterances
    for b, (x, y) in enumerate(zip(got, want)):
        assert x == y, (args, b, x, y)
    return got


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
        got = check(made, host=host)
        assert check(uploaded, host=host) == got
        assert all(r.iterations >= 1 and r.risk < INF for r in got)
        check(made, 0.5, 2.0, host=host)


def test_unquantised_scores():
    x = NC.unquantised_scores().to(dev())
    for lb in NC.UNQUANTISED_BEAMS:
        with quiet():
            batch, redone = decode_lattice_device(x, NC.UNQUANTISED_LENS, NC.bigram_graph(), beam=16.0,
                                                  lattice_beam=lb)
        assert redone == []
        got = check(batch)
        check(batch, 0.5, 2.0)
    assert any(len(row) > 1 for r in got for row in r.sausage)          # alternatives indeed


def test_fan_lattice():
    """3000 in-arcs at one node, all summed by one wave; gamma ties in the slots"""
    lat = NC.fan_lattice()
    with quiet():
        batch = DeviceLatticeBatch.from_lattices([lat, lat], dev())
    assert int((batch.in_ptr[1:] - batch.in_ptr[:-1]).max()) >= 3000
    host = LatticeBatch([lat, lat])
    got = check(batch, host=host)
    assert got[0] == got[1] and got[0].risk > 0
    check(batch, 0.0, 1.0, host=host)                   # no acoustic cost: the posteriors tie in hundreds


def test_more_than_32_words():
    """S + 1 > 64 columns: a wave takes two rounds over the slots, with a carry between them"""
    g, lp = MC.long_inputs()
    with quiet():
        batch, _ = decode_lattice_device(lp.to(dev()), MC.LONG_LENS, g, beam=16.0, lattice_beam=2.0)
    got = check(batch)
    assert len(got[0].words) >= 33 and len(got[1].words) <= 1
    sents = batch.sentences(3)
    for i in range(3):
        check(batch, max_iterations=0, hypotheses=[s[min(i, len(s) - 1)] for s in sents])


def test_large():
    """the shape of tests/test_lattice_dp_gpu.py: more than 65536 arcs in one lattice"""
    import test_lattice_dp_gpu as D
    g, lp, lens, batch = D.large()
    assert np.diff(batch.arc_off).max() > 65536
    got = check(batch, max_iterations=2)
    assert all(r.risk < INF and r.iterations >= 1 for r in got)


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
    for batch, empty in ((gone, [0, 2]), (mixed, [0]), (partial, [])):
        got = check(batch)
        assert [b for b, r in enumerate(got) if r == MBR_NONE] == empty
    res = check(silent)[0]
    assert res.words == [] and res.risk == 0.0 and res.sausage == []
    assert nothing.mbr() == [MBR_NONE]


def test_evaluation_only_and_expected_errors():
    x = NC.unquantised_scores().to(dev())
    with quiet():
        batch, _ = decode_lattice_device(x, NC.UNQUANTISED_LENS, NC.bigram_graph(), beam=16.0, lattice_beam=4.0)
    sents = batch.sentences(5)
    host = LatticeBatch(batch.lattices())
    risks = [[] for _ in sents]
    for i in range(5):
        hyps = [s[min(i, len(s) - 1)] for s in sents]
        got = check(batch, max_iterations=0, hypotheses=hyps, host=host)
        assert [r.words for r in got] == hyps and all(r.iterations == 1 for r in got)
        for b, s in enumerate(sents):
            if i < len(s):
                risks[b].append(got[b].risk)
    arc, end = host.conditionals()
    batch.launches = 0
    assert batch.expected_errors(sents, arc_cond=arc, end_cond=end) == risks and batch.launches == 5
    best = check(batch, host=host)
    assert all(r.risk <= min(row) + 1e-9 for r, row in zip(best, risks))       # MBR is no worse than its start


def test_run_to_run_and_workgroup_sizes(monkeypatch):
    lat = NC.fan_lattice()
    with quiet():
        batches = [DeviceLatticeBatch.from_lattices([lat], dev()),
                   DeviceLatticeBatch.from_lattices(NC.unquantised_lattices(6.0), dev()),
                   DeviceLatticeBatch.from_lattices(MC.long_lattices(), dev())]
    for batch in batches:
        first = check(batch)
        own = device_mbr(batch)                         # its own posteriors: the same bits every time too
        assert device_mbr(batch) == own
        for threads in (64, 128, 256):
            monkeypatch.setattr(lattice_dp, 'THREADS_PER_WORKGROUP', threads)
            assert check(batch) == first, threads
            assert device_mbr(batch) == own, threads
        monkeypatch.setattr(lattice_dp, 'THREADS_PER_WORKGROUP', 0)


def test_chunking():
    """a workspace that does not hold all utterances: several launches, the same results"""
    with quiet():
        batch = DeviceLatticeBatch.from_lattices(NC.unquantised_lattices(4.0), dev())
    whole = check(batch)
    nodes = np.diff(batch.node_off)
    W = int(np.diff(batch.level_off).max())
    per_node = 16 * (2 * W + 2) + 8
    one_each = check(batch, workspace_bytes=per_node * int(nodes.max()) + 192, launches=None)
    assert batch.launches >= 3
    pairs = check(batch, workspace_bytes=per_node * int(nodes[:2].sum()) + 192, launches=None)
    assert batch.launches == 2
    assert whole == one_each == pairs
    with pytest.raises(ValueError, match='workspace_bytes'):
        batch.mbr(workspace_bytes=per_node * int(nodes.max()))


def end_to_end_cases():
    g, lp = MC.long_inputs()
    out = [('single', [MC.single_path()]), ('tree', [MC.tree_lattice()]), ('fan', [NC.fan_lattice()]),
           ('long', MC.long_lattices())]
    out += [('toy %s %s %s' % c, NC.toy_lattices(*c)[0]) for c in MC.toy_sweep()]
    out += [('unquantised %s' % lb, NC.unquantised_lattices(lb)) for lb in NC.UNQUANTISED_BEAMS]
    return out


def test_end_to_end():
    """no overrides: the device runs its own log-semiring forward pass"""
    worst = 0.0
    for name, lats in end_to_end_cases():
        with quiet():
            batch = DeviceLatticeBatch.from_lattices(lats, dev())
        host = LatticeBatch(lats)
        for args in ((), (0.5, 2.0)):
            got, want = device_mbr(batch, *args), host.mbr(*args)
            for b, (x, y) in enumerate(zip(got, want)):
                assert (x.risk < INF) == (y.risk < INF), (name, b)
                if y.risk < INF:
                    diff = abs(x.risk - y.risk)
                    worst = max(worst, diff)
                    print('%s #%d %s: risk %.17g twin %.17g diff %.3g' % (name, b, args, x.risk, y.risk, diff))
                    assert diff <= RISK_TOL, (name, b, args, x.risk, y.risk)
                if name in ('single', 'tree') or name.startswith('toy'):
                    assert x.words == y.words, (name, b, args)
    print('largest difference %.3g' % worst)
    assert RISK_TOL <= 1e-6


def test_fallbacks(monkeypatch):
    """a hypothesis above the device's words and a sausage above its buffer: the twin, one warning"""
    lats = NC.unquantised_lattices(4.0)
    with quiet():
        batch = DeviceLatticeBatch.from_lattices(lats, dev())
    host = LatticeBatch(lats)
    arc, end = host.conditionals()
    want = host.mbr(arc_cond=arc, end_cond=end)
    assert check(batch, host=host) == want
    longest = max(len(r.words) for r in want)
    for attr, value in (('MBR_DEVICE_MAX_WORDS', longest - 1), ('MBR_SAUSAGE_ENTRIES', 5)):
        monkeypatch.setattr(lattice_dp, attr, value)
        batch.launches = 0
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            got = batch.mbr(arc_cond=arc, end_cond=end)
        assert batch.launches == 1 and got == want
        assert len([w for w in rec if 'redone on the host' in str(w.message)]) == 1
        monkeypatch.undo()
    assert lattice_dp.MBR_DEVICE_MAX_WORDS >= 255
    too_long = [[1] * 300 for _ in lats]               # above ASR_LATTICE_MBR_MAX_WORDS itself
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        got = batch.mbr(max_iterations=0, hypotheses=too_long, arc_cond=arc, end_cond=end)
    assert batch.launches == 1                          # launched: the kernel itself hands every utterance back
    assert got == host.mbr(max_iterations=0, hypotheses=too_long, arc_cond=arc, end_cond=end)
    assert len([w for w in rec if 'redone on the host' in str(w.message)]) == 1


def test_env_switch(monkeypatch):
    g, lp = NC.toy_inputs('b')
    with quiet():
        batch, _ = decode_lattice_device(torch.from_numpy(lp).to(dev()), NC.LENS, g, beam=INF, lattice_beam=INF)
    host = LatticeBatch(batch.lattices())
    arc, end = host.conditionals()
    native = device_mbr(batch, arc_cond=arc, end_cond=end)
    calls = []
    real = LatticeBatch.mbr
    monkeypatch.setattr(LatticeBatch, 'mbr', lambda self, *a, **k: calls.append(a) or real(self, *a, **k))
    monkeypatch.setenv('ASR_LATTICE_MBR_NATIVE', '0')
    batch.launches = 0
    assert batch.mbr(arc_cond=arc, end_cond=end) == native and batch.launches == 0 and len(calls) == 1
    monkeypatch.delenv('ASR_LATTICE_MBR_NATIVE')
    assert device_mbr(batch, arc_cond=arc, end_cond=end) == native and len(calls) == 1


def test_a_malformed_batch_is_refused():
    """tensors changed behind the constructor's checks: the kernel's own range checks answer"""
    lats, _ = NC.toy_lattices('a', 1.0, 2.0)
    for field, index, value in (('dst', 3, 10 ** 6), ('arc', 1, 10 ** 6), ('node_level', 0, 10 ** 6),
                                ('in_ptr', 2, 10 ** 6), ('level_node', 1, 10 ** 6), ('in_arc', 1, 10 ** 6)):
        with quiet():
            batch = DeviceLatticeBatch.from_lattices(lats, dev())
        getattr(batch, field)[index] = value
        with pytest.raises(ValueError, match='inconsistent'):
            batch.mbr()
        assert batch.launches == 1
    with quiet():                                       # an arc turned round: the level does not rise
        batch = DeviceLatticeBatch.from_lattices(lats, dev())
    j = int(np.nonzero(lats[0].src != lats[0].dst)[0][0])
    batch.dst[j] = batch.src[j]
    with pytest.raises(ValueError, match='inconsistent'):
        batch.mbr()


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
    cpu = FSTDecoder({'features': torch.zeros(B, T, D)}, 49, gg, decode_mbr=True, **kw)
    plain = copy.deepcopy(cpu)
    plain.decode_mbr = False
    gpu = copy.deepcopy(cpu).to(dev())
    enc = torch.randn(T, B, D) * 3
    elens = torch.tensor([16, 11], dtype=torch.int32)
    launched = []
    real = DeviceLatticeBatch.mbr

    def counted(self, *a, **k):
        out = real(self, *a, **k)
        launched.append((self.device.type, self.launches))
        return out
    monkeypatch.setattr(DeviceLatticeBatch, 'mbr', counted)
    with torch.no_grad():
        want = cpu.decode(enc, elens)
        got = gpu.decode(enc.to(dev()), elens)
        bare = plain.to(dev()).decode(enc.to(dev()), elens)
    assert launched == [('cpu', 0), ('cuda', 1)]        # one launch for the batch, none without decode_mbr
    assert 'mbr' not in bare and got['decoded'] == want['decoded'] == bare['decoded']
    assert len(got['mbr']) == len(got['mbr_risk']) == B
    for b in range(B):
        # the projection runs in fp32 on either device: the lattices agree to its rounding, not in bits
        assert got['mbr'][b][0] == want['mbr'][b][0]
        assert got['mbr'][b][1] == pytest.approx(want['mbr'][b][1], abs=1e-3)
        assert len(got['mbr'][b][2]) == len(got['mbr'][b][0])
        assert got['mbr_risk'][b] == pytest.approx(want['mbr_risk'][b], abs=1e-3)
