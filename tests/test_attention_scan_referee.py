"""The referee of the attention training scans (tests/attention_scan_referee.py) proved on the CPU:
in fp64 it is what autograd makes of the modules' own per-position loops; its fp32 yardstick passes
every judge; every one-term mutant is rejected at the cases named for it; the Python mirror of the
launch plans reaches what the case matrix claims and agrees with the kernels' constants.  No native
calls: tests/test_attention_scan_referee_gpu.py holds the kernels to the same judge."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import attention_scan_referee as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
_cache = {}


def run_case(name, mut=None):
    """a stand-in for the kernels (the fp32 yardstick running free, `mut` one wrong term) through the
    judge exactly as the GPU file sends the launches: forward teacher-forced, backward from an
    unmutated forward's tensors -> complaints"""
    c = ar.build(name)
    key = 'att' if c['spec']['kind'] == 'tcn' else 'states'
    if name not in _cache:
        _cache[name] = ar.yardstick(c, 'fwd', None)
    kern = ar.yardstick(c, 'fwd', None, mut) if mut else _cache[name]
    want, tol = ar.referee(c, 'fwd', kern[key])
    bad = ar.judge(c, 'fwd', kern, want, tol)
    saved = _cache[name]
    got = ar.yardstick(c, 'bwd', saved, mut)
    want, tol = ar.referee(c, 'bwd', saved, got)
    return bad + ar.judge(c, 'bwd', got, want, tol)


@pytest.mark.parametrize('name', ar.cases())
def test_yardstick_passes_the_judge(name):
    assert run_case(name) == []


MUTANT_PAIRS = [(m, n) for m, names in ar.MUTANT_CASES.items() for n in names]


def test_every_mutant_has_a_case_named_for_it():
    assert set(ar.MUTANT_CASES) == set(ar.TCN_MUTANTS + ar.GRU_MUTANTS)
    assert all(ar.MUTANT_CASES[m] for m in ar.MUTANT_CASES)
    for m, n in MUTANT_PAIRS:
        assert ar.SPECS[n]['kind'] == ('tcn' if m in ar.TCN_MUTANTS else 'gru')


@pytest.mark.parametrize('mut,name', MUTANT_PAIRS)
def test_mutant_is_rejected(mut, name):
    bad = run_case(name, mut)
    assert bad, '%s passes the judge at %s' % (mut, name)


# (mutant, case) pairs the judge cannot tell from the real thing, and why: the wrong term is not
# exercised by the case, so the mutant computes the same numbers
BLIND = {
    ('mask_before_temperature', 'tcn/T33B2L3A8'): '-1e5 * 1.25 underflows as -1e5 does',
    ('tile_tail_frames_dropped', 'tcn/T64B2L3A64'): 'T is a whole tile',
    ('carry_misses_tile_seam', 'tcn/T63B2L3A64'): 'one tile, no seam',
    ('last_unit_chunk_dropped', 'tcn/T1B1L1A1'): 'T = 1: the alignment is 1 and every gradient 0',
    ('d_wb_first_utterance_only', 'tcn/T1100B1L2A64'): 'one utterance',
    ('carry_not_cleared', 'tcn/T70B2L1A64'): 'one position: the carry is used once',
    ('d_eproj_last_position_only', 'tcn/T70B2L1A64'): 'one position',
    ('a0_at_every_position', 'tcn/T70B2L1A64'): 'one position',
    ('len_0_is_empty', 'gru/T33B3L4A12E36H20_short'): 'no length is 0',
    ('d_att_ignored', 'gru/T33B3L4A12E36H20_no_d_att'): 'd_att is null',
    ('d_states_ignored', 'gru/T33B3L4A12E36H20_no_d_states'): 'd_states is null',
    ('context_groups_miss_tail', 'gru/T4096B1L2A4E4H4'): '4096 frames are whole groups of eight',
}


@pytest.mark.parametrize('mut,name', sorted(BLIND))
def test_blind_pairs_are_what_they_are_said_to_be(mut, name):
    assert run_case(name, mut) == [], BLIND[(mut, name)]


# ------------------------------------------------------------------ the launch plans

def _hip_constants(path):
    text = open(os.path.join(ROOT, path)).read()
    return {k: int(v) for k, v in re.findall(r'constexpr int (\w+) = (\d+);', text)}


def test_plan_mirror_agrees_with_the_kernels_constants_and_the_header():
    k = _hip_constants('pytorch-asr_amd/csrc/tcn_train.hip')
    assert (k['NT'], k['KF'], k['TMAX'], k['AMAX'], k['PART_CAP'], k['TILE_CAP'], k['TT_MAX']) == \
        (ar.NT, ar.KF, ar.TMAX, ar.AMAX, ar.PART_CAP, ar.TILE_CAP, ar.TT_MAX)
    g = _hip_constants('pytorch-asr_amd/csrc/att_gru.hip')
    assert (g['TMAX'], g['HMAX'], g['AMAX'], g['EMAX'], g['CG'], g['NT'] // 64) == \
        (ar.GRU_TMAX, ar.GRU_HMAX, ar.GRU_AMAX, ar.GRU_EMAX, ar.GRU_CG, ar.GRU_NW)
    header = ' '.join(open(os.path.join(ROOT, 'include/asr_amd.h')).read().split())
    assert 'Limits: Kf == %d, * 1 <= A <= %d, 1 <= T <= %d (ASR_EUNSUPPORTED beyond)' % (ar.KF, ar.AMAX, ar.TMAX) in header
    assert 'Limits: 1 <= T <= %d, A <= %d, H <= %d, E <= %d' % (ar.GRU_TMAX, ar.GRU_AMAX, ar.GRU_HMAX, ar.GRU_EMAX) in header
    from att_speech.modules import tcn
    assert (tcn._SCAN_MAX_FRAMES, tcn._SCAN_MAX_WIDTH) == (ar.TMAX, ar.AMAX)


def test_every_admitted_plan_is_whole_and_fits():
    for A in range(1, ar.AMAX + 1):
        TT, G2, AC2 = ar.bwd_tiles(A)
        assert TT * G2 <= ar.NT and TT * A <= ar.TILE_CAP and G2 * AC2 >= A > (G2 - 1) * AC2
        assert A * ar.KF <= 16 * ar.NT                                  # QMAX accumulators a thread
        for T in (1, 31, 70, 512, 600, 1100, 2048, 2100, 4095, 4096):
            G, AC = ar.fwd_split(T, A)
            assert G * AC >= A > (G - 1) * AC and (G == 1 or G * T <= ar.PART_CAP)
            assert ar.fwd_lds(T, A) <= ar.LDS_CAP and ar.bwd_lds(T, A) <= ar.LDS_CAP


def test_the_matrix_reaches_what_it_claims():
    p = ar.plan(70, 100)
    assert (p['TT'], p['AC2'], p['G2']) == (40, 9, 12) and 100 - (p['G2'] - 1) * p['AC2'] == 1
    ragged = [A for A in (1, 7, 100, 200, 255, 256) if ar.plan(70, A)['G'] > 1 and A % ar.plan(70, A)['AC']]
    assert len(ragged) >= 2, ragged
    assert ar.plan(63, 64)['TT'] == 64 and ar.plan(15, 256)['TT'] == 16
    assert ar.plan(600, 64)['G'] > ar.plan(1100, 64)['G'] > 1 and ar.plan(2100, 8)['G'] == 1
    assert ar.plan(4096, 256)['G'] == 1
    assert ar.bwd_lds(4096, 256) == max(ar.bwd_lds(T, A) for T in (4095, 4096) for A in range(1, 257))
    assert ar.fwd_lds(4096, 256) == max(ar.fwd_lds(T, A) for T in (4095, 4096) for A in range(1, 257))
    names = ar.cases('tcn')
    shapes = {tuple(ar.SPECS[n][k] for k in 'TBLA') for n in names}
    for want in [(1, 1, 1, 1), (4096, 1, 2, 256), (600, 2, 2, 64), (1100, 1, 2, 64), (2100, 1, 2, 8)] + \
            [(T, 2, 3, 8) for T in (5, 31, 32, 33)] + [(70, 2, 3, A) for A in (1, 7, 100, 200, 255, 256)] + \
            [(T, 2, 3, 64) for T in (63, 64, 65, 129)] + [(T, 2, 3, 256) for T in (15, 16, 17, 33)]:
        assert want in shapes, want
    assert {ar.SPECS[n]['L'] for n in names} >= {1, 2, 5}
    seen = set()
    for n in names:
        s, c = ar.SPECS[n], ar.build(n)
        TT = ar.bwd_tiles(s['A'])[0]
        for v in c['lens'].tolist():
            assert 1 <= v <= s['T']
            seen.add('T' if v == s['T'] else '1' if v == 1 else 'mid' if v == s['T'] // 2 else
                     'inside' if v % TT else 'seam')
    assert seen >= {'T', '1', 'mid', 'inside'}
    gshapes = [tuple(ar.SPECS[n][k] for k in 'TBLAEH') for n in ar.cases('gru')]
    for want in ((1, 1, 1, 4, 4, 4), (33, 3, 4, 12, 36, 20), (70, 2, 3, 320, 64, 64), (50, 4, 5, 64, 320, 256),
                 (334, 2, 3, 128, 512, 320), (1100, 1, 2, 8, 8, 8), (4096, 1, 2, 4, 4, 4)):
        assert want in gshapes
    glens = [ar.build(n)['lens'].tolist() for n in ar.cases('gru')]
    assert [3, 9, 15] in glens and any(0 in v for v in glens)
    assert any(v[i] == ar.SPECS[n]['T'] + 5 for n, v in zip(ar.cases('gru'), glens) for i in range(len(v)))
    assert {(ar.SPECS[n]['d_att'], ar.SPECS[n]['d_states']) for n in ar.cases('gru')} == \
        {(True, True), (False, True), (True, False)}


# ------------------------------------------------------------------ the references against autograd

def _tcn_loop(c):
    """LocalAttention.scores / forward position after position (modules/tcn.py), in fp64"""
    leaf = {k: c[k].double().requires_grad_() for k in ('eproj', 'filt', 'glob', 'a0', 'w_score', 'b_score')}
    T, B, A = leaf['eproj'].shape
    pad = (torch.arange(T)[:, None] >= c['lens'][None, :].long()).double() * ar.MASKED
    prev, rows = leaf['a0'], []
    for l in range(c['spec']['L']):
        windows = F.pad(prev.t(), (ar.KF - 1, 0)).unfold(1, ar.KF, 1)
        filters = leaf['filt'][l].view(B, A, ar.KF)
        moved = torch.bmm(windows, filters.transpose(1, 2))
        hidden = leaf['eproj'].transpose(0, 1) + moved + leaf['glob'][l][:, None, :]
        energy = (torch.tanh(hidden) @ leaf['w_score'] + leaf['b_score']) * c['temperature']
        r = F.softmax(energy + pad.t(), 1)
        rows.append(r)
        prev = r.t()
    return leaf, torch.stack(rows)


SMALL_TCN = [n for n in ar.cases('tcn') if ar.SPECS[n]['T'] <= 129]
SMALL_GRU = [n for n in ar.cases('gru') if ar.SPECS[n]['T'] <= 70]


def _close(a, b, what):
    assert float((a - b).abs().max()) <= 1e-10, (what, float((a - b).abs().max()))


@pytest.mark.parametrize('name', SMALL_TCN)
def test_tcn_referee_is_autograd_through_the_loop(name):
    c = ar.build(name)
    leaf, att = _tcn_loop(c)
    (att * c['d_att'].double()).sum().backward()
    want = ar.forward(c)['att']
    _close(want, att.detach(), 'att')
    got = ar.backward(c, dict(att=want))
    A = c['spec']['A']
    for k in ('eproj', 'filt', 'glob', 'a0'):
        _close(got['d_' + k], leaf[k].grad, k)
    _close(got['d_wb'].sum(0)[:A], leaf['w_score'].grad, 'w_score')
    _close(got['d_wb'].sum(0)[A:], leaf['b_score'].grad, 'b_score')


def _gru_loop(c):
    """Attention.forward + one nn.GRU step position after position (modules/decoders/
    attention_decoder.py), in fp64; the embedding half of the input product enters as gx_emb"""
    keys = ('eproj', 'encoded', 'gx_emb', 'w_ic', 'w_hh', 'b_hh', 'w_rec', 'w_score', 'b_score', 'h0')
    leaf = {k: c[k].double().requires_grad_() for k in keys}
    T, B, A = leaf['eproj'].shape
    H = c['spec']['H']
    mask = (torch.arange(T)[:, None] >= ar.clamp_len(c['lens'], T)[None, :]).double() * ar.MASKED
    w_ih = torch.cat((leaf['w_ic'], torch.eye(3 * H, dtype=F64)), 1)
    h, rows = leaf['h0'], []
    for l in range(c['spec']['L']):
        rec = h @ leaf['w_rec'].t()
        hidden = leaf['eproj'] + rec[None]
        scores = torch.tanh(hidden) @ leaf['w_score'] + leaf['b_score']
        a = F.softmax(scores + mask, 0)                              # [T, B]
        ctx = (a[:, :, None] * leaf['encoded']).sum(0)
        h_new = torch.gru_cell(torch.cat((ctx, leaf['gx_emb'][l]), 1), h, w_ih, leaf['w_hh'],
                               torch.zeros(3 * H, dtype=F64), leaf['b_hh'])
        for x in (rec, ctx):
            x.retain_grad()
        rows.append((a.t(), h_new, ctx, rec, h))
        h = h_new
    return leaf, rows


@pytest.mark.parametrize('name', SMALL_GRU)
def test_gru_referee_is_autograd_through_the_loop(name):
    c = ar.build(name)
    s = c['spec']
    leaf, rows = _gru_loop(c)
    att, states = torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])
    loss = (states * 0).sum()
    if c['d_att'] is not None:
        loss = loss + (att * c['d_att'].double()).sum()
    if c['d_states'] is not None:
        loss = loss + (states * c['d_states'].double()).sum()
    loss.backward()
    fwd = ar.forward(c)
    _close(fwd['att'], att.detach(), 'att')
    _close(fwd['states'], states.detach(), 'states')
    _close(fwd['contexts'], torch.stack([r[2] for r in rows]).detach(), 'contexts')
    _close(fwd['rec'], torch.stack([r[3] for r in rows]).detach(), 'rec')
    got = ar.backward(c, fwd)
    H = s['H']
    zero = lambda x: torch.zeros_like(x) if x.grad is None else x.grad  # noqa: E731
    _close(got['d_eproj'] - c['d_eproj_prefill'].double(), zero(leaf['eproj']), 'd_eproj')
    _close(got['d_h0'], zero(leaf['h0']), 'd_h0')
    _close(got['d_w_score'].sum(0), zero(leaf['w_score']), 'd_w_score')
    _close(got['d_gates'][:, :, :3 * H], zero(leaf['gx_emb']), 'd_gates (dr, dz, dn)')
    _close(got['d_contexts'], torch.stack([zero(r[2]) for r in rows]), 'd_contexts')
    _close(got['d_rec'], torch.stack([zero(r[3]) for r in rows]), 'd_rec')
    h_prev = torch.stack([r[4] for r in rows]).detach()
    d_gh = torch.cat((got['d_gates'][:, :, :2 * H], got['d_gates'][:, :, 3 * H:]), 2)
    _close(torch.einsum('lbg,lbh->gh', d_gh, h_prev), zero(leaf['w_hh']), 'd w_hh from (dr, dz, dn r)')
    _close(d_gh.sum((0, 1)), zero(leaf['b_hh']), 'd b_hh')
    _close(torch.einsum('lbg,lbe->ge', got['d_gates'][:, :, :3 * H], fwd['contexts']), zero(leaf['w_ic']), 'd w_ic')
    _close(torch.einsum('lba,lbh->ah', got['d_rec'], h_prev), zero(leaf['w_rec']), 'd w_rec')
    _close(torch.einsum('lbt,lbe->tbe', fwd['att'], got['d_contexts']), zero(leaf['encoded']), 'd encoded')
    # the pre-fill is kept bit for bit at and past len, and the teacher-forced reverse scan fed its
    # own d_gates and d_rec is the free one
    forced = ar.backward(c, fwd, forced=got)
    for k in ar.GRU_BWD_KEYS:
        _close(forced[k], got[k], k)


def test_gates_record_is_r_z_n_ghn():
    """the fourth quarter of the record is gh_n = (w_hh h + b_hh)_n, what r multiplies"""
    c = ar.build('gru/T33B3L4A12E36H20')
    fwd = ar.forward(c)
    H = c['spec']['H']
    h_prev = torch.cat((c['h0'].double()[None], fwd['states'][:-1]))
    gh = h_prev @ c['w_hh'].double().t() + c['b_hh'].double()
    _close(fwd['gates'][:, :, 3 * H:], gh[:, :, 2 * H:], 'gh_n')
    r, z, n = (fwd['gates'][:, :, i * H:(i + 1) * H] for i in range(3))
    _close(fwd['states'], (1 - z) * n + z * h_prev, 'states')
    gi_n = c['gx_emb'].double()[:, :, 2 * H:] + fwd['contexts'] @ c['w_ic'].double()[2 * H:].t()
    _close(n, torch.tanh(gi_n + r * gh[:, :, 2 * H:]), 'n')
