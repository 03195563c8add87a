"""fp64 referee of asr_tcn_attention_step_win_f32 (include/asr_amd.h): the local-attention
decode step under LocalAttention's force_forward window, one launch at a time, beside the
referees of tests/decode_referee.py, whose operands, cases and tolerance rule it reuses.

Written from the header and from modules/tcn.py (LocalAttention.recompute_forward_mask); plain
torch on the CPU, no native calls.  With a = att_prev[parent[h]]:

    peak = max_t a[t], where = the FIRST t with a[t] = peak, active = peak >= float32(0.1)
    m(t) = [t >= len] + [active and (t < where + lo or t >= where + hi)]        masks on frame t
    att_new = softmax_t(score_t + m(t) * -1e5), context = sum_t att_new[t] enc[t]

`window_masks` also returns what the launch's rows exercise (`kinds`), so that the tests can
assert that the matrix below reaches every corner the kernel has a branch for.  Frames with
m(t) > min_t m(t) are off the support: the kernel writes an exact zero there.

Mutants, one wrong term each (tests/test_tcn_ff.py proves on the CPU that the matrix tells each
from the real thing): peak_from_own_row, hi_inclusive, lo_exclusive, mask_when_diffuse,
last_max_wins, single_mask_when_both."""
import numpy as np
import torch

import decode_referee as dr

F64 = dr.F64
MASKED = dr.MASKED
KF = dr.KF
# the reference compares the fp32 peak with the double 0.1: no fp32 value lies between that and
# float32(0.1), so on fp32 rows `not peak < 0.1` is `peak >= float32(0.1)`
ACTIVE_FROM = float(np.float32(0.1))

FF_MUTANTS = ('peak_from_own_row', 'hi_inclusive', 'lo_exclusive', 'mask_when_diffuse',
              'last_max_wins', 'single_mask_when_both')
FF_WINDOWS = ((-10, 50), (-2, 6), (1, 6), (0, 1))
FF_SHAPES = ((1, 1, 1, 4, 4), (9, 2, 3, 8, 20), (40, 3, 3, 8, 16), (255, 1, 2, 64, 320),
             (257, 2, 2, 64, 321), (334, 3, 10, 64, 320), (600, 1, 1, 16, 7))
FF_CASES = [(s, d, w) for s in FF_SHAPES for d in (0, 1) for w in FF_WINDOWS]
FF_KINDS = ('inside', 'clipped_at_0', 'clipped_at_len', 'clipped_at_T', 'straddles_256',
            'behind_len', 'diffuse', 'peak_is_0.1f', 'tie_in_short_row', 'siblings_peak_elsewhere')


def window_masks(att_prev, parent, lens, beam, window, mut=None):
    """-> (m [hyps, T] int64: masks per frame, info dict: peak, where, active [hyps], kinds: the
    names of FF_KINDS (and 'clipped_to_nothing', 'two_pieces') that occur among the rows)"""
    a_all = torch.as_tensor(att_prev).double()
    hyps, T = a_all.shape
    own = torch.arange(hyps)
    par = own if parent is None else torch.as_tensor(parent).long()
    a = a_all[own if mut == 'peak_from_own_row' else par]
    t = torch.arange(T)[None, :]
    peak = a.max(1)[0]
    at_peak = a == peak[:, None]
    first = torch.where(at_peak, t, torch.full_like(t, T)).min(1)[0]       # explicit first maximum
    last = torch.where(at_peak, t, torch.full_like(t, -1)).max(1)[0]
    where = last if mut == 'last_max_wins' else first
    active = peak >= ACTIVE_FROM
    if mut == 'mask_when_diffuse':
        active = torch.ones_like(active)
    lo, hi = (where + window[0])[:, None], (where + window[1])[:, None]
    below = (t <= lo) if mut == 'lo_exclusive' else (t < lo)
    above = (t > hi) if mut == 'hi_inclusive' else (t >= hi)
    outside = (below | above) & active[:, None]
    ln = torch.as_tensor(lens).long().repeat_interleave(beam)[:, None]
    m = (t >= ln).long() + outside.long()
    if mut == 'single_mask_when_both':
        m = m.clamp(max=1)

    kinds = set()
    ln1, lo1, hi1 = ln[:, 0], lo[:, 0], hi[:, 0]
    ws, we = lo1.clamp(0, T), hi1.clamp(0, T)
    def note(name, cond):  # noqa: E306
        if bool((cond & active).any()):
            kinds.add(name)
    note('inside', (lo1 > 0) & (hi1 < ln1))
    note('clipped_at_0', (lo1 < 0) & (we > 0))
    note('clipped_at_len', (lo1 < ln1) & (ln1 < hi1) & (ln1 < T))
    note('clipped_at_T', (lo1 < T) & (hi1 > T))
    note('straddles_256', (ws < 256) & (256 < torch.minimum(we, ln1)))
    note('behind_len', (ws >= ln1) & (ws < we) & (ln1 < T))
    note('clipped_to_nothing', ws >= we)
    note('two_pieces', (ws > ln1) & (ws < we) & (ln1 > 0))
    note('peak_is_0.1f', peak == ACTIVE_FROM)
    note('tie_in_short_row', (at_peak.sum(1) > 1) & torch.tensor(T <= 10))
    if bool((~active).any()):
        kinds.add('diffuse')
    if parent is not None and len(par) == hyps:     # (rows and previous rows correspond: siblings)
        own_first = torch.where(a_all == a_all.max(1)[0][:, None], t, torch.full_like(t, T)).min(1)[0]
        elsewhere = (own_first != own_first[par]) & active
        for p in set(par.tolist()):
            if int(((par == p) & elsewhere).sum()) >= 2:
                kinds.add('siblings_peak_elsewhere')
    return m, dict(peak=peak, where=where, active=active, kinds=kinds)


def tcn_attention_step_win_ref(eproj, enc, lens, filt, glob, w_score, b_score, temperature,
                               att_prev, parent, beam, window, dtype=F64, mut=None, tanh_form=None):
    """decode_referee.tcn_attention_step_ref with m(t) * -1e5 in place of the padding term
    -> (att_new [B*beam, T], context [B*beam, E])"""
    c = lambda x: torch.as_tensor(x).to(dtype)  # noqa: E731
    T, B, A = eproj.shape
    hyps = B * beam
    u = torch.arange(hyps) // beam
    src = torch.arange(hyps) if parent is None else torch.as_tensor(parent).long()
    a = torch.cat([torch.zeros(hyps, KF - 1, dtype=dtype), c(att_prev)[src]], 1)
    f = c(filt).view(hyps, A, KF)
    hid = c(eproj).permute(1, 0, 2)[u] + c(glob)[:, None, :]                   # [hyps, T, A]
    for j in range(KF):
        hid = hid + a[:, j:j + T, None] * f[:, None, :, j]
    e = (dr._tanh(hid, tanh_form) @ c(w_score) + b_score) * temperature
    m, _ = window_masks(att_prev, parent, lens, beam, window, mut=mut)
    ln = (torch.arange(T)[None, :] >= torch.as_tensor(lens).long()[u][:, None])
    pad = ln.to(dtype) * MASKED
    e = e + (pad + (m - ln.long()).to(dtype) * MASKED)          # a frame with both carries -2e5
    att = torch.softmax(e, 1)
    ctx = torch.einsum('ht,the->he', att, c(enc)[:, u])
    return att, ctx


def off_support(c):
    """[hyps, T] bool: frames that carry more masks than the least masked frame of their row"""
    m, _ = window_masks(c['att_prev'], c['parent'], c['lens'], c['beam'], c['window'])
    return m > m.min(1, keepdim=True)[0]


def support_closed_form(where, active, ln, T, window):
    """the kernel's closed form of the support of one row (csrc/tcn_step.hip): -> (M, P, Q), the
    least number of masks on a frame and the two intervals [p0, p1), [q0, q1) that carry it"""
    lenc = min(max(int(ln), 0), T)
    p0, p1, q0, q1, M = 0, lenc, 0, 0, 0
    if active:
        ws = min(max(int(where) + window[0], 0), T)
        we = min(max(int(where) + window[1], 0), T)
        if ws < min(we, lenc):
            p0, p1 = ws, min(we, lenc)
        else:
            M = 1
            if ws < we:
                q0, q1 = ws, we
    if p1 - p0 + q1 - q0 == 0:
        M, p0, p1 = M + 1, 0, T
    return M, (p0, p1), (q0, q1)


def _crafted_row(kind, T, ln, gen):
    """one previous alignment (not normalised: the kernel does not ask for that) by kind"""
    row = 0.01 * torch.rand(T, generator=gen)
    ln = max(1, min(int(ln), T))
    if kind == 0:                                   # a sharp peak in the middle of the utterance
        row[ln // 2] = 0.7
    elif kind == 1:                                 # peak on the first frame
        row[0] = 0.6
    elif kind == 2:                                 # peak on the utterance's last frame
        row[ln - 1] = 0.5
    elif kind == 3:                                 # peak on the last frame of the row
        row[T - 1] = 0.9
    elif kind == 4:                                 # diffuse
        row = 0.05 + 0.04 * torch.rand(T, generator=gen)
    elif kind == 5:                                 # peak exactly float32(0.1)
        row[min(T - 1, 3)] = 0.1
    elif kind == 6:                                 # an exact tie of the maximum
        row[min(T - 1, 2)] = 0.4
        row[min(T - 1, 6)] = 0.4
    elif kind == 7:                                 # peak at frame 250: (-10, 50) straddles 256
        row[min(T - 1, 250)] = 0.8
    elif kind == 8:                                 # just below the threshold
        row[ln // 2] = float(np.nextafter(np.float32(0.1), np.float32(0)))
    return row


N_KINDS = 10        # kind 9: the random row of decode_referee.att_case


# lengths att_case never draws: 0 (every frame padded; with a window clipped to nothing every
# frame carries two masks) and values above T' (no frame padded), as (shape, draw, window, lens)
FF_LENGTH_CASES = [((40, 3, 3, 8, 16), d, w, lens) for d in (0, 1) for w in ((1, 6), (-2, 6))
                   for lens in ((0, 45, 40), (41, 0, 1000))]


def ff_case(shape, draw, window, lens=None):
    """decode_referee.att_case(shape, draw) with the window and with crafted previous alignments:
    row h is of kind (h + offset) % N_KINDS, the offset moving with shape, draw and window so
    that the one-row shapes get their share of the kinds too."""
    c = dr.att_case(shape, draw)
    T, B, beam = shape[0], shape[1], shape[2]
    gen = torch.Generator().manual_seed(T * 977 + draw * 31 + FF_WINDOWS.index(tuple(window)))
    offset = FF_SHAPES.index(tuple(shape)) * 5 + draw * 7 + FF_WINDOWS.index(tuple(window)) * 3
    if lens is not None:
        offset += 1 + list(lens).index(0)
    prev = c['att_prev'].clone()
    for h in range(B * beam):
        kind = (h + offset) % N_KINDS
        if kind != 9:
            prev[h] = _crafted_row(kind, T, c['lens'][h // beam], gen)
    if lens is not None:            # (the rows stay crafted for att_case's lengths)
        c = dict(c, lens=torch.tensor(lens, dtype=torch.int32))
    return dict(c, att_prev=prev, window=tuple(window))


def ff_args(c, dev=None):
    """positional operands of tcn_attention_step_win_ref; _native.tcn_attention_step takes the
    last one as `window=`"""
    return dr.att_args(c, dev) + (c['window'],)


def ff_tolerance(c, want):
    """decode_referee.att_tolerance with the windowed formula: 4x the distance of its fp32
    evaluation from fp64 plus the tanh term; no new constant"""
    a32, c32 = tcn_attention_step_win_ref(*ff_args(c), dtype=torch.float32)
    d_att = float((a32.double() - want[0]).abs().max())
    d_ctx = float((c32.double() - want[1]).abs().max())
    de = 2 * c['temperature'] * float(c['w_score'].abs().sum()) * dr.TANH_ABS
    return (4 * d_att + de * float(want[0].max()) + 4 * dr.EPS32 * float(want[0].max()),
            4 * d_ctx + de * float(c['enc'].abs().max()) + 4 * dr.EPS32 * float(want[1].abs().max()),
            d_att, d_ctx)


def kinds_seen(cases):
    """{kind: [cases]} over window_masks of every case"""
    seen = {}
    for key in cases:
        c = ff_case(*key)
        _, info = window_masks(c['att_prev'], c['parent'], c['lens'], c['beam'], c['window'])
        for k in info['kinds']:
            seen.setdefault(k, []).append(key)
    return seen


def judge_ff_step(c, got_att, got_ctx, want, tols):
    """within the tolerances, rows sum to 1 within 1e-5, every frame off the support exactly 0"""
    bad = []
    att, ctx = got_att.double(), got_ctx.double()
    for name, g, w, tol in (('att_new', att, want[0], tols[0]), ('context', ctx, want[1], tols[1])):
        err = (g - w).abs().max()
        if not bool(err <= tol):
            bad.append('%s: max error %.3g > tol %.3g' % (name, float(err), tol))
    if not bool(((att.sum(1) - 1).abs() <= 1e-5).all()):
        bad.append('rows do not sum to 1: %.3g' % float((att.sum(1) - 1).abs().max()))
    off = off_support(c)
    if bool((att[off] != 0).any()):
        bad.append('%d frames off the support are not exactly 0' % int((att[off] != 0).sum()))
    return bad


_WANT = {}


def want_of(key):
    """the fp64 referee's outputs and the tolerances of a case, computed once"""
    if key not in _WANT:
        c = ff_case(*key)
        want = tcn_attention_step_win_ref(*ff_args(c))
        _WANT[key] = (c, want, ff_tolerance(c, want))
    return _WANT[key]


# ------------------------------------------------------------------ tests/golden/tcn_beam_ff.npz

FIXTURE_KW = dict(tcn_hidden_size=24, att_hidden_size=8, dropout_p=0.0, kernel_size=3,
                  dilation_sizes=[1, 2], beam_size=3, length_normalization=0.6,
                  attention_temperature=1.25, tcn_layers_per_block=2, learnable_initial_attention=False)


def fixture_decoder(g, device, window='fixture'):
    from att_speech.modules.tcn import AttentionDecoderTCN
    enc = torch.from_numpy(g['enc'])
    if window == 'fixture':
        window = tuple(int(v) for v in g['window'])
    dec = AttentionDecoderTCN({'features': torch.zeros(enc.shape)}, int(g['S']),
                              att_force_forward=window, **FIXTURE_KW)
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('sd_')}
    assert set(sd) == set(dec.state_dict())
    dec.load_state_dict(sd)
    dec.TRANSCRIPTION_LEN_GUARD = int(g['guard'])
    return dec.eval().to(device), enc.to(device)


def as_lists(decoded):
    return [[int(c) for c in (d.tolist() if hasattr(d, 'tolist') else d)] for d in decoded]


def check_fixture_decode(g, res, beam, att_tol, score_tol):
    key = 'b%d_' % beam
    off, want = 0, []
    for n in g[key + 'lens']:
        want.append(g[key + 'flat'][off:off + n].tolist())
        off += n
    assert as_lists(res['decoded']) == want
    bs = res['beam_search']
    assert list(bs.finished_count) == g[key + 'finished_count'].tolist()
    np.testing.assert_array_equal(bs.estimations.cpu().numpy(), g[key + 'final_estimations'])
    np.testing.assert_allclose(bs.scores.cpu().numpy(), g[key + 'final_beam_scores'],
                               rtol=score_tol, atol=score_tol)
    np.testing.assert_allclose(np.array(res['decoded_scores']['acoustic'], np.float64),
                               g[key + 'scores'], rtol=score_tol, atol=score_tol)
    att = torch.stack([a.cpu() for a in res['attweights']]).numpy()
    assert att.shape == g[key + 'att'].shape
    np.testing.assert_allclose(att, g[key + 'att'], atol=att_tol)
