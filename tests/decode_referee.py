"""fp64 referees of the three kernels that run once per label step of beam-search decoding
(include/asr_amd.h): asr_beam_step_f32, asr_tcn_attention_step_f32 and asr_att_gru_scan_fwd_f32
with L = 1 and beam > 1.  One launch at a time: random logits give decision margins of 1e-4 to
1e-5 once there are hundreds of candidates, so a whole trajectory of a device search against a
host search at beam 32 is decided by rounding; one launch from a given state is not.

Written from the header and from modules/beam_search.py, modules/tcn.py and
modules/decoders/attention_decoder.py; plain numpy / torch on the CPU, no native calls.  Every
reference takes `dtype` (the same arithmetic in fp32 is the yardstick the kernels' tolerance is
measured with) and `mut`, one wrong term, for tests/test_decode_referee.py, which proves on the
CPU that the case matrix below tells the mutants from the real thing.

The beam step decides by comparing scores.  `beam_step_ref` returns, beside the expected
outputs, the margin of every kind of decision of the launch; a comparison counts only where it
is live (finite operands, an outcome that can change an output).  The cases below are seeded so
that every margin is above MARGIN_FLOOR = 1e-3, 10x the score error allowed to the kernel;
the tie cases are exact instead (dyadic logits, zero running scores).

Hypotheses whose running score is -inf (the padding of `_get_topk` when an utterance has fewer
candidates than beams, and all their descendants) are dead: they can never finish, never win
a comparison against a live one, and the EOS test reads -inf for their row.  Which -inf
candidate fills a slot is a tie: the stable sort gives the lowest flat index (torch.topk on the
host leaves it unspecified, so the comparison with the host class looks at live slots only)."""
import numpy as np
import torch

F64 = torch.float64
EPS32 = 2.0 ** -23
MARGIN_FLOOR = 1e-3
MASKED = -1e5                       # additive score of a padded encoder frame (both decoders)
POISON = -7                         # pre-fill of what a launch must leave alone
LENGTH_NORMALIZATION = 0.6
INF = float('inf')

# |tanh(x) - (1 - 2 / (exp(2x) + 1))| of the kernels' fp32 form: 2^-23 from the rounding of the
# exp argument times |x| (1 - tanh^2) <= 0.45, 2^-23 from the sum at 2 / (e + 1) <= 2, 2^-24 from
# the quotient, 2^-24 from the difference: below 2^-21.  Measured through the kernel (A = 1,
# w = 1: the log of the alignment is tanh(x) up to a constant) on the MI355X: 4.3e-7 for the
# difference of two values, the softmax's own rounding included.
TANH_ABS = 2.0 ** -21


# ------------------------------------------------------------------ beam step

BEAM_MUTANTS = ('eos_row_b_times_beam', 'count_below_beam', 'normalised_score_stored',
                'highest_index_on_ties', 'first_step_all_beams', 'padding_repeats_index_0')


def len_div(step):
    return float(step ** LENGTH_NORMALIZATION) if step > 0 else 1.0


def fresh_state(B, Lcap):
    return dict(finished_count=np.zeros(B, np.int32), best_score=np.full(B, -INF, np.float32),
                best_len=np.zeros(B, np.int32), best_tokens=np.zeros((B, Lcap), np.int32),
                done=np.zeros(3, np.int32))


def _finite(*xs):
    return all(np.isfinite(x) for x in xs)


def beam_step_ref(logits, scores_in, est_in, step, B, beam, len_div, state, dtype=np.float64,
                  mut=None):
    """One asr_beam_step_f32 launch = BeamSearch.step + _save_best_finished, quirks included.
    logits [B*beam, C], scores_in [B*beam], est_in [B*beam, Lcap] (`step` labels each), state =
    dict finished_count [B], best_score [B], best_len [B], best_tokens [B, Lcap], done [3]
    (host copies of what the kernel received; not modified).
    -> (out, margins).  out: scores_out [B*beam], est [B*beam, step+1], new_input, parent,
    the state fields after the launch, improved [B] (utterances whose best finished hypothesis
    was replaced) and noop (the done flag was set: nothing may change).  margins: the smallest
    difference of each kind of live comparison (inf where there was none):
      topk_cut       last kept against first dropped candidate
      topk_adjacent  neighbouring kept candidates (their order is the order of the slots)
      eos_vs_class   EOS against the best other class of flat row b
      eos_beams      best against second-best normalised EOS score of the utterance's beams
      best_vs_eos    best_score[b] against the winning normalised EOS score"""
    logits = np.asarray(logits)
    hyps, C = logits.shape
    Cm = C - 1
    assert hyps == B * beam
    st = {k: np.array(state[k], copy=True) for k in
          ('finished_count', 'best_score', 'best_len', 'best_tokens', 'done')}
    st['best_score'] = st['best_score'].astype(dtype)
    m = dict(topk_cut=INF, topk_adjacent=INF, eos_vs_class=INF, eos_beams=INF, best_vs_eos=INF)
    out = dict(st, noop=bool(st['done'][0]), improved=np.zeros(B, bool))
    if out['noop']:
        return out, m
    local = torch.log_softmax(torch.from_numpy(logits.astype(dtype)), 1).numpy()
    g = local + np.asarray(scores_in).astype(dtype)[:, None]            # global scores

    # ---- best finished hypothesis (_save_best_finished; not before the first label)
    if step > 0:
        for b in range(B):
            # quirk: is_eos_best is indexed with the batch id, i.e. reads FLAT row b
            row = g[b * beam if mut == 'eos_row_b_times_beam' else b]
            eos_best = int(np.argmax(row)) == Cm                        # first maximum
            open_ = (st['finished_count'][b] < beam if mut == 'count_below_beam'
                     else st['finished_count'][b] <= beam)
            if open_ and _finite(row[Cm], row[:Cm].max()):
                m['eos_vs_class'] = min(m['eos_vs_class'], abs(row[Cm] - row[:Cm].max()))
            if not (eos_best and open_):
                continue
            st['finished_count'][b] += 1
            raw = g[b * beam:(b + 1) * beam, Cm]
            nrm = raw / np.asarray(len_div, dtype)
            ind = int(np.argmax(nrm))                                   # first maximum
            if _finite(st['best_score'][b], nrm[ind]):
                m['best_vs_eos'] = min(m['best_vs_eos'], abs(st['best_score'][b] - nrm[ind]))
            if st['best_score'][b] < nrm[ind]:
                others = np.delete(nrm, ind)
                if others.size and _finite(nrm[ind], others.max()):
                    m['eos_beams'] = min(m['eos_beams'], nrm[ind] - others.max())
                # quirk: the aliased score lists keep the RAW score
                st['best_score'][b] = nrm[ind] if mut == 'normalised_score_stored' else raw[ind]
                st['best_tokens'][b, :step] = est_in[b * beam + ind, :step]
                st['best_len'][b] = step
                out['improved'][b] = True

    # ---- top-`beam` of the non-EOS extensions; the first step looks at beam 0 only
    ncand = (beam if step > 0 or mut == 'first_step_all_beams' else 1) * Cm
    scores_out = np.empty(hyps, dtype)
    parent = np.empty(hyps, np.int32)
    letter = np.empty(hyps, np.int32)
    for b in range(B):
        cand = g[b * beam:(b + 1) * beam, :Cm].reshape(-1)[:ncand]
        if mut == 'highest_index_on_ties':
            order = ncand - 1 - np.argsort(-cand[::-1], kind='stable')
        else:
            order = np.argsort(-cand, kind='stable')                    # lowest index wins a tie
        k = min(beam, ncand)
        sel, val = order[:k], cand[order[:k]]
        if ncand > k and _finite(val[-1], cand[order[k]]):
            m['topk_cut'] = min(m['topk_cut'], val[-1] - cand[order[k]])
        live = val[np.isfinite(val)]
        if live.size > 1:
            m['topk_adjacent'] = min(m['topk_adjacent'], float(-np.diff(live).max()))
        if k < beam:                            # _get_topk's second branch
            last = 0 if mut == 'padding_repeats_index_0' else sel[-1]
            sel = np.concatenate([sel, np.full(beam - k, last)])
            val = np.concatenate([val, np.full(beam - k, -INF, dtype)])
        sl = slice(b * beam, (b + 1) * beam)
        scores_out[sl], parent[sl], letter[sl] = val, b * beam + sel // Cm, sel % Cm
    est = np.concatenate([np.asarray(est_in)[parent, :step], letter[:, None]], 1).astype(np.int32)

    # ---- all finished?  (has_finished, evaluated on the device)
    st['done'][2] += 1
    if int((st['finished_count'] < beam).sum()) == 0:
        st['done'][0] = 1
    st['done'][1] = 0
    out.update(st, scores_out=scores_out, est=est, new_input=letter, parent=parent)
    return out, m


def min_margin(m):
    return min(m.values())


def beam_logits(B, beam, C, seed, steps, eos_bias=25.0):
    """the scripted logits of a trajectory: 30 N(0,1) with eos_bias on EOS, [steps, B*beam, C]"""
    gen = torch.Generator().manual_seed(seed)
    x = 30 * torch.randn(steps, B * beam, C, generator=gen)
    x[:, :, -1] += eos_bias
    return x.numpy()


def run_trajectory(B, beam, C, logits, mut=None):
    """the referee free-running in fp64 from fresh state over logits [steps, B*beam, C]
    -> [(out, margins)] per step"""
    steps = logits.shape[0]
    Lcap = steps + 1
    state = fresh_state(B, Lcap)
    scores = np.zeros(B * beam)
    est = np.zeros((B * beam, Lcap), np.int32)
    res = []
    for s in range(steps):
        out, m = beam_step_ref(logits[s], scores, est, s, B, beam, len_div(s), state, mut=mut)
        res.append((out, m))
        if out['noop']:
            continue
        scores = out['scores_out']
        est = np.zeros((B * beam, Lcap), np.int32)
        est[:, :s + 1] = out['est']
        state = {k: out[k] for k in state}
    return res


# (B, beam, C) -> seed of beam_logits with a minimum margin > 1.5e-3 over 12 steps from fresh
# state (test_decode_referee.py asserts > MARGIN_FLOOR over them)
TRAJECTORIES = {(1, 1, 2): 0, (3, 3, 5): 0, (2, 10, 50): 0, (1, 32, 65): 0, (4, 8, 4): 0,
                (5, 32, 3): 0, (7, 10, 50): 0, (2, 16, 129): 3, (3, 32, 65): 81}
TRAJECTORY_STEPS = 12
FINISHING = ((3, 3, 5), 1, 60.0)        # shape, seed, EOS bias: every utterance done in the 6th launch

SINGLE_SHAPES = tuple(TRAJECTORIES) + ((40, 4, 7), (2, 32, 9))
SINGLE_LCAP = 12
SINGLE_STEPS = (0, 1, 7, SINGLE_LCAP - 1)
# (B, beam, C, step) -> seed of beam_case with every margin > 1.5e-3 (0 where not listed)
SINGLE_SEEDS = {(3, 32, 65, 1): 3, (3, 32, 65, 7): 1}
SINGLE_CASES = [s + (t,) for s in SINGLE_SHAPES for t in SINGLE_STEPS]


def single_case(B, beam, C, step):
    return beam_case(B, beam, C, step, SINGLE_SEEDS.get((B, beam, C, step), 0))


def beam_case(B, beam, C, step, seed, Lcap=SINGLE_LCAP):
    """One launch from arbitrary state: scores_in ~ 5 N(0,1) with a fifth of the entries -inf,
    random label histories over random best_tokens, finished_count from {0, beam-1, beam,
    beam+1}, best_score from {-inf, far below, far above} per utterance."""
    gen = torch.Generator().manual_seed(1000 * seed + step)
    hyps = B * beam
    logits = 30 * torch.randn(hyps, C, generator=gen)
    logits[:, -1] += 25
    scores = 5 * torch.randn(hyps, generator=gen)
    scores[torch.rand(hyps, generator=gen) < 0.2] = -INF
    if step == 0:
        scores[::beam] = 5 * torch.randn(B, generator=gen)      # beam 0 is what step 0 reads
    pick = lambda vals: torch.tensor(vals)[torch.randint(len(vals), (B,), generator=gen)]  # noqa: E731
    state = dict(
        finished_count=pick([0, max(beam - 1, 0), beam, beam + 1]).to(torch.int32).numpy(),
        best_score=pick([-INF, -1e4, 1e4]).to(torch.float32).numpy(),
        best_len=torch.randint(0, Lcap, (B,), generator=gen).to(torch.int32).numpy(),
        best_tokens=torch.randint(0, C, (B, Lcap), generator=gen).to(torch.int32).numpy(),
        done=np.array([0, 0, step], np.int32))
    est_in = torch.randint(0, C - 1, (hyps, Lcap), generator=gen).to(torch.int32).numpy()
    return dict(logits=logits.numpy(), scores_in=scores.numpy(), est_in=est_in, step=step, B=B,
                beam=beam, C=C, Lcap=Lcap, len_div=len_div(step), state=state)


def tie_cases():
    """Exact cases: dyadic logits and zero running scores, so that equal logits give bit-equal
    log-softmax values whatever the reduction order.  -> {name: case}"""
    def case(rows, B, beam, step=1, fc=0):
        logits = np.array(rows, np.float32)
        hyps, C = logits.shape
        est = (np.arange(hyps * SINGLE_LCAP, dtype=np.int32).reshape(hyps, -1) * 3) % (C - 1)
        est[:, 0] = np.arange(hyps) % (C - 1)           # the beams' histories differ
        st = fresh_state(B, SINGLE_LCAP)
        st['finished_count'][:] = fc
        st['best_tokens'][:] = POISON
        return dict(logits=logits, scores_in=np.zeros(hyps, np.float32), est_in=est, step=step, B=B,
                    beam=beam, C=C, Lcap=SINGLE_LCAP, len_div=len_div(step), state=st)
    row = [1.0, 0.5, -2.0, 0.25, -1.0]
    eos = [1.0, 0.5, -2.0, 0.25, 4.0]
    return {
        'all_equal_row': case([[0.0] * 5, [0.5, 0.25, -1.0, 2.0, 0.0]], 1, 2),
        'all_equal_everywhere': case([[0.0] * 5] * 6, 2, 3),
        'identical_rows': case([row, row, row], 1, 3),
        'eos_equals_best_class': case([[3.0, 1.0, 3.0], [0.0, 1.0, 5.0], [2.0, 2.0, 2.0], [1.0, 0.0, 9.0]], 2, 2),
        'equal_eos_scores': case([eos, eos, eos], 1, 3),
        'first_step_equal': case([[0.0] * 4, [5.0] * 4], 1, 2, step=0),
    }


def beam_tolerance(case, want):
    """4x the distance of the same step in fp32 on the CPU (torch.log_softmax + add) from fp64,
    plus 4 fp32 ulps of the largest operand -> (tolerance, the fp32 distance)"""
    f32, _ = beam_step_ref(case['logits'], case['scores_in'], case['est_in'], case['step'], case['B'],
                           case['beam'], case['len_div'], case['state'], dtype=np.float32)
    d = 0.0
    if not want['noop']:
        d = _max_finite_diff(f32['scores_out'], want['scores_out'])
    d = max(d, _max_finite_diff(f32['best_score'], want['best_score']))
    s = np.asarray(case['scores_in'], np.float64)
    mag = max(float(np.abs(case['logits']).max()), float(np.abs(s[np.isfinite(s)]).max(initial=0.0)))
    return 4 * d + 4 * EPS32 * mag, d


def _max_finite_diff(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = np.isfinite(a) & np.isfinite(b) & (np.abs(b) < 1e3)       # (the far-away best_score presets are copies)
    return float(np.abs(a[ok] - b[ok]).max(initial=0.0))


def kernel_view(case, out, est_prefill=None):
    """what the launch leaves in the kernel's buffers, given the outputs `out` of a reference
    (a stand-in for the kernel): est_out pre-filled with POISON"""
    hyps, Lcap, step = case['B'] * case['beam'], case['Lcap'], case['step']
    est_out = np.full((hyps, Lcap), POISON, np.int32) if est_prefill is None else est_prefill.copy()
    got = {k: np.array(out[k], copy=True) for k in ('finished_count', 'best_score', 'best_len', 'best_tokens', 'done')}
    if out['noop']:
        got.update(est_out=est_out, scores_out=None, new_input=None, parent=None)
        return got
    est_out[:, :step + 1] = out['est']
    got.update(est_out=est_out, scores_out=out['scores_out'], new_input=out['new_input'], parent=out['parent'])
    return got


def judge_beam_step(case, got, want, tol, est_before=None):
    """got: dict est_out [hyps, Lcap] (pre-filled with POISON), scores_out, new_input, parent,
    finished_count, best_score, best_len, best_tokens, done after the launch.  Integer outputs
    bit-equal, scores within tol (and -inf exactly where -inf is due), untouched entries still
    what they were (est_before: the contents of est_out before the launch, POISON by default).
    -> list of complaints"""
    bad = []
    step = case['step']
    before = np.full_like(got['est_out'], POISON) if est_before is None else est_before

    def same(name, a, b):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape or not np.array_equal(a, b):
            n = int((a != b).sum()) if a.shape == b.shape else -1
            bad.append('%s: %d entries differ (got %s want %s)' % (name, n, a.ravel()[:12], b.ravel()[:12]))

    def close(name, a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        fin = np.isfinite(b)
        if not np.array_equal(a[~fin], b[~fin]):
            bad.append('%s: non-finite entries differ' % name)
        err = np.abs(a[fin] - b[fin])
        if err.size and not (err <= tol).all():       # NaN fails
            bad.append('%s: max error %.3g > tol %.3g' % (name, float(np.nanmax(err)), tol))

    for k in ('finished_count', 'best_len', 'best_tokens', 'done'):
        same(k, got[k], want[k])
    keep = ~want['improved']
    same('best_score (kept)', np.asarray(got['best_score'], np.float32)[keep],
         np.asarray(case['state']['best_score'], np.float32)[keep])
    close('best_score', np.asarray(got['best_score'])[~keep], want['best_score'][~keep])
    if want['noop']:
        same('est_out (no-op)', got['est_out'], before)
        return bad
    same('est_out[:, :step+1]', got['est_out'][:, :step + 1], want['est'])
    same('est_out beyond step', got['est_out'][:, step + 1:], before[:, step + 1:])
    same('new_input', got['new_input'], want['new_input'])
    same('parent', got['parent'], want['parent'])
    close('scores_out', got['scores_out'], want['scores_out'])
    return bad


# ------------------------------------------------------------------ local-attention step

ATT_MUTANTS = ('parent_ignored', 'mask_after_len')
KF = 32


def _tanh(x, form):
    """form 'exp': the kernels' 1 - 2 / (exp(2x) + 1) in the dtype of x"""
    return torch.tanh(x) if form is None else 1 - 2 / (torch.exp(2 * x) + 1)


def tcn_attention_step_ref(eproj, enc, lens, filt, glob, w_score, b_score, temperature, att_prev,
                           parent, beam, dtype=F64, mut=None, tanh_form=None):
    """LocalAttention.forward + the context sum of enc_step for hypotheses h = u * beam + k:
    att_new[h] = softmax_t((w . tanh(eproj[t, u] + sum_j a[t - (Kf-1) + j] filt[h, :, j] + glob[h])
    + b) * temperature + pad_t) with a = att_prev[parent[h]] left-padded with zeros and
    pad_t = -1e5 for t >= lens[u]; context[h] = sum_t att_new[h, t] enc[t, u].
    eproj [T, B, A], enc [T, B, E], filt [B*beam, A, Kf], glob [B*beam, A], att_prev [B*beam, T]
    -> (att_new [B*beam, T], context [B*beam, E])"""
    c = lambda x: torch.as_tensor(x).to(dtype)  # noqa: E731
    T, B, A = eproj.shape
    hyps = B * beam
    u = torch.arange(hyps) // beam
    src = torch.arange(hyps) if parent is None or mut == 'parent_ignored' else torch.as_tensor(parent).long()
    a = torch.cat([torch.zeros(hyps, KF - 1, dtype=dtype), c(att_prev)[src]], 1)
    f = c(filt).view(hyps, A, KF)
    hid = c(eproj).permute(1, 0, 2)[u] + c(glob)[:, None, :]                   # [hyps, T, A]
    for j in range(KF):
        hid = hid + a[:, j:j + T, None] * f[:, None, :, j]
    e = (_tanh(hid, tanh_form) @ c(w_score) + b_score) * temperature
    ln = torch.as_tensor(lens).long()[u][:, None]
    t = torch.arange(T)[None, :]
    e = e + ((t > ln) if mut == 'mask_after_len' else (t >= ln)).to(dtype) * MASKED
    att = torch.softmax(e, 1)
    ctx = torch.einsum('ht,the->he', att, c(enc)[:, u])
    return att, ctx


ATT_SHAPES = ((1, 1, 1, 4, 4), (31, 2, 3, 8, 20), (32, 2, 3, 8, 20), (255, 1, 2, 64, 320),
              (256, 1, 2, 64, 320), (257, 2, 2, 64, 321), (334, 3, 10, 64, 320), (600, 1, 1, 16, 7))
ATT_CASES = [(s, d) for s in ATT_SHAPES for d in (0, 1)]


def att_case(shape, draw):
    """draw 0: parent None; draw 1: a random map within each utterance that is no bijection,
    and (at T' = 32 and 257) filters scaled so that |hid| reaches about 60.  Lengths mix T', 1 and
    a value just past a 256-frame chunk."""
    T, B, beam, A, E = shape
    gen = torch.Generator().manual_seed(T * 131 + B * 17 + beam + draw * 7919)
    hyps = B * beam
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    past = 257 if T > 257 else max(1, T // 2)
    lens = torch.tensor(([T, 1, past] if draw == 0 else [past, T, 1])[:B] if B > 1 else
                        [[T, 1 if T < 300 else past][draw]], dtype=torch.int32)
    sat = draw == 1 and T in (32, 257)
    parent = None
    if draw == 1:
        k = torch.randint(0, beam, (hyps,), generator=gen)
        if beam > 1:
            k[0::beam] = k[1::beam]                         # two survivors of one parent
        parent = ((torch.arange(hyps) // beam) * beam + k).to(torch.int32)
    return dict(eproj=r(T, B, A), enc=r(T, B, E), lens=lens, filt=r(hyps, A, KF) * (400.0 if sat else 0.5),
                glob=r(hyps, A), w_score=r(A) * 2 / A ** 0.5, b_score=0.3, temperature=1.25,
                att_prev=torch.softmax(2 * r(hyps, T), 1), parent=parent, beam=beam, sat=sat)


def att_args(c, dev=None):
    """positional operands of _native.tcn_attention_step / tcn_attention_step_ref"""
    mv = (lambda x: x) if dev is None else (lambda x: x.to(dev) if torch.is_tensor(x) else x)
    return tuple(mv(c[k]) for k in ('eproj', 'enc', 'lens', 'filt', 'glob', 'w_score', 'b_score',
                                    'temperature', 'att_prev', 'parent', 'beam'))


def att_tolerance(c, want):
    """(tol_att, tol_ctx, fp32 distances): 4x the distance of the fp32 evaluation from fp64 plus
    the tanh term: an error d = temperature * sum|w| * TANH_ABS of a score moves an alignment by
    at most 2 d of itself, and the context by 2 d max|enc|"""
    a32, c32 = tcn_attention_step_ref(*att_args(c), dtype=torch.float32)
    d_att = float((a32.double() - want[0]).abs().max())
    d_ctx = float((c32.double() - want[1]).abs().max())
    de = 2 * c['temperature'] * float(c['w_score'].abs().sum()) * TANH_ABS
    return (4 * d_att + de * float(want[0].max()) + 4 * EPS32 * float(want[0].max()),
            4 * d_ctx + de * float(c['enc'].abs().max()) + 4 * EPS32 * float(want[1].abs().max()),
            d_att, d_ctx)


def judge_att_step(c, got_att, got_ctx, want, tols):
    bad = []
    att, ctx = got_att.double(), got_ctx.double()
    for name, g, w, tol in (('att_new', att, want[0], tols[0]), ('context', ctx, want[1], tols[1])):
        err = (g - w).abs().max()
        if not bool(err <= tol):
            bad.append('%s: max error %.3g > tol %.3g' % (name, float(err), tol))
    if not bool(((att.sum(1) - 1).abs() <= 1e-5).all()):
        bad.append('rows do not sum to 1: %.3g' % float((att.sum(1) - 1).abs().max()))
    T = att.shape[1]
    ln = c['lens'].long().repeat_interleave(c['beam'])[:, None]
    behind = torch.arange(T)[None, :] >= ln
    if bool((att[behind] != 0).any()):          # exp(-1e5 + O(100)) underflows in every format
        bad.append('%d frames at or past len are not exactly 0' % int((att[behind] != 0).sum()))
    return bad


ATT_STEP_MAX_FRAMES = 8160      # (Kf - 1 + 2 T' + 32) floats of LDS <= 64 KiB


# ------------------------------------------------------------------ attention-GRU step

GRU_MUTANTS = ('u_is_b_mod_nu', 'len_0_is_empty')


def att_gru_step_ref(eproj, encoded, lens, gx_emb, w_ic, w_hh, b_hh, w_rec, w_score, b_score, h0,
                     beam, dtype=F64, mut=None, tanh_form=None, records=False):
    """One position of AttentionDecoderRNN._step for B = NU * beam hypotheses; hypothesis b reads
    utterance b // beam; a length of 0 or above T' means T' (clamp_len).
      rec = w_rec h0;  a = softmax_t(w_score . tanh(eproj[t, u] + rec) + b_score + pad_t)
      c = sum_t a[t] encoded[t, u];  gi = gx_emb + w_ic c;  gh = w_hh h0 + b_hh
      r = s(gi_r + gh_r)  z = s(gi_z + gh_z)  n = tanh(gi_n + r gh_n)  h = (1 - z) n + z h0
    eproj [T, NU, A], encoded [T, NU, E], gx_emb [B, 3H], h0 [B, H] -> (att [B, T], states [B, H]);
    with records=True also what the scan saves for its backward pass: contexts [B, E], gates [B, 4H]
    = (r, z, n, gh_n) and rec [B, A] (tests/attention_scan_referee.py)"""
    c = lambda x: torch.as_tensor(x).to(dtype)  # noqa: E731
    T, NU, A = eproj.shape
    B, H = h0.shape
    b = torch.arange(B)
    u = b % NU if mut == 'u_is_b_mod_nu' else b // beam
    ln = torch.as_tensor(lens).long()[u]
    empty = (ln == 0) if mut == 'len_0_is_empty' else torch.zeros(B, dtype=torch.bool)
    ln = torch.where((ln <= 0) | (ln > T), torch.full_like(ln, T), ln)
    h0 = c(h0)
    rec = h0 @ c(w_rec).t()
    e = _tanh(c(eproj).permute(1, 0, 2)[u] + rec[:, None, :], tanh_form) @ c(w_score) + c(b_score)
    e = e + (torch.arange(T)[None, :] >= ln[:, None]).to(dtype) * MASKED
    att = torch.softmax(e, 1) * (~empty)[:, None].to(dtype)
    ctx = torch.einsum('bt,tbe->be', att, c(encoded)[:, u])
    gi = (c(gx_emb) + ctx @ c(w_ic).t()).view(B, 3, H)
    gh = (h0 @ c(w_hh).t() + c(b_hh)).view(B, 3, H)
    r = torch.sigmoid(gi[:, 0] + gh[:, 0])
    z = torch.sigmoid(gi[:, 1] + gh[:, 1])
    n = torch.tanh(gi[:, 2] + r * gh[:, 2])
    if records:
        return att, (1 - z) * n + z * h0, ctx, torch.cat((r, z, n, gh[:, 2]), 1), rec
    return att, (1 - z) * n + z * h0


GRU_SHAPES = ((1, 1, 1, 4, 4, 4), (50, 3, 4, 64, 320, 256), (334, 2, 10, 128, 512, 320),
              (70, 5, 32, 320, 64, 64), (33, 2, 3, 12, 36, 20))
GRU_KEYS = ('eproj', 'encoded', 'lens', 'gx_emb', 'w_ic', 'w_hh', 'b_hh', 'w_rec', 'w_score',
            'b_score', 'h0')


def gru_case(shape):
    """Lengths include 0 (= T'), T' and one above T'; every utterance has its own encoder rows."""
    T, NU, beam, A, E, H = shape
    gen = torch.Generator().manual_seed(T * 37 + NU * 11 + beam)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    B = NU * beam
    lens = torch.tensor([0, T, max(1, T // 3), T + 5, max(1, T - 1)][:NU], dtype=torch.int32)
    if NU == 2:
        lens = torch.tensor([max(1, T // 3), 0], dtype=torch.int32)
    return dict(eproj=r(T, NU, A), encoded=r(T, NU, E), lens=lens, gx_emb=r(B, 3 * H),
                w_ic=r(3 * H, E) / E ** 0.5, w_hh=r(3 * H, H) / H ** 0.5, b_hh=0.1 * r(3 * H),
                w_rec=r(A, H) / H ** 0.5, w_score=2 * r(A) / A ** 0.5, b_score=torch.tensor([0.3]),
                h0=0.5 * r(B, H), beam=beam)


def gru_args(c, dev=None):
    mv = (lambda x: x) if dev is None else (lambda x: x.to(dev))
    return tuple(mv(c[k]) for k in GRU_KEYS)


def gru_tolerance(c, want):
    """(tol_att, tol_states, fp32 distances): 4x the distance of the fp32 evaluation (with the
    kernel's exp form of the attention tanh) from fp64, plus 4 fp32 ulps of the largest value,
    plus, for the alignment, the tanh term of att_tolerance"""
    a32, s32 = att_gru_step_ref(*gru_args(c), c['beam'], dtype=torch.float32, tanh_form='exp')
    d_att = float((a32.double() - want[0]).abs().max())
    d_st = float((s32.double() - want[1]).abs().max())
    de = 2 * float(c['w_score'].abs().sum()) * TANH_ABS
    return (4 * d_att + (de + 4 * EPS32) * float(want[0].max()),
            4 * d_st + 4 * EPS32 * max(1.0, float(want[1].abs().max())), d_att, d_st)


def judge_gru_step(c, got_att, got_states, want, tols):
    bad = []
    for name, g, w, tol in (('att', got_att.double(), want[0], tols[0]),
                            ('states', got_states.double(), want[1], tols[1])):
        err = (g - w).abs().max()
        if not bool(err <= tol):
            bad.append('%s: max error %.3g > tol %.3g' % (name, float(err), tol))
    return bad
