"""fp64 referees of the three launches of a device LM-fused beam-search step (include/asr_amd.h):
asr_lm_label_costs_f64, asr_beam_lm_step_f32 and asr_lm_bag_advance_f64.  Written from the header
and from modules/beam_search.py (BeamSearchLM); plain numpy on the CPU, no native calls.

The LM referees go the host's way (expand every bag through every label, close over the epsilon
arcs, reduce): they do not use arc_w_closed, the identity the kernel relies on.

`lm_beam_step_ref` returns, beside the expected outputs, the margin of every kind of live decision
of the launch (a comparison counts where its operands are finite and its outcome can change an
output).  The cases below are seeded so that every margin is above decode_referee.MARGIN_FLOOR; the
tie cases are exact instead (dyadic logits, zero LM weight).  `mut` plants one wrong term, for
tests/test_lm_beam_referee.py, which proves on the CPU that the case matrix tells the mutants from
the real thing."""
import os

import numpy as np
import torch

import decode_referee as dr

INF = float('inf')
POISON = dr.POISON
BAG_CAP = 32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

MUTANTS = ('padded_length_in_min_pos', 'coverage_not_reindexed', 'frozen_still_updating',
           'elements_of_finishing_step', 'z_omitted', 'closure_before_label', 'newest_first_on_ties')


# ------------------------------------------------------------------ LMs

def toy_lm():
    from att_speech.lm_fst import LmFst, SymbolTable
    g = np.load(os.path.join(GOLDEN, 'beam_lm.npz'))
    syms = SymbolTable([(0, '<eps>'), (1, '<spc>'), (2, 'a'), (3, 'b'), (4, 'c')])
    return LmFst(6, 0, g['lm_src'], g['lm_dst'], g['lm_il'], g['lm_il'], g['lm_w'], g['lm_final'],
                 syms, syms)


TOY_MAPPING = [1, 1, 1, 2, 3, 4, 1]          # classes <pad> <unk> ' ' a b c <eos>  (C = 7)
_LMS = {}


def shipped_lm(order):
    from att_speech.lm_fst import LmFst
    if order not in _LMS:
        _LMS[order] = LmFst.read(os.path.join(GOLDEN, 'G_char_%s_syms.fst.gz' % order))
    return _LMS[order]


def wsj_mapping(lm, num_classes=None):
    """tcn.py create_alphabet_mapping over wsj_vocabulary.txt (+ EOS), cut to num_classes"""
    with open(os.path.join(GOLDEN, 'wsj_vocabulary.txt')) as f:
        vocab = [line.rstrip('\n') for line in f]
    while vocab and vocab[-1] == '':
        vocab.pop()
    label_of = {sym: lab for lab, sym in lm.input_symbols()}
    names = ['<spc>' if s == ' ' else s for s in vocab + ['<eos>']]
    m = [label_of.get(n, label_of['<spc>']) for n in names]
    if num_classes is not None:
        m = (m + [label_of['<spc>']] * num_classes)[:num_classes]
    return m


def walk_bag(lm, labels):
    """the bag of a hypothesis that read `labels` (LM labels) from the start state"""
    from att_speech import fst_utils as P
    bag = P.expand_epsilon(lm, {lm.start(): 0.0}, True)      # (the shipped LMs leave their start state over an epsilon arc)
    for l in labels:
        nxt = P.expand(lm, bag, int(l), True)
        if nxt:
            bag = nxt
    return bag


# ------------------------------------------------------------------ LM launches

def label_costs_ref(lm, bags, mapping, C, mut=None):
    """cost [hyps, C] fp64 the host's way: BeamSearchLM._step_lm without the weight"""
    from att_speech import fst_utils as P
    hyps = len(bags)
    sizes = [len(d) for d in bags]
    grp = np.repeat(np.arange(hyps), sizes)
    st = np.fromiter((k for d in bags for k in d), np.int64, sum(sizes))
    w = np.fromiter((v for d in bags for v in d.values()), np.float64, sum(sizes))
    nlab = max(C, int(lm.ilabel.max()) + 1)
    cost = np.full(hyps * nlab, INF)
    if mut == 'z_omitted':                        # the arcs alone, no epsilon paths behind them
        owner, arcs = P._gather_arcs(lm.ptr[:-1][st], lm.ptr[1:][st])
        bag, ww = grp[owner] * nlab + lm.ilabel[arcs], w[owner] + lm.weight[arcs]
    else:
        if mut == 'closure_before_label':
            grp, st, w = P._epsilon_closure(lm, grp, st, w, True)
        bag, _, ww = P.expand_all_batched(lm, nlab, grp, st, w, True)
    if bag.size:
        ub, red = P._reduce_by_key(bag, ww, True)
        cost[ub] = red
    return cost.reshape(hyps, nlab)[:, np.asarray(mapping, np.int64)]


def bag_advance_ref(lm, bags, parent, letters, mapping):
    """the survivors' bags: list of dicts in ascending state order"""
    from att_speech import fst_utils as P
    out = []
    for hp, letter in zip(parent, letters):
        d = P.expand(lm, dict(bags[int(hp)]), int(mapping[int(letter)]), True)
        out.append(dict(sorted(d.items())))
    return out


def bags_to_arrays(bags, cap=BAG_CAP, fill_state=POISON, fill_cost=np.nan):
    hyps = len(bags)
    st = np.full((hyps, cap), fill_state, np.int32)
    w = np.full((hyps, cap), fill_cost, np.float64)
    n = np.zeros(hyps, np.int32)
    for h, d in enumerate(bags):
        n[h] = len(d)
        st[h, :len(d)] = list(d.keys())
        w[h, :len(d)] = list(d.values())
    return st, w, n


def arrays_to_bags(st, w, n):
    return [dict(zip(st[h, :n[h]].tolist(), w[h, :n[h]].tolist())) for h in range(len(n))]


# ------------------------------------------------------------------ beam bookkeeping

def fresh_state(B, beam, Lcap):
    return dict(fin_count=np.zeros(B, np.int32), fin_parity=np.zeros(B, np.int32),
                fin_score=np.zeros((2, B, beam), np.float32), fin_len=np.zeros((2, B, beam), np.int32),
                fin_beam=np.zeros((2, B, beam), np.int32), fin_tokens=np.zeros((2, B, beam, Lcap), np.int32),
                best_score=np.full(B, -INF, np.float32), best_len=np.zeros(B, np.int32),
                best_tokens=np.zeros((B, Lcap), np.int32), best_elems=np.zeros((B, 3), np.float32),
                frozen=np.zeros(B, np.int32), nsteps=np.zeros(B, np.int32))


STATE_KEYS = tuple(fresh_state(1, 1, 1))


def lm_beam_step_ref(c, dtype=np.float64, mut=None):
    """One asr_beam_lm_step_f32 launch.  c: dict logits [hyps, C], att [hyps, T], lens [B], lm_cost
    [hyps, C] fp64 or None, lm_weight, scores_in, est_in [hyps, Lcap], cov_in [hyps, T] or None,
    min_eos [hyps] or None, step, B, beam, len_div, min_attention_pos, coverage_tau,
    coverage_weight, state (fresh_state layout; not modified).
    -> (out, margins).  out: the state fields after the launch, scores_out, est [hyps, step+1],
    cov_out, min_eos, new_input, parent (rows of frozen utterances: None-like, see `live`), live [B],
    added [B], improved [B].  margins: topk_cut, topk_adjacent, eos_vs_class, far, finished_order,
    best_vs_candidate, coverage_tau, eos_floor."""
    logits = np.asarray(c['logits'], dtype)
    hyps, C = logits.shape
    B, beam, step, Cm = c['B'], c['beam'], c['step'], C - 1
    T = c['att'].shape[1]
    st = {k: np.array(c['state'][k], copy=True) for k in STATE_KEYS}
    for k in ('fin_score', 'best_score', 'best_elems'):
        st[k] = st[k].astype(dtype)
    m = dict(topk_cut=INF, topk_adjacent=INF, eos_vs_class=INF, far=INF, finished_order=INF,
             best_vs_candidate=INF, coverage_tau=INF, eos_floor=INF)
    cov_on = c['coverage_weight'] > 0
    att = np.asarray(c['att'], dtype)
    scores_out = np.array(c['scores_out_before'], dtype) if 'scores_out_before' in c else np.full(hyps, np.nan, dtype)
    est = np.full((hyps, step + 1), POISON, np.int32)
    new_input = np.full(hyps, POISON, np.int32)
    parent = np.full(hyps, POISON, np.int32)
    cov_out = None if not cov_on else np.full((hyps, T), np.nan, dtype)
    min_eos = None if c.get('min_eos') is None else np.array(c['min_eos'], dtype)
    live = np.zeros(B, bool)
    added = np.zeros(B, bool)
    improved = np.zeros(B, bool)
    for b in range(B):
        if st['frozen'][b] and mut != 'frozen_still_updating':
            continue
        live[b] = True
        sl = slice(b * beam, (b + 1) * beam)
        ln = int(c['lens'][b])
        x = logits[sl].copy()
        if min_eos is not None:
            fl = min_eos[sl]
            if np.isfinite(fl).all():
                m['eos_floor'] = min(m['eos_floor'], float(np.abs(x[:, Cm] - fl).min()))
            x[:, Cm] = np.where(x[:, Cm] > fl, x[:, Cm], fl)
            floors = x[:, Cm].copy()
        local = torch.log_softmax(torch.from_numpy(x), 1).numpy()
        acoustic = local + np.asarray(c['scores_in'], dtype)[sl, None]
        if c.get('lm_cost') is not None:
            lm = (-c['lm_weight'] * np.minimum(1e20, np.asarray(c['lm_cost'], np.float64)[sl])).astype(np.float32).astype(dtype)
        else:
            lm = np.zeros((beam, C), dtype)
        total = acoustic + lm
        covs = np.zeros(beam, dtype)
        if cov_on:
            cur = np.asarray(c['cov_in'], dtype)[sl] + att[sl]                   # [beam, T]
            d = np.abs(cur[:, :ln] - c['coverage_tau'])
            m['coverage_tau'] = min(m['coverage_tau'], float(d.min()) if d.size else INF)
            covs = np.asarray(c['coverage_weight'], dtype) * (cur[:, :ln] > c['coverage_tau']).sum(1).astype(dtype)
            total = total + covs[:, None]
        # ---- finished hypotheses
        if step > 0:
            par = int(st['fin_parity'][b])
            n_old = int(st['fin_count'][b])
            entries = [(st['fin_score'][par, b, i], st['fin_tokens'][par, b, i, :st['fin_len'][par, b, i]].copy(),
                        int(st['fin_beam'][par, b, i])) for i in range(n_old)]
            tlen = T if mut == 'padded_length_in_min_pos' else ln
            min_pos = np.float32(c['min_attention_pos'] * tlen)
            for k in range(beam):
                row = total[k]
                if not np.isfinite(row[:Cm].max()) or abs(row[:Cm].max()) >= 1e18 and abs(row[Cm]) >= 1e18:
                    continue
                peak = int(np.argmax(att[b * beam + k, :ln])) if ln else 0
                eos_best = row[Cm] > row[:Cm].max()
                far = np.float32(peak) > min_pos
                nrm = row[Cm] / np.asarray(c['len_div'], dtype)
                if far:
                    m['eos_vs_class'] = min(m['eos_vs_class'], abs(row[Cm] - row[:Cm].max()))
                if eos_best:
                    m['far'] = min(m['far'], abs(float(peak) - float(c['min_attention_pos'] * tlen)))
                if eos_best and far and nrm > -1e10:
                    entries.append((nrm, np.asarray(c['est_in'])[b * beam + k, :step].copy(), k))
                    added[b] = True
            if added[b]:
                sc = np.array([e[0] for e in entries], np.float64)
                if mut == 'newest_first_on_ties':
                    order = len(sc) - 1 - np.argsort(-sc[::-1], kind='stable')
                else:
                    order = np.argsort(-sc, kind='stable')
                ss = sc[order]
                if len(ss) > 1:
                    # (old entries are sorted among themselves; only orders involving a new one are live)
                    new_pos = [i for i, o in enumerate(order) if o >= n_old]
                    for i in new_pos:
                        for j in (i - 1, i + 1):
                            if 0 <= j < len(ss) and (i < beam or j < beam):
                                m['finished_order'] = min(m['finished_order'], abs(ss[i] - ss[j]))
                entries = [entries[i] for i in order[:beam]]
                npar = par ^ 1
                for r, (s_, tok, bi) in enumerate(entries):
                    st['fin_score'][npar, b, r] = s_
                    st['fin_len'][npar, b, r] = len(tok)
                    st['fin_beam'][npar, b, r] = bi
                    st['fin_tokens'][npar, b, r, :len(tok)] = tok
                st['fin_parity'][b] = npar
                st['fin_count'][b] = len(entries)
                top = entries[0]
                if np.isfinite(st['best_score'][b]) and order[0] >= n_old:   # (an old entry 0 is where best came from)
                    m['best_vs_candidate'] = min(m['best_vs_candidate'], abs(top[0] - st['best_score'][b]))
                if top[0] > st['best_score'][b]:
                    improved[b] = True
                    st['best_score'][b] = top[0]
                    st['best_len'][b] = len(top[1])
                    st['best_tokens'][b, :len(top[1])] = top[1]
                    bi = top[2]
                    # quirk: THIS step's elements at the stored beam index, also for an entry that
                    # joined the list in an earlier step (the mutant has no elements for those)
                    if not (mut == 'elements_of_finishing_step' and order[0] < n_old):
                        st['best_elems'][b] = (acoustic[bi, Cm], lm[bi, Cm], covs[bi])
        # ---- top-k on the fused score; acoustic scores of the chosen
        ncand = (beam if step > 0 else 1) * Cm
        cand = total[:, :Cm].reshape(-1)[:ncand]
        ac = acoustic[:, :Cm].reshape(-1)[:ncand]
        order = np.argsort(-cand, kind='stable')
        k = min(beam, ncand)
        sel, val = order[:k], cand[order[:k]]
        # (extensions the LM has no arc for sit at -lm_weight * 1e20, where fp32 and fp64 both tie exactly)
        real = lambda v: np.isfinite(v) & (np.abs(v) < 1e18)  # noqa: E731
        if ncand > k and real(val[-1]) and real(cand[order[k]]):
            m['topk_cut'] = min(m['topk_cut'], val[-1] - cand[order[k]])
        lv = val[real(val)]
        if lv.size > 1:
            m['topk_adjacent'] = min(m['topk_adjacent'], float(-np.diff(lv).max()))
        if k < beam:
            sel = np.concatenate([sel, np.full(beam - k, sel[-1])])
        new_sc = ac[sel].copy()
        if beam >= ncand:
            pad_from = ncand if beam > ncand else 0           # the host's `[-0:]` slice: every slot
            new_sc[pad_from:] = -INF
        kb, letter = sel // Cm, sel % Cm
        scores_out[sl] = new_sc
        parent[sl] = b * beam + kb
        new_input[sl] = letter
        est[sl] = np.concatenate([np.asarray(c['est_in'])[b * beam + kb, :step], letter[:, None]], 1)
        if cov_on:
            cov_out[sl] = cur if mut == 'coverage_not_reindexed' else cur[kb]
        if min_eos is not None:
            min_eos[sl] = floors[kb]
        st['nsteps'][b] = step + 1
        if st['fin_count'][b] >= beam:
            st['frozen'][b] = 1
    out = dict(st, scores_out=scores_out, est=est, new_input=new_input, parent=parent, cov_out=cov_out,
               min_eos=min_eos, live=live, added=added, improved=improved)
    return out, m


def min_margin(m):
    return min(m.values())


# ------------------------------------------------------------------ cases

LN = dr.LENGTH_NORMALIZATION
PARAMS = dict(lm_weight=0.5, min_attention_pos=0.3, coverage_tau=0.1, coverage_weight=0.2)
T_FRAMES = 13
LENS = [13, 9, 5]
SINGLE_LCAP = 12
# (B, beam, C, step, lm) -> seed with every margin > MARGIN_FLOOR (0 where not listed)
SINGLE_SHAPES = ((1, 1, 6, 'toy'), (3, 3, 6, 'toy'), (2, 8, 6, 'toy'), (2, 4, 50, 'bg'))
SINGLE_STEPS = (0, 1, 7)
SINGLE_SEEDS = {(1, 1, 6, 1, 'toy'): 5, (1, 1, 6, 7, 'toy'): 7, (3, 3, 6, 1, 'toy'): 8, (3, 3, 6, 7, 'toy'): 2,
                (2, 8, 6, 1, 'toy'): 3, (2, 8, 6, 7, 'toy'): 4, (2, 4, 50, 1, 'bg'): 13, (2, 4, 50, 7, 'bg'): 3}
SINGLE_CASES = [s[:3] + (t, s[3]) for s in SINGLE_SHAPES for t in SINGLE_STEPS]


def case_lm(name, C):
    if name == 'toy':
        return toy_lm(), (TOY_MAPPING + [1] * C)[:C - 1] + [1]
    lm = shipped_lm(name)
    return lm, wsj_mapping(lm, C)


def peaked_att(gen, hyps, T, lens, beam):
    """alignments that sum to one over the own frames, zero behind them, with one clear peak"""
    att = torch.rand(hyps, T, generator=gen) * 0.04
    for h in range(hyps):
        ln = lens[h // beam]
        att[h, ln:] = 0
        att[h, int(torch.randint(ln, (1,), generator=gen))] += 0.6
        att[h] /= att[h].sum()
    return att.numpy()


def single_case(B, beam, C, step, lm_name, seed=None, keep_eos=None):
    """one launch from arbitrary state; bags of 1 to 3 entries from walks through the LM"""
    if seed is None:
        seed = SINGLE_SEEDS.get((B, beam, C, step, lm_name), 0)
    gen = torch.Generator().manual_seed(7000 * seed + 10 * step + B)
    lm, mapping = case_lm(lm_name, C)
    hyps, T, Lcap = B * beam, T_FRAMES, SINGLE_LCAP
    lens = LENS[:B]
    logits = 8 * torch.randn(hyps, C, generator=gen)
    logits[:, -1] += 6
    scores = 5 * torch.randn(hyps, generator=gen)
    if step > 0:
        scores[torch.rand(hyps, generator=gen) < 0.15] = -INF
    est_in = torch.randint(0, C - 1, (hyps, Lcap), generator=gen).to(torch.int32).numpy()
    bags = []
    for h in range(hyps):
        n = int(torch.randint(0, 4, (1,), generator=gen))
        labs = [mapping[int(v)] for v in torch.randint(2, C - 1, (n,), generator=gen)]
        bags.append(dict(sorted(walk_bag(lm, labs).items())))
    state = fresh_state(B, beam, Lcap)
    pick = lambda vals: torch.tensor(vals)[torch.randint(len(vals), (B,), generator=gen)]  # noqa: E731
    state['fin_count'] = pick([0, max(beam - 2, 0), beam - 1]).to(torch.int32).numpy() if step > 0 else state['fin_count']
    state['fin_parity'] = torch.randint(0, 2, (B,), generator=gen).to(torch.int32).numpy()
    for k in ('fin_len', 'fin_beam', 'fin_tokens', 'best_tokens'):
        state[k][:] = POISON
    state['fin_score'][:] = np.nan
    for b in range(B):
        p, n = state['fin_parity'][b], state['fin_count'][b]
        state['fin_score'][p, b, :n] = np.sort(torch.randn(n, generator=gen).numpy() * 3 - 4)[::-1]
        state['fin_len'][p, b, :n] = torch.randint(1, Lcap, (n,), generator=gen).numpy()
        state['fin_beam'][p, b, :n] = torch.randint(0, beam, (n,), generator=gen).numpy()
        state['fin_tokens'][p, b, :n] = torch.randint(0, C - 1, (n, Lcap), generator=gen).numpy()
    state['best_score'] = pick([-INF, -1e4, 1e4]).to(torch.float32).numpy()
    if B > 1 and step > 0:
        state['frozen'][B - 1] = 1                       # one utterance is frozen already
    state['nsteps'][:] = step
    if keep_eos is None:
        keep_eos = (seed + step) % 2 == 1
    c = dict(logits=logits.numpy(), att=peaked_att(gen, hyps, T, lens, beam), lens=np.array(lens, np.int32),
             scores_in=scores.numpy(), est_in=est_in,
             cov_in=(torch.rand(hyps, T, generator=gen) * 0.2).numpy() * (step > 0),
             min_eos=(3 * torch.randn(hyps, generator=gen)).numpy() if keep_eos else None,
             step=step, B=B, beam=beam, C=C, T=T, Lcap=Lcap, len_div=dr.len_div(step), state=state,
             bags=bags, lm=lm, mapping=mapping, **PARAMS)
    c['lm_cost'] = label_costs_ref(lm, bags, mapping, C)
    return c


def tie_cases():
    """dyadic logits, zero LM weight, no coverage: equal logits give bit-equal scores"""
    def case(rows, B, beam, step=1, **kw):
        logits = np.array(rows, np.float32)
        hyps, C = logits.shape
        T, Lcap = 4, SINGLE_LCAP
        att = np.zeros((hyps, T), np.float32)
        att[:, 3] = 1.0
        est = (np.arange(hyps * Lcap, dtype=np.int32).reshape(hyps, -1) * 3) % (C - 1)
        est[:, 0] = np.arange(hyps) % (C - 1)
        st = fresh_state(B, beam, Lcap)
        st['best_tokens'][:] = POISON
        st.update(kw)
        return dict(logits=logits, att=att, lens=np.full(B, T, np.int32), scores_in=np.zeros(hyps, np.float32),
                    est_in=est, cov_in=None, min_eos=None, lm_cost=None, step=step, B=B, beam=beam, C=C, T=T,
                    Lcap=Lcap, len_div=1.0, state=st, lm_weight=0.0, min_attention_pos=0.3,
                    coverage_tau=0.1, coverage_weight=0.0)
    row = [1.0, 0.5, -2.0, 0.25, -1.0]
    eos = [1.0, 0.5, -2.0, 0.25, 4.0]
    return {
        'lowest_flat_index_wins': case([row, row, row], 1, 3),
        'all_equal_everywhere': case([[0.0] * 5] * 6, 2, 3),
        'first_step_equal': case([[0.0] * 4, [5.0] * 4], 1, 2, step=0),
        # two launches, see tie_second_launch: beam 0 finishes, then beam 1 with the same score
        'finish_beam_0': case([eos, row, row], 1, 3),
    }


def tie_second_launch(first, state_after):
    """The launch after tie_cases()['finish_beam_0'], from the state that one left: the same rows
    with beam 1 finishing, bit for bit at the score beam 0 had (same arithmetic on the same numbers
    in another row).  Expected: the older entry stays first (fin_beam [0, 1]) and the equal score
    does not replace the best hypothesis (best_tokens stay beam 0's)."""
    logits = first['logits'][[1, 0, 2]]
    return dict(first, logits=np.ascontiguousarray(logits), state=state_after)


def tolerance(c, want):
    """4x the distance of the same launch in fp32 on the CPU from fp64, plus 4 fp32 ulps of the
    largest operand -> (tolerance, the fp32 distance)"""
    f32, _ = lm_beam_step_ref(c, dtype=np.float32)
    d = 0.0
    for k in ('scores_out', 'best_score', 'fin_score', 'best_elems'):
        a, b = np.asarray(f32[k], np.float64), np.asarray(want[k], np.float64)
        ok = np.isfinite(a) & np.isfinite(b) & (np.abs(b) < 1e3)
        d = max(d, float(np.abs(a[ok] - b[ok]).max(initial=0.0)))
    s = np.asarray(c['scores_in'], np.float64)
    mag = max(float(np.abs(c['logits']).max()), float(np.abs(s[np.isfinite(s)]).max(initial=0.0)))
    if c.get('lm_cost') is not None:
        lc = np.asarray(c['lm_cost'])
        mag = max(mag, abs(c['lm_weight']) * float(np.abs(lc[np.isfinite(lc)]).max(initial=0.0)))
    return 4 * d + 4 * dr.EPS32 * mag, d


def prefilled(c):
    """the buffers of a launch as the kernel finds them: outputs pre-filled with POISON / NaN"""
    hyps, T = c['B'] * c['beam'], c['T']
    return dict(scores_out=np.full(hyps, np.nan, np.float32),
                est_out=np.full((hyps, c['Lcap']), POISON, np.int32),
                cov_out=np.full((hyps, T), np.nan, np.float32),
                new_input=np.full(hyps, POISON, np.int32), parent=np.full(hyps, POISON, np.int32))


def kernel_view(c, out, before=None):
    """what the launch leaves in the kernel's buffers given the outputs `out` of a referee"""
    pre = prefilled(c) if before is None else {k: v.copy() for k, v in before.items()}
    step, beam = c['step'], c['beam']
    got = {k: np.array(out[k], copy=True) for k in STATE_KEYS}
    rows = np.repeat(out['live'], beam)
    pre['scores_out'][rows] = out['scores_out'][rows]
    pre['est_out'][rows, :step + 1] = out['est'][rows]
    pre['new_input'][rows] = out['new_input'][rows]
    pre['parent'][rows] = out['parent'][rows]
    if out['cov_out'] is not None:
        pre['cov_out'][rows] = out['cov_out'][rows]
    got.update(pre, min_eos=None if out['min_eos'] is None else np.array(out['min_eos'], copy=True))
    return got


def judge(c, got, want, tol, before=None):
    """got: the buffers after the launch (STATE_KEYS, scores_out, est_out, cov_out, min_eos,
    new_input, parent); before: what est_out / scores_out / cov_out / new_input / parent held
    (prefilled() by default).  Integer outputs bit-equal, scores within tol, -inf exactly where
    due, everything a launch must leave alone still what it was.  -> list of complaints"""
    bad = []
    before = prefilled(c) if before is None else before
    step, beam, B = c['step'], c['beam'], c['B']

    def same(name, a, b):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape or not np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'):
            bad.append('%s differs (got %s want %s)' % (name, a.ravel()[:12], b.ravel()[:12]))

    def close(name, a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        fin = np.isfinite(b)
        if a.shape != b.shape or not np.array_equal(a[~fin], b[~fin], equal_nan=True):
            bad.append('%s: non-finite entries differ' % name)
            return
        err = np.abs(a[fin] - b[fin])
        if err.size and not (err <= tol).all():
            bad.append('%s: max error %.3g > tol %.3g' % (name, float(np.nanmax(err)), tol))

    for k in ('fin_count', 'fin_parity', 'fin_len', 'fin_beam', 'fin_tokens', 'best_len', 'best_tokens',
              'frozen', 'nsteps'):
        same(k, got[k], want[k])
    for k in ('fin_score', 'best_score', 'best_elems'):
        touched = np.zeros(np.asarray(want[k]).shape, bool)
        if k == 'fin_score':
            for b in range(B):
                if want['added'][b]:
                    touched[want['fin_parity'][b], b, :want['fin_count'][b]] = True
        else:
            touched[want['improved']] = True
            if k == 'best_elems' and not c['coverage_weight'] > 0:
                touched[:, 2] &= False
        same(k + ' (kept)', np.asarray(got[k], np.float32)[~touched], np.asarray(c['state'][k], np.float32)[~touched])
        close(k, np.asarray(got[k])[touched], np.asarray(want[k])[touched])
    rows = np.repeat(want['live'], beam)
    same('est_out live', got['est_out'][rows, :step + 1], want['est'][rows])
    same('est_out beyond step', got['est_out'][rows, step + 1:], before['est_out'][rows, step + 1:])
    for k in ('est_out', 'scores_out', 'new_input', 'parent') + (('cov_out',) if c['coverage_weight'] > 0 else ()):
        same(k + ' of frozen utterances', got[k][~rows], before[k][~rows])
    same('new_input', got['new_input'][rows], want['new_input'][rows])
    same('parent', got['parent'][rows], want['parent'][rows])
    close('scores_out', got['scores_out'][rows], want['scores_out'][rows])
    if c['coverage_weight'] > 0:
        close('cov_out', got['cov_out'][rows], want['cov_out'][rows])
    else:
        same('cov_out untouched', got['cov_out'], before['cov_out'])
    if want['min_eos'] is not None:
        same('min_eos of frozen utterances', np.asarray(got['min_eos'], np.float32)[~rows],
             np.asarray(c['min_eos'], np.float32)[~rows])
        close('min_eos', got['min_eos'][rows], want['min_eos'][rows])
    return bad


# ------------------------------------------------------------------ trajectories

TRAJ = dict(B=3, beam=3, C=7, steps=12, seed=160, lens=[13, 9, 5])


def traj_inputs(B, beam, C, steps, seed, lens, eos_bias=(0.0, 2.0, 9.0)):
    """scripted logits / alignments; the EOS bias grows with the utterance index, so the last
    utterance fills its finished list early and freezes while the others run"""
    gen = torch.Generator().manual_seed(seed)
    logits = 4 * torch.randn(steps, B * beam, C, generator=gen)
    for b in range(B):
        logits[:, b * beam:(b + 1) * beam, -1] += eos_bias[b % len(eos_bias)]
    att = np.stack([peaked_att(gen, B * beam, T_FRAMES, lens, beam) for _ in range(steps)])
    # the peak moves to the end of each utterance, so min_attention_pos lets hypotheses finish
    for s in range(steps):
        for h in range(B * beam):
            ln = lens[h // beam]
            a = att[s, h, :ln]
            k = int(np.argmax(a))
            tgt = min(ln - 1, (s * ln) // 4 + (h % 2))
            a[k], a[tgt] = a[tgt], a[k]
    return logits.numpy(), att


class RefSearch(object):
    """the three referees chained: a free-running B-utterance search in `dtype`"""

    def __init__(self, lm, mapping, B, beam, C, T, lens, Lcap, keep_eos=False, dtype=np.float64, mut=None,
                 **params):
        self.lm, self.mapping, self.B, self.beam, self.C, self.T = lm, mapping, B, beam, C, T
        self.lens, self.Lcap, self.dtype, self.mut = np.asarray(lens, np.int32), Lcap, dtype, mut
        self.p = dict(PARAMS, **params)
        hyps = B * beam
        self.state = fresh_state(B, beam, Lcap)
        self.scores = np.zeros(hyps, dtype)
        self.est = np.zeros((hyps, Lcap), np.int32)
        self.cov = np.zeros((hyps, T), dtype)
        self.min_eos = np.full(hyps, -INF, dtype) if keep_eos else None
        self.bags = [{lm.start(): 0.0} for _ in range(hyps)]
        self.step_no = 0
        self.margins = []

    def case(self, logits, att):
        s = self.step_no
        c = dict(logits=logits, att=att, lens=self.lens, scores_in=self.scores, est_in=self.est,
                 cov_in=self.cov, min_eos=self.min_eos, step=s, B=self.B, beam=self.beam, C=self.C,
                 T=self.T, Lcap=self.Lcap, len_div=float(s ** LN) if s > 0 else 1.0, state=self.state,
                 bags=self.bags, lm=self.lm, mapping=self.mapping, **self.p)
        mut = self.mut if self.mut in ('z_omitted', 'closure_before_label') else None
        c['lm_cost'] = label_costs_ref(self.lm, self.bags, self.mapping, self.C, mut) if self.p['lm_weight'] != 0 else None
        return c

    def step(self, logits, att):
        c = self.case(logits, att)
        out, m = lm_beam_step_ref(c, self.dtype, self.mut)
        self.margins.append(m)
        rows = np.repeat(out['live'], self.beam)
        s = self.step_no
        self.scores = np.where(rows, out['scores_out'], self.scores)
        self.est = self.est.copy()
        self.est[rows, :s + 1] = out['est'][rows]
        if out['cov_out'] is not None:
            self.cov = np.where(rows[:, None], out['cov_out'], self.cov)
        if out['min_eos'] is not None:
            self.min_eos = out['min_eos']
        if self.p['lm_weight'] != 0:
            new = bag_advance_ref(self.lm, self.bags, np.where(rows, out['parent'], 0),
                                  np.where(rows, out['new_input'], 0), self.mapping)
            self.bags = [new[h] if rows[h] else self.bags[h] for h in range(len(rows))]
        self.state = {k: out[k] for k in STATE_KEYS}
        self.step_no = s + 1
        return out, c
