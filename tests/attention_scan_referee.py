"""fp64 referees of the two attention training scans, one launch at a time:
asr_tcn_attention_scan_fwd_f32 / _bwd_f32 (csrc/tcn_train.hip) and asr_att_gru_scan_fwd_f32 /
_bwd_f32 (csrc/att_gru.hip).  Written from include/asr_amd.h, modules/tcn.py and
modules/decoders/attention_decoder.py; plain torch on the CPU, no native calls.  The decode form of
the GRU forward (L = 1, beam > 1) is refereed in tests/decode_referee.py; one position of the scan
here IS decode_referee.att_gru_step_ref.

Every reference takes `dtype` (fp64; the same arithmetic in fp32 is the yardstick) and `mut`, one
wrong term (TCN_MUTANTS, GRU_MUTANTS).  tests/test_attention_scan_referee.py proves on the CPU that
the references are what autograd makes of the modules' per-position loops, that the fp32 yardstick
passes every judge and that each mutant is rejected at the cases named for it (MUTANT_CASES).

Forward launches are judged TEACHER-FORCED: position l of the reference starts from the launch's
own a_{l-1} (TCN) or h_{l-1} (GRU), so every position is judged on its own and no drift enters.
Backward launches take the saved forward tensors as given, exactly as the kernels do.

Tolerances (nothing is fitted to what a kernel returns).  Every output has an OWNER ROW: (l, b) for
att, d_filt, d_glob, states, contexts, gates, rec, d_gates, d_contexts, d_rec; b for d_a0, d_wb,
d_w_score, d_h0 and for the utterance's slab [:, b, :] of d_eproj.  The bound of a row is

    4 max_row |fp32 yardstick - fp64|  +  4 * 2^-23 max_row |fp64|  +  max_row (tanh term)

(decode_referee.att_tolerance's rule, row by row: the factor 4 is the project's margin for a
different summation order).  The yardstick evaluates the attention tanh in the kernels' form
1 - 2 / (exp(2x) + 1); the device exp differs from the host's, which the tanh term covers:
TANH_ABS = 2^-21 bounds |tanh x - device form| (decode_referee).

  forward  a score moves by at most d = temperature sum|w| TANH_ABS (GRU: temperature 1), an
           alignment by 2 d of itself.  GRU records, with e_c = 2 d sum_t a_t |encoded_t| (a vector
           over E) and e_gi = |w_ic| e_c:  contexts e_c;  r and z  e_gi / 4 (sigmoid' <= 1/4);
           n  e_gi_n + |gh_n| e_r;  states |1 - z| e_n + |n - h_prev| e_z;  rec and gh_n none.
  backward dh = ds w (1 - th^2) moves by 2 |ds w th| TANH_ABS and ds th by |ds| TANH_ABS.  These
           are injected where they arise and carried to every output BY THE SAME SUMS THAT FORM
           IT, every coefficient replaced by its magnitude and every difference by a sum.
           TCN (`_tcn_bound`): through d_eproj, d_glob, d_filt, d w, the location filter into the
           carry, the softmax backward a (g - <a, g>) of the position before, and so on down to
           d_a0.  GRU (`_gru_bound`): the same walk through |w_rec|, |w_hh|, |w_ic| and |encoded|
           grows by about sqrt(width) per product and reached 4e5 at (50, 4, 5, 64, 320, 256), a
           bound that judges nothing.  But the GRU's carry is a function of OUTPUTS, carry_{l-1} =
           dh_l z_l + (dr, dz, dn r)_l w_hh + d_rec_l w_rec, so its reverse scan is teacher-forced
           like the forward: the reference forms the carry from the launch's own d_gates[l] and
           d_rec[l], each position is judged on its own, and the tanh term stays where it arises
           (d_eproj, d_rec, d_w_score); d_gates, d_contexts and d_h0 have none.

Exact conditions (held with equality, `judge`): rows of att sum to 1 within 1e-5; frames at or past
len are exactly 0 (exp(-1e5 + O(100)) underflows in every format); TCN backward with d_att non-zero
at one position l0: d_filt[l], d_glob[l] = 0 for l > l0; with d_att non-zero on padded frames only:
every output 0; TCN forward with w_score = 0: float32(1) / float32(len) bit for bit on the
utterance's own frames; GRU backward: d_eproj rows at or past len keep the caller's pre-fill bit for
bit, and no other output keeps a POISON.

Case inputs are held as the ABI holds them (time-major eproj, [L, B, ...] label-major rows)."""
import zlib

import torch

import decode_referee as dr
from decode_referee import EPS32, F64, KF, MASKED, TANH_ABS, _tanh

F32 = torch.float32
POISON = -776.0

# ------------------------------------------------------------------ launch plans of tcn_train.hip

NT, TMAX, AMAX = 512, 4096, 256
PART_CAP, TILE_CAP, TT_MAX = 4096, 4096, 64
FS = KF + 1
LDS_CAP = 160 * 1024
GRU_TMAX, GRU_AMAX, GRU_HMAX, GRU_EMAX, GRU_CG, GRU_NW = 4096, 320, 320, 512, 8, 16


def _cdiv(a, b):
    return -(-a // b)


def fwd_split(T, A):
    """-> (G, AC): the forward's G chunks of AC units (G T <= PART_CAP or G = 1)"""
    bg, best = 1, -1
    for g in range(1, A + 1):
        if g > 1 and g * T > PART_CAP:
            break
        ac = _cdiv(A, g)
        if g > 1 and _cdiv(A, g - 1) == ac:
            continue
        cost = _cdiv(g * T, NT) * (ac * (KF + 8) + 2 * KF)
        if best < 0 or cost < best:
            best, bg = cost, g
    return bg, _cdiv(A, bg)


def bwd_tiles(A):
    """-> (TT, G2, AC2): frames per backward tile, unit chunks per tile, units per chunk"""
    tt = min(TT_MAX, max(1, TILE_CAP // A))
    g2 = min(A, max(1, NT // tt))
    ac2 = _cdiv(A, g2)
    return tt, _cdiv(A, ac2), ac2


def plan(T, A):
    G, AC = fwd_split(T, A)
    TT, G2, AC2 = bwd_tiles(A)
    return dict(G=G, AC=AC, TT=TT, G2=G2, AC2=AC2)


def fwd_lds(T, A):
    G = fwd_split(T, A)[0]
    TP = (KF - 1 + T + 3) & ~3
    return 4 * (TP + ((max(G * T, T) + 3) & ~3) + A * FS + 2 * A + 32)


def bwd_lds(T, A):
    TT = bwd_tiles(A)[0]
    TP = (KF - 1 + T + TT + 3) & ~3
    return 4 * (TP + 3 * ((T + 3) & ~3) + A * FS + 2 * A + 2 * TT * (A + 1) + TT * FS + 32)


# ------------------------------------------------------------------ TCN scan

TCN_MUTANTS = ('window_shift_by_one', 'taps_reversed', 'mask_before_temperature', 'len_off_by_one',
               'last_unit_chunk_dropped', 'tile_tail_frames_dropped', 'carry_misses_tile_seam',
               'carry_not_cleared', 'd_eproj_last_position_only', 'softmax_bwd_without_dot',
               'a0_at_every_position', 'd_wb_first_utterance_only', 'temperature_missing_in_bwd')


def _tcn_hidden(eproj, filt_l, glob_l, prev, mut):
    """prev [B, T] -> (hidden [B, T, A], windows [B, T, Kf], filters [B, A, Kf])"""
    B, T = prev.shape
    A = glob_l.shape[1]
    if mut == 'window_shift_by_one':
        ap = torch.nn.functional.pad(prev, (KF, 0))[:, :KF - 1 + T]
    else:
        ap = torch.nn.functional.pad(prev, (KF - 1, 0))
    win = ap.unfold(1, KF, 1)
    f = filt_l.view(B, A, KF)
    if mut == 'taps_reversed':
        f = f.flip(2)
    hid = eproj.permute(1, 0, 2) + glob_l[:, None, :] + torch.einsum('btj,baj->bta', win, f)
    return hid, win, f


def tcn_scan_fwd_ref(eproj, filt, glob, a0, w_score, b_score, temperature, lens, forced=None,
                     dtype=F64, mut=None, tanh_form=None):
    """a_l = softmax_t(temperature (w . tanh(eproj_t + glob_l + sum_j a_{l-1}[t-31+j] filt_l[., j])
    + b) + pad_t), a_{-1} = a0, pad_t = -1e5 for t >= lens[b].  eproj [T, B, A], filt [L, B, A*32],
    glob [L, B, A], a0 [T, B] -> att [L, B, T].  forced [L, B, T]: position l takes forced[l-1]."""
    c = lambda x: torch.as_tensor(x).to(dtype)  # noqa: E731
    eproj, filt, glob, w = c(eproj), c(filt), c(glob), c(w_score).reshape(-1)
    T, B, A = eproj.shape
    L = glob.shape[0]
    b = float(torch.as_tensor(b_score).reshape(-1)[0])
    ln = torch.as_tensor(lens).long()[:, None]
    t = torch.arange(T)[None, :]
    mask = ((t > ln) if mut == 'len_off_by_one' else (t >= ln)).to(dtype) * MASKED
    first = c(a0).t()
    if mut == 'last_unit_chunk_dropped':
        G, AC = fwd_split(T, A)
        w = w.clone()
        if G > 1:
            w[(G - 1) * AC:] = 0
    out = []
    for l in range(L):
        prev = first if l == 0 or mut == 'a0_at_every_position' else \
            (c(forced[l - 1]) if forced is not None else out[l - 1])
        hid, _, _ = _tcn_hidden(eproj, filt[l], glob[l], prev, mut)
        e = _tanh(hid, tanh_form) @ w + b
        e = (e + mask) * temperature if mut == 'mask_before_temperature' else e * temperature + mask
        out.append(torch.softmax(e, 1))
    return torch.stack(out)


def _fold(u):
    """u [B, T, Kf] -> [B, T]: frame s collects u[t, j] with t - 31 + j = s"""
    B, T, _ = u.shape
    cp = u.new_zeros(B, T + KF - 1)
    for j in range(KF):
        cp[:, j:j + T] += u[:, :, j]
    return cp[:, KF - 1:]


def tcn_scan_bwd_ref(eproj, filt, glob, a0, w_score, temperature, lens, att, d_att, dtype=F64,
                     mut=None, tanh_form=None, aux=None):
    """The reverse scan from the GIVEN alignments (h is recomputed from them, as the kernel does):
    g_l = d_att_l + carry_l, ds = temperature a_l (g - <a_l, g>), dh = ds w (1 - tanh^2 h),
    d_eproj = sum_l dh, d_glob_l = sum_t dh, d_filt_l[a, j] = sum_t dh[t, a] a_{l-1}[t-31+j],
    carry_{l-1}[s] = sum_{t-31+j=s} sum_a dh[t, a] filt_l[a, j], d_a0 = carry_{-1},
    d_wb[b] = (sum_l sum_t ds tanh h, sum_l sum_t ds).
    -> d_eproj [T, B, A], d_filt [L, B, A*32], d_glob [L, B, A], d_a0 [T, B], d_wb [B, A+1]"""
    c = lambda x: torch.as_tensor(x).to(dtype)  # noqa: E731
    eproj, filt, glob, w = c(eproj), c(filt), c(glob), c(w_score).reshape(-1)
    att, d_att, first = c(att), c(d_att), c(a0).t()
    T, B, A = eproj.shape
    L = glob.shape[0]
    TT, G2, AC2 = bwd_tiles(A)
    temp = 1.0 if mut == 'temperature_missing_in_bwd' else temperature
    tt = torch.arange(T)
    d_eproj = eproj.new_zeros(B, T, A)
    d_filt, d_glob = torch.zeros_like(filt), torch.zeros_like(glob)
    d_w, d_b = eproj.new_zeros(B, A), eproj.new_zeros(B)
    carry = eproj.new_zeros(B, T)
    for l in range(L - 1, -1, -1):
        a = att[l]
        prev = first if l == 0 or mut == 'a0_at_every_position' else att[l - 1]
        g = d_att[l] + carry
        dot = 0.0 if mut == 'softmax_bwd_without_dot' else (a * g).sum(1, keepdim=True)
        ds = temp * (a * (g - dot))
        hid, win, f = _tcn_hidden(eproj, filt[l], glob[l], prev, mut)
        th = _tanh(hid, tanh_form)
        dh = ds[:, :, None] * w * (1 - th * th)
        if mut == 'last_unit_chunk_dropped':
            dh[:, :, (G2 - 1) * AC2:] = 0
        if mut == 'tile_tail_frames_dropped' and T % TT:
            dh[:, T // TT * TT:, :] = 0
        if mut == 'd_eproj_last_position_only':
            d_eproj = dh if l == L - 1 else d_eproj
        else:
            d_eproj = d_eproj + dh
        d_glob[l] = dh.sum(1)
        d_filt[l] = torch.einsum('bta,btj->baj', dh, win).reshape(B, A * KF)
        d_w += (ds[:, :, None] * th).sum(1)
        d_b += ds.sum(1)
        u = torch.einsum('bta,baj->btj', dh, f)
        if mut == 'carry_misses_tile_seam':
            s = tt[:, None] - (KF - 1) + torch.arange(KF)[None, :]
            u = u * (s // TT == tt[:, None] // TT).to(dtype)
        new = _fold(u)
        carry = carry + new if mut == 'carry_not_cleared' else new
        if aux is not None:
            aux[l] = (ds, th, win, f, a)
    d_wb = torch.cat((d_w, d_b[:, None]), 1)
    if mut == 'd_wb_first_utterance_only':
        d_wb[1:] = 0
    return dict(d_eproj=d_eproj.permute(1, 0, 2).contiguous(), d_filt=d_filt, d_glob=d_glob,
                d_a0=carry.t().contiguous(), d_wb=d_wb)


def _tcn_bound(aux, w_score, temperature, L):
    """the tanh term of every output of the reverse scan (module docstring): the same sums on
    magnitudes, 2 |ds w th| TANH_ABS injected at dh and |ds| TANH_ABS at ds th"""
    w = torch.as_tensor(w_score).to(F64).reshape(-1).abs()
    ds0 = aux[L - 1][0]
    B, T = ds0.shape
    A = w.numel()
    b_eproj = ds0.new_zeros(B, T, A)
    b_filt, b_glob = ds0.new_zeros(L, B, A * KF), ds0.new_zeros(L, B, A)
    b_w, b_b = ds0.new_zeros(B, A), ds0.new_zeros(B)
    carry = ds0.new_zeros(B, T)
    for l in range(L - 1, -1, -1):
        ds, th, win, f, a = aux[l]
        dds = abs(temperature) * a * (carry + (a * carry).sum(1, keepdim=True))
        ddh = dds[:, :, None] * w * (1 - th * th) + 2 * (ds[:, :, None] * w * th).abs() * TANH_ABS
        b_eproj += ddh
        b_glob[l] = ddh.sum(1)
        b_filt[l] = torch.einsum('bta,btj->baj', ddh, win.abs()).reshape(B, A * KF)
        b_w += (dds[:, :, None] * th.abs()).sum(1) + ds.abs().sum(1, keepdim=True) * TANH_ABS
        b_b += dds.sum(1)
        carry = _fold(torch.einsum('bta,baj->btj', ddh, f.abs()))
    return dict(d_eproj=b_eproj.permute(1, 0, 2), d_filt=b_filt, d_glob=b_glob, d_a0=carry.t(),
                d_wb=torch.cat((b_w, b_b[:, None]), 1))


# ------------------------------------------------------------------ attention-GRU scan

GRU_MUTANTS = ('carry_without_z_path', 'dgh_n_without_r', 'h_prev_from_same_row', 'w_rec_carry_dropped',
               'd_att_ignored', 'd_states_ignored', 'context_groups_miss_tail',
               'd_eproj_overwrites_prefill', 'len_0_is_empty')
GRU_FWD_KEYS = ('att', 'states', 'contexts', 'gates', 'rec')
GRU_BWD_KEYS = ('d_eproj', 'd_gates', 'd_contexts', 'd_rec', 'd_w_score', 'd_h0')
TCN_BWD_KEYS = ('d_eproj', 'd_filt', 'd_glob', 'd_a0', 'd_wb')


def clamp_len(lens, T):
    ln = torch.as_tensor(lens).long()
    return torch.where((ln <= 0) | (ln > T), torch.full_like(ln, T), ln)


def _tail_mask(lens, T, dtype):
    """[B, T]: 0 on the frames past the last whole group of eight of each utterance"""
    ln = clamp_len(lens, T)
    return (torch.arange(T)[None, :] < (ln // GRU_CG * GRU_CG)[:, None]).to(dtype)


def att_gru_scan_fwd_ref(eproj, encoded, lens, gx_emb, w_ic, w_hh, b_hh, w_rec, w_score, b_score, h0,
                         beam=1, forced=None, dtype=F64, mut=None, tanh_form=None):
    """decode_referee.att_gru_step_ref position after position; gx_emb [L, B, 3H]; forced [L, B, H]:
    position l starts from forced[l-1].  -> dict att [L, B, T], states [L, B, H], contexts [L, B, E],
    gates [L, B, 4H] = (r, z, n, gh_n), rec [L, B, A]"""
    L = gx_emb.shape[0]
    T = eproj.shape[0]
    step_mut = mut if mut == 'len_0_is_empty' else None
    rows = []
    h = torch.as_tensor(h0).to(dtype)
    for l in range(L):
        if l > 0:
            h = torch.as_tensor(forced[l - 1]).to(dtype) if forced is not None else rows[l - 1][1]
        att, st, ctx, gates, rec = dr.att_gru_step_ref(
            eproj, encoded, lens, gx_emb[l], w_ic, w_hh, b_hh, w_rec, w_score, b_score, h, beam,
            dtype=dtype, mut=step_mut, tanh_form=tanh_form, records=True)
        if mut == 'context_groups_miss_tail':       # the cell and the state are then what follows
            u = torch.arange(h.shape[0]) // beam
            keep = _tail_mask(lens, T, dtype)[u]
            ctx = torch.einsum('bt,tbe->be', att * keep, torch.as_tensor(encoded).to(dtype)[:, u])
            st, gates = _gru_cell(ctx, gx_emb[l], w_ic, w_hh, b_hh, h, dtype)
        rows.append((att, st, ctx, gates, rec))
    return {k: torch.stack([r[i] for r in rows]) for i, k in enumerate(GRU_FWD_KEYS)}


def _gru_cell(ctx, gx, w_ic, w_hh, b_hh, h, dtype):
    c = lambda x: torch.as_tensor(x).to(dtype)  # noqa: E731
    B, H = h.shape
    gi = (c(gx) + ctx @ c(w_ic).t()).view(B, 3, H)
    gh = (h @ c(w_hh).t() + c(b_hh)).view(B, 3, H)
    r = torch.sigmoid(gi[:, 0] + gh[:, 0])
    z = torch.sigmoid(gi[:, 1] + gh[:, 1])
    n = torch.tanh(gi[:, 2] + r * gh[:, 2])
    return (1 - z) * n + z * h, torch.cat((r, z, n, gh[:, 2]), 1)


def att_gru_scan_bwd_ref(eproj, encoded, lens, w_ic, w_hh, w_rec, w_score, h0, att, states, gates, rec,
                         d_att=None, d_states=None, d_eproj=None, forced=None, dtype=F64, mut=None,
                         tanh_form=None, aux=None):
    """The reverse scan from the saved att / states / gates / rec (beam = 1).  With dh = carry +
    d_states_l:  dn = dh (1-z)(1-n^2), dz = dh (h_{l-1} - n) z (1-z), dr = dn gh_n r (1-r);
    d_gates_l = (dr, dz, dn, dn r);  d c = (dr, dz, dn) w_ic;  g_t = <encoded_t, d c> + d_att_l[t];
    ds = a (g - <a, g>) on the frames before len (a length of 0 or above T means T);
    dpre = ds w_score (1 - tanh^2(eproj_t + rec_l));  d_eproj[t] += dpre;  d_rec_l = sum_t dpre;
    d_w_score[b] += sum_t ds tanh;  carry = dh z + (dr, dz, dn r) w_hh + d_rec_l w_rec;  d_h0 = the
    last carry.  d_att / d_states None = zero; d_eproj: the caller's pre-fill (None = zeros), which
    the gradient is ADDED to.  forced = dict(d_gates, d_rec), the launch's own: the carry handed to
    position l-1 is then formed from forced d_gates[l] and d_rec[l] (and the reference's own dh z), so
    every position is judged on its own.  -> dict of GRU_BWD_KEYS"""
    c = lambda x: torch.as_tensor(x).to(dtype)  # noqa: E731
    eproj, encoded, w_ic, w_hh, w_rec = c(eproj), c(encoded), c(w_ic), c(w_hh), c(w_rec)
    v, h0, att, states, gates, rec = c(w_score).reshape(-1), c(h0), c(att), c(states), c(gates), c(rec)
    T, B, A = eproj.shape
    L, _, H = states.shape
    ln = torch.as_tensor(lens).long()
    empty = (ln == 0) if mut == 'len_0_is_empty' else torch.zeros(B, dtype=torch.bool)
    live = ((torch.arange(T)[None, :] < clamp_len(lens, T)[:, None]) & ~empty[:, None]).to(dtype)
    tail = _tail_mask(lens, T, dtype) if mut == 'context_groups_miss_tail' else 1.0
    if mut == 'd_att_ignored':
        d_att = None
    if mut == 'd_states_ignored':
        d_states = None
    grad = eproj.new_zeros(B, T, A)
    d_gates, d_ctx, d_rec = torch.zeros_like(gates), encoded.new_zeros(L, B, encoded.shape[2]), torch.zeros_like(rec)
    d_v = eproj.new_zeros(B, A)
    carry = eproj.new_zeros(B, H)
    ep = eproj.permute(1, 0, 2)
    for l in range(L - 1, -1, -1):
        r, z, n, hn = gates[l].view(B, 4, H).unbind(1)
        hp = states[l] if mut == 'h_prev_from_same_row' else (states[l - 1] if l > 0 else h0)
        dh = carry + (c(d_states[l]) if d_states is not None else 0.0)
        dn = dh * (1 - z) * (1 - n * n)
        dz = dh * (hp - n) * z * (1 - z)
        dr = dn * hn * r * (1 - r)
        dghn = dn if mut == 'dgh_n_without_r' else dn * r
        d_gates[l] = torch.cat((dr, dz, dn, dghn), 1)
        fg = d_gates[l] if forced is None else c(forced['d_gates'][l])
        carry = (0.0 if mut == 'carry_without_z_path' else dh * z) + \
            torch.cat((fg[:, :2 * H], fg[:, 3 * H:]), 1) @ w_hh
        dc = torch.cat((dr, dz, dn), 1) @ w_ic
        d_ctx[l] = dc
        g = torch.einsum('tbe,be->bt', encoded, dc) * tail
        if d_att is not None:
            g = g + c(d_att[l])
        a = att[l] * live
        ds = a * (g - (a * g).sum(1, keepdim=True))
        th = _tanh(ep + rec[l][:, None, :], tanh_form)
        dpre = ds[:, :, None] * v * (1 - th * th)
        grad = grad + dpre
        d_rec[l] = dpre.sum(1)
        d_v += (ds[:, :, None] * th).sum(1)
        if mut != 'w_rec_carry_dropped':
            carry = carry + (d_rec[l] if forced is None else c(forced['d_rec'][l])) @ w_rec
        if aux is not None:
            aux[l] = (r, z, n, hn, hp, a, ds, th)
    grad = grad.permute(1, 0, 2)
    pre = torch.zeros_like(grad) if d_eproj is None else c(d_eproj)
    wrote = live.t()[:, :, None].bool()
    total = torch.where(wrote, grad if mut == 'd_eproj_overwrites_prefill' else pre + grad, pre)
    return dict(d_eproj=total, d_gates=d_gates, d_contexts=d_ctx, d_rec=d_rec, d_w_score=d_v, d_h0=carry)


def _gru_bound(aux, w_score, L):
    """the tanh term of the outputs of the teacher-forced GRU reverse scan: 2 |ds w th| TANH_ABS
    summed into d_eproj (over l) and d_rec (over t), |ds| TANH_ABS into d_w_score; the carry is
    formed from the launch's own d_rec, so nothing reaches the other outputs"""
    v = torch.as_tensor(w_score).to(F64).reshape(-1).abs()
    b_eproj, b_v, b_rec = 0.0, 0.0, []
    for l in range(L):
        ds, th = aux[l][6], aux[l][7]
        e = 2 * (ds[:, :, None] * v * th).abs() * TANH_ABS
        b_eproj = b_eproj + e
        b_rec.append(e.sum(1))
        b_v = b_v + ds.abs().sum(1, keepdim=True) * TANH_ABS * torch.ones_like(v)
    return dict(d_eproj=b_eproj.permute(1, 0, 2), d_rec=torch.stack(b_rec), d_w_score=b_v)


# ------------------------------------------------------------------ the case matrix

SPECS = {}
# mutant -> the cases named for it (tests/test_attention_scan_referee.py: rejected at every one)
MUTANT_CASES = {m: [] for m in TCN_MUTANTS + GRU_MUTANTS}


def _tcn(T, B, L, A, tag='', kills=(), **kw):
    name = 'tcn/T%dB%dL%dA%d%s' % (T, B, L, A, '_' + tag if tag else '')
    assert name not in SPECS, name
    SPECS[name] = dict(dict(kind='tcn', name=name, T=T, B=B, L=L, A=A, data='randn', a0='softmax',
                            d_att='randn', temperature=1.25), **kw)
    for m in kills:
        MUTANT_CASES[m].append(name)
    return name


def _gru(T, B, L, A, E, H, tag='', kills=(), **kw):
    name = 'gru/T%dB%dL%dA%dE%dH%d%s' % (T, B, L, A, E, H, '_' + tag if tag else '')
    assert name not in SPECS, name
    SPECS[name] = dict(dict(kind='gru', name=name, T=T, B=B, L=L, A=A, E=E, H=H, lens=None, d_att=True,
                            d_states=True), **kw)
    for m in kills:
        MUTANT_CASES[m].append(name)
    return name


def _matrix():
    _tcn(1, 1, 1, 1)
    # T around the 32 taps
    for T in (5, 31, 32, 33):
        _tcn(T, 2, 3, 8, kills=('window_shift_by_one', 'taps_reversed', 'softmax_bwd_without_dot',
                                'temperature_missing_in_bwd') if T == 33 else ())
    # every kind of unit split at T = 70 (plan(70, A): test_attention_scan_referee.py)
    for A in (1, 7, 100, 200, 255, 256):
        _tcn(70, 2, 3, A, kills=('last_unit_chunk_dropped',) if A in (100, 255) else ())
    # T around the backward tile: TT = 64 at A = 64, 16 at A = 256
    for A, Ts in ((64, (63, 64, 65, 129)), (256, (15, 16, 17, 33))):
        for T in Ts:
            kills = ()
            if T in (65, 17):
                kills = ('tile_tail_frames_dropped', 'carry_misses_tile_seam')
            if T in (129, 33):
                kills = ('carry_misses_tile_seam', 'tile_tail_frames_dropped')
            _tcn(T, 2, 3, A, kills=kills)
    # past one pass of 512 threads: the forward split shrinks, down to G = 1
    _tcn(600, 2, 2, 64, kills=('last_unit_chunk_dropped',))
    _tcn(1100, 1, 2, 64)
    _tcn(2100, 1, 2, 8)
    _tcn(4096, 1, 2, 256)                       # the largest LDS plan of both kernels
    # L = 1: d_eproj assigned once, the carry straight into d_a0; L = 5
    _tcn(70, 2, 1, 64, kills=('d_wb_first_utterance_only',))
    _tcn(70, 2, 2, 64, kills=('d_eproj_last_position_only', 'a0_at_every_position'))
    _tcn(70, 2, 5, 64, kills=('carry_not_cleared', 'd_eproj_last_position_only', 'a0_at_every_position',
                              'len_off_by_one'))
    # saturation
    _tcn(70, 2, 3, 64, 'sat', data='sat')                       # exp(2h) overflows
    _tcn(70, 2, 3, 64, 'peaky', data='peaky', temperature=5.0)  # weights underflow
    _tcn(70, 2, 3, 64, 'diffuse', data='diffuse')
    # initial alignments
    _tcn(70, 2, 3, 8, 'a0_onehot', a0='onehot')
    _tcn(70, 2, 3, 8, 'a0_softmax')
    _tcn(70, 2, 3, 8, 'a0_past_len', a0='past_len')
    # exact conditions
    _tcn(70, 2, 2, 8, 'w0', data='w0')
    _tcn(70, 2, 5, 8, 'd_att_single', d_att='single')
    _tcn(70, 2, 3, 8, 'd_att_padded', d_att='padded')
    # a temperature so small that a mask scaled by it no longer underflows
    _tcn(33, 2, 2, 8, 'temperature_1e-4', temperature=1e-4, kills=('mask_before_temperature',))

    _gru(1, 1, 1, 4, 4, 4)
    every = ('carry_without_z_path', 'dgh_n_without_r', 'h_prev_from_same_row', 'w_rec_carry_dropped',
             'd_att_ignored', 'd_states_ignored', 'd_eproj_overwrites_prefill')
    _gru(33, 3, 4, 12, 36, 20, kills=every + ('context_groups_miss_tail', 'len_0_is_empty'))
    _gru(33, 3, 4, 12, 36, 20, 'no_d_att', d_att=False, kills=('d_states_ignored',))
    _gru(33, 3, 4, 12, 36, 20, 'no_d_states', d_states=False, kills=('d_att_ignored',))
    _gru(33, 3, 4, 12, 36, 20, 'short', lens=[3, 9, 15], kills=('context_groups_miss_tail',))
    _gru(33, 3, 1, 12, 36, 20)                  # one position: the carry goes straight into d_h0
    _gru(70, 2, 3, 320, 64, 64, kills=('len_0_is_empty',))
    _gru(50, 4, 5, 64, 320, 256, kills=every)
    _gru(334, 2, 3, 128, 512, 320)
    _gru(1100, 1, 2, 8, 8, 8)
    _gru(4096, 1, 2, 4, 4, 4)


_matrix()


def cases(kind=None):
    return [n for n, s in SPECS.items() if kind is None or s['kind'] == kind]


def tcn_lens(T, B, A, pick):
    """the lengths mix T, 1, a value inside a backward tile and a mid value; one utterance alone
    takes turns (`pick`)"""
    TT = bwd_tiles(A)[0]
    inside = max(1, min(T - 1, TT // 2 + 5 + (TT if T > 2 * TT else 0)))
    vals = [T, inside, max(1, T // 2), 1]
    if B == 1:
        return [vals[pick % 3]]
    pairs = ([T, inside], [1, T], [max(1, T // 2), T], [T, 1])
    return (pairs[pick % 4] + vals)[:B]


def gru_lens(T, B):
    """0 (= T) and T + 5 (= T) among T, 1 and a third of T"""
    return {1: [T + 5 if T < 2000 else 0], 2: [max(1, T // 3), 0], 3: [0, max(1, T // 3), T + 5],
            4: [T, 1, T + 5, max(1, T // 2)]}[B] if T > 1 else [1]


def build(name):
    """the operands of a case as the ABI holds them (fp32 CPU tensors), seeded by its name"""
    s = SPECS[name]
    seed = zlib.crc32(name.encode())
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=gen)  # noqa: E731
    T, B, L, A = s['T'], s['B'], s['L'], s['A']
    tt = torch.arange(T)[:, None]
    if s['kind'] == 'tcn':
        lens = torch.tensor(tcn_lens(T, B, A, seed >> 3), dtype=torch.int32)
        pad = (tt >= lens[None, :].long())
        c = dict(spec=s, eproj=r(T, B, A), filt=0.5 * r(L, B, A * KF), glob=r(L, B, A),
                 w_score=2 * r(A) / A ** 0.5, b_score=torch.tensor([0.3]), temperature=s['temperature'], lens=lens)
        if s['data'] == 'sat':
            c['eproj'] = 20 * c['eproj']
        elif s['data'] == 'peaky':
            c['w_score'] = 10 * c['w_score']
        elif s['data'] == 'diffuse':
            c['w_score'] = 0.01 * c['w_score']
        elif s['data'] == 'w0':
            c['w_score'] = torch.zeros(A)
        init = 2 * r(T, B)
        if s['a0'] == 'onehot':
            c['a0'] = (tt == 0).float().expand(T, B).contiguous()
        elif s['a0'] == 'past_len':
            c['a0'] = torch.softmax(init, 0)
        else:
            c['a0'] = torch.softmax(init + pad.float() * MASKED, 0)
        d = r(L, B, T)
        if s['d_att'] == 'single':
            keep = torch.zeros(L, 1, 1)
            keep[s['L'] // 2] = 1
            d = d * keep
        elif s['d_att'] == 'padded':
            d = d * pad.t()[None].float()
        c['d_att'] = d
        return c
    E, H = s['E'], s['H']
    lens = torch.tensor(s['lens'] or gru_lens(T, B), dtype=torch.int32)
    c = dict(spec=s, eproj=r(T, B, A), encoded=r(T, B, E), lens=lens, gx_emb=r(L, B, 3 * H),
             w_ic=r(3 * H, E) / E ** 0.5, w_hh=r(3 * H, H) / H ** 0.5, b_hh=0.1 * r(3 * H),
             w_rec=r(A, H) / H ** 0.5, w_score=2 * r(A) / A ** 0.5, b_score=torch.tensor([0.3]), h0=0.5 * r(B, H))
    c['d_att'] = r(L, B, T) if s['d_att'] else None
    c['d_states'] = r(L, B, H) if s['d_states'] else None
    c['d_eproj_prefill'] = r(T, B, A)
    return c


# ------------------------------------------------------------------ references, tolerances, judge

TCN_FWD_ARGS = ('eproj', 'filt', 'glob', 'a0', 'w_score', 'b_score', 'temperature', 'lens')
TCN_BWD_ARGS = ('eproj', 'filt', 'glob', 'a0', 'w_score', 'temperature', 'lens')
GRU_FWD_ARGS = ('eproj', 'encoded', 'lens', 'gx_emb', 'w_ic', 'w_hh', 'b_hh', 'w_rec', 'w_score', 'b_score', 'h0')
GRU_BWD_ARGS = ('eproj', 'encoded', 'lens', 'w_ic', 'w_hh', 'w_rec', 'w_score', 'h0')
GRU_SAVED = ('att', 'states', 'gates', 'rec')
ROW_DIMS = dict(att=(2,), states=(2,), contexts=(2,), gates=(2,), rec=(2,), d_filt=(2,), d_glob=(2,),
                d_gates=(2,), d_contexts=(2,), d_rec=(2,), d_eproj=(0, 2), d_a0=(0,), d_wb=(1,),
                d_w_score=(1,), d_h0=(1,))


def forward(c, forced=None, dtype=F64, mut=None, tanh_form=None):
    """-> dict of the forward outputs; forced: the launch's own att (TCN) / states (GRU)"""
    if c['spec']['kind'] == 'tcn':
        return dict(att=tcn_scan_fwd_ref(*(c[k] for k in TCN_FWD_ARGS), forced=forced, dtype=dtype, mut=mut,
                                         tanh_form=tanh_form))
    return att_gru_scan_fwd_ref(*(c[k] for k in GRU_FWD_ARGS), forced=forced, dtype=dtype, mut=mut,
                                tanh_form=tanh_form)


def backward(c, saved, dtype=F64, mut=None, tanh_form=None, aux=None, forced=None):
    """saved: the forward tensors the launch is given (att; for the GRU also states, gates, rec);
    forced: the launch's own d_gates and d_rec (GRU: att_gru_scan_bwd_ref)"""
    if c['spec']['kind'] == 'tcn':
        return tcn_scan_bwd_ref(*(c[k] for k in TCN_BWD_ARGS), saved['att'], c['d_att'], dtype=dtype, mut=mut,
                                tanh_form=tanh_form, aux=aux)
    return att_gru_scan_bwd_ref(*(c[k] for k in GRU_BWD_ARGS), *(saved[k] for k in GRU_SAVED), d_att=c['d_att'],
                                d_states=c['d_states'], d_eproj=c['d_eproj_prefill'], forced=forced, dtype=dtype,
                                mut=mut, tanh_form=tanh_form, aux=aux)


def yardstick(c, op, given, mut=None, forced=None):
    """the same arithmetic in fp32 with the kernels' form of the attention tanh; also the stand-in
    for a kernel on the CPU (`mut`: a wrong one)"""
    out = forward(c, given, F32, mut, 'exp') if op == 'fwd' else backward(c, given, F32, mut, 'exp', forced=forced)
    return {k: v.double() for k, v in out.items()}


def _rowmax(x, name):
    return x.abs().amax(ROW_DIMS[name], keepdim=True)


def _fwd_tanh_terms(c, want, forced):
    s = c['spec']
    if s['kind'] == 'tcn':
        de = 2 * abs(c['temperature']) * float(c['w_score'].abs().sum()) * TANH_ABS
        return dict(att=de * want['att'])
    de = 2 * float(c['w_score'].abs().sum()) * TANH_ABS
    B, H = c['h0'].shape
    e_c = de * torch.einsum('lbt,tbe->lbe', want['att'], c['encoded'].double().abs())
    e_gi = (e_c @ c['w_ic'].double().abs().t()).view(-1, B, 3, H)
    r, z, n, hn = want['gates'].view(-1, B, 4, H).unbind(2)
    hp = torch.cat((c['h0'].double()[None], forced.double()[:-1]))
    e_r, e_z = e_gi[:, :, 0] / 4, e_gi[:, :, 1] / 4
    e_n = e_gi[:, :, 2] + hn.abs() * e_r
    return dict(att=de * want['att'], contexts=e_c, gates=torch.cat((e_r, e_z, e_n, torch.zeros_like(e_n)), 2),
                states=(1 - z).abs() * e_n + (n - hp).abs() * e_z, rec=torch.zeros_like(want['rec']))


def referee(c, op, given, got=None):
    """-> (want, tol): the fp64 reference of one launch and the per-row bounds (module docstring).
    op 'fwd': given = the launch's own att (TCN) / states (GRU), teacher forcing; op 'bwd': given =
    dict of the saved forward tensors the launch read, got = the launch's outputs (the GRU reverse
    scan is teacher-forced with its d_gates and d_rec; None: it runs free)"""
    s = c['spec']
    if op == 'fwd':
        want = forward(c, given)
        terms = _fwd_tanh_terms(c, want, given)
    else:
        aux = {}
        forced = got if s['kind'] == 'gru' else None
        want = backward(c, given, aux=aux, forced=forced)
        if s['kind'] == 'tcn':
            terms = _tcn_bound(aux, c['w_score'], c['temperature'], s['L'])
        else:
            terms = _gru_bound(aux, c['w_score'], s['L'])
    y32 = yardstick(c, op, given, forced=forced if op == 'bwd' else None)
    tol = {}
    for k, w in want.items():
        tol[k] = 4 * _rowmax(y32[k] - w, k) + 4 * EPS32 * _rowmax(w, k)
        if k in terms:
            tol[k] = tol[k] + _rowmax(terms[k], k)
    return want, tol


def tolerances(c, op, given, got=None):
    return referee(c, op, given, got)[1]


def _exact_zero(name, x, bad):
    if bool((x != 0).any()):
        bad.append('%s: %d entries are not exactly 0' % (name, int((x != 0).sum())))


def judge(c, op, got, want, tol, stats=None):
    """the complaints about the outputs `got` (fp32 CPU tensors, or fp64 values of them) of one launch"""
    s = c['spec']
    bad, stats = [], ({} if stats is None else stats)
    got = {k: torch.as_tensor(v).double() for k, v in got.items()}
    for k, w in want.items():
        g = got[k]
        if g.shape != w.shape:
            bad.append('%s: shape %s, want %s' % (k, tuple(g.shape), tuple(w.shape)))
            continue
        err = (g - w).abs()
        ok = err <= tol[k]                                  # NaN fails
        share = torch.where(err > 0, err / tol[k], torch.zeros_like(err))      # (a zero bound: inf)
        stats[k] = float(err.max())
        stats[k + ':share'] = float(torch.nan_to_num(share, nan=float('inf')).max())
        if not bool(ok.all()):
            i = tuple(int(x) for x in (~ok).nonzero()[0])
            bad.append('%s: %d entries outside, first at %s: got %.9g want %.9g tol %.3g' % (
                k, int((~ok).sum()), i, float(g[i]), float(w[i]), float(tol[k].expand_as(w)[i])))
    T = s['T']
    t = torch.arange(T)
    if op == 'fwd':
        att = got['att']
        ln = (c['lens'].long() if s['kind'] == 'tcn' else clamp_len(c['lens'], T))
        rows = (att.sum(2) - 1).abs()
        if not bool((rows <= 1e-5).all()):
            bad.append('rows of att do not sum to 1: %.3g' % float(rows.max()))
        behind = (t[None, :] >= ln[:, None])[None].expand_as(att)
        _exact_zero('att at or past len', att[behind], bad)
        if s.get('data') == 'w0':
            flat = (1 / ln.float())[None, :, None].expand_as(att).double()
            if not torch.equal(att[~behind], flat[~behind]):
                bad.append('att with w_score = 0 is not float32(1) / float32(len) bit for bit')
        return bad
    for k in want:
        if bool((got[k] == POISON).any()) and not (s['kind'] == 'gru' and k == 'd_eproj'):
            bad.append('%s: %d entries still hold the POISON' % (k, int((got[k] == POISON).sum())))
    if s['kind'] == 'tcn':
        if s['d_att'] == 'single':
            l0 = s['L'] // 2
            _exact_zero('d_filt past l0', got['d_filt'][l0 + 1:], bad)
            _exact_zero('d_glob past l0', got['d_glob'][l0 + 1:], bad)
        if s['d_att'] == 'padded':
            for k in TCN_BWD_KEYS:
                _exact_zero(k, got[k], bad)
    else:
        kept = (t[:, None] >= clamp_len(c['lens'], T)[None, :])[:, :, None].expand_as(got['d_eproj'])
        if not torch.equal(got['d_eproj'][kept], c['d_eproj_prefill'].double()[kept]):
            bad.append('d_eproj: rows at or past len do not keep the pre-fill bit for bit')
    return bad
