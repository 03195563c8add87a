// The LM-fused beam search on the device (BeamSearchLM, reference
// att_speech/modules/beam_search.py:185-363, for any number of utterances):
//
//  asr_lm_label_costs_f64 — the LM cost of EVERY (hypothesis, class) extension, straight from the
//      hypothesis' bag {LM state: cost}: cost = -log sum over bag entries and over the arcs with
//      the class' LM label of exp(-(w + arc_w_closed)), where arc_w_closed = weight - log Z(dst)
//      already carries the total weight of the epsilon paths behind the arc (the closure is linear
//      in the log semiring), so no closure is run here.
//  asr_beam_lm_step_f32 — BeamSearchLM.step for every utterance in one launch, one workgroup per
//      utterance: log-softmax with the EOS floor, acoustic + LM + coverage, the finish test with
//      this step's alignment, the sorted finished list, the best hypothesis and its score
//      elements, the top-k on the fused score, the gather of the acoustic scores, the re-indexing
//      of histories / coverage / EOS floors, and the per-utterance freeze.
//  asr_beam_lm_step_graph_f32 — the same kernel with the two outputs GraphSearch.step needs on top:
//      the finish mask of the old slots and the fused score of the chosen extensions.
//  asr_graph_merge_f32 — the merge bookkeeping of GraphSearch.step (reference :466-476, :518-590)
//      on a caller-owned node store, one workgroup per utterance, after the bags advanced.
//  asr_lm_bag_advance_f64 — the bags of the survivors only: arcs of the chosen label out of the
//      parent's bag (range search in the ilabel-sorted arcs), equal targets merged, then the
//      epsilon closure level by level in eps_rank order.  One wave per survivor; lane i keeps
//      entry i of the bag in registers, so no LDS ordering is needed inside the wave.
//
// fp64 for everything the LM touches (as the host's numpy), fp32 for the scores (as torch).  Every
// sum has one owner and a fixed order; the only atomic is an integer max for the overflow word.
#include "common.h"
#include "../../include/asr_amd.h"

namespace {

using namespace asr;

constexpr int CAP = ASR_LM_BAG_CAP;
static_assert(CAP <= 64, "one lane per bag entry");

// -log(exp(-a) + exp(-b)) the way numpy's logaddexp does it
__device__ __forceinline__ double cost_add(double a, double b) {
    const double lo = fmin(a, b), hi = fmax(a, b);
    if (!(hi < INFINITY)) return lo;
    return lo - log1p(exp(lo - hi));
}

// first arc of [lo, hi) whose ilabel is >= l (the arcs of a state are ilabel-sorted)
__device__ __forceinline__ int arc_lower_bound(const int32_t *ilabel, int lo, int hi, int l) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ilabel[mid] < l) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------ label costs
struct CostParams {
    const int32_t *ptr, *ilabel;
    const double *w_closed;
    int nstates;
    const int32_t *bag_state, *bag_n;
    const double *bag_cost;
    const int32_t *mapping, *frozen;
    int hyps, beam, C;
    double *cost;
};

__global__ __launch_bounds__(256) void lm_label_costs_kernel(CostParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.hyps * p.C) return;
    const int h = i / p.C, c = i % p.C;
    if (p.frozen && p.frozen[h / p.beam]) return;
    const int l = p.mapping[c];
    int n = p.bag_n[h];
    n = n < 0 ? 0 : (n > CAP ? CAP : n);
    // online log-sum-exp of v = -(w + arc weight), in the order (bag entry, arc)
    double m = -INFINITY, s = 0.0;
    for (int j = 0; j < n; ++j) {
        const int st = p.bag_state[(size_t)h * CAP + j];
        if (st < 0 || st >= p.nstates) continue;
        const double w = p.bag_cost[(size_t)h * CAP + j];
        const int hi = p.ptr[st + 1];
        for (int a = arc_lower_bound(p.ilabel, p.ptr[st], hi, l); a < hi && p.ilabel[a] == l; ++a) {
            const double v = -(w + p.w_closed[a]);
            if (!(v > -INFINITY)) continue;
            if (v > m) { s = s * exp(m - v) + 1.0; m = v; }
            else s += exp(v - m);
        }
    }
    p.cost[i] = s > 0.0 ? -(m + log(s)) : INFINITY;
}

// ------------------------------------------------------------------ survivors' bags
struct AdvParams {
    const int32_t *ptr, *ptr_ne, *dst, *ilabel, *rank;
    const double *weight;
    int nstates, max_rank;
    const int32_t *mapping;
    const int32_t *in_state, *in_n;
    const double *in_cost;
    const int32_t *parent, *new_input, *nsteps;
    int step, hyps, beam;
    int32_t *out_state, *out_n;
    double *out_cost;
    int32_t *overflow;
};

// lane i holds entry i; (s, c) joins the bag: merged into an equal state, or appended
__device__ __forceinline__ void bag_insert(int &st, double &w, int &n, int s, double c, int lane) {
    const bool hit = lane < n && lane < CAP && st == s;
    if (__ballot(hit)) {
        if (hit) w = cost_add(w, c);
    } else {
        if (lane == n && lane < CAP) { st = s; w = c; }
        n += 1;                         // counts on beyond the cap: the size the bag asked for
    }
}

__global__ __launch_bounds__(256) void lm_bag_advance_kernel(AdvParams p) {
    const int lane = threadIdx.x & 63;
    const int hn = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (hn >= p.hyps) return;
    if (p.nsteps[hn / p.beam] != p.step + 1) return;       // frozen before this step
    const int hp = p.parent[hn];
    const int letter = p.new_input[hn];
    if (hp < 0 || hp >= p.hyps || letter < 0) return;
    const int l = p.mapping[letter];
    int n_src = p.in_n[hp];
    n_src = n_src < 0 ? 0 : (n_src > CAP ? CAP : n_src);
    const int src_s = lane < n_src ? p.in_state[(size_t)hp * CAP + lane] : -1;
    const double src_w = lane < n_src ? p.in_cost[(size_t)hp * CAP + lane] : INFINITY;
    int st = -1, n = 0;
    double w = INFINITY;
    for (int j = 0; j < n_src; ++j) {
        const int s = __shfl(src_s, j, 64);
        const double c0 = __shfl(src_w, j, 64);
        if (s < 0 || s >= p.nstates) continue;
        const int hi = p.ptr[s + 1];
        for (int a = arc_lower_bound(p.ilabel, p.ptr[s], hi, l); a < hi && p.ilabel[a] == l; ++a)
            bag_insert(st, w, n, p.dst[a], c0 + p.weight[a], lane);
    }
    // epsilon closure: a state of rank r is final once the levels below r are pushed
    for (int level = 0; level <= p.max_rank; ++level) {
        const int n0 = n < CAP ? n : CAP;
        for (int i = 0; i < n0; ++i) {
            const int s = __shfl(st, i, 64);
            if (s < 0 || s >= p.nstates || p.rank[s] != level) continue;
            const double c0 = __shfl(w, i, 64);
            const int hi = p.ptr_ne[s];
            for (int a = p.ptr[s]; a < hi; ++a)
                bag_insert(st, w, n, p.dst[a], c0 + p.weight[a], lane);
        }
    }
    if (n > CAP) {
        if (lane == 0) atomicMax(p.overflow, n);
        n = CAP;
    }
    // ascending state order, the order of the host's bags
    int pos = 0;
    for (int j = 0; j < n; ++j) pos += __shfl(st, j, 64) < st ? 1 : 0;
    if (lane < n) {
        p.out_state[(size_t)hn * CAP + pos] = st;
        p.out_cost[(size_t)hn * CAP + pos] = w;
    }
    if (lane == 0) p.out_n[hn] = n;
}

// ------------------------------------------------------------------ beam bookkeeping
struct StepParams {
    const float *logits, *att, *scores_in;
    float *scores_out;
    const int32_t *est_in;
    int32_t *est_out;
    const double *lm_cost;
    const float *cov_in;
    float *cov_out, *min_eos;
    const int32_t *lens;
    int step, B, beam, C, T, Lcap;
    float len_div, cov_tau, cov_weight;
    double min_att_pos, lm_weight;
    int32_t *fin_count, *fin_par;
    float *fin_score;
    int32_t *fin_len, *fin_beam, *fin_tokens;
    float *best_score;
    int32_t *best_len, *best_tokens;
    float *best_elems;
    int32_t *new_input, *parent, *frozen, *nsteps;
    int32_t *fin_mask;                       // graph entry only (NULL otherwise): [hyps]
    float *tot_out;                          // graph entry only (NULL otherwise): [hyps]
};

constexpr int NT = 128;
constexpr int BEAM_MAX = 32;
constexpr int CAND_PER_THREAD = 16;

__global__ __launch_bounds__(NT) void beam_lm_step_kernel(StepParams p) {
    __shared__ float lz[BEAM_MAX], eosl[BEAM_MAX], sc[BEAM_MAX], covs[BEAM_MAX];
    __shared__ int amax[BEAM_MAX];
    __shared__ float el_ac[BEAM_MAX], el_lm[BEAM_MAX], c_nrm[BEAM_MAX];
    __shared__ int c_ok[BEAM_MAX];
    __shared__ float m_score[2 * BEAM_MAX], o_score[BEAM_MAX];
    __shared__ int m_src[2 * BEAM_MAX], o_src[BEAM_MAX];
    __shared__ int s_ntot, s_nfin, s_added;
    __shared__ float red_v[NT / 64], sel_v[BEAM_MAX], sel_t[BEAM_MAX];
    __shared__ int red_i[NT / 64], sel_i[BEAM_MAX];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (p.frozen[b]) return;                 // its finished list was full after an earlier step
    const int beam = p.beam, C = p.C, Cm = C - 1, T = p.T, step = p.step;
    const int h0 = b * beam;
    int len = p.lens[b];
    len = len < 0 ? 0 : (len > T ? T : len);
    const bool cov_on = p.cov_weight > 0.f;

    // ---- per hypothesis: EOS floor, log-partition, coverage count, alignment peak ----------
    for (int k = wave; k < beam; k += NT / 64) {
        const int h = h0 + k;
        const float *row = p.logits + (size_t)h * C;
        float e = row[Cm];
        if (p.min_eos) {                     // keep_eos_score: EOS never drops below its past value
            const float floor_ = p.min_eos[h];
            e = e > floor_ ? e : floor_;
        }
        float m = -INFINITY;
        for (int c = lane; c < C; c += 64) m = fmaxf(m, c == Cm ? e : row[c]);
        m = wave_max(m);
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += __expf((c == Cm ? e : row[c]) - m);
        s = wave_sum(s);
        float cnt = 0.f, bv = -INFINITY;
        int bi = 0x7fffffff;
        const float *a = p.att + (size_t)h * T;
        for (int t = lane; t < len; t += 64) {
            const float av = a[t];
            if (cov_on && p.cov_in[(size_t)h * T + t] + av > p.cov_tau) cnt += 1.f;
            if (av > bv) { bv = av; bi = t; }                    // first maximum of this lane
        }
        cnt = wave_sum(cnt);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) {
            lz[k] = m + __logf(s);
            eosl[k] = e;
            sc[k] = p.scores_in[h];
            covs[k] = cov_on ? p.cov_weight * cnt : 0.f;
            amax[k] = bi == 0x7fffffff ? 0 : bi;
        }
    }
    if (tid == 0) { s_ntot = 0; s_added = 0; s_nfin = p.fin_count[b]; }
    __syncthreads();
    auto acoustic = [&](int k, int c) -> float {
        const float x = c == Cm ? eosl[k] : p.logits[(size_t)(h0 + k) * C + c];
        return (x - lz[k]) + sc[k];
    };
    auto lmscore = [&](int k, int c) -> float {
        if (!p.lm_cost) return 0.f;
        return (float)(-p.lm_weight * fmin(1e20, p.lm_cost[(size_t)(h0 + k) * C + c]));
    };
    auto total = [&](int k, int c) -> float {
        float t = acoustic(k, c) + lmscore(k, c);
        if (cov_on) t += covs[k];
        return t;
    };

    // ---- finished hypotheses (_add_finished, _set_best); not before the first label --------
    const int par = p.fin_par[b];
    if (step > 0) {
        const float min_pos = (float)(p.min_att_pos * (double)len);
        for (int k = wave; k < beam; k += NT / 64) {
            float mo = -INFINITY;
            for (int c = lane; c < Cm; c += 64) mo = fmaxf(mo, total(k, c));
            mo = wave_max(mo);
            if (lane == 0) {
                const float te = total(k, Cm), nrm = te / p.len_div;
                el_ac[k] = acoustic(k, Cm);
                el_lm[k] = lmscore(k, Cm);
                c_nrm[k] = nrm;
                // EOS strictly above every class (first maximum), the alignment far enough in
                c_ok[k] = te > mo && (float)amax[k] > min_pos && (double)nrm > -1e10;
                if (p.fin_mask) p.fin_mask[h0 + k] = c_ok[k];
            }
        }
        __syncthreads();
        if (tid == 0) {
            int n = s_nfin;
            for (int i = 0; i < n; ++i) {                        // the old list, sorted
                m_score[i] = p.fin_score[((size_t)par * p.B + b) * beam + i];
                m_src[i] = i;
            }
            for (int k = 0; k < beam; ++k)
                if (c_ok[k]) { m_score[n] = c_nrm[k]; m_src[n] = BEAM_MAX + k; ++n; }
            s_added = n > s_nfin;
            s_ntot = n;
        }
        __syncthreads();
        if (s_added) {
            // stable descending sort: older entries first on ties, then cut to `beam`
            const int ntot = s_ntot;
            if (tid < ntot) {
                int pos = 0;
                const float v = m_score[tid];
                for (int j = 0; j < ntot; ++j)
                    pos += (m_score[j] > v || (m_score[j] == v && j < tid)) ? 1 : 0;
                if (pos < beam) { o_score[pos] = v; o_src[pos] = m_src[tid]; }
            }
            __syncthreads();
            const int nkeep = ntot < beam ? ntot : beam;
            const size_t oldb = ((size_t)par * p.B + b) * beam, newb = ((size_t)(par ^ 1) * p.B + b) * beam;
            for (int r = wave; r <= nkeep; r += NT / 64) {
                // r == nkeep: the best hypothesis, from entry 0, on a strict improvement
                const bool best = r == nkeep;
                if (best && !(o_score[0] > p.best_score[b])) continue;
                const int src = o_src[best ? 0 : r];
                const int32_t *tok;
                int tl, bi;
                if (src < BEAM_MAX) {
                    tok = p.fin_tokens + (oldb + src) * p.Lcap;
                    tl = p.fin_len[oldb + src];
                    bi = p.fin_beam[oldb + src];
                } else {
                    tok = p.est_in + (size_t)(h0 + src - BEAM_MAX) * p.Lcap;
                    tl = step;
                    bi = src - BEAM_MAX;
                }
                tl = tl < 0 ? 0 : (tl > p.Lcap ? p.Lcap : tl);
                int32_t *out = best ? p.best_tokens + (size_t)b * p.Lcap
                                    : p.fin_tokens + (newb + r) * p.Lcap;
                for (int i = lane; i < tl; i += 64) out[i] = tok[i];
                if (lane == 0) {
                    if (best) {
                        p.best_len[b] = tl;
                        // quirk kept: THIS step's score elements at the stored beam index
                        bi = bi < 0 ? 0 : (bi >= beam ? beam - 1 : bi);
                        p.best_elems[b * 3 + 0] = el_ac[bi];
                        p.best_elems[b * 3 + 1] = el_lm[bi];
                        if (cov_on) p.best_elems[b * 3 + 2] = covs[bi];
                    } else {
                        p.fin_score[newb + r] = o_score[r];
                        p.fin_len[newb + r] = tl;
                        p.fin_beam[newb + r] = bi;
                    }
                }
            }
            __syncthreads();                 // best_score is read above, written below
            if (tid == 0) {
                if (o_score[0] > p.best_score[b]) p.best_score[b] = o_score[0];
                p.fin_par[b] = par ^ 1;
                p.fin_count[b] = nkeep;
                s_nfin = nkeep;
            }
        }
    } else if (p.fin_mask && tid < beam) {
        p.fin_mask[h0 + tid] = 0;
    }
    __syncthreads();

    // ---- top-`beam` of the non-EOS extensions on the fused score ----------------------------
    const int ncand = (step == 0 ? 1 : beam) * Cm;              // first step: beam 0 only
    float cv[CAND_PER_THREAD];
#pragma unroll
    for (int i = 0; i < CAND_PER_THREAD; ++i) {
        const int idx = tid + i * NT;
        cv[i] = idx < ncand ? total(idx / Cm, idx % Cm) : -INFINITY;
    }
    for (int r = 0; r < beam; ++r) {
        float bv = -INFINITY;
        int bidx = 0x7fffffff;
#pragma unroll
        for (int i = 0; i < CAND_PER_THREAD; ++i) {
            const int idx = tid + i * NT;
            // (-inf candidates are taken too, in index order; a taken one is NaN, compares false)
            if (idx < ncand && (cv[i] > bv || (cv[i] == bv && idx < bidx))) { bv = cv[i]; bidx = idx; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bidx, o, 64);
            if (ov > bv || (ov == bv && oi < bidx)) { bv = ov; bidx = oi; }
        }
        if (lane == 0) { red_v[wave] = bv; red_i[wave] = bidx; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < NT / 64; ++w)
                if (red_v[w] > bv || (red_v[w] == bv && red_i[w] < bidx)) { bv = red_v[w]; bidx = red_i[w]; }
            sel_v[r] = bv;
            sel_i[r] = bidx;
        }
        __syncthreads();
        const int win = sel_i[r];
#pragma unroll
        for (int i = 0; i < CAND_PER_THREAD; ++i)
            if (tid + i * NT == win) cv[i] = NAN;
    }
    if (tid == 0) {
        // fewer candidates than beams: the last sorted index repeated.  _select's padding rule
        // `new_scores[:, -(beam - ncand):] = -inf` covers EVERY slot when beam == ncand (quirk)
        const int pad_from = beam > ncand ? ncand : (beam == ncand ? 0 : beam);
        int last = 0;
        for (int r = 0; r < beam; ++r) {
            if (sel_i[r] == 0x7fffffff) sel_i[r] = last;
            else last = sel_i[r];
            const int it = sel_i[r];
            sel_v[r] = r >= pad_from ? -INFINITY : acoustic(it / Cm, it % Cm);   // acoustic only
            if (p.tot_out) sel_t[r] = r >= pad_from ? -INFINITY : total(it / Cm, it % Cm);
        }
    }
    __syncthreads();

    // ---- re-index histories, coverage and EOS floors ----------------------------------------
    for (int r = wave; r < beam; r += NT / 64) {
        const int it = sel_i[r], kb = it / Cm, letter = it % Cm;
        const int hp = h0 + kb, hn = h0 + r;
        const int32_t *src = p.est_in + (size_t)hp * p.Lcap;
        int32_t *dst = p.est_out + (size_t)hn * p.Lcap;
        for (int i = lane; i < step; i += 64) dst[i] = src[i];
        if (cov_on)
            for (int t = lane; t < T; t += 64)
                p.cov_out[(size_t)hn * T + t] = p.cov_in[(size_t)hp * T + t] + p.att[(size_t)hp * T + t];
        if (lane == 0) {
            dst[step] = letter;
            p.scores_out[hn] = sel_v[r];
            if (p.tot_out) p.tot_out[hn] = sel_t[r];
            p.new_input[hn] = letter;
            p.parent[hn] = hp;
            if (p.min_eos) p.min_eos[hn] = eosl[kb];             // (all floors were read before the first barrier)
        }
    }
    if (tid == 0) {
        p.nsteps[b] = step + 1;
        if (s_nfin >= beam) p.frozen[b] = 1;
    }
}

// ------------------------------------------------------------------ graph search: hypothesis merging
// GraphSearch.step's two host loops on the node store of one utterance per workgroup.  The walk
// over the new slots is sequential (each sees what the earlier ones did); inside it the key /
// uplink / LM-state filters run one thread per node, the matches are compacted in node order, one
// wave per candidate takes the min-sum (per-lane partial sums in frame order, then the xor
// tree), and wave 0 takes the decisions in candidate order with uniform control flow.  A node
// appended in this launch reads its score from the slot it came from (the host stores a view of
// new_tot_scores[cur]); the store is written back at the end.
struct MergeParams {
    const float *att;
    const int32_t *lens;
    float *scores, *tot;
    const int32_t *est_in, *est_out, *fin_mask, *bag_state, *bag_n, *nsteps;
    const float *len_pow;
    int step, B, beam, T, Lcap, span, Ncap;
    float thr;
    int32_t *node_count;
    float *node_score;
    int32_t *node_len, *node_tokens;
    float *node_att;
    int32_t *node_bag_n, *node_bag_state, *node_fin, *node_uplink;
};

constexpr int MT = 256;
constexpr int T_MAX = 8160;

// the last `span` labels, left-filled with -1, agree (positions past both histories are fill)
__device__ __forceinline__ bool key_equal(const int32_t *ta, int la, const int32_t *tb, int lb, int span) {
    const int mx = la > lb ? la : lb;
    const int n = span < mx ? span : mx;
    for (int j = 1; j <= n; ++j) {
        const int va = j <= la ? ta[la - j] : -1, vb = j <= lb ? tb[lb - j] : -1;
        if (va != vb) return false;
    }
    return true;
}

__global__ __launch_bounds__(MT) void graph_merge_kernel(MergeParams p) {
    __shared__ float s_ns[BEAM_MAX], s_nt[BEAM_MAX], s_sum[MT];
    __shared__ int s_node[BEAM_MAX], s_slot[BEAM_MAX], s_cand[MT], s_wcnt[MT / 64];
    __shared__ int s_count, s_break, s_up;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (p.nsteps[b] != p.step + 1) return;                  // frozen before this step
    const int beam = p.beam, T = p.T, Lcap = p.Lcap, step = p.step, L = step + 1, Ncap = p.Ncap;
    const int h0 = b * beam;
    int len = p.lens[b];
    len = len < 0 ? 0 : (len > T ? T : len);
    float *nscore = p.node_score + (size_t)b * Ncap;
    int32_t *nlen = p.node_len + (size_t)b * Ncap, *nfin = p.node_fin + (size_t)b * Ncap;
    int32_t *nup = p.node_uplink + (size_t)b * Ncap, *nbagn = p.node_bag_n + (size_t)b * Ncap;
    int32_t *ntok = p.node_tokens + (size_t)b * Ncap * Lcap;
    int32_t *nbag = p.node_bag_state + (size_t)b * Ncap * CAP;
    float *natt = p.node_att + (size_t)b * Ncap * T;
    int count0 = p.node_count[b];
    count0 = count0 < 0 ? 0 : (count0 > Ncap ? Ncap : count0);
    if (tid < beam) {
        s_ns[tid] = p.scores[h0 + tid];
        s_nt[tid] = p.tot[h0 + tid];
        s_node[tid] = -1;
    }
    if (tid == 0) s_count = count0;

    // ---- finished marks first: the nodes that ARE the history of an old slot that finished ----
    if (step > 0) {
        for (int k = 0; k < beam; ++k) {
            if (!p.fin_mask[h0 + k]) continue;
            const int32_t *e = p.est_in + (size_t)(h0 + k) * Lcap;
            for (int i = tid; i < count0; i += MT) {
                if (nlen[i] != step) continue;
                bool eq = true;
                for (int j = 0; j < step && eq; ++j) eq = ntok[(size_t)i * Lcap + j] == e[j];
                if (eq) nfin[i] = 1;
            }
        }
    }
    volatile float *vns = s_ns, *vnt = s_nt;

    // ---- the new slots in order ----------------------------------------------------------------
    for (int cur = 0; cur < beam; ++cur) {
        __syncthreads();
        if (vns[cur] == -INFINITY) continue;                 // a dropped slot appends nothing
        const int cnt = s_count;
        const int32_t *e = p.est_out + (size_t)(h0 + cur) * Lcap;
        // (the column at the NEW slot index of this step's alignment, not the parent's: the quirk)
        const float *a = p.att + (size_t)(h0 + cur) * T;
        int bn = 0;
        const int32_t *bs = nullptr;
        if (p.bag_state) {
            bn = p.bag_n[h0 + cur];
            bn = bn < 0 ? 0 : (bn > CAP ? CAP : bn);
            bs = p.bag_state + (size_t)(h0 + cur) * CAP;
        }
        if (tid == 0) { s_break = 0; s_up = -1; }
        for (int base = 0; base < cnt; base += MT) {
            __syncthreads();
            if (s_break) break;
            const int i = base + tid;
            bool pass = false;
            if (i < cnt && nup[i] < 0) {                     // a node with an uplink is dead
                int nl = nlen[i];
                nl = nl < 0 ? 0 : (nl > Lcap ? Lcap : nl);
                pass = key_equal(ntok + (size_t)i * Lcap, nl, e, L, p.span);
                if (pass && bs) {                            // the LM-state sets, as sorted arrays
                    pass = nbagn[i] == bn;
                    for (int j = 0; j < bn && pass; ++j) pass = nbag[(size_t)i * CAP + j] == bs[j];
                }
            }
            const unsigned long long m = __ballot(pass);
            if (lane == 0) s_wcnt[wave] = __popcll(m);
            __syncthreads();
            int off = 0, ncand = 0;
            for (int w = 0; w < MT / 64; ++w) {
                if (w < wave) off += s_wcnt[w];
                ncand += s_wcnt[w];
            }
            if (ncand == 0) continue;
            if (pass) s_cand[off + __popcll(m & ((1ull << lane) - 1ull))] = i;
            __syncthreads();
            for (int c = wave; c < ncand; c += MT / 64) {
                const float *na = natt + (size_t)s_cand[c] * T;
                float s = 0.f;
                for (int t = lane; t < len; t += 64) s += fminf(na[t], a[t]);
                s = wave_sum(s);
                if (lane == 0) s_sum[c] = s;
            }
            __syncthreads();
            if (wave == 0) {
                const float mine = vnt[cur] / p.len_pow[L];
                for (int c = 0; c < ncand; ++c) {
                    if (s_sum[c] < p.thr) continue;          // a different branch
                    const int i = s_cand[c];
                    int nl = nlen[i];
                    nl = nl < 0 ? 0 : (nl > Lcap ? Lcap : nl);
                    const float old = i >= count0 ? vnt[s_slot[i - count0]] : nscore[i];
                    if (old / p.len_pow[nl] >= mine) {       // the old branch is better (ties too)
                        if (lane == 0) { vns[cur] = -INFINITY; vnt[cur] = -INFINITY; s_up = i; s_break = 1; }
                        break;
                    }
                    if (lane == 0) nup[i] = cnt;             // the index the new node is about to get
                    if (lane < beam && lane != cur) {        // drop the candidate's descendants
                        const int32_t *ct = ntok + (size_t)i * Lcap;
                        const int32_t *o = p.est_out + (size_t)(h0 + lane) * Lcap;
                        bool pre = nl <= L;
                        for (int j = 0; j < nl && pre; ++j) pre = ct[j] == o[j];
                        if (pre) { vns[lane] = -INFINITY; vnt[lane] = -INFINITY; }
                    }
                }
            }
        }
        __syncthreads();
        if (cnt < Ncap) {                                    // (cannot fail: Ncap >= (step + 1) * beam)
            for (int j = tid; j < L; j += MT) ntok[(size_t)cnt * Lcap + j] = e[j];
            for (int t = tid; t < T; t += MT) natt[(size_t)cnt * T + t] = a[t];
            for (int j = tid; j < bn; j += MT) nbag[(size_t)cnt * CAP + j] = bs[j];
            if (tid == 0) {
                nlen[cnt] = L;
                nbagn[cnt] = bn;
                nfin[cnt] = 0;
                nup[cnt] = s_up;
                s_node[cur] = cnt;
                s_slot[cnt - count0] = cur;
                s_count = cnt + 1;
            }
        }
    }
    __syncthreads();
    if (tid < beam) {
        p.scores[h0 + tid] = s_ns[tid];
        p.tot[h0 + tid] = s_nt[tid];
        if (s_node[tid] >= 0) nscore[s_node[tid]] = s_nt[tid];   // the view: later drops show
    }
    if (tid == 0) p.node_count[b] = s_count;
}

}  // namespace

extern "C" int asr_beam_lm_supported(int beam, int C, int bag_cap) {
    return beam >= 1 && C >= 2 && beam <= BEAM_MAX && (long)beam * (C - 1) <= (long)NT * CAND_PER_THREAD &&
           bag_cap == CAP;
}

extern "C" int asr_lm_label_costs_f64(const int32_t *ptr, const int32_t *ilabel, const double *arc_w_closed,
                                      int nstates, const int32_t *bag_state, const double *bag_cost,
                                      const int32_t *bag_n, int bag_cap, const int32_t *mapping,
                                      const int32_t *frozen, int B, int beam, int C, double *cost,
                                      void *stream) {
    if (B <= 0 || beam <= 0 || C < 2 || nstates <= 0) return ASR_EINVAL;
    if (bag_cap != CAP || (long)B * beam * C > 0x7fffffffL) return ASR_EUNSUPPORTED;
    if (!ptr || !ilabel || !arc_w_closed || !bag_state || !bag_cost || !bag_n || !mapping || !cost)
        return ASR_EINVAL;
    CostParams p;
    p.ptr = ptr; p.ilabel = ilabel; p.w_closed = arc_w_closed; p.nstates = nstates;
    p.bag_state = bag_state; p.bag_n = bag_n; p.bag_cost = bag_cost; p.mapping = mapping;
    p.frozen = frozen; p.hyps = B * beam; p.beam = beam; p.C = C; p.cost = cost;
    const int n = B * beam * C;
    hipLaunchKernelGGL(lm_label_costs_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}

extern "C" int asr_lm_bag_advance_f64(const int32_t *ptr, const int32_t *ptr_ne, const int32_t *dst,
                                      const int32_t *ilabel, const double *weight, const int32_t *rank,
                                      int nstates, int max_rank, const int32_t *mapping,
                                      const int32_t *in_state, const double *in_cost, const int32_t *in_n,
                                      int32_t *out_state, double *out_cost, int32_t *out_n, int bag_cap,
                                      const int32_t *parent, const int32_t *new_input,
                                      const int32_t *nsteps, int step, int B, int beam,
                                      int32_t *overflow, void *stream) {
    if (B <= 0 || beam <= 0 || nstates <= 0 || max_rank < 0 || step < 0) return ASR_EINVAL;
    if (bag_cap != CAP) return ASR_EUNSUPPORTED;
    if (!ptr || !ptr_ne || !dst || !ilabel || !weight || !rank || !mapping || !in_state || !in_cost ||
        !in_n || !out_state || !out_cost || !out_n || !parent || !new_input || !nsteps || !overflow)
        return ASR_EINVAL;
    if (in_state == out_state || in_cost == out_cost || in_n == out_n) return ASR_EINVAL;
    AdvParams p;
    p.ptr = ptr; p.ptr_ne = ptr_ne; p.dst = dst; p.ilabel = ilabel; p.rank = rank; p.weight = weight;
    p.nstates = nstates; p.max_rank = max_rank; p.mapping = mapping;
    p.in_state = in_state; p.in_n = in_n; p.in_cost = in_cost;
    p.parent = parent; p.new_input = new_input; p.nsteps = nsteps; p.step = step;
    p.hyps = B * beam; p.beam = beam;
    p.out_state = out_state; p.out_n = out_n; p.out_cost = out_cost; p.overflow = overflow;
    hipLaunchKernelGGL(lm_bag_advance_kernel, dim3((p.hyps + 3) / 4), dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}

static int beam_lm_step_launch(const float *logits, const float *att, const int32_t *enc_lens,
                                    const double *lm_cost, double lm_weight,
                                    const float *scores_in, float *scores_out,
                                    const int32_t *est_in, int32_t *est_out,
                                    const float *cov_in, float *cov_out, float *min_eos,
                                    int step, int B, int beam, int C, int T, int Lcap, float len_div,
                                    double min_attention_pos, float coverage_tau, float coverage_weight,
                                    int32_t *fin_count, int32_t *fin_parity, float *fin_score,
                                    int32_t *fin_len, int32_t *fin_beam, int32_t *fin_tokens,
                                    float *best_score, int32_t *best_len, int32_t *best_tokens,
                                    float *best_elems, int32_t *new_input, int32_t *parent,
                                    int32_t *frozen, int32_t *nsteps, int32_t *fin_mask, float *tot_out,
                                    void *stream) {
    if (B <= 0 || beam <= 0 || C < 2 || T <= 0 || step < 0 || Lcap <= step) return ASR_EINVAL;
    if (!asr_beam_lm_supported(beam, C, CAP)) return ASR_EUNSUPPORTED;
    if (!logits || !att || !enc_lens || !scores_in || !scores_out || !est_in || !est_out || !fin_count ||
        !fin_parity || !fin_score || !fin_len || !fin_beam || !fin_tokens || !best_score || !best_len ||
        !best_tokens || !best_elems || !new_input || !parent || !frozen || !nsteps)
        return ASR_EINVAL;
    if (coverage_weight > 0.f && (!cov_in || !cov_out || cov_in == cov_out)) return ASR_EINVAL;
    if (scores_in == scores_out || est_in == est_out) return ASR_EINVAL;
    StepParams p;
    p.logits = logits; p.att = att; p.scores_in = scores_in; p.scores_out = scores_out;
    p.est_in = est_in; p.est_out = est_out; p.lm_cost = lm_cost; p.cov_in = cov_in; p.cov_out = cov_out;
    p.min_eos = min_eos; p.lens = enc_lens;
    p.step = step; p.B = B; p.beam = beam; p.C = C; p.T = T; p.Lcap = Lcap;
    p.len_div = len_div; p.cov_tau = coverage_tau; p.cov_weight = coverage_weight;
    p.min_att_pos = min_attention_pos; p.lm_weight = lm_weight;
    p.fin_count = fin_count; p.fin_par = fin_parity; p.fin_score = fin_score; p.fin_len = fin_len;
    p.fin_beam = fin_beam; p.fin_tokens = fin_tokens; p.best_score = best_score; p.best_len = best_len;
    p.best_tokens = best_tokens; p.best_elems = best_elems; p.new_input = new_input; p.parent = parent;
    p.frozen = frozen; p.nsteps = nsteps; p.fin_mask = fin_mask; p.tot_out = tot_out;
    hipLaunchKernelGGL(beam_lm_step_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}

extern "C" int asr_beam_lm_step_f32(const float *logits, const float *att, const int32_t *enc_lens,
                                    const double *lm_cost, double lm_weight,
                                    const float *scores_in, float *scores_out,
                                    const int32_t *est_in, int32_t *est_out,
                                    const float *cov_in, float *cov_out, float *min_eos,
                                    int step, int B, int beam, int C, int T, int Lcap, float len_div,
                                    double min_attention_pos, float coverage_tau, float coverage_weight,
                                    int32_t *fin_count, int32_t *fin_parity, float *fin_score,
                                    int32_t *fin_len, int32_t *fin_beam, int32_t *fin_tokens,
                                    float *best_score, int32_t *best_len, int32_t *best_tokens,
                                    float *best_elems, int32_t *new_input, int32_t *parent,
                                    int32_t *frozen, int32_t *nsteps, void *stream) {
    return beam_lm_step_launch(logits, att, enc_lens, lm_cost, lm_weight, scores_in, scores_out, est_in, est_out,
                              cov_in, cov_out, min_eos, step, B, beam, C, T, Lcap, len_div, min_attention_pos,
                              coverage_tau, coverage_weight, fin_count, fin_parity, fin_score, fin_len, fin_beam,
                              fin_tokens, best_score, best_len, best_tokens, best_elems, new_input, parent, frozen,
                              nsteps, nullptr, nullptr, stream);
}

extern "C" int asr_beam_lm_step_graph_f32(const float *logits, const float *att, const int32_t *enc_lens,
                                    const double *lm_cost, double lm_weight,
                                    const float *scores_in, float *scores_out,
                                    const int32_t *est_in, int32_t *est_out,
                                    const float *cov_in, float *cov_out, float *min_eos,
                                    int step, int B, int beam, int C, int T, int Lcap, float len_div,
                                    double min_attention_pos, float coverage_tau, float coverage_weight,
                                    int32_t *fin_count, int32_t *fin_parity, float *fin_score,
                                    int32_t *fin_len, int32_t *fin_beam, int32_t *fin_tokens,
                                    float *best_score, int32_t *best_len, int32_t *best_tokens,
                                    float *best_elems, int32_t *new_input, int32_t *parent,
                                    int32_t *frozen, int32_t *nsteps, int32_t *fin_mask, float *tot_out,
                                    void *stream) {
    if (!fin_mask || !tot_out || tot_out == scores_out || tot_out == scores_in) return ASR_EINVAL;
    return beam_lm_step_launch(logits, att, enc_lens, lm_cost, lm_weight, scores_in, scores_out, est_in, est_out,
                              cov_in, cov_out, min_eos, step, B, beam, C, T, Lcap, len_div, min_attention_pos,
                              coverage_tau, coverage_weight, fin_count, fin_parity, fin_score, fin_len, fin_beam,
                              fin_tokens, best_score, best_len, best_tokens, best_elems, new_input, parent, frozen,
                              nsteps, fin_mask, tot_out, stream);
}

extern "C" int asr_graph_search_supported(int beam, int span, int T, int bag_cap) {
    return beam >= 1 && beam <= BEAM_MAX && span >= 0 && T >= 1 && T <= T_MAX && bag_cap == CAP;
}

extern "C" int asr_graph_merge_f32(const float *att, const int32_t *enc_lens, float *scores, float *tot,
                                   const int32_t *est_in, const int32_t *est_out, const int32_t *fin_mask,
                                   const int32_t *bag_state, const int32_t *bag_n, int bag_cap,
                                   const int32_t *nsteps, const float *len_pow, int step, int B, int beam,
                                   int T, int Lcap, int span, float merge_threshold, int Ncap,
                                   int32_t *node_count, float *node_score, int32_t *node_len,
                                   int32_t *node_tokens, float *node_att, int32_t *node_bag_n,
                                   int32_t *node_bag_state, int32_t *node_fin, int32_t *node_uplink,
                                   void *stream) {
    if (B <= 0 || beam <= 0 || T <= 0 || step < 0 || Lcap <= step || span < 0 || Ncap <= 0) return ASR_EINVAL;
    if (!asr_graph_search_supported(beam, span, T, bag_cap)) return ASR_EUNSUPPORTED;
    if (!att || !enc_lens || !scores || !tot || !est_in || !est_out || !fin_mask || !nsteps || !len_pow ||
        !node_count || !node_score || !node_len || !node_tokens || !node_att || !node_bag_n ||
        !node_bag_state || !node_fin || !node_uplink)
        return ASR_EINVAL;
    if ((bag_state == nullptr) != (bag_n == nullptr) || scores == tot || est_in == est_out) return ASR_EINVAL;
    if (!(merge_threshold == merge_threshold)) return ASR_EINVAL;
    if ((long)(step + 1) * beam > (long)Ncap) return ASR_EINVAL;   // the store holds every step's slots
    MergeParams p;
    p.att = att; p.lens = enc_lens; p.scores = scores; p.tot = tot; p.est_in = est_in; p.est_out = est_out;
    p.fin_mask = fin_mask; p.bag_state = bag_state; p.bag_n = bag_n; p.nsteps = nsteps; p.len_pow = len_pow;
    p.step = step; p.B = B; p.beam = beam; p.T = T; p.Lcap = Lcap; p.span = span; p.Ncap = Ncap;
    p.thr = merge_threshold;
    p.node_count = node_count; p.node_score = node_score; p.node_len = node_len; p.node_tokens = node_tokens;
    p.node_att = node_att; p.node_bag_n = node_bag_n; p.node_bag_state = node_bag_state;
    p.node_fin = node_fin; p.node_uplink = node_uplink;
    hipLaunchKernelGGL(graph_merge_kernel, dim3(B), dim3(MT), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
