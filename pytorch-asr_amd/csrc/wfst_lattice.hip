// Lattice generation from the beam-pruned search over one shared decoding graph (include/asr_amd.h:
// asr_wfst_lattice_f32, asr_wfst_lattice_supported, asr_wfst_lattice_workspace_bytes).
//
// Where the recipe ran Kaldi's decode-faster once per acoustic scale (egs/wsj/ctc_kaldi_decode.sh:
// 160-163), this keeps every arc that lies within lattice_beam of the best path, graph and acoustic
// cost apart (latgen-faster), with the order-independent semantics of DESIGN.md section 4.20.
//
// One workgroup owns one utterance, forward and backward, and synchronises with workgroup barriers
// only.  The forward is wfst_decode.hip's (the shared device code is wfst_search.h); every record of
// its log additionally holds the token's state, its cost alpha, a survivor bit, and room for beta;
// per time k the utterance keeps the offset of its records and the threshold of the emitting phase.
// The backward walks the times down.  Per time k:
//   emitting   (k < n) the scores of frame k are staged again; the arcs of the survivors of time k
//              are expanded exactly as in the forward (block prefix sum of out-degrees, binary
//              search in LDS).  An arc whose proposal passed the frame's threshold finds its
//              destination's record of time k + 1 through the per-state slot table, forms
//              q = (w + a) + beta(dst), lowers beta(src) by a 32-bit atomic minimum over the
//              order-preserving key, and is appended when alpha(src) + q <= best + lattice_beam
//              (or when the search's own traceback took it); both end records are marked;
//   scatter    the records of time k go into the slot table (a hit is validated by record range
//              and state: the table keeps entries of other times);
//   epsilon    the levels in descending rank through the epsilon CSR, the same per-arc work with
//              q = w + beta(dst): beta(dst) is final before its sources' level.
// Then the marked records are compacted into the node arrays, the arcs' end points are renumbered,
// and the counts are written.  Only those leave the device; the order of nodes and arcs is whatever
// the lanes made it, the caller sorts.  Every loop is bounded as in wfst_decode.hip; an utterance
// that outgrows a list (flag 1), the log (2), node_cap (3) or arc_cap (4) raises its flag and ends.
#include "wfst_search.h"
#include "../../include/asr_amd.h"

namespace {

constexpr uint32_t F_SURVIVOR = 1, F_KEPT = 2, F_BEST = 4;

struct Params {
    Graph g;
    const float *lp;            // lp[t * frame_stride + b * C + c]
    int64_t frame_stride;
    const int32_t *lens;
    int T, B, C;
    float beam, lbeam, scale;
    int allow_partial;
    uint32_t list_cap, log_cap, node_cap, arc_cap;
    float *out_cost;
    int32_t *out_final, *out_nnodes, *out_narcs, *out_overflow;
    int32_t *node_time, *node_state;        // [B][node_cap]
    float *node_alpha, *node_beta;
    int32_t *arc_src, *arc_dst;             // [B][arc_cap]
    uint32_t *arc_idx;
    float *arc_lp;
    unsigned long long *tab;    // [B][N]
    uint32_t *slot;             // [B][N]
    uint32_t *lists;            // [B][5][list_cap]
    uint32_t *rec;              // [B][6][log_cap]: arc, source record, state, alpha, beta key, marks
    uint32_t *toff;             // [B][T + 2] first record of every time, and the end
    float *thr;                 // [B][T + 2] thr[k]: threshold of the emitting phase into time k
};

struct Records {
    uint32_t *a, *p, *s, *b, *f;
    float *c;
};

struct Extra {
    uint32_t n_arcs, have;
    float limit;
};

__device__ __forceinline__ uint32_t peek32(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void mark(uint32_t *f, uint32_t bits) {
    if ((peek32(f) & bits) != bits) atomicOr(f, bits);
}

// The records [rbase, rend) of time k over their emitting arcs into the records [dlo, dhi) of time
// k + 1 (EPS = false: survivors only, scores from sc, threshold thr) or, for the records whose state
// has rank `level`, over their epsilon arcs into the same time (dlo = rbase, dhi = rend).
template <int NT, bool EPS>
__device__ __forceinline__ void back_expand(const Params &p, Shared<NT> &sh, Extra &ex, const float *sc,
                                            const Records &R, const uint32_t *slot, uint32_t rbase,
                                            uint32_t rend, uint32_t dlo, uint32_t dhi, int level, float thr,
                                            const float *row, int b) {
    const Graph &g = p.g;
    const int tid = threadIdx.x, C = p.C;
    const uint32_t count = rend - rbase;
    int32_t *const o_src = p.arc_src + (int64_t)b * p.arc_cap;
    int32_t *const o_dst = p.arc_dst + (int64_t)b * p.arc_cap;
    uint32_t *const o_arc = p.arc_idx + (int64_t)b * p.arc_cap;
    float *const o_lp = p.arc_lp + (int64_t)b * p.arc_cap;
    for (uint32_t base = 0; base < count; base += NT) {
        const uint32_t i = base + tid;
        uint32_t deg = 0, first = 0;
        float cs = 0.f;
        if (i < count) {
            const uint32_t r = rbase + i, s = R.s[r];
            if (s >= g.N) {
            } else if (EPS) {
                if (g.rank[s] == level) {
                    first = g.eps_ptr[s];
                    deg = g.eps_ptr[s + 1] - first;
                    if (first > g.E || deg > g.E - first) deg = 0;
                }
            } else if (peek32(R.f + r) & F_SURVIVOR) {
                first = g.ptr[s];
                deg = g.ptr[s + 1] - first;
                if (first > g.A || deg > g.A - first) deg = 0;
            }
            cs = R.c[r];
        }
        uint32_t total;
        const uint32_t off = block_scan<NT>(deg, sh.wsum, total);
        sh.offs[tid] = off;
        sh.first[tid] = first;
        sh.cost[tid] = cs;
        __syncthreads();
        for (uint32_t j = tid; j < total; j += NT) {
            int lo = 0, hi = NT - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (sh.offs[mid] <= j) lo = mid;
                else hi = mid - 1;
            }
            uint32_t a = sh.first[lo] + (j - sh.offs[lo]);
            if (EPS) a = g.eps_arc[a];
            if (a >= g.A) continue;
            const int il = g.il[a];
            if (EPS ? il != 0 : (il <= 0 || il > C)) continue;
            const uint32_t d = (uint32_t)g.dst[a];
            if (d >= g.N) continue;
            const float alpha = sh.cost[lo], w = g.w[a];
            float c = __fadd_rn(alpha, w), x = w;
            if (!EPS) {
                c = __fadd_rn(c, sc[il - 1]);
                x = __fadd_rn(w, sc[il - 1]);
            }
            c = __fadd_rn(c, 0.f);
            if (!(c < INFINITY)) continue;
            if (!EPS && !(c <= thr)) continue;      // the proposal was dropped by the frame's first prune
            const uint32_t dr = slot[d];
            if (dr < dlo || dr >= dhi || R.s[dr] != d) continue;        // a stale entry: d has no token here
            const uint32_t sr = rbase + base + (uint32_t)lo;
            const float q = __fadd_rn(__fadd_rn(x, keyf(peek32(R.b + dr))), 0.f);
            if (q < INFINITY) {
                const uint32_t key = fkey(q);
                if (key < peek32(R.b + sr)) atomicMin(R.b + sr, key);
            }
            const float val = __fadd_rn(alpha, q);
            const bool best_arc = (peek32(R.f + dr) & F_BEST) && R.a[dr] == a;
            if (!((val < INFINITY && val <= ex.limit) || best_arc)) continue;
            const uint32_t pos = atomicAdd(&ex.n_arcs, 1u);
            if (pos < p.arc_cap) {
                o_src[pos] = (int32_t)sr;
                o_dst[pos] = (int32_t)dr;
                o_arc[pos] = a;
                o_lp[pos] = EPS ? 0.f : row[il - 1];
                mark(R.f + sr, F_KEPT);
                mark(R.f + dr, F_KEPT);
            } else {
                sh.ovf = 4;
            }
        }
        __syncthreads();
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void wfst_lattice_kernel(const Params p) {
    constexpr int PRE = MAX_C / NT;                 // score registers per lane
    extern __shared__ __align__(16) float sc[];     // [C] scaled scores of the frame
    __shared__ Shared<NT> sh;
    __shared__ Extra ex;
    const Graph &g = p.g;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = p.T, C = p.C;
    if (tid == 0) {
        p.out_cost[b] = INFINITY;
        p.out_final[b] = 0;
        p.out_nnodes[b] = 0;
        p.out_narcs[b] = 0;
        p.out_overflow[b] = 0;
    }
    const int n = p.lens[b];
    if (n < 1 || n > T) return;

    unsigned long long *const tab = p.tab + (int64_t)b * g.N;
    uint32_t *const slot = p.slot + (int64_t)b * g.N;
    const uint32_t cap = p.list_cap;
    uint32_t *const cur_s = p.lists + (int64_t)b * 5 * cap;
    float *const cur_c = (float *)(cur_s + cap);
    uint32_t *const raw_s = cur_s + 2 * (int64_t)cap;
    uint32_t *const new_s = cur_s + 3 * (int64_t)cap;
    uint32_t *const new_p = cur_s + 4 * (int64_t)cap;
    Records R;
    R.a = p.rec + (int64_t)b * 6 * p.log_cap;
    R.p = R.a + p.log_cap;
    R.s = R.p + p.log_cap;
    R.c = (float *)(R.s + p.log_cap);
    R.b = R.s + 2 * (int64_t)p.log_cap;
    R.f = R.s + 3 * (int64_t)p.log_cap;
    uint32_t *const toff = p.toff + (int64_t)b * (T + 2);
    float *const thrs = p.thr + (int64_t)b * (T + 2);
    const float *const col = p.lp + (int64_t)b * C;

    float pre[PRE];
    auto load_row = [&](int t) {
        const float *const row = col + p.frame_stride * t;
#pragma unroll
        for (int k = 0; k < PRE; ++k) {
            const int c = tid + k * NT;
            pre[k] = c < C ? row[c] : 0.f;
        }
    };
    load_row(0);
    if (tid == 0) {
        sh.ovf = 0;
        sh.rec_used = 0;
        sh.cnt_a = 0;
        sh.cnt_b = 1;
        sh.min_key = NONE;
        ex.n_arcs = 0;
        ex.have = 0;
        new_s[0] = g.start;
        new_p[0] = NONE;
        tab[g.start] = ((unsigned long long)fkey(0.f) << 32) | NONE;
    }
    __syncthreads();
    uint32_t ncur = 0;

    // ---- forward: wfst_decode.hip's frame loop; the log step also keeps state, cost and survivor bit
    for (int t = -1; t < n; ++t) {
        if (t >= 0) {
#pragma unroll
            for (int k = 0; k < PRE; ++k) {
                const int c = tid + k * NT;
                if (c < C) sc[c] = -__fmul_rn(p.scale, pre[k]);
            }
            if (t + 1 < n) load_row(t + 1);
            __syncthreads();
            expand<NT, false>(g, sh, sc, C, cur_s, cur_c, ncur, 0, tab, raw_s, nullptr, &sh.cnt_a, cap);
            __syncthreads();
            if (sh.ovf) break;
            const uint32_t nraw = sh.cnt_a;
            uint32_t m = NONE;
            for (uint32_t i = tid; i < nraw; i += NT) m = min(m, (uint32_t)(tab[raw_s[i]] >> 32));
            m = wave_min_u32(m);
            if ((tid & 63) == 0 && m != NONE) atomicMin(&sh.min_key, m);
            __syncthreads();
            const float thr = __fadd_rn(keyf(sh.min_key), p.beam);
            if (tid == 0) thrs[t + 1] = thr;
            for (uint32_t i = tid; i < nraw; i += NT) {
                const uint32_t s = raw_s[i];
                const unsigned long long k = tab[s];
                if (keyf((uint32_t)(k >> 32)) <= thr) {
                    const uint32_t pos = atomicAdd(&sh.cnt_b, 1u);      // <= nraw <= cap
                    new_s[pos] = s;
                    new_p[pos] = slot[g.src[(uint32_t)k]];
                } else {
                    tab[s] = EMPTY;
                }
            }
        }
        for (int level = 0; level < g.num_ranks; ++level) {
            __syncthreads();
            const bool full = sh.ovf != 0;
            const uint32_t cnt = min(sh.cnt_b, cap);
            __syncthreads();
            if (full) break;
            expand<NT, true>(g, sh, sc, C, new_s, nullptr, cnt, level, tab, new_s, new_p, &sh.cnt_b, cap);
        }
        __syncthreads();
        if (sh.ovf) break;
        const uint32_t n2 = sh.cnt_b, rec_base = sh.rec_used;
        if (n2 > p.log_cap - rec_base) {            // uniform
            if (tid == 0) sh.ovf = 2;
            __syncthreads();
            break;
        }
        if (tid == 0) {
            sh.min_key = NONE;
            sh.cnt_a = 0;
            toff[t + 1] = rec_base;
        }
        __syncthreads();
        {
            uint32_t m = NONE;
            for (uint32_t i = tid; i < n2; i += NT) {
                const uint32_t s = new_s[i];
                slot[s] = rec_base + i;
                m = min(m, (uint32_t)(tab[s] >> 32));
            }
            m = wave_min_u32(m);
            if ((tid & 63) == 0 && m != NONE) atomicMin(&sh.min_key, m);
        }
        __syncthreads();
        const bool last = t == n - 1;
        const float thr = __fadd_rn(keyf(sh.min_key), p.beam);
        for (uint32_t i = tid; i < n2; i += NT) {
            const uint32_t s = new_s[i];
            const unsigned long long k = tab[s];
            const uint32_t a = (uint32_t)k;
            uint32_t prev = NONE;
            if (a != NONE) prev = g.il[a] == 0 ? slot[g.src[a]] : new_p[i];
            const float c = keyf((uint32_t)(k >> 32));
            const bool survives = last || c <= thr;
            const uint32_t r = rec_base + i;
            R.a[r] = a;
            R.p[r] = prev;
            R.s[r] = s;
            R.c[r] = c;
            R.b[r] = fkey(INFINITY);
            R.f[r] = survives ? F_SURVIVOR : 0u;
            if (survives) {
                const uint32_t pos = atomicAdd(&sh.cnt_a, 1u);          // <= n2 <= cap
                cur_s[pos] = s;
                cur_c[pos] = c;
            }
            tab[s] = EMPTY;
        }
        __syncthreads();
        ncur = sh.cnt_a;
        __syncthreads();
        if (tid == 0) {
            sh.rec_used = rec_base + n2;
            sh.cnt_a = 0;
            sh.cnt_b = 0;
            sh.min_key = NONE;
        }
    }
    if (sh.ovf) {       // uniform: every way to the flag passes a barrier
        if (tid == 0) p.out_overflow[b] = (int32_t)sh.ovf;
        return;
    }

    // ---- the search's answer; one lane marks its traceback
    if (tid == 0) sh.best_final = sh.best_any = EMPTY;
    __syncthreads();
    for (uint32_t i = tid; i < ncur; i += NT) {
        const uint32_t s = cur_s[i];
        const float c = cur_c[i], f = g.fin[s];
        atomicMin(&sh.best_any, ((unsigned long long)fkey(c) << 32) | s);
        if (f < INFINITY) {
            const float tot = __fadd_rn(__fadd_rn(c, f), 0.f);
            if (tot < INFINITY) atomicMin(&sh.best_final, ((unsigned long long)fkey(tot) << 32) | s);
        }
    }
    __syncthreads();
    const uint32_t total = sh.rec_used;
    const bool reached = sh.best_final != EMPTY;
    if (tid == 0) {
        const unsigned long long best = reached ? sh.best_final : sh.best_any;
        if (best != EMPTY && (reached || p.allow_partial)) {
            const float cost = keyf((uint32_t)(best >> 32));
            ex.have = 1;
            ex.limit = __fadd_rn(cost, p.lbeam);
            toff[n + 1] = total;
            uint32_t r = slot[(uint32_t)best];
            for (uint32_t step = 0; step < total && r < total; ++step) {
                if (R.a[r] == NONE) break;          // the start token
                R.f[r] |= F_BEST;
                r = R.p[r];
            }
            p.out_cost[b] = cost;
            p.out_final[b] = reached ? 1 : 0;
        }
    }
    __syncthreads();
    if (!ex.have) return;       // uniform: no lattice

    // ---- backward
    for (int k = n; k >= 0; --k) {
        const uint32_t rbase = toff[k], rend = toff[k + 1];
        if (k < n) {
            const float *const row = col + p.frame_stride * k;
            for (int c = tid; c < C; c += NT) sc[c] = -__fmul_rn(p.scale, row[c]);
            __syncthreads();
            back_expand<NT, false>(p, sh, ex, sc, R, slot, rbase, rend, rend, toff[k + 2], 0, thrs[k + 1], row, b);
        }
        for (uint32_t r = rbase + tid; r < rend; r += NT) {
            const uint32_t s = R.s[r];
            slot[s] = r;
            if (k == n) R.b[r] = reached ? fkey(__fadd_rn(g.fin[s], 0.f)) : fkey(0.f);
            if (k == 0 && s == g.start) R.f[r] |= F_KEPT;       // no other lane touches the marks here
        }
        __syncthreads();
        for (int level = g.num_ranks - 1; level >= 0; --level) {
            back_expand<NT, true>(p, sh, ex, sc, R, slot, rbase, rend, rbase, rend, level, 0.f, nullptr, b);
        }
        if (sh.ovf) break;      // uniform: back_expand ends with a barrier
    }
    if (sh.ovf) {
        if (tid == 0) p.out_overflow[b] = (int32_t)sh.ovf;
        return;
    }

    // ---- output: marked records become nodes (their number goes where the source record was)
    int32_t *const n_time = p.node_time + (int64_t)b * p.node_cap;
    int32_t *const n_state = p.node_state + (int64_t)b * p.node_cap;
    float *const n_alpha = p.node_alpha + (int64_t)b * p.node_cap;
    float *const n_beta = p.node_beta + (int64_t)b * p.node_cap;
    uint32_t nodes = 0;
    for (uint32_t base = 0; base < total; base += NT) {
        const uint32_t r = base + tid;
        const uint32_t kept = (r < total && (R.f[r] & F_KEPT)) ? 1u : 0u;
        uint32_t cnt;
        const uint32_t idx = nodes + block_scan<NT>(kept, sh.wsum, cnt);
        if (kept && idx < p.node_cap) {
            int lo = 0, hi = n;                     // the last time whose first record is <= r
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (toff[mid] <= r) lo = mid;
                else hi = mid - 1;
            }
            n_time[idx] = lo;
            n_state[idx] = (int32_t)R.s[r];
            n_alpha[idx] = R.c[r];
            n_beta[idx] = keyf(R.b[r]);
            R.p[r] = idx;
        }
        nodes += cnt;
        __syncthreads();                            // wsum is reused by the next round
    }
    if (nodes > p.node_cap) {                       // uniform
        if (tid == 0) p.out_overflow[b] = 3;
        return;
    }
    __syncthreads();
    const uint32_t narcs = ex.n_arcs;               // <= arc_cap: otherwise the flag was raised above
    int32_t *const o_src = p.arc_src + (int64_t)b * p.arc_cap;
    int32_t *const o_dst = p.arc_dst + (int64_t)b * p.arc_cap;
    for (uint32_t j = tid; j < narcs; j += NT) {
        o_src[j] = (int32_t)R.p[(uint32_t)o_src[j]];
        o_dst[j] = (int32_t)R.p[(uint32_t)o_dst[j]];
    }
    if (tid == 0) {
        p.out_nnodes[b] = (int32_t)nodes;
        p.out_narcs[b] = (int32_t)narcs;
    }
}

struct Layout {
    int64_t tab, slot, lists, rec, toff, thr, total;
};

Layout layout(int64_t N, int64_t B, int64_t T, int64_t list_cap, int64_t log_cap) {
    Layout l;
    l.tab = 0;
    l.slot = up16(B * N * 8);
    l.lists = l.slot + up16(B * N * 4);
    l.rec = l.lists + up16(B * 5 * list_cap * 4);
    l.toff = l.rec + up16(B * 6 * log_cap * 4);
    l.thr = l.toff + up16(B * (T + 2) * 4);
    l.total = l.thr + up16(B * (T + 2) * 4);
    return l;
}

bool cap_ok(int64_t v) { return v >= 1 && v < ((int64_t)1 << 31); }

}  // namespace

extern "C" int asr_wfst_lattice_supported(int64_t N, int64_t A, int C, int T) { return shapes_ok(N, A, C, T) ? 1 : 0; }

extern "C" int64_t asr_wfst_lattice_workspace_bytes(int64_t N, int B, int T, int64_t list_cap, int64_t log_cap) {
    if (N < 1 || B < 1 || T < 1 || !cap_ok(list_cap) || !cap_ok(log_cap)) return 0;
    return layout(N, B, T, list_cap, log_cap).total;
}

extern "C" int asr_wfst_lattice_f32(const float *lp, int64_t frame_stride, const int32_t *lens, int T, int B, int C,
                                    int64_t N, int64_t A, const uint32_t *arc_ptr, const int32_t *arc_src,
                                    const int32_t *arc_dst, const int32_t *arc_ilabel, const int32_t *arc_olabel,
                                    const float *arc_weight, const float *final_cost, const uint32_t *eps_ptr,
                                    const uint32_t *eps_arc, int64_t E, const int32_t *eps_rank, int num_ranks,
                                    int start, float beam, float lattice_beam, float acoustic_scale,
                                    int allow_partial, int64_t list_cap, int64_t log_cap, int64_t node_cap,
                                    int64_t arc_cap, int threads, float *out_cost, int32_t *out_reached_final,
                                    int32_t *out_num_nodes, int32_t *out_num_arcs, int32_t *node_time,
                                    int32_t *node_state, float *node_alpha, float *node_beta,
                                    int32_t *lat_src, int32_t *lat_dst, uint32_t *lat_arc, float *lat_lp,
                                    int32_t *out_overflow, void *workspace, int64_t workspace_bytes,
                                    void *stream) {
    if (B < 0 || T < 0 || C < 1 || N < 1 || A < 0 || E < 0 || E > A || num_ranks < 0) return ASR_EINVAL;
    if (threads != 0 && threads != 256 && threads != 512 && threads != 1024) return ASR_EINVAL;
    if (start < 0 || start >= N || !(beam >= 0.f) || !(lattice_beam >= 0.f)) return ASR_EINVAL;
    if (!cap_ok(list_cap) || !cap_ok(log_cap) || !cap_ok(node_cap) || !cap_ok(arc_cap)) return ASR_EINVAL;
    if (frame_stride < (int64_t)B * C) return ASR_EINVAL;
    if (B == 0) return ASR_OK;
    if (!shapes_ok(N, A, C, T)) return ASR_EUNSUPPORTED;
    if (!lp || !lens || !arc_ptr || !final_cost || !eps_ptr || !eps_rank || !out_cost || !out_reached_final ||
        !out_num_nodes || !out_num_arcs || !node_time || !node_state || !node_alpha || !node_beta || !lat_src ||
        !lat_dst || !lat_arc || !lat_lp || !out_overflow)
        return ASR_EINVAL;
    if (A > 0 && (!arc_src || !arc_dst || !arc_ilabel || !arc_weight)) return ASR_EINVAL;
    if (E > 0 && !eps_arc) return ASR_EINVAL;
    const Layout l = layout(N, B, T, list_cap, log_cap);
    if (!workspace || workspace_bytes < l.total) return ASR_EINVAL;
    uint8_t *const ws = (uint8_t *)workspace;
    if (hipMemsetAsync(ws + l.tab, 0xFF, (size_t)B * N * 8, (hipStream_t)stream) != hipSuccess) return ASR_ELAUNCH;
    Params p;
    p.g = Graph{(uint32_t)N, (uint32_t)A, (uint32_t)E, arc_ptr, arc_src, arc_dst, arc_ilabel, arc_olabel, arc_weight,
                final_cost, eps_ptr, eps_arc, eps_rank, num_ranks, (uint32_t)start};
    p.lp = lp;
    p.frame_stride = frame_stride;
    p.lens = lens;
    p.T = T;
    p.B = B;
    p.C = C;
    p.beam = beam;
    p.lbeam = lattice_beam;
    p.scale = acoustic_scale;
    p.allow_partial = allow_partial;
    p.list_cap = (uint32_t)list_cap;
    p.log_cap = (uint32_t)log_cap;
    p.node_cap = (uint32_t)node_cap;
    p.arc_cap = (uint32_t)arc_cap;
    p.out_cost = out_cost;
    p.out_final = out_reached_final;
    p.out_nnodes = out_num_nodes;
    p.out_narcs = out_num_arcs;
    p.out_overflow = out_overflow;
    p.node_time = node_time;
    p.node_state = node_state;
    p.node_alpha = node_alpha;
    p.node_beta = node_beta;
    p.arc_src = lat_src;
    p.arc_dst = lat_dst;
    p.arc_idx = lat_arc;
    p.arc_lp = lat_lp;
    p.tab = (unsigned long long *)(ws + l.tab);
    p.slot = (uint32_t *)(ws + l.slot);
    p.lists = (uint32_t *)(ws + l.lists);
    p.rec = (uint32_t *)(ws + l.rec);
    p.toff = (uint32_t *)(ws + l.toff);
    p.thr = (float *)(ws + l.thr);
    const size_t lds = (size_t)C * sizeof(float);
    switch (pick_threads(B, threads)) {
    case 256: hipLaunchKernelGGL(wfst_lattice_kernel<256>, dim3(B), dim3(256), lds, (hipStream_t)stream, p); break;
    case 512: hipLaunchKernelGGL(wfst_lattice_kernel<512>, dim3(B), dim3(512), lds, (hipStream_t)stream, p); break;
    default: hipLaunchKernelGGL(wfst_lattice_kernel<1024>, dim3(B), dim3(1024), lds, (hipStream_t)stream, p); break;
    }
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
