// Beam-pruned Viterbi search over one shared decoding graph (include/asr_amd.h: asr_wfst_decode_f32,
// asr_wfst_decode_supported, asr_wfst_decode_workspace_bytes).
//
// The reference scores its systems by dumping log-probs and running Kaldi's decode-faster over a
// tropical decoding graph with a beam (egs/wsj/ctc_kaldi_decode.sh:141-147).  This is that search
// as frame-synchronous token passing with the order-independent semantics of DESIGN.md section 4.19:
// every arithmetic step is one fp32 operation without contraction, a state's cost is the minimum of
// its proposals, and of equal proposals the smallest arc index wins.  Both fall out of ONE 64-bit
// unsigned atomic minimum over (order-preserving bits of the cost) << 32 | arc index.
//
// One workgroup owns one utterance for all of its frames and synchronises with workgroup barriers
// only.  Per utterance the workspace holds a table of one such 64-bit word per graph state (all ones
// = no token), a table of record indices per state, three token lists and the back-pointer log.  A
// frame:
//   stage    the frame's C scaled scores -(acoustic_scale * lp) go to LDS from registers that were
//            loaded one frame earlier;
//   expand   NT tokens at a time (NT = the workgroup's threads, pick_threads below): a block-wide
//            prefix sum of their out-degrees, then every lane takes arcs j, j + NT, ... of the
//            chunk and finds its token by binary search over the prefix
//            sums, so a state with thousands of arcs is spread over the whole workgroup;
//   propose  a plain read of the destination's word skips proposals that cannot win (the word only
//            falls during a phase), the others go through the atomic; the lane that finds the word
//            empty appends the state to the new list;
//   prune    against the best emitting cost + beam while compacting the list; pruned words are emptied;
//   closure  the epsilon levels in rank order, over the states of the list whose rank is the level's
//            (a state's cost is final before its level), through a CSR of the epsilon arcs alone;
//   log      every token that exists after the closure gets a record (arc, record of the source's
//            token): the source of an epsilon arc may be pruned below while its target survives;
//   prune    against the best cost + beam into the next frame's list (state, cost); every word that
//            was touched is emptied, so the table is clean for the next frame.
// Every loop is bounded by the frame count, the number of epsilon ranks, the list lengths and the
// arc counts of the listed states; an utterance that outgrows a list or the log raises its flag and
// ends (the caller redoes it on the host).  One lane walks the records back at the end.
#include "common.h"
#include "../../include/asr_amd.h"

namespace {

constexpr int MAX_C = 4096;
constexpr uint32_t NONE = 0xFFFFFFFFu;          // no arc / no record
constexpr unsigned long long EMPTY = ~0ull;     // no token: above the word of every cost, +inf included

struct Graph {
    uint32_t N, A, E;           // states, arcs, epsilon-input arcs
    const uint32_t *ptr;        // [N + 1] arcs of state s: [ptr[s], ptr[s + 1])
    const int32_t *src, *dst, *il, *ol;     // [A]
    const float *w;             // [A]
    const float *fin;           // [N] final cost, +inf = not final
    const uint32_t *eps_ptr;    // [N + 1] into eps_arc
    const uint32_t *eps_arc;    // arc indices of the epsilon-input arcs, by source
    const int32_t *rank;        // [N] epsilon rank
    int num_ranks;              // levels that have epsilon arcs leaving them
    uint32_t start;
};

struct Params {
    Graph g;
    const float *lp;            // lp[t * frame_stride + b * C + c]
    int64_t frame_stride;
    const int32_t *lens;
    int T, B, C;
    float beam, scale;
    int allow_partial;
    uint32_t list_cap, log_cap;
    int word_cap;
    float *out_cost;
    int32_t *out_final, *out_align, *out_nact, *out_words, *out_nwords, *out_overflow;
    unsigned long long *tab;    // [B][N]
    uint32_t *slot;             // [B][N]
    uint32_t *lists;            // [B][5][list_cap]
    uint32_t *rec;              // [B][2][log_cap]
};

__device__ __forceinline__ uint32_t fkey(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float keyf(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ unsigned long long peek(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, ASR_WAVE));
    return v;
}

template <int NT>
struct Shared {
    uint32_t offs[NT], first[NT];
    float cost[NT];
    uint32_t wsum[NT / ASR_WAVE];
    uint32_t cnt_a, cnt_b, ovf, min_key, rec_used;
    unsigned long long best_final, best_any;
};

// exclusive prefix sum of v over the workgroup; total to every thread
template <int NT>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *wsum, uint32_t &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < ASR_WAVE; o <<= 1) {
        const uint32_t nb = (uint32_t)__shfl_up((int)inc, o, ASR_WAVE);
        if (lane >= o) inc += nb;
    }
    __syncthreads();
    if (lane == ASR_WAVE - 1) wsum[wv] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < NT / ASR_WAVE; ++i) {
        const uint32_t s = wsum[i];
        if (i < wv) base += s;
        total += s;
    }
    return base + inc - v;
}

// Pushes the tokens list_s[0 .. count) over their emitting arcs (EPS = false: costs from list_c, scores
// from sc) or, for the tokens whose rank is `level`, over their epsilon arcs (costs from the table).
// New states are appended to out_s through *out_cnt; count is uniform over the workgroup.
template <int NT, bool EPS>
__device__ __forceinline__ void expand(const Graph &g, Shared<NT> &sh, const float *sc, int C,
                                       const uint32_t *list_s, const float *list_c, uint32_t count, int level,
                                       unsigned long long *tab, uint32_t *out_s, uint32_t *out_p,
                                       uint32_t *out_cnt, uint32_t cap) {
    const int tid = threadIdx.x;
    for (uint32_t base = 0; base < count; base += NT) {
        const uint32_t i = base + tid;
        uint32_t deg = 0, first = 0;
        float cs = 0.f;
        if (i < count) {
            const uint32_t s = list_s[i];
            if (s >= g.N) {                         // never written by this kernel; a broken list ends here
            } else if (EPS) {
                if (g.rank[s] == level) {
                    first = g.eps_ptr[s];
                    deg = g.eps_ptr[s + 1] - first;
                    if (first > g.E || deg > g.E - first) deg = 0;      // a broken index ends here
                    if (deg) cs = keyf((uint32_t)(peek(tab + s) >> 32));
                }
            } else {
                first = g.ptr[s];
                deg = g.ptr[s + 1] - first;
                if (first > g.A || deg > g.A - first) deg = 0;
                cs = list_c[i];
            }
        }
        uint32_t total;
        const uint32_t off = block_scan<NT>(deg, sh.wsum, total);
        sh.offs[tid] = off;
        sh.first[tid] = first;
        sh.cost[tid] = cs;
        __syncthreads();
        for (uint32_t j = tid; j < total; j += NT) {
            int lo = 0, hi = NT - 1;                // the last token whose prefix sum is <= j
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
            float c = __fadd_rn(sh.cost[lo], g.w[a]);
            if (!EPS) c = __fadd_rn(c, sc[il - 1]);
            c = __fadd_rn(c, 0.f);                  // -0 and +0 compare equal and must share one word
            if (!(c < INFINITY)) continue;
            const unsigned long long key = ((unsigned long long)fkey(c) << 32) | a;
            if (key >= peek(tab + d)) continue;
            const unsigned long long old = atomicMin(tab + d, key);
            if (old == EMPTY) {
                const uint32_t pos = atomicAdd(out_cnt, 1u);
                if (pos < cap) {
                    out_s[pos] = d;
                    if (EPS) out_p[pos] = NONE;
                } else {
                    sh.ovf = 1;
                }
            }
        }
        __syncthreads();
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void wfst_decode_kernel(const Params p) {
    constexpr int PRE = MAX_C / NT;                 // score registers per lane
    extern __shared__ __align__(16) float sc[];     // [C] scaled scores of the frame
    __shared__ Shared<NT> sh;
    const Graph &g = p.g;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = p.T, C = p.C;
    int32_t *const align = p.out_align + (int64_t)b * T;
    int32_t *const nact = p.out_nact + (int64_t)b * T;
    for (int t = tid; t < T; t += NT) {
        align[t] = -1;
        nact[t] = 0;
    }
    if (tid == 0) {
        p.out_cost[b] = INFINITY;
        p.out_final[b] = 0;
        p.out_nwords[b] = 0;
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
    uint32_t *const rec_a = p.rec + (int64_t)b * 2 * p.log_cap;
    uint32_t *const rec_p = rec_a + p.log_cap;
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
        new_s[0] = g.start;
        new_p[0] = NONE;
        tab[g.start] = ((unsigned long long)fkey(0.f) << 32) | NONE;
    }
    __syncthreads();
    uint32_t ncur = 0;

    for (int t = -1; t < n; ++t) {
        if (t >= 0) {
#pragma unroll
            for (int k = 0; k < PRE; ++k) {
                const int c = tid + k * NT;
                if (c < C) sc[c] = -__fmul_rn(p.scale, pre[k]);
            }
            if (t + 1 < n) load_row(t + 1);
            __syncthreads();                        // scores staged; cnt_a == 0, cnt_b == 0, min_key == NONE
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
            for (uint32_t i = tid; i < nraw; i += NT) {
                const uint32_t s = raw_s[i];
                const unsigned long long k = tab[s];
                if (keyf((uint32_t)(k >> 32)) <= thr) {
                    const uint32_t pos = atomicAdd(&sh.cnt_b, 1u);      // <= nraw <= cap
                    new_s[pos] = s;
                    new_p[pos] = slot[g.src[(uint32_t)k]];              // the source survived the previous frame
                } else {
                    tab[s] = EMPTY;
                }
            }
        }
        for (int level = 0; level < g.num_ranks; ++level) {
            __syncthreads();
            // a level that outgrew the list has counted past its end: the entries beyond cap were never
            // written, so the closure stops here (uniform) and the count is never taken above cap
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
            if (tid == 0) sh.ovf = 1;
            __syncthreads();
            break;
        }
        if (tid == 0) {
            sh.min_key = NONE;
            sh.cnt_a = 0;
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
            rec_a[rec_base + i] = a;
            rec_p[rec_base + i] = prev;
            const float c = keyf((uint32_t)(k >> 32));
            if (last || c <= thr) {
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
            if (t >= 0) nact[t] = (int32_t)ncur;
        }
    }
    if (sh.ovf) {       // uniform: every way to the flag passes a barrier
        if (tid == 0) p.out_overflow[b] = 1;
        return;
    }

    // the best final state, or the best state: ties to the smallest state id
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
    if (tid != 0) return;
    const bool reached = sh.best_final != EMPTY;
    const unsigned long long best = reached ? sh.best_final : sh.best_any;
    if (best == EMPTY || (!reached && !p.allow_partial)) return;
    int32_t *const words = p.out_words + (int64_t)b * p.word_cap;
    const uint32_t total = sh.rec_used;
    uint32_t r = slot[(uint32_t)best];
    int t = n - 1, nw = 0;
    for (uint32_t step = 0; step < total && r < total; ++step) {
        const uint32_t a = rec_a[r];
        if (a == NONE) break;                       // the start token
        const int il = g.il[a], ol = g.ol[a];
        if (il > 0) {
            if (t >= 0) align[t] = il;
            --t;
        }
        if (ol != 0) {
            if (nw < p.word_cap) words[nw] = ol;    // last word first
            ++nw;
        }
        r = rec_p[r];
    }
    if (nw > p.word_cap) {
        p.out_overflow[b] = 1;
        return;
    }
    p.out_nwords[b] = nw;
    p.out_cost[b] = keyf((uint32_t)(best >> 32));
    p.out_final[b] = reached ? 1 : 0;
}

inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

struct Layout {
    int64_t tab, slot, lists, rec, total;
};

Layout layout(int64_t N, int64_t B, int64_t list_cap, int64_t log_cap) {
    Layout l;
    l.tab = 0;
    l.slot = up16(B * N * 8);
    l.lists = l.slot + up16(B * N * 4);
    l.rec = l.lists + up16(B * 5 * list_cap * 4);
    l.total = l.rec + up16(B * 2 * log_cap * 4);
    return l;
}

bool shapes_ok(int64_t N, int64_t A, int C, int T) {
    return N >= 1 && N < ((int64_t)1 << 31) && A >= 0 && A < 0xFFFFFFFFll && C >= 1 && C <= MAX_C && T >= 1;
}

bool caps_ok(int64_t list_cap, int64_t log_cap) {
    return list_cap >= 1 && list_cap < ((int64_t)1 << 31) && log_cap >= 1 && log_cap < ((int64_t)1 << 31);
}

// Threads per workgroup.  The per-arc work is a chain of dependent loads and one atomic, so waves in
// flight are what hides it.  Measured at T' = 334: with 768 utterances 512
// threads took two thirds of the time of 256 and of 1024 (three workgroups a CU: 1024 threads no longer
// fit side by side); with 16 utterances 1024 threads beat 512 by a fifth.  Up to one workgroup per CU
// (256 of them) nothing competes for the CU, hence 1024 there; sizes in between were not timed.
// `threads` != 0 is the caller's choice (tools/bench_wfst_decode.py --sweep-threads).
int pick_threads(int B, int threads) { return threads ? threads : B <= 256 ? 1024 : 512; }

}  // namespace

extern "C" int asr_wfst_decode_supported(int64_t N, int64_t A, int C, int T) { return shapes_ok(N, A, C, T) ? 1 : 0; }

extern "C" int64_t asr_wfst_decode_workspace_bytes(int64_t N, int B, int64_t list_cap, int64_t log_cap) {
    if (N < 1 || B < 1 || !caps_ok(list_cap, log_cap)) return 0;
    return layout(N, B, list_cap, log_cap).total;
}

extern "C" int asr_wfst_decode_f32(const float *lp, int64_t frame_stride, const int32_t *lens, int T, int B, int C,
                                   int64_t N, int64_t A, const uint32_t *arc_ptr, const int32_t *arc_src,
                                   const int32_t *arc_dst, const int32_t *arc_ilabel, const int32_t *arc_olabel,
                                   const float *arc_weight, const float *final_cost, const uint32_t *eps_ptr,
                                   const uint32_t *eps_arc, int64_t E, const int32_t *eps_rank, int num_ranks,
                                   int start,
                                   float beam, float acoustic_scale, int allow_partial, int64_t list_cap,
                                   int64_t log_cap, int word_cap, int threads, float *out_cost,
                                   int32_t *out_reached_final,
                                   int32_t *out_alignment, int32_t *out_num_active, int32_t *out_words,
                                   int32_t *out_num_words, int32_t *out_overflow, void *workspace,
                                   int64_t workspace_bytes, void *stream) {
    if (B < 0 || T < 0 || C < 1 || N < 1 || A < 0 || E < 0 || E > A || num_ranks < 0 || word_cap < 1) return ASR_EINVAL;
    if (threads != 0 && threads != 256 && threads != 512 && threads != 1024) return ASR_EINVAL;
    if (start < 0 || start >= N || !(beam >= 0.f) || !caps_ok(list_cap, log_cap)) return ASR_EINVAL;
    if (frame_stride < (int64_t)B * C) return ASR_EINVAL;
    if (B == 0) return ASR_OK;
    if (!shapes_ok(N, A, C, T)) return ASR_EUNSUPPORTED;
    if (!lp || !lens || !arc_ptr || !final_cost || !eps_ptr || !eps_rank || !out_cost || !out_reached_final ||
        !out_alignment || !out_num_active || !out_words || !out_num_words || !out_overflow)
        return ASR_EINVAL;
    if (A > 0 && (!arc_src || !arc_dst || !arc_ilabel || !arc_olabel || !arc_weight)) return ASR_EINVAL;
    if (E > 0 && !eps_arc) return ASR_EINVAL;
    const Layout l = layout(N, B, list_cap, log_cap);
    if (!workspace || workspace_bytes < l.total) return ASR_EINVAL;
    uint8_t *const ws = (uint8_t *)workspace;
    if (hipMemsetAsync(ws + l.tab, 0xFF, (size_t)B * N * 8, (hipStream_t)stream) != hipSuccess) return ASR_ELAUNCH;
    Params p;
    p.g = Graph{(uint32_t)N, (uint32_t)A, (uint32_t)E, arc_ptr, arc_src, arc_dst, arc_ilabel, arc_olabel, arc_weight, final_cost,
                eps_ptr, eps_arc, eps_rank, num_ranks, (uint32_t)start};
    p.lp = lp;
    p.frame_stride = frame_stride;
    p.lens = lens;
    p.T = T;
    p.B = B;
    p.C = C;
    p.beam = beam;
    p.scale = acoustic_scale;
    p.allow_partial = allow_partial;
    p.list_cap = (uint32_t)list_cap;
    p.log_cap = (uint32_t)log_cap;
    p.word_cap = word_cap;
    p.out_cost = out_cost;
    p.out_final = out_reached_final;
    p.out_align = out_alignment;
    p.out_nact = out_num_active;
    p.out_words = out_words;
    p.out_nwords = out_num_words;
    p.out_overflow = out_overflow;
    p.tab = (unsigned long long *)(ws + l.tab);
    p.slot = (uint32_t *)(ws + l.slot);
    p.lists = (uint32_t *)(ws + l.lists);
    p.rec = (uint32_t *)(ws + l.rec);
    const size_t lds = (size_t)C * sizeof(float);
    switch (pick_threads(B, threads)) {
    case 256: hipLaunchKernelGGL(wfst_decode_kernel<256>, dim3(B), dim3(256), lds, (hipStream_t)stream, p); break;
    case 512: hipLaunchKernelGGL(wfst_decode_kernel<512>, dim3(B), dim3(512), lds, (hipStream_t)stream, p); break;
    default: hipLaunchKernelGGL(wfst_decode_kernel<1024>, dim3(B), dim3(1024), lds, (hipStream_t)stream, p); break;
    }
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
