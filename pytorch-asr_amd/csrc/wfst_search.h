// Device code shared by the searches over one decoding graph: wfst_decode.hip (the best path) and
// wfst_lattice.hip (the lattice).  Costs are fp32, every step one rounding (both files are built
// with -ffp-contract=off); a token is ONE 64-bit word per state, (order-preserving bits of the
// cost) << 32 | arc index, so a minimum over that word takes the cheapest proposal and among equal
// ones the smallest arc index.
#pragma once
#include "common.h"

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

inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

inline bool shapes_ok(int64_t N, int64_t A, int C, int T) {
    return N >= 1 && N < ((int64_t)1 << 31) && A >= 0 && A < 0xFFFFFFFFll && C >= 1 && C <= MAX_C && T >= 1;
}

// Threads per workgroup.  The per-arc work is a chain of dependent loads and one atomic, so waves in
// flight are what hides it.  Measured at T' = 334: with 768 utterances 512
// threads took two thirds of the time of 256 and of 1024 (three workgroups a CU: 1024 threads no longer
// fit side by side); with 16 utterances 1024 threads beat 512 by a fifth.  Up to one workgroup per CU
// (256 of them) nothing competes for the CU, hence 1024 there; sizes in between were not timed.
// `threads` != 0 is the caller's choice (tools/bench_wfst_decode.py --sweep-threads).
inline int pick_threads(int B, int threads) { return threads ? threads : B <= 256 ? 1024 : 512; }

}  // namespace
