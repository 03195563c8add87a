// Lattice scans over ONE weighted sparse graph shared by the whole batch (Bg == 1), in CSR
// form: the CTC token transducer composed with a character n-gram LM (HC o G), i.e. the
// denominator of the globally normalised loss and the search graph of FSTDecoder.decode when a
// grammar FST is given (reference att_speech/fst_utils.py:633-640; arithmetic of PathLogSumExp
// :400-488 and of path_reduction's alpha scan :349-397, viterbi branch :366-370).
//
// Such a graph has 10^2 - 10^4 states whose in-degree runs from 2 to ~N (the state behind the
// LM's unigram back-off is entered from everywhere), so its padded [N,K] matrices are mostly
// padding.  Mapping: one workgroup per utterance; alpha / beta of a frame in LDS (double
// buffered, one barrier per frame); the arcs are streamed from L2 every frame as 8-byte records
// (16-bit neighbour state | 16-bit input label, f32 weight); the log-prob row of the NEXT frame
// is fetched into a register before the recurrence of this one and lands in LDS at its end; the
// per-frame gradient row is accumulated in LDS and written once, densely.
//
// Load balance: the host orders the states by degree.  The first n_light states of the order
// are each reduced by a group of `lanes` (1..64, a power of two) adjacent lanes, the remaining
// (heavy) ones by a whole wave each; partial (max, sum) pairs meet through wave shuffles.
#include <stdlib.h>

#include "common.h"
#include "../../include/asr_amd.h"

namespace {

using namespace asr;

constexpr int MAX_N = 7168;       // 2 * N floats of alpha/beta + rows stay below 64 KiB of LDS
constexpr int MAX_C = 1024;       // one log-prob per thread in the row prefetch

struct SharedParams {
    const float *lp;
    int T, B, C;
    const int32_t *lens;
    int N;
    const int32_t *in_ptr, *out_ptr;
    const uint2 *in_arc, *out_arc;      // .x = neighbour | ilabel << 16, .y = weight bits
    const float *term;
    const int32_t *order_in, *order_out;
    int n_light_in, lanes_in, n_light_out, lanes_out;
    float neg_inf, gsign;
    int accumulate;
    float *logZ, *grad, *logZ_bwd, *alphas;
    float *score;
    int32_t *best_il;
    uint16_t *bp;
};

__device__ __forceinline__ void lse_merge(Lse &a, float om, float os) {
    const float M = fmaxf(a.m, om);
    if (M == -INFINITY) return;                   // both empty: exp(-inf - -inf) must not happen
    a.s = a.s * __expf(a.m - M) + os * __expf(om - M);
    a.m = M;
}

// alpha_{t+1}[n] = logsumexp over the in-arcs of n of (alpha_t[src] + w) + lp_t[il], for the
// states order[first .. first + count), each by a group of L lanes.  Every thread of the block
// runs the same number of outer iterations, so the shuffles see whole waves.
__device__ __forceinline__ void relax_sum(const SharedParams &p, const int32_t *order, int count, int L,
                                          const int32_t *ptr, const uint2 *arc, const float *a,
                                          const float *lrow, float *an) {
    const int NT = blockDim.x, gid = threadIdx.x / L, gl = threadIdx.x % L, ngroups = NT / L;
    for (int i0 = 0; i0 < count; i0 += ngroups) {
        const int i = i0 + gid;
        const bool act = i < count;
        const int n = act ? order[i] : 0;
        const int lo = act ? ptr[n] : 0, hi = act ? ptr[n + 1] : 0;
        Lse acc;
        acc.init();
        for (int e = lo + gl; e < hi; e += L) {
            const uint2 r = arc[e];
            acc.add((a[r.x & 0xffffu] + __uint_as_float(r.y)) + lrow[r.x >> 16]);
        }
        for (int o = L >> 1; o > 0; o >>= 1) {
            const float om = __shfl_xor(acc.m, o, ASR_WAVE), os = __shfl_xor(acc.s, o, ASR_WAVE);
            lse_merge(acc, om, os);
        }
        // a state nothing enters stays at the sentinel (the padded form has a padding arc there)
        if (act && gl == 0) an[n] = acc.m == -INFINITY ? p.neg_inf : acc.value();
    }
}

// max-plus form; slot = position of the first maximum among the in-arcs of n
__device__ __forceinline__ void relax_max(const SharedParams &p, const int32_t *order, int count, int L,
                                          const int32_t *ptr, const uint2 *arc, const float *a,
                                          const float *lrow, float *an, uint16_t *bp_row) {
    const int NT = blockDim.x, gid = threadIdx.x / L, gl = threadIdx.x % L, ngroups = NT / L;
    for (int i0 = 0; i0 < count; i0 += ngroups) {
        const int i = i0 + gid;
        const bool act = i < count;
        const int n = act ? order[i] : 0;
        const int lo = act ? ptr[n] : 0, hi = act ? ptr[n + 1] : 0;
        float best = -INFINITY;
        int arg = 0x7fffffff;
        for (int e = lo + gl; e < hi; e += L) {
            const uint2 r = arc[e];
            // same association as the reference: (alpha + w) + lp (:387-390)
            const float v = (a[r.x & 0xffffu] + __uint_as_float(r.y)) + lrow[r.x >> 16];
            if (v > best) { best = v; arg = e - lo; }
        }
        for (int o = L >> 1; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, ASR_WAVE);
            const int oa = __shfl_xor(arg, o, ASR_WAVE);
            if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
        }
        if (act && gl == 0) {
            an[n] = hi > lo ? best : p.neg_inf;
            if (bp_row) bp_row[n] = (uint16_t)(hi > lo ? arg : 0);
        }
    }
}

// beta_t[n] = logsumexp over the out-arcs of n of w + beta_{t+1}[dst] + lp_t[il]; every arc
// token times alpha_t[n] / Z is that arc's occupancy, added to the frame's gradient row
__device__ __forceinline__ void relax_back(const SharedParams &p, const int32_t *order, int count, int L,
                                           const int32_t *ptr, const uint2 *arc, const float *bt,
                                           const float *lrow, const float *arow, float logZ,
                                           float *bn, float *grow) {
    const int NT = blockDim.x, gid = threadIdx.x / L, gl = threadIdx.x % L, ngroups = NT / L;
    for (int i0 = 0; i0 < count; i0 += ngroups) {
        const int i = i0 + gid;
        const bool act = i < count;
        const int n = act ? order[i] : 0;
        const int lo = act ? ptr[n] : 0, hi = act ? ptr[n + 1] : 0;
        const float an = act ? arow[n] - logZ : 0.f;
        Lse acc;
        acc.init();
        for (int e = lo + gl; e < hi; e += L) {
            const uint2 r = arc[e];
            const int il = r.x >> 16;
            const float v = __uint_as_float(r.y) + bt[r.x & 0xffffu] + lrow[il];
            acc.add(v);
            const float o = __expf(v + an) * p.gsign;
            if (o != 0.f) atomicAdd(&grow[il], o);
        }
        for (int o = L >> 1; o > 0; o >>= 1) {
            const float om = __shfl_xor(acc.m, o, ASR_WAVE), os = __shfl_xor(acc.s, o, ASR_WAVE);
            lse_merge(acc, om, os);
        }
        if (act && gl == 0) bn[n] = acc.m == -INFINITY ? p.neg_inf : acc.value();
    }
}

__device__ __forceinline__ float block_lse_term(const float *a, const float *term, int N, float *red) {
    const int tid = threadIdx.x, NT = blockDim.x;
    float m = -INFINITY;
    for (int n = tid; n < N; n += NT) m = fmaxf(m, a[n] + term[n]);
    m = block_max(m, red);
    float s = 0.f;
    for (int n = tid; n < N; n += NT) s += __expf(a[n] + term[n] - m);
    s = block_sum(s, red);
    return m + __logf(s);
}

__global__ void __launch_bounds__(1024) shared_fwbw_kernel(SharedParams p) {
    extern __shared__ float smem[];
    const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
    const int N = p.N, C = p.C;
    const int Npad = (N + 3) & ~3, Cpad = (C + 3) & ~3;
    float *abuf = smem;                     // [2][Npad] alpha, then beta
    float *lbuf = abuf + 2 * Npad;          // [2][Cpad] log-prob row of this frame / the next
    float *gbuf = lbuf + 2 * Cpad;          // [2][Cpad] gradient row being summed / being written
    float *red = gbuf + 2 * Cpad;           // [64]

    int len = p.lens[b];
    len = len < 0 ? 0 : (len > p.T ? p.T : len);
    const size_t tstride = (size_t)p.B * C;
    const float *lp_b = p.lp + (size_t)b * C;
    float *grad_b = p.grad + (size_t)b * C;
    float *alphas_b = p.alphas + (size_t)b * N;
    const size_t astride = (size_t)p.B * N;
    const int n_heavy_in = N - p.n_light_in, n_heavy_out = N - p.n_light_out;

    // rows past the utterance end are zeros (fst_utils.py:448); left alone when accumulating
    if (!p.accumulate)
        for (int t = len; t < p.T; ++t)
            for (int c = tid; c < C; c += NT) grad_b[(size_t)t * tstride + c] = 0.f;

    for (int n = tid; n < Npad; n += NT) abuf[n] = (n == 0) ? 0.f : p.neg_inf;
    for (int c = tid; c < 2 * Cpad; c += NT) gbuf[c] = 0.f;
    if (len > 0 && tid < C) lbuf[tid] = lp_b[tid];
    __syncthreads();

    // ---------------- forward ----------------
    int cur = 0;
    for (int t = 0; t < len; ++t) {
        const float *a = abuf + cur * Npad;
        float *an = abuf + (cur ^ 1) * Npad;
        const float *lrow = lbuf + cur * Cpad;
        float nxt = 0.f;
        if (t + 1 < len && tid < C) nxt = lp_b[(size_t)(t + 1) * tstride + tid];
        float *arow = alphas_b + (size_t)t * astride;
        for (int n = tid; n < N; n += NT) arow[n] = a[n];            // alphas[t] = pre-update (:437)
        relax_sum(p, p.order_in, p.n_light_in, p.lanes_in, p.in_ptr, p.in_arc, a, lrow, an);
        relax_sum(p, p.order_in + p.n_light_in, n_heavy_in, ASR_WAVE, p.in_ptr, p.in_arc, a, lrow, an);
        if (tid < C) lbuf[(cur ^ 1) * Cpad + tid] = nxt;
        cur ^= 1;
        __syncthreads();
    }

    // logZ = logsumexp_n(alpha + terminal)   (fst_utils.py:445)
    const float logZ = block_lse_term(abuf + cur * Npad, p.term, N, red);
    if (tid == 0) p.logZ[b] = logZ;
    __syncthreads();

    // ---------------- backward ----------------
    for (int n = tid; n < N; n += NT) abuf[n] = p.term[n];          // beta = terminal (:447)
    if (len > 0 && tid < C) lbuf[tid] = lp_b[(size_t)(len - 1) * tstride + tid];
    cur = 0;
    __syncthreads();

    int rcur = 0;
    for (int t = len - 1; t >= 0; --t) {
        const float *bt = abuf + cur * Npad;
        float *bn = abuf + (cur ^ 1) * Npad;
        const float *lrow = lbuf + cur * Cpad;
        float *rw = gbuf + rcur * Cpad;
        float *rprev = gbuf + (rcur ^ 1) * Cpad;
        float nxt = 0.f;
        if (t > 0 && tid < C) nxt = lp_b[(size_t)(t - 1) * tstride + tid];
        // write the row finished in the previous step (frame t+1), re-zero it
        if (t + 1 < len) {
            float *gout = grad_b + (size_t)(t + 1) * tstride;
            for (int c = tid; c < C; c += NT) {
                gout[c] = p.accumulate ? gout[c] + rprev[c] : rprev[c];
                rprev[c] = 0.f;
            }
        }
        const float *arow = alphas_b + (size_t)t * astride;
        relax_back(p, p.order_out, p.n_light_out, p.lanes_out, p.out_ptr, p.out_arc, bt, lrow, arow,
                   logZ, bn, rw);
        relax_back(p, p.order_out + p.n_light_out, n_heavy_out, ASR_WAVE, p.out_ptr, p.out_arc, bt, lrow,
                   arow, logZ, bn, rw);
        if (tid < C) lbuf[(cur ^ 1) * Cpad + tid] = nxt;
        cur ^= 1;
        rcur ^= 1;
        __syncthreads();
    }
    if (len > 0) {
        const float *rprev = gbuf + (rcur ^ 1) * Cpad;
        for (int c = tid; c < C; c += NT) grad_b[c] = p.accumulate ? grad_b[c] + rprev[c] : rprev[c];
    }
    // fst_utils.py:476: logsumexp(alpha_0 + beta_0), alpha_0 = 0 at the start state and the
    // sentinel elsewhere
    if (p.logZ_bwd) {
        const float *bt = abuf + cur * Npad;
        float m = -INFINITY;
        for (int n = tid; n < N; n += NT) m = fmaxf(m, bt[n] + (n == 0 ? 0.f : p.neg_inf));
        m = block_max(m, red);
        float s = 0.f;
        for (int n = tid; n < N; n += NT) s += __expf(bt[n] + (n == 0 ? 0.f : p.neg_inf) - m);
        s = block_sum(s, red);
        if (tid == 0) p.logZ_bwd[b] = m + __logf(s);
    }
}

template <bool VITERBI>
__global__ void __launch_bounds__(1024) shared_forward_kernel(SharedParams p) {
    extern __shared__ float smem[];
    const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
    const int N = p.N, C = p.C;
    const int Npad = (N + 3) & ~3, Cpad = (C + 3) & ~3;
    float *abuf = smem;                     // [2][Npad]
    float *lbuf = abuf + 2 * Npad;          // [2][Cpad]
    float *red = lbuf + 2 * Cpad;           // [64]
    int *redi = (int *)(red + 32);

    int len = p.lens[b];
    len = len < 0 ? 0 : (len > p.T ? p.T : len);
    const size_t tstride = (size_t)p.B * C;
    const float *lp_b = p.lp + (size_t)b * C;
    const bool want_path = VITERBI && p.best_il != nullptr;
    uint16_t *bp_b = want_path ? p.bp + (size_t)b * N : nullptr;
    const size_t bstride = (size_t)p.B * N;
    const int n_heavy_in = N - p.n_light_in;

    for (int n = tid; n < Npad; n += NT) abuf[n] = (n == 0) ? 0.f : p.neg_inf;
    if (want_path)
        for (int t = len + tid; t < p.T; t += NT) p.best_il[(size_t)t * p.B + b] = 0;
    if (len > 0 && tid < C) lbuf[tid] = lp_b[tid];
    __syncthreads();

    int cur = 0;
    for (int t = 0; t < len; ++t) {
        const float *a = abuf + cur * Npad;
        float *an = abuf + (cur ^ 1) * Npad;
        const float *lrow = lbuf + cur * Cpad;
        float nxt = 0.f;
        if (t + 1 < len && tid < C) nxt = lp_b[(size_t)(t + 1) * tstride + tid];
        if (VITERBI) {
            uint16_t *bp_row = want_path ? bp_b + (size_t)t * bstride : nullptr;
            relax_max(p, p.order_in, p.n_light_in, p.lanes_in, p.in_ptr, p.in_arc, a, lrow, an, bp_row);
            relax_max(p, p.order_in + p.n_light_in, n_heavy_in, ASR_WAVE, p.in_ptr, p.in_arc, a, lrow, an,
                      bp_row);
        } else {
            relax_sum(p, p.order_in, p.n_light_in, p.lanes_in, p.in_ptr, p.in_arc, a, lrow, an);
            relax_sum(p, p.order_in + p.n_light_in, n_heavy_in, ASR_WAVE, p.in_ptr, p.in_arc, a, lrow, an);
        }
        if (tid < C) lbuf[(cur ^ 1) * Cpad + tid] = nxt;
        cur ^= 1;
        __syncthreads();
    }

    const float *a = abuf + cur * Npad;
    if (VITERBI) {
        // first maximum over n of alpha + terminal (:396)
        float best = -INFINITY;
        int arg = 0x7fffffff;
        for (int n = tid; n < N; n += NT) {
            const float v = a[n] + p.term[n];
            if (v > best) { best = v; arg = n; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, ASR_WAVE);
            const int oa = __shfl_xor(arg, o, ASR_WAVE);
            if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
        }
        const int lane = tid & 63, w = tid >> 6, nw = (NT + 63) >> 6;
        if (lane == 0) { red[w] = best; redi[w] = arg; }
        __syncthreads();
        if (tid == 0) {
            for (int i = 1; i < nw; ++i)
                if (red[i] > best || (red[i] == best && redi[i] < arg)) {
                    best = red[i];
                    arg = redi[i];
                }
            p.score[b] = best;
            if (want_path) {
                int st = arg < N ? arg : 0;
                for (int t = len - 1; t >= 0; --t) {
                    const int lo = p.in_ptr[st], deg = p.in_ptr[st + 1] - lo;
                    int k = bp_b[(size_t)t * bstride + st];
                    if (deg <= 0) {                               // nothing enters: no arc to report
                        p.best_il[(size_t)t * p.B + b] = 0;
                        continue;
                    }
                    k = k < deg ? k : deg - 1;
                    const uint2 r = p.in_arc[lo + k];
                    p.best_il[(size_t)t * p.B + b] = (int32_t)(r.x >> 16);
                    st = (int)(r.x & 0xffffu);
                }
            }
        }
    } else {
        const float z = block_lse_term(a, p.term, N, red);
        if (tid == 0) p.score[b] = z;
    }
}

inline int round_up64(int v) { return (v + 63) / 64 * 64; }

inline bool pow2_lanes(int l) { return l >= 1 && l <= 64 && (l & (l - 1)) == 0; }

inline int block_threads(int N, int E, int C) {
    // small graphs: a narrow workgroup (more utterances per CU); from a few thousand arcs on
    // the frame time is the arc stream and the widest workgroup wins
    int nt = E > 4096 ? 1024 : round_up64(N < 256 ? 256 : N);
    if (nt > 1024) nt = 1024;
    if (nt < round_up64(C)) nt = round_up64(C);
    return nt;
}

}  // namespace

extern "C" int asr_lattice_shared_supported(int N, int E, int C) {
    return N >= 1 && N <= MAX_N && E >= 1 && C >= 1 && C <= MAX_C;
}

extern "C" int64_t asr_lattice_shared_workspace_bytes(int T, int B, int N) {
    if (T < 0 || B < 0 || N < 0) return -1;
    // fwbw: alphas f32 [T,B,N]; viterbi: arg-max arc slots u16 [T,B,N]
    return (int64_t)T * B * N * (int64_t)sizeof(float) + 256;
}

extern "C" int asr_lattice_shared_fwbw_f32(
    const float *lp, int T, int B, int C, const int32_t *lens, int N, int E,
    const int32_t *in_ptr, const uint32_t *in_arc, const int32_t *out_ptr, const uint32_t *out_arc,
    const float *term, const int32_t *order_in, int n_light_in, int lanes_in,
    const int32_t *order_out, int n_light_out, int lanes_out, float neg_inf, float grad_sign,
    int accumulate, float *out_logZ, float *out_grad, float *out_logZ_bwd, void *workspace,
    int64_t workspace_bytes, void *stream) {
    if (T < 0 || B < 0 || C <= 0 || N <= 0 || E <= 0) return ASR_EINVAL;
    if (!(grad_sign == 1.f || grad_sign == -1.f) || !(neg_inf < 0.f)) return ASR_EINVAL;
    if (!pow2_lanes(lanes_in) || !pow2_lanes(lanes_out)) return ASR_EINVAL;
    if (n_light_in < 0 || n_light_in > N || n_light_out < 0 || n_light_out > N) return ASR_EINVAL;
    if (!asr_lattice_shared_supported(N, E, C)) return ASR_EUNSUPPORTED;
    if (B == 0) return ASR_OK;
    if (!lens || !in_ptr || !in_arc || !out_ptr || !out_arc || !term || !order_in || !order_out ||
        !out_logZ || (T > 0 && (!lp || !out_grad)))
        return ASR_EINVAL;
    if (!workspace || workspace_bytes < asr_lattice_shared_workspace_bytes(T, B, N)) return ASR_EINVAL;
    SharedParams p = {};
    p.lp = lp; p.T = T; p.B = B; p.C = C; p.lens = lens; p.N = N;
    p.in_ptr = in_ptr; p.out_ptr = out_ptr;
    p.in_arc = (const uint2 *)in_arc; p.out_arc = (const uint2 *)out_arc;
    p.term = term; p.order_in = order_in; p.order_out = order_out;
    p.n_light_in = n_light_in; p.lanes_in = lanes_in;
    p.n_light_out = n_light_out; p.lanes_out = lanes_out;
    p.neg_inf = neg_inf; p.gsign = grad_sign; p.accumulate = accumulate ? 1 : 0;
    p.logZ = out_logZ; p.grad = out_grad; p.logZ_bwd = out_logZ_bwd;
    p.alphas = (float *)workspace;
    const int Npad = (N + 3) & ~3, Cpad = (C + 3) & ~3;
    const size_t lds = (size_t)(2 * Npad + 4 * Cpad + 64) * sizeof(float);
    if (lds > 160 * 1024) return ASR_EUNSUPPORTED;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void *)shared_fwbw_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        return ASR_EUNSUPPORTED;
    hipLaunchKernelGGL(shared_fwbw_kernel, dim3(B), dim3(block_threads(N, E, C)), lds, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}

extern "C" int asr_lattice_shared_forward_f32(
    const float *lp, int T, int B, int C, const int32_t *lens, int N, int E,
    const int32_t *in_ptr, const uint32_t *in_arc, const float *term, const int32_t *order_in,
    int n_light_in, int lanes_in, float neg_inf, int viterbi, float *out_score,
    int32_t *out_best_il, void *workspace, int64_t workspace_bytes, void *stream) {
    if (T < 0 || B < 0 || C <= 0 || N <= 0 || E <= 0 || !(neg_inf < 0.f)) return ASR_EINVAL;
    if (!pow2_lanes(lanes_in) || n_light_in < 0 || n_light_in > N) return ASR_EINVAL;
    if (!asr_lattice_shared_supported(N, E, C)) return ASR_EUNSUPPORTED;
    if (B == 0) return ASR_OK;
    if (!lens || !in_ptr || !in_arc || !term || !order_in || !out_score || (T > 0 && !lp))
        return ASR_EINVAL;
    const bool want_path = viterbi && out_best_il;
    if (want_path && T > 0 &&
        (!workspace || workspace_bytes < asr_lattice_shared_workspace_bytes(T, B, N)))
        return ASR_EINVAL;
    SharedParams p = {};
    p.lp = lp; p.T = T; p.B = B; p.C = C; p.lens = lens; p.N = N;
    p.in_ptr = in_ptr; p.in_arc = (const uint2 *)in_arc; p.term = term;
    p.order_in = order_in; p.n_light_in = n_light_in; p.lanes_in = lanes_in;
    p.neg_inf = neg_inf;
    p.score = out_score;
    p.best_il = want_path ? out_best_il : nullptr;
    p.bp = (uint16_t *)workspace;
    const int Npad = (N + 3) & ~3, Cpad = (C + 3) & ~3;
    const size_t lds = (size_t)(2 * Npad + 2 * Cpad + 64) * sizeof(float);
    if (lds > 160 * 1024) return ASR_EUNSUPPORTED;
    void (*kern)(SharedParams) = viterbi ? shared_forward_kernel<true> : shared_forward_kernel<false>;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess)
        return ASR_EUNSUPPORTED;
    hipLaunchKernelGGL(kern, dim3(B), dim3(block_threads(N, E, C)), lds, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
