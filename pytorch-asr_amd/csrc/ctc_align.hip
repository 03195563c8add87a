// CTC forced alignment: batched Viterbi with traceback (include/asr_amd.h: asr_ctc_align_f64,
// asr_ctc_align_supported, asr_ctc_align_workspace_bytes).
//
// The reference aligns one utterance at a time on the host (att_speech/modules/ctc_losses.py:
// raw_generic_viterbi :412-457 under mono_CTC_viterbi_align :475-481 and bi_CTC_viterbi_align
// :505-511): a dense [N, N] log-transition matrix added to the alpha column every frame and an
// argmax over the source axis.  The lattices it feeds in (get_CTC_matrices_mono :67-94,
// get_CTC_matrices_bicontext :111-166) are bands of N = 2 L + 1 states in which state n is entered
// only from {n - 2, n - 1, n}, so here one workgroup owns one utterance, derives every state's
// class and its self-loop / skip flags from the labels, and keeps the alpha column in registers:
// four consecutive states per lane, as fp64, because the reference's accumulator is a float64
// array and every step is ONE IEEE addition of a float32 log-prob.  Doing the same additions and
// comparing the three candidates in ascending source order with a strict `>` (np.argmax takes
// the first maximum) makes the cost, the path and every tie bit-identical to the reference.
//
// Single wave (N <= 256): the two upper states of the lane below arrive by cross-lane moves; the
// recurrence has no barrier and no LDS traffic except the back-pointer byte.  Multi wave
// (N <= 1023, 256 threads): the same two values cross through a double-buffered LDS exchange, one
// barrier per frame.  The emission gather lp[t, b, class(n)] does not depend on the recurrence
// and is issued PF frames ahead (lanes read scattered words of a row; rows are never staged).  The
// frame loop runs whole groups of PF frames without a branch, then a tail: a length test inside the
// unrolled body made the compiler wait for every outstanding load each frame.
//
// Back-pointers: two bits per state (0 self, 1 n - 1, 2 n - 2), i.e. one byte per lane and
// frame, in LDS when T * stride fits BP_LDS_BYTES and in the caller's workspace otherwise.  One
// thread walks them once after the last frame; frames, segments and padding are then written by
// the whole workgroup from the state path.  Latency-bound: about T dependent steps per utterance.
#include "common.h"
#include "../../include/asr_amd.h"

namespace {

constexpr int SPL = 4;                          // states per lane
constexpr int MAX_L = 511;                      // N = 2 L + 1 <= 1023
constexpr int SINGLE_N = SPL * ASR_WAVE;        // 256 states in one wave
constexpr int MULTI_THREADS = 256;
constexpr int BP_LDS_BYTES = 48 * 1024;         // with the tables below the launch stays under 64 KiB
constexpr int PF = 16;                          // frames of emissions in flight

// bytes of back-pointers per frame: one per lane that owns a state, padded to a multiple of four
inline int bp_stride(int Lmax) { return (((2 * Lmax + 1 + SPL - 1) / SPL) + 3) & ~3; }

struct Topo {
    int cls;
    bool self, prev, skip;      // entered from n, n - 1, n - 2
};

__device__ __forceinline__ Topo state_topo(const int32_t *__restrict__ lab, int N, int n, int S, int order,
                                           bool loops, bool eval_rep) {
    Topo r = {0, false, false, false};
    if (n >= N) return r;
    const int i = n >> 1;       // odd n: its label; even n: the label this blank precedes (L for the last)
    const bool odd = n & 1;
    r.prev = n >= 1;
    if (order == 1) {
        r.self = true;
        if (odd) {
            r.cls = lab[i];
            r.skip = i >= 1 && lab[i] != lab[i - 1];
        }
        return r;
    }
    const int ctx = i >= 1 ? lab[i - 1] % S : 0;
    if (!odd) {
        r.cls = ctx * S;
        r.self = true;
        return r;
    }
    const int l = lab[i] % S;
    r.cls = ctx * S + l;
    r.self = loops;
    if (i >= 1) {
        const int pctx = i >= 2 ? lab[i - 2] % S : 0;
        const bool rep = eval_rep ? (pctx * S + ctx == ctx * S + l) : (ctx == l);
        r.skip = !rep;
    }
    return r;
}

// best of the three candidates in ascending source order, first maximum wins
__device__ __forceinline__ double pick(double c2, bool f2, double c1, bool f1, double c0, bool f0, float em,
                                       uint32_t &code) {
    double best = -INFINITY;
    code = 0;
    if (f2 && c2 > best) { best = c2; code = 2; }
    if (f1 && c1 > best) { best = c1; code = 1; }
    if (f0 && c0 > best) { best = c0; code = 0; }
    return best + (double)em;
}

template <bool MULTI, bool BP_LDS>
__global__ __launch_bounds__(MULTI ? MULTI_THREADS : ASR_WAVE) void ctc_align_kernel(
        const float *__restrict__ lp, const int32_t *__restrict__ lens, const int32_t *__restrict__ labels,
        const int32_t *__restrict__ label_lens, int B, int T, int C, int Lmax, int S, int order, int loops,
        int eval_rep, int stride, double *__restrict__ out_cost, int32_t *__restrict__ out_frames,
        int32_t *__restrict__ out_states, int32_t *__restrict__ out_segments, uint8_t *__restrict__ ws) {
    constexpr int NT = MULTI ? MULTI_THREADS : ASR_WAVE;
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int feasible_s;
    int32_t *const cls_s = (int32_t *)smem;                 // [NT * SPL] class of every state
    double *const fin = (double *)(cls_s + NT * SPL);       // [2] alpha of states N - 2, N - 1
    double *const xch = fin + 2;                            // MULTI: [2][NT][2] upper two states of every lane
    uint8_t *const bp_lds = (uint8_t *)(xch + (MULTI ? 4 * NT : 0));

    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tb = lens[b], Lb = label_lens[b];
    const int32_t *const lab = labels + (int64_t)b * Lmax;
    int32_t *const frames = out_frames + (int64_t)b * T;
    int32_t *const states = out_states + (int64_t)b * T;
    int32_t *const seg = out_segments + (int64_t)b * Lmax * 2;

    bool ok = Tb >= 1 && Tb <= T && Lb >= 1 && Lb <= Lmax;      // uniform over the workgroup
    if (ok) {
        int bad = 0;
        for (int i = tid; i < Lb; i += NT) {
            const int v = lab[i];
            bad |= v < 0 || (order == 1 && v >= C);
        }
        ok = !__syncthreads_or(bad);
    }
    if (ok) {
        const int N = 2 * Lb + 1, n0 = tid * SPL;
        Topo tp[SPL];
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            tp[j] = state_topo(lab, N, n0 + j, S, order, loops != 0, eval_rep != 0);
            cls_s[n0 + j] = tp[j].cls;
        }
        // two pointers, not one generic one: a flat store would tie the emission loads' wait counter to it
        uint8_t *const bp_glb = BP_LDS ? nullptr : ws + (int64_t)b * T * stride;
        const int64_t frame = (int64_t)B * C;
        const float *const col = lp + (int64_t)b * C;

        double a[SPL];
#pragma unroll
        for (int j = 0; j < SPL; ++j) a[j] = n0 + j < 2 ? (double)col[tp[j].cls] : -INFINITY;
        float e[PF][SPL];
#pragma unroll
        for (int d = 0; d < PF; ++d) {
            const float *const row = col + frame * min(1 + d, Tb - 1);
#pragma unroll
            for (int j = 0; j < SPL; ++j) e[d][j] = row[tp[j].cls];
        }

        // one frame: e4 are the emissions of frame t for this lane's four states
        auto step = [&](int t, const float (&e4)[SPL]) {
            double p2, p3;                                      // states n0 - 2, n0 - 1
            if (MULTI) {
                double *const x = xch + (size_t)(t & 1) * NT * 2;
                x[tid * 2] = a[2];
                x[tid * 2 + 1] = a[3];
                __syncthreads();
                p2 = tid > 0 ? x[tid * 2 - 2] : -INFINITY;
                p3 = tid > 0 ? x[tid * 2 - 1] : -INFINITY;
            } else {
                p2 = __shfl_up(a[2], 1, ASR_WAVE);
                p3 = __shfl_up(a[3], 1, ASR_WAVE);
                if (tid == 0) p2 = p3 = -INFINITY;
            }
            uint32_t c0, c1, c2, c3;
            const double n0v = pick(p2, tp[0].skip, p3, tp[0].prev, a[0], tp[0].self, e4[0], c0);
            const double n1v = pick(p3, tp[1].skip, a[0], tp[1].prev, a[1], tp[1].self, e4[1], c1);
            const double n2v = pick(a[0], tp[2].skip, a[1], tp[2].prev, a[2], tp[2].self, e4[2], c2);
            const double n3v = pick(a[1], tp[3].skip, a[2], tp[3].prev, a[3], tp[3].self, e4[3], c3);
            a[0] = n0v; a[1] = n1v; a[2] = n2v; a[3] = n3v;
            const uint8_t code = (uint8_t)(c0 | (c1 << 2) | (c2 << 4) | (c3 << 6));
            if (tid < stride) {
                if (BP_LDS) bp_lds[t * stride + tid] = code;
                else bp_glb[(int64_t)t * stride + tid] = code;
            }
        };
        // whole groups of PF frames, no branch in the body: e[d] holds frame t0 + d and is refilled
        // for frame t0 + d + PF as soon as it has been read
        int t0 = 1;
        for (; t0 + PF <= Tb; t0 += PF) {
#pragma unroll
            for (int d = 0; d < PF; ++d) {
                float e4[SPL];
                const float *const row = col + frame * min(t0 + d + PF, Tb - 1);
#pragma unroll
                for (int j = 0; j < SPL; ++j) {
                    e4[j] = e[d][j];
                    e[d][j] = row[tp[j].cls];
                }
                step(t0 + d, e4);
            }
        }
#pragma unroll
        for (int d = 0; d < PF - 1; ++d)                        // the last Tb - t0 < PF frames are loaded already
            if (t0 + d < Tb) step(t0 + d, e[d]);                // uniform
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            if (n0 + j == N - 2) fin[0] = a[j];
            if (n0 + j == N - 1) fin[1] = a[j];
        }
        __syncthreads();
        if (tid == 0) {
            const double f0 = fin[0], f1 = fin[1];
            int st = f1 > f0 ? N - 1 : N - 2;                   // N - 2 wins ties
            const double best = f1 > f0 ? f1 : f0;
            const int feasible = best > -INFINITY;              // false for NaN as well
            feasible_s = feasible;
            if (feasible) {
                out_cost[b] = -best;
                for (int t = Tb - 1; t >= 0; --t) {
                    states[t] = st;
                    if (t > 0) {
                        const uint32_t byte = BP_LDS ? bp_lds[t * stride + (st >> 2)]
                                                        : bp_glb[(int64_t)t * stride + (st >> 2)];
                        st = max(st - (int)((byte >> (2 * (st & 3))) & 3u), 0);
                    }
                }
            }
        }
        __syncthreads();
        ok = feasible_s != 0;
    }
    if (!ok) {      // no alignment: cost = +inf and -1 everywhere
        if (tid == 0) out_cost[b] = INFINITY;
        for (int t = tid; t < T; t += NT) frames[t] = states[t] = -1;
        for (int i = tid; i < 2 * Lmax; i += NT) seg[i] = -1;
        return;
    }
    for (int t = tid; t < T; t += NT) {
        if (t >= Tb) {
            frames[t] = -1;
            continue;
        }
        const int s = states[t];
        frames[t] = cls_s[s];
        if (s & 1) {    // a frame starts a segment when its state differs from the previous frame's
            if ((t > 0 ? states[t - 1] : -1) != s) seg[s - 1] = t;          // 2 * (s >> 1)
            if ((t + 1 < Tb ? states[t + 1] : -1) != s) seg[s] = t + 1;     // 2 * (s >> 1) + 1
        }
    }
    __syncthreads();    // the state path is read above by other threads than the one padding it below
    for (int t = Tb + tid; t < T; t += NT) states[t] = -1;
    for (int i = 2 * Lb + tid; i < 2 * Lmax; i += NT) seg[i] = -1;
}

bool shapes_ok(int T, int Lmax, int C) { return T >= 1 && Lmax >= 1 && Lmax <= MAX_L && C >= 1; }

}  // namespace

extern "C" int asr_ctc_align_supported(int T, int Lmax, int C) { return shapes_ok(T, Lmax, C) ? 1 : 0; }

extern "C" int64_t asr_ctc_align_workspace_bytes(int T, int B, int Lmax) {
    if (T < 1 || B < 1 || Lmax < 1 || Lmax > MAX_L) return 0;
    const int64_t per_utt = (int64_t)T * bp_stride(Lmax);
    return per_utt <= BP_LDS_BYTES ? 0 : per_utt * B;
}

extern "C" int asr_ctc_align_f64(const float *lp, const int32_t *lens, const int32_t *labels,
                                 const int32_t *label_lens, int B, int T, int C, int Lmax, int S,
                                 int context_order, int allow_nonblank_selfloops, int eval_repeats_in_context,
                                 double *out_cost, int32_t *out_frames, int32_t *out_states,
                                 int32_t *out_segments, void *workspace, int64_t workspace_bytes, void *stream) {
    if (B < 0 || T < 0 || C < 1 || Lmax < 0) return ASR_EINVAL;
    if (context_order != 1 && context_order != 2) return ASR_EINVAL;
    if (context_order == 2 && (S < 1 || (int64_t)S * S > C)) return ASR_EINVAL;
    if (B == 0) return ASR_OK;
    if (!shapes_ok(T, Lmax, C)) return ASR_EUNSUPPORTED;
    if (!lp || !lens || !labels || !label_lens || !out_cost || !out_frames || !out_states || !out_segments)
        return ASR_EINVAL;
    const int64_t need = asr_ctc_align_workspace_bytes(T, B, Lmax);
    if (need > 0 && (!workspace || workspace_bytes < need)) return ASR_EINVAL;
    const int stride = bp_stride(Lmax);
    const bool in_lds = need == 0;
    const bool multi = 2 * Lmax + 1 > SINGLE_N;
    const int nt = multi ? MULTI_THREADS : ASR_WAVE;
    const size_t lds = (size_t)nt * SPL * sizeof(int32_t) + 2 * sizeof(double) +
                       (multi ? (size_t)4 * nt * sizeof(double) : 0) + (in_lds ? (size_t)T * stride : 0);
    auto kernel = multi ? (in_lds ? ctc_align_kernel<true, true> : ctc_align_kernel<true, false>)
                        : (in_lds ? ctc_align_kernel<false, true> : ctc_align_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(B), dim3(nt), lds, (hipStream_t)stream, lp, lens, labels, label_lens, B, T, C,
                       Lmax, S, context_order, allow_nonblank_selfloops, eval_repeats_in_context, stride, out_cost,
                       out_frames, out_states, out_segments, (uint8_t *)workspace);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
