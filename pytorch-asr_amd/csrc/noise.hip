// Counter-based Gaussian noise over a segment table (include/asr_amd.h: asr_gaussian_noise_f32,
// asr_noise_chunk_elems) and the non-finite loss flag (asr_nonfinite_flag_f32).
//
// The reference's weight-noise hooks (att_speech/modules/hooks/weight_noise.py:63-99) draw
// `randn_like(weight)` per parameter, add it before the forward pass and subtract the stored
// tensor after backward; ConstantGradientNoise (gradient_noise.py:10-16) adds `randn_like(grad)`
// times its sigma.  Here one launch covers every noised piece: z[i] is a function of (seed, tag,
// iteration, global index i) only — Philox4x32-10 with key = seed and counter =
// (i >> 2, tag, iteration lo, iteration hi), the four output words giving two Box-Muller pairs —
// so the removal pass regenerates exactly the noise it adds, nothing is stored in between, and
// every rank of a data-parallel run draws the same noise.
//
// apply: p += sign * (sigma * z), the product rounded once and the sum rounded once (no FMA
// contraction), so (w + r) - r is the reference's `add_(rand); add_(-rand)` in fp32.
// write: p = z (the tests' view of the draw).
// HBM-bound: 8 bytes per element per pass; a group of four elements is one 16-byte access where
// the piece is aligned for it.
#include "common.h"
#include "noise_draw.h"
#include "../../include/asr_amd.h"

namespace {

constexpr int TPB = 256;
constexpr int CHUNK = 4096;             // elements per table entry: <= 1025 groups of 4, four per thread

using asr::U4;
using asr::philox4x32_10;
using asr::box_muller;

struct NoiseParams {
    const AsrNoiseSegment *segs;
    int nsegs;
    uint32_t k0, k1, tag, it_lo, it_hi;
    int mode;
    float sign;
};

__device__ __forceinline__ float apply_one(float p, float sigma, float z, float sign) {
    const float r = __fmul_rn(sigma, z);
    return sign > 0.f ? __fadd_rn(p, r) : __fadd_rn(p, -r);
}

__global__ __launch_bounds__(TPB) void noise_kernel(NoiseParams p) {
    for (int si = blockIdx.x; si < p.nsegs; si += gridDim.x) {
        const AsrNoiseSegment sg = p.segs[si];
        if (sg.count == 0) continue;
        float *const base = (float *)sg.data;
        const uint64_t i0 = sg.index, i1 = sg.index + sg.count;       // [i0, i1)
        const uint64_t g0 = i0 >> 2, g1 = (i1 - 1) >> 2;
        for (uint64_t g = g0 + threadIdx.x; g <= g1; g += TPB) {
            float z[4];
            const U4 o = philox4x32_10(U4{(uint32_t)g, p.tag, p.it_lo, p.it_hi}, p.k0, p.k1);
            box_muller(o.x, o.y, z[0], z[1]);
            box_muller(o.z, o.w, z[2], z[3]);
            const uint64_t gi = g << 2;
            // element gi + j lives at base[gi + j - i0]
            float *const q = base + (int64_t)(gi - i0);
            const bool full = gi >= i0 && gi + 4 <= i1;
            if (full && (((uintptr_t)q & 15u) == 0)) {
                float4 *const q4 = (float4 *)q;
                if (p.mode == ASR_NOISE_WRITE) {
                    *q4 = make_float4(z[0], z[1], z[2], z[3]);
                } else {
                    float4 v = *q4;
                    v.x = apply_one(v.x, sg.sigma, z[0], p.sign);
                    v.y = apply_one(v.y, sg.sigma, z[1], p.sign);
                    v.z = apply_one(v.z, sg.sigma, z[2], p.sign);
                    v.w = apply_one(v.w, sg.sigma, z[3], p.sign);
                    *q4 = v;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint64_t i = gi + j;
                    if (i < i0 || i >= i1) continue;
                    float *const e = base + (int64_t)(i - i0);
                    *e = p.mode == ASR_NOISE_WRITE ? z[j] : apply_one(*e, sg.sigma, z[j], p.sign);
                }
            }
        }
    }
}

__global__ __launch_bounds__(TPB) void nonfinite_flag_kernel(const float *__restrict__ x, int n,
                                                             uint32_t *__restrict__ flag) {
    __shared__ float scratch[32];
    float bad = 0.f;
    for (int i = threadIdx.x; i < n; i += TPB)
        if (!isfinite(x[i])) bad = 1.f;
    bad = asr::block_max(bad, scratch);
    if (threadIdx.x == 0) *flag = bad != 0.f ? 1u : 0u;
}

}  // namespace

extern "C" int asr_noise_chunk_elems(void) { return CHUNK; }

extern "C" int asr_gaussian_noise_f32(const AsrNoiseSegment *segs, int nsegs, uint64_t seed,
                                      uint32_t tag, uint64_t iteration, int mode, int sign,
                                      void *stream) {
    if (nsegs < 0 || (nsegs > 0 && !segs)) return ASR_EINVAL;
    if (mode != ASR_NOISE_APPLY && mode != ASR_NOISE_WRITE) return ASR_EINVAL;
    if (mode == ASR_NOISE_APPLY && sign != 1 && sign != -1) return ASR_EINVAL;
    if (nsegs == 0) return ASR_OK;
    NoiseParams p;
    p.segs = segs;
    p.nsegs = nsegs;
    p.k0 = (uint32_t)seed;
    p.k1 = (uint32_t)(seed >> 32);
    p.tag = tag;
    p.it_lo = (uint32_t)iteration;
    p.it_hi = (uint32_t)(iteration >> 32);
    p.mode = mode;
    p.sign = sign > 0 ? 1.f : -1.f;
    hipLaunchKernelGGL(noise_kernel, dim3(nsegs < 8192 ? nsegs : 8192), dim3(TPB), 0,
                       (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}

extern "C" int asr_nonfinite_flag_f32(const float *x, int n, uint32_t *flag, void *stream) {
    if (n < 0 || (n > 0 && !x) || !flag) return ASR_EINVAL;
    hipLaunchKernelGGL(nonfinite_flag_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, x, n, flag);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
