// The counter-based Gaussian draw of include/asr_amd.h (asr_gaussian_noise_f32): Philox4x32-10
// and Box-Muller, shared by the noise kernel (noise.hip) and the dither of the feature front-end
// (fbank.hip).
#pragma once
#include "common.h"

namespace asr {

struct U4 {
    uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) {
            k0 += W0;
            k1 += W1;
        }
        const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
        const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    }
    return c;
}

// (x >> 9) * 2^-23 + 2^-24: exact in fp32, strictly inside (0, 1)
__device__ __forceinline__ float unit_open(uint32_t x) {
    return __fadd_rn((float)(x >> 9) * 0x1p-23f, 0x1p-24f);
}

__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float &za, float &zb) {
    const float r = sqrtf(-2.f * logf(unit_open(a)));
    float s, c;
    sincospif(2.f * unit_open(b), &s, &c);
    za = r * c;
    zb = r * s;
}

}  // namespace asr
