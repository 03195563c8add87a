// Pieces shared by the persistent recurrences (lstm.hip, gru.hip): MFMA operand types,
// the fragment-major operand layout and its pack kernel, the bounded team hand-off wait,
// the team control block and the generic persistent launcher with its admission check.
#pragma once
#include "common.h"
#include <stdlib.h>

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

// The four post-activation gates of one (frame, direction, utterance, hidden unit) are
// saved for the backward pass as ONE 8-byte record of four bf16 (i,f,g,o): a single
// coalesced 8 B/lane store / load per element instead of four fp32 ones with stride H
// (the saved gates were the recurrence's largest stream: 1.75 GB per layer at B=512).
__device__ __forceinline__ u32x2 pack_gates(const float g[4]) {
    const unsigned s0 = __builtin_bit_cast(unsigned short, (__bf16)g[0]);
    const unsigned s1 = __builtin_bit_cast(unsigned short, (__bf16)g[1]);
    const unsigned s2 = __builtin_bit_cast(unsigned short, (__bf16)g[2]);
    const unsigned s3 = __builtin_bit_cast(unsigned short, (__bf16)g[3]);
    u32x2 v;
    v[0] = s0 | (s1 << 16);
    v[1] = s2 | (s3 << 16);
    return v;
}
__device__ __forceinline__ void unpack_gates(u32x2 v, float g[4]) {
    const unsigned lo = v[0], hi = v[1];
    g[0] = __builtin_bit_cast(float, lo << 16);
    g[1] = __builtin_bit_cast(float, lo & 0xFFFF0000u);
    g[2] = __builtin_bit_cast(float, hi << 16);
    g[3] = __builtin_bit_cast(float, hi & 0xFFFF0000u);
}
typedef __attribute__((ext_vector_type(16))) float f32x16;

// v_exp_f32 / v_rcp_f32 forms (about 1 ulp each): four instructions per
// sigmoid instead of a full-precision division sequence
__device__ __forceinline__ float sigmoidf_(float x) {
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
__device__ __forceinline__ float tanhf_(float x) {
    return 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-2.8853900817779268f * x)) - 1.f;
}

// element (row b, column k) of a [rows x 16*KS] operand in fragment-major order
__device__ __forceinline__ size_t frag_off(int b, int k, int KS) {
    return ((((size_t)(b >> 5) * KS + (k >> 4)) * 64 + ((b & 31) + 32 * ((k >> 3) & 1))) << 3) + (k & 7);
}

// out = fragment-major copy of `rows` x `cols` (cols % 16 == 0, rows % 32 == 0)
// row-major bf16 matrices, `nmat` of them; transpose != 0 reads in[c][r].
__global__ void lstm_pack_kernel(const __bf16 *in, __bf16 *out, int nmat, int rows,
                                 int cols, int transpose) {
    const size_t per = (size_t)rows * cols;
    const size_t total = per * nmat;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / per);
        const size_t rem = i % per;
        const int r = (int)(rem / cols), c = (int)(rem % cols);
        const __bf16 v = transpose ? in[(size_t)m * per + (size_t)c * rows + r]
                                   : in[(size_t)m * per + rem];
        out[(size_t)m * per + frag_off(r, c, cols / 16)] = v;
    }
}

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
#define ASR_SC1 16

__device__ __forceinline__ bool team_wait(unsigned *ctr, unsigned target, unsigned limit,
                                          unsigned *err) {
    for (unsigned it = 0; it < limit; ++it) {
        if (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target)
            return true;
        __builtin_amdgcn_s_sleep(1);
    }
    __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return false;
}

// acc += A[32 x 16*(K1-K0)] · B over the k-steps K0..K1-1: the A fragments (1 KiB apart in
// LDS, fragment-major) are read D k-steps ahead into a rotating register set.  Written as
// one dependent ds_read -> MFMA pair per k-step the chain pays the LDS latency (~100
// cycles) 20 times per phase: measured 1998 cycles for 20 MFMAs that need 640 in the pipe.
template <int K0, int K1, int D, int KS>
__device__ __forceinline__ f32x16 mfma_chain(const bf16x8 *al, const bf16x8 (&fb)[KS], f32x16 acc) {
    bf16x8 a[D];
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (K0 + d < K1) a[d] = al[(K0 + d) * 64];
#pragma unroll
    for (int k = K0; k < K1; ++k) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[(k - K0) % D], fb[k], acc, 0, 0, 0);
        if (k + D < K1) a[(k - K0) % D] = al[(k + D) * 64];
    }
    // keep that order: the scheduler otherwise sinks every read next to its MFMA again
#pragma unroll
    for (int d = 0; d < D; ++d) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
    for (int k = K0; k < K1; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (k + D < K1) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    return acc;
}

struct LstmTeamCtl {
    unsigned *ctr;          // [2 dir][nbt] counters, 32 words (128 B) apart, zeroed per call
    unsigned *err;          // timeout word
    unsigned spin_limit;
    int bt0, nbt;           // first batch tile of this launch, batch tiles in total
    int xcd_teams;          // 0: grid (jt, batch tile, dir); else teams of the XCD-affine 1-D grid
    size_t rows;            // rows of one hbuf / dgbuf plane (>= 32 * nbt)
};

// several ranges in ONE launch (a forward call clears its state buffers, the four pad frames
// of y_bf16 and the team counters: six 5-us launches per layer and direction pair otherwise)
struct ZeroRanges { uint32_t *p[6]; size_t n[6]; int count; };
__global__ void zero_ranges_kernel(ZeroRanges z) {
    for (int r = 0; r < z.count; ++r) {
        size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
        const size_t stride = (size_t)gridDim.x * blockDim.x;
        for (; i < z.n[r]; i += stride) z.p[r][i] = 0u;
    }
}
struct ZeroList {
    ZeroRanges z;
    ZeroList() { z.count = 0; }
    void add(void *p, size_t bytes) {
        if (bytes / 4 == 0) return;
        z.p[z.count] = (uint32_t *)p; z.n[z.count] = bytes / 4; ++z.count;
    }
    void launch(hipStream_t s) {
        if (!z.count) return;
        size_t most = 0;
        for (int r = 0; r < z.count; ++r) most = z.n[r] > most ? z.n[r] : most;
        int blocks = (int)((most + 255) / 256);
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(zero_ranges_kernel, dim3(blocks), dim3(256), 0, s, z);
    }
};

inline int64_t ctl_bytes(int B) { return ((int64_t)2 * ((B + 15) / 16) * 128 + 256 + 255) / 256 * 256; }

// persistent path on unless ASR_LSTM_PERSIST=0 (A/B switch for tests and profiling)
inline bool persist_enabled() {
    const char *e = getenv("ASR_LSTM_PERSIST");
    return !(e && e[0] == '0');
}

inline int cu_count() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return cus;
}

// Launch a persistent kernel over all batch tiles, at most one workgroup per CU
// per launch (every team of a launch must be resident).  Returns false if the
// shape cannot run persistently (caller falls back to one launch per step).
// rows of one hbuf / dgbuf plane: 32 per batch tile of the smallest tile (16 rows), or
// the 64-row padding of the per-step kernels, whichever is larger
inline int64_t plane_rows(int B) {
    const int64_t a = (int64_t)(B + 63) / 64 * 64, b = (int64_t)((B + 15) / 16) * 32;
    return a > b ? a : b;
}

inline int pick_tile_rows(int B, int njt, int cus) {
    for (int cand = 2; cand <= 4; ++cand)
        if (2 * njt * ((B + 8 * cand - 1) / (8 * cand)) <= cus) return cand;
    return 4;
}

template <typename P>
bool launch_persist(void (*const kerns[3])(P, LstmTeamCtl), const P &p, int B, int H,
                    size_t lds_need, unsigned *ctl_words, unsigned *err_flag, hipStream_t s) {
    const int njt = H / 64;
    const int cus = cu_count();
    if ((H % 64) != 0 || njt < 1 || cus < 2 * njt || lds_need > 160 * 1024) return false;
    // batch-tile rows: the smallest of 16 / 24 / 32 whose whole grid is one launch with one
    // workgroup per CU (more workgroups = less work on each one's critical path); 32-row
    // tiles in several launches when the batch is too large for that
    const int ne = pick_tile_rows(B, njt, cus);
    void (*kern)(P, LstmTeamCtl) = kerns[ne - 2];
    if (!kern) return false;
    const int nbt = (B + 8 * ne - 1) / (8 * ne);
    const size_t lds = lds_need > 84 * 1024 ? lds_need : 84 * 1024;     // > half the LDS: 1 workgroup per CU
    if (hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        return false;
    const int max_bt = cus / (2 * njt);
    LstmTeamCtl ctl;
    ctl.ctr = ctl_words + 64;
    ctl.err = err_flag ? err_flag : ctl_words;
    ctl.spin_limit = 1u << 18;
    if (const char *e = getenv("ASR_LSTM_SPIN_LIMIT")) ctl.spin_limit = (unsigned)strtoul(e, nullptr, 10);
    ctl.nbt = nbt;
    ctl.rows = (size_t)plane_rows(B);
    for (int bt0 = 0; bt0 < nbt; bt0 += max_bt) {
        ctl.bt0 = bt0;
        const int n = nbt - bt0 < max_bt ? nbt - bt0 : max_bt;
        // XCD-affine placement of the teams when the grid padded to a multiple of 8 teams
        // still is one workgroup per CU (ASR_LSTM_XCD=0: plain 3-D grid)
        const int padded = 8 * njt * ((2 * n + 7) / 8);
        static const bool xcd_on = !(getenv("ASR_LSTM_XCD") && getenv("ASR_LSTM_XCD")[0] == '0');
        if (xcd_on && padded <= cus) {
            ctl.xcd_teams = 2 * n;
            hipLaunchKernelGGL(kern, dim3(padded), dim3(512), lds, s, p, ctl);
        } else {
            ctl.xcd_teams = 0;
            hipLaunchKernelGGL(kern, dim3(njt, n, 2), dim3(512), lds, s, p, ctl);
        }
    }
    return true;
}

}  // namespace
