// Batched Levenshtein distance with operation counts (include/asr_amd.h:
// asr_edit_distance_stats_i32, asr_edit_distance_max_len).
//
// The reference scores every utterance twice, characters and words, with
// edit_distance_with_stats (att_speech/utils.py:35-65): a Python double loop with an np.argmin per
// cell, an operation matrix and a trace-back.  Here one wave owns one pair.  Its lanes own 64
// columns of y (the reference text) and sweep the anti-diagonals of that strip: at step t lane l
// holds row i = t - l, takes the cell to its left from lane l - 1 (one cross-lane move), the
// diagonal one from what it took a step earlier and the upper one from its own previous step.
// A cell is one 64-bit value (dist, ins, del, sub: 16 bits each), and the counts travel forward
// with the distance from the chosen predecessor, which is the reference's trace-back read the
// other way: first minimum wins in the order up ("ins"), left ("del"), diagonal ("sub"), and a
// move counts only where the distance grows.  A y longer than 64 goes strip by strip; the last
// column of a strip is the left boundary of the next and stays in LDS (in place: row i is
// written 63 steps after it was read).  x is staged in LDS once.
//
// Latency-bound and tiny (one wave per pair, about 10^4 cells for a 100-character utterance);
// nothing here is near a roofline.  Integer arithmetic only: every result is exact.
#include "common.h"
#include "../../include/asr_amd.h"

namespace {

constexpr int MAX_LEN = 4096;           // per side: (MAX_LEN + 1) * 8 + MAX_LEN * 4 bytes of LDS < 64 KiB
typedef unsigned long long u64;

__device__ __forceinline__ u64 cell(uint32_t dist, uint32_t ins, uint32_t del, uint32_t sub) {
    return (u64)(dist | (ins << 16)) | ((u64)(del | (sub << 16)) << 32);
}

constexpr u64 STEP_INS = 1ull | (1ull << 16);
constexpr u64 STEP_DEL = 1ull | (1ull << 32);
constexpr u64 STEP_SUB = 1ull | (1ull << 48);

__device__ __forceinline__ u64 lane_up(u64 v) {
    const uint32_t lo = __shfl_up((uint32_t)v, 1, ASR_WAVE);
    const uint32_t hi = __shfl_up((uint32_t)(v >> 32), 1, ASR_WAVE);
    return (u64)lo | ((u64)hi << 32);
}

__global__ __launch_bounds__(ASR_WAVE) void edit_distance_stats_kernel(
        const int32_t *__restrict__ x, const int32_t *__restrict__ x_off,
        const int32_t *__restrict__ y, const int32_t *__restrict__ y_off, int max_x, int max_y,
        int32_t *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    u64 *const bnd = (u64 *)smem;                           // [max_x + 1]: cell(i, first column of the strip - 1)
    int32_t *const xs = (int32_t *)(bnd + max_x + 1);       // [max_x]
    const int p = blockIdx.x, lane = threadIdx.x;
    const int x0 = x_off[p], y0 = y_off[p];
    const int n = x_off[p + 1] - x0, m = y_off[p + 1] - y0;
    int32_t *const o = out + 4 * (int64_t)p;
    if (n < 0 || m < 0 || n > max_x || m > max_y) {         // not what the launch was sized for
        if (lane < 4) o[lane] = -1;
        return;
    }
    for (int i = lane; i <= n; i += ASR_WAVE) bnd[i] = cell(i, i, 0, 0);     // first column: all "ins"
    for (int i = lane; i < n; i += ASR_WAVE) xs[i] = x[x0 + i];
    __syncthreads();

    u64 cur = cell(n, n, 0, 0);                             // the answer when y is empty
    for (int c0 = 0; c0 < m; c0 += ASR_WAVE) {
        const int w = min(ASR_WAVE, m - c0);                // columns of this strip
        const bool last = c0 + ASR_WAVE >= m;
        const int j = c0 + lane + 1;                        // this lane's column, 1-based
        const bool col = lane < w;
        const int32_t yj = col ? y[y0 + j - 1] : 0;
        cur = cell(j, 0, j, 0);                             // cell(0, j): first row, all "del"
        u64 diag = cell(j - 1, 0, j - 1, 0);                // cell(0, j - 1)
        const int steps = n > 0 ? n + w - 1 : 0;
        // the LDS reads of step t + 1 are issued before the arithmetic of step t
        u64 b = n > 0 ? bnd[1] : 0;
        int32_t xi = n > 0 ? xs[min(max(-lane, 0), n - 1)] : 0;
        for (int t = 1; t <= steps; ++t) {
            const int i = t - lane;
            const u64 b_next = bnd[min(t + 1, n)];
            const int32_t x_next = xs[min(max(i, 0), n - 1)];
            u64 left = lane_up(cur);
            if (lane == 0) left = b;
            if (col && i >= 1 && i <= n) {
                const uint32_t neq = xi != yj;
                const uint32_t cu = ((uint32_t)cur & 0xffffu) + 1u;
                const uint32_t cl = ((uint32_t)left & 0xffffu) + 1u;
                const uint32_t cd = ((uint32_t)diag & 0xffffu) + neq;
                if (cu <= cl && cu <= cd) cur = cur + STEP_INS;
                else if (cl <= cd) cur = left + STEP_DEL;
                else cur = diag + (neq ? STEP_SUB : 0ull);
                if (!last && lane == ASR_WAVE - 1) bnd[i] = cur;
            }
            diag = left;
            b = b_next;
            xi = x_next;
        }
        __syncthreads();                                    // one wave per block: orders the LDS hand-over
    }
    const int owner = m > 0 ? (m - 1) & (ASR_WAVE - 1) : 0;
    if (lane == owner) {
        o[0] = (int32_t)(cur & 0xffffu);
        o[1] = (int32_t)((cur >> 16) & 0xffffu);
        o[2] = (int32_t)((cur >> 32) & 0xffffu);
        o[3] = (int32_t)((cur >> 48) & 0xffffu);
    }
}

}  // namespace

extern "C" int asr_edit_distance_max_len(void) { return MAX_LEN; }

extern "C" int asr_edit_distance_stats_i32(const int32_t *x, const int32_t *x_off, const int32_t *y,
                                           const int32_t *y_off, int n_pairs, int max_x, int max_y,
                                           int32_t *out, void *stream) {
    if (n_pairs < 0 || max_x < 0 || max_y < 0) return ASR_EINVAL;
    if (max_x > MAX_LEN || max_y > MAX_LEN) return ASR_EINVAL;
    if (n_pairs == 0) return ASR_OK;
    if (!x_off || !y_off || !out || (max_x > 0 && !x) || (max_y > 0 && !y)) return ASR_EINVAL;
    const size_t lds = (size_t)(max_x + 1) * sizeof(u64) + (size_t)max_x * sizeof(int32_t);
    hipLaunchKernelGGL(edit_distance_stats_kernel, dim3(n_pairs), dim3(ASR_WAVE), lds,
                       (hipStream_t)stream, x, x_off, y, y_off, max_x, max_y, out);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
