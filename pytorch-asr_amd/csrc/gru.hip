// Bidirectional GRU recurrence (no bias) for gfx950: the recurrent part of a BatchRNN built
// with rnn_type=nn.GRU (att_speech/modules/encoders/encoder_utils.py), with the arithmetic of
// torch.nn.GRU(bias=False).  Per direction, rows of W_ih / W_hh in torch's order r | z | n:
//   r = σ(gx_r + h·W_hrᵀ)      z = σ(gx_z + h·W_hzᵀ)
//   hn = h·W_hnᵀ               n = tanh(gx_n + r ⊙ hn)          (r multiplies hn, not the sum)
//   h' = (1 − z) ⊙ n + z ⊙ h
// x·W_ihᵀ of all frames and both directions (`gx`) is one dense GEMM done by the caller.
//
// Same contract and the same two implementations as lstm.hip (bit-identical outputs, see
// tests/test_gru_gpu.py):
//   * PER-STEP (ASR_LSTM_PERSIST=0, and the fallback for shapes the persistent kernels do not
//     take): one launch per time step for both directions, grid (H/32, ceil(B/32), 2); a
//     192-thread workgroup owns a [32 batch x 32 hidden] tile, wave g computes the h·W_hhᵀ
//     tile of gate g (v_mfma_f32_32x32x16_bf16, K = H) from the fragment-major h_{t-1} plane
//     staged in LDS and its W_hh fragments read from L2;
//   * PERSISTENT (default): one launch walks all T steps.  A 512-thread workgroup owns a
//     [8·NE batch x 64 hidden] tile for the whole sequence: waves 0-5 = (gate, 32-column half)
//     keep their W_hh fragments in registers, every wave keeps the fp32 state of its rows
//     (rows e·8 + wave) in registers.  Teams of H/64 workgroups (one direction, one batch tile)
//     hand h_t (forward) / [dr, dz, dhn]_t (backward) over through L2 once per step with the
//     protocol of lstm.hip: sc1 (write-through) tile stores, vmcnt(0), workgroup barrier, one
//     relaxed agent-scope counter add; consumers poll the counter from one lane with a bounded
//     spin (ASR_LSTM_SPIN_LIMIT), pass a barrier and read the tile with sc1 loads only.  A
//     timeout sets the caller's error word and poisons the outputs with NaN.
// Waves 6 and 7 of the persistent kernels take no MFMA tile (a 64-unit tile has 3 x 64 = 192
// gate columns, six 32-column MFMA tiles); they share the pointwise work, which keeps the row
// mapping of the LSTM kernels (8 waves x NE rows).
//
// Packed-sequence semantics with a padded batch: utterance b is active at frame t iff
// t < lens[b]; inactive frames emit zeros and reset the state to zero, so the reverse direction
// starts from the zero state at each utterance's own last frame, and no value of a padding
// frame (gx rows included) reaches an output.  The saved h_{t-1} of the backward pass is the
// fp32 output y of the neighbouring frame (zero where that frame is inactive).
#include "common.h"
#include "../../include/asr_amd.h"
#include "recurrence.h"

namespace {

// Forward cell: a* are the h·W_hhᵀ terms of the three gates.  rec = the record saved for the
// backward pass (r, z, n, hn).  Contraction is off so both kernels round identically.
__device__ __forceinline__ float gru_cell_fwd(float gr, float gz, float gn, float ar, float az,
                                              float hn, float hprev, float rec[4]) {
#pragma clang fp contract(off)
    const float r = sigmoidf_(gr + ar);
    const float z = sigmoidf_(gz + az);
    const float n = tanhf_(gn + r * hn);
    rec[0] = r; rec[1] = z; rec[2] = n; rec[3] = hn;
    return (1.f - z) * n + z * hprev;
}

// Backward cell.  dh = dL/dh' (incoming dy + recurrent gradient + carried dh'·z of the later
// step); d[] = (dr_pre, dz_pre, dn_pre, dhn); carry = dh·z, the pointwise part of dL/dh.
__device__ __forceinline__ void gru_cell_bwd(const float g[4], float hprev, float dh, float d[4],
                                             float &carry) {
#pragma clang fp contract(off)
    const float r = g[0], z = g[1], n = g[2], hn = g[3];
    const float dn = dh * (1.f - z) * (1.f - n * n);
    d[0] = dn * hn * r * (1.f - r);
    d[1] = dh * (hprev - n) * z * (1.f - z);
    d[2] = dn;
    d[3] = dn * r;
    carry = dh * z;
}

// (dy + carry) + the three K-block partial sums of dh_rec, one fixed order for both kernels
__device__ __forceinline__ float gru_dh(float dy, float carry, float p0, float p1, float p2) {
#pragma clang fp contract(off)
    return (dy + carry) + ((p0 + p1) + p2);
}

template <int GXB>
__device__ __forceinline__ float gru_load_gx(const void *gx, size_t i) {
    if constexpr (GXB) return (float)((const __bf16 *)gx)[i];
    else return ((const float *)gx)[i];
}

// element (row, col) of a 64-column tile staged in LDS in fragment-major order (4 k-steps)
__device__ __forceinline__ int tile_slot(int row, int col) {
    return ((col >> 4) * 64 + row + 32 * ((col >> 3) & 1)) * 8 + (col & 7);
}

struct GruFwdParams {
    const void *gx;         // [T,B,2,3H] x·W_ihᵀ, gate order r,z,n; float or (gx_bf16) __bf16
    int gx_bf16;
    const __bf16 *whh;      // fragment-major pack of [2*3 (dir,gate)][H rows][H cols]
    const int32_t *lens;    // [B]
    int T, B, H;
    size_t rows;            // rows of one hbuf plane
    __bf16 *hbuf;           // [2 pingpong][2 dir] fragment-major [rows x H]
    float *y;               // [T,B,2,H] per-direction outputs (zeros when inactive)
    __bf16 *ybf;            // [2,T+2,B,H] bf16 copy, frame t at index t+1 (zero frames at both ends)
    u32x2 *gates;           // [T,2,B,H] records of 4 bf16 (r, z, n, hn); zeros when inactive
    int step;
};

struct GruBwdParams {
    const float *dy;        // [T,B,2,H], or [T,B,H] with dy_shared (one gradient for both directions)
    int dy_shared;
    const __bf16 *whhT;     // fragment-major pack of W_hhᵀ: [2 dir][H rows][3H cols]
    const int32_t *lens;
    int T, B, H;
    size_t rows;            // rows of one dgbuf plane
    const u32x2 *gates;     // [T,2,B,H] records (r, z, n, hn)
    const float *y;         // [T,B,2,H] forward outputs: h_{t-1}
    __bf16 *dgbuf;          // [2 pingpong][2 dir] fragment-major [rows x 3H]: [dr, dz, dhn] of the previous step
    float *dcbuf;           // [2 dir][B][H] carried dh'·z (per-step kernels)
    __bf16 *dgx;            // [T,B,2,3H] (dr, dz, dn) pre-activation gradients = d gx
    __bf16 *dhn;            // [T,B,2,H]  dhn = dn·r: the n-third of the W_hh gradient operand
    int step;
};

// ---------------------------------------------------------------------------
// Per-step kernels

template <int KS, int GXB>
__global__ __launch_bounds__(192) void gru_fwd_step_kernel(GruFwdParams p) {
    __shared__ __attribute__((aligned(16))) __bf16 a_lds[KS * 512];
    __shared__ float g_lds[3][32][33];
    const int H = p.H, B = p.B, T = p.T;
    const int j0 = blockIdx.x * 32, b0 = blockIdx.y * 32, dir = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = dir == 0 ? p.step : T - 1 - p.step;
    const int tp = dir == 0 ? t - 1 : t + 1;
    const __bf16 *hprev = p.hbuf + ((size_t)(p.step & 1) * 2 + dir) * p.rows * H;
    __bf16 *hnext = p.hbuf + ((size_t)((p.step + 1) & 1) * 2 + dir) * p.rows * H;

    bf16x8 fb[KS];
    {
        const __bf16 *bp = p.whh + (size_t)(dir * 3 + wave) * H * H + ((size_t)blockIdx.x * KS * 64 + lane) * 8;
#pragma unroll
        for (int k = 0; k < KS; ++k) fb[k] = *reinterpret_cast<const bf16x8 *>(bp + k * 512);
    }
    {
        const bf16x8 *src = reinterpret_cast<const bf16x8 *>(hprev + (size_t)blockIdx.y * KS * 512);
        bf16x8 *dst = reinterpret_cast<bf16x8 *>(a_lds);
        for (int c = threadIdx.x; c < KS * 64; c += 192) dst[c] = src[c];
    }

    constexpr int NE = (1024 + 191) / 192;
    float pgx[NE][3], php[NE];
    bool pact[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int idx = e * 192 + threadIdx.x;
        const int b = b0 + ((idx & 1023) >> 5), j = j0 + (idx & 31);
        const int bc = b < B ? b : B - 1;
        const int len = p.lens[bc];
        pact[e] = idx < 1024 && b < B && t < len;
        const size_t gxo = (((size_t)t * B + bc) * 2 + dir) * 3 * H + j;
#pragma unroll
        for (int g = 0; g < 3; ++g) pgx[e][g] = gru_load_gx<GXB>(p.gx, gxo + (size_t)g * H);
        const int tpc = tp < 0 ? 0 : (tp >= T ? T - 1 : tp);
        const float hv = p.y[(((size_t)tpc * B + bc) * 2 + dir) * H + j];
        php[e] = (tp >= 0 && tp < len) ? hv : 0.f;
    }
    __syncthreads();

    {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        const bf16x8 *al = reinterpret_cast<const bf16x8 *>(a_lds) + lane;
#pragma unroll
        for (int k = 0; k < KS; ++k)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[k * 64], fb[k], acc, 0, 0, 0);
        const int col = lane & 31;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
            g_lds[wave][row][col] = acc[i];
        }
    }
    __syncthreads();

#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int idx = e * 192 + threadIdx.x;
        if (idx >= 1024) continue;
        const int row = idx >> 5, col = idx & 31;
        const int b = b0 + row, j = j0 + col;
        if (b >= B) continue;
        float rec[4] = {0.f, 0.f, 0.f, 0.f}, h = 0.f;
        if (pact[e])
            h = gru_cell_fwd(pgx[e][0], pgx[e][1], pgx[e][2], g_lds[0][row][col], g_lds[1][row][col],
                             g_lds[2][row][col], php[e], rec);
        hnext[frag_off(b, j, KS)] = (__bf16)h;
        p.y[(((size_t)t * B + b) * 2 + dir) * H + j] = h;
        p.ybf[(((size_t)dir * (T + 2) + t + 1) * B + b) * H + j] = (__bf16)h;
        p.gates[(((size_t)t * 2 + dir) * B + b) * H + j] = pack_gates(rec);
    }
}

template <int KS>
__global__ __launch_bounds__(192) void gru_bwd_step_kernel(GruBwdParams p) {
    __shared__ float part[3][32][33];
    constexpr int KS3 = 3 * KS;
    const int H = p.H, B = p.B, T = p.T, H3 = 3 * p.H;
    const int j0 = blockIdx.x * 32, b0 = blockIdx.y * 32, dir = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // the backward scan visits frames in the opposite order of the forward one
    const int t = dir == 0 ? T - 1 - p.step : p.step;
    const int tp = dir == 0 ? t - 1 : t + 1;
    const __bf16 *dgprev = p.dgbuf + ((size_t)(p.step & 1) * 2 + dir) * p.rows * H3;
    __bf16 *dgnext = p.dgbuf + ((size_t)((p.step + 1) & 1) * 2 + dir) * p.rows * H3;

    // wave w: the K block of gate w (columns w*H .. w*H + H-1 of [dr, dz, dhn])
    bf16x8 fb[KS], fa[KS];
    {
        const __bf16 *bp = p.whhT + (size_t)dir * H * H3 +
                           (((size_t)blockIdx.x * KS3 + (size_t)wave * KS) * 64 + lane) * 8;
        const __bf16 *ap = dgprev + (((size_t)blockIdx.y * KS3 + (size_t)wave * KS) * 64 + lane) * 8;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            fb[k] = *reinterpret_cast<const bf16x8 *>(bp + k * 512);
            fa[k] = *reinterpret_cast<const bf16x8 *>(ap + k * 512);
        }
    }

    constexpr int NE = (1024 + 191) / 192;
    u32x2 pg[NE];
    float php[NE], pdy[NE], pdc[NE];
    bool pact[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int idx = e * 192 + threadIdx.x;
        const int b = b0 + ((idx & 1023) >> 5), j = j0 + (idx & 31);
        const int bc = b < B ? b : B - 1;
        const int len = p.lens[bc];
        pact[e] = idx < 1024 && b < B && t < len;
        pg[e] = p.gates[(((size_t)t * 2 + dir) * B + bc) * H + j];
        const int tpc = tp < 0 ? 0 : (tp >= T ? T - 1 : tp);
        const float hv = p.y[(((size_t)tpc * B + bc) * 2 + dir) * H + j];
        php[e] = (tp >= 0 && tp < len) ? hv : 0.f;
        pdy[e] = p.dy[p.dy_shared ? ((size_t)t * B + bc) * H + j : (((size_t)t * B + bc) * 2 + dir) * H + j];
        pdc[e] = p.dcbuf[((size_t)dir * B + bc) * H + j];
    }

    {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int k = 0; k < KS; ++k)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[k], fb[k], acc, 0, 0, 0);
        const int col = lane & 31;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
            part[wave][row][col] = acc[i];
        }
    }
    __syncthreads();

#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int idx = e * 192 + threadIdx.x;
        if (idx >= 1024) continue;
        const int row = idx >> 5, col = idx & 31;
        const int b = b0 + row, j = j0 + col;
        if (b >= B) continue;
        float d[4] = {0.f, 0.f, 0.f, 0.f}, carry = 0.f;
        if (pact[e]) {
            float g[4];
            unpack_gates(pg[e], g);
            const float dh = gru_dh(pdy[e], pdc[e], part[0][row][col], part[1][row][col], part[2][row][col]);
            gru_cell_bwd(g, php[e], dh, d, carry);
        }
        // no gradient reaches a padding frame; the carried gradient restarts from zero
        p.dcbuf[((size_t)dir * B + b) * H + j] = carry;
        __bf16 *dgo = p.dgx + (((size_t)t * B + b) * 2 + dir) * H3 + j;
        dgo[0] = (__bf16)d[0]; dgo[H] = (__bf16)d[1]; dgo[2 * H] = (__bf16)d[2];
        p.dhn[(((size_t)t * B + b) * 2 + dir) * H + j] = (__bf16)d[3];
        dgnext[frag_off(b, j, KS3)] = (__bf16)d[0];
        dgnext[frag_off(b, H + j, KS3)] = (__bf16)d[1];
        dgnext[frag_off(b, 2 * H + j, KS3)] = (__bf16)d[3];
    }
}

// ---------------------------------------------------------------------------
// Persistent kernels

#define ASR_GRU_PART_BYTES (3 * 32 * 65 * 4)

// team position of this workgroup: the plain 3-D grid (jt, batch tile, dir) or, with
// ctl.xcd_teams, the XCD-affine 1-D grid of launch_persist (speed only, as in lstm.hip)
__device__ __forceinline__ bool gru_team_pos(const LstmTeamCtl &ctl, int H, int &jt, int &btile, int &dir) {
    jt = blockIdx.x; btile = blockIdx.y + ctl.bt0; dir = blockIdx.z;
    if (ctl.xcd_teams) {
        const int slot = blockIdx.x >> 3, team = (slot / (H / 64)) * 8 + (blockIdx.x & 7);
        if (team >= ctl.xcd_teams) return false;
        jt = slot % (H / 64);
        btile = (team >> 1) + ctl.bt0;
        dir = team & 1;
    }
    return true;
}

template <int KS, int NE, int GXB>
__global__ __launch_bounds__(512) void gru_fwd_persist_kernel(GruFwdParams p, LstmTeamCtl ctl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __bf16 *a_lds = reinterpret_cast<__bf16 *>(smem);                                  // KS KiB
    float (*g_lds)[32][65] = reinterpret_cast<float (*)[32][65]>(smem + KS * 1024);
    __bf16 *h_lds = reinterpret_cast<__bf16 *>(smem + KS * 1024 + ASR_GRU_PART_BYTES);  // 4 KiB
    __shared__ int dead_s;
    const int H = p.H, B = p.B, T = p.T;
    int jt, btile, dir;
    if (!gru_team_pos(ctl, H, jt, btile, dir)) return;
    const int j0 = jt * 64, b0 = btile * (8 * NE), njt = H / 64;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int gate = wave >> 1, js = wave & 1;
    const size_t Bp = ctl.rows;
    unsigned *myctr = ctl.ctr + ((size_t)dir * ctl.nbt + btile) * 32;
    if (tid == 0) dead_s = 0;
    for (int i = tid; i < 2048; i += 512) h_lds[i] = (__bf16)0.f;       // padding rows stay 0

    bf16x8 fb[KS];
    if (wave < 6) {
        const size_t wo = (size_t)(dir * 3 + gate) * H * H + ((size_t)(2 * jt + js) * KS * 64 + lane) * 8;
#pragma unroll
        for (int k = 0; k < KS; ++k) fb[k] = *reinterpret_cast<const bf16x8 *>(p.whh + wo + k * 512);
    }
    const __amdgpu_buffer_rsrc_t hres = __builtin_amdgcn_make_buffer_rsrc(
        p.hbuf, 0, (int)(2 * 2 * Bp * H * 2), 0x00020000);

    const int col = lane, j = j0 + col;
    float hs[NE];
    int len[NE], bcl[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int b = b0 + e * 8 + wave;
        hs[e] = 0.f;
        len[e] = b < B ? p.lens[b] : 0;
        bcl[e] = b < B ? b : B - 1;
    }

    for (int step = 0; step < T; ++step) {
        const int t = dir == 0 ? step : T - 1 - step;
        float pgx[NE][3];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const size_t gxo = (((size_t)t * B + bcl[e]) * 2 + dir) * 3 * H + j;
#pragma unroll
            for (int g = 0; g < 3; ++g) pgx[e][g] = gru_load_gx<GXB>(p.gx, gxo + (size_t)g * H);
        }
        if (step > 0 && tid == 0 && !dead_s) {
            if (!team_wait(myctr, (unsigned)(njt * step), ctl.spin_limit, ctl.err)) dead_s = 1;
        }
        __syncthreads();
        // h_{t-1} of the team's batch tile: all H columns, 32 rows (rows past the tile are zero)
        {
            const unsigned base = (unsigned)((((size_t)(step & 1) * 2 + dir) * Bp * H +
                                              (size_t)btile * KS * 512) * 2);
            for (int c = tid; c < KS * 64; c += 512)
                reinterpret_cast<u32x4 *>(a_lds)[c] =
                    __builtin_amdgcn_raw_buffer_load_b128(hres, base + (unsigned)c * 16u, 0, ASR_SC1);
        }
        __syncthreads();
        if (wave < 6) {
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            const bf16x8 *al = reinterpret_cast<const bf16x8 *>(a_lds) + lane;
            acc = mfma_chain<0, KS, 4>(al, fb, acc);
            const int c32 = lane & 31;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                g_lds[gate][row][js * 32 + c32] = acc[i];
            }
        }
        __syncthreads();
        const bool dead = dead_s != 0;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int row = e * 8 + wave, b = b0 + row;
            float rec[4] = {0.f, 0.f, 0.f, 0.f}, h = 0.f;
            if (t < len[e]) {
                h = gru_cell_fwd(pgx[e][0], pgx[e][1], pgx[e][2], g_lds[0][row][col], g_lds[1][row][col],
                                 g_lds[2][row][col], hs[e], rec);
                if (dead) h = __builtin_nanf("");
            }
            hs[e] = h;
            h_lds[tile_slot(row, col)] = (__bf16)h;
            if (b < B) {
                p.y[(((size_t)t * B + b) * 2 + dir) * H + j] = h;
                p.ybf[(((size_t)dir * (T + 2) + t + 1) * B + b) * H + j] = (__bf16)h;
                p.gates[(((size_t)t * 2 + dir) * B + b) * H + j] = pack_gates(rec);
            }
        }
        __syncthreads();
        if (wave < 4) {
            const u32x4 v = reinterpret_cast<const u32x4 *>(h_lds)[wave * 64 + lane];
            const unsigned off = (unsigned)(((((size_t)((step + 1) & 1) * 2 + dir) * Bp * H) +
                                             ((size_t)btile * KS + 4 * jt + wave) * 512 + lane * 8) * 2);
            __builtin_amdgcn_raw_buffer_store_b128(v, hres, off, 0, ASR_SC1);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(myctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int KS, int NE>
__global__ __launch_bounds__(512) void gru_bwd_persist_kernel(GruBwdParams p, LstmTeamCtl ctl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int KS3 = 3 * KS;
    __bf16 *a_lds = reinterpret_cast<__bf16 *>(smem);                                  // 3*KS KiB
    float (*part)[32][65] = reinterpret_cast<float (*)[32][65]>(smem + KS3 * 1024);
    __bf16 *dg_lds = reinterpret_cast<__bf16 *>(smem + KS3 * 1024 + ASR_GRU_PART_BYTES);   // 12 KiB
    __shared__ int dead_s;
    const int H = p.H, B = p.B, T = p.T, H3 = 3 * p.H;
    int jt, btile, dir;
    if (!gru_team_pos(ctl, H, jt, btile, dir)) return;
    const int j0 = jt * 64, b0 = btile * (8 * NE), njt = H / 64;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int kq = wave >> 1, js = wave & 1;
    const size_t Bp = ctl.rows;
    unsigned *myctr = ctl.ctr + ((size_t)dir * ctl.nbt + btile) * 32;
    if (tid == 0) dead_s = 0;
    for (int i = tid; i < 3 * 2048; i += 512) dg_lds[i] = (__bf16)0.f;   // padding rows stay 0

    bf16x8 fb[KS];
    if (wave < 6) {
        const __bf16 *bp = p.whhT + (size_t)dir * H * H3 +
                           (((size_t)(2 * jt + js) * KS3 + (size_t)kq * KS) * 64 + lane) * 8;
#pragma unroll
        for (int k = 0; k < KS; ++k) fb[k] = *reinterpret_cast<const bf16x8 *>(bp + k * 512);
    }
    const __amdgpu_buffer_rsrc_t dres = __builtin_amdgcn_make_buffer_rsrc(
        p.dgbuf, 0, (int)(2 * 2 * Bp * H3 * 2), 0x00020000);

    const int col = lane, j = j0 + col;
    float carry[NE];
    int len[NE], bcl[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int b = b0 + e * 8 + wave;
        carry[e] = 0.f;
        len[e] = b < B ? p.lens[b] : 0;
        bcl[e] = b < B ? b : B - 1;
    }

    for (int step = 0; step < T; ++step) {
        const int t = dir == 0 ? T - 1 - step : step;
        const int tp = dir == 0 ? t - 1 : t + 1;
        const int tpc = tp < 0 ? 0 : (tp >= T ? T - 1 : tp);
        u32x2 pg[NE];
        float php[NE], pdy[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int bc = bcl[e];
            pg[e] = p.gates[(((size_t)t * 2 + dir) * B + bc) * H + j];
            php[e] = p.y[(((size_t)tpc * B + bc) * 2 + dir) * H + j];
            pdy[e] = p.dy[p.dy_shared ? ((size_t)t * B + bc) * H + j : (((size_t)t * B + bc) * 2 + dir) * H + j];
        }
        if (step > 0 && tid == 0 && !dead_s) {
            if (!team_wait(myctr, (unsigned)(njt * step), ctl.spin_limit, ctl.err)) dead_s = 1;
        }
        __syncthreads();
        // [dr, dz, dhn] of the previous step, the team's batch tile: all 3H columns, 32 rows
        {
            const unsigned base = (unsigned)((((size_t)(step & 1) * 2 + dir) * Bp * H3 +
                                              (size_t)btile * KS3 * 512) * 2);
            for (int c = tid; c < KS3 * 64; c += 512)
                reinterpret_cast<u32x4 *>(a_lds)[c] =
                    __builtin_amdgcn_raw_buffer_load_b128(dres, base + (unsigned)c * 16u, 0, ASR_SC1);
        }
        __syncthreads();
        if (wave < 6) {
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            const bf16x8 *al = reinterpret_cast<const bf16x8 *>(a_lds) + (size_t)kq * KS * 64 + lane;
            acc = mfma_chain<0, KS, 4>(al, fb, acc);
            const int c32 = lane & 31;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                part[kq][row][js * 32 + c32] = acc[i];
            }
        }
        __syncthreads();
        const bool dead = dead_s != 0;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int row = e * 8 + wave, b = b0 + row;
            float d[4] = {0.f, 0.f, 0.f, 0.f}, cout = 0.f;
            if (t < len[e]) {
                float g[4];
                unpack_gates(pg[e], g);
                const float hp = (tp >= 0 && tp < len[e]) ? php[e] : 0.f;
                const float dh = gru_dh(pdy[e], carry[e], part[0][row][col], part[1][row][col], part[2][row][col]);
                gru_cell_bwd(g, hp, dh, d, cout);
                if (dead) d[0] = d[1] = d[2] = d[3] = __builtin_nanf("");
            }
            carry[e] = cout;
            const int slot = tile_slot(row, col);
            dg_lds[slot] = (__bf16)d[0];
            dg_lds[2048 + slot] = (__bf16)d[1];
            dg_lds[4096 + slot] = (__bf16)d[3];
            if (b < B) {
                __bf16 *dgo = p.dgx + (((size_t)t * B + b) * 2 + dir) * H3 + j;
                dgo[0] = (__bf16)d[0]; dgo[H] = (__bf16)d[1]; dgo[2 * H] = (__bf16)d[2];
                p.dhn[(((size_t)t * B + b) * 2 + dir) * H + j] = (__bf16)d[3];
            }
        }
        __syncthreads();
        if (wave < 6) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int bi = wave * 2 + r, g = bi >> 2, kk = bi & 3;
                const u32x4 v = reinterpret_cast<const u32x4 *>(dg_lds)[bi * 64 + lane];
                const unsigned off = (unsigned)(((((size_t)((step + 1) & 1) * 2 + dir) * Bp * H3) +
                                                 ((size_t)btile * KS3 + g * KS + 4 * jt + kk) * 512 + lane * 8) * 2);
                __builtin_amdgcn_raw_buffer_store_b128(v, dres, off, 0, ASR_SC1);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(myctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

inline bool gru_built(int H) { return H == 64 || H == 128 || H == 256 || H == 320; }

// workspace: hand-off planes [2][2][rows][3H] bf16 (the forward pass uses the first third),
// carried gradient [2][B][H] f32, packed W_hh / W_hhᵀ [2][3H][H] bf16, team counters
inline size_t gru_planes_bytes(int B, int H) { return (size_t)2 * 2 * plane_rows(B) * 3 * H * 2; }
inline size_t gru_carry_bytes(int B, int H) { return (size_t)2 * B * H * 4; }
inline int64_t gru_ws_bytes(int B, int H) {
    return (int64_t)gru_planes_bytes(B, H) + (int64_t)gru_carry_bytes(B, H) +
           (int64_t)2 * 3 * H * H * 2 + 256 + ctl_bytes(B);
}

// the persistent kernels address the hand-off planes through 32-bit buffer offsets
inline bool gru_persist_fits(int B, int H) { return gru_planes_bytes(B, H) < (1ull << 31); }

}  // namespace

extern "C" int64_t asr_gru_workspace_bytes(int B, int H) {
    if (B < 0 || H < 0) return -1;
    return gru_ws_bytes(B, H);
}

extern "C" int asr_gru_supported(int B, int H) {
    if (B <= 0 || !gru_built(H)) return 0;
    const int cus = cu_count();
    return 1 | (persist_enabled() && cus >= 2 * (H / 64) && gru_persist_fits(B, H) ? 2 : 0);
}

extern "C" int asr_gru_bidir_fwd_bf16(const void *gx, int gx_bf16, const void *whh_bf16,
                                      const int32_t *lens, int T, int B, int H,
                                      float *y, void *y_bf16, void *gates_bf16,
                                      void *workspace, int64_t workspace_bytes,
                                      uint32_t *err_flag, void *stream) {
    if (T < 0 || B <= 0 || H <= 0 || (H % 32) != 0 || gx_bf16 < 0 || gx_bf16 > 1) return ASR_EINVAL;
    if (!gx || !whh_bf16 || !lens || !y || !y_bf16 || !gates_bf16 || !workspace) return ASR_EINVAL;
    if (!gru_built(H)) return ASR_EUNSUPPORTED;
    if (workspace_bytes < gru_ws_bytes(B, H)) return ASR_EINVAL;
    if (T == 0) return ASR_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t pb = gru_planes_bytes(B, H), cb = gru_carry_bytes(B, H);
    __bf16 *wpack = (__bf16 *)((char *)workspace + pb + cb);
    unsigned *ctl_words = (unsigned *)((char *)workspace + gru_ws_bytes(B, H) - ctl_bytes(B));
    GruFwdParams p;
    p.gx = gx; p.gx_bf16 = gx_bf16; p.whh = wpack; p.lens = lens;
    p.T = T; p.B = B; p.H = H; p.rows = (size_t)plane_rows(B);
    p.hbuf = (__bf16 *)workspace;
    p.y = y; p.ybf = (__bf16 *)y_bf16; p.gates = (u32x2 *)gates_bf16; p.step = 0;
    ZeroList zl;
    zl.add(workspace, pb / 3);                      // the two h_t planes of both directions
    for (int d = 0; d < 2; ++d) {                   // the pad frames of y_bf16
        zl.add(p.ybf + (size_t)d * (T + 2) * B * H, (size_t)B * H * 2);
        zl.add(p.ybf + ((size_t)d * (T + 2) + T + 1) * B * H, (size_t)B * H * 2);
    }
    if (persist_enabled()) zl.add(ctl_words, (size_t)ctl_bytes(B));
    zl.launch(s);
    // [2 dir x 3 gates] matrices of H x H (rows = hidden unit, cols = k)
    hipLaunchKernelGGL(lstm_pack_kernel, dim3(1024), dim3(256), 0, s,
                       (const __bf16 *)whh_bf16, wpack, 6, H, H, 0);
    if (persist_enabled() && gru_persist_fits(B, H)) {
        void (*pk[3])(GruFwdParams, LstmTeamCtl) = {nullptr, nullptr, nullptr};
#define ASR_PICK(KSV) if (H == 16 * KSV) {                                                          \
        if (gx_bf16) { pk[0] = gru_fwd_persist_kernel<KSV, 2, 1>; pk[1] = gru_fwd_persist_kernel<KSV, 3, 1>; \
                       pk[2] = gru_fwd_persist_kernel<KSV, 4, 1>; }                                   \
        else { pk[0] = gru_fwd_persist_kernel<KSV, 2, 0>; pk[1] = gru_fwd_persist_kernel<KSV, 3, 0>;   \
               pk[2] = gru_fwd_persist_kernel<KSV, 4, 0>; } }
        ASR_PICK(4) ASR_PICK(8) ASR_PICK(16) ASR_PICK(20)
#undef ASR_PICK
        const size_t lds = (size_t)(H / 16) * 1024 + ASR_GRU_PART_BYTES + 4096;
        if (launch_persist(pk, p, B, H, lds, ctl_words, err_flag, s))
            return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
    }
    const dim3 grid(H / 32, (B + 31) / 32, 2);
    void (*kern)(GruFwdParams) = nullptr;
#define ASR_PICK(KSV) if (H == 16 * KSV) kern = gx_bf16 ? gru_fwd_step_kernel<KSV, 1> : gru_fwd_step_kernel<KSV, 0>;
    ASR_PICK(4) ASR_PICK(8) ASR_PICK(16) ASR_PICK(20)
#undef ASR_PICK
    if (!kern) return ASR_EUNSUPPORTED;
    for (int step = 0; step < T; ++step) {
        p.step = step;
        hipLaunchKernelGGL(kern, grid, dim3(192), 0, s, p);
    }
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}

extern "C" int asr_gru_bidir_bwd_bf16(const float *dy, int dy_shared, const void *whhT_bf16,
                                      const int32_t *lens, int T, int B, int H,
                                      const void *gates_bf16, const float *y,
                                      void *dgx_bf16, void *dhn_bf16,
                                      void *workspace, int64_t workspace_bytes,
                                      uint32_t *err_flag, void *stream) {
    if (T < 0 || B <= 0 || H <= 0 || (H % 32) != 0 || dy_shared < 0 || dy_shared > 1) return ASR_EINVAL;
    if (!dy || !whhT_bf16 || !lens || !gates_bf16 || !y || !dgx_bf16 || !dhn_bf16 || !workspace)
        return ASR_EINVAL;
    if (!gru_built(H)) return ASR_EUNSUPPORTED;
    if (workspace_bytes < gru_ws_bytes(B, H)) return ASR_EINVAL;
    if (T == 0) return ASR_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t pb = gru_planes_bytes(B, H), cb = gru_carry_bytes(B, H);
    __bf16 *wpack = (__bf16 *)((char *)workspace + pb + cb);
    unsigned *ctl_words = (unsigned *)((char *)workspace + gru_ws_bytes(B, H) - ctl_bytes(B));
    GruBwdParams p;
    p.dy = dy; p.dy_shared = dy_shared; p.whhT = wpack; p.lens = lens;
    p.T = T; p.B = B; p.H = H; p.rows = (size_t)plane_rows(B);
    p.gates = (const u32x2 *)gates_bf16; p.y = y;
    p.dgbuf = (__bf16 *)workspace;
    p.dcbuf = (float *)((char *)workspace + pb);
    p.dgx = (__bf16 *)dgx_bf16; p.dhn = (__bf16 *)dhn_bf16; p.step = 0;
    {
        ZeroList zl;
        zl.add(workspace, pb + cb);
        if (persist_enabled()) zl.add(ctl_words, (size_t)ctl_bytes(B));
        zl.launch(s);
    }
    // whhT_bf16 is [2][H][3H] row-major: rows = hidden unit j, cols = k over 3H
    hipLaunchKernelGGL(lstm_pack_kernel, dim3(1024), dim3(256), 0, s,
                       (const __bf16 *)whhT_bf16, wpack, 2, H, 3 * H, 0);
    if (persist_enabled() && gru_persist_fits(B, H)) {
        void (*pk[3])(GruBwdParams, LstmTeamCtl) = {nullptr, nullptr, nullptr};
#define ASR_PICK(KSV) if (H == 16 * KSV) { pk[0] = gru_bwd_persist_kernel<KSV, 2>; \
        pk[1] = gru_bwd_persist_kernel<KSV, 3>; pk[2] = gru_bwd_persist_kernel<KSV, 4>; }
        ASR_PICK(4) ASR_PICK(8) ASR_PICK(16) ASR_PICK(20)
#undef ASR_PICK
        const size_t lds = (size_t)(3 * H / 16) * 1024 + ASR_GRU_PART_BYTES + 3 * 4096;
        if (launch_persist(pk, p, B, H, lds, ctl_words, err_flag, s))
            return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
    }
    const dim3 grid(H / 32, (B + 31) / 32, 2);
    void (*kern)(GruBwdParams) = nullptr;
#define ASR_PICK(KSV) if (H == 16 * KSV) kern = gru_bwd_step_kernel<KSV>;
    ASR_PICK(4) ASR_PICK(8) ASR_PICK(16) ASR_PICK(20)
#undef ASR_PICK
    if (!kern) return ASR_EUNSUPPORTED;
    for (int step = 0; step < T; ++step) {
        p.step = step;
        hipLaunchKernelGGL(kern, grid, dim3(192), 0, s, p);
    }
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
