// Bidirectional LSTM recurrence (no bias) for gfx950 — the recurrent part of
// the reference's BatchRNN (att_speech/modules/encoders/encoder_utils.py:55-124:
// nn.LSTM(bidirectional=True, bias=False) on a packed batch).
//
// The input projection x_t·W_ihᵀ of all frames and both directions is one
// dense GEMM done by the caller; this file owns the sequential part:
//   gates_t = gx_t + h_{t-1}·W_hhᵀ ;  i,f,o = σ(.), g = tanh(.)
//   c_t = f·c_{t-1} + i·g ;  h_t = o·tanh(c_t)
// Two implementations of the same arithmetic (bit-identical outputs, see
// tests/test_lstm_gpu.py):
//   * PERSISTENT (default): one launch walks all T steps; a 512-thread workgroup
//     keeps its W_hh fragments and the cell state in registers for the whole
//     sequence and teams of H/64 workgroups hand h_t / dgates_t over through L2
//     once per step (sc1 write-through + agent-scope counters) — further down;
//   * PER-STEP (ASR_LSTM_PERSIST=0, and the fallback for shapes the persistent
//     kernels do not take): one launch per time step covering BOTH directions
//     (forward frame s, reverse frame T-1-s), grid 2·(B/32)·(H/32); a workgroup
//     owns a [32 batch x 32 hidden] tile, wave g computes the pre-activation of
//     gate g with v_mfma_f32_32x32x16_bf16 (K = H), operands read from L2 straight
//     in MFMA fragment order (W_hh is 0.8 MB per direction and stays L2-resident
//     across the steps), the four gate tiles meet in LDS for the fp32 cell update.
//
// MFMA operand layout: both GEMM operands live in memory in FRAGMENT-MAJOR
// order — for a [32 rows x K] tile, k-step ks is the 1 KiB block
// [64 lanes][8 bf16] with lane l = (row & 31) + 32*((k>>3)&1) — so a wave's
// fragment load is one fully coalesced 1 KiB access (a row-major tile makes
// every load touch 32 cache lines and the address coalescer, not the MFMA,
// sets the pace: measured 9k cycles just to ISSUE the 40 loads).  The h /
// dgates ping-pong buffers are written in that order by the pointwise phase;
// W_hh is re-packed once per call by lstm_pack_kernel.
//
// Packed-sequence semantics with a padded batch: utterance b is active at
// frame t iff t < lens[b]; inactive frames keep (h, c) and emit zeros, so the
// reverse direction starts from the zero state at each utterance's own last
// frame exactly like pack_padded_sequence does.
#include "common.h"
#include "../../include/asr_amd.h"
#include "recurrence.h"
#include <stdlib.h>

namespace {

// The cell update and its derivative, shared by the per-step and the persistent
// kernels.  Contraction is off so both kernels round identically (the tests
// compare them bit for bit to catch a stale hand-off).
__device__ __forceinline__ void lstm_cell_fwd(const float pre[4], float cprev, float gate[4],
                                              float &c, float &h) {
#pragma clang fp contract(off)
    gate[0] = sigmoidf_(pre[0]);
    gate[1] = sigmoidf_(pre[1]);
    gate[2] = tanhf_(pre[2]);
    gate[3] = sigmoidf_(pre[3]);
    c = gate[1] * cprev + gate[0] * gate[2];
    h = gate[3] * tanhf_(c);
}

// Two elements at a time: the multiplies and adds around the transcendentals as packed fp32
// operations (v_pk_mul_f32 / v_pk_add_f32), half the instructions; the same IEEE operations in
// the same order per element, so the results are bit for bit those of lstm_cell_fwd.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 sigmoid2_(f32x2 x) {
#pragma clang fp contract(off)
    const f32x2 t = x * -1.4426950408889634f;
    f32x2 e = {__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
    e = e + 1.f;
    return f32x2{__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
}
__device__ __forceinline__ f32x2 tanh2_(f32x2 x) {
#pragma clang fp contract(off)
    const f32x2 t = x * -2.8853900817779268f;
    f32x2 e = {__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
    e = e + 1.f;
    const f32x2 r = {__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
    return r * 2.f - 1.f;
}
__device__ __forceinline__ void lstm_cell_fwd2(const f32x2 pre[4], f32x2 cprev, f32x2 gate[4],
                                               f32x2 &c, f32x2 &h) {
#pragma clang fp contract(off)
    gate[0] = sigmoid2_(pre[0]);
    gate[1] = sigmoid2_(pre[1]);
    gate[2] = tanh2_(pre[2]);
    gate[3] = sigmoid2_(pre[3]);
    c = gate[1] * cprev + gate[0] * gate[2];
    h = gate[3] * tanh2_(c);
}

// dh: gradient reaching h_t; dcin: carried dL/dc_t from the later step; cs: c_t;
// cp: c_{t-1}.  d[] = pre-activation gate gradients (i, f, g, o).
__device__ __forceinline__ void lstm_cell_bwd(const float g[4], float cs, float cp, float dh,
                                              float dcin, float d[4], float &dcout) {
#pragma clang fp contract(off)
    const float gi = g[0], gf = g[1], gg = g[2], go = g[3];
    const float tc = tanhf_(cs);
    const float dc = dh * go * (1.f - tc * tc) + dcin;
    d[3] = dh * tc * go * (1.f - go);
    d[0] = dc * gg * gi * (1.f - gi);
    d[1] = dc * cp * gf * (1.f - gf);
    d[2] = dc * gi * (1.f - gg * gg);
    dcout = dc * gf;
}

// x·W_ih term: fp32, or the bf16 the input-projection GEMM emits (halves its 1.75 GB
// output at B=512 and this kernel's reads; fp32 accumulation either way)
template <int GXB>
__device__ __forceinline__ float load_gx(const void *gx, size_t i) {
    if constexpr (GXB) return (float)((const __bf16 *)gx)[i];
    else return ((const float *)gx)[i];
}

struct LstmFwdParams {
    const void *gx;         // [T,B,2,4H] x·W_ihᵀ, gate order i,f,g,o; float or (gx_bf16) __bf16
    int gx_bf16;
    const __bf16 *x;        // fused input projection (persistent kernel, F == H): x [T,B,H] bf16 row-major
    const __bf16 *wih;      // ... and the fragment-major pack of W_ih [2*4 (dir,gate)][H rows][F cols]
    const __bf16 *whh;      // fragment-major pack of [2*4 (dir,gate)][H rows][H cols]
    const int32_t *lens;    // [B]
    int T, B, H;
    __bf16 *hbuf;           // [2 pingpong][2 dir] fragment-major [Bp x H], Bp = B padded to 32
    float *cbuf;            // [2 dir][B][H]
    float *y;               // [T,B,2,H] per-direction outputs (zeros when inactive)
    __bf16 *ybf;            // [2,T+2,B,H] bf16 copy, frame t at index t+1 (zero frames at both ends)
    u32x2 *gates;           // [T,2,B,H] records of 4 bf16 post-activation gates (saved for backward)
    float *csave;           // [T,2,B,H] cell state after the step
    int step;
};

// K-loop of one wave: acc += A[32 x 16*KS] * B[16*KS x 32] with both operands
// read from global memory (L2) in MFMA fragment order.  With KS known at
// compile time the loop is fully unrolled and every fragment load is issued
// before the first MFMA, so the L2 latency is paid once, not per k-step.

// grid: x = hidden tile (H/32), y = batch tile (ceil(B/32)), z = direction
#ifdef ASR_LSTM_STAMPS
#define STAMP(i) stamp[i] = __builtin_amdgcn_s_memtime()
#else
#define STAMP(i) do {} while (0)
#endif

// One time step of the forward recurrence for a [32 batch] x [32 hidden]
// tile (all four gates).  KS = H/16 k-steps (compile time).  Wave g owns gate
// g: its W_hh fragments (KS x 16 B per lane) are loaded straight to registers,
// the h_{t-1} tile — needed by all four waves — is staged once through LDS.
template <int KS, int GXB>
__global__ __launch_bounds__(256) void lstm_fwd_step_kernel(LstmFwdParams p) {
#ifdef ASR_LSTM_STAMPS
    unsigned long long stamp[4];
    const unsigned long long stamp_start = __builtin_amdgcn_s_memtime();
#endif
    __shared__ __attribute__((aligned(16))) __bf16 a_lds[KS * 512];
    __shared__ float g_lds[4][32][33];
    const int H = p.H, B = p.B;
    const int j0 = blockIdx.x * 32, b0 = blockIdx.y * 32, dir = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = dir == 0 ? p.step : p.T - 1 - p.step;
    const int Bp = (B + 63) & ~63;
    const __bf16 *hprev = p.hbuf + ((size_t)(p.step & 1) * 2 + dir) * Bp * H;
    __bf16 *hnext = p.hbuf + ((size_t)((p.step + 1) & 1) * 2 + dir) * Bp * H;

    // ---- W_hh fragments of this wave's gate (vmcnt retires in order: keep the
    // L2-resident operand loads ahead of the HBM loads of the pointwise phase)
    bf16x8 fb[KS];
    {
        const __bf16 *bp = p.whh + ((size_t)(dir * 4 + wave) * H * H) +
                           ((size_t)blockIdx.x * KS * 64 + lane) * 8;
#pragma unroll
        for (int k = 0; k < KS; ++k) fb[k] = *reinterpret_cast<const bf16x8 *>(bp + k * 512);
    }
    // ---- h_{t-1} tile: KS KiB, contiguous in fragment-major order
    {
        const bf16x8 *src = reinterpret_cast<const bf16x8 *>(
            hprev + (size_t)blockIdx.y * KS * 512);
        bf16x8 *dst = reinterpret_cast<bf16x8 *>(a_lds);
        constexpr int CH = KS * 64;                 // 16-byte chunks
        bf16x8 tmp[(CH + 255) / 256];
#pragma unroll
        for (int i = 0; i < (CH + 255) / 256; ++i) {
            const int c = i * 256 + threadIdx.x;
            if (c < CH) tmp[i] = src[c];
        }
#pragma unroll
        for (int i = 0; i < (CH + 255) / 256; ++i) {
            const int c = i * 256 + threadIdx.x;
            if (c < CH) dst[c] = tmp[i];
        }
    }
    STAMP(0);

    // ---- operands of the pointwise phase: issued now, consumed after the GEMM
    constexpr int NE = 4;
    float pgx[NE][4], pc[NE];
    bool pact[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int idx = e * 256 + threadIdx.x;
        const int b = b0 + (idx >> 5), j = j0 + (idx & 31);
        const int bc = b < B ? b : B - 1;
        pact[e] = b < B && t < p.lens[bc];
        const size_t gxo = (((size_t)t * B + bc) * 2 + dir) * 4 * H + j;
#pragma unroll
        for (int g = 0; g < 4; ++g) pgx[e][g] = load_gx<GXB>(p.gx, gxo + (size_t)g * H);
        pc[e] = p.cbuf[((size_t)dir * B + bc) * H + j];
    }
    __syncthreads();

    // ---- gate pre-activation tiles
    {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        const bf16x8 *al = reinterpret_cast<const bf16x8 *>(a_lds) + lane;
#pragma unroll
        for (int k = 0; k < KS; ++k)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[k * 64], fb[k], acc, 0, 0, 0);
        STAMP(1);
        const int col = lane & 31;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
            g_lds[wave][row][col] = acc[i];
        }
    }
    __syncthreads();
    STAMP(2);

    // ---- pointwise cell update: 1024 (b, j) elements over 256 threads
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int idx = e * 256 + threadIdx.x;
        const int row = idx >> 5, col = idx & 31;
        const int b = b0 + row, j = j0 + col;
        if (b < B) {
            const size_t sidx = ((size_t)dir * B + b) * H + j;
            float *yo = p.y + (((size_t)t * B + b) * 2 + dir) * H + j;
            __bf16 *ybo = p.ybf + (((size_t)dir * (p.T + 2) + t + 1) * B + b) * H + j;
            const size_t csv = (((size_t)t * 2 + dir) * B + b) * H + j;
            if (pact[e]) {
                float pre[4], gt[4], c, h;
#pragma unroll
                for (int g = 0; g < 4; ++g) pre[g] = g_lds[g][row][col] + pgx[e][g];
                lstm_cell_fwd(pre, pc[e], gt, c, h);
                p.cbuf[sidx] = c;
                hnext[frag_off(b, j, KS)] = (__bf16)h;
                if (p.y) *yo = h;
                *ybo = (__bf16)h;
                p.gates[csv] = pack_gates(gt);
                p.csave[csv] = c;
            } else {
                hnext[frag_off(b, j, KS)] = hprev[frag_off(b, j, KS)];
                if (p.y) *yo = 0.f;
                *ybo = (__bf16)0.f;
                p.csave[csv] = pc[e];
            }
        }
    }
    STAMP(3);
#ifdef ASR_LSTM_STAMPS
    __syncthreads();
    if (threadIdx.x == 0 && b0 < B) {
        float *o = p.y + (((size_t)t * B + b0) * 2 + dir) * H + j0;
        o[0] = (float)(stamp[0] - stamp_start);
        for (int i = 1; i < 4; ++i) o[i] = (float)(stamp[i] - stamp[i - 1]);
    }
#endif
}

struct LstmBwdParams {
    const float *dy;        // [T,B,2,H] gradient w.r.t. the per-direction outputs, or [T,B,H]
    int dy_shared;          // 1: one gradient for both directions (the directions are summed)
    const __bf16 *whhT;     // fragment-major pack of W_hhᵀ: [2 dir][H rows][4H cols]
    const int32_t *lens;
    int T, B, H;
    const u32x2 *gates;     // [T,2,B,H] records of 4 bf16 (i,f,g,o)
    const float *csave;     // [T,2,B,H]
    __bf16 *dgbuf;          // [2 pingpong][2 dir] fragment-major [Bp x 4H]: dgates of the previous step
    float *dcbuf;           // [2 dir][B][H] carried dL/dc
    __bf16 *dgates;         // [T,B,2,4H] pre-activation gate gradients (output, bf16: GEMM operand)
    int step;
};

// One time step of the backward recurrence for a [32 batch] x [32 hidden]
// tile: dh_rec[b][j] = sum_k dgates_prev[b][k] * W_hh[k][j] with K = 4H split
// over the four waves (wave w takes the columns of gate w), then the LSTM cell
// backward in fp32.
template <int KS>
__global__ __launch_bounds__(256) void lstm_bwd_step_kernel(LstmBwdParams p) {
    __shared__ float part[4][32][33];
    const int H = p.H, B = p.B, H4 = 4 * p.H;
    const int j0 = blockIdx.x * 32, b0 = blockIdx.y * 32, dir = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // the backward scan visits frames in the opposite order of the forward one
    const int t = dir == 0 ? p.T - 1 - p.step : p.step;
    const int Bp = (B + 63) & ~63;
    constexpr int KS4 = 4 * KS;
    const __bf16 *dgprev = p.dgbuf + ((size_t)(p.step & 1) * 2 + dir) * Bp * H4;
    __bf16 *dgnext = p.dgbuf + ((size_t)((p.step + 1) & 1) * 2 + dir) * Bp * H4;

    // ---- operands: W_hhᵀ slice of this wave (registers) and the dgates tile
    bf16x8 fb[KS], fa[KS];
    {
        const __bf16 *bp = p.whhT + (size_t)dir * H * H4 +
                           (((size_t)blockIdx.x * KS4 + (size_t)wave * KS) * 64 + lane) * 8;
#pragma unroll
        for (int k = 0; k < KS; ++k) fb[k] = *reinterpret_cast<const bf16x8 *>(bp + k * 512);
        const __bf16 *ap = dgprev + (((size_t)blockIdx.y * KS4 + (size_t)wave * KS) * 64 + lane) * 8;
#pragma unroll
        for (int k = 0; k < KS; ++k) fa[k] = *reinterpret_cast<const bf16x8 *>(ap + k * 512);
    }

    // ---- operands of the pointwise phase: issued now, consumed after the GEMM
    constexpr int NE = 4;
    float pg[NE][4], pcs[NE], pcp[NE], pdy[NE], pdc[NE];
    bool pact[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int idx = e * 256 + threadIdx.x;
        const int b = b0 + (idx >> 5), j = j0 + (idx & 31);
        const int bc = b < B ? b : B - 1;
        const int len = p.lens[bc];
        pact[e] = b < B && t < len;
        unpack_gates(p.gates[(((size_t)t * 2 + dir) * B + bc) * H + j], pg[e]);
        pcs[e] = p.csave[(((size_t)t * 2 + dir) * B + bc) * H + j];
        const int tp = dir == 0 ? t - 1 : t + 1;
        const int tpc = tp < 0 ? 0 : (tp >= p.T ? p.T - 1 : tp);
        const float cpv = p.csave[(((size_t)tpc * 2 + dir) * B + bc) * H + j];
        pcp[e] = (tp >= 0 && tp < len) ? cpv : 0.f;
        pdy[e] = p.dy[p.dy_shared ? ((size_t)t * B + bc) * H + j : (((size_t)t * B + bc) * 2 + dir) * H + j];
        pdc[e] = p.dcbuf[((size_t)dir * B + bc) * H + j];
    }

    {
        const int col = lane & 31;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int k = 0; k < KS; ++k)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[k], fb[k], acc, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
            part[wave][row][col] = acc[i];
        }
    }
    __syncthreads();

#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int idx = e * 256 + threadIdx.x;
        const int row = idx >> 5, col = idx & 31;
        const int b = b0 + row, j = j0 + col;
        if (b < B) {
            const size_t sidx = ((size_t)dir * B + b) * H + j;
            __bf16 *dgo = p.dgates + (((size_t)t * B + b) * 2 + dir) * H4 + j;
            if (pact[e]) {
                const float dh = pdy[e] + (part[0][row][col] + part[1][row][col]) +
                                 (part[2][row][col] + part[3][row][col]);
                float d[4], dcout;
                lstm_cell_bwd(pg[e], pcs[e], pcp[e], dh, pdc[e], d, dcout);   // pcp: cell state the step started from
                const float d_i = d[0], d_f = d[1], d_g = d[2], d_o = d[3];
                p.dcbuf[sidx] = dcout;
                dgo[0] = (__bf16)d_i; dgo[H] = (__bf16)d_f;
                dgo[2 * H] = (__bf16)d_g; dgo[3 * H] = (__bf16)d_o;
                dgnext[frag_off(b, j, KS4)] = (__bf16)d_i;
                dgnext[frag_off(b, H + j, KS4)] = (__bf16)d_f;
                dgnext[frag_off(b, 2 * H + j, KS4)] = (__bf16)d_g;
                dgnext[frag_off(b, 3 * H + j, KS4)] = (__bf16)d_o;
            } else {
                // no gradient reaches a padding frame; the carried state gradient
                // restarts from zero (forward: beyond the end; reverse: before the start)
                p.dcbuf[sidx] = 0.f;
                dgo[0] = (__bf16)0.f; dgo[H] = (__bf16)0.f;
                dgo[2 * H] = (__bf16)0.f; dgo[3 * H] = (__bf16)0.f;
                dgnext[frag_off(b, j, KS4)] = (__bf16)0.f;
                dgnext[frag_off(b, H + j, KS4)] = (__bf16)0.f;
                dgnext[frag_off(b, 2 * H + j, KS4)] = (__bf16)0.f;
                dgnext[frag_off(b, 3 * H + j, KS4)] = (__bf16)0.f;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Persistent recurrence: ONE launch walks all T steps.  A workgroup (512
// threads) owns a [32 batch x 64 hidden] tile for the whole sequence: its W_hh
// fragments (KS x 16 B per lane per wave) and the cell state never leave
// registers; only h_t (forward) / dgates_t (backward) crosses workgroups, once
// per step, inside a TEAM = the H/64 workgroups of one (direction, batch tile).
// Hand-off (MI355X_MICROARCH.md § visibility, sc1 table rows 1/3): the tile is
// staged in LDS in fragment order and stored as whole 1 KiB blocks, one
// `buffer_store_dwordx4 sc1` (write-through) per wave; every wave drains
// vmcnt(0), the workgroup meets at a barrier, ONE lane adds 1 to the team
// counter (agent scope); consumers poll that counter with an sc1 load from one
// lane, pass a workgroup barrier, then read the tile with `buffer_load_dwordx4
// sc1` only.  The grid never exceeds one workgroup per CU (LDS request > 80 KiB
// and grid <= #CUs, the batch is cut into several launches if needed), so every
// team mate is resident; every spin is bounded and a timeout poisons the
// outputs with NaN instead of hanging.

#ifdef ASR_LSTM_STAMPS
#define PSTAMP_DECL unsigned long long pst[6] = {0, 0, 0, 0, 0, 0}, plast = __builtin_amdgcn_s_memtime()
#define PSTAMP(i) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
                       pst[i] += now_ - plast; plast = now_; } while (0)
#else
#define PSTAMP_DECL do {} while (0)
#define PSTAMP(i) do {} while (0)
#endif

// LDS-DMA: 64 lanes x 16 bytes from a bounds-checked raw buffer straight to LDS at
// `lds_byte` + lane * 16 (out-of-range lanes write zeros).  Inline asm: hipcc would order
// every later LDS read behind it with s_waitcnt vmcnt(0) (cdna_hip_programming.md §5.7);
// the kernel waits where it needs the data.
typedef __attribute__((ext_vector_type(4))) int rsrc_words;
__device__ __forceinline__ rsrc_words raw_rsrc(const void *base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    rsrc_words r;            // (readfirstlane: the descriptor must sit in SGPRs for the asm)
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
    r.y = __builtin_amdgcn_readfirstlane((int)((unsigned)(a >> 32) & 0xffffu));
    r.z = __builtin_amdgcn_readfirstlane((int)bytes);
    r.w = 0x00020000;
    return r;
}
__device__ __forceinline__ void dma16_s(rsrc_words r, unsigned lds_byte, unsigned voff, unsigned soff) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
                 "buffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "s"(lds_byte), "v"(voff), "s"(r), "s"(soff)
                 : "memory");
}
__device__ __forceinline__ void dma16_sc1(rsrc_words r, unsigned lds_byte, unsigned voff, unsigned soff) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t"
                 "buffer_load_dwordx4 %2, %3, %4 offen sc1 lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "s"(lds_byte), "v"(voff), "s"(r), "s"(soff)
                 : "memory");
}
__device__ __forceinline__ unsigned lds_addr(const void *ptr) {
    return (unsigned)(size_t)((__attribute__((address_space(3))) const void *)ptr);
}

#define ASR_GLDS_BYTES (4 * 32 * 65 * 4)

// NE = batch rows of the tile / 8 (tiles of 16, 24 or 32 rows: fewer rows per workgroup
// = more workgroups; the host picks the smallest tile whose grid still fits one
// workgroup per CU).  Rows >= 8*NE of the 32-row MFMA tile are padding.
//
// XF > 0 (= the input size F / 16: the projection's k-steps) fuses the input projection: instead of reading x·W_ihᵀ (`gx`, the output of a
// [T·B, F] x [F, 8H] library GEMM: 0.37 ms and 2 GB of HBM traffic per layer at B=576) the
// workgroup keeps its W_ih slice in registers next to W_hh (F == H, or the first layer's
// F = 352 behind the conv front-end: 22 k-steps) and multiplies the x_t
// tile itself — x_t does not depend on the recurrence, so waves 4-7 do it while the
// workgroup waits for the team's counter and waves 0-3 while the hand-off tile is in
// flight: both windows (911 / 1036 cycles at B=512) were idle.  The sum x_t·W_ih + h·W_hh
// is accumulated in fp32 in one MFMA chain (the bf16 rounding of `gx` is gone).
template <int KS, int NE, int GXB, int XF>
__global__ __launch_bounds__(512) void lstm_fwd_persist_kernel(LstmFwdParams p, LstmTeamCtl ctl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __bf16 *a_lds = reinterpret_cast<__bf16 *>(smem);                       // KS KiB
    float (*g_lds)[32][65] = reinterpret_cast<float (*)[32][65]>(smem + KS * 1024);
    __bf16 *h_lds = reinterpret_cast<__bf16 *>(smem + KS * 1024 + ASR_GLDS_BYTES);   // 4 KiB
    __bf16 *x_lds = reinterpret_cast<__bf16 *>(smem + KS * 1024 + ASR_GLDS_BYTES + 4096);   // XF KiB
    constexpr int KX = XF > 0 ? XF : 1;
    __shared__ int dead_s;
    const int H = p.H, B = p.B, T = p.T;
    int jt = blockIdx.x, btile = blockIdx.y + ctl.bt0, dir = blockIdx.z;
    if (ctl.xcd_teams) {
        // 1-D grid, team = blockIdx.x % 8 + 8 * (slot / njt): the H/64 workgroups that
        // exchange h_t / dgates_t every step have equal blockIdx % 8, i.e. sit on one XCD
        // under the observed round-robin placement (speed only — the hand-off protocol
        // does not depend on it); surplus workgroups of the padded grid leave at once
        const int slot = blockIdx.x >> 3, team = (slot / (p.H / 64)) * 8 + (blockIdx.x & 7);
        if (team >= ctl.xcd_teams) return;
        jt = slot % (p.H / 64);
        btile = (team >> 1) + ctl.bt0;
        dir = team & 1;
    }
    const int j0 = jt * 64, b0 = btile * (8 * NE), njt = H / 64;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int gate = wave >> 1, js = wave & 1;
    const size_t Bp = ctl.rows;              // rows of an hbuf / dgbuf plane (32 per batch tile)
    unsigned *myctr = ctl.ctr + ((size_t)dir * ctl.nbt + btile) * 32;
    if (tid == 0) dead_s = 0;
    for (int i = tid; i < 2048; i += 512) h_lds[i] = (__bf16)0.f;       // padding rows stay 0
    for (int i = tid; i < KS * 64; i += 512)                            // (the tile's too: never loaded)
        reinterpret_cast<u32x4 *>(a_lds)[i] = u32x4{0u, 0u, 0u, 0u};
    if constexpr (XF)
        for (int i = tid; i < KX * 64; i += 512)
            reinterpret_cast<u32x4 *>(x_lds)[i] = u32x4{0u, 0u, 0u, 0u};

    bf16x8 fb[KS], fx[KX];
    {
        const size_t wo = ((size_t)(dir * 4 + gate) * H * H) + ((size_t)(2 * jt + js) * KS * 64 + lane) * 8;
#pragma unroll
        for (int k = 0; k < KS; ++k) fb[k] = *reinterpret_cast<const bf16x8 *>(p.whh + wo + k * 512);
        if constexpr (XF) {       // W_ih pack: [2*4][H rows][16*KX cols], fragment-major
            const size_t wox = ((size_t)(dir * 4 + gate) * H * (16 * KX)) + ((size_t)(2 * jt + js) * KX * 64 + lane) * 8;
#pragma unroll
            for (int k = 0; k < KX; ++k) fx[k] = *reinterpret_cast<const bf16x8 *>(p.wih + wox + k * 512);
        }
    }
    const __amdgpu_buffer_rsrc_t hres = __builtin_amdgcn_make_buffer_rsrc(
        p.hbuf, 0, (int)(2 * 2 * Bp * H * 2), 0x00020000);
    const rsrc_words hresD = raw_rsrc(p.hbuf, (unsigned)(2 * 2 * Bp * H * 2));

    // the thread's four (row, col) elements: row = e*8 + wave, col = lane
    const int col = lane;
    float c[NE];
    __bf16 hq[NE];
    int len[NE];
    // Every per-step global access of the pointwise part goes through a raw buffer: the
    // lane's column as the only per-lane offset (4, 2 or 8 bytes per column), the row and
    // frame parts — wave-uniform: a wave's rows are b0 + 8 e + wave — in SGPRs; no 64-bit
    // address arithmetic in the step loop, and masked rows simply carry an out-of-range lane
    // offset (stores dropped).  The host checks every tensor is < 4 GiB.
    typedef unsigned int u32;
    constexpr u32 OOBV = 0xFFFFFFFFu;
    constexpr u32 GXE = GXB ? 2u : 4u;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const u32 l4 = (u32)col * 4u, l2 = (u32)col * 2u;
    u32 sgx[NE], sy[NE], syb[NE], scs[NE];     // row parts (bytes); gate records: 2 * scs
    bool inb[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int b = b0 + e * 8 + wv;
        const int bc = b < B ? b : B - 1;
        inb[e] = b < B;
        c[e] = 0.f;
        hq[e] = (__bf16)0.f;
        len[e] = __builtin_amdgcn_readfirstlane(b < B ? p.lens[bc] : 0);
        sgx[e] = (u32)((bc * 2 + dir) * 4 * H + j0) * GXE;
        sy[e] = (u32)((b * 2 + dir) * H + j0) * 4u;
        syb[e] = (u32)(((size_t)(dir * (T + 2) + 1) * B + b) * H + j0) * 2u;
        scs[e] = (u32)((dir * B + b) * H + j0) * 4u;
    }
    const u32 fgx = (u32)B * 8u * H * GXE, fy = (u32)B * 2u * H * 4u, fyb = (u32)B * H * 2u;
    const u32 fcs = (u32)B * 2u * H * 4u, fg = (u32)B * 2u * H * 8u;
    const __amdgpu_buffer_rsrc_t gxR = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void *>(p.gx), 0, XF ? 0 : (int)((u32)T * fgx), 0x00020000);
    // XF: the x_t tile goes global -> LDS by LDS-DMA, no registers: the 1 KiB A fragment of
    // k-step k is lane-linear in LDS (lane = row + 32 * k-half, 16 bytes each), which is
    // exactly the destination pattern of one `buffer_load_dwordx4 ... lds`; lanes of the
    // tile's padding rows carry an out-of-range offset and write zeros.  Wave w moves
    // k-steps w, w + 8, w + 16.
    const rsrc_words xD = raw_rsrc(p.x, XF ? (unsigned)((u32)T * B * (16 * KX) * 2u) : 0u);
    const u32 fx_frame = (u32)B * (16 * KX) * 2u;
    u32 vx = 0x80000000u;
    if constexpr (XF) {
        const int xr = lane & 31, b = b0 + xr < B ? b0 + xr : B - 1;
        if (xr < 8 * NE) vx = (u32)(b * (16 * KX) + 16 * wv + 8 * (lane >> 5)) * 2u;
    }
    auto x_dma = [&](int tq) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (wave + 8 * i < KX)
                dma16_s(xD, (unsigned)__builtin_amdgcn_readfirstlane(
                                (int)(lds_addr(x_lds) + (unsigned)(wave + 8 * i) * 1024u)),
                        vx + (u32)i * 256u, (u32)__builtin_amdgcn_readfirstlane((int)((u32)tq * fx_frame)));
    };
    // y == null: zero records, every fp32 output store is dropped by the bounds check
    const __amdgpu_buffer_rsrc_t yR = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, p.y ? (int)((u32)T * fy) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t ybR = __builtin_amdgcn_make_buffer_rsrc(
        p.ybf, 0, (int)((u32)(2 * (T + 2)) * fyb), 0x00020000);
    const __amdgpu_buffer_rsrc_t csR = __builtin_amdgcn_make_buffer_rsrc(p.csave, 0, (int)((u32)T * fcs), 0x00020000);
    const __amdgpu_buffer_rsrc_t gR = __builtin_amdgcn_make_buffer_rsrc(p.gates, 0, (int)((u32)T * fg), 0x00020000);
    auto ld_gx = [&](u32 voff, u32 soff) -> float {
        if constexpr (GXB)
            return (float)__builtin_bit_cast(__bf16, (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(gxR, voff, soff, 0));
        else
            return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(gxR, voff, soff, 0));
    };

    // Software pipeline: the x·W_ih terms of step s+1 are fetched during step s
    // (behind the hand-off tile in the wave's in-order vmcnt queue, never in
    // front of the team poll); the outputs nobody inside the launch reads are
    // stored after the team signal, under the hand-off latency.
    float pgx[XF ? 1 : NE][4];
    {
        const int t0 = dir == 0 ? 0 : T - 1;
        if constexpr (XF) {
            __syncthreads();            // the zero fill above
            x_dma(t0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        } else {
#pragma unroll
            for (int e = 0; e < NE; ++e)
#pragma unroll
                for (int g = 0; g < 4; ++g) pgx[e][g] = ld_gx((u32)col * GXE, sgx[e] + (u32)t0 * fgx + (u32)g * H * GXE);
        }
    }
    // A fragments in flight (registers are short with two weight slices: read one k-step ahead
    // there — one by one the chain pays the LDS latency per MFMA, 3x the window it has to fit).
    // The first layer's variant (22 input k-steps) writes no fp32 y: it is never the last layer
    // of a stack.
    constexpr int AD = XF ? 2 : 4;
    constexpr bool NOY = XF > KS;
    f32x16 accx;                 // XF: x_t · W_ih of this wave's (gate, column half)
    auto x_mfma = [&]() {
#pragma unroll
        for (int i = 0; i < 16; ++i) accx[i] = 0.f;
        const bf16x8 *xl = reinterpret_cast<const bf16x8 *>(x_lds) + lane;
        if constexpr (XF) accx = mfma_chain<0, KX, AD>(xl, fx, accx);
    };
    u32x2 sog[NE] = {};
    float soh[NE] = {}, sc[NE] = {};
    __bf16 shq[NE] = {};                 // NOY: the bf16 output of the step (0 on padding frames)
    bool sact[NE] = {};
    int st = 0;
    // live == false (the first step has nothing to store yet): every offset out of range,
    // so the call has the same VMEM count on every step (counted vmcnt waits around it)
    auto bulk_store = [&](bool live) {
        const u32 ust = (u32)st;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const bool on = live && inb[e];
            if constexpr (!NOY)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, soh[e]), yR,
                                                      on ? l4 : OOBV, ust * fy + sy[e], 0);
            __builtin_amdgcn_raw_buffer_store_b16(
                (short)__builtin_bit_cast(unsigned short, NOY ? shq[e] : (__bf16)soh[e]), ybR,
                on ? l2 : OOBV, ust * fyb + syb[e], 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, sc[e]), csR,
                                                  on ? l4 : OOBV, ust * fcs + scs[e], 0);
            __builtin_amdgcn_raw_buffer_store_b64(sog[e], gR,
                                                  on && sact[e] ? l4 * 2u : OOBV, ust * fg + scs[e] * 2u, 0);
        }
    };
    if constexpr (XF) {
        // Everything the prologue loaded must have landed BEFORE the loop: the compiler does
        // not see the LDS-DMA inside the asm, so a wait it places inside the loop for one of
        // these (first use of a weight fragment / a length) is counted without them and
        // degenerates to vmcnt(0) right behind the x_{t+1} DMA — the MFMA phase then waits
        // for the DMA (measured: 1992 -> 4091 cycles).  Naming the registers as asm operands
        // makes it wait here.
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            asm volatile("" : "+v"(fb[k]));
        }
#pragma unroll
        for (int k = 0; k < KX; ++k) asm volatile("" : "+v"(fx[k]));
#pragma unroll
        for (int e = 0; e < NE; ++e) asm volatile("" : "+v"(len[e]));
    }
    PSTAMP_DECL;
    for (int step = 0; step < T; ++step) {
        const int t = dir == 0 ? step : T - 1 - step;
        if constexpr (XF) if (wave >= 4) x_mfma();          // under the team wait
        if (step > 0 && tid == 0 && !dead_s) {
            if (!team_wait(myctr, (unsigned)(njt * step), ctl.spin_limit, ctl.err)) dead_s = 1;
        }
        PSTAMP(0);
        __syncthreads();
        // ---- h_{t-1} tile of the team: the KS - 4 KiB of the OTHER workgroups come over
        // sc1 loads; this workgroup's own 4 KiB are still in h_lds (staged there for the
        // store of the previous step: the same bytes) and are copied LDS -> LDS
        // (only the 2 * 8*NE chunks of a k-step that carry real batch rows move; the
        // padding rows of the 32-row MFMA tile stay zero in LDS)
        constexpr int RL = 8 * NE, CPK = 2 * RL;
        constexpr int CHO = (KS - 4) * CPK, NI = XF ? 0 : (CHO + 511) / 512;
        u32x4 tmp[NI > 0 ? NI : 1];
        if constexpr (XF) {
            // with two weight slices in registers there is none left to stage the tile in: it
            // comes global -> LDS by LDS-DMA (the hand-off buffer is fragment-major, 1 KiB per
            // k-step, lane-linear on both sides; padding rows read out of range = zeros)
            const unsigned base = (unsigned)((((size_t)(step & 1) * 2 + dir) * Bp * H +
                                              (size_t)btile * KS * 512) * 2);
            const u32 voffT = (lane & 31) < RL ? (u32)lane * 16u : 0x80000000u;
            for (int ko = wv; ko < KS - 4; ko += 8) {
                const int kk = ko < 4 * jt ? ko : ko + 4;
                dma16_sc1(hresD, (unsigned)__builtin_amdgcn_readfirstlane((int)(lds_addr(a_lds) + (unsigned)kk * 1024u)),
                          voffT, (unsigned)__builtin_amdgcn_readfirstlane((int)(base + (unsigned)kk * 1024u)));
            }
        }
        if constexpr (NI > 0) {
            const unsigned base = (unsigned)((((size_t)(step & 1) * 2 + dir) * Bp * H +
                                              (size_t)btile * KS * 512) * 2);
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int co = i * 512 + tid;       // lanes past the tile re-read its last chunk
                const int cc = co < CHO ? co : CHO - 1;
                const int ko = cc / CPK, q = cc - ko * CPK, k = ko < 4 * jt ? ko : ko + 4;
                tmp[i] = __builtin_amdgcn_raw_buffer_load_b128(
                    hres, base + (k * 64 + (q < RL ? q : q + (32 - RL))) * 16, 0, ASR_SC1);
            }
        }
        if (tid < 256)
            reinterpret_cast<u32x4 *>(a_lds)[(4 * jt + (tid >> 6)) * 64 + (tid & 63)] =
                reinterpret_cast<const u32x4 *>(h_lds)[tid];
        if constexpr (XF) {
            if (wave < 4) x_mfma();                         // under the hand-off tile's flight
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the tile
        }
        if constexpr (NI > 0) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int co = i * 512 + tid;
                const int ko = co / CPK, q = co - ko * CPK, k = ko < 4 * jt ? ko : ko + 4;
                if (co < CHO)
                    reinterpret_cast<u32x4 *>(a_lds)[k * 64 + (q < RL ? q : q + (32 - RL))] = tmp[i];
            }
        }
        __syncthreads();
        PSTAMP(1);
        float ngx[XF ? 1 : NE][4];
        {
            const int sn = step + 1 < T ? step + 1 : step;
            const int tn = dir == 0 ? sn : T - 1 - sn;
            if constexpr (XF) {
                // x_{t+1}: every read of x_lds for this step lies before the tile barrier above;
                // landed at the s_waitcnt vmcnt(0) in front of the signal barrier below
                // (32-row tiles keep two weight fragments in scratch; their reloads inside the
                // MFMA loop would wait for this DMA: issued behind the loop there)
                if constexpr (NE < 4) x_dma(tn);
            } else {
#pragma unroll
                for (int e = 0; e < NE; ++e)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        ngx[e][g] = ld_gx((u32)col * GXE, sgx[e] + (u32)tn * fgx + (u32)g * H * GXE);
            }
        }
        {
            f32x16 acc;
            if constexpr (XF) acc = accx;
            else {
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            }
            const bf16x8 *al = reinterpret_cast<const bf16x8 *>(a_lds) + lane;
            acc = mfma_chain<0, KS, AD>(al, fb, acc);
            const int c32 = lane & 31;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                g_lds[gate][row][js * 32 + c32] = acc[i];
            }
        }
        if constexpr (XF && NE == 4) {
            const int sn = step + 1 < T ? step + 1 : step;
            x_dma(dir == 0 ? sn : T - 1 - sn);
        }
        __syncthreads();
        PSTAMP(2);
        const bool dead = dead_s != 0;
        st = t;
        auto cell_one = [&](int e) {
            const int row = e * 8 + wave;
            if (sact[e]) {
                float pre[4], cn, og[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) pre[g] = XF ? g_lds[g][row][col] : g_lds[g][row][col] + pgx[XF ? 0 : e][g];
                lstm_cell_fwd(pre, c[e], og, cn, soh[e]);
                sog[e] = pack_gates(og);
                c[e] = cn;
                if (dead) soh[e] = __builtin_nanf("");
                hq[e] = (__bf16)soh[e];
                shq[e] = hq[e];
            } else {
                soh[e] = 0.f;
                shq[e] = (__bf16)0.f;
            }
        };
#pragma unroll
        for (int e = 0; e < NE; ++e) sact[e] = t < len[e];
#pragma unroll
        for (int e = 0; e < NE; e += 2) {
            if (e + 1 < NE && sact[e] && sact[e + 1]) {       // (lengths are wave-uniform)
                const int row = e * 8 + wave;
                f32x2 pre[4], cn, hn, og[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    pre[g] = f32x2{g_lds[g][row][col], g_lds[g][row + 8][col]};
                    if constexpr (!XF) pre[g] = pre[g] + f32x2{pgx[XF ? 0 : e][g], pgx[XF ? 0 : e + 1][g]};
                }
                lstm_cell_fwd2(pre, f32x2{c[e], c[e + 1]}, og, cn, hn);
                const float og0[4] = {og[0].x, og[1].x, og[2].x, og[3].x}, og1[4] = {og[0].y, og[1].y, og[2].y, og[3].y};
                sog[e] = pack_gates(og0);
                sog[e + 1] = pack_gates(og1);
                c[e] = cn.x; c[e + 1] = cn.y;
                soh[e] = dead ? __builtin_nanf("") : hn.x;
                soh[e + 1] = dead ? __builtin_nanf("") : hn.y;
                hq[e] = (__bf16)soh[e]; hq[e + 1] = (__bf16)soh[e + 1];
                shq[e] = hq[e]; shq[e + 1] = hq[e + 1];
            } else {
                cell_one(e);
                if (e + 1 < NE) cell_one(e + 1);
            }
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int row = e * 8 + wave;
            sc[e] = c[e];
            h_lds[(((col >> 4) * 64) + row + 32 * ((col >> 3) & 1)) * 8 + (col & 7)] = hq[e];
        }
        __syncthreads();
        if (wave < 4) {
            const u32x4 v = reinterpret_cast<const u32x4 *>(h_lds)[wave * 64 + lane];
            const unsigned off = (unsigned)(((((size_t)((step + 1) & 1) * 2 + dir) * Bp * H) +
                                             ((size_t)btile * KS + 4 * jt + wave) * 512 + lane * 8) * 2);
            // padding rows are not handed over (nobody loads them)
            __builtin_amdgcn_raw_buffer_store_b128(v, hres, (lane & 31) < 8 * NE ? off : 0xFFFFFFFFu,
                                                   0, ASR_SC1);
        }
        PSTAMP(3);
        // outputs nobody inside this launch reads: issued BEHIND the hand-off store and not
        // waited for — the counted wait retires everything up to the hand-off store (VMEM
        // retires in issue order), so its write-through latency (613 cycles of pure waiting)
        // runs under the issue of these stores.  (Issuing them behind the NEXT step's tile
        // loads instead, as the backward kernel does, was measured 1 % slower here.)
        bulk_store(true);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NOY ? 3 : 4) * NE) : "memory");
        __syncthreads();
        PSTAMP(4);
        if (tid == 0) __hip_atomic_fetch_add(myctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (!XF) {
#pragma unroll
            for (int e = 0; e < NE; ++e)
#pragma unroll
                for (int g = 0; g < 4; ++g) pgx[e][g] = ngx[e][g];
        }
        PSTAMP(5);
    }
#ifdef ASR_LSTM_STAMPS
    __syncthreads();
    if (tid == 0 && b0 < B)
        for (int i = 0; i < 6; ++i) p.y[(((size_t)0 * B + b0) * 2 + dir) * H + j0 + i] = (float)pst[i] / T;
#endif
}

template <int KS, int NE>
__global__ __launch_bounds__(512) void lstm_bwd_persist_kernel(LstmBwdParams p, LstmTeamCtl ctl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int KS4 = 4 * KS;
    __bf16 *a_lds = reinterpret_cast<__bf16 *>(smem);                       // 4*KS KiB
    float (*part)[32][65] = reinterpret_cast<float (*)[32][65]>(smem + KS4 * 1024);
    __bf16 *dg_lds = reinterpret_cast<__bf16 *>(smem + KS4 * 1024 + ASR_GLDS_BYTES);   // 16 KiB
    __shared__ int dead_s;
    const int H = p.H, B = p.B, T = p.T, H4 = 4 * p.H;
    int jt = blockIdx.x, btile = blockIdx.y + ctl.bt0, dir = blockIdx.z;
    if (ctl.xcd_teams) {
        // 1-D grid, team = blockIdx.x % 8 + 8 * (slot / njt): the H/64 workgroups that
        // exchange h_t / dgates_t every step have equal blockIdx % 8, i.e. sit on one XCD
        // under the observed round-robin placement (speed only — the hand-off protocol
        // does not depend on it); surplus workgroups of the padded grid leave at once
        const int slot = blockIdx.x >> 3, team = (slot / (p.H / 64)) * 8 + (blockIdx.x & 7);
        if (team >= ctl.xcd_teams) return;
        jt = slot % (p.H / 64);
        btile = (team >> 1) + ctl.bt0;
        dir = team & 1;
    }
    const int j0 = jt * 64, b0 = btile * (8 * NE), njt = H / 64;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int kq = wave >> 1, js = wave & 1;
    const size_t Bp = ctl.rows;              // rows of an hbuf / dgbuf plane (32 per batch tile)
    unsigned *myctr = ctl.ctr + ((size_t)dir * ctl.nbt + btile) * 32;
    if (tid == 0) dead_s = 0;
    for (int i = tid; i < 8192; i += 512) dg_lds[i] = (__bf16)0.f;      // padding rows stay 0
    for (int i = tid; i < KS4 * 64; i += 512)                           // (the tile's too: never loaded)
        reinterpret_cast<u32x4 *>(a_lds)[i] = u32x4{0u, 0u, 0u, 0u};

    bf16x8 fb[KS];
    {
        const __bf16 *bp = p.whhT + (size_t)dir * H * H4 +
                           (((size_t)(2 * jt + js) * KS4 + (size_t)kq * KS) * 64 + lane) * 8;
#pragma unroll
        for (int k = 0; k < KS; ++k) fb[k] = *reinterpret_cast<const bf16x8 *>(bp + k * 512);
    }
    const __amdgpu_buffer_rsrc_t dres = __builtin_amdgcn_make_buffer_rsrc(
        p.dgbuf, 0, (int)(2 * 2 * Bp * H4 * 2), 0x00020000);

    const int col = lane, j = j0 + col;
    float dcarry[NE];
    int len[NE], bcl[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int b = b0 + e * 8 + wave;
        dcarry[e] = 0.f;
        len[e] = b < B ? p.lens[b] : 0;
        bcl[e] = b < B ? b : B - 1;
    }

    // operands of the cell backward at frame t: saved gates, dy, and the cell
    // state the step started from (c of the neighbouring frame, raw); c_t itself
    // is the neighbour value fetched one step earlier
    // raw buffers, per-element 32-bit byte offsets computed once, frame offsets in SGPRs
    // (as in the forward kernel; the host checks every tensor is < 4 GiB)
    typedef unsigned int u32;
    constexpr u32 OOBV = 0xFFFFFFFFu;
    u32 vcs[NE], vdy[NE], vdg[NE];        // gate records: 2 * vcs
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int b = b0 + e * 8 + wave;
        vcs[e] = (u32)((dir * B + bcl[e]) * H + j) * 4u;
        vdy[e] = (u32)(p.dy_shared ? bcl[e] * H + j : (bcl[e] * 2 + dir) * H + j) * 4u;
        vdg[e] = b < B ? (u32)((b * 2 + dir) * H4 + j) * 2u : OOBV;
    }
    const u32 fg = (u32)B * 2u * H * 8u, fcs = (u32)B * 2u * H * 4u;
    const u32 fdy = (u32)B * H * 4u * (p.dy_shared ? 1u : 2u), fdg = (u32)B * 2u * H4 * 2u;
    const __amdgpu_buffer_rsrc_t gR = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<u32x2 *>(p.gates), 0, (int)((u32)T * fg), 0x00020000);
    const __amdgpu_buffer_rsrc_t csR = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(p.csave), 0, (int)((u32)T * fcs), 0x00020000);
    const __amdgpu_buffer_rsrc_t dyR = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(p.dy), 0,
        __builtin_amdgcn_readfirstlane((int)((u32)T * fdy)), 0x00020000);
    const __amdgpu_buffer_rsrc_t dgR = __builtin_amdgcn_make_buffer_rsrc(
        p.dgates, 0, (int)((u32)T * fdg), 0x00020000);
    auto ldf = [&](__amdgpu_buffer_rsrc_t R, u32 voff, u32 soff) -> float {
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(R, voff, soff, 0));
    };
    struct Pre { u32x2 g[NE]; float cp[NE], dy[NE]; };     // gates stay packed until used
    auto fetch = [&](int t, Pre &q) {
        const int tp = dir == 0 ? t - 1 : t + 1;
        const int tpc = tp < 0 ? 0 : (tp >= T ? T - 1 : tp);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            q.g[e] = __builtin_amdgcn_raw_buffer_load_b64(gR, vcs[e] * 2u, (u32)t * fg, 0);
            q.cp[e] = ldf(csR, vcs[e], (u32)tpc * fcs);
            q.dy[e] = ldf(dyR, vdy[e], (u32)t * fdy);
        }
    };
    Pre cur;
    float pcs[NE];
    {
        const int t0 = dir == 0 ? T - 1 : 0;
        fetch(t0, cur);
#pragma unroll
        for (int e = 0; e < NE; ++e) pcs[e] = ldf(csR, vcs[e], (u32)t0 * fcs);
    }
    __bf16 sod[NE][4] = {};
    int st = 0;
    auto bulk_store = [&](bool live) {      // live == false: offsets out of range (first step)
#pragma unroll
        for (int e = 0; e < NE; ++e)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                __builtin_amdgcn_raw_buffer_store_b16(
                    (short)__builtin_bit_cast(unsigned short, sod[e][g]), dgR, live ? vdg[e] : OOBV,
                    (u32)st * fdg + (u32)g * H * 2u, 0);
    };

    PSTAMP_DECL;
    for (int step = 0; step < T; ++step) {
        const int t = dir == 0 ? T - 1 - step : step;
        if (step > 0 && tid == 0 && !dead_s) {
            if (!team_wait(myctr, (unsigned)(njt * step), ctl.spin_limit, ctl.err)) dead_s = 1;
        }
        PSTAMP(0);
        __syncthreads();
        // ---- dgates_{prev step} rows of this batch tile, all 4H columns (4*KS KiB): the
        // 16 KiB this workgroup produced itself are still in dg_lds (LDS -> LDS copy), the
        // rest comes from the team mates over sc1 loads
        // (real batch rows only, as in the forward kernel)
        constexpr int RL = 8 * NE, CPK = 2 * RL;
        constexpr int CHO = (KS4 - 16) * CPK, NI = (CHO + 511) / 512;
        u32x4 tmp[NI > 0 ? NI : 1];
        if constexpr (NI > 0) {
            const unsigned base = (unsigned)((((size_t)(step & 1) * 2 + dir) * Bp * H4 +
                                              (size_t)btile * KS4 * 512) * 2);
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int co = i * 512 + tid;
                const int cc = co < CHO ? co : CHO - 1;
                const int kq = cc / CPK, q = cc - kq * CPK, g = kq / (KS - 4), r = kq - g * (KS - 4);
                const int k = g * KS + (r < 4 * jt ? r : r + 4);
                tmp[i] = __builtin_amdgcn_raw_buffer_load_b128(
                    dres, base + (k * 64 + (q < RL ? q : q + (32 - RL))) * 16, 0, ASR_SC1);
            }
        }
        bulk_store(step > 0);     // previous step's dgates rows, under the tile-load latency
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = i * 512 + tid, bi = c >> 6;         // bi = gate * 4 + kk
            reinterpret_cast<u32x4 *>(a_lds)[((bi >> 2) * KS + 4 * jt + (bi & 3)) * 64 + (c & 63)] =
                reinterpret_cast<const u32x4 *>(dg_lds)[c];
        }
        if constexpr (NI > 0) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int co = i * 512 + tid;
                const int kq = co / CPK, q = co - kq * CPK, g = kq / (KS - 4), r = kq - g * (KS - 4);
                const int k = g * KS + (r < 4 * jt ? r : r + 4);
                if (co < CHO)
                    reinterpret_cast<u32x4 *>(a_lds)[k * 64 + (q < RL ? q : q + (32 - RL))] = tmp[i];
            }
        }
        __syncthreads();
        PSTAMP(1);
        Pre nxt;
        {
            const int sn = step + 1 < T ? step + 1 : step;
            fetch(dir == 0 ? T - 1 - sn : sn, nxt);
        }
        {
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
        PSTAMP(2);
        const bool dead = dead_s != 0;
        st = t;
        const int tp = dir == 0 ? t - 1 : t + 1;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int row = e * 8 + wave;
            float od[4];
            if (t < len[e]) {
                const float dh = cur.dy[e] + (part[0][row][col] + part[1][row][col]) +
                                 (part[2][row][col] + part[3][row][col]);
                const float cp = (tp >= 0 && tp < len[e]) ? cur.cp[e] : 0.f;
                float dcout, gt[4];
                unpack_gates(cur.g[e], gt);
                lstm_cell_bwd(gt, pcs[e], cp, dh, dcarry[e], od, dcout);
                dcarry[e] = dcout;
                if (dead) od[0] = od[1] = od[2] = od[3] = __builtin_nanf("");
            } else {
                // no gradient reaches a padding frame; the carried state gradient restarts from zero
                od[0] = od[1] = od[2] = od[3] = 0.f;
                dcarry[e] = 0.f;
            }
            const int slot = ((col >> 4) * 64 + row + 32 * ((col >> 3) & 1)) * 8 + (col & 7);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                sod[e][g] = (__bf16)od[g];
                dg_lds[g * 2048 + slot] = sod[e][g];
            }
            pcs[e] = cur.cp[e];         // c of the frame the next step visits
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int bi = wave * 2 + r, g = bi >> 2, kk = bi & 3;
            const u32x4 v = reinterpret_cast<const u32x4 *>(dg_lds)[bi * 64 + lane];
            const unsigned off = (unsigned)(((((size_t)((step + 1) & 1) * 2 + dir) * Bp * H4) +
                                             ((size_t)btile * KS4 + g * KS + 4 * jt + kk) * 512 + lane * 8) * 2);
            __builtin_amdgcn_raw_buffer_store_b128(v, dres, (lane & 31) < 8 * NE ? off : 0xFFFFFFFFu,
                                                   0, ASR_SC1);
        }
        PSTAMP(3);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        PSTAMP(4);
        if (tid == 0) __hip_atomic_fetch_add(myctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cur = nxt;
        PSTAMP(5);
    }
    if (T > 0) bulk_store(true);          // the last step's
#ifdef ASR_LSTM_STAMPS
    __syncthreads();
    if (tid == 0 && b0 < B)
        for (int i = 0; i < 6; ++i)
            p.dgates[(((size_t)0 * B + b0) * 2 + dir) * H4 + j0 + i] = (__bf16)((float)pst[i] / T / 16.f);
#endif
}

}  // namespace

extern "C" int64_t asr_lstm_workspace_bytes(int B, int H) {
    if (B < 0 || H < 0) return -1;
    // forward: hbuf bf16 [2][2][Bp][H] + cbuf f32 [2][B][H] + packed W_hh
    // backward: dgbuf bf16 [2][2][Bp][4H] + dcbuf f32 [2][B][H] + packed W_hhᵀ (larger)
    // + team counters of the persistent kernels: [2 dir][ceil(B/32)] x 128 B and a timeout word
    const int64_t Bp = plane_rows(B);
    // (forward with the fused input projection: a second packed matrix, W_ih)
    return (int64_t)2 * 2 * Bp * 4 * H * 2 + (int64_t)2 * B * H * 4 +
           (int64_t)2 * 4 * H * H * 2 + (int64_t)2 * 4 * H * (H + 64) * 2 + 256 + ctl_bytes(B);
}

namespace {
int lstm_fwd_impl(const void *gx, int gx_bf16, const void *x_bf16, const void *wih_bf16, int F,
                  const void *whh_bf16, const int32_t *lens, int T, int B, int H,
                  float *y, void *y_bf16, void *gates_bf16, float *csave,
                  void *workspace, int64_t workspace_bytes, uint32_t *err_flag, void *stream);
}

extern "C" int asr_lstm_bidir_fwd_bf16(const void *gx, int gx_bf16, const void *whh_bf16,
                                       const int32_t *lens, int T, int B, int H,
                                       float *y, void *y_bf16, void *gates_bf16,
                                       float *csave,
                                       void *workspace, int64_t workspace_bytes,
                                       uint32_t *err_flag, void *stream) {
    if (!gx) return ASR_EINVAL;
    return lstm_fwd_impl(gx, gx_bf16, nullptr, nullptr, 0, whh_bf16, lens, T, B, H, y, y_bf16,
                         gates_bf16, csave, workspace, workspace_bytes, err_flag, stream);
}

extern "C" int asr_lstm_bidir_fwd_fused_bf16(const void *x_bf16, const void *wih_bf16,
                                             const void *whh_bf16, const int32_t *lens,
                                             int T, int B, int H, int F, float *y, void *y_bf16,
                                             void *gates_bf16, float *csave, void *workspace,
                                             int64_t workspace_bytes, uint32_t *err_flag,
                                             void *stream) {
    if (!x_bf16 || !wih_bf16) return ASR_EINVAL;
    return lstm_fwd_impl(nullptr, 1, x_bf16, wih_bf16, F, whh_bf16, lens, T, B, H, y, y_bf16,
                         gates_bf16, csave, workspace, workspace_bytes, err_flag, stream);
}

extern "C" int asr_lstm_fused_supported(int B, int H, int F) {
    if (!persist_enabled() || B <= 0) return 0;
    if (H != 64 && H != 128 && H != 256 && H != 320) return 0;
    // input size: the hidden size, or (H = 320) the 352 features of the conv front-end
    if (F != H && !(H == 320 && F == 352)) return 0;
    return cu_count() >= 2 * (H / 64) ? 1 : 0;
}

namespace {
int lstm_fwd_impl(const void *gx, int gx_bf16, const void *x_bf16, const void *wih_bf16, int F,
                  const void *whh_bf16, const int32_t *lens, int T, int B, int H,
                  float *y, void *y_bf16, void *gates_bf16, float *csave,
                  void *workspace, int64_t workspace_bytes, uint32_t *err_flag, void *stream) {
    const bool fused = x_bf16 != nullptr;
    if (T < 0 || B <= 0 || H <= 0 || (H % 32) != 0) return ASR_EINVAL;
    if (T == 0) return ASR_OK;
    if (!whh_bf16 || !lens || !y_bf16 || !gates_bf16 || !csave || !workspace)
        return ASR_EINVAL;
    if (fused && (!asr_lstm_fused_supported(B, H, F) || (uint64_t)T * B * F * 2 >= (1ull << 31)))
        return ASR_EUNSUPPORTED;
    if (fused && F != H && y) return ASR_EINVAL;      // that variant writes the bf16 outputs only
    if (workspace_bytes < asr_lstm_workspace_bytes(B, H)) return ASR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    LstmFwdParams p;
    const size_t Bp = (size_t)plane_rows(B);
    const size_t hbytes = (size_t)2 * 2 * Bp * H * 2, cbytes = (size_t)2 * B * H * 4;
    __bf16 *wpack = (__bf16 *)((char *)workspace + hbytes + cbytes);
    p.gx = gx; p.gx_bf16 = gx_bf16; p.whh = wpack; p.lens = lens;
    p.x = (const __bf16 *)x_bf16; p.wih = wpack + (size_t)8 * H * H;
    p.T = T; p.B = B; p.H = H;
    p.hbuf = (__bf16 *)workspace;
    p.cbuf = (float *)((char *)workspace + hbytes);
    p.y = y; p.ybf = (__bf16 *)y_bf16; p.gates = (u32x2 *)gates_bf16; p.csave = csave;
    p.step = 0;
    ZeroList zl;
    zl.add(workspace, hbytes + cbytes);
    // the two pad frames of every direction of y_bf16
    for (int d = 0; d < 2; ++d) {
        zl.add(p.ybf + (size_t)d * (T + 2) * B * H, (size_t)B * H * 2);
        zl.add(p.ybf + ((size_t)d * (T + 2) + T + 1) * B * H, (size_t)B * H * 2);
    }
    if (persist_enabled())
        zl.add((char *)workspace + asr_lstm_workspace_bytes(B, H) - ctl_bytes(B), (size_t)ctl_bytes(B));
    zl.launch(s);
    // [2 dir x 4 gates] matrices of H x H (rows = hidden unit, cols = k)
    hipLaunchKernelGGL(lstm_pack_kernel, dim3(1024), dim3(256), 0, s,
                       (const __bf16 *)whh_bf16, wpack, 8, H, H, 0);
    if (fused)          // wih_bf16: [2 dir][4H rows (gate-major)][F cols] row-major
        hipLaunchKernelGGL(lstm_pack_kernel, dim3(1024), dim3(256), 0, s,
                           (const __bf16 *)wih_bf16, wpack + (size_t)8 * H * H, 8, H, F, 0);
    if (persist_enabled()) {
        unsigned *ctl_words = (unsigned *)((char *)workspace + asr_lstm_workspace_bytes(B, H) - ctl_bytes(B));
        void (*pk[3])(LstmFwdParams, LstmTeamCtl) = {nullptr, nullptr, nullptr};
#define ASR_PICK(KSV) if (H == 16 * KSV && !fused) {                                           \
        if (gx_bf16) { pk[0] = lstm_fwd_persist_kernel<KSV, 2, 1, 0>; pk[1] = lstm_fwd_persist_kernel<KSV, 3, 1, 0>; \
                       pk[2] = lstm_fwd_persist_kernel<KSV, 4, 1, 0>; }                             \
        else { pk[0] = lstm_fwd_persist_kernel<KSV, 2, 0, 0>; pk[1] = lstm_fwd_persist_kernel<KSV, 3, 0, 0>; \
               pk[2] = lstm_fwd_persist_kernel<KSV, 4, 0, 0>; } }
        ASR_PICK(20) ASR_PICK(4) ASR_PICK(8) ASR_PICK(16) ASR_PICK(24) ASR_PICK(32)   // 48: W_hh slice spills
#undef ASR_PICK
#define ASR_PICK(KSV) if (H == 16 * KSV && fused && F == H) { pk[0] = lstm_fwd_persist_kernel<KSV, 2, 1, KSV>; \
        pk[1] = lstm_fwd_persist_kernel<KSV, 3, 1, KSV>; pk[2] = lstm_fwd_persist_kernel<KSV, 4, 1, KSV>; }
        ASR_PICK(20) ASR_PICK(4) ASR_PICK(8) ASR_PICK(16)     // two weight slices in registers
#undef ASR_PICK
        if (H == 320 && fused && F == 352) {                  // the first layer behind the conv front-end
            pk[0] = lstm_fwd_persist_kernel<20, 2, 1, 22>; pk[1] = lstm_fwd_persist_kernel<20, 3, 1, 22>;
            pk[2] = lstm_fwd_persist_kernel<20, 4, 1, 22>;
        }
        // the persistent kernel addresses gx / y / gates / ... with 32-bit byte offsets
        const bool fits32 = (uint64_t)T * B * 8 * H * 4 < (1ull << 32) &&
                            (uint64_t)2 * (T + 2) * B * H * 2 < (1ull << 32);
        const size_t lds_need = (size_t)(H / 16) * 1024 + (fused ? (size_t)(F / 16) * 1024 : 0) + ASR_GLDS_BYTES + 4096;
        if (fits32 && pk[2] && launch_persist(pk, p, B, H, lds_need, ctl_words, err_flag, s))
            return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
    }
    if (fused) return ASR_EUNSUPPORTED;
    // one launch per step.  64-row tiles would halve the W_hh re-reads but were
    // measured SLOWER (13.7 vs 11.4 us at B=512): the step is latency-bound per
    // workgroup, not fetch-bound
    const dim3 grid(H / 32, (B + 31) / 32, 2);
    void (*kern)(LstmFwdParams) = nullptr;
#define ASR_PICK(KSV)                                                              \
    if (H == 16 * KSV) kern = gx_bf16 ? lstm_fwd_step_kernel<KSV, 1> : lstm_fwd_step_kernel<KSV, 0>;
    ASR_PICK(20) ASR_PICK(4) ASR_PICK(8) ASR_PICK(16) ASR_PICK(24) ASR_PICK(32) ASR_PICK(48)
#undef ASR_PICK
    if (!kern) return ASR_EUNSUPPORTED;       // hidden sizes built: 64,128,256,320,384,512,768
    for (int step = 0; step < T; ++step) {
        p.step = step;
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, p);
    }
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
}  // namespace

extern "C" int asr_lstm_bidir_bwd_bf16(const float *dy, int dy_shared, const void *whhT_bf16,
                                       const int32_t *lens, int T, int B, int H,
                                       const void *gates_bf16, const float *csave,
                                       void *dgates_bf16,
                                       void *workspace, int64_t workspace_bytes,
                                       uint32_t *err_flag, void *stream) {
    if (T < 0 || B <= 0 || H <= 0 || (H % 32) != 0 || dy_shared < 0 || dy_shared > 1) return ASR_EINVAL;
    if (T == 0) return ASR_OK;
    if (!dy || !whhT_bf16 || !lens || !gates_bf16 || !csave || !dgates_bf16 || !workspace)
        return ASR_EINVAL;
    if (workspace_bytes < asr_lstm_workspace_bytes(B, H)) return ASR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    LstmBwdParams p;
    const size_t Bp = (size_t)plane_rows(B);
    const size_t dbytes = (size_t)2 * 2 * Bp * 4 * H * 2, cbytes = (size_t)2 * B * H * 4;
    __bf16 *wpack = (__bf16 *)((char *)workspace + dbytes + cbytes);
    p.dy = dy; p.dy_shared = dy_shared; p.whhT = wpack; p.lens = lens;
    p.T = T; p.B = B; p.H = H;
    p.gates = (const u32x2 *)gates_bf16; p.csave = csave;
    p.dgbuf = (__bf16 *)workspace;
    p.dcbuf = (float *)((char *)workspace + dbytes);
    p.dgates = (__bf16 *)dgates_bf16;
    {
        ZeroList zl;
        zl.add(workspace, dbytes + cbytes);
        if (persist_enabled())
            zl.add((char *)workspace + asr_lstm_workspace_bytes(B, H) - ctl_bytes(B), (size_t)ctl_bytes(B));
        zl.launch(s);
    }
    // whhT_bf16 is [2][H][4H] row-major: rows = hidden unit j, cols = k over 4H
    hipLaunchKernelGGL(lstm_pack_kernel, dim3(1024), dim3(256), 0, s,
                       (const __bf16 *)whhT_bf16, wpack, 2, H, 4 * H, 0);
    if (persist_enabled()) {
        unsigned *ctl_words = (unsigned *)((char *)workspace + asr_lstm_workspace_bytes(B, H) - ctl_bytes(B));
        void (*pk[3])(LstmBwdParams, LstmTeamCtl) = {nullptr, nullptr, nullptr};
#define ASR_PICK(KSV) if (H == 16 * KSV) { pk[0] = lstm_bwd_persist_kernel<KSV, 2>; \
        pk[1] = lstm_bwd_persist_kernel<KSV, 3>; pk[2] = lstm_bwd_persist_kernel<KSV, 4>; }
        ASR_PICK(20) ASR_PICK(4) ASR_PICK(8) ASR_PICK(16) ASR_PICK(24)
#undef ASR_PICK
        const bool fits32 = (uint64_t)T * B * 8 * H * 4 < (1ull << 32);      // 32-bit byte offsets
        const size_t lds = (size_t)(H / 4) * 1024 + ASR_GLDS_BYTES + 16384;
        if (fits32 && pk[2] && launch_persist(pk, p, B, H, lds, ctl_words, err_flag, s))
            return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
    }
    const dim3 grid(H / 32, (B + 31) / 32, 2);
    void (*kern)(LstmBwdParams) = nullptr;
#define ASR_PICK(KSV)                                                              \
    if (H == 16 * KSV) kern = lstm_bwd_step_kernel<KSV>;
    ASR_PICK(20) ASR_PICK(4) ASR_PICK(8) ASR_PICK(16) ASR_PICK(24) ASR_PICK(32) ASR_PICK(48)
#undef ASR_PICK
    if (!kern) return ASR_EUNSUPPORTED;
    for (int step = 0; step < T; ++step) {
        p.step = step;
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, p);
    }
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
