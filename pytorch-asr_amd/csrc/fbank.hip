// Feature front-end in one launch (include/asr_amd.h: asr_fbank_f32, asr_fbank_supported):
// padded waveforms -> Kaldi filter-bank features, deltas, CMVN -> the model's [B, T_max, F, C]
// fp32 input.  The reference computes them in a Kaldi pipe per DataLoader worker
// (att_speech/data/kaldi_dataset.py:194-202; egs/wsj/compute_features.sh:17-18:
// compute-fbank-feats | add-deltas, then apply-cmvn); att_speech/features.py states the same
// arithmetic in numpy.
//
// A workgroup owns TILE = 32 output frames of one utterance and computes the static features of
// those and of the 4 + 4 neighbours the delta-delta taps reach (recomputed, not read back from
// HBM) into an LDS tile.  One wave takes one frame at a time, at its own pace (wave_sync): the
// window's samples through dither, mean, energy, pre-emphasis and the Povey window into LDS; the 512-point real FFT as a
// 256-point complex FFT, radix 4, one butterfly per lane and stage, twiddles from the uploaded
// table; the split into the real signal's spectrum, power, and the mel products with lanes over
// banks, each bank over its own bins.  Then the workgroup forms the channels from the tile with
// the clamp at the utterance's own first and last frame, applies CMVN and writes whole
// [t][f][c] rows, zeros at t >= T_b.
//
// fp32 throughout, every sum in a fixed order (lane partials, then the xor-butterfly of
// asr::wave_sum): two runs give the same bits, and a frame's value depends on its utterance's
// samples only, not on B, the batch position or T_max (dither apart: its index holds them).
#include "common.h"
#include "noise_draw.h"
#include "../../include/asr_amd.h"

#include <float.h>

namespace {

constexpr int TPB = 256;
constexpr int NW = TPB / 64;
constexpr int TILE = 32;
constexpr int HALO = 4;                         // the 9 delta-delta taps reach t - 4 .. t + 4
constexpr int ROWS = TILE + 2 * HALO;
constexpr int P = 512, HALF = 256;
constexpr int MAX_BINS = 128;
constexpr int MAX_F = MAX_BINS + 1;
constexpr int PER_LANE = P / 64;
constexpr int MAX_MEL_W = 2 * HALF;             // an FFT bin feeds at most two banks
constexpr int TW_USED = 384;                    // the butterflies read up to tw[6 * 63], the split tw[255]
constexpr uint32_t TAG_DITHER = 2;

struct FbankParams {
    const void *waves;
    int64_t wave_stride;
    int n_max, is_i16;
    const int32_t *wave_lens;
    int B, T_max, tiles;
    const float *window;
    const float2 *tw;
    const int32_t *mel_idx;
    const float *mel_w;
    int mel_w_len;
    int L, shift, nb, use_energy, order;
    float preemph;
    const float *cmvn_offset, *cmvn_scale;
    float dither;
    uint32_t k0, k1, it_lo, it_hi;
    float *out;
    int32_t *feat_lens;
};

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// the radix-4 decimation in frequency leaves frequency f at the position with f's base-4 digits reversed
__device__ __forceinline__ int rev4(int x) {
    return ((x & 3) << 6) | ((x & 0xC) << 2) | ((x & 0x30) >> 2) | ((x & 0xC0) >> 6);
}

// A frame's LDS buffers belong to one wave, whose LDS operations execute in the order issued: what its
// lanes hand each other needs the ordering of a barrier without the wait for the other waves.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float dither_draw(const FbankParams &p, uint64_t index) {
    const asr::U4 o = asr::philox4x32_10(asr::U4{(uint32_t)(index >> 2), TAG_DITHER, p.it_lo, p.it_hi}, p.k0, p.k1);
    float za, zb;
    if (index & 2)
        asr::box_muller(o.z, o.w, za, zb);
    else
        asr::box_muller(o.x, o.y, za, zb);
    return (index & 1) ? zb : za;
}

__global__ __launch_bounds__(TPB) void fbank_kernel(FbankParams p) {
    __shared__ float s_win[P];
    __shared__ float2 s_tw[TW_USED];
    __shared__ float s_buf[NW][P];              // one frame per wave: samples, then 256 complex points
    __shared__ float s_pw[NW][HALF];
    __shared__ float s_tile[ROWS][MAX_F];       // static features of frames t0 - 4 .. t0 + 35
    __shared__ float s_mel_w[MAX_MEL_W];
    __shared__ int16_t s_mel_first[MAX_BINS], s_mel_end[MAX_BINS], s_mel_off[MAX_BINS];   // 40 KiB in all: 4 per CU

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x / p.tiles, t0 = (blockIdx.x - b * p.tiles) * TILE;
    const int L = p.L, F = p.nb + p.use_energy, C = p.order + 1, FC = F * C;
    int N = p.wave_lens[b];
    N = N < p.n_max ? N : p.n_max;
    int T = N >= L ? 1 + (N - L) / p.shift : 0;
    T = T < p.T_max ? T : p.T_max;
    const int nt = p.T_max - t0 < TILE ? p.T_max - t0 : TILE;
    float *const out = p.out + ((int64_t)b * p.T_max + t0) * FC;
    if (t0 == 0 && tid == 0) p.feat_lens[b] = T;
    if (t0 >= T) {                              // a tile of padding frames only
        for (int e = tid; e < nt * FC; e += TPB) out[e] = 0.f;
        return;
    }

    for (int i = tid; i < P; i += TPB) {
        s_win[i] = i < L ? p.window[i] : 0.f;
        if (i < TW_USED) s_tw[i] = p.tw[i];
        if (i < p.mel_w_len) s_mel_w[i] = p.mel_w[i];
        if (i < p.nb) {                         // a bank whose range leaves the tables counts as empty
            int first = p.mel_idx[3 * i], end = p.mel_idx[3 * i + 1];
            const int off = p.mel_idx[3 * i + 2];
            first = first < 0 ? 0 : (first > HALF ? HALF : first);
            end = end < first ? first : (end > HALF ? HALF : end);
            if (off < 0 || off + (end - first) > p.mel_w_len) end = first;
            s_mel_first[i] = (int16_t)first;
            s_mel_end[i] = (int16_t)end;
            s_mel_off[i] = (int16_t)(end > first ? off : 0);
        }
    }
    __syncthreads();

    float *const buf = s_buf[w];
    float2 *const cbuf = (float2 *)buf;
    // the tile's rows that are frames of the utterance, dealt round the waves
    const int r_lo = t0 < HALO ? HALO - t0 : 0, r_hi = T - t0 + HALO < ROWS ? T - t0 + HALO : ROWS;
    for (int r = r_lo + w; r < r_hi; r += NW) {
        const int t = t0 - HALO + r;
        float x[PER_LANE];
        float energy = 0.f;
        {
            const int64_t first = (int64_t)b * p.wave_stride + (int64_t)t * p.shift;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) {
                const int i = lane + 64 * k;
                float v = 0.f;
                if (i < L) {
                    v = p.is_i16 ? (float)((const int16_t *)p.waves)[first + i] : ((const float *)p.waves)[first + i];
                    if (p.dither != 0.f)
                        v += p.dither * dither_draw(p, ((uint64_t)b * p.T_max + t) * P + i);
                }
                x[k] = v;
                s += v;
            }
            const float mean = asr::wave_sum(s) / (float)L;
            float e = 0.f;
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) {
                x[k] = lane + 64 * k < L ? x[k] - mean : 0.f;
                e += x[k] * x[k];
                buf[lane + 64 * k] = x[k];
            }
            energy = logf(fmaxf(asr::wave_sum(e), FLT_EPSILON));
        }
        wave_sync();
        {
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) {
                const int i = lane + 64 * k;
                const float prev = i > 0 ? buf[i - 1] : x[k];       // x[0] -= preemph * x[0]
                x[k] = (x[k] - p.preemph * prev) * s_win[i];        // s_win is 0 from L on: the padding
            }
        }
        wave_sync();
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) buf[lane + 64 * k] = x[k];
        wave_sync();
        // z[n] = x[2n] + i x[2n+1] is the buffer as it lies; 256-point FFT, in place
#pragma unroll
        for (int q = 64; q >= 1; q >>= 2) {
            {
                const int k = lane & (q - 1), at = (lane - k) * 4 + k, e = k * (64 / q);
                const float2 a0 = cbuf[at], a1 = cbuf[at + q], a2 = cbuf[at + 2 * q], a3 = cbuf[at + 3 * q];
                const float2 u0 = cadd(a0, a2), u1 = csub(a0, a2), u2 = cadd(a1, a3), d = csub(a1, a3);
                const float2 u3 = make_float2(d.y, -d.x);           // -i (a1 - a3)
                cbuf[at] = cadd(u0, u2);
                cbuf[at + q] = cmul(cadd(u1, u3), s_tw[2 * e]);     // exp(-2 pi i e / 256) = tw[2 e]
                cbuf[at + 2 * q] = cmul(csub(u0, u2), s_tw[4 * e]);
                cbuf[at + 3 * q] = cmul(csub(u1, u3), s_tw[6 * e]);
            }
            wave_sync();
        }
        {
            // X[k] = E[k] + W^k O[k] from Z[k] and conj Z[256 - k]; bins 0..255 (no Nyquist bin)
#pragma unroll
            for (int m = 0; m < HALF / 64; ++m) {
                const int k = lane + 64 * m;
                const float2 z = cbuf[rev4(k)], zm = cbuf[rev4((HALF - k) & (HALF - 1))];
                const float2 ev = make_float2(0.5f * (z.x + zm.x), 0.5f * (z.y - zm.y));
                const float2 od = make_float2(0.5f * (z.y + zm.y), -0.5f * (z.x - zm.x));
                const float2 xk = cadd(ev, cmul(od, s_tw[k]));
                s_pw[w][k] = xk.x * xk.x + xk.y * xk.y;
            }
        }
        wave_sync();
        {
            for (int bank = lane; bank < p.nb; bank += 64) {
                const int first = s_mel_first[bank], end = s_mel_end[bank], off = s_mel_off[bank];
                float acc = 0.f;
                for (int k = first; k < end; ++k) acc += s_mel_w[off + k - first] * s_pw[w][k];
                s_tile[r][p.use_energy + bank] = logf(fmaxf(acc, FLT_EPSILON));
            }
            if (p.use_energy && lane == 0) s_tile[r][0] = energy;
        }
        wave_sync();                            // the next frame overwrites buf and s_pw
    }
    __syncthreads();

    const float s1[5] = {-0.2f, -0.1f, 0.f, 0.1f, 0.2f};
    const float s2[9] = {0.04f, 0.04f, 0.01f, -0.04f, -0.1f, -0.04f, 0.01f, 0.04f, 0.04f};
    for (int tl = 0; tl < nt; ++tl)
    for (int rem = tid; rem < FC; rem += TPB) {
        const int f = C == 3 ? rem / 3 : (C == 2 ? rem >> 1 : rem), c = rem - f * C, t = t0 + tl;
        float v = 0.f;
        if (t < T) {
            if (c == 0) {
                v = s_tile[tl + HALO][f];
            } else {
                const int reach = 2 * c;
                for (int j = -reach; j <= reach; ++j) {
                    int tj = t + j;
                    tj = tj < 0 ? 0 : (tj > T - 1 ? T - 1 : tj);
                    v += (c == 1 ? s1[j + 2] : s2[j + 4]) * s_tile[tj - t0 + HALO][f];
                }
            }
            if (p.cmvn_offset) v -= p.cmvn_offset[c * F + f];
            if (p.cmvn_scale) v *= p.cmvn_scale[c * F + f];
        }
        out[tl * FC + rem] = v;
    }
}

}  // namespace

extern "C" int asr_fbank_supported(int frame_length, int frame_shift, int padded, int num_mel_bins,
                                   int delta_order, int delta_window) {
    return padded == P && frame_length > HALF && frame_length <= P && frame_shift >= 1 &&
           num_mel_bins >= 1 && num_mel_bins <= MAX_BINS && delta_order >= 0 && delta_order <= 2 &&
           delta_window == 2;
}

extern "C" int asr_fbank_f32(const void *waves, int64_t wave_stride, int n_max, int waves_int16,
                             const int32_t *wave_lens, int B, int T_max, const float *window,
                             const float *twiddles, const int32_t *mel_idx, const float *mel_w,
                             int mel_w_len, int frame_length, int frame_shift, int padded,
                             int num_mel_bins, int use_energy, int delta_order, int delta_window,
                             float preemph, const float *cmvn_offset, const float *cmvn_scale,
                             float dither, uint64_t seed, uint64_t iteration, float *out,
                             int32_t *feat_lens, void *stream) {
    if (B < 0 || T_max < 0 || n_max < 0 || wave_stride < n_max || mel_w_len < 1 || mel_w_len > MAX_MEL_W)
        return ASR_EINVAL;
    if (waves_int16 != 0 && waves_int16 != 1) return ASR_EINVAL;
    if (use_energy != 0 && use_energy != 1) return ASR_EINVAL;
    if (frame_length < 1 || frame_shift < 1 || num_mel_bins < 1 || delta_order < 0) return ASR_EINVAL;
    if (!window || !twiddles || !mel_idx || !mel_w) return ASR_EINVAL;
    if (B > 0 && (!waves || !wave_lens || !out || !feat_lens || T_max < 1)) return ASR_EINVAL;
    if (!asr_fbank_supported(frame_length, frame_shift, padded, num_mel_bins, delta_order, delta_window))
        return ASR_EUNSUPPORTED;
    if (B == 0) return ASR_OK;
    const int64_t tiles = ((int64_t)T_max + TILE - 1) / TILE;
    if (tiles * B > INT32_MAX) return ASR_EUNSUPPORTED;
    // the draw's counter holds index >> 2 in 32 bits
    if (dither != 0.f && (int64_t)B * T_max >= ((int64_t)1 << 34) / P) return ASR_EUNSUPPORTED;
    FbankParams p;
    p.waves = waves;
    p.wave_stride = wave_stride;
    p.n_max = n_max;
    p.is_i16 = waves_int16;
    p.wave_lens = wave_lens;
    p.B = B;
    p.T_max = T_max;
    p.tiles = (int)tiles;
    p.window = window;
    p.tw = (const float2 *)twiddles;
    p.mel_idx = mel_idx;
    p.mel_w = mel_w;
    p.mel_w_len = mel_w_len;
    p.L = frame_length;
    p.shift = frame_shift;
    p.nb = num_mel_bins;
    p.use_energy = use_energy;
    p.order = delta_order;
    p.preemph = preemph;
    p.cmvn_offset = cmvn_offset;
    p.cmvn_scale = cmvn_scale;
    p.dither = dither;
    p.k0 = (uint32_t)seed;
    p.k1 = (uint32_t)(seed >> 32);
    p.it_lo = (uint32_t)iteration;
    p.it_hi = (uint32_t)(iteration >> 32);
    p.out = out;
    p.feat_lens = feat_lens;
    hipLaunchKernelGGL(fbank_kernel, dim3((unsigned)(tiles * B)), dim3(TPB), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? ASR_OK : ASR_ELAUNCH;
}
