// decode_kernels.hpp — the device pieces the decoders share (decode.hip, lstm.hip, beam.hip): each stands here ONCE, so the greedy
// loop, its lockstep LSTM twin, the persistent loop and the beam searches take the same sums, the same tie rule and the same advance
// rule by construction (tests/test_decode_bits_gpu.py pins their bits).  One exception: k_dec_persist writes the advance rule out
// (see there).
#pragma once
#include "kernels.hpp"

// ---- the greedy loop's state words (int32[RNNT_DECODE_STATE_WORDS] per utterance; a caller's view: include/rnnt_engine.h).  Word 6 has
// one meaning per loop: the lockstep LSTM loop's "settled", the persistent loop's workgroup count.  CAP and BASE exist only in the
// int32[10] state of a stream's push on the kernel-per-layer loop (k_stream_loop_prep).
enum {
    DEC_ST_T = RNNT_DECODE_T, DEC_ST_EMITTED = RNNT_DECODE_EMITTED, DEC_ST_NTOK = RNNT_DECODE_NTOK, DEC_ST_DONE = RNNT_DECODE_DONE,
    DEC_ST_NEWTOK = RNNT_DECODE_NEWTOK, DEC_ST_ITERS = RNNT_DECODE_ITERATIONS, DEC_ST_SETTLED = RNNT_DECODE_SETTLED,
    DEC_ST_GROUPS = RNNT_DECODE_WORKGROUPS, DEC_ST_CODE = RNNT_DECODE_CODE, DEC_ST_WORDS = RNNT_DECODE_STATE_WORDS,
    DEC_ST_CAP = 8,   // the push's cap on 1 + ntok
    DEC_ST_BASE = 9   // position of the newest token the push began with
};
// a fresh loop: nothing consumed, the leading blank awaits the predictor
__device__ __forceinline__ void dec_state_init(int32_t *s)
{
#pragma unroll
    for (int i = 0; i < DEC_ST_WORDS; ++i) s[i] = i == DEC_ST_NEWTOK ? 1 : 0;
}

// utterance u's copy of a per-search buffer of the beam searches, `off` = u * stride bytes on (0 for the single search)
template <typename T> __device__ __forceinline__ T *beam_utt(T *p, size_t off) { return (T *)((char *)p + off); }

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }

// the sum of v over the workgroup's 256 threads, in every thread: the wave butterfly, then (w0 + w1) + (w2 + w3).  red: 4 floats of LDS;
// the barrier BEFORE the store makes a second call on the same `red` safe (every read of the first has happened)
__device__ __forceinline__ float block_sum(float v, float *red)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// block_sum of two values at once (red: 8 floats), for the kernels that need both sums before they go on (lstm.hip's k_lstm_step_bwd):
// the same butterfly and the same (w0 + w1) + (w2 + w3) per value.  Its barriers stand AFTER the store and after the read — one call
// leaves `red` free for the next without a barrier in front, which block_sum has instead; a kernel uses one form or the other on a `red`.
__device__ __forceinline__ void block_sum2(float &a, float &b, float *red)
{
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) { a += __shfl_xor(a, k, 64); b += __shfl_xor(b, k, 64); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave] = a; red[4 + wave] = b; }
    __syncthreads();
    a = (red[0] + red[1]) + (red[2] + red[3]);
    b = (red[4] + red[5]) + (red[6] + red[7]);
    __syncthreads();
}

// mean and 1 / sqrt(var + eps) of the row x[K] by the workgroup's 256 threads: two passes, each a stride-256 loop and a block_sum.
// The apply-and-store loop stays with the caller (LDS, ring + LDS, global).  row_ln_rstd alone: the second pass, for a caller whose
// loop that PRODUCES the row has summed it on the way (ld_rowfin_row: no second trip to memory for the mean).
__device__ __forceinline__ float row_ln_rstd(const float *x, int K, float mean, float eps, float *red)
{
    float s2 = 0.f;
    for (int i = threadIdx.x; i < K; i += 256) { const float d = x[i] - mean; s2 += d * d; }
    return rsqrtf(block_sum(s2, red) / K + eps);
}
__device__ __forceinline__ void row_ln_stats(const float *x, int K, float eps, float *red, float &mean, float &rstd)
{
    float s = 0.f;
    for (int i = threadIdx.x; i < K; i += 256) s += x[i];
    mean = block_sum(s, red) / K;
    rstd = row_ln_rstd(x, K, mean, eps, red);
}

// ---- the scan tile: 32 frames x 32 vocabulary entries of tanh(frame + text) . W^T on v_mfma_f32_32x32x2_f32 with the engine's K
// permutation (a lane's float4 of 4 consecutive h feeds 4 MFMAs, for frame / text and W alike; W in its natural [V,H] layout).  The
// workgroup's 4 waves split H — chunk c of 8 h goes to wave c % 4 — and meet in LDS.  er / pr / wr: the lane's frame row, text vector
// and W row, each + 4 * (lane >> 5).  NC = H / 8.
// A chunk (4 MFMAs, ~256 matrix-pipe cycles) does not cover an L2 round trip and a 32-frame block is only V/32 workgroups: the wave's
// chunks go in GROUPS of 8 with all 24 loads of the next group in flight while the current one is multiplied (two chunks ahead
// measured 21 us per block at H = 1024: one round trip per chunk).
__device__ __forceinline__ void scan_tile_mul(f32x16 &acc, const float *er, const float *pr, const float *wr, int NC, int wave)
{
    struct Ops { f32x4 e, p, w; };
    auto load = [&](Ops &o, int c) {
        const int cc = c < NC ? c : NC - 1;
        o.e = *(const f32x4 *)(er + 8 * cc); o.p = *(const f32x4 *)(pr + 8 * cc); o.w = *(const f32x4 *)(wr + 8 * cc);
    };
    auto load8 = [&](Ops (&g)[8], int c0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) load(g[j], c0 + 4 * j);
    };
    auto mul8 = [&](const Ops (&g)[8], int c0) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (c0 + 4 * j < NC) {  // wave-uniform
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fast_tanh(g[j].e[s] + g[j].p[s]), g[j].w[s], acc, 0, 0, 0);
            }
    };
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    Ops ga[8], gb[8];
    load8(ga, wave);
    for (int c = wave; c < NC; c += 64) {  // two groups (2 x 8 chunks x 4 waves) per trip
        load8(gb, c + 32);
        mul8(ga, c);
        load8(ga, c + 64);
        mul8(gb, c + 32);
    }
}

// the four waves' partial tiles, summed (w0 + w1) + (w2 + w3) into wave 0's acc: element r of lane (i, half) is frame
// (r & 3) + 8 (r >> 2) + 4 half of the tile, vocabulary entry i.  Only wave 0 goes on to an epilogue.
__device__ __forceinline__ void scan_tile_reduce(f32x16 &acc, float (&s_acc)[3][16][64], int lane, int wave)
{
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s_acc[wave - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = (acc[r] + s_acc[0][r][lane]) + (s_acc[1][r][lane] + s_acc[2][r][lane]);
    }
}
__device__ __forceinline__ int scan_tile_frame(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// wave 0: the tile leaves as ONE (max, first index) candidate per frame — part[frame][vocabulary block], blocks = gridDim.x, this one
// blockIdx.x — not as logits: the update looks at V/32 candidates per frame instead of V values
__device__ __forceinline__ void scan_tile_candidates(const f32x16 &acc, const float *__restrict__ bias, int v0, int k0, int K, int V,
                                                     float2 *__restrict__ part, int lane)
{
    const int i = lane & 31, half = lane >> 5, v = v0 + i;
    const int NB = gridDim.x, vb = blockIdx.x;
    const float bv = v < V ? bias[v] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int k = k0 + scan_tile_frame(r, half);
        float x = acc[r] + bv;
        if (v >= V) x = RNNT_NEG_INF;
        const float M = half_max_dpp(x, half);  // every lane of the half: the maximum of the frame's 32 entries
        const unsigned long long hit = __ballot(x == M);  // first lane of the half that holds it = the lowest index
        const unsigned h32 = half ? (unsigned)(hit >> 32) : (unsigned)hit;
        if (i == 0 && k < K) part[(long)k * NB + vb] = float2{M, __int_as_float(v0 + __builtin_ctz(h32))};
    }
}

// argmax of a frame from its NB candidates (first index on ties, like torch.argmax: candidates are in increasing index order)
__device__ __forceinline__ int cand_argmax(const float2 *__restrict__ p, int NB)
{
    float best = RNNT_NEG_INF;
    int bi = 0;
    for (int j = 0; j < NB; ++j) {
        const float2 c = p[j];
        if (c.x > best) { best = c.x; bi = __float_as_int(c.y); }
    }
    return bi;
}
// the first of the n frame tokens that is not blank, or -1
__device__ __forceinline__ int dec_first_hit(const int *tok, int n, int blank)
{
    for (int k = 0; k < n; ++k)
        if (tok[k] != blank) return k;
    return -1;
}

// the loop's advance rule (rnnt/model.py:108-125; the host-side twin: rnnt_amd/model.py) after a scan of the n frames [t, t + n),
// `hit` = the first of them whose argmax is not blank, or -1:
//   none: t += n, emitted = 0                                  (an all-blank block)
//   else: t = the hit's frame (emitted = 0 if it moved), one more token — `append(position)` is the caller's store of it —, ++emitted;
//         emitted == max_per_frame: ++t, emitted = 0
//   done = t >= T or 1 + ntok >= maxlen
// (by value, in and out: the position lives in registers)
struct DecPos { int t, emitted, ntok, newtok, done; };
template <typename Append>
__device__ __forceinline__ DecPos dec_advance(int t, int emitted, int ntok, int hit, int n, int T, int maxlen, int max_per_frame,
                                              Append &&append)
{
    int newtok = 0;
    if (hit < 0) { t += n; emitted = 0; }
    else {
        if (hit > 0) emitted = 0;
        t += hit;
        append(++ntok);
        newtok = 1;
        if (++emitted >= max_per_frame) { ++t; emitted = 0; }
    }
    return DecPos{t, emitted, ntok, newtok, (t >= T || ntok + 1 >= maxlen) ? 1 : 0};
}
