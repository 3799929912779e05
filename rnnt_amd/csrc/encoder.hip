// encoder.hip — the Jasper AudioEncoder's inference forward (reference rnnt/jasper.py, rnnt/causalconv.py) on the device:
// whole utterances and streaming pushes.  Every layer is  causal conv -> [norm] -> [+ residual] -> [GELU]  and runs as two
// launches: a convolution kernel that leaves fp32 partial sums in slabs, and k_enc_norm<false>, which adds the slabs up in a
// fixed order and does everything else (bias, norm, residual, GELU, time-major store, the conv's next streaming state).
//
// The conv input X~ (N, C, len) is never built: it is `slen` frames of state (N, C, slen) — zeros for a whole utterance —
// followed by the chunk, each read with its own strides (EncSrc).  Output frame t, tap j reads X~ frame t*stride + j*dilation.
// Activations between layers are time-major [N][L][ldc] (ldc = channels rounded up to 4) so that a row of channels is one
// contiguous run; weights are packed once as [tap][out][in rounded up to 4, zero filled] (rnnt_engine_encoder_pack).
//
// Two convolution kernels:
//   k_enc_conv_few   N*L_out <= 64 rows (streaming pushes): a weight-streaming kernel.  The contraction (taps x C_in) is cut
//                    over workgroups by 64-channel chunk and tap range; a workgroup stages its chunk of X~ in LDS once, then
//                    streams its weights with one 16-byte load per lane per (tap, out channel) straight into registers and
//                    multiplies them into per-row accumulators.  Up to 16 rows each weight is loaded once per push; beyond that
//                    the row tiles of 16 walk the workgroup's weight slice (16 KB per tap) again — 2 passes at 25 rows, 4 at 64 —
//                    and whether the later passes are served by L2 has not been measured.
//   k_enc_conv_mfma  any number of rows (whole utterances): k_sgemm_nt's structure (smallgemm.hip) with the tap shift
//                    generalised to stride and dilation: v_mfma_f32_32x32x2_f32, exact fp32 products, the four waves split the
//                    contraction and add their tiles up through LDS in wave order.
// No atomics anywhere: the same inputs give the same bits.
// The second half of the file is the encoder's TRAINING (rnnt_engine_encoder_train_*): the same conv kernels, the same epilogue
// instantiated as k_enc_norm<true>, which also saves what the backward reads, and the backward's kernels; see "training" below.
#include "../../include/rnnt_engine.h"

#include <cstdint>

#include "kernels.hpp"
#include "smallgemm.hpp"

namespace {

constexpr int ENC_FEW_ROWS = 64;     // k_enc_conv_few: at most this many output rows (N * L_out) ...
constexpr int ENC_FEW_FRAMES = 224;  // ... and this many frames of X~ (N * len) in its LDS stage (224 x 64 floats = 56 KB)
constexpr int ENC_FEW_WGS = 256;     // workgroups a few-row conv aims for: one per CU
constexpr int ENC_MFMA_WGS = 512;    // workgroups the MFMA conv aims for by cutting the taps (at most ENC_MFMA_SPLITS ranges)
constexpr int ENC_MFMA_SPLITS = 8;
constexpr int ENC_NORM_LANES = 64;   // k_enc_norm: frame lanes per channel; a workgroup = 16 channels x ENC_NORM_LANES
constexpr int ENC_NORM_THREADS = 16 * ENC_NORM_LANES;

struct EncSrc {
    const float *st;   // state (N, C, slen) contiguous, or NULL: zeros
    int slen;          // frames of state in front of the chunk
    const float *x;    // chunk
    long xn, xc, xt;   // its strides (floats) per batch entry, channel, frame
    int xlen;          // its frames; frames behind the last read as zeros (only the training dX conv asks for any)
    int C;             // channels
};

__device__ __forceinline__ float enc_src(const EncSrc &s, int n, int c, int tau)
{
    if (tau < s.slen) return s.st ? s.st[((long)n * s.C + c) * s.slen + tau] : 0.f;
    if (tau - s.slen >= s.xlen) return 0.f;
    return s.x[n * s.xn + c * s.xc + (long)(tau - s.slen) * s.xt];
}

struct EncConv {
    EncSrc src;
    const float *wp;  // [taps][cout][cinp]
    int cinp, cout, taps, stride, dil;
    int N, Lout;      // output rows m = n * Lout + t
    float *slabs;     // [split][N * Lout][cout]
    int tsplit;       // tap ranges (few-row: per channel chunk), one slab each
    int xvec;         // mfma: the chunk's channels are contiguous and every row 16-byte aligned
};

__device__ __forceinline__ float gelu_exact(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }

// ---- few rows.  grid (ceil(cout/64), ceil(cinp/64), tsplit), 256 threads: lane & 15 = the channel quad of the chunk, tid >> 4 =
// one of 16 output channels per pass, 4 passes = 64 output channels.  Rows in tiles of 16 (64 accumulators per lane).
__global__ __launch_bounds__(256) void k_enc_conv_few(EncConv a)
{
    __shared__ f32x4 xs[ENC_FEW_FRAMES * 16];
    const int tid = threadIdx.x, quad = tid & 15, og = tid >> 4;
    const int o0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int j0 = (int)((long)a.taps * blockIdx.z / a.tsplit), j1 = (int)((long)a.taps * (blockIdx.z + 1) / a.tsplit);
    const int Lt = a.src.slen + a.src.xlen, frames = a.N * Lt, M = a.N * a.Lout;
    {   // stage X~[.., c0 .. c0+63, ..] as [frame][channel]
        float *xf = (float *)xs;
        const int cc = tid & 63, c = c0 + cc;
        for (int f = tid >> 6; f < frames; f += 4) {
            const int n = f / Lt, tau = f - n * Lt;
            xf[f * 64 + cc] = c < a.src.C ? enc_src(a.src, n, c, tau) : 0.f;
        }
    }
    __syncthreads();
    const bool cok = c0 + 4 * quad < a.cinp;
    const int split = blockIdx.y * a.tsplit + blockIdx.z;
    float *slab = a.slabs + (long)split * M * a.cout;
    for (int m0 = 0; m0 < M; m0 += 16) {
        int fb[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = min(m0 + r, M - 1), n = m / a.Lout, t = m - n * a.Lout;
            fb[r] = n * Lt + t * a.stride;
        }
        float acc[4][16];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[p][r] = 0.f;
        for (int j = j0; j < j1; ++j) {
            f32x4 w[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int o = o0 + 16 * p + og;
                w[p] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (cok && o < a.cout) w[p] = *(const f32x4 *)(a.wp + ((long)j * a.cout + o) * a.cinp + c0 + 4 * quad);
            }
            const int shift = j * a.dil;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (m0 + r >= M) continue;  // (uniform)
                const f32x4 x = xs[(fb[r] + shift) * 16 + quad];
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    acc[p][r] += w[p][0] * x[0] + w[p][1] * x[1] + w[p][2] * x[2] + w[p][3] * x[3];
            }
        }
        // sum over the 16 channel quads (lanes of one 16-lane row), fixed order; lane `quad` keeps row m0 + quad
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float mine = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[p][r];
                v += __shfl_xor(v, 8, 64);
                v += __shfl_xor(v, 4, 64);
                v += __shfl_xor(v, 2, 64);
                v += __shfl_xor(v, 1, 64);
                if (quad == r) mine = v;
            }
            const int m = m0 + quad, o = o0 + 16 * p + og;
            if (m < M && o < a.cout) slab[(long)m * a.cout + o] = mine;
        }
    }
}

// ---- any number of rows.  Wave tile 32 rows x 128 output channels (4 tiles of 32); grid (ceil(cout/128), ceil(M/32), tsplit):
// a workgroup takes one tap range (its own slab) and its 4 waves the contraction chunks (tap, 8 channels) c = wave, wave+4, ..;
// operands straight into registers, two chunks ahead.
__global__ __launch_bounds__(256) void k_enc_conv_mfma(EncConv a)
{
    __shared__ float red[4 * 1024];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 31, half = lane >> 5;
    const int M = a.N * a.Lout, N = a.cout, K = a.cinp, C = a.src.C;
    const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 128;
    const int row = min(m0 + i, M - 1), bn = row / a.Lout, t = row - bn * a.Lout;
    const int KC = (K + 7) / 8;
    const int j0 = (int)((long)a.taps * blockIdx.z / a.tsplit), j1 = (int)((long)a.taps * (blockIdx.z + 1) / a.tsplit);
    const int first = j0 * KC, total = (j1 - j0) * KC;  // this workgroup's chunks: first .. first + total - 1
    long wrow[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) wrow[q] = (long)min(n0 + 32 * q + i, N - 1) * K;

    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

    struct Ops { f32x4 x, w[4]; };
    auto load = [&](Ops &o, int cl) {
        const int c = first + cl;
        const int tap = c / KC, kc = c - tap * KC;
        const int k = 8 * kc + 4 * half;
        const bool kok = k < K;  // K % 4 == 0: a quad of packed weights exists or not as a whole
        const int kk = kok ? k : K - 4;
        const int tau = t * a.stride + tap * a.dil;
        o.x = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kok && tau - a.src.slen < a.src.xlen) {
            if (tau >= a.src.slen && a.xvec && k + 3 < C) {
                o.x = *(const f32x4 *)(a.src.x + bn * a.src.xn + (long)(tau - a.src.slen) * a.src.xt + k);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e < C) o.x[e] = enc_src(a.src, bn, k + e, tau);
            }
        }
        const float *wt = a.wp + (long)tap * N * K + kk;
#pragma unroll
        for (int q = 0; q < 4; ++q) o.w[q] = *(const f32x4 *)(wt + wrow[q]);
    };
    auto compute = [&](const Ops &o) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.x[s], o.w[q][s], acc[q], 0, 0, 0);
    };
    if (wave < total) {
        Ops cur, nxt, nx2;
        load(cur, wave);
        if (wave + 4 < total) load(nxt, wave + 4);
        for (int c = wave; c < total; c += 4) {
            if (c + 8 < total) load(nx2, c + 8);
            compute(cur);
            cur = nxt;
            nxt = nx2;
        }
    }
    // acc += the other waves' partial tiles, in wave order
#pragma unroll 1
    for (int w = 1; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[(q * 16 + r) * 64 + lane] = acc[q][r];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[q][r] += red[(q * 16 + r) * 64 + lane];
        }
        __syncthreads();
    }
    if (wave != 0) return;
    float *slab = a.slabs + (long)blockIdx.z * M * N;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int n = n0 + 32 * q + i;
        if (n >= N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (m < M) slab[(long)m * N + n] = acc[q][r];
        }
    }
}

// ---- the two sums every epilogue and k_enc_bwd_norm share.  v + s[0] + s[step] + .. + s[(n-1) step], added in index order, AHEAD
// slabs requested together: eight, but one in k_enc_norm<true>, which sees at most ENC_MFMA_SPLITS slabs and where eight loads in
// flight cost the registers that let two workgroups share a CU (80 VGPRs against 35).
template <int AHEAD = 8>
__device__ __forceinline__ float enc_slab_sum(float v, const float *s, int n, long step)
{
    int k = 0;
    for (; AHEAD > 1 && k + AHEAD <= n; k += AHEAD) {
        float p[AHEAD];
#pragma unroll
        for (int e = 0; e < AHEAD; ++e) p[e] = s[(long)(k + e) * step];
#pragma unroll
        for (int e = 0; e < AHEAD; ++e) v += p[e];
    }
    for (; k < n; ++k) v += s[(long)k * step];
    return v;
}

// the 64 frame lanes' partial sums of this thread's channel (tid & 15), in lane order; every thread of the workgroup calls it, and
// red[] is free again when it returns
__device__ __forceinline__ float enc_lane_sum(float s)
{
    __shared__ float red[ENC_NORM_THREADS];
    red[threadIdx.x] = s;
    __syncthreads();
    float r = 0.f;
    for (int k = 0; k < ENC_NORM_LANES; ++k) r += red[16 * k + (threadIdx.x & 15)];
    __syncthreads();
    return r;
}

// ---- everything after the products.  Blocks 0 .. nb_norm-1: block (channel group of 16, batch entry n), thread (channel
// tid & 15, frame lane tid >> 4 of 64): v = bias + the slabs in index order; instance norm: mean, then the biased variance about that
// mean (two passes over the frames of this call, partial sums combined in lane order); batch norm: the running statistics;
// gamma / beta; + residual; GELU; store time-major.  One body, two instantiations that give the same `out` bit for bit:
//   <false>  inference.  The conv output is parked in `out` between the passes.  Blocks behind nb_norm: the conv's next streaming
//            state, X~ from frame Lout * stride on, into a buffer of its own (N, C, slen_out).
//   <true>   training: whole utterances only (no state blocks).  Besides the layer's output it leaves z (the value in front of the
//            GELU), xhat (the normalised conv output; the conv output is parked in its place) and, for instance norm, rstd per
//            (n, channel); a keep mask [N][Lout][cout] (one byte per value) zeroes the output or scales it by `scale` = 1 / (1 - p).
struct EncNorm {
    const float *slabs; int nsplit;
    const float *bias, *gamma, *beta, *mean, *var;
    int norm; float eps;
    const float *res; long ldres;  // [N][Lout][ldres] or NULL
    int act;
    float *out; long ldo;          // [N][Lout][ldo]
    int N, Lout, cout, nb_norm;
    EncSrc src; float *state_out; int slen_out, stride;  // <false> only
    const uint8_t *keep; float scale;                    // <true> only, as the next line
    float *z, *xh, *rstd; long lds;  // z, xhat [N][Lout][lds]; rstd [N][cout]; NULL where the layer keeps none
};

template <bool TRAIN>
__global__ __launch_bounds__(ENC_NORM_THREADS) void k_enc_norm(EncNorm a)
{
    const int tid = threadIdx.x;
    if constexpr (!TRAIN) {
        if ((int)blockIdx.x >= a.nb_norm) {
            const long idx = (long)((int)blockIdx.x - a.nb_norm) * ENC_NORM_THREADS + tid;
            const long total = (long)a.N * a.src.C * a.slen_out;
            if (idx >= total) return;
            const int p = (int)(idx % a.slen_out);
            const long nc = idx / a.slen_out;
            const int c = (int)(nc % a.src.C), n = (int)(nc / a.src.C);
            a.state_out[idx] = enc_src(a.src, n, c, a.Lout * a.stride + p);
            return;
        }
    }
    const int cl = tid & 15, tl = tid >> 4;
    const int cgroups = (a.cout + 15) / 16;
    const int n = (int)blockIdx.x / cgroups, c = ((int)blockIdx.x - n * cgroups) * 16 + cl;
    const bool ok = c < a.cout;
    const long M = (long)a.N * a.Lout, row0 = (long)n * a.Lout;
    const float b = ok && a.bias ? a.bias[c] : 0.f;
    auto pre = [&](int t) {
        const float *s = a.slabs + (row0 + t) * a.cout + c;
        const long step = M * a.cout;
        return enc_slab_sum<TRAIN ? 1 : 8>(s[0], s + step, a.nsplit - 1, step) + b;
    };
    float *const park = TRAIN ? a.xh : a.out;  // the conv output between the passes; each thread reads back what it wrote
    const long ldp = TRAIN ? a.lds : a.ldo;
    float mu = 0.f, rstd = 1.f;
    const bool inst = a.norm == RNNT_ENC_NORM_INSTANCE;
    if (inst) {
        float s = 0.f;
        if (ok)
            for (int t = tl; t < a.Lout; t += ENC_NORM_LANES) {
                const float v = pre(t);
                park[(row0 + t) * ldp + c] = v;
                s += v;
            }
        mu = enc_lane_sum(s) / (float)a.Lout;
        float q = 0.f;
        if (ok)
            for (int t = tl; t < a.Lout; t += ENC_NORM_LANES) {
                const float d = park[(row0 + t) * ldp + c] - mu;
                q += d * d;
            }
        rstd = 1.f / sqrtf(enc_lane_sum(q) / (float)a.Lout + a.eps);
        if constexpr (TRAIN)
            if (ok && tl == 0) a.rstd[(long)n * a.cout + c] = rstd;
    } else if (a.norm == RNNT_ENC_NORM_BATCH && ok) {
        mu = a.mean[c];
        rstd = 1.f / sqrtf(a.var[c] + a.eps);
    }
    if (!ok) return;
    const float g = a.norm != RNNT_ENC_NORM_NONE && a.gamma ? a.gamma[c] : 1.f;
    const float be = a.norm != RNNT_ENC_NORM_NONE && a.beta ? a.beta[c] : 0.f;
    for (int t = tl; t < a.Lout; t += ENC_NORM_LANES) {
        const long row = row0 + t;
        float v = inst ? park[row * ldp + c] : pre(t);
        if (a.norm != RNNT_ENC_NORM_NONE) {
            v = (v - mu) * rstd;
            if constexpr (TRAIN) a.xh[row * a.lds + c] = v;
            v = v * g + be;
        }
        if (a.res) v += a.res[row * a.ldres + c];
        if (a.act) {
            if constexpr (TRAIN) a.z[row * a.lds + c] = v;
            v = gelu_exact(v);
        }
        if constexpr (TRAIN)
            if (a.keep) v = a.keep[row * a.cout + c] ? v * a.scale : 0.f;
        a.out[row * a.ldo + c] = v;
    }
}

// The packed tables, [tap][rows][cols rounded up to 4, zero filled].  The convs' table: rows = out channels, cols = in channels.
// transposed: the dX conv's, k_enc_conv_mfma's layout with in and out exchanged and the taps reversed.
__global__ __launch_bounds__(256) void k_enc_pack(const float *__restrict__ w, float *__restrict__ wp, int out_c, int in_c, int taps,
                                                  int transposed)
{
    const int rows = transposed ? in_c : out_c, cols = transposed ? out_c : in_c, colp = (cols + 3) & ~3;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // walks the packed layout
    if (idx >= (long)taps * rows * colp) return;
    const int col = (int)(idx % colp);
    const long tr = idx / colp;
    const int r = (int)(tr % rows), t = (int)(tr / rows);
    const int co = transposed ? col : r, ci = transposed ? r : col;
    wp[idx] = col < cols ? w[((long)co * in_c + ci) * taps + (transposed ? taps - 1 - t : t)] : 0.f;
}


// =============================================================================================================== training
// rnnt_engine_encoder_train_*: a forward that keeps what the backward reads, and the backward.  Per layer the
// forward is the conv kernel above and k_enc_norm<true>; the backward is k_enc_bwd_norm (dO -> dz -> dy, the per-entry partial
// sums of dgamma / dbeta / dbias, the copy of dz into the residual branch, the sum of the two dx of a block input), k_enc_dw (the
// weight gradient's products, one slab per row range), k_enc_bwd_sum (slabs and partial sums added in index order, dW stored in
// torch's [out][in][tap]) and, for every layer but those that read the list's input, k_enc_conv_mfma over dy with the second
// packed table [tap reversed][in][out rounded up to 4].  Every sum has a fixed order.
constexpr int ENC_DW_WGS = 512;    // workgroups k_enc_dw aims for by cutting the rows ...
constexpr int ENC_DW_RANGES = 16;  // ... into at most this many ranges, each a multiple of ...
constexpr int ENC_DW_STEP = 8;     // ... the rows of one pipeline step

__device__ __forceinline__ float gelu_grad(float z)  // Phi(z) + z phi(z)
{
    return 0.5f * (1.f + erff(z * 0.70710678118654752f)) + z * 0.3989422804014327f * expf(-0.5f * z * z);
}

// ---- dO -> dz -> dy of one layer.  Block (channel group of 16, batch entry n), thread (channel, frame lane), as k_enc_norm.
// dO[row][c] = the slabs of source a in index order, then those of source b (the two dx of a block input: first layer's, then the
// residual 1x1's); a caller's gradient or the residual branch's is a source of one slab.
struct EncGradSrc { const float *p; int nsplit; long split, ld; };
struct EncNormB {
    EncGradSrc a, b;
    const uint8_t *keep; float scale;
    const float *z; int act;
    const float *xh, *rstd, *gamma, *var;
    int norm; float eps; long lds;
    float *dy; long ldy;
    float *dres; long ldres;  // LAST layers: dz, the residual layer's dO; else NULL
    float *part;              // [3][N][cout]: sum_t dz xhat, sum_t dz, sum_t dy of batch entry n
    int N, Lout, cout;
};

__global__ __launch_bounds__(ENC_NORM_THREADS) void k_enc_bwd_norm(EncNormB a)
{
    const int tid = threadIdx.x, cl = tid & 15, tl = tid >> 4;
    const int cgroups = (a.cout + 15) / 16;
    const int n = (int)blockIdx.x / cgroups, c = ((int)blockIdx.x - n * cgroups) * 16 + cl;
    const bool ok = c < a.cout;
    const long row0 = (long)n * a.Lout;
    const bool normed = a.norm != RNNT_ENC_NORM_NONE;
    float s1 = 0.f, s2 = 0.f;
    if (ok)
        for (int t = tl; t < a.Lout; t += ENC_NORM_LANES) {
            const long row = row0 + t;
            const float *s = a.a.p + row * a.a.ld + c;
            float v = enc_slab_sum(s[0], s + a.a.split, a.a.nsplit - 1, a.a.split);
            if (a.b.p) v = enc_slab_sum(v, a.b.p + row * a.b.ld + c, a.b.nsplit, a.b.split);
            if (a.keep) v = a.keep[row * a.cout + c] ? v * a.scale : 0.f;
            if (a.act) v *= gelu_grad(a.z[row * a.lds + c]);
            a.dy[row * a.ldy + c] = v;  // dz, parked; this thread reads it back below
            if (a.dres) a.dres[row * a.ldres + c] = v;
            s1 += v;
            if (normed) s2 += v * a.xh[row * a.lds + c];
        }
    const float S1 = enc_lane_sum(s1), S2 = enc_lane_sum(s2);
    float s3 = 0.f;
    if (ok) {
        const float gam = normed && a.gamma ? a.gamma[c] : 1.f;
        if (a.norm == RNNT_ENC_NORM_INSTANCE) {
            const float rs = a.rstd[(long)n * a.cout + c], inv = 1.f / (float)a.Lout;
            const float mg = gam * S1 * inv, mgx = gam * S2 * inv;  // mean_t g, mean_t (g xhat) with g = dz gamma
            for (int t = tl; t < a.Lout; t += ENC_NORM_LANES) {
                const long row = row0 + t;
                const float v = rs * (a.dy[row * a.ldy + c] * gam - mg - a.xh[row * a.lds + c] * mgx);
                a.dy[row * a.ldy + c] = v;
                s3 += v;
            }
        } else {
            const float f = a.norm == RNNT_ENC_NORM_BATCH ? gam * (1.f / sqrtf(a.var[c] + a.eps)) : 1.f;
            for (int t = tl; t < a.Lout; t += ENC_NORM_LANES) {
                const long row = row0 + t;
                const float v = a.dy[row * a.ldy + c] * f;
                a.dy[row * a.ldy + c] = v;
                s3 += v;
            }
        }
    }
    const float S3 = enc_lane_sum(s3);
    if (ok && tl == 0) {
        const long NC = (long)a.N * a.cout, at = (long)n * a.cout + c;
        a.part[at] = S2;
        a.part[NC + at] = S1;
        a.part[2 * NC + at] = S3;
    }
}

// ---- the weight gradient's products.  dW[o][i][j] = sum over the rows m = (n, t) of dy[m][o] X~[n][t*stride + j*dil][i]: per tap
// a cout x cin product contracted over the rows, v_mfma_f32_32x32x2_f32 with A = dy^T (lane: out channel, row parity) and
// B = the tap-shifted input (lane: in channel, row parity).  grid (taps * ranges, ceil(cin/128), ceil(cout/128)); a workgroup's four
// waves take 32 out channels each by the same 128 in channels, so nothing is shared but cache lines and nothing is reduced
// between waves: every element is one wave's fmaf chain over its row range, in row order.  Each row finds its own (n, t), so a
// step whose rows cross from one batch entry to the next reads each entry's own frames; a row whose frame lies in the zero lead,
// or behind the range's end, gives a zero operand and is not read.  Slab [range][tap][out][in].
struct EncDW {
    EncSrc src;       // the layer's input; src.slen = lead, src.st = NULL
    const float *dy; long ldy;
    int cout, taps, stride, dil, N, Lout;
    float *slabs;
    int ranges, rows;  // row ranges and rows per range (a multiple of ENC_DW_STEP)
};

__global__ __launch_bounds__(256) void k_enc_dw(EncDW a)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 31, half = lane >> 5;
    const int o0 = blockIdx.z * 128 + 32 * wave, i0 = blockIdx.y * 128;
    if (o0 >= a.cout) return;
    const int cin = a.src.C, M = a.N * a.Lout;
    const int tap = (int)blockIdx.x / a.ranges, rg = (int)blockIdx.x - tap * a.ranges;
    const int m0 = rg * a.rows, m1 = min(M, m0 + a.rows);
    const bool ook = o0 + i < a.cout;
    const float *dyc = a.dy + min(o0 + i, a.cout - 1);
    bool cok[4];
    long xcol[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ci = i0 + 32 * q + i;
        cok[q] = ci < cin;
        xcol[q] = (long)min(ci, cin - 1) * a.src.xc;
    }
    const int shift = tap * a.dil - a.src.slen;  // input frame of output frame t: t * stride + shift

    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

    struct Ops { float d[ENC_DW_STEP / 2], x[ENC_DW_STEP / 2][4]; };
    auto load = [&](Ops &o, int m) {
#pragma unroll
        for (int s = 0; s < ENC_DW_STEP / 2; ++s) {
            const int row = m + 2 * s + half;
            const bool live = row < m1;
            const int rr = live ? row : m1 - 1;
            const int n = rr / a.Lout, t = rr - n * a.Lout;
            const int f = t * a.stride + shift;
            o.d[s] = live && ook ? dyc[(long)rr * a.ldy] : 0.f;
            const bool xl = live && f >= 0;
            const float *xp = a.src.x + n * a.src.xn + (long)(xl ? f : 0) * a.src.xt;
#pragma unroll
            for (int q = 0; q < 4; ++q) o.x[s][q] = xl && cok[q] ? xp[xcol[q]] : 0.f;
        }
    };
    Ops cur, nxt;
    load(cur, m0);
    for (int m = m0; m < m1; m += ENC_DW_STEP) {
        if (m + ENC_DW_STEP < m1) load(nxt, m + ENC_DW_STEP);
#pragma unroll
        for (int s = 0; s < ENC_DW_STEP / 2; ++s)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.d[s], cur.x[s][q], acc[q], 0, 0, 0);
        cur = nxt;
    }
    float *slab = a.slabs + ((long)rg * a.taps + tap) * a.cout * cin;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ci = i0 + 32 * q + i;
        if (ci >= cin) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = o0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (o < a.cout) slab[(long)o * cin + ci] = acc[q][r];
        }
    }
}

// ---- the sums that close a layer's backward.  Blocks 0 .. nb_w-1: thread = one element of a slab [tap][out][in]; the ranges' slabs
// in index order, stored at dW[out][in][tap].  Blocks behind those: thread = (which of dgamma / dbeta / dbias, channel): the batch
// entries' partial sums in index order.
struct EncSumB {
    const float *slabs; int ranges, taps, cout, cin;
    float *dw;           // [cout][cin][taps] or NULL
    int nb_w;
    const float *part; int N;
    float *dst[3];       // dgamma, dbeta, dbias or NULL
};

__global__ __launch_bounds__(256) void k_enc_bwd_sum(EncSumB a)
{
    if ((int)blockIdx.x < a.nb_w) {
        const long per = (long)a.taps * a.cout * a.cin;
        const long idx = (long)blockIdx.x * 256 + threadIdx.x;
        if (idx >= per) return;
        float v = a.slabs[idx];
        for (int r = 1; r < a.ranges; ++r) v += a.slabs[(long)r * per + idx];
        const int ci = (int)(idx % a.cin);
        const long to = idx / a.cin;
        const int o = (int)(to % a.cout), t = (int)(to / a.cout);
        a.dw[((long)o * a.cin + ci) * a.taps + t] = v;
        return;
    }
    const int idx = ((int)blockIdx.x - a.nb_w) * 256 + threadIdx.x;
    if (idx >= 3 * a.cout) return;
    const int which = idx / a.cout, c = idx - which * a.cout;
    if (!a.dst[which]) return;
    const float *p = a.part + (long)which * a.N * a.cout + c;
    float v = p[0];
    for (int n = 1; n < a.N; ++n) v += p[(long)n * a.cout];
    a.dst[which][c] = v;
}

// ---------------------------------------------------------------------------------------------------------------- host side
#define fail engine_fail

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }
inline int pad4(int c) { return (c + 3) & ~3; }
inline bool is_1x1(const rnnt_encoder_layer &l) { return (l.role & (RNNT_ENC_ROLE_RESIDUAL | RNNT_ENC_ROLE_FINAL)) != 0; }

int check_layers(const rnnt_encoder_layer *layers, int n_layers)
{
    if (!layers) return fail(RNNT_ERR_INVALID_ARG, "null layer list");
    if (n_layers < 1 || n_layers > RNNT_ENC_MAX_LAYERS)
        return fail(RNNT_ERR_INVALID_ARG, "empty or too long layer list (n_layers=%d, 1 .. %d)", n_layers, RNNT_ENC_MAX_LAYERS);
    int c = layers[0].cin, res_c = 0;
    bool in_block = false, want_first = false;
    for (int i = 0; i < n_layers; ++i) {
        const rnnt_encoder_layer &l = layers[i];
        if (l.taps < 1) return fail(RNNT_ERR_INVALID_ARG, "layer %d: taps=%d must be >= 1", i, l.taps);
        if (l.stride < 1) return fail(RNNT_ERR_INVALID_ARG, "layer %d: stride=%d must be >= 1", i, l.stride);
        if (l.dilation < 1) return fail(RNNT_ERR_INVALID_ARG, "layer %d: dilation=%d must be >= 1", i, l.dilation);
        if (l.cin < 1 || l.cout < 1) return fail(RNNT_ERR_INVALID_ARG, "layer %d: non-positive channels cin=%d cout=%d", i, l.cin, l.cout);
        if ((long)l.taps * l.dilation > 4096 || l.stride > 64 || l.cin > 65536 || l.cout > 65536)
            return fail(RNNT_ERR_UNSUPPORTED, "layer %d: taps * dilation <= 4096, stride <= 64, channels <= 65536", i);
        if (l.norm != RNNT_ENC_NORM_NONE && l.norm != RNNT_ENC_NORM_BATCH && l.norm != RNNT_ENC_NORM_INSTANCE)
            return fail(RNNT_ERR_INVALID_ARG, "layer %d: norm kind %d", i, l.norm);
        if (l.norm != RNNT_ENC_NORM_NONE && !(l.eps > 0.f)) return fail(RNNT_ERR_INVALID_ARG, "layer %d: eps must be > 0", i);
        if (l.cin != c) return fail(RNNT_ERR_INVALID_ARG, "layer %d: inconsistent list, cin=%d but the previous cout is %d", i, l.cin, c);
        const int role = l.role;
        if (role != RNNT_ENC_ROLE_PLAIN && role != RNNT_ENC_ROLE_FIRST && role != RNNT_ENC_ROLE_LAST &&
            role != (RNNT_ENC_ROLE_FIRST | RNNT_ENC_ROLE_LAST) && role != RNNT_ENC_ROLE_RESIDUAL && role != RNNT_ENC_ROLE_FINAL)
            return fail(RNNT_ERR_INVALID_ARG, "layer %d: role %d", i, role);
        if (want_first && !(role & RNNT_ENC_ROLE_FIRST))
            return fail(RNNT_ERR_INVALID_ARG, "layer %d: inconsistent list, a residual 1x1 must be followed by its block's first layer", i);
        if (role == RNNT_ENC_ROLE_RESIDUAL) {
            if (in_block) return fail(RNNT_ERR_INVALID_ARG, "layer %d: inconsistent list, residual 1x1 inside a block", i);
            if (l.taps != 1 || l.stride != 1) return fail(RNNT_ERR_INVALID_ARG, "layer %d: a residual layer is a 1x1 conv of stride 1", i);
            res_c = l.cout;
            want_first = true;
            continue;  // the block's first layer reads the same input
        }
        if (role & RNNT_ENC_ROLE_FIRST) {
            if (!want_first) return fail(RNNT_ERR_INVALID_ARG, "layer %d: inconsistent list, a block's first layer needs its residual 1x1 in front", i);
            want_first = false;
            in_block = true;
        } else if (role == RNNT_ENC_ROLE_FINAL) {
            if (l.taps != 1 || l.stride != 1) return fail(RNNT_ERR_INVALID_ARG, "layer %d: the final layer is a 1x1 conv of stride 1", i);
            if (i != n_layers - 1) return fail(RNNT_ERR_INVALID_ARG, "layer %d: inconsistent list, the final 1x1 is not the last layer", i);
        }
        if ((role & RNNT_ENC_ROLE_LAST) && !in_block)
            return fail(RNNT_ERR_INVALID_ARG, "layer %d: inconsistent list, last-of-block outside a block", i);
        if (in_block && l.stride != 1) return fail(RNNT_ERR_UNSUPPORTED, "layer %d: stride %d inside a residual block", i, l.stride);
        if (role & RNNT_ENC_ROLE_LAST) {
            if (l.cout != res_c) return fail(RNNT_ERR_INVALID_ARG, "layer %d: inconsistent list, cout=%d but the residual branch has %d", i, l.cout, res_c);
            in_block = false;
        }
        c = l.cout;
    }
    if (want_first || in_block) return fail(RNNT_ERR_INVALID_ARG, "inconsistent list: it ends inside a block");
    return RNNT_OK;
}

// floats of one layer's packed table (k_enc_pack), a multiple of 256 bytes
size_t packed_floats(const rnnt_encoder_layer &l, bool transposed)
{
    const int rows = transposed ? l.cin : l.cout, cols = transposed ? l.cout : l.cin;
    return align_up((size_t)l.taps * rows * pad4(cols) * 4) / 4;
}

// tap ranges of an MFMA conv: aim for ENC_MFMA_WGS workgroups, at most `taps`, at most ENC_MFMA_SPLITS
int mfma_tap_split(long rows, int cout, int taps)
{
    const long wgs = ((cout + 127) / 128) * ((rows + 31) / 32);
    long ts = (ENC_MFMA_WGS + wgs - 1) / wgs;
    ts = ts > taps ? taps : ts;
    return (int)(ts > ENC_MFMA_SPLITS ? ENC_MFMA_SPLITS : ts);
}

// lengths, kernel choice and workspace of one call; state_lens NULL: whole utterance (every state is (taps-1)*dilation-stride+1 zeros)
struct Plan {
    int Lin[RNNT_ENC_MAX_LAYERS], Lout[RNNT_ENC_MAX_LAYERS], slen[RNNT_ENC_MAX_LAYERS], slen_out[RNNT_ENC_MAX_LAYERS];
    bool few[RNNT_ENC_MAX_LAYERS];
    int tsplit[RNNT_ENC_MAX_LAYERS], nsplit[RNNT_ENC_MAX_LAYERS];
    size_t act, res, slab, total;  // floats: one activation buffer (two are carved), the residual buffer, the slabs
    int L_final;
};

int make_plan(const rnnt_encoder_layer *layers, int n_layers, int N, int L, const int32_t *state_lens, int regime, Plan &P)
{
    if (N < 1 || L < 1) return fail(RNNT_ERR_INVALID_ARG, "non-positive N=%d or L=%d", N, L);
    if (regime != RNNT_ENC_REGIME_AUTO && regime != RNNT_ENC_REGIME_MANY_ROWS) return fail(RNNT_ERR_INVALID_ARG, "regime %d", regime);
    long cur = L;
    size_t act = 0, res = 0, slab = 0;
    for (int i = 0; i < n_layers; ++i) {
        const rnnt_encoder_layer &l = layers[i];
        const int span = (l.taps - 1) * l.dilation, pad = span - l.stride + 1;
        long slen = 0;
        if (!is_1x1(l)) {
            if (state_lens) {
                if (state_lens[i] < 0 || state_lens[i] > (1 << 20))
                    return fail(RNNT_ERR_INVALID_ARG, "layer %d: state length %d outside 0 .. 2^20", i, state_lens[i]);
                slen = state_lens[i];
            } else {
                if (pad < 0) return fail(RNNT_ERR_UNSUPPORTED, "layer %d: stride %d beyond the kernel's span", i, l.stride);
                slen = pad;
            }
        }
        const long Lt = slen + cur;
        if (Lt < span + 1) return fail(RNNT_ERR_INVALID_ARG, "layer %d: %ld frames of state and input are too short for one output frame (needs %d)", i, Lt, span + 1);
        const long Lout = (Lt - span - 1) / l.stride + 1;
        if (l.norm == RNNT_ENC_NORM_INSTANCE && Lout == 1)
            return fail(RNNT_ERR_INVALID_ARG, "layer %d: instance norm over a single output frame (its variance is undefined)", i);
        const long M = (long)N * Lout;
        if (M > 65535L * 32 || (long)N * Lt > 0x7fffffffL / 4) return fail(RNNT_ERR_UNSUPPORTED, "N * L too large");
        P.Lin[i] = (int)cur; P.Lout[i] = (int)Lout; P.slen[i] = (int)slen;
        P.slen_out[i] = is_1x1(l) ? 0 : (int)(Lt - Lout * l.stride);
        P.few[i] = regime == RNNT_ENC_REGIME_AUTO && M <= ENC_FEW_ROWS && (long)N * Lt <= ENC_FEW_FRAMES;
        if (P.few[i]) {
            const int wgs = ((l.cout + 63) / 64) * ((pad4(l.cin) + 63) / 64);
            int ts = (ENC_FEW_WGS + wgs - 1) / wgs;
            ts = ts > l.taps ? l.taps : ts;
            P.tsplit[i] = ts;
            P.nsplit[i] = ((pad4(l.cin) + 63) / 64) * ts;
        } else {
            P.tsplit[i] = P.nsplit[i] = mfma_tap_split(M, l.cout, l.taps);
        }
        const size_t s = (size_t)P.nsplit[i] * M * l.cout;
        slab = s > slab ? s : slab;
        const size_t o = (size_t)M * pad4(l.cout);
        if (l.role == RNNT_ENC_ROLE_RESIDUAL) { res = o > res ? o : res; continue; }
        if (l.role != RNNT_ENC_ROLE_FINAL) act = o > act ? o : act;
        cur = Lout;
    }
    P.L_final = (int)cur;
    P.act = align_up(act * 4) / 4; P.res = align_up(res * 4) / 4; P.slab = align_up(slab * 4) / 4;
    P.total = (2 * P.act + P.res + P.slab) * 4;
    return RNNT_OK;
}

int status(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RNNT_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return RNNT_OK;
}

// what the run entries check of their buffers (saved: the training entries') and of a layer's parameters
int check_buffers(const void *packed, const float *x, const int64_t xs[3], const void *io, const void *ws, const void *saved, bool train)
{
    if (!packed || !x || !xs || !io || !ws || (train && !saved)) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    if (((uintptr_t)packed & 15) || ((uintptr_t)ws & 15) || ((uintptr_t)saved & 15) || ((uintptr_t)x & 3) || ((uintptr_t)io & 3))
        return fail(RNNT_ERR_INVALID_ARG, train ? "packed weights, saved and workspace must be 16-byte aligned, x and out / dout 4-byte"
                                                : "packed weights and workspace must be 16-byte aligned, x and out 4-byte");
    return RNNT_OK;
}

int check_params(const rnnt_encoder_layer &l, int i)
{
    if (!l.bias) return fail(RNNT_ERR_INVALID_ARG, "layer %d: null bias", i);
    if (l.norm == RNNT_ENC_NORM_BATCH && (!l.mean || !l.var)) return fail(RNNT_ERR_INVALID_ARG, "layer %d: batch norm without running statistics", i);
    return RNNT_OK;
}

// Where a layer reads its chunk (the caller sets src.st / src.slen) and whether k_enc_conv_mfma may read its rows as float4:
// the caller's x with its strides, or a time-major activation [N][len][ld] of the engine's own.
struct EncIn { EncSrc src; bool vec; };

EncIn caller_x(const float *x, const int64_t xs[3], int L, int C)
{
    return {{nullptr, 0, x, (long)xs[0], (long)xs[1], (long)xs[2], L, C},
            xs[1] == 1 && xs[0] % 4 == 0 && xs[2] % 4 == 0 && ((uintptr_t)x & 15) == 0};
}

EncIn time_major(const float *p, long ld, int len, int C) { return {{nullptr, 0, p, (long)len * ld, 1, ld, len, C}, true}; }

// the conv of `in` with the table wp [taps][cout][in's channels rounded up to 4] into `tsplit` slabs, and its launch
EncConv conv_args(const EncIn &in, const float *wp, int cout, int taps, int stride, int dil, int N, int Lout, float *slabs, int tsplit)
{
    EncConv c;
    c.src = in.src; c.wp = wp; c.cinp = pad4(in.src.C); c.cout = cout; c.taps = taps; c.stride = stride; c.dil = dil;
    c.N = N; c.Lout = Lout; c.slabs = slabs; c.tsplit = tsplit; c.xvec = in.vec;
    return c;
}

void launch_conv(const EncConv &c, bool few, hipStream_t st)
{
    if (few)
        hipLaunchKernelGGL(k_enc_conv_few, dim3((c.cout + 63) / 64, (c.cinp + 63) / 64, c.tsplit), dim3(256), 0, st, c);
    else
        hipLaunchKernelGGL(k_enc_conv_mfma, dim3((c.cout + 127) / 128, (unsigned)(((long)c.N * c.Lout + 31) / 32), c.tsplit), dim3(256), 0, st, c);
}

// the epilogue of layer i into out [N][Lout][ldo], either instantiation's: the caller adds the state blocks or what training keeps
EncNorm norm_args(const rnnt_encoder_layer &l, const Plan &P, int i, int N, const float *slabs, const float *res, float *out, long ldo)
{
    EncNorm nm = {};
    nm.slabs = slabs; nm.nsplit = P.nsplit[i];
    nm.bias = (const float *)l.bias; nm.gamma = (const float *)l.gamma; nm.beta = (const float *)l.beta;
    nm.mean = (const float *)l.mean; nm.var = (const float *)l.var; nm.norm = l.norm; nm.eps = l.eps;
    nm.res = (l.role & RNNT_ENC_ROLE_LAST) ? res : nullptr; nm.ldres = pad4(l.cout);
    nm.act = !is_1x1(l);
    nm.out = out; nm.ldo = ldo; nm.N = N; nm.Lout = P.Lout[i]; nm.cout = l.cout;
    nm.nb_norm = N * ((l.cout + 15) / 16);
    return nm;
}

int run(const char *what, const rnnt_encoder_layer *layers, int n_layers, const void *packed, const float *x, const int64_t xs[3],
        int N, int L, void *const *state_in, const int32_t *state_in_lens, void *const *state_out, const int32_t *state_out_lens,
        int regime, float *out, void *ws, size_t ws_bytes, void *stream)
{
    if (int rc = check_layers(layers, n_layers)) return rc;
    if (int rc = check_buffers(packed, x, xs, out, ws, nullptr, false)) return rc;
    const bool streaming = state_in_lens != nullptr;
    if (streaming && (!state_in || !state_out || !state_out_lens)) return fail(RNNT_ERR_INVALID_ARG, "null state argument");
    Plan P;
    if (int rc = make_plan(layers, n_layers, N, L, state_in_lens, regime, P)) return rc;
    if (ws_bytes < P.total) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, P.total);
    for (int i = 0; i < n_layers; ++i) {
        const rnnt_encoder_layer &l = layers[i];
        if (int rc = check_params(l, i)) return rc;
        if (streaming && !is_1x1(l)) {
            if (state_out_lens[i] != P.slen_out[i])
                return fail(RNNT_ERR_INVALID_ARG, "layer %d: state_out length %d, this push leaves %d", i, state_out_lens[i], P.slen_out[i]);
            if ((P.slen[i] > 0 && !state_in[i]) || (P.slen_out[i] > 0 && !state_out[i]))
                return fail(RNNT_ERR_INVALID_ARG, "layer %d: null state pointer", i);
            if (P.slen_out[i] > 0 && state_out[i] == state_in[i]) return fail(RNNT_ERR_INVALID_ARG, "layer %d: the state is never updated in place", i);
        }
    }
    hipStream_t st = (hipStream_t)stream;
    float *w = (float *)ws;
    float *buf[2] = {w, w + P.act}, *res = w + 2 * P.act, *slabs = res + P.res;
    const float *wp = (const float *)packed;
    EncIn cur = caller_x(x, xs, L, layers[0].cin);
    int flip = 0;
    for (int i = 0; i < n_layers; ++i) {
        const rnnt_encoder_layer &l = layers[i];
        const int Lout = P.Lout[i];
        cur.src.st = streaming && P.slen[i] > 0 ? (const float *)state_in[i] : nullptr;
        cur.src.slen = P.slen[i];
        launch_conv(conv_args(cur, wp, l.cout, l.taps, l.stride, l.dilation, N, Lout, slabs, P.tsplit[i]), P.few[i], st);

        const bool to_res = l.role == RNNT_ENC_ROLE_RESIDUAL;
        const bool to_out = i == n_layers - 1;  // the list's last layer, FINAL or not, leaves `out` [N][L_out][cout]
        float *dst = to_out ? out : to_res ? res : buf[flip];
        const long ldo = to_out ? l.cout : pad4(l.cout);
        EncNorm nm = norm_args(l, P, i, N, slabs, res, dst, ldo);
        nm.src = cur.src; nm.stride = l.stride;
        const bool wr_state = streaming && !is_1x1(l) && P.slen_out[i] > 0;
        nm.state_out = wr_state ? (float *)state_out[i] : nullptr;
        nm.slen_out = wr_state ? P.slen_out[i] : 0;
        const long nb_state = wr_state ? ((long)N * l.cin * P.slen_out[i] + ENC_NORM_THREADS - 1) / ENC_NORM_THREADS : 0;
        hipLaunchKernelGGL(k_enc_norm<false>, dim3((unsigned)(nm.nb_norm + nb_state)), dim3(ENC_NORM_THREADS), 0, st, nm);

        wp += packed_floats(l, false);
        if (to_res) continue;
        cur = time_major(dst, ldo, Lout, l.cout);
        flip ^= 1;
    }
    return status(what);
}

// ---- training: host side
inline bool reads_input(const rnnt_encoder_layer *layers, int i) { return i == 0 || (i == 1 && layers[0].role == RNNT_ENC_ROLE_RESIDUAL); }
constexpr size_t NOT_KEPT = ~(size_t)0;

// The forward's Plan with `lead` for the state lengths, the layout of `saved`, and the backward's splits and workspace.
struct TrainPlan {
    Plan P;
    int32_t lead[RNNT_ENC_MAX_LAYERS];
    int in_of[RNNT_ENC_MAX_LAYERS];                                 // the layer whose output layer i reads; -1: x
    size_t off_o[RNNT_ENC_MAX_LAYERS], off_z[RNNT_ENC_MAX_LAYERS];  // floats into `saved`, or NOT_KEPT
    size_t off_xh[RNNT_ENC_MAX_LAYERS], off_rstd[RNNT_ENC_MAX_LAYERS];
    size_t saved;                                                   // bytes
    int dx_split[RNNT_ENC_MAX_LAYERS];                              // tap ranges of the dX conv; 0: no dX
    int dw_ranges[RNNT_ENC_MAX_LAYERS], dw_rows[RNNT_ENC_MAX_LAYERS];
    size_t dy, dres, x1, x2, dw, part;                              // floats, each a multiple of 256 bytes
    size_t ws_fwd, ws_bwd;                                          // bytes; the size query answers the larger
};

int make_train_plan(const rnnt_encoder_layer *layers, int n_layers, int N, int L, const int32_t *lead, int regime, TrainPlan &T)
{
    for (int i = 0; i < n_layers; ++i) {
        const rnnt_encoder_layer &l = layers[i];
        const int pad = (l.taps - 1) * l.dilation - l.stride + 1;
        T.lead[i] = 0;
        if (is_1x1(l)) continue;
        if (pad < 0) return fail(RNNT_ERR_UNSUPPORTED, "layer %d: stride %d beyond the kernel's span", i, l.stride);
        T.lead[i] = lead ? lead[i] : pad;
        if (T.lead[i] < 0 || T.lead[i] > pad)
            return fail(RNNT_ERR_INVALID_ARG, "layer %d: lead %d outside 0 .. %d = (taps-1)*dilation - stride + 1", i, T.lead[i], pad);
        if (!reads_input(layers, i) && l.stride != 1)
            return fail(RNNT_ERR_UNSUPPORTED, "layer %d: stride %d behind the list's first layer (dX exists for stride 1 only)", i, l.stride);
    }
    if (int rc = make_plan(layers, n_layers, N, L, T.lead, regime, T.P)) return rc;
    for (int i = 0, res = 0; i < n_layers; ++i) {  // a block's last layer adds the residual branch frame by frame
        if (layers[i].role == RNNT_ENC_ROLE_RESIDUAL) res = i;
        if ((layers[i].role & RNNT_ENC_ROLE_LAST) && T.P.Lout[i] != T.P.Lout[res])
            return fail(RNNT_ERR_INVALID_ARG, "layer %d: lead (look-ahead) inside a block leaves %d frames, its residual branch has %d", i,
                        T.P.Lout[i], T.P.Lout[res]);
    }
    size_t off = 0, dy = 0, dres = 0, x1 = 0, x2 = 0, dw = 0, part = 0;
    auto take = [&](size_t floats) { const size_t at = off; off += align_up(floats * 4) / 4; return at; };
    int cur = -1;
    for (int i = 0; i < n_layers; ++i) {
        const rnnt_encoder_layer &l = layers[i];
        const size_t M = (size_t)N * T.P.Lout[i], act = M * pad4(l.cout);
        const bool res = l.role == RNNT_ENC_ROLE_RESIDUAL, gelu = !is_1x1(l);
        T.in_of[i] = cur;
        T.off_o[i] = i != n_layers - 1 && !res ? take(act) : NOT_KEPT;
        T.off_z[i] = gelu ? take(act) : NOT_KEPT;
        T.off_xh[i] = l.norm != RNNT_ENC_NORM_NONE ? take(act) : NOT_KEPT;
        T.off_rstd[i] = l.norm == RNNT_ENC_NORM_INSTANCE ? take((size_t)N * l.cout) : NOT_KEPT;
        if (!res) cur = i;
        dy = act > dy ? act : dy;
        if ((l.role & RNNT_ENC_ROLE_LAST) && act > dres) dres = act;
        const size_t p3 = (size_t)3 * N * l.cout;
        part = p3 > part ? p3 : part;
        T.dx_split[i] = 0;
        if (!reads_input(layers, i)) {
            const long Min = (long)N * T.P.Lin[i];
            if (Min > 65535L * 32) return fail(RNNT_ERR_UNSUPPORTED, "N * L too large");
            T.dx_split[i] = mfma_tap_split(Min, l.cin, l.taps);
            const size_t s = (size_t)T.dx_split[i] * Min * l.cin;
            if (res) x2 = s > x2 ? s : x2; else x1 = s > x1 ? s : x1;
        }
        const long tiles = (long)((l.cin + 127) / 128) * ((l.cout + 127) / 128) * l.taps;
        long R = (ENC_DW_WGS + tiles - 1) / tiles;
        R = R > ENC_DW_RANGES ? ENC_DW_RANGES : R;
        long rows = ((long)M + R - 1) / R;
        rows = (rows + ENC_DW_STEP - 1) / ENC_DW_STEP * ENC_DW_STEP;
        T.dw_rows[i] = (int)rows;
        T.dw_ranges[i] = (int)(((long)M + rows - 1) / rows);
        const size_t s = (size_t)T.dw_ranges[i] * l.taps * l.cout * l.cin;
        dw = s > dw ? s : dw;
    }
    T.saved = off * 4;
    T.dy = align_up(dy * 4) / 4; T.dres = align_up(dres * 4) / 4; T.x1 = align_up(x1 * 4) / 4; T.x2 = align_up(x2 * 4) / 4;
    T.dw = align_up(dw * 4) / 4; T.part = align_up(part * 4) / 4;
    const size_t fwd = (T.P.res + T.P.slab) * 4, bwd = (T.dy + T.dres + T.x1 + T.x2 + T.dw + T.part) * 4;
    T.ws_fwd = fwd; T.ws_bwd = bwd;  // (the forward's depends on `regime`, the backward's does not)
    return RNNT_OK;
}

// what both training run entries check before anything is enqueued
int check_train(const rnnt_encoder_layer *layers, int n_layers, const void *packed, const float *x, const int64_t xs[3],
                const void *const *keep, const float *p, const void *io, const void *saved, size_t saved_bytes, const void *ws,
                size_t ws_bytes, size_t ws_need, const TrainPlan &T)
{
    if (int rc = check_buffers(packed, x, xs, io, ws, saved, true)) return rc;
    if (saved_bytes < T.saved) return fail(RNNT_ERR_WORKSPACE, "saved %zu < required %zu bytes", saved_bytes, T.saved);
    if (ws_bytes < ws_need) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, ws_need);
    for (int i = 0; i < n_layers; ++i) {
        if (int rc = check_params(layers[i], i)) return rc;
        if (p && !(p[i] >= 0.f && p[i] < 1.f)) return fail(RNNT_ERR_INVALID_ARG, "layer %d: dropout p=%g outside [0, 1)", i, (double)p[i]);
        if (keep && keep[i] && is_1x1(layers[i])) return fail(RNNT_ERR_INVALID_ARG, "layer %d: a keep mask on a residual / final layer", i);
    }
    return RNNT_OK;
}

// layer i's input in training: x or a kept output, `lead` zero frames in front
EncIn train_in(const rnnt_encoder_layer *layers, const TrainPlan &T, int i, const float *x, const int64_t xs[3], int L, const float *saved)
{
    const int from = T.in_of[i], C = layers[i].cin;
    EncIn in = from < 0 ? caller_x(x, xs, L, C) : time_major(saved + T.off_o[from], pad4(C), T.P.Lout[from], C);
    in.src.slen = T.lead[i];
    return in;
}

// ---- entries: host side
// what every size query checks first
int check_query(const rnnt_encoder_layer *layers, int n_layers, const size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null output pointer");
    return check_layers(layers, n_layers);
}

size_t packed_total(const rnnt_encoder_layer *layers, int n_layers, bool transposed)  // floats
{
    size_t n = 0;
    for (int i = 0; i < n_layers; ++i) n += packed_floats(layers[i], transposed);
    return n;
}

int check_packed(const void *packed, size_t packed_bytes, size_t need)
{
    if (!packed || ((uintptr_t)packed & 15)) return fail(RNNT_ERR_INVALID_ARG, "null or not 16-byte aligned packed buffer");
    if (packed_bytes < need) return fail(RNNT_ERR_WORKSPACE, "packed buffer %zu < required %zu bytes", packed_bytes, need);
    return RNNT_OK;
}

// one kind of table for the whole list, layer behind layer from wp on
void pack_tables(const rnnt_encoder_layer *layers, int n_layers, float *wp, bool transposed, hipStream_t st)
{
    for (int i = 0; i < n_layers; ++i) {
        const rnnt_encoder_layer &l = layers[i];
        const long n = (long)l.taps * (transposed ? (long)l.cin * pad4(l.cout) : (long)l.cout * pad4(l.cin));
        hipLaunchKernelGGL(k_enc_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float *)l.weight, wp, l.cout, l.cin,
                           l.taps, (int)transposed);
        wp += packed_floats(l, transposed);
    }
}

}  // namespace

extern "C" {

int rnnt_engine_encoder_packed_bytes(const rnnt_encoder_layer *layers, int n_layers, size_t *out)
{
    if (int rc = check_query(layers, n_layers, out)) return rc;
    *out = packed_total(layers, n_layers, false) * 4;
    return RNNT_OK;
}

int rnnt_engine_encoder_pack(const rnnt_encoder_layer *layers, int n_layers, void *packed, size_t packed_bytes, void *stream)
{
    size_t need = 0;
    if (int rc = rnnt_engine_encoder_packed_bytes(layers, n_layers, &need)) return rc;
    if (int rc = check_packed(packed, packed_bytes, need)) return rc;
    for (int i = 0; i < n_layers; ++i)
        if (!layers[i].weight) return fail(RNNT_ERR_INVALID_ARG, "layer %d: null weight", i);
    pack_tables(layers, n_layers, (float *)packed, false, (hipStream_t)stream);
    return status("rnnt_engine_encoder_pack");
}

int rnnt_engine_encoder_workspace_bytes(const rnnt_encoder_layer *layers, int n_layers, int N, int L, int regime,
                                        const int32_t *state_lens, size_t *out)
{
    if (int rc = check_query(layers, n_layers, out)) return rc;
    Plan P;
    if (int rc = make_plan(layers, n_layers, N, L, state_lens, regime, P)) return rc;
    *out = P.total;
    return RNNT_OK;
}

int rnnt_engine_encoder_fwd(const rnnt_encoder_layer *layers, int n_layers, const void *packed, const float *x,
                            const int64_t x_strides[3], int N, int L, int regime, float *out, void *workspace, size_t ws_bytes,
                            void *stream)
{
    return run("rnnt_engine_encoder_fwd", layers, n_layers, packed, x, x_strides, N, L, nullptr, nullptr, nullptr, nullptr, regime, out,
               workspace, ws_bytes, stream);
}

int rnnt_engine_encoder_stream_push(const rnnt_encoder_layer *layers, int n_layers, const void *packed, const float *x,
                                    const int64_t x_strides[3], int N, int L, void *const *state_in, const int32_t *state_in_lens,
                                    void *const *state_out, const int32_t *state_out_lens, int regime, float *out, void *workspace,
                                    size_t ws_bytes, void *stream)
{
    if (!state_in_lens) return fail(RNNT_ERR_INVALID_ARG, "null state argument");
    return run("rnnt_engine_encoder_stream_push", layers, n_layers, packed, x, x_strides, N, L, state_in, state_in_lens, state_out,
               state_out_lens, regime, out, workspace, ws_bytes, stream);
}

int rnnt_engine_encoder_train_packed_bytes(const rnnt_encoder_layer *layers, int n_layers, size_t *out)
{
    if (int rc = check_query(layers, n_layers, out)) return rc;
    *out = (packed_total(layers, n_layers, false) + packed_total(layers, n_layers, true)) * 4;
    return RNNT_OK;
}

int rnnt_engine_encoder_train_pack(const rnnt_encoder_layer *layers, int n_layers, void *packed, size_t packed_bytes, void *stream)
{
    size_t need = 0;
    if (int rc = rnnt_engine_encoder_train_packed_bytes(layers, n_layers, &need)) return rc;
    if (int rc = check_packed(packed, packed_bytes, need)) return rc;
    const size_t fwd = packed_total(layers, n_layers, false);  // the forward's tables come first
    if (int rc = rnnt_engine_encoder_pack(layers, n_layers, packed, fwd * 4, stream)) return rc;
    pack_tables(layers, n_layers, (float *)packed + fwd, true, (hipStream_t)stream);
    return status("rnnt_engine_encoder_train_pack");
}

int rnnt_engine_encoder_train_saved_bytes(const rnnt_encoder_layer *layers, int n_layers, int N, int L, const int32_t *lead,
                                          size_t *out)
{
    if (int rc = check_query(layers, n_layers, out)) return rc;
    TrainPlan T;
    if (int rc = make_train_plan(layers, n_layers, N, L, lead, RNNT_ENC_REGIME_AUTO, T)) return rc;
    *out = T.saved;
    return RNNT_OK;
}

int rnnt_engine_encoder_train_workspace_bytes(const rnnt_encoder_layer *layers, int n_layers, int N, int L, int regime,
                                              const int32_t *lead, size_t *out)
{
    if (int rc = check_query(layers, n_layers, out)) return rc;
    TrainPlan T;
    if (int rc = make_train_plan(layers, n_layers, N, L, lead, regime, T)) return rc;
    *out = T.ws_fwd > T.ws_bwd ? T.ws_fwd : T.ws_bwd;
    return RNNT_OK;
}

int rnnt_engine_encoder_train_fwd(const rnnt_encoder_layer *layers, int n_layers, const void *packed, const float *x,
                                  const int64_t xs[3], int N, int L, const int32_t *lead, const void *const *keep, const float *p,
                                  int regime, float *out, void *saved_v, size_t saved_bytes, void *ws, size_t ws_bytes, void *stream)
{
    if (int rc = check_layers(layers, n_layers)) return rc;
    TrainPlan T;
    if (int rc = make_train_plan(layers, n_layers, N, L, lead, regime, T)) return rc;
    if (int rc = check_train(layers, n_layers, packed, x, xs, keep, p, out, saved_v, saved_bytes, ws, ws_bytes, T.ws_fwd, T)) return rc;
    const Plan &P = T.P;
    hipStream_t st = (hipStream_t)stream;
    float *saved = (float *)saved_v, *res = (float *)ws, *slabs = res + P.res;
    const float *wp = (const float *)packed;
    for (int i = 0; i < n_layers; ++i) {
        const rnnt_encoder_layer &l = layers[i];
        const EncIn in = train_in(layers, T, i, x, xs, L, saved);
        launch_conv(conv_args(in, wp, l.cout, l.taps, l.stride, l.dilation, N, P.Lout[i], slabs, P.tsplit[i]), P.few[i], st);

        const bool to_res = l.role == RNNT_ENC_ROLE_RESIDUAL, to_out = i == n_layers - 1;
        auto at = [&](size_t off) { return off == NOT_KEPT ? nullptr : saved + off; };
        EncNorm nm = norm_args(l, P, i, N, slabs, res, to_out ? out : to_res ? res : at(T.off_o[i]), to_out ? l.cout : pad4(l.cout));
        nm.keep = keep ? (const uint8_t *)keep[i] : nullptr;
        nm.scale = 1.f / (1.f - (p ? p[i] : 0.f));
        nm.z = at(T.off_z[i]); nm.xh = at(T.off_xh[i]); nm.rstd = at(T.off_rstd[i]); nm.lds = pad4(l.cout);
        hipLaunchKernelGGL(k_enc_norm<true>, dim3((unsigned)nm.nb_norm), dim3(ENC_NORM_THREADS), 0, st, nm);
        wp += packed_floats(l, false);
    }
    return status("rnnt_engine_encoder_train_fwd");
}

int rnnt_engine_encoder_train_bwd(const rnnt_encoder_layer *layers, int n_layers, const void *packed, const float *x,
                                  const int64_t xs[3], int N, int L, const int32_t *lead, const void *const *keep, const float *p,
                                  const float *dout, const void *saved_v, size_t saved_bytes, const rnnt_encoder_grads *grads, void *ws,
                                  size_t ws_bytes, void *stream)
{
    if (int rc = check_layers(layers, n_layers)) return rc;
    TrainPlan T;
    if (int rc = make_train_plan(layers, n_layers, N, L, lead, RNNT_ENC_REGIME_AUTO, T)) return rc;
    if (int rc = check_train(layers, n_layers, packed, x, xs, keep, p, dout, saved_v, saved_bytes, ws, ws_bytes, T.ws_bwd, T)) return rc;
    if (!grads) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    for (int i = 0; i < n_layers; ++i)
        if (layers[i].norm == RNNT_ENC_NORM_NONE && (grads[i].gamma || grads[i].beta))
            return fail(RNNT_ERR_INVALID_ARG, "layer %d: a gamma / beta gradient asked of a layer without a norm", i);
    const Plan &P = T.P;
    hipStream_t st = (hipStream_t)stream;
    const float *saved = (const float *)saved_v;
    float *dy = (float *)ws, *dres = dy + T.dy, *x1 = dres + T.dres, *x2 = x1 + T.x1, *dws = x2 + T.x2, *part = dws + T.dw;
    const float *wt[RNNT_ENC_MAX_LAYERS];  // the dX tables lie behind the forward's
    {
        const float *w = (const float *)packed + packed_total(layers, n_layers, false);
        for (int i = 0; i < n_layers; ++i) { wt[i] = w; w += packed_floats(layers[i], true); }
    }
    auto at = [&](size_t off) { return off == NOT_KEPT ? nullptr : saved + off; };
    for (int i = n_layers - 1; i >= 0; --i) {
        const rnnt_encoder_layer &l = layers[i];
        const int Lout = P.Lout[i];
        const long M = (long)N * Lout, ldp = pad4(l.cout);
        const bool is_res = l.role == RNNT_ENC_ROLE_RESIDUAL;
        EncNormB nb;
        nb.b = {nullptr, 0, 0, 0};
        if (i == n_layers - 1) {
            nb.a = {dout, 1, 0, l.cout};
        } else if (is_res) {
            nb.a = {dres, 1, 0, ldp};
        } else {  // the dx of the layer(s) that read this output: the next layer, or a block's first layer and its residual 1x1
            const int j = layers[i + 1].role == RNNT_ENC_ROLE_RESIDUAL ? i + 2 : i + 1;
            nb.a = {x1, T.dx_split[j], M * l.cout, l.cout};
            if (j == i + 2) nb.b = {x2, T.dx_split[i + 1], M * l.cout, l.cout};
        }
        nb.keep = keep ? (const uint8_t *)keep[i] : nullptr;
        nb.scale = 1.f / (1.f - (p ? p[i] : 0.f));
        nb.z = at(T.off_z[i]); nb.act = !is_1x1(l);
        nb.xh = at(T.off_xh[i]); nb.rstd = at(T.off_rstd[i]);
        nb.gamma = (const float *)l.gamma; nb.var = (const float *)l.var; nb.norm = l.norm; nb.eps = l.eps; nb.lds = ldp;
        nb.dy = dy; nb.ldy = ldp;
        nb.dres = (l.role & RNNT_ENC_ROLE_LAST) ? dres : nullptr; nb.ldres = ldp;
        nb.part = part; nb.N = N; nb.Lout = Lout; nb.cout = l.cout;
        hipLaunchKernelGGL(k_enc_bwd_norm, dim3((unsigned)(N * ((l.cout + 15) / 16))), dim3(ENC_NORM_THREADS), 0, st, nb);

        const rnnt_encoder_grads &g = grads[i];
        if (g.weight) {
            EncDW d;
            d.src = train_in(layers, T, i, x, xs, L, saved).src;
            d.dy = dy; d.ldy = ldp; d.cout = l.cout; d.taps = l.taps; d.stride = l.stride; d.dil = l.dilation; d.N = N; d.Lout = Lout;
            d.slabs = dws; d.ranges = T.dw_ranges[i]; d.rows = T.dw_rows[i];
            hipLaunchKernelGGL(k_enc_dw, dim3((unsigned)(l.taps * d.ranges), (l.cin + 127) / 128, (l.cout + 127) / 128), dim3(256), 0, st, d);
        }
        if (g.weight || g.bias || g.gamma || g.beta) {
            EncSumB s;
            const long per = (long)l.taps * l.cout * l.cin;
            s.slabs = dws; s.ranges = T.dw_ranges[i]; s.taps = l.taps; s.cout = l.cout; s.cin = l.cin;
            s.dw = (float *)g.weight; s.nb_w = g.weight ? (int)((per + 255) / 256) : 0;
            s.part = part; s.N = N;
            s.dst[0] = (float *)g.gamma; s.dst[1] = (float *)g.beta; s.dst[2] = (float *)g.bias;
            hipLaunchKernelGGL(k_enc_bwd_sum, dim3((unsigned)(s.nb_w + (3 * l.cout + 255) / 256)), dim3(256), 0, st, s);
        }
        if (T.dx_split[i]) {  // dx = conv of dy, span - lead zero frames in front and zeros behind its last frame, with the reversed taps
            EncIn in = time_major(dy, ldp, Lout, l.cout);
            in.src.slen = (l.taps - 1) * l.dilation - T.lead[i];
            launch_conv(conv_args(in, wt[i], l.cin, l.taps, 1, l.dilation, N, P.Lin[i], is_res ? x2 : x1, T.dx_split[i]), false, st);
        }
    }
    return status("rnnt_engine_encoder_train_bwd");
}

}  // extern "C"
