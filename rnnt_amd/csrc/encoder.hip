// encoder.hip — the Jasper AudioEncoder's inference forward (reference rnnt/jasper.py, rnnt/causalconv.py) on the device:
// whole utterances and streaming pushes.  Every layer is  causal conv -> [norm] -> [+ residual] -> [GELU]  and runs as two
// launches: a convolution kernel that leaves fp32 partial sums in slabs, and k_enc_norm, which adds the slabs up in a
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
    int xlen;          // its frames
    int C;             // channels
};

__device__ __forceinline__ float enc_src(const EncSrc &s, int n, int c, int tau)
{
    if (tau < s.slen) return s.st ? s.st[((long)n * s.C + c) * s.slen + tau] : 0.f;
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
        if (kok) {
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

// ---- everything after the products.  Blocks 0 .. nb_norm-1: block (channel group of 16, batch entry n), thread (channel
// tid & 15, frame lane tid >> 4 of 64): v = bias + the slabs in index order; instance norm: mean, then the biased variance about that
// mean (two passes over the frames of this call, partial sums combined in lane order); batch norm: the running statistics;
// gamma / beta; + residual; GELU; store time-major.  Blocks behind those: the conv's next streaming state, X~ from frame
// Lout * stride on, into a buffer of its own (N, C, slen_out).
struct EncNorm {
    const float *slabs; int nsplit;
    const float *bias, *gamma, *beta, *mean, *var;
    int norm; float eps;
    const float *res; long ldres;  // [N][Lout][ldres] or NULL
    int act;
    float *out; long ldo;          // [N][Lout][ldo]
    int N, Lout, cout, nb_norm;
    EncSrc src; float *state_out; int slen_out, stride;
};

__global__ __launch_bounds__(ENC_NORM_THREADS) void k_enc_norm(EncNorm a)
{
    __shared__ float red[ENC_NORM_THREADS];
    const int tid = threadIdx.x;
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
    const int cl = tid & 15, tl = tid >> 4;
    const int cgroups = (a.cout + 15) / 16;
    const int n = (int)blockIdx.x / cgroups, c = ((int)blockIdx.x - n * cgroups) * 16 + cl;
    const bool ok = c < a.cout;
    const long M = (long)a.N * a.Lout, row0 = (long)n * a.Lout;
    const float b = ok && a.bias ? a.bias[c] : 0.f;
    auto pre = [&](int t) {
        const float *s = a.slabs + (row0 + t) * a.cout + c;
        const long step = M * a.cout;
        float v = s[0];
        int k = 1;
        for (; k + 8 <= a.nsplit; k += 8) {  // eight slabs requested together, added in index order
            float p[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) p[e] = s[(long)(k + e) * step];
#pragma unroll
            for (int e = 0; e < 8; ++e) v += p[e];
        }
        for (; k < a.nsplit; ++k) v += s[(long)k * step];
        return v + b;
    };
    float mu = 0.f, rstd = 1.f;
    const bool inst = a.norm == RNNT_ENC_NORM_INSTANCE;
    if (inst) {
        float s = 0.f;
        if (ok)
            for (int t = tl; t < a.Lout; t += ENC_NORM_LANES) {
                const float v = pre(t);
                a.out[(row0 + t) * a.ldo + c] = v;  // parked; this thread reads it back below
                s += v;
            }
        red[tid] = s;
        __syncthreads();
        s = 0.f;
        for (int k = 0; k < ENC_NORM_LANES; ++k) s += red[16 * k + cl];
        mu = s / (float)a.Lout;
        __syncthreads();
        float q = 0.f;
        if (ok)
            for (int t = tl; t < a.Lout; t += ENC_NORM_LANES) {
                const float d = a.out[(row0 + t) * a.ldo + c] - mu;
                q += d * d;
            }
        red[tid] = q;
        __syncthreads();
        q = 0.f;
        for (int k = 0; k < ENC_NORM_LANES; ++k) q += red[16 * k + cl];
        rstd = 1.f / sqrtf(q / (float)a.Lout + a.eps);
    } else if (a.norm == RNNT_ENC_NORM_BATCH && ok) {
        mu = a.mean[c];
        rstd = 1.f / sqrtf(a.var[c] + a.eps);
    }
    if (!ok) return;
    const float g = a.norm != RNNT_ENC_NORM_NONE && a.gamma ? a.gamma[c] : 1.f;
    const float be = a.norm != RNNT_ENC_NORM_NONE && a.beta ? a.beta[c] : 0.f;
    for (int t = tl; t < a.Lout; t += ENC_NORM_LANES) {
        float v = inst ? a.out[(row0 + t) * a.ldo + c] : pre(t);
        if (a.norm != RNNT_ENC_NORM_NONE) v = (v - mu) * rstd * g + be;
        if (a.res) v += a.res[(row0 + t) * a.ldres + c];
        if (a.act) v = gelu_exact(v);
        a.out[(row0 + t) * a.ldo + c] = v;
    }
}

__global__ __launch_bounds__(256) void k_enc_pack_w(const float *__restrict__ w, float *__restrict__ wp, int out_c, int in_c,
                                                    int in_p, int taps)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // walks the packed layout [tap][out][in_p]
    if (idx >= (long)taps * out_c * in_p) return;
    const int ci = (int)(idx % in_p);
    const long to = idx / in_p;
    const int co = (int)(to % out_c), t = (int)(to / out_c);
    wp[idx] = ci < in_c ? w[((long)co * in_c + ci) * taps + t] : 0.f;
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

size_t packed_floats(const rnnt_encoder_layer &l) { return align_up((size_t)l.taps * l.cout * pad4(l.cin) * 4) / 4; }

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
            const long wgs = ((l.cout + 127) / 128) * ((M + 31) / 32);
            long ts = (ENC_MFMA_WGS + wgs - 1) / wgs;
            ts = ts > l.taps ? l.taps : ts;
            ts = ts > ENC_MFMA_SPLITS ? ENC_MFMA_SPLITS : ts;
            P.tsplit[i] = P.nsplit[i] = (int)ts;
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

int run(const char *what, const rnnt_encoder_layer *layers, int n_layers, const void *packed, const float *x, const int64_t xs[3],
        int N, int L, void *const *state_in, const int32_t *state_in_lens, void *const *state_out, const int32_t *state_out_lens,
        int regime, float *out, void *ws, size_t ws_bytes, void *stream)
{
    if (int rc = check_layers(layers, n_layers)) return rc;
    if (!packed || !x || !xs || !out || !ws) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    if (((uintptr_t)packed & 15) || ((uintptr_t)ws & 15) || ((uintptr_t)x & 3) || ((uintptr_t)out & 3))
        return fail(RNNT_ERR_INVALID_ARG, "packed weights and workspace must be 16-byte aligned, x and out 4-byte");
    const bool streaming = state_in_lens != nullptr;
    if (streaming && (!state_in || !state_out || !state_out_lens)) return fail(RNNT_ERR_INVALID_ARG, "null state argument");
    Plan P;
    if (int rc = make_plan(layers, n_layers, N, L, state_in_lens, regime, P)) return rc;
    if (ws_bytes < P.total) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, P.total);
    for (int i = 0; i < n_layers; ++i) {
        const rnnt_encoder_layer &l = layers[i];
        if (!l.bias) return fail(RNNT_ERR_INVALID_ARG, "layer %d: null bias", i);
        if (l.norm == RNNT_ENC_NORM_BATCH && (!l.mean || !l.var)) return fail(RNNT_ERR_INVALID_ARG, "layer %d: batch norm without running statistics", i);
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

    struct Cur { const float *p; long sn, sc, stt; int len, C; bool vec; };
    Cur cur = {x, (long)xs[0], (long)xs[1], (long)xs[2], L, layers[0].cin,
               xs[1] == 1 && xs[0] % 4 == 0 && xs[2] % 4 == 0 && ((uintptr_t)x & 15) == 0};
    int flip = 0;
    for (int i = 0; i < n_layers; ++i) {
        const rnnt_encoder_layer &l = layers[i];
        const int Lout = P.Lout[i], cinp = pad4(l.cin);
        EncSrc src;
        src.st = streaming && P.slen[i] > 0 ? (const float *)state_in[i] : nullptr;
        src.slen = P.slen[i];
        src.x = cur.p; src.xn = cur.sn; src.xc = cur.sc; src.xt = cur.stt; src.xlen = cur.len; src.C = l.cin;
        EncConv c;
        c.src = src; c.wp = wp; c.cinp = cinp; c.cout = l.cout; c.taps = l.taps; c.stride = l.stride; c.dil = l.dilation;
        c.N = N; c.Lout = Lout; c.slabs = slabs; c.tsplit = P.tsplit[i]; c.xvec = cur.vec;
        if (P.few[i])
            hipLaunchKernelGGL(k_enc_conv_few, dim3((l.cout + 63) / 64, (cinp + 63) / 64, P.tsplit[i]), dim3(256), 0, st, c);
        else
            hipLaunchKernelGGL(k_enc_conv_mfma, dim3((l.cout + 127) / 128, (N * Lout + 31) / 32, P.tsplit[i]), dim3(256), 0, st, c);

        const bool to_res = l.role == RNNT_ENC_ROLE_RESIDUAL, fin = l.role == RNNT_ENC_ROLE_FINAL;
        const bool to_out = i == n_layers - 1;  // the list's last layer, FINAL or not, leaves `out` [N][L_out][cout]
        float *dst = to_out ? out : to_res ? res : buf[flip];
        const long ldo = to_out ? l.cout : pad4(l.cout);
        EncNorm nm;
        nm.slabs = slabs; nm.nsplit = P.nsplit[i];
        nm.bias = (const float *)l.bias; nm.gamma = (const float *)l.gamma; nm.beta = (const float *)l.beta;
        nm.mean = (const float *)l.mean; nm.var = (const float *)l.var; nm.norm = l.norm; nm.eps = l.eps;
        nm.res = (l.role & RNNT_ENC_ROLE_LAST) ? res : nullptr; nm.ldres = pad4(l.cout);
        nm.act = !(to_res || fin);
        nm.out = dst; nm.ldo = ldo; nm.N = N; nm.Lout = Lout; nm.cout = l.cout;
        nm.nb_norm = N * ((l.cout + 15) / 16);
        nm.src = src; nm.stride = l.stride;
        const bool wr_state = streaming && !is_1x1(l) && P.slen_out[i] > 0;
        nm.state_out = wr_state ? (float *)state_out[i] : nullptr;
        nm.slen_out = wr_state ? P.slen_out[i] : 0;
        const long nb_state = wr_state ? ((long)N * l.cin * P.slen_out[i] + ENC_NORM_THREADS - 1) / ENC_NORM_THREADS : 0;
        hipLaunchKernelGGL(k_enc_norm, dim3((unsigned)(nm.nb_norm + nb_state)), dim3(ENC_NORM_THREADS), 0, st, nm);

        wp += packed_floats(l);
        if (to_res) continue;
        cur = {dst, (long)Lout * ldo, 1, ldo, Lout, l.cout, true};
        flip ^= 1;
    }
    return status(what);
}

}  // namespace

extern "C" {

int rnnt_engine_encoder_packed_bytes(const rnnt_encoder_layer *layers, int n_layers, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null output pointer");
    if (int rc = check_layers(layers, n_layers)) return rc;
    size_t n = 0;
    for (int i = 0; i < n_layers; ++i) n += packed_floats(layers[i]);
    *out = n * 4;
    return RNNT_OK;
}

int rnnt_engine_encoder_pack(const rnnt_encoder_layer *layers, int n_layers, void *packed, size_t packed_bytes, void *stream)
{
    size_t need = 0;
    if (int rc = rnnt_engine_encoder_packed_bytes(layers, n_layers, &need)) return rc;
    if (!packed || ((uintptr_t)packed & 15)) return fail(RNNT_ERR_INVALID_ARG, "null or not 16-byte aligned packed buffer");
    if (packed_bytes < need) return fail(RNNT_ERR_WORKSPACE, "packed buffer %zu < required %zu bytes", packed_bytes, need);
    for (int i = 0; i < n_layers; ++i)
        if (!layers[i].weight) return fail(RNNT_ERR_INVALID_ARG, "layer %d: null weight", i);
    float *wp = (float *)packed;
    for (int i = 0; i < n_layers; ++i) {
        const rnnt_encoder_layer &l = layers[i];
        const long n = (long)l.taps * l.cout * pad4(l.cin);
        hipLaunchKernelGGL(k_enc_pack_w, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float *)l.weight, wp, l.cout, l.cin, pad4(l.cin), l.taps);
        wp += packed_floats(l);
    }
    return status("rnnt_engine_encoder_pack");
}

int rnnt_engine_encoder_workspace_bytes(const rnnt_encoder_layer *layers, int n_layers, int N, int L, int regime,
                                        const int32_t *state_lens, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null output pointer");
    if (int rc = check_layers(layers, n_layers)) return rc;
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

}  // extern "C"
