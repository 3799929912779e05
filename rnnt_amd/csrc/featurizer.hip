// featurizer.hip — audio samples to the encoder's input features on the device (reference rnnt/featurizer.py): the power
// spectrum of overlapping frames, a log stage, per-bin normalisation; optionally a filterbank in front of the log stage.
// Whole (ragged) batches and streaming pushes.
//
// The spectrum is a GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products): the windowed DFT basis (bins x n_fft, cosine and
// -sine) against the frames (n_fft x frames).  Bins are the MFMA's rows, frames its columns, so a lane's accumulator
// registers hold re and im of the same (bin, frame) — re^2 + im^2 needs no exchange — and lanes run along the frames, the
// contiguous axis of an (N, F, L) output.
//
//   k_feat_basis   once per featurizer: [bin tile of 32][chunk q of 4 samples][lane][4] = for bin (lane & 31) and the
//                  samples n0 = 4q + 2(lane >> 5), n0 + 1:  w[n0] cos, -w[n0] sin, w[n0+1] cos, -w[n0+1] sin  of the
//                  angle 2 pi ((n k) mod n_fft) / n_fft, taken in double; zeros beyond n_fft and beyond the last bin.
//                  A wave reads one chunk of its bin tile as ONE 16-byte load per lane, 1 KB contiguous.
//   k_feat_power   grid (bin tiles, frame tiles of 32 + state blocks, batch entries), 256 threads.  The workgroup stages the
//                  31 hop + n_fft samples its frames cover in LDS once, read through FeatSrc: streaming state followed by
//                  the chunk (nothing is concatenated), fp32 or int16 / 32768, reflected at both ends when centred.  Frame
//                  i's row starts at sample i hop; for an even hop one pad word per hop samples makes the row stride odd, so
//                  the 32 rows of an operand read fall on 32 different banks.  The four waves take the chunks q = wave,
//                  wave + 4, ... and add their tiles up through LDS in wave order; wave 0 then does power -> log stage ->
//                  (v - mean) invstd -> store through the caller's strides (or power -> workspace when a filterbank follows).
//                  The blocks behind the frame tiles write the next streaming state into a buffer of its own.
//   k_feat_fbank   power (frames x bins) . filterbank (bins x filters), one thread per (frame, filter), bins in index order,
//                  then the same log stage, normalisation and store.
// One (bin, frame) is summed in ONE order — samples 4q, 4q+2, 4q+1, 4q+3 within a chunk, a wave's chunks ascending, the
// waves in order — whatever the frame's place in a tile, a batch or a chunk: the same samples give the same bits.  No atomics.
#include "../../include/rnnt_engine.h"

#include <cstdint>

#include "kernels.hpp"

namespace {

constexpr int FEAT_SLICE = 64;          // batch entries per launch (their lengths travel in the kernel arguments)
constexpr int FEAT_LDS_MAX = 64 * 1024; // the staged span (with its pad words) must fit

struct FeatSrc {
    const float *st;  // state (N, slen) contiguous fp32, or NULL (slen == 0)
    int slen;         // samples of state in front of the chunk
    const void *x;    // chunk: fp32 or int16 samples
    long xn;          // its batch stride in samples
    int fmt;          // RNNT_FEAT_PCM_*
    int pad;          // centred: n_fft / 2 samples reflected in front and behind; else 0
};

// sample p of utterance n, in the coordinates the frames are cut from (padded when centred); `len` = state + chunk samples
__device__ __forceinline__ float feat_src(const FeatSrc &s, int n, long p, long len)
{
    if (p >= len + 2 * s.pad) return 0.f;
    long q = p - s.pad;
    if (q < 0) q = -q;
    if (q >= len) q = 2 * (len - 1) - q;
    if (q < s.slen) return s.st[(long)n * s.slen + q];
    q -= s.slen;
    if (s.fmt == RNNT_FEAT_PCM_S16) return (float)((const int16_t *)s.x)[n * s.xn + q] * (1.f / 32768.f);
    return ((const float *)s.x)[n * s.xn + q];
}

struct FeatTail {  // what follows the power (or the filterbank's output)
    int log_kind;
    float gain;
    const float *mean, *invstd;  // per output bin
    float *out;
    long on, of, ol;             // strides (floats): batch entry, bin, frame
};

__device__ __forceinline__ float feat_tail(const FeatTail &t, float p, int k)
{
    float v;
    if (t.log_kind == RNNT_FEAT_LOG_PIECEWISE)
        v = p > 0.01f ? logf(p) : 50.f * p + (-4.605170185988091f - 0.5f);
    else if (t.log_kind == RNNT_FEAT_LOG_GAIN)
        v = logf((p + 1e-6f) * t.gain);
    else
        v = logf(p + 1e-6f);
    return (v - t.mean[k]) * t.invstd[k];
}

__device__ __forceinline__ int feat_count(long len, int n_fft, int hop, int center)
{
    if (center) return (int)((len + 2 * (n_fft / 2) - n_fft) / hop) + 1;
    return len >= n_fft ? (int)((len - n_fft) / hop) + 1 : 0;
}

struct FeatPow {
    FeatSrc src;
    int lens[FEAT_SLICE];  // samples (state + chunk) per utterance of this slice
    int n_base;            // first batch entry of the slice
    const f32x4 *basis;
    int n_fft, hop, padw, Q, n_freq, center;
    int L, nft;            // frames stored per utterance, frame tiles
    FeatTail tail;
    float *power;          // [N][n_freq][L] instead of the tail, when a filterbank follows; else NULL
    float *state_out;      // (N, slen_out) or NULL
    int slen_out;
    long state_from;       // first sample of the next state
};

__global__ __launch_bounds__(256) void k_feat_power(FeatPow a)
{
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, half = lane >> 5;
    const int n = a.n_base + (int)blockIdx.z;
    const long len = a.lens[blockIdx.z];
    if ((int)blockIdx.y >= a.nft) {  // the next streaming state
        const long idx = ((long)((int)blockIdx.y - a.nft) * gridDim.x + blockIdx.x) * 256 + tid;
        if (idx < a.slen_out) a.state_out[(long)n * a.slen_out + idx] = feat_src(a.src, n, a.state_from + idx, len);
        return;
    }
    const int cnt = feat_count(len, a.n_fft, a.hop, a.center);
    const int f0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
    if (f0 >= cnt) {  // a tile behind the utterance's last frame: zeros (the filterbank kernel writes its own)
        if (!a.power && wave == 0) {
            const int f = f0 + i;
            for (int r = half; r < 32; r += 2)
                if (k0 + r < a.n_freq && f < a.L) a.tail.out[n * a.tail.on + (k0 + r) * a.tail.of + f * a.tail.ol] = 0.f;
        }
        return;
    }
    const int span = 31 * a.hop + a.n_fft;
    const long p0 = (long)f0 * a.hop;
    for (int c = tid; c < span; c += 256) lds[c + c / a.hop * a.padw] = feat_src(a.src, n, p0 + c, len);
    __syncthreads();

    f32x16 re, im;
#pragma unroll
    for (int r = 0; r < 16; ++r) re[r] = im[r] = 0.f;
    const int row = i * (a.hop + a.padw);
    const f32x4 *b = a.basis + (long)blockIdx.x * a.Q * 64 + lane;
    if (wave < a.Q) {
        f32x4 w = b[(long)wave * 64];
        for (int q = wave; q < a.Q; q += 4) {
            f32x4 wn = w;
            if (q + 4 < a.Q) wn = b[(long)(q + 4) * 64];
            const int n0 = 4 * q + 2 * half, n1 = n0 + 1;
            const float x0 = n0 < a.n_fft ? lds[row + n0 + n0 / a.hop * a.padw] : 0.f;
            const float x1 = n1 < a.n_fft ? lds[row + n1 + n1 / a.hop * a.padw] : 0.f;
            re = __builtin_amdgcn_mfma_f32_32x32x2f32(w[0], x0, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_32x32x2f32(w[1], x0, im, 0, 0, 0);
            re = __builtin_amdgcn_mfma_f32_32x32x2f32(w[2], x1, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_32x32x2f32(w[3], x1, im, 0, 0, 0);
            w = wn;
        }
    }
    __syncthreads();  // the staged span is done with: its LDS carries the waves' partial tiles now
#pragma unroll 1
    for (int w = 1; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                lds[r * 64 + lane] = re[r];
                lds[(16 + r) * 64 + lane] = im[r];
            }
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                re[r] += lds[r * 64 + lane];
                im[r] += lds[(16 + r) * 64 + lane];
            }
        }
        __syncthreads();
    }
    if (wave != 0) return;
    const int f = f0 + i;
    if (f >= a.L) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int k = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (k >= a.n_freq) continue;
        const float p = re[r] * re[r] + im[r] * im[r];
        if (a.power) {
            if (f < cnt) a.power[((long)n * a.n_freq + k) * a.L + f] = p;
        } else {
            a.tail.out[n * a.tail.on + k * a.tail.of + f * a.tail.ol] = f < cnt ? feat_tail(a.tail, p, k) : 0.f;
        }
    }
}

struct FeatFbank {
    int lens[FEAT_SLICE];
    int n_base;
    const float *power;  // [N][n_freq][L]
    const float *fb;     // [n_freq][n_filters]
    int n_fft, hop, center, n_freq, n_filters, L;
    FeatTail tail;
};

// grid (ceil(L / 64), ceil(n_filters / 4), batch entries), 256 threads: frame lane tid & 63, filter tid >> 6
__global__ __launch_bounds__(256) void k_feat_fbank(FeatFbank a)
{
    const int f = blockIdx.x * 64 + (threadIdx.x & 63), m = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int n = a.n_base + (int)blockIdx.z;
    if (f >= a.L || m >= a.n_filters) return;
    float v = 0.f;
    if (f < feat_count(a.lens[blockIdx.z], a.n_fft, a.hop, a.center)) {
        const float *p = a.power + (long)n * a.n_freq * a.L + f;
        float s = 0.f;
        for (int k = 0; k < a.n_freq; ++k) s = fmaf(p[(long)k * a.L], a.fb[(long)k * a.n_filters + m], s);
        v = feat_tail(a.tail, s, m);
    }
    a.tail.out[n * a.tail.on + m * a.tail.of + f * a.tail.ol] = v;
}

__global__ __launch_bounds__(256) void k_feat_basis(const float *__restrict__ win, f32x4 *__restrict__ basis, int n_fft, int win_length,
                                                    int Q, int n_freq, int nbt)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // walks [bin tile][chunk][lane]
    if (idx >= (long)nbt * Q * 64) return;
    const int lane = (int)(idx & 63);
    const int q = (int)((idx >> 6) % Q), bt = (int)((idx >> 6) / Q);
    const int k = bt * 32 + (lane & 31), n0 = 4 * q + 2 * (lane >> 5);
    const int left = (n_fft - win_length) / 2;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int e = 0; e < 2; ++e) {
        const int n = n0 + e;
        if (k >= n_freq || n >= n_fft || n < left || n >= left + win_length) continue;
        const double w = (double)win[n - left];
        const double ang = 6.283185307179586476925286766559 * (double)(((long)n * k) % n_fft) / (double)n_fft;
        v[2 * e] = (float)(w * cos(ang));
        v[2 * e + 1] = (float)(-w * sin(ang));
    }
    basis[idx] = v;
}

// ---------------------------------------------------------------------------------------------------------------- host side
#define fail engine_fail

struct Geo { int n_freq, nbt, Q, padw, F; size_t lds; };

int check_desc(const rnnt_featurizer_desc *d, Geo &g)
{
    if (!d) return fail(RNNT_ERR_INVALID_ARG, "null featurizer description");
    if (d->hop_length < 1) return fail(RNNT_ERR_INVALID_ARG, "hop_length=%d must be >= 1", d->hop_length);
    if (d->n_fft < 2) return fail(RNNT_ERR_INVALID_ARG, "n_fft=%d must be >= 2", d->n_fft);
    if (d->win_length < 1 || d->win_length > d->n_fft)
        return fail(RNNT_ERR_INVALID_ARG, "win_length=%d outside 1 .. n_fft=%d", d->win_length, d->n_fft);
    if ((d->n_fft - d->win_length) & 1)
        return fail(RNNT_ERR_INVALID_ARG, "n_fft - win_length = %d is odd: the window cannot be centred", d->n_fft - d->win_length);
    if (d->center != 0 && d->center != 1) return fail(RNNT_ERR_INVALID_ARG, "center=%d is not 0 or 1", d->center);
    if (d->log_kind != RNNT_FEAT_LOG_PLAIN && d->log_kind != RNNT_FEAT_LOG_PIECEWISE && d->log_kind != RNNT_FEAT_LOG_GAIN)
        return fail(RNNT_ERR_INVALID_ARG, "log kind %d", d->log_kind);
    if (d->log_kind == RNNT_FEAT_LOG_GAIN && !(d->gain > 0.f)) return fail(RNNT_ERR_INVALID_ARG, "gain must be > 0");
    if (d->n_filters < 0) return fail(RNNT_ERR_INVALID_ARG, "n_filters=%d is negative", d->n_filters);
    if (d->n_fft > (1 << 16) || d->hop_length > (1 << 16) || d->n_filters > (1 << 16))
        return fail(RNNT_ERR_UNSUPPORTED, "n_fft, hop_length and n_filters are at most 65536");
    g.n_freq = d->n_fft / 2 + 1;
    g.nbt = (g.n_freq + 31) / 32;
    g.Q = (d->n_fft + 3) / 4;
    g.padw = d->hop_length % 2 == 0 ? 1 : 0;
    g.F = d->n_filters ? d->n_filters : g.n_freq;
    const size_t span = 31 * (size_t)d->hop_length + d->n_fft;
    const size_t words = span + span / d->hop_length * g.padw + 1;
    g.lds = (words > 2048 ? words : 2048) * 4;  // at least the 8 KB of one wave's partial tiles
    if (g.lds > (size_t)FEAT_LDS_MAX)
        return fail(RNNT_ERR_UNSUPPORTED, "31 hop_length + n_fft = %zu samples do not fit the %d KB stage", span, FEAT_LDS_MAX / 1024);
    return RNNT_OK;
}

inline long frames_of(const rnnt_featurizer_desc *d, long len)
{
    if (d->center) return (len + 2 * (d->n_fft / 2) - d->n_fft) / d->hop_length + 1;
    return len >= d->n_fft ? (len - d->n_fft) / d->hop_length + 1 : 0;
}

size_t ws_bytes_of(const rnnt_featurizer_desc *d, const Geo &g, int N, long L)
{
    return d->n_filters ? (((size_t)N * g.n_freq * (size_t)L * 4 + 255) & ~(size_t)255) : 0;
}

int status(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RNNT_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return RNNT_OK;
}

// one call: N utterances of state (slen samples, may be 0) + chunk (T samples, or lens[n] of them)
int run(const char *what, const rnnt_featurizer_desc *d, const void *basis, const void *fbank, const float *state_in, int slen,
        const void *wave, int64_t wave_stride, int N, int T, const int32_t *lens, int pcm, const float *mean, const float *invstd,
        float *out, const int64_t os[3], int L, float *state_out, int slen_out, long state_from, void *ws, size_t ws_bytes,
        void *stream)
{
    Geo g;
    if (int rc = check_desc(d, g)) return rc;
    if (N < 1 || T < 0 || L < 0) return fail(RNNT_ERR_INVALID_ARG, "N=%d < 1, or negative T=%d or L=%d", N, T, L);
    if (pcm != RNNT_FEAT_PCM_F32 && pcm != RNNT_FEAT_PCM_S16) return fail(RNNT_ERR_INVALID_ARG, "sample format %d", pcm);
    if (!basis || !mean || !invstd || !os || (T > 0 && !wave) || (L > 0 && !out) || (d->n_filters && !fbank))
        return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    if (((uintptr_t)basis & 15) || ((uintptr_t)wave & (pcm == RNNT_FEAT_PCM_S16 ? 1 : 3)) || ((uintptr_t)out & 3) || ((uintptr_t)ws & 3))
        return fail(RNNT_ERR_INVALID_ARG, "the basis must be 16-byte aligned, samples, out and workspace aligned to their element");
    if ((long)L * d->hop_length + d->n_fft > 0x7fffffffL || (long)N * L > 0x7fffffffL / 4 || (L + 31) / 32 > 60000)
        return fail(RNNT_ERR_UNSUPPORTED, "N * L or L * hop_length too large");
    const long pad = d->center ? d->n_fft / 2 : 0;
    long most = 0;
    for (int n = 0; n < N; ++n) {
        const long len = slen + (long)(lens ? lens[n] : T);
        if (lens && (lens[n] < 0 || lens[n] > T)) return fail(RNNT_ERR_INVALID_ARG, "utterance %d: length %d outside 0 .. T=%d", n, lens[n], T);
        if (d->center && len <= pad)
            return fail(RNNT_ERR_INVALID_ARG, "utterance %d: %ld samples, the reflect pad of %ld must be shorter than the utterance", n, len, pad);
        const long c = frames_of(d, len);
        most = c > most ? c : most;
    }
    if (most > L) return fail(RNNT_ERR_INVALID_ARG, "out holds L=%d frames, the longest utterance gives %ld", L, most);
    const size_t need = ws_bytes_of(d, g, N, L);
    if (need && (!ws || ws_bytes < need)) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, need);

    hipStream_t st = (hipStream_t)stream;
    const int nft = (L + 31) / 32;
    const int nb_state = slen_out > 0 ? (slen_out + 256 * g.nbt - 1) / (256 * g.nbt) : 0;
    FeatTail tail = {d->log_kind, d->gain, mean, invstd, out, (long)os[0], (long)os[1], (long)os[2]};
    for (int n0 = 0; n0 < N; n0 += FEAT_SLICE) {
        const int ns = N - n0 < FEAT_SLICE ? N - n0 : FEAT_SLICE;
        FeatPow a;
        a.src = {state_in, slen, wave, (long)wave_stride, pcm, (int)pad};
        for (int j = 0; j < ns; ++j) a.lens[j] = slen + (lens ? lens[n0 + j] : T);
        a.n_base = n0;
        a.basis = (const f32x4 *)basis;
        a.n_fft = d->n_fft; a.hop = d->hop_length; a.padw = g.padw; a.Q = g.Q; a.n_freq = g.n_freq; a.center = d->center;
        a.L = L; a.nft = nft;
        a.tail = tail;
        a.power = d->n_filters ? (float *)ws : nullptr;
        a.state_out = state_out; a.slen_out = slen_out; a.state_from = state_from;
        if (nft + nb_state > 0)
            hipLaunchKernelGGL(k_feat_power, dim3(g.nbt, nft + nb_state, ns), dim3(256), g.lds, st, a);
        if (d->n_filters && L > 0) {
            FeatFbank b;
            for (int j = 0; j < ns; ++j) b.lens[j] = a.lens[j];
            b.n_base = n0;
            b.power = (const float *)ws; b.fb = (const float *)fbank;
            b.n_fft = d->n_fft; b.hop = d->hop_length; b.center = d->center; b.n_freq = g.n_freq; b.n_filters = d->n_filters; b.L = L;
            b.tail = tail;
            hipLaunchKernelGGL(k_feat_fbank, dim3((L + 63) / 64, (d->n_filters + 3) / 4, ns), dim3(256), 0, st, b);
        }
    }
    return status(what);
}

}  // namespace

extern "C" {

int rnnt_engine_featurizer_basis_bytes(const rnnt_featurizer_desc *desc, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null output pointer");
    Geo g;
    if (int rc = check_desc(desc, g)) return rc;
    *out = (size_t)g.nbt * g.Q * 64 * 16;
    return RNNT_OK;
}

int rnnt_engine_featurizer_pack(const rnnt_featurizer_desc *desc, const float *window, void *basis, size_t basis_bytes, void *stream)
{
    size_t need = 0;
    if (int rc = rnnt_engine_featurizer_basis_bytes(desc, &need)) return rc;
    if (!window || !basis || ((uintptr_t)basis & 15) || ((uintptr_t)window & 3))
        return fail(RNNT_ERR_INVALID_ARG, "null window, or null or not 16-byte aligned basis buffer");
    if (basis_bytes < need) return fail(RNNT_ERR_WORKSPACE, "basis buffer %zu < required %zu bytes", basis_bytes, need);
    Geo g;
    check_desc(desc, g);
    const long n = (long)g.nbt * g.Q * 64;
    hipLaunchKernelGGL(k_feat_basis, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, window, (f32x4 *)basis,
                       desc->n_fft, desc->win_length, g.Q, g.n_freq, g.nbt);
    return status("rnnt_engine_featurizer_pack");
}

int rnnt_engine_featurizer_workspace_bytes(const rnnt_featurizer_desc *desc, int N, int L, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null output pointer");
    Geo g;
    if (int rc = check_desc(desc, g)) return rc;
    if (N < 1 || L < 0) return fail(RNNT_ERR_INVALID_ARG, "N=%d < 1 or negative L=%d", N, L);
    *out = ws_bytes_of(desc, g, N, L);
    return RNNT_OK;
}

int rnnt_engine_featurizer_fwd(const rnnt_featurizer_desc *desc, const void *basis, const void *fbank, const void *wave,
                               int64_t wave_stride, int N, int T, const int32_t *lens, int pcm, const float *mean,
                               const float *invstd, float *out, const int64_t out_strides[3], int L, void *workspace,
                               size_t ws_bytes, void *stream)
{
    return run("rnnt_engine_featurizer_fwd", desc, basis, fbank, nullptr, 0, wave, wave_stride, N, T, lens, pcm, mean, invstd, out,
               out_strides, L, nullptr, 0, 0, workspace, ws_bytes, stream);
}

int rnnt_engine_featurizer_stream_push(const rnnt_featurizer_desc *desc, const void *basis, const void *fbank,
                                       const float *state_in, int state_in_len, const void *chunk, int64_t chunk_stride, int N, int T,
                                       int pcm, const float *mean, const float *invstd, float *out, const int64_t out_strides[3],
                                       int L, float *state_out, int state_out_len, void *workspace, size_t ws_bytes, void *stream)
{
    Geo g;
    if (int rc = check_desc(desc, g)) return rc;
    if (desc->center) return fail(RNNT_ERR_INVALID_ARG, "a centred featurizer cannot stream (the reflected end is not known yet)");
    if (desc->hop_length > desc->n_fft)
        return fail(RNNT_ERR_UNSUPPORTED, "streaming with hop_length=%d beyond n_fft=%d (samples between frames would be skipped, not carried)",
                    desc->hop_length, desc->n_fft);
    if (state_in_len < 0 || state_in_len > (1 << 24) || T < 0)
        return fail(RNNT_ERR_INVALID_ARG, "state length %d outside 0 .. 2^24, or negative T=%d", state_in_len, T);
    const long total = (long)state_in_len + T, frames = frames_of(desc, total), left = total - frames * desc->hop_length;
    if (L != frames) return fail(RNNT_ERR_INVALID_ARG, "L=%d, this push completes %ld frames", L, frames);
    if (state_out_len != left) return fail(RNNT_ERR_INVALID_ARG, "state_out length %d, this push leaves %ld samples", state_out_len, left);
    if ((state_in_len > 0 && !state_in) || (left > 0 && !state_out)) return fail(RNNT_ERR_INVALID_ARG, "null state pointer");
    if (left > 0 && state_out == state_in) return fail(RNNT_ERR_INVALID_ARG, "the state is never updated in place");
    if (((uintptr_t)state_in & 3) || ((uintptr_t)state_out & 3)) return fail(RNNT_ERR_INVALID_ARG, "the states must be 4-byte aligned");
    return run("rnnt_engine_featurizer_stream_push", desc, basis, fbank, state_in, state_in_len, chunk, chunk_stride, N, T, nullptr, pcm,
               mean, invstd, out, out_strides, L, state_out, (int)left, frames * desc->hop_length, workspace, ws_bytes, stream);
}

}  // extern "C"
