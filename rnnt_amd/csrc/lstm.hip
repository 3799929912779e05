// lstm.hip — LSTMPredictor forward / backward / stateful step for gfx950 behind the C ABI.
//
// Reference rnnt/predictor.py:11-186:
//   x  = LayerNorm_E(embedding(ids))                                        [B,U1,E]
//   per layer l, per step t:  gates = g_norm(x2g(x_t) + p2g(h_{t-1}))       [B,4Hd], order input / forget / cell / output
//                             c_t = c_norm(sigmoid(f) c_{t-1} + sigmoid(i) tanh(g));  h_t = sigmoid(o) tanh(c_t)
//   x  = dropout(h)  (after every layer);   y = LayerNorm_O(linear(x))       [B,U1,O]
// Rows are (b,u) with features contiguous, as in predictor.hip.  x2g of a whole layer is ONE batched NT GEMM; the
// recurrence is two launches per step: the recurrent product h_{t-1} p2g^T (k_rec_gemm, rows U1*Hd apart) and one row
// kernel (k_lstm_step_fwd: a workgroup per batch row).  The backward walks the steps in reverse with a row kernel
// (k_lstm_step_bwd) and the product dgates_t p2g (k_rec_gemm again); the weight gradients, dx and the affine gradients are
// batched GEMMs and fixed-order column sums over all rows after the loop.
// The recurrent products have M = B rows (one 32-row tile at the reference's batch) and sit on every step's critical path.
// smallgemm's kernels give such a product 16 (NT) or 4 (NN) workgroups at Hd = 512 — 256 resp. 1024 dependent MFMAs per wave,
// 7 and 27 us of matrix pipe alone —, so k_rec_gemm cuts it into 32 x 32 tiles AND contraction ranges, one workgroup each
// (256 of them at Hd = 512, <= 32 MFMAs per wave); the partial tiles are added, in order, by the row kernel that follows.
// Exact fp32 products (v_mfma_f32_32x32x2_f32 / FMA) only.
// No workgroup waits on another; no atomics on results: every sum has a fixed order.
// The greedy decode with this predictor as a device loop (rnnt_engine_greedy_decode_lstm, k_ld_*) is at the end of the file, and after it
// the predictor step of a beam-search round (rnnt_engine_beam_decode_lstm, k_bl_*; the search itself is beam.hip's).  The LSTM cell is
// written once (lstm_cell) for training and the decode loops, and the scratch of a predictor step is laid out once (step_layout).
#include "../../include/rnnt_engine.h"
#include "decode_kernels.hpp"
#include "smallgemm.hpp"
#include "predictor_kernels.hpp"

namespace {

constexpr int MAX_L = 8, MAX_HD = 1024, MAX_E = 2048;
constexpr int UNITS = MAX_HD / 256;  // hidden units per thread of a row kernel: unit j = tid + 256 k, k < UNITS

inline size_t al(size_t x) { return (x + 63) & ~(size_t)63; }  // in floats

struct Dims { int B, U1, S, E, Hd, O, L, ln; };

// contraction ranges of a recurrent product over K: a wave gets at most 4 chunks of 8 (8 beyond 16 ranges)
inline int rec_splits(int K) { const int s = ((K + 7) / 8 + 15) / 16; return s < 1 ? 1 : (s > 16 ? 16 : s); }

// what the forward keeps for the backward, per row: E + O + 4 floats and 8 Hd + 2 per layer
struct SavedLayout {
    size_t x1, st1, z, st2;
    size_t ghat[MAX_L], chat[MAX_L], hp[MAX_L], cp[MAX_L], y[MAX_L], rs[MAX_L];
    size_t total;
};
SavedLayout saved_layout(const Dims &d)
{
    const size_t M = (size_t)d.B * d.U1, Hd = d.Hd;
    SavedLayout s;
    size_t o = 0;
    s.x1 = o;  o += al(M * d.E);
    s.st1 = o; o += al(2 * M);
    for (int l = 0; l < d.L; ++l) {
        s.ghat[l] = o; o += al(M * 4 * Hd);  // normalised gates before the affine (no layer norm: the summed gates)
        s.chat[l] = o; o += al(M * Hd);      // normalised cell before the affine (no layer norm: the cell)
        s.hp[l] = o;   o += al(M * Hd);      // h_{t-1} of every step: row (b,0) is the initial state
        s.cp[l] = o;   o += al(M * Hd);      // c_{t-1}
        s.y[l] = o;    o += al(M * Hd);      // the layer's output after dropout
        s.rs[l] = o;   o += al(2 * M);       // rstd of g_norm, c_norm
    }
    s.z = o;   o += al(M * d.O);
    s.st2 = o; o += al(2 * M);
    s.total = o;
    return s;
}

// forward scratch: the x2g product of one layer, one step's recurrent product and — for a call that keeps nothing — the activations
struct FwdLayout { size_t xg, rg, x1, st1, ya, yb, hb, cb, z, st2, total; };
FwdLayout fwd_layout(const Dims &d)
{
    const size_t M = (size_t)d.B * d.U1, Hd = d.Hd;
    FwdLayout f;
    size_t o = 0;
    f.xg = o;  o += al(M * 4 * Hd);
    f.rg = o;  o += al((size_t)rec_splits(d.Hd) * d.B * 4 * Hd);  // the recurrent product's partial tiles
    f.x1 = o;  o += al(M * d.E);
    f.st1 = o; o += al(2 * M);
    f.ya = o;  o += al(M * Hd);
    f.yb = o;  o += al(M * Hd);
    f.hb = o;  o += al(2 * (size_t)d.B * Hd);  // h and c of the running step, ping-pong
    f.cb = o;  o += al(2 * (size_t)d.B * Hd);
    f.z = o;   o += al(M * d.O);
    f.st2 = o; o += al(2 * M);
    f.total = o;
    return f;
}

struct BwdLayout { size_t dz, t, dy, dpre, tg, draw, dcn, tc, dhrec, dc, slabs, cs, total; };
BwdLayout bwd_layout(const Dims &d)
{
    const size_t M = (size_t)d.B * d.U1, Hd = d.Hd;
    const size_t W = d.E > d.O ? d.E : d.O, Wi = d.E > d.Hd ? d.E : d.Hd;
    BwdLayout b;
    size_t o = 0;
    b.dz = o;    o += al(M * W);
    b.t = o;     o += al(M * W);
    b.dy = o;    o += al(M * Wi);
    b.dpre = o;  o += al(M * 4 * Hd);
    b.tg = o;    o += al(M * 4 * Hd);
    b.draw = o;  o += al(M * 4 * Hd);
    b.dcn = o;   o += al(M * Hd);
    b.tc = o;    o += al(M * Hd);
    b.dhrec = o; o += al((size_t)rec_splits(4 * d.Hd) * d.B * Hd);
    b.dc = o;    o += al((size_t)d.B * Hd);
    const size_t wmax = 4 * Hd * Wi > (size_t)d.O * Hd ? 4 * Hd * Wi : (size_t)d.O * Hd;
    b.slabs = o; o += al((size_t)sgemm_tn_splits((int)M) * wmax);
    const size_t cw = 4 * Hd > W ? 4 * Hd : W;
    b.cs = o;    o += al(colsum_scratch_floats((int)M, (int)cw));
    b.total = o;
    return b;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// training: row (b,0) of the h_{t-1} / c_{t-1} sequences = the initial state (NULL: zeros)
__global__ __launch_bounds__(256) void k_lstm_init(const float *__restrict__ h0, const float *__restrict__ c0, int Hd, long ld,
                                                   float *__restrict__ hp, float *__restrict__ cp)
{
    const int b = blockIdx.x;
    for (int j = threadIdx.x; j < Hd; j += 256) {
        hp[b * ld + j] = h0 ? h0[(long)b * Hd + j] : 0.f;
        cp[b * ld + j] = c0 ? c0[(long)b * Hd + j] : 0.f;
    }
}

// ---- the recurrent products: P[split][m][n] = sum over the split's k of A[m,k] W(n,k), M = B rows.
// NN = false: W [N][K] rows ldw apart (h p2g^T: N = 4 Hd, K = Hd); NN = true: W [K][N] (dgates p2g: N = Hd, K = 4 Hd).
// grid (ceil(N/32), KS, ceil(M/32)); chunk c of 8 contraction elements belongs to wave c % 4 of split (c / 4) % KS; the four
// waves' tiles are added through LDS in wave order.
// `rows` (NULL for every product but the beam search's): operand row m is A's row rows[m], held inside [0, R) — a hypothesis reads the
// LSTM state it continues through its index (DESIGN.md §4h "LSTM"); the output row stays m.
struct RecArgs { const float *A; long lda; const float *W; long ldw; float *P; int M, N, K, KS; const int *rows = nullptr; int R = 0; };

// one workgroup's tile of such a product: output columns n0 .. n0 + 31, rows m0 .. m0 + 31, contraction range `split`; red: 3 * 1024 floats of LDS
template <bool NN>
__device__ __forceinline__ void rec_tile(const RecArgs &a, int n0, int split, int m0, float *red)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 31, half = lane >> 5;
    const int row = min(m0 + i, a.M - 1), col = min(n0 + i, a.N - 1);
    const int arow = a.rows ? min(max(a.rows[row], 0), a.R - 1) : row;
    const int KC = (a.K + 7) / 8;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int c0 = split * 4 + wave; c0 < KC; c0 += 16 * a.KS) {  // four chunks in flight
        f32x4 x[4], w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + 4 * a.KS * j, k = 8 * c + 4 * half;
            const bool ok = c < KC && k < a.K;
            const int kk = ok ? k : 0;
            x[j] = *(const f32x4 *)(a.A + (long)arow * a.lda + kk);
            if (!ok) x[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (NN) {
#pragma unroll
                for (int s = 0; s < 4; ++s) w[j][s] = a.W[(long)(kk + s) * a.ldw + col];
            } else {
                w[j] = *(const f32x4 *)(a.W + (long)col * a.ldw + kk);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[j][s], w[j][s], acc, 0, 0, 0);
    }
    if (wave != 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(wave - 1) * 1024 + r * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (wave != 0 || n0 + i >= a.N) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m >= a.M) continue;
        const float v = ((acc[r] + red[r * 64 + lane]) + red[1024 + r * 64 + lane]) + red[2048 + r * 64 + lane];
        a.P[((long)split * a.M + m) * a.N + n0 + i] = v;
    }
}

template <bool NN>
__global__ __launch_bounds__(256) void k_rec_gemm(RecArgs a)
{
    __shared__ float red[3 * 1024];
    rec_tile<NN>(a, blockIdx.x * 32, blockIdx.y, blockIdx.z * 32, red);
}

template <bool NN>
void launch_rec_gemm(const float *A, long lda, const float *W, long ldw, float *P, int M, int N, int K, hipStream_t st)
{
    const RecArgs a = {A, lda, W, ldw, P, M, N, K, rec_splits(K)};
    hipLaunchKernelGGL(k_rec_gemm<NN>, dim3((N + 31) / 32, a.KS, (M + 31) / 32), dim3(256), 0, st, a);
}

struct StepF {
    const float *xg; long xg_ld;        // x2g(x_t): row b at xg + b xg_ld
    const float *rg; int rg_n; long rg_ld;  // p2g(h_{t-1}): rg_n partial products [B,4Hd], rg_ld apart; NULL: h_{t-1} = 0
    const float *cprev; long cprev_ld;  // c_{t-1}; NULL: zeros
    const float *gw, *gb, *cw, *cb;     // g_norm / c_norm affines (LN only)
    float eps;
    float *hnext; long hnext_ld;        // h_t before dropout: the next step's h_{t-1}, or the state out
    float *cnext; long cnext_ld;
    float *y; long y_ld;                // h_t after dropout: the layer's output row
    const unsigned char *keep; long keep_ld; float scale;
    float *ghat; long ghat_ld; float *chat; long chat_ld; float *rs; long rs_ld;  // kept for the backward (NULL: inference)
    int Hd;
};

// The LSTM cell of ONE row by the workgroup's 256 threads, from the row's summed gates `g` (unit j = tid + 256 k; zeros in a lane j >= Hd):
// g_norm over the 4 Hd gates, the nonlinearities, the cell update on c_prev[c_row + j] (c_prev NULL: zeros), c_norm, h = o tanh(c).
// Two sinks: kept(j, q, v) gets what a backward needs, each value where it is known — q < 4: unit j's normalised gate q before its
// affine, q == 4: its normalised cell before the affine (handing all of it over at the end holds 16 gates per thread in registers
// through the cell) —, unit(j, cn, h) the unit's new cell and h; unit may write where c_prev lies (a thread has read a unit's cell
// before it hands the unit over).  Returns (rstd of g_norm, rstd of c_norm).  red: 4 floats of LDS.
// The training forward and the decode loops share this body and differ in ONE thing that reaches the bits: the order in which they add
// a row's gates up — xg + (r0 + r1 + ...) there, ((p0 + p1) + ...) + bias here.
template <bool LN, class Kept, class Unit>
__device__ __forceinline__ float2 lstm_cell(float (&g)[UNITS][4], const float *c_prev, long c_row, const float *gw, const float *gb, const float *cw,
                                            const float *cb, float eps, int Hd, float *red, Kept kept, Unit unit)
{
    const int tid = threadIdx.x;
    float rstd_g = 1.f, rstd_c = 1.f;
    if (LN) {
        const float n = 4.f * Hd;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < UNITS; ++k) s += (g[k][0] + g[k][1]) + (g[k][2] + g[k][3]);
        s = block_sum(s, red);
        const float mean = s / n;
        float q2 = 0.f;
#pragma unroll
        for (int k = 0; k < UNITS; ++k)
            if (tid + 256 * k < Hd)
#pragma unroll
                for (int q = 0; q < 4; ++q) q2 += (g[k][q] - mean) * (g[k][q] - mean);
        q2 = block_sum(q2, red);
        rstd_g = rsqrtf(q2 / n + eps);
#pragma unroll
        for (int k = 0; k < UNITS; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) g[k][q] = (g[k][q] - mean) * rstd_g;
    }
    float c[UNITS], o[UNITS];
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
        const int j = tid + 256 * k;
        c[k] = 0.f; o[k] = 0.f;
        if (j >= Hd) continue;
        float pre[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            kept(j, q, g[k][q]);
            pre[q] = LN ? g[k][q] * gw[q * Hd + j] + gb[q * Hd + j] : g[k][q];
        }
        const float cp = c_prev ? c_prev[c_row + j] : 0.f;
        c[k] = sigmoidf(pre[1]) * cp + sigmoidf(pre[0]) * tanhf(pre[2]);
        o[k] = sigmoidf(pre[3]);
    }
    if (LN) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < UNITS; ++k) s += c[k];
        s = block_sum(s, red);
        const float mean = s / Hd;
        float q2 = 0.f;
#pragma unroll
        for (int k = 0; k < UNITS; ++k)
            if (tid + 256 * k < Hd) q2 += (c[k] - mean) * (c[k] - mean);
        q2 = block_sum(q2, red);
        rstd_c = rsqrtf(q2 / Hd + eps);
#pragma unroll
        for (int k = 0; k < UNITS; ++k) c[k] = (c[k] - mean) * rstd_c;
    }
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
        const int j = tid + 256 * k;
        if (j >= Hd) continue;
        const float cn = LN ? c[k] * cw[j] + cb[j] : c[k];
        kept(j, 4, c[k]);
        unit(j, cn, o[k] * tanhf(cn));
    }
    return make_float2(rstd_g, rstd_c);
}

// One workgroup per batch row: gates = xg + rg, the cell, and what the backward needs, the keep mask and the next row of the sequence.
template <bool LN>
__global__ __launch_bounds__(256) void k_lstm_step_fwd(StepF a)
{
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x, Hd = a.Hd;
    const float *xg = a.xg + b * a.xg_ld;
    const float *rg = a.rg ? a.rg + (long)b * 4 * Hd : nullptr;
    float g[UNITS][4];
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
        const int j = tid + 256 * k;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v = 0.f;
            if (j < Hd) {
                v = xg[q * Hd + j];
                if (rg) {
                    float r = rg[q * Hd + j];
                    for (int sp = 1; sp < a.rg_n; ++sp) r += rg[sp * a.rg_ld + q * Hd + j];
                    v += r;
                }
            }
            g[k][q] = v;
        }
    }
    // (the sinks hold the arguments by value: held by reference, the row offsets were recomputed in every unit pass)
    const float2 rstd = lstm_cell<LN>(
        g, a.cprev, b * a.cprev_ld, a.gw, a.gb, a.cw, a.cb, a.eps, Hd, red,
        [=](int j, int q, float v) {
            if (q < 4) {
                if (a.ghat) a.ghat[b * a.ghat_ld + q * Hd + j] = v;
            } else if (a.chat) a.chat[b * a.chat_ld + j] = v;
        },
        [=](int j, float cn, float h) {
            a.cnext[b * a.cnext_ld + j] = cn;
            a.hnext[b * a.hnext_ld + j] = h;
            float yv = h;
            if (a.keep) yv = a.keep[b * a.keep_ld + j] ? h * a.scale : 0.f;
            a.y[b * a.y_ld + j] = yv;
        });
    if (a.rs && tid == 0) { a.rs[b * a.rs_ld] = rstd.x; a.rs[b * a.rs_ld + 1] = rstd.y; }
}

struct StepB {
    const float *dy; long dy_ld;        // gradient of the layer's output row (after dropout)
    const unsigned char *keep; long keep_ld; float scale;
    const float *dhrec; int dh_n; long dh_ld;  // recurrent part of dh_t (from step t+1): dh_n partial products [B,Hd]; NULL at the last step
    float *dc; int dc_valid;            // [B,Hd] carried dc: read when valid, always written (dc_{t-1})
    const float *ghat; long ghat_ld; const float *chat; long chat_ld; const float *rs; long rs_ld;
    const float *cprev; long cprev_ld;
    const float *gw, *gb, *cw, *cb;
    float *dpre, *tg, *draw; long g_ld;  // rows of [M,4Hd]: d(gates after the affine), dpre * ghat, d(summed gates)
    float *dcn, *tc; long c_ld;          // rows of [M,Hd]: d(normalised cell), dcn * chat
    int Hd;
};

// One workgroup per batch row: back through h = o tanh(c), c_norm, the cell update, the gate nonlinearities and g_norm.
template <bool LN>
__global__ __launch_bounds__(256) void k_lstm_step_bwd(StepB a)
{
    __shared__ float red[8];
    const int b = blockIdx.x, tid = threadIdx.x, Hd = a.Hd;
    const float rstd_g = LN ? a.rs[b * a.rs_ld] : 1.f, rstd_c = LN ? a.rs[b * a.rs_ld + 1] : 1.f;
    float gh[UNITS][4], act[UNITS][4], ch[UNITS], dcn[UNITS], dout[UNITS];
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
        const int j = tid + 256 * k;
        ch[k] = 0.f; dcn[k] = 0.f; dout[k] = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) { gh[k][q] = 0.f; act[k][q] = 0.f; }
        if (j >= Hd) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            gh[k][q] = a.ghat[b * a.ghat_ld + q * Hd + j];
            const float pre = LN ? gh[k][q] * a.gw[q * Hd + j] + a.gb[q * Hd + j] : gh[k][q];
            act[k][q] = q == 2 ? tanhf(pre) : sigmoidf(pre);
        }
        ch[k] = a.chat[b * a.chat_ld + j];
        const float cn = LN ? ch[k] * a.cw[j] + a.cb[j] : ch[k];
        const float tc = tanhf(cn);
        float dh = a.dy[b * a.dy_ld + j];
        if (a.keep) dh = a.keep[b * a.keep_ld + j] ? dh * a.scale : 0.f;
        if (a.dhrec) {
            float r = a.dhrec[(long)b * Hd + j];
            for (int sp = 1; sp < a.dh_n; ++sp) r += a.dhrec[sp * a.dh_ld + (long)b * Hd + j];
            dh += r;
        }
        dout[k] = dh * tc;
        dcn[k] = dh * act[k][3] * (1.f - tc * tc);
        if (a.dc_valid) dcn[k] += a.dc[(long)b * Hd + j];
    }
    float dcr[UNITS];  // d(cell before c_norm)
    if (LN) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < UNITS; ++k) {
            const int j = tid + 256 * k;
            dcr[k] = 0.f;
            if (j >= Hd) continue;
            a.dcn[b * a.c_ld + j] = dcn[k];
            a.tc[b * a.c_ld + j] = dcn[k] * ch[k];
            dcr[k] = dcn[k] * a.cw[j];
            s1 += dcr[k];
            s2 += dcr[k] * ch[k];
        }
        block_sum2(s1, s2, red);
        const float c1 = s1 / Hd, c2 = s2 / Hd;
#pragma unroll
        for (int k = 0; k < UNITS; ++k) dcr[k] = rstd_c * (dcr[k] - c1 - ch[k] * c2);
    } else {
#pragma unroll
        for (int k = 0; k < UNITS; ++k) dcr[k] = dcn[k];
    }
    float dp[UNITS][4];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
        const int j = tid + 256 * k;
#pragma unroll
        for (int q = 0; q < 4; ++q) dp[k][q] = 0.f;
        if (j >= Hd) continue;
        const float i_ = act[k][0], f_ = act[k][1], g_ = act[k][2], o_ = act[k][3];
        const float cp = a.cprev[b * a.cprev_ld + j];
        a.dc[(long)b * Hd + j] = dcr[k] * f_;
        dp[k][0] = dcr[k] * g_ * i_ * (1.f - i_);
        dp[k][1] = dcr[k] * cp * f_ * (1.f - f_);
        dp[k][2] = dcr[k] * i_ * (1.f - g_ * g_);
        dp[k][3] = dout[k] * o_ * (1.f - o_);
        if (LN) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a.dpre[b * a.g_ld + q * Hd + j] = dp[k][q];
                a.tg[b * a.g_ld + q * Hd + j] = dp[k][q] * gh[k][q];
                dp[k][q] *= a.gw[q * Hd + j];
                s1 += dp[k][q];
                s2 += dp[k][q] * gh[k][q];
            }
        }
    }
    float c1 = 0.f, c2 = 0.f;
    if (LN) {
        block_sum2(s1, s2, red);
        c1 = s1 / (4.f * Hd); c2 = s2 / (4.f * Hd);
    }
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
        const int j = tid + 256 * k;
        if (j >= Hd) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            a.draw[b * a.g_ld + q * Hd + j] = LN ? rstd_g * (dp[k][q] - c1 - gh[k][q] * c2) : dp[k][q];
    }
}

int check_dims(const Dims &d)
{
    if (d.B <= 0 || d.U1 <= 0 || d.S <= 0 || d.E <= 0 || d.Hd <= 0 || d.O <= 0 || d.L <= 0)
        return engine_fail(RNNT_ERR_INVALID_ARG, "non-positive dimension B=%d U1=%d S=%d E=%d Hd=%d O=%d L=%d", d.B, d.U1, d.S, d.E,
                           d.Hd, d.O, d.L);
    if (d.E % 4 != 0 || d.Hd % 4 != 0 || d.O % 4 != 0 || d.Hd > MAX_HD || d.E > MAX_E || d.L > MAX_L)
        return engine_fail(RNNT_ERR_UNSUPPORTED,
                           "LSTMPredictor kernels need E %% 4 == 0, Hd %% 4 == 0, O %% 4 == 0, Hd <= %d, E <= %d and L <= %d (E=%d Hd=%d O=%d L=%d)",
                           MAX_HD, MAX_E, MAX_L, d.E, d.Hd, d.O, d.L);
    if ((long)d.B * d.U1 > 0x3fffffffL / 4) return engine_fail(RNNT_ERR_UNSUPPORTED, "B*U1 too large");
    return RNNT_OK;
}

bool bad(const void *q) { return !q || ((uintptr_t)q & 15); }

int check_params(const rnnt_lstm_predictor_params *p, int L, int ln, const char *what)
{
    if (!p || !p->layers) return engine_fail(RNNT_ERR_INVALID_ARG, "null %s struct or layer array", what);
    const void *outer[] = {p->embedding, p->ln_in_w, p->ln_in_b, p->linear_w, p->linear_b, p->ln_out_w, p->ln_out_b};
    for (const void *q : outer)
        if (bad(q)) return engine_fail(RNNT_ERR_INVALID_ARG, "null or not 16-byte aligned %s pointer", what);
    for (int l = 0; l < L; ++l) {
        const rnnt_lstm_layer_params &y = p->layers[l];
        if (bad(y.x2g_w) || bad(y.p2g_w)) return engine_fail(RNNT_ERR_INVALID_ARG, "layer %d: null or not 16-byte aligned %s weight", l, what);
        if (ln) {
            if (bad(y.g_norm_w) || bad(y.g_norm_b) || bad(y.c_norm_w) || bad(y.c_norm_b))
                return engine_fail(RNNT_ERR_INVALID_ARG, "layer %d: null or not 16-byte aligned %s g_norm / c_norm pointer", l, what);
        } else if (bad(y.x2g_b)) {
            return engine_fail(RNNT_ERR_INVALID_ARG, "layer %d: null or not 16-byte aligned %s x2g bias (no layer norm)", l, what);
        }
    }
    return RNNT_OK;
}

int status(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return engine_fail(RNNT_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return RNNT_OK;
}

SgArgs sg(const float *A, long lda, const float *B, long ldb, float *C, long ldc, int M, int N, int K)
{
    SgArgs a;
    a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.C = C; a.ldc = ldc;
    a.bias = nullptr; a.Cpre = nullptr; a.mask = nullptr; a.mask_scale = 1.f;
    a.M = M; a.N = N; a.K = K; a.taps = 1; a.seg = M; a.act = 0; a.ksplit = 1;
    return a;
}


// ---------------------------------------------------------------------------------------
// Device-resident greedy decode with this predictor (rnnt_engine_greedy_decode_lstm; DESIGN.md §4p "Device decode"): the loop of
// reference rnnt/model.py:45-87 for n_utt <= 32 independent utterances in lockstep — the rows of ONE 32-row tile of every product —
// as a fixed kernel sequence per ITERATION, every decision on the device (the control flow is decode.hip's k_dec_update):
//   [embedding + input LayerNorm of the rows that emitted a label]  per layer [both gate products: x x2g^T and h p2g^T, one launch]
//   [row step: gates, g_norm, cell, c_norm, h — in place]  [linear product] [+ bias, output LayerNorm]  with joint.text_ln
//   [its product] [+ bias]  [scan of scan_frames frames from each utterance's own t]  [argmax + bookkeeping per utterance].
// state (int32[n_utt][8], the DEC_ST_* words of decode_kernels.hpp): t, emitted, ntok, done, newtok: the predictor has a label to
//   take in, iterations that did work, settled: done and the last label taken in (nothing is left to do for the utterance).
// A row whose utterance emitted nothing leaves h, c and its text vector untouched; a product computes every row of the tile and
// the row kernels ignore the others.  Row m of a product reads row m of its operand only and the contraction ranges depend on K
// alone, so an utterance's numbers do not depend on its neighbours, its position or n_utt.  No atomics on results (one counter of
// settled utterances raises the host's flag), no workgroup waits on another, every sum in a fixed order.
// ---------------------------------------------------------------------------------------
// floats per row of the partial tiles of the widest product of a predictor step (gates: both products of a layer; linear; text_ln)
size_t ld_gp_floats(int E, int Hd, int O, int H)
{
    size_t g = (size_t)(rec_splits(E) + rec_splits(Hd)) * 4 * Hd;
    if ((size_t)2 * rec_splits(Hd) * 4 * Hd > g) g = (size_t)2 * rec_splits(Hd) * 4 * Hd;
    if ((size_t)rec_splits(Hd) * O > g) g = (size_t)rec_splits(Hd) * O;
    if ((size_t)rec_splits(O) * H > g) g = (size_t)rec_splits(O) * H;
    return g;
}

// the scratch of a predictor step of `rows` rows, in floats: x1, y and gp; for a greedy loop (scan_frames > 0) the scan's candidates and
// the control words as well; owns_state: the rows' text vectors [rows][H] — first, the ABI says so — and h, c [L][2][rows][Hd] too (the
// offline loop; a stream keeps them in its block, a beam round in its pool)
struct StepLayout { size_t text, x1, hc, y, gp, part, ctrl, total; };
StepLayout step_layout(int rows, int E, int Hd, int O, int L, int H, int V, int scan_frames, bool owns_state)
{
    const size_t n = rows;
    StepLayout w;
    size_t o = 0;
    w.text = o; if (owns_state) o += al(n * H);
    w.x1 = o;   o += al(n * E);
    w.hc = o;   if (owns_state) o += al((size_t)L * 2 * n * Hd);
    w.y = o;    o += al(n * O);
    w.gp = o;   o += al(ld_gp_floats(E, Hd, O, H) * n);
    w.part = o; if (scan_frames) o += al(n * scan_frames * ((V + 31) / 32) * 2);
    w.ctrl = o; if (scan_frames) o += 64;
    w.total = o;
    return w;
}

// ---- the streaming form (rnnt_engine_greedy_stream_lstm_*): a stream's words are the loop's — the kernels below read them at the same
// places, `st_ld` words from one row to the next — with "done" split in two: PAUSED (nothing to scan: the push's frames are consumed or
// the cap is reached; the loop's DONE) and DONE (the cap alone, which outlives the push), "settled" read as AT REST, and the words a
// stream needs beyond an utterance's
enum {
    LS_WORDS = RNNT_LSTM_STREAM_STATE_WORDS, LS_DONE = RNNT_LSTM_STREAM_DONE, LS_FRAMES = RNNT_LSTM_STREAM_FRAMES,
    LS_NEWEST = RNNT_LSTM_STREAM_NEWEST, LS_PUSH_LABELS = RNNT_LSTM_STREAM_PUSH_LABELS, LS_BASE = RNNT_LSTM_STREAM_BASE
};
static_assert(RNNT_LSTM_STREAM_T == DEC_ST_T && RNNT_LSTM_STREAM_EMITTED == DEC_ST_EMITTED && RNNT_LSTM_STREAM_LABELS == DEC_ST_NTOK &&
              RNNT_LSTM_STREAM_PAUSED == DEC_ST_DONE && RNNT_LSTM_STREAM_NEWTOK == DEC_ST_NEWTOK &&
              RNNT_LSTM_STREAM_PUSH_ITERATIONS == DEC_ST_ITERS && RNNT_LSTM_STREAM_AT_REST == DEC_ST_SETTLED,
              "a stream's words are the loop's");

// the block of n streams: state words | h, c [L][2][n][Hd] | text vectors [n][H], in floats (= int32 words), each section 256-byte aligned
struct LsBlock { size_t state, hc, text, total; };
LsBlock ls_block(int n, int Hd, int L, int H)
{
    LsBlock b;
    size_t o = 0;
    b.state = o; o += al((size_t)n * LS_WORDS);
    b.hc = o;    o += al((size_t)L * 2 * n * Hd);
    b.text = o;  o += al((size_t)n * H);
    b.total = o;
    return b;
}

// whether the predictor has a label of this row's to take in NOW (a stream at rest keeps its start blank for the push that brings it a
// frame; an utterance of the offline loop never has both words set)
__device__ __forceinline__ bool ld_takes_label(const int32_t *st) { return st[DEC_ST_NEWTOK] != 0 && st[DEC_ST_SETTLED] == 0; }

__global__ __launch_bounds__(256) void k_ld_init(int32_t *__restrict__ states, int32_t *__restrict__ tokens, int max_length, int blank,
                                                 int n_utt, float *__restrict__ hc, int nhc, int32_t *__restrict__ ctrl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nhc) hc[i] = 0.f;
    if (i < n_utt) {
        dec_state_init(states + DEC_ST_WORDS * i);
        tokens[(long)i * max_length] = blank;
    }
    if (i == 0) ctrl[0] = 0;
}

// one row of the embedding + input LayerNorm: out[E] = LayerNorm_E(embedding[tok]) (the workgroup's 256 threads; red: 4 floats of LDS)
__device__ __forceinline__ void ld_embed_row(const float *__restrict__ emb, int S, int tok, const float *__restrict__ gamma,
                                             const float *__restrict__ beta, float eps, int E, float *__restrict__ out, float *red)
{
    const int tid = threadIdx.x;
    tok = tok < 0 ? 0 : (tok >= S ? S - 1 : tok);
    const float *e = emb + (long)tok * E;
    float mean, rstd;
    row_ln_stats(e, E, eps, red, mean, rstd);
    for (int i = tid; i < E; i += 256) out[i] = (e[i] - mean) * rstd * gamma[i] + beta[i];
}

// x1[u] = LayerNorm_E(embedding[the utterance's newest token]) for the utterances that have one; tokens NULL (a stream): the token is
// the state's LS_NEWEST word
__global__ __launch_bounds__(256) void k_ld_embed(const int32_t *__restrict__ states, int st_ld, const int32_t *__restrict__ tokens, int max_length,
                                                  const float *__restrict__ emb, int S, const float *__restrict__ gamma,
                                                  const float *__restrict__ beta, float eps, int E, float *__restrict__ x1)
{
    __shared__ float red[4];
    const int u = blockIdx.x;
    const int32_t *st = states + st_ld * u;
    if (!ld_takes_label(st)) return;
    ld_embed_row(emb, S, tokens ? tokens[(long)u * max_length + st[DEC_ST_NTOK]] : st[LS_NEWEST], gamma, beta, eps, E, x1 + (long)u * E, red);
}

// whether any utterance has a label for the predictor to take in (workgroup-uniform; n_utt <= 32)
__device__ __forceinline__ bool ld_any_new(const int32_t *states, int st_ld, int n_utt)
{
    const int u = threadIdx.x & 63;
    return __ballot(u < n_utt && ld_takes_label(states + st_ld * u)) != 0ull;
}

// up to two NT products of the same M = n_utt rows and N columns in one launch: grid (ceil(N/32), KS0 + KS1); the partial tiles of
// product 0's ranges, then product 1's, at P[range][m][n] — the row kernel that follows adds them in that order
struct LdGemm { const int32_t *states; int st_ld, n_utt; RecArgs g[2]; };
__global__ __launch_bounds__(256) void k_ld_gemm(LdGemm a)
{
    __shared__ float red[3 * 1024];
    if (!ld_any_new(a.states, a.st_ld, a.n_utt)) return;
    const int which = (int)blockIdx.y >= a.g[0].KS ? 1 : 0;
    rec_tile<false>(a.g[which], blockIdx.x * 32, blockIdx.y - (which ? a.g[0].KS : 0), 0, red);
}

struct LdStep {
    const int32_t *states; int st_ld;
    const float *gp; int nsp; long gp_ld;  // nsp partial products [n_utt,4Hd], gp_ld apart
    const float *xb;                       // x2g bias (no layer norm) or NULL
    const float *gw, *gb, *cw, *cb; float eps;
    float *h, *c;                          // [n_utt,Hd], updated in place
    float *h_out, *c_out;                  // the caller's state_out rows, or NULL
    int Hd;
};

// k_lstm_step_fwd's cell (lstm_cell) in eval mode, nothing kept, for ONE row (the workgroup's 256 threads; red: 4 floats of LDS): `gp` the
// row's first partial product, `c_prev` [Hd] the cell it continues, `h` / `c` [Hd] where the new state goes (c may be c_prev: a thread
// reads a unit's cell before it writes it), `h2` / `c2` a second copy or NULL
template <bool LN>
__device__ __forceinline__ void ld_step_row(const LdStep &a, const float *__restrict__ gp, const float *c_prev, float *h, float *c_new,
                                            float *h2, float *c2, float *red)
{
    const int tid = threadIdx.x, Hd = a.Hd;
    float g[UNITS][4];
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
        const int j = tid + 256 * k;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v = 0.f;
            if (j < Hd) {
                v = gp[q * Hd + j];
                for (int sp = 1; sp < a.nsp; ++sp) v += gp[sp * a.gp_ld + q * Hd + j];
                if (a.xb) v += a.xb[q * Hd + j];
            }
            g[k][q] = v;
        }
    }
    __builtin_assume(c_prev != nullptr);
    lstm_cell<LN>(g, c_prev, 0, a.gw, a.gb, a.cw, a.cb, a.eps, Hd, red, [](int, int, float) {}, [&](int j, float cn, float hv) {
        c_new[j] = cn;
        h[j] = hv;
        if (h2) { c2[j] = cn; h2[j] = hv; }
    });
}

// the step of the rows whose utterance has a new label: one workgroup per utterance, h and c in place
template <bool LN>
__global__ __launch_bounds__(256) void k_ld_step(LdStep a)
{
    __shared__ float red[4];
    const int b = blockIdx.x, Hd = a.Hd;
    if (!ld_takes_label(a.states + a.st_ld * b)) return;
    float *h = a.h + (long)b * Hd, *c = a.c + (long)b * Hd;
    ld_step_row<LN>(a, a.gp + (long)b * 4 * Hd, c, h, c, a.h_out ? a.h_out + (long)b * Hd : nullptr,
                    a.h_out ? a.c_out + (long)b * Hd : nullptr, red);
}

// one row: y[N] = sum of the nsp partial products (the row's first at `gp`, gp_ld apart) + bias, LN: then LayerNorm_N (gamma, beta, eps)
template <bool LN>
__device__ __forceinline__ void ld_rowfin_row(const float *__restrict__ gp, int nsp, long gp_ld, int N, const float *__restrict__ bias,
                                              const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                              float *__restrict__ y, float *red)
{
    const int tid = threadIdx.x;
    float s = 0.f;
    for (int i = tid; i < N; i += 256) {  // (a thread reads back only what it wrote itself)
        float v = gp[i];
        for (int sp = 1; sp < nsp; ++sp) v += gp[sp * gp_ld + i];
        v += bias[i];
        y[i] = v;
        s += v;
    }
    if (!LN) return;
    const float mean = block_sum(s, red) / N, rstd = row_ln_rstd(y, N, mean, eps, red);
    for (int i = tid; i < N; i += 256) y[i] = (y[i] - mean) * rstd * gamma[i] + beta[i];
}

// out[u] = that row — for the utterances with a new label
template <bool LN>
__global__ __launch_bounds__(256) void k_ld_rowfin(const int32_t *__restrict__ states, int st_ld, const float *__restrict__ gp, int nsp, long gp_ld, int N,
                                                   const float *__restrict__ bias, const float *__restrict__ gamma,
                                                   const float *__restrict__ beta, float eps, float *__restrict__ out)
{
    __shared__ float red[4];
    const int u = blockIdx.x;
    if (!ld_takes_label(states + st_ld * u)) return;
    ld_rowfin_row<LN>(gp + (long)u * N, nsp, gp_ld, N, bias, gamma, beta, eps, out + (long)u * N, red);
}

// an utterance's first row and frame count from the caller's device table, held inside the packed buffer whatever the table says
__device__ __forceinline__ void ld_utt(const int32_t *utt, int u, int rows, int &first, int &T)
{
    first = min(max(utt[2 * u], 0), rows - 1);
    T = min(max(utt[2 * u + 1], 1), rows - first);
}

// decode.hip's k_dec_scan_logits<false> with the utterance as grid dimension z: scan_frames frames from the utterance's own t against
// its own text vector (the scan tile of decode_kernels.hpp), one (max, first index) candidate per frame and 32 vocabulary entries
__global__ __launch_bounds__(256) void k_ld_scan(const int32_t *__restrict__ states, int st_ld, const float *__restrict__ enc, long enc_st,
                                                 const int32_t *__restrict__ utt, int rows, const float *__restrict__ text,
                                                 const float *__restrict__ W, const float *__restrict__ bias, float2 *__restrict__ part, int K,
                                                 int H, int V)
{
    __shared__ float s_acc[3][16][64];
    const int u = blockIdx.z;
    const int32_t *state = states + st_ld * u;
    if (state[DEC_ST_DONE]) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, half = lane >> 5;
    const int v0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    int first, T;
    ld_utt(utt, u, rows, first, T);
    const int t0 = min(max(state[DEC_ST_T], 0), T - 1);
    const int frame = first + min(t0 + min(k0 + i, K - 1), T - 1), vrow = min(v0 + i, V - 1);
    const float *er = enc + (long)frame * enc_st + 4 * half;
    const float *pr = text + (long)u * H + 4 * half;
    const float *wr = W + (long)vrow * H + 4 * half;
    f32x16 acc;
    scan_tile_mul(acc, er, pr, wr, H / 8, wave);
    scan_tile_reduce(acc, s_acc, lane, wave);
    if (wave == 0) scan_tile_candidates(acc, bias, v0, k0, K, V, part + (long)u * K * gridDim.x, lane);
}

// k_dec_update's rules per utterance (one workgroup each).  An utterance that ended on a label keeps newtok for one more iteration —
// the predictor takes the label in, so that state_out and the text vector are those AFTER the last label — and settles in the next;
// ctrl[0] counts the settled utterances, the last one raises the host's flag.
//
// STREAM (rnnt_engine_greedy_stream_lstm_push): the same rules with the push as the utterance — T its frame count, t relative to it, the
// row's "done" word PAUSED, "settled" AT REST — and what a stream adds: a label goes to the push's out_tokens row and into the state's
// NEWEST word (there is no tokens[max_length] row to index: max_length 0 is unbounded), the frames are counted over all pushes, and the
// cap is kept in a word of its own, which outlives the push.
struct LdUpdate {
    const float2 *part; int K, NB, blank; const int32_t *utt; int rows, max_length, max_per_frame, n_utt;
    int32_t *states;
    int32_t *tokens; int tok_ld;  // [n_utt][max_length] with the leading blank; a stream: the push's out_tokens [n_streams][tok_ld]
    int32_t *ctrl, *host_flag;
};
template <bool STREAM>
__global__ __launch_bounds__(128) void k_ld_update(LdUpdate a)
{
    __shared__ int s_tok[128];
    const int u = blockIdx.x, K = a.K;
    int32_t *state = a.states + (STREAM ? (int)LS_WORDS : (int)DEC_ST_WORDS) * u;
    if (state[DEC_ST_SETTLED]) return;
    const bool was_done = state[DEC_ST_DONE] != 0;
    if (!was_done && (int)threadIdx.x < K) s_tok[threadIdx.x] = cand_argmax(a.part + ((long)u * K + threadIdx.x) * a.NB, a.NB);
    __syncthreads();
    if (threadIdx.x != 0) return;
    int done = 1, newtok = 0;
    if (!was_done) {
        int first, T;
        ld_utt(a.utt, u, a.rows, first, T);
        const int t = state[DEC_ST_T], n = min(K, T - t);
        const int hit = dec_first_hit(s_tok, n, a.blank);
        const int maxlen = STREAM && a.max_length == 0 ? 0x7fffffff : a.max_length;
        const DecPos p = dec_advance(t, state[DEC_ST_EMITTED], state[DEC_ST_NTOK], hit, n, T, maxlen, a.max_per_frame, [&](int at) {
            if (STREAM) {  // (held inside the row whatever the caller's table says)
                a.tokens[(long)u * a.tok_ld + min(state[LS_PUSH_LABELS], a.tok_ld - 1)] = s_tok[hit];
                state[LS_PUSH_LABELS] += 1;
                state[LS_NEWEST] = s_tok[hit];
            } else
                a.tokens[(long)u * a.tok_ld + at] = s_tok[hit];
        });
        state[DEC_ST_T] = p.t; state[DEC_ST_EMITTED] = p.emitted; state[DEC_ST_NTOK] = p.ntok; state[DEC_ST_DONE] = p.done;
        if (STREAM) {
            state[LS_FRAMES] = state[LS_BASE] + p.t;
            state[LS_DONE] = p.ntok + 1 >= maxlen ? 1 : 0;
        }
        done = p.done; newtok = p.newtok;
        state[DEC_ST_ITERS] += 1;
    }
    state[DEC_ST_NEWTOK] = newtok;
    if (done && !newtok) {
        state[DEC_ST_SETTLED] = 1;
        if (atomicAdd(a.ctrl, 1) + 1 == a.n_utt && a.host_flag) __hip_atomic_store(a.host_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// all streams (index < 0) or stream `index` alone start a new utterance: grid (ceil(max(2 L Hd, H, LS_WORDS) / 256), streams started).
// Nothing of another stream's is written.
__global__ __launch_bounds__(256) void k_ls_init(int32_t *__restrict__ states, float *__restrict__ hc, float *__restrict__ text, int n, int Hd,
                                                 int L, int H, int blank, int index)
{
    const int u = index < 0 ? (int)blockIdx.y : index, i = blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * L * Hd) hc[((long)(i / Hd) * n + u) * Hd + i % Hd] = 0.f;
    if (i < H) text[(long)u * H + i] = 0.f;
    if (i < LS_WORDS)  // zero frames: at rest, the start blank waiting for the push that brings a frame
        states[LS_WORDS * u + i] = i == DEC_ST_NEWTOK || i == DEC_ST_DONE || i == DEC_ST_SETTLED ? 1 : i == LS_NEWEST ? blank : 0;
}

// a push begins (one workgroup of 64, a lane per stream): a stream that got frames and is not done leaves its rest — base latched, the
// per-push words cleared —, the others stay as they are, bit for bit, and are counted as at rest already
__global__ __launch_bounds__(64) void k_ls_begin(int32_t *__restrict__ states, const int32_t *__restrict__ table, int n,
                                                 int32_t *__restrict__ ctrl, int32_t *host_flag)
{
    const int u = threadIdx.x;
    bool rests = false;
    if (u < n) {
        int32_t *st = states + LS_WORDS * u;
        rests = table[2 * u + 1] <= 0 || st[LS_DONE] != 0;
        if (!rests) {
            st[LS_BASE] = st[LS_FRAMES];
            st[DEC_ST_T] = 0; st[DEC_ST_DONE] = 0; st[DEC_ST_SETTLED] = 0; st[DEC_ST_ITERS] = 0; st[LS_PUSH_LABELS] = 0;
        }
    }
    const int at_rest = __popcll(__ballot(rests));
    if (u == 0) {
        ctrl[0] = at_rest;
        if (at_rest == n && host_flag) __hip_atomic_store(host_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// where a loop's buffers are: the offline loop keeps all of them in its workspace, a stream its states, hc and text in its block
struct LdArgs {
    const float *frames; long frame_stride; int rows; const int32_t *utt; int n_utt;
    rnnt_lstm_predictor_params p; int S, E, Hd, O, L, ln; float eps_in, eps_lstm, eps_out;
    const float *text_W, *text_b, *W, *bias; int H, V, blank, max_length, max_per_frame, scan_frames, iterations, init;
    int32_t *host_flag, *state, *tokens; float *state_out;
    float *text, *x1, *hc, *y, *gp; float2 *part; int32_t *ctrl;
    int stream = 0, tok_ld = 0;  // a stream's push: `init` = begin, `tokens` = out_tokens [n_utt][tok_ld], `utt` = the push table
};

RecArgs ld_prod(const float *A, const float *W, float *P, int M, int N, int K)
{
    return RecArgs{A, (long)K, W, (long)K, P, M, N, K, rec_splits(K)};
}

void launch_ld_loop(const LdArgs &a, hipStream_t st)
{
    const int n = a.n_utt, E = a.E, Hd = a.Hd, O = a.O, L = a.L, H = a.H, V = a.V, K = a.scan_frames, NB = (V + 31) / 32;
    float *text = a.text, *x1 = a.x1, *hc = a.hc, *y = a.y, *gp = a.gp;
    float2 *part = a.part;
    int32_t *ctrl = a.ctrl;
    const long nH = (long)n * Hd;
    const int st_ld = a.stream ? (int)LS_WORDS : (int)DEC_ST_WORDS;
    if (a.init && a.stream) hipLaunchKernelGGL(k_ls_begin, dim3(1), dim3(64), 0, st, a.state, a.utt, n, ctrl, a.host_flag);
    else if (a.init) {
        const int nhc = (int)(2 * L * nH);
        hipLaunchKernelGGL(k_ld_init, dim3((nhc + 255) / 256), dim3(256), 0, st, a.state, a.tokens, a.max_length, a.blank, n, hc, nhc, ctrl);
    }
    LdUpdate up{part, K, NB, a.blank, a.utt, a.rows, a.max_length, a.max_per_frame, n, a.state, a.tokens, a.stream ? a.tok_ld : a.max_length,
                ctrl, a.host_flag};
    for (int it = 0; it < a.iterations; ++it) {
        hipLaunchKernelGGL(k_ld_embed, dim3(n), dim3(256), 0, st, a.state, st_ld, a.stream ? (const int32_t *)nullptr : a.tokens, a.max_length, a.p.embedding, a.S, a.p.ln_in_w,
                           a.p.ln_in_b, a.eps_in, E, x1);
        for (int l = 0; l < L; ++l) {
            const rnnt_lstm_layer_params &q = a.p.layers[l];
            float *h = hc + (long)(2 * l) * nH, *c = h + nH;
            const int in = l ? Hd : E;
            LdGemm g;
            g.states = a.state; g.st_ld = st_ld; g.n_utt = n;
            g.g[0] = ld_prod(l ? h - 2 * nH : x1, q.x2g_w, gp, n, 4 * Hd, in);  // the layer below's NEW h (its row kernel has run)
            g.g[1] = ld_prod(h, q.p2g_w, gp + (long)g.g[0].KS * n * 4 * Hd, n, 4 * Hd, Hd);  // this layer's h of the step before
            hipLaunchKernelGGL(k_ld_gemm, dim3((4 * Hd + 31) / 32, g.g[0].KS + g.g[1].KS), dim3(256), 0, st, g);
            LdStep s;
            s.states = a.state; s.st_ld = st_ld; s.gp = gp; s.nsp = g.g[0].KS + g.g[1].KS; s.gp_ld = 4 * nH;
            s.xb = a.ln ? nullptr : q.x2g_b;
            s.gw = q.g_norm_w; s.gb = q.g_norm_b; s.cw = q.c_norm_w; s.cb = q.c_norm_b; s.eps = a.eps_lstm;
            s.h = h; s.c = c;
            s.h_out = a.state_out ? a.state_out + (long)(2 * l) * nH : nullptr; s.c_out = a.state_out ? s.h_out + nH : nullptr;
            s.Hd = Hd;
            if (a.ln) hipLaunchKernelGGL(k_ld_step<true>, dim3(n), dim3(256), 0, st, s);
            else hipLaunchKernelGGL(k_ld_step<false>, dim3(n), dim3(256), 0, st, s);
        }
        LdGemm g;
        g.states = a.state; g.st_ld = st_ld; g.n_utt = n;
        g.g[0] = ld_prod(hc + (long)(2 * (L - 1)) * nH, a.p.linear_w, gp, n, O, Hd);
        g.g[1] = g.g[0]; g.g[1].KS = 0;
        hipLaunchKernelGGL(k_ld_gemm, dim3((O + 31) / 32, g.g[0].KS), dim3(256), 0, st, g);
        // without joint.text_ln the output LayerNorm's row IS the text vector (O == H)
        hipLaunchKernelGGL(k_ld_rowfin<true>, dim3(n), dim3(256), 0, st, a.state, st_ld, gp, g.g[0].KS, (long)n * O, O, a.p.linear_b, a.p.ln_out_w,
                           a.p.ln_out_b, a.eps_out, a.text_W ? y : text);
        if (a.text_W) {
            g.g[0] = ld_prod(y, a.text_W, gp, n, H, O);
            g.g[1] = g.g[0]; g.g[1].KS = 0;
            hipLaunchKernelGGL(k_ld_gemm, dim3((H + 31) / 32, g.g[0].KS), dim3(256), 0, st, g);
            hipLaunchKernelGGL(k_ld_rowfin<false>, dim3(n), dim3(256), 0, st, a.state, st_ld, gp, g.g[0].KS, (long)n * H, H, a.text_b,
                               (const float *)nullptr, (const float *)nullptr, 0.f, text);
        }
        hipLaunchKernelGGL(k_ld_scan, dim3(NB, (K + 31) / 32, n), dim3(256), 0, st, a.state, st_ld, a.frames, a.frame_stride, a.utt, a.rows, text, a.W,
                           a.bias, part, K, H, V);
        if (a.stream) hipLaunchKernelGGL(k_ld_update<true>, dim3(n), dim3(128), 0, st, up);
        else hipLaunchKernelGGL(k_ld_update<false>, dim3(n), dim3(128), 0, st, up);
    }
}

// ---------------------------------------------------------------------------------------
// The predictor step of a beam-search round (rnnt_engine_beam_decode_lstm; DESIGN.md §4h "LSTM"): the kernels above with a beam's slots
// as rows — row 16 u + s is slot s of utterance u, so a 32-row tile holds two utterances — for the slots that took a label
// (BeamSlots::need of the search's current buffer).  A slot CONTINUES the state in pool row par[row] (its parent hypothesis's: siblings
// share it) and writes its own to pool row own[row]; the selection (beam.hip) hands out rows so that nothing read in a round is written
// in it.  Same tile body, contraction ranges and row definitions as the greedy loop: the numbers of a slot depend on its token
// sequence alone.  Every kernel returns at once where nothing needs a step.
// ---------------------------------------------------------------------------------------
// the slot (u, s) of this workgroup (grid (16, n_utt)) if it awaits its step: its search's current buffer, else -1
__device__ __forceinline__ int bl_slot_cur(const BeamLstmStep &a, int u, int s)
{
    const int32_t *st = a.state + 32 * u;
    if (st[BEAM_ST_DONE] || !st[BEAM_ST_NEW]) return -1;
    const int cur = st[BEAM_ST_CUR] & 1;
    return beam_utt(a.need, u * a.stride)[cur * 16 + s] ? cur : -1;
}
__device__ __forceinline__ long bl_pool_row(const BeamLstmStep &a, const int *idx, int row)
{
    return (long)min(max(idx[row], 0), 32 * a.n_utt - 1) * a.L * 2 * a.Hd;
}

__global__ __launch_bounds__(256) void k_bl_embed(BeamLstmStep a, float *__restrict__ x1)
{
    __shared__ float red[4];
    const int s = blockIdx.x, u = blockIdx.y;
    const int cur = bl_slot_cur(a, u, s);
    if (cur < 0) return;
    const int len = min(max(beam_utt(a.len, u * a.stride)[cur * 16 + s], 0), a.max_length - 1);
    const int tok = beam_utt(a.tok, u * a.stride)[((long)cur * 16 + s) * a.max_length + len];  // the newest token (the start blank at len 0)
    ld_embed_row(a.p.embedding, a.S, tok, a.p.ln_in_w, a.p.ln_in_b, a.eps_in, a.E, x1 + (long)(16 * u + s) * a.E, red);
}

// k_ld_gemm with the row tile as grid.z: a tile none of whose two utterances awaits a step is skipped
struct BlGemm { const int32_t *state; int n_utt; RecArgs g[2]; };
__global__ __launch_bounds__(256) void k_bl_gemm(BlGemm a)
{
    __shared__ float red[3 * 1024];
    bool any = false;
    for (int u = 2 * blockIdx.z; u < min(2 * (int)blockIdx.z + 2, a.n_utt); ++u)
        any |= !a.state[32 * u + BEAM_ST_DONE] && a.state[32 * u + BEAM_ST_NEW];
    if (!any) return;
    const int which = (int)blockIdx.y >= a.g[0].KS ? 1 : 0;
    rec_tile<false>(a.g[which], blockIdx.x * 32, blockIdx.y - (which ? a.g[0].KS : 0), blockIdx.z * 32, red);
}

template <bool LN>
__global__ __launch_bounds__(256) void k_bl_step(BeamLstmStep a, LdStep q, int layer)
{
    __shared__ float red[4];
    const int s = blockIdx.x, u = blockIdx.y, row = 16 * u + s;
    if (bl_slot_cur(a, u, s) < 0) return;
    const long at = (long)(2 * layer) * a.Hd;
    float *mine = a.pool + bl_pool_row(a, a.own, row) + at;
    ld_step_row<LN>(q, q.gp + (long)row * 4 * a.Hd, a.pool + bl_pool_row(a, a.par, row) + at + a.Hd, mine, mine + a.Hd, nullptr, nullptr, red);
}

// to_pvec: the row is the slot's text vector (N == H), else row 16 u + s of `out`
template <bool LN>
__global__ __launch_bounds__(256) void k_bl_rowfin(BeamLstmStep a, const float *__restrict__ gp, int nsp, long gp_ld, int N,
                                                   const float *__restrict__ bias, const float *__restrict__ gamma,
                                                   const float *__restrict__ beta, float eps, float *__restrict__ out, int to_pvec)
{
    __shared__ float red[4];
    const int s = blockIdx.x, u = blockIdx.y, row = 16 * u + s;
    const int cur = bl_slot_cur(a, u, s);
    if (cur < 0) return;
    float *y = to_pvec ? beam_utt(a.pvec, u * a.stride) + ((long)cur * 16 + s) * N : out + (long)row * N;
    ld_rowfin_row<LN>(gp + (long)row * N, nsp, gp_ld, N, bias, gamma, beta, eps, y, red);
}

int ld_check_sizes(int n_utt, int S, int E, int Hd, int O, int L, int ln, int H, int V, int has_text, int scan_frames)
{
    if (n_utt < 1) return engine_fail(RNNT_ERR_INVALID_ARG, "n_utt=%d must be >= 1", n_utt);
    if (H <= 0 || V <= 0) return engine_fail(RNNT_ERR_INVALID_ARG, "non-positive dimension H=%d V=%d", H, V);
    const Dims d = {n_utt, 1, S, E, Hd, O, L, ln};
    if (int rc = check_dims(d)) return rc;
    if (n_utt > 32) return engine_fail(RNNT_ERR_UNSUPPORTED, "the LSTM decode entries take 1 <= n_utt <= 32 (n_utt=%d)", n_utt);
    if (H % 8 != 0 || V % 4 != 0) return engine_fail(RNNT_ERR_UNSUPPORTED, "the LSTM decode entries need H %% 8 == 0 and V %% 4 == 0 (H=%d V=%d)", H, V);
    if (scan_frames < 1 || scan_frames > 128)
        return engine_fail(RNNT_ERR_UNSUPPORTED, "the LSTM greedy decode takes scan_frames in [1,128] (scan_frames=%d)", scan_frames);
    if (!has_text && O != H) return engine_fail(RNNT_ERR_INVALID_ARG, "without text_ln the predictor's output dim (%d) must equal H (%d)", O, H);
    return RNNT_OK;
}

}  // namespace

// a beam round's predictor step: one row per slot, its state in the search's pool
static StepLayout bl_layout(int n_utt, int E, int Hd, int O, int H) { return step_layout(16 * n_utt, E, Hd, O, 0, H, 0, 0, false); }

size_t beam_lstm_step_floats(int n_utt, int E, int Hd, int O, int H) { return bl_layout(n_utt, E, Hd, O, H).total; }

void launch_beam_lstm_step(const BeamLstmStep &a, hipStream_t st)
{
    const int n = a.n_utt, M = 16 * n, E = a.E, Hd = a.Hd, O = a.O, L = a.L, H = a.H;
    const StepLayout w = bl_layout(n, E, Hd, O, H);
    float *x1 = a.scratch + w.x1, *y = a.scratch + w.y, *gp = a.scratch + w.gp;
    const long ld = (long)L * 2 * Hd;  // floats from one pool row to the next
    const dim3 slots(16, n), tiles_z((M + 31) / 32);
    auto pooled = [&](int at, const int *idx, const float *W, float *P, int N) {  // operand rows read from the pool through `idx`
        RecArgs g = RecArgs{a.pool + (long)at * Hd, ld, W, (long)Hd, P, M, N, Hd, rec_splits(Hd)};
        g.rows = idx; g.R = 32 * n;
        return g;
    };
    hipLaunchKernelGGL(k_bl_embed, slots, dim3(256), 0, st, a, x1);
    for (int l = 0; l < L; ++l) {
        const rnnt_lstm_layer_params &q = a.p.layers[l];
        BlGemm g;
        g.state = a.state; g.n_utt = n;
        // the layer below's NEW h (the slot's own row: its row kernel has run), and this layer's h of the state the slot continues
        g.g[0] = l ? pooled(2 * (l - 1), a.own, q.x2g_w, gp, 4 * Hd) : ld_prod(x1, q.x2g_w, gp, M, 4 * Hd, E);
        g.g[1] = pooled(2 * l, a.par, q.p2g_w, gp + (long)g.g[0].KS * M * 4 * Hd, 4 * Hd);
        hipLaunchKernelGGL(k_bl_gemm, dim3((4 * Hd + 31) / 32, g.g[0].KS + g.g[1].KS, tiles_z.x), dim3(256), 0, st, g);
        LdStep s;
        s.states = nullptr; s.st_ld = 0; s.gp = gp; s.nsp = g.g[0].KS + g.g[1].KS; s.gp_ld = (long)M * 4 * Hd;
        s.xb = a.ln ? nullptr : q.x2g_b;
        s.gw = q.g_norm_w; s.gb = q.g_norm_b; s.cw = q.c_norm_w; s.cb = q.c_norm_b; s.eps = a.eps_lstm;
        s.h = s.c = s.h_out = s.c_out = nullptr;
        s.Hd = Hd;
        if (a.ln) hipLaunchKernelGGL(k_bl_step<true>, slots, dim3(256), 0, st, a, s, l);
        else hipLaunchKernelGGL(k_bl_step<false>, slots, dim3(256), 0, st, a, s, l);
    }
    BlGemm g;
    g.state = a.state; g.n_utt = n;
    g.g[0] = pooled(2 * (L - 1), a.own, a.p.linear_w, gp, O);
    g.g[1] = g.g[0]; g.g[1].KS = 0;
    hipLaunchKernelGGL(k_bl_gemm, dim3((O + 31) / 32, g.g[0].KS, tiles_z.x), dim3(256), 0, st, g);
    // without joint.text_ln the output LayerNorm's row IS the text vector (O == H)
    hipLaunchKernelGGL(k_bl_rowfin<true>, slots, dim3(256), 0, st, a, gp, g.g[0].KS, (long)M * O, O, a.p.linear_b, a.p.ln_out_w, a.p.ln_out_b,
                       a.eps_out, y, a.text_W ? 0 : 1);
    if (a.text_W) {
        g.g[0] = ld_prod(y, a.text_W, gp, M, H, O);
        g.g[1] = g.g[0]; g.g[1].KS = 0;
        hipLaunchKernelGGL(k_bl_gemm, dim3((H + 31) / 32, g.g[0].KS, tiles_z.x), dim3(256), 0, st, g);
        hipLaunchKernelGGL(k_bl_rowfin<false>, slots, dim3(256), 0, st, a, gp, g.g[0].KS, (long)M * H, H, a.text_b, (const float *)nullptr,
                           (const float *)nullptr, 0.f, y, 1);
    }
}

// the device's address of a caller's pinned flag word (an ordinary host pointer is refused, never written through); NULL stays NULL
static int ld_host_flag(int32_t *host_flag, int32_t **dev)
{
    *dev = nullptr;
    if (!host_flag) return RNNT_OK;
    void *dp = nullptr;
    if (hipHostGetDevicePointer(&dp, host_flag, 0) != hipSuccess || !dp) {
        (void)hipGetLastError();
        return engine_fail(RNNT_ERR_INVALID_ARG, "host_flag is not mapped pinned host memory (hipHostMalloc / torch pin_memory)");
    }
    *dev = (int32_t *)dp;
    return RNNT_OK;
}

// What the three decode entries (greedy, stream push, beam) check alike, in two halves so that an entry's own geometry, blank and limit
// checks stand between them and every error is reported in the order it always was.  `need`: the workspace size the entry's query asks
// for (the query has checked the dimensions).
struct DecodeCall {
    const void *frames; const rnnt_lstm_predictor_params *p; int L, ln; const void *text_W, *text_b, *W, *bias;
    int iterations; int32_t *host_flag; void *workspace; size_t ws_bytes, need;
};
// own_null / own_misaligned: one of the entry's own pointers is null / off the alignment `rule` names
static int ld_check_pointers(const DecodeCall &c, bool own_null, bool own_misaligned, const char *rule)
{
    if (c.iterations < 0) return engine_fail(RNNT_ERR_INVALID_ARG, "iterations=%d", c.iterations);
    if (bad(c.frames) || bad(c.W) || bad(c.bias) || !c.workspace || own_null)
        return engine_fail(RNNT_ERR_INVALID_ARG, "null or not 16-byte aligned pointer argument");
    if (((uintptr_t)c.workspace & 255) || own_misaligned) return engine_fail(RNNT_ERR_INVALID_ARG, "%s", rule);
    if (int rc = check_params(c.p, c.L, c.ln, "parameter")) return rc;
    if ((c.text_W == nullptr) != (c.text_b == nullptr) || (c.text_W && (bad(c.text_W) || bad(c.text_b))))
        return engine_fail(RNNT_ERR_INVALID_ARG, "text_W / text_b: both or neither, 16-byte aligned");
    return RNNT_OK;
}
static int ld_check_flag_and_size(const DecodeCall &c, int32_t **flag_dev)
{
    if (int rc = ld_host_flag(c.host_flag, flag_dev)) return rc;
    if (c.ws_bytes < c.need) return engine_fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", c.ws_bytes, c.need);
    return RNNT_OK;
}
static bool bad_stride(int64_t frame_stride, int H) { return frame_stride < H || frame_stride % 4; }
static int check_blank(int blank, int V)
{
    return blank < 0 || blank >= V ? engine_fail(RNNT_ERR_INVALID_ARG, "blank=%d outside [0,%d)", blank, V) : RNNT_OK;
}

// the model's part of a decode's arguments (checked by the caller): of a greedy loop's LdArgs or a beam search's BeamLstmStep
template <class Model>
static void ld_model(Model &a, const rnnt_lstm_predictor_params *p, int S, int E, int Hd, int O, int L, int layer_norm, float eps_in,
                     float eps_lstm, float eps_out, const void *text_W, const void *text_b, int H)
{
    a.p = *p; a.S = S; a.E = E; a.Hd = Hd; a.O = O; a.L = L; a.ln = layer_norm != 0;
    a.eps_in = eps_in; a.eps_lstm = eps_lstm; a.eps_out = eps_out;
    a.text_W = (const float *)text_W; a.text_b = (const float *)text_b; a.H = H;
}

extern "C" {

int rnnt_engine_lstm_predictor_saved_bytes(int B, int U1, int S, int E, int Hd, int O, int L, int layer_norm, size_t *out)
{
    if (!out) return engine_fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    const Dims d = {B, U1, S, E, Hd, O, L, layer_norm != 0};
    if (int rc = check_dims(d)) return rc;
    *out = saved_layout(d).total * 4;
    return RNNT_OK;
}

int rnnt_engine_lstm_predictor_workspace_bytes(int B, int U1, int S, int E, int Hd, int O, int L, int layer_norm, int backward,
                                               size_t *out)
{
    if (!out) return engine_fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    const Dims d = {B, U1, S, E, Hd, O, L, layer_norm != 0};
    if (int rc = check_dims(d)) return rc;
    *out = (backward ? bwd_layout(d).total : fwd_layout(d).total) * 4;
    return RNNT_OK;
}

int rnnt_engine_lstm_predictor_fwd(const int64_t *ids, int B, int U1, int S, int E, int Hd, int O, int L, int layer_norm,
                                   const rnnt_lstm_predictor_params *p, const float *state_in, const uint8_t *keep,
                                   float dropout_p, float eps_in, float eps_lstm, float eps_out, float *out, float *state_out,
                                   void *saved, size_t saved_bytes, void *ws, size_t ws_bytes, void *stream)
{
    const Dims d = {B, U1, S, E, Hd, O, L, layer_norm != 0};
    if (int rc = check_dims(d)) return rc;
    if (!ids || bad(out) || bad(state_out) || bad(ws)) return engine_fail(RNNT_ERR_INVALID_ARG, "null or not 16-byte aligned pointer argument");
    if ((state_in && ((uintptr_t)state_in & 15)) || (saved && ((uintptr_t)saved & 15)))
        return engine_fail(RNNT_ERR_INVALID_ARG, "state_in / saved not 16-byte aligned");
    if (int rc = check_params(p, L, d.ln, "parameter")) return rc;
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return engine_fail(RNNT_ERR_INVALID_ARG, "dropout_p outside [0,1)");
    const SavedLayout SL = saved_layout(d);
    const FwdLayout FL = fwd_layout(d);
    if (saved && saved_bytes < SL.total * 4)
        return engine_fail(RNNT_ERR_WORKSPACE, "saved buffer %zu < required %zu bytes", saved_bytes, SL.total * 4);
    if (ws_bytes < FL.total * 4) return engine_fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, FL.total * 4);
    hipStream_t st = (hipStream_t)stream;
    float *w = (float *)ws, *sv = (float *)saved;
    const int M = B * U1;
    const long seq = (long)U1 * Hd, BH = (long)B * Hd;
    const float scale = 1.f / (1.f - dropout_p);
    const bool train = saved != nullptr;
    if (dropout_p == 0.f) keep = nullptr;

    float *x1 = train ? sv + SL.x1 : w + FL.x1;
    launch_ln_fwd(p->embedding, ids, S, p->ln_in_w, p->ln_in_b, eps_in, M, E, x1, train ? sv + SL.st1 : w + FL.st1, st);
    const float *x = x1;
    int in = E;
    for (int l = 0; l < L; ++l) {
        const rnnt_lstm_layer_params &y = p->layers[l];
        SgArgs gx = sg(x, in, y.x2g_w, in, w + FL.xg, 4 * Hd, M, 4 * Hd, in);
        gx.bias = d.ln ? nullptr : y.x2g_b;
        launch_sgemm_nt(gx, st);
        const float *h0 = state_in ? state_in + (long)(2 * l) * BH : nullptr, *c0 = state_in ? h0 + BH : nullptr;
        float *hout = state_out + (long)(2 * l) * BH, *cout = hout + BH;
        float *yl = train ? sv + SL.y[l] : w + ((l & 1) ? FL.yb : FL.ya);
        if (train)
            hipLaunchKernelGGL(k_lstm_init, dim3(B), dim3(256), 0, st, h0, c0, Hd, seq, sv + SL.hp[l], sv + SL.cp[l]);
        for (int t = 0; t < U1; ++t) {
            StepF a;
            const float *hprev; long hprev_ld;
            if (train) {
                hprev = sv + SL.hp[l] + (long)t * Hd; hprev_ld = seq;
                a.cprev = sv + SL.cp[l] + (long)t * Hd; a.cprev_ld = seq;
            } else if (t == 0) {
                hprev = h0; hprev_ld = Hd;
                a.cprev = c0; a.cprev_ld = Hd;
            } else {
                hprev = w + FL.hb + (t & 1) * BH; hprev_ld = Hd;
                a.cprev = w + FL.cb + (t & 1) * BH; a.cprev_ld = Hd;
            }
            const bool rec = t > 0 || state_in;  // h_{t-1} = 0: no recurrent product
            if (rec) launch_rec_gemm<false>(hprev, hprev_ld, y.p2g_w, Hd, w + FL.rg, B, 4 * Hd, Hd, st);
            a.xg = w + FL.xg + (long)t * 4 * Hd; a.xg_ld = 4 * seq;
            a.rg = rec ? w + FL.rg : nullptr; a.rg_n = rec_splits(Hd); a.rg_ld = 4 * BH;
            a.gw = y.g_norm_w; a.gb = y.g_norm_b; a.cw = y.c_norm_w; a.cb = y.c_norm_b;
            a.eps = eps_lstm;
            if (t + 1 == U1) {
                a.hnext = hout; a.cnext = cout; a.hnext_ld = a.cnext_ld = Hd;
            } else if (train) {
                a.hnext = sv + SL.hp[l] + (long)(t + 1) * Hd; a.cnext = sv + SL.cp[l] + (long)(t + 1) * Hd;
                a.hnext_ld = a.cnext_ld = seq;
            } else {
                a.hnext = w + FL.hb + ((t + 1) & 1) * BH; a.cnext = w + FL.cb + ((t + 1) & 1) * BH;
                a.hnext_ld = a.cnext_ld = Hd;
            }
            a.y = yl + (long)t * Hd; a.y_ld = seq;
            a.keep = keep ? keep + (long)l * M * Hd + (long)t * Hd : nullptr; a.keep_ld = seq; a.scale = scale;
            a.ghat = train ? sv + SL.ghat[l] + (long)t * 4 * Hd : nullptr; a.ghat_ld = 4 * seq;
            a.chat = train ? sv + SL.chat[l] + (long)t * Hd : nullptr; a.chat_ld = seq;
            a.rs = train ? sv + SL.rs[l] + 2 * t : nullptr; a.rs_ld = 2 * (long)U1;
            a.Hd = Hd;
            if (d.ln) hipLaunchKernelGGL(k_lstm_step_fwd<true>, dim3(B), dim3(256), 0, st, a);
            else hipLaunchKernelGGL(k_lstm_step_fwd<false>, dim3(B), dim3(256), 0, st, a);
        }
        x = yl;
        in = Hd;
    }
    float *z = train ? sv + SL.z : w + FL.z;
    SgArgs lin = sg(x, Hd, p->linear_w, Hd, z, O, M, O, Hd);
    lin.bias = p->linear_b;
    launch_sgemm_nt(lin, st);
    launch_ln_fwd(z, nullptr, 0, p->ln_out_w, p->ln_out_b, eps_out, M, O, out, train ? sv + SL.st2 : w + FL.st2, st);
    return status("rnnt_engine_lstm_predictor_fwd");
}

int rnnt_engine_lstm_predictor_bwd(const int64_t *ids, int B, int U1, int S, int E, int Hd, int O, int L, int layer_norm,
                                   const rnnt_lstm_predictor_params *p, const uint8_t *keep, float dropout_p, float eps_in,
                                   float eps_lstm, float eps_out, const float *d_out, const rnnt_lstm_predictor_params *g,
                                   const void *saved, size_t saved_bytes, void *ws, size_t ws_bytes, void *stream)
{
    (void)eps_in; (void)eps_lstm; (void)eps_out;  // the forward kept every rstd
    const Dims d = {B, U1, S, E, Hd, O, L, layer_norm != 0};
    if (int rc = check_dims(d)) return rc;
    if (!ids || bad(d_out) || bad(saved) || bad(ws)) return engine_fail(RNNT_ERR_INVALID_ARG, "null or not 16-byte aligned pointer argument");
    if (int rc = check_params(p, L, d.ln, "parameter")) return rc;
    if (int rc = check_params(g, L, d.ln, "gradient")) return rc;
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return engine_fail(RNNT_ERR_INVALID_ARG, "dropout_p outside [0,1)");
    const SavedLayout SL = saved_layout(d);
    const BwdLayout BL = bwd_layout(d);
    if (saved_bytes < SL.total * 4) return engine_fail(RNNT_ERR_WORKSPACE, "saved buffer %zu < required %zu bytes", saved_bytes, SL.total * 4);
    if (ws_bytes < BL.total * 4) return engine_fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, BL.total * 4);
    hipStream_t st = (hipStream_t)stream;
    float *w = (float *)ws;
    const float *sv = (const float *)saved;
    const int M = B * U1;
    const long seq = (long)U1 * Hd;
    const float scale = 1.f / (1.f - dropout_p);
    if (dropout_p == 0.f) keep = nullptr;
    float *cs = w + BL.cs, *dy = w + BL.dy, *draw = w + BL.draw;

    // weight gradient dW [N,K] = Y^T X over the M rows: split-K slabs, summed in order; db = colsum(Y) where asked for
    auto wgrad = [&](const float *Y, int N, const float *X, int K, float *dW, float *db) {
        SgArgs a = sg(Y, N, X, K, w + BL.slabs, K, M, N, K);
        a.ksplit = sgemm_tn_splits_for(M, N, K, 1);
        launch_sgemm_tn(a, st);
        if (db) launch_colsum_stage1(Y, N, M, N, cs, st);
        launch_wgrad_finish(w + BL.slabs, a.ksplit, dW, N, K, 1, cs, colsum_slabs(M), N, db, st);
    };

    // output LayerNorm and linear
    launch_ln_bwd(sv + SL.z, nullptr, 0, p->ln_out_w, sv + SL.st2, d_out, M, O, w + BL.dz, w + BL.t, st);
    launch_colsum_pair(w + BL.t, d_out, O, M, O, (float *)g->ln_out_w, (float *)g->ln_out_b, cs, st);
    wgrad(w + BL.dz, O, sv + SL.y[L - 1], Hd, (float *)g->linear_w, (float *)g->linear_b);
    launch_sgemm_nn(sg(w + BL.dz, O, p->linear_w, Hd, dy, Hd, M, Hd, O), st);

    for (int l = L - 1; l >= 0; --l) {
        const rnnt_lstm_layer_params &y = p->layers[l], &gy = g->layers[l];
        const int in = l ? Hd : E;
        const float *x = l ? sv + SL.y[l - 1] : sv + SL.x1;
        for (int t = U1 - 1; t >= 0; --t) {
            StepB a;
            a.dy = dy + (long)t * Hd; a.dy_ld = seq;
            a.keep = keep ? keep + (long)l * M * Hd + (long)t * Hd : nullptr; a.keep_ld = seq; a.scale = scale;
            a.dhrec = t + 1 < U1 ? w + BL.dhrec : nullptr; a.dh_n = rec_splits(4 * Hd); a.dh_ld = (long)B * Hd;
            a.dc = w + BL.dc; a.dc_valid = t + 1 < U1;
            a.ghat = sv + SL.ghat[l] + (long)t * 4 * Hd; a.ghat_ld = 4 * seq;
            a.chat = sv + SL.chat[l] + (long)t * Hd; a.chat_ld = seq;
            a.rs = sv + SL.rs[l] + 2 * t; a.rs_ld = 2 * (long)U1;
            a.cprev = sv + SL.cp[l] + (long)t * Hd; a.cprev_ld = seq;
            a.gw = y.g_norm_w; a.gb = y.g_norm_b; a.cw = y.c_norm_w; a.cb = y.c_norm_b;
            a.dpre = w + BL.dpre + (long)t * 4 * Hd; a.tg = w + BL.tg + (long)t * 4 * Hd; a.draw = draw + (long)t * 4 * Hd;
            a.g_ld = 4 * seq;
            a.dcn = w + BL.dcn + (long)t * Hd; a.tc = w + BL.tc + (long)t * Hd; a.c_ld = seq;
            a.Hd = Hd;
            if (d.ln) hipLaunchKernelGGL(k_lstm_step_bwd<true>, dim3(B), dim3(256), 0, st, a);
            else hipLaunchKernelGGL(k_lstm_step_bwd<false>, dim3(B), dim3(256), 0, st, a);
            // recurrent part of dh_{t-1} = dgates_t p2g (nothing flows into the initial state)
            if (t > 0) launch_rec_gemm<true>(draw + (long)t * 4 * Hd, 4 * seq, y.p2g_w, Hd, w + BL.dhrec, B, Hd, 4 * Hd, st);
        }
        // d p2g = sum_t dgates_t^T h_{t-1} (row (b,0) of the kept h_{t-1} sequence is the initial state), d x2g (+ bias), the affines
        wgrad(draw, 4 * Hd, sv + SL.hp[l], Hd, (float *)gy.p2g_w, nullptr);
        wgrad(draw, 4 * Hd, x, in, (float *)gy.x2g_w, d.ln ? nullptr : (float *)gy.x2g_b);
        if (d.ln) {
            launch_colsum_pair(w + BL.tg, w + BL.dpre, 4 * Hd, M, 4 * Hd, (float *)gy.g_norm_w, (float *)gy.g_norm_b, cs, st);
            launch_colsum_pair(w + BL.tc, w + BL.dcn, Hd, M, Hd, (float *)gy.c_norm_w, (float *)gy.c_norm_b, cs, st);
        }
        // dx: the gradient of the layer below's output, or of the input LayerNorm's
        launch_sgemm_nn(sg(draw, 4 * Hd, y.x2g_w, in, dy, in, M, in, 4 * Hd), st);
    }
    // input LayerNorm (its input is the embedding row) and the embedding table
    launch_ln_bwd(p->embedding, ids, S, p->ln_in_w, sv + SL.st1, dy, M, E, w + BL.dz, w + BL.t, st);
    launch_colsum_pair(w + BL.t, dy, E, M, E, (float *)g->ln_in_w, (float *)g->ln_in_b, cs, st);
    launch_embed_bwd(ids, w + BL.dz, M, E, S, (float *)g->embedding, st);
    return status("rnnt_engine_lstm_predictor_bwd");
}

int rnnt_engine_greedy_decode_lstm_workspace_bytes(int n_utt, int S, int E, int Hd, int O, int L, int layer_norm, int H, int V, int has_text,
                                                   int scan_frames, size_t *out)
{
    if (!out) return engine_fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    if (int rc = ld_check_sizes(n_utt, S, E, Hd, O, L, layer_norm != 0, H, V, has_text, scan_frames)) return rc;
    *out = (step_layout(n_utt, E, Hd, O, L, H, V, scan_frames, true).total * 4 + 255) & ~(size_t)255;
    return RNNT_OK;
}

int rnnt_engine_greedy_decode_lstm(const void *frames, int64_t frame_stride, int rows, const int32_t *utt, int n_utt, int max_frames,
                                   const rnnt_lstm_predictor_params *p, int S, int E, int Hd, int O, int L, int layer_norm, float eps_in,
                                   float eps_lstm, float eps_out, const void *text_W, const void *text_b, const void *W, const void *bias,
                                   int H, int V, int blank, int max_length, int max_per_frame, int scan_frames, int iterations, int init,
                                   int32_t *host_flag, int32_t *state, int32_t *tokens, float *state_out, void *workspace, size_t ws_bytes,
                                   void *stream)
{
    size_t need;
    if (int rc = rnnt_engine_greedy_decode_lstm_workspace_bytes(n_utt, S, E, Hd, O, L, layer_norm, H, V, text_W ? 1 : 0, scan_frames, &need))
        return rc;
    const DecodeCall c{frames, p, L, layer_norm != 0, text_W, text_b, W, bias, iterations, host_flag, workspace, ws_bytes, need};
    int32_t *flag_dev;
    if (int rc = ld_check_pointers(c, !utt || !state || !tokens, ((uintptr_t)utt & 7) || (state_out && ((uintptr_t)state_out & 15)),
                                   "utt must be 8-byte, state_out 16-byte and the workspace 256-byte aligned"))
        return rc;
    if (max_length < 2 || max_per_frame < 1 || max_frames < 1 || rows < max_frames || bad_stride(frame_stride, H))
        return engine_fail(RNNT_ERR_INVALID_ARG, "max_length=%d max_per_frame=%d max_frames=%d rows=%d frame_stride=%lld", max_length,
                           max_per_frame, max_frames, rows, (long long)frame_stride);
    if (int rc = check_blank(blank, V)) return rc;
    if ((long)n_utt * max_length > 0x7fffffffL) return engine_fail(RNNT_ERR_UNSUPPORTED, "n_utt * max_length must stay below 2^31");
    if (int rc = ld_check_flag_and_size(c, &flag_dev)) return rc;
    LdArgs a;
    a.frames = (const float *)frames; a.frame_stride = (long)frame_stride; a.rows = rows; a.utt = utt; a.n_utt = n_utt;
    ld_model(a, p, S, E, Hd, O, L, layer_norm, eps_in, eps_lstm, eps_out, text_W, text_b, H);
    a.W = (const float *)W; a.bias = (const float *)bias; a.V = V; a.blank = blank; a.max_length = max_length; a.max_per_frame = max_per_frame;
    a.scan_frames = scan_frames;
    a.iterations = iterations ? iterations : max_length + (max_frames + scan_frames - 1) / scan_frames + 1;
    a.init = init;
    a.host_flag = flag_dev; a.state = state; a.tokens = tokens; a.state_out = state_out;
    const StepLayout w = step_layout(n_utt, E, Hd, O, L, H, V, scan_frames, true);
    float *ws = (float *)workspace;
    a.text = ws + w.text; a.x1 = ws + w.x1; a.hc = ws + w.hc; a.y = ws + w.y; a.gp = ws + w.gp;
    a.part = (float2 *)(ws + w.part); a.ctrl = (int32_t *)(ws + w.ctrl);
    launch_ld_loop(a, (hipStream_t)stream);
    return status("rnnt_engine_greedy_decode_lstm");
}

int rnnt_engine_greedy_stream_lstm_bytes(int n_streams, int S, int E, int Hd, int O, int L, int layer_norm, int H, int V, int has_text,
                                         size_t *out)
{
    if (!out) return engine_fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    if (int rc = ld_check_sizes(n_streams, S, E, Hd, O, L, layer_norm != 0, H, V, has_text, 1)) return rc;
    *out = ls_block(n_streams, Hd, L, H).total * 4;
    return RNNT_OK;
}

int rnnt_engine_greedy_stream_lstm_init(int n_streams, int Hd, int L, int H, int blank, int index, void *block, size_t bytes, void *stream)
{
    if (n_streams < 1 || Hd < 1 || L < 1 || H < 1 || blank < 0)
        return engine_fail(RNNT_ERR_INVALID_ARG, "n_streams=%d Hd=%d L=%d H=%d blank=%d", n_streams, Hd, L, H, blank);
    if (n_streams > 32 || Hd > 1024 || L > 8)
        return engine_fail(RNNT_ERR_UNSUPPORTED, "the LSTM stream takes n_streams <= 32, Hd <= 1024, L <= 8 (n_streams=%d Hd=%d L=%d)", n_streams, Hd, L);
    if (index < -1 || index >= n_streams) return engine_fail(RNNT_ERR_INVALID_ARG, "index=%d outside [-1,%d)", index, n_streams);
    if (!block || ((uintptr_t)block & 255)) return engine_fail(RNNT_ERR_INVALID_ARG, "the block must be non-null and 256-byte aligned");
    const LsBlock b = ls_block(n_streams, Hd, L, H);
    if (bytes < b.total * 4) return engine_fail(RNNT_ERR_WORKSPACE, "block %zu < required %zu bytes", bytes, b.total * 4);
    float *f = (float *)block;
    const int widest = std::max(std::max(2 * L * Hd, H), (int)LS_WORDS);
    hipLaunchKernelGGL(k_ls_init, dim3((widest + 255) / 256, index < 0 ? n_streams : 1), dim3(256), 0, (hipStream_t)stream,
                       (int32_t *)(f + b.state), f + b.hc, f + b.text, n_streams, Hd, L, H, blank, index);
    return status("rnnt_engine_greedy_stream_lstm_init");
}

int rnnt_engine_greedy_stream_lstm_push_workspace_bytes(int n_streams, int S, int E, int Hd, int O, int L, int layer_norm, int H, int V,
                                                        int has_text, int scan_frames, size_t *out)
{
    if (!out) return engine_fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    if (int rc = ld_check_sizes(n_streams, S, E, Hd, O, L, layer_norm != 0, H, V, has_text, scan_frames)) return rc;
    *out = (step_layout(n_streams, E, Hd, O, L, H, V, scan_frames, false).total * 4 + 255) & ~(size_t)255;
    return RNNT_OK;
}

int rnnt_engine_greedy_stream_lstm_push(const void *frames, int64_t frame_stride, int rows, const int32_t *push_table, int n_streams,
                                        int max_count, const rnnt_lstm_predictor_params *p, int S, int E, int Hd, int O, int L,
                                        int layer_norm, float eps_in, float eps_lstm, float eps_out, const void *text_W,
                                        const void *text_b, const void *W, const void *bias, int H, int V, int blank, int max_length,
                                        int max_per_frame, int scan_frames, int iterations, int begin, int32_t *host_flag,
                                        int32_t *out_tokens, int out_stride, void *block, size_t bytes, void *workspace, size_t ws_bytes,
                                        void *stream)
{
    size_t need, need_block;
    if (int rc = rnnt_engine_greedy_stream_lstm_push_workspace_bytes(n_streams, S, E, Hd, O, L, layer_norm, H, V, text_W ? 1 : 0, scan_frames,
                                                                     &need))
        return rc;
    if (int rc = rnnt_engine_greedy_stream_lstm_bytes(n_streams, S, E, Hd, O, L, layer_norm, H, V, text_W ? 1 : 0, &need_block)) return rc;
    const DecodeCall c{frames, p, L, layer_norm != 0, text_W, text_b, W, bias, iterations, host_flag, workspace, ws_bytes, need};
    int32_t *flag_dev;
    if (int rc = ld_check_pointers(c, !push_table || !out_tokens || !block,
                                   ((uintptr_t)push_table & 7) || ((uintptr_t)out_tokens & 3) || ((uintptr_t)block & 255),
                                   "push_table must be 8-byte, out_tokens 4-byte, the workspace and the block 256-byte aligned"))
        return rc;
    if ((max_length != 0 && max_length < 2) || max_per_frame < 1 || max_count < 0 || rows < 1 || rows < max_count || bad_stride(frame_stride, H))
        return engine_fail(RNNT_ERR_INVALID_ARG, "max_length=%d (0 or >= 2) max_per_frame=%d max_count=%d rows=%d frame_stride=%lld", max_length,
                           max_per_frame, max_count, rows, (long long)frame_stride);
    if (int rc = check_blank(blank, V)) return rc;
    const long most = (long)max_count * max_per_frame;  // labels a stream can emit in this push
    if (out_stride < 1 || out_stride < most)
        return engine_fail(RNNT_ERR_INVALID_ARG, "out_stride=%d below max_count * max_per_frame = %ld (and 1)", out_stride, most);
    const long bound = most + (max_count + scan_frames - 1) / scan_frames + 1;
    if (bound > 0x7fffffffL || (long)n_streams * out_stride > 0x7fffffffL)
        return engine_fail(RNNT_ERR_UNSUPPORTED, "max_count * max_per_frame and n_streams * out_stride must stay below 2^31");
    if (int rc = ld_check_flag_and_size(c, &flag_dev)) return rc;
    if (bytes < need_block) return engine_fail(RNNT_ERR_WORKSPACE, "block %zu < required %zu bytes", bytes, need_block);
    LdArgs a;
    a.frames = (const float *)frames; a.frame_stride = (long)frame_stride; a.rows = rows; a.utt = push_table; a.n_utt = n_streams;
    ld_model(a, p, S, E, Hd, O, L, layer_norm, eps_in, eps_lstm, eps_out, text_W, text_b, H);
    a.W = (const float *)W; a.bias = (const float *)bias; a.V = V; a.blank = blank; a.max_length = max_length; a.max_per_frame = max_per_frame;
    a.scan_frames = scan_frames;
    a.iterations = iterations ? iterations : (int)bound;
    a.init = begin;
    a.stream = 1; a.tokens = out_tokens; a.tok_ld = out_stride;
    a.host_flag = flag_dev; a.state_out = nullptr;
    const LsBlock b = ls_block(n_streams, Hd, L, H);
    const StepLayout w = step_layout(n_streams, E, Hd, O, L, H, V, scan_frames, false);
    float *bl = (float *)block, *ws = (float *)workspace;
    a.state = (int32_t *)(bl + b.state); a.hc = bl + b.hc; a.text = bl + b.text;
    a.x1 = ws + w.x1; a.y = ws + w.y; a.gp = ws + w.gp; a.part = (float2 *)(ws + w.part); a.ctrl = (int32_t *)(ws + w.ctrl);
    launch_ld_loop(a, (hipStream_t)stream);
    return status("rnnt_engine_greedy_stream_lstm_push");
}

int rnnt_engine_beam_decode_lstm_workspace_bytes(int n_utt, int S, int E, int Hd, int O, int L, int layer_norm, int H, int V, int has_text,
                                                 int max_length, int beam, size_t *out)
{
    if (!out) return engine_fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    if (beam < 1) return engine_fail(RNNT_ERR_INVALID_ARG, "beam=%d must be >= 1", beam);
    if (beam > 16) return engine_fail(RNNT_ERR_UNSUPPORTED, "beam decode takes beam <= 16 (beam=%d)", beam);
    if (max_length < 2) return engine_fail(RNNT_ERR_INVALID_ARG, "max_length=%d must be >= 2", max_length);
    if (max_length > 65536) return engine_fail(RNNT_ERR_UNSUPPORTED, "beam decode takes max_length <= 65536 (max_length=%d)", max_length);
    if (int rc = ld_check_sizes(n_utt, S, E, Hd, O, L, layer_norm != 0, H, V, has_text, 1)) return rc;
    *out = beam_lstm_workspace_bytes(n_utt, E, Hd, O, L, H, V, max_length);
    return RNNT_OK;
}

int rnnt_engine_beam_decode_lstm(const void *frames, int64_t frame_stride, int rows, const int32_t *utt, int n_utt, int max_frames,
                                 const rnnt_lstm_predictor_params *p, int S, int E, int Hd, int O, int L, int layer_norm, float eps_in,
                                 float eps_lstm, float eps_out, const void *text_W, const void *text_b, const void *W, const void *bias,
                                 int H, int V, int blank, int max_length, int max_per_frame, int beam, int iterations, int init,
                                 int32_t *host_flag, int32_t *state, int32_t *tokens, double *scores, void *workspace, size_t ws_bytes,
                                 void *stream)
{
    size_t need;
    if (int rc = rnnt_engine_beam_decode_lstm_workspace_bytes(n_utt, S, E, Hd, O, L, layer_norm, H, V, text_W ? 1 : 0, max_length, beam, &need))
        return rc;
    const DecodeCall c{frames, p, L, layer_norm != 0, text_W, text_b, W, bias, iterations, host_flag, workspace, ws_bytes, need};
    int32_t *flag_dev;
    if (int rc = ld_check_pointers(c, !utt || !state || !tokens || !scores, ((uintptr_t)utt & 7) || ((uintptr_t)scores & 7),
                                   "utt and scores must be 8-byte and the workspace 256-byte aligned"))
        return rc;
    if (max_per_frame < 1 || max_frames < 1 || rows < max_frames || bad_stride(frame_stride, H))
        return engine_fail(RNNT_ERR_INVALID_ARG, "max_per_frame=%d max_frames=%d rows=%d frame_stride=%lld", max_per_frame, max_frames, rows,
                           (long long)frame_stride);
    if (int rc = check_blank(blank, V)) return rc;
    if ((long)max_frames * max_per_frame + 1 > 0x7fffffffL)
        return engine_fail(RNNT_ERR_UNSUPPORTED, "max_frames * max_per_frame must stay below 2^31 (max_frames=%d, max_per_frame=%d)", max_frames,
                           max_per_frame);
    if (int rc = ld_check_flag_and_size(c, &flag_dev)) return rc;
    BeamLstmArgs a{};
    a.s.n_utt = n_utt; a.s.max_length = max_length;
    ld_model(a.s, p, S, E, Hd, O, L, layer_norm, eps_in, eps_lstm, eps_out, text_W, text_b, H);
    a.frames = (const float *)frames; a.frame_stride = (long)frame_stride; a.rows = rows; a.utt = utt;
    a.W = (const float *)W; a.bias = (const float *)bias; a.V = V; a.blank = blank; a.max_per_frame = max_per_frame; a.beam = beam;
    a.iterations = iterations ? iterations : max_frames * max_per_frame + 1;
    a.init = init;
    a.host_flag = flag_dev; a.state = state; a.tokens = tokens; a.scores = scores; a.workspace = workspace;
    launch_beam_decode_lstm(a, (hipStream_t)stream);
    return status("rnnt_engine_beam_decode_lstm");
}

}  // extern "C"
