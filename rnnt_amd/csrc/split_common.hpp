// split_common.hpp — what the two split routes (x3.hip: bf16x3, x2.hip: f16x2) share: the piece format of a route as a trait type, and
// the plain kernels and host functions that differ between the routes in the piece format only, written once over it.
//
// A format F gives
//   NP                      planes per operand (hi, mid[, lo])
//   G_LO                    G's last plane does not fit into the logits row it replaces and lies beside it (X3Args::g_lo)
//   prepare(x, s)           what is done to an fp32 value in front of the split: nothing, or clamp(s x); prepare4: to four
//   hidden_scale(), w_scale(scales)   the s of the hidden operand and of W
//   split2(a, b)            two (prepared) fp32 values -> their pieces, packed pairwise (element 0 in the low half)
//   split4(x4, planes.., d) four consecutive values -> 2 packed dwords per plane at dword positions d, d+1 of the plane vectors,
//                           the planes as separate vectors or as one array u32x4[NP]
//   mfma(a, b, c)           its 32x32x16 MFMA; mfma_v(c, a, b): the same with the accumulator held in VGPRs, spelled as asm (left to hipcc an
//                           accumulator tile beside 256 others is shuttled through the full AGPR file); ONES: a pair of its ones
//   SCALED                  its operands carry scales: sums of products are rescaled where they leave (X3Args::dw_rescale, db_rescale)
//   split_g4(g4, gs, p, d)  split4 of four values of G, gs = X3Args::g_scale (a format without a scale ignores it; no clamp: |G| <= grad_scale)
//   dh_unscale(a)           what dHidden's sums are multiplied by: 4 (its tanh' form) over the operands' scales
#pragma once
#include "kernels.hpp"
#include "mma_common.hpp"

// bf16x3: x = hi + mid + lo, hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) (RNE each).  No scale, no clamp: bf16 has fp32's range.
struct Bf16x3 {
    static constexpr int NP = 3;
    static constexpr bool G_LO = true;
    struct Pieces { unsigned h, m, l; };
    static __device__ __forceinline__ float prepare(float x, float) { return x; }
    static __device__ __forceinline__ f32x4 prepare4(f32x4 x, float) { return x; }
    static __device__ __forceinline__ float hidden_scale() { return 1.f; }
    static __device__ __forceinline__ float w_scale(const float *) { return 1.f; }
    static __device__ __forceinline__ Pieces split2(float a, float b)
    {
        Pieces p;
        p.h = pack_bf16(a, b);
        const float ra = a - bf16_lo(p.h), rb = b - bf16_hi(p.h);  // exact: the residual has <= 16 significant bits
        p.m = pack_bf16(ra, rb);
        p.l = pack_bf16(ra - bf16_lo(p.m), rb - bf16_hi(p.m));
        return p;
    }
    template <class X4> static __device__ __forceinline__ void split4(const X4 &x4, u32x4 &ph, u32x4 &pm, u32x4 &pl, int d)
    {
        const Pieces p0 = split2(x4[0], x4[1]), p1 = split2(x4[2], x4[3]);
        ph[d] = p0.h; pm[d] = p0.m; pl[d] = p0.l;
        ph[d + 1] = p1.h; pm[d + 1] = p1.m; pl[d + 1] = p1.l;
    }
    template <class X4> static __device__ __forceinline__ void split4(const X4 &x4, u32x4 (&p)[NP], int d) { split4(x4, p[0], p[1], p[2], d); }
    static __device__ __forceinline__ void set(u32x4 (&p)[NP], int d, const Pieces &q) { p[0][d] = q.h; p[1][d] = q.m; p[2][d] = q.l; }
    template <class X4> static __device__ __forceinline__ void split_g4(const X4 &g4, float, u32x4 (&p)[NP], int d) { split4(g4, p, d); }
    static __device__ __forceinline__ float dh_unscale(const X3Args &) { return 4.0f; }
    static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) { return mfma_bf16(a, b, c); }
    static constexpr bool SCALED = false;
    static constexpr unsigned ONES = 0x3f803f80u;
    static __device__ __forceinline__ void mfma_v(f32x16 &c, u32x4 a, u32x4 b) { asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b)); }
};

// f16x2: x = (hi + mid) / s, hi = f16(s x), mid = f16(s x - hi) (RNE each), s a power of two that lifts the operand's largest magnitude to
// ~2^14 (fp16's 5-bit exponent needs it).  Values beyond fp16's range after scaling (only possible for non-finite or garbage operands) are
// clamped to +-65504 in front of the split.
#define X2_SH 16384.0f          // scale of the hidden operand (|tanh| <= 1)
#define X2_INV_SH (1.0f / 16384.0f)
#define X2_F16_MAX 65504.0f
struct F16x2 {
    static constexpr int NP = 2;
    static constexpr bool G_LO = false;
    struct Pieces { unsigned h, m; };
    static __device__ __forceinline__ float clamp(float x) { return __builtin_amdgcn_fmed3f(x, -X2_F16_MAX, X2_F16_MAX); }
    static __device__ __forceinline__ float prepare(float x, float s) { return clamp(x * s); }
    static __device__ __forceinline__ f32x4 prepare4(f32x4 x, float s)
    {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = prepare(x[k], s);
        return x;
    }
    static __device__ __forceinline__ float hidden_scale() { return X2_SH; }
    static __device__ __forceinline__ float w_scale(const float *scales) { return scales[0]; }  // s_W (k_x2_wscale)
    static __device__ __forceinline__ Pieces split2(float a, float b)  // 4 instructions
    {
        Pieces p;
        p.h = pack_f16_pair(a, b);
        float ra, rb;  // x - hi, exact (the residual has <= 14 significant bits): v_fma_mix reads the fp16 half in place
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(ra) : "v"(p.h), "v"(a));
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(rb) : "v"(p.h), "v"(b));
        p.m = pack_f16_pair(ra, rb);
        return p;
    }
    template <class X4> static __device__ __forceinline__ void split4(const X4 &x4, u32x4 &ph, u32x4 &pm, int d)
    {
        const Pieces p0 = split2(x4[0], x4[1]), p1 = split2(x4[2], x4[3]);
        ph[d] = p0.h; pm[d] = p0.m;
        ph[d + 1] = p1.h; pm[d + 1] = p1.m;
    }
    template <class X4> static __device__ __forceinline__ void split4(const X4 &x4, u32x4 (&p)[NP], int d) { split4(x4, p[0], p[1], d); }
    static __device__ __forceinline__ void set(u32x4 (&p)[NP], int d, const Pieces &q) { p[0][d] = q.h; p[1][d] = q.m; }
    template <class X4> static __device__ __forceinline__ void split_g4(const X4 &g4, float gs, u32x4 (&p)[NP], int d)
    {
        const f32x4 s4 = g4 * gs;  // (|G| <= grad_scale: no clamp needed; exact: a power of two)
        split4(s4, p, d);
    }
    static __device__ __forceinline__ float dh_unscale(const X3Args &a) { return 4.0f * a.db_rescale * a.scales[1]; }  // 4 / (g_scale s_W)
    static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) { return mfma_f16(a, b, c); }
    static constexpr bool SCALED = true;
    static constexpr unsigned ONES = 0x3c003c00u;
    static __device__ __forceinline__ void mfma_v(f32x16 &c, u32x4 a, u32x4 b) { asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b)); }
};

// ---------------------------------------------------------------------------------------
// Plain producers.  k_split_make_hidden / k_split_g are the one-thread-per-piece forms of what the forward prologue and the
// dHidden kernel do in their tiles: they serve the unfused variants (RNNT_VARIANT_X3_FP32_*), which exist so that every fused
// kernel can be checked against the same pipeline with one stage swapped, and as the plain statement of the data layout.
// ---------------------------------------------------------------------------------------
// hidden planes [NP][rows_alloc][H] of hidden_scale tanh(enc + pred), every cell (also dead ones: the backward multiplies them by
// exact zeros, they only have to be finite).  One thread = 8 columns of one row.
// (f16x2: hidden = tanh(.) is finite or NaN; v_med3 maps a NaN to -65504: non-finite enc / pred are caught upstream by k_x2_make_ep's
// flag and run the exact form)
template <class F>
__global__ __launch_bounds__(256) void k_split_make_hidden(X3Args a)
{
    const int H8 = a.H / 8;
    const long cells = (long)a.B * a.T * a.U1;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= cells * H8) return;
    const long c = idx / H8;
    const int h = (int)(idx - c * H8) * 8;
    const int u = (int)(c % a.U1);
    const long bt = c / a.U1;
    const int t = (int)(bt % a.T), b = (int)(bt / a.T);
    const float *ep = a.enc + (long)b * a.enc_sb + (long)t * a.enc_st + h;
    const float *pp = a.pred + ((long)b * a.U1 + u) * a.H + h;
    const f32x4 t0 = F::prepare4(fast_tanh_sum4(*(const f32x4 *)ep, *(const f32x4 *)pp), F::hidden_scale());
    const f32x4 t1 = F::prepare4(fast_tanh_sum4(*(const f32x4 *)(ep + 4), *(const f32x4 *)(pp + 4)), F::hidden_scale());
    u32x4 p[F::NP];
    F::split4(t0, p, 0);
    F::split4(t1, p, 2);
    u32x4 *o = (u32x4 *)(a.hidden + c * a.H + h);
    const long ps = a.plane_stride / 8;  // u32x4 units
#pragma unroll
    for (int q = 0; q < F::NP; ++q) o[q * ps] = p[q];
}

// fp32 G (what the fp32 route's k_dhidden_gen / k_make_g leave in place of the logits) -> the planes of g_scale G: hi | mid over the
// same 128 bytes of every 32-wide chunk, a third plane beside (g_lo).  One thread = one chunk of one row (it reads the whole 128
// bytes before it overwrites them).
template <class F>
__global__ __launch_bounds__(256) void k_split_g(X3Args a, long rows)
{
    const int VC = a.V / 32;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * VC) return;
    const long r = idx / VC;
    const int c = (int)(idx - r * VC);
    f32x4 *p = (f32x4 *)(a.logits + r * a.V + 32 * c);
    f32x4 x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = F::prepare4(p[i], a.g_scale);
    u32x4 pl[4][F::NP];
#pragma unroll
    for (int i = 0; i < 8; ++i) F::split4(x[i], pl[i >> 1], 2 * (i & 1));
    u32x4 *o = (u32x4 *)p;
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[i] = pl[i][0]; o[4 + i] = pl[i][1]; }
    if constexpr (F::G_LO) {
        u32x4 *ol = (u32x4 *)(a.g_lo + r * a.V + 32 * c);
#pragma unroll
        for (int i = 0; i < 4; ++i) ol[i] = pl[i][2];
    }
}

template <class F> void launch_split_make_hidden(const X3Args &a, hipStream_t st)
{
    const long n = (long)a.B * a.T * a.U1 * (a.H / 8);
    hipLaunchKernelGGL(k_split_make_hidden<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
}
template <class F> void launch_split_g(const X3Args &a, hipStream_t st)
{
    const long rows = (long)a.B * a.T * a.U1;
    const long n = rows * (a.V / 32);
    hipLaunchKernelGGL(k_split_g<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, rows);
}
// zero rows past the last cell, all planes (the dW ring walks up to 96 of them; the "dead row" source of dHidden tiles).
// `what` 1: hidden (before the forward), 2: G (after the forward, whose last tile writes logits there)
template <class F> void launch_split_zero_padding(const X3Args &a, int what, hipStream_t st)
{
    const long cells = (long)a.B * a.T * a.U1;
    const size_t pad = (size_t)(a.rows_alloc - cells);
    if (what & 1)
        for (int p = 0; p < F::NP; ++p) launch_fill32(a.hidden + p * a.plane_stride + cells * a.H, 0u, pad * a.H * 2, st);
    if (what & 2) {
        launch_fill32(a.logits + cells * a.V, 0u, pad * a.V * 4, st);
        if (F::G_LO) launch_fill32(a.g_lo + cells * a.V, 0u, pad * a.V * 2, st);
    }
}

// ---------------------------------------------------------------------------------------
// W (times w_scale) for the forward product, fragment order, NP planes:
//   [pass (512 logits columns)][c (16-deep k-step)][plane][tile(16)][lane] x 8 pieces,
//   element j = piece_plane(W[v = 512pass + 128*(tile>>2) + 4*(lane&31) + (tile&3)][h = 16c + 8*(lane>>5) + j])
// (columns interleaved by 4, as in the dHidden pack: a lane's 4 tiles of a 128-column group are 4 adjacent logits).
// Tiles past V are zeros.
// ---------------------------------------------------------------------------------------
template <class F>
__global__ __launch_bounds__(256) void k_split_pack_w_fwd(const float *__restrict__ W, const float *__restrict__ scales, u32x4 *__restrict__ out, int H, int V, long n)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // (pass, c, tile, lane): one thread writes every plane
    if (idx >= n) return;
    const int lane = (int)(idx & 63), tile = (int)(idx >> 6) & 15;
    const int KC = H / 16;
    const int c = (int)((idx >> 10) % KC), pass = (int)((idx >> 10) / KC);
    const int v = 512 * pass + 128 * (tile >> 2) + 4 * (lane & 31) + (tile & 3);
    const int h0 = 16 * c + 8 * (lane >> 5);
    const float sw = F::w_scale(scales);
    u32x4 p[F::NP];
#pragma unroll
    for (int q = 0; q < F::NP; ++q) p[q] = u32x4{0u, 0u, 0u, 0u};
    if (v < V) {
        const float *w = W + (long)v * H + h0;
        const f32x4 w0 = F::prepare4(*(const f32x4 *)w, sw), w1 = F::prepare4(*(const f32x4 *)(w + 4), sw);
        F::split4(w0, p, 0);
        F::split4(w1, p, 2);
    }
    u32x4 *o = out + ((long)pass * KC + c) * (F::NP * 1024) + tile * 64 + lane;
#pragma unroll
    for (int q = 0; q < F::NP; ++q) o[q * 1024] = p[q];
}
template <class F> size_t split_wpack_fwd_bytes(int H, int V) { return (size_t)((V + 511) / 512) * (H / 16) * F::NP * 16 * 64 * 16; }

// ---------------------------------------------------------------------------------------
// W (times w_scale) for the dHidden product, fragment order, NP planes:
//   [hp (512-column pass)][c (16-deep k-step = 16 vocabulary rows)][plane][tile(16)][lane] x 8 pieces,
//   element j = piece_plane(W[v = 16c + 8*(lane>>5) + j][h = 512hp + 128*(tile>>2) + 4*(lane&31) + (tile&3)])
// (columns interleaved by 4: a lane's 4 tiles of a 128-column group are 4 adjacent columns -> 16-byte epilogue accesses).
// One k-step = NP x 16 KiB, staged by one linear LDS-DMA copy.  Tiles past H are zeros.
// ---------------------------------------------------------------------------------------
template <class F>
__global__ __launch_bounds__(256) void k_split_pack_w_dh(const float *__restrict__ W, const float *__restrict__ scales, u32x4 *__restrict__ out, int H, int V, long n)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // (hp, c, tile, lane): one thread writes every plane
    if (idx >= n) return;
    const int lane = (int)(idx & 63), tile = (int)(idx >> 6) & 15;
    const int VC = V / 16;
    const int c = (int)((idx >> 10) % VC), hp = (int)((idx >> 10) / VC);
    const int h = 512 * hp + 128 * (tile >> 2) + 4 * (lane & 31) + (tile & 3);
    const int v0 = 16 * c + 8 * (lane >> 5);
    const float sw = F::w_scale(scales);
    u32x4 p[F::NP];
#pragma unroll
    for (int q = 0; q < F::NP; ++q) p[q] = u32x4{0u, 0u, 0u, 0u};
    if (h < H) {
        const float *w = W + (long)v0 * H + h;
#pragma unroll
        for (int j = 0; j < 4; ++j) F::set(p, j, F::split2(F::prepare(w[(long)(2 * j) * H], sw), F::prepare(w[(long)(2 * j + 1) * H], sw)));
    }
    u32x4 *o = out + ((long)hp * VC + c) * (F::NP * 1024) + tile * 64 + lane;
#pragma unroll
    for (int q = 0; q < F::NP; ++q) o[q * 1024] = p[q];
}
template <class F> size_t split_wpack_dh_bytes(int H, int V) { return (size_t)((H + 511) / 512) * (V / 16) * F::NP * 16 * 64 * 16; }

// both packs of the joint's W (`scales`: device {s_W, 1 / s_W} for a format with a scale, else unread)
template <class F> void launch_split_pack_w(const X3Args &a, const float *scales, hipStream_t st)
{
    const long nd = (long)((a.H + 511) / 512) * (a.V / 16) * 16 * 64;
    hipLaunchKernelGGL(k_split_pack_w_dh<F>, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, a.W, scales, (u32x4 *)a.wpack_dh, a.H, a.V, nd);
    const long nf = (long)((a.V + 511) / 512) * (a.H / 16) * 16 * 64;
    hipLaunchKernelGGL(k_split_pack_w_fwd<F>, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, a.W, scales, (u32x4 *)a.wpack_fwd, a.H, a.V, nf);
}
