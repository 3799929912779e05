// split_dhidden.hpp — what the hand-scheduled dHidden kernels of the two split routes (x3.hip: k_dhidden_x3; x2.hip: k_dhidden_x2,
// k_dhidden_x2r) share, written once over the piece format F (split_common.hpp): everything that is not a kernel's k-step schedule.
//   dh_tile            (b, tt, ub) -> the tile's first cell and the utterance's lengths
//   DhCell             the producer role of a lane: its cell, the cell's coefficients (dead cells normalised), its source row
//   DhLines<F>         whole-line stores of G's hi | mid planes: LDS read address, raw buffer over the tile's rows, per-line offsets
//   DhRaw<F>, DhProd<F>, dh_xload_logits, dh_produce_slice<F, FIRST>, dh_produce   raw logits -> G -> F::NP planes in the LDS exchange
//   dh_dfac2, split_dhidden_epilogue.inc      x (1 - hidden^2), sum over u -> dEnc slab, sum over t -> dPred slab, over acc[MT][4 NG]
// Tile = DH_BT t x DH_BU u cells = four M tiles of 32 cells: row r of M tile m = cell (t0 + 2m + (r >> 4), u0 + (r & 15)).
// LDS exchange of one k-step: [M tile][plane][lane] x 16 bytes = F::NP KiB per M tile; two slots (k-step parity) lie 4 M tiles apart.
// What stays in each kernel: where its tile comes from, the W DMA, the ring prologue, the k-step loops with their product blocks and
// every vmcnt / lgkmcnt — the order of a kernel's memory operations is its own, the counts depend on it.
#pragma once
#include "split_common.hpp"

typedef float f2 __attribute__((ext_vector_type(2)));

#define DH_BT 8
#define DH_BU 16

struct DhTile { int b, tt, ub, t0, u0, Tb, Ub; };
__device__ __forceinline__ DhTile dh_tile(const X3Args &a, int b, int tt, int ub)
{
    DhTile tl;
    tl.b = b; tl.tt = tt; tl.ub = ub;
    len_tu_uniform(a.logit_lens, a.target_lens, b, a.T, a.U1, tl.Tb, tl.Ub);
    tl.t0 = tt * DH_BT; tl.u0 = ub * DH_BU;
    return tl;
}

// ---- producer role: wave w turns M tile w into G, lane (i = lane & 31, half = lane >> 5) owns the 8 vocabulary entries 16c + 8 half .. +7
// of row i per k-step c — its slot of the MFMA A fragment.  The lane's memory per k-step:
//   logits (fp32): 32 bytes at row + 64c + 32half               (f32x4 index 4c + 2half, +1)
//   G hi: 16 bytes at row + 128(c>>1) + 32(c&1) + 16half        (u32x4 index 8(c>>1) + 2(c&1) + half);  G mid: + 64 bytes
// Rows outside the lattice read the zero padding row (finite) with c1 = -inf -> G = 0; FIRST = false (a later column pass): every
// existing row holds its G planes already.
struct DhCell {
    int pt;
    bool pexists, live;
    long zrow, pcell;   // first zero padding row; the cell's row (zrow where it does not exist)
    CellCoef cf;
    const float *xsrc;
    __device__ __forceinline__ void at(const X3Args &a, const DhTile &tl, int wave, int lane)
    {
        const int prow = wave * 32 + (lane & 31);
        pt = tl.t0 + (prow >> 4);
        const int pu = tl.u0 + (prow & 15);
        pexists = pt < a.T && pu < a.U1;
        zrow = (long)a.B * a.T * a.U1;
        pcell = pexists ? ((long)tl.b * a.T + pt) * a.U1 + pu : zrow;
    }
    template <bool FIRST> __device__ __forceinline__ void load_coef(const X3Args &a, const DhTile &tl)
    {
        cf = a.coef[pexists ? pcell : 0];
        live = pexists && pt < tl.Tb && cf.c1 != RNNT_NEG_INF;
        if (!live) { cf.c1 = RNNT_NEG_INF; cf.sb = 0.f; cf.se = 0.f; cf.y = -1; }
        xsrc = a.logits + ((FIRST ? live : pexists) ? pcell : zrow) * a.V;
    }
};

// ---- whole-line stores: G's hi | mid planes leave in WHOLE 128-byte lines.  A line = the 32 x hi | 32 x mid of one cell and one 32-wide
// chunk = the fragments of two k-steps (c even, c odd) x two wave halves x two planes — eight 16-byte pieces that the producing wave
// reads back from ITS part of the exchange (both slots hold the pair between the exchange write of the odd k-step and the next even
// one's) in row order: lane L -> row 8n + (L >> 3) of the M tile (n = 0..3: four store instructions, 8 whole lines each), piece L & 7 =
// (plane, k-step parity, half).  Raw-buffer stores over the tile's rows: rows outside the lattice get an offset past the range
// (dropped), so every wave issues the same store instructions.
template <class F> struct DhLines {
    int xl;                        // LDS: [slot = parity][M tile wave][plane][lane slot = row + 32 half]
    __amdgpu_buffer_rsrc_t grs;    // the tile's logits rows
    int lvo[4];                    // byte offset of this lane's piece of line n: row (t0 + 2 wave + (n >> 1), u0 + 8 (n & 1) + lrow)
    __device__ __forceinline__ void at(const X3Args &a, const DhTile &tl, int xbase, int wave, int lane)
    {
        const int lpiece = lane & 7, lrow = lane >> 3;
        xl = xbase + ((lpiece >> 1) & 1) * (4 * F::NP * 1024) + wave * (F::NP * 1024) + (lpiece >> 2) * 1024 + 16 * (lrow + 32 * (lpiece & 1));
        const long tile_cell0 = ((long)tl.b * a.T + tl.t0) * a.U1 + tl.u0;  // the tile's first cell (exists: t0 < Tb <= T, u0 <= Ub < U1)
        grs = __builtin_amdgcn_make_buffer_rsrc((void *)(a.logits + tile_cell0 * a.V), 0, (int)((((long)(DH_BT - 1) * a.U1 + DH_BU) * a.V) * 4), 0x00020000);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int lt = 2 * wave + (n >> 1), lu = 8 * (n & 1) + lrow;
            const bool ex = tl.t0 + lt < a.T && tl.u0 + lu < a.U1;
            lvo[n] = ex ? (int)(((long)lt * a.U1 + lu) * a.V * 4) + 64 * (lpiece >> 2) + 16 * (lpiece & 3) : 0x7ffffff0;
        }
    }
    template <int N> __device__ __forceinline__ void read(u32x4 &v) const  // rows 8N .. 8N+7 of the M tile: lane slot + 8N
    {
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(xl), "n"(128 * N));
    }
    __device__ __forceinline__ void store(u32x4 &v, int n, int ce) const  // line n of the pair (ce, ce + 1): chunk ce >> 1 of the rows
    {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v) :: "memory");
        __builtin_amdgcn_raw_buffer_store_b128(v, grs, lvo[n], 128 * (ce >> 1), 0);
    }
};

// ---- G production.  Raw: FIRST: the lane's 8 fp32 logits of a k-step in p[0], p[1]; else its piece of each of G's planes.
template <class F> struct DhRaw { u32x4 p[F::NP]; };
template <class F> struct DhProd { f32x4 g0, g1; u32x4 p[F::NP]; };
// part: 1 first half, 2 second half, 3 both (the later passes' form, from the stored planes, is each kernel's own)
template <class F> __device__ __forceinline__ void dh_xload_logits(DhRaw<F> &r, const float *xsrc, int cc, int half, int part)
{
    const u32x4 *p = (const u32x4 *)xsrc + 4 * cc + 2 * half;
    if (part & 1) r.p[0] = p[0];
    if (part & 2) r.p[1] = p[1];
}
// G of k-step c from the raw values -> exchange slot (c & 1), write address xw (+ the slot).  The work is cut into slices (0..8) that a
// kernel threads through the gaps of its first MFMA blocks: one wave per SIMD issues ~1 instruction per 4-5 cycles and an MFMA leaves
// 24 of its 32 cycles to other instructions, so ~150 instructions in FRONT of a k-step's MFMAs would cost a quarter of it.
// 0-3 exp2, 4 label correction, 5 blank correction, 6-7 the split (F::split_g4: G times g_scale where the format has one), 8 exchange.
template <class F, bool FIRST>
__device__ __forceinline__ void dh_produce_slice(DhProd<F> &P, const DhRaw<F> &r, int c, int sl, const CellCoef &cf, int half, int blank, float gs, int xw)
{
    if (!FIRST) {
        if (sl == 0) {
#pragma unroll
            for (int q = 0; q < F::NP; ++q) P.p[q] = r.p[q];
        }
    } else if (sl < 4) {
        P.g0[sl] = __builtin_amdgcn_exp2f(fmaf(__builtin_bit_cast(f32x4, r.p[0])[sl], RNNT_LOG2E, cf.c1));
        P.g1[sl] = __builtin_amdgcn_exp2f(fmaf(__builtin_bit_cast(f32x4, r.p[1])[sl], RNNT_LOG2E, cf.c1));
    } else if (sl == 4) {
        const int vb = 16 * c + 8 * half;
        const unsigned dy = (unsigned)(cf.y - vb);
        if (__any(dy < 8u)) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                P.g0[e] = (dy == (unsigned)e) ? P.g0[e] - cf.se : P.g0[e];
                P.g1[e] = (dy == (unsigned)(e + 4)) ? P.g1[e] - cf.se : P.g1[e];
            }
        }
    } else if (sl == 5) {
        const int vb = 16 * c + 8 * half;
        if ((unsigned)(blank - 16 * c) < 16u) {  // wave-uniform
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                P.g0[e] = (vb + e == blank) ? P.g0[e] - cf.sb : P.g0[e];
                P.g1[e] = (vb + e + 4 == blank) ? P.g1[e] - cf.sb : P.g1[e];
            }
        }
    } else if (sl == 6) {
        F::split_g4(P.g0, gs, P.p, 0);
    } else if (sl == 7) {
        F::split_g4(P.g1, gs, P.p, 2);
    }
    if (sl == 8) {
        const int dst = xw + (c & 1) * (4 * F::NP * 1024);
        asm volatile("ds_write_b128 %0, %1" :: "v"(dst), "v"(P.p[0]) : "memory");
#pragma unroll
        for (int q = 1; q < F::NP; ++q) asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(dst), "v"(P.p[q]), "n"(q * 1024) : "memory");
    }
}
// all slices at once (pipeline prologue)
template <class F, bool FIRST>
__device__ __forceinline__ void dh_produce(const DhRaw<F> &r, int c, const CellCoef &cf, int half, int blank, float gs, int xw)
{
    DhProd<F> P;
#pragma unroll
    for (int sl = 0; sl < 9; ++sl) dh_produce_slice<F, FIRST>(P, r, c, sl, cf, half, blank, gs, xw);
}

// ---- epilogue.  The tanh' factor 1 - hidden^2 is RECOMPUTED from enc and pred (two small, cache-resident operands) instead of re-reading
// hidden's planes, in the form 1 - tanh^2(x) = 4 w / (1 + w)^2, w = exp(-2|x|): one exp2, one reciprocal and three multiplies per
// element on register PAIRS (v_pk_*; no MFMA runs beside this phase), no cancellation near |hidden| = 1, no overflow (w <= 1).  The
// factor 4 is applied to the sums (exact), with the format's 1 / (g_scale s_W) (F::dh_unscale, a power of two).
// Rows outside the lattice have G = 0 and therefore an exactly zero accumulator: any finite value will do.
__device__ __forceinline__ f2 dh_dfac2(f2 x)  // (1 - tanh^2 x) / 4 of two values
{
    const f2 a = x * (2.0f * RNNT_LOG2E);
    const f2 w = {__builtin_amdgcn_exp2f(-__builtin_fabsf(a[0])), __builtin_amdgcn_exp2f(-__builtin_fabsf(a[1]))};
    const f2 e1 = w + 1.0f;
    const f2 r = {__builtin_amdgcn_rcpf(e1[0]), __builtin_amdgcn_rcpf(e1[1])};
    return (w * r) * r;
}
// The epilogue's body is split_dhidden_epilogue.inc, expanded inside the three kernels: as an always-inline function — its arguments by
// reference, by value or as scalars — it compiled to the same MFMA loops but cost k_dhidden_x3 and k_dhidden_x2 9 to 18 scratch
// instructions and ~350 more in their epilogues (profiles/dhidden_toolkit_isa.txt).
