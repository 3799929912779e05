// split_dw.hpp — what the hand-scheduled dW kernels of the MFMA routes (bf16.hip: k_dw_bf16; x3.hip: k_dw_x3; x2.hip: k_dw_x2, k_dw_x2m)
// share, written once over the piece format F (split_common.hpp; Bf16x1 below for the one-plane route) and a ring depth NST: everything
// about a dW kernel that is not its schedule.
//   DwRing<F, NST>        ring geometry of one operand tile: [stage][plane][16 rows x 256 B]; the counted wait of a k-step
//   DW_GRAN, DW_ROWS_PAST the granule of the live-row table; the rows a ring may read past rows_pad
//   dw_xcd_remap, dw_tile workgroup id -> XCD remap -> (tile, split, vb, hb, wm, wn, v0, h0) of the 2 x 2 wave layout
//   DwSource<F>, dw_source, dw_soff   plane bases and row strides of a wave's operand tile; the swizzled per-lane source offsets
//   dw_dma_imm            one LDS-DMA piece whose instruction carries the immediate 1024 i (the four-way ladder)
//   dw_frag_off, dw_frag_addr, dw_reads, dw_product, dw_bias_read, dw_bias_mfma, DwBias, dw_bias_setup   fragment addressing and the
//                         k-step pieces; dw_kstep2 / dw_kstep3: one k-step on two / three planes
//   DwLockstep<LAG, PERIOD>    the soft lockstep of the tiles of a split (the f16x2 kernels'; k_dw_bf16 keeps its own text, see there)
//   dw_ring               one pipeline run of a 4-stage ring (the f16x2 kernels')
//   DwShare, dw_walk_ranges   a split's share of the live-row table; its walk: each live range -> the kernel's pipeline run (k_dw_x3;
//                         k_dw_bf16 spells the loop over DwShare's fields, see there)
//   dw_store<F, GUARD>, dw_store_w    the slab and bias epilogue with the format's rescale
// Tile = 256 v x 256 h, 4 waves = 2 (M) x 2 (N), wave 128 x 128 = 16 accumulator tiles.  Operand tile = 128 columns x 16 cells of one
// plane = 4 KiB: 256-byte rows, 16-byte chunk ch of row r at 16 (ch ^ swz(r)), swz(r) = ((r & 3) << 2) | ((r >> 2) & 3), applied on the
// DMA's SOURCE side (the DMA writes LDS linearly).
// What stays in each kernel: which operand tile a wave stages and from which rows (its list or range walk), the counted wait in front of
// a k-step, the placement of the DMA pieces in the products, the unrolling of the ring, dead tiles.
// The pieces are plain `inline`, not __forceinline__: the regular inliner takes them bottom-up, as it took the lambdas they replace, and
// the k loops come out instruction for instruction as before; inlined by force (before any simplification) every k-step of k_dw_x2
// gained eight v_mov of zeros for the db fragments (profiles/x2_dw_refactor_isa.txt).  Nothing here may stay a call: the accumulators go
// by reference.  The ablation word of the diagnostic builds is an argument of the pieces and read through RNNT_XP only (1024 no MFMA,
// 2048 no bias, 4096 no fragment reads, 8192 no DMA pieces): the shipped build compiles it to nothing.
#pragma once
#include "split_common.hpp"

// the one-plane format of the bf16 route: G and hidden are plain bf16 matrices
// (k_dw_bf16 keeps its own k-step — mma_step on mfma_bf16, db by v_dot2c — so the format is its plane count and no more)
struct Bf16x1 {
    static constexpr int NP = 1;
};

// ---- ring geometry
#define DW_ROWS 16        // cells per MFMA k-step = rows of an operand tile
// DW_GRAN (cells per granule of the live-row table: 2 k-steps) and DW_ROWS_PAST (rows a ring may read past rows_pad) are kernels.hpp's: the
// host's layout uses them too
template <class F, int NST_> struct DwRing {
    static constexpr int NP = F::NP, NST = NST_;
    static constexpr int PLANE = 4096;           // one operand tile of one plane: 16 rows x 256 B
    static constexpr int STAGE = NP * PLANE;     // one stage of one operand tile
    static constexpr int TILE = NST * STAGE;     // ring of one operand tile: [stage][plane][16 x 256 B]
    static constexpr int ND = 4 * NP;            // DMA pieces (4 rows x 256 B) per wave and stage
    // the counted wait in front of k-step ks: stage ks landed while the pieces of the NST - 2 stages behind it may still fly
    static constexpr int WAIT = ND * (NST - 2);
};

// ---- tile decode.  XCD-aware remap of the workgroup id: the tiles of one split share an XCD's L2
__device__ inline int dw_xcd_remap(int id, int total)
{
    const int q8 = total / 8, r8 = total % 8, x = id % 8;
    return (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + id / 8;
}
// the 256 x 256 tile of a workgroup and the 128 x 128 tile of a wave in it (2 x 2 waves)
struct DwTile { int n_hblk, tiles, tile, split, vb, hb, wm, wn, v0, h0; };
__device__ inline DwTile dw_tile(int block, int wave, int H, int V, int n_split)
{
    DwTile t;
    const int n_vblk = (V + 255) / 256;
    t.n_hblk = (H + 255) / 256;
    t.tiles = n_vblk * t.n_hblk;
    const int id = dw_xcd_remap(block, t.tiles * n_split);
    t.tile = id % t.tiles; t.split = id / t.tiles;
    t.vb = t.tile / t.n_hblk; t.hb = t.tile % t.n_hblk;
    t.wm = wave >> 1; t.wn = wave & 1;
    t.v0 = t.vb * 256 + t.wm * 128; t.h0 = t.hb * 256 + t.wn * 128;
    return t;
}

// ---- operand source of a wave: plane p of its operand tile — base pointer of the tile's first column (wave-uniform) and row stride in
// bytes.  G's hi | mid planes are interleaved in 128-byte chunks of the logits row they replace (bf16x3: the lo plane beside them, g_lo);
// the hidden planes lie plane_stride apart.  A tile beyond the matrix is never stored: it reads column 0.
template <class F> struct DwSource { const char *pbase[F::NP]; long rstride[F::NP]; };
__device__ inline int dw_col0(bool is_g, int blk, int sub, int H, int V)
{
    const int col0 = blk * 256 + 128 * sub;
    return col0 >= (is_g ? V : H) ? 0 : col0;
}
template <class F> __device__ inline void dw_source(DwSource<F> &s, const X3Args &a, bool is_g, int col0)
{
    if (is_g) {
        s.pbase[0] = (const char *)a.logits + 4L * col0;        // hi: first 64 bytes of each 128-byte chunk
        s.pbase[1] = (const char *)a.logits + 4L * col0 + 64;   // mid: last 64
        s.rstride[0] = s.rstride[1] = 4L * a.V;
        if constexpr (F::G_LO) { s.pbase[2] = (const char *)a.g_lo + 2L * col0; s.rstride[2] = 2L * a.V; }
    } else {
#pragma unroll
        for (int p = 0; p < F::NP; ++p) { s.pbase[p] = (const char *)(a.hidden + p * a.plane_stride) + 2L * col0; s.rstride[p] = 2L * a.H; }
    }
}
__device__ inline void dw_source(DwSource<Bf16x1> &s, const Bf16Args &a, bool is_g, int col0)
{
    s.pbase[0] = (is_g ? (const char *)a.logits : (const char *)a.hidden) + 2L * col0;
    s.rstride[0] = is_g ? 2L * a.V : 2L * a.H;
}
// Per-lane source offset of DMA piece i (ring rows 4i .. 4i + 3 of a plane's 16; i & 3 decides the swizzle): lane L fetches row
// row0 + (L >> 4) of the piece's buffer, LDS chunk position L & 15 <- global chunk jg = (L & 15) ^ swz(ring row),
// swz = ((L >> 4) << 2) | (i & 3); interleaved planes (G hi / mid): chunk jg of the plane is 16 bytes at 128 (jg >> 2) + 16 (jg & 3).
// imm: the immediate offset the piece's instruction carries (it advances the memory address too), taken back out here — 0 where the
// instruction carries none or the buffer's base has it taken out (k_dw_x2: x2_piece_rsrc)
__device__ inline int dw_soff(int lane, int i, int row0, long rstride, bool interleaved, int imm)
{
    const int jg = (lane & 15) ^ (((lane >> 4) << 2) | (i & 3));
    const int cb = interleaved ? 128 * (jg >> 2) + 16 * (jg & 3) : 16 * jg;
    return (int)((row0 + (lane >> 4)) * rstride) + cb - imm;
}
#define DW_SOFF_DEAD 0x7ffffff0  // past every buffer's range: the DMA moves no bytes (the instruction and its vmcnt stay)

// ---- one DMA piece into ring rows 4i .. of the plane at d: the four pieces of a plane share one LDS base (M0), piece i carries the
// immediate offset 1024 i (i: a constant once the caller's loop is unrolled)
__device__ inline void dw_dma_imm(__amdgpu_buffer_rsrc_t r, lds_vptr d, int soff, int i)
{
    if ((i & 3) == 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(r, d, 16, soff, 0, 0, 0);
    if ((i & 3) == 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(r, d, 16, soff, 0, 1024, 0);
    if ((i & 3) == 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(r, d, 16, soff, 0, 2048, 0);
    if ((i & 3) == 3) __builtin_amdgcn_raw_ptr_buffer_load_lds(r, d, 16, soff, 0, 3072, 0);
}
// nrows rows from `row` on of a plane as a raw buffer (wave-uniform base: scalar arithmetic only; the per-lane part of a DMA address is
// the 32-bit soff)
__device__ inline __amdgpu_buffer_rsrc_t dw_rows_rsrc(const char *pbase, long row, long rstride, int nrows)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)(pbase + row * rstride), 0, (int)(nrows * rstride), 0x00020000);
}

// ---- transposed fragment reads.  Fragment of 32-column tile m of an operand tile: lane (g = lane>>4, q = (lane&15)>>2, p = lane&3) reads
// rows 8(g>>1) + 4sec + q at chunk 4m + 2(g&1) + (p>>1), +8(p&1) bytes, sec = 0,1 — its byte offset in the tile's 16 rows, the chunk
// where the DMA's source-side swizzle put it; dw_frag_addr: its LDS address in stage 0, plane 0 of operand tile otile's ring (lds0: the ring's)
__device__ inline int dw_frag_off(int m, int sec, int lane)
{
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3, hh = g >> 1;
    const int row = 8 * hh + 4 * sec + q;
    const int swz = ((row & 3) << 2) | ((row >> 2) & 3);
    const int ch = 4 * m + 2 * (g & 1) + (pp >> 1);
    return 256 * row + 16 * (ch ^ swz) + 8 * (pp & 1);
}
template <class R> __device__ inline int dw_frag_addr(int lds0, int otile, int m, int sec, int lane)
{
    return lds0 + otile * R::TILE + dw_frag_off(m, sec, lane);
}
// 8 transposed reads of plane P, ring stage ST (compile-time: every LDS offset is an immediate) of an operand (inline asm: hipcc guards
// every LDS read it can see behind an LDS-DMA with vmcnt(0)); results are used only after FRAG8_LANDED named them
template <class R, int ST, int P>
__device__ inline void dw_reads(Frag8 &f, const int (&base)[4][2], int ablate)
{
    constexpr int off = ST * R::STAGE + P * R::PLANE;
    if (RNNT_XP(ablate, 4096)) return;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f.lo[m]) : "v"(base[m][0]), "n"(off));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f.hi[m]) : "v"(base[m][1]), "n"(off));
    }
}
// 16 MFMAs of one product with DMA pieces of the stage being refilled threaded through them, one behind a row of wave tiles.  WHERE is
// the kernel's schedule: bit qm of ROWS puts a piece behind row qm; the pieces are N0, N0 + 1, .. in row order.  dma_piece(Int<n>)
// issues piece n; live_n: this wave's h columns exist (wave-uniform)
template <int ROWS, int QM, int N0, class Piece> __device__ inline void dw_place(const Piece &dma_piece)
{
    if constexpr ((ROWS >> QM) & 1) dma_piece(Int<N0 + __builtin_popcount(ROWS & ((1 << QM) - 1))>{});
}
template <class F, int ROWS, int N0, class Piece>
__device__ inline void dw_product(f32x16 (&acc)[4][4], const Frag8 &fa_, const Frag8 &fb_, bool live_n, int ablate, const Piece &dma_piece)
{
    u32x4 fa[4], fb[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        fa[m] = u32x4{fa_.lo[m][0], fa_.lo[m][1], fa_.hi[m][0], fa_.hi[m][1]};
        fb[m] = u32x4{fb_.lo[m][0], fb_.lo[m][1], fb_.hi[m][0], fb_.hi[m][1]};
    }
#pragma unroll
    for (int qm = 0; qm < 4; ++qm) {
        if (live_n && !RNNT_XP(ablate, 1024)) {
#pragma unroll
            for (int qn = 0; qn < 4; ++qn) acc[qm][qn] = F::mfma(fa[qm], fb[qn], acc[qm][qn]);
        }
        if (!RNNT_XP(ablate, 8192)) {
            if (qm == 0) dw_place<ROWS, 0, N0>(dma_piece);
            if (qm == 1) dw_place<ROWS, 1, N0>(dma_piece);
            if (qm == 2) dw_place<ROWS, 2, N0>(dma_piece);
            if (qm == 3) dw_place<ROWS, 3, N0>(dma_piece);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
constexpr int dw_rows_of(int cnt) { return cnt == 4 ? 0xf : cnt == 3 ? 0xb : cnt == 2 ? 0x3 : cnt == 1 ? 0x1 : 0; }  // f16x2's placements: rows {0, 1, 3}, all four, {0, 1}
// db rides the matrix pipe: one more MFMA per plane and k-step against a column SELECTOR of ones (sv: the format's ones in the selector's
// column: column j of the product = the row sums of the M tile), for one (one h block: two) of the wave's M tiles — fragment bases sbase,
// read once more through their own base registers (a run-time choice among the wave's four fragment sets would be branches or selects
// around the MFMA) — into a 17th accumulator tile held in VGPRs.  (fp32 adds of unpacked halves cost ~50 VALU per k-step;
// v_dot2c_f32_bf16 with a pair of ones — the bf16 route's form — is not fp32-exact: 9e-3 relative error on db.)
template <class R, int ST, int P>
__device__ inline void dw_bias_read(u32x2 &lo, u32x2 &hi, const int (&sbase)[2])
{
    constexpr int off = ST * R::STAGE + P * R::PLANE;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(lo) : "v"(sbase[0]), "n"(off));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi) : "v"(sbase[1]), "n"(off));
}
template <class F> __device__ inline void dw_bias_mfma(u32x2 &lo, u32x2 &hi, f32x16 &dacc, unsigned sv)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo), "+v"(hi) :: "memory");
    const u32x4 fa = {lo[0], lo[1], hi[0], hi[1]};
    const u32x4 sel = {sv, sv, sv, sv};
    F::mfma_v(dacc, fa, sel);
}
// what a wave sums into db: nothing, the tile at sbase[0] (selector column 0), or with one h block (two_b, H <= 256 only) also the one at
// sbase[1] (column 1).  The 8 M tiles of a v block are shared out over the waves of the h blocks 0 and 1: (hb, wn) -> M tile bsel0 of this
// wave's wm half (one h block: each wave takes two tiles, bsel0 and bsel0 + 2)
struct DwBias { bool do_b, two_b; unsigned sel0, sel1; int sbase[2][2]; };
template <class F> __device__ inline int dw_bias_setup(DwBias &b, int n_hblk, int hb, int wn, int lane)
{
    b.do_b = hb < 2;  // workgroup-uniform
    b.two_b = n_hblk < 2;
    b.sel0 = (lane & 31) == 0 ? F::ONES : 0u; b.sel1 = (lane & 31) == 1 ? F::ONES : 0u;
    return n_hblk >= 2 ? (hb & 1) * 2 + wn : wn;
}
template <class R> __device__ inline void dw_bias_bases(DwBias &b, int lds0, int otile, int bsel0, int lane)
{
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int sec = 0; sec < 2; ++sec) b.sbase[k][sec] = dw_frag_addr<R>(lds0, otile, (bsel0 + 2 * k) & 3, sec, lane);
}
__device__ inline void dw_zero(f32x16 (&acc)[4][4], f32x16 &dacc)
{
#pragma unroll
    for (int qm = 0; qm < 4; ++qm)
#pragma unroll
        for (int qn = 0; qn < 4; ++qn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[qm][qn][r] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) dacc[r] = 0.f;
}

// ---- one k-step on ring stage ST, behind the kernel's counted wait for the stage: one barrier publishes it (every wave is past its reads
// of the stage before, whose ring slot the DMA pieces refill), then the products with the DMA pieces threaded through them; the fragment
// reads run one product ahead of their MFMAs.
// Two planes: products ah.bh, am.bh, ah.bm with C0 + C1 + C2 pieces (placements dw_rows_of)
template <class R, int ST, int C0, int C1, int C2, class Piece>
__device__ inline void dw_kstep2(f32x16 (&acc)[4][4], f32x16 &dacc, const int (&abase)[4][2], const int (&bbase)[4][2], const DwBias &b,
                                 bool live_n, int ablate, const Piece &dma_piece)
{
    lds_barrier();
    Frag8 Ah, Bh, Am, Bm;
    u32x2 dl[2], dh[2];
    dw_reads<R, ST, 0>(Ah, abase, ablate);
    dw_reads<R, ST, 0>(Bh, bbase, ablate);
    dw_reads<R, ST, 1>(Am, abase, ablate);
    FRAG8_LANDED(Ah, 8);
    FRAG8_LANDED(Bh, 8);
    dw_product<F16x2, dw_rows_of(C0), 0>(acc, Ah, Bh, live_n, ablate, dma_piece);
    dw_reads<R, ST, 1>(Bm, bbase, ablate);
    FRAG8_LANDED(Am, 8);
    dw_product<F16x2, dw_rows_of(C1), C0>(acc, Am, Bh, live_n, ablate, dma_piece);
    FRAG8_LANDED(Bm, 0);
    if (b.do_b) { dw_bias_read<R, ST, 0>(dl[0], dh[0], b.sbase[0]); dw_bias_read<R, ST, 1>(dl[1], dh[1], b.sbase[0]); }
    dw_product<F16x2, dw_rows_of(C2), C0 + C1>(acc, Ah, Bm, live_n, ablate, dma_piece);
    if (b.do_b && !RNNT_XP(ablate, 2048)) {
        dw_bias_mfma<F16x2>(dl[0], dh[0], dacc, b.sel0); dw_bias_mfma<F16x2>(dl[1], dh[1], dacc, b.sel0);
        if (b.two_b) {
            dw_bias_read<R, ST, 0>(dl[0], dh[0], b.sbase[1]); dw_bias_read<R, ST, 1>(dl[1], dh[1], b.sbase[1]);
            dw_bias_mfma<F16x2>(dl[0], dh[0], dacc, b.sel1); dw_bias_mfma<F16x2>(dl[1], dh[1], dacc, b.sel1);
        }
    }
}
// Three planes: products ah.bh, am.bh, am.bm, ah.bm, al.bh, ah.bl (at most five of the six fragment sets live: four + one landing), two
// pieces behind rows {1, 3} of every product
template <class R, int ST, class Piece>
__device__ inline void dw_kstep3(f32x16 (&acc)[4][4], f32x16 &dacc, const int (&abase)[4][2], const int (&bbase)[4][2], const DwBias &b,
                                 int ablate, const Piece &dma_piece)
{
    lds_barrier();
    Frag8 Ah, Bh, Am, Bm, Al, Bl;
    u32x2 dl[3], dh[3];
    dw_reads<R, ST, 0>(Ah, abase, ablate);
    dw_reads<R, ST, 0>(Bh, bbase, ablate);
    dw_reads<R, ST, 1>(Am, abase, ablate);
    FRAG8_LANDED(Ah, 8);
    FRAG8_LANDED(Bh, 8);
    dw_product<Bf16x3, 0xa, 0>(acc, Ah, Bh, true, ablate, dma_piece);
    dw_reads<R, ST, 1>(Bm, bbase, ablate);
    FRAG8_LANDED(Am, 8);
    dw_product<Bf16x3, 0xa, 2>(acc, Am, Bh, true, ablate, dma_piece);
    FRAG8_LANDED(Bm, 0);
    dw_product<Bf16x3, 0xa, 4>(acc, Am, Bm, true, ablate, dma_piece);
    dw_reads<R, ST, 2>(Al, abase, ablate);
    if (b.do_b) { dw_bias_read<R, ST, 0>(dl[0], dh[0], b.sbase[0]); dw_bias_read<R, ST, 1>(dl[1], dh[1], b.sbase[0]); dw_bias_read<R, ST, 2>(dl[2], dh[2], b.sbase[0]); }
    dw_product<Bf16x3, 0xa, 6>(acc, Ah, Bm, true, ablate, dma_piece);
    dw_reads<R, ST, 2>(Bl, bbase, ablate);
    FRAG8_LANDED(Al, 8);
    dw_product<Bf16x3, 0xa, 8>(acc, Al, Bh, true, ablate, dma_piece);
    FRAG8_LANDED(Bl, 0);
    dw_product<Bf16x3, 0xa, 10>(acc, Ah, Bl, true, ablate, dma_piece);
    if (b.do_b && !RNNT_XP(ablate, 2048)) {
        dw_bias_mfma<Bf16x3>(dl[0], dh[0], dacc, b.sel0); dw_bias_mfma<Bf16x3>(dl[1], dh[1], dacc, b.sel0); dw_bias_mfma<Bf16x3>(dl[2], dh[2], dacc, b.sel0);
        if (b.two_b) {
            dw_bias_read<R, ST, 0>(dl[0], dh[0], b.sbase[1]); dw_bias_read<R, ST, 1>(dl[1], dh[1], b.sbase[1]); dw_bias_read<R, ST, 2>(dl[2], dh[2], b.sbase[1]);
            dw_bias_mfma<Bf16x3>(dl[0], dh[0], dacc, b.sel1); dw_bias_mfma<Bf16x3>(dl[1], dh[1], dacc, b.sel1); dw_bias_mfma<Bf16x3>(dl[2], dh[2], dacc, b.sel1);
        }
    }
}

// ---- soft lockstep of the tiles of a split (k_dw_bf16's, round 3).  They walk the same k-steps and share every operand byte through
// their XCD's L2 (G between the h blocks, hidden between the v blocks); nothing else holds them together, and a tile that falls behind
// finds its lines evicted and becomes its own HBM stream — counted: 1.85x the algorithmic traffic on bf16, 83 GB fetched for 39.5 GB of
// operands on f16x2 (profiles/r04_f16x2_hbm_traffic_pmc.txt, first pass).  Every PERIOD steps a tile publishes its step count and looks
// at its right-hand neighbour's in the ring of the split's tiles (one coherent scalar load, issued a look before its value is used); a
// tile more than LAG steps ahead of that neighbour naps.  Bounded: after DW_NAPS naps without the neighbour catching up (a partner that
// is not resident) the tile stops looking, so every wave reaches the end whatever the others do.
// The wait in front of the comparison names nb_at, so that no copy of the register made before the data arrived can be what the
// comparison reads (round-4 advice: a stale value only mis-paces, but makes timing and traffic depend on the compiler's register copies).
// k_dw_bf16 (lag 3 stages, a look every 4th stage, a count that runs over all ranges of the split, 0x7fffffff stored at the end) keeps its
// own text without that wait: as this struct's look() its nap loop was unrolled into the k loop (profiles/dw_toolkit_isa.txt).
template <int LAG, int PERIOD> struct DwLockstep {
    int *prog;      // the progress words of the split's tiles
    const int *nb;  // the right-hand neighbour's word
    int nb_at;      // the neighbour's step count as of the last look
    bool sync_on;
    __device__ inline void init(int *dw_prog, int split, int tile, int tiles)
    {
        prog = dw_prog ? dw_prog + split * 16 : nullptr;
        sync_on = prog != nullptr && tiles > 1 && tiles <= 16;
        nb = prog ? prog + (tile + 1 < tiles ? tile + 1 : 0) : nullptr;
        nb_at = 0x7fffffff;
    }
    __device__ inline void look(int mine, int tile, int tid)  // (wave-uniform)
    {
        constexpr int DW_NAPS = 256;
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(nb_at) :: "memory");
        int naps = 0;
        while (sync_on && nb_at + LAG + PERIOD < mine) {  // (+PERIOD: the value is one look old)
            if (++naps > DW_NAPS) { sync_on = false; break; }
            __builtin_amdgcn_s_sleep(4);
            asm volatile("s_load_dword %0, %1, 0x0 glc\n\ts_waitcnt lgkmcnt(0)" : "=s"(nb_at) : "s"(nb) : "memory");
        }
        if (sync_on) {
            if (tid == 0) __hip_atomic_store(prog + tile, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (one more outstanding store only makes the counted waits stricter)
            asm volatile("s_load_dword %0, %1, 0x0 glc" : "=s"(nb_at) : "s"(nb) : "memory");  // used at the next look
        }
    }
};

// ---- the ring driver of the 4-stage kernels: ONE pipeline run over a split's nks k-steps.  dma_stage(ks, st) issues this wave's DMA
// pieces of k-step ks into ring stage st (prologue: NST - 1 stages ahead); kstep(Int<ST>, ks) is k-step ks on ring stage ST = ks % NST —
// its counted wait for the stage, dw_kstep2, and inside it the pieces of k-step ks + NST - 1.  The loop is unrolled by NST with a look at
// the lockstep in front of stage 0.
template <class LS, class KStep, class DmaStage>
__device__ inline void dw_ring(int nks, LS &ls, int tile, int tid, const KStep &kstep, const DmaStage &dma_stage)
{
    int runs = 1;  // ONE pipeline run; the count is opaque to hipcc, which keeps the accumulators in their registers across a loop of
    asm volatile("" : "+s"(runs));  // runs (the per-range walk's shape) and spills all 256 of them around a straight-line run
    for (int run = 0; run < runs; ++run) {
        dma_stage(0, 0);
        dma_stage(1, 1);
        dma_stage(2, 2);
        for (int ks = 0;;) {
            if (ks >= nks) break;
            ls.look(ks, tile, tid);
            kstep(Int<0>{}, ks); ++ks;
            if (ks >= nks) break;
            kstep(Int<1>{}, ks); ++ks;
            if (ks >= nks) break;
            kstep(Int<2>{}, ks); ++ks;
            if (ks >= nks) break;
            kstep(Int<3>{}, ks); ++ks;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the over-issued DMAs before the ring
        lds_barrier();                                  // is refilled / the kernel exits
    }
}

// ---- the walk of the live-row table (k_dw_table: tab[b] = first granule of utterance b's live range, tab[B + 1 + b] = live granules
// before it, tab[2B + 1] = their total).  A split's share [g_lo, g_hi) of the live granules is walked utterance by utterance:
// run(first row, granules) is one pipeline run over one live range (workgroup-uniform)
struct DwShare { const long *tab; int B; long nlive, g_lo, g_hi; };
__device__ inline DwShare dw_share(const long *tab, int B, int split, int n_split)
{
    DwShare s;
    s.tab = tab; s.B = B;
    s.nlive = tab[2 * B + 1];
    s.g_lo = s.nlive * split / n_split; s.g_hi = s.nlive * (split + 1) / n_split;
    return s;
}
template <class Run> __device__ inline void dw_walk_ranges(const DwShare &s, const Run &run)
{
    const long *tab = s.tab;
    const int B = s.B;
    int ub = 0;
    while (ub + 1 < B && tab[B + 1 + ub + 1] <= s.g_lo) ++ub;  // utterance holding live granule g_lo
    for (long gq = s.g_lo; gq < s.g_hi; ++ub) {
        const long cum0 = tab[B + 1 + ub], cum1 = ub + 1 < B ? tab[B + 1 + ub + 1] : s.nlive;
        const long ge = cum1 < s.g_hi ? cum1 : s.g_hi;
        if (ge <= gq) continue;
        const long row_first = (tab[ub] + (gq - cum0)) * DW_GRAN, ngran = ge - gq;
        gq = ge;
        run(row_first, ngran);
    }
}

// ---- epilogue: partial slab [split][V,H]; bias partial [split][V].  Wave tile at (v0, h0); accumulator register r of tile (qm,qn):
// v = v0 + 32qm + (r&3) + 8(r>>2) + 4half, h = h0 + 32qn + (lane&31).  GUARD: rows / columns beyond V / H are not stored (without it
// the column is added in 64 bits: the addresses of a row's four tiles differ by immediates).  RESCALE: the accumulators hold a power of
// two times dW (f16x2: g_scale x 2^14; X3Args::dw_rescale, db_rescale); a format without scales multiplies by nothing.
// db: column k of the selector products (lanes k / 32+k) holds M tile bsel0 + 2k, k = 0 (two_b: 0, 1)
template <bool GUARD, bool RESCALE>
__device__ inline void dw_store_w(float *slab_w, int split, int H, int V, int v0, int h0, int lane, const f32x16 (&acc)[4][4], float rw)
{
    const int half = lane >> 5;
    float *sw = slab_w + (long)split * V * H;
#pragma unroll
    for (int qm = 0; qm < 4; ++qm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int v = v0 + 32 * qm + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (!GUARD || v < V) {
#pragma unroll
                for (int qn = 0; qn < 4; ++qn) {
                    const int h = h0 + 32 * qn + (lane & 31);
                    if (!GUARD || h < H) sw[GUARD ? (long)v * H + h : (long)v * H + h0 + 32 * qn + (lane & 31)] = RESCALE ? acc[qm][qn][r] * rw : acc[qm][qn][r];
                }
            }
        }
}
template <class F, bool GUARD>
__device__ inline void dw_store(const X3Args &a, int split, int v0, int h0, int lane, const f32x16 (&acc)[4][4], const f32x16 &dacc,
                                bool do_b, bool two_b, int bsel0)
{
    constexpr bool RESCALE = F::SCALED;
    const int half = lane >> 5, V = a.V;
    dw_store_w<GUARD, RESCALE>(a.slab_w, split, a.H, V, v0, h0, lane, acc, RESCALE ? a.dw_rescale : 1.f);
    if (do_b && (lane & 31) < (two_b ? 2 : 1)) {
        const int m = bsel0 + 2 * (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int v = v0 + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (!GUARD || v < V) a.slab_b[(long)split * V + v] = RESCALE ? dacc[r] * a.db_rescale : dacc[r];
        }
    }
}
