// x3.hip — the RNNT_DTYPE_F32_BF16X3 route: fp32-accurate arithmetic on the bf16 matrix pipes.
//
// Same path and same boundary as the fp32 route (reference rnnt/joint.py:32-39 + torchaudio rnnt_loss
// called at rnnt/model.py:35-41 + their autograd; fp32 tensors in and out, 1e-4 parity bar), but the
// three GEMMs run on v_mfma_f32_32x32x16_bf16 instead of v_mfma_f32_32x32x2_f32 (1/16 of its rate):
// every fp32 operand x is split ONCE, where it is produced, into three bf16 pieces
//       x = hi + mid + lo     hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)   (RNE each)
// (8 + 8 + 8 significant bits: the sum is x to 2^-25 relative) and a product a.b is evaluated as the
// six bf16 products  ah.bh + ah.bm + am.bh + am.bm + ah.bl + al.bh  accumulated in fp32 by the MFMA —
// the terms dropped are <= 2^-24 |a.b|.  Measured against fp64 (tools/bf16x3_accuracy.py): rms error
// 4.4e-8 of the logit scale, against 1.2e-7 for the fp32 MFMA's 512-long fp32 accumulation chain.
// Logits, log-softmax, the lattice, the gradient coefficients and every reduction are the fp32 / fp64
// code of the fp32 route (lattice.hip); only the operands of the matrix products are split.
//
// Data (workspace):
//   hidden  3 planes bf16 [3][rows_alloc][H]      written by the forward tile's prologue
//   logits  fp32 [rows_alloc][V]                  forward -> k_dhidden_x3
//   G       hi and mid planes IN PLACE of the logits: the 128 bytes of every 32-wide chunk of a logits
//           row become [32 x hi | 32 x mid]; lo plane bf16 [rows_alloc][V] beside it (workspace `g_lo`)
//   W       re-packed per call into MFMA-fragment order, 3 planes (forward: wpack_fwd, dHidden: wpack_dh)
//
// MFMA operand maps (cdna_hip_programming.md §3): lane l = (r = l&31, h = l>>5) holds A[row r][k = 8h+j]
// and B[k = 8h+j][col r], j = 0..7; C/D: col = l&31, row = (reg&3) + 8*(reg>>2) + 4*(l>>5).
// Every kernel here is 4 waves (one per SIMD) with 256 accumulator registers per wave, hand-pipelined
// around long MFMA streams (96 MFMAs = 3072 matrix-pipe cycles per 16-deep k-step), like the fp32 route's.
#include "split_dhidden.hpp"
#include "split_dw.hpp"

// The plain producers and the W packs are split_common.hpp's, at the bf16x3 format (no scales: the pointer is null and unread)
void launch_x3_make_hidden(const X3Args &a, hipStream_t st) { launch_split_make_hidden<Bf16x3>(a, st); }
void launch_x3_split_g(const X3Args &a, hipStream_t st) { launch_split_g<Bf16x3>(a, st); }
void launch_x3_zero_padding(const X3Args &a, int what, hipStream_t st) { launch_split_zero_padding<Bf16x3>(a, what, st); }
void launch_x3_pack_w(const X3Args &a, hipStream_t st) { launch_split_pack_w<Bf16x3>(a, nullptr, st); }
size_t x3_wpack_fwd_bytes(int H, int V) { return split_wpack_fwd_bytes<Bf16x3>(H, V); }
size_t x3_wpack_dh_bytes(int H, int V) { return split_wpack_dh_bytes<Bf16x3>(H, V); }

// ---------------------------------------------------------------------------------------
// k_dw_x3: dW[v,h] = sum_c G[c,v] hidden[c,h] (split-K slabs), db[v] = sum_c G[c,v].
// 4 waves = 2 (M) x 2 (N), workgroup tile 256 v x 256 h, wave 128 x 128 = 16 accumulator tiles (256
// registers).  Both operands are row-major with K (the cell) as the ROW, three planes each:
//  * HBM -> LDS by LDS-DMA (no VGPRs), ring of 3 stages of 16 cells x (256 v + 256 h) x 3 planes = 48 KiB;
//    wave w fills operand tile w (w = 0,1: the two 128-column halves of the G tile, 2,3: of the hidden
//    tile), 12 DMAs of 1 KiB (4 rows x 256 B) per stage;
//  * LDS -> VGPR by ds_read_b64_tr_b16 (hardware 4x16 transpose read, cdna_hip_programming.md T10): two
//    reads give a lane its 8 consecutive cells of one column = the MFMA fragment;
//  * tile image (b) of T10: 256-byte rows, 16-byte chunk ch of row r at 16*(ch ^ swz(r)),
//    swz(r) = ((r&3)<<2) | ((r>>2)&3); the DMA writes LDS linearly, so the swizzle is applied on the
//    SOURCE side: LDS chunk position p of row r is fetched from global chunk p ^ swz(r).
// One k-step = 16 cells = 6 products x 16 tiles = 96 MFMAs (3072 matrix-pipe cycles) against 48 KiB staged.
// Per k-step: counted vmcnt + one barrier publish stage ks (and prove stage ks-1 read by every wave), the
// DMAs of stage ks+2 go into the slot of ks-1 threaded through the MFMAs, fragment reads run one product
// ahead of their MFMAs.  Product order ah.bh, am.bh, am.bm, ah.bm, al.bh, ah.bl keeps at most five of the
// six 16-register fragment sets live.
// ---------------------------------------------------------------------------------------
typedef DwRing<Bf16x3, 3> XW;  // ring of 3 stages: the DMAs of stage ks + 2 are issued during k-step ks; 3 x 12 KiB per operand tile
// a range's last k-step issues the pieces of the two k-steps behind it: 32 rows past the range's end, at most that far past rows_pad
static_assert((XW::NST - 1) * DW_ROWS <= DW_ROWS_PAST, "read-ahead of the ring past the last live row");

__global__ __launch_bounds__(256, 1) void k_dw_x3(X3Args a)
{
    // LDS: 4 operand tiles (wave w fills tile w: 0,1 = the 128-column halves of the G tile, 2,3 = of the hidden
    // tile), each a ring [stage][plane][16 x 256 B]: every fragment read of a wave is one of 8 base registers
    // plus an immediate (stage, plane) offset < 64 KiB — no address arithmetic in the loop (one wave per SIMD
    // issues ~1 instruction per 4-5 cycles: every instruction between two MFMAs counts)
    extern __shared__ __attribute__((aligned(1024))) char s_ring[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const DwTile tl = dw_tile(blockIdx.x, wave, a.H, a.V, a.n_split);
    const DwShare share = dw_share(a.dw_tab, a.B, tl.split, a.n_split);
    X_CLOCK_STAMP(128 + 104);

    f32x16 acc[4][4], dacc;
    dw_zero(acc, dacc);
    DwBias bias;
    const int bsel0 = dw_bias_setup<Bf16x3>(bias, tl.n_hblk, tl.hb, tl.wn, lane);

    if (share.g_hi > share.g_lo) {
        // ---- DMA source of this wave's operand tile; DMA i (0..3) of a plane's 16 rows: rows 4i .. 4i+3 of the stage's buffer
        const bool is_g = wave < 2;
        DwSource<Bf16x3> src;
        dw_source(src, a, is_g, dw_col0(is_g, is_g ? tl.vb : tl.hb, wave & 1, a.H, a.V));
        int soff[3][4];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int i = 0; i < 4; ++i) soff[p][i] = dw_soff(lane, i, 4 * i, src.rstride[p], is_g && p < 2, 0);
        long row_first = 0;  // first cell of the range being walked
        // ---- fragment bases: A from operand tile wm, B from operand tile 2 + wn; db: the M tile(s) this wave sums
        const int lds0 = (int)(size_t)(lds_vptr)s_ring;
        int abase[4][2], bbase[4][2];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int sec = 0; sec < 2; ++sec) {
                abase[m][sec] = dw_frag_addr<XW>(lds0, tl.wm, m, sec, lane);
                bbase[m][sec] = dw_frag_addr<XW>(lds0, 2 + tl.wn, m, sec, lane);
            }
        dw_bias_bases<XW>(bias, lds0, tl.wm, bsel0, lane);

        // one k-step on ring stage ST (compile-time: every LDS offset is an immediate)
        auto kstep = [&](auto st_c, long ks) {
            constexpr int ST = decltype(st_c)::value, DST = (ST + 2) % 3;
            // the 16 rows of stage ks+2 as three raw buffers
            __amdgpu_buffer_rsrc_t rs[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) rs[p] = dw_rows_rsrc(src.pbase[p], row_first + (ks + 2) * DW_ROWS, src.rstride[p], DW_ROWS);
            auto dma_piece = [&](auto n_c) {  // piece n of stage ks+2 -> ring stage DST: plane n>>2, rows 4(n&3)..
                constexpr int n = decltype(n_c)::value, p = n >> 2, i = n & 3;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs[p], (lds_vptr)(s_ring + wave * XW::TILE + DST * XW::STAGE + p * XW::PLANE + 1024 * i),
                                                         16, soff[p][i], 0, 0, 0);
            };
            // stage ks landed (the 12 younger pieces of ks+1 may still fly); the k-step's barrier: every wave is past its
            // reads of stage ks-1, whose ring stage the pieces refill
            static_assert(XW::WAIT == 12, "the counted wait");
            asm volatile(RNNT_VMCNT(12) ::: "memory");
            dw_kstep3<XW, ST>(acc, dacc, abase, bbase, bias, a.ablate, dma_piece);
        };
        auto dma_stage = [&](long ks, int st) {  // pipeline prologue: all 12 pieces of stage ks
#pragma unroll
            for (int n = 0; n < XW::ND; ++n) {
                const int p = n >> 2, i = n & 3;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(dw_rows_rsrc(src.pbase[p], row_first + ks * DW_ROWS, src.rstride[p], DW_ROWS),
                                                         (lds_vptr)(s_ring + wave * XW::TILE + st * XW::STAGE + p * XW::PLANE + 1024 * i),
                                                         16, soff[p][i], 0, 0, 0);
            }
        };
        dw_walk_ranges(share, [&](long first, long ngran) {  // one pipeline run per live range
            __builtin_assume(ngran > 0);  // (dw_walk_ranges hands over non-empty ranges; said here, the k loop keeps its unsigned exit compares: do not delete)
            const long nks = (DW_GRAN / DW_ROWS) * ngran;  // 16-cell k-steps of this range
            row_first = first;
            dma_stage(0, 0);
            dma_stage(1, 1);
            for (long ks = 0;;) {  // the ring stage of a k-step is ks % 3: unrolled by 3
                if (ks >= nks) break;
                kstep(Int<0>{}, ks); ++ks;
                if (ks >= nks) break;
                kstep(Int<1>{}, ks); ++ks;
                if (ks >= nks) break;
                kstep(Int<2>{}, ks); ++ks;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the over-issued DMAs before the ring
            lds_barrier();                                  // is refilled / the kernel exits
        });
    }

    X_CLOCK_STAMP(128 + 106);
    dw_store<Bf16x3, true>(a, tl.split, tl.v0, tl.h0, lane, acc, dacc, bias.do_b, bias.two_b, bsel0);
}

void launch_dw_x3(const X3Args &a, hipStream_t st)
{
    launch_dw_table(a.logit_lens, a.B, a.T, a.U1, DW_GRAN, a.dw_tab, st);
    const int tiles = ((a.V + 255) / 256) * ((a.H + 255) / 256);
    static LdsOptIn lds_opt_in;
    lds_opt_in.raise(4 * XW::TILE, k_dw_x3);
    hipLaunchKernelGGL(k_dw_x3, dim3(tiles * a.n_split), dim3(256), 4 * XW::TILE, st, a);
}


// ---------------------------------------------------------------------------------------
// k_joint_fwd_x3: hidden = tanh(enc + pred) split into its planes (tile prologue), logits = hidden . W^T + bias
// (fp32, stored), log-softmax statistics and the two log-probs per lattice cell (as the fp32 route's forward).
// Tile = 128 consecutive cells; 4 waves = 2 (M) x 2 (N), wave tile 64 cells x 256 columns = 16 accumulator tiles
// (256 registers); a pass = 512 logits columns, passes run back to back over one linear k-step sequence.
//  * A (hidden planes, written by this workgroup's prologue) and B (packed W) of a k-step both arrive by LDS-DMA:
//    12 KiB + 48 KiB into 2-slot rings (3 + 12 DMAs per wave and k-step), A's image = MFMA fragment order
//    [M tile][plane][lane] (a lane fetches its own 16 bytes: row = its cell, k = 16c + 8*(lane>>5) ..);
//  * per k-step ONE barrier (the DMAs are the only memory operations in flight: vmcnt(0)), then fragment
//    reads and 6 products x 16 MFMAs with the next k-step's DMAs threaded through the first blocks;
//  * pass end: bias rode in the accumulators' initial value; logits leave as 16 bytes per lane (4 adjacent
//    columns; a wave-instruction writes 512 contiguous bytes of two rows); per-lane running (max, sum exp) of every
//    row slot live in 64 registers and are combined across lanes and the two column halves once per tile.
// grid = rows_alloc / 128 workgroups.  Requires H % 128 == 0, V % 128 == 0.
// ---------------------------------------------------------------------------------------
#define XF_WSLOT 49152
#define XF_ASLOT 12288
#ifdef RNNT_STAMPS
// Diagnostic build only (-DRNNT_STAMPS): s_memtime stamps of workgroup 0, wave XS_WAVE, k-steps 8..23 of its first tile:
// debug[(step-8)*8 + slot]
#ifndef XS_WAVE
#define XS_WAVE 0
#endif
#define XSTAMP(slot)                                                                                        \
    do {                                                                                                    \
        if (a.debug && blockIdx.x == 0 && wave == XS_WAVE && lane == 0 && it == 1 && cs >= 8 && cs < 24) {   \
            unsigned long long t_;                                                                          \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                       \
            a.debug[(cs - 8) * 8 + (slot)] = t_;                                                            \
        }                                                                                                   \
    } while (0)
#define XESTAMP(k)                                                                                          \
    do {                                                                                                    \
        if (a.debug && blockIdx.x == 0 && wave == XS_WAVE && lane == 0 && it == 3) {                         \
            unsigned long long t_;                                                                          \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                       \
            a.debug[128 + (k)] = t_;                                                                        \
        }                                                                                                   \
    } while (0)
#else
#define XSTAMP(slot) do {} while (0)
#define XESTAMP(k) do {} while (0)
#endif
__global__ __launch_bounds__(256, 1) void k_joint_fwd_x3(X3Args a, const int ntiles)
{
    // [0, 96 KiB): W ring;  [96, 120 KiB): A ring;  then: s_den[128], s_part[2][128][2], s_next[2]
    extern __shared__ __attribute__((aligned(1024))) char s_fw[];
    float *s_den = (float *)(s_fw + 2 * XF_WSLOT + 2 * XF_ASLOT);
    float *s_part = s_den + 128;  // [wn][row][max, sum]
    int *s_next = (int *)(s_part + 512);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int i = lane & 31, half = lane >> 5;
    const int H = a.H, V = a.V, KC = H / 16, U1 = a.U1, T = a.T;
    const int npass = (V + 511) / 512;
    const int NS = npass * KC;  // k-steps of a tile
    const long cells = (long)a.B * T * U1;

    const int lds0 = (int)(size_t)(lds_vptr)s_fw;
    const int xa = lds0 + 2 * XF_WSLOT + (2 * wm) * 3072 + 16 * lane;  // A read: M tiles 2wm, 2wm+1: [slot][M tile][plane][lane]
    const int xw = lds0 + 2 * XF_WSLOT + wave * 3072 + 16 * lane;       // A write: M tile `wave` (this lane's own fragment slot)
    const int wb = lds0 + (8 * wn) * 1024 + 16 * lane;                 // W read: tiles 8wn .. 8wn+7 of each plane
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(a.wpack_fwd, 0, npass * KC * 49152, 0x00020000);
    const int wvo = lane * 16;

    // Persistent workgroups (one per CU: 120 KiB of LDS), tiles from one atomic counter, the next tile requested a
    // tile ahead.
#ifdef RNNT_STAMPS
    if (a.debug && blockIdx.x == 0 && tid == 0) {  // clock of this launch: core-clock ticks per 100 MHz reference tick
        unsigned long long t0_, r0_;
        asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0_), "=s"(r0_)::"memory");
        a.debug[128 + 100] = t0_; a.debug[128 + 101] = r0_;
    }
#endif
    if (tid == 0) s_next[0] = (int)atomicAdd(a.counter, 1u);
    __syncthreads();
    int tile = s_next[0];
    for (int it = 1; tile < ntiles; ++it) {
        if (tid == 0) s_next[it & 1] = (int)atomicAdd(a.counter, 1u);
        const long row0 = (long)tile * 128;
        // running (max, sum exp) of every row over the columns seen so far, per column half (wn): s_part[wn][row],
        // kept by the lanes 31 / 63 that end up with a row slot's wave-level statistics
        for (int k = tid; k < 256; k += 256) { s_part[2 * k] = RNNT_NEG_INF; s_part[2 * k + 1] = 0.f; }
        __syncthreads();  // s_next, s_part visible; every wave is past the previous tile's LDS reads
        const int next = s_next[it & 1];
        // A tile entirely in the time steps past one utterance's length: its logits are never read (k_dhidden_x3
        // zero-fills the G rows of dead tiles itself), but its hidden rows must be finite (k_dw_x3 multiplies them by
        // zeros): such a tile runs the production of its first pass WITHOUT the MFMAs (DEAD below).
        bool dead;
        {
            const long per = (long)T * U1, c_last = row0 + 127;
            const long b_first = row0 / per;
            dead = c_last < cells && c_last / per == b_first && (row0 - b_first * per) / U1 >= len_t(a.logit_lens, (int)b_first, T);
        }

        // ---- hidden = tanh(enc + pred), produced per k-step IN FRAGMENT ORDER by the lane that owns the slot: lane
        // (i, half) of wave w holds row 32w + i, k = 16c + 8*half .. +7 of the MFMA A operand — 8 values from 2 x 32
        // bytes of enc and pred (small, cache-resident operands), split three ways, 16 bytes per plane into the LDS
        // ring of k-step c+1 (every wave reads its two M tiles from there) and, in the first pass, to the hidden
        // planes in memory for k_dw_x3.  The forward never re-reads hidden from memory: later passes produce it again
        // (~130 instructions per lane and k-step, threaded through the gaps of 96 MFMAs).
        const long prow = row0 + 32 * wave + i;
        const long pc_ = prow < cells ? prow : cells - 1;  // rows past the lattice (last tile): any valid cell, never stored
        const int pu = (int)(pc_ % U1);
        const long pbt = pc_ / U1;
        const int pt = (int)(pbt % T), pb = (int)(pbt / T);
        const float *ep = a.enc + (long)pb * a.enc_sb + (long)pt * a.enc_st + 8 * half;
        const float *pp = a.pred + ((long)pb * U1 + pu) * H + 8 * half;
        // (rows past the lattice produce — and store, unconditionally — the last cell's row again: the same bits to the
        // same place; hipcc counts vmcnt exactly only through unconditional memory operations)
        u32x4 *hdst = (u32x4 *)a.hidden + pc_ * (H / 8) + half;  // + 2c: this lane's 16 bytes of k-step c; planes `ps` apart
        const long ps = a.plane_stride / 8;
        struct Opd { f32x4 e0, e1, p0, p1; };
        struct Prod { f2 w[4]; float ra, rb; u32x4 ph, pm, pl; };
        auto op_load = [&](Opd &o, int kcs) {  // operands of k index kcs (inside a pass)
            o.e0 = *(const f32x4 *)(ep + 16 * kcs); o.e1 = *(const f32x4 *)(ep + 16 * kcs + 4);
            o.p0 = *(const f32x4 *)(pp + 16 * kcs); o.p1 = *(const f32x4 *)(pp + 16 * kcs + 4);
        };
        // pieces 0-7: tanh of the 4 pairs (fast_tanh2's arithmetic: exp2 half, reciprocal half); 8-15: the 3-way split
        // of each pair (hi, then mid + lo); 16: the three ring writes
        auto prod_piece = [&](Prod &P, const Opd &o, int slot, int k) {
            if (k < 8) {
                const int j = k >> 1;
                if (!(k & 1)) {
                    const f32x4 &e = j < 2 ? o.e0 : o.e1, &pv = j < 2 ? o.p0 : o.p1;
                    const int q = 2 * (j & 1);
                    const f2 x = {e[q] + pv[q], e[q + 1] + pv[q + 1]};
                    const f2 av = x * (2.0f * RNNT_LOG2E);
                    P.w[j] = f2{__builtin_amdgcn_exp2f(av[0]), __builtin_amdgcn_exp2f(av[1])};
                } else {
                    const f2 ex = P.w[j] + 1.0f;
                    const f2 rr = {__builtin_amdgcn_rcpf(ex[0]), __builtin_amdgcn_rcpf(ex[1])};
                    P.w[j] = 1.0f - 2.0f * rr;
                }
            } else if (k < 16) {
                const int j = (k - 8) >> 1;
                if (!(k & 1)) {
                    const unsigned hh = pack_bf16(P.w[j][0], P.w[j][1]);
                    P.ph[j] = hh;
                    P.ra = P.w[j][0] - bf16_lo(hh); P.rb = P.w[j][1] - bf16_hi(hh);
                } else {
                    const unsigned mm = pack_bf16(P.ra, P.rb);
                    P.pm[j] = mm;
                    P.pl[j] = pack_bf16(P.ra - bf16_lo(mm), P.rb - bf16_hi(mm));
                }
            } else {
                const int dst = xw + slot * XF_ASLOT;
                asm volatile("ds_write_b128 %0, %1" :: "v"(dst), "v"(P.ph) : "memory");
                asm volatile("ds_write_b128 %0, %1 offset:1024" :: "v"(dst), "v"(P.pm) : "memory");
                asm volatile("ds_write_b128 %0, %1 offset:2048" :: "v"(dst), "v"(P.pl) : "memory");
            }
        };
        auto hid_store = [&](const Prod &P, int kcs) { hdst[2 * kcs] = P.ph; hdst[2 * kcs + ps] = P.pm; hdst[2 * kcs + 2 * ps] = P.pl; };
        // piece n (0..11) of this wave's share of W k-step cs -> ring slot cs & 1
        auto wdma = [&](int cs, int n) {  // raw-buffer form: scalar base and offsets, one constant per-lane offset register
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (lds_vptr)(s_fw + (cs & 1) * XF_WSLOT + (wave * 12 + n) * 1024), 16, wvo,
                                                     (cs * 48 + wave * 12 + n) * 1024, 0, 0);
        };

        if (dead) {  // hidden rows only (finite values for k_dw_x3), no products
            for (int kc = 0; kc < KC; ++kc) {
                Opd o; Prod P;
                op_load(o, kc);
#pragma unroll
                for (int pc = 0; pc < 16; ++pc) prod_piece(P, o, 0, pc);
                hid_store(P, kc);
            }
            tile = next;
            continue;
        }

        f32x16 acc[2][8];
        auto acc_init = [&](int pass) {  // the bias of this lane's 2 x 4 adjacent columns of the pass
            const int c0 = 512 * pass + 256 * wn + 4 * i;
            const f32x4 b0 = c0 < V ? *(const f32x4 *)(a.bias + c0) : f32x4{0.f, 0.f, 0.f, 0.f};
            const f32x4 b1 = c0 + 128 < V ? *(const f32x4 *)(a.bias + c0 + 128) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int q = 0; q < 8; ++q)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[mt][q][r] = q < 4 ? b0[q] : b1[q - 4];
        };
        // pipeline prologue: W of k-step 0 by DMA; A of k-step 0 produced, stored, written to ring slot 0; operands of
        // k-step 1 requested
        Opd oset[2];  // operands of k-step cs+1 live in oset[(cs+1) & 1] during k-step cs (KC is even: the k loop is unrolled by 2)
        {
#pragma unroll
            for (int n = 0; n < 12; ++n) wdma(0, n);
            Opd o; Prod P;
            op_load(o, 0);
            op_load(oset[1], KC > 1 ? 1 : 0);
#pragma unroll
            for (int pc = 0; pc < 17; ++pc) prod_piece(P, o, 0, pc);
            hid_store(P, 0);
        }

        int cs = 0;
        // one pass; STORE: the first — the produced planes also go to memory.  Two straight-line instantiations, the
        // first pass outside the loop over the others (a branch between two k loops, like a conditional accumulator
        // re-initialisation inside one, makes hipcc carry the 256 accumulator registers through VGPR phis and spill)
        auto run_pass = [&](auto store_c, const int pass) {
          XESTAMP(32 * pass + 0);
          acc_init(pass);
          // one k-step; STORE: first pass — the produced planes also go to memory.  Two straight-line instantiations
          // (hipcc counts vmcnt exactly only through straight-line code).
          constexpr bool STORE = decltype(store_c)::value != 0;
          for (int kc0 = 0; kc0 < KC; kc0 += 2)
#pragma unroll
          for (int par = 0; par < 2; ++par, ++cs) {
            const int kc = kc0 + par;
            // W of k-step cs landed (this wave's share).  vmcnt retires in order: behind a k-step's DMAs come only its
            // 4 operand loads and (first pass) 3 hidden stores, which stay in flight; the first k-step of a pass also
            // follows the previous pass's logits stores
            XSTAMP(0);
            if (kc == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            // (behind the k-step's last DMA (block 2) come only the first pass's 3 hidden stores; the 4 operand loads sit
            // between the two DMA groups and retire with them)
            else if (STORE) asm volatile(RNNT_VMCNT(3) ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            XSTAMP(1);
            lds_barrier();  // publishes W slot and A slot of k-step cs; every wave is past its reads of cs-1
            XSTAMP(2);
            const int ws = wb + (cs & 1) * XF_WSLOT, xs = xa + (cs & 1) * XF_ASLOT;
            // the next k-step (past the end: its own, never read) and the one after (operand loads)
            const int csn = cs + 1 < NS ? cs + 1 : cs, kcn = kc + 1 < KC ? kc + 1 : 0, kcnn = kcn + 1 < KC ? kcn + 1 : 0;
            const Opd &ocur = oset[(par + 1) & 1];  // operands of k-step cs+1 (requested during the previous k-step)
            Opd &onext = oset[par & 1];             // refilled with those of k-step cs+2
            Prod P;
            u32x4 af[2][3], bf[8], bn[8];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(af[mt][p]) : "v"(xs), "n"(mt * 3072 + p * 1024));
#pragma unroll
            for (int q = 0; q < 8; ++q) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bf[q]) : "v"(ws), "n"(q * 1024));
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(af[0][0]), "+v"(af[0][1]), "+v"(af[0][2]), "+v"(af[1][0]), "+v"(af[1][1]), "+v"(af[1][2]),
                           "+v"(bf[0]), "+v"(bf[1]), "+v"(bf[2]), "+v"(bf[3]), "+v"(bf[4]), "+v"(bf[5]), "+v"(bf[6]), "+v"(bf[7])
                         :: "memory");
            auto block = [&](auto pa_c, const u32x4 (&bcur)[8], u32x4 (&bnext)[8], auto nb_c, auto d0_c, auto pb_c) {
                constexpr int PA = decltype(pa_c)::value, NB = decltype(nb_c)::value, D0 = decltype(d0_c)::value, PB = decltype(pb_c)::value;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    acc[0][q] = mfma_bf16(af[0][PA], bcur[q], acc[0][q]);
                    acc[1][q] = mfma_bf16(af[1][PA], bcur[q], acc[1][q]);
                    if (NB >= 0) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bnext[q]) : "v"(ws), "n"((NB < 0 ? 0 : NB) * 16384 + q * 1024));
                    // D0: the tag of the block's W DMA pieces of k-step cs+1 (8: pieces 0-5, -2: pieces 6-11, else none); PB: production pieces PB+q of A's k-step cs+1
                    // six DMA pieces each in blocks 1 and 2, none beside block 0's eight fragment reads
                    // (round 3 had 8 + 4 in blocks 0 and 1: 36.5 -> 35.9 ms on one box)
                    if (D0 == 8 && q < 6) wdma(csn, q);
                    if (D0 == -2 && q < 6) wdma(csn, 6 + q);
                    if (PB >= 0 && PB + q < 17) prod_piece(P, ocur, (cs + 1) & 1, (PB < 0 ? 0 : PB) + q);
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            // every fragment read is issued at least a block (16 MFMAs) before the wait that covers it
            XSTAMP(3);
            block(Int<0>{}, bf, bn, Int<1>{}, Int<-1>{}, Int<-1>{});   // ah.bh + reads of W mid
            block(Int<1>{}, bf, bn, Int<-1>{}, Int<8>{}, Int<-1>{});   // am.bh + DMA 0-5
            XSTAMP(4);
            op_load(onext, kcnn);  // operands of k-step cs+2: behind the DMAs (they are needed a whole k-step from now)
            block(Int<2>{}, bf, bf, Int<-1>{}, Int<-2>{}, Int<0>{});   // al.bh + DMA 6-11 (D0 = -2: the tag of this block) + A(cs+1): tanh pieces
            LDS_WAIT8(bn);
            block(Int<0>{}, bn, bf, Int<2>{}, Int<-1>{}, Int<8>{});    // ah.bm + reads of W lo (into the hi registers), A(cs+1): split pieces
            XSTAMP(5);
            block(Int<1>{}, bn, bn, Int<-1>{}, Int<-1>{}, Int<16>{});  // am.bm + A(cs+1): ring writes
            if (STORE) hid_store(P, kcn);  // (the youngest memory operations of the k-step; the pass's last k-step re-stores k-step 0)
            LDS_WAIT8_BUT(bf, 3);           // the three ring writes above may still fly
            block(Int<0>{}, bf, bf, Int<-1>{}, Int<-1>{}, Int<-1>{});  // ah.bl
            XSTAMP(6);
            (void)kcn;
          }
          // pass complete: store the logits, update the statistics.  V % 128 == 0: a lane's two 4-column groups exist
          // or not for the whole wave.  The row loop is ONE basic block per case; the store address is a scalar row
          // pointer + one 32-bit per-lane offset.
          XESTAMP(32 * pass + 1);
          {
            const int cw = 512 * pass + 256 * wn;
            const unsigned lane_off = (unsigned)(((4 * half) * V + 4 * i) * 4);
            char *tile_base = (char *)(a.logits + row0 * V + cw);
            auto epilogue = [&](auto both_c) {
                constexpr bool BOTH = decltype(both_c)::value != 0;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        // accumulator reads spelled as (volatile) asm: they stay here, one row slot at a time — left to
                        // hipcc, all 256 v_accvgpr_read are hoisted in front of the first store and spilled
                        f32x4 o0, o1;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            float x0, x1;
                            asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(x0) : "a"(acc[mt][q][r]));
                            asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(x1) : "a"(acc[mt][4 + q][r]));
                            o0[q] = x0; o1[q] = x1;
                        }
                        char *rowp = tile_base + (long)(32 * (2 * wm + mt) + (r & 3) + 8 * (r >> 2)) * V * 4;  // wave-uniform
                        __builtin_nontemporal_store(o0, (f32x4 *)(rowp + lane_off));
                        if (BOTH) __builtin_nontemporal_store(o1, (f32x4 *)(rowp + lane_off + 512));
                        // the row slot's (max, sum exp) over this wave's 128 / 256 columns of the pass: 8 values per
                        // lane, then the 32 lanes of the half on the DPP crossbar
                        float m8 = fmaxf(fmaxf(o0[0], o0[1]), fmaxf(o0[2], o0[3]));
                        if (BOTH) m8 = fmaxf(m8, fmaxf(fmaxf(o1[0], o1[1]), fmaxf(o1[2], o1[3])));
                        const float M = half_max_dpp(m8, half);
                        const float nm2 = -M * RNNT_LOG2E;
                        float e = (__builtin_amdgcn_exp2f(fmaf(o0[0], RNNT_LOG2E, nm2)) + __builtin_amdgcn_exp2f(fmaf(o0[1], RNNT_LOG2E, nm2))) +
                                  (__builtin_amdgcn_exp2f(fmaf(o0[2], RNNT_LOG2E, nm2)) + __builtin_amdgcn_exp2f(fmaf(o0[3], RNNT_LOG2E, nm2)));
                        if (BOTH)
                            e += (__builtin_amdgcn_exp2f(fmaf(o1[0], RNNT_LOG2E, nm2)) + __builtin_amdgcn_exp2f(fmaf(o1[1], RNNT_LOG2E, nm2))) +
                                 (__builtin_amdgcn_exp2f(fmaf(o1[2], RNNT_LOG2E, nm2)) + __builtin_amdgcn_exp2f(fmaf(o1[3], RNNT_LOG2E, nm2)));
                        const float S_ = half_sum_dpp(e, half);  // lanes 31 / 63 hold the sums
                        if (i == 31) {
                            float *sp = s_part + (wn * 128 + 32 * (2 * wm + mt) + (r & 3) + 8 * (r >> 2) + 4 * half) * 2;
                            const float m_o = sp[0], s_o = sp[1];
                            const float mn = fmaxf(m_o, M);
                            sp[0] = mn;
                            sp[1] = s_o * __builtin_amdgcn_exp2f((m_o - mn) * RNNT_LOG2E) + S_ * __builtin_amdgcn_exp2f((M - mn) * RNNT_LOG2E);
                        }
                        __builtin_amdgcn_sched_barrier(0);  // one row slot at a time
                        if ((r & 7) == 7) XESTAMP(32 * pass + 2 + 2 * mt + (r >> 3));
                    }
            };
            if (cw + 128 < V) epilogue(Int<1>{});
            else if (cw < V) epilogue(Int<0>{});
          }
          XESTAMP(32 * pass + 6);
        };
        run_pass(Int<1>{}, 0);
        for (int pass = 1; pass < npass; ++pass) run_pass(Int<0>{}, pass);

        XESTAMP(96);
        // ---- log-softmax denominators: the two column halves (wn) of every row
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        XESTAMP(97);
        __syncthreads();  // every logits / hidden store of the workgroup has left its wave; s_part complete
        if (tid < 128) {
            const float m0 = s_part[tid * 2], s0 = s_part[tid * 2 + 1];
            const float m1 = s_part[(128 + tid) * 2], s1 = s_part[(128 + tid) * 2 + 1];
            const float M = fmaxf(m0, m1);
            const float S_ = s0 * __builtin_amdgcn_exp2f((m0 - M) * RNNT_LOG2E) + s1 * __builtin_amdgcn_exp2f((m1 - M) * RNNT_LOG2E);
            s_den[tid] = M + __logf(S_);
        }
        __syncthreads();
        // thread = (row = tid & 127, which = tid >> 7): logit[blank] / logit[label] of the row, read through L2
        // (agent-scope loads bypass the CU's vector L1; the stores above are complete: vmcnt(0) + barrier)
        {
            const int row = tid & 127, which = tid >> 7;
            const long cell = row0 + row;
            if (cell < cells) {
                const int u = (int)(cell % U1);
                const long bt = cell / U1;
                const int t = (int)(bt % T), b = (int)(bt / T);
                const int Ub = len_u(a.target_lens, b, U1);
                if (t < len_t(a.logit_lens, b, T) && u <= Ub) {
                    const float den = s_den[row];
                    const float *lrow = a.logits + cell * V;
                    const long si = skew_index(b, t, u, a.D, U1);
                    if (which == 0) {
                        const float lb = __hip_atomic_load(lrow + a.blank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        a.denom_s[si] = den;
                        a.lpb_s[si] = lb - den;
                    } else {
                        float le = 0.f;
                        if (u < Ub) {
                            const int y = a.targets[(long)b * (U1 - 1) + u];
                            le = __hip_atomic_load(lrow + y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - den;
                        }
                        a.lpe_s[si] = le;
                    }
                }
            }
        }
        XESTAMP(98);
        tile = next;
    }
#ifdef RNNT_STAMPS
    if (a.debug && blockIdx.x == 0 && tid == 0) {
        unsigned long long t1_, r1_;
        asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1_), "=s"(r1_)::"memory");
        a.debug[128 + 102] = t1_; a.debug[128 + 103] = r1_;
    }
#endif
}

void launch_joint_fwd_x3(const X3Args &a, hipStream_t st)
{
    const int lds = 2 * XF_WSLOT + 2 * XF_ASLOT + 128 * 4 + 2 * 128 * 2 * 4 + 16;
    static LdsOptIn lds_opt_in;
    lds_opt_in.raise(lds, k_joint_fwd_x3);
    const long cells = (long)a.B * a.T * a.U1;
    const int ntiles = (int)((cells + 127) / 128);
    launch_fill32(a.counter, 0u, 4, st);  // tile counter of the persistent workgroups
    const int nwg = ntiles < a.n_cu ? ntiles : a.n_cu;  // one workgroup per CU (120 KiB of LDS each)
    hipLaunchKernelGGL(k_joint_fwd_x3, dim3((unsigned)nwg), dim3(256), lds, st, a, ntiles);
}


// ---------------------------------------------------------------------------------------
// k_dhidden_x3: G from the fp32 logits (exp2 + the two occupancy corrections, as the fp32 route), split
// into its three planes, stored in place (hi | mid over each 32-wide chunk of the logits row, lo beside)
// and multiplied: dHidden = G . W over 512 columns of H per launch; epilogue as the fp32 kernel:
// x (1 - hidden^2), sum over u -> dEnc slab, sum over t -> dPred slab.  Tile = 8 t x 16 u cells.
// 4 waves = 2 (M) x 2 (N), wave tile 64 cells x 256 columns = 16 accumulator tiles (256 registers).
//  * production: wave w turns M tile w (32 cells) into G: lane (cell i = l&31, half) owns the 8 vocabulary
//    entries 16c + 8*half .. +7 of its cell per k-step — exactly its slot of the MFMA A fragment — and drops
//    16 bytes per plane into the LDS exchange [2 slots][M tile][plane][lane]; logits requested 4 k-steps ahead
//    (register ring), G stored from the producer's registers (3 x 16 B per lane and k-step);
//  * W: one linear LDS-DMA copy of 48 KiB per k-step into a 2-slot ring (12 DMAs per wave);
//  * per k-step ONE barrier publishes W slot c and exchange slot c; behind it the wave first issues its
//    fragment reads, then produces G of step c+1 while they land (the production fills the LDS latency),
//    then runs 6 products x 16 MFMAs with the DMAs of W step c+1 threaded through the first ones (their
//    target slot was read during step c-1: every wave is past it).
// Product order keeps the 8 B fragments of one W plane live at a time: (ah,am,al).bh, (ah,am).bm, ah.bl.
// FIRST = false (H > 512: columns 512.., one launch per further 512): G's planes are read back from
// memory into the exchange instead of being produced; nothing is stored but the slabs.
// grid (n_ublk, ceil(T/8), B).  Requires V % 128 == 0, H % 128 == 0.
// ---------------------------------------------------------------------------------------
#define XG_BT 8
#define XG_BU 16
#define XG_WSLOT 49152   // one k-step of W: 3 planes x 16 tiles x 1 KiB
#define XG_XSLOT 12288   // one k-step of G fragments: 4 M tiles x 3 planes x 1 KiB
#ifdef RNNT_STAMPS
#define GXSTAMP(slot)                                                                                                  \
    do {                                                                                                               \
        if (FIRST && a.debug && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && wave == XS_WAVE && lane == 0 && c >= 8 && c < 24) { \
            unsigned long long t_;                                                                                     \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                                  \
            a.debug[(c - 8) * 8 + (slot)] = t_;                                                                        \
        }                                                                                                              \
    } while (0)
#else
#define GXSTAMP(slot) do {} while (0)
#endif
template <bool FIRST>
__global__ __launch_bounds__(256, 1) void k_dhidden_x3(X3Args a, const int hp)
{
    // [0, 96 KiB): W ring, 2 slots;  [96, 120 KiB): G exchange, 2 slots.  The epilogue reuses the W ring.
    extern __shared__ __attribute__((aligned(1024))) char s_dh[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int i = lane & 31, half = lane >> 5;
    const int T = a.T, U1 = a.U1, H = a.H, V = a.V;
    const DhTile tl = dh_tile(a, blockIdx.z, blockIdx.y, blockIdx.x);
    const int VC = V / 16;
    if (FIRST) X_CLOCK_STAMP(128 + 108);  // (one tile of ~0.1 ms: 1e-4 resolution at the 100 MHz reference)

    DhCell pc;  // producer role: M tile `wave`, row i
    pc.at(a, tl, wave, lane);

    // workgroup-uniform: no products past the utterance's length or in a u block past U_b (no lattice cell; the
    // reductions skip its slabs), but k_dw_x3 must find zeros in these rows (all three planes)
    if (tl.t0 >= tl.Tb || tl.u0 > tl.Ub) {
        if (FIRST && pc.pexists) {
            const u32x4 z = {0u, 0u, 0u, 0u};
            u32x4 *g = (u32x4 *)(a.logits + pc.pcell * V) + half;
            u32x4 *gl = (u32x4 *)(a.g_lo + pc.pcell * V) + half;
            for (int c = 0; c < VC; ++c) {  // this lane's 16 B of each plane per k-step (layout: split_dhidden.hpp, DhCell; lo: below)
                g[8 * (c >> 1) + 2 * (c & 1)] = z;
                g[8 * (c >> 1) + 4 + 2 * (c & 1)] = z;
                gl[2 * c] = z;
            }
        }
        return;
    }

    pc.load_coef<FIRST>(a, tl);
    // G lo of k-step c: 16 bytes at lo row + 32c + 16half
    const u32x4 *lsrc = (const u32x4 *)(a.g_lo + (pc.pexists ? pc.pcell : pc.zrow) * V) + half;
    const int blank = a.blank;
    // whole-line stores of the pair's hi | mid planes.  (Producer-shaped stores wrote 32-byte pieces of these lines in four
    // instructions a k-step apart: WRITE_SIZE 60.7 GB for 39.5 GB of G, profiles/r03_traffic.json.)
    const int lds0 = (int)(size_t)(lds_vptr)s_dh;
    DhLines<Bf16x3> lines;
    lines.at(a, tl, lds0 + 2 * XG_WSLOT, wave, lane);
    const int t0 = tl.t0, u0 = tl.u0;
    const long tile_cell0 = ((long)tl.b * T + t0) * U1 + u0;  // the tile's first cell (exists: t0 < Tb <= T, u0 <= Ub < U1)
    const __amdgpu_buffer_rsrc_t lrs = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(a.g_lo + tile_cell0 * V), 0, (int)((((long)(XG_BT - 1) * U1 + XG_BU) * V) * 2), 0x00020000);
    // lo plane: the pair's 64 bytes per row (half a line: a whole line would need four k-steps of fragments in the exchange),
    // lane L -> row 16n + (L >> 2) (n = 0, 1: two store instructions, 16 half lines each), piece L & 3 = (k-step parity, half)
    const int xl2 = lds0 + 2 * XG_WSLOT + ((lane >> 1) & 1) * XG_XSLOT + wave * 3072 + 2 * 1024 + 16 * ((lane >> 2) + 32 * (lane & 1));
    int lvo2[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int lt = 2 * wave + n, lu = lane >> 2;
        const bool ex = t0 + lt < T && u0 + lu < U1;
        lvo2[n] = ex ? (int)(((long)lt * U1 + lu) * V * 2) + 16 * (lane & 3) : 0x7ffffff0;
    }

    f32x16 acc[2][8];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][q][r] = 0.f;

    const int xw = lds0 + 2 * XG_WSLOT + wave * 3072 + 16 * lane;       // exchange write: [slot][M tile wave][plane][lane]
    const int xa = lds0 + 2 * XG_WSLOT + (2 * wm) * 3072 + 16 * lane;   // exchange read: M tiles 2wm, 2wm+1
    const int wb = lds0 + (8 * wn) * 1024 + 16 * lane;                  // W read: tiles 8wn .. 8wn+7 of each plane
    // W DMA: wave w copies pieces 12w .. 12w+11 of the k-step's 48 (piece = 1 KiB = one (plane, tile))
    // W k-steps by raw-buffer LDS-DMA: scalar base (this launch's 512-column pass) and offsets, one constant per-lane offset
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((char *)a.wpack_dh + (long)hp * VC * 49152, 0, VC * 49152, 0x00020000);
    const int wvo = lane * 16;

    typedef DhRaw<Bf16x3> Raw;    // FIRST: 8 fp32 logits; else: hi | mid | lo planes
    typedef DhProd<Bf16x3> Prod;
    auto xload = [&](Raw &r, int c, int part = 3) {  // part: 1 first half, 2 second half, 3 both (FIRST)
        const int cc = c < VC ? c : VC - 1;
        if (FIRST) dh_xload_logits(r, pc.xsrc, cc, half, part);
        else if (part & 1) {
            const u32x4 *p = (const u32x4 *)pc.xsrc + 8 * (cc >> 1) + 2 * (cc & 1) + half;
            r.p[0] = p[0]; r.p[1] = p[4];
            r.p[2] = lsrc[2 * cc];
        }
    };
    // G of k-step c from the raw values -> exchange slot (c & 1); (FIRST) it leaves for memory from there, as whole lines
    // (lines.read / lines.store, lo_read / lo_store below)
    auto produce_slice = [&](Prod &P, const Raw &r, int c, int sl) { dh_produce_slice<Bf16x3, FIRST>(P, r, c, sl, pc.cf, half, blank, 1.f, xw); };
    auto wdma = [&](int c, int n) {  // piece n (0..11) of this wave's share of W k-step c -> ring slot c & 1
        const int cc = c < VC ? c : VC - 1;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (lds_vptr)(s_dh + (c & 1) * XG_WSLOT + (wave * 12 + n) * 1024), 16, wvo,
                                                 (cc * 48 + wave * 12 + n) * 1024, 0, 0);
    };

    Raw xr[4];  // raw ring (slot = k-step & 3), 4 k-steps ahead of production
    xload(xr[0], 0); xload(xr[1], 1); xload(xr[2], 2); xload(xr[3], 3);
#pragma unroll
    for (int n = 0; n < 12; ++n) wdma(0, n);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the in-place stores of k-step 0 overwrite logits of k-step 1
    dh_produce<Bf16x3, FIRST>(xr[0], 0, pc.cf, half, blank, 1.f, xw);
    xload(xr[0], 4);

    for (int c0 = 0; c0 < VC; c0 += 4) {  // VC % 4 == 0 (V % 128 == 0)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j;
            // W k-step c landed (this wave's share), G fragments of step c written: publish both; every wave is
            // past its reads of step c-1 (W slot and exchange slot of c+1)
            // (vmcnt retires in order: all but the G stores and raw-ring loads issued behind the previous k-step's
            // DMAs.  In-place safety: a store of k-step s's G overwrites logits bytes of k-steps <= s+1, every one of
            // them loaded — and waited for by this counter — at least two k-steps before the store is issued.)
            GXSTAMP(0);
            if (FIRST && (j & 1)) asm volatile(RNNT_VMCNT(8) ::: "memory");  // behind the previous (even) k-step's DMAs: 4 + 2 line stores, 2 raw loads
            else if (FIRST) asm volatile(RNNT_VMCNT(2) ::: "memory");            // previous k-step odd: 2 raw loads
            else asm volatile(RNNT_VMCNT(3) ::: "memory");
            GXSTAMP(1);
            lds_barrier();
            GXSTAMP(2);
            const int ws = wb + (j & 1) * XG_WSLOT, xs = xa + (j & 1) * XG_XSLOT;
            u32x4 af[2][3], bf[8], bn[8];
            // fragment reads: A (6) and the hi plane of W (8)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(af[mt][p]) : "v"(xs), "n"(mt * 3072 + p * 1024));
#pragma unroll
            for (int q = 0; q < 8; ++q) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bf[q]) : "v"(ws), "n"(q * 1024));
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(af[0][0]), "+v"(af[0][1]), "+v"(af[0][2]), "+v"(af[1][0]), "+v"(af[1][1]), "+v"(af[1][2]),
                           "+v"(bf[0]), "+v"(bf[1]), "+v"(bf[2]), "+v"(bf[3]), "+v"(bf[4]), "+v"(bf[5]), "+v"(bf[6]), "+v"(bf[7])
                         :: "memory");
            // one product block: 16 MFMAs = (2 M tiles) x (8 column tiles) for A plane PA against the B plane held
            // in `bcur`; optionally the next B plane's 8 fragment reads (NB: plane index, -1 none), W DMA pieces of
            // k-step c+1 (D0 = 4: pieces 0-5, 8: pieces 6-11, else none) and production slices of G's k-step c+1 (S0: first slice, -1 none)
            Prod P;
            const bool prod_on = c + 1 < VC;  // workgroup-uniform
            const Raw &rawn = xr[(j + 1) & 3];
            // MEM: the k-step's five HBM operations, spread one per half block behind the DMAs (0: none; 1: G hi + mid
            // stores; 2: G lo store + first logits load; 3: second logits load)
            u32x4 ln[4];  // the pair's lines, 16 bytes per lane each (even k-steps)
            u32x4 ll[2];  // the pair's lo half lines
            auto lo_read = [&](u32x4 &v, auto n_c) {  // rows 16n .. 16n+15 of the M tile
                const int xl_ = xl2;
                asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(xl_), "n"(256 * decltype(n_c)::value));
            };
            auto lo_store = [&](u32x4 &v, int n, int ce) {
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v) :: "memory");
                __builtin_amdgcn_raw_buffer_store_b128(v, lrs, lvo2[n], 64 * (ce >> 1), 0);
            };
            auto block = [&](auto pa_c, const u32x4 (&bcur)[8], u32x4 (&bnext)[8], auto nb_c, auto d0_c, auto s0_c, auto mem_c) {
                constexpr int PA = decltype(pa_c)::value, NB = decltype(nb_c)::value, D0 = decltype(d0_c)::value, S0 = decltype(s0_c)::value;
                constexpr int MEM = decltype(mem_c)::value;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    acc[0][q] = mfma_bf16(af[0][PA], bcur[q], acc[0][q]);
                    acc[1][q] = mfma_bf16(af[1][PA], bcur[q], acc[1][q]);
                    if (NB >= 0)
                        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bnext[q]) : "v"(ws), "n"((NB < 0 ? 0 : NB) * 16384 + q * 1024));
                    // the 12 W DMAs of k-step c+1 ride in blocks 1 and 2 (six each, one per MFMA pair), none beside block 0's eight
                    // fragment reads and exp2 slices: 32.7 -> 32.3 ms against four per block in blocks 0-2 (a DMA's issue costs the
                    // more the more LDS / VALU traffic its phase carries); a burst of 12 at one point: 36 ms
                    if (D0 == 4 && q < 6) wdma(c + 1, q);
                    if (D0 == 8 && q < 6) wdma(c + 1, 6 + q);
                    if (S0 >= 0 && S0 + q < 9 && prod_on) produce_slice(P, rawn, c + 1, (S0 < 0 ? 0 : S0) + q);
                    if (FIRST) {
                        // even k-step c: G of k-steps c and c+1 is in the exchange -> the pair's lines (hi | mid) and lo half lines; every k-step: 2 raw loads
                        if (MEM == 1 && q == 1 && !(j & 1) && prod_on) { lines.read<0>(ln[0]); lines.read<1>(ln[1]); }
                        if (MEM == 1 && q == 3 && !(j & 1) && prod_on) { lines.read<2>(ln[2]); lines.read<3>(ln[3]); }
                        if (MEM == 1 && q == 5 && !(j & 1) && prod_on) { lo_read(ll[0], Int<0>{}); lo_read(ll[1], Int<1>{}); }
                        if (MEM == 3 && q == 2 && !(j & 1) && prod_on) lo_store(ll[0], 0, c);
                        if (MEM == 3 && q == 4 && !(j & 1) && prod_on) lo_store(ll[1], 1, c);
                        if (MEM == 2 && q == 1 && !(j & 1) && prod_on) lines.store(ln[0], 0, c);
                        if (MEM == 2 && q == 3 && !(j & 1) && prod_on) lines.store(ln[1], 1, c);
                        if (MEM == 2 && q == 5 && !(j & 1) && prod_on) lines.store(ln[2], 2, c);
                        if (MEM == 3 && q == 1 && !(j & 1) && prod_on) lines.store(ln[3], 3, c);
                        if (MEM == 3 && q == 3) xload(xr[(j + 1) & 3], c + 5, 1);
                        if (MEM == 3 && q == 5) xload(xr[(j + 1) & 3], c + 5, 2);
                    } else {  // the later column passes store nothing: the raw ring's refill (hi | mid and lo planes in one go)
                        if (MEM == 2 && q == 5) xload(xr[(j + 1) & 3], c + 5, 1);
                        if (MEM == 3 && q == 1) xload(xr[(j + 1) & 3], c + 5, 2);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            // every fragment read is issued at least a block (16 MFMAs) before the wait that covers it
            GXSTAMP(3);
            block(Int<0>{}, bf, bn, Int<1>{}, Int<-1>{}, Int<0>{}, Int<0>{});    // ah.bh + reads of W mid, G slices 0-7 (exp2, corrections, split)
            block(Int<1>{}, bf, bn, Int<-1>{}, Int<4>{}, Int<8>{}, Int<0>{});    // am.bh + DMA 0-5, G slice 8 (exchange)
            GXSTAMP(4);
            block(Int<2>{}, bf, bf, Int<-1>{}, Int<8>{}, Int<-1>{}, Int<0>{});   // al.bh + DMA 6-11
            // G's stores and the raw ring refill come AFTER the k-step's DMAs (vmcnt retires in order: the next k-step's
            // wait for the DMAs must not also wait out a store acknowledgement or an HBM load needed 4 k-steps from
            // now), one per half block: five back-to-back HBM operations fill the CU's memory queue and block the wave
            LDS_WAIT8(bn);
            block(Int<0>{}, bn, bf, Int<2>{}, Int<-1>{}, Int<-1>{}, Int<1>{});   // ah.bm + reads of W lo (into the hi registers); G hi, mid stores
            GXSTAMP(5);
            block(Int<1>{}, bn, bn, Int<-1>{}, Int<-1>{}, Int<-1>{}, Int<2>{});  // am.bm; G lo store, logits load
            LDS_WAIT8(bf);
            block(Int<0>{}, bf, bf, Int<-1>{}, Int<-1>{}, Int<-1>{}, Int<3>{});  // ah.bl; logits load
            GXSTAMP(6);
        }
    }
    {   // the shared epilogue: pred rows requested, drain, barrier, x (1 - hidden^2), the two slabs
        typedef Bf16x3 F;
        constexpr int MT = 2, NG = 2;
        constexpr bool XWAVE = true;
        const int mbase = 2 * wm, colbase = 512 * hp + 256 * wn;
        float (*s_red)[64][65] = (float (*)[64][65])s_dh;  // the W ring is free behind the epilogue's barrier
#include "split_dhidden_epilogue.inc"
    }
    if (FIRST) X_CLOCK_STAMP(128 + 110);
}

bool x3_dhidden_ok(int U1, int H, int V)
{
    // raw buffers over one tile's hidden rows (32-bit byte offsets), W pack addressing
    return (long)((XG_BT - 1) * (long)U1 + XG_BU) * H * 2 < 0x7fffffffL && V % 128 == 0 && H % 128 == 0;
}

void launch_dhidden_x3(const X3Args &a, hipStream_t st)
{
    const int lds = 2 * XG_WSLOT + 2 * XG_XSLOT;
    static LdsOptIn lds_opt_in;
    lds_opt_in.raise(lds, k_dhidden_x3<true>, k_dhidden_x3<false>);
    dim3 grid(a.n_ublk16, (a.T + XG_BT - 1) / XG_BT, a.B);
    hipLaunchKernelGGL(k_dhidden_x3<true>, grid, dim3(256), lds, st, a, 0);
    for (int hp = 1; hp * 512 < a.H; ++hp) hipLaunchKernelGGL(k_dhidden_x3<false>, grid, dim3(256), lds, st, a, hp);
}
