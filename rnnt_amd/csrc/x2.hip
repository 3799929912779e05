// x2.hip — the RNNT_DTYPE_F32_F16X2 route: the bf16x3 route's design (x3.hip) at HALF its matrix work.
//
// Why (round 4, tools/exp_x3_clock.py): the three bf16x3 GEMM kernels are not issue-bound but POWER-bound — under their
// six-product MFMA stream plus its HBM traffic the chip holds 1.7-2.1 GHz instead of 2.4 (k_dw_x3: 1.77 GHz at 0.82
// MFMA-busy), so every cycle saved by a tighter schedule comes back as a lower clock.  What is left is less work per
// product.  fp16 carries 11 significant bits per piece against bf16's 8, so TWO pieces hold 22 bits and THREE products
//       x = hi + mid,  hi = f16(s x), mid = f16(s x - hi)   (RNE each; s = a power of two that lifts the operand's largest
//                                                            magnitude to ~2^14: fp16's 5-bit exponent needs it)
//       a.b  ~  ah.bh + ah.bm + am.bh                         (dropped: am.bm and the residuals, <= 3 x 2^-22 |a.b|)
// give the fp32 class of error (measured beside the fp32-MFMA route in tests/test_x2_gpu.py) on half the MFMAs and
// two thirds of the operand bytes of bf16x3: 3 products instead of 6, 2 planes instead of 3 (4 bytes per element — G's
// planes exactly fill the logits they replace, no third plane beside them).
// Scales: hidden = tanh(.) in [-1, 1] -> 2^14 (constant); G: |G| <= grad_scale -> 2^k from grad_scale (host, X3Args::
// g_scale); W: 2^k from max |W|, found on the device every call (k_x2_wscale -> X3Args::scales = {s_W, 1 / s_W}).  Powers of
// two: scaling and unscaling are exact.  Values beyond fp16's range after scaling (only possible for non-finite or
// garbage operands) are clamped to +-65504 where they are split.
// Same boundary, same workspace objects, same stage structure and variants as the bf16x3 route (engine.hip runs both through
// one code path); logits, log-softmax, lattice, coefficients and all reductions are the fp32 / fp64 code of the fp32 route.
// Flush rule (below, "The flush rule and the live structures of the backward"): fp16's narrow exponent makes both planes of g_scale G
// exactly zero wherever the lattice's occupancy is below ~2^-38 — half the cells of the benchmark's batch.  The coefficient kernel
// proves that per cell (|g_scale G| < 2^-26, one binade inside what rounds to zero: lattice.hip k_coef), and the two backward GEMMs
// run the dHidden tiles and the 4-cell dW groups that hold another cell, each from an ascending list built on the device: k_dhidden_x2's
// workgroups are the entries of the live-tile list, a k-step of k_dw_x2 is four entries of the live-group list.  RNNT_VARIANT_X2_NO_FLUSH_SKIP switches the rule off per call (same lists, by length).
//
// MFMA operand maps (v_mfma_f32_32x32x16_f16, as the bf16 form): lane l = (r = l&31, h = l>>5) holds A[row r][k = 8h+j] and
// B[k = 8h+j][col r], j = 0..7; C/D: col = l&31, row = (reg&3) + 8*(reg>>2) + 4*(l>>5).
#include "split_dhidden.hpp"
#include "split_dw.hpp"

typedef __attribute__((ext_vector_type(4))) int i32x4;

#define XW2_ROWS DW_ROWS  // cells per dW k-step (the live structures below are built in these units)
#define XG2_BT 8     // the dHidden tile: 8 t x 16 u cells
#define XG2_BU 16

// ---------------------------------------------------------------------------------------
// s_W = 2^(14 - ceil(log2 max|W|)) (1 for an all-zero W): one workgroup, V*H/4 float4 reads.  A W with a NaN or an infinity in it (a diverged
// run) keeps s_W = 1 and gets a NaN as 1 / s_W: the packs' clamp (v_med3) would otherwise turn the entry into a finite fp16 and the loss would stay
// finite, where every other route — and the reference — report NaN.  Every logit and every dHidden entry is multiplied by 1 / s_W.
// ---------------------------------------------------------------------------------------
#define X2_F32_MAX 3.4028234663852886e38f
__global__ __launch_bounds__(1024) void k_x2_wscale(const float *__restrict__ W, long n4, float *__restrict__ scales)
{
    __shared__ float s_m[16];
    float m = 0.f;
    bool bad = false;
    long i = threadIdx.x;
    for (; i + 7 * 1024 < n4; i += 8 * 1024) {  // eight loads in flight per thread (one at a time: a round trip per 16 KiB, 58 us for 2 MB)
        f32x4 w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = ((const f32x4 *)W)[i + 1024 * k];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float mw = fmaxf(fmaxf(fabsf(w[k][0]), fabsf(w[k][1])), fmaxf(fabsf(w[k][2]), fabsf(w[k][3])));
            bad |= (w[k][0] != w[k][0]) | (w[k][1] != w[k][1]) | (w[k][2] != w[k][2]) | (w[k][3] != w[k][3]);  // (infinities show in the maximum)
            m = fmaxf(m, mw);
        }
    }
    for (; i < n4; i += 1024) {
        const f32x4 w = ((const f32x4 *)W)[i];
        bad |= (w[0] != w[0]) | (w[1] != w[1]) | (w[2] != w[2]) | (w[3] != w[3]);
        m = fmaxf(fmaxf(m, fmaxf(fabsf(w[0]), fabsf(w[1]))), fmaxf(fabsf(w[2]), fabsf(w[3])));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 16; ++k) m = fmaxf(m, s_m[k]);
        float s = 1.0f;
        const unsigned bits = __float_as_uint(m);
        const int e = (int)(bits >> 23) & 0xff;  // m in [2^(e-127), 2^(e-126))
        if (e > 0 && e < 255) {
            int k = 14 - (e - 126);               // m * 2^k in [2^13, 2^14)
            k = k > 100 ? 100 : (k < -100 ? -100 : k);
            s = __uint_as_float((unsigned)(127 + k) << 23);
        }
        scales[0] = s;
        scales[1] = (any_bad || e == 255) ? __uint_as_float(0x7fc00000u) : 1.0f / s;
    }
}

// The plain producers and the W packs are split_common.hpp's, at the f16x2 format
void launch_x2_make_hidden(const X3Args &a, hipStream_t st) { launch_split_make_hidden<F16x2>(a, st); }
void launch_x2_split_g(const X3Args &a, hipStream_t st) { launch_split_g<F16x2>(a, st); }
void launch_x2_zero_padding(const X3Args &a, int what, hipStream_t st) { launch_split_zero_padding<F16x2>(a, what, st); }
size_t x2_wpack_fwd_bytes(int H, int V) { return split_wpack_fwd_bytes<F16x2>(H, V); }
size_t x2_wpack_dh_bytes(int H, int V) { return split_wpack_dh_bytes<F16x2>(H, V); }

// ---------------------------------------------------------------------------------------
// The flush rule and the live structures of the backward.
// g_scale G is split into two fp16 planes with round-to-nearest-even: a value of magnitude <= 2^-25 becomes hi = +-0, mid = +-0, and
// a zero plane entry adds nothing to an MFMA accumulator.  |G[c,:]| <= grad_scale gamma(c), gamma = exp(alpha + beta - log P) the
// posterior occupancy of lattice node c: an RNN-T lattice is occupied in a band around the alignment, and about half the cells of the
// benchmark's batch lie below that threshold.  k_coef<.., FLUSH, ..> (lattice.hip: the bound, its margin and the rounding it covers are
// derived there) gives every such cell the coefficients of a cell OUTSIDE the lattice — for which k_dhidden_x2 always produced
// G = 0 from the zero padding row — and the kernels below turn the coefficients into what lets the two backward GEMMs skip:
//   tile_live[b][tt][ub]  the dHidden tile (8 t x 16 u) holds a cell with non-null coefficients;
//   tile_list             the ascending indices of those tiles (k_x2_live_scan: counted and scanned, no atomics): workgroup g of
//                         k_dhidden_x2 (every pass) runs tile_list[g], the workgroups past the list's length return at once.  A tile that
//                         is not on it costs nothing there and writes nothing: its slab pieces may hold anything — k_reduce_enc /
//                         k_reduce_pred add a piece only where the tile's flag is 1 (JointBwdArgs::tile_flag; the sums start at +0 and the
//                         pieces left out were exact zeros) — and the G rows dW reads of it are zeroed by k_x2_dead_rows;
//   grp_bitmap / grp_list the 4-cell groups of the dW GEMM (linear cell index / 4: the rows of one DMA piece) that hold such a cell, as a
//                         bitmap and as the ascending list k_dw_x2 walks four entries to a k-step (fixed order: dW stays bitwise
//                         reproducible); the list is 16-byte aligned and padded with entries that name the first group of the zero
//                         padding rows, for the ring's read-ahead and the missing groups of the last k-step.  The live cells of a (b, t)
//                         line form a band of ~100 cells; 16-cell k-steps cut it at 16-cell boundaries and list ~12 % more rows;
//   ks_bitmap / ks_list   the same for the 16-cell k-steps (linear cell index / 16): what k_dw_x2m walks;
//   live_stats            the counts (readable from the workspace: rnnt_engine_ws_layout::x2_live).
// Dropping a flushed cell changes no bit of costs, dEnc or dPred (its products were exact zeros); dW / db change in summation
// order only (the splits cut the live list at other cells).  RNNT_VARIANT_X2_NO_FLUSH_SKIP flags no cell: the structures then hold
// what is live by the utterances' lengths.  Everything is built on the device from the coefficients: no host read-back.
// ---------------------------------------------------------------------------------------
#define XL2_BLK 1024
__device__ __forceinline__ bool x2_coef_live(const CellCoef &c) { return !(c.c1 == RNNT_NEG_INF && c.sb == 0.f && c.se == 0.f); }
namespace {
#define XL2_GPAD 32  // padding entries behind the group list (k_dw_x2 reads up to 4 XW2::NST + 3 entries past the live ones: asserted there)
struct X2LiveWs { size_t tiles, bitmap, blk, list, tlist, gbitmap, gblk, glist, total; long nks, ntile; int nblk; };
X2LiveWs x2_live_layout(int B, int T, int U1, long rows_pad)
{
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    X2LiveWs L{};
    L.nks = rows_pad / XW2_ROWS;
    L.ntile = (long)B * ((T + 7) / 8) * ((U1 + 15) / 16);
    L.nblk = (int)((L.nks + XL2_BLK - 1) / XL2_BLK);
    size_t o = 256;  // live_stats
    L.tiles = o; o += al((size_t)L.ntile);
    L.bitmap = o; o += al((size_t)L.nblk * (XL2_BLK / 8));
    L.blk = o; o += al((size_t)L.nblk * 4);
    L.list = o; o += al((size_t)(L.nks + 8) * 4);
    L.tlist = o; o += al((size_t)L.ntile * 4);
    // the 4-cell groups (4 per k-step): bitmap, live groups per 1024 (4 counts per block of 1024 k-steps), list (256-byte aligned)
    L.gbitmap = o; o += al((size_t)L.nblk * (XL2_BLK / 2));
    L.gblk = o; o += al((size_t)L.nblk * 16);
    L.glist = o; o += al((size_t)(4 * L.nks + XL2_GPAD) * 4);
    L.total = o;
    return L;
}
}  // namespace
size_t x2_live_bytes(int B, int T, int U1, long rows_pad) { return x2_live_layout(B, T, U1, rows_pad).total; }
void x2_live_carve(void *region, int B, int T, int U1, long rows_pad, X3Args &a)
{
    const X2LiveWs L = x2_live_layout(B, T, U1, rows_pad);
    char *r = (char *)region;
    a.live_stats = (int *)r; a.tile_live = (const unsigned char *)(r + L.tiles); a.ks_bitmap = (const unsigned *)(r + L.bitmap);
    a.ks_list = (int *)(r + L.list); a.tile_list = (const int *)(r + L.tlist);
    a.grp_bitmap = (const unsigned *)(r + L.gbitmap); a.grp_list = (int *)(r + L.glist);
}
// one workgroup per 1024 k-steps (16384 cells, read coalesced: 16 rounds of one cell per thread; a wave's ballot covers 4 k-steps):
// live flags -> 16 bitmap words, their number -> blk.  The same ballots give the 4-cell groups (16 per wave and round: 64 bitmap words per
// workgroup, their number per 1024 groups -> gblk[4 block + 0..3]: the unit k_x2_live_scan / k_x2_live_write work in)
__global__ __launch_bounds__(XL2_BLK) void k_x2_live_count(const CellCoef *__restrict__ coef, long cells,
                                                           unsigned long long *__restrict__ bitmap, int *__restrict__ blk,
                                                           unsigned long long *__restrict__ gbitmap, int *__restrict__ gblk)
{
    __shared__ unsigned short s_nib[16][16];  // [round = bitmap word][wave]: the wave's 4 k-step flags
    __shared__ unsigned short s_grp[16][16];  // [round][wave]: the wave's 16 group flags
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = (long)blockIdx.x * XL2_BLK * XW2_ROWS;
    for (int it = 0; it < 16; ++it) {
        const long c = base + (long)it * XL2_BLK + threadIdx.x;
        const bool live = c < cells && x2_coef_live(coef[c]);
        const unsigned long long bal = __ballot(live);
        if (lane == 0)
            s_nib[it][wave] = (unsigned short)(((bal & 0xffffull) ? 1 : 0) | ((bal & 0xffff0000ull) ? 2 : 0) |
                                               ((bal & 0xffff00000000ull) ? 4 : 0) | ((bal & 0xffff000000000000ull) ? 8 : 0));
        // bit 4j of x: any of the ballot's bits 4j .. 4j+3; then every fourth bit gathered into the low 16
        unsigned long long x = bal | (bal >> 1);
        x = (x | (x >> 2)) & 0x1111111111111111ull;
        x = (x | (x >> 3)) & 0x0303030303030303ull;
        x = (x | (x >> 6)) & 0x000f000f000f000full;
        x = (x | (x >> 12)) & 0x000000ff000000ffull;
        x = (x | (x >> 24)) & 0xffffull;
        if (lane == 0) s_grp[it][wave] = (unsigned short)x;
    }
    __syncthreads();
    int cnt = 0;
    if (threadIdx.x < 16) {
        unsigned long long w = 0;
        for (int k = 0; k < 16; ++k) w |= (unsigned long long)s_nib[threadIdx.x][k] << (4 * k);
        bitmap[(long)blockIdx.x * 16 + threadIdx.x] = w;
        cnt = __popcll(w);
    }
    if (wave == 0) {
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0) blk[blockIdx.x] = cnt;
        // group word j = lane: groups 64 j .. of the workgroup's 4096 = round j >> 2, waves 4 (j & 3) .. + 3
        unsigned long long w = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) w |= (unsigned long long)s_grp[lane >> 2][4 * (lane & 3) + k] << (16 * k);
        gbitmap[(long)blockIdx.x * 64 + lane] = w;
        int gcnt = __popcll(w);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) gcnt += __shfl_xor(gcnt, o, 64);  // 16 words = 1024 groups
        if ((lane & 15) == 0) gblk[(long)blockIdx.x * 4 + (lane >> 4)] = gcnt;
    }
}
// exclusive scan of the block counts in place (one workgroup, k_dw_list_scan's), k-steps then groups; the counts; the lists' padding entries; and the live-tile
// list: a thread takes 64 consecutive flag bytes (four 16-byte loads; the flag region is padded to 256 bytes, bytes past ntile are masked),
// counts them, the workgroup scans the counts and the thread writes its tiles' indices at its offset — 65536 tiles per round, positions by
// counting and scanning alone (ascending, the same every call).
#define XL2_TPT 64  // tiles per thread and round
__global__ __launch_bounds__(1024) void k_x2_live_scan(int *__restrict__ blk, int nblk, int *__restrict__ stats, int *__restrict__ list,
                                                       long cells, long nks, long ntile, const unsigned char *__restrict__ tile_live,
                                                       int *__restrict__ tile_list, int *__restrict__ gblk, int *__restrict__ glist)
{
    __shared__ int s_w[16];
    __shared__ int s_carry;
    auto scan_counts = [&](int *cnt, int n) {  // exclusive scan of cnt[0 .. n) in place; returns the sum
        if (threadIdx.x == 0) s_carry = 0;
        __syncthreads();
        for (int base = 0; base < n; base += 1024) {
            const int i = base + threadIdx.x;
            const int v = i < n ? cnt[i] : 0;
            int x = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d, 64); if ((threadIdx.x & 63) >= d) x += y; }
            if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = x;
            __syncthreads();
            int off = s_carry;
            for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) off += s_w[w];
            if (i < n) cnt[i] = off + x - v;
            __syncthreads();
            if (threadIdx.x == 1023) s_carry = off + x;
            __syncthreads();
        }
        const int sum = s_carry;
        __syncthreads();
        return sum;
    };
    const int total = scan_counts(blk, nblk);
    const int gtotal = scan_counts(gblk, 4 * nblk);
    if (threadIdx.x == 0) s_carry = 0;  // now: live tiles before this round (their number = the sum of k_x2_live_tiles' flag bytes)
    __syncthreads();
    for (long base = 0; base < ntile; base += 1024L * XL2_TPT) {
        const long k0 = base + (long)threadIdx.x * XL2_TPT;
        unsigned long long m = 0;  // bit j: tile k0 + j is live
        if (k0 < ntile) {
            u32x4 f[XL2_TPT / 16];
#pragma unroll
            for (int q = 0; q < XL2_TPT / 16; ++q) f[q] = ((const u32x4 *)(tile_live + k0))[q];
#pragma unroll
            for (int q = 0; q < XL2_TPT / 16; ++q)
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if ((f[q][j >> 2] >> (8 * (j & 3))) & 0xffu) m |= 1ull << (16 * q + j);
            if (ntile - k0 < XL2_TPT) m &= (1ull << (ntile - k0)) - 1ull;
        }
        const int v = __popcll(m);
        int x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d, 64); if ((threadIdx.x & 63) >= d) x += y; }
        if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = x;
        __syncthreads();
        int off = s_carry;
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) off += s_w[w];
        off += x - v;
        for (; m; m &= m - 1) tile_list[off++] = (int)(k0 + __builtin_ctzll(m));
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = off;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[0] = total; stats[1] = (int)((cells + XW2_ROWS - 1) / XW2_ROWS); stats[2] = s_carry; stats[3] = (int)ntile;
        stats[4] = gtotal; stats[5] = (int)((cells + 3) / 4);
    }
    if (threadIdx.x < 8) list[total + threadIdx.x] = (int)nks;  // rows rows_pad ..: zero padding (rows_alloc >= rows_pad + 96)
    if (threadIdx.x < XL2_GPAD) glist[gtotal + threadIdx.x] = (int)(4 * nks);  // group rows_pad / 4: the same rows' first four
}
// workgroups [0, nblk): 1024 k-steps each -> list; workgroups [nblk, 5 nblk): 1024 groups each -> glist (same code on the groups' bitmap and offsets)
__global__ __launch_bounds__(XL2_BLK) void k_x2_live_write(const unsigned long long *__restrict__ bitmap, int nblk, const int *__restrict__ blk,
                                                           int *__restrict__ list, const unsigned long long *__restrict__ gbitmap,
                                                           const int *__restrict__ gblk, int *__restrict__ glist)
{
    __shared__ int s_w[XL2_BLK / 64];
    int bid = blockIdx.x;  // (workgroup-uniform)
    if (bid >= nblk) { bid -= nblk; bitmap = gbitmap; blk = gblk; list = glist; }
    const long k = (long)bid * XL2_BLK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = bitmap[k >> 6];
    if (lane == 0) s_w[wave] = __popcll(bal);
    __syncthreads();
    int off = blk[bid];
    for (int w = 0; w < wave; ++w) off += s_w[w];
    if ((bal >> lane) & 1ull) list[off + __popcll(bal & ((1ull << lane) - 1ull))] = (int)k;
}
// one wave per dHidden tile [b][tt][ub] (two rounds of 64 cells), four tiles per workgroup: the tile's flag byte.  (No counting here:
// an atomic per live tile on one word cost 0.28 ms at config 2 — k_x2_live_scan sums the bytes.)
__global__ __launch_bounds__(256) void k_x2_live_tiles(const CellCoef *__restrict__ coef, int T, int U1, int ntt, int nub, long ntile,
                                                       unsigned char *__restrict__ tile_live)
{
    const int lane = threadIdx.x & 63;
    const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);  // (wave-uniform)
    if (tile >= ntile) return;
    const int ub = (int)(tile % nub), tt = (int)((tile / nub) % ntt);
    const long b = tile / ((long)nub * ntt);
    bool live = false;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int r = it * 64 + lane;
        const int t = tt * XG2_BT + (r >> 4), u = ub * XG2_BU + (r & 15);
        if (t < T && u < U1) live = live || x2_coef_live(coef[(b * T + t) * U1 + u]);
    }
    const bool any = __any(live ? 1 : 0) != 0;
    if (lane == 0) tile_live[tile] = any ? 1 : 0;
}
void launch_x2_live(const X3Args &a, hipStream_t st)
{
    const X2LiveWs L = x2_live_layout(a.B, a.T, a.U1, a.rows_pad);
    const long cells = (long)a.B * a.T * a.U1;
    int *blk = (int *)((char *)a.live_stats + L.blk);
    int *gblk = (int *)((char *)a.live_stats + L.gblk);
    unsigned long long *bitmap = (unsigned long long *)a.ks_bitmap, *gbitmap = (unsigned long long *)a.grp_bitmap;
    const int ntt = (a.T + XG2_BT - 1) / XG2_BT, nub = (a.U1 + XG2_BU - 1) / XG2_BU;
    hipLaunchKernelGGL(k_x2_live_tiles, dim3((unsigned)((L.ntile + 3) / 4)), dim3(256), 0, st, a.coef, a.T, a.U1, ntt, nub, L.ntile, (unsigned char *)a.tile_live);
    hipLaunchKernelGGL(k_x2_live_count, dim3(L.nblk), dim3(XL2_BLK), 0, st, a.coef, cells, bitmap, blk, gbitmap, gblk);
    hipLaunchKernelGGL(k_x2_live_scan, dim3(1), dim3(1024), 0, st, blk, L.nblk, a.live_stats, a.ks_list, cells, L.nks, L.ntile, a.tile_live, (int *)a.tile_list, gblk, a.grp_list);
    hipLaunchKernelGGL(k_x2_live_write, dim3(5 * L.nblk), dim3(XL2_BLK), 0, st, bitmap, L.nblk, blk, a.ks_list, gbitmap, gblk, a.grp_list);
}

// dW / db = the sum of the split-K slabs, accumulated in fp64 and rounded ONCE (fixed order: bitwise reproducible).  The splits cut the
// live k-step list evenly, so WHERE they cut depends on how many k-steps the flush rule left: an fp32 running sum over up to 256 slabs
// rounds at every step at the size of the total (measured: 3 ulp of the largest dW entries between a call with and without
// RNNT_VARIANT_X2_NO_FLUSH_SKIP), where the slabs themselves — fp32 sums of 1 / n_split of the cells — differ far below an ulp of the
// total.  With one rounding the result no longer follows the cuts beyond that ulp.  Same bytes read, 0.03 ms at config 2.
__global__ __launch_bounds__(256) void k_x2_reduce_slabs(const float *__restrict__ slab, float *__restrict__ out, long n4, int ns)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n4) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int k = 0; k < ns; ++k) {
        const f32x4 v = ((const f32x4 *)slab)[(long)k * n4 + idx];
        s0 += (double)v[0]; s1 += (double)v[1]; s2 += (double)v[2]; s3 += (double)v[3];
    }
    ((f32x4 *)out)[idx] = f32x4{(float)s0, (float)s1, (float)s2, (float)s3};
}
void launch_dw_reduce_x2(const X3Args &a, float *grad_W, float *grad_bias, hipStream_t st)
{
    const long n4w = (long)a.V * a.H / 4, n4b = a.V / 4;
    hipLaunchKernelGGL(k_x2_reduce_slabs, dim3((unsigned)((n4w + 255) / 256)), dim3(256), 0, st, a.slab_w, grad_W, n4w, a.n_split);
    hipLaunchKernelGGL(k_x2_reduce_slabs, dim3((unsigned)((n4b + 255) / 256)), dim3(256), 0, st, a.slab_b, grad_bias, n4b, a.n_split);
}

// ---------------------------------------------------------------------------------------
// k_dw_x2: dW[v,h] = sum_c G[c,v] hidden[c,h] (split-K slabs), db[v] = sum_c G[c,v] — k_dw_x3's design on two planes:
// 4 waves = 2 (M) x 2 (N), workgroup tile 256 v x 256 h, wave 128 x 128 = 16 accumulator tiles (256 registers).  Both
// operands row-major with K (the cell) as the ROW, two fp16 planes each:
//  * HBM -> LDS by LDS-DMA, ring of XW2::NST (4) stages of 16 cells x (256 v + 256 h) x 2 planes = 32 KiB; wave w fills operand tile w
//    (0,1: the 128-column halves of the G tile, 2,3: of the hidden tile), 8 DMAs of 1 KiB (4 rows x 256 B) per stage;
//  * LDS -> VGPR by ds_read_b64_tr_b16 (4x16 transpose read): two reads give a lane its 8 consecutive cells of one column;
//  * tile image: 256-byte rows, 16-byte chunk ch of row r at 16*(ch ^ swz(r)), swz(r) = ((r&3)<<2) | ((r>>2)&3), applied
//    on the DMA's SOURCE side (the DMA writes LDS linearly).
// One k-step = 16 cells = 3 products x 16 tiles = 48 MFMAs (1536 matrix-pipe cycles) against 32 KiB staged.  Per k-step:
// counted vmcnt + one barrier publish stage ks, the 8 DMAs of stage ks+3 go into the slot of ks-1 threaded through the
// MFMAs (3 + 3 + 2), fragment reads run one product ahead of their MFMAs.  Products ah.bh, am.bh, ah.bm.
// K walk: the split-K ranges are cut from the ascending list of LIVE 4-cell groups (X3Args::grp_list: the groups that hold a cell with
// non-null coefficients — inside the lengths, reachable, not flushed) in units of k-steps of four entries, n_k = ceil(live groups / 4),
// evenly, so the splits are balanced whatever the lattices' shapes; k-step ks of a split multiplies the 16 rows of the groups
// list[4 (g_lo + ks)] .. + 3 — DMA piece i of a plane reads the four rows of entry i through a raw buffer of its own — one pipeline run per
// split; the groups the last k-step lacks are padding entries (zero rows, read like any other: every vector memory operation of a k-step
// is unconditional and in one order, the counted waits do not know the difference).  Rows of a live group that belong to no live cell
// hold zeros (k_dhidden_x2 writes them inside its live tiles, k_x2_dead_rows those of the tiles that are not live).
// The accumulators hold g_scale x 2^14 x dW: the epilogue multiplies by X3Args::dw_rescale (a power of two).
// The pieces of the kernel are split_dw.hpp's (ring geometry, sources, fragment addressing, the k-step on two planes, lockstep, ring driver,
// store); what stands here is the group-list walk with its counted wait and the placement of the pieces.
// ---------------------------------------------------------------------------------------
typedef DwRing<F16x2, 4> XW2;  // ring stages: the DMAs of stage ks + NST - 1 are issued during k-step ks; 4 x 8 KiB per operand tile
typedef DwLockstep<6, XW2::NST> XW2Lockstep;  // lag 6 k-steps, a look every NST k-steps, the count of the one pipeline run

// the four list entries of a k-step (X3Args::grp_list): ONE 16-byte scalar load, then WAIT (a counted vmcnt or nothing), then the wait for
// the load itself — one statement, so that the entries have landed wherever they are named
#define XW2_LOAD_ENT4(ent, ep, WAIT) asm volatile("s_load_dwordx4 %0, %1, 0x0\n\t" WAIT "s_waitcnt lgkmcnt(0)" : "=s"(ent) : "s"(ep) : "memory")
// rows 4 ent .. 4 ent + 3 of a plane (base: the plane's row 0, gbytes: four rows) as the raw buffer of a DMA piece whose instruction carries the
// immediate offset imm: taken back out of the base, added to the range (wave-uniform)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x2_piece_rsrc(const char *base, int ent, unsigned gbytes, int imm)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)(base + (unsigned long long)(unsigned)ent * gbytes - imm), 0, (int)gbytes + imm, 0x00020000);
}

// NW = waves per workgroup: 4, one wave per SIMD, wave tile 128 v x 128 h = 16 accumulator tiles.  (Two waves per SIMD with 8 tiles each
// were measured equal, 15.5 ms both at cfg2: the kernel is bound by the bytes it stages — 32 KiB per k-step and CU at ~12.6 B/clk/CU, the
// rate the forward's and dHidden's W streams reach — not by issue stalls.  The parameter stays in the kernel's name: profiles/, DESIGN.md.)
// PARTH (H % 256 == 128: the last h block is half empty — H = 640): the waves of the dead 128-column half run no product MFMAs and the
// dead hidden tile's DMAs are requested past their buffer's range (no bytes moved; the instruction and its vmcnt stay).
template <int NW, bool PARTH = false>
__global__ __launch_bounds__(64 * NW, 1) void k_dw_x2(X3Args a)
{
    static_assert(NW == 4, "one wave per SIMD");
    constexpr int QN = 4;  // 32-column h tiles per wave
    constexpr int ND = 8;  // DMA pieces per wave and stage
    extern __shared__ __attribute__((aligned(1024))) char s_ring[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = a.H;
    const DwTile tl = dw_tile(blockIdx.x, wave, H, a.V, a.n_split);
    const int tile = tl.tile, tiles = tl.tiles, split = tl.split, vb = tl.vb, hb = tl.hb, wm = tl.wm, wn = tl.wn;
    // this split's share [g_lo, g_hi) of the k-steps of LIVE groups, four list entries each (X3Args::grp_list, launch_x2_live; the Linear
    // layer: every group); the last k-step is filled up with the list's padding entries
    static_assert(XL2_GPAD >= 4 * XW2::NST + 3, "read-ahead of NST k-steps behind a partly filled last one");
    const long nlive = (__builtin_amdgcn_readfirstlane(a.live_stats[4]) + 3) / 4;  // (uniform by construction; said so: the walk's control flow is scalar)
    // (the 64-bit divisions run on the vector ALU: the quotients, at most nlive, are handed back to scalar registers)
    const int g_lo = __builtin_amdgcn_readfirstlane((int)(nlive * split / a.n_split));
    const int g_hi = __builtin_amdgcn_readfirstlane((int)(nlive * (split + 1) / a.n_split));
    X_CLOCK_STAMP(128 + 104);

    // db (dw_bias_mfma): the waves of h blocks 0 and 1 each take one of their wm half's four M tiles; one h block: two each
    f32x16 acc[4][QN], dacc;
    dw_zero(acc, dacc);
    DwBias bias;
    const int bsel0 = dw_bias_setup<F16x2>(bias, tl.n_hblk, hb, wn, lane);

    if (g_hi > g_lo) {
        // ---- DMA source of this wave's operand tile
        const int otile = wave;
        const bool is_g = otile < 2;
        const bool dead_tile = PARTH && !is_g && hb * 256 + 128 * (otile & 1) >= H;  // (wave-uniform)
        DwSource<F16x2> src;
        dw_source(src, a, is_g, dw_col0(is_g, is_g ? vb : hb, otile & 1, H, a.V));
        const long rstride = src.rstride[0];  // (both planes')
        // DMA i (0..3) of a plane's 16 rows: ring rows 4i .. 4i+3 <- the four rows of the k-step's list entry i, a raw buffer of its own
        // (row 0 of the group: the immediate is taken out of the buffer's base below)
        int soff[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) soff[i] = dead_tile ? DW_SOFF_DEAD : dw_soff(lane, i, 0, rstride, is_g, 0);
        // The four pieces of a plane share one LDS base (M0); piece i carries the immediate offset 1024 i, which advances the memory
        // address too and counts in the range check.  It is taken back out of the piece's buffer BASE and added to its range (the per-lane
        // offset of the group's row 0 is below 1024 i: subtracting there would wrap, and the range check would hand back zeros)
        const unsigned gbytes = (unsigned)(4 * rstride);  // one group of one plane (rstride < 2^29: x2_dhidden_ok / x2_linear_ok)
        const bool live_n = !PARTH || hb * 256 + wn * 32 * QN < H;  // this wave's h columns exist (wave-uniform)
        // The walk: ONE pipeline run over the split's list entries — k-step ks multiplies the 16 cells of the four groups
        // list[4 (g_lo + ks)] .. + 3 of the [cells] buffers.  The four entries are fetched by ONE 16-byte scalar load (the list is 16-byte
        // aligned; wave-uniform, outside the counted vector-memory stream; they only feed the buffer resources' bases) that is waited
        // for in the same asm statement, so no register copy made before the data arrived can be what an address is built from; inside
        // the k loop it is issued in front of the counted vmcnt wait it shares its latency with.  Past the split's end the read-ahead
        // fetches the next split's entries (real rows, never multiplied) or the list's padding entries (zero rows).
        const int *lptr = a.grp_list + 4L * g_lo;
        // ---- fragment bases: A from operand tile wm; this wave's h tiles, columns 128 wn + 32 m of the 256, from operand tile 2 + wn;
        // db: the M tile(s) this wave sums (bsel0, and bsel0 + 2 with one h block)
        const int lds0 = (int)(size_t)(lds_vptr)s_ring;
        int abase[4][2], bbase[QN][2];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int sec = 0; sec < 2; ++sec) {
                abase[m][sec] = dw_frag_addr<XW2>(lds0, wm, m, sec, lane);
                bbase[m][sec] = dw_frag_addr<XW2>(lds0, 2 + wn, m, sec, lane);
            }
        dw_bias_bases<XW2>(bias, lds0, wm, bsel0, lane);

        auto kstep = [&](auto st_c, long ks) {
            constexpr int ST = decltype(st_c)::value, DST = (ST + XW2::NST - 1) % XW2::NST;
            // stage ks landed (the 8 (NST - 2) younger pieces of the stages after it may still fly).  In front of the wait: the four list
            // entries of stage ks + NST - 1
            i32x4 ent;
            const int *ep = lptr + 4 * (ks + (XW2::NST - 1));
            static_assert(ND == XW2::ND && XW2::WAIT == 16, "the counted wait");
            XW2_LOAD_ENT4(ent, ep, RNNT_VMCNT(16) "\n\t");
            // piece n of this wave's share of stage ks+NST-1 -> ring stage DST: plane n>>2, ring rows 4(n&3).. <- the
            // four rows of entry n&3 as a raw buffer (wave-uniform base, built here between the MFMAs; the per-lane part is the 32-bit soff)
            auto dma_piece = [&](auto n_c) {
                constexpr int n = decltype(n_c)::value, i = n & 3, p = (n >> 2) & 1, imm = 1024 * i;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(x2_piece_rsrc(src.pbase[p], ent[i], gbytes, imm),
                                                         (lds_vptr)(s_ring + otile * XW2::TILE + DST * XW2::STAGE + p * XW2::PLANE),
                                                         16, soff[i], 0, imm, 0);
            };
            dw_kstep2<XW2, ST, 3, 3, 2>(acc, dacc, abase, bbase, bias, live_n, a.ablate, dma_piece);
        };
        auto dma_stage = [&](long ks, int st) {  // pipeline prologue: this wave's pieces of stage ks
            i32x4 ent;
            const int *ep = lptr + 4 * ks;
            XW2_LOAD_ENT4(ent, ep, "");
#pragma unroll
            for (int n = 0; n < ND; ++n) {
                const int p = n >> 2, i = n & 3;
                dw_dma_imm(x2_piece_rsrc(src.pbase[p], ent[i], gbytes, 1024 * i), (lds_vptr)(s_ring + otile * XW2::TILE + st * XW2::STAGE + p * XW2::PLANE),
                           soff[i], i);
            }
        };
        XW2Lockstep ls;
        ls.init(a.dw_prog, split, tile, tiles);
        dw_ring(g_hi - g_lo, ls, tile, tid, kstep, dma_stage);
    }

    X_CLOCK_STAMP(128 + 106);
    dw_store<F16x2, true>(a, split, tl.v0, tl.h0, lane, acc, dacc, bias.do_b, bias.two_b, bsel0);
}


// ---------------------------------------------------------------------------------------
// k_dw_x2m (round 6): dW for H % 256 == 128 with at least two whole 256-column h blocks and an even number of v blocks (config 4:
// H = 640, V = 1024).  k_dw_x2<4, true> covers the odd last 128 columns with one half-empty 256 x 256 tile per v block: two of its four
// waves run no MFMAs, the workgroup naps in the split's lockstep, and the split count is sized for 3 tiles per v block although only 2.5
// tiles' worth of products exist (config 4: 12 tiles x 21 splits, dW 13 % over its time per cell at config 2).  Here the odd block of TWO v
// blocks is one TALL tile — 512 v x 128 h, four waves stacked along v, wave tile 128 x 128 as everywhere (16 accumulator tiles, 48 MFMAs per
// k-step: every wave of every workgroup works) — beside the ordinary 256 x 256 tiles of the whole h blocks: (V/256) (H/256) + V/512 tiles
// per split (config 4: 10 tiles x 25 splits).  A tall tile stages 4 G operand tiles (one per wave: the wave's own A rows) and 1 hidden
// operand tile (its 8 DMA pieces per stage shared out two per wave): 40 KiB per k-step instead of 32, a 5-tile ring = 160 KiB of LDS.
// The two tile kinds are two instantiations of the body behind ONE workgroup-uniform branch (a branch inside the k loop would split the
// hand-placed MFMA / DMA / read schedule into scheduling regions).  Everything but the geometry, the DMA sources (tall: 10 pieces per wave
// and stage, threaded 4 + 3 + 3) and the walk of the live k-step list (X3Args::ks_list: one entry per k-step, one buffer resource per
// plane) is split_dw.hpp's, shared with k_dw_x2<4>; db from whole h blocks 0 and 1 only.
// ---------------------------------------------------------------------------------------
int x2_dw_mixed_ok(int H, int V) { return H % 256 == 128 && H >= 640 && V % 512 == 0; }
int x2_dw_tiles(int H, int V) { return x2_dw_mixed_ok(H, V) ? (V / 256) * (H / 256) + V / 512 : ((V + 255) / 256) * ((H + 255) / 256); }

__global__ __launch_bounds__(256, 1) void k_dw_x2m(X3Args a)
{
    extern __shared__ __attribute__((aligned(1024))) char s_ring[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = a.H, V = a.V;
    const int n_vblk = V / 256, n_fh = H / 256;  // whole h blocks; the odd block = columns 256 n_fh .. +127
    const int n_full = n_vblk * n_fh, tiles = n_full + n_vblk / 2;
    const int id = dw_xcd_remap(blockIdx.x, tiles * a.n_split);
    const int tile = id % tiles, split = id / tiles;
    // this split's share [g_lo, g_hi) of the live k-steps (k_dw_x2's walk: X3Args::ks_list)
    const long nlive = __builtin_amdgcn_readfirstlane(a.live_stats[0]);
    const int g_lo = __builtin_amdgcn_readfirstlane((int)(nlive * split / a.n_split));
    const int g_hi = __builtin_amdgcn_readfirstlane((int)(nlive * (split + 1) / a.n_split));

    auto body = [&](auto tall_c) {
        constexpr bool TALL = decltype(tall_c)::value != 0;
        // tile geometry.  Whole-block tile: (vb, hb), waves 2 (v) x 2 (h).  Tall tile: v blocks 2 vt, 2 vt + 1, the odd h block, waves 4 (v) x 1
        const int vb = TALL ? 0 : tile / n_fh, hb = TALL ? n_fh : tile % n_fh, vt = TALL ? tile - n_full : 0;
        const int wm = TALL ? wave : wave >> 1, wn = TALL ? 0 : wave & 1;
        const int v0 = TALL ? vt * 512 + wave * 128 : vb * 256 + wm * 128;
        const int h0 = TALL ? n_fh * 256 : hb * 256 + wn * 128;

        // db as in k_dw_x2<4>: the waves of the whole-block tiles of h blocks 0 and 1 each take one of their wm half's four M tiles
        f32x16 acc[4][4], dacc;
        dw_zero(acc, dacc);
        DwBias bias;
        bias.do_b = !TALL && hb < 2;  // workgroup-uniform
        bias.two_b = false;
        const int bsel0 = (hb & 1) * 2 + wn;
        bias.sel0 = (lane & 31) == 0 ? F16x2::ONES : 0u; bias.sel1 = 0u;  // ones in column 0 of the selector fragment

        if (g_hi > g_lo) {
            // ---- DMA sources.  Own operand tile (8 pieces per stage): whole-block tile: waves 0, 1 the G tile's 128-column halves, waves 2, 3
            // the hidden tile's; tall tile: every wave the 128 G columns of its own A rows.  Tall tile, in addition: pieces 2 (wave & 1),
            // 2 (wave & 1) + 1 of plane wave >> 1 of the ONE hidden operand tile all four waves multiply by.
            const bool is_g = TALL || wave < 2;
            const int col0 = TALL ? v0 : (is_g ? vb : hb) * 256 + 128 * (wave & 1);
            DwSource<F16x2> src;
            dw_source(src, a, is_g, col0);
            const long rstride = src.rstride[0];  // (both planes')
            int soff[4];  // (the piece's immediate offset 1024 i advances the memory address too: taken out here)
#pragma unroll
            for (int i = 0; i < 4; ++i) soff[i] = dw_soff(lane, i, 4 * i, rstride, is_g, 1024 * i);
            const int xp = wave >> 1, xi0 = 2 * (wave & 1);  // tall: this wave's two pieces of the hidden tile — plane xp, pieces xi0, xi0 + 1
            const char *xbase = (const char *)(a.hidden + xp * a.plane_stride) + 2L * h0;
            const long xstride = 2L * H;
            int xoff[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) xoff[k] = dw_soff(lane, xi0 + k, 4 * (xi0 + k), xstride, false, 0);
            const int *lptr = a.ks_list + g_lo;  // k-step ks multiplies the 16 rows of k-step lptr[ks] (k_dw_x2's walk)
            // ---- fragment bases: A from operand tile wm (tall: wave), the tile this wave stages when TALL; B from the hidden tile(s)
            const int lds0 = (int)(size_t)(lds_vptr)s_ring;
            const int own_tile = wave;  // operand tile this wave stages
            int abase[4][2], bbase[4][2];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int sec = 0; sec < 2; ++sec) {
                    abase[m][sec] = dw_frag_addr<XW2>(lds0, wm, m, sec, lane);
                    bbase[m][sec] = dw_frag_addr<XW2>(lds0, TALL ? 4 : 2 + wn, m, sec, lane);
                    bias.sbase[1][sec] = bias.sbase[0][sec] = dw_frag_addr<XW2>(lds0, wm, bsel0 & 3, sec, lane);
                }

            auto kstep = [&](auto st_c, long ks) {
                constexpr int ST = decltype(st_c)::value, DST = (ST + XW2::NST - 1) % XW2::NST;
                // stage ks landed (the ND (NST - 2) younger pieces of the stages after it may still fly: ND = 8, tall 10).  In front of the
                // wait: the list entry of stage ks + NST - 1 (k_dw_x2's)
                int ent;
                const int *ep = lptr + ks + (XW2::NST - 1);
                static_assert(XW2::WAIT == 16 && (XW2::ND + 2) * (XW2::NST - 2) == 20, "the counted waits: 8 pieces per wave and stage, tall 10");
                if (TALL) asm volatile("s_load_dword %0, %1, 0x0\n\t" RNNT_VMCNT(20) "\n\ts_waitcnt lgkmcnt(0)" : "=s"(ent) : "s"(ep) : "memory");
                else asm volatile("s_load_dword %0, %1, 0x0\n\t" RNNT_VMCNT(16) "\n\ts_waitcnt lgkmcnt(0)" : "=s"(ent) : "s"(ep) : "memory");
                __amdgpu_buffer_rsrc_t rs[2];
#pragma unroll
                for (int p = 0; p < 2; ++p) rs[p] = dw_rows_rsrc(src.pbase[p], (long)ent * DW_ROWS, rstride, DW_ROWS);
                const __amdgpu_buffer_rsrc_t xrs = dw_rows_rsrc(xbase, (long)ent * DW_ROWS, xstride, DW_ROWS);
                auto dma_piece = [&](auto n_c) {  // piece n of this wave's share of stage ks+NST-1 -> ring stage DST
                    constexpr int n = decltype(n_c)::value;
                    if constexpr (n < 8) {
                        constexpr int i = n & 3, p = (n >> 2) & 1;
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs[p], (lds_vptr)(s_ring + own_tile * XW2::TILE + DST * XW2::STAGE + p * XW2::PLANE),
                                                                 16, soff[i], 0, 1024 * i, 0);
                    } else {  // (tall) the hidden tile: operand tile 4
                        constexpr int k = n - 8;
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (lds_vptr)(s_ring + 4 * XW2::TILE + DST * XW2::STAGE + xp * XW2::PLANE + 1024 * (xi0 + k)),
                                                                 16, xoff[k], 0, 0, 0);
                    }
                };
                dw_kstep2<XW2, ST, (TALL ? 4 : 3), 3, (TALL ? 3 : 2)>(acc, dacc, abase, bbase, bias, true, a.ablate, dma_piece);
            };
            auto dma_stage = [&](long ks, int st) {  // pipeline prologue: this wave's pieces of stage ks
                int ent;
                const int *ep = lptr + ks;
                asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(ent) : "s"(ep) : "memory");
#pragma unroll
                for (int n = 0; n < 8; ++n) {
                    const int p = n >> 2, i = n & 3;
                    dw_dma_imm(dw_rows_rsrc(src.pbase[p], (long)ent * DW_ROWS, rstride, DW_ROWS),
                               (lds_vptr)(s_ring + own_tile * XW2::TILE + st * XW2::STAGE + p * XW2::PLANE), soff[i], i);
                }
                if (TALL) {
                    const __amdgpu_buffer_rsrc_t r = dw_rows_rsrc(xbase, (long)ent * DW_ROWS, xstride, DW_ROWS);
#pragma unroll
                    for (int k = 0; k < 2; ++k)
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_vptr)(s_ring + 4 * XW2::TILE + st * XW2::STAGE + xp * XW2::PLANE + 1024 * (xi0 + k)),
                                                                 16, xoff[k], 0, 0, 0);
                }
            };
            // (tall and whole-block tiles walk the same k-steps and share G through L2: one lockstep ring)
            XW2Lockstep ls;
            ls.init(a.dw_prog, split, tile, tiles);
            dw_ring(g_hi - g_lo, ls, tile, tid, kstep, dma_stage);
        }
        dw_store<F16x2, false>(a, split, v0, h0, lane, acc, dacc, bias.do_b, false, bsel0);  // (V % 512 == 0, H % 128 == 0: every row and column exists)
    };
    if (tile >= n_full) body(Int<1>{});  // (workgroup-uniform)
    else body(Int<0>{});
}

// the dW kernel launch_dw_x2 picks for this call walks the 16-cell k-step list (k_dw_x2m), not the group list: k_x2_dead_rows walks it too
bool x2_dw_walks_ksteps(int H, int V) { return x2_dw_mixed_ok(H, V) != 0; }

void launch_dw_x2(const X3Args &a, hipStream_t st, bool zero_prog)
{
    if (a.dw_prog && zero_prog) launch_fill32(a.dw_prog, 0u, (size_t)a.n_split * 64, st);
    const int tiles = x2_dw_tiles(a.H, a.V);
    static LdsOptIn lds_opt_in;
    lds_opt_in.raise(4 * XW2::TILE, k_dw_x2<4>, k_dw_x2<4, true>);
    static LdsOptIn lds_opt_in_m;
    lds_opt_in_m.raise(5 * XW2::TILE, k_dw_x2m);
    // H % 256 == 128: whole-block tiles + tall tiles over the odd block (k_dw_x2m) where the shape allows; else the half-empty last h block
    if (x2_dw_mixed_ok(a.H, a.V)) hipLaunchKernelGGL(k_dw_x2m, dim3(tiles * a.n_split), dim3(256), 5 * XW2::TILE, st, a);
    else if (a.H % 256 != 0) hipLaunchKernelGGL((k_dw_x2<4, true>), dim3(((a.V + 255) / 256) * ((a.H + 255) / 256) * a.n_split), dim3(256), 4 * XW2::TILE, st, a);
    else hipLaunchKernelGGL(k_dw_x2<4>, dim3(tiles * a.n_split), dim3(256), 4 * XW2::TILE, st, a);
}


// ---------------------------------------------------------------------------------------
// k_dhidden_x2: k_dhidden_x3 on two planes.  G from the fp32 logits (exp2 + the two occupancy corrections, as the fp32 route),
// scaled by g_scale, split into its two fp16 planes, stored in place (hi | mid over each 32-wide chunk of the logits row: the
// planes fill exactly the bytes of the logits they replace) and multiplied: dHidden = G . W over 512 columns of H per launch;
// epilogue as the fp32 kernel: x (1 - hidden^2), sum over u -> dEnc slab, sum over t -> dPred slab.  Tile = 8 t x 16 u cells.
// 4 waves = 2 (M) x 2 (N), wave tile 64 cells x 256 columns = 16 accumulator tiles (256 registers).
//  * production: wave w turns M tile w (32 cells) into G: lane (cell i = l&31, half) owns the 8 vocabulary entries 16c +
//    8*half .. +7 of its cell per k-step — its slot of the MFMA A fragment — and drops 16 bytes per plane into the LDS exchange
//    [2 slots][M tile][plane][lane]; logits requested 4 k-steps ahead (register ring);
//  * G leaves in WHOLE 128-byte lines (32 x hi | 32 x mid of one cell and chunk = the fragments of two k-steps x two halves x
//    two planes), read back by the producing wave from its part of the exchange every second k-step: 4 store instructions;
//  * W: one linear LDS-DMA copy of 32 KiB per k-step into a 3-slot ring, two k-steps ahead (8 DMAs per wave);
//  * per k-step ONE barrier publishes W slot c and exchange slot c; then 3 products x 16 MFMAs:
//      block 0  ah.bh   + the 8 fragment reads of W's mid plane + production slices 0-7 of G(c+1) (exp2, corrections, split)
//      block 1  am.bh   + exchange write of G(c+1), W DMAs 0-6 of k-step c+2, (even c) the pair's line reads
//      block 2  ah.bm   + W DMA 7, (even c) the 4 line stores, the 2 raw logits loads of k-step c+5
//    (memory operations in ONE fixed order per k-step — DMAs, then stores, then loads — so that every vmcnt is a count).
// FIRST = false (H > 512: columns 512.., one launch per further 512): G's planes are read back from memory into the exchange
// instead of being produced; nothing is stored but the slabs.
// The accumulators hold g_scale s_W dHidden: the epilogue's sums are multiplied by 1 / (g_scale s_W) (a power of two).
// grid: one workgroup per tile, 1-D; workgroup g runs tile tile_list[g] = [b][tt][ub] (the live tiles, ascending) and returns at once when
// g >= live_stats[2].  Requires V % 128 == 0, H % 128 == 0.
// ---------------------------------------------------------------------------------------
#define XG2_WSLOT 32768   // one k-step of W: 2 planes x 16 tiles x 1 KiB
#define XG2_XSLOT 8192    // one k-step of G fragments: 4 M tiles x 2 planes x 1 KiB
#define XG2_NW 3          // W ring slots: the DMAs of k-step c+2 are issued during k-step c (as in k_joint_fwd_x2)
// PART: the pass covers fewer than 512 columns (H = 640: the second pass has 128; H < 512): the dead 128-column groups run no MFMAs
// and their W pieces are requested past the pack's range (an out-of-range LDS-DMA moves no bytes and writes zeros: the instruction
// stays, so every vmcnt stays a count) — a pass then costs what its live columns cost plus the G stream.
template <bool FIRST, bool PART>
__global__ __launch_bounds__(256, 1) void k_dhidden_x2(X3Args a, const int hp)
{
    // [0, 96 KiB): W ring, 3 slots;  [96, 112 KiB): G exchange, 2 slots.  The epilogue reuses the W ring.
    extern __shared__ __attribute__((aligned(1024))) char s_dh[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int i = lane & 31, half = lane >> 5;
    const int T = a.T, U1 = a.U1, H = a.H, V = a.V;
    // workgroup g runs the g-th LIVE tile (X3Args::tile_list, ascending [b][tt][ub]: the order the full grid was dispatched in); the grid
    // has a workgroup per tile, those past the list's length leave here: one scalar load, no store
    if ((int)blockIdx.x >= a.live_stats[2]) return;
    const int tile = __builtin_amdgcn_readfirstlane(a.tile_list[blockIdx.x]);
    const int nub = a.n_ublk16, ntt = (T + XG2_BT - 1) / XG2_BT;
    const int ub = __builtin_amdgcn_readfirstlane(tile % nub), tt = __builtin_amdgcn_readfirstlane((tile / nub) % ntt);
    const int b = __builtin_amdgcn_readfirstlane(tile / (nub * ntt));
    const DhTile tl = dh_tile(a, b, tt, ub);
    const int VC = V / 16;
    const int ngrp = PART ? (H - 512 * hp) / 128 : 4;  // live 128-column groups of this pass (H % 128 == 0)
    if (FIRST) X_CLOCK_STAMP(128 + 108);  // (one tile of ~0.1 ms: 1e-4 resolution at the 100 MHz reference)

    // A live tile holds a cell with non-null coefficients, so it lies inside the lengths (t0 < T_b, u0 <= U_b).  The tiles that are not on
    // the list — past the lengths, or every cell outside the lattice, unreachable or flushed: each would have produced G = 0 — run nowhere
    // and owe nothing here: the G rows the dW GEMM reads of them are zeroed by k_x2_dead_rows, their slab pieces are never written and the
    // reductions leave them out by the same flag (JointBwdArgs::tile_flag).  The later column passes (FIRST = false) walk the same list.

    DhCell pc;  // producer role: M tile `wave`, row i
    pc.at(a, tl, wave, lane);
    pc.load_coef<FIRST>(a, tl);
    const float gs = a.g_scale;
    const int blank = a.blank;
    const int lds0 = (int)(size_t)(lds_vptr)s_dh;
    DhLines<F16x2> lines;  // whole-line stores of the pair's G
    lines.at(a, tl, lds0 + XG2_NW * XG2_WSLOT, wave, lane);

    f32x16 acc[2][8];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][q][r] = 0.f;

    const int xw = lds0 + XG2_NW * XG2_WSLOT + wave * 2048 + 16 * lane;       // exchange write: [slot][M tile wave][plane][lane]
    const int xa = lds0 + XG2_NW * XG2_WSLOT + (2 * wm) * 2048 + 16 * lane;   // exchange read: M tiles 2wm, 2wm+1
    const int wb = lds0 + (8 * wn) * 1024 + 16 * lane;                   // W read: tiles 8wn .. 8wn+7 of each plane
    // W DMA: wave w copies pieces 8w .. 8w+7 of the k-step's 32 (piece = 1 KiB = one (plane, tile)); raw-buffer form: scalar
    // base (this launch's 512-column pass) and offsets, one constant per-lane offset
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((char *)a.wpack_dh + (long)hp * VC * XG2_WSLOT, 0, VC * XG2_WSLOT, 0x00020000);
    const int wvo = lane * 16;

    typedef DhRaw<F16x2> Raw;    // FIRST: 8 fp32 logits; else: hi | mid planes
    typedef DhProd<F16x2> Prod;
    auto xload = [&](Raw &r, int c, int part = 3) {  // part: 1 first half, 2 second half, 3 both
        const int cc = c < VC ? c : VC - 1;
        if (FIRST) dh_xload_logits(r, pc.xsrc, cc, half, part);
        else {
            const u32x4 *p = (const u32x4 *)pc.xsrc + 8 * (cc >> 1) + 2 * (cc & 1) + half;
            if (part & 1) r.p[0] = p[0];
            if (part & 2) r.p[1] = p[4];
        }
    };
    auto produce_slice = [&](Prod &P, const Raw &r, int c, int sl) { dh_produce_slice<F16x2, FIRST>(P, r, c, sl, pc.cf, half, blank, gs, xw); };
    auto wdma = [&](int c, int slot, int n) {  // piece n (0..7) of this wave's share of W k-step c -> ring slot `slot`
        const int cc = c < VC ? c : VC - 1;
        const int vo = (!PART || (((wave * 8 + n) & 15) >> 2) < ngrp) ? wvo : 0x7ffffff0;  // (piece = plane (pc >> 4), tile pc & 15 = group (pc & 15) >> 2)
        // pieces 4g .. 4g+3 on one LDS base (M0) and one scalar offset, told apart by the immediate offset (as the forward's)
        const int g4 = n & 4;
        lds_vptr dst = (lds_vptr)(s_dh + slot * XG2_WSLOT + (wave * 8 + g4) * 1024);
        const int so = (cc * 32 + wave * 8 + g4) * 1024;
        if ((n & 3) == 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, dst, 16, vo, so, 0, 0);
        if ((n & 3) == 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, dst, 16, vo, so, 1024, 0);
        if ((n & 3) == 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, dst, 16, vo, so, 2048, 0);
        if ((n & 3) == 3) __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, dst, 16, vo, so, 3072, 0);
    };

    Raw xr[4];  // raw ring (slot = k-step & 3), 4 k-steps ahead of production
    xload(xr[0], 0); xload(xr[1], 1); xload(xr[2], 2); xload(xr[3], 3);
#pragma unroll
    for (int n = 0; n < 8; ++n) wdma(0, 0, n);
#pragma unroll
    for (int n = 0; n < 8; ++n) wdma(1, 1, n);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the in-place stores of the first pair overwrite logits of k-steps 0, 1
    dh_produce<F16x2, FIRST>(xr[0], 0, pc.cf, half, blank, gs, xw);
    xload(xr[0], 4);

    int wsl = 0;  // W ring slot of k-step c (c % 3)
    for (int c0 = 0; c0 < VC; c0 += 4) {  // VC % 4 == 0 (V % 128 == 0)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j;
            // W k-step c landed (this wave's share; requested during k-step c-2), G fragments of step c written: publish both; every
            // wave is past its reads of step c-1 (W slot of c+2, exchange slot of c+1).  vmcnt retires in order: behind the DMAs of
            // k-step c-2 come its (even) 4 line stores and 2 raw loads, then k-step c-1's 8 DMAs, (even) 4 line stores and 2 raw
            // loads: 16 operations whatever c's parity.  In-place safety: a pair's line overwrites the logits of its own two
            // k-steps, both loaded and consumed (production) before the store is issued.
            if (FIRST) asm volatile(RNNT_VMCNT(16) ::: "memory");
            else asm volatile(RNNT_VMCNT(12) ::: "memory");
            lds_barrier();
            const int ws = wb + wsl * XG2_WSLOT, xs = xa + (j & 1) * XG2_XSLOT;
            const int wsn = wsl == 0 ? 2 : wsl - 1;  // (c + 2) % 3
            u32x4 af[2][2], bf[8], bn[8];
            // fragment reads: A (4) and the hi plane of W (8)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int p = 0; p < 2; ++p)
                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(af[mt][p]) : "v"(xs), "n"(mt * 2048 + p * 1024));
#pragma unroll
            for (int q = 0; q < 8; ++q) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bf[q]) : "v"(ws), "n"(q * 1024));
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(af[0][0]), "+v"(af[0][1]), "+v"(af[1][0]), "+v"(af[1][1]),
                           "+v"(bf[0]), "+v"(bf[1]), "+v"(bf[2]), "+v"(bf[3]), "+v"(bf[4]), "+v"(bf[5]), "+v"(bf[6]), "+v"(bf[7])
                         :: "memory");
            Prod P;
            // (round 5: G(c+1) is produced UNCONDITIONALLY — at the last k-step that is a k-step past the end, made from the clamped raw loads
            // and written into an exchange slot nobody reads any more: fourteen uniform branches per k-step cut the MFMA stream into as
            // many scheduling regions before)
            constexpr bool prod_on = true;
            const Raw &rawn = xr[(j + 1) & 3];
            u32x4 ln[4];  // the pair's lines, 16 bytes per lane each (even k-steps)
            // one product block: 16 MFMAs = (2 M tiles) x (8 column tiles) for A plane PA against the B plane held in `bcur`;
            // BLK names the work threaded through it (the kernel comment's table)
            auto block = [&](auto pa_c, const u32x4 (&bcur)[8], auto blk_c) {
                constexpr int PA = decltype(pa_c)::value, BLK = decltype(blk_c)::value;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    if (!PART || 2 * wn + (q >> 2) < ngrp) {  // (wave-uniform)
                        acc[0][q] = mfma_f16(af[0][PA], bcur[q], acc[0][q]);
                        acc[1][q] = mfma_f16(af[1][PA], bcur[q], acc[1][q]);
                    }
                    if (BLK == 0) {
                        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bn[q]) : "v"(ws), "n"(16384 + q * 1024));
                        if (prod_on) produce_slice(P, rawn, c + 1, q);
                    }
                    if (BLK == 1) {
                        if (q == 0 && prod_on) produce_slice(P, rawn, c + 1, 8);
                        if (q >= 1) wdma(c + 2, wsn, q - 1);
                        if (FIRST && q == 2 && !(j & 1) && prod_on) { lines.read<0>(ln[0]); lines.read<1>(ln[1]); }
                        if (FIRST && q == 4 && !(j & 1) && prod_on) { lines.read<2>(ln[2]); lines.read<3>(ln[3]); }
                    }
                    if (BLK == 2) {
                        if (q == 0) wdma(c + 2, wsn, 7);
                        if (FIRST && q >= 2 && q <= 5 && !(j & 1)) {
                            if (prod_on) lines.store(ln[q - 2 < 0 ? 0 : (q - 2 > 3 ? 3 : q - 2)], q - 2, c);
                            else { u32x4 z = {0u, 0u, 0u, 0u}; __builtin_amdgcn_raw_buffer_store_b128(z, lines.grs, 0x7ffffff0, 0, 0); }  // (never: VC is even; keeps the count)
                        }
                        if (q == 6) xload(xr[(j + 1) & 3], c + 5, 1);
                        if (q == 7) xload(xr[(j + 1) & 3], c + 5, 2);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            block(Int<0>{}, bf, Int<0>{});   // ah.bh
            block(Int<1>{}, bf, Int<1>{});   // am.bh
            LDS_WAIT8(bn);
            block(Int<0>{}, bn, Int<2>{});   // ah.bm
            wsl = wsl == 2 ? 0 : wsl + 1;
        }
    }
    {   // the shared epilogue: pred rows requested, drain, barrier, x (1 - hidden^2), the two slabs
        typedef F16x2 F;
        constexpr int MT = 2, NG = 2;
        constexpr bool XWAVE = true;
        const int mbase = 2 * wm, colbase = 512 * hp + 256 * wn;
        float (*s_red)[64][65] = (float (*)[64][65])s_dh;  // the W ring is free behind the epilogue's barrier
#include "split_dhidden_epilogue.inc"
    }
    if (FIRST) X_CLOCK_STAMP(128 + 110);
}

// ---------------------------------------------------------------------------------------
// k_dhidden_x2r (round 5): the LAST 128 columns of dHidden when H % 512 == 128 (config 4: H = 640).  k_dhidden_x2<false, true> ran them as
// a second full-cost pass — G re-read into the exchange, barrier, 12 fragment reads and a 32-piece W stage per k-step for a quarter of
// the MFMAs: ~2 600 cycles per k-step whatever rides in it (round 4).  Here a wave owns a whole 8 t x 16 u block of cells (128 rows = four
// M tiles) x the 128 columns (four N tiles): 16 accumulator tiles, 48 MFMAs per k-step like every other kernel of the route, and
//  * its A fragments come STRAIGHT from G's planes in memory — lane (i, half) of M tile m loads the 16 bytes of hi and of mid of row i,
//    k = 8 half .. +7, which IS the MFMA fragment: no exchange, no producer role — into a 4-deep register ring, three k-steps ahead;
//  * the 8 KiB of W per k-step (2 planes x 4 tiles of the pass's pack) go through a 4-slot LDS ring, 2 DMA pieces per wave, shared by the
//    workgroup's four waves = four consecutive t blocks of one u block; one barrier per k-step publishes a slot;
//  * the epilogue is k_dhidden_x2's for one wave: x (1 - hidden^2) recomputed from enc and pred, sum over u -> dEnc slab, sum over the
//    block's 8 t -> dPred slab (no cross-wave reduction: the block's t rows all sit in this wave).
// ---------------------------------------------------------------------------------------
#define XR2_WSLOT 8192
#define XR2_NW 4
__global__ __launch_bounds__(256, 1) void k_dhidden_x2r(X3Args a, const int hp)
{
    extern __shared__ __attribute__((aligned(1024))) char s_dr[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, half = lane >> 5;
    const int T = a.T, U1 = a.U1, H = a.H, V = a.V;
    const int ub = blockIdx.x, tq = blockIdx.y, b = blockIdx.z;
    const DhTile tl = dh_tile(a, b, 4 * tq + wave, ub);  // this wave's t block
    const int tt = tl.tt, t0 = tl.t0, u0 = tl.u0, Tb = tl.Tb, Ub = tl.Ub;
    const int VC = V / 16;
    if (4 * tq * XG2_BT >= Tb || u0 > Ub) return;    // workgroup-uniform: no lattice cell in any of the four blocks
    const bool winlen = t0 < Tb;                       // wave-uniform: this wave's block lies inside the lengths (else: zeros in, nothing out)
    // k_dhidden_x2's dead-tile rule: a block without a live cell (X3Args::tile_live) was not run by the first pass — its rows may hold
    // logits — so it reads the zero padding row, and writes nothing: the reductions leave a dead tile's slab pieces out by the same flag
    const bool wlive = winlen && a.tile_live[((long)b * ((T + XG2_BT - 1) / XG2_BT) + tt) * gridDim.x + ub] != 0;
    const int any_live = __syncthreads_or(wlive ? 1 : 0);
    if (!any_live) return;  // workgroup-uniform: none of the four blocks has a live cell
    const long zrow = (long)a.B * T * U1;              // first zero padding row
    // row i of M tile m = cell (t0 + 2m + (i >> 4), u0 + (i & 15)); rows outside the lattice read the zero padding row.  G's planes of
    // k-step c: hi = 16 bytes at u32x4 index 8 (c >> 1) + 2 (c & 1) + half of the row, mid 64 bytes behind (k_dhidden_x2's layout)
    const u32x4 *arow[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int t = t0 + 2 * m + (i >> 4), u = u0 + (i & 15);
        const bool ex = wlive && t < T && u < U1;
        arow[m] = (const u32x4 *)(a.logits + (ex ? ((long)b * T + t) * U1 + u : zrow) * V) + half;
    }
    struct AFrag { u32x4 h[4], m[4]; };
    auto aload = [&](AFrag &f, int c) {
        const int cc = c < VC ? c : VC - 1;
        const int o = 8 * (cc >> 1) + 2 * (cc & 1);
#pragma unroll
        for (int m = 0; m < 4; ++m) { f.h[m] = arow[m][o]; f.m[m] = arow[m][o + 4]; }
    };
    // W: piece (plane p, tile tl) of k-step c at ((c 2 + p) 16 + tl) KiB of the pass's pack; wave w stages plane w >> 1, tiles 2 (w & 1), +1
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((char *)a.wpack_dh + (long)hp * VC * XG2_WSLOT, 0, VC * XG2_WSLOT, 0x00020000);
    const int wvo = lane * 16;
    const int wp = wave >> 1, wt2 = 2 * (wave & 1);
    auto wdma = [&](int c, int slot) {  // both pieces on one M0 / scalar offset (the immediate offset advances memory and LDS address)
        const int cc = c < VC ? c : VC - 1;
        lds_vptr dst = (lds_vptr)(s_dr + slot * XR2_WSLOT + (wp * 4 + wt2) * 1024);
        const int so = ((cc * 2 + wp) * 16 + wt2) * 1024;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, dst, 16, wvo, so, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, dst, 16, wvo, so, 1024, 0);
    };
    const int lds0 = (int)(size_t)(lds_vptr)s_dr;
    const int wb = lds0 + 16 * lane;  // W read: tile n of plane p of slot s at wb + s * XR2_WSLOT + (p * 4 + n) * 1024

    f32x16 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    AFrag ar[4];  // ring: k-step c in ar[c & 3], loaded three k-steps ahead
    aload(ar[0], 0); aload(ar[1], 1); aload(ar[2], 2);
    wdma(0, 0); wdma(1, 1);
    int wsl = 0;  // W ring slot of k-step c (c & 3)
    for (int c0 = 0; c0 < VC; c0 += 4) {  // VC % 4 == 0 (V % 128 == 0)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j;
            // this wave's pieces of W(c) landed: issued at the end of k-step c-2; younger: k-step c-1's 8 A loads and 2 DMAs
            asm volatile(RNNT_VMCNT(10) ::: "memory");
            lds_barrier();  // publishes W(c); every wave is past its reads of W(c-1): slot (c + 3) & 3 ... (c + 2) & 3 are free
            const int ws = wb + wsl * XR2_WSLOT;
            u32x4 bh[4], bm[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bh[n]) : "v"(ws), "n"(n * 1024));
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bh[0]), "+v"(bh[1]), "+v"(bh[2]), "+v"(bh[3]) :: "memory");
            AFrag &ac = ar[j], &an = ar[(j + 3) & 3];
            const int cn = c + 3;
            const int o = 8 * ((cn < VC ? cn : VC - 1) >> 1) + 2 * ((cn < VC ? cn : VC - 1) & 1);
            // block 0: ah.bh + the mid plane's reads + the A loads of k-step c+3 (one per two MFMAs)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    acc[m][n] = mfma_f16(ac.h[m], bh[n], acc[m][n]);
                    if (m == 0) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bm[n]) : "v"(ws), "n"(4096 + n * 1024));
                    if (n == 1) an.h[m] = arow[m][o];
                    if (n == 3) an.m[m] = arow[m][o + 4];
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // block 1: am.bh
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    acc[m][n] = mfma_f16(ac.m[m], bh[n], acc[m][n]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bm[0]), "+v"(bm[1]), "+v"(bm[2]), "+v"(bm[3]) :: "memory");
            // block 2: ah.bm + the 2 DMA pieces of W(c+2) (the youngest memory operations of the k-step)
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    acc[m][n] = mfma_f16(ac.h[m], bm[n], acc[m][n]);
                    if (m == 3 && n == 0) wdma(c + 2, (wsl + 2) & 3);
                    __builtin_amdgcn_sched_barrier(0);
                }
            wsl = (wsl + 1) & 3;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the over-issued loads / DMAs: none may land in an LDS the next workgroup owns
    if (!wlive) return;

    {   // the shared epilogue: one wave = one block, all 8 t rows sit in this wave: no cross-wave step
        typedef F16x2 F;
        constexpr int MT = 4, NG = 1;
        constexpr bool XWAVE = false;
        const int mbase = 0, colbase = 512 * hp;
        float (*s_red)[64][65] = nullptr;
        const int wm = 0, wn = 0;
#include "split_dhidden_epilogue.inc"
    }
}

// ---------------------------------------------------------------------------------------
// k_x2_dead_rows: the zeros the dW GEMM must find.  k_dw_x2 reads all four rows of every LIVE group (X3Args::grp_list); the rows that belong
// to a live dHidden tile are written by k_dhidden_x2 (G, or zeros for cells outside the lattice), the rows of tiles that are not live —
// a group straddles tile edges: 4 consecutive cells of the linear cell order against 16-aligned u blocks of a (b, t) line — still hold logits.
// One lane per row, so a wave round covers 16 list entries (grid-stride over the list): lane l looks up the tile flag of cell l & 3 of entry
// l >> 2, then the whole wave zeroes each flagged row, both planes = the V x 4 bytes of the logits row, 16 bytes per lane and store.  Most
// rounds have no such row and cost two loads.  No LDS, 4 waves per workgroup: it runs beside anything.
// X3Args::dw_ksteps (the call's dW kernel is k_dw_x2m, which reads all 16 rows of every live k-step): the same walk over ks_list, 4 entries
// of 16 rows per round.
// Rows of dead tiles and rows of live tiles are disjoint: the order against k_dhidden_x2 is free; both precede the dW kernel.
// ---------------------------------------------------------------------------------------
#define XZ2_WG_WAVES 4
__global__ __launch_bounds__(64 * XZ2_WG_WAVES) void k_x2_dead_rows(X3Args a, int ntt, int nub)
{
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * XZ2_WG_WAVES + (threadIdx.x >> 6), nwave = (long)gridDim.x * XZ2_WG_WAVES;
    const long cells = (long)a.B * a.T * a.U1;
    const bool by_ks = a.dw_ksteps;  // (kernel-uniform)
    const int sh = by_ks ? 4 : 2, per = 64 >> sh;   // rows per list entry = 1 << sh; entries per wave round
    const int *list = by_ks ? a.ks_list : a.grp_list;
    const long n = a.live_stats[by_ks ? 0 : 4];
    const int V4 = a.V / 4;
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (long k = per * wave; k < n; k += per * nwave) {
        const long kk = k + (lane >> sh);
        int e = 0;  // (an entry fits an int: the lists' entries do)
        bool dead = false;
        if (kk < n) {
            e = list[kk];
            const long c = ((long)e << sh) + (lane & ((1 << sh) - 1));
            if (c < cells) {
                const int u = (int)(c % a.U1);
                const long bt = c / a.U1;
                const int t = (int)(bt % a.T);
                const long b = bt / a.T;
                dead = a.tile_live[(b * ntt + t / XG2_BT) * nub + u / XG2_BU] == 0;
            }
        }
        unsigned long long m = __ballot(dead);  // (wave-uniform) bit l: row (l & (1 << sh) - 1) of entry l >> sh belongs to a tile that is not live
        for (; m; m &= m - 1) {
            const int r = __builtin_ctzll(m);
            u32x4 *row = (u32x4 *)(a.logits + (((long)__shfl(e, r, 64) << sh) + (r & ((1 << sh) - 1))) * a.V);
            for (int q = lane; q < V4; q += 64) row[q] = z;
        }
    }
}
void launch_x2_dead_rows(const X3Args &a, hipStream_t st)
{
    const long rounds = ((long)a.B * a.T * a.U1 + 63) / 64;  // wave rounds of 64 rows: the most the walk can hold
    const long want = (rounds + XZ2_WG_WAVES - 1) / XZ2_WG_WAVES, cap = (long)(a.n_cu > 0 ? a.n_cu : 256) * 8;
    const int ntt = (a.T + XG2_BT - 1) / XG2_BT;
    hipLaunchKernelGGL(k_x2_dead_rows, dim3((unsigned)(want < cap ? want : cap)), dim3(64 * XZ2_WG_WAVES), 0, st, a, ntt, a.n_ublk16);
}

bool x2_dhidden_ok(int U1, int H, int V)
{
    // raw buffers over one tile's logits rows (32-bit byte offsets), W pack addressing
    return (long)((XG2_BT - 1) * (long)U1 + XG2_BU) * V * 4 < 0x7fffffffL && V % 128 == 0 && H % 128 == 0;
}

void launch_dhidden_x2(const X3Args &a, hipStream_t st)
{
    const int lds = XG2_NW * XG2_WSLOT + 2 * XG2_XSLOT;
    static LdsOptIn lds_opt_in;
    lds_opt_in.raise(lds, k_dhidden_x2<true, false>, k_dhidden_x2<false, false>, k_dhidden_x2<true, true>, k_dhidden_x2<false, true>);
    // one workgroup per tile; those past the live-tile list's length (known on the device only) return at once
    dim3 grid((unsigned)((long)a.n_ublk16 * ((a.T + XG2_BT - 1) / XG2_BT) * a.B));
    if (a.H < 512) hipLaunchKernelGGL((k_dhidden_x2<true, true>), grid, dim3(256), lds, st, a, 0);
    else hipLaunchKernelGGL((k_dhidden_x2<true, false>), grid, dim3(256), lds, st, a, 0);
    for (int hp = 1; hp * 512 < a.H; ++hp) {
        if (a.H - 512 * hp == 128) {  // the last 128 columns: a wave per 8 t x 16 u block, A fragments straight from G's planes
            dim3 gr(a.n_ublk16, ((a.T + XG2_BT - 1) / XG2_BT + 3) / 4, a.B);
            hipLaunchKernelGGL(k_dhidden_x2r, gr, dim3(256), XR2_NW * XR2_WSLOT, st, a, hp);
        }
        else if (a.H - 512 * hp < 512) hipLaunchKernelGGL((k_dhidden_x2<false, true>), grid, dim3(256), lds, st, a, hp);
        else hipLaunchKernelGGL((k_dhidden_x2<false, false>), grid, dim3(256), lds, st, a, hp);
    }
}

// ---------------------------------------------------------------------------------------
// k_x2_make_ep (round 5): the forward produces hidden = tanh(enc + pred) once per column pass for every cell, H values per cell and
// pass — its largest VALU cost (2.3 ms of 22 at config 2 when compiled out).  tanh(e + p) = 1 - 2 / (1 + exp(2e) exp(2p)): with
//      E[b,t,h] = exp(2 enc[b,t,h])      P[b,u,h] = exp(2 pred[b,u,h])
// computed ONCE per call here (B (T + U1) H exponentials, in double, rounded once to fp32), a hidden value costs the forward one fma,
// one reciprocal and one fma instead of add, multiply, exp2, add, reciprocal, fma.  Layout: k-step major,
//      Et[b][kc][t][16]   Pt[b][kc][u][16]      (kc = h / 16)
// so that the 32 rows of an MFMA tile (consecutive u) read one contiguous 2 KiB per k-step instead of 32 half cache lines.
// The factored form is exact only while neither factor has to be clamped: |enc|, |pred| <= 43 (2 x 43 x log2 e = 124 < 126; the
// product then over- / underflows to inf / 0 exactly where tanh saturates to +-1).  Beyond that — or with non-finite inputs — this
// kernel raises `ep_flag` and the forward runs its exact form (k_joint_fwd_x2<false>: tanh of the sum, from enc and pred) instead.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_x2_make_ep(X3Args a)
{
    const int H = a.H, H4 = H / 4, KC = H / 16;
    const long n_enc = (long)a.B * a.T * H4, n_all = n_enc + (long)a.B * a.U1 * H4;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    bool big = false;
    if (idx < n_all) {
        const bool is_enc = idx < n_enc;
        const long j = is_enc ? idx : idx - n_enc;
        const long row = j / H4;            // (b, t) or (b, u)
        const int h = (int)(j - row * H4) * 4;
        const int R = is_enc ? a.T : a.U1;  // rows per utterance
        const int b = (int)(row / R), r = (int)(row - (long)b * R);
        const float *src = is_enc ? a.enc + (long)b * a.enc_sb + (long)r * a.enc_st + h : a.pred + row * H + h;
        const f32x4 x = *(const f32x4 *)src;
        f32x4 y;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            big = big || !(fabsf(x[k]) <= 43.0f);  // (a NaN compares false: flagged too)
            double arg = (double)x[k] * 2.8853900817779268;  // 2 log2 e
            arg = arg > 126.0 ? 126.0 : (arg < -126.0 ? -126.0 : arg);
            y[k] = (float)exp2(arg);
        }
        float *dst = (is_enc ? a.ep_enc : a.ep_pred) + (((long)b * KC + (h >> 4)) * R + r) * 16 + (h & 15);
        *(f32x4 *)dst = y;
    }
    if (__builtin_amdgcn_ballot_w64(big) != 0 && (threadIdx.x & 63) == 0) atomicOr(a.ep_flag, 1u);
}
void launch_x2_make_ep(const X3Args &a, hipStream_t st)
{
    launch_fill32(a.ep_flag, 0u, 4, st);
    const long n = ((long)a.B * a.T + (long)a.B * a.U1) * (a.H / 4);
    hipLaunchKernelGGL(k_x2_make_ep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
}
size_t x2_ep_bytes(int B, int T, int U1, int H) { return ((size_t)B * T + (size_t)B * U1) * H * 4; }

// ---------------------------------------------------------------------------------------
// k_joint_fwd_x2: k_joint_fwd_x3 on two planes.  hidden = 2^14 tanh(enc + pred) split into its two fp16 planes (produced per
// k-step in fragment order by the lane that owns the slot), logits = hidden . W^T + bias (fp32, stored), log-softmax statistics
// and the two log-probs per lattice cell (as the fp32 route's forward).  Tile = 128 consecutive cells; 4 waves = 2 (M) x 2 (N),
// wave tile 64 cells x 256 columns = 16 accumulator tiles (256 registers); a pass = 512 logits columns, passes run back to
// back over one linear k-step sequence.  Per k-step 3 products x 16 MFMAs and ONE barrier, in the MIDDLE of the k-step (round 5):
//      block 0  ah.bh   + the 8 fragment reads of W(cs)'s mid plane + A(cs+1): the rcp / fma (tanh) pieces
//      block 1  am.bh   + the operand loads of k-step cs+2 + A(cs+1): the split pieces, then (5th tile) the two ring writes
//      --- this wave's share of W(cs+1) landed (one counted vmcnt), ONE barrier: A(cs+1), W(cs+1) published; W(cs)'s slot free ---
//      block 2  ah.bm   + the 12 fragment reads of k-step cs+1 (other register set) + the 8 DMAs of W(cs+3) + (first pass) 2 hidden stores
// (memory operations unconditional and in one fixed order per k-step — loads, DMAs, stores: every vmcnt is a count; every one of them
// is issued inside an MFMA's shadow, one per MFMA pair: four loads in a row in front of a block cost ~500 cycles of stall).
// W ring of THREE slots, filled THREE k-steps ahead (round 4: two ahead, barrier + 12 fragment reads in front of every k-step).
// The accumulators hold 2^14 s_W (logits - bias): the pass end multiplies by 2^-14 / s_W and adds the bias (one fma; the bias
// cannot ride in the accumulators' initial value here: the padding columns' -1e30 would overflow under the scale).
// Persistent workgroups, one per CU (115 KiB of LDS), tiles from one atomic counter.  Requires H % 128 == 0, V % 128 == 0.
// ---------------------------------------------------------------------------------------
#define XF2_WSLOT 32768
#define XF2_ASLOT 8192
#define XF2_NW 3   // W ring slots: the DMAs of k-step cs+3 are issued during k-step cs, behind its mid-step barrier
#ifdef RNNT_STAMPS
#ifndef X2S_WAVE
#define X2S_WAVE 0
#endif
// Diagnostic build only (-DRNNT_STAMPS): s_memtime stamps of workgroup 0, wave X2S_WAVE (0), k-steps 8..23 of its first tile:
// debug[(step-8)*8 + slot] (tools/exp_x3_stamps.py)
#define X2STAMP(slot)                                                                                       \
    do {                                                                                                    \
        if (a.debug && blockIdx.x == 0 && wave == X2S_WAVE && lane == 0 && it == 1 && cs >= 8 && cs < 24) {  \
            unsigned long long t_;                                                                          \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                       \
            a.debug[(cs - 8) * 8 + (slot)] = t_;                                                            \
        }                                                                                                   \
    } while (0)
#else
#define X2STAMP(slot) do {} while (0)
#endif
// MODE 1 (EP): hidden from the factored exponentials of k_x2_make_ep (the shipped form); MODE 0: the exact form — tanh of the sum, from
// enc and pred — for inputs outside the factored form's range.  Both are launched; `ep_flag` says which one runs (the other exits at once).
// MODE 2 (LIN): the same pipeline as a plain GEMM  Y[M,N] = X[M,K] W[N,K]^T (+ bias)  on the f16x2 pipes — the joint's input projections
// audio_ln / text_ln (reference rnnt/joint.py:8-12,26-30) and their data gradient: the A operand is a row of X scaled by a
// power of two and split (no tanh, no second operand, nothing stored beside Y), rows = cells with T = U1 = 1 (B = M, enc = X, enc_sb = its
// row stride, H = K, V = N, logits = Y, scales = {s_W, 1/s_W, s_X, 1/s_X}), no statistics, no lattice outputs; rows >= M are not stored.
template <int MODE>
__global__ __launch_bounds__(256, 1) void k_joint_fwd_x2(X3Args a, const int ntiles)
{
    constexpr bool EP = MODE == 1, LIN = MODE == 2;
    if (!LIN && (*a.ep_flag != 0) == EP) return;  // (wave-uniform: the whole grid of the form that is not selected leaves here)
    // [0, 96 KiB): W ring, 3 slots;  [96, 112 KiB): A ring, 2 slots;  then: s_den[128], s_part[2][128][2], s_next[2]
    extern __shared__ __attribute__((aligned(1024))) char s_fw[];
    float *s_den = (float *)(s_fw + XF2_NW * XF2_WSLOT + 2 * XF2_ASLOT);
    float *s_part = s_den + 128;  // [wn][row][max, sum]
    int *s_next = (int *)(s_part + 512);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int i = lane & 31, half = lane >> 5;
    const int H = a.H, V = a.V, KC = H / 16, U1 = a.U1, T = a.T;
    const int npass = (V + 511) / 512;
    const int NS = LIN ? KC : npass * KC;  // k-steps of a tile (LIN: a tile is ONE column pass of a row block — the passes of a plain GEMM share nothing)
    const long cells = (long)a.B * T * U1;
    const float unscale = (LIN ? a.scales[3] : X2_INV_SH) * a.scales[1];
    const float sx = LIN ? a.scales[2] : 1.0f;

    const int lds0 = (int)(size_t)(lds_vptr)s_fw;
    const int xa = lds0 + XF2_NW * XF2_WSLOT + (2 * wm) * 2048 + 16 * lane;  // A read: M tiles 2wm, 2wm+1: [slot][M tile][plane][lane]
    const int xw = lds0 + XF2_NW * XF2_WSLOT + wave * 2048 + 16 * lane;       // A write: M tile `wave` (this lane's own fragment slot)
    const int wb = lds0 + (8 * wn) * 1024 + 16 * lane;                  // W read: tiles 8wn .. 8wn+7 of each plane
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(a.wpack_fwd, 0, npass * KC * XF2_WSLOT, 0x00020000);
    const int wvo = lane * 16;

    X_CLOCK_STAMP(128 + 100);
    if (tid == 0) s_next[0] = (int)atomicAdd(a.counter, 1u);
    __syncthreads();
    int tile = s_next[0];
    for (int it = 1; tile < ntiles; ++it) {
        if (tid == 0) s_next[it & 1] = (int)atomicAdd(a.counter, 1u);
        const long row0 = (long)(LIN ? tile / npass : tile) * 128;
        const int pass0 = LIN ? tile % npass : 0, cs0 = pass0 * KC;  // LIN: this tile's column pass and the pack index of its first k-step
        __syncthreads();  // s_next visible; every wave is past the previous tile's LDS reads
        const int next = s_next[it & 1];
        // A tile entirely in the time steps past one utterance's length: its logits are never read (k_x2_dead_rows zeroes the
        // G rows dW reads of the tiles k_dhidden_x2 does not run), but its hidden rows must be finite (k_dw_x2 multiplies them by zeros): such a tile runs
        // the production of its first pass WITHOUT the MFMAs.
        bool dead = false;
        if (!LIN) {
            const long per = (long)T * U1, c_last = row0 + 127;
            const long b_first = row0 / per;
            dead = c_last < cells && c_last / per == b_first && (row0 - b_first * per) / U1 >= len_t(a.logit_lens, (int)b_first, T);
        }

        // ---- hidden = 2^14 tanh(enc + pred), produced per k-step IN FRAGMENT ORDER by the lane that owns the slot: lane
        // (i, half) of wave w holds row 32w + i, k = 16c + 8*half .. +7 of the MFMA A operand — 8 values from 2 x 32 bytes of
        // enc and pred, split two ways, 16 bytes per plane into the LDS ring of k-step c+1 and, in the first pass, to the
        // hidden planes in memory for k_dw_x2.  Later passes produce it again (the forward never re-reads hidden from memory).
        const long prow = row0 + 32 * wave + i;
        const long pc_ = prow < cells ? prow : cells - 1;  // rows past the lattice (last tile): any valid cell, never stored
        const int pu = (int)(pc_ % U1);
        const long pbt = pc_ / U1;
        const int pt = (int)(pbt % T), pb = (int)(pbt / T);
        // operand rows of this lane's cell.  EP: E = exp(2 enc), P = exp(2 pred), k-step major ([b][kc][row][16]: consecutive rows of a
        // k-step are contiguous); else enc and pred themselves, row major
        const float *ep = EP ? a.ep_enc + ((long)pb * KC * T + pt) * 16 + 8 * half : a.enc + (long)pb * a.enc_sb + (long)pt * a.enc_st + 8 * half;
        const float *pp = LIN ? ep : EP ? a.ep_pred + ((long)pb * KC * U1 + pu) * 16 + 8 * half : a.pred + ((long)pb * U1 + pu) * H + 8 * half;
        const long ek = EP ? (long)T * 16 : 16, pk = EP ? (long)U1 * 16 : 16;  // floats from one k-step's operands to the next's
        // (rows past the lattice produce — and store, unconditionally — the last cell's row again: the same bits to the
        // same place; hipcc counts vmcnt exactly only through unconditional memory operations)
        u32x4 *hdst = (u32x4 *)a.hidden + pc_ * (H / 8) + half;  // + 2c: this lane's 16 bytes of k-step c; planes `ps` apart
        const long ps = a.plane_stride / 8;
        struct Opd { f32x4 e0, e1, p0, p1; };
        struct Prod { f2 w[4]; float ra, rb; u32x4 ph, pm; };
        // operands of k index kcs (inside a pass): plain loads, hipcc keeps their vmcnt.  (Its count for a loop-carried register is
        // the MINIMUM over every path into the loop — vmcnt(3) / vmcnt(0) in front of block 0 here, which also waits for the W
        // DMAs issued behind these loads a k-step ago.  Spelling the loads as asm with a counted wait was tried and is WRONG: the
        // loaded registers are loop-carried, and the copies hipcc places on the loop's back edge read them before the data has
        // landed — intermittently different results at full size, tools/dbg_x2_loss.py.)
        auto op_load1 = [&](Opd &o, int kcs, int k) {  // one of the four 16-byte operand loads of k index kcs
            const float *e = ep + ek * kcs, *q = pp + pk * kcs;
            if (k == 0) o.e0 = *(const f32x4 *)e;
            else if (k == 1) o.e1 = *(const f32x4 *)(e + 4);
            else if (LIN) return;  // (one operand: two loads per k-step)
            else if (k == 2) o.p0 = *(const f32x4 *)q;
            else o.p1 = *(const f32x4 *)(q + 4);
        };
        auto op_load = [&](Opd &o, int kcs) {
#pragma unroll
            for (int k = 0; k < 4; ++k) op_load1(o, kcs, k);
        };
        // pieces 0-7: 2^14 tanh of the 4 pairs (fast_tanh2's arithmetic: exp2 half, reciprocal half); 8-15: the 2-way split
        // of each pair (hi + residuals, then mid); 16: the two ring writes
        auto prod_piece = [&](Prod &P, const Opd &o, auto off_c, int k) {  // off_c: byte offset of the target A slot in the ring
            if (k < 8) {
                const int j = k >> 1;
                const f32x4 &e = j < 2 ? o.e0 : o.e1, &pv = j < 2 ? o.p0 : o.p1;
                const int q = 2 * (j & 1);
                if (LIN) {  // s_X x, clamped into fp16's range (non-finite / garbage operands only)
                    if (!(k & 1)) P.w[j] = f2{F16x2::clamp(e[q] * sx), F16x2::clamp(e[q + 1] * sx)};
                } else if (EP) {  // 2^14 (1 - 2 / (1 + E P)): E P overflows to inf / underflows to 0 exactly where tanh is +-1
                    if (!(k & 1)) {
                        P.w[j] = f2{__builtin_amdgcn_rcpf(fmaf(e[q], pv[q], 1.0f)), __builtin_amdgcn_rcpf(fmaf(e[q + 1], pv[q + 1], 1.0f))};
                    } else {
                        P.w[j] = f2{fmaf(-2.0f * X2_SH, P.w[j][0], X2_SH), fmaf(-2.0f * X2_SH, P.w[j][1], X2_SH)};
                    }
                } else if (!(k & 1)) {
                    const f2 x = {e[q] + pv[q], e[q + 1] + pv[q + 1]};
                    const f2 av = x * (2.0f * RNNT_LOG2E);
                    P.w[j] = f2{__builtin_amdgcn_exp2f(av[0]), __builtin_amdgcn_exp2f(av[1])};
                } else {
                    const f2 ex = P.w[j] + 1.0f;
                    const f2 rr = {__builtin_amdgcn_rcpf(ex[0]), __builtin_amdgcn_rcpf(ex[1])};
                    P.w[j] = X2_SH - (2.0f * X2_SH) * rr;  // 2^14 (1 - 2 / (1 + e^2x)): the same rounding as the unscaled form
                }
            } else if (k < 16) {
                const int j = (k - 8) >> 1;
                if (!(k & 1)) {
                    const unsigned hh = pack_f16_pair(P.w[j][0], P.w[j][1]);
                    P.ph[j] = hh;
                    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(P.ra) : "v"(hh), "v"(P.w[j][0]));
                    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(P.rb) : "v"(hh), "v"(P.w[j][1]));
                } else {
                    P.pm[j] = pack_f16_pair(P.ra, P.rb);
                }
            } else {
                const int dst = xw;  // (a local: asm operands cannot name a capture of the enclosing generic lambda)
                asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(dst), "v"(P.ph), "n"(decltype(off_c)::value) : "memory");
                asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(dst), "v"(P.pm), "n"(decltype(off_c)::value + 1024) : "memory");
            }
        };
        auto hid_store = [&](const Prod &P, int kcs) { hdst[2 * kcs] = P.ph; hdst[2 * kcs + ps] = P.pm; };
        // piece n (0..7) of this wave's share of W k-step cs -> ring slot `slot`
        auto wdma = [&](int cs, int slot, int n) {  // raw-buffer form: scalar base and offsets, one constant per-lane offset register
            // pieces n = 4g .. 4g+3 share one LDS base (M0) and one scalar offset: the instruction's 12-bit immediate offset advances the
            // memory address AND the LDS address (LDS_ADDR = M0 + inst_offset + lane x 16) — the pack and the ring slot are both linear in n
            const int g4 = n & 4;
            if ((n & 3) == 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (lds_vptr)(s_fw + slot * XF2_WSLOT + (wave * 8 + g4) * 1024), 16, wvo, (cs * 32 + wave * 8 + g4) * 1024, 0, 0);
            if ((n & 3) == 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (lds_vptr)(s_fw + slot * XF2_WSLOT + (wave * 8 + g4) * 1024), 16, wvo, (cs * 32 + wave * 8 + g4) * 1024, 1024, 0);
            if ((n & 3) == 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (lds_vptr)(s_fw + slot * XF2_WSLOT + (wave * 8 + g4) * 1024), 16, wvo, (cs * 32 + wave * 8 + g4) * 1024, 2048, 0);
            if ((n & 3) == 3) __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (lds_vptr)(s_fw + slot * XF2_WSLOT + (wave * 8 + g4) * 1024), 16, wvo, (cs * 32 + wave * 8 + g4) * 1024, 3072, 0);
        };

        if (dead) {  // hidden rows only (finite values for k_dw_x2), no products
            for (int kc = 0; kc < KC; ++kc) {
                Opd o; Prod P;
                op_load(o, kc);
#pragma unroll
                for (int pc = 0; pc < 16; ++pc) prod_piece(P, o, Int<0>{}, pc);
                hid_store(P, kc);
            }
            tile = next;
            continue;
        }

        f32x16 acc[2][8];
        // running (max, sum exp) over the columns of this wave's half (wn) seen so far, in registers across the passes: lane
        // (i, half) keeps row slot i = 16 mt + r of the wave's 2 x 16 (row_of(mt, r) + 4 half) and hands it to s_part behind the last pass
        float m_run = RNNT_NEG_INF, s_run = 0.f;
        auto acc_init = [&]() {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int q = 0; q < 8; ++q)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[mt][q][r] = 0.f;
        };
        // pipeline prologue: W of k-steps 0, 1 and 2 by DMA; A of k-step 0 produced, stored, written to ring slot 0; operands of
        // k-step 1 requested; then everything landed + one barrier, and the fragments of k-step 0 (A slot 0, W slot 0: hi plane) read
        Opd oset[2];  // operands of k-step cs+1 live in oset[(cs+1) & 1] during k-step cs (KC is even: the k loop is unrolled by 2)
        // MFMA fragments of the CURRENT k-step, read during the previous one (two sets alternating by k-step parity: compile-time)
        struct Frag { u32x4 af[2][2], bf[8]; };
        Frag fr[2];
        // read n (0..11) of a k-step's fragments: 0-3 the A fragments (slot at byte offset xs_c of the A ring), 4-11 W's hi plane (slot `wslot`)
        auto frag_read1 = [&](Frag &f, auto xs_c, const int wslot, const int n) {  // (n: a constant once the caller's loop is unrolled)
            const int xs = xa, ws = wb + wslot * XF2_WSLOT;
            if (n < 4) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(f.af[(n >> 1) & 1][n & 1]) : "v"(xs), "n"(decltype(xs_c)::value + ((n >> 1) & 1) * 2048 + (n & 1) * 1024));
            else asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(f.bf[n >= 4 ? n - 4 : 0]) : "v"(ws), "n"((n >= 4 ? n - 4 : 0) * 1024));
        };
        auto frag_read = [&](Frag &f, auto xs_c, const int wslot) {
#pragma unroll
            for (int n = 0; n < 12; ++n) frag_read1(f, xs_c, wslot, n);
        };
        // the fragments have landed: every register of the set is named, so that nothing hipcc places behind this point (the loop's
        // back-edge copies of loop-carried registers included) reads one before its data is there
        auto frag_landed = [&](Frag &f) {
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(f.af[0][0]), "+v"(f.af[0][1]), "+v"(f.af[1][0]), "+v"(f.af[1][1]),
                           "+v"(f.bf[0]), "+v"(f.bf[1]), "+v"(f.bf[2]), "+v"(f.bf[3]), "+v"(f.bf[4]), "+v"(f.bf[5]), "+v"(f.bf[6]), "+v"(f.bf[7])
                         :: "memory");
        };
        {
#pragma unroll
            for (int n = 0; n < 8; ++n) wdma(cs0, 0, n);
#pragma unroll
            for (int n = 0; n < 8; ++n) wdma(cs0 + (NS > 1 ? 1 : 0), 1, n);
#pragma unroll
            for (int n = 0; n < 8; ++n) wdma(cs0 + (NS > 2 ? 2 : NS - 1), 2, n);
            Opd o; Prod P;
            op_load(oset[1], KC > 1 ? 1 : 0);
            op_load(o, 0);
#pragma unroll
            for (int pc = 0; pc < 17; ++pc) prod_piece(P, o, Int<0>{}, pc);
            if (!LIN) hid_store(P, 0);  // (the plain GEMM stores nothing beside Y: X3Args::hidden is null there)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // W of k-steps 0-2 (this wave's share), operands, the stores
            lds_barrier();                                 // ... of every wave; A slot 0 written
            frag_read(fr[0], Int<0>{}, 0);
            frag_landed(fr[0]);
        }

        int cs = 0, wsl = 0;  // k-step (linear over the passes) and its W ring slot (cs % 3)
        // one pass; STORE: the first — the produced planes also go to memory.  Two straight-line instantiations, the first pass
        // outside the loop over the others (a branch between two k loops, like a conditional accumulator re-initialisation
        // inside one, makes hipcc carry the 256 accumulator registers through VGPR phis and spill)
        auto run_pass = [&](auto store_c, const int pass) {
          acc_init();
          constexpr bool STORE = decltype(store_c)::value != 0;
          // One k-step (round 5: the barrier sits in the MIDDLE of the k-step and the fragments of a k-step are read during the
          // one before — the round-4 form paid barrier + 12 fragment reads, ~370 of 2 860 cycles, in front of every k-step's MFMAs):
          //   block 0  ah.bh  + the 8 reads of W(cs)'s mid plane + A(cs+1): the tanh pieces
          //            the operand loads of k-step cs+2
          //   block 1  am.bh  + A(cs+1): the split pieces, then its two ring writes
          //   --- this wave's share of W(cs+1) landed (counted vmcnt), its ring writes done, ONE barrier: A(cs+1) and W(cs+1) are
          //       published, and every wave is past its last read of W(cs): that ring slot is free ---
          //   block 2  ah.bm  + the 12 fragment reads of k-step cs+1 (into the other register set) + the 8 DMAs of W(cs+3) into
          //            the slot W(cs) just left (three slots, filled THREE k-steps ahead) + (first pass) the 2 hidden stores
          // PAR = the k-step's parity = its A ring slot and fragment register set (KC is even: cs and kc have the same parity).
          auto kstep = [&](auto par_c, const int kc) {
            constexpr int par = decltype(par_c)::value;
            constexpr int XN = (1 - par) * XF2_ASLOT;
            Frag &fc = fr[par], &fn = fr[1 - par];
            const int ws = wb + wsl * XF2_WSLOT;  // (the W slot is a run-time third: one v_add per k-step)
            // the k-step whose W is requested now (past the end: the last one again, never read), the next k-step of the pass and
            // the one after (operand loads)
            const int csn = cs0 + (cs + 3 < NS ? cs + 3 : NS - 1), kcn = kc + 1 < KC ? kc + 1 : 0, kcnn = kcn + 1 < KC ? kcn + 1 : 0;
            const int wsn = wsl == 2 ? 0 : wsl + 1;  // (cs + 1) % 3: the slot whose fragments are read in block 2
            const Opd &ocur = oset[(par + 1) & 1];  // operands of k-step cs+1 (requested during the previous k-step)
            Opd &onext = oset[par & 1];       // refilled with those of k-step cs+2
            Prod P;
            u32x4 bn[8];
            X2STAMP(0);
            auto block = [&](auto pa_c, const u32x4 (&bcur)[8], auto blk_c) {
                constexpr int PA = decltype(pa_c)::value, BLK = decltype(blk_c)::value;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    acc[0][q] = mfma_f16(fc.af[0][PA], bcur[q], acc[0][q]);
                    acc[1][q] = mfma_f16(fc.af[1][PA], bcur[q], acc[1][q]);
                    if (BLK == 0) {
                        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bn[q]) : "v"(ws), "n"(16384 + q * 1024));
                        prod_piece(P, ocur, Int<XN>{}, q);
                    }
                    if (BLK == 1) {
                        if (q < (LIN ? 2 : 4)) op_load1(onext, kcnn, q);  // operands of k-step cs+2 (needed a whole k-step from now): in FRONT of the k-step's DMAs
                        if (q < 4) { prod_piece(P, ocur, Int<XN>{}, 8 + 2 * q); prod_piece(P, ocur, Int<XN>{}, 9 + 2 * q); }
                        if (q == 4) prod_piece(P, ocur, Int<XN>{}, 16);  // the ring writes: done well before the barrier's lgkmcnt(0)
                    }
                    if (BLK == 2) {  // nothing of the k-step is issued outside an MFMA's shadow: the 12 fragment reads of k-step cs+1, the 8 DMAs, the 2 stores
                        if (q < 4) { frag_read1(fn, Int<XN>{}, wsn, 2 * q); frag_read1(fn, Int<XN>{}, wsn, 2 * q + 1); }
                        else frag_read1(fn, Int<XN>{}, wsn, 4 + q);
                        wdma(csn, wsl, q);
                        if (STORE && q == 6) hdst[2 * kcn] = P.ph;
                        if (STORE && q == 7) hdst[2 * kcn + ps] = P.pm;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            block(Int<0>{}, fc.bf, Int<0>{});   // ah.bh
            X2STAMP(1);
            block(Int<1>{}, fc.bf, Int<1>{});   // am.bh
            X2STAMP(2);
            // this wave's share of W(cs+1) landed: its DMAs were issued in block 2 of k-step cs-2.  vmcnt retires in order; behind
            // them came (first pass) 2 hidden stores, k-step cs-1's 4 operand loads, 8 DMAs and (first pass) 2 stores, and this
            // k-step's 4 operand loads.  The first two k-steps of a pass: their W(cs+1) was waited for before the previous pass's
            // logits stores (pass end below) / with the tile prologue.
            if (kc >= 2) {
                constexpr int NV = LIN ? 12 : (STORE ? 4 : 0) + 4 + 8 + 4;
                static_assert(NV == 12 || NV == 16 || NV == 20, "counted vmcnt of the forward's k-step");
                if (NV == 12) asm volatile(RNNT_VMCNT(12) ::: "memory");  // (LIN: 2 operand loads per k-step: 2 + 8 + 2)
                else if (NV == 16) asm volatile(RNNT_VMCNT(16) ::: "memory");
                else asm volatile(RNNT_VMCNT(20) ::: "memory");
            }
            X2STAMP(3);
            lds_barrier();  // (lgkmcnt(0): bn and the ring writes) publishes A(cs+1), W(cs+1); frees W(cs)'s slot
            X2STAMP(4);
            asm volatile("" : "+v"(bn[0]), "+v"(bn[1]), "+v"(bn[2]), "+v"(bn[3]), "+v"(bn[4]), "+v"(bn[5]), "+v"(bn[6]), "+v"(bn[7]));
            block(Int<0>{}, bn, Int<2>{});   // ah.bm  (the hidden stores: the youngest memory operations of the k-step; the pass's last k-step re-stores k-step 0)
            frag_landed(fn);
            X2STAMP(5);
            (void)kcn;
            ++cs;
            wsl = wsn;
          };
          for (int kc0 = 0; kc0 < KC; kc0 += 2) { kstep(Int<0>{}, kc0); kstep(Int<1>{}, kc0 + 1); }
          // pass complete: unscale, add the bias, store the logits, update the statistics.  V % 128 == 0: a lane's two 4-column
          // groups exist or not for the whole wave.  The row loop is ONE basic block per case; the store address is a scalar
          // row pointer + one 32-bit per-lane offset.
          // (W of the next pass's first two k-steps — requested during the last two above — lands before the logits stores are
          // queued behind it: the k-steps' counted waits cannot see past 63 younger operations)
          if (STORE) asm volatile(RNNT_VMCNT(2) ::: "memory");
          else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          {
            const int cw = 512 * pass + 256 * wn;
            const unsigned lane_off = (unsigned)(((4 * half) * V + 4 * i) * 4);
            char *tile_base = (char *)(a.logits + row0 * V + cw);
            const bool has_b = !LIN || a.bias != nullptr;
            const f32x4 b0 = has_b && cw + 4 * i < V ? *(const f32x4 *)(a.bias + cw + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
            const f32x4 b1 = has_b && cw + 128 + 4 * i < V ? *(const f32x4 *)(a.bias + cw + 128 + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
            auto epilogue = [&](auto both_c) {
                constexpr bool BOTH = decltype(both_c)::value != 0;
                // one row slot's logits: unscale + bias.  The accumulator reads are spelled as (volatile) asm: they stay here —
                // left to hipcc, all 256 v_accvgpr_read are hoisted in front of the first store and spilled
                auto read_slot = [&](int mt, int r, f32x4 &o0, f32x4 &o1) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float x0, x1;
                        asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(x0) : "a"(acc[mt][q][r]));
                        asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(x1) : "a"(acc[mt][4 + q][r]));
                        o0[q] = fmaf(x0, unscale, b0[q]); o1[q] = fmaf(x1, unscale, b1[q]);
                    }
                };
                auto row_of = [&](int mt, int r) { return 32 * (2 * wm + mt) + (r & 3) + 8 * (r >> 2); };  // (+ 4 half: this lane's row of the slot)
                if constexpr (LIN) {  // the plain GEMM: the stores alone, a pair of row slots at a time
                    // (reads and row spelled out here, not through read_slot / row_of: at 255 VGPRs this form's register allocation
                    // turns on such details — through them hipcc spilled 70 registers across the k loop instead of 11)
                    auto slot = [&](int mt, int r) {
                        f32x4 o0, o1;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            float x0, x1;
                            asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(x0) : "a"(acc[mt][q][r]));
                            asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(x1) : "a"(acc[mt][4 + q][r]));
                            o0[q] = fmaf(x0, unscale, b0[q]); o1[q] = fmaf(x1, unscale, b1[q]);
                        }
                        char *rowp = tile_base + (long)(32 * (2 * wm + mt) + (r & 3) + 8 * (r >> 2)) * V * 4;  // wave-uniform
                        // Y has no padding rows: rows past M are not stored (the k loop's memory operations stay unconditional)
                        if (row0 + 32 * (2 * wm + mt) + (r & 3) + 8 * (r >> 2) + 4 * half < cells) {
                            *(f32x4 *)(rowp + lane_off) = o0;
                            if (BOTH) *(f32x4 *)(rowp + lane_off + 512) = o1;
                        }
                    };
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int r = 0; r < 16; r += 2) {
                            slot(mt, r);
                            slot(mt, r + 1);
                            __builtin_amdgcn_sched_barrier(0);  // (a pair at a time: see the accumulator reads)
                        }
                } else {
                    // FOUR row slots at a time, in straight-line phases with no branch and no LDS access: with one wave per SIMD a slot
                    // is a chain of dependent latencies (accumulator reads, the two DPP reductions, exp2); the phases put the four
                    // slots' chains side by side, and the two reductions run interleaved step by step (half_max_dpp_x4 / half_sum_dpp_x4).
                    // A slot's (max, sum exp) over this pass's columns go from lanes 31 / 63 to the lanes that keep the slot's rows
                    // (v_readlane + v_writelane); the running update is ONE unconditional sequence per pass, behind the last group.
                    int m_pass = 0, s_pass = 0;  // (every lane is written: 32 slots x 2 halves)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int r0 = 0; r0 < 16; r0 += 4) {
                            f32x4 o0[4], o1[4];
                            float mx[4], sm[4];
                            // (a) unscale + bias, store, the lane's maximum over its 4 / 8 columns
#pragma unroll
                            for (int g = 0; g < 4; ++g) {
                                read_slot(mt, r0 + g, o0[g], o1[g]);
                                char *rowp = tile_base + (long)row_of(mt, r0 + g) * V * 4;  // wave-uniform
                                __builtin_nontemporal_store(o0[g], (f32x4 *)(rowp + lane_off));
                                if (BOTH) __builtin_nontemporal_store(o1[g], (f32x4 *)(rowp + lane_off + 512));
                                float m8 = fmaxf(fmaxf(o0[g][0], o0[g][1]), fmaxf(o0[g][2], o0[g][3]));
                                if (BOTH) m8 = fmaxf(m8, fmaxf(fmaxf(o1[g][0], o1[g][1]), fmaxf(o1[g][2], o1[g][3])));
                                mx[g] = m8;
                            }
                            // (b) the maxima over the 32 lanes of each half (lanes 31 / 63 hold them)
                            half_max_dpp_x4(mx[0], mx[1], mx[2], mx[3]);
                            // (c) to every lane of the half and to the slot's lane pair of m_pass; sum exp over the lane's columns
#pragma unroll
                            for (int g = 0; g < 4; ++g) {
                                const int lo = __builtin_amdgcn_readlane(__float_as_int(mx[g]), 31), hi = __builtin_amdgcn_readlane(__float_as_int(mx[g]), 63);
                                asm("v_writelane_b32 %0, %1, %2" : "+v"(m_pass) : "s"(lo), "n"(16 * mt + r0 + g));
                                asm("v_writelane_b32 %0, %1, %2" : "+v"(m_pass) : "s"(hi), "n"(32 + 16 * mt + r0 + g));
                                const float M = __int_as_float(half ? hi : lo);
                                const float nm2 = -M * RNNT_LOG2E;
                                float e = (__builtin_amdgcn_exp2f(fmaf(o0[g][0], RNNT_LOG2E, nm2)) + __builtin_amdgcn_exp2f(fmaf(o0[g][1], RNNT_LOG2E, nm2))) +
                                          (__builtin_amdgcn_exp2f(fmaf(o0[g][2], RNNT_LOG2E, nm2)) + __builtin_amdgcn_exp2f(fmaf(o0[g][3], RNNT_LOG2E, nm2)));
                                if (BOTH)
                                    e += (__builtin_amdgcn_exp2f(fmaf(o1[g][0], RNNT_LOG2E, nm2)) + __builtin_amdgcn_exp2f(fmaf(o1[g][1], RNNT_LOG2E, nm2))) +
                                         (__builtin_amdgcn_exp2f(fmaf(o1[g][2], RNNT_LOG2E, nm2)) + __builtin_amdgcn_exp2f(fmaf(o1[g][3], RNNT_LOG2E, nm2)));
                                sm[g] = e;
                            }
                            // (d) the sums over the 32 lanes of each half (lanes 31 / 63 hold them), to the slot's lane pair of s_pass
                            half_sum_dpp_x4(sm[0], sm[1], sm[2], sm[3]);
#pragma unroll
                            for (int g = 0; g < 4; ++g) {
                                const int lo = __builtin_amdgcn_readlane(__float_as_int(sm[g]), 31), hi = __builtin_amdgcn_readlane(__float_as_int(sm[g]), 63);
                                asm("v_writelane_b32 %0, %1, %2" : "+v"(s_pass) : "s"(lo), "n"(16 * mt + r0 + g));
                                asm("v_writelane_b32 %0, %1, %2" : "+v"(s_pass) : "s"(hi), "n"(32 + 16 * mt + r0 + g));
                            }
                            __builtin_amdgcn_sched_barrier(0);  // (a group at a time: see the accumulator reads)
                        }
                    // (e) the running statistics of all 32 slots at once, each lane its own row's
                    const float M = __int_as_float(m_pass), S_ = __int_as_float(s_pass);
                    const float m_o = m_run, s_o = s_run;
                    const float mn = fmaxf(m_o, M);
                    m_run = mn;
                    // (the fma spelled out, its addend a rounded product: what hipcc made of  s_o exp2(..) + S exp2(..)  when the update was
                    // the tail of a row slot — left to contraction, the same line comes out as other roundings here)
                    s_run = fmaf(s_o, __builtin_amdgcn_exp2f((m_o - mn) * RNNT_LOG2E), S_ * __builtin_amdgcn_exp2f((M - mn) * RNNT_LOG2E));
                }
            };
            if (cw + 128 < V) epilogue(Int<1>{});
            else if (cw < V) epilogue(Int<0>{});
          }
        };
        run_pass(Int<(LIN ? 0 : 1)>{}, pass0);
        if (!LIN)
            for (int pass = 1; pass < npass; ++pass) run_pass(Int<0>{}, pass);

        // ---- log-softmax denominators: the two column halves (wn) of every row.  s_part[wn][row] = the row's (max, sum exp) over
        // that half's columns of every pass: all 256 entries are written, a half without columns (V = 128) leaves (-inf, 0)
        if (!LIN) {
            float *sp = s_part + (wn * 128 + 32 * (2 * wm + (i >> 4)) + (i & 3) + 8 * ((i & 15) >> 2) + 4 * half) * 2;
            sp[0] = m_run;
            sp[1] = s_run;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // every logits / hidden store of the workgroup has left its wave; s_part complete
        if (LIN) { tile = next; continue; }
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
        tile = next;
    }
    X_CLOCK_STAMP(128 + 102);
}

void launch_joint_fwd_x2(const X3Args &a, hipStream_t st, bool lin /* the plain-GEMM form, k_joint_fwd_x2<2>: the joint's input projections */)
{
    const int lds = XF2_NW * XF2_WSLOT + 2 * XF2_ASLOT + 128 * 4 + 2 * 128 * 2 * 4 + 16;
    static LdsOptIn lds_opt_in;
    lds_opt_in.raise(lds, k_joint_fwd_x2<1>, k_joint_fwd_x2<0>, k_joint_fwd_x2<2>);
    const long cells = (long)a.B * a.T * a.U1;
    const int ntiles = (int)((cells + 127) / 128) * (lin ? (a.V + 511) / 512 : 1);  // (plain GEMM: a tile = one column pass of a row block)
    if (!lin) launch_fill32(a.counter, 0u, 4, st);  // tile counter of the persistent workgroups (plain GEMM: zeroed with its scales, k_x2_lin_scales)
    const int nwg = ntiles < a.n_cu ? ntiles : a.n_cu;  // one workgroup per CU
    // both forms; k_x2_make_ep's flag (device memory: no host round trip) selects the one that runs, the other's workgroups exit at once
    if (lin) { hipLaunchKernelGGL(k_joint_fwd_x2<2>, dim3((unsigned)nwg), dim3(256), lds, st, a, ntiles); return; }
    hipLaunchKernelGGL(k_joint_fwd_x2<1>, dim3((unsigned)nwg), dim3(256), lds, st, a, ntiles);
    hipLaunchKernelGGL(k_joint_fwd_x2<0>, dim3((unsigned)nwg), dim3(256), lds, st, a, ntiles);
}

void launch_x2_pack_w(const X3Args &a, float *scales, hipStream_t st)
{
    hipLaunchKernelGGL(k_x2_wscale, dim3(1), dim3(1024), 0, st, a.W, (long)a.V * a.H / 4, scales);
    launch_split_pack_w<F16x2>(a, scales, st);
}


// ---------------------------------------------------------------------------------------
// The joint's input projections on the f16x2 pipes (round 5; reference rnnt/joint.py:8-12,26-30: audio_ln / text_ln are
// nn.Linear layers applied to the encoder / predictor outputs before the joint).  A Linear layer and its backward are three GEMMs:
//      y  = x W^T + b        (M x K) (N x K)^T   -> k_joint_fwd_x2<2>: the joint forward's pipeline as a plain GEMM (rows of x split on the fly)
//      dx = dy W             (M x N) (K x N)^T   -> the same kernel on W^T (a 64 x 64-tiled transposing copy of the weight)
//      dW = dy^T x, db = column sums of dy       -> k_dw_x2<4>, unchanged: dy as the "G" operand (two fp16 planes interleaved per
//                                                   32-column chunk), x as the "hidden" operand (two separate planes), K = the M rows
// Operand scales (powers of two) come from the data's largest magnitude, found on the device every call (k_x2_absmax + k_x2_lin_scales);
// the packs / planes are scaled when they are made and the outputs unscaled where they are written.  K % 128 == 0, N % 128 == 0.
// Workspace (caller-owned, rnnt_engine_linear_x2_workspace_bytes): 512 B of scale / counter words, then the forward's W pack
// (forward) or W^T, its pack, dy's and x's planes and the dW split-K slabs (backward).
// ---------------------------------------------------------------------------------------
// largest magnitudes of up to three row-major matrices in ONE launch: grid (256, n), workgroup (b, t) leaves the maximum of its share of
// tensor t in partial[t][b] — no atomics, nothing to zero first (round 5: an atomicMax per wave of 1 024 workgroups on one word took 48 us for
// a 4 MB tensor — the 4 096 same-address atomics, not the bytes — five times per Linear forward + backward: 0.25 of its 0.62 ms at 6 432 rows)
struct X2AbsArgs { const float *x[3]; long ld[3], rows[3]; int cols4[3]; };
__global__ __launch_bounds__(256) void k_x2_absmax(X2AbsArgs a, float *__restrict__ partial)
{
    __shared__ float s_m[4];
    const int t = blockIdx.y;
    const float *x = a.x[t];
    const long ld = a.ld[t], n = a.rows[t] * a.cols4[t];
    const int cols4 = a.cols4[t];
    float m = 0.f;
    bool bad = false;  // a NaN or an infinity among the entries (fmaxf drops NaNs; the split's clamp would turn either into a finite fp16)
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
        const long r = idx / cols4;
        const int c = (int)(idx - r * cols4);
        const f32x4 w = *(const f32x4 *)(x + r * ld + 4 * c);
        const float mw = fmaxf(fmaxf(fabsf(w[0]), fabsf(w[1])), fmaxf(fabsf(w[2]), fabsf(w[3])));
        bad = bad || !(fabsf(w[0]) <= X2_F32_MAX) || !(fabsf(w[1]) <= X2_F32_MAX) || !(fabsf(w[2]) <= X2_F32_MAX) || !(fabsf(w[3]) <= X2_F32_MAX);
        m = fmaxf(m, mw);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    // a non-finite operand leaves a NaN as its workgroup's "maximum": k_x2_lin_scales turns it into a NaN reciprocal scale, and every output
    // the operand feeds is multiplied by that — non-finite inputs give non-finite outputs, as torch.nn.functional.linear's do (round-5 advice)
    if (threadIdx.x == 0) partial[t * 256 + blockIdx.x] = any_bad ? __uint_as_float(0x7fc00000u) : fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
}
// one workgroup of 256: scales[2i] = 2^(14 - ceil(log2 max_i)), scales[2i + 1] = its reciprocal (1 for an all-zero operand; NaN for an operand with a NaN or an infinity in it),
// i = 0 .. n-1, from the partial maxima; the call's counter words zeroed (the forward's tile counter; dW's progress words) and dW's lists written
// (nks 16-row k-steps, every one live) — what four more launches did before
__global__ __launch_bounds__(256) void k_x2_lin_scales(const float *__restrict__ partial, float *__restrict__ scales, int n, unsigned *__restrict__ zero0,
                                                       int nzero0, unsigned *__restrict__ zero1, int nzero1, long nks,
                                                       int *__restrict__ list, int *__restrict__ stats, int *__restrict__ glist)
{
    __shared__ float s_m[4];
    for (int i = 0; i < n; ++i) {
        float m = partial[i * 256 + threadIdx.x];
        const int nonfinite = __syncthreads_or(m != m ? 1 : 0);  // (k_x2_absmax: NaN = the operand holds a NaN or an infinity)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        __syncthreads();
        if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0 && nonfinite) {  // the planes / packs are finite garbage (scale 1, clamped); the outputs' unscale factor is NaN
            scales[2 * i] = 1.0f;
            scales[2 * i + 1] = __uint_as_float(0x7fc00000u);
        } else if (threadIdx.x == 0) {
            const unsigned bits = __float_as_uint(fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3])));
            float s = 1.0f;
            const int e = (int)(bits >> 23) & 0xff;
            if (e > 0 && e < 255) {
                int k = 14 - (e - 126);
                k = k > 100 ? 100 : (k < -100 ? -100 : k);
                s = __uint_as_float((unsigned)(127 + k) << 23);
            }
            scales[2 * i] = s;
            scales[2 * i + 1] = 1.0f / s;
        }
    }
    for (int j = threadIdx.x; j < nzero0; j += 256) zero0[j] = 0u;
    for (int j = threadIdx.x; j < nzero1; j += 256) zero1[j] = 0u;
    if (list) {  // the dW kernels' lists (launch_x2_live's format): every 16-row k-step (k_dw_x2m) and every 4-row group (k_dw_x2), then the padding entries
        const long ngrp = 4 * nks;
        for (long j = threadIdx.x; j < nks + 8; j += 256) list[j] = (int)(j < nks ? j : nks);
        for (long j = threadIdx.x; j < ngrp + XL2_GPAD; j += 256) glist[j] = (int)(j < ngrp ? j : ngrp);
        if (threadIdx.x == 0) { stats[0] = (int)nks; stats[1] = (int)nks; stats[2] = 0; stats[3] = 0; stats[4] = (int)ngrp; stats[5] = (int)ngrp; }
    }
}
// rows of a row-major fp32 matrix -> s x as two fp16 planes.  INTER: the planes interleaved per 32-column chunk, [32 x hi | 32 x mid] over the
// chunk's 128 bytes (the G operand's layout: one thread = one chunk); else two separate planes `plane_stride` elements apart (the hidden
// operand's layout: one thread = 8 columns).
template <bool INTER>
__global__ __launch_bounds__(256) void k_x2_split_rows(const float *__restrict__ x, long ld, long rows, long rows_out, int cols,
                                                       const float *__restrict__ scale, void *__restrict__ dst, long plane_stride)
{
    // rows [rows, rows_out): zeros (the padding rows the dW kernel's last k-steps read; three fill launches before)
    const float s = scale[0];
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (INTER) {
        const int VC = cols / 32;
        if (idx >= rows_out * VC) return;
        const long r = idx / VC;
        const int c = (int)(idx - r * VC);
        const f32x4 *p = (const f32x4 *)(x + (r < rows ? r : 0) * ld + 32 * c);
        u32x4 ph[4], pm[4];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            f32x4 v = r < rows ? p[i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = F16x2::clamp(v[k] * s);
            F16x2::split4(v, ph[i >> 1], pm[i >> 1], 2 * (i & 1));
        }
        u32x4 *o = (u32x4 *)((float *)dst + r * cols + 32 * c);
#pragma unroll
        for (int i = 0; i < 4; ++i) { o[i] = ph[i]; o[4 + i] = pm[i]; }
    } else {
        const int H8 = cols / 8;
        if (idx >= rows_out * H8) return;
        const long r = idx / H8;
        const int h = (int)(idx - r * H8) * 8;
        const float *xr = x + (r < rows ? r : 0) * ld + h;
        f32x4 t0 = *(const f32x4 *)xr, t1 = *(const f32x4 *)(xr + 4);
        if (r >= rows) t0 = t1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) { t0[k] = F16x2::clamp(t0[k] * s); t1[k] = F16x2::clamp(t1[k] * s); }
        u32x4 ph, pm;
        F16x2::split4(t0, ph, pm, 0);
        F16x2::split4(t1, ph, pm, 2);
        u32x4 *o = (u32x4 *)((unsigned short *)dst + r * cols + h);
        o[0] = ph; o[plane_stride / 8] = pm;
    }
}
// out[i] = scale_a scale_b sum_s slab[s][i]  (fixed order: bitwise reproducible)
__global__ __launch_bounds__(256) void k_x2_reduce_scaled(const float *__restrict__ slab, float *__restrict__ out, long n4, long stride4, int nsplit,
                                                          const float *__restrict__ sa, const float *__restrict__ sb)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 acc = ((const f32x4 *)slab)[i];
    for (int s = 1; s < nsplit; ++s) acc += ((const f32x4 *)slab)[i + s * stride4];
    const float r = sa[0] * (sb ? sb[0] : 1.0f);
    ((f32x4 *)out)[i] = acc * r;
}

// compute units of the CURRENT device (the caller makes the tensors' device current); read-only facts of the hardware, cached per device id
int device_cus()
{
    static thread_local int cus[16] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
    if (!cus[dev]) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, dev) == hipSuccess) cus[dev] = p.multiProcessorCount;
        if (cus[dev] <= 0) cus[dev] = 256;
    }
    return cus[dev];
}

namespace {
struct LinWs { size_t wt, pack, pa, pb, slab_w, slab_b, prog, list, glist, total; long rows_pad, rows_alloc; int n_split; };
LinWs lin_layout(int M, int K, int N, bool bwd)
{
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    LinWs L{};
    size_t o = 4096;  // +0 scales[8], +128 tile counter, +1024 the partial maxima [3][256]
    if (!bwd) { L.pack = o; o += al(x2_wpack_fwd_bytes(K, N)); L.total = o; return L; }
    L.rows_pad = ((long)M + 1 + 31) / 32 * 32;
    L.rows_alloc = (L.rows_pad + 96 + 127) / 128 * 128;
    const long tiles = x2_dw_tiles(K, N);  // (the dW kernel's H = K, V = N)
    long ns = 256 / tiles;
    if (ns < 1) ns = 1;
    if (ns > L.rows_pad / 32) ns = L.rows_pad / 32;
    L.n_split = (int)ns;
    L.wt = o; o += al((size_t)N * K * 4);
    L.pack = o; o += al(x2_wpack_fwd_bytes(N, K));       // pack of W^T as the [K x N] "weight" of dx = dy (W^T)^T
    L.pa = o; o += al((size_t)L.rows_alloc * N * 4);     // dy: interleaved planes
    L.pb = o; o += al((size_t)L.rows_alloc * K * 4);     // x: two planes
    L.slab_w = o; o += al((size_t)L.n_split * N * K * 4);
    L.slab_b = o; o += al((size_t)L.n_split * N * 4);
    L.prog = o; o += al((size_t)L.n_split * 64);
    L.list = o; o += al(64 + (size_t)(L.rows_pad / XW2_ROWS + 8) * 4);  // the count words, then the k-step list
    L.glist = o; o += al((size_t)(L.rows_pad / 4 + XL2_GPAD) * 4);        // the group list
    L.total = o;
    return L;
}
// the operand scales of a call: one launch for the maxima of its n tensors, one for the scales (+ the counter words and dW's lists)
struct LinT { const float *x; long ld, rows; int cols; };
void lin_scales(const LinT *t, int n, char *w, unsigned *zero1, int nzero1, long nks, int *list, int *glist, hipStream_t st)
{
    X2AbsArgs a{};
    for (int i = 0; i < n; ++i) { a.x[i] = t[i].x; a.ld[i] = t[i].ld; a.rows[i] = t[i].rows; a.cols4[i] = t[i].cols / 4; }
    float *partial = (float *)(w + 1024);
    hipLaunchKernelGGL(k_x2_absmax, dim3(256, n), dim3(256), 0, st, a, partial);
    hipLaunchKernelGGL(k_x2_lin_scales, dim3(1), dim3(256), 0, st, partial, (float *)w, n, (unsigned *)(w + 128), 16, zero1, nzero1, nks,
                       list ? list + 16 : nullptr, list, glist);
}
// y[M,N] = x[M,K] wmat[N,K]^T (+ bias) through k_joint_fwd_x2<2>; scales = {s_W, 1/s_W, s_X, 1/s_X} on the device, the pack made here
void lin_gemm_nt(const float *x, long ldx, const float *wmat, const float *bias, int M, int K, int N, float *y, const float *scales, void *pack,
                 unsigned *counter, hipStream_t st)
{
    const long nf = (long)((N + 511) / 512) * (K / 16) * 16 * 64;
    hipLaunchKernelGGL(k_split_pack_w_fwd<F16x2>, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, wmat, scales, (u32x4 *)pack, K, N, nf);
    X3Args a{};
    a.enc = x; a.enc_sb = ldx; a.enc_st = 0; a.pred = nullptr; a.W = wmat; a.bias = bias;
    a.B = M; a.T = 1; a.U1 = 1; a.H = K; a.V = N; a.logits = y; a.wpack_fwd = pack; a.scales = scales;
    a.counter = counter; a.n_cu = device_cus();  // (the counter was zeroed by k_x2_lin_scales)
    launch_joint_fwd_x2(a, st, true);  // the plain-GEMM form
}
}  // namespace

size_t x2_linear_ws_bytes(int M, int K, int N, bool bwd) { return lin_layout(M, K, N, bwd).total; }
bool x2_linear_ok(int M, int K, int N) { return M > 0 && K % 128 == 0 && N % 128 == 0 && split_fwd_ok(1, K, N) && split_fwd_ok(1, N, K); }

void launch_linear_x2_fwd(const float *x, long ldx, const float *W, const float *bias, int M, int K, int N, float *y, void *ws, hipStream_t st)
{
    const LinWs L = lin_layout(M, K, N, false);
    char *w = (char *)ws;
    float *scales = (float *)w;
    const LinT t[2] = {{W, K, N, K}, {x, ldx, M, K}};
    lin_scales(t, 2, w, nullptr, 0, 0, nullptr, nullptr, st);
    lin_gemm_nt(x, ldx, W, bias, M, K, N, y, scales, w + L.pack, (unsigned *)(w + 128), st);
}

void launch_linear_x2_bwd(const float *x, long ldx, const float *W, const float *dy, int M, int K, int N, float *dx, float *dW, float *db, void *ws,
                          hipStream_t st)
{
    const LinWs L = lin_layout(M, K, N, true);
    char *w = (char *)ws;
    float *scales = (float *)w;             // {s_W, 1/s_W, s_dy, 1/s_dy, s_x, 1/s_x}
    const LinT t[3] = {{W, K, N, K}, {dy, N, M, N}, {x, ldx, M, K}};
    lin_scales(t, 3, w, (unsigned *)(w + L.prog), L.n_split * 16, L.rows_pad / XW2_ROWS, (int *)(w + L.list), (int *)(w + L.glist), st);
    if (dx) {  // dx[M,K] = dy[M,N] (W^T)[K,N]^T
        float *wt = (float *)(w + L.wt);
        launch_copy_enc(W, 0, 1, K, wt, 1, K, N, st);  // wt[k][n] = W[n][k]
        lin_gemm_nt(dy, N, wt, nullptr, M, N, K, dx, scales, w + L.pack, (unsigned *)(w + 128), st);
    }
    // dW[N,K] = dy^T x, db = column sums of dy: k_dw_x2 on dy's interleaved planes (its G operand) and x's planes (its hidden operand);
    // the padding rows [M, rows_alloc) are written as zeros by the split kernels
    float *pa = (float *)(w + L.pa);
    unsigned short *pb = (unsigned short *)(w + L.pb);
    {
        const long na = L.rows_alloc * (N / 32), nb = L.rows_alloc * (K / 8);
        hipLaunchKernelGGL(k_x2_split_rows<true>, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, st, dy, (long)N, (long)M, L.rows_alloc, N, scales + 2, (void *)pa, 0L);
        hipLaunchKernelGGL(k_x2_split_rows<false>, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, x, ldx, (long)M, L.rows_alloc, K, scales + 4, (void *)pb,
                           L.rows_alloc * (long)K);
    }
    X3Args a{};
    a.logits = pa; a.hidden = pb; a.plane_stride = L.rows_alloc * (long)K; a.rows_pad = L.rows_pad; a.rows_alloc = L.rows_alloc;
    a.B = 1; a.T = 1; a.U1 = 1; a.H = K; a.V = N; a.n_split = L.n_split; a.dw_prog = (int *)(w + L.prog);
    a.slab_w = (float *)(w + L.slab_w); a.slab_b = (float *)(w + L.slab_b); a.dw_rescale = 1.0f; a.db_rescale = 1.0f; a.n_cu = device_cus();
    a.live_stats = (int *)(w + L.list); a.ks_list = a.live_stats + 16; a.grp_list = (int *)(w + L.glist);
    launch_dw_x2(a, st, false);  // (no list kernels, no progress-word fill: all done by k_x2_lin_scales)
    const long n4w = (long)N * K / 4, n4b = N / 4;
    hipLaunchKernelGGL(k_x2_reduce_scaled, dim3((unsigned)((n4w + 255) / 256)), dim3(256), 0, st, a.slab_w, dW, n4w, n4w, L.n_split,
                       (const float *)(scales + 3), (const float *)(scales + 5));
    if (db)
        hipLaunchKernelGGL(k_x2_reduce_scaled, dim3((unsigned)((n4b + 255) / 256)), dim3(256), 0, st, a.slab_b, db, n4b, n4b, L.n_split,
                           (const float *)(scales + 3), (const float *)nullptr);
}
