// joint_fwd.hip — joint-network forward GEMM for gfx950 with the log-softmax fused in.
//
// Replaces reference rnnt/joint.py:32-39 (broadcast add -> tanh -> Linear H->V) and the
// log-softmax / gather half of the loss called at rnnt/model.py:35-41:
//   logits[b,t,u,:] = tanh(enc[b,t,:] + pred[b,u,:]) @ W^T + bias          (materialised)
//   denom = logsumexp_v logits ; lp_blank = logits[blank]-denom ; lp_emit = logits[y_u]-denom
//
// Design (MI355X-first, fp32 exact):
//  * GEMM M = lattice cells (64 per tile, linear cell index inside one utterance), K = H, N = V.
//    v_mfma_f32_32x32x2_f32 takes ONE f32 VGPR per operand and occupies the matrix pipe for 64
//    cycles, so operands go straight from L2 to registers — no LDS staging and no barrier in the
//    default main loop; LDS only carries the per-row softmax state.
//  * hidden = tanh(enc + pred) is produced ONCE, by the tile's own prologue (wave = rows, lane = 4 h),
//    stored to the workspace (both backward GEMMs read it again) and read back from L2 as the A
//    operand: a lane's 16-byte load supplies 4 k-steps because the k order inside an 8-wide chunk is
//    a free permutation (lanes 0-31 take k0..k0+3, lanes 32-63 take k0+4..k0+7, for A and B alike).
//    The plain joint (rnnt_engine_joint_fwd, no workspace for hidden) computes tanh in the loop.
//  * W is re-packed once per call (k_pack_w_fwd) into MFMA-fragment order: a B fragment is one
//    lane-linear 1 KiB load; columns are interleaved by 4 (tile q of a 128-column group holds columns
//    4j+q) so that a lane's accumulators for q = 0..3 are 4 consecutive logits -> 16-byte stores.
//  * 4 waves = 2 (M) x 2 (N), one per SIMD; each wave owns a 32 x 256 tile (8 accumulator tiles, 128
//    registers), so TWO workgroups share a CU; the workgroup walks V in passes of 512 columns keeping
//    a per-lane running (max, sum) per row in LDS — the row's log-sum-exp is complete when the last
//    pass ends.  Default main loop (BREG): A slices and B fragments stream into two register sets that
//    alternate by chunk parity, read by the MFMAs directly, one counted vmcnt per chunk.  The LDS-DMA
//    ring form is kept for odd chunk counts / the plain joint and as a per-call variant
//    (RNNT_VARIANT_FWD_LDS_RING).
//  * Persistent launch: 2 workgroups per CU for the whole kernel, tiles from one atomic counter; the
//    non-MFMA phases of a tile issue at s_setprio 1 so they overlap the co-resident workgroup's MFMAs.
#include "kernels.hpp"
#include "mma_common.hpp"

#define FWD_MWAVES 2  // 4 waves = 2 (M) x 2 (N), one per SIMD; TWO workgroups per CU (BREG path)
#define FWD_ROWS (32 * FWD_MWAVES)
#define FWD_THREADS (128 * FWD_MWAVES)

size_t wpack_floats(int H, int V)
{
    const size_t HK = (size_t)(H + 7) / 8, NG = (size_t)(V + 127) / 128;
    return HK * NG * 1024;
}

// wpack float4 index ((c8*NG + ng)*4 + q)*64 + lane holds
//   W[ng*128 + 4*(lane&31) + q][8*c8 + 4*(lane>>5) + 0..3]   (zero outside [V,H]).
__global__ __launch_bounds__(256) void k_pack_w_fwd(const float *__restrict__ W,
                                                    f32x4 *__restrict__ wpack, int H, int V,
                                                    int HK, int NG)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long n = (long)HK * NG * 256;
    if (idx >= n) return;
    const int lane = (int)(idx & 63);
    const int q = (int)((idx >> 6) & 3);
    const long r = idx >> 8;
    const int ng = (int)(r % NG);
    const int c8 = (int)(r / NG);
    const int v = ng * 128 + 4 * (lane & 31) + q;
    const int h = 8 * c8 + 4 * (lane >> 5);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (v < V) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (h + s < H) o[s] = W[(long)v * H + h + s];
    }
    wpack[idx] = o;
}

void launch_pack_w_fwd(const float *W, float *wpack, int H, int V, hipStream_t st)
{
    const int HK = (H + 7) / 8, NG = (V + 127) / 128;
    const long n = (long)HK * NG * 256;
    hipLaunchKernelGGL(k_pack_w_fwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, W,
                       (f32x4 *)wpack, H, V, HK, NG);
}

__global__ __launch_bounds__(256) void k_copy_enc(const float *__restrict__ enc, long sb, long st_,
                                                  long sh, float *__restrict__ dst, int B, int T,
                                                  int H)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long n = (long)B * T * H;
    if (idx >= n) return;
    const int h = (int)(idx % H);
    const long bt = idx / H;
    const int t = (int)(bt % T);
    const int b = (int)(bt / T);
    dst[idx] = enc[(long)b * sb + (long)t * st_ + (long)h * sh];
}

// The forward produces hidden only for lattice cells.  The backward GEMMs also touch a few dead cells
// — they multiply them by exact zeros (G == 0 there), so the rows only have to be finite: the cells
// that share a dHidden tile (<= 16 t x 16 u) or a 16-row dW granule with a lattice cell.  Zeroed
// here: for t < T_b the cells u in (U_b, U_b+16] and the last 16 of the row (the granule of the next
// row's first cell reaches back into them); every cell of the 16 time steps after T_b; the last 16
// cells of the utterance (the granule of the NEXT utterance's first cell reaches back into them).
// A batch of full-length utterances has no such cell and the kernel writes nothing.  grid (T, B).
__global__ __launch_bounds__(256) void k_zero_dead_hidden(float *__restrict__ hidden,
                                                          const int32_t *__restrict__ logit_lens,
                                                          const int32_t *__restrict__ target_lens,
                                                          int B, int T, int U1, int H)
{
    const int t = blockIdx.x, b = blockIdx.y;
    const int Tb = len_t(logit_lens, b, T), Ub = len_u(target_lens, b, U1);
    const int tail0 = T * U1 - 16;  // first of the utterance's last 16 cells
    if (t >= Tb + 16 && (t + 1) * U1 <= tail0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    float *row0 = hidden + ((long)b * T + t) * U1 * H;
    auto zero_row = [&](int u) {
        for (int h = lane * 4; h < H; h += 256) *(f32x4 *)(row0 + (long)u * H + h) = z;
    };
    if (t < Tb) {
        const int e1 = min(U1 - 1, Ub + 16);                  // (U_b, U_b + 16]
        for (int u = Ub + 1 + wave; u <= e1; u += 4) zero_row(u);
        for (int u = max(e1 + 1, U1 - 16) + wave; u < U1; u += 4) zero_row(u);  // the row's last 16
    } else if (t < Tb + 16) {
        for (int u = wave; u < U1; u += 4) zero_row(u);
    } else {
        for (int u = max(0, tail0 - t * U1) + wave; u < U1; u += 4) zero_row(u);
    }
}

void launch_zero_dead_hidden(float *hidden, const int32_t *logit_lens, const int32_t *target_lens, int B, int T,
                             int U1, int H, hipStream_t st)
{
    hipLaunchKernelGGL(k_zero_dead_hidden, dim3(T, B), dim3(256), 0, st, hidden, logit_lens, target_lens, B, T, U1, H);
}

// The view the reference really hands over: `encoder(mel).permute(0, 2, 1)` (rnnt/model.py:27-28) —
// shape (B,T,H) over an (N,C,L) tensor, so consecutive t are contiguous (t-stride 1) and consecutive h
// are T floats apart.  The element-per-thread copy above reads it with 64 lanes in 64 different rows
// (the guide's worst access shape, ~17x slower than coalesced).  Here a 64 t x 64 h tile goes through
// LDS: global reads run along t (256 contiguous bytes per wave-instruction), global writes along h;
// the 65-float row pitch keeps both LDS phases conflict-free.  grid (ceil(T/64), ceil(H/64), B).
__global__ __launch_bounds__(256) void k_transpose_enc(const float *__restrict__ enc, long sb, long sh,
                                                       float *__restrict__ dst, int T, int H)
{
    __shared__ float tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int t0 = blockIdx.x * 64, h0 = blockIdx.y * 64;
    const long b = blockIdx.z;
    const float *src = enc + b * sb;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int h = h0 + ty + 4 * i, t = t0 + tx;
        if (h < H && t < T) tile[ty + 4 * i][tx] = src[(long)h * sh + t];
    }
    __syncthreads();
    float *out = dst + b * T * H;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int t = t0 + ty + 4 * i, h = h0 + tx;
        if (t < T && h < H) out[(long)t * H + h] = tile[tx][ty + 4 * i];
    }
}

void launch_copy_enc(const float *enc, long sb, long st_, long sh, float *dst, int B, int T, int H,
                     hipStream_t st)
{
    if (st_ == 1 && sh != 1) {  // the permuted (N,C,L) view: tiled transpose
        hipLaunchKernelGGL(k_transpose_enc, dim3((T + 63) / 64, (H + 63) / 64, B), dim3(256), 0, st, enc, sb, sh,
                           dst, T, H);
        return;
    }
    const long n = (long)B * T * H;
    hipLaunchKernelGGL(k_copy_enc, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, enc, sb,
                       st_, sh, dst, B, T, H);
}

#define FWD_NBUF 4         // LDS ring of B chunks
#define FWD_BCHUNK 1024    // float4 per staged chunk: 512 columns x 8 k

// Register-destination loads that hipcc must NOT see: next to an LDS-DMA in flight it would
// guard their first use with s_waitcnt vmcnt(0) and drain the DMA ring every chunk.  The
// destinations are only read after vm_wait<N>(), which names them as in/out operands so no
// consumer can be scheduled above the wait (cdna_hip_programming.md §5.7, form (ii)).
__device__ __forceinline__ void asm_load16(f32x4 &dst, const float *ptr)
{
    // "+v": (1) the destination cannot share registers with the address pair — an overlapping
    // vdst/vaddr returned garbage whenever the access straddled a 2 GiB boundary; (2) the
    // loop-carried variable keeps ONE physical register, so hipcc has no reason to copy the
    // still-pending destination at the loop back-edge (with "=v" it did, reading stale data).
    asm volatile("global_load_dwordx4 %0, %1, off" : "+v"(dst) : "v"(ptr) : "memory");
}
template <int N>
__device__ __forceinline__ void vm_wait(f32x4 &e, f32x4 &p)
{
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(e), "+v"(p) : "n"(N) : "memory");
}

// Main loop over H in 8-wide chunks: 32 MFMAs per wave and chunk (8 accumulator tiles x 4
// k-steps); the workgroup's 8 waves = 4 (M) x 2 (N) cover 128 cells x 512 columns.
//
// What was measured before this design (tools/mfma_mix2.hip, s_memtime stamps in the kernel):
//  * the SIMD arbitrates oldest-first: unsynchronised, the older of the two waves sharing a
//    SIMD runs a whole pass ahead and the younger one finishes alone, bubbles unfilled;
//  * vmcnt retires in order: one young load that is waited for (the A slices) drags every
//    older B-fragment load with it, and B fragments streamed from L2 cost ~8 % even alone.
// Hence:
//  * B (W) chunks go global -> LDS by LDS-DMA (global_load_lds, no VGPRs), FWD_NBUF-deep ring,
//    issued two chunks ahead; fragments are then read LDS -> VGPR (ds_read_b128, its own
//    lgkmcnt counter, short fixed latency) right after the 4 MFMAs that used the previous one;
//  * the only register-destination VMEM loads are the A slices (enc/pred), issued right after
//    tanh consumed the previous ones and BEFORE the chunk's DMA, so `vmcnt(2)` at the top of
//    the next chunk retires them and the 2-chunk-old DMA but leaves the newest DMA in flight;
//  * tanh for chunk c+1 is computed one element per MFMA group while chunk c's MFMAs issue;
//  * one s_barrier per chunk publishes the ring slot and keeps the SIMD partners in step.
// (A per-workgroup rotation of the chunk order, meant to spread the CUs over wpack, measured
// no difference and was dropped with its wrap-around arithmetic.)  W is zero-padded in wpack,
// tanh of any finite input is finite, and address clamps keep every load in bounds, so no load
// in the loop is conditional.
template <bool USE_HID, bool PAIRS, bool BREG = false>  // USE_HID: erow points at the precomputed hidden row (no tanh, no pred)
                                     // PAIRS (with USE_HID, even chunk count): two-set form below
                                     // BREG (with PAIRS): B fragments straight L2 -> VGPR, no LDS, no barrier
__device__ __forceinline__ void fwd_mainloop(const float *erow, const float *prow,
                                             const f32x4 *wpass, int gvalid, int HK,
                                             long wstride, int H, int half, int wave,
                                             int lane, int wn, f32x4 *ldsb, f32x16 (&acc)[8])
{
    // Chunks run in order 0 .. HK-1; fetches that would run past the last chunk re-read it
    // (clamped, never used).  Every instruction issued between MFMAs costs ~6 matrix-pipe
    // cycles (measured on k_dhidden_gen), so the per-chunk bookkeeping is kept to scalar adds:
    // a running uniform DMA source, scalar chunk counters, ring slots by masking.
    // H % 8 == 4: in the last chunk lanes 32-63 would read k >= H; step them back 4 floats
    // (their B values are zero in wpack, so whatever finite A they form contributes 0)
    const int back = (((H & 7) != 0) && half == 1) ? 4 : 0;
    const int last = HK - 1;
    const int a_last = 8 * last - back;  // per-lane offset of the last chunk's A slice
    // this wave's share of a chunk's DMA: float4 [wave*128, +128) of the 1024; column groups
    // beyond the last valid one of a partial pass re-read group 0 (their tiles are discarded)
    constexpr int DPW = 1024 / FWD_THREADS;  // 1 KiB DMA pieces per wave and chunk
    const int dgrp = wave * DPW / 4;
    const unsigned dlane = (unsigned)(((dgrp < gvalid ? wave * 64 * DPW : (wave * 64 * DPW) % 256) + lane) * 16);  // bytes
    // LDS-DMA: the chunk's two 1 KiB pieces share one address and one M0 — the second is the
    // first at instruction offset 1024, which moves the global AND the LDS address.  (As MUBUF
    // `buffer_load ... lds` with a scalar chunk offset the address arithmetic disappears too, but
    // hipcc then guards every following ds_read with an s_waitcnt lgkmcnt.)
    const unsigned wstride_b = (unsigned)(wstride * 16);
    const char *wlane = (const char *)wpass + dlane;  // per-lane source of chunk 0
    auto dma = [&](unsigned chunk_off, int slot) {  // chunk_off: uniform byte offset of the chunk
        f32x4 *dst = ldsb + slot * FWD_BCHUNK + wave * 64 * DPW;  // wave-uniform (goes to M0)
        __builtin_amdgcn_global_load_lds((const void *)(wlane + chunk_off), (lds_vptr)dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const void *)(wlane + chunk_off), (lds_vptr)dst, 16, 1024, 0);
        if (DPW == 4) {
            __builtin_amdgcn_global_load_lds((const void *)(wlane + chunk_off), (lds_vptr)dst, 16, 2048, 0);
            __builtin_amdgcn_global_load_lds((const void *)(wlane + chunk_off), (lds_vptr)dst, 16, 3072, 0);
        }
    };
    const int roff = wn * 512 + lane;  // this wave's first fragment inside a staged chunk
    unsigned wnext = 0;  // byte offset of the chunk the next DMA fetches

    if constexpr (USE_HID && PAIRS && BREG) {
        // Default path.  No LDS in the loop: every wave streams its own 8 B fragments per chunk from wpack
        // (fragment order: one coalesced 1 KiB load each; the four M-waves of a column half and
        // the CU's other workgroup hit the same lines in L1/L2) into two register sets that
        // alternate by chunk parity, exactly like the A slices.  A fragment register is
        // re-requested for chunk c+2 one tile (4 MFMAs) after its last use — a refill issued
        // while MFMAs still read the register blocks the wave's issue.  No DMA, no ds_read, no
        // s_barrier: the loop carries ~10 non-MFMA instructions per 32 MFMAs instead of ~30.
        // Measured against the LDS-DMA ring below (8-wave workgroups, one per CU): the same
        // 52.1 ms at cfg2 — and the same again with one or two of these 4-wave workgroups per CU
        // (52.9 / 52.2 ms): neither the instruction count, the barrier, LDS nor a second wave per
        // SIMD is what holds the loop at ~89 % of the matrix pipe.  Kept because it is the simpler
        // loop and leaves the LDS to the softmax state.
        const int g0i = 2 * wn, g1i = 2 * wn + 1;  // this wave's column groups of the pass
        const unsigned v0 = (unsigned)(((g0i < gvalid ? g0i * 256 : 0) + lane) * 16);  // groups past the
        const unsigned v1 = (unsigned)(((g1i < gvalid ? g1i * 256 : 0) + lane) * 16);  // matrix re-read group 0
        const char *wbase = (const char *)wpass;
        const unsigned wsb = (unsigned)(wstride * 16);
        auto aoff = [&](int c) { return c >= last ? a_last : 8 * c; };
        // hipcc-invisible loads (see asm_load16): uniform chunk base in SGPRs + 32-bit lane offset
        // + immediate tile offset, so a chunk's address update is two scalar adds
#define LDW(dst, base, q)                                                                        \
        asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3"                                  \
                     : "+v"(dst) : "v"((q) < 4 ? v0 : v1), "s"(base), "n"(((q) & 3) * 1024) : "memory")
        f32x4 ea = {0.f, 0.f, 0.f, 0.f}, eb = ea, wa[8], wb[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) { wa[q] = ea; wb[q] = ea; }
        const char *b1 = wbase + (HK > 1 ? wsb : 0);              // chunk c8+1 (clamped to the last)
        const char *b2 = HK > 2 ? wbase + 2 * (size_t)wsb : b1;    // chunk c8+2
        asm_load16(ea, erow + aoff(0));
#pragma unroll
        for (int q = 0; q < 8; ++q) LDW(wa[q], wbase, q);
#pragma unroll
        for (int q = 0; q < 7; ++q) LDW(wb[q], b1, q);
        __builtin_amdgcn_sched_barrier(0);
        // In flight at the top of chunk c8: the 7 re-requests chunk c8-1 made for its own set.
        // Everything older — this chunk's A slice and fragment 7 (requested at the start of
        // c8-1), fragments 0-6 (during c8-2) — has landed once vmcnt <= 7.
        auto chunk = [&](int c8, f32x4 &eu, f32x4 (&wu)[8], f32x4 &ep, f32x4 (&wp)[8]) {
            asm volatile(RNNT_VMCNT(7)
                         : "+v"(eu), "+v"(wu[0]), "+v"(wu[1]), "+v"(wu[2]), "+v"(wu[3]), "+v"(wu[4]),
                           "+v"(wu[5]), "+v"(wu[6]), "+v"(wu[7])
                         :: "memory");
#pragma unroll
            for (int q = 0; q < 8; ++q) {
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(eu[s], wu[q][s], acc[q], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (q == 0) {  // what chunk c8-1 could not re-request while its last MFMAs ran
                    LDW(wp[7], b1, 7);
                    asm_load16(ep, erow + aoff(c8 + 1));
                } else {
                    LDW(wu[q - 1], b2, q - 1);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            b1 = b2;
            if (c8 + 3 <= last) b2 += wsb;
        };
        for (int c8 = 0; c8 < HK; c8 += 2) {
            chunk(c8, ea, wa, eb, wb);
            chunk(c8 + 1, eb, wb, ea, wa);
        }
#undef LDW
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // nothing may land after the registers are reused
        return;
    }
    f32x4 w[8];
    if constexpr (USE_HID && PAIRS) {
        // Hot path (A = precomputed hidden rows): the MFMAs read the loaded registers themselves.
        // Two register sets alternate by chunk parity: chunk c8 multiplies set c8&1 and, when its
        // last MFMA has issued, re-requests that set for chunk c8+2 — a whole chunk of slack, no
        // conversion, no copies (8 v_mov per chunk in the generic form below).
        f32x4 ea = {0.f, 0.f, 0.f, 0.f}, eb = {0.f, 0.f, 0.f, 0.f};
        auto aoff = [&](int c) { return c >= last ? a_last : 8 * c; };
        dma(wnext, 0);
        if (HK > 1) wnext += wstride_b;
        dma(wnext, 1);
        if (HK > 2) wnext += wstride_b;
        asm_load16(ea, erow + aoff(0));
        vm_wait<0>(ea, eb);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] = ldsb[roff + q * 64];
        __builtin_amdgcn_sched_barrier(0);
        dma(wnext, 2);
        if (HK > 3) wnext += wstride_b;
        asm_load16(eb, erow + aoff(1));
        __builtin_amdgcn_sched_barrier(0);
        // per chunk this wave issues: 2 DMA pieces (at q == 3), then 1 A load (after the last
        // MFMA).  At the top of chunk c8 the 3 ops of chunk c8-1 may stay in flight; everything
        // older — this chunk's A (requested at the end of c8-2) and the B of chunk c8+1 — is in.
        auto chunk = [&](int c8, f32x4 &eu) {
            vm_wait<DPW + 1>(ea, eb);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            const f32x4 *rd = ldsb + ((c8 + 1) & (FWD_NBUF - 1)) * FWD_BCHUNK + roff;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(eu[s], w[q][s], acc[q], 0, 0, 0);
                w[q] = rd[q * 64];
                if (q == 3) {
                    __builtin_amdgcn_sched_barrier(0);
                    dma(wnext, (c8 + 3) & (FWD_NBUF - 1));  // step c8+3's B
                    if (c8 + 4 < HK) wnext += wstride_b;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            asm_load16(eu, erow + aoff(c8 + 2));
            __builtin_amdgcn_sched_barrier(0);
        };
        for (int c8 = 0; c8 < HK; c8 += 2) {
            chunk(c8, ea);
            chunk(c8 + 1, eb);
        }
        vm_wait<0>(ea, eb);
        __builtin_amdgcn_s_barrier();
        return;
    }
    float a_cur[4], a_nxt[4];
    dma(wnext, 0);
    if (HK > 1) wnext += wstride_b;
    dma(wnext, 1);
    if (HK > 2) wnext += wstride_b;
    f32x4 e = {0.f, 0.f, 0.f, 0.f}, p = {0.f, 0.f, 0.f, 0.f};
    asm_load16(e, erow + (last == 0 ? a_last : 0));
    if (!USE_HID) asm_load16(p, prow + (last == 0 ? a_last : 0));
    vm_wait<0>(e, p);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < 8; ++q) w[q] = ldsb[roff + q * 64];
#pragma unroll
    for (int s = 0; s < 4; ++s) a_cur[s] = USE_HID ? e[s] : fast_tanh(e[s] + p[s]);
    __builtin_amdgcn_sched_barrier(0);
    {
        const int o1 = last <= 1 ? a_last : 8;
        asm_load16(e, erow + o1);
        if (!USE_HID) asm_load16(p, prow + o1);
    }
    __builtin_amdgcn_sched_barrier(0);
    dma(wnext, 2);
    if (HK > 3) wnext += wstride_b;
    __builtin_amdgcn_sched_barrier(0);
    for (int c8 = 0; c8 < HK; ++c8) {
        // retire this wave's A slices and its share of the DMA issued two chunks ago (step
        // c8+1's B); the newest DMA (2 ops) stays in flight across the barrier
        vm_wait<DPW>(e, p);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        const f32x4 *rd = ldsb + ((c8 + 1) & (FWD_NBUF - 1)) * FWD_BCHUNK + roff;
        const int a2 = (c8 + 2 >= last) ? a_last : 8 * (c8 + 2);  // A slice of step c8+2 (clamped)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (q < 4) {
                if (USE_HID)  // an opaque move: without it hipcc aliases a_nxt to e, keeps the old
                              // e live and rotates the PENDING new e through a copy at the back-edge
                    asm volatile("v_mov_b32 %0, %1" : "=v"(a_nxt[q]) : "v"(e[q]));
                else
                    a_nxt[q] = fast_tanh(e[q] + p[q]);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[s], w[q][s], acc[q], 0, 0, 0);
            w[q] = rd[q * 64];
            if (q == 3) {
                __builtin_amdgcn_sched_barrier(0);
                asm_load16(e, erow + a2);
                if (!USE_HID) asm_load16(p, prow + a2);
                __builtin_amdgcn_sched_barrier(0);
                dma(wnext, (c8 + 3) & (FWD_NBUF - 1));  // step c8+3's B
                if (c8 + 4 < HK) wnext += wstride_b;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) a_cur[s] = a_nxt[s];
    }
    // drain the DMA that ran ahead past the last step before the ring is reused / the
    // workgroup exits, and make sure every wave is done reading
    vm_wait<0>(e, p);
    __builtin_amdgcn_s_barrier();
}

#ifdef RNNT_STAMPS
// Diagnostic build only (make EXTRA=-DRNNT_STAMPS): per-workgroup s_memtime stamps written to a
// debug buffer no kernel reads; never enabled in the shipped library.
#define STAMP(slot)                                                                          \
    do {                                                                                     \
        if (a.debug && tid == 0) {                                                           \
            unsigned long long t_;                                                           \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");      \
            a.debug[((long)by_ * ntx_ + bx_) * 32 + (slot)] = t_;          \
        }                                                                                    \
    } while (0)
#else
#define STAMP(slot)
#endif

// One tile (FWD_ROWS cells of utterance by_, tile bx_ of ntx_) of the forward GEMM + epilogues.
template <bool WITH_LOSS, bool USE_HID, bool PAIRS, bool MAKE_HID, bool BREG>
__device__ __forceinline__ void fwd_tile(const JointFwdArgs &a, const int bx_, const int by_, const int ntx_, char *smem)
{
    // ALL LDS in one array (hipcc otherwise guards every ds_read with vmcnt(0) while an LDS-DMA
    // is in flight): [B ring | per-lane running softmax state | per-row (max,sum) of 2 N-waves]
    // The BREG main loop keeps no B ring: 33 KB, so two workgroups share a CU and one's prologue /
    // epilogues / finalisation run under the other's MFMAs; the ring variants (odd chunk counts,
    // the plain joint) need 97 KB and run one workgroup per CU.
    constexpr int RING = BREG ? 0 : FWD_NBUF * FWD_BCHUNK * 16;
    f32x4 *s_b = (f32x4 *)smem;
    float2(*s_run2)[FWD_THREADS] = (float2(*)[FWD_THREADS])(smem + RING);
    float(*s_m)[FWD_ROWS] = (float(*)[FWD_ROWS])(smem + RING + 16 * FWD_THREADS * 8);
    float(*s_s)[FWD_ROWS] = s_m + 2;
    int *s_nat = (int *)(s_s + 2);  // natural row (t*U1 + u) of the tile's compact rows

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // uniform: M0 of the DMAs, no per-use readfirstlane
    const int wm = wave >> 1, wn = wave & 1;
    const int i = lane & 31, half = lane >> 5;
    const int b = by_;
    const int m0 = bx_ * FWD_ROWS;
    const int T = a.T, U1 = a.U1, H = a.H, V = a.V;
    int Tb = T, Ub_ = U1 - 1;
    if (WITH_LOSS) len_tu_uniform(a.logit_lens, a.target_lens, b, a.T, a.U1, Tb, Ub_);
    // Rows of the GEMM = the utterance's LIVE cells only, in (t, u <= U_b) order: compact index m is
    // cell (t = m / W1, u = m % W1), W1 = U_b + 1 live columns, stored at its natural row t*U1 + u of
    // the [cells] buffers.  A ragged batch costs its live cells; a full one (W1 == U1) is unchanged.
    const int W1 = Ub_ + 1;
    const int ncell = Tb * W1;
    // Two workgroups share every SIMD of the CU.  A wave in one of its short non-MFMA phases (hidden
    // production, pass epilogue, finalisation) issues at priority 1, a wave in its main loop at 0: the
    // partner's MFMA stream needs one issue slot per 64 cycles and is not slowed, while the phase that
    // used to wait behind it (the SIMD arbitrates oldest-first at equal priority) overlaps it
    // (cfg2: 51.1 -> 50.3 ms).
    __builtin_amdgcn_s_setprio(1);
    if (tid < FWD_ROWS) {  // one division per row and tile, shared through LDS by the pass epilogues
        const int c = min(m0 + tid, ncell > 0 ? ncell - 1 : 0);
        const int ct = c / W1;
        s_nat[tid] = ct * U1 + (c - ct * W1);
    }
    if (!MAKE_HID) __syncthreads();
    if (MAKE_HID) {
        // hidden = tanh(enc + pred) for this tile's cells, produced here instead of by a separate
        // 13 GB pass (k_make_hidden): ~1 % of the tile's time, and the main loop's loads of it hit
        // L2.  Only lattice cells are produced; the dead cells the backward GEMMs can still touch
        // (they multiply them by exact zeros, so the rows must be finite) are zeroed by
        // k_zero_dead_hidden.
        // Wave w takes rows w, w+8, ...; a lane takes 4 consecutive h.  Loads are batched ahead of
        // the first tanh so a tile pays a few memory round trips, not one per row: when the tile
        // spans at most two time steps (U1 >= 127) its two enc rows are loaded once and all 16 pred
        // rows of the wave are in flight together (one round trip per 256 columns); otherwise
        // batches of 8 (enc, pred) row pairs.
        const int nrow = ncell - m0 < FWD_ROWS ? ncell - m0 : FWD_ROWS;  // <= 0: no live cell in this tile
        float *hidb = (float *)a.hidden + (long)b * T * U1 * H;
        const float *encb = a.enc + (long)b * a.enc_sb, *predb = a.pred + (long)b * U1 * H;
        constexpr int NW = FWD_THREADS / 64, RPW = FWD_ROWS / NW;
        const int t_first = m0 / W1;
        const int cut = (t_first + 1) * W1 - m0;  // tile rows >= cut belong to time step t_first + 1
        if (nrow <= 0) {
        } else if ((m0 + nrow - 1) / W1 <= t_first + 1) {
            const int t_second = t_first + 1 < T ? t_first + 1 : t_first;
            for (int h = (tid & 63) * 4; h < H; h += 256) {
                const f32x4 e0 = *(const f32x4 *)(encb + (long)t_first * a.enc_st + h);
                const f32x4 e1 = *(const f32x4 *)(encb + (long)t_second * a.enc_st + h);
                f32x4 p[RPW];
#pragma unroll
                for (int i = 0; i < RPW; ++i) {
                    const int r0 = wave + i * NW;
                    const int r = r0 < nrow ? r0 : nrow - 1;  // clamped: loads stay unconditional
                    const int u = m0 + r - (r >= cut ? t_first + 1 : t_first) * W1;
                    p[i] = *(const f32x4 *)(predb + (long)u * H + h);
                }
#pragma unroll
                for (int i = 0; i < RPW; ++i) {
                    const int r = wave + i * NW;
                    const f32x4 e = r >= cut ? e1 : e0;  // wave-uniform
                    const int tr = r >= cut ? t_first + 1 : t_first;
                    const f32x4 o = fast_tanh_sum4(e, p[i]);
                    if (r < nrow) *(f32x4 *)(hidb + ((long)tr * U1 + (m0 + r - tr * W1)) * H + h) = o;
                }
            }
        } else {
            constexpr int BATCH = 8;
            for (int h = (tid & 63) * 4; h < H; h += 256) {
                for (int rb = 0; rb < RPW; rb += BATCH) {
                    f32x4 e[BATCH], p[BATCH];
#pragma unroll
                    for (int i = 0; i < BATCH; ++i) {
                        const int r = wave + (rb + i) * NW;
                        const int c = m0 + (r < nrow ? r : nrow - 1);
                        const int t = c / W1, u = c - t * W1;
                        e[i] = *(const f32x4 *)(encb + (long)t * a.enc_st + h);
                        p[i] = *(const f32x4 *)(predb + (long)u * H + h);
                    }
#pragma unroll
                    for (int i = 0; i < BATCH; ++i) {
                        const int r = wave + (rb + i) * NW;
                        const int c = m0 + r;
                        const int t = c / W1, u = c - t * W1;
                        const f32x4 o = fast_tanh_sum4(e[i], p[i]);
                        if (r < nrow) *(f32x4 *)(hidb + ((long)t * U1 + u) * H + h) = o;
                    }
                }
            }
        }
        __syncthreads();  // stores acknowledged (vmcnt(0)) and every wave past them
    }
    if (m0 >= ncell) return;
    STAMP(0);
#ifdef RNNT_STAMPS
    if (a.debug && lane == 0) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        a.debug[((long)by_ * ntx_ + bx_) * 32 + 8 + wave] =
            ((unsigned long long)xcc << 32) | hw;
        if (wave == 0)
            a.debug[((long)by_ * ntx_ + bx_) * 32 + 7] =
                ((unsigned long long)xcc << 32) | hw;
    }
#endif
    const int Ub = Ub_;

    // per-lane running (max, sum-exp) of the 16 accumulator rows this lane sees, parked in LDS
    // between passes (slot [r][tid]: conflict-free) so it costs no VGPRs in the main loop;
    // folded in-lane after every pass and combined across lanes only once per tile.
    if (WITH_LOSS) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s_run2[r][tid] = make_float2(RNNT_NEG_INF, 0.f);
    }

    // this lane's A row: cell -> (t,u) -> 16-byte slices of enc / pred
    const int crow = min(m0 + wm * 32 + i, ncell - 1);
    const int trow = crow / W1, urow = crow - trow * W1;
    // fused path: A comes from the hidden buffer k_make_hidden filled (the backward GEMMs need
    // it anyway), so the loop carries no tanh; the plain joint computes tanh in-loop
    const float *erow = USE_HID ? a.hidden + ((long)b * T * U1 + (long)trow * U1 + urow) * H + 4 * half
                                  : a.enc + (long)b * a.enc_sb + (long)trow * a.enc_st + 4 * half;
    const float *prow = a.pred + ((long)b * U1 + urow) * H + 4 * half;
    // The last tile of an utterance: a wave whose 32 rows all lie past the live cells has nothing to
    // compute.  The default main loop has no barrier, so such a wave simply skips it (and its
    // epilogue); the workgroup-wide barriers of the finalisation are outside the skipped region.
    bool wave_dead = false;
    if (WITH_LOSS && BREG) wave_dead = m0 + wm * 32 >= ncell;
    const int HK = (H + 7) / 8, NG = (V + 127) / 128;
    const long wstride = (long)NG * 256;  // float4 per 8-wide k chunk
    const int npass = (NG + 3) / 4;


    for (int pass = 0; pass < npass; ++pass) {
        const int ng0 = pass * 4 + wn * 2;
        const bool g0 = ng0 < NG, g1 = (ng0 + 1) < NG;
        const int col0[2] = {ng0 * 128 + 4 * i, (ng0 + 1) * 128 + 4 * i};
        const bool cok[2] = {g0 && col0[0] < V, g1 && col0[1] < V};

        f32x16 acc[8];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            f32x4 bq = {0.f, 0.f, 0.f, 0.f};
            if (cok[g]) bq = *(const f32x4 *)(a.bias + col0[g]);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[g * 4 + q][r] = bq[q];
        }

        const f32x4 *wpass = (const f32x4 *)a.wpack + (long)pass * 1024;
        const int gvalid = min(4, NG - pass * 4);
        STAMP(1 + 2 * (pass & 1));
        if (wave_dead) continue;  // wave-uniform
        __builtin_amdgcn_s_setprio(0);
        fwd_mainloop<USE_HID, PAIRS, BREG>(erow, prow, wpass, gvalid, HK, wstride, H, half, wave, lane, wn,
                                s_b, acc);
        __builtin_amdgcn_s_setprio(1);
        STAMP(2 + 2 * (pass & 1));

        // ---- epilogue: store logits, fold this pass into the running row log-sum-exp
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rowl = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const int c = m0 + rowl;
            const bool rv = c < ncell;
            float *lrow = a.logits + ((long)b * T * U1 + s_nat[rowl]) * V;  // compact -> natural row
#pragma unroll
            for (int g = 0; g < 2; ++g)
                if (rv && cok[g]) {
                    f32x4 o = {acc[g * 4 + 0][r], acc[g * 4 + 1][r], acc[g * 4 + 2][r],
                               acc[g * 4 + 3][r]};
                    if (RNNT_XP(a.ablate, 1))
                        __builtin_nontemporal_store(o, (f32x4 *)(lrow + col0[g]));
                    else
                        *(f32x4 *)(lrow + col0[g]) = o;
                }
            if (WITH_LOSS && cok[0]) {  // cok[1] implies cok[0]
                float ml = fmaxf(fmaxf(acc[0][r], acc[1][r]), fmaxf(acc[2][r], acc[3][r]));
                if (cok[1])
                    ml = fmaxf(ml, fmaxf(fmaxf(acc[4][r], acc[5][r]), fmaxf(acc[6][r], acc[7][r])));
                const float2 ms = s_run2[r][tid];
                const float mn = fmaxf(ms.x, ml);
                const float nm2 = -mn * RNNT_LOG2E;  // exp(x - mn) = exp2(fma(x, log2e, nm2)): 2 instructions
                auto ex = [&](float x) { return __builtin_amdgcn_exp2f(fmaf(x, RNNT_LOG2E, nm2)); };
                float sl = (ex(acc[0][r]) + ex(acc[1][r])) + (ex(acc[2][r]) + ex(acc[3][r]));
                if (cok[1]) sl += (ex(acc[4][r]) + ex(acc[5][r])) + (ex(acc[6][r]) + ex(acc[7][r]));
                // exp2(-inf * log2e + finite) = 0 on the first pass
                s_run2[r][tid] = make_float2(mn, ms.y * ex(ms.x) + sl);
            }
        }
    }

    STAMP(5);
#ifdef RNNT_STAMPS
    if (a.debug && lane == 0) {
        unsigned long long t_;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");
        a.debug[((long)by_ * ntx_ + bx_) * 32 + 16 + wave] = t_;
    }
#endif
    if (WITH_LOSS) {
        // ---- once per tile: combine the 32 lanes that share a row, then the two N-waves
        float m_run[16], s_run[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float2 ms = s_run2[r][tid];
            m_run[r] = ms.x; s_run[r] = ms.y;
        }
        // row max over the 32 lanes, per-lane sums rescaled to it, row sum — on the DPP crossbar
        // (the butterfly of (max, sum) pairs through ds_bpermute was ~1100 instructions here)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float M = half_max_dpp(m_run[r], half);
            // exp2(-inf - M) = 0 for lanes (and rows) that saw nothing; a row that is -inf
            // everywhere keeps M = -inf and a zero sum
            const float sc = (m_run[r] == RNNT_NEG_INF) ? 0.f : __builtin_amdgcn_exp2f((m_run[r] - M) * RNNT_LOG2E);
            s_run[r] = half_sum_dpp(s_run[r] * sc, half);
            m_run[r] = M;
        }
        if (i == 31) {  // lanes 31 / 63 hold the sums of their half
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rowl = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                s_m[wn][rowl] = m_run[r];
                s_s[wn][rowl] = s_run[r];
            }
        }
        __syncthreads();  // also drains this workgroup's logits stores (vmcnt(0))
        if (tid < FWD_ROWS) {
            const int c = m0 + tid;
            const int t = c / W1, u = c - t * W1;
            if (c < ncell) {
                const float ma = s_m[0][tid], mb = s_m[1][tid];
                const float m = fmaxf(ma, mb);
                const float ea = (ma == RNNT_NEG_INF) ? 0.f : __expf(ma - m);
                const float eb = (mb == RNNT_NEG_INF) ? 0.f : __expf(mb - m);
                const float den = m + logf(s_s[0][tid] * ea + s_s[1][tid] * eb);
                // the two logits the lattice needs were stored by this workgroup a moment ago:
                // read them back from L2 (agent-scope loads bypass the CU's vector L1)
                const float *lrow = a.logits + ((long)b * T * U1 + (long)t * U1 + u) * V;
                const float lb = __hip_atomic_load(lrow + a.blank, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
                const int y = (u < Ub) ? a.targets[(long)b * (U1 - 1) + u] : -1;
                const float le = (y >= 0) ? __hip_atomic_load(lrow + y, __ATOMIC_RELAXED,
                                                              __HIP_MEMORY_SCOPE_AGENT)
                                          : den;
                const long si = skew_index(b, t, u, a.D, U1);
                a.denom_s[si] = den;
                a.lpb_s[si] = lb - den;
                a.lpe_s[si] = le - den;
            }
        }
    }
    STAMP(6);
}

#define FWD_SMEM(BREG) ((BREG ? 0 : FWD_NBUF * FWD_BCHUNK * 16) + 16 * FWD_THREADS * 8 + 4 * FWD_ROWS * 4 + FWD_ROWS * 4)

// one workgroup per tile, grid (tiles per utterance, B)
template <bool WITH_LOSS, bool USE_HID, bool PAIRS = false, bool MAKE_HID = false, bool BREG = false>
__global__ __launch_bounds__(FWD_THREADS, 2) void k_joint_fwd(JointFwdArgs a)
{
    __shared__ __attribute__((aligned(16))) char smem[FWD_SMEM(BREG)];
    fwd_tile<WITH_LOSS, USE_HID, PAIRS, MAKE_HID, BREG>(a, blockIdx.x, blockIdx.y, gridDim.x, smem);
}

// Persistent form of the default path: 2 workgroups per CU for the whole launch, tiles handed out
// by one atomic counter.  With one workgroup per tile the dispatcher does not keep the second
// slot of a CU filled (stamps: 1.1-1.2 resident workgroups per CU on average, every tile's
// prologue / epilogues / finalisation — 10 % of its time — run with the matrix pipe idle);
// resident workgroups drift apart and one's non-MFMA phases run under the other's MFMAs.
template <bool WITH_LOSS, bool USE_HID, bool PAIRS, bool MAKE_HID, bool BREG>
__global__ __launch_bounds__(FWD_THREADS, 2) void k_joint_fwd_persist(JointFwdArgs a, int ntx, int ntot)
{
    __shared__ __attribute__((aligned(16))) char smem[FWD_SMEM(BREG)];
    __shared__ int s_next[2];
    if (threadIdx.x == 0) s_next[0] = (int)atomicAdd(a.counter, 1u);
    __syncthreads();
    int t = s_next[0];
    for (int it = 1; t < ntot; ++it) {
        // the next tile is requested while this one is computed: the atomic's round trip is hidden
        if (threadIdx.x == 0) s_next[it & 1] = (int)atomicAdd(a.counter, 1u);
        fwd_tile<WITH_LOSS, USE_HID, PAIRS, MAKE_HID, BREG>(a, t % ntx, t / ntx, ntx, smem);
        __syncthreads();  // every wave done with the tile's LDS state; s_next[it & 1] visible
        t = s_next[it & 1];
    }
}

void launch_joint_fwd(const JointFwdArgs &a, hipStream_t st, bool lds_ring, bool one_wg_per_tile)
{
    const int tiles = (int)(((long)a.T * a.U1 + FWD_ROWS - 1) / FWD_ROWS);
    dim3 grid(tiles, a.B), block(FWD_THREADS);
    if (a.denom_s && a.hidden) {
        const bool pairs = ((a.H + 7) / 8) % 2 == 0;  // even number of 8-wide chunks: the two-register-set main loop
        if (pairs && !lds_ring) {
            const long ntot = (long)tiles * a.B;
            if (a.counter && !one_wg_per_tile && ntot < 0x7fffffffL) {
                launch_fill32(a.counter, 0u, 4, st);
                const int nwg = (int)(ntot < 2L * a.n_cu ? ntot : 2L * a.n_cu);
                if (a.make_hidden)
                    hipLaunchKernelGGL((k_joint_fwd_persist<true, true, true, true, true>), dim3(nwg), block, 0, st, a, tiles, (int)ntot);
                else  // hidden comes from the separate k_make_hidden pass (rnnt_engine_set_flags(64))
                    hipLaunchKernelGGL((k_joint_fwd_persist<true, true, true, false, true>), dim3(nwg), block, 0, st, a, tiles, (int)ntot);
            } else if (!a.make_hidden) {
                hipLaunchKernelGGL((k_joint_fwd<true, true, true, false, true>), grid, block, 0, st, a);
            } else {
                hipLaunchKernelGGL((k_joint_fwd<true, true, true, true, true>), grid, block, 0, st, a);
            }
        }
        else if (a.make_hidden && pairs) hipLaunchKernelGGL((k_joint_fwd<true, true, true, true>), grid, block, 0, st, a);
        else if (a.make_hidden) hipLaunchKernelGGL((k_joint_fwd<true, true, false, true>), grid, block, 0, st, a);
        else if (pairs) hipLaunchKernelGGL((k_joint_fwd<true, true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_joint_fwd<true, true>), grid, block, 0, st, a);
    } else if (a.denom_s)
        hipLaunchKernelGGL((k_joint_fwd<true, false>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_joint_fwd<false, false>), grid, block, 0, st, a);
}

// Diagnostic: resident workgroups per CU the runtime predicts for the forward kernel.
int fwd_occupancy(int with_loss)
{
    int n = -1;
    if (with_loss)
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_joint_fwd<true, true>, FWD_THREADS, 0);
    else
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_joint_fwd<false, false>, FWD_THREADS, 0);
    return n;
}
