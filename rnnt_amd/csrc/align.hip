// align.hip — forced alignment on the transducer lattice for gfx950.
//
// The best (Viterbi) path through the same T x (U+1) lattice, with the same per-cell log-probs
// (lp_blank / lp_emit in the skewed layout of common.hpp) that the loss sums over:
//   k_viterbi    max-plus counterpart of k_lattice: one workgroup per utterance, thread u owns
//                column u, previous diagonal in a double-buffered LDS line; values in fp64; one
//                backpointer bit per cell, packed per diagonal by a wave ballot (bit u % 64 of
//                word u / 64: 1 = the cell was entered by a label arc from (t, u-1), 0 = by a blank
//                arc from (t-1, u); on an exact tie the blank arc)
//   k_backtrace  one wave per utterance walks the bits from (T_b-1, U_b) back to (0,0) and writes
//                the frame of every label.  Within 64 consecutive diagonals the path's column moves by
//                at most 63, so the lanes load the <= 2 candidate words of 64 diagonals at once and
//                the walk runs on them in registers: ~(T_b+U_b)/64 dependent loads per utterance.
#include "common.hpp"
#include "kernels.hpp"

typedef unsigned long long u64;

// Workgroup of ceil(U1/64) waves, grid B.  Writes bp[b][d][w] for the diagonals d < T_b + U_b of
// utterance b (the backtrace reads no other word), and scores[b] = best path log-probability, or
// NaN when a log-prob the recurrence reads is NaN (fmax-style selects would drop it silently).
__global__ __launch_bounds__(1024) void k_viterbi(
    const float *__restrict__ lpb_s, const float *__restrict__ lpe_s, u64 *__restrict__ bp,
    const int32_t *__restrict__ logit_lens, const int32_t *__restrict__ target_lens,
    float *__restrict__ scores, int U1, int D)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int NT = blockDim.x, NW = NT >> 6;
    const int b = blockIdx.x;
    const int u = threadIdx.x, lane = u & 63, w = u >> 6;
    const int T = D - U1 + 1;
    const int Tb = len_t(logit_lens, b, T);
    const int Ub = len_u(target_lens, b, U1);
    const int nd = Tb + Ub;  // valid anti-diagonals 0 .. nd-1
    const double NINF = (double)RNNT_NEG_INF;
    // buf[x][u + 1] = column u of a diagonal; buf[x][0] = column -1 (always -inf)
    double *buf[2] = {sm, sm + NT + 1};
    buf[0][u + 1] = NINF;
    buf[1][u + 1] = NINF;
    if (u == 0) { buf[0][0] = NINF; buf[1][0] = NINF; }
    __syncthreads();
    const long base = (long)b * D * U1;
    const float *lpb = lpb_s + base, *lpe = lpe_s + base;
    u64 *bpb = bp + (long)b * D * NW;
    const bool col_ok = u <= Ub;
    const int uc = u < U1 ? u : U1 - 1;  // the block is padded to whole waves: stay inside the row

    // log-probs of the two arcs INTO the cells of diagonal k, from diagonal k-1: blank from column
    // u, label from column u-1.  Loaded unconditionally (clamped indices) and used only under the
    // arc's own validity below: slots outside the lattice are never written and may hold anything.
    auto fetch = [&](int k, float &lb, float &le) {
        const int d = k < nd ? k : nd - 1;
        const long r = (long)(d > 0 ? d - 1 : 0) * U1;
        lb = lpb[r + uc];
        le = lpe[r + (uc > 0 ? uc - 1 : 0)];
    };
    bool bad = false;
    double last = NINF;
    auto step = [&](int k, float lb, float le) {
        const double *prev = buf[(k & 1) ^ 1];
        double *cur = buf[k & 1];
        const int t = k - u;
        const bool valid = (k < nd) && col_ok && t >= 0 && t < Tb;
        const bool hb = valid && t > 0, he = valid && u > 0;  // the cell has a blank / label predecessor
        const double a = hb ? prev[u + 1] + (double)lb : NINF;
        const double e = he ? prev[u] + (double)le : NINF;
        // the tie rule: the label arc only when strictly better; row 0 has no blank predecessor, column 0
        // no label predecessor (forced, so that the backtrace stays inside the lattice whatever the values)
        const bool emit = he && (t == 0 || e > a);
        double v = emit ? e : a;
        if (k == 0) v = 0.0;  // (0,0); k is uniform, only thread 0 is valid
        v = valid ? v : NINF;
        bad = bad || (hb && lb != lb) || (he && le != le);
        cur[u + 1] = v;
        const u64 word = __ballot(emit ? 1 : 0);
        if (k < nd && lane == 0) bpb[(long)k * NW + w] = word;
        if (k == nd - 1) last = v;  // thread Ub holds the path's last cell (T_b-1, U_b)
        // LDS-only barrier (as in k_lattice): the bp store and the lp prefetch stay in flight
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };

    float lb0, le0, lb1, le1, lb2, le2, lb3, le3;
    fetch(0, lb0, le0); fetch(1, lb1, le1); fetch(2, lb2, le2); fetch(3, lb3, le3);
    for (int k = 0; k < nd; k += 4) {  // nd is workgroup-uniform: every thread runs the same barriers
        step(k, lb0, le0);
        fetch(k + 4, lb0, le0);
        step(k + 1, lb1, le1);
        fetch(k + 5, lb1, le1);
        step(k + 2, lb2, le2);
        fetch(k + 6, lb2, le2);
        step(k + 3, lb3, le3);
        fetch(k + 7, lb3, le3);
    }
    // the path ends with the blank arc out of (T_b-1, U_b)
    float fb = 0.f;
    if (u == Ub) {
        fb = lpb[(long)(nd - 1) * U1 + Ub];
        bad = bad || fb != fb;
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (u == Ub) scores[b] = any_bad ? __builtin_nanf("") : (float)(last + (double)fb);
}

__device__ __forceinline__ u64 readlane64(u64 v, int l)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}

// One wave per utterance (grid B).  frames[b][u] = frame of label u for u < U_b, -1 for U_b <= u < U1-1;
// every entry -1 when scores[b] is NaN.  The walk issues no memory operation between its window loads:
// on gfx9 a store counts in vmcnt, so a store per label would make the next window's load wait for it.
// The frames of a window collect in a VGPR (lane j: the window's j-th label), go to LDS at the window's
// end, and to HBM once at the end of the walk.
__global__ __launch_bounds__(64) void k_backtrace(
    const u64 *__restrict__ bp, const int32_t *__restrict__ logit_lens,
    const int32_t *__restrict__ target_lens, const float *__restrict__ scores,
    int32_t *__restrict__ frames, int U1, int D)
{
    __shared__ int32_t sfr[1024];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int NW = (U1 + 63) >> 6;
    const int T = D - U1 + 1, U = U1 - 1;
    const int Tb = len_t(logit_lens, b, T), Ub = len_u(target_lens, b, U1);
    int32_t *fr = frames + (long)b * U;
    const float sc = scores[b];
    const bool nan = sc != sc;
    for (int j = (nan ? 0 : Ub) + lane; j < U; j += 64) fr[j] = -1;
    if (nan) return;
    const u64 *bpb = bp + (long)b * D * NW;
    int t = Tb - 1, u = Ub;  // wave-uniform walk state
    while (t + u > 0) {
        // lane i: the words of diagonal t+u-i that can hold the path's column (it lies in [u-63, u])
        const int d0 = t + u, whi = u >> 6, wlo = whi > 0 ? whi - 1 : 0;
        const int dl = d0 - lane;
        u64 hi = 0, lo = 0;
        if (dl >= 1) {
            hi = bpb[(long)dl * NW + whi];
            lo = bpb[(long)dl * NW + wlo];
        }
        const int ubase = wlo * 64, u0 = u;
        int fv = 0;
        // 64 steps, unrolled and branch-free (the words of each step are read from a constant lane, off the
        // dependent chain); a step after the walk reached (0,0) changes nothing
#pragma unroll
        for (int k = 0; k < 64; ++k) {  // lane k holds diagonal t + u
            const u64 wh = readlane64(hi, k), wl = readlane64(lo, k);
            const int r = u - ubase;  // in [0, 128)
            const u64 wd = r >= 64 ? wh : wl;
            const int bit = (int)(wd >> (r & 63)) & 1;
            // u == 0: only a blank arc exists; t == 0: only a label arc (the sweep writes the same)
            const int live = (t + u) > 0;
            const int emit = live & (u > 0) & ((t == 0) | bit);
            fv = (emit && lane == u0 - u) ? t : fv;  // label u - 1 is the window's (u0 - u)-th
            u -= emit;
            t -= live & (emit ^ 1);
        }
        if (lane < u0 - u) sfr[u0 - 1 - lane] = fv;
    }
    __syncthreads();
    for (int j = lane; j < Ub; j += 64) fr[j] = sfr[j];
}

void launch_align(const LatticeArgs &a, void *bp, float *scores, int32_t *frames, hipStream_t st)
{
    const int NT = ((a.U1 + 63) / 64) * 64;
    const size_t lds = 2 * (size_t)(NT + 1) * sizeof(double);
    hipLaunchKernelGGL(k_viterbi, dim3(a.B), dim3(NT), lds, st, a.lpb_s, a.lpe_s, (u64 *)bp, a.logit_lens,
                       a.target_lens, scores, a.U1, a.D);
    hipLaunchKernelGGL(k_backtrace, dim3(a.B), dim3(64), 0, st, (const u64 *)bp, a.logit_lens,
                       a.target_lens, (const float *)scores, frames, a.U1, a.D);
}
