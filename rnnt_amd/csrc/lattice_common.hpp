// lattice_common.hpp — leaf pieces shared by the transducer lattice (lattice.hip) and the CTC head (ctc.hip).  The two chain bodies
// (lattice_chain, ctc_chain) keep their own step loops, mailbox protocol and prefetch; what they share is below.
#pragma once
#include "common.hpp"

typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));

// A double moved one lane along the wave by two DPP moves (0x138: wave_shr, from lane - 1; 0x130: wave_shl, from lane + 1); the
// lane without a source keeps `fill`.
template <int CTRL>
__device__ __forceinline__ double wave_shift(double v, double fill)
{
    const u32x2_t x = __builtin_bit_cast(u32x2_t, v), f = __builtin_bit_cast(u32x2_t, fill);
    u32x2_t r;
    r[0] = (unsigned)__builtin_amdgcn_update_dpp((int)f[0], (int)x[0], CTRL, 0xf, 0xf, false);
    r[1] = (unsigned)__builtin_amdgcn_update_dpp((int)f[1], (int)x[1], CTRL, 0xf, 0xf, false);
    return __builtin_bit_cast(double, r);
}

// log(exp a + exp b) = max + log(1 + exp(-|a - b|)): fp64 maximum, the correction (< ln 2) in fp32 on the hardware exp2 / log2.
// -inf-safe: a state INSIDE a lattice may have no reachable predecessor, and -inf + log 2 = -inf instead of the NaN of (-inf) - (-inf).
__device__ __forceinline__ double lse2_safe(double a, double b)
{
    const double m = fmax(a, b);
    const float d = m == (double)RNNT_NEG_INF ? 0.f : -fabsf((float)(a - b));
    return m + (double)(__builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(d * RNNT_LOG2E)) * 0.6931471805599453f);
}

// One wave over a row of V logits (V % 4 == 0): m = the maximum, s = the sum of exp(x - m), in every lane; the row's log-sum-exp
// is m + logf(s), formed by the caller.  A NaN logit is skipped by the max and lands in the sum: NaN denominator, NaN lp_blank.
__device__ __forceinline__ void row_max_sumexp(const float *__restrict__ x, int V, int lane, float &m, float &s)
{
    m = RNNT_NEG_INF;
    for (int v = lane * 4; v < V; v += 256) {
        const f32x4 q = *(const f32x4 *)(x + v);
        m = fmaxf(m, fmaxf(fmaxf(q[0], q[1]), fmaxf(q[2], q[3])));
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) m = fmaxf(m, __shfl_xor(m, k, 64));
    s = 0.f;
    for (int v = lane * 4; v < V; v += 256) {
        const f32x4 q = *(const f32x4 *)(x + v);
        s += __expf(q[0] - m) + __expf(q[1] - m) + __expf(q[2] - m) + __expf(q[3] - m);
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) s += __shfl_xor(s, k, 64);
}

// LDS bytes of a chained sweep's mailboxes: 8 B value + 4 B tag per wave boundary and step.  The chain runs while they fit in
// 64 KiB; a workgroup of one wave has none (no error word to clear, no status to report).
inline size_t chain_mailbox_bytes(int columns, int steps) { return (size_t)((columns + 63) / 64 - 1) * steps * 12; }
