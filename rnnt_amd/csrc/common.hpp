// common.hpp — shared device helpers for the gfx950 RNN-T engine kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define RNNT_NEG_INF (-__builtin_inff())
// Ablation switches (rnnt_engine_set_flags) exist only in diagnostic builds
// (make EXTRA=-DRNNT_ABLATE, used by tools/exp_*.py); the shipped kernels carry none.
#ifdef RNNT_ABLATE
#define RNNT_XP(flags, bit) ((flags) & (bit))
#else
#define RNNT_XP(flags, bit) (0)
#endif
#define RNNT_LOG2E 1.4426950408889634f

// Counted vmcnt waits of the hand-scheduled kernels (a count is right only while the compiler keeps their VMEM instructions in program
// order).  -DRNNT_VMCNT0 turns every counted wait into vmcnt(0): slower, but right whatever the order — tools/check_vmcnt0.sh builds that
// library and compares a step's outputs with the shipped library's bit for bit (round-4 advice: catches a miscount after a compiler upgrade).
#ifdef RNNT_VMCNT0
#define RNNT_VMCNT(n) "s_waitcnt vmcnt(0)"
#else
#define RNNT_VMCNT(n) "s_waitcnt vmcnt(" #n ")"
#endif

// Skewed ("anti-diagonal major") lattice layout used by every per-cell work array the
// sweep touches: cell (b,t,u) lives at [b][d = t+u][u], D = T+U1-1 diagonals per utterance,
// so that one anti-diagonal is contiguous in HBM (coalesced sweep loads/stores).
__device__ __forceinline__ long skew_index(int b, int t, int u, int D, int U1)
{
    return ((long)b * D + (t + u)) * U1 + u;
}

// Utterance lengths as every kernel reads them: clamped into the lattice (1 <= T_b <= T,
// 0 <= U_b <= U1-1), so a bad length from a caller that skipped the host-side checks
// (check_lengths=False, or the C ABI called directly) can never index outside the per-utterance
// arrays or the LDS mailboxes; it yields the loss of the clamped lattice instead of a fault.
__device__ __forceinline__ int len_t(const int32_t *logit_lens, int b, int T)
{
    const int v = logit_lens[b];
    return v < 1 ? 1 : (v > T ? T : v);
}
__device__ __forceinline__ int len_u(const int32_t *target_lens, int b, int U1)
{
    const int v = target_lens[b];
    return v < 0 ? 0 : (v > U1 - 1 ? U1 - 1 : v);
}

// Both lengths of utterance b (wave-uniform b) by two scalar loads issued together — one round trip
// through the scalar cache instead of two serialised vector loads + readfirstlane at the head of a tile.
// Kernels never write the length arrays, so the scalar cache cannot be stale within a launch.
__device__ __forceinline__ void len_tu_uniform(const int32_t *logit_lens, const int32_t *target_lens, int b, int T, int U1,
                                               int &Tb, int &Ub)
{
    int x, y;
    const int32_t *pl = logit_lens + b, *pt = target_lens + b;
    asm volatile("s_load_dword %0, %2, 0x0\n\ts_load_dword %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(x), "=&s"(y) : "s"(pl), "s"(pt) : "memory");
    Tb = x < 1 ? 1 : (x > T ? T : x);
    Ub = y < 0 ? 0 : (y > U1 - 1 ? U1 - 1 : y);
}

// tanh via one v_exp_f32 + one v_rcp_f32: 1 - 2/(exp(2x)+1).  Saturates correctly at
// +-inf; absolute error <~3e-7 (the result feeds a dot product, absolute error matters).
__device__ __forceinline__ float fast_tanh(float x)
{
    float e = __builtin_amdgcn_exp2f(x * (2.0f * RNNT_LOG2E));
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

// Two at a time on register pairs (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 around the two
// transcendentals of each element): the same operations per element, bit for bit, in 4 + 4 issue slots
// per pair instead of 6 + 4 — VALU instructions share the SIMD's issue port with the MFMA stream.
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2_t fast_tanh2(f32x2_t x)
{
    const f32x2_t a = x * (2.0f * RNNT_LOG2E);
    f32x2_t e = {__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};
    e += 1.0f;
    const f32x2_t r = {__builtin_amdgcn_rcpf(e[0]), __builtin_amdgcn_rcpf(e[1])};
    return 1.0f - 2.0f * r;
}
// tanh(e + p) for four consecutive elements
__device__ __forceinline__ f32x4 fast_tanh_sum4(f32x4 e, f32x4 p)
{
    const f32x2_t lo = fast_tanh2(__builtin_shufflevector(e, e, 0, 1) + __builtin_shufflevector(p, p, 0, 1));
    const f32x2_t hi = fast_tanh2(__builtin_shufflevector(e, e, 2, 3) + __builtin_shufflevector(p, p, 2, 3));
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
}

// 32-lane (half-wave) butterfly reductions; xor masks < 32 never cross the wave halves,
// matching the 32x32 MFMA accumulator layout where lanes 0-31 / 32-63 hold different rows.
__device__ __forceinline__ float half_max(float v)
{
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float half_sum(float v)
{
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// The same reductions on the DPP crossbar (VALU rate, no LDS round trip: __shfl_xor lowers to
// ds_bpermute_b32): quad_perm xor 1, xor 2, row_ror 4, 8 give every lane its 16-lane row's
// result; row_bcast15 into rows 1 and 3 completes the 32-lane half in lanes 16-31 / 48-63;
// half_bcast() hands that to every lane of the half.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_mov(float old, float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float half_bcast(float v, int half)
{
    const float lo = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 31));
    const float hi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
    return half ? hi : lo;
}
// The first four steps have the DPP operand fused into the max / add itself (hipcc keeps v_mov_b32_dpp +
// the operation + a register copy apart: three VALU issue slots per step instead of one).  Inputs are
// finite or -inf (max) / finite (sum): no NaN canonicalisation needed.  s_nop 1: the two wait states
// between a VALU write and a DPP read of the same register, which the assembler does not add inside asm.
__device__ __forceinline__ float half_max_dpp(float v, int half)
{
    asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf"
                 : "+v"(v));
    v = fmaxf(v, dpp_mov<0x142, 0xa>(RNNT_NEG_INF, v));
    return half_bcast(v, half);
}
__device__ __forceinline__ float half_sum_dpp(float v, int half)  // valid in lanes 16-31 / 48-63
{
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf"
                 : "+v"(v));
    v += dpp_mov<0x142, 0xa>(0.f, v);
    return v;
}

// FOUR independent reductions at once, interleaved step by step in one block: the same five steps per value (the row_bcast15 step,
// row_mask 0xa, included: rows 0 and 2 keep their value, which is what max(v, -inf) / v + 0 leave), so every result has the bits of
// half_max_dpp before its broadcast / of half_sum_dpp.  Between a register's write and the next DPP read of it stand the three
// instructions of the other values: more than the two wait states, which only the block's first step has to buy with an s_nop
// (the values come from VALU instructions right in front).  The trailing s_nop covers whatever the compiler places behind the block.
#define RNNT_DPP4_STEP(op, ctrl)                     \
    op " %0, %0, %0 " ctrl " bank_mask:0xf\n\t"     \
    op " %1, %1, %1 " ctrl " bank_mask:0xf\n\t"     \
    op " %2, %2, %2 " ctrl " bank_mask:0xf\n\t"     \
    op " %3, %3, %3 " ctrl " bank_mask:0xf\n\t"
#define RNNT_DPP4_TREE(op)                                        \
    "s_nop 1\n\t"                                                 \
    RNNT_DPP4_STEP(op, "quad_perm:[1,0,3,2] row_mask:0xf")        \
    RNNT_DPP4_STEP(op, "quad_perm:[2,3,0,1] row_mask:0xf")        \
    RNNT_DPP4_STEP(op, "row_ror:4 row_mask:0xf")                  \
    RNNT_DPP4_STEP(op, "row_ror:8 row_mask:0xf")                  \
    RNNT_DPP4_STEP(op, "row_bcast:15 row_mask:0xa")               \
    "s_nop 1"
__device__ __forceinline__ void half_max_dpp_x4(float &a, float &b, float &c, float &d)  // valid in lanes 16-31 / 48-63: half_bcast() next
{
    asm volatile(RNNT_DPP4_TREE("v_max_f32_dpp") : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
__device__ __forceinline__ void half_sum_dpp_x4(float &a, float &b, float &c, float &d)  // valid in lanes 16-31 / 48-63
{
    asm volatile(RNNT_DPP4_TREE("v_add_f32_dpp") : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}

// Packed per-cell gradient coefficients written by k_coef, read by the backward GEMMs:
//   G[v] = exp2(logit[v]*log2e + c1) - (v==blank)*sb - (v==y)*se
struct __attribute__((aligned(16))) CellCoef {
    float c1;  // (alpha+beta+cost-denom+log(scale))*log2e, -inf for cells outside the lattice
    float sb;  // blank-transition occupancy * scale
    float se;  // emit-transition occupancy * scale
    int y;     // emit label of this cell (targets[b][u]) or -1
};
