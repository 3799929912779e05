// mma_common.hpp — the toolkit of the MFMA route files (bf16.hip, x3.hip, x2.hip; typedefs also joint_fwd.hip, joint_bwd.hip, engine.hip):
// vector types, 16-bit pack / unpack, the two 32x32x16 MFMA wrappers, the LDS barrier, counted LDS waits that name the registers
// they release, the workgroup-0 clock stamp of the diagnostic builds and the host's opt-in to more than 64 KiB of dynamic LDS.
#pragma once
#include "common.hpp"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((address_space(3))) void *lds_vptr;

// two fp32 values -> one dword of two 16-bit values, element 0 in the low half
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi)
{
    bf16x2 v = {(__bf16)lo, (__bf16)hi};  // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
    return __builtin_bit_cast(unsigned, v);
}
// fp16 in two spellings of one conversion (both v_cvt_pk_f16_f32: RNE, the same bits): the vector convert (bf16.hip) and the pair of
// scalar converts (x2.hip).  The compiler schedules and allocates the code around them differently, and every hand-scheduled kernel
// keeps the spelling it was tuned with: with the other one k_joint_fwd_bf16* gain scratch, k_joint_fwd_x2<1> changes its registers.
__device__ __forceinline__ unsigned pack_f16(float lo, float hi)
{
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
}
__device__ __forceinline__ unsigned pack_f16_pair(float lo, float hi)
{
    f16x2 v = {(_Float16)lo, (_Float16)hi};
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ float f16_lo(unsigned u) { return (float)__builtin_bit_cast(f16x2, u)[0]; }
__device__ __forceinline__ float f16_hi(unsigned u) { return (float)__builtin_bit_cast(f16x2, u)[1]; }

__device__ __forceinline__ f32x16 mfma_bf16(u32x4 a, u32x4 b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_f16(u32x4 a, u32x4 b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// publish this wave's LDS writes / retire its LDS reads, then join the workgroup.  Not __syncthreads(): that also waits
// vmcnt(0) and would drain the global prefetch rings.
__device__ __forceinline__ void lds_barrier()
{
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// a compile-time integer as a lambda argument: ring stages, planes and piece numbers become immediates
template <int N> struct Int { static constexpr int value = N; };

// Results of inline-asm LDS reads may be used only after a wait that NAMES their registers: the compiler orders nothing else.
// Eight dwords of transposed reads (4 tiles: cells 0-3 / 4-7 of a lane's 8), landed once at most N later LDS operations are in flight:
struct Frag8 { u32x2 lo[4], hi[4]; };
#define FRAG8_LANDED(f, N)                                                                                       \
    asm volatile("s_waitcnt lgkmcnt(" #N ")"                                                                     \
                 : "+v"(f.lo[0]), "+v"(f.lo[1]), "+v"(f.lo[2]), "+v"(f.lo[3]), "+v"(f.hi[0]), "+v"(f.hi[1]),     \
                   "+v"(f.hi[2]), "+v"(f.hi[3])                                                                  \
                 :: "memory")
// the same for eight registers b[0..7]
#define LDS_WAIT8_BUT(b, N) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]) :: "memory")
#define LDS_WAIT8(b) LDS_WAIT8_BUT(b, 0)

// Diagnostic builds only: workgroup (0,0,0) of a kernel with an argument block `a` stamps the core clock counter and the 100 MHz
// reference into a.debug[SLOT], a.debug[SLOT + 1] (a buffer nothing else reads), once at its start and once at its end: the clock
// the launch ran at = d(s_memtime) / d(s_memrealtime) x 100 MHz.  BF_CLOCK_STAMP (bf16.hip) is compiled in by -DBF_CLOCK, with an
// engine.o built -DRNNT_STAMPS so that Bf16Args::debug is set (tools/exp_bf16_clock.py); X_CLOCK_STAMP (x3.hip, x2.hip) by
// -DRNNT_STAMPS (tools/exp_x3_clock.py).  The shipped build compiles both to nothing.
#define CLOCK_STAMP_BODY(SLOT)                                                                                             \
    do {                                                                                                                   \
        if (a.debug && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) {                        \
            unsigned long long t_, r_;                                                                                     \
            asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_), "=s"(r_)::"memory");      \
            a.debug[SLOT] = t_; a.debug[(SLOT) + 1] = r_;                                                                  \
        }                                                                                                                  \
    } while (0)
#ifdef BF_CLOCK
#define BF_CLOCK_STAMP(SLOT) CLOCK_STAMP_BODY(SLOT)
#else
#define BF_CLOCK_STAMP(SLOT) do {} while (0)
#endif
#ifdef RNNT_STAMPS
#define X_CLOCK_STAMP(SLOT) CLOCK_STAMP_BODY(SLOT)
#else
#define X_CLOCK_STAMP(SLOT) do {} while (0)
#endif

// More than 64 KiB of dynamic LDS is an opt-in per kernel and device.  One static LdsOptIn per launcher; raise() names every
// kernel the launcher may start with `bytes` and sets the attribute the first time it is called on a device (a read-mostly fact;
// device unknown or past the table: every call).
struct LdsOptIn {
    bool set[16] = {false};
    template <class... K> void raise(int bytes, K... kernels)
    {
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = -1;
        if (dev >= 0 && set[dev]) return;
        ((void)hipFuncSetAttribute((const void *)kernels, hipFuncAttributeMaxDynamicSharedMemorySize, bytes), ...);
        if (dev >= 0) set[dev] = true;
    }
};
