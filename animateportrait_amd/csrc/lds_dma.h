// lds_dma.h -- what the matrix kernels share below the level of a kernel: the bf16 fragment type and the head / tail split, the
// raw LDS-DMA issue, and the compile-time loop that gives every piece of a stage a constant index.
// Users: conv_bf16x3.h (with conv_bf3_dma.h), conv_ph4.h, conv_tapgemm.h, wgrad_bf16x3.h, wgrad_xs.h, wgrad_operand.h, tools/variants/.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <utility>

namespace apamd {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split_bf16(float v, __bf16& hi, __bf16& lo) {
    hi = (__bf16)v;
    lo = (__bf16)(v - (float)hi);
}

// LDS-DMA issued behind the compiler's back.  With the builtin, the compiler books every in-flight
// global_load_lds as a "flat access that may touch LDS" and degrades each later s_waitcnt on an LDS read to
// lgkmcnt(0) for as long as the DMA is pending -- i.e. through the whole MFMA stage this kernel overlaps it with.
// Raw issue keeps the fragment-read waits exact; the price is that completion must be awaited explicitly
// (dma_wait_all) before the barrier that publishes the stage.  lds_addr: wave-uniform LDS byte address of
// lane 0's 16 bytes (lane i lands at +16 i).
// Source address = scalar base + per-lane unsigned 32-bit byte offset.
__device__ __forceinline__ void glds16_sv(const void* sbase, unsigned voff, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_addr)
                 : "memory", "m0");
}
// The same with the LDS address as scalar base + compile-time offset: one s_add into M0 per piece.  (Passing each piece's
// LDS address as a value kept 19 scalars alive per stage; with ~100 SGPRs in use the compiler spilled them into VGPR lanes
// and read them back with v_readlane in front of every piece: profiles/r05_dominant_cycle_account.md.)
template <int IMM>
__device__ __forceinline__ void glds16_si(const void* sbase, unsigned voff, unsigned lds_base) {
    asm volatile("s_add_u32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_base), "n"(IMM)
                 : "memory", "m0", "scc");
}
// LDS-DMA with a per-lane 64-bit source address (lane i lands at lds_addr + 16 i)
__device__ __forceinline__ void glds16_vv(const void* src, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(lds_addr) : "memory", "m0");
}
__device__ __forceinline__ void dma_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

template <class F, int... J>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, J...>) {
    (f(std::integral_constant<int, J>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

}  // namespace apamd
