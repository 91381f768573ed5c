// What more than one implicit-GEMM kernel family shares (igemm_generic.hip, igemm_ws.hip, igemm_m32.hip, igemm_ws64.hip): the LDS-DMA
// pieces, the 16x16 MFMA wrappers, the row decode of the persistent kernels and the host side of its magics.  Every family is its own
// translation unit and exports one launcher (conv_plan.h); conv_launch.cpp switches over them.
//
// GEMM view (per workgroup):   D[ch][pix] = sum_k W[ch][k] * X[k][pix]
//   A operand = weights  [BCH rows ][BK]  (K contiguous; pre-packed, BN folded, zero padded)
//   B operand = gathered [BPIX rows][BK]  input patch (NDHWC, k = tap*Cin + c)
// Both operand tiles travel global -> LDS with `global_load_lds_dwordx4` (no VGPR staging, no ds_write pass).  The LDS image of a
// tile is lane-linear (wave-uniform base + lane*16 bytes), therefore the bank-conflict swizzle is applied on the SOURCE side: the
// lane that fills LDS slot (row, j) fetches global chunk j ^ ((row>>1)&7), and readers XOR the same value (an involution).
#pragma once
#include <type_traits>
#include "common.h"
#include "conv_plan.h"
#include "kernels.h"
#include "prof.h"

namespace rgbm {

// Zero-initialised device memory: the source of every padded chunk of the kernels that request through 64-bit addresses.  One copy
// per translation unit (internal linkage): device code is not relocatable, so the families cannot share one.
[[maybe_unused]] static __device__ uint4 g_zero_page[4];

// LDS-DMA issued from inline asm ON PURPOSE: for the builtin, hipcc (ROCm 7.2) conservatively places `s_waitcnt vmcnt(0)`
// in front of the first ds_read that follows, which drains the loads of the NEXT K tile before the current one is
// multiplied (seen in the ISA: issue -> vmcnt(0) -> ds_read -> mfma, i.e. no load/compute overlap inside a workgroup).
// An asm DMA is invisible to that bookkeeping; completion is enforced by our own counted `s_waitcnt vmcnt(N)` + barrier.
// lds_off: wave-uniform LDS byte address of this wave's 1 KiB slot (hardware adds lane*16).  M0 is left modified: nothing
// else in these kernels reads it (gfx9+ DS instructions do not), and saving/restoring it cost 2 SALU per piece.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_off) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(gsrc), "s"(lds_off) : "memory");
}
// one LDS-DMA piece through a buffer descriptor: lane address = base + voff + soff (soff is not part of the range check: a lane whose
// voff is >= num_records reads nothing and delivers zeros).  tools/micro/cu_fill_rate.hip: one wave sustains 37-43 GB/s of 1 KiB pieces
// this way against 27-32 GB/s with 64-bit global addresses, four waves 120-144 against 104-114
__device__ __forceinline__ void blds16(unsigned voff, const __amdgpu_buffer_rsrc_t& rsrc, unsigned soff, unsigned lds_off) {
  asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" :: "v"(voff), "s"(rsrc), "s"(soff), "s"(lds_off) : "memory");
}
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(unsigned long long)(__attribute__((address_space(3))) const void*)p;
}

// s_barrier with the LDS accesses pinned to their side of it: the builtin alone is IntrNoMem for the compiler, which may hoist a
// later ds_read above it (seen in conv0_sweep.hip's ISA) — a read of a stage another wave has not finished filling
#define RGBM_BARRIER() do { asm volatile("" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } while (0)

template <typename T> struct MmaG;
template <> struct MmaG<unsigned short> {
  __device__ static __forceinline__ void run(const uint4& a, const uint4& b, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
  __device__ static __forceinline__ f32x4 run2(const uint4& a, const uint4& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};
template <> struct MmaG<f16_t> {
  __device__ static __forceinline__ void run(const uint4& a, const uint4& b, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  __device__ static __forceinline__ f32x4 run2(const uint4& a, const uint4& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};
template <> struct MmaG<float> {
  __device__ static __forceinline__ void run(const uint4& a, const uint4& b, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
  }
};

template <> struct MmaG<bx3_t> {
  __device__ static __forceinline__ void run(const uint4& a, const uint4& b, f32x4& c) { c = mma_bx3_k16(a, b, c); }
};
// profiler row (prof.h) of the 128 x 256 launches: conv_igemm_ws_kernel and its non-uniform-tap fallback conv_igemm_v3_kernel
template <typename T> constexpr int prof_row_ws() { return std::is_same<T, bx3_t>::value ? 29 : sizeof(T) == 2 ? 13 : 12; }

template <int N> struct IC { static constexpr int value = N; };

__device__ __forceinline__ float apply_act_g(float v, int act, float slope) {
  if (act == ACT_RELU) return v < 0.f ? 0.f : v;          // NaN propagates like torch
  if (act == ACT_PRELU) return v < 0.f ? v * slope : v;
  if (act == ACT_TANH) return tanhf(v);
  return v;
}

// n / divisor for n < 2^31 with a host-made magic: one 32x32->64 multiply and a shift instead of ~35 instructions
__device__ __forceinline__ unsigned fdiv(unsigned n, unsigned m, int sh) {
  return (unsigned)(((unsigned long long)n * m) >> sh);
}
// output-grid coordinates of GEMM row m
__device__ __forceinline__ void decode_row(const ConvDesc& d, unsigned m, unsigned& n, unsigned& qd, unsigned& qh, unsigned& qw) {
  unsigned t = m;
  unsigned q = fdiv(t, d.fd_m[0], d.fd_s[0]); qw = t - q * (unsigned)d.Wq; t = q;
  q = fdiv(t, d.fd_m[1], d.fd_s[1]); qh = t - q * (unsigned)d.Hq; t = q;
  q = fdiv(t, d.fd_m[2], d.fd_s[2]); qd = t - q * (unsigned)d.Dq; n = q;
}

// magic for n / dvs, n < 2^31: q = (n * m) >> sh  (round-up method, sh = 31 + ceil(log2 dvs))
static void make_fastdiv(int dvs, unsigned& m, int& sh) {
  int s = 0;
  while ((1ll << s) < (long long)dvs) ++s;
  sh = 31 + s;
  m = (unsigned)(((1ull << sh) + (unsigned long long)dvs - 1ull) / (unsigned long long)dvs);
}

// the persistent kernels' decode_row magics for Wq / Hq / Dq
static void fill_fastdiv(ConvDesc& d) {
  make_fastdiv(d.Wq, d.fd_m[0], d.fd_s[0]);
  make_fastdiv(d.Hq, d.fd_m[1], d.fd_s[1]);
  make_fastdiv(d.Dq, d.fd_m[2], d.fd_s[2]);
}

}  // namespace rgbm
