// What attention.hip (f16 operands) and attention_split.hip (hi/lo operand pairs) share: tile constants, the cross-lane
// steps of the online softmax, the hand-counted LDS reads, and the argument checks of the two launchers.
#pragma once
#include "kernels.h"
#include "wca_common.h"

namespace wca {

constexpr int KT = 64;               // keys per tile
constexpr int TILE = 64 * 64;        // f16 elements of one 64-key x 64-dim K or V tile
constexpr float LOG2E = 1.4426950408889634f;
// Deferred running-max update of the lazy online softmax: a row's running maximum m is only raised (and O, l rescaled)
// when a tile's scores exceed it by more than RESCALE_THR in the log2 domain; until then p = exp2(s' - m) may be as large as
// 2^THR = 256 -- exact to f16's 11 bits like any other p (f16 keeps its relative precision up to 65504), sums are fp32.
// Without the threshold the wave-uniform rescale branch fires on almost every tile (32 rows per wave: on random data at
// least one row's maximum grows in 75-100 % of the tiles), ~90 extra vector instructions per wave-tile.
constexpr float RESCALE_THR = 8.0f;

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float max3f(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// max / sum over the lanes {l, l^16} / {l, l^32} without LDS: the swap returns {own, partner} in some order
__device__ __forceinline__ float xor16_max(float v) {
  const unsigned u = __float_as_uint(v);
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xor32_max(float v) {
  const unsigned u = __float_as_uint(v);
  auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xor16_sum(float v) {
  const unsigned u = __float_as_uint(v);
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float xor32_sum(float v) {
  const unsigned u = __float_as_uint(v);
  auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ---- LDS reads the compiler must not schedule or wait for itself. hipcc (ROCm 7.2) puts `s_waitcnt vmcnt(0)` in front of the
// first ds_read_b64_tr_b16 *builtin* of the loop -- it cannot tell the transposed read from the LDS-DMA writes in flight --
// which drains the K/V prefetch on every tile; and it issues a compiler-visible ds_read_b128 only right before its MFMA
// (one read in flight, `lgkmcnt(0)` each). These inline-asm forms are invisible to that bookkeeping: the caller counts
// lgkmcnt itself (LDS operations return in issue order) and names the destinations in the wait statement, so that no
// consumer can be scheduled above the wait (cdna_hip_programming.md 5.7, form (ii)). (On attn_split_kernel the prefetch has
// landed by then anyway: 2.13 vs 2.20 ms per encoder layer at B = 64, within box variance -- kept there because it removes the
// dependence on that timing.)
__device__ __forceinline__ unsigned lds_off(const void* p) { return (unsigned)(size_t)(const WCA_LDS char*)p; }
template <int OFF>
__device__ __forceinline__ half8 lds_read_b128_asm(unsigned addr) {
  half8 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "i"(OFF));
  return r;
}
template <int OFF>
__device__ __forceinline__ half4 lds_read_tr_asm(unsigned addr) {
  half4 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "i"(OFF));
  return r;
}
#define WCA_LGKM_WAIT4(N, A, B, C, D)                                                                         \
  do {                                                                                                        \
    asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(A), "+v"(B), "+v"(C), "+v"(D)::"memory");              \
    __builtin_amdgcn_sched_barrier(0);                                                                        \
  } while (0)
#define WCA_LGKM_WAIT8(N, A, B, C, D, E, F, G, H)                                                             \
  do {                                                                                                        \
    asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(A), "+v"(B), "+v"(C), "+v"(D), "+v"(E), "+v"(F), "+v"(G), "+v"(H)::"memory"); \
    __builtin_amdgcn_sched_barrier(0);                                                                        \
  } while (0)

// What both launchers ask of AttnArgs once nq and B are known to be positive: keys, 16-byte Q / K / V rows, 8-byte O rows, and
// capture rows of whole float4s that hold cap_cols
inline bool attn_args_ok(const AttnArgs& a) {
  if (a.nk <= 0) return false;
  if ((a.q_rs % 8) || (a.k_rs % 8) || (a.v_rs % 8) || (a.o_rs % 4)) return false;
  return a.cap == nullptr || ((a.cap_ld % 4) == 0 && a.cap_ld >= ((a.cap_cols + 3) & ~3));
}

}  // namespace wca
