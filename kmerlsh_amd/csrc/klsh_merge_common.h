// What every merge header shares (one translation unit, klsh_merge.hip): fences and the LDS-only
// barrier, the profile macros and their device counters (diagnostics build), wave shuffles,
// the list append, the dirty mark, the sequential dot products and the Gram pre-screen of a pair.
// Defines no kernel.
#pragma once

#include "klsh_device.h"

namespace klsh {

// ------------------------------------------------------------------------------- helpers -----
__device__ __forceinline__ void lds_fence() {
  // orders this workgroup's LDS and global stores before later loads from other lanes of the same
  // wave (waits for outstanding global stores: use only where a global store must be seen)
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}
__device__ __forceinline__ void wave_lds_fence() {
  // LDS executes one wave's instructions in order: within a wave only the compiler must be kept
  // from moving LDS accesses across this point (no wait for outstanding global stores)
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}
// The all-pairs decisions of 65..896-row runs go through the certified MFMA Gram screen when the
// decider has a fast path and d is a multiple of 16 (else the exact VALU tiles).
constexpr bool kGramTiles = true;

// Merge profiling (diagnostics build only: -DKLSH_MERGE_PROF, make prof): per size class, the
// runs, rows, merges and wall-clock ticks (100 MHz) of each phase, summed over the call.
#ifdef KLSH_MERGE_PROF
__device__ unsigned long long g_mprof[8][12];  // [k] 8: loads, 9: norms, 10: walk loop
#define MPROF_T() wall_clock64()
#define MPROF_ADD(c, k, v) atomicAdd(&g_mprof[c][k], (unsigned long long)(v))
#define MPROF_MAX(c, k, v) atomicMax(&g_mprof[c][k], (unsigned long long)(v))
__device__ unsigned long long g_sprof[8][8];  // small-run batches per G class: batches, clocks in
                                              // stage, pairwise, walk, write-back
__device__ unsigned long long g_wprof[8][8];  // walk phases in shader clocks: find, select+
                                              // consensus, dots, bits, steps, find rounds
#define WPROF_CLK() __builtin_amdgcn_s_memtime()
__device__ unsigned long long g_gprof[8];  // Gram tiles: tiles, ambiguous pairs, sum of the wave's
                                           // longest lane list, clocks: acc, screen, exact, bits
#define GPROF_ADD(k, v) atomicAdd(&g_gprof[k], (unsigned long long)(v))
__device__ unsigned long long g_tprof[8];  // k_tail_local phases (10-ns ticks summed over
                                           // workgroups): base, counts, lists, scatter; workgroups;
                                           // max total
#define TPROF_ADD(k, v) atomicAdd(&g_tprof[k], (unsigned long long)(v))
#else
#define TPROF_ADD(k, v) (void)0
#define GPROF_ADD(k, v) (void)0
#define MPROF_T() 0ull
#define MPROF_ADD(c, k, v) (void)0
#define MPROF_MAX(c, k, v) (void)0
#define WPROF_CLK() 0ull
#endif

__device__ __forceinline__ void lds_barrier() {
  // workgroup barrier for LDS data only: this wave's LDS stores have landed (lgkmcnt(0)), then
  // s_barrier — without the vmcnt(0) wait of __syncthreads for outstanding global stores
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t shfl32(uint32_t v, uint32_t src) {
  return (uint32_t)__shfl((int)v, (int)src, 64);
}
__device__ __forceinline__ float shflf(float v, uint32_t src) { return __shfl(v, (int)src, 64); }
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src) {
  const uint32_t lo = shfl32((uint32_t)v, src), hi = shfl32((uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}
// v_writelane_b32: lane `l` (a constant after unrolling) of v becomes the wave-uniform value s
__device__ __forceinline__ uint32_t writelane(uint32_t v, uint32_t s, int l) {
#ifdef __OPTIMIZE__
  asm volatile("v_writelane_b32 %0, %1, %2"
               : "=v"(v)
               : "s"(__builtin_amdgcn_readfirstlane(s)), "i"(l), "0"(v));
  return v;
#else  // (the host-sanitizer build compiles device code at -O0: no constant lane to encode)
  return (int)__lane_id() == l ? s : v;
#endif
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ __forceinline__ uint64_t lanes_below(uint32_t lane) {
  return lane ? (~0ull >> (64 - lane)) : 0ull;
}

// Wave-aggregated append of `slot` for the lanes with `pred` (all lanes of the wave must call).
__device__ __forceinline__ void append_slot(bool pred, uint32_t slot, uint32_t* list,
                                            uint32_t* counter) {
  const uint64_t m = __ballot(pred);
  if (m == 0ull) return;
  const uint32_t lane = __lane_id();
  const uint32_t leader = (uint32_t)(__ffsll((unsigned long long)m) - 1);
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
  base = shfl32(base, leader);
  if (pred) list[base + (uint32_t)__popcll(m & lanes_below(lane))] = slot;
}

// In-place kernels: record `slot` as rewritten once per iteration.
__device__ __forceinline__ void mark_dirty(uint32_t slot, const DeltaSink& k, Counters* ctr) {
  if (k.dlist && k.mark[slot] != k.stamp) {
    k.mark[slot] = k.stamp;
    k.dlist[atomicAdd(&ctr->n_delta, 1u)] = slot;
  }
}

template <int D>
__device__ __forceinline__ float dot_reg_lds(const float (&a)[D], const float* b) {
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < D; k += 4) {
    const float4 v = *reinterpret_cast<const float4*>(b + k);
    s = s + a[k] * v.x;
    s = s + a[k + 1] * v.y;
    s = s + a[k + 2] * v.z;
    s = s + a[k + 3] * v.w;
  }
  return s;
}

template <int D>
__device__ __forceinline__ void dot2_reg_lds(const float (&a)[D], const float* b0, const float* b1,
                                             float& s0, float& s1) {
  s0 = 0.0f;
  s1 = 0.0f;
#pragma unroll
  for (int k = 0; k < D; k += 4) {
    const float4 u = *reinterpret_cast<const float4*>(b0 + k);
    const float4 v = *reinterpret_cast<const float4*>(b1 + k);
    s0 = s0 + a[k] * u.x;
    s1 = s1 + a[k] * v.x;
    s0 = s0 + a[k + 1] * u.y;
    s1 = s1 + a[k + 1] * v.y;
    s0 = s0 + a[k + 2] * u.z;
    s1 = s1 + a[k + 2] * v.z;
    s0 = s0 + a[k + 3] * u.w;
    s1 = s1 + a[k + 3] * v.w;
  }
}

__device__ __forceinline__ int size_class(uint32_t b) {  // G = 2 << class lanes per run
  return b <= 2 ? 0 : b <= 4 ? 1 : b <= 8 ? 2 : b <= 16 ? 3 : b <= 32 ? 4 : 5;
}

// Pre-screen of one pair from an approximate dot product g (a Gram tile, or short chains) within
// kGramMargin * |a||b| of the reference's sequential one: 1 = merge, 0 = no merge, 2 = too close
// to call (or den outside the fast range): the exact sequential dot decides.
__device__ __forceinline__ uint32_t prescreen(const Decider& dc, float g, float den) {
  if (den >= 0x1p-60f && den <= 0x1p60f) {
    const float q = g * __builtin_amdgcn_rcpf(den);
    if (q >= dc.g_hi) return 1u;
    if (q <= dc.g_lo) return 0u;
  }
  return 2u;
}

// s + sequential sum of a[e] * b[e], e < n, a and b in memory (16-B aligned rows)
__device__ __forceinline__ float dot_acc_mem(float s, const float* a, const float* b, int n) {
  int k = 0;
  for (; k + 4 <= n; k += 4) {
    const float4 u = *reinterpret_cast<const float4*>(a + k);
    const float4 v = *reinterpret_cast<const float4*>(b + k);
    s = s + u.x * v.x;
    s = s + u.y * v.y;
    s = s + u.z * v.z;
    s = s + u.w * v.w;
  }
  for (; k < n; ++k) s = s + a[k] * b[k];
  return s;
}

// The same sequential sum for a compile-time width D (a multiple of 4; D == 0: runtime d): every
// load is issued before the chain starts, so the chain does not wait on a load every 4 terms.
template <int D>
__device__ __forceinline__ float dot_seq(const float* a, const float* b, int d) {
  if constexpr (D == 0) {
    return dot_acc_mem(0.0f, a, b, d);
  } else {
    float4 u[D / 4], v[D / 4];
#pragma unroll
    for (int k = 0; k < D / 4; ++k) {
      u[k] = *reinterpret_cast<const float4*>(a + 4 * k);
      v[k] = *reinterpret_cast<const float4*>(b + 4 * k);
    }
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < D / 4; ++k) {
      s = s + u[k].x * v[k].x;
      s = s + u[k].y * v[k].y;
      s = s + u[k].z * v[k].z;
      s = s + u[k].w * v[k].w;
    }
    return s;
  }
}

}  // namespace klsh
