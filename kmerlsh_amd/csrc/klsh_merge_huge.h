// Runs longer than 896 rows at any d: the reference walk directly, one workgroup per run.
// Kernel: k_merge_huge; huge_runs is also folded into k_merge_big<.., 896, ..>, k_merge_tail,
// k_merge_big_wide and k_merge_long (runs past kLongRows).
#pragma once

#include "klsh_merge_common.h"

namespace klsh {

// ------------------------------------------------------ runs longer than 896 rows: workgroups -----
// The reference walk directly (no decision matrix: it would not fit), one workgroup of NT lanes
// per run: the visited row i sits in LDS, every lane tests one candidate j < i per chunk (rows
// from memory, one exact sequential dot product each), and the first hit of the chunk is found
// by a ballot + cross-wave min.  The run's slots and sqrtf(norms) live in LDS when they fit.
constexpr int kHugeNT = 512;
constexpr int kHugeKB = 8;  // visited rows tested per pass (half at d = 64); 16 measured the same
constexpr uint32_t kHugeLdsRows = 8192;  // a huge run's slots and norms in LDS up to this length

// The runs li = first, first + stride, ... (< count) of the huge list, one workgroup of NT lanes
// per run (k_merge_huge: 512 lanes; k_merge_tail's big-run workgroups: 256), smem = huge_lds().
template <int D, int NT>  // D: d at compile time (unrolled dots), 0 = any d
__device__ __forceinline__ void huge_runs(const uint2* __restrict__ list, uint32_t count,
                                          uint32_t first, uint32_t stride,
                                          uint32_t* __restrict__ slots, const Decider& dc,
                                          const Rows& r, const DeltaSink& sink, Counters* ctr,
                                          unsigned char* smem) {
  constexpr int NW = NT / 64;
  constexpr int kHugeNT = NT;  // (the body below is written for any NT)
  uint32_t* ls = reinterpret_cast<uint32_t*>(smem);             // [kHugeLdsRows] slots
  float* lq = reinterpret_cast<float*>(ls + kHugeLdsRows);       // [kHugeLdsRows] sqrtf(nrm)
  float* xi = lq + kHugeLdsRows;                                 // [dp] the visited row
  __shared__ uint32_t wmin[2][NW];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const int d = r.d, dp = r.dp;
  uint32_t par = 0;
  for (uint32_t li = first; li < count; li += stride) {
    const uint2 e = list[li];
    const uint32_t p = e.x, b = e.y;
    const bool in_lds = b <= kHugeLdsRows;
    [[maybe_unused]] const uint64_t pt0 = MPROF_T();
    uint32_t* S = in_lds ? ls : slots + p;
    if (in_lds)
      for (uint32_t a = t; a < b; a += kHugeNT) {
        const uint32_t sa = slots[p + a];
        ls[a] = sa;
        lq[a] = __builtin_sqrtf(r.nrm[sa]);
      }
    __syncthreads();
    auto sqrt_at = [&](uint32_t a) { return in_lds ? lq[a] : __builtin_sqrtf(r.nrm[S[a]]); };
    uint32_t size = b, i = 1;
    if constexpr (D > 0) {
      // KB visited rows at once: positions i .. i+kc-1 are tested against every position below
      // them in one pass over the run (each candidate row j loaded once for KB dot products).
      // Until some candidate matches, the walk would visit exactly these rows in this order with
      // nothing changed, so the first candidate a* with a match (smallest j) is the reference's
      // next merge and the candidates before it simply advance i; the ones after it are
      // re-tested next pass.  A hit of candidate 0 ends the pass at its chunk (as the one-row walk
      // did), so merge-dense runs pay no extra chunks.
      constexpr int KB = D <= 32 ? kHugeKB : kHugeKB / 2;
      float* xk = xi;                          // [KB][dp] candidate rows
      float* sqk = xk + KB * dp;               // [KB] their sqrtf(norms)
      uint32_t* wk = reinterpret_cast<uint32_t*>(sqk + KB);  // [KB][NW] per-wave first hits
      while (i < size) {  // block-uniform
        const uint32_t kc = min((uint32_t)KB, size - i);
        for (uint32_t q = t; q < kc * (uint32_t)(D / 4); q += kHugeNT) {
          const uint32_t a = q / (D / 4), k4 = q % (D / 4);
          *reinterpret_cast<float4*>(xk + a * dp + 4 * k4) =
              *reinterpret_cast<const float4*>(r.x + (size_t)S[i + a] * dp + 4 * k4);
        }
        if (t < kc) sqk[t] = sqrt_at(i + t);
        __syncthreads();
        uint32_t first[KB];  // this wave's first hit per candidate (wave-uniform)
#pragma unroll
        for (int a = 0; a < KB; ++a) first[a] = 0xFFFFFFFFu;
        const uint32_t jend = i + kc - 1;  // candidate a tests positions j < i + a
        for (uint32_t c0 = 0; c0 < jend; c0 += kHugeNT) {
          const uint32_t j = c0 + t;
          bool ok[KB];
#pragma unroll
          for (int a = 0; a < KB; ++a) ok[a] = false;
          if (j < jend) {
            float xj[D];
            load_row<D>(r.x + (size_t)S[j] * dp, xj);
            const float sqj = sqrt_at(j);
#pragma unroll
            for (int a = 0; a < KB; ++a)
              if ((uint32_t)a < kc && j < i + (uint32_t)a)
                ok[a] = decide(dc, dot_reg_lds<D>(xj, xk + a * dp), sqk[a] * sqj);
          }
#pragma unroll
          for (int a = 0; a < KB; ++a) {
            const uint64_t m = __ballot(ok[a]);
            if (m && first[a] == 0xFFFFFFFFu)
              first[a] = c0 + wv * 64u + (uint32_t)(__ffsll((unsigned long long)m) - 1);
          }
          if (lane == 0) wmin[par][wv] = first[0];
          __syncthreads();
          bool hit0 = false;
#pragma unroll
          for (int q = 0; q < NW; ++q) hit0 = hit0 || wmin[par][q] != 0xFFFFFFFFu;
          par ^= 1u;
          if (hit0) break;  // block-uniform
        }
        if (lane < (uint32_t)KB) {
          uint32_t v = 0xFFFFFFFFu;
#pragma unroll
          for (int a = 0; a < KB; ++a)
            if (lane == (uint32_t)a) v = first[a];
          wk[lane * NW + wv] = v;
        }
        __syncthreads();
        uint32_t astar = 0xFFFFFFFFu, found = 0xFFFFFFFFu;
        for (uint32_t a = 0; a < kc && astar == 0xFFFFFFFFu; ++a) {
          uint32_t best = 0xFFFFFFFFu;
#pragma unroll
          for (int q = 0; q < NW; ++q) best = min(best, wk[a * NW + q]);
          if (best != 0xFFFFFFFFu) {
            astar = a;
            found = best;
          }
        }
        __syncthreads();  // wk and xk are rewritten by the next pass
        if (astar == 0xFFFFFFFFu) {
          i += kc;
          continue;
        }
        i += astar;
        float* xa = xk + astar * dp;
        const uint32_t si = S[i];
        // c[j] = SetConsensus(c[i], c[j]); c[i] = c[--size]  (cluster.cc:70-75)
        const uint32_t sj = S[found];
        const uint32_t ca = r.cnt[si], cb = r.cnt[sj];
        const float fa = (float)(int)ca, fb = (float)(int)cb, fn = (float)(int)(ca + cb);
        float* xj = r.x + (size_t)sj * dp;
        for (int k = (int)t; k < d; k += kHugeNT) {
          const float v = consensus(xa[k], fa, xj[k], fb, fn);
          xa[k] = v;  // the new row, for its norm
          store_row1(r, (size_t)sj * dp + k, v);
        }
        __syncthreads();  // the new row is in memory and in LDS
        if (t == 0) {
          const float nn = dot_seq<D>(xa, xa, d);  // distance.cc:33-34
          r.nrm[sj] = nn;
          if (in_lds) lq[found] = __builtin_sqrtf(nn);
          link_members(r, si, sj);
          mark_dirty(sj, sink, ctr);
          S[i] = S[size - 1];
          if (in_lds) lq[i] = lq[size - 1];
        }
        __syncthreads();
        --size;
      }
    } else {
      while (i < size) {  // block-uniform
        const uint32_t si = S[i];
        const float sqi = sqrt_at(i);
        for (int k = (int)t * 4; k < dp; k += kHugeNT * 4)
          *reinterpret_cast<float4*>(xi + k) =
              *reinterpret_cast<const float4*>(r.x + (size_t)si * dp + k);
        __syncthreads();
        uint32_t found = 0xFFFFFFFFu;
        for (uint32_t c0 = 0; c0 < i; c0 += kHugeNT) {  // the first j < i that matches
          const uint32_t j = c0 + t;
          bool ok = false;
          if (j < i) {
            const uint32_t sj = S[j];
            ok = decide(dc, dot_seq<D>(xi, r.x + (size_t)sj * dp, d), sqi * sqrt_at(j));
          }
          const uint64_t m = __ballot(ok);
          if (lane == 0)
            wmin[par][wv] = m ? c0 + wv * 64u + (uint32_t)(__ffsll((unsigned long long)m) - 1)
                              : 0xFFFFFFFFu;
          __syncthreads();
          uint32_t best = 0xFFFFFFFFu;
#pragma unroll
          for (int q = 0; q < NW; ++q) best = min(best, wmin[par][q]);
          par ^= 1u;
          if (best != 0xFFFFFFFFu) {  // block-uniform
            found = best;
            break;
          }
        }
        if (found == 0xFFFFFFFFu) {
          ++i;
          continue;
        }
        // c[j] = SetConsensus(c[i], c[j]); c[i] = c[--size]  (cluster.cc:70-75)
        const uint32_t sj = S[found];
        const uint32_t ca = r.cnt[si], cb = r.cnt[sj];
        const float fa = (float)(int)ca, fb = (float)(int)cb, fn = (float)(int)(ca + cb);
        float* xj = r.x + (size_t)sj * dp;
        for (int k = (int)t; k < d; k += kHugeNT) {
          const float v = consensus(xi[k], fa, xj[k], fb, fn);
          xi[k] = v;  // the new row, for its norm
          store_row1(r, (size_t)sj * dp + k, v);
        }
        __syncthreads();  // the new row is in memory and in LDS
        if (t == 0) {
          const float nn = dot_seq<D>(xi, xi, d);  // distance.cc:33-34
          r.nrm[sj] = nn;
          if (in_lds) lq[found] = __builtin_sqrtf(nn);
          link_members(r, si, sj);
          mark_dirty(sj, sink, ctr);
          S[i] = S[size - 1];
          if (in_lds) lq[i] = lq[size - 1];
        }
        __syncthreads();
        --size;
      }
    }
    if (in_lds)
      for (uint32_t a = t; a < size; a += kHugeNT) slots[p + a] = ls[a];
    for (uint32_t a = size + t; a < b; a += kHugeNT) slots[p + a] = kInvalid;
    __syncthreads();
    if (t == 0) {
      MPROF_ADD(kBigClasses, 0, 1);
      MPROF_ADD(kBigClasses, 1, b);
      MPROF_ADD(kBigClasses, 2, b - size);
      MPROF_ADD(kBigClasses, 4, MPROF_T() - pt0);
      MPROF_MAX(kBigClasses, 5, MPROF_T() - pt0);
      MPROF_MAX(kBigClasses, 6, b);
    }
  }
}

template <int D>
__global__ __launch_bounds__(kHugeNT) void k_merge_huge(const uint2* __restrict__ list,
                                                       const uint32_t* count_ptr,
                                                       uint32_t* __restrict__ slots, Decider dc,
                                                       Rows r, MergeView w, Counters* ctr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  kt_begin(w.kt, KC_HUGE);
  const uint32_t count = __hip_atomic_load(count_ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  huge_runs<D, kHugeNT>(list, count, blockIdx.x, gridDim.x, slots, dc, r, w.sink, ctr, smem);
  kt_end(w.kt, KC_HUGE);
}

// LDS of huge_runs: slots + sqrt norms, then the candidate rows + their norms + per-wave first
// hits (register widths), or the visited row
static size_t huge_lds(int d, int dp, int nt) {
  const bool batched = d == 8 || d == 16 || d == 32 || d == 64;
  return sizeof(uint32_t) * kHugeLdsRows * 2 +
         (batched ? sizeof(float) * (size_t)dp * kHugeKB + sizeof(float) * kHugeKB +
                        sizeof(uint32_t) * kHugeKB * (nt / 64)
                  : sizeof(float) * (size_t)dp);
}

}  // namespace klsh
