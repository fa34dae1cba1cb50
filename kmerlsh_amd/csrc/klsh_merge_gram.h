// The certified MFMA Gram tiles (bf16x3 split, exact chains for the close calls): the all-pairs
// decisions of runs of 65 rows and more (klsh_merge_big.h, klsh_merge_long.h) and of the wide
// rows' groups at d = 512 (klsh_merge_wide.h).  Defines no kernel.
#pragma once

#include "klsh_merge_common.h"

namespace klsh {

// ---------------------------------------------------------------- MFMA pre-screen -----
// The all-pairs decisions of a run are a Gram matrix X X^T (b x b x d).  The matrix cores compute
// it with a bf16x3 split (x = hi + lo, hi = bf16(x), lo = bf16(x - hi); G = hi.hi + hi.lo + lo.hi
// accumulated in f32), within kGramMargin * |a||b| of the reference's sequential f32 dot — so
// G / den settles every pair whose quotient is not within the margin of s*; the few that are
// take the exact sequential dot (the reference's order), so every decision is still bit-exact.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ void split8(const float* p, bool ok, bf16x8& hi, bf16x8& lo) {
  float x[8];
  if (ok) {
    const float4 u = *reinterpret_cast<const float4*>(p);
    const float4 v = *reinterpret_cast<const float4*>(p + 4);
    x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w;
    x[4] = v.x; x[5] = v.y; x[6] = v.z; x[7] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = 0.0f;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 h = (__bf16)x[j];
    hi[j] = h;
    lo[j] = (__bf16)(x[j] - (float)h);  // x - hi is exact in f32
  }
}

// One wave: the decisions of rows [R*64, R*64+64) against rows [C*64, C*64+64) (C <= R; pairs
// c < a only), ORed into the position-space matrix P (W words per row, both P[a] bit c and
// P[c] bit a).  rowA(a) / rowB(c) give the rows (LDS or memory); D = d, a multiple of 16.
// The bf16x3 products of rows [a0, a0+64) x [c0, c0+64) over KD columns, accumulated into acc:
// rowA(a) / rowB(c) point at the columns to take (LDS or memory), KD a multiple of 16.
template <int KD, class RowA, class RowB>
__device__ __forceinline__ void gram_acc(uint32_t a0, uint32_t c0, uint32_t b, RowA rowA,
                                         RowB rowB, f32x16 (&acc)[2][2]) {
  const uint32_t lane = __lane_id(), r = lane & 31u, h = lane >> 5;
#pragma unroll
  for (int s = 0; s < KD / 16; ++s) {
    bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const uint32_t a = a0 + m * 32u + r, c = c0 + m * 32u + r;
      split8(a < b ? rowA(a) + 16 * s + 8 * h : nullptr, a < b, ah[m], al[m]);
      split8(c < b ? rowB(c) + 16 * s + 8 * h : nullptr, c < b, bh[m], bl[m]);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[m], bh[n], acc[m][n], 0, 0, 0);
        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[m], bl[n], acc[m][n], 0, 0, 0);
        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[m], bh[n], acc[m][n], 0, 0, 0);
      }
  }
}

template <int D, class RowA, class RowB>
__device__ __forceinline__ void gram_decide_slow(uint32_t R, uint32_t C, uint32_t b,
                                                 const f32x16 (&acc)[2][2], RowA rowA, RowB rowB,
                                                 const float* sq, const Decider& dc, uint64_t* P,
                                                 int W, uint32_t* fb);

// The decisions from accumulated Gram values (gram_acc) as wave masks: every compare of the
// 64 x 64 tile is one v_cmp whose lane mask IS the ballot the matrix words are assembled from, so
// the screen has no branches, no per-pair LDS reads and no per-lane bit packing.  A pair is a hit
// when G >= g_hi * den and a miss when G <= g_lo * den (den = sqrt|a|^2 * sqrt|b|^2, the
// reference's, distance.cc:37; the products' rounding is ~1e-7 of a margin of 1e-4 -- a pair it
// moves across g_hi or g_lo only changes between "settled" and "close call").  Rows past b enter
// with sq = 1 and a zero Gram row/column (gram_acc's zero fill), so they are misses; the diagonal
// tile masks c >= a.  A tile with any close call (or NaN, or a norm outside [2^-30, 2^30], where
// den may leave the screen's range) goes to gram_decide_slow, which decides it exactly as before.
// A tile without a hit writes nothing: P and fb start empty.
template <int D, class RowA, class RowB>
__device__ __forceinline__ void gram_decide(uint32_t R, uint32_t C, uint32_t b,
                                            const f32x16 (&acc)[2][2], RowA rowA, RowB rowB,
                                            const float* sq, const Decider& dc, uint64_t* P,
                                            int W, uint32_t* fb) {
  // d <= 32 (C4's 32-sample rows): tiles with a close call are common enough there that the mask
  // pass is mostly paid twice -- the lane-by-lane path alone measured C4 992-996 -> 925 ms (one box,
  // interleaved); at d = 64 the masks win (C2 214 -> 203 ms)
  if constexpr (D <= 32) {
    gram_decide_slow<D>(R, C, b, acc, rowA, rowB, sq, dc, P, W, fb);
    return;
  }
  const uint32_t lane = __lane_id(), r = lane & 31u, h = lane >> 5;
  const uint32_t a0 = R * 64u, c0 = C * 64u;
  // the norms of my two columns and of my 32 rows (loaded together: one LDS wait)
  float sc[2], sa[2][16];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const uint32_t c = c0 + 32u * n + r;
    sc[n] = sq[min(c, b - 1u)];
    sc[n] = c < b ? sc[n] : 1.0f;
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t a = a0 + 32u * m + (i & 3) + 8u * (i >> 2) + 4u * h;
      sa[m][i] = sq[min(a, b - 1u)];
      sa[m][i] = a < b ? sa[m][i] : 1.0f;
    }
  bool bad = false;
  auto out = [](float v) { return !(v >= 0x1p-30f && v <= 0x1p30f); };
#pragma unroll
  for (int n = 0; n < 2; ++n) bad = bad || out(sc[n]);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) bad = bad || out(sa[m][i]);
  const bool diag = R == C;
  uint64_t anyhit = 0ull, close = __ballot(bad);
  uint64_t own = 0ull;                       // lane L: the word of row a0 + L over the block's columns
  uint32_t tm[2][2] = {{0u, 0u}, {0u, 0u}};  // column c0 + 32n + r: bits over rows 32m + .. (h = 0)
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float thi = dc.g_hi * sa[m][i], tlo = dc.g_lo * sa[m][i];
      const uint32_t ar = (uint32_t)((i & 3) + 8 * (i >> 2));  // row within the half block (h = 0)
      uint64_t bal[2];
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const float g = acc[m][n][i];
        uint64_t H = __ballot(g >= thi * sc[n]);
        uint64_t L = __ballot(g <= tlo * sc[n]);
        if (diag) {  // pairs c < a only (uniform branch)
          const uint64_t lt = m < n ? 0ull : m > n ? ~0ull : __ballot(r < ar + 4u * h);
          H &= lt;
          L |= ~lt;
        }
        close |= ~(H | L);
        anyhit |= H;
        bal[n] = H;
        tm[n][m] |= ((H >> lane) & 1ull) ? (1u << ar) : 0u;
      }
      // rows 32m + ar (lanes h = 0) and 32m + ar + 4 (h = 1): their words over the block's columns
      const uint64_t w0 = (bal[0] & 0xFFFFFFFFull) | (bal[1] << 32);
      const uint64_t w1 = (bal[0] >> 32) | (bal[1] & 0xFFFFFFFF00000000ull);
      const int r0 = 32 * m + (int)ar;
      uint32_t olo = (uint32_t)own, ohi = (uint32_t)(own >> 32);
      olo = writelane(olo, (uint32_t)w0, r0);
      ohi = writelane(ohi, (uint32_t)(w0 >> 32), r0);
      olo = writelane(olo, (uint32_t)w1, r0 + 4);
      ohi = writelane(ohi, (uint32_t)(w1 >> 32), r0 + 4);
      own = ((uint64_t)ohi << 32) | olo;
    }
  if (close) {  // (wave-uniform) rare: the lane-by-lane path with the exact chains
    gram_decide_slow<D>(R, C, b, acc, rowA, rowB, sq, dc, P, W, fb);
    return;
  }
  if (!anyhit) return;
  if (own && a0 + lane < b) {
    atomicOr((unsigned long long*)&P[(a0 + lane) * W + C], (unsigned long long)own);
    // fb (k_merge_long): row a's first match below it, over every column block
    if (fb) atomicMin(&fb[a0 + lane], C * 64u + (uint32_t)__builtin_ctzll(own));
  }
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    // my column's bits: rows 32m + ar + 4h of the block
    const uint64_t mine = ((uint64_t)tm[n][1] << 32 | tm[n][0]) << (4u * h);
    const uint64_t full = mine | shfl64(mine, lane ^ 32u);
    const uint32_t c = c0 + 32u * n + r;
    if (h == 0 && full && c < b) atomicOr((unsigned long long*)&P[c * W + R], (unsigned long long)full);
  }
}

// One wave: the decisions of rows [R*64, R*64+64) against rows [C*64, C*64+64) (C <= R; pairs
// c < a only), ORed into the position-space matrix P (W words per row, both P[a] bit c and
// P[c] bit a).  rowA(a) / rowB(c) give the rows (LDS or memory); D = d, a multiple of 16.
template <int D, class RowA, class RowB>
__device__ __forceinline__ void gram_tile(uint32_t R, uint32_t C, uint32_t b, RowA rowA, RowB rowB,
                                          const float* sq, const Decider& dc, uint64_t* P, int W,
                                          uint32_t* fb = nullptr) {
  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[m][n][i] = 0.0f;
  [[maybe_unused]] const uint64_t gc0 = WPROF_CLK();
  gram_acc<D>(R * 64u, C * 64u, b, rowA, rowB, acc);
#ifdef KLSH_MERGE_PROF
  asm volatile("s_nop 0" ::"v"(acc[1][1][15]) : "memory");
  if (__lane_id() == 0) GPROF_ADD(3, WPROF_CLK() - gc0);
#endif
  [[maybe_unused]] const uint64_t gc1 = WPROF_CLK();
  gram_decide<D>(R, C, b, acc, rowA, rowB, sq, dc, P, W, fb);
#ifdef KLSH_MERGE_PROF
  if (__lane_id() == 0) {
    GPROF_ADD(7, 1);
    GPROF_ADD(4, WPROF_CLK() - gc1);
  }
#endif
}

// The decisions from accumulated Gram values (gram_acc), lane by lane: pre-screen against dc's
// margin, the reference's sequential dot over D columns (rowA / rowB: whole rows) for the close
// calls.  gram_decide's path for a tile with a close call or a row of extreme norm.
template <int D, class RowA, class RowB>
__device__ __forceinline__ void gram_decide_slow(uint32_t R, uint32_t C, uint32_t b,
                                                 const f32x16 (&acc)[2][2], RowA rowA, RowB rowB,
                                                 const float* sq, const Decider& dc, uint64_t* P,
                                                 int W, uint32_t* fb) {
  const uint32_t lane = __lane_id(), r = lane & 31u, h = lane >> 5;
  const uint32_t a0 = R * 64u, c0 = C * 64u;
  [[maybe_unused]] const uint64_t gcd = WPROF_CLK();
  // decisions: acc[m][n][i] is G[a][c] with a = a0 + 32m + (i&3) + 8(i>>2) + 4h, c = c0 + 32n + r;
  // bit e = 32m + 16n + i of hitm / ambm
  uint64_t hitm = 0ull, ambm = 0ull;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint32_t a = a0 + 32u * m + (i & 3) + 8u * (i >> 2) + 4u * h;
        const uint32_t c = c0 + 32u * n + r;
        if (a < b && c < a) {
          const uint32_t v = prescreen(dc, acc[m][n][i], sq[a] * sq[c]);
          const int e = 32 * m + 16 * n + i;
          hitm |= (uint64_t)(v & 1u) << e;
          ambm |= (uint64_t)(v >> 1) << e;
        }
      }
#ifdef KLSH_MERGE_PROF
  asm volatile("s_nop 0" ::"v"((uint32_t)ambm) : "memory");
  [[maybe_unused]] uint64_t gc1 = WPROF_CLK();
  {
    const uint32_t na = (uint32_t)__builtin_popcountll(ambm);
    uint32_t mx = na;
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    uint32_t sm = na;
    for (int o = 32; o > 0; o >>= 1) sm += (uint32_t)__shfl_xor((int)sm, o, 64);
    if (lane == 0) {
      GPROF_ADD(0, 1);
      GPROF_ADD(1, sm);
      GPROF_ADD(2, mx);
    }
  }
#endif
  while (ambm) {  // rare: the exact sequential dot (the reference's order) decides
    const int e = __builtin_ctzll(ambm);
    ambm &= ambm - 1ull;
    const int m = e >> 5, n = (e >> 4) & 1, i = e & 15;
    const uint32_t a = a0 + 32u * m + (i & 3) + 8u * (i >> 2) + 4u * h;
    const uint32_t c = c0 + 32u * n + r;
    const float* pa = rowA(a);
    const float* pc = rowB(c);
    float sdot = 0.0f;
    for (int k = 0; k < D; k += 4) {
      const float4 u = *reinterpret_cast<const float4*>(pa + k);
      const float4 v = *reinterpret_cast<const float4*>(pc + k);
      sdot = sdot + u.x * v.x;
      sdot = sdot + u.y * v.y;
      sdot = sdot + u.z * v.z;
      sdot = sdot + u.w * v.w;
    }
    if (decide(dc, sdot, sq[a] * sq[c])) hitm |= 1ull << e;
  }
#ifdef KLSH_MERGE_PROF
  {
    asm volatile("s_nop 0" ::"v"((uint32_t)hitm) : "memory");
    const uint64_t gc2 = WPROF_CLK();
    if (lane == 0) GPROF_ADD(5, gc2 - gc1);
    gc1 = gc2;
  }
#endif
  uint64_t tmask[2] = {0ull, 0ull};  // column c0+32n+r: bits over the 64 rows of block R
  uint64_t own = 0ull;                // lane L ends up with the word of row a0 + L
#pragma unroll
  for (int m = 0; m < 2; ++m) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t ar = 32u * m + (i & 3) + 8u * (i >> 2) + 4u * h;  // row within the block
      uint64_t bal[2];
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const bool hit = (hitm >> (32 * m + 16 * n + i)) & 1ull;
        tmask[n] |= (hit ? 1ull : 0ull) << ar;
        bal[n] = __ballot(hit);
      }
      // rows r0 (lanes with h = 0) and r0 + 4 (h = 1): their 64-bit words over the block's columns
      const uint32_t r0 = 32u * m + (i & 3) + 8u * (i >> 2);
      const uint64_t w0 = (bal[0] & 0xFFFFFFFFull) | (bal[1] << 32);
      const uint64_t w1 = (bal[0] >> 32) | (bal[1] & 0xFFFFFFFF00000000ull);
      if (lane == r0) own = w0;
      if (lane == r0 + 4u) own = w1;
    }
  }
  if (own && a0 + lane < b) {
    atomicOr((unsigned long long*)&P[(a0 + lane) * W + C], (unsigned long long)own);
    // fb (k_merge_long): row a's first match below it, over every column block
    if (fb) atomicMin(&fb[a0 + lane], C * 64u + (uint32_t)__builtin_ctzll(own));
  }
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const uint64_t full = tmask[n] | shfl64(tmask[n], lane ^ 32u);
    const uint32_t c = c0 + 32u * n + r;
    if (h == 0 && full && c < b) atomicOr((unsigned long long*)&P[c * W + R], (unsigned long long)full);
  }
}

}  // namespace klsh
