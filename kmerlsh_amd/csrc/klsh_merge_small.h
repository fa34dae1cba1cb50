// Runs of 2..64 rows at d = 8, 16, 32, 64 (rows in registers), merged in place by G-lane groups,
// and their fp16 screen (d = 32, 64 with the fp16 row image).  Kernels: k_small_screen,
// k_merge_small; small_loop is also the small-run half of k_merge_tail (klsh_merge_big.h).
#pragma once

#include "klsh_merge_common.h"

namespace klsh {

// --------------------------------------------------------------------- G-lane groups -----
// One batch: 64/G runs of one size class, G lanes per run; lane g of a group is position g of its
// run and holds that position's row (registers, and LDS row `lane` for its partners).  The lane's
// slot is already loaded (the caller pipelines it one batch ahead).
//
// 1. Every pairwise decision of the run, each unordered pair once (lane g pairs with the rows
//    k = 1 .. b/2 positions after it, cyclically; decide(a, c) == decide(c, a): the same products
//    in the same order and the same sqrt product, so the partner receives the bit).  The result is
//    the symmetric decision matrix, one row of position bits per lane.
// 2. The walk, kept in POSITION space: lane q holds the bits of the row at position q against the
//    rows at every position (P), that row's id, slot, metadata and data.  The next merge is the
//    first lane q >= i whose P has a bit below q (one ballot); its first match j is the lowest lane
//    p < i whose bit i is set (the matrix is symmetric: one more ballot).  A merge rewrites the row
//    at j (consensus, split over the group's lanes, in LDS), moves the last position's row and
//    state to lane i (swap-remove), remaps bit `last` to bit i everywhere, and re-decides bit j
//    for the positions still to be visited — through the certified short-chain screen, exact
//    chains only for close calls — whose ballot is the new row's P.
// GT: the group width at compile time, or 0: g_rt at run time (one code path for every class:
// the persistent small-run loop then needs the registers of one instance, not of five).
template <int GT, int D>
__device__ __forceinline__ void merge_batch(uint32_t p, uint32_t b, uint32_t slot,
                                            uint32_t* slots, const Decider& dc, const Rows& r,
                                            float* lds, uint32_t* dlist, Counters* ctr,
                                            uint32_t g_rt = 0) {
  const uint32_t G = GT ? (uint32_t)GT : g_rt;
  constexpr int ST = D + 4;  // padded row stride: 16 lanes of a ds_read_b128 hit distinct banks
  const uint32_t lane = __lane_id();
  const uint32_t g = lane & (G - 1);
  const uint32_t gbase = lane - g;
  const uint64_t gmask = (G == 64) ? ~0ull : (((1ull << (G & 63)) - 1ull) << gbase);
  float* myrow = lds + lane * ST;
  [[maybe_unused]] const uint64_t sp0 = WPROF_CLK();
  [[maybe_unused]] uint64_t sp1 = 0, sp2 = 0, sp3 = 0;
  const bool valid = g < b;
  // the lane's own row straight from memory (no cross-lane address shuffles), then to LDS for its
  // partners
  float x[D];
  if (valid) {
    load_row<D>(r.x + (size_t)slot * r.dp, x);
  } else {
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = 0.0f;
  }
#pragma unroll
  for (int k = 0; k < D; k += 4)
    *reinterpret_cast<float4*>(myrow + k) = make_float4(x[k], x[k + 1], x[k + 2], x[k + 3]);
  wave_lds_fence();
  // the row's norm: recomputed from the row (the same sequential chain that made the cached
  // value, distance.cc:33-34, so the same bits) instead of a random 4-B read of r.nrm
  float nrm = 0.0f;
#pragma unroll
  for (int k = 0; k < D; ++k) nrm = nrm + x[k] * x[k];
  float sq = __builtin_sqrtf(nrm);  // this row's sqrtf(|x|^2), distance.cc:37
  const uint32_t bmax = wave_max(b);
#ifdef KLSH_MERGE_PROF
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  sp1 = WPROF_CLK();
#endif

  // 1. the pairwise decisions
  uint64_t P = 0ull;  // group-local position bits
  {
    const uint32_t half = b / 2;
    auto partner = [&](uint32_t k) {  // (g + k) mod b, for k <= b
      const uint32_t j = g + k;
      return j >= b ? j - b : j;
    };
    auto share = [&](uint32_t k, bool bit) {  // bit = decide(g, g + k); give it to g + k
      const uint32_t src = g >= k ? g - k : g + b - k;  // lane holding decide(src, g)
      const uint32_t in = (uint32_t)__shfl((int)bit, (int)(gbase + (src & (G - 1))), 64);
      if (valid && k <= half) {
        P |= (uint64_t)bit << partner(k);
        P |= (uint64_t)in << src;
      }
    };
    for (uint32_t k = 1; k <= bmax / 2; k += 2) {  // two partners per step: independent chains
      const uint32_t j0 = partner(min(k, b)), j1 = partner(min(k + 1, b));
      const float s0 = shflf(sq, gbase + (j0 & (G - 1))), s1 = shflf(sq, gbase + (j1 & (G - 1)));
      bool h0 = false, h1 = false;
      if (valid && k <= half) {
        float d0, d1;
        dot2_reg_lds<D>(x, lds + (gbase + j0) * ST, lds + (gbase + j1) * ST, d0, d1);
        h0 = decide(dc, d0, sq * s0);
        h1 = k + 1 <= half && decide(dc, d1, sq * s1);
      }
      share(k, h0);
      share(k + 1, h1);
    }
  }
#ifdef KLSH_MERGE_PROF
  sp2 = WPROF_CLK();
#endif

  // 2. the walk.  Per position lane: row id, slot, member count / list ends (loaded only by waves
  //    with a matching pair: three random 4-B reads per row, as much traffic as the row itself),
  //    the row's sqrt-norm, the row (x), dirty = rewritten by a merge.
  uint32_t size = b;
  uint32_t nmerged = 0;
  bool dirty = false;
  const uint64_t matched = __ballot(valid && P != 0ull);
  if (matched) {
    uint32_t rid = g, cnt = 0u, hd = 0u, tl = 0u;
    // metadata only for the runs with a matching pair: ~1 % of the rows merge per iteration, and
    // three random 4-B reads cost a line each (as much traffic as the row itself)
    if (valid && (matched & gmask) != 0ull) {
      cnt = r.cnt[slot];
      hd = r.head[slot];
      tl = r.tail[slot];
    }
    uint32_t i = 1;  // group-uniform
    while (true) {
      const uint64_t below = g ? (~0ull >> (64u - g)) : 0ull;
      const bool hit = g >= i && g < size && (P & below) != 0ull;
      const uint64_t m = __ballot(hit) & gmask;
      if (__ballot(m != 0ull) == 0ull) break;  // every group of the wave is done
      const bool active = m != 0ull;
      uint32_t j = 0, last = 0;
      if (active) {
        i = (uint32_t)__builtin_ctzll(m >> gbase);
        j = (uint32_t)__builtin_ctzll((__ballot(g < i && ((P >> i) & 1ull)) & gmask) >> gbase);
        last = size - 1;
      }
      // the rows at positions i (current), j (candidate), last (moves to i)
      const uint32_t li = gbase + (i & (G - 1)), lj = gbase + (j & (G - 1));
      const uint32_t ll = gbase + (last & (G - 1));
      const uint32_t ri = shfl32(rid, li), rj = shfl32(rid, lj);
      const uint32_t ci = shfl32(cnt, li), cj = shfl32(cnt, lj);
      const uint32_t hi_ = shfl32(hd, li), ti = shfl32(tl, li), hj = shfl32(hd, lj);
      const uint32_t m_rid = shfl32(rid, ll), m_slot = shfl32(slot, ll), m_cnt = shfl32(cnt, ll);
      const uint32_t m_hd = shfl32(hd, ll), m_tl = shfl32(tl, ll);
      const float m_sq = shflf(sq, ll);
      const uint64_t m_P = shfl64(P, ll);
      if (active) {
        // consensus (funcAB.cc:65), current row first, split over the group's lanes, in place
        const float fa = (float)(int)ci, fb = (float)(int)cj, fn = (float)(int)(ci + cj);
        const float* rowr = lds + (gbase + ri) * ST;
        float* rowc = lds + (gbase + rj) * ST;
        for (int k = (int)g; k < D; k += G) rowc[k] = consensus(rowr[k], fa, rowc[k], fb, fn);
        if (g == j) {
          r.nxt[ti] = hj;  // ids_current ++ ids_candidate (funcAB.cc:51-55)
          cnt = ci + cj;
          hd = hi_;
          dirty = true;
        }
        if (g == i) r.cnt[slot] = 0u;  // the current row is gone
        // swap-remove: the last position's row and state move to position i
        if (g == i && i != last) {
          rid = m_rid;
          slot = m_slot;
          cnt = m_cnt;
          hd = m_hd;
          tl = m_tl;
          sq = m_sq;
          P = m_P;
        }
        if (i != last) {
          const uint64_t bl = (P >> last) & 1ull;
          P = (P & ~((1ull << i) | (1ull << last))) | (bl << i);
        }
        --size;
        ++nmerged;
      }
      wave_lds_fence();
      const bool need = active && g >= i && g < size;
      // decisions of the positions still to be visited against the new row at j; both rows are
      // read from LDS 16 B at a time (the lane's own row is its row id's: no registers held
      // across the walk)
      const float* cr = lds + (gbase + rj) * ST;
      const float* xr = lds + (gbase + rid) * ST;
      float n4[4] = {0.0f, 0.0f, 0.0f, 0.0f}, d4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int k = 0; k < D; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(cr + k);
        const float4 u = *reinterpret_cast<const float4*>(xr + k);
        n4[0] = n4[0] + v.x * v.x;
        n4[1] = n4[1] + v.y * v.y;
        n4[2] = n4[2] + v.z * v.z;
        n4[3] = n4[3] + v.w * v.w;
        d4[0] = d4[0] + u.x * v.x;
        d4[1] = d4[1] + u.y * v.y;
        d4[2] = d4[2] + u.z * v.z;
        d4[3] = d4[3] + u.w * v.w;
      }
      uint32_t dn = 0u;
      if (need) {
        const float sc_a = __builtin_sqrtf((n4[0] + n4[1]) + (n4[2] + n4[3]));
        dn = dc.fast ? prescreen(dc, (d4[0] + d4[1]) + (d4[2] + d4[3]), sq * sc_a) : 2u;
      }
      if (__ballot(dn == 2u)) {  // rare: the reference's sequential chains settle the close calls
        float nn = 0.0f, dot = 0.0f;
#pragma unroll
        for (int k = 0; k < D; k += 4) {
          const float4 v = *reinterpret_cast<const float4*>(cr + k);
          const float4 u = *reinterpret_cast<const float4*>(xr + k);
          nn = nn + v.x * v.x;
          nn = nn + v.y * v.y;
          nn = nn + v.z * v.z;
          nn = nn + v.w * v.w;
          dot = dot + u.x * v.x;
          dot = dot + u.y * v.y;
          dot = dot + u.z * v.z;
          dot = dot + u.w * v.w;
        }
        if (dn == 2u) dn = decide(dc, dot, sq * __builtin_sqrtf(nn)) ? 1u : 0u;
      }
      const uint64_t dm = (__ballot(need && dn == 1u) & gmask) >> gbase;
      if (need) P = dn ? (P | (1ull << j)) : (P & ~(1ull << j));
      if (active && g == j) P = dm;  // the new row against the positions still to be visited
    }
    // write back: survivors in position order, kInvalid after; rewritten rows and metadata
    if (valid && size < b) slots[p + g] = g < size ? slot : kInvalid;
    if (valid && dirty) {  // a rewritten row sits at a position below every merge after it
      const float* src = lds + (gbase + rid) * ST;
      const size_t xo = (size_t)slot * r.dp;
      float nv = 0.0f;  // its exact sequential norm (distance.cc:33-34)
#pragma unroll
      for (int k = 0; k < D; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(src + k);
        nv = nv + v.x * v.x;
        nv = nv + v.y * v.y;
        nv = nv + v.z * v.z;
        nv = nv + v.w * v.w;
        store_row4(r, xo + k, v);
      }
      r.nrm[slot] = nv;
      r.cnt[slot] = cnt;
      r.head[slot] = hd;
    }
  }
#ifdef KLSH_MERGE_PROF
  sp3 = WPROF_CLK();
#endif
  if (dlist) append_slot(valid && dirty, slot, dlist, &ctr->n_delta);
  wave_lds_fence();
#ifdef KLSH_MERGE_PROF
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  if (lane == 0) {
    const int c = (int)__builtin_ctz(G) - 1;
    const uint64_t sp4 = WPROF_CLK();
    atomicAdd(&g_sprof[c][0], 1ull);
    atomicAdd(&g_sprof[c][1], sp1 - sp0);
    atomicAdd(&g_sprof[c][2], sp2 - sp1);
    atomicAdd(&g_sprof[c][3], sp3 - sp2);
    atomicAdd(&g_sprof[c][4], sp4 - sp3);
  }
#endif
  (void)nmerged;
}

// ------------------------------------------------- the fp16 screen of one batch -----
typedef _Float16 sh16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 sh16x2 __attribute__((ext_vector_type(2)));
typedef float pf16acc __attribute__((ext_vector_type(16)));
typedef float pf4acc __attribute__((ext_vector_type(4)));

// The fp16 screen of one batch: 64/G runs of class c (G = 2 << c lanes each, lane g = position g
// of its run, b = its run's length, x = its fp16 row).  True on the lanes of a run that some pair
// of which the screen cannot rule out (or that holds a row without a usable norm); false: the run
// cannot merge.  LDS (this wave's): lrow [64][D + 8] halves, linv / lsrow / lflag [64].
template <int D>
__device__ __forceinline__ bool screen_batch(int c, uint32_t b, const sh16x8 (&x)[D / 8],
                                             _Float16* lrow, float* linv, float* lsrow,
                                             uint32_t* lflag, float s_star, float m0, float a2) {
  constexpr int STH = D + 8;  // LDS row stride in halves (16-B pad)
  const uint32_t lane = __lane_id();
  const uint32_t G = 2u << c;
  const uint32_t g = lane & (G - 1);
  const bool valid = g < b;
  float ss = 0.0f;
#pragma unroll
  for (int q = 0; q < D / 8; ++q) {
    *reinterpret_cast<sh16x8*>(lrow + lane * STH + 8 * q) = valid ? x[q] : sh16x8{};
#pragma unroll
    for (int hi2 = 0; hi2 < 8; hi2 += 2) {
      const sh16x2 v = {x[q][hi2], x[q][hi2 + 1]};
      ss = __builtin_amdgcn_fdot2(v, v, ss, false);
    }
  }
  // a row without a usable norm (zero, tiny, fp16 overflow, NaN) cannot be screened: its run
  // goes to the exact merge
  const bool bad = valid && !(ss >= 0x1p-100f && ss <= 0x1p100f);
  const uint32_t lg = (uint32_t)__builtin_ctz(G);  // log2 G
  const float il = valid && !bad ? 1.0f / __builtin_sqrtf(ss) : 0.0f;
  linv[lane] = il;
  lsrow[lane] = s_star - (m0 + a2 * il);
  lflag[lane] = 0u;
  wave_lds_fence();
  if (bad) lflag[lane >> lg] = 1u;
  const uint64_t vmask = __ballot(valid && !bad);  // rows the Gram test reads
  // The Gram blocks of the batch's runs on the matrix cores (x~ . x~ exact products, f32 sums):
  // 32 x 32 tiles for runs of 17..64 rows (the upper-triangular tiles of each run), 16 x 16
  // diagonal tiles for shorter runs (4 per batch, runs never cross a 16-row block).  A pair
  // (R < C) of one run that the screen cannot rule out flags the run in LDS.  The tests are
  // branch-free over per-row terms loaded up front (a load inside each test's branch was a wait
  // on LDS per entry): a pair is ruled out when G/(|x~a||x~b|) < s* - (m0 + a2 (1/|x~a| +
  // 1/|x~b|)), evaluated as (G ir) ic < lsrow[R] - a2 ic — the margin's terms summed in another
  // order, a few ulps of s* against the margin's 1.5x headroom; pair validity is one per-lane
  // mask per tile, applied once to the tile's failures.
  auto test = [&](float sv, float ir, float sr, float ic, float kc) -> bool {
    return !(sv * ir * ic < sr - kc);  // NaN / inf: not ruled out
  };
  // bits (q & 3) + 8 (q >> 2) of w -> bit q (the tile rows of a lane, 32 x 32 layout)
  auto rows16 = [](uint32_t w) -> uint32_t {
    return (w & 0xFu) | ((w >> 4) & 0xF0u) | ((w >> 8) & 0xF00u) | ((w >> 12) & 0xF000u);
  };
  if constexpr (D < 32) {  // (not launched: screen_ok needs d >= 32) rule nothing out
    lflag[lane] = 1u;
  } else if (G >= 32u) {
    const uint32_t r32 = lane & 31u, k8 = 8u * (lane >> 5);
#pragma unroll 1
    for (int tt = 0; tt < 3; ++tt) {
      const uint32_t tr = tt == 2 ? 1u : 0u, tc = tt == 0 ? 0u : 1u;
      if (G == 32u && tt == 1) continue;  // two runs: their diagonal tiles only
      pf16acc acc;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
#pragma unroll
      for (int ks = 0; ks < D / 16; ++ks) {
        const sh16x8 fa = *reinterpret_cast<const sh16x8*>(lrow + (tr * 32u + r32) * STH + 16 * ks + k8);
        const sh16x8 fb = *reinterpret_cast<const sh16x8*>(lrow + (tc * 32u + r32) * STH + 16 * ks + k8);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc, 0, 0, 0);
      }
      const uint32_t C = tc * 32u + r32, hb = 4u * (lane >> 5);
      const float ic = linv[C], kc = a2 * ic;
      float4 irv[4], srv[4];  // rows tr*32 + 8j + hb + (0..3)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        irv[j] = *reinterpret_cast<const float4*>(linv + tr * 32u + 8u * (uint32_t)j + hb);
        srv[j] = *reinterpret_cast<const float4*>(lsrow + tr * 32u + 8u * (uint32_t)j + hb);
      }
      // the lane's pairs (one run per tested tile): rows the image carries, column too, and
      // R < C on a diagonal tile (local row (q&3) + 8(q>>2) + hb below r32)
      uint32_t pm = rows16((uint32_t)(vmask >> (tr * 32u + hb)));
      if (tr == tc) {
        const uint32_t lim = r32 > hb ? r32 - hb : 0u;
        pm &= rows16(lim >= 32u ? 0xFFFFFFFFu : ((1u << lim) - 1u));
      }
      if (!((vmask >> C) & 1ull)) pm = 0u;
      uint32_t fm = 0u;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float4 v = irv[q >> 2], u = srv[q >> 2];
        const float ir = (q & 3) == 0 ? v.x : (q & 3) == 1 ? v.y : (q & 3) == 2 ? v.z : v.w;
        const float sr = (q & 3) == 0 ? u.x : (q & 3) == 1 ? u.y : (q & 3) == 2 ? u.z : u.w;
        fm |= test(acc[q], ir, sr, ic, kc) ? (1u << q) : 0u;
      }
      if (fm & pm) lflag[C >> lg] = 1u;
    }
  } else {
    const uint32_t r16 = lane & 15u, k8 = 8u * (lane >> 4);
#pragma unroll 1
    for (int tb = 0; tb < 4; ++tb) {
      pf4acc acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int ks = 0; ks < D / 32; ++ks) {
        const sh16x8 f = *reinterpret_cast<const sh16x8*>(lrow + (16u * tb + r16) * STH + 32 * ks + k8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(f, f, acc, 0, 0, 0);
      }
      const uint32_t C = 16u * tb + r16, rb = 16u * tb + 4u * (lane >> 4);
      const float ic = linv[C], kc = a2 * ic;
      const float4 v = *reinterpret_cast<const float4*>(linv + rb);
      const float4 u = *reinterpret_cast<const float4*>(lsrow + rb);
      const float irq[4] = {v.x, v.y, v.z, v.w}, srq[4] = {u.x, u.y, u.z, u.w};
      bool fail = false;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t R = rb + (uint32_t)q;
        const bool pair = (R < C) & ((R >> lg) == (C >> lg)) & (((vmask >> R) & (vmask >> C) & 1ull) != 0ull);
        fail |= pair & test(acc[q], irq[q], srq[q], ic, kc);
      }
      if (fail) lflag[C >> lg] = 1u;
    }
  }
  wave_lds_fence();
  return lflag[lane >> lg] != 0u;
}

// ------------------------------------------------- all small-run classes in one launch -----
// Runs of 2..64 rows of every size class in ONE persistent launch: the batches of all classes
// (a batch = one wave's 64/G runs of class G; 64 runs of 2 for the pair class) are numbered in
// one space, most expensive class first, and wave w takes batches w, w + grid, ...  Compared
// with one kernel per class on three streams this removes the per-class launch chains and the
// idle tails of the small classes.  The next batch's list entry and slot are loaded while the
// current batch is merged.
template <int G>
__device__ __forceinline__ uint32_t batches_of(uint32_t n) {
  return (n + (64u / G) - 1) / (64u / G);
}

template <int D>
__device__ __forceinline__ void pair_batch(const uint2* __restrict__ list, uint32_t n, uint32_t bi,
                                           uint32_t* __restrict__ slots, const Decider& dc,
                                           const Rows& r, Counters* ctr, uint32_t* dlist) {
  const uint32_t k = bi * 64u + __lane_id();
  bool merged = false;
  uint32_t s0 = 0;
  if (k < n) {
    const uint2 e = list[k];
    s0 = slots[e.x];
    const uint32_t s1 = slots[e.x + 1];
    float x0[D], x1[D];
    load_row<D>(r.x + (size_t)s0 * r.dp, x0);
    load_row<D>(r.x + (size_t)s1 * r.dp, x1);
    float dot = 0.0f;
#pragma unroll
    for (int q = 0; q < D; ++q) dot = dot + x1[q] * x0[q];  // cosine(c[1], c[0]), in order
    // the norms, recomputed from the rows in registers (the cached chain, distance.cc:33-34)
    float n0 = 0.0f, n1 = 0.0f;
#pragma unroll
    for (int q = 0; q < D; ++q) {
      n0 = n0 + x0[q] * x0[q];
      n1 = n1 + x1[q] * x1[q];
    }
    if (decide(dc, dot, __builtin_sqrtf(n1) * __builtin_sqrtf(n0))) {
      merged = true;
      const uint32_t ca = r.cnt[s1], cb = r.cnt[s0];  // current = row 1, candidate = row 0
      const float fa = (float)(int)ca, fb = (float)(int)cb, fn = (float)(int)(ca + cb);
      float nn = 0.0f;
      const size_t xo = (size_t)s0 * r.dp;
#pragma unroll
      for (int q = 0; q < D; q += 4) {
        float4 v;
        v.x = consensus(x1[q], fa, x0[q], fb, fn);
        v.y = consensus(x1[q + 1], fa, x0[q + 1], fb, fn);
        v.z = consensus(x1[q + 2], fa, x0[q + 2], fb, fn);
        v.w = consensus(x1[q + 3], fa, x0[q + 3], fb, fn);
        nn = nn + v.x * v.x;
        nn = nn + v.y * v.y;
        nn = nn + v.z * v.z;
        nn = nn + v.w * v.w;
        store_row4(r, xo + q, v);
      }
      r.nrm[s0] = nn;
      link_members(r, s1, s0);  // ids_current ++ ids_candidate; cnt[s1] = 0
      slots[e.x + 1] = kInvalid;
    }
  }
  if (dlist) append_slot(merged, s0, dlist, &ctr->n_delta);
}

// One wave's share of the small-run batches: waves `wave`, `wave + nwaves`, ... of the batch
// space; lds = this wave's 64 * (D + 4) floats.
template <int D>
__device__ __forceinline__ void small_loop(const MergeView& w, uint32_t* __restrict__ slots,
                                           const Decider& dc, const Rows& r, Counters* ctr,
                                           float* lds, uint32_t wave, uint32_t nwaves) {
  constexpr int NC = kGroupClasses;
  uint32_t n[NC], nb[NC], start[NC + 1];
  // after the fp16 screen: only the runs it could not rule out (the others merge nothing)
  const CountLine* counts = w.screened ? w.rc->n_act : w.rc->n_cls;
  const uint2* const* lists = w.screened ? w.act : w.cls;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    n[c] = __hip_atomic_load(&counts[c].v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  nb[0] = (n[0] + 63u) / 64u;
  nb[1] = batches_of<4>(n[1]);
  nb[2] = batches_of<8>(n[2]);
  nb[3] = batches_of<16>(n[3]);
  nb[4] = batches_of<32>(n[4]);
  nb[5] = batches_of<64>(n[5]);
  // batch space: class 5 (64-row runs) first ... class 0 (pairs) last
  start[NC] = 0;
  {
    uint32_t a = 0;
#pragma unroll
    for (int c = NC - 1; c >= 0; --c) {
      start[c] = a;
      a += nb[c];
    }
    start[NC] = a;  // total
  }
  const uint32_t total = start[NC];
  const uint32_t lane = __lane_id();
  auto locate = [&](uint32_t t, int& c, uint32_t& bi) {
    c = 0;
#pragma unroll
    for (int q = NC - 1; q >= 0; --q)
      if (t >= start[q] && t < start[q] + nb[q]) c = q;
    bi = t - start[c];
  };
  // the lane's (run, position) in batch bi of class c: entry and slot
  auto fetch = [&](uint32_t t, uint2& e, uint32_t& slot) {
    e = make_uint2(0u, 0u);
    slot = 0u;
    if (t >= total) return;
    int c;
    uint32_t bi;
    locate(t, c, bi);
    if (c == 0) return;  // pairs load their own
    const uint32_t G = 2u << c, NG = 64u / G;
    const uint32_t k = bi * NG + lane / G, g = lane & (G - 1);
    if (k < n[c]) {
      e = lists[c][k];
      if (g < e.y) slot = slots[e.x + g];
    }
  };
  uint2 e;
  uint32_t slot;
  fetch(wave, e, slot);
  for (uint32_t t = wave; t < total; t += nwaves) {
    uint2 e_next;
    uint32_t slot_next;
    fetch(t + nwaves, e_next, slot_next);
    int c;
    uint32_t bi;
    locate(t, c, bi);
    switch (c) {  // wave-uniform
      case 0: pair_batch<D>(lists[0], n[0], bi, slots, dc, r, ctr, w.sink.dlist); break;
      case 1: merge_batch<4, D>(e.x, e.y, slot, slots, dc, r, lds, w.sink.dlist, ctr); break;
      case 2: merge_batch<8, D>(e.x, e.y, slot, slots, dc, r, lds, w.sink.dlist, ctr); break;
      case 3: merge_batch<16, D>(e.x, e.y, slot, slots, dc, r, lds, w.sink.dlist, ctr); break;
      case 4: merge_batch<32, D>(e.x, e.y, slot, slots, dc, r, lds, w.sink.dlist, ctr); break;
      default: merge_batch<64, D>(e.x, e.y, slot, slots, dc, r, lds, w.sink.dlist, ctr); break;
    }
    e = e_next;
    slot = slot_next;
  }
}


// ------------------------------------------------- the fp16 screen of the small runs -----
// Every run of 2..64 rows is first tested on the fp16 row image (Rows::xh, half the bytes of the
// f32 rows): a run can merge only if some pair (a, b) passes cosine >= s* (cluster.cc:66-69), and
//   |x~a.x~b / (|x~a| |x~b|) - fl(dot_ref / fl(sqrtf(nrm_a) sqrtf(nrm_b)))| <= m
// with m = m0 + a2 (1/|x~a| + 1/|x~b|): the fp16 rounding of both rows (2^-11 each, relative, plus
// 2^-25 absolute per element for subnormals), the screen's f32 sums, the reference's own sequential
// sums and the quotient's roundings, 1.5x headroom (screen_margins).  A run none of whose pairs
// reaches s* - m cannot merge: it is left as it is — the walk's result for it is "no change" — and
// only the others go on to k_merge_small (lists RunLists::act), which decides them exactly on the
// f32 rows.  A row whose image has no usable norm (zero, tiny, fp16 overflow, NaN) keeps its run.
//
// The screen is a gather of 64 fp16 rows per batch followed by little arithmetic (the Gram blocks
// on the matrix cores), so what bounds it is the bytes in flight: each wave keeps the rows of the
// next kAhead batches loading in registers while it screens one (and the slots and list entries
// of the batches after those), so a wave has up to kAhead * 8 KB of row loads outstanding instead
// of waiting for one batch at a time.  One wave per workgroup; the batches of every class (64/G
// runs of G lanes, lane g = position g) in one persistent space, most expensive class first;
// passed runs collect in LDS per class and go out 32+ at a time (one atomic per flush).
// (lookahead 1 / 3 and 3 waves per EU measured the same as 2 / 2)
constexpr int kScreenAhead = 2;  // batches whose rows are in flight while one is screened

template <int D>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_small_screen(MergeView w, const uint32_t* __restrict__ slots,
                                                     Rows r, float s_star, float m0, float a2,
                                                     KTime kt) {
  constexpr int NC = kGroupClasses, STH = D + 8;  // LDS row stride in halves (16-B pad)
  constexpr int NR = kScreenAhead + 1;            // row buffers: the screened batch + the ones ahead
  constexpr uint32_t kBuf = 256;                  // passed runs kept in LDS before a flush
  __shared__ __attribute__((aligned(16))) _Float16 lrow[64 * STH];
  __shared__ __attribute__((aligned(16))) float linv[64];
  __shared__ __attribute__((aligned(16))) float lsrow[64];  // s* - (m0 + a2 / |x~|): the row's part
  __shared__ uint32_t lflag[64];  // per run of the batch: some pair not ruled out
  __shared__ uint2 buf[kBuf];     // passed runs (start, length | class << 16)
  __shared__ uint32_t fcnt[NC], fbase[NC];
  kt_begin(kt, KC_SCREEN);
  const uint32_t lane = __lane_id();
  if (blockIdx.x == 0 && lane == 0) w.rc->screened.v = 1u;
  uint32_t n[NC], nb[NC], start[NC + 1];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    // (scalar: every batch index and class below is wave-uniform, so list pointers stay in SGPRs
    // and no vector load of a pointer makes the wave wait for its outstanding row loads)
    n[c] = __builtin_amdgcn_readfirstlane(
        __hip_atomic_load(&w.rc->n_cls[c].v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const uint32_t per = 32u >> c;  // runs per batch: 64 / G, G = 2 << c
    nb[c] = (n[c] + per - 1u) / per;
  }
  {
    uint32_t a = 0;
#pragma unroll
    for (int c = NC - 1; c >= 0; --c) {
      start[c] = a;
      a += nb[c];
    }
    start[NC] = a;
  }
  const uint32_t total = start[NC], stride = gridDim.x;
  uint32_t nbuf = 0, brows = 0;  // (wave-uniform)
  // this wave's passed runs to the global lists: per class, one add and the entries
  auto flush = [&]() {
    if (lane < (uint32_t)NC) fcnt[lane] = 0u;
    wave_lds_fence();
    for (uint32_t i = lane; i < nbuf; i += 64) atomicAdd(&fcnt[buf[i].y >> 16], 1u);
    wave_lds_fence();
    if (lane < (uint32_t)NC) {
      const uint32_t c = fcnt[lane];
      fbase[lane] = c ? atomicAdd(&w.rc->n_act[lane].v, c) : 0u;
      fcnt[lane] = 0u;
    }
    if (lane == 0 && brows) atomicAdd(&w.rc->n_act_rows.v, brows);
    wave_lds_fence();
    for (uint32_t i = lane; i < nbuf; i += 64) {
      const uint2 e = buf[i];
      const uint32_t c = e.y >> 16;
      const uint32_t at = fbase[c] + atomicAdd(&fcnt[c], 1u);
      w.act[c][at] = make_uint2(e.x, e.y & 0xFFFFu);
    }
    wave_lds_fence();
    nbuf = brows = 0u;
  };
  const uint64_t below = lanes_below(lane);
  auto class_of = [&](uint32_t t) -> int {  // (wave-uniform: t is)
    int c = 0;
#pragma unroll
    for (int q = NC - 1; q >= 0; --q)
      if (t >= start[q] && t < start[q] + nb[q]) c = q;
    return __builtin_amdgcn_readfirstlane(c);
  };
  auto list_of = [&](int c) -> const uint2* {
    return c == 0 ? w.cls[0] : c == 1 ? w.cls[1] : c == 2 ? w.cls[2] : c == 3 ? w.cls[3]
         : c == 4 ? w.cls[4] : w.cls[5];
  };
  // Every load below is unconditional (a lane with nothing to load reads a valid dummy address),
  // so the loads of the batches ahead are never waited for early: the compiler counts them.
  // the lane's run entry in batch t ((0, 0) past the end)
  auto entry_of = [&](uint32_t t) -> uint2 {
    const int c = class_of(t);
    const uint32_t G = 2u << c, NG = 64u / G;
    const uint32_t k = (t - start[c]) * NG + lane / G;
    const bool ok = t < total && k < n[c];
    const uint2 e = list_of(c)[ok ? k : 0u];  // (every list holds >= 64 entries)
    return ok ? e : make_uint2(0u, 0u);
  };
  auto slot_of = [&](uint32_t t, const uint2& e) -> uint32_t {
    const uint32_t g = lane & ((2u << class_of(t)) - 1u);
    return slots[g < e.y ? e.x + g : e.x];
  };
  auto load_rows = [&](uint32_t slot, sh16x8 (&x)[D / 8]) {
    const uint16_t* src = r.xh + (size_t)slot * r.dp;
#pragma unroll
    for (int q = 0; q < D / 8; ++q) x[q] = *reinterpret_cast<const sh16x8*>(src + 8 * q);
  };
  // one batch: rows x (arrived), entry e
  auto screen = [&](uint32_t t, const uint2& e, const sh16x8 (&x)[D / 8]) {
    const int c = class_of(t);
    const uint32_t G = 2u << c;
    const uint32_t g = lane & (G - 1);
    const uint32_t b = e.y;
    const bool grp = screen_batch<D>(c, b, x, lrow, linv, lsrow, lflag, s_star, m0, a2);
    const bool leader = g == 0u && b >= 2u && grp;
    const uint64_t lead = __ballot(leader);
    if (lead) {
      if (nbuf + 64u > kBuf) flush();  // (rare: the buffer holds a wave's passed runs)
      if (leader)
        buf[nbuf + (uint32_t)__popcll(lead & below)] = make_uint2(e.x, b | ((uint32_t)c << 16));
      uint32_t rsum = leader ? b : 0u;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) rsum += (uint32_t)__shfl_xor((int)rsum, o, 64);
      nbuf += (uint32_t)__popcll(lead);
      brows += rsum;
    }
    wave_lds_fence();  // the rows of this batch are read before the next batch overwrites them
  };
  // The pipeline (batches t0, t0 + stride, ...): batch j is screened while the rows of j+1 ..
  // j+kAhead, the slot of j+kAhead+1 and the entries of j+kAhead+1, j+kAhead+2 are in flight.
  // Row buffers rotate through NR register arrays (the loop is unrolled NR times so every index
  // is static).
  sh16x8 xb[NR][D / 8];
  uint2 eb[NR];  // entries of the batches whose rows are (to be) in xb (same index)
  const uint32_t t0 = blockIdx.x;
  {
    uint2 e0[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) e0[k] = entry_of(t0 + (uint32_t)k * stride);
#pragma unroll
    for (int k = 0; k < NR - 1; ++k) {
      eb[k] = e0[k];
      load_rows(slot_of(t0 + (uint32_t)k * stride, e0[k]), xb[k]);
    }
    eb[NR - 1] = e0[NR - 1];
  }
  uint32_t s_next = slot_of(t0 + (uint32_t)(NR - 1) * stride, eb[NR - 1]);
  uint2 e_next = entry_of(t0 + (uint32_t)NR * stride);
  // Issue order matters: the slot and entry loads go out BEFORE the row loads, so that waiting
  // for them next step (vmcnt counts in issue order) leaves the rows in flight.
  auto step = [&](uint32_t t, int cur) {  // cur: the buffer of batch t
    const int nxt = (cur + NR - 1) % NR;  // the buffer of batch t + kAhead * stride
    const uint32_t ta = t + (uint32_t)NR * stride;
    const uint32_t s_rows = s_next;       // slot of batch t + kAhead (arrived a step ago)
    s_next = slot_of(ta, e_next);
    const uint2 e_after = entry_of(ta + stride);
    load_rows(s_rows, xb[nxt]);
    const uint2 e_cur = eb[cur];
    eb[cur] = e_next;  // batch t + NR * stride's rows go to this buffer next time round
    e_next = e_after;
    screen(t, e_cur, xb[cur]);
  };
  // (whole rounds of NR steps: a batch past the end screens nothing, and a branch-free body
  // keeps the compiler's count of the loads in flight exact across the loop)
  for (uint32_t t = t0; t < total; t += (uint32_t)NR * stride) {
#pragma unroll
    for (int k = 0; k < NR; ++k) step(__builtin_amdgcn_readfirstlane(t + (uint32_t)k * stride), k);
  }
  if (nbuf) flush();
  kt_end(kt, KC_SCREEN);
}

template <int D>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_merge_small(
    MergeView w, uint32_t* __restrict__ slots,
                                                    Decider dc, Rows r, Counters* ctr) {
  __shared__ __attribute__((aligned(16))) float lds[64 * (D + 4)];
  kt_begin(w.kt, KC_SMALL);
  small_loop<D>(w, slots, dc, r, ctr, lds, blockIdx.x, gridDim.x);
  kt_end(w.kt, KC_SMALL);
}

}  // namespace klsh
