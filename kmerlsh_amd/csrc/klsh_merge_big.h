// Runs of 65..896 rows at d = 8, 16, 32, 64, one workgroup per run over a position-space decision
// matrix in LDS.  Kernels: k_merge_big (one size class per launch) and k_merge_tail (every class
// of a small iteration in one launch: small_loop, big_runs and huge_runs).
#pragma once

#include "klsh_merge_common.h"
#include "klsh_merge_gram.h"
#include "klsh_merge_huge.h"
#include "klsh_merge_small.h"

namespace klsh {

// ------------------------------------------------------------------- runs of 65..896 rows -----
// One workgroup per run.  The run's metadata and its decision matrix live in LDS, the rows too
// when they fit (ROWS_LDS; otherwise they are read from memory, L2-resident, and staged one
// 64-row column block at a time for the decision phase).  The matrix is kept in POSITION space:
// P[y] bit q = decide(row y, row at position q), so the walk's "first j < i" is a
// find-first-set over W words, and positions that find nothing are skipped in bulk.

// The walk of one 65..896-row run over its position-space decision matrix P (k_merge_big*),
// shared by the whole workgroup: every step finds the first position q >= i whose row matches a
// position below q (positions that find nothing change nothing), does the reference's merge
// there, and recomputes the decisions of the rows still to be visited against the new row —
// spread over all NT lanes (the new row's norm on one lane meanwhile).  Rows are read from
// rowsL (LDS, stride ST) if given, else from memory; the new row is kept in LDS (cbuf).
template <int RB, int NT, bool ROWS_LDS, int D = 0>
__device__ __forceinline__ void big_walk(uint32_t p, uint32_t b, uint64_t* P, uint32_t* slot,
                                         float* nrm, uint32_t* cnt, uint32_t* hd, uint32_t* tl,
                                         uint32_t* pos2row, float* sq, float* rowsL, int ST,
                                         float* cbuf, uint32_t* wbuf, const Rows& r,
                                         const Decider& dc, uint32_t* slots, uint32_t* dlist,
                                         Counters* ctr) {
  constexpr int W = RB / 64, NW = NT / 64, KP = (RB + NT - 1) / NT;
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const int d = r.d, dp = r.dp;
  auto rowp = [&](uint32_t a) -> const float* {
    return ROWS_LDS ? rowsL + a * ST : r.x + (size_t)slot[a] * dp;
  };
  uint32_t i = 1, size = b, par = 0;
  [[maybe_unused]] uint64_t wp[6] = {0, 0, 0, 0, 0, 0}, c0 = 0, c1 = 0;
  while (true) {
    // 1. the next position that merges
    c0 = WPROF_CLK();
    uint32_t q = size;
    for (uint32_t q0 = i; q0 < size; q0 += NT) {
      ++wp[5];
      const uint32_t qq = q0 + t;
      bool hit = false;
      if (qq < size) {
        const uint64_t* Py = P + pos2row[qq] * W;
#pragma unroll
        for (int k = 0; k < W; ++k) {
          const uint32_t lo = (uint32_t)k * 64u;
          if (lo < qq) {
            const uint64_t wk = Py[k];
            hit |= (qq - lo >= 64u ? wk : (wk & ((1ull << (qq - lo)) - 1ull))) != 0ull;
          }
        }
      }
      const uint64_t m = __ballot(hit);
      if (lane == 0)
        wbuf[par * NW + wv] = m ? q0 + wv * 64u + (uint32_t)(__ffsll((unsigned long long)m) - 1)
                                : 0xFFFFFFFFu;
      lds_barrier();
      uint32_t best = 0xFFFFFFFFu;
#pragma unroll
      for (int w = 0; w < NW; ++w) best = min(best, wbuf[par * NW + w]);
      par ^= 1u;
      if (best != 0xFFFFFFFFu) {  // block-uniform
        q = best;
        break;
      }
    }
    c1 = WPROF_CLK();
    wp[0] += c1 - c0;
    c0 = c1;
    if (q >= size) break;
    ++wp[4];
    i = q;
    // 2. its first matching position j < i (every wave computes it)
    const uint32_t rr = pos2row[i];
    uint64_t word = 0ull;
    if (lane < (uint32_t)W) {
      word = P[rr * W + lane];
      const uint32_t lo = lane * 64u;
      if (lo >= i) word = 0ull;
      else if (i - lo < 64u) word &= (1ull << (i - lo)) - 1ull;
    }
    const uint64_t nz = __ballot(word != 0ull);
    const uint32_t wd = (uint32_t)(__ffsll((unsigned long long)nz) - 1);
    const uint64_t wbits = shfl64(word, wd);
    const uint32_t j = wd * 64u + (uint32_t)(__ffsll((unsigned long long)wbits) - 1);
    const uint32_t c = pos2row[j];
    const uint32_t ca = cnt[rr], cb = cnt[c];
    const uint32_t hr = hd[rr], tr = tl[rr], hc = hd[c];
    const uint32_t moved_row = pos2row[size - 1];
    lds_barrier();  // all reads of the old state are done
    // 3. consensus (funcAB.cc:65), current row first; member links and the swap-remove
    const float fa = (float)(int)ca, fb = (float)(int)cb, fn = (float)(int)(ca + cb);
    float* xc = r.x + (size_t)slot[c] * dp;
    const float* xr = rowp(rr);
    float* lc = ROWS_LDS ? rowsL + c * ST : cbuf;  // the new row c, in LDS
    for (int k = (int)t; k < d; k += NT) {
      const float v = consensus(xr[k], fa, ROWS_LDS ? lc[k] : xc[k], fb, fn);
      lc[k] = v;
      if (!ROWS_LDS) store_row1(r, (size_t)slot[c] * dp + k, v);  // LDS rows go out at the end
    }
    if (t == 0) {
      r.nxt[tr] = hc;  // ids_current ++ ids_candidate (funcAB.cc:51-55)
      hd[c] = hr;
      cnt[c] = ca + cb;
      cnt[rr] = 0u;
      pos2row[i] = moved_row;
    }
    if (ROWS_LDS) lds_barrier();
    else __syncthreads();  // the new row in memory is visible to the workgroup
    --size;
    const uint32_t moved = size;  // old position of the row now at i
    c1 = WPROF_CLK();
    wp[1] += c1 - c0;
    c0 = c1;
    // 4. dot products of the rows still to be visited with row c; row c's norm
    float dots[KP];
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) {
      const uint32_t qq = i + t + (uint32_t)kp * NT;
      dots[kp] = qq < size ? dot_seq<D>(rowp(pos2row[qq]), lc, d) : 0.0f;
    }
    if (t == NT - 1) {
      const float nn = dot_seq<D>(lc, lc, d);  // distance.cc:33-34
      nrm[c] = nn;
      sq[c] = __builtin_sqrtf(nn);
    }
    lds_barrier();
    c1 = WPROF_CLK();
    wp[2] += c1 - c0;
    c0 = c1;
    // 5. position-space bits: the moved row's bit goes to position i, bit j is re-decided
    const float sc = sq[c];
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) {
      const uint32_t qq = i + t + (uint32_t)kp * NT;
      if (qq < size) {
        const uint32_t y = pos2row[qq];
        uint64_t* Py = P + y * W;
        const bool bm = (Py[moved / 64] >> (moved & 63u)) & 1ull;
        Py[moved / 64] &= ~(1ull << (moved & 63u));
        Py[i / 64] = bm ? (Py[i / 64] | (1ull << (i & 63u))) : (Py[i / 64] & ~(1ull << (i & 63u)));
        const bool dn = decide(dc, dots[kp], sq[y] * sc);
        Py[j / 64] = dn ? (Py[j / 64] | (1ull << (j & 63u))) : (Py[j / 64] & ~(1ull << (j & 63u)));
      }
    }
    lds_barrier();
    c1 = WPROF_CLK();
    wp[3] += c1 - c0;
  }
#ifdef KLSH_MERGE_PROF
  if (t == 0) {
    const int cls = RB <= 128 ? 0 : RB <= 384 ? 1 : 2;
    for (int k = 0; k < 6; ++k) atomicAdd(&g_wprof[cls][k], (unsigned long long)wp[k]);
  }
#endif
  // write back: survivors in position order, kInvalid after; rewritten rows; metadata
  for (uint32_t q = t; q < b; q += NT) slots[p + q] = q < size ? slot[pos2row[q]] : kInvalid;
  if (ROWS_LDS) {  // a survivor was rewritten iff its count rose (the global count is still old)
    const uint32_t c4 = (uint32_t)dp / 4;
    for (uint32_t idx = t; idx < size * c4; idx += NT) {
      const uint32_t q = idx / c4, k = (idx % c4) * 4;
      const uint32_t y = pos2row[q];
      if (r.cnt[slot[y]] != cnt[y])
        store_row4(r, (size_t)slot[y] * dp + k, *reinterpret_cast<const float4*>(rowsL + y * ST + k));
    }
    __syncthreads();
  }
  for (uint32_t q0 = 0; q0 < size; q0 += NT) {  // uniform trip count (ballot inside)
    const uint32_t q = q0 + t;
    bool rewritten = false;
    if (q < size) {
      const uint32_t y = pos2row[q];
      rewritten = r.cnt[slot[y]] != cnt[y];  // every merge into a row raises its count
      r.nrm[slot[y]] = nrm[y];
      r.cnt[slot[y]] = cnt[y];
      r.head[slot[y]] = hd[y];
    }
    if (dlist) append_slot(rewritten, q < size ? slot[pos2row[q]] : 0u, dlist, &ctr->n_delta);
  }
}

// The same walk for runs whose rows sit in LDS at a register width (D = 8..64), built around ONE
// workgroup barrier per merge step (big_walk needs four):
//  * positions are owned statically — lane t holds positions t, t + NT, ... — with their rows in
//    registers (a row at a position >= i never changes; only the row moved into position i by the
//    swap-remove is reloaded, by its one owner);
//  * the owner of a position updates its P row after a merge and tests it at once, so the next
//    merge (its position, first matching position j, and both row ids) is a wave ballot + one
//    64-bit word per wave in LDS, read by every wave after the barrier;
//  * every wave computes the merge itself (consensus into a wave-private copy of the new row, the
//    member links by one lane) and applies the step's writes to the shared state (pos2row, counts,
//    list heads, the new row) at the START of the next step: every wave writes the same values,
//    each before its own reads, so no wave can see a half-written step and no second barrier is
//    needed;
//  * the decisions against the new row come from short chains (four interleaved partial sums of
//    its norm and of each dot product, |error| <= 2 * 64 * 2^-24 |a||b| each — far inside
//    kGramMargin), settled by the same certified pre-screen as the Gram tiles; only pairs within
//    the margin of the threshold run the reference's sequential chains.  The new row's exact norm
//    (distance.cc:33-34) is needed by nobody during the walk — rows at positions below i are never
//    tested again — so it is computed once per rewritten row at the write-back.
template <int RB, int NT, int D>
__device__ __forceinline__ void big_walk_reg(uint32_t p, uint32_t b, uint64_t* P, uint32_t* slot,
                                             float* nrm, uint32_t* cnt, const uint32_t* cnt0,
                                             uint32_t* hd, uint32_t* tl,
                                             uint32_t* pos2row, float* sq, float* rowsL,
                                             float* cwall, uint64_t* wbuf, const Rows& r,
                                             const Decider& dc, uint32_t* slots, uint32_t* dlist,
                                             Counters* ctr) {
  constexpr int W = RB / 64, NW = NT / 64, KP = (RB + NT - 1) / NT, ST = D + 4;
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  constexpr uint64_t kNone64 = ~0ull;
  static_assert(RB <= 1024, "positions are packed in 10 bits");
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  float* cw = cwall + wv * 64;  // this wave's copy of the newest row
  float xr[KP][D];              // the rows at my positions t + kp * NT
  uint32_t yr[KP];              // their row ids
  float sqy[KP];                // their sqrtf(norm)
#pragma unroll
  for (int kp = 0; kp < KP; ++kp) {
    const uint32_t q = t + (uint32_t)kp * NT;
    yr[kp] = q;
    sqy[kp] = 0.0f;
    if (q < b) {
      load_row<D>(rowsL + q * ST, xr[kp]);
      sqy[kp] = sq[q];
    }
  }
  // the first position below q that row y (words w) matches, or kNone
  auto first_below = [&](const uint64_t (&w)[W], uint32_t q) -> uint32_t {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const uint32_t lo = (uint32_t)k * 64u;
      if (lo < q) {
        uint64_t m = w[k];
        if (q - lo < 64u) m &= (1ull << (q - lo)) - 1ull;
        if (m) return lo + (uint32_t)__builtin_ctzll(m);
      }
    }
    return kNone;
  };
  // a hit: (position << 20 | its first match << 10 | its row) << 32 | the matching row
  auto pack = [](uint32_t q, uint32_t j, uint32_t y, uint32_t c) -> uint64_t {
    return ((uint64_t)((q << 20) | (j << 10) | y) << 32) | c;
  };
  // the wave's first hit (lowest position: kp-major, then lane order) -> wbuf[par][wv]
  auto publish = [&](uint32_t par, const uint64_t (&hit)[KP]) {
    uint64_t best = kNone64;
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) {
      const uint64_t m = __ballot(hit[kp] != kNone64);
      if (m && best == kNone64) best = shfl64(hit[kp], (uint32_t)__builtin_ctzll(m));
    }
    if (lane == 0) wbuf[par * NW + wv] = best;
  };
  uint32_t size = b, par = 0;
  [[maybe_unused]] const uint64_t wt0 = MPROF_T();
  {
    uint64_t hit[KP];
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) {
      const uint32_t q = t + (uint32_t)kp * NT;
      hit[kp] = kNone64;
      if (q >= 1 && q < b) {
        uint64_t w[W];
#pragma unroll
        for (int k = 0; k < W; ++k) w[k] = P[q * W + k];
        const uint32_t j = first_below(w, q);
        if (j != kNone) hit[kp] = pack(q, j, q, j);  // positions are the rows before any merge
      }
    }
    publish(par, hit);
  }
  lds_barrier();
  // the previous step's writes, applied by every wave at the start of the next step
  bool have = false;
  uint32_t ip = 0, mp = 0, cp = 0, rp = 0, cntp = 0, hdp = 0;
  float cvp = 0.0f;
  [[maybe_unused]] uint64_t steps = 0, wp[6] = {0, 0, 0, 0, 0, 0}, ck = WPROF_CLK(), ck1 = 0;
  while (true) {
    uint64_t best = kNone64;
#pragma unroll
    for (int w = 0; w < NW; ++w) best = min(best, wbuf[par * NW + w]);
    par ^= 1u;
    if (have) {
      if (lane == 0) {
        pos2row[ip] = mp;
        cnt[cp] = cntp;
        cnt[rp] = 0u;
        hd[cp] = hdp;
      }
      if (lane < (uint32_t)D) rowsL[cp * ST + lane] = cvp;
      wave_lds_fence();
    }
    if (best == kNone64) break;
    ++steps;
    const uint32_t hi = (uint32_t)(best >> 32);
    const uint32_t i = hi >> 20, j = (hi >> 10) & 1023u, rr = hi & 1023u, c = (uint32_t)best;
    const uint32_t moved = pos2row[size - 1];
    const uint32_t ca = cnt[rr], cb = cnt[c], hr = hd[rr], tr = tl[rr], hc = hd[c];
#ifdef KLSH_MERGE_PROF
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    ck1 = WPROF_CLK(); wp[0] += ck1 - ck; ck = ck1;
#endif
    // consensus (funcAB.cc:65), current row first, into this wave's copy of the new row c
    const float fa = (float)(int)ca, fb = (float)(int)cb, fn = (float)(int)(ca + cb);
    float cv = 0.0f;
    if (lane < (uint32_t)D) {
      cv = consensus(rowsL[rr * ST + lane], fa, rowsL[c * ST + lane], fb, fn);
      cw[lane] = cv;
    }
    if (t == 0) r.nxt[tr] = hc;  // ids_current ++ ids_candidate (funcAB.cc:51-55)
    wave_lds_fence();
    --size;  // swap-remove: the row at the old last position (size) moves to position i
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) {
      if (t + (uint32_t)kp * NT == i && i < size) {
        yr[kp] = moved;
        load_row<D>(rowsL + moved * ST, xr[kp]);
        sqy[kp] = sq[moved];
      }
    }
    float cvec[D];
    load_row<D>(cw, cvec);
#ifdef KLSH_MERGE_PROF
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    ck1 = WPROF_CLK(); wp[1] += ck1 - ck; ck = ck1;
#endif
    // short chains: four interleaved partial sums (a screen, not the reference's order)
    float n4[4] = {0.0f, 0.0f, 0.0f, 0.0f}, d4[KP][4];
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) d4[kp][0] = d4[kp][1] = d4[kp][2] = d4[kp][3] = 0.0f;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      n4[k & 3] = n4[k & 3] + cvec[k] * cvec[k];
#pragma unroll
      for (int kp = 0; kp < KP; ++kp) d4[kp][k & 3] = d4[kp][k & 3] + xr[kp][k] * cvec[k];
    }
    const float sc_a = __builtin_sqrtf((n4[0] + n4[1]) + (n4[2] + n4[3]));
    uint32_t dn[KP];
    bool amb = false;
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) {
      const uint32_t q = t + (uint32_t)kp * NT;
      dn[kp] = 0u;
      if (q >= i && q < size) {
        const float dot_a = (d4[kp][0] + d4[kp][1]) + (d4[kp][2] + d4[kp][3]);
        dn[kp] = dc.fast ? prescreen(dc, dot_a, sqy[kp] * sc_a) : 2u;
        amb = amb || dn[kp] == 2u;
      }
    }
    if (__ballot(amb)) {  // rare: the reference's sequential chains settle the close calls
      float nn = 0.0f;
#pragma unroll
      for (int k = 0; k < D; ++k) nn = nn + cvec[k] * cvec[k];
      const float sc = __builtin_sqrtf(nn);
#pragma unroll
      for (int kp = 0; kp < KP; ++kp) {
        if (dn[kp] == 2u) {
          float dot = 0.0f;
#pragma unroll
          for (int k = 0; k < D; ++k) dot = dot + xr[kp][k] * cvec[k];
          dn[kp] = decide(dc, dot, sqy[kp] * sc) ? 1u : 0u;
        }
      }
    }
#ifdef KLSH_MERGE_PROF
    asm volatile("s_nop 0" ::"v"(dn[0]) : "memory");
    ck1 = WPROF_CLK(); wp[2] += ck1 - ck; ck = ck1;
#endif
    uint64_t hit[KP];
#pragma unroll
    for (int kp = 0; kp < KP; ++kp) {
      const uint32_t q = t + (uint32_t)kp * NT;
      hit[kp] = kNone64;
      if (q >= i && q < size) {
        const uint32_t y = yr[kp];
        uint64_t w[W];
#pragma unroll
        for (int k = 0; k < W; ++k) w[k] = P[y * W + k];
        // position-space bits: the moved row's bit goes to position i, bit j is re-decided
        const bool bm = (w[size >> 6] >> (size & 63u)) & 1ull;
#pragma unroll
        for (int k = 0; k < W; ++k) {
          uint64_t v = w[k];
          if ((uint32_t)k == (size >> 6)) v &= ~(1ull << (size & 63u));
          if ((uint32_t)k == (i >> 6)) v = bm ? (v | (1ull << (i & 63u))) : (v & ~(1ull << (i & 63u)));
          if ((uint32_t)k == (j >> 6))
            v = dn[kp] ? (v | (1ull << (j & 63u))) : (v & ~(1ull << (j & 63u)));
          if (v != w[k]) P[y * W + k] = v;
          w[k] = v;
        }
        const uint32_t jj = first_below(w, q);
        // the row at position jj as of this step (position i now holds the moved row)
        if (jj != kNone) hit[kp] = pack(q, jj, y, jj == i ? moved : pos2row[jj]);
      }
    }
    publish(par, hit);
    have = true;
    ip = i;
    mp = moved;
    cp = c;
    rp = rr;
    cntp = ca + cb;
    hdp = hr;
    cvp = cv;
#ifdef KLSH_MERGE_PROF
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    ck1 = WPROF_CLK(); wp[3] += ck1 - ck; ck = ck1;
#endif
    lds_barrier();
#ifdef KLSH_MERGE_PROF
    ck1 = WPROF_CLK(); wp[5] += ck1 - ck; ck = ck1;
#endif
  }
#ifdef KLSH_MERGE_PROF
  if (t == 0) {
    const int cls = RB <= 128 ? 0 : RB <= 192 ? 1 : 2;
    atomicAdd(&g_wprof[cls][4], (unsigned long long)steps);
    for (int k = 0; k < 4; ++k) atomicAdd(&g_wprof[cls][k], (unsigned long long)wp[k]);
    atomicAdd(&g_wprof[cls][5], (unsigned long long)wp[5]);
    MPROF_ADD(RB <= 128 ? 0 : RB <= 192 ? 1 : RB <= 384 ? 2 : 3, 10, MPROF_T() - wt0);
  }
#endif
  __syncthreads();
  if (size == b) return;  // (block-uniform) no merge: the run, its rows and metadata are as loaded
  // write back: survivors in position order, kInvalid after; rewritten rows; metadata
  for (uint32_t q = t; q < b; q += NT) slots[p + q] = q < size ? slot[pos2row[q]] : kInvalid;
  {  // a survivor was rewritten iff its count rose
    constexpr uint32_t c4 = (uint32_t)D / 4;
    for (uint32_t idx = t; idx < size * c4; idx += NT) {
      const uint32_t q = idx / c4, k = (idx % c4) * 4;
      const uint32_t y = pos2row[q];
      if (cnt0[y] != cnt[y])
        store_row4(r, (size_t)slot[y] * r.dp + k, *reinterpret_cast<const float4*>(rowsL + y * ST + k));
    }
  }
  for (uint32_t q0 = 0; q0 < size; q0 += NT) {  // uniform trip count (ballot inside)
    const uint32_t q = q0 + t;
    bool rewritten = false;
    if (q < size) {
      const uint32_t y = pos2row[q];
      // every merge into a row raises its count, and a row's head changes only through a merge
      // into it (SetConsensus, funcAB.cc:49-71: ids = ids_cur ++ ids_cand, so the candidate's
      // slot takes the merged-away row's head and the sum of both counts); swap-remove moves a
      // row's position, never its slot's data.  So "count unchanged" implies "head, norm and row
      // unchanged" and those slots need no write-back.
      rewritten = cnt0[y] != cnt[y];
      if (rewritten) {  // the exact sequential norm of the new row (distance.cc:33-34)
        float nv = 0.0f;
#pragma unroll
        for (int k = 0; k < D; ++k) nv = nv + rowsL[y * ST + k] * rowsL[y * ST + k];
        r.nrm[slot[y]] = nv;
        r.cnt[slot[y]] = cnt[y];
        r.head[slot[y]] = hd[y];
      }
    }
    if (dlist) append_slot(rewritten, q < size ? slot[pos2row[q]] : 0u, dlist, &ctr->n_delta);
  }
}

template <int D, int RB, bool ROWS_LDS>
struct BigLayout {
  static constexpr int ST = D + 4;
  static constexpr int W = RB / 64;
  static constexpr size_t rows = 0;
  static constexpr size_t P = rows + sizeof(float) * ST * (ROWS_LDS ? RB : 64);
  static constexpr size_t meta = P + sizeof(uint64_t) * RB * W;
  static constexpr size_t bytes = meta + sizeof(uint32_t) * RB * 8;
};

// The fp16 screen of one big run (k_merge_tail, option tail_big_screen): k_small_screen's certified
// test (screen_margins) over every pair of the run's image rows, 32 x 32 blocks on
// v_mfma_f32_32x32x16_f16.  Returns whether the run can merge at all (some pair not ruled out, or a
// row whose image has no usable norm); false: the walk would change nothing — no f32 row is read.
// slot[0, b): the run's slots (LDS); hrows: room for b x (D + 8) halves; linv: b floats.
template <int D, int NT>
__device__ __forceinline__ bool big_screen_pass(uint32_t b, const uint32_t* slot, const Rows& r,
                                                float s_star, float m0, float a2,
                                                _Float16* hrows, float* linv, uint32_t* flag) {
  constexpr int STH = D + 8, LPR = D / 8, NW = NT / 64;  // a lane loads 16 B = 8 halves
  constexpr uint32_t RPR = NT / LPR;                      // rows per round
  constexpr int KB = 4;
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  if (t == 0) *flag = 0u;
  {
    const uint32_t sub = (t % LPR) * 8u, rr = t / LPR;
    const uint32_t rounds = (b + RPR - 1u) / RPR;
    for (uint32_t g0 = 0; g0 < rounds; g0 += KB) {  // block-uniform
      sh16x8 v[KB];
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        const uint32_t a = min((g0 + (uint32_t)k) * RPR + rr, b - 1u);
        v[k] = *reinterpret_cast<const sh16x8*>(r.xh + (size_t)slot[a] * r.dp + sub);
      }
#pragma unroll
      for (int k = 0; k < KB; ++k) {  // (unconditional at the clamped index, as in big_runs)
        const uint32_t a = min((g0 + (uint32_t)k) * RPR + rr, b - 1u);
        *reinterpret_cast<sh16x8*>(hrows + a * STH + sub) = v[k];
      }
    }
  }
  lds_barrier();
  bool bad = false;
  for (uint32_t a = t; a < b; a += NT) {  // |x~|, as k_small_screen computes it
    float ss = 0.0f;
#pragma unroll
    for (int q = 0; q < D / 8; ++q) {
      const sh16x8 x = *reinterpret_cast<const sh16x8*>(hrows + a * STH + 8 * q);
#pragma unroll
      for (int h2 = 0; h2 < 8; h2 += 2) {
        const sh16x2 v = {x[h2], x[h2 + 1]};
        ss = __builtin_amdgcn_fdot2(v, v, ss, false);
      }
    }
    const bool bd = !(ss >= 0x1p-100f && ss <= 0x1p100f);
    bad = bad || bd;
    linv[a] = bd ? 0.0f : 1.0f / __builtin_sqrtf(ss);
  }
  if (bad) *flag = 1u;
  lds_barrier();
  if (*flag) return true;  // (block-uniform) a row the image cannot carry: the exact merge
  const uint32_t nb = (b + 31u) / 32u, r32 = lane & 31u, k8 = 8u * (lane >> 5);
  const uint32_t ntiles = nb * (nb + 1u) / 2u;
  bool fail = false;
  for (uint32_t ti = wv; ti < ntiles; ti += NW) {  // wave-uniform: blocks tr <= tc
    uint32_t tc = (uint32_t)((__builtin_sqrtf(8.0f * (float)ti + 1.0f) - 1.0f) * 0.5f);
    while (tc * (tc + 1u) / 2u > ti) --tc;
    while ((tc + 1u) * (tc + 2u) / 2u <= ti) ++tc;
    const uint32_t tr = ti - tc * (tc + 1u) / 2u;
    pf16acc acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    const uint32_t ra = min(tr * 32u + r32, b - 1u), ca = min(tc * 32u + r32, b - 1u);
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
      const sh16x8 fa = *reinterpret_cast<const sh16x8*>(hrows + ra * STH + 16 * ks + k8);
      const sh16x8 fb = *reinterpret_cast<const sh16x8*>(hrows + ca * STH + 16 * ks + k8);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc, 0, 0, 0);
    }
    const uint32_t C = tc * 32u + r32;
    const float ic = linv[ca];
    float4 irv[4];  // rows tr*32 + 8j + 4h + (0..3)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      irv[j] = *reinterpret_cast<const float4*>(linv + min(tr * 32u + 8u * (uint32_t)j + 4u * (lane >> 5), (b - 1u) & ~3u));
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const uint32_t R = tr * 32u + (uint32_t)(q & 3) + 8u * (uint32_t)(q >> 2) + 4u * (lane >> 5);
      const float4 v = irv[q >> 2];
      const float ir = (q & 3) == 0 ? v.x : (q & 3) == 1 ? v.y : (q & 3) == 2 ? v.z : v.w;
      const float qv = acc[q] * ir * ic;
      const float m = m0 + a2 * (ir + ic);
      fail = fail | ((R < C) & (C < b) & !(qv < s_star - m));  // NaN / inf: not ruled out
    }
  }
  if (fail) *flag = 1u;
  lds_barrier();
  return *flag != 0u;
}


// The runs li = first, first + stride, ... (< count) of list `list` (size class cls), one
// workgroup of NT lanes per run, with smem = BigLayout<D, RB, ROWS_LDS>::bytes of LDS.
// bs.on (k_merge_tail, d = 32 / 64 with the fp16 image): each run is screened first
// (big_screen_pass) and left alone when no pair of it can merge.
template <int D, int RB, int NT, bool ROWS_LDS>
__device__ __forceinline__ void big_runs(const uint2* __restrict__ list, int cls, uint32_t count,
                                         uint32_t first, uint32_t stride,
                                         uint32_t* __restrict__ slots, const Decider& dc,
                                         const Rows& r, Counters* ctr, uint32_t* dlist,
                                         unsigned char* smem, BigScreen bs = BigScreen{0u, 0.0f, 0.0f, 0.0f}) {
  using L = BigLayout<D, RB, ROWS_LDS>;
  constexpr int ST = L::ST, W = L::W, NW = NT / 64;
  float* rows = reinterpret_cast<float*>(smem + L::rows);  // rows, or one staged column block
  uint64_t* P = reinterpret_cast<uint64_t*>(smem + L::P);  // [row][W] position-space masks
  uint32_t* slot = reinterpret_cast<uint32_t*>(smem + L::meta);
  float* nrm = reinterpret_cast<float*>(slot + RB);
  uint32_t* cnt = slot + 2 * RB;
  uint32_t* hd = slot + 3 * RB;
  uint32_t* tl = slot + 4 * RB;
  uint32_t* pos2row = slot + 5 * RB;
  float* sq = reinterpret_cast<float*>(slot + 6 * RB);  // sqrtf(nrm), distance.cc:37
  uint32_t* cnt0 = slot + 7 * RB;                       // the counts as loaded (rewritten rows)
  __shared__ uint32_t wbuf[2 * NW];
  __shared__ __attribute__((aligned(16))) float cwall[NW * 64];  // big_walk_reg's new-row copies
  __shared__ uint64_t wbuf64[2 * NW];                              // big_walk_reg's published hits
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  auto row_ptr = [&](uint32_t a) -> const float* {
    return ROWS_LDS ? rows + a * ST : r.x + (size_t)slot[a] * r.dp;
  };

  for (uint32_t li = first; li < count; li += stride) {
    const uint2 e = list[li];
    const uint32_t p = e.x, b = e.y;
    const uint32_t nblk = (b + 63) / 64;
    [[maybe_unused]] const uint64_t pt0 = MPROF_T();
    if constexpr (!ROWS_LDS) {
      for (uint32_t a = t; a < b; a += NT) {
        const uint32_t s = slots[p + a];
        slot[a] = s;
        nrm[a] = r.nrm[s];
        sq[a] = __builtin_sqrtf(nrm[a]);
        cnt[a] = cnt0[a] = r.cnt[s];
        hd[a] = r.head[s];
        tl[a] = r.tail[s];
        pos2row[a] = a;
      }
    }
    for (uint32_t a = t; a < b * (uint32_t)W; a += NT) P[a] = 0ull;
    if constexpr (ROWS_LDS) {
      // Three memory latencies, every load of a round in flight at once (loads under a bounds
      // branch would each be waited for on the spot): the run's slots; then the metadata and
      // the rows by slot, d/4 lanes per row, a float4 each, KB rows per lane per round.
      constexpr int KA = (RB + NT - 1) / NT;
      uint32_t sl[KA], mc[KA], mh[KA], mt[KA];
#pragma unroll
      for (int ka = 0; ka < KA; ++ka) sl[ka] = slots[p + min(t + (uint32_t)ka * NT, b - 1u)];
      if constexpr (D == 32 || D == 64) {
        if (bs.on) {  // (uniform) the fp16 screen first: a run that cannot merge is left as it is
          __shared__ uint32_t sflag;
#pragma unroll
          for (int ka = 0; ka < KA; ++ka) {
            const uint32_t a = t + (uint32_t)ka * NT;
            if (a < b) slot[a] = sl[ka];
          }
          lds_barrier();
          if (!big_screen_pass<D, NT>(b, slot, r, bs.s_star, bs.m0, bs.a2,
                                      reinterpret_cast<_Float16*>(rows), sq, &sflag)) {
            __syncthreads();
            continue;
          }
        }
      }
#pragma unroll
      for (int ka = 0; ka < KA; ++ka) {
        mc[ka] = r.cnt[sl[ka]];
        mh[ka] = r.head[sl[ka]];
        mt[ka] = r.tail[sl[ka]];
      }
#pragma unroll
      for (int ka = 0; ka < KA; ++ka) {
        const uint32_t a = t + (uint32_t)ka * NT;
        if (a < b) {
          slot[a] = sl[ka];
          pos2row[a] = a;
        }
      }
      lds_barrier();  // slot[] (the metadata loads stay in flight)
      constexpr uint32_t LPR = (uint32_t)D / 4;  // lanes per row: a float4 each
      constexpr uint32_t RPR = NT / LPR;         // rows per workgroup round
      constexpr int KB = D >= 64 ? 8 : D >= 32 ? 4 : 2;
      static_assert(D % 4 == 0 && NT % LPR == 0, "whole rows per round");
      const uint32_t sub = (t % LPR) * 4u, rr = t / LPR;
      const uint32_t rounds = (b + RPR - 1u) / RPR;
      for (uint32_t g0 = 0; g0 < rounds; g0 += KB) {  // block-uniform
        float4 v[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          const uint32_t a = min((g0 + (uint32_t)k) * RPR + rr, b - 1u);
          v[k] = *reinterpret_cast<const float4*>(r.x + (size_t)slot[a] * r.dp + sub);
        }
        // (stores unconditional at the clamped index — a row past b rewrites row b - 1 with its own
        // value: a store under `a < b` lets the compiler sink its load into the branch, and the KB
        // loads become KB round trips.  A scheduling barrier between the two loops, to keep
        // k_merge_tail's register-tight schedule from pairing the rest, spilled: not used)
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          const uint32_t a = min((g0 + (uint32_t)k) * RPR + rr, b - 1u);
          *reinterpret_cast<float4*>(rows + a * ST + sub) = v[k];
        }
      }
#pragma unroll
      for (int ka = 0; ka < KA; ++ka) {
        const uint32_t a = t + (uint32_t)ka * NT;
        if (a < b) {
          cnt[a] = cnt0[a] = mc[ka];
          hd[a] = mh[ka];
          tl[a] = mt[ka];
        }
      }
      lds_barrier();
#ifdef KLSH_MERGE_PROF
      if (t == 0) MPROF_ADD(cls, 8, MPROF_T() - pt0);
#endif
      // norms recomputed from the rows in LDS (the cached chain, distance.cc:33-34: same bits)
      // instead of a random 4-B read each
      for (uint32_t a = t; a < b; a += NT) {
        float n = 0.0f;
#pragma unroll
        for (int k = 0; k < D; k += 4) {
          const float4 v = *reinterpret_cast<const float4*>(rows + a * ST + k);
          n = n + v.x * v.x;
          n = n + v.y * v.y;
          n = n + v.z * v.z;
          n = n + v.w * v.w;
        }
        nrm[a] = n;
        sq[a] = __builtin_sqrtf(n);
      }
    }
    __syncthreads();
#ifdef KLSH_MERGE_PROF
    if (t == 0) MPROF_ADD(cls, 9, MPROF_T() - pt0);
#endif

    // decisions in 64x64 tiles (row block R, column block C <= R): lanes = rows of R with the
    // row in registers, columns walked in order (LDS broadcast); the wave's ballot at column c
    // is P[c]'s word R, the lane's own bits form P[a]'s word C.
    auto tile = [&](uint32_t R, uint32_t C, const float* colrows) {
      const uint32_t a = R * 64u + lane;
      float xa[D];
      if (a < b) {
        load_row<D>(row_ptr(a), xa);
      } else {
#pragma unroll
        for (int k = 0; k < D; ++k) xa[k] = 0.0f;
      }
      const float sa = a < b ? sq[a] : 0.0f;
      uint64_t own = 0ull;
      const uint32_t c0 = C * 64u, c1 = min(b, c0 + 64u);
      for (uint32_t c = c0; c < c1; c += 2) {
        const uint32_t cb = (c + 1 < c1) ? c + 1 : c;
        float d0, d1;
        dot2_reg_lds<D>(xa, colrows + (c - c0) * ST, colrows + (cb - c0) * ST, d0, d1);
        const bool h0 = a < b && c < a && decide(dc, d0, sa * sq[c]);
        const bool h1 = a < b && c + 1 < c1 && c + 1 < a && decide(dc, d1, sa * sq[cb]);
        const uint64_t m0 = __ballot(h0), m1 = __ballot(h1);
        if (lane == 0) {
          if (m0) atomicOr((unsigned long long*)&P[c * W + R], (unsigned long long)m0);
          if (m1) atomicOr((unsigned long long*)&P[cb * W + R], (unsigned long long)m1);
        }
        own |= (h0 ? 1ull : 0ull) << (c - c0);
        if (c + 1 < c1) own |= (h1 ? 1ull : 0ull) << (c + 1 - c0);
      }
      if (a < b && own) atomicOr((unsigned long long*)&P[a * W + C], (unsigned long long)own);
    };
    const bool gram = kGramTiles && D % 16 == 0 && dc.fast;  // uniform
    if constexpr (ROWS_LDS) {
      const uint32_t ntiles = nblk * (nblk + 1) / 2;
      for (uint32_t ti = wv; ti < ntiles; ti += NW) {
        uint32_t R = 0;
        while ((R + 1) * (R + 2) / 2 <= ti) ++R;
        const uint32_t C = ti - R * (R + 1) / 2;
        if constexpr (D % 16 == 0) {
          if (gram) {
            auto rl = [&](uint32_t a) -> const float* { return rows + a * ST; };
            gram_tile<D>(R, C, b, rl, rl, sq, dc, P, W);
            continue;
          }
        }
        tile(R, C, rows + C * 64u * ST);
      }
    } else if (gram) {
      if constexpr (D % 16 == 0) {
        auto rm = [&](uint32_t a) -> const float* { return r.x + (size_t)slot[a] * r.dp; };
        const uint32_t ntiles = nblk * (nblk + 1) / 2;
        for (uint32_t ti = wv; ti < ntiles; ti += NW) {
          uint32_t R = 0;
          while ((R + 1) * (R + 2) / 2 <= ti) ++R;
          const uint32_t C = ti - R * (R + 1) / 2;
          gram_tile<D>(R, C, b, rm, rm, sq, dc, P, W);
        }
      }
    } else {
      for (uint32_t C = 0; C < nblk; ++C) {
        for (uint32_t q = t; q < 64u * (uint32_t)(D / 4); q += NT) {
          const uint32_t a = C * 64u + q / (D / 4), k = (q % (D / 4)) * 4;
          if (a < b)
            *reinterpret_cast<float4*>(rows + (a - C * 64u) * ST + k) =
                *reinterpret_cast<const float4*>(r.x + (size_t)slot[a] * r.dp + k);
        }
        __syncthreads();
        for (uint32_t R = C + wv; R < nblk; R += NW) tile(R, C, rows);
        __syncthreads();
      }
    }
    __syncthreads();
    [[maybe_unused]] const uint64_t pt1 = MPROF_T();
    if constexpr (ROWS_LDS && D > 0 && D <= 64) {
      big_walk_reg<RB, NT, D>(p, b, P, slot, nrm, cnt, cnt0, hd, tl, pos2row, sq, rows, cwall,
                              wbuf64, r, dc, slots, dlist, ctr);
    } else {
      big_walk<RB, NT, ROWS_LDS, D>(p, b, P, slot, nrm, cnt, hd, tl, pos2row, sq,
                                 ROWS_LDS ? rows : nullptr, ST, rows, wbuf, r, dc, slots, dlist,
                                 ctr);
    }
    __syncthreads();
#ifdef KLSH_MERGE_PROF
    if (t == 0) {
      const uint64_t pt2 = MPROF_T();
      uint32_t live = 0;
      for (uint32_t q = 0; q < b; ++q) live += slots[p + q] != kInvalid ? 1u : 0u;
      MPROF_ADD(cls, 0, 1);
      MPROF_ADD(cls, 1, b);
      MPROF_ADD(cls, 2, b - live);
      MPROF_ADD(cls, 3, pt1 - pt0);
      MPROF_ADD(cls, 4, pt2 - pt1);
      MPROF_MAX(cls, 5, pt2 - pt0);
      MPROF_MAX(cls, 6, b);
    }
#endif
  }
}

// One size class of 65..896-row runs (w.big[cls]).  w.huge_fold (385..896 class only): the
// workgroups also walk the >896-row runs afterwards (huge_runs with NT lanes), so no k_merge_huge
// is launched — the engine sets it after iterations without such runs, where a launch of its own
// would have been empty.
template <int D, int RB, int NT, bool ROWS_LDS>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(RB <= 192 ? 2 : 1))) void k_merge_big(
    MergeView w, int cls, uint32_t* __restrict__ slots, Decider dc, Rows r, Counters* ctr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  kt_begin(w.kt, KC_BIG128 + cls);
  const uint32_t count =
      __hip_atomic_load(&w.rc->n_big[cls].v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  big_runs<D, RB, NT, ROWS_LDS>(w.big[cls], cls, count, blockIdx.x, gridDim.x, slots, dc, r, ctr,
                                w.sink.dlist, smem);
  if constexpr (RB == kBigRows[kBigClasses - 1]) {
    if (w.huge_fold) {
      __syncthreads();  // (the LDS layouts overlap)
      const uint32_t nh =
          __hip_atomic_load(&w.rc->n_huge.v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      huge_runs<D, NT>(w.huge, nh, blockIdx.x, gridDim.x, slots, dc, r, w.sink, ctr, smem);
    }
  }
  kt_end(w.kt, KC_BIG128 + cls);
}

// Small iterations: every merge class in ONE launch on the main stream (no fork/join across
// streams, ≈35 us per iteration there): workgroups [0, nbig) take the 65..896-row runs (the
// longest class first), the others run four small-run waves each.
template <int D>
__global__ __launch_bounds__(256) void k_merge_tail(MergeView w, uint32_t* __restrict__ slots,
                                                    Decider dc, Rows r, Counters* ctr,
                                                    uint32_t nbig) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  kt_begin(w.kt, KC_TAIL);
  if (blockIdx.x < nbig) {
    uint32_t cnt[kBigClasses];
#pragma unroll
    for (int c = 0; c < kBigClasses; ++c)
      cnt[c] = __hip_atomic_load(&w.rc->n_big[c].v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t nh = __hip_atomic_load(&w.rc->n_huge.v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // one index space, longest runs first: > 896 (no k_merge_huge launch in these iterations),
    // 385..896, 193..384, 129..192, 65..128
    const uint32_t a4 = nh, a3 = a4 + cnt[3], a2 = a3 + cnt[2], a1 = a2 + cnt[1],
                   total = a1 + cnt[0];
    const BigScreen bs = w.bs;
    for (uint32_t li = blockIdx.x; li < total; li += nbig) {  // block-uniform
      if (li < a4)
        huge_runs<D, 256>(w.huge, li + 1, li, 1u << 30, slots, dc, r, w.sink, ctr, smem);
      else if (li < a3)
        big_runs<D, 896, 256, false>(w.big[3], 3, li - a4 + 1, li - a4, 1u << 30, slots, dc, r,
                                     ctr, w.sink.dlist, smem);
      else if (li < a2)
        big_runs<D, 384, 256, true>(w.big[2], 2, li - a3 + 1, li - a3, 1u << 30, slots, dc, r, ctr,
                                    w.sink.dlist, smem, bs);
      else if (li < a1)
        big_runs<D, 192, 256, true>(w.big[1], 1, li - a2 + 1, li - a2, 1u << 30, slots, dc, r, ctr,
                                    w.sink.dlist, smem, bs);
      else
        big_runs<D, 128, 256, true>(w.big[0], 0, li - a1 + 1, li - a1, 1u << 30, slots, dc, r, ctr,
                                    w.sink.dlist, smem, bs);
      __syncthreads();
    }
  } else {
    const uint32_t wv = threadIdx.x >> 6;
    float* lds = reinterpret_cast<float*>(smem) + wv * 64 * (D + 4);
    small_loop<D>(w, slots, dc, r, ctr, lds, (blockIdx.x - nbig) * 4u + wv, (gridDim.x - nbig) * 4u);
  }
  kt_end(w.kt, KC_TAIL);
}

}  // namespace klsh
