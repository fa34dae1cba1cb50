// Wide rows (d > 64, or a width without a register kernel), every run length: the G-lane groups
// with the rows staged through LDS in column chunks, and the 65..896-row walk with the rows in
// memory.  Kernels: k_merge_group_wide (runs of 2..64 rows), k_merge_big_wide (65..896, and
// huge_runs folded into its 896 class).
#pragma once

#include "klsh_merge_big.h"
#include "klsh_merge_common.h"
#include "klsh_merge_gram.h"
#include "klsh_merge_huge.h"

namespace klsh {

// ------------------------------------------------------------------ wide rows (any d) -----
// Rows that do not fit in registers (d > 64, or a width without a register kernel): the same
// G-lane group scheme, but the pairwise decisions are accumulated over 64-column chunks staged
// through LDS (each lane's chains continue across chunks, so every dot product keeps the
// reference's k order), and the walk's recomputations read the two rows from memory.
constexpr int kWideKC = 64;

// The exact group merges' chunk width (C5: 32 columns halve the staged tile to 9 KB per wave, so
// LDS no longer caps the waves per CU below what the registers allow)
constexpr int kWideXKC = 32;

// Columns [c0, c0 + kcp) of the 64 lanes' rows -> LDS rows (stride KC + 4), coalesced:
// KC/4 lanes per row, 256/KC rows per wave instruction.  kcp is a multiple of 4.
template <int KC = kWideKC>
__device__ __forceinline__ void stage_chunk(const float* __restrict__ X, int dp, uint32_t slot,
                                            bool valid, int c0, int kcp, float* tile) {
  constexpr int ST = KC + 4, LPR = KC / 4, RPI = 64 / LPR;
  const uint32_t lane = __lane_id();
  const uint32_t q = lane & (LPR - 1u), rsub = lane / LPR;
  const bool col_ok = (int)(4 * q) < kcp;
  // Loads and stores unconditional (a lane past its run reads its slot's row, valid memory — the
  // callers pass slot 0 there — and the column clamped to c0; both zeroed after the load): a
  // load under `ok && col_ok` was a branch per row with its shuffles waited in front of it, and
  // a store under `col_ok` lets the compiler sink the load into it.  Columns kcp .. KC of the
  // tile (a partial last chunk) get zeros; the readers use n <= kcp of them.
  uint32_t s[LPR];
  bool ok[LPR];
#pragma unroll
  for (int it = 0; it < LPR; ++it) {
    const uint32_t row = it * RPI + rsub;
    s[it] = shfl32(slot, row);
    const int vr = __shfl(valid ? 1 : 0, (int)row, 64);  // (every lane: a shuffle under col_ok
    ok[it] = col_ok && vr != 0;                           // reads inactive lanes as 0)
  }
  float4 v[LPR];
#pragma unroll
  for (int it = 0; it < LPR; ++it)
    v[it] = *reinterpret_cast<const float4*>(X + (size_t)s[it] * dp + c0 + (col_ok ? 4 * q : 0u));
#pragma unroll
  for (int it = 0; it < LPR; ++it) {
    if (!ok[it]) v[it] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    *reinterpret_cast<float4*>(tile + (it * RPI + rsub) * ST + 4 * q) = v[it];
  }
}

template <int N>
__device__ __forceinline__ float dot_acc_reg(float s, const float (&a)[N], const float* b) {
#pragma unroll
  for (int k = 0; k < N; k += 4) {
    const float4 v = *reinterpret_cast<const float4*>(b + k);
    s = s + a[k] * v.x;
    s = s + a[k + 1] * v.y;
    s = s + a[k + 2] * v.z;
    s = s + a[k + 3] * v.w;
  }
  return s;
}

// DG: d at compile time for the runs of G >= 8 rows (their pairwise decisions from one 64x64
// MFMA Gram tile, certified with the wide margin the caller's decider carries, exact chains only
// for the close calls), 0 = every pair by its exact chain.
template <int G, int DG = 0>
__device__ __forceinline__ void merge_batch_wide(uint32_t p, uint32_t b, uint32_t slot,
                                                 uint32_t* slots, const Decider& dc,
                                                 const Rows& r, float* tile, uint32_t* dlist,
                                                 Counters* ctr) {
  constexpr int ST = kWideKC + 4;
  constexpr int NK = G / 2;  // partners per lane: k = 1 .. b/2 <= G/2
  const uint32_t lane = threadIdx.x;
  const uint32_t g = lane & (G - 1);
  const uint32_t gbase = lane - g;
  const uint64_t gmask = (G == 64) ? ~0ull : (((1ull << (G & 63)) - 1ull) << gbase);
  const int d = r.d, dp = r.dp;
  const bool valid = g < b;
  float nrm = valid ? r.nrm[slot] : 0.0f;
  float sq = __builtin_sqrtf(nrm);  // distance.cc:37
  const float* myx = r.x + (size_t)slot * dp;
  const uint32_t bmax = wave_max(b);
  const uint32_t half = b / 2, kmax = bmax / 2;
  auto partner = [&](uint32_t k) {  // (g + k) mod b, for k <= b
    const uint32_t j = g + k;
    return j >= b ? j - b : j;
  };

  uint64_t full = 0ull;
  if constexpr (DG > 0 && G >= 8) {
    // 1'. the batch's decisions from one Gram tile on the matrix cores (bf16x3): the 64 lanes'
    //     rows against each other, accumulated over the same LDS-staged 64-column chunks, pairs
    //     across runs masked off afterwards; close calls by the exact chain (gram_decide)
    __shared__ uint64_t Pw[64];  // position masks
    __shared__ uint32_t sl[64];
    __shared__ float sqs[64];
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[m][n][i] = 0.0f;
    for (int c0 = 0; c0 < DG; c0 += kWideKC) {
      wave_lds_fence();  // the previous chunk's reads are done
      stage_chunk(r.x, dp, slot, valid, c0, kWideKC, tile);
      wave_lds_fence();
      auto rl = [&](uint32_t a) -> const float* { return tile + a * ST; };
      gram_acc<kWideKC>(0u, 0u, 64u, rl, rl, acc);
    }
    wave_lds_fence();
    Pw[lane] = 0ull;
    sl[lane] = slot;  // (a lane past its run holds a valid row: slot 0)
    sqs[lane] = valid ? sq : 1.0f;
    wave_lds_fence();
    auto rm = [&](uint32_t a) -> const float* { return r.x + (size_t)sl[a] * dp; };
    gram_decide<DG>(0u, 0u, 64u, acc, rm, rm, sqs, dc, Pw, 1, nullptr);
    __builtin_amdgcn_s_waitcnt(0x0070);  // (its atomics into LDS) vmcnt(0) lgkmcnt(0)
    wave_lds_fence();
    const uint64_t runbits = b >= 64u ? ~0ull : ((1ull << b) - 1ull);
    full = valid ? ((Pw[lane] >> gbase) & runbits & ~(1ull << g)) : 0ull;
    wave_lds_fence();
  } else {
  // 1. every pairwise dot product of the run, chunk by chunk (lane g vs positions g + k)
  constexpr int XKC = kWideXKC, XST = XKC + 4;
  float acc[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) acc[k] = 0.0f;
  for (int c0 = 0; c0 < d; c0 += XKC) {
    const int n = min(XKC, d - c0), kcp = min(XKC, dp - c0);
    wave_lds_fence();  // the previous chunk's reads are done
    stage_chunk<XKC>(r.x, dp, slot, valid, c0, kcp, tile);
    wave_lds_fence();
    const float* mine = tile + lane * XST;
    if (n == XKC) {
      float x[XKC];
      load_row<XKC>(mine, x);
#pragma unroll
      for (int k = 1; k <= NK; ++k)
        if ((uint32_t)k <= kmax && valid && (uint32_t)k <= half)
          acc[k - 1] = dot_acc_reg<XKC>(acc[k - 1], x, tile + (gbase + partner(k)) * XST);
    } else {
#pragma unroll
      for (int k = 1; k <= NK; ++k)
        if ((uint32_t)k <= kmax && valid && (uint32_t)k <= half)
          acc[k - 1] = dot_acc_mem(acc[k - 1], mine, tile + (gbase + partner(k)) * XST, n);
    }
  }
#pragma unroll
  for (int k = 1; k <= NK; ++k) {
    if ((uint32_t)k <= kmax) {  // wave-uniform
      const uint32_t j = partner(min((uint32_t)k, b));
      const float sj = shflf(sq, gbase + (j & (G - 1)));
      const bool bit = valid && (uint32_t)k <= half && decide(dc, acc[k - 1], sq * sj);
      const uint32_t src = g >= (uint32_t)k ? g - k : g + b - k;  // lane holding decide(src, g)
      const uint32_t in = (uint32_t)__shfl((int)bit, (int)(gbase + (src & (G - 1))), 64);
      if (valid && (uint32_t)k <= half) {
        full |= (uint64_t)bit << j;
        full |= (uint64_t)in << src;
      }
    }
  }
  }

  // member counts and list ends only for the runs with a matching pair (as merge_batch)
  const bool grp = (__ballot(valid && full != 0ull) & gmask) != 0ull;
  uint32_t cnt = 0u, hd = 0u, tl = 0u;
  if (valid && grp) {
    cnt = r.cnt[slot];
    hd = r.head[slot];
    tl = r.tail[slot];
  }

  // 2. the walk, replayed on the bits (as merge_batch); rows live in memory
  uint32_t rowid = g, mypos = g;
  bool alive = valid, dirty = false;
  uint32_t i = 1, size = b;
  while (true) {
    const uint64_t mybit = g < size ? (1ull << rowid) : 0ull;
    uint64_t incl = mybit;
#pragma unroll
    for (uint32_t o = 1; o < (uint32_t)G; o <<= 1) {
      const uint64_t y = shfl64(incl, lane >= o ? lane - o : lane);
      if (g >= o) incl |= y;
    }
    const uint64_t frow = shfl64(full, gbase + rowid);
    const bool hit = g >= i && g < size && (frow & (incl & ~mybit)) != 0ull;
    const uint64_t m = __ballot(hit) & gmask;
    if (__ballot(m != 0ull) == 0ull) break;
    if (m != 0ull) {
      i = (uint32_t)(__ffsll((unsigned long long)m) - 1) - gbase;
      const uint32_t rr = shfl32(rowid, gbase + i);
      const uint64_t fr = shfl64(frow, gbase + i);
      const uint64_t mj = __ballot(g < i && ((fr >> rowid) & 1ull)) & gmask;
      const uint32_t jpos = (uint32_t)(__ffsll((unsigned long long)mj) - 1) - gbase;
      const uint32_t c = shfl32(rowid, gbase + jpos);
      const uint32_t ca = shfl32(cnt, gbase + rr), cb = shfl32(cnt, gbase + c);
      const uint32_t hr = shfl32(hd, gbase + rr), tr = shfl32(tl, gbase + rr);
      const uint32_t hc = shfl32(hd, gbase + c);
      const uint32_t slot_r = shfl32(slot, gbase + rr), slot_c = shfl32(slot, gbase + c);
      const float fa = (float)(int)ca, fb = (float)(int)cb, fn = (float)(int)(ca + cb);
      const float* xr = r.x + (size_t)slot_r * dp;
      float* xc = r.x + (size_t)slot_c * dp;
      for (int k = (int)g; k < d; k += G)
        store_row1(r, (size_t)slot_c * dp + k, consensus(xr[k], fa, xc[k], fb, fn));
      lds_fence();  // the new row c is visible to the group's lanes
      if (g == rr) alive = false;
      if (g == 0) r.nxt[tr] = hc;  // ids_current ++ ids_candidate (funcAB.cc:51-55)
      const uint32_t last = shfl32(rowid, gbase + size - 1);  // swap-remove
      if (g == i) rowid = last;
      if (g == last) mypos = i;
      --size;
      // lane c: its exact sequential norm; rows still to be visited: their dot with row c
      const bool todo = alive && mypos >= i && mypos < size;
      float dot = 0.0f;
      if (g == c || todo) dot = dot_acc_mem(0.0f, myx, xc, d);
      if (g == c) {
        nrm = dot;
        sq = __builtin_sqrtf(dot);
        cnt = ca + cb;
        hd = hr;
        dirty = true;
      }
      const float sc = shflf(sq, gbase + c);
      if (todo) full = decide(dc, dot, sq * sc) ? (full | (1ull << c)) : (full & ~(1ull << c));
    }
  }

  // 3. write back
  const uint32_t pos_slot = shfl32(slot, gbase + rowid);
  if (valid && size < b) slots[p + g] = g < size ? pos_slot : kInvalid;
  if (valid && alive && dirty) {
    r.nrm[slot] = nrm;
    r.cnt[slot] = cnt;
    r.head[slot] = hd;
  }
  if (dlist) append_slot(valid && alive && dirty, slot, dlist, &ctr->n_delta);
  if (valid && !alive) r.cnt[slot] = 0u;
  lds_fence();
}

template <int G, int DG = 0>
__global__ __launch_bounds__(64) void k_merge_group_wide(const uint2* __restrict__ list,
                                                         const uint32_t* count_ptr,
                                                         uint32_t* __restrict__ slots, Decider dc,
                                                         Rows r, Counters* ctr, uint32_t* dlist,
                                                         KTime kt) {
  __shared__ __attribute__((aligned(16))) float tile[64 * ((DG > 0 && G >= 8 ? kWideKC : kWideXKC) + 4)];
  constexpr uint32_t NG = 64 / G;
  kt_begin(kt, KC_SMALL);
  const uint32_t n = __hip_atomic_load(count_ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t nb = (n + NG - 1) / NG;
  const uint32_t g = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  for (uint32_t bi = blockIdx.x; bi < nb; bi += gridDim.x) {
    const uint32_t k = bi * NG + grp;
    const uint2 e = k < n ? list[k] : make_uint2(0u, 0u);
    const uint32_t slot = g < e.y ? slots[e.x + g] : 0u;
    merge_batch_wide<G, DG>(e.x, e.y, slot, slots, dc, r, tile, dlist, ctr);
  }
  kt_end(kt, KC_SMALL);
}

// Runs of 65..896 rows with wide rows: one workgroup per run, the decision matrix in LDS in
// position space (as k_merge_big).  A 64x64 decision tile is one wave's job: its 64 rows'
// chains (one per lane, 64 columns each) run over KC-column chunks, the column block's chunk
// staged in the wave's own LDS region and read by broadcast.
template <int RB, int NT, int KC>
struct BigWideLayout {
  static constexpr int W = RB / 64;
  static constexpr int NW = NT / 64;
  static constexpr int STB = KC;  // unpadded: the tile is filled lane-linearly (and read by broadcast)
  static constexpr size_t tiles = 0;
  static constexpr size_t P = tiles + sizeof(float) * NW * 64 * STB;
  static constexpr size_t meta = P + sizeof(uint64_t) * RB * W;
  static constexpr size_t bytes = meta + sizeof(uint32_t) * RB * 8;
};

template <int RB, int NT, int KC>
__global__ __launch_bounds__(NT) void k_merge_big_wide(MergeView w, int cls,
                                                       uint32_t* __restrict__ slots, Decider dc,
                                                       Rows r, Counters* ctr) {
  using L = BigWideLayout<RB, NT, KC>;
  const uint2* __restrict__ list = w.big[cls];
  uint32_t* const dlist = w.sink.dlist;
  RunCounters* const rc = w.rc;
  const KTime kt = w.kt;
  kt_begin(kt, KC_BIG128 + cls);
  constexpr int W = L::W, NW = L::NW, STB = L::STB;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* P = reinterpret_cast<uint64_t*>(smem + L::P);
  uint32_t* slot = reinterpret_cast<uint32_t*>(smem + L::meta);
  float* nrm = reinterpret_cast<float*>(slot + RB);
  uint32_t* cnt = slot + 2 * RB;
  uint32_t* hd = slot + 3 * RB;
  uint32_t* tl = slot + 4 * RB;
  uint32_t* pos2row = slot + 5 * RB;
  float* sq = reinterpret_cast<float*>(slot + 6 * RB);
  __shared__ uint32_t wbuf[2 * NW];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  float* ctile = reinterpret_cast<float*>(smem + L::tiles) + wv * 64 * STB;  // this wave's
  const int d = r.d, dp = r.dp;
  const uint32_t count =
      __hip_atomic_load(&rc->n_big[cls].v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  auto row_ptr = [&](uint32_t a) -> const float* { return r.x + (size_t)slot[a] * dp; };

  for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
    const uint2 e = list[li];
    const uint32_t p = e.x, b = e.y;
    const uint32_t nblk = (b + 63) / 64;
    [[maybe_unused]] const uint64_t pt0 = MPROF_T();
    for (uint32_t a = t; a < b; a += NT) {
      const uint32_t s = slots[p + a];
      slot[a] = s;
      nrm[a] = r.nrm[s];
      sq[a] = __builtin_sqrtf(nrm[a]);
      cnt[a] = r.cnt[s];
      hd[a] = r.head[s];
      tl[a] = r.tail[s];
      pos2row[a] = a;
    }
    for (uint32_t a = t; a < b * (uint32_t)W; a += NT) P[a] = 0ull;
    __syncthreads();

    // decision tiles (R, C <= R), one per wave at a time
    const uint32_t ntiles = nblk * (nblk + 1) / 2;
    for (uint32_t ti = wv; ti < ntiles; ti += NW) {
      uint32_t R = 0;
      while ((R + 1) * (R + 2) / 2 <= ti) ++R;
      const uint32_t C = ti - R * (R + 1) / 2;
      const uint32_t a = R * 64u + lane;
      const bool va = a < b;
      const float* xa = row_ptr(va ? a : 0u);  // (a lane past the run reads row 0, unused)
      const uint32_t c0 = C * 64u, c1 = min(b, c0 + 64u);
      float acc[64];
#pragma unroll
      for (int c = 0; c < 64; ++c) acc[c] = 0.0f;
      for (int k0 = 0; k0 < d; k0 += KC) {
        const int n = min(KC, d - k0), kcp = min(KC, dp - k0);
        lds_fence();
        if (kcp == KC) {
          // a full chunk straight into LDS (global_load_lds, 16 B a lane: the tile is unpadded, so
          // instruction i fills floats [256 i, 256 i + 256) lane-linearly) — no registers, every
          // load in flight at once; rows past the run read row c0 (never read back)
          constexpr uint32_t PER = KC / 4;
#pragma unroll
          for (uint32_t i = 0; i < PER; ++i) {
            const uint32_t q = lane + 64u * i, row = q / PER, e4 = q % PER;
            const uint32_t sr = slot[c0 + row < c1 ? c0 + row : c0];
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(r.x + (size_t)sr * dp + k0 + 4 * e4),
                (__attribute__((address_space(3))) void*)(ctile + 256u * i), 16, 0, 0);
          }
          __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the tile has landed
        } else {
          for (uint32_t q = lane; q < 64u * (uint32_t)(kcp / 4); q += 64) {
            const uint32_t row = q / (uint32_t)(kcp / 4), e4 = q % (uint32_t)(kcp / 4);
            if (c0 + row < c1)
              *reinterpret_cast<float4*>(ctile + row * STB + 4 * e4) =
                  *reinterpret_cast<const float4*>(r.x + (size_t)slot[c0 + row] * dp + k0 + 4 * e4);
          }
        }
        lds_fence();
        if (n == KC) {
          float x[KC];
#pragma unroll
          for (int k = 0; k < KC; k += 4) {
            float4 v = *reinterpret_cast<const float4*>(xa + k0 + k);
            if (!va) v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            x[k] = v.x; x[k + 1] = v.y; x[k + 2] = v.z; x[k + 3] = v.w;
          }
#pragma unroll
          for (int c = 0; c < 64; ++c)
            if (c0 + c < c1) acc[c] = dot_acc_reg<KC>(acc[c], x, ctile + c * STB);
        } else {
#pragma unroll
          for (int c = 0; c < 64; ++c)
            if (c0 + c < c1 && va) {
              float s = acc[c];
              for (int k = 0; k < n; ++k) s = s + xa[k0 + k] * ctile[c * STB + k];
              acc[c] = s;
            }
        }
      }
      const float sa = va ? sq[a] : 0.0f;
      uint64_t own = 0ull;
#pragma unroll
      for (int c = 0; c < 64; ++c) {
        const uint32_t cc = c0 + c;
        if (cc < c1) {  // wave-uniform
          const bool h = va && cc < a && decide(dc, acc[c], sa * sq[cc]);
          const uint64_t m = __ballot(h);
          if (lane == 0 && m) atomicOr((unsigned long long*)&P[cc * W + R], (unsigned long long)m);
          own |= (h ? 1ull : 0ull) << c;
        }
      }
      if (va && own) atomicOr((unsigned long long*)&P[a * W + C], (unsigned long long)own);
    }
    __syncthreads();

    big_walk<RB, NT, false>(p, b, P, slot, nrm, cnt, hd, tl, pos2row, sq, nullptr, 0,
                     reinterpret_cast<float*>(smem + L::tiles), wbuf, r, dc, slots, dlist, ctr);
    __syncthreads();
  }
  if constexpr (RB == kBigRows[kBigClasses - 1]) {
    if (w.huge_fold) {  // the >896-row runs too (see k_merge_big)
      const uint32_t nh =
          __hip_atomic_load(&w.rc->n_huge.v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      huge_runs<0, NT>(w.huge, nh, blockIdx.x, gridDim.x, slots, dc, r, w.sink, ctr, smem);
    }
  }
  kt_end(kt, KC_BIG128 + cls);
}

}  // namespace klsh
