// The run listing, not a merge: runs of equal keys of any length, sorted into the per-class lists
// the merge kernels read.  Kernels: k_runs_count, k_runs_scan, k_runs_write, and k_tail_local (the
// small iterations' local bucket sort with the listing in the same launch).
#pragma once

#include "klsh_merge_common.h"

namespace klsh {

// Runs of equal keys, listed by size class, in three launches and no contended atomics:
//   k_runs_count  a tile of 4096 positions is read coalesced (position k*256 + t by thread t), its
//                 head flags become a 4096-bit bitmap (wave ballots, kept in global memory with the
//                 first head past the tile end), each head finds its run's end as the next set bit
//                 and its list (size class, big class, huge, oversize); per-list counts per tile
//   k_runs_scan   one workgroup per list: exclusive scan of its counts over the tiles, the total
//                 into the list's counter
//   k_runs_write  every head again from the stored bitmap, its entry at the tile's base + a rank
// (one global add per list per tile — the single-kernel version — serialised ~2300 adds per counter
// at C2 size, 80-100 us).  Entries within a list are in no particular order; every merge result is
// positional.
constexpr uint32_t kRunTile = 4096;
constexpr int kRunLists = kGroupClasses + kBigClasses + 2;  // small classes, big classes, huge, over
// + the head count (n_seg), rows in small runs, rows in each big class and in huge runs
constexpr int kRunRows = kRunLists + 2 + kBigClasses + 1;

__device__ __forceinline__ uint32_t* run_counter(RunCounters* rc, int l) {
  return l < kGroupClasses ? &rc->n_cls[l].v
         : l < kGroupClasses + kBigClasses ? &rc->n_big[l - kGroupClasses].v
         : l == kRunLists - 2 ? &rc->n_huge.v
         : l == kRunLists - 1 ? &rc->n_over.v
         : l == kRunLists ? &rc->n_seg.v
         : l == kRunLists + 1 ? &rc->n_small_rows.v
         : l < kRunLists + 2 + kBigClasses ? &rc->n_big_rows[l - kRunLists - 2].v
                                           : &rc->n_huge_rows.v;
}

// The list of a run of b rows (-1: one row).
__device__ __forceinline__ int run_class(uint32_t b, int bucket_thr) {
  // one row is in no list under any threshold: at bucket_thr = 0 the tile kernels listed every
  // such run as oversize (k_tail_local never did), a nested call on one row that draws nothing
  if (b < 2u) return -1;
  if (bucket_thr >= 0 && b > (uint32_t)bucket_thr) return kRunLists - 1;  // cluster.cc:286
  if (b > 64u) {
    if (b > (uint32_t)kBigRows[kBigClasses - 1]) return kRunLists - 2;
    int c = 0;
    while (b > (uint32_t)kBigRows[c]) ++c;
    return kGroupClasses + c;
  }
  return b >= 2 ? size_class(b) : -1;
}

// The entries of list l (0 <= l < kRunLists).  With a per-lane l this is a vector load from the
// kernel-argument block, and a store through it waits for that load: the run-listing kernels read
// the pointers once into an LDS table (run_list_table) instead of once per entry.
__device__ __forceinline__ uint2* run_list_ptr(const RunLists& w, int l) {
  uint2* p = l == kRunLists - 2 ? w.huge : w.over;
#pragma unroll
  for (int c = 0; c < kBigClasses; ++c) p = l == kGroupClasses + c ? w.big[c] : p;
#pragma unroll
  for (int c = 0; c < kGroupClasses; ++c) p = l == c ? w.cls[c] : p;
  return p;
}

// Threads 0 .. kRunLists-1 fill tab with the list pointers (visible after the next barrier),
// typed as global memory: a generic pointer read back from LDS would make every entry store a
// flat store, which the LDS waits that follow it also wait for.
using RunListPtr = __attribute__((address_space(1))) uint64_t*;
__device__ __forceinline__ void run_list_table(const RunLists& w, RunListPtr* tab) {
  const uint32_t t = threadIdx.x;
  RunListPtr p = (RunListPtr)(uint64_t*)run_list_ptr(w, (int)min(t, (uint32_t)kRunLists - 1u));
  if (t < (uint32_t)kRunLists) tab[t] = p;
}
// A (start, length) entry as one 64-bit store (uint2 layout: x in the low word).
__device__ __forceinline__ uint64_t run_entry(uint32_t start, uint32_t len) {
  return (uint64_t)len << 32 | start;
}

// What run counter `l` (kRunRows of them) receives for a run of b rows in list lr.
__device__ __forceinline__ uint32_t run_contrib(int l, int lr, uint32_t b) {
  if (l < kRunLists) return l == lr ? 1u : 0u;
  if (l == kRunLists) return 0u;  // heads: counted where the head is found
  if (l == kRunLists + 1) return (lr >= 0 && lr < kGroupClasses) ? b : 0u;
  if (l < kRunLists + 2 + kBigClasses) return lr == kGroupClasses + (l - kRunLists - 2) ? b : 0u;
  return lr == kRunLists - 2 ? b : 0u;
}

// Exclusive suffix minimum over the 256 threads of a workgroup: min of v over threads > t (~0u if
// none).  Every thread must call it.
__device__ __forceinline__ uint32_t block_excl_suffix_min_256(uint32_t v) {
  __shared__ uint32_t sm[256];
  const uint32_t t = threadIdx.x;
  sm[t] = v;
  __syncthreads();
  for (uint32_t o = 1; o < 256; o <<= 1) {  // inclusive suffix min, Hillis-Steele
    const uint32_t u = t + o < 256 ? sm[t + o] : ~0u;
    __syncthreads();
    sm[t] = min(sm[t], u);
    __syncthreads();
  }
  const uint32_t r = t + 1 < 256 ? sm[t + 1] : ~0u;
  __syncthreads();
  return r;
}

// The run starting at tile-local position q (a head of bitmap hb): its length and list (-1: one row).
__device__ __forceinline__ int run_list(const uint64_t* hb, uint32_t T0, uint32_t tail_end,
                                        uint32_t q, int bucket_thr, uint32_t& b) {
  uint32_t wi = q >> 6;
  uint64_t m = hb[wi] & ~((2ull << (q & 63u)) - 1ull);  // heads after q in its word
  while (!m && ++wi < kRunTile / 64) m = hb[wi];
  const uint32_t next = m ? T0 + wi * 64u + (uint32_t)__builtin_ctzll(m) : tail_end;
  b = next - (T0 + q);
  return run_class(b, bucket_thr);
}

// Per tile: the head bitmap, the first head (global position, ~0u = none) and the last head
// (tile-local, ~0u = none), and per-list counts of every run that starts in the tile EXCEPT its
// last one: that run's end is the first head of a later tile (tail_end), found by a suffix minimum
// over the tiles' first heads in the scan / write kernel — so no tile walks forward past its end
// (linear in n at any run length).
__global__ __launch_bounds__(256) void k_runs_count(const uint32_t* __restrict__ key, uint32_t lo,
                                                    uint32_t n, int bucket_thr, uint32_t ntiles,
                                                    uint64_t* __restrict__ hbits,
                                                    uint2* __restrict__ heads_fl,
                                                    uint32_t* __restrict__ counts, KTime kt,
                                                    const uint32_t* __restrict__ n_dev) {
  kt_begin(kt, KC_RUNS);
  if (n_dev) n = *n_dev;  // tiles past it find no heads and count nothing
  __shared__ uint64_t hb[kRunTile / 64];
  __shared__ uint32_t lcnt[kRunRows];
  __shared__ uint32_t s_last;
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const uint32_t T0 = blockIdx.x * kRunTile;
  if (t < (uint32_t)kRunRows) lcnt[t] = 0u;
  const uint32_t* kp = key + lo;
  uint32_t a[16], pv[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t i = T0 + (uint32_t)k * 256u + t;
    a[k] = i < n ? kp[i] : 0u;
    pv[k] = (i < n && i > 0) ? kp[i - 1] : 0u;
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t i = T0 + (uint32_t)k * 256u + t;
    const uint64_t m = __ballot(i < n && (i == 0 || a[k] != pv[k]));
    if (lane == 0) {
      hb[k * 4 + wv] = m;
      hbits[(size_t)blockIdx.x * (kRunTile / 64) + k * 4 + wv] = m;
    }
  }
  __syncthreads();
  if (wv == 0) {  // the tile's first and last heads (bitmap word `lane`)
    const uint64_t m = hb[lane];
    const uint64_t nz = __ballot(m != 0ull);
    uint32_t first = ~0u, last = ~0u;
    if (nz) {
      const uint32_t wf = (uint32_t)__builtin_ctzll(nz), wl = 63u - (uint32_t)__builtin_clzll(nz);
      first = T0 + wf * 64u + (uint32_t)__builtin_ctzll(hb[wf]);
      last = wl * 64u + 63u - (uint32_t)__builtin_clzll(hb[wl]);
    }
    if (lane == 0) {
      s_last = last;
      heads_fl[blockIdx.x] = make_uint2(first, last);
    }
  }
  __syncthreads();
  const uint32_t lastq = s_last;
  const uint64_t lt = lane ? (~0ull >> (64u - lane)) : 0ull;
  uint32_t heads = 0, small_rows = 0;
  uint32_t lrows[kBigClasses + 1] = {};  // rows per big class, then huge
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const uint32_t q = (uint32_t)k * 256u + t;
    int l = -1;
    if ((hb[q >> 6] >> (q & 63u)) & 1ull) {
      ++heads;
      if (q != lastq) {  // (the last run's list: the scan / write kernel)
        uint32_t b;
        l = run_list(hb, T0, 0u, q, bucket_thr, b);
        if (l >= 0 && l < kGroupClasses) small_rows += b;
#pragma unroll
        for (int c = 0; c <= kBigClasses; ++c)
          if (l == kGroupClasses + c) lrows[c] += b;
      }
    }
    // lanes with the same list: one LDS add by the lowest of them
    const uint32_t id = (uint32_t)(l + 1);  // 0 = no entry
    uint64_t match = ~0ull;
#pragma unroll
    for (int bit = 0; bit < 4; ++bit) {
      const uint64_t mb = __ballot((id >> bit) & 1u);
      match &= ((id >> bit) & 1u) ? mb : ~mb;
    }
    if (l >= 0 && (match & lt) == 0ull) atomicAdd(&lcnt[l], (uint32_t)__popcll(match));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    heads += __shfl_xor(heads, o, 64);
    small_rows += __shfl_xor(small_rows, o, 64);
#pragma unroll
    for (int c = 0; c <= kBigClasses; ++c) lrows[c] += __shfl_xor(lrows[c], o, 64);
  }
  if (lane == 0 && heads) atomicAdd(&lcnt[kRunLists], heads);
  if (lane == 0 && small_rows) atomicAdd(&lcnt[kRunLists + 1], small_rows);
#pragma unroll
  for (int c = 0; c <= kBigClasses; ++c)
    if (lane == 0 && lrows[c]) atomicAdd(&lcnt[kRunLists + 2 + c], lrows[c]);
  __syncthreads();
  if (t < (uint32_t)kRunRows) counts[(size_t)t * ntiles + blockIdx.x] = lcnt[t];
}

// The last run of tile j (tile-local head `last`, ~0u = none) ends at tail_end: its length.
__device__ __forceinline__ uint32_t last_run_len(uint32_t j, uint32_t last, uint32_t tail_end) {
  return last == ~0u ? 0u : tail_end - (j * kRunTile + last);
}

// Workgroup l: the tiles' last runs (their ends from a suffix minimum over the first heads; list
// 0's workgroup writes the tail ends) into counts[l], then counts[l][0..ntiles) -> exclusive prefix
// over the tiles; the total -> list l's counter.
__global__ __launch_bounds__(256) void k_runs_scan(uint32_t* __restrict__ counts, uint32_t ntiles,
                                                   uint32_t n, int bucket_thr,
                                                   const uint2* __restrict__ heads_fl,
                                                   uint32_t* __restrict__ tail_ends,
                                                   RunCounters* rc) {
  const int l = (int)blockIdx.x;
  uint32_t* row = counts + (size_t)l * ntiles;
  const uint32_t t = threadIdx.x;
  const uint32_t per = (ntiles + 255u) / 256u;
  const uint32_t a = min(ntiles, t * per), e = min(ntiles, a + per);
  // A thread's tiles are read CH at a time, every load of a chunk issued before any use (index
  // clamped into the chunk, no branch around a load): one round trip per chunk, not per tile —
  // this one-workgroup-per-list launch is a latency chain.
  constexpr uint32_t CH = 8;
  uint32_t fmin = ~0u;  // first head of this thread's tiles
  for (uint32_t i0 = a; i0 < e; i0 += CH) {
    uint32_t hx[CH];
#pragma unroll
    for (uint32_t c = 0; c < CH; ++c) hx[c] = heads_fl[min(i0 + c, e - 1u)].x;
#pragma unroll
    for (uint32_t c = 0; c < CH; ++c) fmin = min(fmin, hx[c]);  // (clamped repeats: harmless)
  }
  uint32_t after = block_excl_suffix_min_256(fmin);  // first head after this thread's tiles
  uint32_t acc = 0;
  for (uint32_t i1 = e; i1 > a;) {  // reverse: `after` is the first head after tile i
    const uint32_t i0 = i1 - a > CH ? i1 - CH : a;
    uint2 hf[CH];
    uint32_t rv[CH];
#pragma unroll
    for (uint32_t c = 0; c < CH; ++c) {
      const uint32_t j = min(i0 + c, i1 - 1u);
      hf[c] = heads_fl[j];
      rv[c] = row[j];
    }
#pragma unroll
    for (int c = (int)CH - 1; c >= 0; --c) {
      const uint32_t i = i0 + (uint32_t)c;
      if (i < i1) {
        const uint32_t te = min(after, n);
        if (l == 0) tail_ends[i] = te;
        const uint32_t b = last_run_len(i, hf[c].y, te);
        uint32_t v = rv[c];
        if (b) v += run_contrib(l, run_class(b, bucket_thr), b);
        row[i] = v;
        acc += v;
        after = min(after, hf[c].x);
      }
    }
    i1 = i0;
  }
  uint32_t total;
  uint32_t run = block_excl_scan_256(acc, &total);
  for (uint32_t i0 = a; i0 < e; i0 += CH) {
    uint32_t rv[CH];
#pragma unroll
    for (uint32_t c = 0; c < CH; ++c) rv[c] = row[min(i0 + c, e - 1u)];
#pragma unroll
    for (uint32_t c = 0; c < CH; ++c)
      if (i0 + c < e) {
        row[i0 + c] = run;
        run += rv[c];
      }
  }
  if (t == 0) *run_counter(rc, l) = total;
}

// SCAN (ntiles <= 256, every iteration below 2^20 positions): `counts` are the raw per-tile counts
// and each workgroup sums its own list bases (the tiles before it; thread t holds tile t, and adds
// tile t's last run once the suffix minimum of the first heads gives its end) — and workgroup 0
// the list totals — so k_runs_scan is not launched: one dependent launch less.
template <bool SCAN>
__global__ __launch_bounds__(256) void k_runs_write(uint32_t lo, uint32_t n, int bucket_thr,
                                                    uint32_t ntiles,
                                                    const uint64_t* __restrict__ hbits,
                                                    const uint2* __restrict__ heads_fl,
                                                    const uint32_t* __restrict__ tail_ends,
                                                    const uint32_t* __restrict__ counts,
                                                    MergeView w, const uint32_t* __restrict__ n_dev) {
  __shared__ uint64_t hb[kRunTile / 64];
  __shared__ uint32_t lbase[kRunLists], lfill[kRunLists];
  __shared__ uint32_t s_tail_end;
  __shared__ RunListPtr lptr[kRunLists];
  const uint32_t t = threadIdx.x;
  const uint32_t T0 = blockIdx.x * kRunTile;
  // (the header loads unconditional, index clamped: issued together, one round trip)
  uint32_t cb = 0u, te = 0u;
  if constexpr (!SCAN) {
    cb = counts[(size_t)min(t, (uint32_t)kRunLists - 1u) * ntiles + blockIdx.x];
    te = tail_ends[blockIdx.x];
  }
  const uint64_t hv = hbits[(size_t)blockIdx.x * (kRunTile / 64) + (t & (kRunTile / 64 - 1u))];
  run_list_table(w, lptr);
  if (t < kRunTile / 64) hb[t] = hv;
  if constexpr (SCAN) {
    if (n_dev) n = *n_dev;
    __shared__ uint32_t red[2][4][kRunRows];
    const uint32_t lane = t & 63u, wv = t >> 6;
    uint32_t cv[kRunRows];  // every load in flight before the reductions
#pragma unroll
    for (int l = 0; l < kRunRows; ++l) cv[l] = t < ntiles ? counts[(size_t)l * ntiles + t] : 0u;
    const uint2 hf = t < ntiles ? heads_fl[t] : make_uint2(~0u, ~0u);
    const uint32_t te = min(block_excl_suffix_min_256(hf.x), n);  // the end of tile t's last run
    if (t == blockIdx.x) s_tail_end = te;
    const uint32_t lb = t < ntiles ? last_run_len(t, hf.y, te) : 0u;
    const int lr = lb ? run_class(lb, bucket_thr) : -1;
#pragma unroll
    for (int l = 0; l < kRunRows; ++l) cv[l] += lb ? run_contrib(l, lr, lb) : 0u;
#pragma unroll
    for (int l = 0; l < kRunRows; ++l) {
      const uint32_t v = cv[l];
      uint32_t before = t < blockIdx.x ? v : 0u, all = v;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        before += __shfl_xor(before, o, 64);
        all += __shfl_xor(all, o, 64);
      }
      if (lane == 0) {
        red[0][wv][l] = before;
        red[1][wv][l] = all;
      }
    }
    __syncthreads();
    if (t < (uint32_t)kRunLists) {
      lbase[t] = red[0][0][t] + red[0][1][t] + red[0][2][t] + red[0][3][t];
      lfill[t] = 0u;
    }
    if (blockIdx.x == 0 && t < (uint32_t)kRunRows)
      *run_counter(w.rc, (int)t) = red[1][0][t] + red[1][1][t] + red[1][2][t] + red[1][3][t];
  } else {
    if (t < (uint32_t)kRunLists) {
      lbase[t] = cb;
      lfill[t] = 0u;
    }
    if (t == 0) s_tail_end = te;
  }
  __syncthreads();
  const uint32_t tail_end = s_tail_end;
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const uint32_t q = (uint32_t)k * 256u + t;
    if ((hb[q >> 6] >> (q & 63u)) & 1ull) {
      uint32_t b;
      const int l = run_list(hb, T0, tail_end, q, bucket_thr, b);
      if (l < 0) continue;
      const uint32_t at = lbase[l] + atomicAdd(&lfill[l], 1u);
      lptr[l][at] = run_entry(lo + T0 + q, b);
    }
  }
  kt_end(w.kt, KC_RUNS);
}

// ------------------------------------------- small iterations: local bucket sort + runs -----
// Below 2^20 positions the stable bucket order (merge_hashtable, cluster.cc:15-30) is built in two
// steps: a stable partition by the top kTailTopBits = 9 key bits (radix_sort_top: one hist / dscan / scatter
// pass), then this kernel — workgroup d takes top bucket d, a contiguous range of the partition in
// canonical order, and sorts it stably by the remaining `lb` low bits (a counting sort in LDS:
// digit counts, their exclusive scan, then ranks among equal digits in position order from wave
// ballots, 4096 keys per round).  Equal keys of one top bucket have equal low bits, so the runs
// of the iteration are exactly the low digits with a count >= 2: their (start, length) entries
// come straight from the digit counts, classified as k_runs_write does (run_class), with one
// list-counter add per list per bucket — the whole run finding of these iterations without the
// tile kernels (k_runs_count / k_runs_write) or the second radix pass (3 launches).
__global__ __launch_bounds__(256) void k_tail_local(const uint32_t* __restrict__ kin,
                                                    const uint32_t* __restrict__ vin,
                                                    uint32_t* __restrict__ kout,
                                                    uint32_t* __restrict__ vout,
                                                    const uint32_t* __restrict__ dtot, int lb,
                                                    int bucket_thr, MergeView w) {
  // (4 or 8 keys per lane per round measured the same as 16; J adaptive vs always 16: C2 run
  // listing 18.2 vs 18.4 ms per step, one box, three rounds)
  constexpr uint32_t kItems = 16;  // keys per lane per round at most
  constexpr uint32_t kRad = 1u << kTailLowBits, kPer = kRad / 256u;  // digits per thread
  __shared__ uint32_t cnt[kRad];      // low-digit counts, then their exclusive starts
  __shared__ uint32_t run_[kRad];     // running count of each digit over the rounds
  __shared__ uint32_t wc[4][kRad];    // per-wave digit counts of a round, then wave prefixes
  __shared__ uint32_t lcnt[kRunRows];  // this bucket's list counts, rows, heads
  __shared__ uint32_t lbase[kRunLists];
  __shared__ RunListPtr lptr[kRunLists];
  __shared__ uint32_t red[4];
  kt_begin(w.kt, KC_RUNS);
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const uint32_t d = blockIdx.x;
  const uint32_t RAD = 1u << lb, MASK = RAD - 1u;
  [[maybe_unused]] uint64_t tp0 = MPROF_T(), tp1 = 0;
  // the bucket: [base, base + m) of the partition
  // (every global load of this kernel is unconditional, index clamped into range: a load under a
  // branch is waited for at once, and these few-hundred-key buckets are a chain of round trips)
  uint32_t part = 0;
  const uint32_t m = dtot[d];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t i = t * 4u + (uint32_t)q;
    const uint32_t x = dtot[i < d ? i : 0u];
    part += i < d ? x : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if (lane == 0) red[wv] = part;
  for (uint32_t i = t; i < kRad; i += 256) {
    cnt[i] = 0u;
    run_[i] = 0u;
    wc[0][i] = wc[1][i] = wc[2][i] = wc[3][i] = 0u;
  }
  if (t < (uint32_t)kRunRows) lcnt[t] = 0u;
  __syncthreads();
  const uint32_t base = red[0] + red[1] + red[2] + red[3];
  if (m == 0u) {
    kt_end(w.kt, KC_RUNS);
    return;
  }
#ifdef KLSH_MERGE_PROF
  if (t == 0) { tp1 = MPROF_T(); TPROF_ADD(0, tp1 - tp0); TPROF_ADD(4, 1); }
#endif
  // 1. low-digit counts, in the scatter's layout: a round covers J * 256 positions, wave wv the J*64
  //    consecutive ones from wv*J*64 (item j of lane l: + j*64 + l), J = ceil(m / 256) up to 16 —
  //    so a bucket of a few hundred keys is spread over all four waves instead of being wave 0's
  //    chain of ranks.  The keys and slots of the first round are loaded together: a bucket of one
  //    round (almost all of them) is read once, the scatter below reuses the registers
  const uint32_t J = min(kItems, (m + 255u) / 256u), kChunk = J * 256u, kWave = J * 64u;
  uint32_t k[kItems], v[kItems];
#pragma unroll
  for (int j = 0; j < (int)kItems; ++j) {
    const uint32_t p = wv * kWave + (uint32_t)j * 64u + lane;
    const bool ok = (uint32_t)j < J && p < m;
    k[j] = kin[base + (ok ? p : 0u)];
    v[j] = vin[base + (ok ? p : 0u)];
  }
#pragma unroll
  for (int j = 0; j < (int)kItems; ++j)
    if ((uint32_t)j < J && wv * kWave + (uint32_t)j * 64u + lane < m) atomicAdd(&cnt[k[j] & MASK], 1u);
  for (uint32_t r0 = kChunk; r0 < m; r0 += kChunk) {  // (rare) further rounds: keys only
    uint32_t kk[kItems];
#pragma unroll
    for (int j = 0; j < (int)kItems; ++j) {
      const uint32_t p = r0 + wv * kWave + (uint32_t)j * 64u + lane;
      kk[j] = kin[base + (p < m ? p : 0u)];
    }
#pragma unroll
    for (int j = 0; j < (int)kItems; ++j)
      if (r0 + wv * kWave + (uint32_t)j * 64u + lane < m) atomicAdd(&cnt[kk[j] & MASK], 1u);
  }
  __syncthreads();
#ifdef KLSH_MERGE_PROF
  if (t == 0) { const uint64_t x = MPROF_T(); TPROF_ADD(1, x - tp1); tp1 = x; }
#endif
  // 2. the runs (digits with a count >= 2) per list, and the digit starts
  uint32_t c4[kPer], acc = 0, heads = 0, small_rows = 0;
  uint32_t lrows[kBigClasses + 1] = {};
  int l4[kPer];
#pragma unroll
  for (int q = 0; q < (int)kPer; ++q) {
    const uint32_t dg = t * kPer + (uint32_t)q;
    c4[q] = dg < RAD ? cnt[dg] : 0u;
    acc += c4[q];
    heads += c4[q] ? 1u : 0u;
    l4[q] = c4[q] >= 2u ? run_class(c4[q], bucket_thr) : -1;
    if (l4[q] >= 0) {
      atomicAdd(&lcnt[l4[q]], 1u);
      if (l4[q] < kGroupClasses) small_rows += c4[q];
#pragma unroll
      for (int c = 0; c <= kBigClasses; ++c)
        if (l4[q] == kGroupClasses + c) lrows[c] += c4[q];
    }
  }
  uint32_t total;
  uint32_t pre = block_excl_scan_256(acc, &total);  // (syncs: every lcnt add is in)
#pragma unroll
  for (int q = 0; q < (int)kPer; ++q) {
    const uint32_t dg = t * kPer + (uint32_t)q;
    if (dg < RAD) cnt[dg] = pre;
    pre += c4[q];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    heads += __shfl_xor(heads, o, 64);
    small_rows += __shfl_xor(small_rows, o, 64);
#pragma unroll
    for (int c = 0; c <= kBigClasses; ++c) lrows[c] += __shfl_xor(lrows[c], o, 64);
  }
  if (lane == 0) {
    if (heads) atomicAdd(&lcnt[kRunLists], heads);
    if (small_rows) atomicAdd(&lcnt[kRunLists + 1], small_rows);
#pragma unroll
    for (int c = 0; c <= kBigClasses; ++c)
      if (lrows[c]) atomicAdd(&lcnt[kRunLists + 2 + c], lrows[c]);
  }
  __syncthreads();
  if (t < (uint32_t)kRunRows && lcnt[t]) {  // one add per list (and counter) per bucket
    const uint32_t v = atomicAdd(run_counter(w.rc, (int)t), lcnt[t]);
    if (t < (uint32_t)kRunLists) lbase[t] = v;
  }
  if (t < (uint32_t)kRunLists) lcnt[t] = 0u;  // (reused as the list cursors)
  run_list_table(w, lptr);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < (int)kPer; ++q) {
    const int l = l4[q];
    if (l >= 0) {
      const uint32_t dg = t * kPer + (uint32_t)q;
      const uint32_t at = lbase[l] + atomicAdd(&lcnt[l], 1u);
      lptr[l][at] = run_entry(base + cnt[dg], c4[q]);
    }
  }
  // 3. the stable scatter, J * 256 keys per round (wave wv: positions wv*J*64 + j*64 + lane)
#ifdef KLSH_MERGE_PROF
  __syncthreads();
  if (t == 0) { const uint64_t x = MPROF_T(); TPROF_ADD(2, x - tp1); tp1 = x; }
#endif
  const uint64_t lt = lane ? (~0ull >> (64u - lane)) : 0ull;
  for (uint32_t r0 = 0; r0 < m; r0 += kChunk) {
    uint32_t lr[kItems];
    if (m > kChunk) {  // (block-uniform) a bucket of several rounds reloads each round
#pragma unroll
      for (int j = 0; j < (int)kItems; ++j) {
        const uint32_t p = r0 + wv * kWave + (uint32_t)j * 64u + lane;
        k[j] = kin[base + (p < m ? p : 0u)];
        v[j] = vin[base + (p < m ? p : 0u)];
      }
    }
#pragma unroll
    for (int j = 0; j < (int)kItems; ++j) {
      lr[j] = 0u;
      if ((uint32_t)j < J) {  // (uniform)
        const bool valid = r0 + wv * kWave + (uint32_t)j * 64u + lane < m;
        const uint32_t dig = k[j] & MASK;
        uint64_t match = __ballot(valid);
        for (int b = 0; b < lb; ++b) {
          const bool bit = (dig >> b) & 1u;
          const uint64_t mb = __ballot(bit);
          match &= bit ? mb : ~mb;
        }
        const uint32_t old = wc[wv][dig];  // every lane reads before the group's leader writes
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (valid && (match & lt) == 0ull) wc[wv][dig] = old + (uint32_t)__popcll(match);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        lr[j] = old + (uint32_t)__popcll(match & lt);
      }
    }
    __syncthreads();
    for (uint32_t dg = t; dg < RAD; dg += 256) {  // wave prefixes of this round
      const uint32_t c0 = wc[0][dg], c1 = wc[1][dg], c2 = wc[2][dg], c3 = wc[3][dg];
      const uint32_t at = cnt[dg] + run_[dg];
      wc[0][dg] = at;
      wc[1][dg] = at + c0;
      wc[2][dg] = at + c0 + c1;
      wc[3][dg] = at + c0 + c1 + c2;
      run_[dg] += c0 + c1 + c2 + c3;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < (int)kItems; ++j) {
      if ((uint32_t)j < J && r0 + wv * kWave + (uint32_t)j * 64u + lane < m) {
        const uint32_t o = base + wc[wv][k[j] & MASK] + lr[j];
        kout[o] = k[j];
        vout[o] = v[j];
      }
    }
    __syncthreads();
    for (uint32_t dg = t; dg < RAD; dg += 256) wc[0][dg] = wc[1][dg] = wc[2][dg] = wc[3][dg] = 0u;
    __syncthreads();
  }
#ifdef KLSH_MERGE_PROF
  if (t == 0) {
    const uint64_t x = MPROF_T();
    TPROF_ADD(3, x - tp1);
    atomicMax(&g_tprof[5], (unsigned long long)(x - tp0));
  }
#endif
  kt_end(w.kt, KC_RUNS);
}

}  // namespace klsh
