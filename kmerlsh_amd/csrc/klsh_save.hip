// gfx950 kernels of klsh_save_clusters: the reference's cluster files from the
// device-side result (off, nodes of klsh_result.hip).
//
//   k_save_keep_sums / _scan / _write   rows with more than ignore_small members: their count,
//                     their members, kslot[rank] = the row's slot (the binary file's row gather)
//   k_save_tile_len / k_save_scan_pos   the text's byte length per tile of 256 entries, and the
//                     64-bit position of every tile (three-launch scan with k_save_emit)
//   k_save_emit       a window [w0, w1) of the text: one token per lane ('\t' id; the row's first
//                     entry leads with the member count, its last ends with '\n'), laid out in an
//                     LDS byte tile and streamed out as aligned 16-byte stores, the window's and
//                     the tile's unaligned ends bytewise
//
// Every kernel strides over its tiles on its own (no workgroup waits for another), so every launch
// takes option "grid_cap".  Integer work only.
//
// Bound: the id gather — one random 8-B read per entry (ids[nodes[q]]), twice (lengths, emit);
// the text itself is written once, in 16-byte stores.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "klsh_device.h"
#include "klsh_save_plan.h"

namespace klsh {

namespace {

constexpr uint32_t kSaveGridMax = 2048;  // workgroups per launch, at most (the rest is strided)

inline uint32_t save_grid(uint64_t tiles, uint32_t grid_cap) {
  return cap_grid((uint32_t)std::min<uint64_t>(std::max<uint64_t>(tiles, 1), kSaveGridMax), grid_cap);
}

// decimal digits of v: one more for every power of ten 10^1 .. 10^19 that v reaches
__device__ __forceinline__ uint32_t dec_digits(uint64_t v) {
  uint32_t nd = 1;
  uint64_t p = 10;
#pragma unroll
  for (int i = 1; i < 20; ++i) {
    nd += v >= p ? 1u : 0u;
    p *= 10u;  // (10^20 wraps after the last comparison)
  }
  return nd;
}

// the nd digits of v at p[0, nd), most significant first: v = a 10^18 + b 10^9 + c, each piece
// divided down in 32 bits (the pieces above the lowest print zero-padded, as they must)
__device__ __forceinline__ void put_dec(uint8_t* p, uint64_t v, uint32_t nd) {
  const uint64_t hi = v / 1000000000ull;
  uint32_t part[3];
  part[0] = (uint32_t)(v - hi * 1000000000ull);
  part[2] = (uint32_t)(hi / 1000000000ull);
  part[1] = (uint32_t)(hi - (uint64_t)part[2] * 1000000000ull);
  uint32_t k = nd;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    uint32_t x = part[j];
    for (int i = 0; i < 9 && k; ++i) {
      const uint32_t y = x / 10u;
      p[--k] = (uint8_t)('0' + (x - y * 10u));
      x = y;
    }
  }
}

struct Token {
  uint64_t id;
  uint32_t cnt;     // the row's members, when this entry leads the row (else 0)
  uint32_t len;     // bytes; 0: the row is not kept, or q is past the entries
  uint32_t id_dig, cnt_dig;
  bool last;
};

// Entry q of tile t.  The tile's first and last entries bound the rows of every lane: two searches
// over all rows, the same in every lane, then one over the rows the tile touches.
__device__ __forceinline__ Token save_token(const SaveText& tx, uint64_t t,
                                            unsigned long long* __restrict__ hdr) {
  Token k{};
  const uint64_t e0 = t * kSaveTile, e1 = e0 + (kSaveTile - 1u);  // (total < 2^32; e1 may not be)
  const uint32_t q0 = (uint32_t)e0, q1 = e1 < tx.total ? (uint32_t)e1 : tx.total - 1u;
  const uint32_t r_lo = row_of(tx.off, 0u, tx.n - 1u, q0), r_hi = row_of(tx.off, r_lo, tx.n - 1u, q1);
  if (e0 + threadIdx.x > q1) return k;
  const uint32_t q = q0 + threadIdx.x;
  const uint32_t r = row_of(tx.off, r_lo, r_hi, q);
  const uint32_t a = tx.off[r], b = tx.off[r + 1u], c = b - a;
  if (!(c > tx.ignore_small)) return k;
  const uint32_t node = tx.nodes[q];
  if (node >= tx.members) {  // (the ranking wrote every entry: a hole is a broken list)
    if (hdr) atomicOr(&hdr[kSaveErr], 1ull);  // (the positions pass reports; emit runs after)
    return k;
  }
  k.id = tx.ids ? tx.ids[node] : tx.id_base + node;
  k.id_dig = dec_digits(k.id);
  k.len = 1u + k.id_dig;
  if (q == a) {
    k.cnt = c;
    k.cnt_dig = dec_digits(c);
    k.len += k.cnt_dig;
  }
  k.last = q + 1u == b;
  k.len += k.last ? 1u : 0u;
  return k;
}

// 256-lane exclusive scan of 64-bit values through LDS (one workgroup runs it; speed is no matter)
__device__ __forceinline__ uint64_t block_excl_scan_256_u64(uint64_t v, uint64_t* total) {
  __shared__ uint64_t sc[256];
  sc[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t o = 1; o < 256u; o <<= 1) {
    const uint64_t y = threadIdx.x >= o ? sc[threadIdx.x - o] : 0ull;
    __syncthreads();
    sc[threadIdx.x] += y;
    __syncthreads();
  }
  const uint64_t incl = sc[threadIdx.x];
  *total = sc[255];
  __syncthreads();
  return incl - v;
}

}  // namespace

// ------------------------------------------------------------------- (a) the kept rows ---------
// Tile t holds live rows [t * kResTile, (t + 1) * kResTile), kResItems consecutive rows per lane.
__global__ __launch_bounds__(256) void k_save_keep_sums(const uint32_t* __restrict__ off, uint32_t n,
                                                        uint32_t ignore_small, uint32_t ntiles,
                                                        uint32_t* __restrict__ tsum,
                                                        unsigned long long* __restrict__ hdr) {
  unsigned long long mem = 0;
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t base = (uint64_t)t * kResTile + threadIdx.x * kResItems;
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t k = 0; k < kResItems; ++k)
      if (base + k < n) {
        const uint32_t c = off[base + k + 1u] - off[base + k];
        if (c > ignore_small) acc += 1u, mem += c;
      }
    uint32_t total;
    block_excl_scan_256(acc, &total);
    if (threadIdx.x == 0) tsum[t] = total;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mem += __shfl_xor(mem, o, 64);
  if ((threadIdx.x & 63u) == 0 && mem) atomicAdd(&hdr[kSaveMembers], mem);
}

// One workgroup: tsum -> its exclusive prefix, hdr[kSaveKept] = the sum.
__global__ __launch_bounds__(256) void k_save_keep_scan(uint32_t* __restrict__ tsum, uint32_t ntiles,
                                                        unsigned long long* __restrict__ hdr) {
  uint32_t carry = 0;
  for (uint32_t t0 = 0; t0 < ntiles; t0 += 256) {
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t v = t < ntiles ? tsum[t] : 0u;
    uint32_t total;
    const uint32_t p = block_excl_scan_256(v, &total);
    if (t < ntiles) tsum[t] = carry + p;
    carry += total;
  }
  if (threadIdx.x == 0) hdr[kSaveKept] = carry;
}

__global__ __launch_bounds__(256) void k_save_keep_write(const uint32_t* __restrict__ order,
                                                         const uint32_t* __restrict__ off,
                                                         uint32_t n, uint32_t ignore_small,
                                                         uint32_t ntiles,
                                                         const uint32_t* __restrict__ tsum,
                                                         uint32_t* __restrict__ kslot) {
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t base = (uint64_t)t * kResTile + threadIdx.x * kResItems;
    bool keep[kResItems];
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t k = 0; k < kResItems; ++k) {
      keep[k] = false;
      if (base + k < n) {
        const uint32_t c = off[base + k + 1u] - off[base + k];
        keep[k] = c > ignore_small;
      }
      acc += keep[k] ? 1u : 0u;
    }
    uint32_t total;
    uint32_t run = block_excl_scan_256(acc, &total) + tsum[t];  // (< the kept rows <= n)
#pragma unroll
    for (uint32_t k = 0; k < kResItems; ++k)
      if (keep[k]) kslot[run++] = order[base + k];
  }
}

void launch_save_keep(const uint32_t* order, const uint32_t* off, uint32_t n, uint32_t ignore_small,
                      uint32_t* tsum, uint32_t* kslot, unsigned long long* hdr, hipStream_t s,
                      uint32_t grid_cap) {
  if (n == 0) return;  // hdr is zero already
  const uint32_t ntiles = result_tiles(n), g = save_grid(ntiles, grid_cap);
  k_save_keep_sums<<<g, 256, 0, s>>>(off, n, ignore_small, ntiles, tsum, hdr);
  k_save_keep_scan<<<1, 256, 0, s>>>(tsum, ntiles, hdr);
  k_save_keep_write<<<g, 256, 0, s>>>(order, off, n, ignore_small, ntiles, tsum, kslot);
}

// ------------------------------------------------------------------- (b) text positions --------
__global__ __launch_bounds__(256) void k_save_tile_len(SaveText tx, uint64_t ntiles,
                                                       uint64_t* __restrict__ tpos,
                                                       unsigned long long* __restrict__ hdr) {
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const Token k = save_token(tx, t, hdr);
    uint32_t total;
    block_excl_scan_256(k.len, &total);  // (<= 256 * kSaveMaxToken)
    if (threadIdx.x == 0) tpos[t] = total;
  }
}

// One workgroup: tpos[t] = pos_base + the lengths of the tiles below t, t <= ntiles; 64-bit sums.
__global__ __launch_bounds__(256) void k_save_scan_pos(uint64_t* __restrict__ tpos, uint64_t ntiles,
                                                       uint64_t pos_base) {
  uint64_t carry = pos_base;
  for (uint64_t t0 = 0; t0 < ntiles; t0 += 256) {
    const uint64_t t = t0 + threadIdx.x;
    const uint64_t v = t < ntiles ? tpos[t] : 0ull;
    uint64_t total;
    const uint64_t p = block_excl_scan_256_u64(v, &total);
    if (t < ntiles) tpos[t] = carry + p;
    carry += total;
  }
  if (threadIdx.x == 0) tpos[ntiles] = carry;
}

void launch_save_positions(const SaveText& tx, uint64_t pos_base, uint64_t* tpos,
                           unsigned long long* hdr, hipStream_t s, uint32_t grid_cap) {
  const uint64_t ntiles = save_tiles(tx.total);
  if (ntiles) k_save_tile_len<<<save_grid(ntiles, grid_cap), 256, 0, s>>>(tx, ntiles, tpos, hdr);
  k_save_scan_pos<<<1, 256, 0, s>>>(tpos, ntiles, pos_base);
}

// ------------------------------------------------------------------- (c) the text --------------
// The tile's bytes sit in LDS shifted so that an aligned 16-byte LDS word is an aligned 16-byte
// global store, and only the bytes at positions [w0, w1) leave (save_clip, klsh_save_plan.h: LDS
// bytes [A, B) to out[g0 + A .. g0 + B)); the words that [A, B) covers only in part go out
// bytewise.
__global__ __launch_bounds__(256) void k_save_emit(SaveText tx, const uint64_t* __restrict__ tpos,
                                                   uint64_t t_lo, uint64_t t_hi, uint64_t w0,
                                                   uint64_t w1, uint8_t* __restrict__ out,
                                                   unsigned long long* __restrict__ hdr) {
  __shared__ uint4 tile[(kSaveTile * kSaveMaxToken + 16u) / 16u + 1u];
  uint8_t* tb = reinterpret_cast<uint8_t*>(tile);
  for (uint64_t t = t_lo + blockIdx.x; t < t_hi; t += gridDim.x) {
    const Token k = save_token(tx, t, hdr);
    uint32_t tlen;
    const uint32_t at = block_excl_scan_256(k.len, &tlen);  // (its barriers: the last tile is out)
    const SaveClip c = save_clip(tpos[t], tlen, w0, w1);  // (the same in every lane)
    if (c.A >= c.B) continue;
    if (k.len) {
      uint8_t* p = tb + c.sh + at;
      if (k.cnt_dig) {
        put_dec(p, k.cnt, k.cnt_dig);
        p += k.cnt_dig;
      }
      *p++ = (uint8_t)'\t';
      put_dec(p, k.id, k.id_dig);
      if (k.last) p[k.id_dig] = (uint8_t)'\n';
    }
    __syncthreads();
    const uint32_t A = c.A, B = c.B;
    const int64_t g0 = c.g0;
    for (uint32_t w = (A >> 4) + threadIdx.x; (w << 4) < B; w += 256u) {
      const uint32_t L = w << 4;
      if (L >= A && L + 16u <= B) {
        *reinterpret_cast<uint4*>(out + (g0 + (int64_t)L)) = tile[w];
      } else {
        const uint32_t e = min(L + 16u, B);
        for (uint32_t j = max(L, A); j < e; ++j) out[g0 + (int64_t)j] = tb[j];
      }
    }
  }
}

void launch_save_emit(const SaveText& tx, const uint64_t* tpos, uint64_t t_lo, uint64_t t_hi,
                      uint64_t w0, uint64_t w1, uint8_t* out, hipStream_t s, uint32_t grid_cap) {
  if (t_lo >= t_hi || w0 >= w1) return;
  k_save_emit<<<save_grid(t_hi - t_lo, grid_cap), 256, 0, s>>>(tx, tpos, t_lo, t_hi, w0, w1, out,
                                                               nullptr);
}

}  // namespace klsh
