// gfx950 kernels of klsh_diff_ksets / klsh_parse_clust: the text of <F>.clust —
// what k_save_emit writes — parsed back on the device, and the two differential k-mer sets
// selected from kmer_set.hex.
//
// The text is REGULAR when every byte is a digit, a newline or one of the other five isspace
// bytes, and no digit run is longer than kDiffMaxDigits: a token is then a maximal digit run, a
// line's tokens are those between its newlines, and the reference's strtol chain is a function of
// the two.  Anything else is found (its smallest offset) and left to the host parser.
//
//   k_diff_tile / k_diff_scan_tiles   per tile of 256 lanes x 16 bytes: newlines, token starts,
//                     the smallest irregular offset; one workgroup scans the tile sums
//   k_diff_tokens     the in-tile scan again: tok_val[t] (each token-start lane parses its own run,
//                     reading across the tile edge from memory), line_tok0[l + 1] (the tokens
//                     before each newline)
//   k_diff_counts / k_diff_scan_counts / k_diff_offsets   n_c = the line's first token; off = its
//                     exclusive sum (64-bit, saturating: refused from 2^32 on)
//   k_diff_ids        one lane per entry: its line by the bounded search of k_save_emit (row_of),
//                     its id the line's token 1 + j, 0 past the line's tokens
//   k_diff_mark / k_diff_count / k_diff_insert   the ids of group-1 / group-2 lines mark bytes of
//                     A / B (same-value stores race), the marks are counted, and row i of
//                     kmer_set.hex is claimed into A if marked A, else into B if marked B
//
// Every kernel strides over its tiles on its own (no workgroup waits for another), so every launch
// takes option "grid_cap".  The text buffer holds newlines from `len` to the end of its last tile
// and kDiffPad bytes past it: a lane's 16-byte load and a token's look-ahead of up to
// kDiffMaxDigits + 1 bytes are unconditional and in bounds (the conditional-load rule).
// Integer work only.
//
// Cost (measured): C2's 79.9 MB text, 10.3M tokens and 10.0M entries take 0.53 ms
// of HIP-event time in all the parser's launches, the marks and the two tables 0.75 ms; the call
// around them is host work (file reads, klsh_wrs).  By construction the text is read twice in
// 16-byte loads and each token once more bytewise; no counter run has split that 0.53 ms further.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "klsh_device.h"
#include "klsh_kmer.h"

namespace klsh {

namespace {

constexpr uint32_t kDiffGridMax = 2048;  // workgroups per launch, at most (the rest is strided)

inline uint32_t diff_grid(uint64_t tiles, uint32_t grid_cap) {
  return cap_grid((uint32_t)std::min<uint64_t>(std::max<uint64_t>(tiles, 1), kDiffGridMax), grid_cap);
}

__device__ __forceinline__ bool is_digit(uint32_t c) { return c - (uint32_t)'0' < 10u; }
// newline aside, the isspace bytes of the C locale: 9, 11, 12, 13, 32
__device__ __forceinline__ bool is_blank(uint32_t c) { return c == 32u || c == 9u || c - 11u < 3u; }

// A lane's 16 bytes of tile t as bit masks (bit i = byte pos + i), only positions below len.
struct LaneBytes {
  uint32_t pos;  // of the lane's first byte (may be >= len: every mask is then empty)
  uint32_t nl;   // newlines
  uint32_t ts;   // token starts: a digit whose predecessor is none
  uint32_t dig;  // digits
  uint32_t bad;  // bytes outside the grammar
};

// (contains barriers: every lane of the workgroup calls it)
__device__ __forceinline__ LaneBytes lane_bytes(const uint8_t* __restrict__ txt, uint32_t len,
                                                uint64_t t) {
  __shared__ uint8_t lastb[256];
  LaneBytes b;
  b.pos = (uint32_t)(t * kDiffTile) + threadIdx.x * 16u;  // (< len rounded up to a tile <= 2^32)
  const uint64_t pos64 = t * kDiffTile + threadIdx.x * 16ull;
  const uint4 w = *reinterpret_cast<const uint4*>(txt + pos64);
  const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
  lastb[threadIdx.x] = (uint8_t)(w.w >> 24);
  __syncthreads();
  // the byte before the lane's 16: the neighbour's last inside the tile, memory at the tile's
  // start, a newline before position 0
  const uint32_t prev = threadIdx.x ? lastb[threadIdx.x - 1u]
                                    : (pos64 ? (uint32_t)txt[pos64 - 1u] : (uint32_t)'\n');
  __syncthreads();
  uint32_t nl = 0, dig = 0, sp = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t c = (ww[i >> 2] >> (8 * (i & 3))) & 0xFFu;
    nl |= (c == (uint32_t)'\n' ? 1u : 0u) << i;
    dig |= (is_digit(c) ? 1u : 0u) << i;
    sp |= (is_blank(c) ? 1u : 0u) << i;
  }
  const uint64_t left = (uint64_t)len > pos64 ? (uint64_t)len - pos64 : 0ull;
  const uint32_t valid = left >= 16u ? 0xFFFFu : ((1u << (uint32_t)left) - 1u);
  const uint32_t before = ((dig << 1) | (is_digit(prev) ? 1u : 0u)) & 0xFFFFu;
  b.nl = nl & valid;
  b.dig = dig & valid;
  b.ts = dig & ~before & valid;
  b.bad = ~(nl | dig | sp) & valid;
  return b;
}

// 256-lane exclusive scan of 64-bit values, the sums saturating at kDiffSat (v <= kDiffSat)
__device__ __forceinline__ uint64_t sat_add(uint64_t a, uint64_t b) {
  const uint64_t c = a + b;  // (<= 2^63)
  return c < kDiffSat ? c : kDiffSat;
}
__device__ __forceinline__ uint64_t block_excl_scan_256_sat(uint64_t v, uint64_t* total) {
  __shared__ uint64_t sc[256];
  sc[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t o = 1; o < 256u; o <<= 1) {
    const uint64_t y = threadIdx.x >= o ? sc[threadIdx.x - o] : 0ull;
    __syncthreads();
    sc[threadIdx.x] = sat_add(sc[threadIdx.x], y);
    __syncthreads();
  }
  const uint64_t excl = threadIdx.x ? sc[threadIdx.x - 1u] : 0ull;
  *total = sc[255];
  __syncthreads();
  return excl;
}

// The line of entry q of tile t (256 entries): the tile's first and last entries bound the lines
// of every lane, as in k_save_emit.  False past the entries.
__device__ __forceinline__ bool entry_line(const uint32_t* __restrict__ off, uint32_t n_lines,
                                           uint32_t total, uint64_t t, uint32_t* q_out,
                                           uint32_t* c_out) {
  const uint64_t e0 = t * kDiffLineTile, e1 = e0 + (kDiffLineTile - 1u);
  const uint32_t q0 = (uint32_t)e0, q1 = e1 < total ? (uint32_t)e1 : total - 1u;
  const uint32_t r_lo = row_of(off, 0u, n_lines - 1u, q0);
  const uint32_t r_hi = row_of(off, r_lo, n_lines - 1u, q1);
  if (e0 + threadIdx.x > q1) return false;
  *q_out = q0 + threadIdx.x;
  *c_out = row_of(off, r_lo, r_hi, *q_out);
  return true;
}

}  // namespace

// ------------------------------------------------------------------- (a) tiles of the text -----
__global__ __launch_bounds__(256) void k_diff_tile(const uint8_t* __restrict__ txt, uint32_t len,
                                                   uint64_t ntiles, uint32_t* __restrict__ tile_nl,
                                                   uint32_t* __restrict__ tile_ts,
                                                   unsigned long long* __restrict__ hdr) {
  uint32_t irr = 0xFFFFFFFFu;  // (an offset is below len <= 2^32 - 1: never all ones)
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const LaneBytes b = lane_bytes(txt, len, t);
    if (b.bad) irr = min(irr, b.pos + (uint32_t)__builtin_ctz(b.bad));
    // a run of more than kDiffMaxDigits digits: its first digit's offset.  The run's digits inside
    // the lane's bytes are known; the rest are read from memory (at most pos + 15 + kDiffMaxDigits
    // < len + kDiffPad).
    uint32_t m = b.ts;
    while (m) {
      const uint32_t i = (uint32_t)__builtin_ctz(m);
      m &= m - 1u;
      uint32_t r = (uint32_t)__builtin_ctz(~(b.dig >> i) | 0x10000u);  // digits from bit i on
      if (i + r == 16u) {
        const uint8_t* p = txt + ((uint64_t)b.pos + i);
        while (r <= kDiffMaxDigits && is_digit(p[r])) ++r;
      }
      if (r > kDiffMaxDigits) irr = min(irr, b.pos + i);
    }
    uint32_t total;
    block_excl_scan_256(((uint32_t)__popc(b.nl) << 16) | (uint32_t)__popc(b.ts), &total);
    if (threadIdx.x == 0) {
      tile_nl[t] = total >> 16;     // (<= 4096)
      tile_ts[t] = total & 0xFFFFu; // (<= 2048)
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) irr = min(irr, (uint32_t)__shfl_xor(irr, o, 64));
  if ((threadIdx.x & 63u) == 0 && irr != 0xFFFFFFFFu) atomicMin(&hdr[kDiffIrregular], (unsigned long long)irr);
}

// One workgroup: both tile arrays -> their exclusive prefixes; the totals and the line count.
__global__ __launch_bounds__(256) void k_diff_scan_tiles(const uint8_t* __restrict__ txt,
                                                         uint32_t len, uint64_t ntiles,
                                                         uint32_t* __restrict__ tile_nl,
                                                         uint32_t* __restrict__ tile_ts,
                                                         unsigned long long* __restrict__ hdr) {
  uint32_t carry_nl = 0, carry_ts = 0;  // (both below len < 2^32)
  for (uint64_t t0 = 0; t0 < ntiles; t0 += 256) {
    const uint64_t t = t0 + threadIdx.x;
    const uint32_t a = t < ntiles ? tile_nl[t] : 0u, b = t < ntiles ? tile_ts[t] : 0u;
    uint32_t ta, tb;
    const uint32_t pa = block_excl_scan_256(a, &ta);
    const uint32_t pb = block_excl_scan_256(b, &tb);
    if (t < ntiles) {
      tile_nl[t] = carry_nl + pa;
      tile_ts[t] = carry_ts + pb;
    }
    carry_nl += ta;
    carry_ts += tb;
  }
  if (threadIdx.x == 0) {
    hdr[kDiffNewlines] = carry_nl;
    hdr[kDiffTokens] = carry_ts;
    hdr[kDiffLines] = (unsigned long long)carry_nl + (len && txt[len - 1u] != (uint8_t)'\n' ? 1u : 0u);
  }
}

void launch_diff_scan(const uint8_t* txt, uint32_t len, uint32_t* tile_nl, uint32_t* tile_ts,
                      unsigned long long* hdr, hipStream_t s, uint32_t grid_cap) {
  const uint64_t ntiles = diff_tiles(len);
  if (ntiles) k_diff_tile<<<diff_grid(ntiles, grid_cap), 256, 0, s>>>(txt, len, ntiles, tile_nl, tile_ts, hdr);
  k_diff_scan_tiles<<<1, 256, 0, s>>>(txt, len, ntiles, tile_nl, tile_ts, hdr);
}

// ------------------------------------------------------------------- (b) tokens and lines ------
__global__ __launch_bounds__(256) void k_diff_tokens(const uint8_t* __restrict__ txt, uint32_t len,
                                                     uint64_t ntiles,
                                                     const uint32_t* __restrict__ tile_nl,
                                                     const uint32_t* __restrict__ tile_ts,
                                                     uint32_t n_lines, uint32_t n_tokens,
                                                     uint64_t* __restrict__ tok_val,
                                                     uint32_t* __restrict__ line_tok0) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    line_tok0[0] = 0u;
    // an unterminated last line ends where the text does
    if (len && txt[len - 1u] != (uint8_t)'\n') line_tok0[n_lines] = n_tokens;
  }
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const LaneBytes b = lane_bytes(txt, len, t);
    uint32_t total;
    const uint32_t ex =
        block_excl_scan_256(((uint32_t)__popc(b.nl) << 16) | (uint32_t)__popc(b.ts), &total);
    uint32_t l = tile_nl[t] + (ex >> 16);     // newlines before the lane's bytes (< n_lines)
    uint32_t k = tile_ts[t] + (ex & 0xFFFFu); // tokens before them
    uint32_t m = b.nl | b.ts;
    while (m) {
      const uint32_t i = (uint32_t)__builtin_ctz(m);
      m &= m - 1u;
      if ((b.nl >> i) & 1u) {
        line_tok0[++l] = k;  // (l <= the newlines <= n_lines)
      } else {
        // the run's value: at most kDiffMaxDigits digits (the text is regular), read up to the
        // first other byte — a newline of the pad at the latest
        const uint8_t* p = txt + ((uint64_t)b.pos + i);
        uint64_t v = 0;
        for (uint32_t j = 0; j < kDiffMaxDigits; ++j) {
          const uint32_t c = p[j];
          if (!is_digit(c)) break;
          v = v * 10u + (c - (uint32_t)'0');
        }
        tok_val[k++] = v;  // (k < n_tokens)
      }
    }
  }
}

void launch_diff_tokens(const uint8_t* txt, uint32_t len, const uint32_t* tile_nl,
                        const uint32_t* tile_ts, uint32_t n_lines, uint32_t n_tokens,
                        uint64_t* tok_val, uint32_t* line_tok0, hipStream_t s, uint32_t grid_cap) {
  const uint64_t ntiles = diff_tiles(len);
  k_diff_tokens<<<diff_grid(ntiles, grid_cap), 256, 0, s>>>(txt, len, ntiles, tile_nl, tile_ts,
                                                           n_lines, n_tokens, tok_val, line_tok0);
}

// ------------------------------------------------------------------- (c) counts and offsets ----
__global__ __launch_bounds__(256) void k_diff_counts(const uint64_t* __restrict__ tok_val,
                                                     const uint32_t* __restrict__ line_tok0,
                                                     uint32_t n_lines, uint64_t ntiles,
                                                     uint64_t* __restrict__ cnt,
                                                     uint64_t* __restrict__ csum) {
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t c = t * kDiffLineTile + threadIdx.x;
    uint64_t n = 0;
    if (c < n_lines) {
      const uint32_t a = line_tok0[c], b = line_tok0[c + 1u];
      n = b > a ? tok_val[a] : 0ull;
      cnt[c] = n;
    }
    uint64_t total;
    block_excl_scan_256_sat(n < kDiffSat ? n : kDiffSat, &total);
    if (threadIdx.x == 0) csum[t] = total;
  }
}

// One workgroup: csum[t] = the saturating sum of the tiles below t, t <= ntiles.
__global__ __launch_bounds__(256) void k_diff_scan_counts(uint64_t* __restrict__ csum,
                                                          uint64_t ntiles,
                                                          unsigned long long* __restrict__ hdr) {
  uint64_t carry = 0;
  for (uint64_t t0 = 0; t0 < ntiles; t0 += 256) {
    const uint64_t t = t0 + threadIdx.x;
    const uint64_t v = t < ntiles ? csum[t] : 0ull;
    uint64_t total;
    const uint64_t p = block_excl_scan_256_sat(v, &total);
    if (t < ntiles) csum[t] = sat_add(carry, p);
    carry = sat_add(carry, total);
  }
  if (threadIdx.x == 0) {
    csum[ntiles] = carry;
    hdr[kDiffEntries] = carry;
  }
}

void launch_diff_counts(const uint64_t* tok_val, const uint32_t* line_tok0, uint32_t n_lines,
                        uint64_t* cnt, uint64_t* csum, unsigned long long* hdr, hipStream_t s,
                        uint32_t grid_cap) {
  const uint64_t ntiles = diff_line_tiles(n_lines);
  if (ntiles)
    k_diff_counts<<<diff_grid(ntiles, grid_cap), 256, 0, s>>>(tok_val, line_tok0, n_lines, ntiles, cnt, csum);
  k_diff_scan_counts<<<1, 256, 0, s>>>(csum, ntiles, hdr);
}

// (the sum is below 2^32 here: every prefix fits 32 bits)
__global__ __launch_bounds__(256) void k_diff_offsets(const uint64_t* __restrict__ cnt,
                                                      const uint64_t* __restrict__ csum,
                                                      uint32_t n_lines, uint64_t ntiles,
                                                      uint32_t* __restrict__ off) {
  if (blockIdx.x == 0 && threadIdx.x == 0) off[n_lines] = (uint32_t)csum[ntiles];
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t c = t * kDiffLineTile + threadIdx.x;
    const uint64_t n = c < n_lines ? cnt[c] : 0ull;
    uint64_t total;
    const uint64_t p = block_excl_scan_256_sat(n, &total);
    if (c < n_lines) off[c] = (uint32_t)(csum[t] + p);
  }
}

void launch_diff_offsets(const uint64_t* cnt, const uint64_t* csum, uint32_t n_lines, uint32_t* off,
                         hipStream_t s, uint32_t grid_cap) {
  const uint64_t ntiles = diff_line_tiles(n_lines);
  k_diff_offsets<<<diff_grid(ntiles, grid_cap), 256, 0, s>>>(cnt, csum, n_lines, ntiles, off);
}

// ------------------------------------------------------------------- (d) the entries' ids ------
__global__ __launch_bounds__(256) void k_diff_ids(const uint64_t* __restrict__ tok_val,
                                                  const uint32_t* __restrict__ line_tok0,
                                                  const uint32_t* __restrict__ off, uint32_t n_lines,
                                                  uint32_t total, uint64_t ntiles,
                                                  uint64_t* __restrict__ ids) {
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint32_t q, c;
    if (!entry_line(off, n_lines, total, t, &q, &c)) continue;
    const uint32_t j = q - off[c];
    const uint32_t a = line_tok0[c], tc = line_tok0[c + 1u] - a;  // (tc >= 1: the line declares j + 1)
    // strtol past the line's last token converts nothing: the entry stays 0
    ids[q] = j + 1u < tc ? tok_val[a + 1u + j] : 0ull;
  }
}

void launch_diff_ids(const uint64_t* tok_val, const uint32_t* line_tok0, const uint32_t* off,
                     uint32_t n_lines, uint32_t total, uint64_t* ids, hipStream_t s,
                     uint32_t grid_cap) {
  if (total == 0 || n_lines == 0) return;
  const uint64_t ntiles = diff_line_tiles(total);
  k_diff_ids<<<diff_grid(ntiles, grid_cap), 256, 0, s>>>(tok_val, line_tok0, off, n_lines, total, ntiles, ids);
}

// ------------------------------------------------------------------- (e) marks and sets --------
__global__ __launch_bounds__(256) void k_diff_mark(const uint32_t* __restrict__ off, uint32_t n_lines,
                                                   const uint64_t* __restrict__ ids, uint32_t total,
                                                   uint64_t ntiles, const uint8_t* __restrict__ group,
                                                   uint64_t kmap, uint8_t* __restrict__ mark_a,
                                                   uint8_t* __restrict__ mark_b) {
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint32_t q, c;
    if (!entry_line(off, n_lines, total, t, &q, &c)) continue;
    const uint32_t g = group[c];
    const uint64_t id = ids[q];
    if (id >= kmap) continue;  // app/kmerLSH.cc looks the row index up in the sets: none that large
    if (g == 1u) mark_a[id] = 1u;
    else if (g == 2u) mark_b[id] = 1u;
  }
}

void launch_diff_mark(const uint32_t* off, uint32_t n_lines, const uint64_t* ids, uint32_t total,
                      const uint8_t* group, uint64_t kmap, uint8_t* mark_a, uint8_t* mark_b,
                      hipStream_t s, uint32_t grid_cap) {
  if (total == 0 || n_lines == 0 || kmap == 0) return;
  const uint64_t ntiles = diff_line_tiles(total);
  k_diff_mark<<<diff_grid(ntiles, grid_cap), 256, 0, s>>>(off, n_lines, ids, total, ntiles, group,
                                                         kmap, mark_a, mark_b);
}

__global__ __launch_bounds__(256) void k_diff_count(const uint8_t* __restrict__ mark_a,
                                                    const uint8_t* __restrict__ mark_b, uint64_t kmap,
                                                    unsigned long long* __restrict__ hdr) {
  uint32_t ia = 0, ib = 0, kb = 0;  // (a lane sees kmap / the launch's lanes rows: far below 2^32)
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < kmap; i += (uint64_t)gridDim.x * 256ull) {
    const uint32_t a = mark_a[i] ? 1u : 0u, b = mark_b[i] ? 1u : 0u;
    ia += a;
    ib += b;
    kb += b & (a ^ 1u);  // a row marked for both goes to A
  }
  unsigned long long va = ia, vb = ib, vk = kb;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    va += __shfl_xor(va, o, 64);
    vb += __shfl_xor(vb, o, 64);
    vk += __shfl_xor(vk, o, 64);
  }
  if ((threadIdx.x & 63u) == 0) {
    if (va) atomicAdd(&hdr[kDiffIdsA], va), atomicAdd(&hdr[kDiffKmersA], va);
    if (vb) atomicAdd(&hdr[kDiffIdsB], vb);
    if (vk) atomicAdd(&hdr[kDiffKmersB], vk);
  }
}

void launch_diff_count(const uint8_t* mark_a, const uint8_t* mark_b, uint64_t kmap,
                       unsigned long long* hdr, hipStream_t s, uint32_t grid_cap) {
  if (kmap == 0) return;
  // (at most 2048 workgroups: a lane's 32-bit counts hold up to 2^32 rows each)
  k_diff_count<<<stride_grid(kmap, grid_cap, kDiffGridMax), 256, 0, s>>>(mark_a, mark_b, kmap, hdr);
}

__global__ __launch_bounds__(256) void k_diff_insert(const uint64_t* __restrict__ kmers,
                                                     const uint8_t* __restrict__ mark_a,
                                                     const uint8_t* __restrict__ mark_b, uint64_t kmap,
                                                     unsigned long long* __restrict__ tab_a,
                                                     uint64_t mask_a,
                                                     unsigned long long* __restrict__ tab_b,
                                                     uint64_t mask_b) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < kmap; i += (uint64_t)gridDim.x * 256ull) {
    const bool a = mark_a[i] != 0;
    if (!a && !mark_b[i]) continue;
    const unsigned long long key = kmers[i];
    if (key == kKtabEmpty) continue;  // cannot be a canonical rep: never looked up (k_kset_insert)
    if (a) (void)ktab_claim(tab_a, mask_a, key);
    else (void)ktab_claim(tab_b, mask_b, key);
  }
}

void launch_diff_insert(const uint64_t* kmers, const uint8_t* mark_a, const uint8_t* mark_b,
                        uint64_t kmap, uint64_t* tab_a, uint64_t mask_a, uint64_t* tab_b,
                        uint64_t mask_b, hipStream_t s, uint32_t grid_cap) {
  if (kmap == 0) return;
  k_diff_insert<<<stride_grid(kmap, grid_cap, 8192), 256, 0, s>>>(
      kmers, mark_a, mark_b, kmap, reinterpret_cast<unsigned long long*>(tab_a), mask_a,
      reinterpret_cast<unsigned long long*>(tab_b), mask_b);
}

}  // namespace klsh
