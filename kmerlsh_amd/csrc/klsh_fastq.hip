// gfx950 kernels of the device FASTQ parser (modes E and K, klsh_parse_fastq): a
// chunk of a plain FASTQ file, starting at a record boundary, split into lines and records on the
// device, and the records' sequences packed into the (seq, off) of a ReadBatch.
//
// Lines are split at '\n'; record r is lines 4r .. 4r + 3, the chunk's complete records are the
// n = newlines / 4 first.  The chunk is REGULAR when every complete record is (L0 '@' + any bytes;
// L1 bytes in [33, 126] but '>', '+', '@'; L2 '+' + bytes below 0x80; L3 len(L1) bytes in
// [33, 127]): the host reader (klsh_fastq_reader.h) then reads exactly these records.  Anything
// else is found, its smallest offset, and left to the host reader.
//
//   k_fq_tile / k_fq_scan_tiles   per tile of 256 lanes x 16 bytes: its newlines; one workgroup
//                     scans the tile sums: hdr[kFqNewlines], hdr[kFqRecords]
//   k_fq_lines        the in-tile scan again: each lane knows the line of its first byte, hence the
//                     kind (line & 3) of every byte; it checks its bytes by kind (a line's first
//                     byte is the one after a newline: the neighbour lane's last byte, memory at a
//                     tile's start, position 0), writes line_start[l + 1] after each newline of a
//                     complete record, and keeps the smallest irregular offset (atomicMin)
//   k_fq_records / k_fq_scan_records / k_fq_offsets   one lane per record: len(L3) == len(L1) or
//                     the offset line_start[4r + 3] + min of the two is irregular; the lengths'
//                     sums per 256 records, their scan, off[r] (64-bit)
//   k_fq_pack         one wave per record: L1 copied to seq + off[r]
//
// Every kernel strides over its tiles on its own (no workgroup waits for another), so every launch
// takes option "grid_cap".  A lane's 16-byte load is unconditional: the buffer holds
// fq_text_alloc(len) bytes, and the bytes from len on are masked out.  Positions are 32-bit
// (len < 2^32).  Integer work only.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "klsh_device.h"

namespace klsh {

namespace {

constexpr uint32_t kFqGridMax = 2048;  // workgroups per launch, at most (the rest is strided)

inline uint32_t fq_grid(uint64_t tiles, uint32_t grid_cap) {
  return cap_grid((uint32_t)std::min<uint64_t>(std::max<uint64_t>(tiles, 1), kFqGridMax), grid_cap);
}

// A lane's 16 bytes of tile t as bit masks (bit i = byte pos + i), only positions below len.
struct FqLane {
  uint32_t pos;    // of the lane's first byte (may be >= len: every mask is then empty)
  uint32_t valid;  // positions below len
  uint32_t nl;     // newlines
  uint32_t first;  // bytes that follow a newline (or are position 0): the first of their line
  uint32_t at, plus;  // '@', '+'
  uint32_t l1ok;   // [33, 126] without '>', '+', '@'
  uint32_t l3ok;   // [33, 127]
  uint32_t hi;     // >= 0x80
};

__device__ __forceinline__ uint4 fq_load(const uint8_t* __restrict__ txt, uint64_t t) {
  return *reinterpret_cast<const uint4*>(txt + (t * kFqTile + threadIdx.x * 16ull));
}

__device__ __forceinline__ uint32_t fq_valid(uint32_t len, uint64_t t) {
  const uint64_t pos64 = t * kFqTile + threadIdx.x * 16ull;
  const uint64_t left = (uint64_t)len > pos64 ? (uint64_t)len - pos64 : 0ull;
  return left >= 16u ? 0xFFFFu : ((1u << (uint32_t)left) - 1u);
}

__device__ __forceinline__ uint32_t fq_newlines(const uint4& w) {
  const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
  uint32_t nl = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t c = (ww[i >> 2] >> (8 * (i & 3))) & 0xFFu;
    nl |= (c == (uint32_t)'\n' ? 1u : 0u) << i;
  }
  return nl;
}

// (contains barriers: every lane of the workgroup calls it)
__device__ __forceinline__ FqLane fq_lane(const uint8_t* __restrict__ txt, uint32_t len, uint64_t t) {
  __shared__ uint8_t lastb[256];
  FqLane b;
  const uint64_t pos64 = t * kFqTile + threadIdx.x * 16ull;
  b.pos = (uint32_t)pos64;  // (< len rounded up to a tile <= 2^32)
  const uint4 w = fq_load(txt, t);
  const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
  lastb[threadIdx.x] = (uint8_t)(w.w >> 24);
  __syncthreads();
  // the byte before the lane's 16: the neighbour's last inside the tile, memory at the tile's
  // start, a newline before position 0
  const uint32_t prev = threadIdx.x ? lastb[threadIdx.x - 1u]
                                    : (pos64 ? (uint32_t)txt[pos64 - 1u] : (uint32_t)'\n');
  __syncthreads();
  uint32_t nl = 0, at = 0, plus = 0, l1 = 0, l3 = 0, hi = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t c = (ww[i >> 2] >> (8 * (i & 3))) & 0xFFu;
    const uint32_t is_at = c == (uint32_t)'@' ? 1u : 0u, is_plus = c == (uint32_t)'+' ? 1u : 0u;
    const uint32_t graph = c - 33u < 94u ? 1u : 0u;  // [33, 126]
    nl |= (c == (uint32_t)'\n' ? 1u : 0u) << i;
    at |= is_at << i;
    plus |= is_plus << i;
    l1 |= (graph & ~(is_at | is_plus | (c == (uint32_t)'>' ? 1u : 0u))) << i;
    l3 |= (c - 33u < 95u ? 1u : 0u) << i;  // [33, 127]
    hi |= (c >> 7) << i;
  }
  b.valid = fq_valid(len, t);
  b.nl = nl & b.valid;
  b.first = ((nl << 1) | (prev == (uint32_t)'\n' ? 1u : 0u)) & b.valid;
  b.at = at;
  b.plus = plus;
  b.l1ok = l1;
  b.l3ok = l3;
  b.hi = hi;
  return b;
}

}  // namespace

// ------------------------------------------------------------------- (a) tiles of the text -----
__global__ __launch_bounds__(256) void k_fq_tile(const uint8_t* __restrict__ txt, uint32_t len,
                                                 uint64_t ntiles, uint32_t* __restrict__ tile_nl) {
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint32_t nl = fq_newlines(fq_load(txt, t)) & fq_valid(len, t);
    uint32_t total;
    block_excl_scan_256((uint32_t)__popc(nl), &total);
    if (threadIdx.x == 0) tile_nl[t] = total;  // (<= 4096)
  }
}

// One workgroup: tile_nl -> its exclusive prefix; the newlines and the complete records.
__global__ __launch_bounds__(256) void k_fq_scan_tiles(uint64_t ntiles, uint32_t* __restrict__ tile_nl,
                                                       unsigned long long* __restrict__ hdr) {
  uint32_t carry = 0;  // (below len < 2^32)
  for (uint64_t t0 = 0; t0 < ntiles; t0 += 256) {
    const uint64_t t = t0 + threadIdx.x;
    const uint32_t a = t < ntiles ? tile_nl[t] : 0u;
    uint32_t ta;
    const uint32_t pa = block_excl_scan_256(a, &ta);
    if (t < ntiles) tile_nl[t] = carry + pa;
    carry += ta;
  }
  if (threadIdx.x == 0) {
    hdr[kFqNewlines] = carry;
    hdr[kFqRecords] = carry >> 2;
  }
}

void launch_fq_scan(const uint8_t* txt, uint32_t len, uint32_t* tile_nl, unsigned long long* hdr,
                    hipStream_t s, uint32_t grid_cap) {
  const uint64_t ntiles = fq_tiles(len);
  if (ntiles) k_fq_tile<<<fq_grid(ntiles, grid_cap), 256, 0, s>>>(txt, len, ntiles, tile_nl);
  k_fq_scan_tiles<<<1, 256, 0, s>>>(ntiles, tile_nl, hdr);
}

// ------------------------------------------------------------------- (b) lines ------------------
// n_lines = 4 * the complete records: only their bytes are checked, only their line starts written
// (line_start: n_lines + 1 entries).
__global__ __launch_bounds__(256) void k_fq_lines(const uint8_t* __restrict__ txt, uint32_t len,
                                                  uint64_t ntiles,
                                                  const uint32_t* __restrict__ tile_nl,
                                                  uint32_t n_lines,
                                                  uint32_t* __restrict__ line_start,
                                                  unsigned long long* __restrict__ hdr) {
  if (blockIdx.x == 0 && threadIdx.x == 0) line_start[0] = 0u;
  uint32_t irr = 0xFFFFFFFFu;  // (an offset is below len <= 2^32 - 1: never all ones)
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const FqLane b = fq_lane(txt, len, t);
    uint32_t total;
    const uint32_t ex = block_excl_scan_256((uint32_t)__popc(b.nl), &total);
    uint32_t l = tile_nl[t] + ex;  // newlines before the lane's bytes = the line of its first byte
    uint32_t rest = b.valid;       // the lane's bytes not yet walked
    uint32_t bad = 0;
    // the lane's bytes line by line: a segment ends with its newline, or with the lane's bytes
    while (rest && l < n_lines) {
      const uint32_t upto = b.nl & rest;  // (bit of the segment's newline, if the lane holds it)
      const uint32_t end_bit = upto ? (upto & (0u - upto)) : 0u;
      const uint32_t seg = end_bit ? (rest & ((end_bit << 1) - 1u)) : rest;
      const uint32_t body = seg & ~b.nl;
      switch (l & 3u) {
        case 0u: bad |= seg & b.first & ~b.at; break;
        case 1u: bad |= body & ~b.l1ok; break;
        case 2u: bad |= (seg & b.first & ~b.plus) | (body & ~b.first & b.hi); break;
        default: bad |= body & ~b.l3ok; break;
      }
      if (end_bit) line_start[++l] = b.pos + (uint32_t)__builtin_ctz(end_bit) + 1u;  // (l <= n_lines)
      rest &= ~seg;
    }
    if (bad) irr = min(irr, b.pos + (uint32_t)__builtin_ctz(bad));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) irr = min(irr, (uint32_t)__shfl_xor(irr, o, 64));
  if ((threadIdx.x & 63u) == 0 && irr != 0xFFFFFFFFu)
    atomicMin(&hdr[kFqIrregular], (unsigned long long)irr);
}

void launch_fq_lines(const uint8_t* txt, uint32_t len, const uint32_t* tile_nl, uint32_t n_records,
                     uint32_t* line_start, unsigned long long* hdr, hipStream_t s,
                     uint32_t grid_cap) {
  const uint64_t ntiles = fq_tiles(len);
  k_fq_lines<<<fq_grid(ntiles, grid_cap), 256, 0, s>>>(txt, len, ntiles, tile_nl, 4u * n_records,
                                                      line_start, hdr);
}

// ------------------------------------------------------------------- (c) records ----------------
// len(L1) of record r, and the offset that a quality line of another length makes irregular
__device__ __forceinline__ uint32_t fq_record_len(const uint32_t* __restrict__ line_start,
                                                  uint32_t r, uint32_t* mismatch_at) {
  const uint32_t s1 = line_start[4u * r + 1u], s2 = line_start[4u * r + 2u];
  const uint32_t s3 = line_start[4u * r + 3u], s4 = line_start[4u * r + 4u];
  const uint32_t l1 = s2 - s1 - 1u, l3 = s4 - s3 - 1u;
  *mismatch_at = l1 == l3 ? 0xFFFFFFFFu : s3 + min(l1, l3);
  return l1;
}

__global__ __launch_bounds__(256) void k_fq_records(const uint32_t* __restrict__ line_start,
                                                    uint32_t n, uint64_t ntiles,
                                                    uint32_t* __restrict__ rec_sum,
                                                    unsigned long long* __restrict__ hdr) {
  uint32_t irr = 0xFFFFFFFFu;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t r = t * kFqRecTile + threadIdx.x;
    uint32_t len = 0, at = 0xFFFFFFFFu;
    if (r < n) len = fq_record_len(line_start, (uint32_t)r, &at);
    irr = min(irr, at);
    uint32_t total;
    block_excl_scan_256(len, &total);  // (the lengths' sum is below the chunk's: 32 bits hold it)
    if (threadIdx.x == 0) rec_sum[t] = total;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) irr = min(irr, (uint32_t)__shfl_xor(irr, o, 64));
  if ((threadIdx.x & 63u) == 0 && irr != 0xFFFFFFFFu)
    atomicMin(&hdr[kFqIrregular], (unsigned long long)irr);
}

// One workgroup: rec_sum[t] = the bases of the record tiles below t; the bases of all.
__global__ __launch_bounds__(256) void k_fq_scan_records(uint32_t* __restrict__ rec_sum,
                                                         uint64_t ntiles,
                                                         unsigned long long* __restrict__ hdr) {
  uint32_t carry = 0;
  for (uint64_t t0 = 0; t0 < ntiles; t0 += 256) {
    const uint64_t t = t0 + threadIdx.x;
    const uint32_t v = t < ntiles ? rec_sum[t] : 0u;
    uint32_t total;
    const uint32_t p = block_excl_scan_256(v, &total);
    if (t < ntiles) rec_sum[t] = carry + p;
    carry += total;
  }
  if (threadIdx.x == 0) hdr[kFqBases] = carry;
}

__global__ __launch_bounds__(256) void k_fq_offsets(const uint32_t* __restrict__ line_start,
                                                    const uint32_t* __restrict__ rec_sum, uint32_t n,
                                                    uint64_t ntiles,
                                                    unsigned long long* __restrict__ hdr,
                                                    uint64_t* __restrict__ off) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    off[n] = hdr[kFqBases];
    hdr[kFqConsumed] = line_start[4u * n];
  }
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t r = t * kFqRecTile + threadIdx.x;
    uint32_t len = 0, at;
    if (r < n) len = fq_record_len(line_start, (uint32_t)r, &at);
    uint32_t total;
    const uint32_t p = block_excl_scan_256(len, &total);
    if (r < n) off[r] = (uint64_t)(rec_sum[t] + p);
  }
}

void launch_fq_records(const uint32_t* line_start, uint32_t n_records, uint32_t* rec_sum,
                       uint64_t* off, unsigned long long* hdr, hipStream_t s, uint32_t grid_cap) {
  const uint64_t ntiles = fq_record_tiles(n_records);
  if (ntiles)
    k_fq_records<<<fq_grid(ntiles, grid_cap), 256, 0, s>>>(line_start, n_records, ntiles, rec_sum, hdr);
  k_fq_scan_records<<<1, 256, 0, s>>>(rec_sum, ntiles, hdr);
  k_fq_offsets<<<fq_grid(ntiles, grid_cap), 256, 0, s>>>(line_start, rec_sum, n_records, ntiles, hdr, off);
}

// ------------------------------------------------------------------- (d) pack -------------------
// One wave per record (4 per workgroup), 64 bytes a trip, a byte per lane from an unaligned source
// to an unaligned destination: the place to widen (dword copies after an alignment prologue) if the
// parser's time ever shows; all its launches are 1.7 ms for 640 MB.  Nothing is copied once the chunk is
// known to be irregular (the host reader takes it), and a record's source and destination are held
// inside the text and the buffer whatever the line starts say.
__global__ __launch_bounds__(256) void k_fq_pack(const uint8_t* __restrict__ txt, uint32_t text_len,
                                                 const uint32_t* __restrict__ line_start,
                                                 const uint64_t* __restrict__ off, uint32_t n,
                                                 const unsigned long long* __restrict__ hdr,
                                                 uint8_t* __restrict__ seq, uint64_t seq_bytes) {
  if (hdr[kFqIrregular] != ~0ull) return;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t r = blockIdx.x * 4ull + (threadIdx.x >> 6); r < n; r += (uint64_t)gridDim.x * 4ull) {
    const uint32_t s1 = line_start[4u * (uint32_t)r + 1u];
    const uint32_t len = line_start[4u * (uint32_t)r + 2u] - s1 - 1u;
    const uint64_t o = off[r];
    if (s1 > text_len || len > text_len - s1 || o > seq_bytes || len > seq_bytes - o) continue;
    const uint8_t* src = txt + s1;
    uint8_t* dst = seq + o;
    for (uint32_t i = lane; i < len; i += 64u) dst[i] = src[i];
  }
}

void launch_fq_pack(const uint8_t* txt, uint32_t len, const uint32_t* line_start, const uint64_t* off,
                    uint32_t n_records, const unsigned long long* hdr, uint8_t* seq,
                    uint64_t seq_bytes, hipStream_t s, uint32_t grid_cap) {
  if (n_records == 0) return;
  k_fq_pack<<<stride_grid((uint64_t)n_records * 64u, grid_cap, 8192), 256, 0, s>>>(
      txt, len, line_start, off, n_records, hdr, seq, seq_bytes);
}

}  // namespace klsh
