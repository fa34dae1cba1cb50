// Mode K on gfx950: counting the canonical k-mers of a sample's reads, what the reference leaves to
// the external `kmc -k<K> -r -cs65535 -ci<C>` (io/ioHT.cc:100-103).
//
// A k-mer is its KMC value (base 0 most significant, A < C < G < T); the canonical one is the
// smaller of the window and its reverse complement.  A character that is not one of ACGTacgt breaks
// the read: no window spans it (KMC's rule; k_check_reads' "anything else is A" is another rule).
//
//   k_kcount_reads    one wave per read: the read's base codes staged in LDS in windows (one byte
//                     each, 4 = break), one lane per k-mer position building its value from LDS;
//                     equal keys of neighbouring lanes (a homopolymer or short-period run) are
//                     combined, and the first lane of a run probes the k-mer table (klsh_kmer.h)
//                     and adds the run's length to the slot's 32-bit count
//   k_kcount_rehash   keys and counts into a table of twice the slots (between batches)
//   k_ktab_collect<ByValue>  slots with count >= count_min -> (low word of the value, slot)
//   k_kcount_emit     the listing in sorted order: value, rep image, min(count, 65535)
//   k_kmcdb_pack      a chunk of the listing as the records of a KMC1-layout .kmc_suf
//   k_kmcdb_lut       the .kmc_pre prefix table: per prefix, the records below it (binary search)
//
// The count word never wraps: a lane adds only while the count it sees is below 65535, so a slot
// ends at most one in-flight add per wave above that (each at most 64), and every slot below
// 65535 is exact.  The same test bounds the same-address adds of a poly-A read: after 65535 its
// lanes only read.
//
// Bound: the probes, as in mode E — one random 8-B key access (and one 4-B count add) per run of
// equal k-mers; the sequence is read once.  A sample's table is far larger than mode E's set, so
// the accesses go to HBM, not L2.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "klsh_internal.h"
#include "klsh_kmer.h"

namespace klsh {

constexpr int kKcWaves = 4;  // waves per workgroup, each on its own reads

__device__ __forceinline__ uint32_t kc_code(uint32_t c) {
  c |= 0x20u;  // the lower-case letter; no other character maps onto a, c, g, t
  return c == 'a' ? 0u : c == 'c' ? 1u : c == 'g' ? 2u : c == 't' ? 3u : 4u;
}

// ctr[0] += slots claimed, ctr[1] += valid k-mer windows (one add per wave and counter)
__global__ __launch_bounds__(256) void k_kcount_reads(const uint8_t* __restrict__ seq,
                                                      const uint64_t* __restrict__ off, uint64_t n,
                                                      int k, unsigned long long* keys,
                                                      uint32_t* cnt, uint64_t mask,
                                                      unsigned long long* ctr) {
  __shared__ uint8_t codes[kKcWaves][kKcountWindow + 64];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint8_t* cw = codes[wv];
  const uint64_t waves = (uint64_t)gridDim.x * kKcWaves;
  uint32_t n_new = 0, n_pos = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * kKcWaves + wv; r < n; r += waves) {  // wave-uniform
    const uint64_t a = off[r];
    const uint64_t len = off[r + 1] - a;
    if (len < (uint64_t)k) continue;
    const uint64_t npos = len - (uint64_t)k + 1u;
    for (uint64_t w0 = 0; w0 < npos; w0 += kKcountWindow) {
      const uint32_t np = (uint32_t)(npos - w0 < kKcountWindow ? npos - w0 : kKcountWindow);
      const uint32_t nb = np + (uint32_t)k - 1u;  // bases of the window (<= kKcountWindow + 31)
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      for (uint32_t q = lane; q < nb; q += 64u) cw[q] = (uint8_t)kc_code(seq[a + w0 + q]);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      for (uint32_t p0 = 0; p0 < np; p0 += 64u) {  // wave-uniform: the lanes stay together
        const uint32_t p = p0 + lane;
        uint64_t v = 0;
        uint32_t brk = p < np ? 0u : 4u;
        if (p < np)
          for (int i = 0; i < k; ++i) {
            const uint32_t c = cw[p + (uint32_t)i];
            brk |= c;
            v = (v << 2) | (uint64_t)(c & 3u);
          }
        const bool valid = brk < 4u;
        const uint64_t key = valid ? kmc_canonical(v, k) : kKtabEmpty;
        // runs of equal keys in neighbouring lanes: the first lane adds the run's length
        const uint64_t prev = __shfl_up((unsigned long long)key, 1, 64);
        const bool head = valid && (lane == 0u || key != prev);
        const uint64_t hm = __ballot(head), vm = __ballot(valid);
        n_pos += valid ? 1u : 0u;
        if (head) {
          const uint64_t stop = (hm | ~vm) & ~((2ull << lane) - 1ull);  // next head or break above
          const uint32_t run = (stop ? (uint32_t)__builtin_ctzll(stop) : 64u) - lane;
          uint32_t fresh = 0;
          const uint64_t h = ktab_claim_read(keys, mask, key, &fresh);
          n_new += fresh;
          if (__hip_atomic_load(&cnt[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 65535u)
            atomicAdd(&cnt[h], run);
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_new += __shfl_xor(n_new, o, 64);
    n_pos += __shfl_xor(n_pos, o, 64);
  }
  if (lane == 0) {
    if (n_new) atomicAdd(&ctr[0], (unsigned long long)n_new);
    if (n_pos) atomicAdd(&ctr[1], (unsigned long long)n_pos);
  }
}

__global__ __launch_bounds__(256) void k_kcount_rehash(const uint64_t* __restrict__ okeys,
                                                       const uint32_t* __restrict__ ocnt,
                                                       uint64_t ocap, unsigned long long* keys,
                                                       uint32_t* __restrict__ cnt, uint64_t mask) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < ocap; i += (uint64_t)gridDim.x * 256ull) {
    const uint64_t key = okeys[i];
    if (key == kKtabEmpty) continue;
    uint32_t fresh = 0;
    const uint64_t h = ktab_claim_read(keys, mask, key, &fresh);
    cnt[h] = ocnt[i];  // the old table holds a key once
  }
}

// k_ktab_collect's selection of mode K: the slots counted count_min times at least, by KMC value
struct ByValue {
  const uint32_t* cnt;
  uint32_t count_min;
  __device__ bool take(uint64_t i) const { return cnt[i] >= count_min; }
  __device__ uint32_t low(uint64_t, uint64_t key) const { return (uint32_t)key; }
};

__global__ __launch_bounds__(256) void k_kcount_emit(const uint64_t* __restrict__ keys,
                                                     const uint32_t* __restrict__ cnt,
                                                     const uint32_t* __restrict__ order, uint64_t n,
                                                     int k, uint64_t* __restrict__ val,
                                                     uint64_t* __restrict__ rep,
                                                     uint32_t* __restrict__ out_cnt) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256ull) {
    const uint32_t s = order[i];
    const uint64_t v = keys[s];
    val[i] = v;
    rep[i] = kmc_value_rep(v, k);  // klsh_kmer.h, shared with mode B's record decode
    out_cnt[i] = min(cnt[s], 65535u);
  }
}

// Records [r0, r0 + m) of a listing as the record bytes of a KMC1-layout .kmc_suf chunk: `suf`
// suffix bytes (the low 8 suf bits of the value, most significant byte first), then the counter
// in 2 bytes, little-endian.  A workgroup takes tiles of 256 records: each lane builds its record
// in the LDS byte tile at lane * rec, and the tile (256 rec bytes, a multiple of 4; `out` is
// 4-byte aligned) leaves as coalesced dword stores, the chunk's last partial tile's odd bytes as
// byte stores.  Both loads are issued, on a clamped index, before the first LDS write.
__global__ __launch_bounds__(256) void k_kmcdb_pack(const uint64_t* __restrict__ val,
                                                    const uint32_t* __restrict__ cnt, uint64_t r0,
                                                    uint64_t m, uint32_t suf,
                                                    uint8_t* __restrict__ out) {
  __shared__ uint32_t tile[256 * kKmcdbMaxRec / 4];
  uint8_t* tb = reinterpret_cast<uint8_t*>(tile);
  const uint32_t rec = suf + 2u, lane = threadIdx.x;
  for (uint64_t base = blockIdx.x * 256ull; base < m; base += (uint64_t)gridDim.x * 256ull) {
    const uint32_t nrec = (uint32_t)(m - base < 256u ? m - base : 256u);
    const uint64_t i = r0 + base + (lane < nrec ? lane : nrec - 1u);  // in range for every lane
    const uint64_t v = val[i];
    const uint32_t c = cnt[i];
    __syncthreads();  // the previous tile has been read out
    uint8_t* q = tb + lane * rec;
    for (uint32_t b = 0; b < suf; ++b) q[b] = (uint8_t)(v >> (8u * (suf - 1u - b)));
    q[suf] = (uint8_t)c;
    q[suf + 1u] = (uint8_t)(c >> 8);
    __syncthreads();
    const uint32_t nbytes = nrec * rec, nd = nbytes >> 2;
    uint8_t* o = out + base * rec;
    uint32_t* od = reinterpret_cast<uint32_t*>(o);
    for (uint32_t d = lane; d < nd; d += 256u) od[d] = tile[d];
    for (uint32_t b = (nd << 2) + lane; b < nbytes; b += 256u) o[b] = tb[b];
  }
}

// lut[i] = the number of listed values below prefix q0 + i, i.e. the lower bound of
// (q0 + i) << shift in val[0, n) (ascending); shift = 2 (k - p), 64 when k = 32 and p = 0 (the one
// prefix 0, whose bound is 0).  An empty listing gives zeros.
__global__ __launch_bounds__(256) void k_kmcdb_lut(const uint64_t* __restrict__ val, uint64_t n,
                                                   uint64_t q0, uint64_t mq, uint32_t shift,
                                                   uint64_t* __restrict__ lut) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < mq; i += (uint64_t)gridDim.x * 256ull) {
    const uint64_t key = shift >= 64u ? 0ull : (q0 + i) << shift;
    uint64_t lo = 0, len = n;
    while (len) {
      const uint64_t half = len >> 1;
      if (val[lo + half] < key) {
        lo += half + 1u;
        len -= half + 1u;
      } else {
        len = half;
      }
    }
    lut[i] = lo;
  }
}

void launch_kcount_reads(const uint8_t* seq, const uint64_t* off, uint64_t n, int k, uint64_t* keys,
                         uint32_t* cnt, uint64_t mask, uint64_t* ctr, hipStream_t s,
                         uint32_t grid_cap) {
  if (n == 0) return;
  // at most 4096 workgroups: each wave ends with two adds to ctr
  const uint64_t w = (n + kKcWaves - 1) / kKcWaves, g = w < 4096 ? w : 4096;
  k_kcount_reads<<<cap_grid((uint32_t)g, grid_cap), 64 * kKcWaves, 0, s>>>(
      seq, off, n, k, reinterpret_cast<unsigned long long*>(keys), cnt, mask,
      reinterpret_cast<unsigned long long*>(ctr));
}
void launch_kcount_rehash(const uint64_t* okeys, const uint32_t* ocnt, uint64_t ocap, uint64_t* keys,
                          uint32_t* cnt, uint64_t mask, hipStream_t s, uint32_t grid_cap) {
  k_kcount_rehash<<<stride_grid(ocap, grid_cap), 256, 0, s>>>(okeys, ocnt, ocap,
                                                          reinterpret_cast<unsigned long long*>(keys),
                                                          cnt, mask);
}
void launch_kcount_collect(const uint64_t* keys, const uint32_t* cnt, uint64_t cap,
                           uint32_t count_min, uint32_t* lo, uint32_t* slot, uint32_t* n_out,
                           hipStream_t s, uint32_t grid_cap) {
  k_ktab_collect<<<stride_grid(cap, grid_cap), 256, 0, s>>>(keys, ByValue{cnt, count_min}, cap, lo,
                                                            slot, n_out);
}
void launch_kcount_emit(const uint64_t* keys, const uint32_t* cnt, const uint32_t* order, uint64_t n,
                        int k, uint64_t* val, uint64_t* rep, uint32_t* out_cnt, hipStream_t s,
                        uint32_t grid_cap) {
  if (n)
    k_kcount_emit<<<stride_grid(n, grid_cap), 256, 0, s>>>(keys, cnt, order, n, k, val, rep, out_cnt);
}
void launch_kmcdb_pack(const uint64_t* val, const uint32_t* cnt, uint64_t r0, uint64_t m,
                       uint32_t sufix_size, uint8_t* out, hipStream_t s, uint32_t grid_cap) {
  if (m) k_kmcdb_pack<<<stride_grid(m, grid_cap), 256, 0, s>>>(val, cnt, r0, m, sufix_size, out);
}
void launch_kmcdb_lut(const uint64_t* val, uint64_t n, uint64_t q0, uint64_t mq, int k, int p,
                      uint64_t* lut, hipStream_t s, uint32_t grid_cap) {
  if (mq)
    k_kmcdb_lut<<<stride_grid(mq, grid_cap), 256, 0, s>>>(val, n, q0, mq, (uint32_t)(2 * (k - p)), lut);
}

}  // namespace klsh
