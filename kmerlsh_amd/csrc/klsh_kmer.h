// Device code shared by the k-mer kernels of modes E, B and K (klsh_extract.hip, klsh_kmc.hip,
// klsh_kcount.hip): the k-mer encodings and the one open-addressing table all three keep.
//
// A k-mer is a KMC value (base 0 in the most significant of its 2k bits, A < C < G < T:
// kmer_api.h:380-395) in modes B and K, and the reference Kmer's 8-byte image (base i at bits 2i,
// kmer/Kmer.cc:115-135) where the reference's own order or bytes matter.  Mode E works on images
// throughout, so its revcomp / base_code stay in klsh_extract.hip: reverse_bases below reverses a
// word of either encoding, but kmc_value_rep and kmc_canonical take KMC values only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace klsh {

__device__ __forceinline__ uint64_t kmer_mask(int k) {
  return k == 32 ? ~0ull : ((1ull << (2 * k)) - 1ull);
}

// the k bases of v (bits [0, 2k)) in reverse order
__device__ __forceinline__ uint64_t reverse_bases(uint64_t v, int k) {
  uint64_t x = v;
  x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
  x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
  x = __builtin_bswap64(x);
  return x >> (64 - 2 * k);
}

// KMC value -> Kmer image -> the reference's canonical form rep = (km < twin) ? km : twin in
// memcmp order (kmer/Kmer.cc:76-187); this may be the other strand than KMC's canonical one
__device__ __forceinline__ uint64_t kmc_value_rep(uint64_t v, int k) {
  const uint64_t img = reverse_bases(v, k);  // base i at bits 2i
  // the twin's base i is the complement of base k-1-i: exactly the complemented KMC value
  const uint64_t tw = ~v & kmer_mask(k);
  return __builtin_bswap64(img) < __builtin_bswap64(tw) ? img : tw;
}

// KMC's canonical k-mer: the smaller of the value and its reverse complement's value
__device__ __forceinline__ uint64_t kmc_canonical(uint64_t v, int k) {
  const uint64_t rc = reverse_bases(~v & kmer_mask(k), k);
  return v < rc ? v : rc;
}

// ---- the k-mer table ---------------------------------------------------------------------------
// 64-bit keys in `mask + 1` slots (a power of two >= 1024, at most half full), linear probing from
// kmer_hash(key) & mask.  All ones marks an empty slot: it is never a canonical k-mer in either
// encoding, because the all-T k-mer's reverse complement is 0, which is smaller.
constexpr uint64_t kKtabEmpty = ~0ull;

__host__ __device__ __forceinline__ uint64_t kmer_hash(uint64_t k) {  // murmur3 finalizer
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// the slot of `key`, all ones if it is absent; ktab_find<false> only says whether it is there (a
// bool, so that the probe loop carries no slot out: mode E's loop as it was measured)
template <bool kSlot = true>
__device__ __forceinline__ auto ktab_find(const uint64_t* tab, uint64_t mask, uint64_t key) {
  uint64_t h = kmer_hash(key) & mask;
  while (true) {
    const uint64_t t = tab[h];
    if (t == key) {
      if constexpr (kSlot) return h;
      else return true;
    }
    if (t == kKtabEmpty) {
      if constexpr (kSlot) return kKtabEmpty;
      else return false;
    }
    h = (h + 1) & mask;
  }
}

// the slot of `key`, claimed if absent: a CAS on every slot probed
__device__ __forceinline__ uint64_t ktab_claim(unsigned long long* tab, uint64_t mask,
                                               uint64_t key) {
  uint64_t h = kmer_hash(key) & mask;
  while (true) {
    const unsigned long long prev = atomicCAS(&tab[h], (unsigned long long)kKtabEmpty,
                                              (unsigned long long)key);
    if (prev == kKtabEmpty || prev == key) return h;
    h = (h + 1) & mask;
  }
}

// the same (*fresh = 1 when this call claimed the slot), for tables whose keys are mostly there
// already: a key never changes once set, so a read of it settles the probe without an atomic
__device__ __forceinline__ uint64_t ktab_claim_read(unsigned long long* tab, uint64_t mask,
                                                    uint64_t key, uint32_t* fresh) {
  uint64_t h = kmer_hash(key) & mask;
  while (true) {
    unsigned long long t = __hip_atomic_load(&tab[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == kKtabEmpty) {
      t = atomicCAS(&tab[h], (unsigned long long)kKtabEmpty, (unsigned long long)key);
      if (t == kKtabEmpty) {
        *fresh = 1u;
        return h;
      }
    }
    if (t == key) return h;
    h = (h + 1) & mask;
  }
}

// The occupied slots i of a table that sel.take(i) accepts, compacted into (sel.low(i, key),
// slot) with one add to *n_out per wave, not per entry (a single counter).  Modes B and K order
// the collected slots by a 64-bit word of which `low` is the low half (order_slots_u64).
// cap is a power of two >= 1024: every wave's 64 lanes are in or out of range together.
template <class Sel>
__global__ __launch_bounds__(256) void k_ktab_collect(const uint64_t* __restrict__ tab, Sel sel,
                                                      uint64_t cap,
                                                      uint32_t* __restrict__ lo,
                                                      uint32_t* __restrict__ slot,
                                                      uint32_t* __restrict__ n_out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t below = lane ? (~0ull >> (64u - lane)) : 0ull;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * 256ull) {
    const uint64_t key = tab[i];
    const bool take = key != kKtabEmpty && sel.take(i);
    const uint64_t m = __ballot(take);
    if (!m) continue;
    uint32_t base = 0;
    if (lane == (uint32_t)__builtin_ctzll(m)) base = atomicAdd(n_out, (uint32_t)__popcll(m));
    base = __shfl(base, (int)__builtin_ctzll(m), 64);
    if (take) {
      const uint32_t o = base + (uint32_t)__popcll(m & below);
      lo[o] = sel.low(i, key);
      slot[o] = (uint32_t)i;
    }
  }
}

}  // namespace klsh
