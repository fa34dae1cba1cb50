// Device code shared by the k-mer table kernels (klsh_kmc.hip, klsh_kcount.hip): a k-mer as a KMC
// value (base 0 in the most significant of its 2k bits, A < C < G < T: kmer_api.h:380-395) and as
// the reference Kmer's 8-byte image (base i at bits 2i, kmer/Kmer.cc:115-135).
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

}  // namespace klsh
