// gfx950 kernels of the device-side result: member offsets by a three-launch scan,
// the member lists flattened by list ranking (pointer jumping, a fixed number of rounds), the
// label of every member node, the singleton state of a load from device memory, and the member
// state of a load of clustered rows (offsets and nodes back into linked lists).  Integer
// bookkeeping only.  Every kernel strides over its index range on its own (no workgroup waits for
// another), so every launch takes option "grid_cap".
#include <hip/hip_runtime.h>

#include "klsh_device.h"

namespace klsh {

namespace {

constexpr uint32_t kResGridMax = 2048;  // workgroups per launch, at most (the rest is strided)

inline uint32_t res_grid(uint64_t items, uint32_t per_group, uint32_t grid_cap) {
  const uint64_t g = (items + per_group - 1) / per_group;
  return cap_grid((uint32_t)std::min<uint64_t>(std::max<uint64_t>(g, 1), kResGridMax), grid_cap);
}

__device__ __forceinline__ uint64_t pack_jd(uint32_t jmp, uint32_t dist) {
  return (uint64_t)jmp | ((uint64_t)dist << 32);
}

// 256-lane maximum (every lane returns it)
__device__ __forceinline__ uint32_t block_max_256(uint32_t v) {
  __shared__ uint32_t wmax[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
  if ((threadIdx.x & 63u) == 0) wmax[threadIdx.x >> 6] = v;
  __syncthreads();
  const uint32_t r = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
  __syncthreads();
  return r;
}

// cnt of live row i (a slot outside the table reads as an empty row and raises the error word)
__device__ __forceinline__ uint32_t live_cnt(const uint32_t* __restrict__ order,
                                             const uint32_t* __restrict__ cnt, uint32_t i,
                                             uint32_t slots, uint32_t* __restrict__ hdr) {
  const uint32_t sl = order[i];
  if (sl >= slots) {
    atomicOr(&hdr[kResErr], kResErrOrder);
    return 0;
  }
  return cnt[sl];
}

}  // namespace

// ------------------------------------------------------------------- (a) member offsets --------
// Tile t holds live rows [t * kResTile, (t + 1) * kResTile), kResItems consecutive rows per lane.
__global__ __launch_bounds__(256) void k_res_tile_sums(const uint32_t* __restrict__ order,
                                                       const uint32_t* __restrict__ cnt,
                                                       uint32_t n, uint32_t slots, uint32_t ntiles,
                                                       uint32_t* __restrict__ tsum,
                                                       uint32_t* __restrict__ tmax,
                                                       uint32_t* __restrict__ hdr) {
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t base = (uint64_t)t * kResTile + threadIdx.x * kResItems;
    uint32_t acc = 0, mx = 0;
#pragma unroll
    for (uint32_t k = 0; k < kResItems; ++k)
      if (base + k < n) {
        const uint32_t c = live_cnt(order, cnt, (uint32_t)(base + k), slots, hdr);
        acc += c;
        mx = max(mx, c);
      }
    uint32_t total;
    block_excl_scan_256(acc, &total);
    mx = block_max_256(mx);
    if (threadIdx.x == 0) {
      tsum[t] = total;
      tmax[t] = mx;
    }
  }
}

// One workgroup: tsum -> its exclusive prefix, hdr[kResTotal] = the sum, hdr[kResMaxCnt] = max.
__global__ __launch_bounds__(256) void k_res_scan_sums(uint32_t* __restrict__ tsum,
                                                       const uint32_t* __restrict__ tmax,
                                                       uint32_t ntiles, uint32_t* __restrict__ hdr) {
  uint32_t carry = 0, mx = 0;
  for (uint32_t t0 = 0; t0 < ntiles; t0 += 256) {
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t v = t < ntiles ? tsum[t] : 0u;
    if (t < ntiles) mx = max(mx, tmax[t]);
    uint32_t total;
    const uint32_t p = block_excl_scan_256(v, &total);
    if (t < ntiles) tsum[t] = carry + p;
    carry += total;
  }
  mx = block_max_256(mx);
  if (threadIdx.x == 0) {
    hdr[kResTotal] = carry;
    hdr[kResMaxCnt] = mx;
  }
}

// off[i] = members of the live rows before i; off[n] = the total.
__global__ __launch_bounds__(256) void k_res_offsets(const uint32_t* __restrict__ order,
                                                     const uint32_t* __restrict__ cnt, uint32_t n,
                                                     uint32_t slots, uint32_t ntiles,
                                                     const uint32_t* __restrict__ tsum,
                                                     uint32_t* __restrict__ off,
                                                     uint32_t* __restrict__ hdr) {
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t base = (uint64_t)t * kResTile + threadIdx.x * kResItems;
    uint32_t c[kResItems];
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t k = 0; k < kResItems; ++k) {
      c[k] = base + k < n ? live_cnt(order, cnt, (uint32_t)(base + k), slots, hdr) : 0u;
      acc += c[k];
    }
    uint32_t total;
    uint32_t run = block_excl_scan_256(acc, &total) + tsum[t];
#pragma unroll
    for (uint32_t k = 0; k < kResItems; ++k) {
      if (base + k < n) {
        off[base + k] = run;
        if (base + k + 1 == n) off[n] = run + c[k];
      }
      run += c[k];
    }
  }
}

void launch_result_offsets(const uint32_t* order, const uint32_t* cnt, uint32_t n, uint32_t slots,
                           uint32_t* tsum, uint32_t* tmax, uint32_t* off, uint32_t* hdr,
                           hipStream_t s, uint32_t grid_cap) {
  if (n == 0) {  // hdr is zero already: no rows, no members
    (void)hipMemsetAsync(off, 0, sizeof(uint32_t), s);
    return;
  }
  const uint32_t ntiles = result_tiles(n);
  const uint32_t g = res_grid(ntiles, 1, grid_cap);
  k_res_tile_sums<<<g, 256, 0, s>>>(order, cnt, n, slots, ntiles, tsum, tmax, hdr);
  k_res_scan_sums<<<1, 256, 0, s>>>(tsum, tmax, ntiles, hdr);
  k_res_offsets<<<g, 256, 0, s>>>(order, cnt, n, slots, ntiles, tsum, off, hdr);
}

// ------------------------------------------------------------------- (b) tails to rows ---------
// rowof[tail of live row i] = i (rowof preset to KLSH_NO_LABEL; an empty row has no tail).
__global__ __launch_bounds__(256) void k_res_rowof(const uint32_t* __restrict__ order,
                                                   const uint32_t* __restrict__ cnt,
                                                   const uint32_t* __restrict__ tail, uint32_t n,
                                                   uint32_t slots, uint32_t members,
                                                   uint32_t* __restrict__ rowof,
                                                   uint32_t* __restrict__ hdr) {
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
    const uint32_t sl = order[i];
    if (sl >= slots || cnt[sl] == 0) continue;  // (a bad slot is reported by the offsets pass)
    const uint32_t t = tail[sl];
    if (t < members)
      rowof[t] = (uint32_t)i;
    else
      atomicOr(&hdr[kResErr], kResErrList);
  }
}

// ------------------------------------------------------------------- (c) list ranking ----------
// st[v] = (jmp, dist): a node dist links behind v on v's chain; a chain's end is a fixed point.
__global__ __launch_bounds__(256) void k_rank_init(const uint32_t* __restrict__ nxt,
                                                   uint32_t members, uint64_t* __restrict__ st,
                                                   uint32_t* __restrict__ hdr) {
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < members; v += stride) {
    const uint32_t nx = nxt[v];
    if (nx == kNil) {
      st[v] = pack_jd((uint32_t)v, 0);
    } else if (nx < members) {
      st[v] = pack_jd(nx, 1);
    } else {  // a link out of the table: the chain ends here, the call fails
      st[v] = pack_jd((uint32_t)v, 0);
      atomicOr(&hdr[kResErr], kResErrList);
    }
  }
}

// One round of pointer jumping: every node's pointer doubles its reach.  Two loads per node,
// whatever its chain's length.
__global__ __launch_bounds__(256) void k_rank_round(const uint64_t* __restrict__ in,
                                                    uint64_t* __restrict__ out, uint32_t members) {
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < members; v += stride) {
    const uint64_t a = in[v];
    const uint64_t b = in[(uint32_t)a];  // (jmp < members: k_rank_init)
    out[v] = pack_jd((uint32_t)b, (uint32_t)(a >> 32) + (uint32_t)(b >> 32));
  }
}

// ------------------------------------------------------------------- (d) emit -----------------
// Node v sits dist links before its chain's end t; the live row i = rowof[t] owns it, at place
// cnt - 1 - dist of its list.  hdr[kResLabelled] += nodes that found a row.
__global__ __launch_bounds__(256) void k_rank_emit(const uint64_t* __restrict__ st,
                                                   const uint32_t* __restrict__ rowof,
                                                   const uint32_t* __restrict__ order,
                                                   const uint32_t* __restrict__ cnt,
                                                   const uint32_t* __restrict__ off,
                                                   uint32_t members, uint32_t n, uint32_t slots,
                                                   uint32_t* __restrict__ labels,
                                                   uint32_t* __restrict__ nodes,
                                                   uint32_t* __restrict__ hdr) {
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  uint32_t found = 0, bad = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < members; v += stride) {
    const uint64_t a = st[v];
    const uint32_t dist = (uint32_t)(a >> 32);
    const uint32_t i = rowof[(uint32_t)a];
    if (labels) labels[v] = i;
    if (i == KLSH_NO_LABEL) continue;
    ++found;
    const uint32_t sl = i < n ? order[i] : slots;
    const uint32_t c = sl < slots ? cnt[sl] : 0u;
    if (dist >= c) {
      bad = 1;
      continue;
    }
    if (nodes) nodes[off[i] + (c - 1 - dist)] = (uint32_t)v;
  }
  uint32_t total;
  block_excl_scan_256(found, &total);
  if (threadIdx.x == 0 && total) atomicAdd(&hdr[kResLabelled], total);
  if (bad) atomicOr(&hdr[kResErr], kResErrList);
}

void launch_result_rowof(const uint32_t* order, const uint32_t* cnt, const uint32_t* tail,
                         uint32_t n, uint32_t slots, uint32_t members, uint32_t* rowof,
                         uint32_t* hdr, hipStream_t s, uint32_t grid_cap) {
  if (members == 0) return;
  (void)hipMemsetAsync(rowof, 0xFF, sizeof(uint32_t) * (size_t)members, s);
  if (n) k_res_rowof<<<res_grid(n, 256, grid_cap), 256, 0, s>>>(order, cnt, tail, n, slots, members,
                                                                rowof, hdr);
}

const uint64_t* launch_list_rank(const uint32_t* nxt, uint32_t members, uint32_t rounds,
                                 uint64_t* st0, uint64_t* st1, uint32_t* hdr, hipStream_t s,
                                 uint32_t grid_cap, hipEvent_t after_init) {
  const uint32_t g = res_grid(members, 256, grid_cap);
  if (members) k_rank_init<<<g, 256, 0, s>>>(nxt, members, st0, hdr);
  if (after_init) (void)hipEventRecord(after_init, s);
  if (members == 0) return st0;
  uint64_t *in = st0, *out = st1;
  for (uint32_t r = 0; r < rounds; ++r) {
    k_rank_round<<<g, 256, 0, s>>>(in, out, members);
    std::swap(in, out);
  }
  return in;
}

void launch_result_emit(const uint64_t* st, const uint32_t* rowof, const uint32_t* order,
                        const uint32_t* cnt, const uint32_t* off, uint32_t members, uint32_t n,
                        uint32_t slots, uint32_t* labels, uint32_t* nodes, uint32_t* hdr,
                        hipStream_t s, uint32_t grid_cap) {
  if (members == 0) return;
  k_rank_emit<<<res_grid(members, 256, grid_cap), 256, 0, s>>>(st, rowof, order, cnt, off, members,
                                                               n, slots, labels, nodes, hdr);
}

// ------------------------------------------------------------------- (e) singleton setup -------
// The member state of n rows loaded as singletons: row i is slot i, live, its own only member.
__global__ __launch_bounds__(256) void k_init_singletons(uint32_t* __restrict__ cnt,
                                                         uint32_t* __restrict__ head,
                                                         uint32_t* __restrict__ tail,
                                                         uint32_t* __restrict__ order,
                                                         uint32_t* __restrict__ nxt, uint32_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
    cnt[i] = 1;
    head[i] = tail[i] = order[i] = (uint32_t)i;
    nxt[i] = kNil;
  }
}

void launch_init_singletons(const Rows& r, uint32_t* order, uint32_t n, hipStream_t s,
                            uint32_t grid_cap) {
  if (n)
    k_init_singletons<<<res_grid(n, 256, grid_cap), 256, 0, s>>>(r.cnt, r.head, r.tail, order,
                                                                 r.nxt, n);
}

// ------------------------------------------------------------------- (f) clustered load --------
// The list ranking run backwards (klsh_load_clusters_device): n + 1 member offsets and a flat
// node array in, cnt / head / tail / nxt out.  Entry q is entry off[0] + q of the caller's node
// array (`nodes` points at it; null: entry q is node q).  The two checking kernels write only the
// call's scratch; the two linking kernels run after the host has read the error word.
namespace {

// *err = the smallest (index << 2 | kind) reported: what the host names never depends on which
// lane got there first
__device__ __forceinline__ void lc_report(unsigned long long* err, uint64_t index, uint32_t kind) {
  atomicMin(err, (unsigned long long)(index << 2 | kind));
}

}  // namespace

// Over rows: off[i] < off[i + 1], and start[off[i] - off[0]] = 1 (start: m bytes, zeroed, or null
// when the end points alone rule the load out; an offset outside [off[0], off[0] + m) marks
// nothing, and the row before or after it is reported).
__global__ __launch_bounds__(256) void k_lc_check_rows(const uint32_t* __restrict__ off, uint32_t n,
                                                       uint32_t m, uint8_t* __restrict__ start,
                                                       unsigned long long* __restrict__ err) {
  const uint32_t base = off[0];
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
    const uint32_t a = off[i], b = off[i + 1];
    if (b <= a)
      lc_report(err, i, kLcErrOffsets);
    else if (start && a >= base && a - base < m)
      start[a - base] = 1;
  }
}

// Over entries: node < members, and no node twice.  owner[v] (preset to kNil) ends as the first
// entry that lists v.  Of the entries listing one node, every atomicMin but the first to arrive
// sees an earlier arrival, and the larger of the two is a repeat; whatever the order, the second
// smallest entry is reported (when it arrives after the smallest, or the smallest after it) and
// the smallest never is.
__global__ __launch_bounds__(256) void k_lc_check_nodes(const uint32_t* __restrict__ nodes,
                                                        uint32_t m, uint32_t members,
                                                        uint32_t* __restrict__ owner,
                                                        unsigned long long* __restrict__ err) {
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < m; q += stride) {
    const uint32_t v = nodes[q];
    if (v >= members) {
      lc_report(err, q, kLcErrRange);
      continue;
    }
    const uint32_t seen = atomicMin(&owner[v], (uint32_t)q);
    if (seen != kNil) lc_report(err, max(seen, (uint32_t)q), kLcErrTwice);
  }
}

// Over entries: the node of entry q links to the node of entry q + 1 unless that entry starts the
// next list (nxt preset to kNil, which is what the nodes in no list keep).  No entry needs its row.
__global__ __launch_bounds__(256) void k_lc_link(const uint32_t* __restrict__ nodes,
                                                 const uint8_t* __restrict__ start, uint32_t m,
                                                 uint32_t* __restrict__ nxt) {
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < m; q += stride) {
    const uint32_t v = nodes ? nodes[q] : (uint32_t)q;
    uint32_t nx = kNil;
    if (q + 1 < m && !start[q + 1]) nx = nodes ? nodes[q + 1] : (uint32_t)(q + 1);
    nxt[v] = nx;
  }
}

// Over rows: row i is slot i, live, with the count and the two ends of its list.
__global__ __launch_bounds__(256) void k_lc_rows(const uint32_t* __restrict__ off,
                                                 const uint32_t* __restrict__ nodes, uint32_t n,
                                                 uint32_t* __restrict__ cnt,
                                                 uint32_t* __restrict__ head,
                                                 uint32_t* __restrict__ tail,
                                                 uint32_t* __restrict__ order) {
  const uint32_t base = off[0];
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
    const uint32_t a = off[i] - base, b = off[i + 1] - base;  // (a < b <= m: checked)
    cnt[i] = b - a;
    head[i] = nodes ? nodes[a] : a;
    tail[i] = nodes ? nodes[b - 1] : b - 1;
    order[i] = (uint32_t)i;
  }
}

void launch_clusters_check_rows(const uint32_t* off, uint32_t n, uint32_t m, uint8_t* start,
                                unsigned long long* err, hipStream_t s, uint32_t grid_cap) {
  if (n) k_lc_check_rows<<<res_grid(n, 256, grid_cap), 256, 0, s>>>(off, n, m, start, err);
}

void launch_clusters_check_nodes(const uint32_t* nodes, uint32_t m, uint32_t members,
                                 uint32_t* owner, unsigned long long* err, hipStream_t s,
                                 uint32_t grid_cap) {
  if (m) k_lc_check_nodes<<<res_grid(m, 256, grid_cap), 256, 0, s>>>(nodes, m, members, owner, err);
}

void launch_clusters_link(const Rows& r, uint32_t* order, const uint32_t* off,
                          const uint32_t* nodes, const uint8_t* start, uint32_t n, uint32_t m,
                          uint32_t members, hipStream_t s, uint32_t grid_cap) {
  if (members) (void)hipMemsetAsync(r.nxt, 0xFF, sizeof(uint32_t) * (size_t)members, s);
  if (n == 0) return;
  k_lc_link<<<res_grid(m, 256, grid_cap), 256, 0, s>>>(nodes, start, m, r.nxt);
  k_lc_rows<<<res_grid(n, 256, grid_cap), 256, 0, s>>>(off, nodes, n, r.cnt, r.head, r.tail, order);
}

}  // namespace klsh
