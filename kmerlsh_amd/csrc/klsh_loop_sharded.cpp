// The sharded loop and the klsh_comm_* entry points that bind a context to a
// group.
//
// Every rank holds a replica of the rows; the canonical order of iteration t is the concatenation
// over ranks of each rank's survivors ("mine").  Per iteration:
//   project mine -> keys; bin histogram (top <= 12 key bits) -> allgather -> every rank derives
//   the same bin -> rank ownership (contiguous key ranges balanced by rows) and send counts;
//   stable partition of (key, slot) by owner -> all-to-all-v -> received pairs are in canonical
//   order restricted to this rank's key range; stable radix sort by key = merge_hashtable's
//   bucket order for those keys; greedy merge + compaction -> the new "mine"; the survivors a
//   merge rewrote are broadcast (allgather-v of rows + metadata) so every replica stays identical.
// The host waits twice per iteration, for the send counts and for every rank's counters, both
// published into mapped memory (k_publish_words) and polled (Comm::wait_flag).
// Oversize buckets (nestedCluster) draw hyperplanes in ascending bucket order, i.e. rank order
// then local order: a small allgather of (runs, hyperplanes) gives each rank its RNG offset.
// Member links are written only by the rank that merged them; the end of the call combines them
// with an element-wise min (an unwritten link is kNil = 0xFFFFFFFF) and gathers the global order.
// Below shard_min_rows live rows every rank runs the rest on its replica (run_single).
#include <string.h>

#include <algorithm>
#include <numeric>

#include "klsh_loop.h"

namespace klsh {

static int cluster_sharded_body(klsh_ctx* ctx, float min_similarity, int iterations,
                                int run_iters, int bucket_size_threshold, uint32_t seed_base,
                                uint64_t* rng_counter, uint64_t* nt_trace, klsh_stats* st) {
  Comm* cm = ctx->comm;
  const int W = cm->world, g = cm->rank;
  hipStream_t s = ctx->stream;
  if (int e = ctx->reserve_shard()) return e;
  auto comm_fail = [&](const char* what) {
    return fail(KLSH_E_HIP, std::string(what) + ": " + cm->err);
  };
  const double t_start = now_ms();
  double t_comm = 0.0;
  auto timed_comm = [&](auto fn) {
    const double t0 = now_ms();
    const int rc = fn();
    t_comm += now_ms() - t0;
    return rc;
  };

  const float max_similarity = 0.95f;  // cluster.cc:190-192 (all float)
  const float sim_step = (max_similarity - min_similarity) / (float)iterations;
  float threshold = max_similarity;

  // my block of the global canonical order
  uint64_t N = ctx->n_live;
  uint32_t n_g = 0;
  {
    const uint64_t lo = N * (uint64_t)g / (uint64_t)W, hi = N * (uint64_t)(g + 1) / (uint64_t)W;
    n_g = (uint32_t)(hi - lo);
    if (n_g) KLSH_HIP(hipMemcpyAsync(ctx->alt, ctx->order + lo, 4ull * n_g, hipMemcpyDeviceToDevice, s));
    std::swap(ctx->order, ctx->alt);
  }
  std::vector<uint32_t> n_all(W, 0);  // survivors per rank after the last exchange
  for (int r = 0; r < W; ++r)
    n_all[r] = (uint32_t)(N * (uint64_t)(r + 1) / W - N * (uint64_t)r / W);
  // every rank's block of the order, gathered into ctx->order
  auto gather_order = [&]() -> int {
    std::vector<size_t> cnt(W), off(W);
    size_t acc = 0;
    for (int r = 0; r < W; ++r) {
      cnt[r] = 4ull * n_all[r];
      off[r] = acc;
      acc += cnt[r];
    }
    if (timed_comm([&] { return cm->allgatherv(ctx->order, ctx->alt, cnt.data(), off.data(), s); }))
      return comm_fail("order allgather");
    std::swap(ctx->order, ctx->alt);
    return 0;
  };

  ctx->w_count = 0;
  if (N > 0 && iterations > 0) {
    if (int e = ctx->predraw_hyperplanes(seed_base, *rng_counter, (uint64_t)floor_log2(N),
                                         iterations, &st->host_ms))
      return e;
  }
  const int R = delta_words(ctx->dp);
  std::vector<size_t> scnt(W), soff(W), rcnt(W), roff(W), dcnt(W), doff(W);

  bool replicated = false;
  for (int it = 0; it < run_iters; ++it) {
    if (!ctx->shards(N)) {  // the replicated tail: every rank runs the rest on its own
      if (int e = gather_order()) return e;
      ctx->n_live = N;
      replicated = true;
      if (int e = run_single(ctx, threshold, sim_step, it, run_iters, bucket_size_threshold,
                             seed_base, rng_counter, nt_trace, st))
        return e;
      N = ctx->n_live;
      break;
    }
    if (nt_trace) nt_trace[it] = N;
    ctx->tick(it);
    if (N == 0) {
      account_iteration(st, 0, 0, 0);
      threshold -= sim_step;
      continue;
    }
    const int h = floor_log2(N);
    const uint64_t k = *rng_counter;
    *rng_counter += (uint64_t)h;
    if (int e = ctx->ensure_hyperplanes(seed_base, k, (uint64_t)h, &st->host_ms)) return e;

    // 1. keys of my rows, key-range ownership, send counts
    if (!ctx->ctr_clean) if (int e = ctx->reset_counters()) return e;
    ctx->ctr_clean = false;
    // (HIP events around the projection only with hip_events / phase_timing: a record is a
    // marker packet the stream waits on, ~9 us per iteration)
    const bool rec = ctx->hip_events || ctx->phase_timing;
    if (rec) KLSH_HIP(hipEventRecord(ctx->ev[EV_PROJECT_BEGIN], s));
    launch_project(ctx->rows, ctx->order, ctx->keys, n_g, ctx->hyperplane_ptr(k), h, 0u, s,
                   &ctx->pp);
    KLSH_HIP(hipGetLastError());
    if (rec) KLSH_HIP(hipEventRecord(ctx->ev[EV_PROJECT_END], s));
    const int B = std::min(h, kMaxBinBits);
    const int shift = h - B;
    const uint32_t nbins = 1u << B;
    launch_bin_hist(ctx->keys, n_g, shift, nbins, ctx->bins, s, ctx->grid_cap);
    if (timed_comm([&] { return cm->allgather(ctx->bins, ctx->bins_all, 4ull * nbins, s); }))
      return comm_fail("bin histogram allgather");
    launch_bin_split(ctx->bins_all, W, nbins, N, ctx->owner, ctx->cntmat, s);
    // the send counts to the host through mapped memory (k_publish_words): no copy, no event
    const uint32_t seq_counts = ++ctx->shp_seq;
    launch_publish_words(ctx->cntmat, (uint32_t)(W * W), nullptr, 0u, ctx->shp_dev + 16,
                         ctx->shp_dev, seq_counts, s);
    // 2a. the stable partition by owner needs only the device's ownership map: it is queued
    //     before the host waits (for the counts only, not for it), so it runs during the round trip
    if (launch_partition(ctx->keys, ctx->order, n_g, shift, ctx->owner, W, ctx->nk1,
                         ctx->tile_sums, ctx->ctr, ctx->sbuf, s))
      return fail(KLSH_E_ARG, "partition: unsupported world size");
    KLSH_HIP(hipGetLastError());
    if (timed_comm([&] { return cm->wait_flag(ctx->shp_host, seq_counts, s); }))
      return comm_fail("send counts");
    std::atomic_thread_fence(std::memory_order_acquire);
    memcpy(ctx->h_small, ctx->shp_host + 16, 4ull * W * W);
    uint32_t m_g = 0;
    for (int r = 0; r < W; ++r) {
      scnt[r] = 8ull * ctx->h_small[g * W + r];
      rcnt[r] = 8ull * ctx->h_small[r * W + g];
      soff[r] = r ? soff[r - 1] + scnt[r - 1] : 0;
      roff[r] = r ? roff[r - 1] + rcnt[r - 1] : 0;
      m_g += ctx->h_small[r * W + g];
    }

    // 2b. exchange the partitioned (key, slot) pairs: all-to-all-v
    if (timed_comm([&] {
          return cm->alltoallv(ctx->sbuf, scnt.data(), soff.data(), ctx->rbuf, rcnt.data(),
                               roff.data(), s);
        }))
      return comm_fail("pair all-to-all");
    launch_unpack_pairs(ctx->rbuf, m_g, ctx->keys, ctx->alt, s);
    if (ctx->phase_timing) KLSH_HIP(hipEventRecord(ctx->ev[EV_EXCHANGE_END], s));

    // 3. bucket order of my key range, merge, compaction, delta list
    uint32_t *fk = nullptr, *fv = nullptr;
    radix_sort(ctx->keys, ctx->alt, ctx->keys2, ctx->order, m_g, h, ctx->hist, &fk, &fv, s);
    KLSH_HIP(hipGetLastError());
    if (ctx->phase_timing) KLSH_HIP(hipEventRecord(ctx->ev[EV_SORT_END], s));
    uint32_t* out = (fv == ctx->order) ? ctx->alt : ctx->order;
    // the merge kernels of this iteration list the survivors they rewrite
    const DeltaSink sink{ctx->dslots, ctx->mark, ++ctx->stamp};
    if (int e = merge_main(ctx, fk, fv, m_g, threshold, bucket_size_threshold, out, st,
                           ctx->phase_timing, /*sync=*/false, nullptr, kNoTime, sink))
      return e;
    // 4. counters of every rank in one exchange and one host sync: oversize runs, survivors,
    //    rewritten rows (n_over, total, n_delta are adjacent in Counters)
    KLSH_HIP(hipMemcpyAsync(ctx->small + 4 * W, &ctx->ctr->n_over, 12, hipMemcpyDeviceToDevice, s));
    if (timed_comm([&] { return cm->allgather(ctx->small + 4 * W, ctx->small, 16, s); }))
      return comm_fail("counter allgather");
    // every rank's counters and this rank's Counters to the host through mapped memory
    static_assert(sizeof(Counters) % 4 == 0, "Counters published as words");
    const uint32_t seq_ctr = ++ctx->shp_seq;
    launch_publish_words(ctx->small, (uint32_t)(4 * W), reinterpret_cast<const uint32_t*>(ctx->ctr),
                         (uint32_t)(sizeof(Counters) / 4), ctx->shp_dev + 16, ctx->shp_dev, seq_ctr,
                         s);
    if (timed_comm([&] { return cm->wait_flag(ctx->shp_host, seq_ctr, s); })) return comm_fail("counters");
    std::atomic_thread_fence(std::memory_order_acquire);
    memcpy(ctx->h_small, ctx->shp_host + 16, 16ull * W);
    memcpy(ctx->h_ctr, ctx->shp_host + 16 + 4 * W, sizeof(Counters));
    if (int e = ctx->check_device_err()) return e;
    if (ctx->phase_timing && st) {
      st->merge_ms += elapsed(ctx->ev[EV_MERGE_BEGIN], ctx->ev[EV_MERGE_END]);
      st->compact_ms += elapsed(ctx->ev[EV_MERGE_END], ctx->ev[EV_COMPACT_END]);
    }
    std::vector<uint32_t> surv(W), ndel(W);
    uint64_t any_over = 0;
    for (int r = 0; r < W; ++r) {
      any_over += ctx->h_small[4 * r];
      surv[r] = ctx->h_small[4 * r + 1];
      ndel[r] = ctx->h_small[4 * r + 2];
    }
    if (any_over) {  // nestedCluster somewhere: RNG offsets need every rank's hyperplane count
      std::vector<uint2> over;
      uint64_t my_hyp = 0;
      if (int e = oversize_runs(ctx, &over, &my_hyp)) return e;
      auto exchange_counters = [&](uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3) -> int {
        uint32_t* hs = ctx->h_small;
        hs[0] = a0; hs[1] = a1; hs[2] = a2; hs[3] = a3;
        KLSH_HIP(hipMemcpyAsync(ctx->small + 4 * W, hs, 16, hipMemcpyHostToDevice, s));
        if (timed_comm([&] { return cm->allgather(ctx->small + 4 * W, ctx->small, 16, s); }))
          return comm_fail("counter allgather");
        KLSH_HIP(hipMemcpyAsync(hs, ctx->small, 16ull * W, hipMemcpyDeviceToHost, s));
        if (timed_comm([&] { return cm->wait(s); })) return comm_fail("counter exchange");
        return 0;
      };
      if (int e = exchange_counters((uint32_t)my_hyp, 0, 0, 0)) return e;
      uint64_t hyp_before = 0, hyp_all = 0;
      for (int r = 0; r < W; ++r) {
        if (r < g) hyp_before += ctx->h_small[4 * r];
        hyp_all += ctx->h_small[4 * r];
      }
      uint64_t rng = *rng_counter + hyp_before;
      if (!over.empty())
        if (int e = merge_nested(ctx, fk, fv, m_g, threshold, over, seed_base, &rng, out, st,
                                     sink))
          return e;
      *rng_counter += hyp_all;
      if (int e = exchange_counters(ctx->h_ctr->total, ctx->h_ctr->n_delta, 0, 0)) return e;
      for (int r = 0; r < W; ++r) {
        surv[r] = ctx->h_small[4 * r];
        ndel[r] = ctx->h_small[4 * r + 1];
      }
    }

    // 5. merge deltas to every replica
    uint64_t nd_all = 0;
    for (int r = 0; r < W; ++r) {
      dcnt[r] = 4ull * R * ndel[r];
      doff[r] = 4ull * R * nd_all;
      nd_all += ndel[r];
    }
    if (nd_all) {
      if (int e = ctx->reserve_words(&ctx->drec, &ctx->drec_cap, (size_t)R * ndel[g] + 1)) return e;
      if (int e = ctx->reserve_words(&ctx->drec_all, &ctx->drec_all_cap, (size_t)R * nd_all)) return e;
      launch_delta_pack(ctx->rows, ctx->dslots, ndel[g], ctx->drec, s, ctx->grid_cap);
      if (timed_comm([&] {
            return cm->allgatherv(ctx->drec, ctx->drec_all, dcnt.data(), doff.data(), s);
          }))
        return comm_fail("delta allgather");
      launch_delta_apply(ctx->rows, ctx->drec_all, (uint32_t)nd_all, s, ctx->grid_cap);
      KLSH_HIP(hipGetLastError());
    }

    if (out == ctx->alt) std::swap(ctx->order, ctx->alt);
    const uint64_t N_next = std::accumulate(surv.begin(), surv.end(), (uint64_t)0);
    if (rec) {
      st->project_ms += elapsed(ctx->ev[EV_PROJECT_BEGIN], ctx->ev[EV_PROJECT_END]);
      st->project_timed_launches += 1;
    }
    if (ctx->phase_timing) st->sort_ms += elapsed(ctx->ev[EV_EXCHANGE_END], ctx->ev[EV_SORT_END]);
    account_iteration(st, N, h, N_next);
    N = N_next;
    n_g = surv[g];
    n_all = surv;
    threshold -= sim_step;
  }

  // global canonical order on every rank, combined member links
  if (!replicated)
    if (int e = gather_order()) return e;
  if (timed_comm([&] { return cm->allreduce_min_u32(ctx->rows.nxt, ctx->members, s); }))
    return comm_fail("member link allreduce");
  if (timed_comm([&] { return cm->wait(s); })) return comm_fail("member link allreduce");
  ctx->n_live = N;
  st->n_final = N;
  st->comm_ms = t_comm;
  st->wall_ms = now_ms() - t_start;
  return 0;
}

// A rank that fails mid-call aborts the group, so the other ranks' pending and next collectives
// fail too instead of waiting for it forever; the context's group is unusable afterwards.
int cluster_sharded(klsh_ctx* ctx, float min_similarity, int iterations, int run_iters,
                    int bucket_size_threshold, uint32_t seed_base, uint64_t* rng_counter,
                    uint64_t* nt_trace, klsh_stats* st) {
  if (ctx->comm->aborted) return fail(KLSH_E_STATE, "communicator aborted by an earlier failure");
  const int rc = cluster_sharded_body(ctx, min_similarity, iterations, run_iters,
                                      bucket_size_threshold, seed_base, rng_counter, nt_trace, st);
  if (rc) {
    const std::string msg = klsh_last_error();  // (the abort must not replace the failure's message)
    ctx->comm->abort();
    return fail(rc, msg);
  }
  return rc;
}

}  // namespace klsh

extern "C" {

int klsh_comm_unique_id(uint8_t* id) {
  if (!id) return fail(KLSH_E_ARG, "null argument");
  std::string err;
  if (klsh::rccl_unique_id(id, &err)) return fail(KLSH_E_HIP, err);
  return 0;
}

int klsh_comm_init(klsh_ctx* ctx, int rank, int world, const uint8_t* id) {
  if (!ctx || !id || world < 1 || rank < 0 || rank >= world || world > klsh::kMaxRanks)
    return fail(KLSH_E_ARG, "bad argument");
  KLSH_HIP(hipSetDevice(ctx->device));
  std::string err;
  klsh::Comm* c = klsh::make_rccl_comm(rank, world, id, ctx->device, &err);
  if (!c) return fail(KLSH_E_HIP, err);
  c->timeout_s = ctx->comm_timeout_s;
  ctx->release_shard();
  delete ctx->comm;
  ctx->comm = c;
  return 0;
}

int klsh_comm_init_local(klsh_ctx** ctxs, int world) {
  if (!ctxs || world < 1 || world > klsh::kMaxRanks) return fail(KLSH_E_ARG, "bad argument");
  for (int r = 0; r < world; ++r)
    if (!ctxs[r]) return fail(KLSH_E_ARG, "null context");
  std::vector<klsh::Comm*> cs(world);
  klsh::make_local_comms(world, cs.data());
  for (int r = 0; r < world; ++r) {
    ctxs[r]->release_shard();
    delete ctxs[r]->comm;
    ctxs[r]->comm = cs[r];
  }
  return 0;
}

int klsh_comm_info(klsh_ctx* ctx, int* rank, int* world) {
  if (!ctx) return fail(KLSH_E_ARG, "null ctx");
  if (rank) *rank = ctx->rank();
  if (world) *world = ctx->world();
  return 0;
}

}  // extern "C"
