// The per-iteration launch sequence of Cluster() (reference function/cluster.cc:181-340) on one
// device, nestedCluster orchestration (:89-178), and klsh_cluster.
//
// Per LSH iteration t (N_t live rows, h_t = floor(log2 N_t)), everything on the context's stream:
//   1. hyperplanes k_t .. k_t+h_t-1 from the call's window (klsh_ctx::ensure_hyperplanes; drawn
//      on the host, in the background for a whole call where they fit)
//   2. projection: the key of every live row, in canonical order
//   3. radix sort (key, slot): the stable bucket order of merge_hashtable
//   4. launch_merge: the runs of equal keys listed by length class, greedy p_cluster in each
//   5. compaction of the survivors -> canonical order of iteration t+1.  Its last workgroup
//      publishes the counters (N_{t+1}, oversize runs, the run classes) into mapped pinned memory
//      with a sequence number; the host polls that word (klsh_ctx::wait_published) instead of a
//      copy and a stream sync.
// Queued projection: where the kernels can read N from the device, step 2 of iteration t+1 is
// enqueued behind the compaction of t, before the host has t's counters (QueuedProjection).
// Oversize buckets (> bucket_size_threshold) are re-hashed with fresh hyperplanes drawn in
// ascending bucket order (the reference's T=1 RNG order), sorted, merged, and 5 is redone; a
// projection queued ahead is then discarded and recomputed.
// Queued tail batches (run_batched): once no bucket can be oversize and N_t < 2^20, whole
// iterations are queued 32 at a time, two chunks in flight, each publishing into its own ring
// slot.
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <deque>

#include "klsh_loop.h"

namespace klsh {

// Rows per kernel class of one iteration (the unit of each class's algorithmic bytes), from the
// counters that iteration published.  tail: the iteration ran every merge class in k_merge_tail.
static void count_class_rows(klsh_stats* st, const Counters& c, uint64_t n, bool tail) {
  uint64_t big_rows = 0, big_runs = 0, small_runs = 0;
  for (int b = 0; b < kBigClasses; ++b) big_rows += c.n_big_rows[b], big_runs += c.n_big[b];
  for (int b = 0; b < kGroupClasses; ++b) small_runs += c.n_cls[b];
  for (int k : {KC_PROJECT, KC_SORT, KC_COMPACT}) st->kern[k].rows += n;
  st->kern[KC_RUNS].rows += n;
  st->kern[KC_RUNS].runs += c.n_seg;
  st->kern[KC_HUGE].rows += c.n_huge_rows;
  st->kern[KC_HUGE].runs += c.n_huge;
  if (c.screened) {  // the screen saw every small run, the merge only the ones it passed
    st->kern[KC_SCREEN].rows += c.n_small_rows;
    st->kern[KC_SCREEN].runs += small_runs;
  }
  const uint64_t merged_small = c.screened ? c.n_act_rows : c.n_small_rows;
  if (tail) {
    st->kern[KC_TAIL].rows += merged_small + big_rows;
    st->kern[KC_TAIL].runs += small_runs + big_runs;
    return;
  }
  st->kern[KC_SMALL].rows += merged_small;
  if (!c.screened) st->kern[KC_SMALL].runs += small_runs;
  for (int b = 0; b < kBigClasses; ++b) {
    st->kern[KC_BIG128 + b].rows += c.n_big_rows[b];
    st->kern[KC_BIG128 + b].runs += c.n_big[b];
  }
}

// The call's per-class spans: fold the last iteration's set, then read and clear the totals.
static int collect_kernel_times(klsh_ctx* ctx, int last_set, klsh_stats* st) {
  hipStream_t s = ctx->stream;
  if (last_set >= 0) launch_stamp_fold(ctx->kstamp, last_set, s);
  KLSH_HIP(hipGetLastError());
  unsigned long long tot[2][KC_COUNT];
  KLSH_HIP(hipMemcpyAsync(tot[0], ctx->kstamp->ticks, sizeof(tot), hipMemcpyDeviceToHost, s));
  KLSH_HIP(hipMemsetAsync(ctx->kstamp->ticks, 0, sizeof(tot), s));
  KLSH_HIP(hipStreamSynchronize(s));
  static_assert(offsetof(KStampBlock, launches) == offsetof(KStampBlock, ticks) + sizeof(unsigned long long) * KC_COUNT,
                "ticks and launches are adjacent");
  for (int k = 0; k < KC_COUNT; ++k) {
    st->kern[k].ms += (double)tot[0][k] * 1e-5;  // 100 MHz ticks
    st->kern[k].launches += tot[1][k];
  }
  return 0;
}

// ---- diagnostics build (make prof): KLSH_BUCKET_STATS=<file> appends every host-driven
// iteration's run-length histogram, KLSH_ITER_LOG=<file> a line per iteration.  Both keep the
// loop host-driven.  Empty in the product build.
#ifdef KLSH_DIAG
static bool diag_bucket_stats_on() { return getenv("KLSH_BUCKET_STATS") != nullptr; }
static FILE* diag_iter_log() {
  static FILE* f = [] {
    const char* e = getenv("KLSH_ITER_LOG");
    return e ? fopen(e, "a") : nullptr;
  }();
  return f;
}
static bool diag_host_driven() { return diag_bucket_stats_on() || getenv("KLSH_ITER_LOG"); }
static double diag_iter_begin() { return diag_iter_log() ? now_ms() : 0.0; }

static int diag_bucket_stats(klsh_ctx* ctx, const uint32_t* fk, uint64_t n, int it, int h) {
  const char* path = getenv("KLSH_BUCKET_STATS");
  if (!path) return 0;
  hipStream_t s = ctx->stream;
  std::vector<uint32_t> hk(n);
  KLSH_HIP(hipMemcpyAsync(hk.data(), fk, 4 * n, hipMemcpyDeviceToHost, s));
  KLSH_HIP(hipStreamSynchronize(s));
  uint64_t hist[12] = {0}, pairs = 0, maxb = 0, rows_in[12] = {0};
  for (uint64_t a = 0; a < n;) {
    uint64_t b = a + 1;
    while (b < n && hk[b] == hk[a]) ++b;
    const uint64_t len = b - a;
    int c = 0;
    while (c < 11 && (1ull << c) < len) ++c;  // class c: len in (2^(c-1), 2^c]
    hist[c]++;
    rows_in[c] += len;
    pairs += len * (len - 1) / 2;
    maxb = std::max(maxb, len);
    a = b;
  }
  if (FILE* f = fopen(path, "a")) {
    fprintf(f, "{\"it\": %d, \"n\": %llu, \"h\": %d, \"pairs\": %llu, \"max\": %llu, \"hist\": [", it,
            (unsigned long long)n, h, (unsigned long long)pairs, (unsigned long long)maxb);
    for (int c = 0; c < 12; ++c) fprintf(f, "%s%llu", c ? ", " : "", (unsigned long long)hist[c]);
    fprintf(f, "], \"rows\": [");
    for (int c = 0; c < 12; ++c) fprintf(f, "%s%llu", c ? ", " : "", (unsigned long long)rows_in[c]);
    fprintf(f, "]}\n");
    fclose(f);
  }
  return 0;
}

// (it, n, h, wall ms, ms until queued, the big run classes)
static void diag_log_iteration(const klsh_ctx* ctx, int it, uint64_t n, int h, double t_it) {
  FILE* f = diag_iter_log();
  if (!f) return;
  const Counters& c = *ctx->h_ctr;
  fprintf(f, "%d %llu %d %.4f %.4f %u %u %u %u\n", it, (unsigned long long)n, h, now_ms() - t_it,
          ctx->t_enqueued - t_it, c.n_big[0], c.n_big[1], c.n_big[2] + c.n_big[3], c.n_huge);
  fflush(f);
}

static void diag_log_batched(int it, uint64_t n, int h, const Counters& cc) {
  FILE* f = diag_iter_log();
  if (!f) return;
  fprintf(f, "%d %llu %d batched runs %u small_rows %u big %u %u %u %u huge %u\n", it,
          (unsigned long long)n, h, cc.n_seg, cc.n_small_rows, cc.n_big[0], cc.n_big[1],
          cc.n_big[2], cc.n_big[3], cc.n_huge);
  fflush(f);
}
#else
static inline bool diag_bucket_stats_on() { return false; }
static inline bool diag_host_driven() { return false; }
static inline double diag_iter_begin() { return 0.0; }
static inline int diag_bucket_stats(klsh_ctx*, const uint32_t*, uint64_t, int, int) { return 0; }
static inline void diag_log_iteration(const klsh_ctx*, int, uint64_t, int, double) {}
static inline void diag_log_batched(int, uint64_t, int, const Counters&) {}
#endif

int merge_main(klsh_ctx* ctx, uint32_t* fk, uint32_t* fv, uint32_t n, float thr, int bucket_thr,
               uint32_t* out, klsh_stats* st, bool timed, bool sync,
               const std::function<int(uint32_t*)>* after, KTime kt, const DeltaSink& sink) {
  hipStream_t s = ctx->stream;
  if (timed) KLSH_HIP(hipEventRecord(ctx->ev[EV_MERGE_BEGIN], s));
  // the small-run merge is a launch of its own at >= 2^20 positions (register widths): its HIP
  // events are the headline's cross-check
  const bool time_small = (ctx->hip_events || ctx->phase_timing) && kt.blk && st && sync &&
                          n >= tail_merge_max(ctx->mp) && project_device_n_ok(ctx->d);
  const MergeCall call{kt, {time_small ? ctx->sev[0] : nullptr, time_small ? ctx->sev[1] : nullptr},
                       sink, ctx->grid_cap};
  launch_merge(ctx->rows, fk, fv, 0, n, thr, bucket_thr, ctx->mp, call, ctx->ctr, s);
  KLSH_HIP(hipGetLastError());
  if (timed) KLSH_HIP(hipEventRecord(ctx->ev[EV_MERGE_END], s));
  const bool zc = sync && ctx->zero_copy;
  Publish pub{ctx->pub_dev, ctx->pub_seq_dev, ++ctx->pub_seq, ctx->n_next_dev};
  launch_compact(fv, n, out, ctx->tile_sums, ctx->ctr, s, zc ? &pub : nullptr, ctx->rc, kt,
                 ctx->lb.status ? &ctx->lb : nullptr);
  KLSH_HIP(hipGetLastError());
  if (timed) KLSH_HIP(hipEventRecord(ctx->ev[EV_COMPACT_END], s));
  if (zc && after)  // work queued behind the compaction before the host waits for it
    if (int e = (*after)(out)) return e;
  if (!sync) return 0;  // the caller fetches the counters with its own exchange
  ctx->t_enqueued = now_ms();
  if (zc) {
    if (int e = ctx->wait_published(pub.seq)) return e;
  } else {
    ctx->ctr_clean = false;
    if (int e = ctx->sync_counters()) return e;
  }
  if (kt.blk && st) {  // this iteration's rows per kernel class
    const bool tail = n < tail_merge_max(ctx->mp) && project_device_n_ok(ctx->d);
    count_class_rows(st, *ctx->h_ctr, n, tail);
  }
  if (time_small) {  // the compaction (published) runs after the merge streams' join
    KLSH_HIP(hipEventSynchronize(ctx->sev[1]));
    st->small_ms += elapsed(ctx->sev[0], ctx->sev[1]);
    st->small_launches += 1;
    st->small_rows += ctx->h_ctr->screened ? ctx->h_ctr->n_act_rows : ctx->h_ctr->n_small_rows;
    st->small_iter_merges += n - ctx->h_ctr->total;
  }
  if (timed && zc) KLSH_HIP(hipEventSynchronize(ctx->ev[EV_COMPACT_END]));
  if (timed && st) {
    st->merge_ms += elapsed(ctx->ev[EV_MERGE_BEGIN], ctx->ev[EV_MERGE_END]);
    st->compact_ms += elapsed(ctx->ev[EV_MERGE_END], ctx->ev[EV_COMPACT_END]);
  }
  return 0;
}

int oversize_runs(klsh_ctx* ctx, std::vector<uint2>* over, uint64_t* hyperplanes) {
  const uint32_t n_over = ctx->h_ctr->n_over;
  over->resize(n_over);
  *hyperplanes = 0;
  if (n_over == 0) return 0;
  KLSH_HIP(hipMemcpy(over->data(), ctx->mp.lists.over, sizeof(uint2) * n_over, hipMemcpyDeviceToHost));
  std::sort(over->begin(), over->end(), [](const uint2& a, const uint2& b) { return a.x < b.x; });
  for (const uint2& o : *over) *hyperplanes += (uint64_t)floor_log2(o.y);
  return 0;
}

int merge_nested(klsh_ctx* ctx, uint32_t* fk, uint32_t* fv, uint32_t n, float thr,
                 const std::vector<uint2>& over, uint32_t seed_base, uint64_t* rng_counter,
                 uint32_t* out, klsh_stats* st, const DeltaSink& sink) {
  hipStream_t s = ctx->stream;
  const MergeCall call{kNoTime, {nullptr, nullptr}, sink, ctx->grid_cap};
  for (uint32_t oi = 0; oi < (uint32_t)over.size(); ++oi) {
    const uint32_t p = over[oi].x, b = over[oi].y;
    const int h2 = floor_log2(b);
    const uint64_t k = *rng_counter;
    *rng_counter += (uint64_t)h2;
    if (st) {
      st->hyperplanes += (uint64_t)h2;
      st->nested_calls += 1;
    }
    if (int e = ctx->ensure_hyperplanes(seed_base, k, (uint64_t)h2, st ? &st->host_ms : nullptr))
      return e;
    // Sub-keys carry bit 31 (main keys are < 2^h <= 2^31, so never have it) and a bit 30 that
    // alternates between consecutive oversize regions, so no run crosses a region boundary.
    const uint32_t key_or = 0x80000000u | ((oi & 1u) << 30);
    launch_project(ctx->rows, fv + p, ctx->nk1, b, ctx->hyperplane_ptr(k), h2, key_or, s, &ctx->pp);
    uint32_t *rk = nullptr, *rv = nullptr;
    radix_sort(ctx->nk1, fv + p, ctx->nk2, ctx->nv2, b, h2, ctx->hist, &rk, &rv, s);
    KLSH_HIP(hipMemcpyAsync(fk + p, rk, 4ull * b, hipMemcpyDeviceToDevice, s));
    if (rv != fv + p) KLSH_HIP(hipMemcpyAsync(fv + p, rv, 4ull * b, hipMemcpyDeviceToDevice, s));
    // fresh run lists for the region
    KLSH_HIP(hipMemsetAsync(ctx->rc, 0, sizeof(RunCounters), s));
    launch_merge(ctx->rows, fk, fv, p, p + b, thr, -1, ctx->mp, call, ctx->ctr, s);
    KLSH_HIP(hipGetLastError());
  }
  launch_compact(fv, n, out, ctx->tile_sums, ctx->ctr, s, nullptr, ctx->rc);
  KLSH_HIP(hipGetLastError());
  return ctx->sync_counters();
}

int merge_and_compact(klsh_ctx* ctx, uint32_t* fk, uint32_t* fv, uint32_t n, float thr,
                      int bucket_thr, uint32_t seed_base, uint64_t* rng_counter, klsh_stats* st,
                      bool timed, const std::function<int(uint32_t*)>* after, KTime kt) {
  uint32_t* out = (fv == ctx->order) ? ctx->alt : ctx->order;
  if (int e = merge_main(ctx, fk, fv, n, thr, bucket_thr, out, st, timed, true, after, kt))
    return e;
  MergePlan& mp = ctx->mp;  // the next iteration's long-run launches, from this one's run counts
  mp.big896_aux = ctx->h_ctr->n_big[kBigClasses - 1] >= 64u ? 1u : 0u;
  // (C4 has iterations without >896-row runs between ones with dozens: a cap of 4 serialised
  // those walks, k_merge_huge<32> 746 -> 1024 ms per step)
  mp.huge_cap = ctx->h_ctr->n_huge == 0 ? 64u : 0u;
  mp.huge_quiet = ctx->h_ctr->n_huge == 0 ? mp.huge_quiet + 1 : 0;
  mp.huge_fold = (mp.huge_quiet >= 4 || mp.huge_fold_always) ? 1u : 0u;
  if (ctx->h_ctr->n_over > 0) {
    std::vector<uint2> over;
    uint64_t hyp = 0;
    if (int e = oversize_runs(ctx, &over, &hyp)) return e;
    if (int e = merge_nested(ctx, fk, fv, n, thr, over, seed_base, rng_counter, out, st))
      return e;
  }
  if (out == ctx->alt) std::swap(ctx->order, ctx->alt);
  ctx->n_live = ctx->h_ctr->total;
  return 0;
}

// ------------------------------------------------------------------ queued tail batches -----
// Once no bucket can be oversize (N_t <= bucket_size_threshold: nestedCluster, which needs the
// host's RNG order, cannot happen) and N_t < 2^20 (the one-launch merge and compaction), the rest
// of the loop needs nothing from the host: every kernel of an iteration reads N_t from
// n_next_dev, the projection finds its hyperplanes at the offset woff (each compaction advances it
// by its own h = floor(log2 N_t), cluster.cc:194-196), the sort runs the passes of the largest h
// ahead (passes over all-zero digits are stable identities), the threshold schedule is known.
// Iterations are queued C at a time, two chunks in flight; every compaction publishes into its own
// ring slot and the host reads a chunk's slots when its last sequence number is in — the trace,
// the RNG counter and the statistics come out exactly as the per-iteration loop's.
static bool batch_eligible(const klsh_ctx* ctx, uint64_t n, int bucket_thr, int iters_left) {
  // (< 2^20 too: the queued compaction is the one-launch look-back over <= 256 tiles)
  if (!ctx->tail_batch || n < 2 || n >= std::min<uint64_t>(tail_merge_max(ctx->mp), 1u << 20) ||
      iters_left < 2)
    return false;
  if (bucket_thr >= 0 && n > (uint64_t)bucket_thr) return false;
  if (!ctx->zero_copy || !ctx->ring_dev || !ctx->lb.status || ctx->phase_timing) return false;
  if (!project_device_n_ok(ctx->d) || ctx->shards(n)) return false;
  if (diag_host_driven()) return false;
  // every queued iteration's hyperplanes resident at once
  return (uint64_t)iters_left * (uint64_t)floor_log2(n) * (uint64_t)ctx->dp <= (64ull << 20);
}

static int run_batched(klsh_ctx* ctx, float& threshold, float sim_step, int it, int it_end,
                       int bucket_size_threshold, uint32_t seed_base, uint64_t* rng_counter,
                       uint64_t* nt_trace, klsh_stats* st,
                       const std::function<KTime(uint64_t)>& ktime) {
  hipStream_t s = ctx->stream;
#ifdef KLSH_MERGE_PROF
  if (getenv("KLSH_MERGE_PROF")) {  // diagnostics: the head's merge profile apart from the tail's
    fprintf(stderr, "[mprof] ---- head: iterations before %d\n", it);
    merge_prof_dump(stderr);
    fprintf(stderr, "[mprof] ---- tail: iterations %d..%d\n", it, it_end - 1);
  }
#endif
  constexpr int C = klsh_ctx::kRing / 2;  // iterations per chunk
  uint64_t n_known = ctx->n_live;         // N after the last iteration the host has read
  const int h0 = floor_log2(n_known);
  const uint64_t k0 = *rng_counter;
  const uint64_t need = (uint64_t)(it_end - it) * (uint64_t)h0;
  if (!(ctx->W && ctx->w_base == seed_base && ctx->w_dp == ctx->dp && ctx->w_d == ctx->d &&
        k0 >= ctx->w_k0 && k0 + need <= ctx->w_k0 + ctx->w_count)) {
    // a window restart may overwrite rows a queued projection still reads; an append may not
    if (!ctx->lazy_covers(seed_base, k0, need)) KLSH_HIP(hipStreamSynchronize(s));
    if (int e = ctx->ensure_hyperplanes(seed_base, k0, need, &st->host_ms)) return e;
  }
  uint32_t* n_dev = ctx->n_next_dev;
  uint32_t* woff_dev = ctx->n_next_dev + 1;
  KLSH_HIP(hipMemsetD32Async(n_dev, (int)(uint32_t)n_known, 1, s));
  KLSH_HIP(hipMemsetD32Async(woff_dev, (int)(uint32_t)(k0 - ctx->w_k0), 1, s));
  const uint64_t queued_k = ctx->spec.k;
  bool queued = ctx->take_queued_projection();  // the first projection is already on the stream
  if (!queued && !ctx->ctr_clean)
    if (int e = ctx->reset_counters()) return e;
  if (queued && queued_k != k0) return fail(KLSH_E_STATE, "queued projection out of step");

  struct Chunk {
    int it0, count, slot0;
    uint32_t seq_last;
  };
  std::deque<Chunk> inflight;
  int next = it, slot = 0;
  float thr = threshold;
  uint64_t n_max = n_known;
  auto enqueue = [&](int count) -> int {
    const int hb = floor_log2(n_max);  // h of every iteration of the chunk is <= hb
    for (int c = 0; c < count; ++c, ++next) {
      const KTime kt = ktime(ctx->kt_iter++);
      if (!queued)
        launch_project_device_n(ctx->rows, ctx->order, ctx->keys, (uint32_t)n_max, ctx->W, n_dev, s,
                                kt, woff_dev, &ctx->pp);
      queued = false;
      uint32_t *fk = nullptr, *fv = nullptr;
      const bool local = ctx->tail_local && tail_local_ok((uint32_t)n_max, hb);
      const MergeCall call{kt, {nullptr, nullptr}, kNoSink, ctx->grid_cap};
      ctx->tail_local_iters += local ? 1u : 0u;
      if (local) {  // top-bits partition, then the buckets sorted in LDS with their runs listed
        const uint32_t* dtot = radix_sort_top(ctx->keys, ctx->order, ctx->keys2, ctx->alt,
                                              (uint32_t)n_max, hb, ctx->hist, s, kt, n_dev);
        launch_tail_local(ctx->keys2, ctx->alt, ctx->keys, ctx->order, dtot, hb,
                          bucket_size_threshold, ctx->mp, call, s);
        fk = ctx->keys;
        fv = ctx->order;
      } else {
        radix_sort(ctx->keys, ctx->order, ctx->keys2, ctx->alt, (uint32_t)n_max, hb, ctx->hist,
                   &fk, &fv, s, kt, n_dev);
      }
      launch_merge(ctx->rows, fk, fv, 0, (uint32_t)n_max, thr, bucket_size_threshold, ctx->mp,
                   call, ctx->ctr, s, n_dev, local);
      uint32_t* out = (fv == ctx->order) ? ctx->alt : ctx->order;
      Publish pub{ctx->ring_dev + slot, ctx->pub_seq_dev, ++ctx->pub_seq, n_dev, woff_dev};
      launch_compact(fv, (uint32_t)n_max, out, ctx->tile_sums, ctx->ctr, s, &pub, ctx->rc, kt,
                     &ctx->lb, n_dev);
      if (out == ctx->alt) std::swap(ctx->order, ctx->alt);
      thr -= sim_step;
      slot = (slot + 1) % klsh_ctx::kRing;
    }
    KLSH_HIP(hipGetLastError());
    return 0;
  };
  while (next < it_end || !inflight.empty()) {
    while (next < it_end && inflight.size() < 2) {
      const Chunk ch{next, std::min(C, it_end - next), slot, 0u};
      if (int e = enqueue(ch.count)) return e;
      inflight.push_back(ch);
      inflight.back().seq_last = ctx->pub_seq;
    }
    const Chunk ch = inflight.front();
    inflight.pop_front();
    if (int e = ctx->wait_seq(ch.seq_last)) return e;
    for (int c = 0; c < ch.count; ++c) {
      const Counters cc = ctx->ring_host[(ch.slot0 + c) % klsh_ctx::kRing];
      const uint64_t n_in = n_known;
      if (cc.err)
        return fail(KLSH_E_HIP, "device protocol failure (look-back wait limit), code " +
                                    std::to_string(cc.err));
      if (cc.n_over || n_in == 0 || cc.total == 0 || cc.total > n_in)
        return fail(KLSH_E_STATE, "queued iteration published inconsistent counters");
      const int h = floor_log2(n_in);
      if (nt_trace) nt_trace[ch.it0 + c] = n_in;
      ctx->tick(ch.it0 + c);
      *rng_counter += (uint64_t)h;
      account_iteration(st, n_in, h, cc.total);  // (no HIP events around queued launches: not in project_ms)
      if (ctx->kernel_timing && ctx->kstamp) count_class_rows(st, cc, n_in, true);
      diag_log_batched(ch.it0 + c, n_in, h, cc);
      *ctx->h_ctr = cc;
      n_known = cc.total;
    }
    n_max = n_known;  // tighter grids for the chunks queued from now on
  }
  threshold = thr;
  ctx->n_live = n_known;
  ctx->ctr_clean = true;  // every publisher zeroed the counters behind it
  return 0;
}

int run_single(klsh_ctx* ctx, float& threshold, float sim_step, int it_begin, int it_end,
               int bucket_size_threshold, uint32_t seed_base, uint64_t* rng_counter,
               uint64_t* nt_trace, klsh_stats* st) {
  hipStream_t s = ctx->stream;
  // per-class stamps: the call's iterations stamp sets 0, 1, 0, ... in turn (ctx->kt_iter), a
  // queued projection the set of the iteration it belongs to; a projection first folds the set
  // of the iteration before it
  const uint64_t kt_first = ctx->kt_iter;
  auto ktime = [&](uint64_t j) -> KTime {
    if (!ctx->kernel_timing || !st) return kNoTime;
    if (!ctx->kstamp) return kNoTime;
    return KTime{ctx->kstamp, (int)(j & 1u), j > kt_first ? (int)((j - 1) & 1u) : -1};
  };
  for (int it = it_begin; it < it_end; ++it) {
    const uint64_t n = ctx->n_live;
    if (batch_eligible(ctx, n, bucket_size_threshold, it_end - it)) {  // the rest, queued
      const std::function<KTime(uint64_t)> kt_fn = ktime;
      if (int e = run_batched(ctx, threshold, sim_step, it, it_end, bucket_size_threshold,
                              seed_base, rng_counter, nt_trace, st, kt_fn))
        return e;
      break;
    }
    const double t_it = diag_iter_begin();
    if (nt_trace) nt_trace[it] = n;
    ctx->tick(it);
    if (n == 0) {  // the reference aborts here (cluster.cc:194 on an empty vector); no-op
      account_iteration(st, 0, 0, 0);
      threshold -= sim_step;
      continue;
    }
    const int h = floor_log2(n);
    const uint64_t k = *rng_counter;
    *rng_counter += (uint64_t)h;
    if (int e = ctx->ensure_hyperplanes(seed_base, k, (uint64_t)h, &st->host_ms)) return e;

    // the projection: queued by the previous iteration (device-side N), or now
    const QueuedProjection spec = ctx->spec;
    const bool queued = ctx->take_queued_projection();
    const uint64_t j = ctx->kt_iter++;  // this iteration's stamp set
    if (queued && spec.k != k) return fail(KLSH_E_STATE, "queued projection out of step");
    const int pair = queued ? spec.pair : 0;  // the event pair around this iteration's projection
    // the projection runs alone on the main stream: with option hip_events an event pair times it
    // (beside its stamps).  Off by default: each record is a marker packet the stream waits on,
    // ~9 us between the projection and the sort of every host-driven iteration (rocprofv3 trace,
    // round 6) — the in-kernel stamps time it without one.
    const bool rec = ctx->hip_events || ctx->phase_timing;
    if (!queued) {
      if (!ctx->ctr_clean) if (int e = ctx->reset_counters()) return e;
      if (rec) KLSH_HIP(hipEventRecord(ctx->project_begin(pair), s));
      launch_project(ctx->rows, ctx->order, ctx->keys, (uint32_t)n, ctx->hyperplane_ptr(k), h, 0u,
                     s, &ctx->pp, ktime(j));
      KLSH_HIP(hipGetLastError());
      if (rec) KLSH_HIP(hipEventRecord(ctx->project_end(pair), s));
    }
    ctx->ctr_clean = false;
    uint32_t *fk = nullptr, *fv = nullptr;
    radix_sort(ctx->keys, ctx->order, ctx->keys2, ctx->alt, (uint32_t)n, h, ctx->hist, &fk, &fv, s,
               ktime(j));
    KLSH_HIP(hipGetLastError());
    if (ctx->phase_timing) KLSH_HIP(hipEventRecord(ctx->ev[EV_SORT_END], s));
    if (int e = diag_bucket_stats(ctx, fk, n, it, h)) return e;
    // Queue the next iteration's projection behind this compaction.  If this iteration turns out
    // to have oversize buckets (nestedCluster changes rows and draws hyperplanes first), the
    // queued keys are simply recomputed; they go to the key buffer the nested work is not reading
    // (this iteration's sorted keys fk stay intact), keys2 when fk is keys — the next iteration
    // then swaps the two pointers.
    const bool ahead = ctx->zero_copy && it + 1 < it_end && project_device_n_ok(ctx->d) &&
                       !diag_bucket_stats_on();
    uint32_t* const spec_out = fk == ctx->keys ? ctx->keys2 : ctx->keys;
    const std::function<int(uint32_t*)> queue_next = [&](uint32_t* next_order) -> int {
      const uint64_t k_next = k + (uint64_t)h;  // h_next <= h: inside the drawn window
      if (int e = ctx->ensure_hyperplanes(seed_base, k_next, (uint64_t)h, &st->host_ms)) return e;
      const int next_pair = 1 - pair;
      if (rec) KLSH_HIP(hipEventRecord(ctx->project_begin(next_pair), s));
      launch_project_device_n(ctx->rows, next_order, spec_out, (uint32_t)n,
                              ctx->hyperplane_ptr(k_next), ctx->n_next_dev, s, ktime(j + 1),
                              nullptr, &ctx->pp);
      KLSH_HIP(hipGetLastError());
      if (rec) KLSH_HIP(hipEventRecord(ctx->project_end(next_pair), s));
      ctx->spec = QueuedProjection{true, k_next, next_pair, spec_out == ctx->keys2};
      return 0;
    };
    if (int e = merge_and_compact(ctx, fk, fv, (uint32_t)n, threshold, bucket_size_threshold,
                                  seed_base, rng_counter, st, ctx->phase_timing,
                                  ahead ? &queue_next : nullptr, ktime(j)))
      return e;
    if (ctx->spec.pending && *rng_counter != ctx->spec.k) {  // nested ran: recomputed next time
      ctx->drop_queued_projection();
      // the discarded launch stamped the next iteration's projection lines: clear them, or the
      // recomputed projection's span would start at the discarded one (across the nested work)
      if (ctx->kernel_timing && ctx->kstamp) {
        KStampSet* set = &ctx->kstamp->set[ctx->kt_iter & 1u];
        KLSH_HIP(hipMemsetAsync(&set->t0[KC_PROJECT][0], 0xFF, sizeof(set->t0[KC_PROJECT]), s));
        KLSH_HIP(hipMemsetAsync(&set->t1[KC_PROJECT][0], 0, sizeof(set->t1[KC_PROJECT]), s));
      }
    }
    if (rec) {
      st->project_ms += elapsed(ctx->project_begin(pair), ctx->project_end(pair));
      st->project_timed_launches += 1;
    }
    // from the end of THIS iteration's projection, whichever pair timed it
    if (rec && ctx->phase_timing)
      st->sort_ms += elapsed(ctx->project_end(pair), ctx->ev[EV_SORT_END]);
    account_iteration(st, n, h, ctx->n_live);
    threshold -= sim_step;
    diag_log_iteration(ctx, it, n, h, t_it);
  }
  if (ctx->kernel_timing && ctx->kstamp && st && ctx->kt_iter > kt_first)  // per-class spans
    if (int e = collect_kernel_times(ctx, (int)((ctx->kt_iter - 1) & 1u), st)) return e;
  return 0;
}

}  // namespace klsh

using namespace klsh;

extern "C" int klsh_cluster(klsh_ctx* ctx, float min_similarity, int iterations,
                            int bucket_size_threshold, uint32_t seed_base, uint64_t* rng_counter,
                            uint64_t* nt_trace, klsh_stats* stats) {
  if (!ctx || !rng_counter) return fail(KLSH_E_ARG, "null argument");
  if (!ctx->loaded) {
    if (ctx->comm) ctx->comm->abort();  // the other ranks must not wait for this one
    return fail(KLSH_E_STATE, "klsh_cluster before a load");
  }
  KLSH_HIP(hipSetDevice(ctx->device));
  if (stats && stats->struct_size != sizeof(klsh_stats))
    return fail(KLSH_E_ARG, "klsh_stats.struct_size != sizeof(klsh_stats): built against another "
                            "klsh.h (KLSH_ABI_VERSION " + std::to_string(KLSH_ABI_VERSION) + ")");
  klsh_stats local{};
  klsh_stats* st = stats ? stats : &local;
  memset(st, 0, sizeof(*st));
  st->struct_size = sizeof(*st);
  st->world = (uint64_t)ctx->world();
  ctx->mp.no_counts(), ctx->mp.huge_quiet = 0;  // (the single-device loop sets it per iteration)
  ctx->tail_local_iters = 0;
  const int run_iters = ctx->stop_after > 0 ? std::min(iterations, ctx->stop_after) : iterations;
  if (ctx->comm)  // any bound group, world 1 included (measures the sharded machinery alone)
    return cluster_sharded(ctx, min_similarity, iterations, run_iters, bucket_size_threshold,
                           seed_base, rng_counter, nt_trace, st);
  const double t_start = now_ms();

  // cluster.cc:190-192 (all float)
  const float max_similarity = 0.95f;
  const float sim_step = (max_similarity - min_similarity) / (float)iterations;
  float threshold = max_similarity;

  ctx->ctr_clean = false;
  ctx->drop_queued_projection();
  // no run counts yet: only very large inputs start with the 385..896-row class on aux 2
  ctx->mp.big896_aux = ctx->n_live >= (1u << 24) ? 1u : 0u;
  // Every call draws its hyperplanes afresh (the reference draws them inside Cluster(),
  // lshash.cc:36-42), so repeated timed calls never reuse a previous call's tables.
  ctx->w_count = 0;
  // Pre-draw the hyperplanes this call can need without nested buckets (h_t is non-increasing),
  // up to a bounded window; later ones are drawn when reached.
  if (ctx->n_live > 0 && iterations > 0) {
    if (int e = ctx->predraw_hyperplanes(seed_base, *rng_counter,
                                         (uint64_t)floor_log2(ctx->n_live), iterations,
                                         &st->host_ms))
      return e;
  }

  if (int e = run_single(ctx, threshold, sim_step, 0, run_iters, bucket_size_threshold, seed_base,
                         rng_counter, nt_trace, st))
    return e;
  // The survivor counters are published by the compaction's last workgroup, which need not be
  // the last to finish writing ctx->order: drain the stream before klsh_count/klsh_result read it.
  KLSH_HIP(hipStreamSynchronize(ctx->stream));
  if (ctx->pp.v.ws) {  // pairs the certified projection screens left to the exact chains
    uint32_t w[64];
    KLSH_HIP(hipMemcpy(w, ctx->pp.v.ws, sizeof(w), hipMemcpyDeviceToHost));
    KLSH_HIP(hipMemset(ctx->pp.v.ws + 4, 0, 8));
    KLSH_HIP(hipMemset(ctx->pp.v.ws + 32, 0, 128));
    st->proj_fix_pairs = proj_close_pairs(w);
  }
  st->n_final = ctx->n_live;
  st->wall_ms = now_ms() - t_start;
#ifdef KLSH_MERGE_PROF
  if (getenv("KLSH_MERGE_PROF")) merge_prof_dump(stderr);
#endif
  return 0;
}
