// The pieces of an LSH iteration the loops share (klsh_loop.cpp: single device and queued tail;
// klsh_loop_sharded.cpp: sharded) and the test hook klsh_pcluster.
#pragma once
#include <functional>
#include <vector>

#include "klsh_ctx.h"

namespace klsh {

// One finished iteration over n rows with h hyperplanes that left n_next (n = 0: the reference
// aborts on an empty vector, here the iteration only counts).
inline void account_iteration(klsh_stats* st, uint64_t n, int h, uint64_t n_next) {
  st->iterations += 1;
  if (n == 0) return;
  st->hyperplanes += (uint64_t)h;
  st->project_launches += 1;
  st->sum_rows += n;
  st->sum_proj_bits += n * (uint64_t)h;
  st->sum_merges += n - n_next;
}

// Merge + compaction of one iteration's sorted runs (fk/fv, n positions, in place on fv) into
// `out`.  Ends with the counters on the host: total (survivors), n_over (oversize runs), n_delta.
// kt: the iteration's stamps (kNoTime: untimed).  sink (sharded loop): where the merge kernels
// list the survivors they rewrote.
int merge_main(klsh_ctx* ctx, uint32_t* fk, uint32_t* fv, uint32_t n, float thr, int bucket_thr,
               uint32_t* out, klsh_stats* st, bool timed, bool sync = true,
               const std::function<int(uint32_t*)>* after = nullptr, KTime kt = kNoTime,
               const DeltaSink& sink = kNoSink);
// The oversize runs of the last merge_main, ascending (the reference's T=1 order):
// (start, length) pairs and the hyperplanes their nestedCluster calls draw (floor(log2 b) each).
int oversize_runs(klsh_ctx* ctx, std::vector<uint2>* over, uint64_t* hyperplanes);
// nestedCluster (cluster.cc:286-288 -> :89-178) for each oversize run, ascending, drawing
// hyperplanes from *rng_counter on; then the survivors are compacted again into `out`.  Ends with
// the counters on the host.
int merge_nested(klsh_ctx* ctx, uint32_t* fk, uint32_t* fv, uint32_t n, float thr,
                 const std::vector<uint2>& over, uint32_t seed_base, uint64_t* rng_counter,
                 uint32_t* out, klsh_stats* st, const DeltaSink& sink = kNoSink);
// Single-GPU: merge, compaction and nested buckets of one iteration.  fk/fv: sorted keys/slots
// (fv is one of ctx->order / ctx->alt).  Returns with the new canonical order in ctx->order and
// ctx->n_live updated.
int merge_and_compact(klsh_ctx* ctx, uint32_t* fk, uint32_t* fv, uint32_t n, float thr,
                      int bucket_thr, uint32_t seed_base, uint64_t* rng_counter, klsh_stats* st,
                      bool timed, const std::function<int(uint32_t*)>* after = nullptr,
                      KTime kt = kNoTime);
// Iterations [it_begin, it_end) of the single-device loop over the whole canonical order
// (cluster.cc:193-334).  `threshold` is advanced by sim_step per iteration.
int run_single(klsh_ctx* ctx, float& threshold, float sim_step, int it_begin, int it_end,
               int bucket_size_threshold, uint32_t seed_base, uint64_t* rng_counter,
               uint64_t* nt_trace, klsh_stats* st);
// klsh_cluster on a context bound to a comm group (klsh_loop_sharded.cpp).
int cluster_sharded(klsh_ctx* ctx, float min_similarity, int iterations, int run_iters,
                    int bucket_size_threshold, uint32_t seed_base, uint64_t* rng_counter,
                    uint64_t* nt_trace, klsh_stats* st);

}  // namespace klsh
