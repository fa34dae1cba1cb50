// The engine's context (klsh_ctx behind include/klsh.h) and the host helpers every host unit
// shares: the one error path, the HIP error macro, the clock, device allocation.  Included only
// by .cpp files; klsh_internal.h stays the host <-> kernel interface the .hip files read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "klsh.h"
#include "klsh_comm.h"
#include "klsh_internal.h"

extern "C" void klsh_host_hyperplanes(uint32_t base, uint64_t k0, uint64_t count, int d,
                                      int stride, float* out, int threads);  // klsh_host_rng.cpp

namespace klsh {

// Sets klsh_last_error() of the calling thread (klsh_ctx.cpp holds the message), returns code.
int fail(int code, const std::string& msg);
inline int set_error(int code, const char* msg) { return fail(code, msg); }
// fail(KLSH_E_HIP, "<call> -> <HIP's error string>")
int hip_fail(const char* call, hipError_t e);

inline double now_ms() {
  return std::chrono::duration<double, std::milli>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

inline int floor_log2(uint64_t n) { return (int)std::floor(std::log2((double)n)); }  // cluster.cc:194

template <class T>
int dalloc(T** p, size_t count) {
  *p = nullptr;
  if (count == 0) count = 1;
  if (hipMalloc((void**)p, sizeof(T) * count) != hipSuccess) {
    *p = nullptr;
    return fail(KLSH_E_NOMEM, "hipMalloc of " + std::to_string(sizeof(T) * count) + " bytes");
  }
  return 0;
}

template <class T>
void dfree(T*& p) {
  if (p) (void)hipFree((void*)p);
  p = nullptr;
}

// Owners of what a function or an object allocates for its own lifetime: device memory, pinned
// host memory, an event, an open file.  Move-only; the destructor releases.  (The long-lived
// members of klsh_ctx, Rows, RunLists and Snapshot stay raw pointers: they are passed to kernels
// by value and released in release().)
template <class T, bool Pinned = false>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.release()) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    reset(o.release());
    return *this;
  }
  ~DevBuf() { reset(); }
  // `count` elements (one at least) in place of what was held
  hipError_t alloc(size_t count) {
    reset();
    const size_t bytes = sizeof(T) * (count ? count : 1);
    const hipError_t e = Pinned ? hipHostMalloc((void**)&p_, bytes, hipHostMallocDefault)
                                : hipMalloc((void**)&p_, bytes);
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* release() { return std::exchange(p_, nullptr); }
  void reset(T* p = nullptr) {
    if (p_) (void)(Pinned ? hipHostFree((void*)p_) : hipFree((void*)p_));
    p_ = p;
  }

 private:
  T* p_ = nullptr;
};
template <class T>
using PinBuf = DevBuf<T, true>;

template <class T>  // dalloc's error for an owned buffer
int dalloc(DevBuf<T>& b, size_t count) {
  if (b.alloc(count) == hipSuccess) return 0;
  return fail(KLSH_E_NOMEM, "hipMalloc of " + std::to_string(sizeof(T) * (count ? count : 1)) + " bytes");
}

class Event {
 public:
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (e_) (void)hipEventDestroy(e_);
  }
  hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e_, flags); }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

struct FileClose {
  void operator()(FILE* f) const { (void)fclose(f); }
};
using File = std::unique_ptr<FILE, FileClose>;

// The (row, hyperplane) pairs the certified projection screens left to the exact chains, from a
// copy of ProjectView::ws: ws[4..6) the wide-row fix-up kernel's total, ws[32..64) the fp16
// screen's 16 counters.
inline uint64_t proj_close_pairs(const uint32_t (&w)[64]) {
  unsigned long long fixed = 0, part = 0;
  for (int i : {4, 32, 34, 36, 38, 40, 42, 44, 46, 48, 50, 52, 54, 56, 58, 60, 62}) {
    memcpy(&part, w + i, sizeof(part));
    fixed += part;
  }
  return fixed;
}

inline float elapsed(hipEvent_t a, hipEvent_t b) {
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0.0f;
  return ms;
}

struct Snapshot {
  bool valid = false;
  uint64_t n_live = 0;
  float* x = nullptr;
  float* nrm = nullptr;
  uint32_t *cnt = nullptr, *head = nullptr, *tail = nullptr, *nxt = nullptr, *order = nullptr;
};

// The timing events of the loops (klsh_ctx::ev).  The projection has two pairs: an iteration's
// projection queued behind the previous compaction is timed by the pair the previous iteration
// did not use (QueuedProjection::pair).
enum Ev {
  EV_PROJECT_BEGIN, EV_PROJECT_END, EV_MERGE_BEGIN, EV_MERGE_END, EV_COMPACT_END, EV_SORT_END,
  EV_PROJECT2_BEGIN, EV_PROJECT2_END, EV_COUNT,
  // the sharded loop never queues a projection: the end of its pair exchange takes that slot
  EV_EXCHANGE_END = EV_PROJECT2_BEGIN,
  // the result's list ranking (no loop is running then)
  EV_RANK_BEGIN = EV_PROJECT_BEGIN, EV_RANK_END = EV_PROJECT_END,
};

// Queued-ahead projection (small iterations, where no bucket can be oversize): the next
// iteration's sign-hash is enqueued behind the compaction, reading N from n_next_dev, before the
// host has the counters.
struct QueuedProjection {
  bool pending = false;
  uint64_t k = 0;     // its first hyperplane
  int pair = 0;       // the event pair around it (klsh_ctx::project_begin / project_end)
  bool swap = false;  // its keys went to keys2 (the queuing iteration's sorted keys were in keys)
};

}  // namespace klsh

using klsh::dalloc;
using klsh::dfree;
using klsh::fail;
using klsh::now_ms;
using klsh::set_error;

#define KLSH_HIP(call)                                        \
  do {                                                        \
    hipError_t e_ = (call);                                   \
    if (e_ != hipSuccess) return klsh::hip_fail(#call, e_);   \
  } while (0)

namespace klsh {

// One batch of reads on the device (modes E and K): the bases, the n + 1
// read offsets, and the event pair around the batch's kernel.  Each buffer is replaced when a
// batch does not fit; how large the new sequence buffer is, is the caller's rule.
struct ReadBatch {
  DevBuf<uint8_t> seq;
  DevBuf<uint64_t> off;
  uint64_t cap_b = 0, cap_r = 0;  // bytes of seq, entries of off
  Event e0, e1;

  int init() {
    KLSH_HIP(e0.create());
    KLSH_HIP(e1.create());
    return KLSH_OK;
  }
  // nb bases and the offsets of n reads queued for upload; a sequence buffer that does not hold
  // nb + 64 bytes is replaced by one of grow_bytes
  int upload(const void* hseq, uint64_t nb, const uint64_t* hoff, uint64_t n, uint64_t grow_bytes,
             hipStream_t s) {
    if (nb + 64 > cap_b) {
      cap_b = 0;
      KLSH_HIP(seq.alloc(grow_bytes));
      cap_b = grow_bytes;
    }
    if (n + 1 > cap_r) {
      cap_r = 0;
      KLSH_HIP(off.alloc(n + 1));
      cap_r = n + 1;
    }
    if (nb) KLSH_HIP(hipMemcpyAsync(seq, hseq, nb, hipMemcpyHostToDevice, s));
    KLSH_HIP(hipMemcpyAsync(off, hoff, (n + 1) * 8, hipMemcpyHostToDevice, s));
    return KLSH_OK;
  }
};

}  // namespace klsh

namespace klsh {

// klsh_save_clusters' test hooks and what the last call on the context reached (klsh_options.cpp)
struct SaveHooks {
  uint64_t chunk_bytes = 0;   // "save_chunk_bytes": bytes per device-to-host chunk (0 = 64 MB)
  uint64_t offset_base = 0;   // "save_offset_base": the position the text scan starts from
  uint64_t chunks = 0;        // "save_chunks"
  uint32_t ids_uploaded = 0;  // "save_ids_uploaded"
};

// klsh_diff_ksets' test hook (klsh_options.cpp)
struct DiffHooks {
  uint64_t chunk_bytes = 0;  // "diff_chunk_bytes": bytes per host-to-device chunk (0 = 64 MB)
};

// The device FASTQ parser's options and what the context's last mode-E / mode-K call reached
// (klsh_options.cpp, klsh_fastq.cpp)
struct FastqHooks {
  int parse = 0;               // "fastq_parse": 0 = auto (device, host on a takeover; the default
                               // by the measurement of DESIGN.md §16.6), 1 = host
                               // reader only, 2 = device only (a takeover is an error)
  uint64_t chunk_bytes = 0;    // "fastq_chunk_bytes": bytes per chunk (0 = 64 MB)
  uint64_t device_chunks = 0;  // "fastq_device_chunks"
  uint64_t device_reads = 0;   // "fastq_device_reads"
  uint64_t host_reads = 0;     // "fastq_host_reads"
  uint64_t takeover_at = ~0ull;  // "fastq_takeover_at": the file offset the host reader started at
  double parse_ms = 0.0;       // "fastq_parse_us": HIP-event time of the parser's kernels
  double read_ms = 0.0;        // "fastq_read_us": host time of the chunks' positioned file reads
};

// klsh_extract.cpp: the reader of klsh_fastq_open on a plain file from byte `offset` on, a record
// boundary (the host takeover of the device parser)
klsh_fastq* fastq_open_at(const char* path, uint64_t offset, int* err);

// klsh_result_host.cpp: the kernels of klsh_result.hip over the live order (see there)
int device_result(klsh_ctx* ctx, uint32_t* d_off, uint32_t* d_nodes, uint32_t* d_labels,
                  uint64_t* total_out);

}  // namespace klsh

struct klsh_ctx {
  using Counters = klsh::Counters;

  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[klsh::EV_COUNT] = {};
  hipEvent_t sev[2] = {};  // around the small-run merge launch (HIP-event cross-check)
  hipEvent_t project_begin(int pair) const {
    return ev[pair ? klsh::EV_PROJECT2_BEGIN : klsh::EV_PROJECT_BEGIN];
  }
  hipEvent_t project_end(int pair) const {
    return ev[pair ? klsh::EV_PROJECT2_END : klsh::EV_PROJECT_END];
  }
  // per-kernel-class stamps (klsh_stats.kern, KStampBlock in klsh_internal.h): the timed
  // iterations of a call stamp sets kt_iter & 1 in turn
  klsh::KStampBlock* kstamp = nullptr;
  uint64_t kt_iter = 0;
  klsh::LookBack lb{nullptr, 0};  // the one-launch compaction of small iterations
  bool kernel_timing = true;  // option "kernel_timing"
  bool hip_events = false;    // option "hip_events": HIP event pairs around the projection and
                              // the small-run merge (cross-checks of the stamps; cost latency)

  // sizes
  int d = 0, dp = 0;
  uint64_t slots = 0, members = 0, n_live = 0;
  uint64_t cap_slots = 0, cap_members = 0;
  int cap_dp = 0;
  bool loaded = false;

  // device state
  klsh::Rows rows{};
  uint32_t* order = nullptr;  // canonical live slots
  uint32_t* alt = nullptr;    // second slot buffer (sort / compaction ping-pong)
  uint32_t* keys = nullptr;
  uint32_t* keys2 = nullptr;
  uint32_t* nk1 = nullptr;    // nested scratch
  uint32_t* nk2 = nullptr;
  uint32_t* nv2 = nullptr;
  uint32_t* hist = nullptr;
  uint32_t* tile_sums = nullptr;
  klsh::MergePlan mp{};
  uint32_t grid_cap = 0;  // option "grid_cap" (tests; 0 = off): every unit's launches (cap_grid)
  klsh::ProjectPlan pp{};     // wide-row matrix-core projection: fix-up list
  Counters* ctr = nullptr;
  Counters* h_ctr = nullptr;  // pinned
  float* W = nullptr;         // hyperplane pool on the device, [k - w_k0][dp]
  uint64_t w_k0 = 0, w_count = 0, w_cap = 0, w_alloc = 0;
  uint32_t w_base = 0;
  int w_dp = 0, w_d = 0;
  // The call's window drawn in the background (predraw_hyperplanes): a host thread draws rows
  // [w_k0, w_k0 + w_target) in order into pinned memory and publishes how many are done
  // (w_drawn); ensure_hyperplanes uploads the drawn rows it needs on the stream, without a
  // stream sync — the host RNG (~3.5 ms per C2 call, ~25 ms at C5's d = 512) runs beside the
  // GPU's first iterations instead of in front of them.
  std::thread drawer;
  std::atomic<uint64_t> w_drawn{0};
  std::atomic<bool> draw_stop{false};
  uint64_t w_target = 0;
  float* w_pin = nullptr;
  size_t w_pin_floats = 0;

  // host
  std::vector<uint64_t> ids;  // member node -> k-mer id
  // the load defined ids[node] = ids_base + node (klsh_load_counts; a null member_ids of the other
  // loads): klsh_save_clusters then formats base + node and uploads nothing.  Cleared by a load
  // that takes explicit ids, kept by a keep-mode klsh_load_clusters_device.
  bool ids_linear = false;
  uint64_t ids_base = 0;
  void set_ids_linear(bool linear, uint64_t base) { ids_linear = linear, ids_base = linear ? base : 0; }
  klsh::Snapshot snap;

  // sharded loop: this rank's exchange and its buffers (sized with the slots)
  klsh::Comm* comm = nullptr;
  uint2* sbuf = nullptr;       // (key, slot) pairs grouped by destination rank
  uint2* rbuf = nullptr;       // (key, slot) pairs received, in source-rank order
  uint32_t* mark = nullptr;    // [slots] iteration stamp of the last rewrite (in-place kernels)
  uint32_t stamp = 0;
  uint32_t* dslots = nullptr;  // survivors rewritten by a merge (this rank)
  uint32_t* bins = nullptr;    // [4096] key-bin histogram of this rank
  uint32_t* bins_all = nullptr;
  uint32_t* owner = nullptr;   // [4096] bin -> rank
  uint32_t* cntmat = nullptr;  // [W][W] pairs rank g sends rank r
  uint32_t* small = nullptr;   // [W + 1][4] per-rank counters exchange
  uint32_t* h_small = nullptr; // pinned: cntmat or the counters exchange
  // mapped: the sharded loop's per-iteration publishes (k_publish_words): [sequence word, 64 B]
  // [payload]; host and device views
  uint32_t* shp_host = nullptr;
  uint32_t* shp_dev = nullptr;
  uint32_t shp_seq = 0;
  uint32_t* drec = nullptr;    // delta records of this rank, then of all ranks
  uint32_t* drec_all = nullptr;
  size_t drec_cap = 0, drec_all_cap = 0;  // words
  uint64_t shard_cap = 0;
  double t_enqueued = 0.0;  // diagnostics (KLSH_ITER_LOG): host time when an iteration was queued
  // Counters through mapped pinned memory (klsh::Publish): the host polls pub_seq instead of a
  // copy launch + stream sync after every iteration (a copy + sync if mapped memory is refused).
  Counters* pub_host = nullptr;   // host view
  Counters* pub_dev = nullptr;    // device view of the same memory
  uint32_t* pub_seq_host = nullptr;
  uint32_t* pub_seq_dev = nullptr;
  uint32_t pub_seq = 0;
  // Queued tail batches (run_batched): every iteration publishes into its own ring slot, the host
  // waits for the last sequence number of a chunk and reads the chunk's slots.
  static constexpr int kRing = 2 * 32;
  Counters* ring_host = nullptr;
  Counters* ring_dev = nullptr;
  bool ctr_clean = false;  // *ctr is known to be zero (the publisher zeroed it)
  uint32_t* n_next_dev = nullptr;  // N (and the hyperplane offset) the queued launches read
  klsh::QueuedProjection spec;
  // This iteration's projection is on the stream already (queued by the previous one): claims it
  // and points `keys` at the buffer it wrote.
  bool take_queued_projection() {
    const bool queued = spec.pending;
    if (queued && spec.swap) std::swap(keys, keys2);
    drop_queued_projection();
    return queued;
  }
  void drop_queued_projection() { spec.pending = spec.swap = false; }
  bool zero_copy = true;
  klsh::RunCounters* rc = nullptr;  // run-list counters (device, one 128-B line each)
  // fp16 image of the rows for the projection's screen (Rows::xh), kept at d = 16, 32, 64 unless
  // option "projection" asks for the exact packed chains; every row store of the merge kernels
  // writes it too (store_row4 / store_row1)
  uint16_t* xh_alloc = nullptr;
  bool shadow_wanted(int d_) const {
    return pp.variant != klsh::kProjPacked && klsh::shadow_width_ok(d_);
  }
  // Queued tail batches (run_batched; option "tail_batch", default on), their bucket sort as a
  // top-bits pass + the LDS bucket sort that lists the runs (option "tail_local", default on)
  bool tail_batch = true;
  bool tail_local = true;
  // queued iterations of the last klsh_cluster call whose sort took that local path (read-only
  // option "tail_local_iters": counted by the host where run_batched enqueues them)
  uint64_t tail_local_iters = 0;
  // klsh_hash_keys diagnostics (klsh_get_option): the projection kernel of the last call and
  // the (row, hyperplane) pairs its screen left to the exact chains
  int last_hash_kernel = klsh::kPkNone;
  int last_hash_variant = klsh::kPvNone;
  uint64_t last_hash_close = 0;
  // the result on the device: option "result_device" (klsh_count / klsh_result
  // through the offsets scan and the list ranking) and the ranking rounds of the last such result
  bool result_device = false;
  uint32_t result_rounds = 0;
  int64_t result_rank_us = 0;  // HIP-event time of those rounds (without the init launch)
  // klsh_build_khtable's test hooks and reach counters (klsh_kmc.cpp)
  klsh::KmcHooks kmc;
  // klsh_count_khtable's (klsh_kcount.cpp)
  klsh::KcountHooks kcount;
  // klsh_save_clusters' (klsh_save.cpp)
  klsh::SaveHooks save;
  // klsh_diff_ksets' (klsh_diff.cpp)
  klsh::DiffHooks diff;
  // the device FASTQ parser's (klsh_fastq.cpp)
  klsh::FastqHooks fastq;

  ~klsh_ctx() { release(); }

  // Per-phase HIP events (sort / merge / compaction) cost latency in every iteration — an event
  // record on the stream is tens of microseconds in the small late iterations — so they are on
  // only with option "phase_timing".  The projection is bracketed with it or with "hip_events".
  bool phase_timing = false;

  // Sharded loop: below this many live rows the per-iteration exchanges cost more than they save
  // (the late iterations are latency-bound on one GPU already), so every rank takes the whole
  // canonical order and runs the remaining iterations on its replica — identically, with no
  // communication.  klsh_set_option(ctx, "shard_min_rows", n); 0 = always sharded.
  uint64_t shard_min_rows = 1u << 21;
  // an iteration over n live rows runs sharded (a bound group, above the threshold)
  bool shards(uint64_t n) const { return comm && n >= shard_min_rows; }
  // option "comm_timeout_s": a collective that has not completed after this long aborts the group
  double comm_timeout_s = 600.0;

  // "stop_after" (klsh_set_option): run only the first k iterations of a call's threshold
  // schedule (0 = all).  Prefix parity tests of the long configs use it; results of the
  // iterations that do run are unchanged.
  int stop_after = 0;
  hipEvent_t counts_ev = nullptr;  // sharded loop: the send counts are on the host
  int progress = 0;  // option "progress": a line on stderr every this many iterations (profiling runs)
  void tick(int it) const {
    if (progress > 0 && it % progress == 0) {
      fprintf(stderr, "[klsh] iteration %d\n", it);
      fflush(stderr);
    }
  }
  // "hyperplane_window" (klsh_set_option): rows drawn up front per call (0 = the default bound)
  uint64_t hyperplane_window = 0;
  // "hyperplane_async" (klsh_set_option): 1 (default) = the call's window drawn by a background
  // thread while the loop starts (predraw_hyperplanes); 0 = drawn and uploaded before it
  uint32_t hyperplane_async = 1;

  int world() const { return comm ? comm->world : 1; }
  int rank() const { return comm ? comm->rank : 0; }

  // ---- klsh_ctx.cpp ----
  void release_shard();
  int reserve_shard();
  int reserve_words(uint32_t** p, size_t* cap, size_t words);
  void release_state();
  void drop_snapshot();
  void join_drawer();
  void release();
  // k_merge_long's bit matrices (runs over 896 rows at d = 16 / 32): one per workgroup, a
  // workgroup per 897 slots up to 256 (2 MB each: up to 512 MB).  None while option long_runs
  // is 0 (k_merge_huge walks those runs; the matrices are released when it is switched off).
  int ensure_long(uint64_t s, int d_);
  // (Re)allocate device state for `ns` slots, `nm` member nodes, row width d.
  int reserve(uint64_t ns, uint64_t nm, int d_);
  // Option "projection" changed: keep the fp16 image (allocated and rebuilt from x) or drop it.
  int apply_projection_variant();
  // Rows [k0, k0 + count) inside the background-drawn window: true when ensure_hyperplanes can
  // append them without touching rows the stream may be reading.
  bool lazy_covers(uint32_t base, uint64_t k0, uint64_t count) const {
    return w_target && W && w_base == base && w_dp == dp && w_d == d && k0 >= w_k0 &&
           k0 + count <= w_k0 + w_target;
  }
  // Make hyperplanes [k0, k0+count) of stream `base` resident on the device (drawn on the host).
  // The resident window [w_k0, w_k0 + w_count) only grows forward; anything else restarts it.
  int ensure_hyperplanes(uint32_t base, uint64_t k0, uint64_t count, double* host_ms);
  // an empty window of stream `base` starting at row k0, with room for `rows` rows at least
  int restart_window(uint32_t base, uint64_t k0, uint64_t rows);
  const float* hyperplane_ptr(uint64_t k) const { return W + (k - w_k0) * (uint64_t)dp; }
  int predraw_hyperplanes(uint32_t base, uint64_t k0, uint64_t hmax, int iterations,
                          double* host_ms);
  // zero the iteration counters (and the run-list counters) on the stream
  int reset_counters();
  int sync_counters();
  // Wait for the counters the compaction published with sequence number `seq`; they are in
  // *h_ctr afterwards.
  int wait_published(uint32_t seq);
  // Wait until the published sequence word reaches `seq` (queued batches publish one sequence
  // number per iteration, so the word may already be past it).
  int wait_seq(uint32_t seq);
  int check_device_err() const;
  // p must be memory of this context's device (the device entry points' pointer arguments).
  int check_device_ptr(const void* p, const char* what) const;
};

// A differential k-mer set (klsh_kset_create in klsh_extract.cpp, klsh_diff_ksets in
// klsh_diff.cpp): the k-mer table of klsh_kmer.h, `mask + 1` slots, built from n keys.
struct klsh_kset {
  klsh_ctx* ctx = nullptr;
  klsh::DevBuf<uint64_t> tab;
  uint64_t mask = 0;
  uint64_t n = 0;
};
