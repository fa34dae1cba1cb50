/* klsh — MI355X-native LSH k-mer clustering engine: the C-ABI drop-in boundary.
 *
 * The reference (wthanone/kmerLSH) has no plugin/FFI layer; its seam for this hot path is the C++
 * function
 *     void Cluster(vector<Abundance*>* rows, float min_similarity, int cluster_iteration,
 *                  unsigned threads_to_use, int dim, int bucket_size_threshold, bool verbose)
 * (reference function/cluster.h:42, body function/cluster.cc:181-340), called from
 * app/kmerLSH.cc:323 (init pass), :377 (re-cluster passes) and :490 (main loop).  The entry points
 * below replace that call and the functions on its path; include/klsh_cluster.hpp wraps them back
 * into the reference's exact signature.
 *
 * Conventions: every int-returning call returns 0 or a negative KLSH_E_* code; no C++ exception
 * crosses this boundary.  The library owns device memory; the caller owns every host buffer
 * (size queries first: klsh_count).  One context per host thread; not re-entrant on one context.
 * All host pointers are plain host memory; nothing here takes or returns a torch type.
 *
 * Determinism: results equal the reference at -T 1 (OMP_THREAD_LIMIT=1) with the seeding
 * convention of SURVEY.md §8(c): hyperplane k of a run is drawn from
 * std::mt19937(seed_base + k*2654435761) with std::normal_distribution<double>(0,1), cast to
 * float.  `rng_counter` carries k across calls (init pass, then main loop).
 */
#ifndef KLSH_H
#define KLSH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KLSH_OK 0
#define KLSH_E_ARG (-1)      /* bad argument (null pointer, d <= 0, sizes) */
#define KLSH_E_HIP (-2)      /* a HIP runtime call failed (message: klsh_last_error) */
#define KLSH_E_NOMEM (-3)    /* device or host allocation failed */
#define KLSH_E_STATE (-4)    /* call out of order (e.g. klsh_cluster before a load) */
#define KLSH_E_NODEVICE (-5) /* no gfx950 device visible: the engine has no CPU fallback */
#define KLSH_E_RANGE (-6)    /* a size exceeds what the engine supports (rows >= 2^32, d > 4096) */

/* ABI version of this header.  2: every statistics struct starts with `struct_size`, which the
 * caller sets to sizeof(the struct) (the library refuses a mismatch instead of writing past a
 * smaller struct); klsh_get_option.  3: klsh_stats.kern has KLSH_KCLASSES = 13 classes (the
 * merge-phase wall, KLSH_K_MERGE). */
#define KLSH_ABI_VERSION 3

typedef struct klsh_ctx klsh_ctx;

/* Per-kernel-class statistics of a call: summed span of the class's launches (first workgroup
 * start to last workgroup end, read from the GPU clock inside the kernels), launches, and the
 * rows they handled (the unit of each class's algorithmic bytes).
 * Index = KLSH_K_*. */
#define KLSH_K_PROJECT 0  /* sign-hash of every live row (k_project_*) */
#define KLSH_K_SORT 1     /* stable bucket sort, all passes (span of the first to last launch) */
#define KLSH_K_RUNS 2     /* run finding and size-class lists (span) */
#define KLSH_K_SMALL 3    /* runs of 2..64 rows (k_merge_small; d > 64: the k_merge_group_wide chain) */
#define KLSH_K_BIG128 4   /* runs of 65..128 rows (k_merge_big / k_merge_big_wide) */
#define KLSH_K_BIG192 5   /* 129..192 */
#define KLSH_K_BIG384 6   /* 193..384 */
#define KLSH_K_BIG896 7   /* 385..896 */
#define KLSH_K_HUGE 8     /* longer runs (k_merge_huge) */
#define KLSH_K_TAIL 9     /* iterations below tail_merge_rows positions (default 2^22): every merge
                             class in one k_merge_tail */
#define KLSH_K_COMPACT 10 /* survivor compaction (span) */
#define KLSH_K_SCREEN 11  /* fp16 screen of the runs of 2..64 rows (SMALL then merges the ones left) */
#define KLSH_K_MERGE 12   /* a phase, not a kernel: the merge launches of each iteration at >=
                             tail_merge_rows positions (default 2^22), and of every iteration at
                             d > 64, together — first workgroup start of any merge class to the
                             last end (their concurrent wall) */
#define KLSH_KCLASSES 13
typedef struct klsh_kstat {
  double ms;
  uint64_t launches;
  uint64_t rows;
  uint64_t runs;
} klsh_kstat;

/* Per-call statistics (all times are milliseconds). */
typedef struct klsh_stats {
  uint64_t struct_size;    /* in: sizeof(klsh_stats) (KLSH_ABI_VERSION check) */
  uint64_t iterations;     /* iterations run */
  uint64_t sum_rows;       /* sum over iterations of N_t (rows projected) */
  uint64_t sum_merges;     /* sum over iterations of M_t = N_t - N_{t+1} */
  uint64_t sum_proj_bits;  /* sum over iterations of N_t * h_t (row-hyperplane dot products) */
  uint64_t nested_calls;   /* oversize buckets sent through nestedCluster */
  uint64_t hyperplanes;    /* hyperplanes drawn by this call */
  uint64_t n_final;        /* live rows after the call */
  uint64_t project_launches;        /* projection launches (every iteration has one) */
  uint64_t project_timed_launches;  /* the ones inside project_ms (queued tail batches carry no
                                       HIP events; their time is in kern[KLSH_K_PROJECT]) */
  double wall_ms;          /* host wall clock of the whole call */
  double project_ms;       /* HIP-event time of project_timed_launches projection launches */
  double sort_ms;          /* HIP-event time of the bucket (radix) sort */
  double merge_ms;         /* HIP-event time of the greedy in-bucket merge kernels */
  double compact_ms;       /* HIP-event time of the survivor compaction */
  double host_ms;          /* host-side hyperplane generation */
  double comm_ms;          /* sharded loop: host time in inter-rank exchanges (incl. waits) */
  uint64_t world;          /* ranks the call ran on (1 = single GPU) */
  /* the small-run merge (runs of 2..64 rows) of the iterations where it is a launch of its own
   * (>= 2^20 positions): HIP-event time on its stream, launches, rows in those runs, merges of
   * the whole iteration (small-run merges are ~97% of them on C2) */
  double small_ms;
  uint64_t small_launches;
  uint64_t small_rows;
  uint64_t small_iter_merges;
  /* per kernel class (single-GPU loop; option "kernel_timing", default on) */
  klsh_kstat kern[KLSH_KCLASSES];
  /* certified projection screens (d > 64, or the fp16 row image at d = 16, 32, 64): the
   * (row, hyperplane) pairs the screen could not call and the exact chains settled */
  uint64_t proj_fix_pairs;
} klsh_stats;

/* ---- lifetime ------------------------------------------------------------------------------- */
/* Create a context on HIP device `device` (ordinal).  *err receives the status. */
klsh_ctx* klsh_create(int device, int* err);
void klsh_destroy(klsh_ctx* ctx);
const char* klsh_last_error(void);  /* thread-local text for the last failure */
const char* klsh_version(void);
int klsh_abi_version(void);         /* KLSH_ABI_VERSION of the built library */

/* ---- loading the rows (replaces building vector<Abundance*>) ---------------------------------- */
/* rows: n x d fp32 row-major (reference common/abundance.h:18-36, `_values`).
 * member_offsets (n+1) / member_ids: each row's id list (`_ids`); NULL member_offsets means row i
 * is the singleton {member_ids ? member_ids[i] : i} (reference io/ioMatrix.cc:373). */
int klsh_load_rows(klsh_ctx* ctx, const float* rows, uint64_t n, int d,
                   const uint64_t* member_offsets, const uint64_t* member_ids);

/* The same load for rows that are in device memory already (an exception to "all pointers are
 * host memory"): d_rows is memory of the context's device, n rows of d floats, row i starting
 * i * row_stride floats in (row_stride >= d; a host pointer, another device's memory or a smaller
 * stride: KLSH_E_ARG, and the previous load stays).  Every row is a singleton, {member_ids ?
 * member_ids[i] : i}; member_ids is HOST memory.  Leaves exactly the state klsh_load_rows leaves
 * for the same rows.  The caller's writes to d_rows must be complete before the call; d_rows is no
 * longer read when it returns.  n = 0 is allowed. */
int klsh_load_rows_device(klsh_ctx* ctx, const float* d_rows, uint64_t n, int d,
                          uint64_t row_stride, const uint64_t* member_ids);

/* Rows that already have member lists, from device memory: the inverse of klsh_result_device,
 * and what klsh_load_rows(rows, n, d, member_offsets, member_ids) does for host arrays.  d_rows,
 * n, d and row_stride as in klsh_load_rows_device.  d_member_offsets (device, n + 1 entries) and
 * d_member_nodes (device, or NULL) give the lists: row i's members are d_member_nodes[offsets[i]
 * .. offsets[i + 1]), absolute indices — offsets[0] need not be 0, so a window `offsets + a` of a
 * longer array loads rows a.. of a concatenated set against its whole node array; m = offsets[n]
 * - offsets[0].  d_member_nodes NULL: entry q is node q - offsets[0].  The offsets must increase
 * strictly (a row without members would weigh 0/0 in a consensus).
 * Nodes are the caller's numbers in [0, M), no node twice; a node in no list is held by no row
 * (klsh_labels: KLSH_NO_LABEL, like a row klsh_load_counts dropped); option "member_nodes" reads M.
 *   n_nodes = M > 0  a new node space: member_ids (HOST memory, M entries, or NULL = k) is the id
 *                    of node k; m <= M
 *   n_nodes = 0      keep: the node space and the host-side ids of the context's current load stay
 *                    (member_ids must be NULL; KLSH_E_STATE if nothing is loaded) — the round trip
 *                    of klsh_result_device's outputs, whole, filtered or sliced, with no id leaving
 *                    the host vector and no host work per node
 * Leaves the state klsh_load_rows(rows, n, d, offsets - offsets[0], ids[nodes]) leaves, the nodes
 * numbered the caller's way: klsh_count, klsh_result and klsh_row_state give the same bytes,
 * klsh_result_device and klsh_labels speak in the caller's nodes.  The lists are checked and linked
 * by kernels, per entry (one row may hold every member).  Complete, and the three device arrays no
 * longer read, when it returns.  n = 0 is an empty load (the offsets may be NULL).
 * Refused before the context is touched, the previous load intact — KLSH_E_ARG: a host or
 * foreign-device pointer, row_stride < d, offsets not strictly increasing, m > M, a node >= M, a
 * node listed twice, member_ids with n_nodes = 0; KLSH_E_RANGE: d outside [1, 4096], n or M >=
 * 2^32.  klsh_last_error names the check and the smallest offending row or entry. */
int klsh_load_clusters_device(klsh_ctx* ctx, const float* d_rows, uint64_t n, int d,
                              uint64_t row_stride,
                              const uint32_t* d_member_offsets, /* device, n + 1 entries */
                              const uint32_t* d_member_nodes,   /* device, or NULL */
                              uint64_t n_nodes,                 /* M, or 0 = keep */
                              const uint64_t* member_ids);      /* HOST, M entries, or NULL */

/* Mode-C producer on the GPU (reference io/ioHT.cc:59-81 ReadHT + io/ioMatrix.cc:353-408
 * convertHTMat): counts is the whole sample-major kmer_count.bin image (d columns of n_total
 * uint16), the batch is rows [batch_offset, batch_offset+batch_size); v_kmers[j] =
 * coverage_j / kmap_size as the reference computes it (app/kmerLSH.cc:471-482).  Rows with
 * sum(count) <= 0.1*d are dropped; ids are batch_offset + i. */
int klsh_load_counts(klsh_ctx* ctx, const uint16_t* counts, uint64_t n_total,
                     uint64_t batch_offset, uint64_t batch_size, int d, const float* v_kmers);

/* Keep a device-side copy of the loaded state / restore it (for repeated timing; both are
 * device-to-device copies). */
int klsh_snapshot(klsh_ctx* ctx);
int klsh_restore(klsh_ctx* ctx);

/* ---- the hot path ------------------------------------------------------------------------------ */
/* Cluster() (reference function/cluster.cc:181-340) over the loaded rows: `iterations` rounds of
 * hyperplane draw -> sign-hash every live row -> stable bucket -> greedy cosine merge per bucket
 * (nestedCluster for buckets above bucket_size_threshold), threshold falling from 0.95 toward
 * min_similarity.  nt_trace (may be NULL) receives N_t at the start of each iteration.
 * stats may be NULL. */
int klsh_cluster(klsh_ctx* ctx, float min_similarity, int iterations, int bucket_size_threshold,
                 uint32_t seed_base, uint64_t* rng_counter, uint64_t* nt_trace, klsh_stats* stats);

/* ---- multi-GPU: one rank per GPU, the loop sharded by key range -------------- */
/* Every rank loads the same rows (replicas) and calls klsh_cluster with the same arguments; the
 * result — order, rows, member lists and rng_counter — is identical to the single-GPU call on
 * every rank.  RCCL (one process per GPU): rank 0 creates the 128-byte id, the caller ships it
 * to the other ranks (any side channel), each rank calls klsh_comm_init on its context. */
int klsh_comm_unique_id(uint8_t* id /* 128 bytes */);
int klsh_comm_init(klsh_ctx* ctx, int rank, int world, const uint8_t* id /* 128 bytes */);
/* In-process group over `world` contexts (any devices, several may share one GPU); each rank's
 * klsh_cluster must then run on its own host thread, concurrently.  For tests on one GPU. */
int klsh_comm_init_local(klsh_ctx** ctxs, int world);
int klsh_comm_info(klsh_ctx* ctx, int* rank, int* world);
/* Options of a context.  Results never depend on them, except "stop_after"
 * (tests/test_gpu_launch_geometry.py holds that claim for the launch sizes: every one of them at
 * 1, and "grid_cap" at 1 to 3, against the oracle and the models).
 *   "shard_min_rows"   sharded loop: below this many live rows every rank runs the remaining
 *                      iterations on its own replica, without exchanges (default 2^21; 0 = always)
 *   "phase_timing"     0/1: per-phase HIP events (adds latency; default 0)
 *   "kernel_timing"    0/1: the per-class statistics of klsh_stats.kern (default 1)
 *   "tail_batch"       0/1: queue the small late iterations 32 at a time (default 1)
 *   "tail_local"       0/1: their bucket sort as a top-10-bit pass + per-bucket LDS sorts that
 *                      also list the runs (default 1; 0 = the LSD passes + run kernels)
 *   "huge_fold"        1 (tests): runs over 896 rows always walked inside the 385..896-row
 *                      kernel (default 0: only after several iterations without such runs)
 *   "projection"       0 = the certified matrix-core screens where they exist (default: the fp16
 *                      row image at d = 16, 32, 64 — kept beside the rows, 2 bytes per value —
 *                      and bf16x3 above 64), 1 = the exact packed VALU chains only (no fp16 image)
 *   "stop_after"       k > 0: klsh_cluster runs only the first k iterations of its threshold
 *                      schedule, e.g. to pin a prefix of a long loop; 0 = all (default)
 *   "hyperplane_window" hyperplane rows drawn up front per call; the rest are drawn when the loop
 *                      reaches them (0 = default: all of them while they fit in 256 MB, else 64
 *                      iterations' worth)
 *   "comm_timeout_s"   a collective still incomplete after this many seconds aborts (default 600)
 *   launch sizes, 0 = the measured default, from 1 workgroup on: "h16_grid", "wide_grid",
 *   "fix_grid" (projection), "small_grid", "tail_big_groups", "tail_small_groups",
 *   "wide_group_grid", "small_screen_grid" (merge);
 *   "grid_cap"         (tests) N in [1, 2^20]: at most N workgroups for every launch that strides
 *                      over a list or an index range and has no size option of its own — the
 *                      per-class merges of 65-row and longer runs (k_merge_big, k_merge_big_wide,
 *                      k_merge_huge, k_merge_long, whose bit matrices stay allocated for the
 *                      uncapped count), the kernels of modes K, B and E, and the sharded loop's
 *                      bin histogram and delta pack / apply; 0 (default) = off.  It does not
 *                      reach the launches with one workgroup per tile, nor the kernels whose
 *                      workgroups wait for one another (the look-back scans and compaction, the
 *                      sort passes, the run listing, the local tail sort, the partition, the
 *                      packed and generic projections): fewer workgroups than tiles there is a
 *                      wrong result or a spin that runs into its limit
 *   "small_screen"     1 = runs of 2..64 rows are screened on the fp16 row image first and only
 *                      the ones the screen cannot rule out are merged on the f32 rows
 *   "tail_screen"      1 (default) = the fp16 small-run screen also runs in front of the one-launch
 *                      merge (k_merge_tail), whose small-run waves then walk only the runs it passed
 *   "tail_big_screen"  1 (default) = there, 65..384-row runs are first screened on the fp16 image
 *                      in their workgroup; a run with no pair within the margin reads no f32 row
 *   "tail_screen_grid" workgroups of that screen's persistent launch (0 = 2048)
 *   "hyperplane_async" 1 (default) = a call's hyperplanes are drawn on the host by a background
 *                      thread while its first iterations run (uploaded as they are needed, no
 *                      stream sync); 0 = drawn and uploaded before the loop starts
 *   "hip_events"       1 = HIP event pairs around the projection and the small-run merge of the
 *                      host-driven iterations (klsh_stats project_ms / small_ms, cross-checks of
 *                      the in-kernel stamps); 0 (default): none — a record costs ~9 us of stream
 *                      time per iteration
 *   "tail_merge_rows"  iterations below this many rows merge every class in one launch (default
 *                      2^22, at most 2^22 — the largest size its parity is pinned at; tests
 *                      lower it to reach the per-class launches at
 *                      small sizes).  Iterations below min(this, 2^20) rows are also queued
 *                      several at a time (one host sync per batch)
 *   "h16_segcap" (tests) caps the fp16 projection's per-workgroup fix-up segment.
 *   "h16_bound"        1 (default) = the fp16 projection (d = 16, 32, 64) certifies a sign against
 *                      eps * sum_k |x_k||w_k| (a third MFMA per k-step); 0 = against eps * |x||w|,
 *                      which leaves ~1.6x as many pairs to the exact chains.  Same keys either way
 *   "long_runs"        4 (default) = runs over 384 rows at d = 16 / 32 through k_merge_long
 *                      (Gram bit matrix + one walk step per merge); 1 = only runs over 896 rows;
 *                      0 = k_merge_huge for those
 *   "wide_unrolled"    1 (default) = d = 512 projected by the unrolled screen; 0 = the generic one
 *   "wide_gram"        at d = 512 the group merges of runs of at least this many rows (8, 16, 32
 *                      or 64; default 32) take their decisions from an MFMA Gram matrix with a
 *                      certified margin, the uncertain pairs from the exact chains; 0 = none
 *   "progress"         N > 0: a line on stderr every N iterations (long profiling runs) */
int klsh_set_option(klsh_ctx* ctx, const char* name, int64_t value);
/* Any option above, plus read-only diagnostics: "fp16_image" (1 = the loaded rows have the fp16
 * image), "last_hash_kernel" (klsh_hash_keys' projection kernel: 0 packed chains, 1 fp16-image
 * screen, 2 f32 fp16x3 wide-row screen, -1 none), "last_hash_variant" (the kernel itself: 0
 * k_project_pk, 1 k_project_wide_pk, 2 k_project_generic, 3 k_project_h16, 4
 * k_project_mfma_wide<512>, 5 k_project_mfma_wide<0>, -1 none),
 * "last_hash_close_pairs" (its (row, hyperplane) pairs settled by the exact chains) and
 * "tail_local_iters" (the queued iterations of the last klsh_cluster call whose bucket sort was
 * the top-bits pass + per-bucket LDS sorts of option "tail_local"; 0 where none was queued). */
int klsh_get_option(klsh_ctx* ctx, const char* name, int64_t* value);

/* ---- results ---------------------------------------------------------------------------------- */
int klsh_count(klsh_ctx* ctx, uint64_t* n_rows, uint64_t* n_members);
/* Canonical order: rows (n_rows*d), member_offsets (n_rows+1), member_ids (n_members); any may
 * be NULL. */
int klsh_result(klsh_ctx* ctx, float* rows, uint64_t* member_offsets, uint64_t* member_ids);

/* The result on the device.  Its currency is the member NODE: the loaded members
 * numbered 0 .. M-1 in load order (M: option "member_nodes"), whatever their ids —
 *   after klsh_load_rows         node k is entry k of the loaded member_ids (row k when
 *                                member_offsets is NULL),
 *   after klsh_load_rows_device  node k is input row k,
 *   after klsh_load_counts       node k is batch row k (the dropped rows included),
 *   after klsh_load_clusters_device  node k is the caller's node k (n_nodes = 0: what it was).
 * Ids stay on the host: with `ids` the loaded member ids in node order, klsh_result's
 * member_ids[m] equals ids[nodes[m]].
 * klsh_result_device writes, into memory of the context's device (each may be NULL; a host
 * pointer or another device's memory is KLSH_E_ARG): d_rows, the n_rows x d centroids, packed,
 * in canonical order; d_member_offsets, n_rows + 1 entries, klsh_result's member_offsets;
 * d_member_nodes, n_members entries, each row's members as nodes, in klsh_result's order;
 * d_labels, M entries, labels[k] = the index in canonical order of the live row whose list holds
 * node k, KLSH_NO_LABEL for a node no live row holds (a row klsh_load_counts dropped).  The lists
 * are flattened by parallel list ranking in ceil(log2(longest list)) rounds (option
 * "result_rounds" reads that count back); a broken member list is KLSH_E_STATE, as in
 * klsh_result, never an endless walk.  Every output is complete when the call returns (the
 * engine's stream is synchronized).  klsh_labels: the labels alone, copied to host memory.
 * Options: "result_device" 1 = klsh_count takes n_members from, and klsh_result builds its
 * offsets and ids with, the same kernels (the outputs are the same bytes; default 0);
 * read-only "member_nodes", "result_rounds" and "result_rank_us" (the HIP-event time of those
 * rounds in the last device result, microseconds). */
#define KLSH_NO_LABEL 0xFFFFFFFFu
int klsh_result_device(klsh_ctx* ctx, float* d_rows, uint32_t* d_member_offsets,
                       uint32_t* d_member_nodes, uint32_t* d_labels);
int klsh_labels(klsh_ctx* ctx, uint32_t* labels /* host, M entries */);

/* The cluster files, written from the device: the reference's IOMat::SaveResult
 * and IOMat::SaveBinary (io/ioMatrix.cc:265-294, 322-351).  For every live row, in klsh_result's
 * order, whose member count c exceeds ignore_small:
 *   clust_path  text: decimal(c), then '\t' decimal(id) per member in klsh_result's order, '\n'
 *               (decimal as ostream << uint64_t prints: no leading zeros, up to 20 digits);
 *   bin_path    the row's d floats, packed, host byte order.
 * Either path may be NULL (that file is not produced; both NULL is KLSH_E_ARG); both files are
 * opened with truncation.  A node that no live row holds is never written.  ignore_small < 0 is
 * KLSH_E_ARG (the reference's two writers disagree there: one compares size_t > int, the other
 * int > int).  Refused before any device work and before a file is opened or truncated: the
 * argument errors, nothing loaded (KLSH_E_STATE), a wrong stats->struct_size, a path that cannot
 * be opened for writing (KLSH_E_ARG; when only the second path fails the first is untouched).  A
 * broken member list is KLSH_E_STATE "corrupt member list", as in klsh_result.  A write that
 * fails later returns KLSH_E_ARG after removing both files.
 * The member lists come from the list ranking of klsh_result_device; the text is formatted by
 * kernels and leaves in windows of option "save_chunk_bytes" (default 64 MB; the binary file in
 * whole rows, one row at least per chunk) through two device and two pinned buffers, a chunk's
 * copy running beside the previous chunk's fwrite.  The files do not depend on the chunk size.
 * The ids are uploaded once per call unless the load defined them as base + node
 * (klsh_load_counts; a NULL member_ids of the other loads).  The call reads the context and
 * changes none of its state: klsh_result, klsh_row_state and the next klsh_cluster are what they
 * would have been.  On a context bound to a comm group it writes this rank's replica.  Both
 * files are complete, and the engine's stream synchronized, when it returns.
 * Options (test hooks): "save_chunk_bytes" (>= 32; 0 = the default), "save_offset_base" (the
 * byte position the text scan starts from, in [0, 2^48]; the file does not change); read-only,
 * of the last call: "save_chunks", "save_ids_uploaded". */
typedef struct klsh_save_stats {
  uint64_t struct_size;      /* in: sizeof(klsh_save_stats) */
  uint64_t clusters;         /* live rows */
  uint64_t clusters_written, members_written;
  uint64_t text_bytes, bin_bytes, chunks /* device-to-host chunks, both files */;
  double rank_ms;    /* offsets + list ranking (the kernels of klsh_result.hip) */
  double format_ms;  /* HIP-event time of the save kernels (keep, lengths, emit, row gather) */
  double write_ms;   /* host fwrite */
  double total_ms;
} klsh_save_stats;
int klsh_save_clusters(klsh_ctx* ctx, const char* clust_path, const char* bin_path,
                       int ignore_small, klsh_save_stats* stats);

/* ---- path functions, exposed for parity tests ------------------------------------------------- */
/* Hash::LSH::random_projection(row, table) (reference hash/lshash.cc:44-59) for n rows on the
 * GPU: keys[i] = MSB-first sign bits of the h hyperplanes (table: h x d, row-major).  The same
 * kernels and options as the loop's projection (the fp16 row image is built from `rows` where
 * the loop would keep one). */
int klsh_hash_keys(klsh_ctx* ctx, const float* rows, uint64_t n, int d, const float* table, int h,
                   uint32_t* keys);
/* merge_hashtable (reference function/cluster.cc:15-30) on the GPU: the stable bucket order of n
 * keys by their low `bits` bits (keys must be < 2^bits for a pure bucket order; higher bits are
 * carried along unsorted).  sorted_keys[i] = keys[perm[i]]; perm lists original positions, equal
 * keys in their original order. */
int klsh_bucket_sort(klsh_ctx* ctx, const uint32_t* keys, uint64_t n, int bits,
                     uint32_t* sorted_keys, uint32_t* perm);
/* The buckets of n sorted keys as the merge step takes them (the runs of equal keys; the
 * reference's lsh_table entries, function/cluster.cc:205-300): every run of 2 or more keys in start
 * order with its length and its list (0..5: 2, 3-4, 5-8, 9-16, 17-32, 33-64 rows; 6..9: 65-128,
 * 129-192, 193-384, 385-896; 10: longer; 11: longer than bucket_thr >= 0, i.e. nestedCluster).
 * *n_runs: in, the capacity of the outputs; out, the run count (KLSH_E_RANGE if it exceeds the
 * capacity).  A test hook. */
int klsh_bucket_runs(klsh_ctx* ctx, const uint32_t* sorted_keys, uint64_t n, int bucket_thr,
                     uint64_t* n_runs, uint32_t* starts, uint32_t* lengths, int32_t* lists);
/* One queued iteration's bucket order and run lists (run_batched, the iterations below 2^20 rows
 * whose row count only the device knows), on caller keys.  Every launch is sized for n_max and
 * reads the real count n_live from device memory; keys[n_live .. n_max) are stale and no kernel
 * may count, move or overwrite them.  path 1: the top-9-bit partition + the per-bucket LDS sorts
 * that list the runs (KLSH_E_RANGE unless bits is 10..19); path 0: the LSD passes of `bits` + the
 * run kernels.  Live keys must be < 2^bits.  1 <= n_live <= n_max < 2^20, 0 <= bits <= 19; all
 * arrays are host memory.  The sort workspace, the run workspace and the buffers the result may
 * land in are filled with the byte 0xA5 first (only the run counters start at zero, as in the
 * loop).  out_keys / out_perm (n_max entries each): the whole result pair, so an entry at or past
 * n_live is 0xA5A5A5A5 or what the input pair held there (perm starts as 0 .. n_max-1).  n_runs,
 * starts, lengths, lists: as klsh_bucket_runs.  counters (7, may be NULL): run heads (runs of one
 * key included), rows in the runs of lists 0..5, in each of lists 6..9, and in list 10.  A test
 * hook. */
int klsh_tail_buckets(klsh_ctx* ctx, const uint32_t* keys, uint64_t n_max, uint64_t n_live,
                      int bits, int bucket_thr, int path, uint32_t* out_keys, uint32_t* out_perm,
                      uint64_t* n_runs, uint32_t* starts, uint32_t* lengths, int32_t* lists,
                      uint32_t* counters);
/* p_cluster (reference function/cluster.cc:56-87) over the loaded rows taken as ONE bucket in
 * load order, at threshold thr.  Afterwards klsh_count/klsh_result give the survivors. */
int klsh_pcluster(klsh_ctx* ctx, float thr);
/* The per-slot state the engine keeps beside the rows and klsh_result never shows, for the live
 * rows in klsh_result's order (read-only; on a context bound to a comm group, this rank's
 * replica): nrm (n floats) = the cached sequential fp32 sum of squares that every later cosine
 * test reads, cnt (n) = the member count that weighs every later consensus, image (n x d uint16)
 * = the fp16 row image of the certified screens, filled only while option "fp16_image" reads 1.
 * Computed on the host: *pad_nonzero = words of the live rows' zero pad (columns d .. d rounded
 * up to 4) whose bits are not +0, *bad_links = live rows whose member chain, walked from its
 * head, does not have exactly cnt nodes or does not end at the cached tail.  Any pointer may be
 * NULL. */
int klsh_row_state(klsh_ctx* ctx, float* nrm, uint32_t* cnt, uint16_t* image,
                   uint64_t* pad_nonzero, uint64_t* bad_links);
/* LSH::generateHashTable (reference hash/lshash.cc:36-42) under the seeding convention:
 * h hyperplanes of d floats starting at draw index *rng_counter (advanced by h). */
int klsh_hyperplanes(uint32_t seed_base, uint64_t* rng_counter, int h, int d, float* table);
/* The merge test's sqrt and division exactly as the kernels evaluate them (sqrt_out[i] =
 * sqrtf(a[i]), div_out[i] = a[i] / b[i]); for checking IEEE correct rounding on the device. */
int klsh_fp_selftest(klsh_ctx* ctx, const float* a, const float* b, uint64_t n, float* sqrt_out,
                     float* div_out);

/* The cluster-text parser of klsh_diff_ksets alone (mode E below; a test hook):
 * `text` (len bytes, host memory) as <F>.clust.  path 0 = as
 * klsh_diff_ksets chooses, 1 = the host parser, 2 = the kernels only (KLSH_E_ARG on an irregular
 * text, or one of 2^32 bytes or more).  *n_lines = the text's lines; counts (n_lines), offsets
 * (n_lines + 1, offsets[c] = the declared counts before line c) and ids (offsets[n_lines]) may all
 * three be NULL for a size query; *n_ids: in, the capacity of ids; out, the entries (KLSH_E_RANGE
 * if the capacity is too small; KLSH_E_RANGE with *n_ids = 2^32 when they sum to 2^32 or more,
 * nothing of that size having been allocated).  *irregular_at = the smallest byte offset that
 * makes the text irregular — a byte outside the grammar, or the first digit of a run of 19 or
 * more — all ones if none does.  *path_used: 0 = kernels, 1 = host.  Every array is host memory;
 * every out-pointer but the three arrays is required. */
int klsh_parse_clust(klsh_ctx* ctx, const char* text, uint64_t len, int path, uint64_t* n_lines,
                     uint64_t* counts, uint64_t* offsets, uint64_t* ids, uint64_t* n_ids,
                     uint64_t* irregular_at, int* path_used);

/* Plain FASTQ parsed on the device (modes E and K: klsh_extract_fastq, klsh_count_khtable,
 * klsh_count_kmc).  A plain file is read in chunks, each starting at a record
 * boundary; lines are split at '\n', record r is lines 4r .. 4r + 3, and a chunk's complete records
 * are those up to the last newline that ends a line 4r + 3.  Record r is REGULAR when
 *   L0 begins with '@' (the name is the rest, any bytes);
 *   L1, the sequence, holds only bytes in [33, 126] other than '>', '+', '@' (it may be empty);
 *   L2 begins with '+', every further byte below 0x80;
 *   L3 holds exactly len(L1) bytes, each in [33, 127];
 * the host reader (klsh_fastq_next) reads such records as exactly these lines.  The kernels parse
 * the complete records of every chunk whose complete records are all regular; the next chunk starts
 * after them.  The host reader takes over at a chunk's file offset, and keeps the rest of the
 * file, when the chunk's complete records hold an irregularity or the chunk holds no complete
 * record (the bytes after the last complete record of the file; a record longer than a chunk).  A
 * file that begins with the gzip magic, and a path that is not a regular file (a FIFO, a process
 * substitution, /dev/stdin: no size, no positioned reads), is read by the host reader alone.  No result depends on any
 * of this: records, files, listings and statistics are the host reader's.
 * Options (klsh_set_option):
 *   "fastq_parse"        0 = the device where it can (the default: DESIGN.md §16.6), 1 = the host
 *                        reader only, 2 = the device only: KLSH_E_ARG, the message naming the
 *                        file offset, where the host reader would have to take over (for tests:
 *                        klsh_extract_fastq then leaves an output file that holds only the
 *                        records of the chunks finished before the refusal)
 *   "fastq_chunk_bytes"  bytes per chunk (0 = the default 64 MB; a test hook, in [64, 2^31]:
 *                        positions inside a chunk are 32-bit)
 * Read-only, of the context's last klsh_extract_fastq / klsh_count_khtable / klsh_count_kmc call:
 *   "fastq_device_chunks", "fastq_device_reads", "fastq_host_reads" (the two add up to the call's
 *   reads), "fastq_takeover_at" (the file offset where the host reader started — 0 for a file it
 *   read whole — in the call's last file that it read any of; all ones (-1) if it read none),
 *   "fastq_parse_us" (HIP-event time of the parser's kernels), "fastq_read_us" (host time of the
 *   chunks' file reads), "fastq_tile" (the kernels' tile, bytes).
 *
 * klsh_parse_fastq (a test hook) parses one chunk, `text` (len < 2^32 bytes, host memory).  path 0 =
 * the kernels, 1 = the host reader over the same bytes.
 *   *n_records    path 0: the complete records, 0 when they are not all regular; path 1: the
 *                 records the reader read (it also reads what follows the complete records)
 *   line_starts   4 n + 1 entries: the offset of each line's first byte, the last = *consumed
 *                 (path 1: the lines of the bytes it consumed, all ones where those are fewer)
 *   seq_off, seq  n + 1 offsets and the sequences they delimit, as klsh_check_reads takes them
 *   *seq_cap      in: the capacity of seq; out: the bases (KLSH_E_RANGE if seq is too small)
 *   *consumed     path 0: the end of the last complete record, 0 when the chunk is irregular;
 *                 path 1: the end of the last record read
 *   *irregular_at path 0: the smallest offset that makes a complete record irregular, all ones if
 *                 none does.  A byte outside its line's class is its own offset; an empty L0 or L2
 *                 is the offset of its newline; an L3 of another length than L1 is
 *                 (start of L3) + min(len(L1), len(L3)): the newline that came too early, or the
 *                 first byte too many.  path 1: all ones (the reader does not classify).
 * The three arrays may be NULL (a size query); every other out-pointer is required. */
int klsh_parse_fastq(klsh_ctx* ctx, const char* text, uint64_t len, int path, uint64_t* n_records,
                     uint32_t* line_starts, uint64_t* seq_off, char* seq, uint64_t* seq_cap,
                     uint64_t* consumed, uint64_t* irregular_at);

/* ---- mode E: differential k-mers and read extraction (reference app/kmerLSH.cc:521-580) ------- */
/* AB::WRS (reference function/funcAB.cc:73-109) for every cluster at once: a cluster with more than
 * size_thresh members (member_counts[c]) is tested with ALGLIB's pooled two-sample Student t-test
 * (alglib::studentttest2, utils/alglib-3.15.0/src/statistics.cpp:12502) of its centroid's first n1
 * values against the next n2 (centroids: n_clusters x (n1+n2) fp32, taken as double).
 * group[c] = 2 if lefttail <= pvalue_thresh (its ids go to group B's k-mers), else 1 if
 * righttail <= pvalue_thresh (group A), else 0.  Host computation, no device needed. */
int klsh_wrs(const float* centroids, uint64_t n_clusters, int n1, int n2,
             const uint64_t* member_counts, float pvalue_thresh, int size_thresh, uint8_t* group);
/* The test itself: alglib::studentttest2(x, n, y, m) -> both / left / right tails (bit-exact). */
int klsh_ttest2(const double* x, int64_t n, const double* y, int64_t m, double* bothtails,
                double* lefttail, double* righttail);

/* FASTQ records as the reference reads them (utils/fastq.cc FastqFile + kmer/kseq.h:153-200, gzip or
 * plain): the name is the whole header line, the sequence its isgraph() characters, the quality
 * the next len characters in [33,127].  klsh_fastq_next reads up to max_reads records into
 * reader-owned buffers valid until the next call (offset arrays have count+1 entries) and returns
 * the count; 0 = end of file (a truncated record ends the file, as in the reference). */
typedef struct klsh_fastq klsh_fastq;
klsh_fastq* klsh_fastq_open(const char* path, int* err);
int64_t klsh_fastq_next(klsh_fastq* f, uint64_t max_reads, const char** seq,
                        const uint64_t** seq_offsets, const char** name,
                        const uint64_t** name_offsets, const char** qual,
                        const uint64_t** qual_offsets);
void klsh_fastq_close(klsh_fastq* f);

/* A differential k-mer set on the context's device (the reference's uset_t, hash/HashTables.h:20):
 * kmers are the 8-byte images of Kmer objects as kmer_set.hex stores them (kmer/Kmer.cc:307),
 * read as little-endian uint64 (base i at bits 2i..2i+1, A/C/G/T = 0..3). */
typedef struct klsh_kset klsh_kset;
klsh_kset* klsh_kset_create(klsh_ctx* ctx, const uint64_t* kmers, uint64_t n, int* err);
void klsh_kset_destroy(klsh_kset* set);
/* IOFQ::CheckRead (reference io/ioFastQ.cc:5-76) on the GPU: read r = seq[read_offsets[r] ..
 * read_offsets[r+1]); hits[r] (may be NULL) = k-mer positions whose canonical k-mer is in the set,
 * flags[r] = 1 iff the read has at least k+10 bases and hits / (len-k+1) > kmer_vote (float). */
int klsh_check_reads(klsh_ctx* ctx, const klsh_kset* set, const char* seq,
                     const uint64_t* read_offsets, uint64_t n_reads, int k, float kmer_vote,
                     uint32_t* hits, uint8_t* flags);
/* Test hooks of the set.  klsh_kset_find: slots[i] = the slot of the set's table that holds
 * keys[i], all ones if the set does not hold it (the key all ones is never held); *n_slots (may be
 * NULL) = the table's slots, a power of two >= 1024 and >= 2 n, a key's home slot being the low
 * bits of the murmur3 finalizer of the key and the table probed linearly from there.  All arrays
 * are host memory; the argument checks are klsh_check_reads'.  Read-only option "extract_window":
 * the k-mer positions per LDS window of the vote kernel. */
int klsh_kset_find(klsh_ctx* ctx, const klsh_kset* set, const uint64_t* keys, uint64_t n,
                   uint64_t* slots, uint64_t* n_slots);
typedef struct klsh_extract_stats {
  uint64_t struct_size; /* in: sizeof(klsh_extract_stats) */
  uint64_t reads, bases, reads_tested, kmers_checked, reads_extracted, abnormal;
  double kernel_ms;  /* HIP-event time of the k-mer vote kernels */
  double parse_ms;   /* host FASTQ parsing (gzip included) */
  double total_ms;
} klsh_extract_stats;
/* IOFQ::ReadExtract (reference io/ioFastQ.cc:78-159) for one sample: every record of in_path whose
 * k-mer vote passes, written to out_path as "@name\nseq\n+\nqual\n" (plain text, byte-identical to
 * the reference's output).  stats may be NULL. */
int klsh_extract_fastq(klsh_ctx* ctx, const klsh_kset* set, const char* in_path,
                       const char* out_path, int k, float kmer_vote, klsh_extract_stats* stats);

/* The first half of mode E on the device (reference app/kmerLSH.cc:541-585,
 * IOMat::ReadClusterAll io/ioMatrix.cc:48-119, AB::WRS): the cluster files to the two differential
 * k-mer sets.  clust_path is <F>, fp32 rows of d = n1 + n2 values; the member lists are the text
 * <F>.clust; kmer_set_path holds kmap_size 8-byte k-mer images (kmer_set.hex).
 *   line_cnt = size(<F>) / (4 d), 0 when d = 0.  The text's lines are getline's (an unterminated,
 *   non-empty last line counts) and must be line_cnt many: otherwise KLSH_E_ARG.
 *   A line is parsed as the reference's strtol chain: the first strtol gives n, the declared member
 *   count; up to n further strtol results are its ids, missing ones are 0, tokens past n are
 *   ignored.  klsh_wrs runs with member_counts[c] = n.  The ids < kmap_size of a group-1 cluster
 *   mark A, of a group-2 cluster B; row i of kmer_set.hex goes to A if marked A, else to B if
 *   marked B.  Each table has the capacity klsh_kset_create gives that many keys, each set is bound
 *   to ctx (klsh_kset_find, klsh_check_reads, klsh_extract_fastq take it unchanged).
 * A text of digits, newlines and the other five isspace bytes (9, 11, 12, 13, 32) whose digit runs
 * are at most 18 long is REGULAR and is parsed by kernels (parse_path 0); any other text, and a
 * text of 2^32 bytes or more, is parsed whole by the host's strtol code (parse_path 1).  The text
 * and kmer_set.hex go up through two pinned buffers in chunks of option "diff_chunk_bytes"
 * (default 64 MB; a test hook, >= 32; 0 = default), the read of a chunk beside the copy of the one
 * before; no result depends on it.  Read-only option "diff_tile_bytes": the parser's tile.
 * Both sets are created or neither (*set_a = *set_b = NULL on any error).  Before any device work,
 * KLSH_E_ARG: NULL arguments, n1 or n2 < 0, a wrong stats->struct_size, an unreadable file, a
 * kmer_set.hex shorter than 8 kmap_size bytes.  KLSH_E_RANGE, before anything of that size is
 * allocated: declared counts that sum (saturating) to 2^32 or more.  The call reads nothing of,
 * and changes nothing in, the context's loaded rows.  stats may be NULL. */
typedef struct klsh_diff_stats {
  uint64_t struct_size;            /* in: sizeof(klsh_diff_stats) */
  uint64_t clusters, entries, text_bytes, tokens;
  uint64_t tested;                 /* clusters with more than size_thresh members */
  uint64_t clusters_a, clusters_b; /* group 1 / group 2 */
  uint64_t ids_a, ids_b;           /* distinct ids < kmap_size per group: the two numbers the CLI prints */
  uint64_t kmers_a, kmers_b;       /* rows of kmer_set.hex claimed into each set */
  uint64_t parse_path;             /* 0 device, 1 host */
  double read_ms, parse_ms /* HIP events */, wrs_ms, select_ms /* HIP events */, total_ms;
} klsh_diff_stats;
int klsh_diff_ksets(klsh_ctx* ctx, const char* clust_path, const char* kmer_set_path,
                    uint64_t kmap_size, int n1, int n2, float pvalue_thresh, int size_thresh,
                    klsh_kset** set_a, klsh_kset** set_b, klsh_diff_stats* stats);
/* ---- mode B: the k-mer table of KMC databases (reference io/ioHT.cc:83-199, kmc = false) ------- */
/* buildKHtable over KMC databases (KMC1 or KMC2/3 layout, <name>.kmc_pre / <name>.kmc_suf, listing
 * as kmer/kmc_api/kmc_file.cpp:66-532): the union of canonical k-mers over the samples, each
 * sample's summed counts clamped at 65535, written to <out_dir>/ kmer_set.hex (8 bytes per k-mer),
 * kmer_count.bin (sample-major uint16) and kmer_count.log ("%llu" rows, "\t%f" coverage = float sum
 * of log(count) per sample).  The files equal the reference's byte for byte: rows in the order of its
 * libcuckoo table after KmcRead's inserts at -T 1 (while the table never grows; a growing
 * reference table re-inserts from hardware_concurrency() threads, and that order is replayed here
 * as if those threads ran one after another).
 * out_dir NULL or "" = the current directory.  stats may be NULL. */
typedef struct klsh_khtable_stats {
  uint64_t struct_size; /* in: sizeof(klsh_khtable_stats) */
  uint64_t kmap_size;
  uint64_t records;        /* records streamed: both passes read every database, so twice their sum */
  uint64_t records_listed; /* records inside [min_count, max_count], each counted once */
  double io_ms;     /* host reads of the .kmc_suf streams */
  double total_ms;
  double order_ms;  /* host replay of the reference's libcuckoo inserts (the row order) */
} klsh_khtable_stats;
/* The row order alone (a test hook): the libcuckoo table order (kmer/Kmer.cc:138 hash, the
 * vendored utils/libcuckoo/cuckoohash_map.hh, 8-slot buckets, 2^16 buckets to start) of n DISTINCT
 * k-mer images inserted in the given order: order[i] = index of the table's i-th element.  Returns
 * the table's final hash power (>= 16), or a negative KLSH_E_* code.  Host only. */
int klsh_cuckoo_order(const uint64_t* images, uint64_t n, int k, uint32_t* order);
/* The host parse of a KMC database's prefix file (<name>.kmc_pre: version, header, prefix LUT) as
 * klsh_build_khtable does it, every file-derived offset checked (a test hook).  Host only. */
int klsh_kmc_info(const char* name, int* k, uint64_t* total, uint64_t* lut_entries);
/* Test hooks of klsh_build_khtable, context options (klsh_set_option / klsh_get_option; the
 * defaults are the product's behaviour and cost nothing):
 *   "kmc_chunk_records"   N > 0: the .kmc_suf streams are read N records at a time, not the 64 MB
 *                         of records a production chunk holds (never more than that; 0 = default),
 *                         so a small database takes the many-chunk path
 *   "kmc_ordinal_base"    the first-appearance ordinal of sample 0's first record (default 0, at
 *                         most 2^48): from 2^32 - records on, the ordinals need their high words
 *   "kmc_keep_first"      1 = a call keeps its first-appearance list for klsh_khtable_first
 *   read-only, of the context's last call: "kmc_decode_launches" (record-decode launches of the
 *   union pass: one per chunk per sample) and "kmc_high_sort" (1 = the second sort, on the
 *   ordinals' high words, ran).
 * klsh_khtable_first: the distinct canonical k-mers of the last call made with "kmc_keep_first"
 * on, in the order of their first ordinal (sample, then record; the all-A k-mer a filtered sample
 * adds comes after that sample's records) — what the libcuckoo replay is fed, before the row
 * order hides most of it.  *n: in, the capacity of images; out, the count (images NULL: only the
 * count; KLSH_E_RANGE if the capacity is too small). */
int klsh_khtable_first(klsh_ctx* ctx, uint64_t* images, uint64_t* n);
int klsh_build_khtable(klsh_ctx* ctx, const char* const* kmc_names, int n_samples, int k,
                       const char* out_dir, klsh_khtable_stats* stats);

/* ---- mode K: the k-mer table from FASTQ files (reference io/ioHT.cc:83-199, kmc = true) ------- */
/* What the reference gets from `kmc -k<K> -r -cs65535 -ci<count_min>` per sample followed by
 * buildKHtable on those databases, without the external counter and without writing databases.
 * Per sample (one FASTQ file, gzip or plain, read once with klsh_fastq_next; only the sequences
 * are used): A C G T a c g t are bases, any other character breaks the read (no k-mer spans it);
 * every window of k bases is one occurrence of its canonical k-mer, the smaller of the window and
 * its reverse complement as KMC values (base 0 most significant, A < C < G < T); a k-mer is listed
 * with min(occurrences, 65535) when occurrences >= count_min (count_min < 1 is taken as 1).  The
 * listing order is ascending KMC value, the order of a KMC1-layout database (a convention: KMC3's
 * own bin-by-bin listing depends on statistics of its input; only the row order of
 * the files depends on it).  The listings then go through the table build of
 * klsh_build_khtable unchanged: kmer_set.hex, kmer_count.bin and kmer_count.log in out_dir.
 * k in [1, 32].  stats may be NULL. */
typedef struct klsh_kcount_stats {
  uint64_t struct_size; /* in: sizeof(klsh_kcount_stats) */
  uint64_t kmap_size, reads, bases, positions /* valid k-mer windows */,
      distinct /* sum over samples, before count_min */, listed /* after */, batches, rehashes;
  double kernel_ms; /* HIP-event time of the counting kernels */
  double parse_ms;  /* host FASTQ parsing (gzip included) */
  double order_ms;  /* host replay of the reference's libcuckoo inserts (the row order) */
  double total_ms;
} klsh_kcount_stats;
int klsh_count_khtable(klsh_ctx* ctx, const char* const* fastq_paths, int n_samples, int k,
                       int count_min, const char* out_dir, klsh_kcount_stats* stats);
/* Test hooks of klsh_count_khtable, context options (the defaults are the product's behaviour and
 * cost nothing):
 *   "kcount_batch_reads"   N > 0: N reads per batch (0 = default, 2^18)
 *   "kcount_table_slots"   a sample's initial table: a power of two >= 1024 (0 = default, 2^22);
 *                          the table doubles between batches when the next batch could load it
 *                          past one half
 *   "kcount_keep_listing"  1 = a call keeps its per-sample listings for klsh_kcount_listing
 *   read-only, of the context's last call: "kcount_batches", "kcount_rehashes",
 *   "kcount_peak_slots" (the largest sample table); and "kcount_window", the k-mer positions per
 *   LDS window of the counting kernel.
 * "kmc_keep_first" / klsh_khtable_first work after klsh_count_khtable as after a build.
 * klsh_kcount_listing: sample `sample`'s listing of the last call made with
 * "kcount_keep_listing" on: KMC values ascending and their counts.  *n: in, the capacity of the
 * outputs; out, the count (both outputs NULL: only the count; KLSH_E_RANGE if too small). */
int klsh_kcount_listing(klsh_ctx* ctx, int sample, uint64_t* kmc_values, uint32_t* counts,
                        uint64_t* n);

/* Mode K with its databases: what klsh_count_khtable does, and each sample's listing written as
 * the KMC database the reference's `kmc` run would leave for mode B (the listing is written from
 * the device right after the sample is counted; no FASTQ file is read twice).  db_names[j] is
 * sample j's database path without extension (the sample lists' second column): <name>.kmc_pre
 * and <name>.kmc_suf, KMC1 layout (version 0), both strands, 2-byte counters (-cs65535):
 *   .kmc_suf  "KMCS", the records in ascending KMC value — (k - p) / 4 suffix bytes (the value's
 *             low 2 (k - p) bits, most significant byte first), then the counter in 2 bytes,
 *             little-endian — "KMCS"
 *   .kmc_pre  "KMCP", 4^p little-endian uint64 (entry q: the records whose prefix,
 *             value >> 2 (k - p), is below q), the header of five uint64 (k; 2 | p << 32;
 *             max(count_min, 1) | 65535 << 32; the record count; 0), the uint32 40, "KMCP"
 * p, the prefix length, is the one in [0, min(k, 15)] with (k - p) % 4 == 0 that makes the two
 * files smallest, 8 * 4^p + records * ((k - p) / 4 + 2) bytes, the smaller p on a tie.
 * out_dir NULL: the databases only (the reference's `-M K --only`): no table is built, none of its
 * three files is written, kmap_size stays 0, and a listing is freed once its database is written.
 * out_dir not NULL ("" = the current directory): the databases, then the table exactly as
 * klsh_count_khtable.  db_names NULL: klsh_count_khtable.  Both NULL: KLSH_E_ARG.
 * Before any device work, KLSH_E_ARG for a NULL or repeated entry of db_names, a database file
 * that cannot be opened for writing, and a forced prefix length that k does not allow.  A failed
 * write returns KLSH_E_ARG after removing that sample's two files; the databases of the samples
 * before it stay.  stats and db_stats may be NULL.
 * Context options (test hooks; the defaults are the product's behaviour):
 *   "kcount_db_prefix"         -1 (default) = p by the size rule, otherwise p itself
 *   "kcount_db_chunk_records"  records packed, copied and written at a time (0 = default, 2^22)
 *   read-only, of the context's last call: "kcount_db_chunks" (record chunks packed: per sample,
 *   its records over the chunk size, rounded up) and "kcount_db_prefix_used" (p of the last
 *   database written; -1 = none). */
typedef struct klsh_kmcdb_stats {
  uint64_t struct_size; /* in: sizeof(klsh_kmcdb_stats) */
  uint64_t databases, records, bytes /* of both files, all samples */, chunks;
  uint32_t prefix_len_min, prefix_len_max;
  double pack_ms;  /* HIP-event time of the record-packing and prefix-table kernels */
  double write_ms; /* host file writes */
} klsh_kmcdb_stats;
int klsh_count_kmc(klsh_ctx* ctx, const char* const* fastq_paths, const char* const* db_names,
                   int n_samples, int k, int count_min, const char* out_dir,
                   klsh_kcount_stats* stats, klsh_kmcdb_stats* db_stats);

/* ---- synthetic workload (klsh-synth v1) ------------------------------------ */
/* Host-side, deterministic on any machine (integer hashing + glibc exp/log/sqrt): fills counts
 * (sample-major d x n uint16, the kmer_count.bin layout) and coverage[d] = sum over i of ln(c)
 * for c > 0, summed in double in ascending i (the kmer_count.log convention).  Rows belong to
 * `genomes` groups (n/50 if 0): profile(g,s) = exp(2 + z), z ~ N(0,1); multiplicity m in {1,2};
 * count = min(Poisson(profile*m), 65535) (inversion below 30, normal approximation above).
 * threads <= 0: all host threads. */
int klsh_synth_counts(uint64_t n, int d, uint64_t seed, uint64_t genomes, int threads,
                      uint16_t* counts, double* coverage);

#ifdef __cplusplus
}
#endif
#endif
