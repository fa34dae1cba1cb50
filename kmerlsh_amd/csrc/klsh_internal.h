// Internal interface between the host units (the .cpp files; their shared context is klsh_ctx.h,
// which the kernels never see) and the gfx950 kernels (the .hip files).  Not part of the C ABI.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>
#include <vector>

#include "klsh.h"

namespace klsh {

constexpr uint32_t kInvalid = 0xFFFFFFFFu;  // dead position marker in a bucket's slot run
constexpr uint32_t kNil = 0xFFFFFFFFu;      // end of a member list
constexpr int kMaxHyperplanes = 32;         // keys are uint32 (h = floor(log2 N) <= 31)
constexpr int kScanTile = 4096;             // items per scan workgroup (256 lanes x 16)
// Sort workspace (u32 words) for `slots` keys: [digit][tile] counts and digit totals
// (klsh_sort.hip).
uint64_t sort_ws_words(uint64_t slots);
// Scan workspace (u32 words): [0, 64) ticket / done / epoch of the look-back scan, then its 64-bit
// tile status words (room for 2^32 items), then the tile sums of the multi-kernel scans and of
// the compaction — apart, so a tile sum can never pass for a look-back status word.
constexpr uint32_t kScanStatusWord = 64;
constexpr uint64_t kScanSumsWord = kScanStatusWord + 2ull * (1ull << 20);
inline uint64_t scan_ws_words(uint64_t slots) {
  return kScanSumsWord + (256 * slots) / kScanTile + 1024;
}

// Bucket runs of 65..896 rows are merged by one workgroup with the run's decision matrix in LDS
// (k_merge_big; three size classes, rows in LDS up to 384); longer runs by one wave from memory
// (k_merge_huge).
// 65..128, 129..192, 193..384, 385..896 rows: the 129..192 class has its own layout (62 KB of
// LDS at d = 64) so two of its workgroups share a CU, where a 384-row layout needs 130 KB
constexpr int kBigClasses = 4;
constexpr int kBigRows[kBigClasses] = {128, 192, 384, 896};

// Runs of 2..64 rows are merged by G-lane groups, one size class per G = 2, 4, ..., 64
// (class c holds runs of 2^c < b <= 2^(c+1) rows).
constexpr int kGroupClasses = 6;
inline uint64_t group_class_capacity(int c, uint64_t cap) { return cap / ((1ull << c) + 1) + 64; }

// Run-list counters: k_runs' workgroups add to each of them once, so each sits on a 128-B line of
// its own (adds to one line serialise at ~5-10 ns each; 13 counters on one line made k_runs
// ~10x slower than its key reads).  Device only: the compaction copies them into Counters for
// the host and zeroes them for the next iteration.
struct alignas(128) CountLine {
  uint32_t v;
  uint32_t pad_[31];
};
struct RunCounters {
  CountLine n_seg, n_cls[kGroupClasses], n_big[kBigClasses], n_huge, n_over, n_small_rows;
  CountLine n_big_rows[kBigClasses], n_huge_rows;  // rows in the big / huge runs (kernel rooflines)
  // the small-run screen (k_small_screen): runs of each class it could not rule out, their rows,
  // and a flag that it ran this iteration
  CountLine n_act[kGroupClasses], n_act_rows, screened;
};

// Run-finding workspace (u32 words) for `slots` positions: 19 counts + a tail end + the first /
// last heads + a 4096-bit head bitmap per 4096-position tile.
inline uint64_t run_ws_words(uint64_t slots) { return (slots / 4096 + 2) * (19 + 1 + 2 + 128) + 64; }

// Device-side per-iteration counters (zeroed by the host before each iteration).
struct Counters {
  uint32_t n_seg;                  // bucket runs (k_runs)
  uint32_t n_cls[kGroupClasses];   // runs of 2..64 rows queued per size class
  uint32_t n_big[kBigClasses];     // runs of 65..896 rows queued for k_merge_big, per class
  uint32_t n_huge;                 // longer runs queued for k_merge_huge
  uint32_t n_over;                 // runs longer than bucket_size_threshold (nestedCluster)
  uint32_t total;                  // result of the last scan/compaction (live rows)
  uint32_t n_delta;                // sharded loop: survivors rewritten by a merge this iteration
  uint32_t err;                    // a device-side protocol failure (look-back wait limit); 0 = ok
  uint32_t n_small_rows;           // rows in the runs of 2..64 rows (the small-run merge's rows)
  uint32_t n_big_rows[kBigClasses];  // rows in the runs of each big class
  uint32_t n_huge_rows;            // rows in the runs of k_merge_huge
  uint32_t n_act_rows;             // rows in the small runs the screen passed to k_merge_small
  uint32_t screened;               // 1: the small-run screen ran this iteration
};

// Per-kernel-class timing (bench.py's roofline) from in-kernel stamps: every workgroup of a timed
// launch stamps the 100 MHz real-time counter (s_memrealtime) at its start (atomicMin) and at its
// end (atomicMax) into one of kStampSlots lines of its class, so a class's span in an iteration is
// first workgroup start -> last workgroup end — the span rocprofv3's kernel trace reports — with
// no marker packets in the streams.  (HIP event pairs measure from the moment a stream reaches a
// kernel, resource waits included: tools/ubench_events shows a 50-us kernel timed at 550 us behind
// a chip-filling kernel of another stream, and event pairs around every merge class added 13-20
// ms to a C2 step.)  Iteration t stamps set t & 1; the first workgroup of iteration t+1's
// projection folds set t into the per-class totals (iteration t is complete by then: stream
// order) and clears it; the engine folds the last set at the end of a call.
enum KClass : int {
  KC_PROJECT = 0, KC_SORT, KC_RUNS, KC_SMALL, KC_BIG128, KC_BIG192, KC_BIG384, KC_BIG896, KC_HUGE,
  KC_TAIL, KC_COMPACT, KC_SCREEN,
  KC_MERGE,  // (a phase) the merge launches of an iteration at >= tail_merge_rows positions
            // (default 2^22; every iteration at d > 64), all classes
  KC_COUNT
};
constexpr int kStampSlots = 16;
struct alignas(128) StampLine {
  unsigned long long v;
  unsigned long long pad_[15];
};
struct KStampSet {
  StampLine t0[KC_COUNT][kStampSlots];  // earliest workgroup start (~0 = none)
  StampLine t1[KC_COUNT][kStampSlots];  // latest workgroup end (0 = none)
};
struct KStampBlock {
  KStampSet set[2];
  unsigned long long ticks[KC_COUNT];  // summed spans (10 ns ticks)
  unsigned long long launches[KC_COUNT];
};
// What a launch carries (by value): blk == nullptr = untimed; set = the set it stamps; fold >= 0:
// the projection folds that set first (the previous iteration's).
struct KTime {
  KStampBlock* blk;
  int set;
  int fold;
  int phase = -1;  // >= 0: the launch also stamps this phase class (its first start, last end)
  KTime with_fold(int f) const { KTime k = *this; k.fold = f; return k; }
  KTime with_phase(int p) const { KTime k = *this; k.phase = p; return k; }
};
constexpr KTime kNoTime{nullptr, 0, -1, -1};
// Fold set `t` into the totals and clear it (one workgroup; device code, klsh_device.h).

// The merge workspace by lifetime: what device code reads (MergeView and its parts), what the host
// keeps (MergePlan), what holds for one call (MergeCall).  First the run lists of an iteration:
struct RunLists {
  uint2* cls[kGroupClasses];  // (start, length) of runs per size class
  // the runs of each class the fp16 screen could not rule out (k_small_screen)
  uint2* act[kGroupClasses];
  uint2* big[kBigClasses];    // (start, length) of runs for k_merge_big, per class
  uint2 *huge, *over;         // ... for k_merge_huge; of oversize runs
  RunCounters* rc;            // the run counts of this iteration
  // runs over 896 rows at d = 16 / 32 (k_merge_long): each workgroup's bit matrix, kLongRows x
  // kLongRows / 64 words (nullptr: k_merge_huge)
  uint64_t* long_P;
};
// Sharded loop only (dlist == nullptr otherwise): every survivor a merge rewrote is appended to
// dlist (ctr->n_delta entries, any order, each slot once); mark[slot] == stamp dedupes the kernels
// that merge in place (stamp: unique per iteration, never reused by a context).
struct DeltaSink { uint32_t *dlist, *mark; uint32_t stamp; };
constexpr DeltaSink kNoSink{nullptr, nullptr, 0u};
// k_merge_tail's 65..384-row runs screened first ("tail_big_screen"): the test's threshold, margins
struct BigScreen { uint32_t on; float s_star, m0, a2; };
// What a merge kernel takes: built by the launch code for one launch, const afterwards.
struct MergeView : RunLists {
  DeltaSink sink;
  KTime kt;            // per-class stamps of this iteration's merge launches
  uint32_t screened;   // 1: the small-run merge reads act instead of cls
  uint32_t huge_fold;  // 1: the 385..896-row kernel's workgroups also walk the >896-row list
  BigScreen bs;
};
static_assert(std::is_trivially_copyable<MergeView>::value, "a kernel argument");
static_assert(sizeof(MergeView) == 232, "the merge kernels' argument block (DESIGN.md §3)");

constexpr int kMergeStreams = 3;
// The host's side (klsh_ctx::mp): the buffers reserve() allocates, the options, the loop's policy
// for the next iteration, the streams.  Never a kernel argument.
struct MergePlan {
  RunLists lists;
  uint32_t *tile_sums, *run_ws;  // run_ws: per-tile list counts, head bitmaps (run_ws_words)
  uint32_t long_groups;  // the workgroups long_P has room for (0: k_merge_huge)
  // ---- options (klsh_set_option; a launch size of 0 = the measured default, see the launch code)
  // "long_runs": 4 (default) = k_merge_long also takes the 385..896-row runs, 1 = only the longer
  // ones, 0 = k_merge_huge for those (long_off = 1)
  uint32_t long_off = 4;
  uint32_t small_grid;       // "small_grid": the small-run merge's persistent launch
  uint32_t tail_nbig;        // "tail_big_groups": k_merge_tail's big-run workgroups
  uint32_t tail_nsmall;      // "tail_small_groups": k_merge_tail's small-run workgroups
  uint32_t wide_group_grid;  // "wide_group_grid": the wide-row group merges, per class
  uint32_t screen_grid;      // "small_screen_grid": the small-run screen's persistent launch
  // "wide_gram": at d = 512 the group merges of runs of at least this many rows (8, 16, 32, 64)
  // decide on the matrix cores; 0 = none
  uint32_t wide_gram = 32;
  uint32_t small_screen = 1;  // "small_screen": 1 = screen the small runs on the fp16 image first
  // "tail_screen": 1 = the small-run screen also runs in front of k_merge_tail (iterations below
  // tail_merge_rows), whose small-run waves then walk only the runs it passed
  uint32_t tail_screen = 1;
  // "tail_big_screen": 1 = there, the 65..384-row runs are first screened on the fp16 image in
  // their workgroup (BigScreen); a run with no pair left reads no f32 row
  uint32_t tail_big_screen = 1;
  uint32_t tail_screen_grid;  // "tail_screen_grid": its persistent launch there (0: 2048)
  // "tail_merge_rows": below this many positions every merge class runs in ONE launch
  // (k_merge_tail); 0 = the default 2^22 (tests lower it to reach the per-class launches)
  uint32_t tail_max;
  bool huge_fold_always = false;  // "huge_fold" (tests): fold in every iteration
  // ---- the next iteration's launches, from the run counts of the last (klsh_loop.cpp)
  // 385..896-row runs on aux 2 instead of ahead of the >896-row runs on the main stream: when the
  // previous iteration had many of them (C4: thousands; C2: < 10)
  uint32_t big896_aux;
  // >896-row runs: the launch's workgroup cap (0 = one per 897 positions, at most 512).  64 after
  // an iteration without such runs: an empty launch of hundreds of 512-lane workgroups waits for
  // CUs behind the other classes (C2: 25 ms per step of span)
  uint32_t huge_cap;
  // 1: no k_merge_huge launch, MergeView::huge_fold instead (after several iterations without such
  // runs: C2 and C5 never have any, an empty launch still costs its dispatch; C4 keeps the kernel)
  uint32_t huge_fold;
  uint32_t huge_quiet;  // consecutive iterations without >896-row runs
  // no run counts yet (a call's start, klsh_pcluster)
  void no_counts() { huge_cap = 0, huge_fold = huge_fold_always ? 1u : 0u; }
  // Size classes run concurrently on kMergeStreams auxiliary streams (fork after the run
  // classification, join before the compaction): in the late, small iterations each class kernel
  // is one long sequential walk, and serialised walks would add up.  aux[0] == nullptr: one stream.
  hipStream_t aux[kMergeStreams];
  hipEvent_t fork, join[kMergeStreams];
};
// What one call of launch_merge / launch_runs / launch_tail_local adds.
struct MergeCall {
  KTime kt = kNoTime;                           // the iteration's stamps
  hipEvent_t small_ev[2] = {nullptr, nullptr};  // HIP events around the small-run launch
  DeltaSink sink = kNoSink;
  uint32_t grid_cap = 0;  // klsh_ctx::grid_cap: the per-class launches that stride over a run list
  MergeCall with_kt(KTime k) const { MergeCall m = *this; m.kt = k; return m; }
};
// Option "grid_cap" (tests; 0 = off): g workgroups, at most `cap`.  Only for launches whose
// workgroups stride over a list or an index range on their own; a kernel whose workgroups take
// one tile each, or wait for one another, must keep its grid.
inline uint32_t cap_grid(uint32_t g, uint32_t cap) { return cap && g > cap ? cap : g; }
// the grid of a kernel that strides over n items with 256 lanes: at most `most` workgroups
inline uint32_t stride_grid(uint64_t n, uint32_t grid_cap, uint64_t most = 16384) {
  const uint64_t g = (n + 255) / 256;
  return cap_grid((uint32_t)(g < most ? (g ? g : 1) : most), grid_cap);
}
constexpr uint32_t kLongRows = 4096;  // the longest run k_merge_long walks (longer: k_merge_huge)
inline bool long_ok(int d) { return d == 16 || d == 32; }
// (2^22 since round 5: with the small-run screen and the big-run prescreen inside it, the one
// launch beat the four-stream fork/join down to 4M positions — C2, one box, interleaved: 2^20
// 200.2, 2^21 196.5, 2^22 193.1, 2^23 ~= 2^22, 2^24 +1 ms per step)
inline uint32_t tail_merge_max(const MergePlan& p) { return p.tail_max ? p.tail_max : (1u << 22); }

// Row state, structure-of-arrays, one entry per slot (a slot is a row of the loaded matrix;
// a merge writes the consensus into the candidate's slot, cluster.cc:70-74).
struct Rows {
  float* x;        // [slots][dp] fp32 rows, dp = d rounded up to 4 (16-B aligned rows)
  float* nrm;      // [slots] sequential sum of squares (distance.cc:33-34), cached exactly
  uint32_t* cnt;   // [slots] member count (|_ids|)
  uint32_t* head;  // [slots] first member node
  uint32_t* tail;  // [slots] last member node
  uint32_t* nxt;   // [members] next member node (kNil = end)
  int d;
  int dp;
  // [slots][dp] fp16 image of x (round to nearest; may be null): the projection's certified
  // screen reads it instead of x (half the bytes of the row gather).  Kept equal to fp16(x):
  // rebuilt after a load / restore, written with x by every merge store (store_row4/store_row1)
  // and by the sharded delta apply.
  uint16_t* xh = nullptr;
};
// The fp16 image is kept for these widths (the matrix-core screen takes 16 columns per step).
// (the wide-row variants that read an fp16 image of d > 64 rows were measured slower and removed)
inline bool shadow_width_ok(int d) { return d == 16 || d == 32 || d == 64; }

// The merge test of cluster.cc:68-69 as a threshold on the quotient.  The reference computes
// sim = dot / (sqrtf(|a|^2) * sqrtf(|b|^2)); dist = 1 - sim; and merges when 1 - dist >= thr.
// s -> fl(1 - fl(1 - s)) is monotone in s, so the test is exactly fl(dot / den) >= s_star for the
// smallest float s_star that passes (computed on the host by make_decider, NaN if none does).
// Fast path (`fast` != 0, s_star a positive normal float): q = dot * rcp(den) is within 2 ulp of
// dot / den, so q >= s_hi (s_star + 8 ulp) or q <= s_lo (s_star - 8 ulp) settles the test and only
// quotients within a few ulp of s_star take the correctly rounded division.
// Pre-screen (`fast` only): a Gram value G from the bf16x3 MFMA tiles (kGramMargin below) settles
// the test when G / den >= g_hi or <= g_lo; pairs in between take the exact sequential dot.
struct Decider {
  float s_star, s_lo, s_hi;
  uint32_t fast;
  float g_lo, g_hi;
};
// |G - dot| <= 5.4e-5 * |a| |b| for the bf16x3 Gram value at d <= 64 (split residuals
// 3.03 * 2^-16, the MFMA sum <= 29 chained f32 adds per term at 2u, the reference's own 65u; see
// the wide-row projection's bound) against the reference's sequential f32 dot; the margin adds headroom for den's
// rounding and the approximate quotient.
constexpr float kGramMargin = 1.0e-4f;
Decider make_decider(float thr);

// Workspace of the wide-row matrix-core projection: the (row, hyperplane) pairs its screen could
// not call (fix[0 .. cap)), a counter and a done counter (ws[0], ws[1]) that the fix-up kernel
// returns to zero.  Zeroed once at allocation.  ProjectView is what the kernels take, ProjectPlan
// the host's side (klsh_ctx::pp): the context's workspace and the options.
struct ProjectView {
  uint2* fix;
  uint32_t* ws;
  uint32_t cap;
  uint32_t h16_cs;  // "h16_bound" = 0: the fp16 projection bounds by |x||w|, not sum |x_k||w_k|
};
static_assert(std::is_trivially_copyable<ProjectView>::value && sizeof(ProjectView) == 24,
              "a kernel argument");
struct ProjectPlan {
  ProjectView v;  // the context's workspace (reserve) and "h16_bound"
  // launch sizes and test hooks (klsh_set_option; 0 = default)
  uint32_t h16_grid;   // "h16_grid": fp16-image projection workgroups, at most
  uint32_t wide_grid;  // "wide_grid": wide-row screen workgroups, at most
  uint32_t fix_grid;   // "fix_grid": wide-row fix-up workgroups
  uint32_t segcap;     // "h16_segcap" (tests): fix-up entries per fp16-projection workgroup
  uint32_t variant;    // "projection": kProjAuto / kProjPacked / kProjScreen
  uint32_t wide_rolled;  // "wide_unrolled" = 0: d = 512 through the generic wide screen
  // the same options over a caller's workspace (klsh_hash_keys)
  ProjectPlan over(uint2* f, uint32_t* w, uint32_t c) const {
    return ProjectPlan{{f, w, c, v.h16_cs}, h16_grid, wide_grid, fix_grid, segcap, variant, wide_rolled};
  }
};
// Projection variants (klsh_set_option "projection"): the default picks the certified
// matrix-core screen where it exists (the fp16 row image at d = 16 / 32 / 64, bf16x3 above 64)
// and the packed exact VALU chains elsewhere; kProjPacked forces the exact chains (no fp16 image
// is kept then); kProjScreen asks for the screen (an error where none exists).  Keys are the
// same bits either way.
constexpr uint32_t kProjAuto = 0, kProjPacked = 1, kProjScreen = 2;
// workgroups of the fp16-image projection, at most (C2 per step: 2048 -> 46.1, 4096 -> 46.5,
// 8192 -> 48.5, 16384 -> 52.9, 32768 -> 55.5 ms, interleaved on one box)
constexpr uint32_t kH16Grid = 2048;

// ---- launch wrappers (all asynchronous on `s`) ------------------------------------------------
// keys[p] = sign-hash of row slots[p] against h hyperplanes W (h x dp), OR'ed with key_or.
// The packed projection of an iteration queued before its row count is known: n and h come from
// the device word n_dev (written by the previous compaction), n_max bounds the grid.  Only for
// d in {8, 16, 32, 64} (project_device_n_ok).
bool project_device_n_ok(int d);
// woff_dev (may be null): the iteration's hyperplanes start woff_dev[0] rows after W (a batch of
// iterations queued at once: each compaction advances it by its own h, see Publish::woff).
void launch_project_device_n(const Rows& r, const uint32_t* slots, uint32_t* keys, uint32_t n_max,
                             const float* W, const uint32_t* n_dev, hipStream_t s,
                             KTime kt = kNoTime, const uint32_t* woff_dev = nullptr,
                             const ProjectPlan* pp = nullptr);

// pp (may be null): the plan that enables the matrix-core screens (the fp16 row image where
// r.xh is set, bf16x3 for d > 64).  Returns the kernel it launched (ProjKernel).
enum ProjKernel : int { kPkNone = -1, kPkPacked = 0, kPkH16 = 1, kPkWide = 2 };
// The kernel behind a ProjKernel (option "last_hash_variant"; mirrored in _native.py): the three
// packed exact-chain kernels share kPkPacked, the two instantiations of the wide screen kPkWide.
enum ProjVariant : int {
  kPvNone = -1,
  kPvPk = 0,          // k_project_pk<D> (d = 8, 16, 32, 64)
  kPvWidePk = 1,      // k_project_wide_pk (hyperplanes in LDS: 16 dp ceil(h / 4) <= 64 KB)
  kPvGeneric = 2,     // k_project_generic (hyperplanes from memory)
  kPvH16 = 3,         // k_project_h16<D>
  kPvMfmaWide512 = 4, // k_project_mfma_wide<512> + k_project_fix
  kPvMfmaWide = 5,    // k_project_mfma_wide<0> + k_project_fix
};
// variant (may be null): receives the ProjVariant launched.
int launch_project(const Rows& r, const uint32_t* slots, uint32_t* keys, uint32_t n,
                   const float* W, int h, uint32_t key_or, hipStream_t s,
                   const ProjectPlan* pp = nullptr, KTime kt = kNoTime, int* variant = nullptr);

// Stable LSD radix sort of (keys, vals)[0..n) on the low `bits` bits (klsh_sort.hip); ping-pong
// buffers, *out_k/*out_v = the pair holding the result.  ws: sort_ws_words(n) words.
// n_dev (may be null): the key count is read on the device (<= n, which sizes the grids).
void radix_sort(uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, uint32_t n, int bits,
                uint32_t* ws, uint32_t** out_k, uint32_t** out_v, hipStream_t s,
                KTime kt = kNoTime, const uint32_t* n_dev = nullptr);

// Greedy merge (p_cluster) over every bucket run of equal key in positions [lo, hi) of
// (key, slots), in place: survivors first in each run, kInvalid after.  Runs longer than
// bucket_thr (>= 0) are queued to p.lists.over (start, length) and left untouched.
// n_dev (may be null; lo == 0 and hi < 2^20 only): the position count is read on the device
// (<= hi, which sizes the grids).
// runs_ready: the run lists of [lo, hi) are already built (launch_tail_local).
void launch_merge(const Rows& r, const uint32_t* key, uint32_t* slots, uint32_t lo, uint32_t hi,
                  float thr, int bucket_thr, const MergePlan& p, const MergeCall& c, Counters* ctr,
                  hipStream_t s, const uint32_t* n_dev = nullptr, bool runs_ready = false);

// Small iterations (< 2^20 positions, keys of 10..19 bits): the stable bucket sort in two steps
// that also builds the run lists.  radix_sort_top: the stable partition of (k0, v0) by the top
// kTailTopBits of `bits` key bits into (k1, v1); returns the top buckets' sizes.
// launch_tail_local: every top bucket of (k1, v1) sorted stably by its low bits - kTailTopBits
// bits into (k0, v0), and its runs of 2+ equal keys listed into p.lists (as launch_runs would).
const uint32_t* radix_sort_top(const uint32_t* k0, const uint32_t* v0, uint32_t* k1, uint32_t* v1,
                               uint32_t n, int bits, uint32_t* ws, hipStream_t s, KTime kt,
                               const uint32_t* n_dev);
void launch_tail_local(const uint32_t* kin, const uint32_t* vin, uint32_t* kout, uint32_t* vout,
                       const uint32_t* dtot, int bits, int bucket_thr, const MergePlan& p,
                       const MergeCall& c, hipStream_t s);
// the top-bits partition's digit width: 9 (512 top buckets of ~1K keys at C2's tail; the local
// sorts then take up to 10 low bits) measured C2 188.0-188.7 -> 186.1-186.4 ms against 10 (one box,
// interleaved, three rounds: the run listing 19.8 -> 18.3 ms per step, half the workgroups and
// half the same-address list-counter adds); 8 (256 buckets, up to 11 low bits) measured slower:
// run listing 18.4 -> 20.7 ms per step
constexpr int kTailTopBits = 9;
// the local sorts' digit capacity: the low bits of a 19-bit key (the queued iterations have
// N < 2^20, so h <= 19), at least 2^10
constexpr int kTailLowBits = 19 - kTailTopBits > 10 ? 19 - kTailTopBits : 10;
inline bool tail_local_ok(uint32_t n_max, int bits) {
  return n_max <= (1u << 20) && bits > kTailTopBits && bits <= kTailTopBits + kTailLowBits;
}

// Bucket runs of positions [lo, lo + n) of sorted keys (n_dev: the count read on the device, as
// launch_merge): every run of 2+ equal keys into its list of p.lists (size classes, big classes,
// huge, oversize), the counts into its rc. (launch_merge's first step; klsh_bucket_runs for tests.)
constexpr int kRunListCount = kGroupClasses + kBigClasses + 2;
void launch_runs(const uint32_t* key, uint32_t lo, uint32_t n, int bucket_thr, const MergePlan& p,
                 const MergeCall& c, hipStream_t s, const uint32_t* n_dev = nullptr);

// Counters handed to the host through mapped pinned memory (no copy launch, no stream sync): the
// compaction's last workgroup writes *ctr (total filled in) to `host`, zeroes *ctr for the next
// iteration, then writes `seq` to *seq_host (system-scope release); the host polls *seq_host.
struct Publish {
  Counters* host;     // device pointer of the mapped host copy (nullptr: no publishing)
  uint32_t* seq_host;
  uint32_t seq;
  uint32_t* n_next;   // device word that also receives the survivor count (may be null)
  // device word advanced by floor(log2 n) of the compacted iteration (may be null): the next
  // iteration's hyperplane offset when a batch of iterations is queued at once (cluster.cc:194-196
  // draws h = floor(log2 N_t) hyperplanes per iteration)
  uint32_t* woff = nullptr;
};

// The look-back compaction's tile status words (>= 256, zeroed once) and the epoch of its last
// launch (status words carry the epoch, so they are never cleared).
struct LookBack {
  unsigned long long* status;
  mutable uint32_t epoch;
};

// out[0..total) = slots[p] for p with slots[p] != kInvalid, stable; ctr->total = count.  rc (may
// be null): the iteration's run counters, copied into *ctr (and zeroed) before the publish.  lb
// (may be null): one launch instead of two when n fits 256 tiles.  n_dev (may be null; needs lb
// and n <= 256 tiles): the slot count is read on the device (<= n, which sizes the grid).
void launch_compact(const uint32_t* slots, uint32_t n, uint32_t* out, uint32_t* tile_sums,
                    Counters* ctr, hipStream_t s, const Publish* pub = nullptr,
                    RunCounters* rc = nullptr, KTime kt = kNoTime,
                    const LookBack* lb = nullptr, const uint32_t* n_dev = nullptr);
// Fold set `set` of blk into its totals and clear it (the end of a timed call).
void launch_stamp_fold(KStampBlock* blk, int set, hipStream_t s);
// a[0..na) then b[0..nb) to dst (mapped host memory, device view), then *seq_host = seq (release)
void launch_publish_words(const uint32_t* a, uint32_t na, const uint32_t* b, uint32_t nb,
                          uint32_t* dst, uint32_t* seq_host, uint32_t seq, hipStream_t s);

// Mode-C producer: rows x[i] (slot i) from counts (d x bs, sample-major), LUT ln(c+1),
// v_kmers; order[] = kept rows (sum > 0.1 d) compacted; ctr->total = kept count.
void launch_convert(const Rows& r, const uint16_t* counts, uint32_t bs, const float* lut,
                    const float* v_kmers, uint32_t* keep, uint32_t* order, uint32_t* tile_sums,
                    Counters* ctr, hipStream_t s);

// Sequential norms nrm[slot] for slots [0, n) (after a load).
void launch_norms(const Rows& r, uint32_t n, hipStream_t s);
// r.xh = fp16(r.x) for slots [0, n).
void launch_shadow_build(const Rows& r, uint64_t n, hipStream_t s);


// out[i*d + k] = x[order[i]][k] (compact result rows).
void launch_gather_rows(const Rows& r, const uint32_t* order, uint32_t n, float* out,
                        hipStream_t s);

// ---- the result on the device (klsh_result.hip) -------------------------------
// Every launch strides over its range on its own and takes option "grid_cap" (cap_grid).
constexpr uint32_t kResItems = 8;                  // live rows per lane of an offsets tile
constexpr uint32_t kResTile = 256 * kResItems;     // live rows per offsets tile
inline uint32_t result_tiles(uint64_t n) { return (uint32_t)((n + kResTile - 1) / kResTile); }
// hdr: kResHdrWords words, zeroed by the caller before the first launch of a result
constexpr uint32_t kResTotal = 0;     // members of the live rows (= off[n])
constexpr uint32_t kResMaxCnt = 1;    // the longest live member list
constexpr uint32_t kResLabelled = 2;  // nodes that found a live row (k_rank_emit)
constexpr uint32_t kResErr = 3;       // kResErr* bits
constexpr uint32_t kResHdrWords = 8;
constexpr uint32_t kResErrOrder = 1u;  // a live slot outside the table
constexpr uint32_t kResErrList = 2u;   // a link or tail outside the table, a node past its row's cnt
// off[i] = sum of cnt[order[j]] over j < i, off[n] = hdr[kResTotal] = the total, hdr[kResMaxCnt] =
// the largest; three launches (tile sums, one workgroup over the sums, apply).  tsum, tmax:
// result_tiles(n) words each.
void launch_result_offsets(const uint32_t* order, const uint32_t* cnt, uint32_t n, uint32_t slots,
                           uint32_t* tsum, uint32_t* tmax, uint32_t* off, uint32_t* hdr,
                           hipStream_t s, uint32_t grid_cap = 0);
// rowof[0..members) = KLSH_NO_LABEL, then rowof[tail[order[i]]] = i for the live rows with members
void launch_result_rowof(const uint32_t* order, const uint32_t* cnt, const uint32_t* tail,
                         uint32_t n, uint32_t slots, uint32_t members, uint32_t* rowof,
                         uint32_t* hdr, hipStream_t s, uint32_t grid_cap = 0);
// List ranking of the member chains by `rounds` >= ceil(log2(longest chain)) rounds of pointer
// jumping over the packed (jmp | dist << 32) words, st0 and st1 in turn (members words each).
// Returns the buffer with the result: jmp = the node's chain end, dist = its links to it.
// after_init (may be null): recorded between the init launch and the first round.
const uint64_t* launch_list_rank(const uint32_t* nxt, uint32_t members, uint32_t rounds,
                                 uint64_t* st0, uint64_t* st1, uint32_t* hdr, hipStream_t s,
                                 uint32_t grid_cap = 0, hipEvent_t after_init = nullptr);
// labels[v] = i = rowof[jmp of v]; nodes[off[i] + cnt[order[i]] - 1 - dist] = v where i is a row
// (labels, nodes: either may be null); hdr[kResLabelled] += such nodes
void launch_result_emit(const uint64_t* st, const uint32_t* rowof, const uint32_t* order,
                        const uint32_t* cnt, const uint32_t* off, uint32_t members, uint32_t n,
                        uint32_t slots, uint32_t* labels, uint32_t* nodes, uint32_t* hdr,
                        hipStream_t s, uint32_t grid_cap = 0);
// cnt = 1, head = tail = order = i, nxt = kNil for i < n (rows loaded as singletons)
void launch_init_singletons(const Rows& r, uint32_t* order, uint32_t n, hipStream_t s,
                            uint32_t grid_cap = 0);
// Clustered rows from device memory (klsh_load_clusters_device): off = the caller's n + 1 member
// offsets, nodes = the caller's node array at entry off[0] (null: entry q is node q), m = off[n] -
// off[0] entries.  *err (preset to ~0) = the smallest (index << 2 | kLcErr*) a check refused.
constexpr uint32_t kLcErrOffsets = 0;  // index = a row with off[i + 1] <= off[i]
constexpr uint32_t kLcErrRange = 1;    // index = an entry whose node is not below `members`
constexpr uint32_t kLcErrTwice = 2;    // index = an entry whose node an earlier entry lists
// rows: strictly increasing offsets; start[off[i] - off[0]] = 1 (m bytes, zeroed by the caller;
// null: check only)
void launch_clusters_check_rows(const uint32_t* off, uint32_t n, uint32_t m, uint8_t* start,
                                unsigned long long* err, hipStream_t s, uint32_t grid_cap = 0);
// entries: every node below `members`, none twice; owner (members words, preset to kNil) ends as
// the first entry listing each node
void launch_clusters_check_nodes(const uint32_t* nodes, uint32_t m, uint32_t members,
                                 uint32_t* owner, unsigned long long* err, hipStream_t s,
                                 uint32_t grid_cap = 0);
// checked input -> r.nxt (kNil for every node in no list), r.cnt, r.head, r.tail, order = identity
void launch_clusters_link(const Rows& r, uint32_t* order, const uint32_t* off,
                          const uint32_t* nodes, const uint8_t* start, uint32_t n, uint32_t m,
                          uint32_t members, hipStream_t s, uint32_t grid_cap = 0);

// ---- the cluster files (klsh_save.hip) -----------------------------------------
// off, nodes: the result's n + 1 member offsets and flat node lists (launch_result_emit).  A row
// is kept when off[i + 1] - off[i] > ignore_small.  Every launch strides over its range on its
// own and takes option "grid_cap".
constexpr uint32_t kSaveTile = 256;        // entries per text tile: one token per lane
constexpr uint32_t kSaveMaxToken = 32;     // header (<= 10 digits), '\t', id (<= 20 digits), '\n'
constexpr uint32_t kSaveKept = 0;          // hdr (64-bit words): kept rows
constexpr uint32_t kSaveMembers = 1;       //   their members
constexpr uint32_t kSaveErr = 2;           //   non-zero: an entry whose node is outside the table
constexpr uint32_t kSaveHdrWords = 4;
inline uint64_t save_tiles(uint64_t total) { return (total + kSaveTile - 1) / kSaveTile; }
// kslot[rank of kept row i] = order[i]; hdr[kSaveKept], hdr[kSaveMembers] (hdr zeroed by the
// caller).  tsum: result_tiles(n) words.
void launch_save_keep(const uint32_t* order, const uint32_t* off, uint32_t n, uint32_t ignore_small,
                      uint32_t* tsum, uint32_t* kslot, unsigned long long* hdr, hipStream_t s,
                      uint32_t grid_cap = 0);
// The text's entries: ids (node -> id; null: id = id_base + node) of `members` nodes.
struct SaveText {
  const uint32_t* off;
  const uint32_t* nodes;
  const uint64_t* ids;
  uint64_t id_base;
  uint32_t n, total, members, ignore_small;
};
// tpos[t] = pos_base + the bytes of the tokens of entries below t * kSaveTile, t <= save_tiles
// (tpos[save_tiles] = pos_base + the text's length): three launches, 64-bit sums.
void launch_save_positions(const SaveText& tx, uint64_t pos_base, uint64_t* tpos,
                           unsigned long long* hdr, hipStream_t s, uint32_t grid_cap = 0);
// The bytes at positions [w0, w1) of the text, from tiles [t_lo, t_hi) (every tile that holds one
// of them), to out[0, w1 - w0) (16-byte aligned).  Nothing outside that range is stored.
void launch_save_emit(const SaveText& tx, const uint64_t* tpos, uint64_t t_lo, uint64_t t_hi,
                      uint64_t w0, uint64_t w1, uint8_t* out, hipStream_t s, uint32_t grid_cap = 0);

// ---- the cluster files read back (klsh_diff.hip) --------------------------------
// The text of <F>.clust on the device: len < 2^32 bytes in a buffer of diff_text_alloc(len) bytes,
// every byte from len on a newline, so that a tile's 16-byte loads and a token's look-ahead are
// unconditional and in bounds.  Every launch strides over its tiles on its own and takes option
// "grid_cap".
constexpr uint32_t kDiffTile = 256 * 16;  // bytes per text tile: 16 aligned bytes per lane
constexpr uint32_t kDiffPad = 32;         // newline bytes past the last tile, at least
constexpr uint32_t kDiffMaxDigits = 18;   // a longer digit run makes the text irregular
constexpr uint32_t kDiffLineTile = 256;   // lines / entries per tile of the later passes
inline uint64_t diff_tiles(uint64_t len) { return (len + kDiffTile - 1) / kDiffTile; }
inline uint64_t diff_text_alloc(uint64_t len) { return diff_tiles(len) * kDiffTile + kDiffPad; }
inline uint64_t diff_line_tiles(uint64_t n) { return (n + kDiffLineTile - 1) / kDiffLineTile; }
// hdr (64-bit words; the caller sets hdr[kDiffIrregular] to all ones and zeroes the rest)
constexpr uint32_t kDiffIrregular = 0;  // the smallest offset that makes the text irregular
constexpr uint32_t kDiffNewlines = 1;
constexpr uint32_t kDiffTokens = 2;     // maximal digit runs
constexpr uint32_t kDiffLines = 3;      // newlines, + 1 for an unterminated last line
constexpr uint32_t kDiffEntries = 4;    // the declared counts' sum, saturating at kDiffSat
constexpr uint32_t kDiffIdsA = 5, kDiffIdsB = 6, kDiffKmersA = 7, kDiffKmersB = 8;
constexpr uint32_t kDiffHdrWords = 16;
constexpr uint64_t kDiffSat = 1ull << 62;
// per tile: newlines, token starts (tile_nl, tile_ts: diff_tiles(len) words each), the smallest
// irregular offset; then their exclusive prefixes in place and hdr[kDiffNewlines .. kDiffLines]
void launch_diff_scan(const uint8_t* txt, uint32_t len, uint32_t* tile_nl, uint32_t* tile_ts,
                      unsigned long long* hdr, hipStream_t s, uint32_t grid_cap = 0);
// tok_val[t] = the value of token t (n_tokens of them), line_tok0[l] = the tokens before line l
// (n_lines + 1 entries): only for a regular text
void launch_diff_tokens(const uint8_t* txt, uint32_t len, const uint32_t* tile_nl,
                        const uint32_t* tile_ts, uint32_t n_lines, uint32_t n_tokens,
                        uint64_t* tok_val, uint32_t* line_tok0, hipStream_t s, uint32_t grid_cap = 0);
// cnt[c] = line c's first token (0 without one); csum[t] = the saturating sum of the counts of the
// lines before tile t, t <= diff_line_tiles(n_lines); hdr[kDiffEntries] = the whole sum
void launch_diff_counts(const uint64_t* tok_val, const uint32_t* line_tok0, uint32_t n_lines,
                        uint64_t* cnt, uint64_t* csum, unsigned long long* hdr, hipStream_t s,
                        uint32_t grid_cap = 0);
// off[c] = the counts before line c, c <= n_lines (only when their sum is below 2^32)
void launch_diff_offsets(const uint64_t* cnt, const uint64_t* csum, uint32_t n_lines, uint32_t* off,
                         hipStream_t s, uint32_t grid_cap = 0);
// ids[q], q < total = off[n_lines]: entry j of line c is the line's token 1 + j, 0 past its tokens
void launch_diff_ids(const uint64_t* tok_val, const uint32_t* line_tok0, const uint32_t* off,
                     uint32_t n_lines, uint32_t total, uint64_t* ids, hipStream_t s,
                     uint32_t grid_cap = 0);
// mark_a[id] = 1 / mark_b[id] = 1 for the ids < kmap of the entries of group-1 / group-2 lines
void launch_diff_mark(const uint32_t* off, uint32_t n_lines, const uint64_t* ids, uint32_t total,
                      const uint8_t* group, uint64_t kmap, uint8_t* mark_a, uint8_t* mark_b,
                      hipStream_t s, uint32_t grid_cap = 0);
// hdr[kDiffIdsA ..] += the marks of each set, and the rows each set takes (A first)
void launch_diff_count(const uint8_t* mark_a, const uint8_t* mark_b, uint64_t kmap,
                       unsigned long long* hdr, hipStream_t s, uint32_t grid_cap = 0);
// row i of kmers (the images of kmer_set.hex) into table A if marked A, else into B if marked B
void launch_diff_insert(const uint64_t* kmers, const uint8_t* mark_a, const uint8_t* mark_b,
                        uint64_t kmap, uint64_t* tab_a, uint64_t mask_a, uint64_t* tab_b,
                        uint64_t mask_b, hipStream_t s, uint32_t grid_cap = 0);

// ---- plain FASTQ parsed on the device (klsh_fastq.hip) --------------------------
// A chunk of the file on the device: len < 2^32 bytes in a buffer of fq_text_alloc(len) bytes (the
// bytes from len on are never looked at).  Record r = lines 4r .. 4r + 3; n = newlines / 4.
constexpr uint32_t kFqTile = 256 * 16;  // bytes per text tile: 16 aligned bytes per lane
constexpr uint32_t kFqRecTile = 256;    // records per tile of the record passes
inline uint64_t fq_tiles(uint64_t len) { return (len + kFqTile - 1) / kFqTile; }
inline uint64_t fq_text_alloc(uint64_t len) { return (fq_tiles(len) + 1) * kFqTile; }
inline uint64_t fq_record_tiles(uint64_t n) { return (n + kFqRecTile - 1) / kFqRecTile; }
// hdr (64-bit words; the caller sets hdr[kFqIrregular] to all ones and zeroes the rest)
constexpr uint32_t kFqIrregular = 0;  // the smallest offset that makes a complete record irregular
constexpr uint32_t kFqNewlines = 1;
constexpr uint32_t kFqRecords = 2;    // newlines / 4
constexpr uint32_t kFqBases = 3;      // the records' len(L1), summed
constexpr uint32_t kFqConsumed = 4;   // line_start[4 n]: the end of the last complete record
constexpr uint32_t kFqHdrWords = 8;
// tile_nl (fq_tiles(len) words) = the newlines before each tile; hdr[kFqNewlines], hdr[kFqRecords]
void launch_fq_scan(const uint8_t* txt, uint32_t len, uint32_t* tile_nl, unsigned long long* hdr,
                    hipStream_t s, uint32_t grid_cap = 0);
// line_start[l] = the offset of line l's first byte, l <= 4 n_records; the bytes of those lines
// checked against their kind: hdr[kFqIrregular] = min(itself, the smallest offender)
void launch_fq_lines(const uint8_t* txt, uint32_t len, const uint32_t* tile_nl, uint32_t n_records,
                     uint32_t* line_start, unsigned long long* hdr, hipStream_t s,
                     uint32_t grid_cap = 0);
// off[r] = the bases before record r, r <= n_records (64-bit, as launch_check_reads and
// launch_kcount_reads take them); hdr[kFqBases], hdr[kFqConsumed]; a record whose L3 is not as long as its L1 puts
// line_start[4r + 3] + min(len(L1), len(L3)) into hdr[kFqIrregular].  rec_sum:
// fq_record_tiles(n_records) words.
void launch_fq_records(const uint32_t* line_start, uint32_t n_records, uint32_t* rec_sum,
                       uint64_t* off, unsigned long long* hdr, hipStream_t s, uint32_t grid_cap = 0);
// seq[off[r] .. off[r + 1]) = record r's L1, unless hdr[kFqIrregular] is set by then; seq holds
// seq_bytes
void launch_fq_pack(const uint8_t* txt, uint32_t len, const uint32_t* line_start, const uint64_t* off,
                    uint32_t n_records, const unsigned long long* hdr, uint8_t* seq,
                    uint64_t seq_bytes, hipStream_t s, uint32_t grid_cap = 0);

// Floating-point self test: sqrt_out[i] = sqrtf(a[i]); div_out[i] = a[i] / b[i] as the merge
// kernels evaluate them.
void launch_fp_selftest(const float* a, const float* b, uint32_t n, float* sqrt_out,
                        float* div_out, hipStream_t s);

// ---- sharded loop (klsh_shard.hip) ----------------------------------------------
constexpr int kMaxBinBits = 12;           // key ranges are unions of 2^12 top-bit bins
constexpr int kMaxRanks = 64;

// hist[bin] += 1 for every key (bin = key >> shift, < nbins); hist zeroed by the caller.
// grid_cap (here and below): option "grid_cap", 0 = off (cap_grid).
void launch_bin_hist(const uint32_t* keys, uint32_t n, int shift, uint32_t nbins, uint32_t* hist,
                     hipStream_t s, uint32_t grid_cap = 0);
// From every rank's histogram (hist_all[W][nbins]) and the total row count: owner[bin] = the rank
// owning the bin (contiguous, balanced by rows), cntmat[g * W + r] = rows rank g sends rank r.
void launch_bin_split(const uint32_t* hist_all, int world, uint32_t nbins, uint64_t total,
                      uint32_t* owner, uint32_t* cntmat, hipStream_t s);
// dest[i] = owner[keys[i] >> shift]; idx[i] = i.
// Stable partition of (keys[i], slots[i]), i < n, by owner[keys[i] >> shift] (world <= 64)
// into out, owner-major (out's owner blocks start at the exclusive prefix of the send counts).
// counts: world * ceil(n / 4096) words of workspace.  Returns -1 for an unsupported world.
int launch_partition(const uint32_t* keys, const uint32_t* slots, uint32_t n, int shift,
                     const uint32_t* owner, int world, uint32_t* counts, uint32_t* tile_sums,
                     Counters* ctr, uint2* out, hipStream_t s);
void launch_dest(const uint32_t* keys, uint32_t n, int shift, const uint32_t* owner,
                 uint32_t* dest, uint32_t* idx, hipStream_t s);
// out[i] = (keys[idx[i]], slots[idx[i]]).
void launch_pack_pairs(const uint32_t* keys, const uint32_t* slots, const uint32_t* idx,
                       uint32_t n, uint2* out, hipStream_t s);
// keys[i] = in[i].x, slots[i] = in[i].y.
void launch_unpack_pairs(const uint2* in, uint32_t n, uint32_t* keys, uint32_t* slots,
                         hipStream_t s);
// Delta records, stride 5 + dp words: slot, cnt, head, tail, nrm bits, row[dp].
__host__ __device__ inline int delta_words(int dp) { return 5 + dp; }
void launch_delta_pack(const Rows& r, const uint32_t* delta_slots, uint32_t n, uint32_t* rec,
                       hipStream_t s, uint32_t grid_cap = 0);
void launch_delta_apply(const Rows& r, const uint32_t* rec, uint32_t n, hipStream_t s,
                        uint32_t grid_cap = 0);
// Merge profile of the diagnostics build (-DKLSH_MERGE_PROF): print and clear.
void merge_prof_dump(FILE* f);

// a[i] = min(a[i], b[i])
void launch_min_u32(uint32_t* a, const uint32_t* b, size_t n, hipStream_t s);

// ---- modes E, B, K: every table below is the k-mer table of klsh_kmer.h (`mask + 1` 64-bit slots,
// all ones = empty); every launch takes option "grid_cap" last ---------------------------------
// mode E (klsh_extract.hip): kmers[i] into the set's table (all ones skipped)
void launch_kset_insert(const uint64_t* kmers, uint64_t n, uint64_t* tab, uint64_t mask,
                        hipStream_t s, uint32_t grid_cap = 0);
// slots[i] = the slot of keys[i] in the set's table, all ones if it is absent (klsh_kset_find)
void launch_kset_find(const uint64_t* keys, uint64_t n, const uint64_t* tab, uint64_t mask,
                      uint64_t* slots, hipStream_t s, uint32_t grid_cap = 0);
constexpr uint32_t kCheckWindow = 2048;  // k-mer positions per LDS window (per wave)
// Read r = seq[off[r] .. off[r+1]): hits[r] = its k-mer positions whose canonical k-mer is in the
// set, flags[r] = hits / (len - k + 1) > vote (float), both 0 for reads shorter than k + 10.
void launch_check_reads(const uint8_t* seq, const uint64_t* off, uint64_t n, int k, float vote,
                        const uint64_t* tab, uint64_t mask, uint32_t* hits, uint8_t* flags,
                        hipStream_t s, uint32_t grid_cap = 0);

// mode B (klsh_kmc.hip): the k-mer table of KMC databases
struct KmcParams {
  int k, p;                   // k-mer length, LUT prefix symbols
  uint32_t sufix_size;        // (k - p) / 4 bytes per record
  uint32_t counter_size;      // bytes
  uint32_t rec_size;          // sufix_size + counter_size
  uint32_t min_count;
  uint64_t max_count;
  uint64_t prefix_mask;       // (1 << 2p) - 1
};
// records [0, n) of a .kmc_suf chunk starting at record rec0 -> canonical rep (all ones = outside
// [min_count, max_count]) and counter; *n_valid += records kept.  lut: lut_n entries, the last the
// total + 1 sentinel.
void launch_kmc_decode(const uint8_t* recs, uint64_t n, uint64_t rec0, const KmcParams& kp,
                       const uint64_t* lut, uint64_t lut_n, uint64_t* rep, uint32_t* cnt,
                       uint32_t* n_valid, hipStream_t s, uint32_t grid_cap = 0);
void launch_kmc_union(const uint64_t* rep, uint64_t n, uint64_t ord0, uint64_t* tab,
                      uint64_t* first, uint64_t mask, hipStream_t s, uint32_t grid_cap = 0);
void launch_kmc_count(const uint64_t* rep, const uint32_t* cnt, uint64_t n, const uint64_t* tab,
                      uint64_t mask, uint32_t* acc, hipStream_t s, uint32_t grid_cap = 0);
// occupied slots -> (low word of their first-appearance ordinal, slot), *n_out of them
void launch_kmc_collect(const uint64_t* tab, const uint64_t* first, uint64_t cap, uint32_t* lo,
                        uint32_t* slot, uint32_t* n_out, hipStream_t s, uint32_t grid_cap = 0);
// out[i] = src[idx[i]], or hi[i] = its high word
void launch_ktab_gather(const uint64_t* src, const uint32_t* idx, uint64_t n, uint64_t* out,
                        hipStream_t s, uint32_t grid_cap = 0);
void launch_ktab_gather(const uint64_t* src, const uint32_t* idx, uint64_t n, uint32_t* hi,
                        hipStream_t s, uint32_t grid_cap = 0);
void launch_kmc_emit(const uint32_t* acc, const uint32_t* order, uint64_t n, uint16_t* out,
                     hipStream_t s, uint32_t grid_cap = 0);
// The n collected slots in stable ascending order of word[slot], a word of `bits` bits (1..64)
// whose low halves are in lo (modes B and K, klsh_kmc.cpp): a radix sort over min(bits, 32) bits,
// then, if the word has high bits, their gather into the free key buffer and a sort over
// bits - 32.  (lo, slots) and (lo2, slots2) ping-pong, ws: sort_ws_words(n) words; *order = the
// slot buffer that holds the result.  Returns whether the high pass ran.
bool order_slots_u64(uint32_t* lo, uint32_t* slots, uint32_t* lo2, uint32_t* slots2, uint32_t n,
                     int bits, uint32_t* ws, const uint64_t* word, hipStream_t s, uint32_t grid_cap,
                     uint32_t** order);

// klsh_build_khtable's test hooks and what its last call on the context reached (options
// "kmc_chunk_records", "kmc_ordinal_base", "kmc_keep_first"; read-only "kmc_decode_launches",
// "kmc_high_sort"; klsh_khtable_first).  The defaults are the product's behaviour.
struct KmcHooks {
  uint64_t chunk_records = 0;    // records per .kmc_suf chunk (0 = what 64 MB hold; never more)
  uint64_t ordinal_base = 0;     // ordinal of sample 0's record 0
  bool keep_first = false;       // keep the first-appearance list of the next calls in `first`
  uint64_t decode_launches = 0;  // pass 1's k_kmc_decode launches
  int high_sort = 0;             // 1 = the ordinals' high words were sorted
  uint32_t grid_cap = 0;         // "grid_cap": workgroups per launch of the table build, at most
  std::vector<uint64_t> first;   // distinct canonical k-mers by first ordinal
};

// The records of a set of samples as the table build streams them, twice: pass 0 (the union, in
// first-appearance order) and pass 1 (the counts).  klsh_build_khtable decodes KMC databases
// (klsh_kmc.cpp), klsh_count_khtable hands over the listings it counted (klsh_kcount.cpp).
// Per pass and sample: begin, then feed for r0 = 0, chunk, 2 chunk, ... below total, then end.
class KhSource {
 public:
  virtual ~KhSource() {}
  virtual uint64_t total(int j) const = 0;  // records of sample j (its ordinals: base .. + total)
  virtual uint64_t chunk(int j) const = 0;  // records per feed, at most
  virtual int begin(int j, int pass, hipStream_t s) = 0;
  // records [r0, r0 + n) of the sample on the device: *rep their canonical images (all ones = not
  // listed), *cnt their counters; queued on s, valid until the next feed
  virtual int feed(int j, int pass, uint64_t r0, uint64_t n, const uint64_t** rep,
                   const uint32_t** cnt, hipStream_t s) = 0;
  // host work on the chunk just fed, while the device runs it (the stream is synchronized after)
  virtual void fed(int j, int pass, uint64_t n) {}
  // pass 0: *listed = records listed; pass 1: *coverage = float running sum of log(count) in
  // listing order (kmer/kmc_reader.cc:143)
  virtual int end(int j, int pass, uint64_t* listed, float* coverage, hipStream_t s) = 0;
};
// The table of those records (buildKHtable, io/ioHT.cc:83-199): union in first-appearance order,
// the reference's libcuckoo row order, kmer_set.hex / kmer_count.bin / kmer_count.log in out_dir.
// Fills st's kmap_size, records, records_listed, order_ms.
int khtable_run(klsh_ctx* ctx, KhSource& src, int n_samples, int k, const char* out_dir,
                klsh_khtable_stats* st);

// mode K (klsh_kcount.hip): counting a sample's canonical k-mers
constexpr uint32_t kKcountWindow = 2048;  // k-mer positions per LDS window (per wave)
// reads seq[off[r] .. off[r+1]) counted into the table (cnt: the slots' occurrence counts);
// ctr[0] += slots claimed, ctr[1] += valid k-mer windows
void launch_kcount_reads(const uint8_t* seq, const uint64_t* off, uint64_t n, int k, uint64_t* keys,
                         uint32_t* cnt, uint64_t mask, uint64_t* ctr, hipStream_t s,
                         uint32_t grid_cap = 0);
// every entry of the old table into the (empty) new one
void launch_kcount_rehash(const uint64_t* okeys, const uint32_t* ocnt, uint64_t ocap, uint64_t* keys,
                          uint32_t* cnt, uint64_t mask, hipStream_t s, uint32_t grid_cap = 0);
// slots with count >= count_min -> (low word of their KMC value, slot), *n_out of them
void launch_kcount_collect(const uint64_t* keys, const uint32_t* cnt, uint64_t cap,
                           uint32_t count_min, uint32_t* lo, uint32_t* slot, uint32_t* n_out,
                           hipStream_t s, uint32_t grid_cap = 0);
// the listing in `order`: KMC value, canonical Kmer image, min(count, 65535)
void launch_kcount_emit(const uint64_t* keys, const uint32_t* cnt, const uint32_t* order, uint64_t n,
                        int k, uint64_t* val, uint64_t* rep, uint32_t* out_cnt, hipStream_t s,
                        uint32_t grid_cap = 0);
// A listing as a KMC1-layout database (klsh_count_kmc): records [r0, r0 + m) of (val, cnt) as
// .kmc_suf record bytes in out[0, m * (sufix_size + 2)) — sufix_size = (k - p) / 4 big-endian
// suffix bytes, then the 2-byte little-endian counter; out 4-byte aligned
constexpr uint32_t kKmcdbMaxRec = 10;  // k = 32, p = 0: 8 suffix bytes + the counter
void launch_kmcdb_pack(const uint64_t* val, const uint32_t* cnt, uint64_t r0, uint64_t m,
                       uint32_t sufix_size, uint8_t* out, hipStream_t s, uint32_t grid_cap = 0);
// lut[i] = records whose prefix (val >> 2 (k - p)) is below q0 + i, for i < mq; val: n ascending
void launch_kmcdb_lut(const uint64_t* val, uint64_t n, uint64_t q0, uint64_t mq, int k, int p,
                      uint64_t* lut, hipStream_t s, uint32_t grid_cap = 0);

// klsh_count_khtable's / klsh_count_kmc's test hooks and what the last call on the context
// reached (options "kcount_batch_reads", "kcount_table_slots", "kcount_keep_listing",
// "kcount_db_prefix", "kcount_db_chunk_records"; read-only "kcount_batches", "kcount_rehashes",
// "kcount_peak_slots", "kcount_window", "kcount_db_chunks", "kcount_db_prefix_used";
// klsh_kcount_listing).
struct KcountHooks {
  uint64_t batch_reads = 0;   // reads per batch (0 = 2^18)
  uint64_t table_slots = 0;   // a sample's initial table (0 = 2^22 slots)
  bool keep_listing = false;  // keep the per-sample listings of the next calls
  uint64_t batches = 0, rehashes = 0;
  uint64_t peak_slots = 0;    // the largest sample table of the last call
  int db_prefix = -1;              // a database's LUT prefix length (-1 = the size rule)
  uint64_t db_chunk_records = 0;   // records per .kmc_suf chunk (0 = 2^22)
  uint64_t db_chunks = 0;          // k_kmcdb_pack launches of the last call
  int db_prefix_used = -1;         // the prefix length of its last database (-1 = none written)
  uint32_t grid_cap = 0;           // "grid_cap": workgroups per counting / packing launch, at most
  std::vector<std::vector<uint64_t>> values;  // per sample: the listed KMC values, ascending
  std::vector<std::vector<uint32_t>> counts;
};

}  // namespace klsh
