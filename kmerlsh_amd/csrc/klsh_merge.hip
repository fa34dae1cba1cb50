// Greedy in-bucket merge for gfx950: p_cluster (reference function/cluster.cc:56-87) with the
// cosine test (function/distance.cc:27-38) and the consensus (function/funcAB.cc:49-71), run
// over every bucket of one LSH iteration.
//
// The reference walks a bucket sequentially: row i merges into the FIRST j < i with
// 1 - cosine(i, j) >= thr; the consensus replaces j, row i is overwritten by the last row and
// re-tested.  A decision only changes when one of its two rows changes, and only the candidate j
// of a merge changes, so the GPU version evaluates decisions in bulk and replays the walk.
// Results are positional (survivors in place, kInvalid after), so they do not depend on which
// wave handled which run or in what order.
//
// The device code, by the runs (rows of one bucket) and row widths d it serves:
//   klsh_merge_common.h  fences, profile macros and counters, shuffles, sequential dots, prescreen
//   klsh_merge_small.h   2..64 rows, d = 8/16/32/64: k_merge_small (G-lane groups, rows in
//                        registers), k_small_screen (fp16 screen in front of it, d = 32/64)
//   klsh_merge_runs.h    the listing of the runs by size class, any length and d: k_runs_count,
//                        k_runs_scan, k_runs_write; k_tail_local (small iterations: bucket sort +
//                        listing in one launch)
//   klsh_merge_gram.h    gram_tile: all-pairs decisions on the matrix cores, d a multiple of 16
//   klsh_merge_huge.h    over 896 rows, any d: k_merge_huge (the reference order directly)
//   klsh_merge_big.h     65..896 rows, d = 8/16/32/64: k_merge_big (one launch per class 65..128,
//                        129..192, 193..384, 385..896; decision matrix in LDS), k_merge_tail (every
//                        class of a small iteration in one launch)
//   klsh_merge_long.h    897..kLongRows rows (optionally from 385), d = 16/32, fast decider:
//                        k_merge_long (decision matrix in global memory, one step per merge)
//   klsh_merge_wide.h    every other d (d > 64, or no register kernel): k_merge_group_wide (2..64
//                        rows), k_merge_big_wide (65..896 rows; longer ones through huge_runs)
// This file is the host side: the decider, the launch geometry of every class and the profile dump.
//
// All of it is ONE translation unit, on purpose: k_merge_tail<D> instantiates every class
// (small_loop, big_runs x4, huge_runs) in one kernel, k_merge_big<.., 896, ..> and
// k_merge_big_wide<896, ..> fold huge_runs in, k_merge_long falls back to it, and the profile
// counters (g_mprof ...) are device globals of this unit that merge_prof_dump reads.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "klsh_merge_common.h"
#include "klsh_merge_small.h"
#include "klsh_merge_runs.h"
#include "klsh_merge_gram.h"
#include "klsh_merge_huge.h"
#include "klsh_merge_big.h"
#include "klsh_merge_long.h"
#include "klsh_merge_wide.h"

namespace klsh {

// ----------------------------------------------------------------------------- launch -----
// The smallest float s with fl(1 - fl(1 - s)) >= thr (cluster.cc:68-69), by bisection over the
// ordered floats; see Decider.
static float sim_roundtrip(float s) {
  volatile float dist = 1.0f - s;
  volatile float sim = 1.0f - dist;
  return sim;
}
static uint32_t ordered(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static float from_ordered(uint32_t o) {
  const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

Decider make_decider(float thr) {
  Decider dc{std::numeric_limits<float>::quiet_NaN(), 0.0f, 0.0f, 0u, 0.0f, 0.0f};
  uint32_t lo = ordered(-std::numeric_limits<float>::infinity());
  uint32_t hi = ordered(std::numeric_limits<float>::infinity());
  if (!(sim_roundtrip(from_ordered(hi)) >= thr)) return dc;  // nothing passes (thr NaN)
  while (lo < hi) {  // invariant: hi passes
    const uint32_t mid = lo + (hi - lo) / 2;
    if (sim_roundtrip(from_ordered(mid)) >= thr) hi = mid;
    else lo = mid + 1;
  }
  dc.s_star = from_ordered(hi);
  if (dc.s_star >= 0x1p-60f && dc.s_star <= 0x1p60f) {
    dc.s_lo = from_ordered(hi - 8);
    dc.s_hi = from_ordered(hi + 8);
    dc.fast = 1u;
    dc.g_lo = dc.s_star - kGramMargin;
    dc.g_hi = dc.s_star + kGramMargin;
  }
  return dc;
}

// Raises the kernels' dynamic-LDS limit to `bytes`.  Every caller keeps the result in a
// function-local static, so a kernel is set once per process, and ignores it.
template <class... K>
static bool raise_lds_limit(size_t bytes, K*... kern) {
  bool ok = true;
  ((ok = ok && hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)bytes) == hipSuccess), ...);
  return ok;
}

// What one launch's kernels read: the plan's lists and fold policy, the call's sink and stamps,
// and the launch's own flags.
static MergeView view(const MergePlan& p, const MergeCall& c, uint32_t screened = 0u,
                      BigScreen bs = BigScreen{0u, 0.0f, 0.0f, 0.0f}) {
  return MergeView{p.lists, c.sink, c.kt, screened, p.huge_fold, bs};
}

static void launch_huge(const MergePlan& p, const MergeCall& c, uint32_t* slots, const Decider& dc,
                        const Rows& r, Counters* ctr, uint32_t n, hipStream_t s) {
  const bool with896 = long896(p, dc, r);
  if (p.huge_fold && !with896) return;  // the 385..896-row kernel walks them (k_merge_big)
  uint32_t g = (uint32_t)std::min<uint64_t>(512, n / (kBigRows[kBigClasses - 1] + 1) + 1);
  if (p.huge_cap && !with896) g = std::min(g, p.huge_cap);  // (the kernel strides over its list)
  if (with896) g = (uint32_t)std::min<uint64_t>(1024, n / (kBigRows[kBigClasses - 2] + 1) + 1);
  const RunLists& l = p.lists;
  const MergeView w = view(p, c);
  if (long_ok_for(p, dc, r)) {
    const size_t lds = std::max(long_lds(), huge_lds(r.d, r.dp, kLongNT));
    static const bool lds_ok = raise_lds_limit(lds, &k_merge_long<16>, &k_merge_long<32>);
    (void)lds_ok;
    // (the matrices stay sized for long_groups workgroups; "grid_cap" only leaves some unused)
    g = cap_grid(std::min(g, p.long_groups), c.grid_cap);
    const uint2* l2 = with896 ? l.big[kBigClasses - 1] : nullptr;
    const uint32_t* c2 = &l.rc->n_big[kBigClasses - 1].v;
    if (r.d == 16)
      k_merge_long<16><<<g, kLongNT, lds, s>>>(l.huge, &l.rc->n_huge.v, l2, c2, slots, dc, r, w, ctr);
    else
      k_merge_long<32><<<g, kLongNT, lds, s>>>(l.huge, &l.rc->n_huge.v, l2, c2, slots, dc, r, w, ctr);
    return;
  }
  g = cap_grid(g, c.grid_cap);
  const size_t lds = huge_lds(r.d, r.dp, kHugeNT);
  static const bool lds_ok =
      raise_lds_limit(96 * 1024, &k_merge_huge<0>, &k_merge_huge<8>, &k_merge_huge<16>,
                      &k_merge_huge<32>, &k_merge_huge<64>);
  (void)lds_ok;
  switch (r.d) {
    case 8: k_merge_huge<8><<<g, kHugeNT, lds, s>>>(l.huge, &l.rc->n_huge.v, slots, dc, r, w, ctr); break;
    case 16: k_merge_huge<16><<<g, kHugeNT, lds, s>>>(l.huge, &l.rc->n_huge.v, slots, dc, r, w, ctr); break;
    case 32: k_merge_huge<32><<<g, kHugeNT, lds, s>>>(l.huge, &l.rc->n_huge.v, slots, dc, r, w, ctr); break;
    case 64: k_merge_huge<64><<<g, kHugeNT, lds, s>>>(l.huge, &l.rc->n_huge.v, slots, dc, r, w, ctr); break;
    default: k_merge_huge<0><<<g, kHugeNT, lds, s>>>(l.huge, &l.rc->n_huge.v, slots, dc, r, w, ctr);
  }
}

// One class c of 65..896-row runs, for k_merge_big and k_merge_big_wide (rb rows per run at the
// most, nt lanes, `layout` bytes of LDS): a workgroup per run that n positions can hold at the
// class's shortest length, up to 1024; the 385..896 class takes huge_runs' LDS too when it folds
// the longer runs in (MergePlan::huge_fold).
template <class Kern>
static void launch_big_class(Kern kern, int rb, int nt, size_t layout, const MergePlan& p,
                             const MergeCall& c, int cls, uint32_t* slots, const Decider& dc,
                             const Rows& r, Counters* ctr, uint32_t n, hipStream_t s) {
  const bool fold = rb == kBigRows[kBigClasses - 1] && p.huge_fold;
  const size_t lds = fold ? std::max(layout, huge_lds(r.d, r.dp, nt)) : layout;
  const uint32_t lo = cls == 0 ? 65u : (uint32_t)kBigRows[cls - 1] + 1u;
  const uint32_t g = cap_grid((uint32_t)std::min<uint64_t>(1024, n / lo + 1), c.grid_cap);
  kern<<<g, nt, lds, s>>>(view(p, c), cls, slots, dc, r, ctr);
}

template <int D, int RB, int NT, bool ROWS_LDS>
static void launch_big(const MergePlan& p, const MergeCall& c, int cls, uint32_t* slots,
                       const Decider& dc, const Rows& r, Counters* ctr, uint32_t n, hipStream_t s) {
  using L = BigLayout<D, RB, ROWS_LDS>;  // (r.d == D: launch_merge)
  const auto kern = &k_merge_big<D, RB, NT, ROWS_LDS>;
  static const bool lds_ok = raise_lds_limit(std::max<size_t>(L::bytes, 96 * 1024), kern);
  (void)lds_ok;
  launch_big_class(kern, RB, NT, L::bytes, p, c, cls, slots, dc, r, ctr, n, s);
}

// Fork the size-class kernels onto the auxiliary streams (after k_runs on s) and join them back
// into s.  Every class writes disjoint runs, so the order between classes is free.
struct Fork {
  const MergePlan& p;
  hipStream_t s;
  bool on;
  Fork(const MergePlan& p_, hipStream_t s_) : p(p_), s(s_) {
#ifdef KLSH_SERIAL_MERGE  // diagnostics build only: every class in order on the main stream
    on = false;
#else
    on = p.aux[0] != nullptr;
#endif
    if (!on) return;
    (void)hipEventRecord(p.fork, s);
    for (int i = 0; i < kMergeStreams; ++i) (void)hipStreamWaitEvent(p.aux[i], p.fork, 0);
  }
  hipStream_t lane(int i) const { return on ? p.aux[i] : s; }
  ~Fork() {
    if (!on) return;
    for (int i = 0; i < kMergeStreams; ++i) {
      (void)hipEventRecord(p.join[i], p.aux[i]);
      (void)hipStreamWaitEvent(s, p.join[i], 0);
    }
  }
};

// The small-run screen's margin (k_small_screen): |q~ - q_ref| <= m0 + a2 (1/|x~a| + 1/|x~b|) for
// the screen's quotient q~ = x~a.x~b / (|x~a| |x~b|) against the reference's fl(dot / den):
//   m0: fp16 rounding of both rows in the dot (2 * 2^-11) and in the two norms (2 * 2^-11),
//       2^-20 for the products of the rounding errors, (4d + 16) 2^-24 for the f32 sums of the
//       screen and of the reference (dot, |a|^2, |b|^2) and the sqrt / product / quotient roundings
//   a2: 2^-25 per element absolute (fp16 subnormals, which gfx950 keeps in the conversion, the
//       MFMA and v_dot2_f32_f16 under the default float mode: tools/denorm_probe.hip), summed with
//       Cauchy-Schwarz: sqrt(d) 2^-25 (|a| + |b|) / (|a||b|), doubled (the norms' own share)
// all times 1.5 for headroom.  Only with a fast decider (a normal s*) and the fp16 image.
static void screen_margins(int d, float* m0, float* a2) {
  *m0 = 1.5f * (0x1p-9f + 0x1p-20f + (4.0f * (float)d + 16.0f) * 0x1p-24f);
  *a2 = 1.5f * 2.0f * 0x1p-25f * std::sqrt((float)d);
}
static bool screen_ok(const Rows& r, const Decider& dc, const MergePlan& p) {
  return p.small_screen && r.xh && dc.fast && (r.d == 32 || r.d == 64);  // (tiles: d >= 32)
}

// Iterations below this many positions run every merge class in ONE launch (k_merge_tail) on the
// main stream: there the cross-stream fork/join (~35 us) costs more than the overlap buys.

template <int D>
static void launch_groups(const Rows& r, uint32_t* slots, const Decider& dc, const MergePlan& p,
                          const MergeCall& c, Counters* ctr, uint32_t n, hipStream_t s) {
  if (n < tail_merge_max(p)) {
    using L896 = BigLayout<D, 896, false>;
    using L384 = BigLayout<D, 384, true>;
    using L192 = BigLayout<D, 192, true>;
    using L128 = BigLayout<D, 128, true>;
    constexpr size_t small_lds = 4 * 64 * (D + 4) * sizeof(float);
    const size_t lds = std::max({L896::bytes, L384::bytes, L192::bytes, L128::bytes, small_lds,
                                 huge_lds(D, r.dp, 256)});
    static const bool lds_ok = raise_lds_limit(lds, &k_merge_tail<D>);
    (void)lds_ok;
    // options "tail_big_groups" / "tail_small_groups": 32 / 64 / 128 / 256 and 128 / 256 / 512 /
    // 1024 swept (round 3)
    const uint32_t nbig = p.tail_nbig ? p.tail_nbig : 128u;
    const uint32_t nsmall = p.tail_nsmall ? p.tail_nsmall : 512u;
    float m0 = 0.0f, a2 = 0.0f;
    const bool can_screen = screen_ok(r, dc, p);
    const bool big_screen = p.tail_big_screen && can_screen;
    const bool small_screen = p.tail_screen && can_screen;
    if (big_screen || small_screen) screen_margins(r.d, &m0, &a2);
    if (small_screen) {
      // the fp16 screen of the small runs first (few of them merge this late in the loop), on
      // the same stream: k_merge_tail's small-run waves then take only the runs it passed
      // (option tail_screen_grid; one box, interleaved C2: 512 → 214.9, 1024 → 210.0, 2048 →
      // 208.1 ms per step; tail_screen = 0: 213.3 ms)
      const uint32_t sgrid = p.tail_screen_grid ? p.tail_screen_grid : 2048u;
      k_small_screen<D><<<sgrid, 64, 0, s>>>(view(p, c), slots, r, dc.s_star, m0, a2, c.kt);
    }
    const BigScreen bs = big_screen ? BigScreen{1u, dc.s_star, m0, a2}
                                    : BigScreen{0u, 0.0f, 0.0f, 0.0f};
    k_merge_tail<D><<<nbig + nsmall, 256, lds, s>>>(view(p, c, small_screen ? 1u : 0u, bs), slots,
                                                    dc, r, ctr, nbig);
    return;
  }
  const Fork f(p, s);
  // The small-run chain (screen + merge: the merge phase's critical path in 146 of C2's 218
  // multi-launch iterations, rocprofv3 trace) on the main stream: it starts without the fork's
  // cross-stream wait, and at the join only the aux streams are waited for; the >384-row classes
  // on aux 2 (C2, one box, interleaved: 203.9 -> 200.8 ms per step).  Not when the previous
  // iteration had many 385..896-row runs (p.big896_aux, C4): the long walks are the critical
  // path there and keep the main stream (C4 989 -> 1120 ms with the small chain on it).
  const bool long_heavy = p.big896_aux != 0u;
  const hipStream_t s_small = long_heavy ? f.lane(2) : s, s_long = long_heavy ? s : f.lane(2);
  // longest walks first on each stream; the longest runs (few, long walks) on the main stream,
  // concurrent with the auxiliary ones (it waits for them at the join)
  launch_big<D, 384, 256, true>(p, c, 2, slots, dc, r, ctr, n, f.lane(0));
  // many 385..896-row runs (p.big896_aux): they go on aux 2, ahead of the small runs, instead of
  // in front of the >896-row runs on the main stream — serialised, the two long-walk classes
  // make the main stream the critical path (C4 1794 -> 1432 ms); with a handful of them (C2)
  // the main stream is the better place (measured 281-285 vs 284-294 ms)
  if (!long896(p, dc, r))
    launch_big<D, 896, 256, false>(p, c, 3, slots, dc, r, ctr, n, long_heavy ? f.lane(2) : s_long);
  launch_huge(p, c, slots, dc, r, ctr, n, s_long);
  // 129..192 rows: two workgroups per CU (62 KB of LDS at d = 64, VGPRs capped at 256 like the
  // 65..128 class), ahead of 65..128 on aux 1
  launch_big<D, 192, 256, true>(p, c, 1, slots, dc, r, ctr, n, f.lane(1));
  launch_big<D, 128, 128, true>(p, c, 0, slots, dc, r, ctr, n, f.lane(1));
  // every small-run class in one persistent launch (the kernel strides over its batches)
  // HIP events on its own stream too (bench.py's headline cross-check: this launch is alone on
  // aux 2, so the event pair measures it, unlike the big-run classes that wait for CU resources)
  // 12288 one-wave workgroups, 6 per resident slot (2048 at 2 waves per SIMD): the batch stride
  // of a persistent wave is long enough that its rows come from all over the lists, and waves
  // retire and re-enter as the big-run workgroups come and go (C2, same box, interleaved:
  // 4608 -> 255.9 / 258.0 ms, 8192 -> 255.4 / 252.3, 12288 -> 250.8 / 251.7, 16384 -> 256.0 /
  // 253.9; small-run merge 79.4 -> 70.5 ms per step)
  // the fp16 screen first (option small_screen, where the row image exists): the merge then
  // takes only the runs it could not rule out
  const bool screened = screen_ok(r, dc, p);
  if (screened) {
    float m0, a2;
    screen_margins(r.d, &m0, &a2);
    // (option small_screen_grid; one-wave workgroups: 2048 → 207.9 / 207.8 vs 3072 → 211.2 /
    // 211.1 ms per C2 step on one box, 1024 → 227–228, 1536 / 2560 within noise of 2048)
    const uint32_t sgrid = p.screen_grid ? p.screen_grid : 2048u;
    k_small_screen<D><<<sgrid, 64, 0, s_small>>>(view(p, c), slots, r, dc.s_star, m0, a2, c.kt);
  }
  if (c.small_ev[0]) (void)hipEventRecord(c.small_ev[0], s_small);
  const uint32_t grid = p.small_grid ? p.small_grid : 12288u;  // option "small_grid"
  k_merge_small<D><<<grid, 64, 0, s_small>>>(view(p, c, screened ? 1u : 0u), slots, dc, r, ctr);
  if (c.small_ev[0]) (void)hipEventRecord(c.small_ev[1], s_small);
}

template <int RB, int NT, int KC>
static void launch_big_wide(const MergePlan& p, const MergeCall& c, int cls, uint32_t* slots,
                            const Decider& dc, const Rows& r, Counters* ctr, uint32_t n,
                            hipStream_t s) {
  using L = BigWideLayout<RB, NT, KC>;
  const auto kern = &k_merge_big_wide<RB, NT, KC>;
  static const bool lds_ok = raise_lds_limit(std::max<size_t>(L::bytes, 96 * 1024), kern);
  (void)lds_ok;
  launch_big_class(kern, RB, NT, L::bytes, p, c, cls, slots, dc, r, ctr, n, s);
}

// |G - dot_ref| / (|a||b|) for the bf16x3 Gram value at width d against the reference's sequential
// f32 dot: split residuals 3.03 * 2^-16, the MFMA's f32 sums (16 internal adds + one per chained
// MFMA, three per k-step, at 2u), the reference's own (d + 1) * 2^-24 and the approximate quotient
// (4 * 2^-24), with 1.5x headroom (kGramMargin, 1e-4, covers d <= 64; at d = 512 this is 1.37e-4).
static float wide_gram_margin(int d) {
  const float ks = (float)((d + 15) / 16);
  return 1.5f * (3.03f * 0x1p-16f + (17.0f + 3.0f * ks) * 0x1p-23f + (float)(d + 1) * 0x1p-24f +
                 4.0f * 0x1p-24f);
}

static void launch_groups_wide(const Rows& r, uint32_t* slots, const Decider& dc,
                               const MergePlan& p, const MergeCall& c, Counters* ctr, uint32_t n,
                               hipStream_t s) {
  auto grid = [&](int cls, uint32_t per_wave) {
    // up to 8192 one-wave workgroups per class (was 2048: C5 2.58 / 2.55 -> 2.36 / 2.33 s per
    // step, interleaved on one box), as for the register-row small-run launch
    // option "wide_group_grid": 4096 -> 1221, 8192 -> 1141, 16384 -> 1103, 32768 -> 1102 ms
    // per C5 step (one box)
    const uint64_t cap = p.wide_group_grid ? p.wide_group_grid : 16384u;
    return (uint32_t)std::min<uint64_t>(cap, group_class_capacity(cls, n) / per_wave + 1);
  };
  const Fork f(p, s);
  launch_big_wide<384, 256, 32>(p, c, 2, slots, dc, r, ctr, n, f.lane(0));
  launch_big_wide<384, 256, 32>(p, c, 1, slots, dc, r, ctr, n, f.lane(0));  // 129..192 rows
  launch_big_wide<896, 256, 16>(p, c, 3, slots, dc, r, ctr, n, f.on ? s : f.lane(0));
  launch_huge(p, c, slots, dc, r, ctr, n, f.on ? s : f.lane(0));
  launch_big_wide<128, 128, 32>(p, c, 0, slots, dc, r, ctr, n, f.lane(1));
  // the small-run classes (runs of 2..64 rows), each a persistent launch of up to 16384
  // one-wave workgroups
  RunCounters* rc = p.lists.rc;
  const hipStream_t sl = f.lane(2);
  // (an fp16-image screen of these runs, k_small_screen_wide, ruled out 96 % of C5's small-run
  // rows and still cost more than it saved — 2.25 -> 2.78 s per step — and was removed in round 5)
  // runs of 8..64 rows at d = 512 (C5): pairwise decisions on the matrix cores (option
  // wide_gram) with the margin of the bf16x3 Gram value at this width (wide_gram_margin)
  const bool gram = p.wide_gram && dc.fast && r.d == 512;
  const uint32_t gmin = p.wide_gram;  // the smallest group width that decides on the matrix cores
  Decider dg = dc;
  if (gram) {
    const float m = wide_gram_margin(r.d);
    dg.g_lo = dc.s_star - m;
    dg.g_hi = dc.s_star + m;
  }
  // The six classes on four streams, not one chain (each class's launch ends with a tail of
  // latency-bound walks that leaves the chip idle, and the classes' register budgets differ, so
  // two of them share a SIMD's register file): the main stream takes 64 (behind the short
  // 385..896-row class), aux 0 32 (behind the 129..384-row classes), aux 1 8 and 4 (behind the
  // 65..128-row class), aux 2 16 and 2.  C5, interleaved on one box: one chain 1896 / 1898 ms,
  // this 1733 / 1736 (1691 / 1716 on a second box, where two other assignments measured
  // 1679–1713 ms).  Index: 5 - class (64, 32, 16, 8, 4, 2).
  const hipStream_t gs[6] = {s, f.lane(0), sl, f.lane(1), f.lane(1), sl};
  auto group = [&](auto kern, int cls, uint32_t per_wave, const Decider& dd) {
    kern<<<grid(cls, per_wave), 64, 0, gs[5 - cls]>>>(p.lists.cls[cls], &rc->n_cls[cls].v, slots,
                                                       dd, r, ctr, c.sink.dlist, c.kt);
  };
  if (gram && gmin <= 64) group(k_merge_group_wide<64, 512>, 5, 1, dg);
  else group(k_merge_group_wide<64>, 5, 1, dc);
  if (gram && gmin <= 32) group(k_merge_group_wide<32, 512>, 4, 2, dg);
  else group(k_merge_group_wide<32>, 4, 2, dc);
  if (gram && gmin <= 16) group(k_merge_group_wide<16, 512>, 3, 4, dg);
  else group(k_merge_group_wide<16>, 3, 4, dc);
  if (gram && gmin <= 8) group(k_merge_group_wide<8, 512>, 2, 8, dg);
  else group(k_merge_group_wide<8>, 2, 8, dc);
  group(k_merge_group_wide<4>, 1, 16, dc);
  group(k_merge_group_wide<2>, 0, 32, dc);
}

void launch_runs(const uint32_t* key, uint32_t lo, uint32_t n, int bucket_thr, const MergePlan& p,
                 const MergeCall& c, hipStream_t s, const uint32_t* n_dev) {
  const uint32_t ntiles = (n + kRunTile - 1) / kRunTile;
  // run_ws: counts [kRunRows][ntiles], tail ends [ntiles], then 8-byte aligned: first / last
  // heads (uint2) [ntiles], head bitmaps [ntiles][64]
  uint32_t* counts = p.run_ws;
  uint32_t* tail_ends = counts + (size_t)kRunRows * ntiles;
  uint2* heads_fl = reinterpret_cast<uint2*>(counts + (((kRunRows + 1u) * ntiles + 1u) & ~1u));
  uint64_t* hbits = reinterpret_cast<uint64_t*>(heads_fl + ntiles);
  k_runs_count<<<ntiles, 256, 0, s>>>(key, lo, n, bucket_thr, ntiles, hbits, heads_fl, counts,
                                      c.kt, n_dev);
  const bool fused = ntiles <= 256u;  // the write kernel scans the counts itself
  if (fused) {
    k_runs_write<true><<<ntiles, 256, 0, s>>>(lo, n, bucket_thr, ntiles, hbits, heads_fl,
                                              tail_ends, counts, view(p, c), n_dev);
  } else {
    k_runs_scan<<<kRunRows, 256, 0, s>>>(counts, ntiles, n, bucket_thr, heads_fl, tail_ends,
                                            p.lists.rc);
    k_runs_write<false><<<ntiles, 256, 0, s>>>(lo, n, bucket_thr, ntiles, hbits, heads_fl,
                                               tail_ends, counts, view(p, c), nullptr);
  }
}

void launch_tail_local(const uint32_t* kin, const uint32_t* vin, uint32_t* kout, uint32_t* vout,
                       const uint32_t* dtot, int bits, int bucket_thr, const MergePlan& p,
                       const MergeCall& c, hipStream_t s) {
  k_tail_local<<<1u << kTailTopBits, 256, 0, s>>>(kin, vin, kout, vout, dtot, bits - kTailTopBits,
                                                   bucket_thr, view(p, c));
}

void launch_merge(const Rows& r, const uint32_t* key, uint32_t* slots, uint32_t lo, uint32_t hi,
                  float thr, int bucket_thr, const MergePlan& p, const MergeCall& c, Counters* ctr,
                  hipStream_t s, const uint32_t* n_dev, bool runs_ready) {
  if (hi <= lo) return;
  const uint32_t n = hi - lo;
  if (n_dev && (lo != 0 || n >= tail_merge_max(p))) return;  // (the caller checks)
  const Decider dc = make_decider(thr);
  if (!runs_ready) launch_runs(key, lo, n, bucket_thr, p, c, s, n_dev);
  // the merge phase of a multi-launch iteration is stamped as a whole too (KC_MERGE: the wall of
  // its concurrent classes, bench.py's roofline phases)
  const bool phase = c.kt.blk && (n >= tail_merge_max(p) || !project_device_n_ok(r.d));
  const MergeCall cm = phase ? c.with_kt(c.kt.with_phase(KC_MERGE)) : c;
  switch (r.d) {
    case 8: launch_groups<8>(r, slots, dc, p, cm, ctr, n, s); break;
    case 16: launch_groups<16>(r, slots, dc, p, cm, ctr, n, s); break;
    case 32: launch_groups<32>(r, slots, dc, p, cm, ctr, n, s); break;
    case 64: launch_groups<64>(r, slots, dc, p, cm, ctr, n, s); break;
    default: launch_groups_wide(r, slots, dc, p, cm, ctr, n, s);
  }
}


// Prints and clears the merge profile (diagnostics build only; a no-op otherwise).
void merge_prof_dump(FILE* f) {
#ifdef KLSH_MERGE_PROF
  unsigned long long h[8][12];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_mprof), sizeof(h)) != hipSuccess) return;
  const char* names[kBigClasses + 1] = {"big128", "big192", "big384", "big896", "huge"};
  for (int c = 0; c <= kBigClasses; ++c)
    if (h[c][0])
      fprintf(f, "[mprof] %-7s runs %8llu rows %10llu merges %9llu  load+tiles %9.3f ms  walk %9.3f ms"
                 "  (per run %7.2f + %7.2f us)  max run %8.2f us  max b %llu\n",
              names[c], h[c][0], h[c][1], h[c][2], h[c][3] * 1e-5, h[c][4] * 1e-5,
              h[c][3] * 1e-2 / h[c][0], h[c][4] * 1e-2 / h[c][0], h[c][5] * 1e-2, h[c][6]);
  for (int c = 0; c <= kBigClasses; ++c)
    if (h[c][0])
      fprintf(f, "[mprof] %-7s per run: loads %7.2f  +norms %7.2f  (cum) us;  walk loop %7.2f us\n",
              names[c], h[c][8] * 1e-2 / h[c][0], h[c][9] * 1e-2 / h[c][0], h[c][10] * 1e-2 / h[c][0]);
  unsigned long long wpf[8][8];
  if (hipMemcpyFromSymbol(wpf, HIP_SYMBOL(g_wprof), sizeof(wpf)) == hipSuccess)
    for (int c = 0; c < kBigClasses; ++c)
      if (wpf[c][4])
        fprintf(f, "[wprof] %-7s steps %9llu  clocks/step: find|select %7.0f  select+consensus|consensus %7.0f"
                   "  dots %7.0f  bits %7.0f   find rounds/step|barrier clocks %.2f\n",
                names[c], wpf[c][4], (double)wpf[c][0] / wpf[c][4], (double)wpf[c][1] / wpf[c][4],
                (double)wpf[c][2] / wpf[c][4], (double)wpf[c][3] / wpf[c][4],
                (double)wpf[c][5] / wpf[c][4]);
  unsigned long long spf[8][8];
  if (hipMemcpyFromSymbol(spf, HIP_SYMBOL(g_sprof), sizeof(spf)) == hipSuccess)
    for (int c = 1; c < 6; ++c)
      if (spf[c][0])
        fprintf(f, "[sprof] G=%-2d batches %9llu  clocks/batch: stage %7.0f  pairwise %7.0f  walk %7.0f"
                   "  write %7.0f\n", 2 << c, spf[c][0], (double)spf[c][1] / spf[c][0],
                (double)spf[c][2] / spf[c][0], (double)spf[c][3] / spf[c][0], (double)spf[c][4] / spf[c][0]);
  unsigned long long g[8];
  if (hipMemcpyFromSymbol(g, HIP_SYMBOL(g_gprof), sizeof(g)) == hipSuccess && g[7])
    fprintf(f, "[gprof] tiles %llu (gram_tile)  clocks/tile: acc %.0f  decide %.0f;  slow-path tiles %llu:"
               " close pairs %llu (longest lane %.2f per slow tile), exact loop clocks/slow tile %.0f\n",
            g[7], (double)g[3] / g[7], (double)g[4] / g[7], g[0], g[1], (double)g[2] / g[0],
            (double)g[5] / g[0]);
  unsigned long long tq[8];
  if (hipMemcpyFromSymbol(tq, HIP_SYMBOL(g_tprof), sizeof(tq)) == hipSuccess && tq[4])
    fprintf(f, "[tprof] k_tail_local workgroups %llu  per workgroup us: base %.2f  counts %.2f  lists %.2f"
               "  scatter %.2f  (max total %.2f)\n", tq[4], tq[0] * 1e-2 / tq[4], tq[1] * 1e-2 / tq[4],
            tq[2] * 1e-2 / tq[4], tq[3] * 1e-2 / tq[4], tq[5] * 1e-2);
  unsigned long long z[8][12] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_tprof), z, sizeof(tq));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_gprof), z, sizeof(g));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_mprof), z, sizeof(z));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wprof), z, sizeof(unsigned long long) * 64);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_sprof), z, sizeof(unsigned long long) * 64);
#else
  (void)f;
#endif
}

}  // namespace klsh
