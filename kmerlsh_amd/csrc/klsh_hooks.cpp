// Test hooks behind the C ABI (include/klsh.h): single steps of the loop on caller data, and the
// per-slot state the result does not show.
#include <string.h>

#include <algorithm>
#include <array>

#include "klsh_loop.h"

using klsh::Counters;
using klsh::DevBuf;
using klsh::Rows;

extern "C" {

// The per-slot state klsh_result does not show, for the live rows in its order: plain copies of
// the device arrays and a host gather (read-only; on a context of a comm group, this rank's
// replica).
int klsh_row_state(klsh_ctx* ctx, float* nrm, uint32_t* cnt, uint16_t* image,
                   uint64_t* pad_nonzero, uint64_t* bad_links) {
  if (!ctx) return fail(KLSH_E_ARG, "null ctx");
  if (!ctx->loaded) return fail(KLSH_E_STATE, "nothing loaded");
  KLSH_HIP(hipSetDevice(ctx->device));
  KLSH_HIP(hipStreamSynchronize(ctx->stream));  // (a load's image build may still be in flight)
  const uint64_t n = ctx->n_live, S = ctx->slots, M = ctx->members;
  const int d = ctx->d, dp = ctx->dp;
  std::vector<uint32_t> ord(n);
  if (n) KLSH_HIP(hipMemcpy(ord.data(), ctx->order, 4 * n, hipMemcpyDeviceToHost));
  for (uint32_t sl : ord)
    if (sl >= S) return fail(KLSH_E_STATE, "corrupt live order");
  if (nrm && n) {
    std::vector<float> a(S);
    KLSH_HIP(hipMemcpy(a.data(), ctx->rows.nrm, 4 * S, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; ++i) nrm[i] = a[ord[i]];
  }
  std::vector<uint32_t> c(S);
  if (S) KLSH_HIP(hipMemcpy(c.data(), ctx->rows.cnt, 4 * S, hipMemcpyDeviceToHost));
  if (cnt)
    for (uint64_t i = 0; i < n; ++i) cnt[i] = c[ord[i]];
  if (image && n && ctx->rows.xh) {
    std::vector<uint16_t> a(S * (uint64_t)dp);
    KLSH_HIP(hipMemcpy(a.data(), ctx->rows.xh, 2 * a.size(), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; ++i)
      memcpy(image + i * d, a.data() + (uint64_t)ord[i] * dp, 2 * (size_t)d);
  }
  if (pad_nonzero) {
    uint64_t bad = 0;
    if (n && dp > d) {
      std::vector<uint32_t> a(S * (uint64_t)dp);
      KLSH_HIP(hipMemcpy(a.data(), ctx->rows.x, 4 * a.size(), hipMemcpyDeviceToHost));
      for (uint64_t i = 0; i < n; ++i)
        for (int k = d; k < dp; ++k) bad += a[(uint64_t)ord[i] * dp + k] != 0u;
    }
    *pad_nonzero = bad;
  }
  if (bad_links) {
    std::vector<uint32_t> head(S), tail(S), nxt(M);
    if (S) {
      KLSH_HIP(hipMemcpy(head.data(), ctx->rows.head, 4 * S, hipMemcpyDeviceToHost));
      KLSH_HIP(hipMemcpy(tail.data(), ctx->rows.tail, 4 * S, hipMemcpyDeviceToHost));
    }
    if (M) KLSH_HIP(hipMemcpy(nxt.data(), ctx->rows.nxt, 4 * M, hipMemcpyDeviceToHost));
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n; ++i) {
      // exactly cnt nodes from head, the last of them tail (an empty list: head == tail == nil)
      const uint32_t want = c[ord[i]];
      uint32_t node = head[ord[i]], last = klsh::kNil, len = 0;
      while (node != klsh::kNil && node < M && len <= want) {
        last = node;
        node = nxt[node];
        ++len;
      }
      bad += !(node == klsh::kNil && len == want && last == tail[ord[i]]);
    }
    *bad_links = bad;
  }
  return 0;
}

// The projection kernels the loop uses, on caller rows: the same dispatch (launch_project) with
// the context's projection options, the fp16 row image built from the rows where the loop keeps
// one (d = 16, 32, 64), so the certified screens and their exact fix-up paths are what a test of
// this entry point exercises.
int klsh_hash_keys(klsh_ctx* ctx, const float* rows, uint64_t n, int d, const float* table, int h,
                   uint32_t* keys) {
  if (!ctx || (!rows && n) || (!keys && n) || (!table && h > 0)) return fail(KLSH_E_ARG, "null argument");
  if (d <= 0 || d > 4096 || h < 0 || h > 31) return fail(KLSH_E_RANGE, "d or h out of range");
  if (n >= 0xFFFFFFF0ull) return fail(KLSH_E_RANGE, "rows >= 2^32");
  ctx->last_hash_kernel = klsh::kPkNone;
  ctx->last_hash_variant = klsh::kPvNone;
  ctx->last_hash_close = 0;
  if (n == 0) return 0;
  KLSH_HIP(hipSetDevice(ctx->device));
  const int dp = (d + 3) & ~3;
  Rows r{};
  r.d = d;
  r.dp = dp;
  DevBuf<float> x, W;
  DevBuf<uint32_t> slots, dkeys, ws;
  DevBuf<uint2> fix;
  DevBuf<uint16_t> xh;
  int e = 0;
  const bool image = ctx->shadow_wanted(d);
  if ((e = dalloc(x, n * dp)) || (e = dalloc(slots, n)) || (e = dalloc(dkeys, n)) ||
      (e = dalloc(W, (uint64_t)std::max(h, 1) * dp)) || (e = dalloc(fix, n)) ||
      (e = dalloc(ws, 64)) || (image && (e = dalloc(xh, n * dp))))
    return e;
  // the context's launch options over fresh workspaces
  const klsh::ProjectPlan pp = ctx->pp.over(fix, ws, (uint32_t)n);
  r.x = x;
  r.xh = xh;
  hipStream_t s = ctx->stream;
  std::vector<uint32_t> iota(n);
  for (uint64_t i = 0; i < n; ++i) iota[i] = (uint32_t)i;
  int rc = 0;
  if (hipMemsetAsync(r.x, 0, sizeof(float) * n * dp, s) != hipSuccess ||
      hipMemcpy2DAsync(r.x, 4 * dp, rows, 4 * d, 4 * d, n, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemsetAsync(W, 0, sizeof(float) * std::max(h, 1) * dp, s) != hipSuccess ||
      hipMemsetAsync(pp.v.ws, 0, sizeof(uint32_t) * 64, s) != hipSuccess ||
      (h > 0 && hipMemcpy2DAsync(W, 4 * dp, table, 4 * d, 4 * d, h, hipMemcpyHostToDevice, s) !=
                    hipSuccess) ||
      hipMemcpyAsync(slots, iota.data(), 4 * n, hipMemcpyHostToDevice, s) != hipSuccess) {
    rc = fail(KLSH_E_HIP, "upload");
  } else {
    if (image) klsh::launch_shadow_build(r, n, s);
    int variant = klsh::kPvNone;
    const int kern = klsh::launch_project(r, slots, dkeys, (uint32_t)n, W, h, 0u, s, &pp,
                                          klsh::kNoTime, &variant);
    uint32_t w[64];
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(keys, dkeys, 4 * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(w, pp.v.ws, sizeof(w), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
      rc = fail(KLSH_E_HIP, "projection");
    } else {
      ctx->last_hash_kernel = kern;
      ctx->last_hash_variant = variant;
      ctx->last_hash_close = klsh::proj_close_pairs(w);
    }
  }
  (void)hipStreamSynchronize(s);
  return rc;
}

int klsh_bucket_sort(klsh_ctx* ctx, const uint32_t* keys, uint64_t n, int bits,
                     uint32_t* sorted_keys, uint32_t* perm) {
  if (!ctx || (n && (!keys || !sorted_keys || !perm))) return fail(KLSH_E_ARG, "null argument");
  if (bits < 0 || bits > 32) return fail(KLSH_E_RANGE, "bits out of range");
  if (n >= 0xFFFFFFF0ull) return fail(KLSH_E_RANGE, "keys >= 2^32");
  if (n == 0) return 0;
  KLSH_HIP(hipSetDevice(ctx->device));
  DevBuf<uint32_t> k0, v0, k1, v1, ws, ts;
  DevBuf<Counters> ctr;
  const uint64_t ts_words = klsh::scan_ws_words(n);
  int e = 0;
  if ((e = dalloc(k0, n)) || (e = dalloc(v0, n)) || (e = dalloc(k1, n)) || (e = dalloc(v1, n)) ||
      (e = dalloc(ws, klsh::sort_ws_words(n))) || (e = dalloc(ts, ts_words)) || (e = dalloc(ctr, 1)))
    return e;
  hipStream_t s = ctx->stream;
  std::vector<uint32_t> iota(n);
  for (uint64_t i = 0; i < n; ++i) iota[i] = (uint32_t)i;
  Counters hc{};
  int rc = 0;
  uint32_t *ok = nullptr, *ov = nullptr;
  if (hipMemsetAsync(ws, 0, sizeof(uint32_t) * klsh::sort_ws_words(n), s) != hipSuccess ||
      hipMemsetAsync(ts, 0, sizeof(uint32_t) * ts_words, s) != hipSuccess ||
      hipMemsetAsync(ctr, 0, sizeof(Counters), s) != hipSuccess ||
      hipMemcpyAsync(k0, keys, 4 * n, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(v0, iota.data(), 4 * n, hipMemcpyHostToDevice, s) != hipSuccess) {
    rc = fail(KLSH_E_HIP, "upload");
  } else {
    klsh::radix_sort(k0, v0, k1, v1, (uint32_t)n, bits, ws, &ok, &ov, s);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(sorted_keys, ok, 4 * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(perm, ov, 4 * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(&hc, ctr, sizeof(Counters), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      rc = fail(KLSH_E_HIP, "sort");
    else if (hc.err)
      rc = fail(KLSH_E_HIP, "device protocol failure in the sort");
  }
  (void)hipStreamSynchronize(s);
  return rc;
}

// The run lists of one hook call: the lists with the context's own capacities for s positions
// (klsh_ctx::alloc), the run workspace and the counters (the caller zeroes them), and the read-back.
struct HookRuns {
  DevBuf<uint32_t> run_ws;
  DevBuf<klsh::RunCounters> rc;
  DevBuf<uint2> huge, over, cls[klsh::kGroupClasses], big[klsh::kBigClasses];
  klsh::MergePlan plan{};  // the lists of this call, no options
  klsh::RunCounters hc{};

  int alloc(uint64_t s) {
    using klsh::kBigClasses;
    using klsh::kGroupClasses;
    int e = 0;
    if ((e = dalloc(rc, 1)) || (e = dalloc(run_ws, klsh::run_ws_words(s))) ||
        (e = dalloc(huge, s / 897 + 64)) || (e = dalloc(over, s + 64)))
      return e;
    for (int c = 0; c < kGroupClasses && !e; ++c) e = dalloc(cls[c], klsh::group_class_capacity(c, s));
    for (int c = 0; c < kBigClasses && !e; ++c)
      e = dalloc(big[c], s / ((c ? klsh::kBigRows[c - 1] : 64) + 1) + 64);
    if (e) return e;
    plan.run_ws = run_ws;
    klsh::RunLists& w = plan.lists;
    w.huge = huge;
    w.over = over;
    for (int c = 0; c < kGroupClasses; ++c) w.cls[c] = cls[c];
    for (int c = 0; c < kBigClasses; ++c) w.big[c] = big[c];
    w.rc = rc;
    return 0;
  }

  // After the listing kernels, on a drained stream: the counters into hc, then every run as
  // (start, length, list) in start order into the caller's arrays (each may be null).  *n_runs:
  // in, their capacity; out, the run count.
  int read_back(uint64_t* n_runs, uint32_t* starts, uint32_t* lengths, int32_t* lists) {
    using klsh::kBigClasses;
    using klsh::kGroupClasses;
    const uint64_t cap = *n_runs;
    *n_runs = 0;
    if (hipMemcpy(&hc, rc, sizeof(hc), hipMemcpyDeviceToHost) != hipSuccess)
      return fail(KLSH_E_HIP, "run counters");
    std::vector<std::array<uint32_t, 3>> runs;
    auto take = [&](const uint2* list, uint32_t count, int l) -> int {
      std::vector<uint2> h(count);
      if (count && hipMemcpy(h.data(), list, sizeof(uint2) * count, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(KLSH_E_HIP, "list copy");
      for (const uint2& x : h) runs.push_back({x.x, x.y, (uint32_t)l});
      return 0;
    };
    const klsh::RunLists& w = plan.lists;
    int e = 0;
    for (int c = 0; c < kGroupClasses && !e; ++c) e = take(w.cls[c], hc.n_cls[c].v, c);
    for (int c = 0; c < kBigClasses && !e; ++c) e = take(w.big[c], hc.n_big[c].v, kGroupClasses + c);
    if (!e) e = take(w.huge, hc.n_huge.v, klsh::kRunListCount - 2);
    if (!e) e = take(w.over, hc.n_over.v, klsh::kRunListCount - 1);
    if (e) return e;
    std::sort(runs.begin(), runs.end());
    *n_runs = runs.size();
    if (runs.size() > cap) return fail(KLSH_E_RANGE, "more runs than the output holds (see *n_runs)");
    for (size_t i = 0; i < runs.size(); ++i) {
      if (starts) starts[i] = runs[i][0];
      if (lengths) lengths[i] = runs[i][1];
      if (lists) lists[i] = (int32_t)runs[i][2];
    }
    return 0;
  }
};

// The run finding of merge_main alone on caller keys (a test hook): every run of 2+ equal keys
// of n sorted keys with its list, in start order.
int klsh_bucket_runs(klsh_ctx* ctx, const uint32_t* sorted_keys, uint64_t n, int bucket_thr,
                     uint64_t* n_runs, uint32_t* starts, uint32_t* lengths, int32_t* lists) {
  if (!ctx || !n_runs || (n && !sorted_keys)) return fail(KLSH_E_ARG, "null argument");
  if (n >= 0xFFFFFFF0ull) return fail(KLSH_E_RANGE, "keys >= 2^32");
  if (n == 0) {
    *n_runs = 0;
    return 0;
  }
  KLSH_HIP(hipSetDevice(ctx->device));
  DevBuf<uint32_t> dk;
  HookRuns hr;
  int e = 0;
  if ((e = dalloc(dk, n)) || (e = hr.alloc(n))) return e;
  hipStream_t s = ctx->stream;
  int rc_ = 0;
  if (hipMemsetAsync(hr.rc, 0, sizeof(klsh::RunCounters), s) != hipSuccess ||
      hipMemcpyAsync(dk, sorted_keys, 4 * n, hipMemcpyHostToDevice, s) != hipSuccess) {
    rc_ = fail(KLSH_E_HIP, "upload");
  } else {
    klsh::launch_runs(dk, 0, (uint32_t)n, bucket_thr, hr.plan, klsh::MergeCall{}, s);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      rc_ = fail(KLSH_E_HIP, "run finding");
  }
  (void)hipStreamSynchronize(s);
  if (rc_) {
    *n_runs = 0;
    return rc_;
  }
  return hr.read_back(n_runs, starts, lengths, lists);
}

// One queued iteration's sort and run listing as run_batched's enqueue launches them (a test
// hook): grids for n_max, the count n_live in device memory, every workspace dirty.
int klsh_tail_buckets(klsh_ctx* ctx, const uint32_t* keys, uint64_t n_max, uint64_t n_live,
                      int bits, int bucket_thr, int path, uint32_t* out_keys, uint32_t* out_perm,
                      uint64_t* n_runs, uint32_t* starts, uint32_t* lengths, int32_t* lists,
                      uint32_t* counters) {
  if (!ctx || !n_runs || !keys || !out_keys || !out_perm) return fail(KLSH_E_ARG, "null argument");
  if (n_live < 1 || n_live > n_max || n_max >= (1ull << 20))
    return fail(KLSH_E_RANGE, "need 1 <= n_live <= n_max < 2^20");
  if (bits < 0 || bits > 19) return fail(KLSH_E_RANGE, "bits out of range");
  if (path != 0 && path != 1) return fail(KLSH_E_RANGE, "path must be 0 or 1");
  if (path == 1 && !klsh::tail_local_ok((uint32_t)n_max, bits))
    return fail(KLSH_E_RANGE, "the local path takes keys of 10..19 bits");
  KLSH_HIP(hipSetDevice(ctx->device));
  const uint64_t n = n_max, ws_words = klsh::sort_ws_words(n);
  DevBuf<uint32_t> k0, v0, k1, v1, ws, n_dev;
  HookRuns hr;
  int e = 0;
  if ((e = dalloc(k0, n)) || (e = dalloc(v0, n)) || (e = dalloc(k1, n)) || (e = dalloc(v1, n)) ||
      (e = dalloc(ws, ws_words)) || (e = dalloc(n_dev, 1)) || (e = hr.alloc(n)))
    return e;
  hipStream_t s = ctx->stream;
  std::vector<uint32_t> iota(n);
  for (uint64_t i = 0; i < n; ++i) iota[i] = (uint32_t)i;
  int rc_ = 0;
  // everything a kernel may read before it wrote it is 0xA5, as after some other iteration; only
  // the run counters start at zero (each compaction's publisher leaves them so)
  if (hipMemsetAsync(ws, 0xA5, 4 * ws_words, s) != hipSuccess ||
      hipMemsetAsync(hr.run_ws, 0xA5, 4 * klsh::run_ws_words(n), s) != hipSuccess ||
      hipMemsetAsync(k1, 0xA5, 4 * n, s) != hipSuccess ||
      hipMemsetAsync(v1, 0xA5, 4 * n, s) != hipSuccess ||
      hipMemsetAsync(hr.rc, 0, sizeof(klsh::RunCounters), s) != hipSuccess ||
      hipMemsetD32Async(n_dev, (int)(uint32_t)n_live, 1, s) != hipSuccess ||
      hipMemcpyAsync(k0, keys, 4 * n, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(v0, iota.data(), 4 * n, hipMemcpyHostToDevice, s) != hipSuccess) {
    rc_ = fail(KLSH_E_HIP, "upload");
  } else {
    uint32_t *fk = nullptr, *fv = nullptr;
    const klsh::MergeCall call{};
    if (path == 1) {  // (k0, v0) -> (k1, v1) by the top bits, back into (k0, v0) by the low ones
      const uint32_t* dtot = klsh::radix_sort_top(k0, v0, k1, v1, (uint32_t)n, bits, ws, s,
                                                  klsh::kNoTime, n_dev);
      klsh::launch_tail_local(k1, v1, k0, v0, dtot, bits, bucket_thr, hr.plan, call, s);
      fk = k0;
      fv = v0;
    } else {
      klsh::radix_sort(k0, v0, k1, v1, (uint32_t)n, bits, ws, &fk, &fv, s, klsh::kNoTime, n_dev);
      klsh::launch_runs(fk, 0, (uint32_t)n, bucket_thr, hr.plan, call, s, n_dev);
    }
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(out_keys, fk, 4 * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(out_perm, fv, 4 * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      rc_ = fail(KLSH_E_HIP, "tail sort and run listing");
  }
  (void)hipStreamSynchronize(s);
  if (rc_) {
    *n_runs = 0;
    return rc_;
  }
  if (int e2 = hr.read_back(n_runs, starts, lengths, lists)) return e2;
  if (counters) {
    const klsh::RunCounters& c = hr.hc;
    counters[0] = c.n_seg.v;
    counters[1] = c.n_small_rows.v;
    for (int b = 0; b < klsh::kBigClasses; ++b) counters[2 + b] = c.n_big_rows[b].v;
    counters[2 + klsh::kBigClasses] = c.n_huge_rows.v;
  }
  return 0;
}

int klsh_pcluster(klsh_ctx* ctx, float thr) {
  if (!ctx) return fail(KLSH_E_ARG, "null ctx");
  if (!ctx->loaded) return fail(KLSH_E_STATE, "nothing loaded");
  KLSH_HIP(hipSetDevice(ctx->device));
  const uint32_t n = (uint32_t)ctx->n_live;
  if (n == 0) return 0;
  hipStream_t s = ctx->stream;
  if (int e = ctx->reset_counters()) return e;
  ctx->mp.no_counts();
  KLSH_HIP(hipMemsetAsync(ctx->keys, 0, 4ull * n, s));  // one bucket: every key equal
  uint64_t dummy = 0;
  if (int e = klsh::merge_and_compact(ctx, ctx->keys, ctx->order, n, thr, -1, 0, &dummy, nullptr,
                                      false))
    return e;
  KLSH_HIP(hipStreamSynchronize(s));  // see klsh_cluster: the order may still be in flight
  return 0;
}

int klsh_hyperplanes(uint32_t seed_base, uint64_t* rng_counter, int h, int d, float* table) {
  if (!rng_counter || (!table && h > 0) || d <= 0 || h < 0) return fail(KLSH_E_ARG, "bad argument");
  klsh_host_hyperplanes(seed_base, *rng_counter, (uint64_t)h, d, d, table, 1);
  *rng_counter += (uint64_t)h;
  return 0;
}

int klsh_fp_selftest(klsh_ctx* ctx, const float* a, const float* b, uint64_t n, float* sqrt_out,
                     float* div_out) {
  if (!ctx || !a || !b || !sqrt_out || !div_out) return fail(KLSH_E_ARG, "null argument");
  if (n == 0) return 0;
  KLSH_HIP(hipSetDevice(ctx->device));
  DevBuf<float> da, db, ds, dd;
  int e = 0;
  if ((e = dalloc(da, n)) || (e = dalloc(db, n)) || (e = dalloc(ds, n)) || (e = dalloc(dd, n))) return e;
  hipStream_t s = ctx->stream;
  int rc = 0;
  if (hipMemcpyAsync(da, a, 4 * n, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(db, b, 4 * n, hipMemcpyHostToDevice, s) != hipSuccess) {
    rc = fail(KLSH_E_HIP, "upload");
  } else {
    klsh::launch_fp_selftest(da, db, (uint32_t)n, ds, dd, s);
    if (hipMemcpyAsync(sqrt_out, ds, 4 * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(div_out, dd, 4 * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      rc = fail(KLSH_E_HIP, "selftest");
  }
  (void)hipStreamSynchronize(s);
  return rc;
}

}  // extern "C"
