// Result extraction behind the C ABI (include/klsh.h): klsh_count, klsh_result,
// klsh_result_device, klsh_labels — through the host walk of the member lists, or through the
// kernels of klsh_result.hip.
#include <string.h>

#include <utility>

#include "klsh_ctx.h"

using klsh::device_result;

// ---- the result on the device ---------------------------------------------------
// The kernels of klsh_result.hip over the live order: d_off (n + 1 member offsets), d_nodes (the
// member lists as nodes, flat) and d_labels (the live row of each of the M nodes), all device
// memory, any may be null; *total_out (may be null) = the live rows' members.  Offsets alone
// need no workspace beyond the tile sums; nodes or labels take the list ranking's 2 x 8 B x M +
// 4 B x M, allocated here and freed before returning.  Ends with the stream synchronized.
// (klsh_save.cpp takes its lists from here too: declared in klsh_ctx.h)
int klsh::device_result(klsh_ctx* ctx, uint32_t* d_off, uint32_t* d_nodes, uint32_t* d_labels,
                        uint64_t* total_out) {
  const uint64_t n = ctx->n_live, M = ctx->members;
  const bool rank = (d_nodes || d_labels) && M;
  const uint32_t cap = ctx->grid_cap;
  hipStream_t s = ctx->stream;
  klsh::DevBuf<uint32_t> hdr, tsum, off_tmp, rowof;
  klsh::DevBuf<uint64_t> st0, st1;
  uint32_t h[klsh::kResHdrWords] = {};
  int rc = 0;
  do {
    const uint32_t ntiles = klsh::result_tiles(n);
    if ((rc = dalloc(hdr, klsh::kResHdrWords)) || (rc = dalloc(tsum, 2 * (size_t)ntiles))) break;
    if (!d_off && (rc = dalloc(off_tmp, n + 1))) break;
    if (rank && ((rc = dalloc(st0, M)) || (rc = dalloc(st1, M)) || (rc = dalloc(rowof, M)))) break;
    uint32_t* off = d_off ? d_off : off_tmp.get();
    if (hipMemsetAsync(hdr, 0, sizeof(h), s) != hipSuccess) {
      rc = fail(KLSH_E_HIP, "result header reset");
      break;
    }
    klsh::launch_result_offsets(ctx->order, ctx->rows.cnt, (uint32_t)n, (uint32_t)ctx->slots, tsum,
                                tsum + ntiles, off, hdr, s, cap);
    // the one small copy the host needs before the rounds: the total and the longest list
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
      rc = fail(KLSH_E_HIP, "result offsets");
      break;
    }
    if (h[klsh::kResErr] & klsh::kResErrOrder) {
      rc = fail(KLSH_E_STATE, "corrupt live order");
      break;
    }
    if (total_out) *total_out = h[klsh::kResTotal];
    if (h[klsh::kResTotal] > M) {  // (before anything is written at these offsets)
      rc = fail(KLSH_E_STATE, "corrupt member list");
      break;
    }
    if (!rank) break;
    uint32_t rounds = 0;  // ceil(log2(longest list)): fixed before the first round
    while ((1ull << rounds) < (uint64_t)h[klsh::kResMaxCnt]) ++rounds;
    ctx->result_rounds = rounds;
#ifdef KLSH_RESULT_SHORT_ROUNDS  // mutation build (tools/build_variant.sh)
    if (rounds) --rounds;
#endif
    klsh::launch_result_rowof(ctx->order, ctx->rows.cnt, ctx->rows.tail, (uint32_t)n,
                              (uint32_t)ctx->slots, (uint32_t)M, rowof, hdr, s, cap);
    // (HIP events around the rounds alone: read-only option "result_rank_us")
    const uint64_t* st = klsh::launch_list_rank(ctx->rows.nxt, (uint32_t)M, rounds, st0, st1, hdr,
                                                s, cap, ctx->ev[klsh::EV_RANK_BEGIN]);
    (void)hipEventRecord(ctx->ev[klsh::EV_RANK_END], s);
    klsh::launch_result_emit(st, rowof, ctx->order, ctx->rows.cnt, off, (uint32_t)M, (uint32_t)n,
                             (uint32_t)ctx->slots, d_labels, d_nodes, hdr, s, cap);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
      rc = fail(KLSH_E_HIP, "result list ranking");
      break;
    }
    float ms = 0.0f;
    ctx->result_rank_us = hipEventElapsedTime(&ms, ctx->ev[klsh::EV_RANK_BEGIN],
                                              ctx->ev[klsh::EV_RANK_END]) == hipSuccess
                              ? (int64_t)(ms * 1e3f)
                              : -1;
    // every member belongs to exactly one live row, at a place inside that row's list
    if (h[klsh::kResErr] || h[klsh::kResLabelled] != h[klsh::kResTotal])
      rc = fail(KLSH_E_STATE, "corrupt member list");
  } while (false);
  (void)hipStreamSynchronize(s);
  return rc;
}

extern "C" {

int klsh_count(klsh_ctx* ctx, uint64_t* n_rows, uint64_t* n_members) {
  if (!ctx) return fail(KLSH_E_ARG, "null ctx");
  if (!ctx->loaded) return fail(KLSH_E_STATE, "nothing loaded");
  if (n_rows) *n_rows = ctx->n_live;
  if (n_members && ctx->result_device) {  // the offsets scan's total: cnt stays on the device
    KLSH_HIP(hipSetDevice(ctx->device));
    return device_result(ctx, nullptr, nullptr, nullptr, n_members);
  }
  if (n_members) {
    KLSH_HIP(hipSetDevice(ctx->device));
    // members of live rows = sum of cnt over the live slots
    std::vector<uint32_t> ord(ctx->n_live), cnt(ctx->slots);
    if (ctx->n_live)
      KLSH_HIP(hipMemcpy(ord.data(), ctx->order, 4 * ctx->n_live, hipMemcpyDeviceToHost));
    if (ctx->slots)
      KLSH_HIP(hipMemcpy(cnt.data(), ctx->rows.cnt, 4 * ctx->slots, hipMemcpyDeviceToHost));
    uint64_t m = 0;
    for (uint32_t sl : ord) m += cnt[sl];
    *n_members = m;
  }
  return 0;
}

int klsh_result(klsh_ctx* ctx, float* rows, uint64_t* member_offsets, uint64_t* member_ids) {
  if (!ctx) return fail(KLSH_E_ARG, "null ctx");
  if (!ctx->loaded) return fail(KLSH_E_STATE, "nothing loaded");
  KLSH_HIP(hipSetDevice(ctx->device));
  const uint64_t n = ctx->n_live;
  hipStream_t s = ctx->stream;
  if (rows && n) {
    klsh::DevBuf<float> tmp;
    if (int e = dalloc(tmp, n * (uint64_t)ctx->d)) return e;
    klsh::launch_gather_rows(ctx->rows, ctx->order, (uint32_t)n, tmp, s);
    hipError_t e1 = hipMemcpyAsync(rows, tmp, sizeof(float) * n * ctx->d, hipMemcpyDeviceToHost, s);
    hipError_t e2 = hipStreamSynchronize(s);
    if (e1 != hipSuccess || e2 != hipSuccess) return fail(KLSH_E_HIP, "result rows copy");
  }
  if ((member_offsets || member_ids) && ctx->result_device) {
    // offsets and nodes from the kernels, then one streaming pass: member_ids[m] = ids[nodes[m]]
    const uint64_t M = ctx->members;
    klsh::DevBuf<uint32_t> d_off, d_nodes;
    int rc = 0;
    if ((rc = dalloc(d_off, n + 1)) || (member_ids && (rc = dalloc(d_nodes, M)))) return rc;
    uint64_t total = 0;
    std::vector<uint32_t> off(n + 1), nodes;
    if (!(rc = device_result(ctx, d_off, d_nodes, nullptr, &total))) {  // (total <= M)
      nodes.resize(member_ids ? total : 0);
      if (hipMemcpy(off.data(), d_off, 4 * (n + 1), hipMemcpyDeviceToHost) != hipSuccess ||
          (!nodes.empty() &&
           hipMemcpy(nodes.data(), d_nodes, 4 * total, hipMemcpyDeviceToHost) != hipSuccess))
        rc = fail(KLSH_E_HIP, "result lists copy");
    }
    if (rc) return rc;
    if (member_offsets)
      for (uint64_t i = 0; i <= n; ++i) member_offsets[i] = off[i];
    if (member_ids)
      for (uint64_t m = 0; m < total; ++m) {
        if (nodes[m] >= M) return fail(KLSH_E_STATE, "corrupt member list");
        member_ids[m] = ctx->ids[nodes[m]];
      }
    return 0;
  }
  if (member_offsets || member_ids) {
    std::vector<uint32_t> ord(n), head(ctx->slots), cnt(ctx->slots), nxt(ctx->members);
    if (n) KLSH_HIP(hipMemcpy(ord.data(), ctx->order, 4 * n, hipMemcpyDeviceToHost));
    if (ctx->slots) {
      KLSH_HIP(hipMemcpy(head.data(), ctx->rows.head, 4 * ctx->slots, hipMemcpyDeviceToHost));
      KLSH_HIP(hipMemcpy(cnt.data(), ctx->rows.cnt, 4 * ctx->slots, hipMemcpyDeviceToHost));
    }
    if (ctx->members)
      KLSH_HIP(hipMemcpy(nxt.data(), ctx->rows.nxt, 4 * ctx->members, hipMemcpyDeviceToHost));
    uint64_t m = 0;
    for (uint64_t i = 0; i < n; ++i) {
      if (member_offsets) member_offsets[i] = m;
      if (ord[i] >= ctx->slots) return fail(KLSH_E_STATE, "corrupt live order");
      // the caller sized member_ids by klsh_count, the sum of cnt (which may be below the node
      // count: nodes in no list): a row's walk past its own cnt would write past that buffer
      uint32_t left = cnt[ord[i]];
      for (uint32_t node = head[ord[i]]; node != klsh::kNil; node = nxt[node]) {
        // every member belongs to exactly one live row: a longer walk is a broken list
        if (node >= ctx->members || m >= ctx->members || left-- == 0)
          return fail(KLSH_E_STATE, "corrupt member list");
        if (member_ids) member_ids[m] = ctx->ids[node];
        ++m;
      }
    }
    if (member_offsets) member_offsets[n] = m;
  }
  return 0;
}

int klsh_result_device(klsh_ctx* ctx, float* d_rows, uint32_t* d_member_offsets,
                       uint32_t* d_member_nodes, uint32_t* d_labels) {
  if (!ctx) return fail(KLSH_E_ARG, "null ctx");
  if (!ctx->loaded) return fail(KLSH_E_STATE, "nothing loaded");
  KLSH_HIP(hipSetDevice(ctx->device));
  const std::pair<const void*, const char*> ptrs[] = {{d_rows, "d_rows"},
                                                      {d_member_offsets, "d_member_offsets"},
                                                      {d_member_nodes, "d_member_nodes"},
                                                      {d_labels, "d_labels"}};
  for (const auto& p : ptrs)
    if (p.first)
      if (int e = ctx->check_device_ptr(p.first, p.second)) return e;
  if (d_rows && ctx->n_live) {  // queued in front of the lists, complete at their last sync
    klsh::launch_gather_rows(ctx->rows, ctx->order, (uint32_t)ctx->n_live, d_rows, ctx->stream);
    KLSH_HIP(hipGetLastError());
  }
  if (d_member_offsets || d_member_nodes || d_labels)
    return device_result(ctx, d_member_offsets, d_member_nodes, d_labels, nullptr);
  KLSH_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int klsh_labels(klsh_ctx* ctx, uint32_t* labels) {
  if (!ctx) return fail(KLSH_E_ARG, "null ctx");
  if (!ctx->loaded) return fail(KLSH_E_STATE, "nothing loaded");
  if (!labels && ctx->members) return fail(KLSH_E_ARG, "null argument");
  KLSH_HIP(hipSetDevice(ctx->device));
  if (ctx->members == 0) return 0;
  klsh::DevBuf<uint32_t> d_labels;
  if (int e = dalloc(d_labels, ctx->members)) return e;
  int rc = device_result(ctx, nullptr, nullptr, d_labels, nullptr);
  if (!rc && hipMemcpy(labels, d_labels, 4 * ctx->members, hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(KLSH_E_HIP, "labels copy");
  return rc;
}

}  // extern "C"
