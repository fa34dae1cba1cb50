// klsh_save_clusters behind the C ABI (include/klsh.h): the reference's two cluster
// files (IOMat::SaveResult / SaveBinary, io/ioMatrix.cc:265-294, 322-351) from the device.
//
// The member lists come from the list ranking (klsh::device_result, klsh_result_host.cpp), the
// rows to write and the text's byte positions from the scans of klsh_save.hip.  Both files then
// leave in chunks through two device and two pinned buffers: while the host writes a chunk from
// one pinned buffer, the next is produced and copied into the other.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "klsh_ctx.h"
#include "klsh_save_plan.h"

namespace {

using klsh::DevBuf;
using klsh::PinBuf;

// The two buffer pairs and the chunk loop of one call.
class ChunkWriter {
 public:
  ChunkWriter(hipStream_t s, klsh_save_stats& st) : s_(s), st_(st) {}
  ~ChunkWriter() { (void)hipStreamSynchronize(s_); }  // no copy into the pinned buffers stays queued
  int init(uint64_t bytes) {
    for (auto& b : buf_) {
      KLSH_HIP(b.e0.create());
      KLSH_HIP(b.e1.create());
      KLSH_HIP(b.done.create());
      if (int e = dalloc(b.dev, bytes)) return e;
      if (b.host.alloc(bytes) != hipSuccess)
        return fail(KLSH_E_NOMEM, "hipHostMalloc of " + std::to_string(bytes) + " bytes");
    }
    return KLSH_OK;
  }

  // Chunks 0 .. nchunks - 1 to f: produce(c, dev) queues the kernels that fill dev with chunk c
  // and returns its bytes.
  template <class Produce>
  int stream(uint64_t nchunks, FILE* f, const std::string& path, uint64_t* total, Produce produce) {
    auto start = [&](uint64_t c) -> int {
      Buf& b = buf_[c & 1];
      KLSH_HIP(hipEventRecord(b.e0, s_));
      b.bytes = produce(c, b.dev.get());
      KLSH_HIP(hipGetLastError());
      KLSH_HIP(hipEventRecord(b.e1, s_));
      KLSH_HIP(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, s_));
      KLSH_HIP(hipEventRecord(b.done, s_));
      st_.chunks += 1;
      return KLSH_OK;
    };
    int rc = KLSH_OK;
    if (nchunks && (rc = start(0))) return rc;
    for (uint64_t c = 0; c < nchunks; ++c) {
      if (c + 1 < nchunks && (rc = start(c + 1))) return rc;
      Buf& b = buf_[c & 1];
      KLSH_HIP(hipEventSynchronize(b.done));
      st_.format_ms += klsh::elapsed(b.e0, b.e1);
      const double tw = now_ms();
      const bool ok = fwrite(b.host, 1, b.bytes, f) == b.bytes;
      st_.write_ms += now_ms() - tw;
      if (!ok) return fail(KLSH_E_ARG, path + ": write failed");
      *total += b.bytes;
    }
    return KLSH_OK;
  }

 private:
  struct Buf {
    DevBuf<uint8_t> dev;
    PinBuf<uint8_t> host;
    klsh::Event e0, e1, done;  // around the kernels; after the copy
    uint64_t bytes = 0;
  } buf_[2];
  hipStream_t s_;
  klsh_save_stats& st_;
};

// Everything after the argument and path checks.  *opened: a file of ours may exist.
int save_run(klsh_ctx* ctx, const char* clust_path, const char* bin_path, uint32_t ignore_small,
             klsh_save_stats& st, bool* opened) {
  const uint64_t n = ctx->n_live, M = ctx->members;
  const uint32_t cap = ctx->grid_cap;
  const int d = ctx->d;
  hipStream_t s = ctx->stream;
  klsh::SaveHooks& hooks = ctx->save;
  st.clusters = n;

  // 1. the lists: n + 1 offsets, the members as nodes (a hole would read as no node)
  DevBuf<uint32_t> d_off, d_nodes;
  if (int e = dalloc(d_off, n + 1)) return e;
  if (int e = dalloc(d_nodes, M)) return e;
  if (M) KLSH_HIP(hipMemsetAsync(d_nodes, 0xFF, 4 * M, s));
  uint64_t total = 0;
  const double tr = now_ms();
  if (int e = klsh::device_result(ctx, d_off, d_nodes, nullptr, &total)) return e;
  st.rank_ms = now_ms() - tr;  // (its workspace is freed: the buffers below take its place)

  // 2. the rows to keep; the text's positions
  const uint64_t ntiles = clust_path ? klsh::save_tiles(total) : 0;
  DevBuf<unsigned long long> hdr;
  DevBuf<uint32_t> tsum, kslot;
  DevBuf<uint64_t> d_ids, tpos;
  klsh::Event pre0, pre1;
  KLSH_HIP(pre0.create());
  KLSH_HIP(pre1.create());
  if (int e = dalloc(hdr, klsh::kSaveHdrWords)) return e;
  if (int e = dalloc(tsum, klsh::result_tiles(n))) return e;
  if (int e = dalloc(kslot, n)) return e;
  KLSH_HIP(hipMemsetAsync(hdr, 0, 8 * klsh::kSaveHdrWords, s));
  klsh::SaveText tx{d_off, d_nodes, nullptr, ctx->ids_base, (uint32_t)n, (uint32_t)total,
                    (uint32_t)M, ignore_small};
  if (clust_path && total && !ctx->ids_linear) {  // node -> id, once per call
    if (ctx->ids.size() < M) return fail(KLSH_E_STATE, "fewer ids than member nodes");
    if (int e = dalloc(d_ids, M)) return e;
    KLSH_HIP(hipMemcpyAsync(d_ids, ctx->ids.data(), 8 * M, hipMemcpyHostToDevice, s));
    tx.ids = d_ids;
    hooks.ids_uploaded = 1;
  }
  std::vector<uint64_t> h_tpos(ntiles + 1, hooks.offset_base);
  unsigned long long h[klsh::kSaveHdrWords] = {};
  KLSH_HIP(hipEventRecord(pre0, s));
  klsh::launch_save_keep(ctx->order, d_off, (uint32_t)n, ignore_small, tsum, kslot, hdr, s, cap);
  if (ntiles) {
    if (int e = dalloc(tpos, ntiles + 1)) return e;
    klsh::launch_save_positions(tx, hooks.offset_base, tpos, hdr, s, cap);
    KLSH_HIP(hipMemcpyAsync(h_tpos.data(), tpos, 8 * (ntiles + 1), hipMemcpyDeviceToHost, s));
  }
  KLSH_HIP(hipGetLastError());
  KLSH_HIP(hipEventRecord(pre1, s));
  KLSH_HIP(hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, s));
  KLSH_HIP(hipStreamSynchronize(s));
  st.format_ms += klsh::elapsed(pre0, pre1);
  if (h[klsh::kSaveErr]) return fail(KLSH_E_STATE, "corrupt member list");
  const uint64_t K = h[klsh::kSaveKept];
  const uint64_t L = h_tpos[ntiles] - hooks.offset_base;
  st.clusters_written = K;
  st.members_written = h[klsh::kSaveMembers];
  tsum.reset();

  // 3. the files
  *opened = true;
  klsh::File fc(clust_path ? fopen(clust_path, "wb") : nullptr);
  if (clust_path && !fc) return fail(KLSH_E_ARG, std::string("cannot write ") + clust_path);
  klsh::File fb(bin_path ? fopen(bin_path, "wb") : nullptr);
  if (bin_path && !fb) return fail(KLSH_E_ARG, std::string("cannot write ") + bin_path);
  int rc = KLSH_OK;
  if (K) {
    const uint64_t chunk = klsh::save_chunk_bytes(hooks.chunk_bytes);
    ChunkWriter w(s, st);
    if ((rc = w.init(klsh::save_buffer_bytes(chunk, L, bin_path ? K : 0, d)))) return rc;
    if (fc)
      rc = w.stream(klsh::save_text_chunks(L, chunk), fc.get(), clust_path, &st.text_bytes,
                    [&](uint64_t c, uint8_t* dev) {
                      const klsh::SaveWindow win = klsh::save_window(h_tpos.data(), ntiles, L, chunk, c);
                      klsh::launch_save_emit(tx, tpos, win.t_lo, win.t_hi, win.w0, win.w1, dev, s, cap);
                      return win.w1 - win.w0;
                    });
    if (rc == KLSH_OK && fb) {
      const uint64_t per = klsh::save_rows_per_chunk(chunk, d);
      rc = w.stream(klsh::save_bin_chunks(K, chunk, d), fb.get(), bin_path, &st.bin_bytes,
                    [&](uint64_t c, uint8_t* dev) {  // whole rows of the kept slots
                      const uint64_t r0 = c * per, m = std::min(per, K - r0);
                      klsh::launch_gather_rows(ctx->rows, kslot + r0, (uint32_t)m,
                                               reinterpret_cast<float*>(dev), s);
                      return m * sizeof(float) * (uint64_t)d;
                    });
    }
  }  // (the writer's destructor: nothing stays queued on the stream)
  const double tw = now_ms();
  if (fc && fclose(fc.release()) != 0 && rc == KLSH_OK)
    rc = fail(KLSH_E_ARG, std::string(clust_path) + ": write failed");
  if (fb && fclose(fb.release()) != 0 && rc == KLSH_OK)
    rc = fail(KLSH_E_ARG, std::string(bin_path) + ": write failed");
  st.write_ms += now_ms() - tw;
  return rc;
}

}  // namespace

extern "C" int klsh_save_clusters(klsh_ctx* ctx, const char* clust_path, const char* bin_path,
                                  int ignore_small, klsh_save_stats* stats) {
  if (!ctx) return fail(KLSH_E_ARG, "null ctx");
  if (!clust_path && !bin_path) return fail(KLSH_E_ARG, "neither file asked for");
  if (ignore_small < 0)
    return fail(KLSH_E_ARG, "ignore_small must be >= 0 (the reference's two writers disagree below)");
  if (stats && stats->struct_size != sizeof(klsh_save_stats))
    return fail(KLSH_E_ARG, "klsh_save_stats.struct_size != sizeof: built against another klsh.h");
  if (!ctx->loaded) return fail(KLSH_E_STATE, "nothing loaded");
  for (const char* path : {clust_path, bin_path})  // before any device work, nothing truncated
    if (path && !klsh::save_path_writable(path))
      return fail(KLSH_E_ARG, std::string("cannot write ") + path);
  const double t_start = now_ms();
  klsh_save_stats local{};
  local.struct_size = sizeof(local);
  ctx->save.chunks = 0;
  ctx->save.ids_uploaded = 0;
  KLSH_HIP(hipSetDevice(ctx->device));
  bool opened = false;
  const int rc = save_run(ctx, clust_path, bin_path, (uint32_t)ignore_small, local, &opened);
  (void)hipStreamSynchronize(ctx->stream);
  if (rc != KLSH_OK && opened) {
    const std::string msg = klsh_last_error();  // (kept across the removals)
    klsh::save_remove(clust_path);
    klsh::save_remove(bin_path);
    fail(rc, msg);
  }
  ctx->save.chunks = local.chunks;
  local.total_ms = now_ms() - t_start;
  if (stats) *stats = local;
  return rc;
}
