// klsh_diff_ksets / klsh_parse_clust behind the C ABI (include/klsh.h): the first
// half of mode E (reference app/kmerLSH.cc:541-585, IOMat::ReadClusterAll io/ioMatrix.cc:48-119,
// AB::WRS) from the cluster files to the two differential k-mer sets.
//
// The text goes up whole through two pinned buffers and is parsed by the kernels of klsh_diff.hip
// when it is regular, by the host's strtol code (klsh_clust_parse.h) otherwise — the whole file
// then: nothing the kernels produced is used.  The declared counts come back for klsh_wrs, which
// stays on the host; meanwhile the ids are emitted and kmer_set.hex streams up.  The groups go
// back as one byte per cluster, the ids mark the rows of each set, a count pass sizes the two
// tables, and the marked rows' images are claimed into them: no id list and no k-mer list crosses
// the bus twice.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <sys/stat.h>

#include <algorithm>
#include <functional>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "klsh_clust_parse.h"
#include "klsh_ctx.h"

namespace {

using klsh::DevBuf;
using klsh::PinBuf;

constexpr uint64_t kChunkDefault = 64ull << 20;
constexpr size_t kHostBlock = 1u << 20;  // the host parser's file blocks

// HIP-event time of the launches between begin() and end(), summed over the pairs of a call.
class Spans {
 public:
  int begin(hipStream_t s) {
    pairs_.emplace_back(new Pair());
    KLSH_HIP(pairs_.back()->a.create());
    KLSH_HIP(pairs_.back()->b.create());
    KLSH_HIP(hipEventRecord(pairs_.back()->a, s));
    return KLSH_OK;
  }
  int end(hipStream_t s) {
    KLSH_HIP(hipGetLastError());
    KLSH_HIP(hipEventRecord(pairs_.back()->b, s));
    return KLSH_OK;
  }
  double ms() const {  // (the stream is synchronized)
    double t = 0.0;
    for (const auto& p : pairs_) t += klsh::elapsed(p->a, p->b);
    return t;
  }

 private:
  struct Pair {
    klsh::Event a, b;
  };
  std::vector<std::unique_ptr<Pair>> pairs_;
};

// `bytes` bytes from read(dst, n) (which returns what it got) to dev, in chunks through two pinned
// buffers: the read of chunk c + 1 runs beside the copy of chunk c.
class Uploader {
 public:
  Uploader(hipStream_t s, uint64_t chunk) : s_(s), chunk_(chunk ? chunk : kChunkDefault) {}
  ~Uploader() { (void)hipStreamSynchronize(s_); }  // no copy out of the pinned buffers stays queued
  int send(uint64_t bytes, uint8_t* dev, const std::function<size_t(void*, size_t)>& read,
           double* read_ms, const char* what) {
    const uint64_t need = std::min(chunk_, bytes);
    if (need > cap_) {
      KLSH_HIP(hipStreamSynchronize(s_));
      for (auto& b : buf_) {
        if (!b.done) {
          b.done.reset(new klsh::Event());
          KLSH_HIP(b.done->create(hipEventDisableTiming));
        }
        if (b.host.alloc(need) != hipSuccess)
          return fail(KLSH_E_NOMEM, "hipHostMalloc of " + std::to_string(need) + " bytes");
        b.used = false;
      }
      cap_ = need;
    }
    for (uint64_t at = 0, c = 0; at < bytes; at += chunk_, ++c) {
      Buf& b = buf_[c & 1];
      const uint64_t n = std::min(chunk_, bytes - at);
      if (b.used) KLSH_HIP(hipEventSynchronize(*b.done));  // its last copy has left the buffer
      const double t0 = now_ms();
      const size_t got = read(b.host.get(), (size_t)n);
      *read_ms += now_ms() - t0;
      if (got != n) return fail(KLSH_E_ARG, std::string(what) + ": short read");
      KLSH_HIP(hipMemcpyAsync(dev + at, b.host.get(), n, hipMemcpyHostToDevice, s_));
      KLSH_HIP(hipEventRecord(*b.done, s_));
      b.used = true;
    }
    return KLSH_OK;
  }

 private:
  struct Buf {
    PinBuf<uint8_t> host;
    std::unique_ptr<klsh::Event> done;
    bool used = false;
  } buf_[2];
  hipStream_t s_;
  uint64_t chunk_, cap_ = 0;
};

// What a parse leaves on the device for the marks: the lines' offsets and the entries' ids.
struct Parsed {
  uint64_t len = 0, lines = 0, tokens = 0, entries = 0;
  uint64_t irregular_at = klsh::kClustRegular;
  bool range = false;  // entries >= 2^32: nothing below is allocated
  int path = 0;        // 0 kernels, 1 host
  // device path
  DevBuf<uint8_t> txt;
  DevBuf<uint32_t> tile_nl, tile_ts, line_tok0;
  DevBuf<uint64_t> tok_val, cnt, csum;
  DevBuf<unsigned long long> hdr;
  // both paths
  DevBuf<uint32_t> off;
  DevBuf<uint64_t> ids;
  // host path
  klsh::ClustParser host;
};

int read_hdr(Parsed& p, unsigned long long (&h)[klsh::kDiffHdrWords], hipStream_t s) {
  KLSH_HIP(hipMemcpyAsync(h, p.hdr, sizeof(h), hipMemcpyDeviceToHost, s));
  KLSH_HIP(hipStreamSynchronize(s));
  return KLSH_OK;
}

// Device path, first half: the text (len < 2^32 bytes, from `read`) up, its grammar checked, its
// tokens, lines and declared counts found.  Stops after the grammar check on an irregular text
// (irregular_at set), after the count sum on one that declares 2^32 entries or more (range set).
int device_counts(klsh_ctx* ctx, Parsed& p, uint64_t len,
                  const std::function<size_t(void*, size_t)>& read, Uploader& up, Spans& spans,
                  double* read_ms) {
  hipStream_t s = ctx->stream;
  const uint32_t cap = ctx->grid_cap;
  p.len = len;
  p.path = 0;
  const uint64_t alloc = klsh::diff_text_alloc(len), ntiles = klsh::diff_tiles(len);
  if (int e = dalloc(p.txt, alloc)) return e;
  if (int e = dalloc(p.tile_nl, ntiles)) return e;
  if (int e = dalloc(p.tile_ts, ntiles)) return e;
  if (int e = dalloc(p.hdr, klsh::kDiffHdrWords)) return e;
  KLSH_HIP(hipMemsetAsync(p.txt.get() + len, '\n', alloc - len, s));
  KLSH_HIP(hipMemsetAsync(p.hdr, 0, 8 * klsh::kDiffHdrWords, s));
  KLSH_HIP(hipMemsetAsync(p.hdr, 0xFF, 8, s));  // hdr[kDiffIrregular]
  if (int e = up.send(len, p.txt, read, read_ms, "cluster text")) return e;
  unsigned long long h[klsh::kDiffHdrWords];
  if (int e = spans.begin(s)) return e;
  klsh::launch_diff_scan(p.txt, (uint32_t)len, p.tile_nl, p.tile_ts, p.hdr, s, cap);
  if (int e = spans.end(s)) return e;
  if (int e = read_hdr(p, h, s)) return e;
  p.irregular_at = h[klsh::kDiffIrregular];
  if (p.irregular_at != klsh::kClustRegular) return KLSH_OK;
  p.lines = h[klsh::kDiffLines];
  p.tokens = h[klsh::kDiffTokens];
  if (p.lines == 0) return KLSH_OK;  // (the empty text)
  const uint64_t ltiles = klsh::diff_line_tiles(p.lines);
  if (int e = dalloc(p.tok_val, p.tokens)) return e;
  if (int e = dalloc(p.line_tok0, p.lines + 1)) return e;
  if (int e = dalloc(p.cnt, p.lines)) return e;
  if (int e = dalloc(p.csum, ltiles + 1)) return e;
  if (int e = spans.begin(s)) return e;
  klsh::launch_diff_tokens(p.txt, (uint32_t)len, p.tile_nl, p.tile_ts, (uint32_t)p.lines,
                           (uint32_t)p.tokens, p.tok_val, p.line_tok0, s, cap);
  klsh::launch_diff_counts(p.tok_val, p.line_tok0, (uint32_t)p.lines, p.cnt, p.csum, p.hdr, s, cap);
  if (int e = spans.end(s)) return e;
  if (int e = read_hdr(p, h, s)) return e;
  p.entries = h[klsh::kDiffEntries];
  p.range = p.entries >= klsh::kClustMaxEntries;
  if (p.range) p.entries = klsh::kClustMaxEntries;
  return KLSH_OK;
}

// Device path, second half (queued, not waited for): the offsets, and the ids if wanted.
int device_ids(klsh_ctx* ctx, Parsed& p, bool want_ids, Spans& spans) {
  hipStream_t s = ctx->stream;
  const uint32_t cap = ctx->grid_cap;
  if (p.lines == 0) return KLSH_OK;
  if (int e = dalloc(p.off, p.lines + 1)) return e;
  if (want_ids)
    if (int e = dalloc(p.ids, p.entries)) return e;
  if (int e = spans.begin(s)) return e;
  klsh::launch_diff_offsets(p.cnt, p.csum, (uint32_t)p.lines, p.off, s, cap);
  if (want_ids)
    klsh::launch_diff_ids(p.tok_val, p.line_tok0, p.off, (uint32_t)p.lines, (uint32_t)p.entries,
                          p.ids, s, cap);
  return spans.end(s);
}

// Host path: the parser's result (fed by the caller) checked; `range` as on the device path.
void host_parsed(Parsed& p) {
  p.path = 1;
  p.lines = p.host.lines;
  p.range = p.host.range;
  p.entries = p.range ? klsh::kClustMaxEntries : p.host.entries;
  p.irregular_at = p.host.grammar.at;
}

// Host path: offsets and ids to the device, for the marks.
int host_upload(klsh_ctx* ctx, Parsed& p) {
  hipStream_t s = ctx->stream;
  if (p.lines == 0) return KLSH_OK;
  std::vector<uint32_t> off32(p.host.off.begin(), p.host.off.end());  // (entries < 2^32)
  if (int e = dalloc(p.off, p.lines + 1)) return e;
  if (int e = dalloc(p.ids, p.entries)) return e;
  KLSH_HIP(hipMemcpyAsync(p.off, off32.data(), 4 * (p.lines + 1), hipMemcpyHostToDevice, s));
  if (p.entries)
    KLSH_HIP(hipMemcpyAsync(p.ids, p.host.ids.data(), 8 * p.entries, hipMemcpyHostToDevice, s));
  KLSH_HIP(hipStreamSynchronize(s));  // (off32 leaves scope)
  return KLSH_OK;
}

uint64_t kset_capacity(uint64_t n) {  // klsh_kset_create's rule
  uint64_t cap = 1024;
  while (cap < 2 * n) cap <<= 1;
  return cap;
}

struct DiffArgs {
  const char* clust_path;
  const char* kmer_set_path;
  uint64_t kmap;
  int n1, n2;
  float pval;
  int size_thresh;
};

int diff_run(klsh_ctx* ctx, const DiffArgs& a, FILE* ftext, uint64_t text_len, FILE* fk,
             const std::vector<float>& values, uint64_t line_cnt, const std::string& text_path,
             std::unique_ptr<klsh_kset>& sa, std::unique_ptr<klsh_kset>& sb, klsh_diff_stats& st) {
  hipStream_t s = ctx->stream;
  const uint32_t cap = ctx->grid_cap;
  // (declared first, released last: the uploader's destructor waits for every copy queued on them)
  std::vector<uint64_t> counts_dev;
  std::vector<uint8_t> grp;
  Spans parse, select;
  Uploader up(s, ctx->diff.chunk_bytes);
  Parsed p;
  st.text_bytes = text_len;
  auto read_text = [&](void* dst, size_t n) { return fread(dst, 1, n, ftext); };
  bool host = text_len >= (1ull << 32);
  if (!host) {
    if (int e = device_counts(ctx, p, text_len, read_text, up, parse, &st.read_ms)) return e;
    host = p.irregular_at != klsh::kClustRegular;
  }
  if (host) {  // the whole file again, through the reference's own parse
    p = Parsed();
    p.len = text_len;
    const double t0 = now_ms();
    try {
      if (!klsh::clust_parse_file(ftext, kHostBlock, true, &p.host))
        return fail(KLSH_E_ARG, text_path + ": read failed");
    } catch (const std::bad_alloc&) {
      return fail(KLSH_E_NOMEM, text_path + ": the declared member counts do not fit host memory");
    }
    st.read_ms += now_ms() - t0;
    host_parsed(p);
  }
  st.parse_path = (uint64_t)p.path;
  st.clusters = p.lines;
  st.tokens = p.tokens;
  st.entries = p.entries;
  if (p.range)
    return fail(KLSH_E_RANGE, text_path + ": the declared member counts sum to 2^32 or more");
  if (p.lines >= (1ull << 32)) return fail(KLSH_E_RANGE, text_path + ": 2^32 clusters or more");
  if (p.lines != line_cnt) {
    char msg[96];
    snprintf(msg, sizeof(msg), " has %llu clusters, ", (unsigned long long)p.lines);
    return fail(KLSH_E_ARG, text_path + msg + a.clust_path + " " + std::to_string(line_cnt) +
                                " rows (the reference requires equal)");
  }

  // the declared counts to the host; the ids (device path) queued behind them
  const uint64_t* counts = nullptr;
  if (p.path == 0) {
    counts_dev.resize(p.lines);
    if (p.lines)
      KLSH_HIP(hipMemcpyAsync(counts_dev.data(), p.cnt, 8 * p.lines, hipMemcpyDeviceToHost, s));
    klsh::Event got;
    KLSH_HIP(got.create(hipEventDisableTiming));
    KLSH_HIP(hipEventRecord(got, s));
    if (int e = device_ids(ctx, p, true, parse)) return e;
    KLSH_HIP(hipEventSynchronize(got));
    counts = counts_dev.data();
  } else {
    if (int e = host_upload(ctx, p)) return e;
    counts = p.host.counts.data();
  }

  // kmer_set.hex streams up behind the ids while the host tests the clusters
  DevBuf<uint64_t> kmers;
  DevBuf<uint8_t> mark_a, mark_b, group;
  if (int e = dalloc(kmers, a.kmap)) return e;
  if (int e = dalloc(mark_a, a.kmap)) return e;
  if (int e = dalloc(mark_b, a.kmap)) return e;
  if (int e = dalloc(group, p.lines)) return e;
  if (a.kmap) {
    KLSH_HIP(hipMemsetAsync(mark_a, 0, a.kmap, s));
    KLSH_HIP(hipMemsetAsync(mark_b, 0, a.kmap, s));
  }
  if (p.path == 1) {
    if (int e = dalloc(p.hdr, klsh::kDiffHdrWords)) return e;
    KLSH_HIP(hipMemsetAsync(p.hdr, 0, 8 * klsh::kDiffHdrWords, s));
  }
  const double tw = now_ms();
  grp.resize(p.lines ? p.lines : 1);
  if (int e = klsh_wrs(values.data(), p.lines, a.n1, a.n2, counts, a.pval, a.size_thresh, grp.data()))
    return e;
  for (uint64_t c = 0; c < p.lines; ++c) {
    st.tested += counts[c] > (uint64_t)(int64_t)a.size_thresh ? 1u : 0u;
    st.clusters_a += grp[c] == 1 ? 1u : 0u;
    st.clusters_b += grp[c] == 2 ? 1u : 0u;
  }
  st.wrs_ms = now_ms() - tw;
  auto read_kmers = [&](void* dst, size_t n) { return fread(dst, 1, n, fk); };
  if (int e = up.send(8 * a.kmap, reinterpret_cast<uint8_t*>(kmers.get()), read_kmers, &st.read_ms,
                      a.kmer_set_path))
    return e;

  // the marks, their counts, the two tables
  if (p.lines) KLSH_HIP(hipMemcpyAsync(group, grp.data(), p.lines, hipMemcpyHostToDevice, s));
  if (int e = select.begin(s)) return e;
  klsh::launch_diff_mark(p.off, (uint32_t)p.lines, p.ids, (uint32_t)p.entries, group, a.kmap, mark_a,
                         mark_b, s, cap);
  klsh::launch_diff_count(mark_a, mark_b, a.kmap, p.hdr, s, cap);
  if (int e = select.end(s)) return e;
  unsigned long long h[klsh::kDiffHdrWords];
  if (int e = read_hdr(p, h, s)) return e;
  st.ids_a = h[klsh::kDiffIdsA];
  st.ids_b = h[klsh::kDiffIdsB];
  st.kmers_a = h[klsh::kDiffKmersA];
  st.kmers_b = h[klsh::kDiffKmersB];
  for (auto* ks : {&sa, &sb}) {
    const uint64_t n = ks == &sa ? st.kmers_a : st.kmers_b, slots = kset_capacity(n);
    ks->reset(new klsh_kset());
    (*ks)->ctx = ctx;
    (*ks)->mask = slots - 1;
    (*ks)->n = n;
    if (int e = dalloc((*ks)->tab, slots)) return e;
    KLSH_HIP(hipMemsetAsync((*ks)->tab, 0xFF, 8 * slots, s));
  }
  if (int e = select.begin(s)) return e;
  klsh::launch_diff_insert(kmers, mark_a, mark_b, a.kmap, sa->tab, sa->mask, sb->tab, sb->mask, s, cap);
  if (int e = select.end(s)) return e;
  KLSH_HIP(hipStreamSynchronize(s));
  st.parse_ms = parse.ms();
  st.select_ms = select.ms();
  return KLSH_OK;
}

bool file_size(FILE* f, uint64_t* size) {
  struct stat sb;
  if (fstat(fileno(f), &sb) != 0 || !S_ISREG(sb.st_mode)) return false;
  *size = (uint64_t)sb.st_size;
  return true;
}

}  // namespace

extern "C" int klsh_diff_ksets(klsh_ctx* ctx, const char* clust_path, const char* kmer_set_path,
                               uint64_t kmap_size, int n1, int n2, float pvalue_thresh,
                               int size_thresh, klsh_kset** set_a, klsh_kset** set_b,
                               klsh_diff_stats* stats) {
  if (set_a) *set_a = nullptr;
  if (set_b) *set_b = nullptr;
  if (!ctx || !clust_path || !kmer_set_path || !set_a || !set_b)
    return fail(KLSH_E_ARG, "null argument");
  if (n1 < 0 || n2 < 0) return fail(KLSH_E_ARG, "n1 and n2 must be >= 0");
  if (stats && stats->struct_size != sizeof(klsh_diff_stats))
    return fail(KLSH_E_ARG, "klsh_diff_stats.struct_size != sizeof: built against another klsh.h");
  const double t_start = now_ms();
  klsh_diff_stats local{};
  local.struct_size = sizeof(local);
  const int d = n1 + n2;
  // the three files, before any device work
  const std::string text_path = std::string(clust_path) + ".clust";
  klsh::File fb(fopen(clust_path, "rb")), ft(fopen(text_path.c_str(), "rb")),
      fk(fopen(kmer_set_path, "rb"));
  uint64_t rows_bytes = 0, text_len = 0, kmer_bytes = 0;
  if (!fb || !file_size(fb.get(), &rows_bytes))
    return fail(KLSH_E_ARG, std::string("cannot read ") + clust_path);
  if (!ft || !file_size(ft.get(), &text_len)) return fail(KLSH_E_ARG, "cannot read " + text_path);
  if (!fk || !file_size(fk.get(), &kmer_bytes))
    return fail(KLSH_E_ARG, std::string("cannot read ") + kmer_set_path);
  if (kmap_size > kmer_bytes / 8)
    return fail(KLSH_E_ARG, std::string(kmer_set_path) + " holds fewer than kmap_size k-mers");
  const uint64_t line_cnt = d > 0 ? rows_bytes / (sizeof(float) * (uint64_t)d) : 0;
  std::vector<float> values;
  const double tr = now_ms();
  try {
    values.resize(line_cnt * (uint64_t)d);
  } catch (const std::bad_alloc&) {
    return fail(KLSH_E_NOMEM, std::string(clust_path) + " does not fit host memory");
  }
  if (line_cnt && fread(values.data(), sizeof(float) * (size_t)d, line_cnt, fb.get()) != line_cnt)
    return fail(KLSH_E_ARG, std::string("short read of ") + clust_path);
  fb.reset();
  local.read_ms += now_ms() - tr;

  KLSH_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<klsh_kset> sa, sb;
  const DiffArgs args{clust_path, kmer_set_path, kmap_size, n1, n2, pvalue_thresh, size_thresh};
  int rc;
  try {
    rc = diff_run(ctx, args, ft.get(), text_len, fk.get(), values, line_cnt, text_path, sa, sb, local);
  } catch (const std::bad_alloc&) {
    rc = fail(KLSH_E_NOMEM, "klsh_diff_ksets: host allocation failed");
  }
  (void)hipStreamSynchronize(ctx->stream);
  local.total_ms = now_ms() - t_start;
  if (stats) *stats = local;
  if (rc != KLSH_OK) return rc;  // (sa, sb: released here, both)
  *set_a = sa.release();
  *set_b = sb.release();
  return KLSH_OK;
}

extern "C" int klsh_parse_clust(klsh_ctx* ctx, const char* text, uint64_t len, int path,
                                uint64_t* n_lines, uint64_t* counts, uint64_t* offsets,
                                uint64_t* ids, uint64_t* n_ids, uint64_t* irregular_at,
                                int* path_used) {
  if (!ctx || (len && !text) || !n_lines || !n_ids || !irregular_at || !path_used)
    return fail(KLSH_E_ARG, "null argument");
  if (path < 0 || path > 2) return fail(KLSH_E_ARG, "path must be 0, 1 or 2");
  const bool query = !counts && !offsets && !ids;
  if (!query && (!counts || !offsets || (!ids && *n_ids)))
    return fail(KLSH_E_ARG, "counts, offsets and ids: all three or none");
  KLSH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  std::vector<uint32_t> off32;  // (before p: its buffers' release waits for the copies)
  Parsed p;
  Spans spans;
  double read_ms = 0.0;
  *irregular_at = klsh::kClustRegular;
  bool host = path == 1;
  if (!host) {
    if (len >= (1ull << 32)) {
      if (path == 2) return fail(KLSH_E_ARG, "a text of 2^32 bytes or more takes the host parser");
      host = true;
    } else {
      Uploader up(s, ctx->diff.chunk_bytes);
      uint64_t at = 0;
      auto read = [&](void* dst, size_t n) {
        memcpy(dst, text + at, n);
        at += n;
        return n;
      };
      if (int e = device_counts(ctx, p, len, read, up, spans, &read_ms)) return e;
      if (p.irregular_at != klsh::kClustRegular) {
        *irregular_at = p.irregular_at;
        if (path == 2)
          return fail(KLSH_E_ARG, "irregular text at byte " + std::to_string(p.irregular_at));
        host = true;
      }
    }
  }
  if (host) {
    p = Parsed();
    p.len = len;
    try {
      (void)klsh::clust_parse_mem(text, (size_t)len, !query, &p.host);
    } catch (const std::bad_alloc&) {
      return fail(KLSH_E_NOMEM, "klsh_parse_clust: the declared member counts do not fit host memory");
    }
    host_parsed(p);
    *irregular_at = p.irregular_at;
  }
  *path_used = p.path;
  *n_lines = p.lines;
  const uint64_t capacity = *n_ids;
  *n_ids = p.entries;
  if (p.range) return fail(KLSH_E_RANGE, "the declared member counts sum to 2^32 or more");
  if (query) return KLSH_OK;
  if (p.entries > capacity) return fail(KLSH_E_RANGE, "ids: capacity too small");
  if (p.path == 1) {
    std::copy(p.host.counts.begin(), p.host.counts.end(), counts);
    std::copy(p.host.off.begin(), p.host.off.end(), offsets);
    std::copy(p.host.ids.begin(), p.host.ids.end(), ids);
    return KLSH_OK;
  }
  offsets[0] = 0;
  if (p.lines == 0) return KLSH_OK;
  if (int e = device_ids(ctx, p, true, spans)) return e;
  off32.resize(p.lines + 1);
  KLSH_HIP(hipMemcpyAsync(counts, p.cnt, 8 * p.lines, hipMemcpyDeviceToHost, s));
  KLSH_HIP(hipMemcpyAsync(off32.data(), p.off, 4 * (p.lines + 1), hipMemcpyDeviceToHost, s));
  if (p.entries) KLSH_HIP(hipMemcpyAsync(ids, p.ids, 8 * p.entries, hipMemcpyDeviceToHost, s));
  KLSH_HIP(hipStreamSynchronize(s));
  std::copy(off32.begin(), off32.end(), offsets);
  return KLSH_OK;
}
