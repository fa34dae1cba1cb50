// The device FASTQ parser behind modes E and K: a plain file read chunk by chunk
// with positioned reads into pinned memory, every chunk starting at a record boundary and parsed
// by the kernels of klsh_fastq.hip; and its test hook klsh_parse_fastq (include/klsh.h).
//
// A chunk's complete records are everything up to the newline that ends its last line 4r + 3; the
// next chunk starts right after it (the partial record is read again, nothing is carried).  Where
// those records hold an irregularity, or the chunk holds no complete record, the host reader
// (klsh_fastq_reader.h) takes over at the chunk's offset and keeps the rest of the file.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <string>
#include <vector>

#include "klsh_fastq_dev.h"
#include "klsh_fastq_reader.h"

namespace klsh {

namespace {

constexpr uint64_t kChunkBytes = 64ull << 20;

// a buffer of `want` elements at least: replaced (with a quarter of headroom) when it is smaller
template <class Buf>
int ensure(Buf& b, uint64_t& cap, uint64_t want) {
  if (want <= cap) return KLSH_OK;
  cap = 0;
  const uint64_t c = want + want / 4;
  if (b.alloc(c) != hipSuccess)
    return fail(KLSH_E_NOMEM, "fastq parser: a buffer of " + std::to_string(c) + " elements");
  cap = c;
  return KLSH_OK;
}

}  // namespace

int FastqSlot::init() {
  if (ready) return KLSH_OK;
  for (auto& ev : e) KLSH_HIP(ev.create());
  KLSH_HIP(hdr.alloc(kFqHdrWords));
  KLSH_HIP(hhdr.alloc(kFqHdrWords));
  ready = true;
  return KLSH_OK;
}

int FastqSlot::parse(const uint8_t* bytes, uint64_t len_, ReadBatch& dst, uint64_t seq_bytes,
                     bool want_lines, bool want_off, hipStream_t s, uint32_t grid_cap) {
  len = len_;
  n = bases = consumed = 0;
  irregular = ~0ull;
  kernel_ms = 0.0f;
  if (len >= (1ull << 32)) return set_error(KLSH_E_RANGE, "fastq parser: a chunk of 2^32 bytes or more");
  if (int rc = init()) return rc;
  if (int rc = ensure(txt, cap_txt, fq_text_alloc(len))) return rc;
  if (int rc = ensure(tile_nl, cap_tiles, fq_tiles(len) + 1)) return rc;
  if (len) KLSH_HIP(hipMemcpyAsync(txt, bytes, len, hipMemcpyHostToDevice, s));
  KLSH_HIP(hipMemsetAsync(hdr, 0, kFqHdrWords * 8, s));
  KLSH_HIP(hipMemsetAsync(hdr, 0xFF, 8, s));  // hdr[kFqIrregular]
  KLSH_HIP(hipEventRecord(e[0], s));
  launch_fq_scan(txt, (uint32_t)len, tile_nl, hdr, s, grid_cap);
  KLSH_HIP(hipGetLastError());
  KLSH_HIP(hipEventRecord(e[1], s));
  KLSH_HIP(hipMemcpyAsync(hhdr, hdr, kFqHdrWords * 8, hipMemcpyDeviceToHost, s));
  KLSH_HIP(hipStreamSynchronize(s));
  kernel_ms = elapsed(e[0], e[1]);
  const uint64_t nr = hhdr[kFqRecords];
  if (nr == 0) return KLSH_OK;  // no complete record
  // now the record count sizes the rest; L1's bytes are fewer than the chunk's
  if (int rc = ensure(line_start, cap_lines, 4 * nr + 1)) return rc;
  if (int rc = ensure(rec_sum, cap_rec, fq_record_tiles(nr) + 1)) return rc;
  if (len + 64 > dst.cap_b) {
    dst.cap_b = 0;
    const uint64_t c = std::max<uint64_t>(seq_bytes, len + 64);
    KLSH_HIP(dst.seq.alloc(c));
    dst.cap_b = c;
  }
  if (nr + 1 > dst.cap_r) {
    dst.cap_r = 0;
    KLSH_HIP(dst.off.alloc(nr + 1 + nr / 4));
    dst.cap_r = nr + 1 + nr / 4;
  }
  if (want_lines)
    if (int rc = ensure(hline, cap_hline, 4 * nr + 1)) return rc;
  if (want_off)
    if (int rc = ensure(hoff, cap_hoff, nr + 1)) return rc;
  KLSH_HIP(hipEventRecord(e[2], s));
  launch_fq_lines(txt, (uint32_t)len, tile_nl, (uint32_t)nr, line_start, hdr, s, grid_cap);
  launch_fq_records(line_start, (uint32_t)nr, rec_sum, dst.off, hdr, s, grid_cap);
  launch_fq_pack(txt, (uint32_t)len, line_start, dst.off, (uint32_t)nr, hdr, dst.seq, dst.cap_b, s, grid_cap);
  KLSH_HIP(hipGetLastError());
  KLSH_HIP(hipEventRecord(e[3], s));
  KLSH_HIP(hipMemcpyAsync(hhdr, hdr, kFqHdrWords * 8, hipMemcpyDeviceToHost, s));
  if (want_lines)
    KLSH_HIP(hipMemcpyAsync(hline, line_start, (4 * nr + 1) * 4, hipMemcpyDeviceToHost, s));
  if (want_off) KLSH_HIP(hipMemcpyAsync(hoff, dst.off, (nr + 1) * 8, hipMemcpyDeviceToHost, s));
  KLSH_HIP(hipStreamSynchronize(s));
  kernel_ms += elapsed(e[2], e[3]);
  irregular = hhdr[kFqIrregular];
  if (irregular != ~0ull) return KLSH_OK;
  n = nr;
  bases = hhdr[kFqBases];
  consumed = hhdr[kFqConsumed];
  return KLSH_OK;
}

FastqChunks::~FastqChunks() {
  if (fd_ >= 0) (void)::close(fd_);
}

void FastqChunks::begin_call(klsh_ctx* ctx) {
  FastqHooks& h = ctx->fastq;
  h.device_chunks = h.device_reads = h.host_reads = 0;
  h.takeover_at = ~0ull;
  h.parse_ms = h.read_ms = 0.0;
}

int FastqChunks::open(const char* path, bool* device) {
  FastqHooks& h = ctx_->fastq;
  *device = false;
  path_ = path;
  off_ = 0;
  if (fd_ >= 0) (void)::close(fd_);
  fd_ = -1;
  // Only a regular file has a size and takes positioned reads; a FIFO, a terminal or a /proc-style
  // file is the host reader's from its first byte (it is not even opened here: opening and closing
  // a FIFO would end its writer).  So is a file whose first bytes cannot be read.
  const char* why = "is gzip";
  if (h.parse != 1) {
    struct stat sb;
    if (stat(path, &sb) != 0) return fail(KLSH_E_ARG, std::string("cannot open ") + path);
    if (!S_ISREG(sb.st_mode)) {
      why = "is not a regular file";
    } else {
      fd_ = ::open(path, O_RDONLY);
      if (fd_ < 0) return fail(KLSH_E_ARG, std::string("cannot open ") + path);
      size_ = (uint64_t)sb.st_size;
      uint8_t magic[2] = {0, 0};
      const ssize_t got = size_ ? pread(fd_, magic, 2, 0) : 0;
      if (got < 0) why = "cannot be read at an offset";
      else *device = !(got == 2 && magic[0] == 0x1f && magic[1] == 0x8b);
    }
  }
  chunk_ = h.chunk_bytes ? h.chunk_bytes : kChunkBytes;
  if (!*device) {
    h.takeover_at = 0;
    if (h.parse == 2)
      return fail(KLSH_E_ARG, "fastq_parse 2: " + path_ + " " + why + ", the host reader takes over at offset 0");
  }
  return KLSH_OK;
}

int FastqChunks::next(int si, ReadBatch& dst, bool want_lines, bool want_off, uint64_t* n, bool* eof) {
  FastqHooks& h = ctx_->fastq;
  FastqSlot& sl = slot[si];
  *n = 0;
  *eof = false;
  if (off_ >= size_) {
    *eof = true;
    return KLSH_OK;
  }
  uint64_t len = std::min<uint64_t>(chunk_, size_ - off_);
  const uint64_t most = std::min<uint64_t>(chunk_, size_);  // (of any chunk of this file)
  if (len > sl.cap_raw) {
    sl.cap_raw = 0;
    KLSH_HIP(sl.raw.alloc(most));
    sl.cap_raw = most;
  }
  uint64_t got = 0;
  const double t_read = now_ms();
  while (got < len) {
    const ssize_t r = pread(fd_, sl.raw.get() + got, (size_t)(len - got), (off_t)(off_ + got));
    if (r < 0) return fail(KLSH_E_ARG, "read failed: " + path_);
    if (r == 0) break;  // the file shrank: what is there is the file
    got += (uint64_t)r;
  }
  h.read_ms += now_ms() - t_read;
  if (got < len) size_ = off_ + got, len = got;
  if (len == 0) {
    *eof = true;
    return KLSH_OK;
  }
  if (int rc = sl.parse(sl.raw, len, dst, most + 64, want_lines, want_off, ctx_->stream, ctx_->grid_cap))
    return rc;
  h.parse_ms += sl.kernel_ms;
  if (sl.n == 0) {  // an irregularity, or no complete record: the host reader from here on
    h.takeover_at = off_;
    if (h.parse == 2)
      return fail(KLSH_E_ARG, "fastq_parse 2: " + path_ + ": the host reader would take over at offset " +
                                  std::to_string(off_));
    return KLSH_OK;
  }
  h.device_chunks += 1;
  h.device_reads += sl.n;
  off_ += sl.consumed;
  *n = sl.n;
  return KLSH_OK;
}

}  // namespace klsh

// Test hook (tests/test_gpu_fastq_parse.py): one chunk, held in host memory, through the kernels
// (path 0) or the host reader (path 1).
extern "C" int klsh_parse_fastq(klsh_ctx* ctx, const char* text, uint64_t len, int path,
                                uint64_t* n_records, uint32_t* line_starts, uint64_t* seq_off,
                                char* seq, uint64_t* seq_cap, uint64_t* consumed,
                                uint64_t* irregular_at) {
  if (!ctx || (len && !text) || !n_records || !seq_cap || !consumed || !irregular_at)
    return set_error(KLSH_E_ARG, "null argument");
  if (path != 0 && path != 1) return set_error(KLSH_E_ARG, "klsh_parse_fastq: path must be 0 or 1");
  if (len >= (1ull << 32)) return set_error(KLSH_E_RANGE, "klsh_parse_fastq: 2^32 bytes or more");
  const uint64_t room = *seq_cap;
  if (path == 1) {
    klsh::FastqReader r;
    r.open_memory(text, len);
    r.seq_off.assign(1, 0);
    r.name_off.assign(1, 0);
    r.qual_off.assign(1, 0);
    uint64_t n = 0, end = 0;
    while (r.next() >= 0) {
      ++n;
      end = r.tell() - (r.last_char ? 1u : 0u);  // (a header byte read ahead belongs to the next record)
    }
    *n_records = n;
    *consumed = end;
    *irregular_at = ~0ull;  // (the reader does not classify)
    *seq_cap = r.seq.size();
    if (seq && room < r.seq.size()) return set_error(KLSH_E_RANGE, "klsh_parse_fastq: seq too small");
    if (seq && !r.seq.empty()) memcpy(seq, r.seq.data(), r.seq.size());
    if (seq_off) memcpy(seq_off, r.seq_off.data(), (n + 1) * 8);
    if (line_starts) {  // the lines of the bytes it consumed, all ones where there are fewer
      uint64_t l = 0, pos = 0;
      line_starts[l++] = 0;
      while (l < 4 * n + 1) {
        const void* nl = pos < end ? memchr(text + pos, '\n', (size_t)(end - pos)) : nullptr;
        if (!nl) break;
        pos = (uint64_t)((const char*)nl - text) + 1;
        line_starts[l++] = (uint32_t)pos;
      }
      while (l < 4 * n + 1) line_starts[l++] = 0xFFFFFFFFu;
    }
    return KLSH_OK;
  }
  KLSH_HIP(hipSetDevice(ctx->device));
  const hipStream_t s = ctx->stream;
  klsh::ReadBatch dst;  // (first: freed after the slot, whose buffers nothing reads by then)
  klsh::FastqSlot sl;
  if (int rc = sl.parse(reinterpret_cast<const uint8_t*>(text), len, dst, len + 64, line_starts != nullptr,
                        seq_off != nullptr, s, ctx->grid_cap))
    return rc;
  *n_records = sl.n;
  *consumed = sl.consumed;
  *irregular_at = sl.irregular;
  *seq_cap = sl.bases;
  if (seq && room < sl.bases) return set_error(KLSH_E_RANGE, "klsh_parse_fastq: seq too small");
  if (sl.n == 0) {
    if (line_starts) line_starts[0] = 0;
    if (seq_off) seq_off[0] = 0;
    return KLSH_OK;
  }
  if (line_starts) memcpy(line_starts, sl.hline.get(), (4 * sl.n + 1) * 4);
  if (seq_off) memcpy(seq_off, sl.hoff.get(), (sl.n + 1) * 8);
  if (seq && sl.bases) {
    KLSH_HIP(hipMemcpyAsync(seq, dst.seq, sl.bases, hipMemcpyDeviceToHost, s));
    KLSH_HIP(hipStreamSynchronize(s));
  }
  return KLSH_OK;
}
