// The device FASTQ parser's host side (klsh_fastq.cpp), as modes E and K use it
// (klsh_extract.cpp, klsh_kcount.cpp): a plain file read chunk by chunk, every chunk starting at a
// record boundary, parsed by the kernels of klsh_fastq.hip into a ReadBatch.
#pragma once
#include "klsh_ctx.h"

namespace klsh {

// One chunk: its bytes in pinned memory and on the device, and what the kernels made of them.
struct FastqSlot {
  PinBuf<uint8_t> raw;  // the chunk as read from the file (FastqChunks; its host writes read it)
  DevBuf<uint8_t> txt;
  DevBuf<uint32_t> tile_nl, line_start, rec_sum;
  DevBuf<unsigned long long> hdr;
  PinBuf<unsigned long long> hhdr;
  PinBuf<uint32_t> hline;  // line_start on the host (want_lines): 4 n + 1 entries
  PinBuf<uint64_t> hoff;   // the batch's offsets on the host (want_off): n + 1 entries
  uint64_t cap_raw = 0, cap_txt = 0, cap_tiles = 0, cap_lines = 0, cap_rec = 0, cap_hline = 0,
           cap_hoff = 0;
  Event e[4];  // around the launches before and after the record count is known
  bool ready = false;

  // what the last parse found
  uint64_t len = 0;        // bytes parsed
  uint64_t n = 0;          // complete records (0 when irregular)
  uint64_t bases = 0;
  uint64_t consumed = 0;   // the end of the last complete record (0 when irregular)
  uint64_t irregular = ~0ull;  // the smallest irregular offset, all ones if none
  float kernel_ms = 0.0f;

  int init();
  // `len` bytes at `bytes` (host memory) uploaded and parsed; the sequences and offsets of the
  // complete records left in dst (seq, off), unless the chunk is irregular.  Returns after the
  // kernels ran: the fields above are set, hline / hoff filled where wanted.
  int parse(const uint8_t* bytes, uint64_t len, ReadBatch& dst, uint64_t seq_bytes, bool want_lines,
            bool want_off, hipStream_t s, uint32_t grid_cap);
};

// A file's chunks in turn, into two slots.
class FastqChunks {
 public:
  explicit FastqChunks(klsh_ctx* ctx) : ctx_(ctx) {}
  ~FastqChunks();
  FastqChunks(const FastqChunks&) = delete;
  FastqChunks& operator=(const FastqChunks&) = delete;
  // The counters of option "fastq_*" cleared (a call's first file) — they describe a whole call.
  static void begin_call(klsh_ctx* ctx);
  // Opens `path`; *device = whether its chunks go to the device (option "fastq_parse" is not 1,
  // and the file does not begin with the gzip magic).  A file the device does not take has
  // taken over at offset 0.
  int open(const char* path, bool* device);
  // The chunk at offset() read into slot si and parsed into dst.  *n > 0: that many records, and
  // offset() has moved behind them.  *n == 0: the end of the file (*eof), or the host reader takes
  // over at offset().  With option "fastq_parse" 2 a takeover is KLSH_E_ARG.
  int next(int si, ReadBatch& dst, bool want_lines, bool want_off, uint64_t* n, bool* eof);
  uint64_t offset() const { return off_; }
  void host_reads(uint64_t n) { ctx_->fastq.host_reads += n; }
  FastqSlot slot[2];

 private:
  klsh_ctx* ctx_;
  int fd_ = -1;
  uint64_t off_ = 0, size_ = 0, chunk_ = 0;
  std::string path_;
};

}  // namespace klsh
