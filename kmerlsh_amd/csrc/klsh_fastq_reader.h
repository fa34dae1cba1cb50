// The host FASTQ reader of modes E and K (klsh_extract.cpp, which mode K reaches through
// klsh_fastq_next; klsh_fastq.cpp's test hook):
// FastqFile + the reference's kseq variant (utils/fastq.cc, kmer/kseq.h:153-200), the exact record
// rules, gzip or plain.  Host code over zlib alone: tests/cpp/fastq_reader_main.cpp links it
// without the HIP runtime.
//
// kmer/kseq.h:60-200 as the reference uses it: the name is the whole header line after '@'/'>'
// (up to '\n'); sequence characters are the isgraph() ones up to the next '>', '+' or '@'; the
// quality is the next seq.l characters in [33, 127] after the '+' line, plus one more character
// consumed; a record whose quality is short ends the file (-2).  Characters are read as signed
// chars, so a 0xFF byte reads as end of input where the reference compares with -1.
#pragma once
#include <stdint.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <vector>

namespace klsh {
namespace {  // (internal linkage, as when it was part of klsh_extract.cpp: see batch())

struct FastqReader {
  gzFile fp = nullptr;
  // a text in memory instead of a file (klsh_parse_fastq): delivered in blocks like a file's
  const char* mem = nullptr;
  uint64_t mem_len = 0, mem_pos = 0;
  std::vector<char> buf;
  int begin = 0, end = 0;
  bool is_eof = false;
  int last_char = 0;
  bool done = false;

  // batch storage (reader-owned; valid until the next batch)
  std::vector<char> seq, name, qual;
  std::vector<uint64_t> seq_off, name_off, qual_off;

  bool open(const char* path) {
    fp = gzopen(path, "r");
    if (!fp) return false;
    (void)gzbuffer(fp, 1 << 20);
    buf.resize(1 << 20);
    return true;
  }
  // a plain (not compressed) file from byte `offset` on, a record boundary: last_char == 0 and
  // the byte at `offset` the next one read
  bool open_at(const char* path, uint64_t offset) {
    if (!open(path)) return false;
    if (offset == 0) return true;
    (void)gzdirect(fp);  // looks at the header: a plain file then seeks instead of reading up to it
    return gzseek(fp, (z_off_t)offset, SEEK_SET) == (z_off_t)offset;
  }
  void open_memory(const char* text, uint64_t len, size_t block = 1 << 20) {
    mem = text;
    mem_len = len;
    mem_pos = 0;
    buf.resize(block ? block : 1);
  }
  ~FastqReader() {
    if (fp) gzclose(fp);
  }
  // the offset, from where the reader was opened, of the next byte getc() would return
  // (a memory text only: a file's position is gztell's)
  uint64_t tell() const { return mem_pos - (uint64_t)(end - begin); }
  __attribute__((noinline)) int read_memory() {
    const int n = (int)std::min<uint64_t>(buf.size(), mem_len - mem_pos);
    if (n > 0) memcpy(buf.data(), mem + mem_pos, (size_t)n);
    mem_pos += (uint64_t)n;
    return n;
  }
  bool fill() {
    if (is_eof) return false;
    begin = 0;
    end = mem ? read_memory() : gzread(fp, buf.data(), (unsigned)buf.size());
    if (end < (int)buf.size()) is_eof = true;  // a short read is the end (ks_getc)
    if (end < 0) end = 0;
    return end > 0;
  }
  // (Everything below is inlined into batch(), as it was inside klsh_extract.cpp; the struct has
  // internal linkage for that.  With external linkage the compiler keeps getc() out of line, a call
  // per byte.)
  int getc() {  // ks_getc, kseq.h:60-68
    if (is_eof && begin >= end) return -1;
    if (begin >= end && !fill()) return -1;
    return (int)(signed char)buf[begin++];
  }
  // one record appended to the batch: >= 0 (its sequence length), -1 end, -2 truncated
  int next() {  // kseq_read, kseq.h:153-200
    int c;
    if (last_char == 0) {
      while ((c = getc()) != -1 && c != '>' && c != '@') {
      }
      if (c == -1) return -1;
      last_char = c;
    }
    // name: ks_getuntil(ks, '\n', ...) — -1 only when nothing is left
    if (begin >= end && is_eof) return -1;
    const size_t n0 = name.size(), s0 = seq.size(), q0 = qual.size();
    while (true) {
      if (begin >= end && !fill()) break;
      const char* b = buf.data() + begin;
      const void* nl = memchr(b, '\n', (size_t)(end - begin));
      const int stop = nl ? (int)((const char*)nl - buf.data()) : end;
      name.insert(name.end(), b, (const char*)buf.data() + stop);
      begin = stop + (nl ? 1 : 0);
      if (nl) break;
    }
    // (a header line ending at EOF would read a comment here: nothing is left to read)
    while ((c = getc()) != -1 && c != '>' && c != '+' && c != '@')
      if (c >= 33 && c <= 126) seq.push_back((char)c);  // isgraph in the C locale
    if (c == '>' || c == '@') last_char = c;
    const size_t sl = seq.size() - s0;
    if (c != '+') {  // no quality: the reference would copy a stale buffer; we keep it empty
      commit();
      return (int)sl;
    }
    while ((c = getc()) != -1 && c != '\n') {
    }
    if (c == -1) {
      rollback(n0, s0, q0);
      return -2;
    }
    size_t ql = 0;
    while ((c = getc()) != -1 && ql < sl)
      if (c >= 33 && c <= 127) {
        qual.push_back((char)c);
        ++ql;
      }
    last_char = 0;
    if (sl != ql) {
      rollback(n0, s0, q0);
      return -2;
    }
    commit();
    return (int)sl;
  }
  void commit() {
    seq_off.push_back(seq.size());
    name_off.push_back(name.size());
    qual_off.push_back(qual.size());
  }
  void rollback(size_t n0, size_t s0, size_t q0) {
    name.resize(n0);
    seq.resize(s0);
    qual.resize(q0);
  }
  // up to max_reads records (or until ~max_bases sequence bytes): FastqFile::read
  // (utils/fastq.cc:54-67) with larger parts — part boundaries change nothing downstream.
  // On a 64-byte boundary: next()'s byte loops are inlined here, and their speed moved with the
  // function's offset inside a cache line (mode K's parse of 2 x 10^6 reads: 660 ms at offset 0,
  // 725 ms at offset 16, which is where growth of the objects linked before this one had put it).
  __attribute__((aligned(64))) uint64_t batch(uint64_t max_reads, uint64_t max_bases) {
    seq.clear();
    name.clear();
    qual.clear();
    seq_off.assign(1, 0);
    name_off.assign(1, 0);
    qual_off.assign(1, 0);
    uint64_t n = 0;
    while (!done && n < max_reads && seq.size() < max_bases) {
      if (next() < 0) {
        done = true;  // -1 (end) and -2 (truncated record) both end the file (fastq.cc:59-66)
        break;
      }
      ++n;
    }
    return n;
  }
};

}  // namespace
}  // namespace klsh
