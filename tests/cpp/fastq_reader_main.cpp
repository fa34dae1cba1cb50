// Driver of the host FASTQ reader of modes E and K (kmerlsh_amd/csrc/klsh_fastq_reader.h) for
// tests/test_fastq_reader_host.py: built with AddressSanitizer + UndefinedBehaviorSanitizer (make
// fastq_reader), zlib and no HIP, nothing loaded into Python.
//   fastq_reader_main <batch_reads> <file> <offset> [<file> <offset>]...
// opens each file at the byte offset (a record boundary: the reader starts as it does at a
// file's first byte), reads it in batches of batch_reads records and prints
//   file <path> offset <offset>
//   one line per record: "<name> <sequence> <quality>", each field in hex ("-" when empty)
//   records <n>
// A file that cannot be opened prints "file <path> unreadable".
#include <stdio.h>
#include <stdlib.h>

#include "klsh_fastq_reader.h"

static void hex(const char* p, uint64_t n) {
  if (n == 0) fputc('-', stdout);
  for (uint64_t i = 0; i < n; ++i) printf("%02x", (unsigned)(unsigned char)p[i]);
}

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 2) % 2 != 0) {
    fprintf(stderr, "usage: fastq_reader_main <batch_reads> <file> <offset> [<file> <offset>]...\n");
    return 2;
  }
  const uint64_t per = strtoull(argv[1], nullptr, 10);
  for (int a = 2; a + 1 < argc; a += 2) {
    const uint64_t offset = strtoull(argv[a + 1], nullptr, 10);
    klsh::FastqReader r;
    if (!r.open_at(argv[a], offset)) {
      printf("file %s unreadable\n", argv[a]);
      continue;
    }
    printf("file %s offset %llu\n", argv[a], (unsigned long long)offset);
    uint64_t total = 0;
    while (true) {
      const uint64_t n = r.batch(per ? per : 1, ~0ull);
      if (n == 0) break;
      if (r.seq_off.size() != n + 1 || r.name_off.size() != n + 1 || r.qual_off.size() != n + 1) {
        printf("inconsistent sizes\n");
        return 1;
      }
      for (uint64_t i = 0; i < n; ++i) {
        hex(r.name.data() + r.name_off[i], r.name_off[i + 1] - r.name_off[i]);
        fputc(' ', stdout);
        hex(r.seq.data() + r.seq_off[i], r.seq_off[i + 1] - r.seq_off[i]);
        fputc(' ', stdout);
        hex(r.qual.data() + r.qual_off[i], r.qual_off[i + 1] - r.qual_off[i]);
        fputc('\n', stdout);
      }
      total += n;
    }
    printf("records %llu\n", (unsigned long long)total);
  }
  return 0;
}
