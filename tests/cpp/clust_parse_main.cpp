// Driver of the host parser of klsh_diff_ksets (kmerlsh_amd/csrc/klsh_clust_parse.h) for
// tests/test_clust_host.py: built with AddressSanitizer + UndefinedBehaviorSanitizer (make
// clust_parse), no HIP, nothing loaded into Python.
//   clust_parse_main <block_bytes> <keep_ids 0|1> <file>...
// parses each file in blocks of block_bytes and prints what it parsed:
//   file <path> lines <L> entries <E> range <0|1> irregular_at <offset or -1>
//   then, unless range, one line per text line: "<n>" and, with keep_ids, " <id>" per entry
// A missing file prints "file <path> unreadable".
#include <stdio.h>
#include <stdlib.h>

#include "klsh_clust_parse.h"

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: clust_parse_main <block_bytes> <keep_ids> <file>...\n");
    return 2;
  }
  const size_t block = (size_t)strtoull(argv[1], nullptr, 10);
  const bool keep_ids = atoi(argv[2]) != 0;
  for (int a = 3; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      printf("file %s unreadable\n", argv[a]);
      continue;
    }
    klsh::ClustParser ps;
    const bool ok = klsh::clust_parse_file(f, block, keep_ids, &ps);
    fclose(f);
    if (!ok) {
      printf("file %s unreadable\n", argv[a]);
      continue;
    }
    printf("file %s lines %llu entries %llu range %d irregular_at %lld\n", argv[a],
           (unsigned long long)ps.lines, (unsigned long long)ps.entries, ps.range ? 1 : 0,
           ps.grammar.at == klsh::kClustRegular ? -1ll : (long long)ps.grammar.at);
    if (ps.range) continue;
    if (ps.counts.size() != ps.lines || ps.off.size() != ps.lines + 1 ||
        (keep_ids && ps.ids.size() != ps.entries) || ps.off.back() != ps.entries) {
      printf("inconsistent sizes\n");
      return 1;
    }
    for (uint64_t c = 0; c < ps.lines; ++c) {
      printf("%llu", (unsigned long long)ps.counts[c]);
      if (keep_ids)
        for (uint64_t q = ps.off[c]; q < ps.off[c + 1]; ++q)
          printf(" %llu", (unsigned long long)ps.ids[q]);
      printf("\n");
    }
  }
  return 0;
}
