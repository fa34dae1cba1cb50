// The host-only pieces of klsh_save_clusters (kmerlsh_amd/csrc/klsh_save_plan.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer; tests/test_save_host.py builds and runs it.
//
//   paths DIR   the path probe: an existing file keeps its bytes, a new file does not stay, a
//               missing directory and a directory are refused; only regular files are removed
//   windows     the chunk rule over random texts: the windows partition the text, their tile
//               ranges hold every byte, and k_save_emit's store loop, replayed on the host over
//               save_clip's numbers into a buffer of exactly the window's bytes, writes each
//               byte once, in bounds, its 16-byte stores aligned
// Exit 0 = every check held (any sanitizer report aborts).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "klsh_save_plan.h"

#define REQUIRE(cond)                                                          \
  do {                                                                         \
    if (!(cond)) {                                                             \
      fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

static std::string slurp(const std::string& path) {
  std::string out;
  FILE* f = fopen(path.c_str(), "rb");
  REQUIRE(f);
  char buf[256];
  size_t k;
  while ((k = fread(buf, 1, sizeof(buf), f)) > 0) out.append(buf, k);
  fclose(f);
  return out;
}

static bool exists(const std::string& path) {
  struct stat st;
  return stat(path.c_str(), &st) == 0;
}

static int paths(const std::string& dir) {
  const std::string old = dir + "/old", fresh = dir + "/fresh", missing = dir + "/none/x";
  FILE* f = fopen(old.c_str(), "wb");
  REQUIRE(f && fwrite("keep me", 1, 7, f) == 7 && fclose(f) == 0);
  REQUIRE(klsh::save_path_writable(old.c_str()) && slurp(old) == "keep me");
  REQUIRE(klsh::save_path_writable(fresh.c_str()) && !exists(fresh));
  REQUIRE(!klsh::save_path_writable(missing.c_str()) && !exists(dir + "/none"));
  REQUIRE(!klsh::save_path_writable(dir.c_str()) && exists(dir));
  klsh::save_remove(dir.c_str());  // not a regular file: stays
  klsh::save_remove(nullptr);
  klsh::save_remove(missing.c_str());
  REQUIRE(exists(dir));
  klsh::save_remove(old.c_str());
  REQUIRE(!exists(old));
  printf("paths ok\n");
  return 0;
}

// one window replayed: what k_save_emit stores, with the kernel's loop bounds
static void emit_window(const std::vector<uint64_t>& tpos, const std::vector<uint8_t>& text,
                        const klsh::SaveWindow& w, std::vector<uint8_t>* all) {
  const uint64_t bytes = w.w1 - w.w0;
  // exactly the window's bytes, 16-byte aligned like the device buffer: ASan sees a store outside
  uint8_t* out = static_cast<uint8_t*>(aligned_alloc(16, (bytes + 15) / 16 * 16));
  REQUIRE(out);
  std::vector<uint8_t> hits(bytes, 0);
  for (uint64_t t = w.t_lo; t < w.t_hi; ++t) {
    const uint32_t tlen = (uint32_t)(tpos[t + 1] - tpos[t]);
    const klsh::SaveClip c = klsh::save_clip(tpos[t], tlen, w.w0, w.w1);
    if (c.A >= c.B) continue;
    REQUIRE(c.sh < 16 && c.g0 % 16 == 0 && c.g0 + (int64_t)c.A >= 0 &&
            (uint64_t)(c.g0 + (int64_t)c.B) <= bytes);
    std::vector<uint8_t> tile(8192 + 32, 0xEE);  // the staging tile: byte j of the tile at sh + j
    REQUIRE(c.sh + tlen <= tile.size());
    memcpy(tile.data() + c.sh, text.data() + (tpos[t] - tpos[0]), tlen);
    for (uint32_t word = c.A >> 4; (word << 4) < c.B; ++word) {
      const uint32_t L = word << 4;
      if (L >= c.A && L + 16 <= c.B) {
        REQUIRE((c.g0 + (int64_t)L) % 16 == 0 && (uint64_t)(c.g0 + L) + 16 <= bytes);
        memcpy(out + (c.g0 + (int64_t)L), tile.data() + L, 16);
        for (int j = 0; j < 16; ++j) hits[(size_t)(c.g0 + L + j)] += 1;
      } else {
        const uint32_t e = std::min(L + 16, c.B);
        for (uint32_t j = std::max(L, c.A); j < e; ++j) {
          REQUIRE(c.g0 + (int64_t)j >= 0 && (uint64_t)(c.g0 + j) < bytes);
          out[c.g0 + (int64_t)j] = tile[j];
          hits[(size_t)(c.g0 + j)] += 1;
        }
      }
    }
  }
  for (uint64_t i = 0; i < bytes; ++i) REQUIRE(hits[i] == 1);
  all->insert(all->end(), out, out + bytes);
  free(out);
}

static int windows() {
  std::mt19937_64 rng(14);
  uint64_t cases = 0;
  for (int round = 0; round < 400; ++round) {
    const uint64_t ntiles = 1 + rng() % 12;
    const uint64_t bases[] = {0, 7, (1ull << 32) - 1000, 1ull << 40, 1ull << 48};
    std::vector<uint64_t> tpos(ntiles + 1, bases[rng() % 5]);
    for (uint64_t t = 0; t < ntiles; ++t) {
      const uint64_t kind = rng() % 4;  // empty tiles, short ones, full ones
      const uint64_t len = kind == 0 ? 0 : kind == 1 ? rng() % 40 : kind == 2 ? 8192 : rng() % 8193;
      tpos[t + 1] = tpos[t] + len;
    }
    const uint64_t L = tpos[ntiles] - tpos[0];
    if (L == 0) continue;
    std::vector<uint8_t> text(L);
    for (auto& b : text) b = (uint8_t)rng();
    const uint64_t chunks[] = {32, 33, 47, 257, 4096, 8191, 8192, 8193, L > 1 ? L - 1 : 1, L, L + 1,
                               klsh::kSaveChunkDefault};
    for (uint64_t chunk : chunks) {
      if (chunk < 32) continue;
      REQUIRE(klsh::save_chunk_bytes(chunk) == chunk);
      const uint64_t n = klsh::save_text_chunks(L, chunk);
      REQUIRE(n >= 1 && (n - 1) * chunk < L && L <= n * chunk);
      std::vector<uint8_t> all;
      uint64_t at = tpos[0];
      for (uint64_t c = 0; c < n; ++c) {
        const klsh::SaveWindow w = klsh::save_window(tpos.data(), ntiles, L, chunk, c);
        REQUIRE(w.w0 == at && w.w1 > w.w0 && w.w1 - w.w0 <= chunk && w.t_lo < w.t_hi &&
                w.t_hi <= ntiles);
        REQUIRE(tpos[w.t_lo] <= w.w0 && tpos[w.t_hi] >= w.w1);
        REQUIRE(w.w1 - w.w0 <= klsh::save_buffer_bytes(chunk, L, 0, 16));
        emit_window(tpos, text, w, &all);
        at = w.w1;
        ++cases;
      }
      REQUIRE(at == tpos[0] + L && all == text);
    }
  }
  REQUIRE(klsh::save_chunk_bytes(0) == klsh::kSaveChunkDefault);
  // the binary file: whole rows, one at least
  REQUIRE(klsh::save_rows_per_chunk(32, 100) == 1 && klsh::save_bin_chunks(35, 32, 100) == 35);
  REQUIRE(klsh::save_rows_per_chunk(4096, 16) == 64 && klsh::save_bin_chunks(65, 4096, 16) == 2);
  REQUIRE(klsh::save_bin_chunks(0, 4096, 16) == 0);
  REQUIRE(klsh::save_buffer_bytes(32, 1000, 35, 100) == 400);
  REQUIRE(klsh::save_buffer_bytes(klsh::kSaveChunkDefault, 1000, 10, 16) == 1000);
  REQUIRE(klsh::save_buffer_bytes(64, 0, 0, 16) == 16);
  printf("windows ok: %llu windows\n", (unsigned long long)cases);
  return 0;
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "paths" && argc > 2) return paths(argv[2]);
  if (cmd == "windows") return windows();
  fprintf(stderr, "usage: save_plan_main paths DIR | windows\n");
  return 2;
}
