// The host-only pieces of klsh_save_clusters (klsh_save.cpp): the path probe,
// the chunk rule and the tiles of a text window.  No HIP here: tests/cpp/save_plan_main.cpp runs
// them under the sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <sys/stat.h>

#include <algorithm>

namespace klsh {

constexpr uint64_t kSaveChunkDefault = 64ull << 20;
inline uint64_t save_chunk_bytes(uint64_t option) { return option ? option : kSaveChunkDefault; }

// `path` can be opened for writing.  Nothing is truncated; a file the probe creates does not stay.
inline bool save_path_writable(const char* path) {
  FILE* old = fopen(path, "rb");
  if (old) fclose(old);
  FILE* f = fopen(path, "ab");
  if (!f) return false;
  fclose(f);
  if (!old) (void)remove(path);
  return true;
}

// a failed save leaves neither file (only a regular file is ever removed)
inline void save_remove(const char* path) {
  struct stat st;
  if (path && stat(path, &st) == 0 && S_ISREG(st.st_mode)) (void)remove(path);
}

// The text leaves in windows of `chunk` bytes, cut anywhere; the last is the rest.
inline uint64_t save_text_chunks(uint64_t length, uint64_t chunk) {
  return (length + chunk - 1) / chunk;
}
// The binary file leaves in whole rows: as many as fit a chunk, one at least.
inline uint64_t save_rows_per_chunk(uint64_t chunk, int d) {
  return std::max<uint64_t>(1, chunk / (sizeof(float) * (uint64_t)d));
}
inline uint64_t save_bin_chunks(uint64_t rows, uint64_t chunk, int d) {
  const uint64_t per = save_rows_per_chunk(chunk, d);
  return (rows + per - 1) / per;
}

// Window c of a text of `length` bytes at positions pos_base ..: its positions [w0, w1) and the
// tiles [t_lo, t_hi) that hold them.  tpos: the ntiles + 1 ascending tile positions, tpos[0] =
// pos_base, tpos[ntiles] = pos_base + length; c < save_text_chunks(length, chunk).
struct SaveWindow {
  uint64_t w0, w1, t_lo, t_hi;
};
inline SaveWindow save_window(const uint64_t* tpos, uint64_t ntiles, uint64_t length,
                              uint64_t chunk, uint64_t c) {
  SaveWindow w;
  w.w0 = tpos[0] + c * chunk;
  w.w1 = std::min(w.w0 + chunk, tpos[0] + length);
  // the last tile that starts at or before w0 (tiles of no bytes before it hold nothing), up to
  // the first tile that starts at or after w1
  w.t_lo = (uint64_t)(std::upper_bound(tpos, tpos + ntiles + 1, w.w0) - tpos) - 1;
  w.t_hi = (uint64_t)(std::lower_bound(tpos, tpos + ntiles + 1, w.w1) - tpos);
  return w;
}

// What of a tile leaves in a window (k_save_emit, klsh_save.hip).  The tile's tlen bytes start at
// position p0 and sit in the staging tile shifted by sh = (p0 - w0) mod 16, so that staged byte j
// goes to out[g0 + j] with g0 a multiple of 16: an aligned 16-byte word of the staging tile is an
// aligned 16-byte store.  Of them only [A, B), the bytes at positions [w0, w1), leave:
// 0 <= g0 + A and g0 + B <= w1 - w0.
#ifdef __HIPCC__
#define KLSH_SAVE_HD __host__ __device__
#else
#define KLSH_SAVE_HD
#endif
struct SaveClip {
  uint32_t sh, A, B;  // A >= B: nothing of the tile is in the window
  int64_t g0;
};
KLSH_SAVE_HD inline SaveClip save_clip(uint64_t p0, uint32_t tlen, uint64_t w0, uint64_t w1) {
  SaveClip c;
  const uint64_t lo = p0 > w0 ? p0 : w0, hi = p0 + tlen < w1 ? p0 + tlen : w1;
  c.sh = (uint32_t)((p0 - w0) & 15ull);
  c.g0 = (int64_t)(p0 - w0) - (int64_t)c.sh;
  c.A = c.B = 0;
  if (lo < hi) {
    c.A = c.sh + (uint32_t)(lo - p0);
    c.B = c.sh + (uint32_t)(hi - p0);
  }
  return c;
}

// bytes of each of the four chunk buffers: a text window or a chunk's rows, whichever is larger,
// and no more than the call needs
inline uint64_t save_buffer_bytes(uint64_t chunk, uint64_t text_bytes, uint64_t rows, int d) {
  const uint64_t row = sizeof(float) * (uint64_t)d;
  const uint64_t bin = std::min(rows, save_rows_per_chunk(chunk, d)) * row;
  return std::max<uint64_t>(std::max(std::min(chunk, text_bytes), bin), 16);
}

}  // namespace klsh
