// The host-only pieces of klsh_diff_ksets / klsh_parse_clust (klsh_diff.cpp): the
// reference's reader of <F>.clust (IOMat::ReadClusterAll, io/ioMatrix.cc:48-119: getline, then a
// strtol chain per line) over blocks of any size, and the grammar that decides whether the device
// kernels may parse a text instead.  No HIP here: tests/cpp/clust_parse_main.cpp runs them under
// the sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

namespace klsh {

constexpr uint64_t kClustMaxEntries = 1ull << 32;  // declared counts must sum to less
constexpr uint32_t kClustMaxDigits = 18;           // a longer digit run could reach LONG_MAX
constexpr uint64_t kClustRegular = ~0ull;          // ClustGrammar::at of a regular text

inline uint64_t clust_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

// The grammar of a REGULAR text, fed in blocks: every byte a digit, a newline or one of the other
// five isspace bytes of the C locale (9, 11, 12, 13, 32), no digit run longer than kClustMaxDigits.
// at = the smallest offset that breaks it (of a byte outside the set, or of the first digit of an
// over-long run), kClustRegular if none does.
struct ClustGrammar {
  uint64_t at = kClustRegular;
  uint64_t pos = 0;  // bytes fed
  uint64_t run = 0;  // digits of the run the last byte fed is in
  void feed(const char* p, size_t n) {
    for (size_t i = 0; i < n; ++i, ++pos) {
      const unsigned char c = (unsigned char)p[i];
      if (c >= '0' && c <= '9') {
        // (a run's first digit precedes every later byte, so `at` takes it only if nothing
        // earlier broke the grammar)
        if (++run == kClustMaxDigits + 1 && pos - kClustMaxDigits < at) at = pos - kClustMaxDigits;
        continue;
      }
      run = 0;
      const bool blank = c == '\n' || c == ' ' || c == '\t' || (c >= 11 && c <= 13);
      if (!blank && pos < at) at = pos;
    }
  }
};

// The reference's parse, fed in blocks: lines are getline's (an unterminated, non-empty last line
// counts, finish()); per line the first strtol gives n, the declared member count, and up to n
// further strtol results are its ids, the missing ones 0 (strtol sees the line up to its first NUL
// byte, as it does through std::string::c_str()).  The declared counts are summed saturating; once
// they reach kClustMaxEntries the parse goes on counting lines and keeps no id (`range`).  Callers
// go through clust_parse_text below, whose first pass keeps no ids at all.
struct ClustParser {
  bool keep_ids = true;           // false: counts and offsets only (a size query)
  std::vector<uint64_t> counts;   // n per line
  std::vector<uint64_t> off{0};   // off[c] = the declared counts before line c
  std::vector<uint64_t> ids;
  uint64_t lines = 0, entries = 0;  // entries: the saturating sum of the declared counts
  bool range = false;               // entries >= kClustMaxEntries
  ClustGrammar grammar;

  void feed(const char* p, size_t n) {
    grammar.feed(p, n);
    any_ = any_ || n > 0;
    const char* end = p + n;
    while (p < end) {
      const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
      if (!nl) {
        line_.append(p, (size_t)(end - p));
        return;
      }
      line_.append(p, (size_t)(nl - p));
      parse_line();
      p = nl + 1;
    }
  }
  void finish() {
    if (any_ && !line_.empty()) parse_line();
  }

 private:
  std::string line_;  // the line the last block left open
  bool any_ = false;

  void parse_line() {
    const char* p = line_.c_str();
    char* e = nullptr;
    const uint64_t n = (uint64_t)strtol(p, &e, 10);
    lines += 1;
    entries = clust_sat_add(entries, n);
    if (entries >= kClustMaxEntries && !range) {
      range = true;
      std::vector<uint64_t>().swap(ids);
    }
    counts.push_back(n);
    if (!range) {
      off.push_back(entries);
      if (keep_ids) {
        const size_t base = ids.size();
        ids.resize(base + n, 0);  // (n < 2^32 here)
        uint64_t got = 0;
        while (p != e && got < n) {
          p = e;
          ids[base + got++] = (uint64_t)strtol(p, &e, 10);
        }
      }
    }
    line_.clear();
  }
};

// The whole of a text through the parser: feed_all(parser) feeds every block.  Two passes, so
// that a text which declares 2^32 entries or more allocates nothing for its ids: the first keeps
// the counts alone; the second, only if the ids are wanted and fit, stores them into a vector
// reserved once.
template <class FeedAll>
inline bool clust_parse_text(FeedAll feed_all, bool want_ids, ClustParser* ps) {
  *ps = ClustParser();
  ps->keep_ids = false;
  if (!feed_all(ps)) return false;
  ps->finish();
  if (!want_ids || ps->range || ps->entries == 0) return true;
  ClustParser second;
  second.ids.reserve(ps->entries);
  second.counts.reserve(ps->lines);
  second.off.reserve(ps->lines + 1);
  if (!feed_all(&second)) return false;
  second.finish();
  *ps = std::move(second);
  return true;
}

// ... of an open file, `block` bytes at a time (at least 1).  False on a read error.
inline bool clust_parse_file(FILE* f, size_t block, bool want_ids, ClustParser* ps) {
  std::vector<char> buf(block ? block : 1);
  return clust_parse_text(
      [&](ClustParser* to) {
        rewind(f);
        while (true) {
          const size_t got = fread(buf.data(), 1, buf.size(), f);
          if (got) to->feed(buf.data(), got);
          if (got < buf.size()) break;
        }
        return !ferror(f);
      },
      want_ids, ps);
}

// ... of a text in memory
inline bool clust_parse_mem(const char* text, size_t len, bool want_ids, ClustParser* ps) {
  return clust_parse_text(
      [&](ClustParser* to) {
        if (len) to->feed(text, len);
        return true;
      },
      want_ids, ps);
}

}  // namespace klsh
