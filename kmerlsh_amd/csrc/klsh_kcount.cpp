// Mode K behind the C ABI (include/klsh.h): kmer_set.hex / kmer_count.bin / kmer_count.log from
// the samples' FASTQ files, with no external k-mer counter (reference buildKHtable with
// kmc = true, io/ioHT.cc:83-199, which runs `kmc -k<K> -r -cs65535 -ci<C>` per sample and then
// reads the databases back).
//
// Per sample: a plain file's chunks are parsed on the device (klsh_fastq.cpp);
// for gzip, and from a chunk the device leaves to it, the host parses a batch of reads
// (klsh_fastq_next).  Either way the GPU counts the previous batch meanwhile into the sample's
// hash table (klsh_kcount.hip), which doubles between batches when the next batch could load it
// past one half.  After the last batch the entries with
// count >= count_min are sorted by their KMC value (two stable radix passes, low word then high
// word): the listing of a KMC1-layout database, the convention of DESIGN.md §8.  The listings
// stay on the device until every sample is counted; the table build of mode B (klsh::khtable_run,
// klsh_kmc.cpp) then streams them as it streams decoded database records.
//
// klsh_count_kmc also writes what the reference's `kmc` run leaves: right after a sample is
// listed, while its values are still in the counter's buffer, the listing goes out as the
// sample's KMC1-layout database (DbWriter below; k_kmcdb_pack / k_kmcdb_lut).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "klsh_ctx.h"
#include "klsh_fastq_dev.h"

namespace {

using klsh::DevBuf;
using klsh::PinBuf;

constexpr uint64_t kBatchReads = 1ull << 18, kTableSlots = 1ull << 22;

// One sample's listing on the device, and its coverage (the float running sum of
// log((double)count) in listing order, kmer/kmc_reader.cc:143).
struct Listing {
  uint64_t n = 0;
  DevBuf<uint64_t> rep;
  DevBuf<uint32_t> cnt;
  float coverage = 0.0f;
};

class ListingSource : public klsh::KhSource {
 public:
  std::vector<Listing> ls;
  uint64_t total(int j) const override { return ls[j].n; }
  uint64_t chunk(int j) const override { return ls[j].n ? ls[j].n : 1; }
  int begin(int, int, hipStream_t) override { return KLSH_OK; }
  int feed(int j, int, uint64_t r0, uint64_t, const uint64_t** rep, const uint32_t** cnt,
           hipStream_t) override {
    *rep = ls[j].rep + r0;
    *cnt = ls[j].cnt + r0;
    return KLSH_OK;
  }
  int end(int j, int pass, uint64_t* listed, float* coverage, hipStream_t) override {
    if (pass == 0) *listed = ls[j].n;
    else *coverage = ls[j].coverage;
    return KLSH_OK;
  }
};

// The prefix length of a database of n records: p in [0, min(k, 15)] with (k - p) % 4 == 0 that
// makes .kmc_pre + .kmc_suf smallest, the smaller p on a tie.
bool db_prefix_ok(int k, int p) { return p >= 0 && p <= k && p <= 15 && (k - p) % 4 == 0; }
int db_prefix_length(int k, uint64_t n) {
  int best = -1;
  uint64_t best_bytes = 0;
  for (int p = k % 4; db_prefix_ok(k, p); p += 4) {
    const uint64_t bytes = (8ull << (2 * p)) + n * (uint64_t)((k - p) / 4 + 2);
    if (best < 0 || bytes < best_bytes) best = p, best_bytes = bytes;
  }
  return best;
}

// A sample's listing, still on the device, written as its KMC1-layout database (klsh.h,
// klsh_count_kmc).  One device buffer and two pinned ones: while the host writes a chunk from one
// pinned buffer, the next chunk is packed and copied into the other.  The prefix table goes
// through the same buffers, a buffer of entries at a time.
class DbWriter {
 public:
  DbWriter(klsh_ctx* ctx, int k, uint32_t count_min, klsh_kmcdb_stats& st)
      : hooks_(ctx->kcount), s_(ctx->stream), k_(k), count_min_(count_min),
        st_(st) {}
  ~DbWriter() { (void)hipStreamSynchronize(s_); }  // no copy into the pinned buffers stays queued
  int init() {
    for (auto& b : buf_) {
      KLSH_HIP(b.e0.create());
      KLSH_HIP(b.e1.create());
      KLSH_HIP(b.done.create());
    }
    return KLSH_OK;
  }

  // the n records (val ascending, cnt) as <name>.kmc_pre / <name>.kmc_suf; on a failure neither
  // file is left
  int write(const std::string& name, const uint64_t* val, const uint32_t* cnt, uint64_t n) {
    const int p = hooks_.db_prefix >= 0 ? hooks_.db_prefix : db_prefix_length(k_, n);
    const std::string pre = name + ".kmc_pre", suf = name + ".kmc_suf";
    FILE* fs = fopen(suf.c_str(), "wb");
    FILE* fp = fs ? fopen(pre.c_str(), "wb") : nullptr;
    int rc = fp ? KLSH_OK : set_error(KLSH_E_ARG, ("cannot write " + (fs ? pre : suf)).c_str());
    uint64_t bytes = 0;
    if (rc == KLSH_OK) rc = records(fs, suf, val, cnt, n, p, &bytes);
    if (rc == KLSH_OK) rc = prefix(fp, pre, val, n, p, &bytes);
    const double tw = now_ms();
    if (fs && fclose(fs) != 0 && rc == KLSH_OK) rc = set_error(KLSH_E_ARG, (suf + ": write failed").c_str());
    if (fp && fclose(fp) != 0 && rc == KLSH_OK) rc = set_error(KLSH_E_ARG, (pre + ": write failed").c_str());
    st_.write_ms += now_ms() - tw;
    if (rc != KLSH_OK) {
      (void)hipStreamSynchronize(s_);
      if (fs) (void)remove(suf.c_str());
      if (fp) (void)remove(pre.c_str());
      return rc;
    }
    st_.prefix_len_min = st_.databases ? std::min<uint32_t>(st_.prefix_len_min, (uint32_t)p) : (uint32_t)p;
    st_.prefix_len_max = std::max<uint32_t>(st_.prefix_len_max, (uint32_t)p);
    st_.databases += 1;
    st_.records += n;
    st_.bytes += bytes;
    hooks_.db_prefix_used = p;
    return KLSH_OK;
  }

 private:
  struct Buf {
    PinBuf<uint8_t> host;
    klsh::Event e0, e1, done;  // around the kernel; after the copy
  } buf_[2];
  klsh::KcountHooks& hooks_;
  hipStream_t s_;
  int k_;
  uint32_t count_min_;
  klsh_kmcdb_stats& st_;
  DevBuf<uint8_t> dev_;
  uint64_t cap_ = 0;  // bytes of dev_ and of each pinned buffer
  static constexpr uint64_t kChunkRecords = 1ull << 22, kMinBytes = 4ull << 20;

  int reserve(uint64_t bytes) {
    if (bytes <= cap_) return KLSH_OK;
    KLSH_HIP(hipStreamSynchronize(s_));
    cap_ = 0;
    dev_.reset();
    for (auto& b : buf_) b.host.reset();
    KLSH_HIP(dev_.alloc(bytes));
    for (auto& b : buf_) KLSH_HIP(b.host.alloc(bytes));
    cap_ = bytes;
    return KLSH_OK;
  }
  int put(FILE* f, const std::string& path, const void* data, uint64_t bytes, uint64_t* total) {
    const double tw = now_ms();
    const bool ok = bytes == 0 || fwrite(data, 1, bytes, f) == bytes;
    st_.write_ms += now_ms() - tw;
    *total += bytes;
    return ok ? KLSH_OK : set_error(KLSH_E_ARG, (path + ": write failed").c_str());
  }
  // a piece finished on the device: its kernel time, then its bytes to the file
  int drain(Buf& b, FILE* f, const std::string& path, uint64_t bytes, uint64_t* total) {
    KLSH_HIP(hipEventSynchronize(b.done));
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, b.e0, b.e1);
    st_.pack_ms += ms;
    return put(f, path, b.host, bytes, total);
  }

  // "KMCS", the records chunk by chunk, "KMCS"
  int records(FILE* f, const std::string& path, const uint64_t* val, const uint32_t* cnt,
              uint64_t n, int p, uint64_t* total) {
    const uint32_t sufix = (uint32_t)(k_ - p) / 4u, rec = sufix + 2u;
    const uint64_t per = hooks_.db_chunk_records ? hooks_.db_chunk_records : kChunkRecords;
    int rc = put(f, path, "KMCS", 4, total);
    if (rc) return rc;
    if ((rc = reserve(std::max<uint64_t>(std::min<uint64_t>(per, n) * rec, kMinBytes)))) return rc;
    auto start = [&](uint64_t r0) {  // chunk r0 / per packed and on its way to its pinned buffer
      Buf& b = buf_[(r0 / per) & 1];
      const uint64_t m = std::min<uint64_t>(per, n - r0);
      KLSH_HIP(hipEventRecord(b.e0, s_));
      klsh::launch_kmcdb_pack(val, cnt, r0, m, sufix, dev_, s_,
                              hooks_.grid_cap);
      KLSH_HIP(hipGetLastError());
      KLSH_HIP(hipEventRecord(b.e1, s_));
      KLSH_HIP(hipMemcpyAsync(b.host, dev_, m * rec, hipMemcpyDeviceToHost, s_));
      KLSH_HIP(hipEventRecord(b.done, s_));
      hooks_.db_chunks += 1;
      st_.chunks += 1;
      return (int)KLSH_OK;
    };
    if (n && (rc = start(0))) return rc;
    for (uint64_t r0 = 0; r0 < n; r0 += per) {
      if (r0 + per < n && (rc = start(r0 + per))) return rc;
      if ((rc = drain(buf_[(r0 / per) & 1], f, path, std::min<uint64_t>(per, n - r0) * rec, total)))
        return rc;
    }
    return put(f, path, "KMCS", 4, total);
  }

  // "KMCP", the prefix table, the header, its size, "KMCP"
  int prefix(FILE* f, const std::string& path, const uint64_t* val, uint64_t n, int p,
             uint64_t* total) {
    const uint64_t entries = 1ull << (2 * p), per = cap_ / 8;
    int rc = put(f, path, "KMCP", 4, total);
    if (rc) return rc;
    auto start = [&](uint64_t q0) {
      Buf& b = buf_[(q0 / per) & 1];
      const uint64_t mq = std::min<uint64_t>(per, entries - q0);
      KLSH_HIP(hipEventRecord(b.e0, s_));
      klsh::launch_kmcdb_lut(val, n, q0, mq, k_, p, reinterpret_cast<uint64_t*>(dev_.get()), s_,
                             hooks_.grid_cap);
      KLSH_HIP(hipGetLastError());
      KLSH_HIP(hipEventRecord(b.e1, s_));
      KLSH_HIP(hipMemcpyAsync(b.host, dev_, mq * 8, hipMemcpyDeviceToHost, s_));
      KLSH_HIP(hipEventRecord(b.done, s_));
      return (int)KLSH_OK;
    };
    if ((rc = start(0))) return rc;
    for (uint64_t q0 = 0; q0 < entries; q0 += per) {
      if (q0 + per < entries && (rc = start(q0 + per))) return rc;
      if ((rc = drain(buf_[(q0 / per) & 1], f, path, std::min<uint64_t>(per, entries - q0) * 8, total)))
        return rc;
    }
    const uint64_t header[5] = {(uint64_t)k_, 2ull | ((uint64_t)p << 32),
                                (uint64_t)count_min_ | (65535ull << 32), n, 0ull};
    const uint32_t header_size = sizeof(header);
    if ((rc = put(f, path, header, sizeof(header), total))) return rc;
    if ((rc = put(f, path, &header_size, 4, total))) return rc;
    return put(f, path, "KMCP", 4, total);
  }
};

// The counting of one call: the sample table, the two batch slots, the sort buffers.
class Counter {
 public:
  Counter(klsh_ctx* ctx, int k, uint32_t count_min, klsh_kcount_stats& st)
      : hooks_(ctx->kcount), s_(ctx->stream), k_(k), count_min_(count_min),
        st_(st), chunks_(ctx) {}
  int init() {
    cap_ = hooks_.table_slots ? hooks_.table_slots : kTableSlots;
    hooks_.peak_slots = cap_;
    KLSH_HIP(keys_.alloc(cap_));
    KLSH_HIP(cnt_.alloc(cap_));
    KLSH_HIP(ctr_.alloc(8));
    KLSH_HIP(hctr_.alloc(8));
    for (auto& sl : slot_)
      if (int rc = sl.dev.init()) return rc;
    return KLSH_OK;
  }

  // path's reads counted, the listing left in *out
  int sample(const char* path, Listing* out, std::vector<uint64_t>* keep_val,
             std::vector<uint32_t>* keep_cnt) {
    // the file's chunks on the device while they are regular, the host reader from
    // where they are not, or from the start
    occ_ = pos_ = 0;
    KLSH_HIP(hipMemsetAsync(keys_, 0xFF, cap_ * 8, s_));
    KLSH_HIP(hipMemsetAsync(cnt_, 0, cap_ * 4, s_));
    KLSH_HIP(hipMemsetAsync(ctr_, 0, 64, s_));
    bool on_device = false, host_rest = true;
    if (int rc = chunks_.open(path, &on_device)) return rc;
    if (on_device) {
      if (int rc = count_chunks(&host_rest)) {
        (void)hipStreamSynchronize(s_);
        return rc;
      }
    }
    if (host_rest) {
      int err = KLSH_OK;
      klsh_fastq* f = klsh::fastq_open_at(path, chunks_.offset(), &err);
      if (!f) return err;
      const uint64_t before = st_.reads;
      const int rc = count(f);
      klsh_fastq_close(f);
      chunks_.host_reads(st_.reads - before);
      if (rc) return rc;
    }
    return list(out, keep_val, keep_cnt);
  }
  // the KMC values of the last sample's listing (device), until the next sample is listed
  const uint64_t* values() const { return val_; }

 private:
  struct Slot {
    std::vector<char> seq;
    std::vector<uint64_t> off;
    klsh::ReadBatch dev;
  } slot_[2];
  klsh::KcountHooks& hooks_;
  hipStream_t s_;
  int k_;
  uint32_t count_min_;
  klsh_kcount_stats& st_;
  uint64_t cap_ = 0, occ_ = 0, pos_ = 0;
  PinBuf<uint64_t> hctr_;
  DevBuf<uint64_t> keys_, ctr_, val_;
  DevBuf<uint32_t> cnt_, lo_, lo2_, sl_, sl2_, ws_;
  uint64_t sort_cap_ = 0;
  klsh::FastqChunks chunks_;

  // the table doubled until `more` further k-mers keep it at most half full
  int grow(uint64_t more) {
    while (occ_ + more > cap_ / 2) {
      const uint64_t ncap = cap_ * 2;
      if (ncap > (1ull << 32)) return set_error(KLSH_E_RANGE, "more than 2^31 distinct k-mers in a sample");
      DevBuf<uint64_t> nkeys;
      DevBuf<uint32_t> ncnt;
      if (nkeys.alloc(ncap) != hipSuccess || ncnt.alloc(ncap) != hipSuccess)
        return set_error(KLSH_E_NOMEM, "count_khtable: the grown k-mer table");
      hipError_t e = hipMemsetAsync(nkeys, 0xFF, ncap * 8, s_);
      if (e == hipSuccess) e = hipMemsetAsync(ncnt, 0, ncap * 4, s_);
      if (e == hipSuccess) {
        klsh::launch_kcount_rehash(keys_, cnt_, cap_, nkeys, ncnt, ncap - 1, s_,
                                   hooks_.grid_cap);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipStreamSynchronize(s_);
      if (e != hipSuccess)
        return set_error(KLSH_E_HIP, (std::string("count_khtable: rehash -> ") + hipGetErrorString(e)).c_str());
      keys_ = std::move(nkeys);  // (the old table is freed)
      cnt_ = std::move(ncnt);
      cap_ = ncap;
      hooks_.peak_slots = cap_;
      hooks_.rehashes += 1;
      st_.rehashes += 1;
    }
    return KLSH_OK;
  }

  int launch(Slot& sl) {
    const uint64_t n = sl.off.size() - 1, nb = sl.seq.size();
    if (int rc = sl.dev.upload(sl.seq.data(), nb, sl.off.data(), n, nb + nb / 4 + 64, s_)) return rc;
    KLSH_HIP(hipEventRecord(sl.dev.e0, s_));
    klsh::launch_kcount_reads(sl.dev.seq, sl.dev.off, n, k_, keys_, cnt_, cap_ - 1, ctr_, s_,
                              hooks_.grid_cap);
    KLSH_HIP(hipGetLastError());
    KLSH_HIP(hipEventRecord(sl.dev.e1, s_));
    KLSH_HIP(hipMemcpyAsync(hctr_, ctr_, 16, hipMemcpyDeviceToHost, s_));
    return KLSH_OK;
  }

  // the batch in flight finished: its kernel time, the table's load and the windows so far
  int finish(Slot& sl) {
    KLSH_HIP(hipStreamSynchronize(s_));
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, sl.dev.e0, sl.dev.e1);
    st_.kernel_ms += ms;
    occ_ = hctr_[0];
    pos_ = hctr_[1];
    return KLSH_OK;
  }

  // The device chunks of the open file: each parsed and packed into its slot's batch, then counted
  // by the protocol of count() below, a launch per `per` reads at an offset into the chunk's
  // offsets.  The next chunk's file read runs while the last launch of this one does; its upload
  // and parse queue behind that launch (the parse synchronises the stream).
  // *host_rest = the host reader has the rest of the file to read, from chunks_.offset().
  int count_chunks(bool* host_rest) {
    const uint64_t per = hooks_.batch_reads ? hooks_.batch_reads : kBatchReads;
    int cur = 0;
    bool pending = false;
    while (true) {
      const double tp = now_ms();
      Slot& sl = slot_[cur];
      uint64_t n = 0;
      bool eof = false;
      if (int rc = chunks_.next(cur, sl.dev, false, true, &n, &eof)) return rc;
      st_.parse_ms += now_ms() - tp;
      if (n == 0) {
        if (pending) {
          if (int rc = finish(slot_[cur ^ 1])) return rc;
        }
        *host_rest = !eof;
        return KLSH_OK;
      }
      st_.reads += n;
      st_.bases += chunks_.slot[cur].bases;
      const uint64_t* off = chunks_.slot[cur].hoff.get();
      for (uint64_t r0 = 0; r0 < n; r0 += per) {
        const uint64_t m = std::min<uint64_t>(per, n - r0);
        uint64_t windows = 0;  // an upper bound of the launch's new k-mers
        for (uint64_t i = r0; i < r0 + m; ++i) {
          const uint64_t len = off[i + 1] - off[i];
          if (len >= (uint64_t)k_) windows += len - (uint64_t)k_ + 1;
        }
        if (pending) {  // (the first launch of a chunk waits for the last of the chunk before)
          if (int rc = finish(r0 ? sl : slot_[cur ^ 1])) return rc;
        }
        pending = false;
        if (int rc = grow(windows)) return rc;
        KLSH_HIP(hipEventRecord(sl.dev.e0, s_));
        klsh::launch_kcount_reads(sl.dev.seq, sl.dev.off.get() + r0, m, k_, keys_, cnt_, cap_ - 1, ctr_,
                                  s_, hooks_.grid_cap);
        KLSH_HIP(hipGetLastError());
        KLSH_HIP(hipEventRecord(sl.dev.e1, s_));
        KLSH_HIP(hipMemcpyAsync(hctr_, ctr_, 16, hipMemcpyDeviceToHost, s_));
        pending = true;
        hooks_.batches += 1;
        st_.batches += 1;
      }
      cur ^= 1;
    }
  }

  // the reads of the host reader, from where it stands
  int count(klsh_fastq* f) {
    const uint64_t per = hooks_.batch_reads ? hooks_.batch_reads : kBatchReads;
    int cur = 0, rc = KLSH_OK;
    bool pending = false;
    while (true) {
      // the host parses this batch while the GPU counts the previous one
      const double tp = now_ms();
      const char* seq = nullptr;
      const uint64_t* off = nullptr;
      const int64_t n = klsh_fastq_next(f, per, &seq, &off, nullptr, nullptr, nullptr, nullptr);
      if (n < 0) {
        rc = (int)n;
        break;
      }
      Slot& sl = slot_[cur];
      uint64_t windows = 0;  // an upper bound of the batch's new k-mers
      if (n > 0) {
        sl.seq.assign(seq + off[0], seq + off[n]);
        sl.off.resize((size_t)n + 1);
        for (int64_t i = 0; i <= n; ++i) sl.off[i] = off[i] - off[0];
        for (int64_t i = 0; i < n; ++i) {
          const uint64_t len = sl.off[i + 1] - sl.off[i];
          if (len >= (uint64_t)k_) windows += len - (uint64_t)k_ + 1;
        }
        st_.reads += (uint64_t)n;
        st_.bases += sl.seq.size();
      }
      st_.parse_ms += now_ms() - tp;
      if (pending && (rc = finish(slot_[cur ^ 1]))) break;
      pending = false;
      if (n == 0) break;
      if ((rc = grow(windows))) break;
      if ((rc = launch(sl))) break;
      pending = true;
      hooks_.batches += 1;
      st_.batches += 1;
      cur ^= 1;
    }
    if (rc) (void)hipStreamSynchronize(s_);  // nothing of this sample stays queued
    return rc;
  }

  int list(Listing* out, std::vector<uint64_t>* keep_val, std::vector<uint32_t>* keep_cnt) {
    st_.positions += pos_;
    st_.distinct += occ_;
    if (occ_ + 64 > sort_cap_) {
      sort_cap_ = 0;
      for (auto* b : {&lo_, &lo2_, &sl_, &sl2_, &ws_}) b->reset();
      val_.reset();
      const uint64_t c = occ_ + occ_ / 4 + 64;
      for (auto* b : {&lo_, &lo2_, &sl_, &sl2_}) KLSH_HIP(b->alloc(c));
      KLSH_HIP(ws_.alloc(klsh::sort_ws_words(c)));
      KLSH_HIP(val_.alloc(c));
      sort_cap_ = c;
    }
    uint32_t* nout = reinterpret_cast<uint32_t*>(ctr_ + 4);
    uint32_t n = 0;
    KLSH_HIP(hipMemsetAsync(nout, 0, 4, s_));
    klsh::launch_kcount_collect(keys_, cnt_, cap_, count_min_, lo_, sl_, nout, s_,
                                hooks_.grid_cap);
    KLSH_HIP(hipGetLastError());
    KLSH_HIP(hipMemcpyAsync(&n, nout, 4, hipMemcpyDeviceToHost, s_));
    KLSH_HIP(hipStreamSynchronize(s_));
    uint32_t* ov = nullptr;  // ascending KMC value, a word of 2k bits
    klsh::order_slots_u64(lo_, sl_, lo2_, sl2_, n, 2 * k_, ws_, keys_, s_, hooks_.grid_cap, &ov);
    KLSH_HIP(hipGetLastError());
    out->n = n;
    KLSH_HIP(out->rep.alloc(n));
    KLSH_HIP(out->cnt.alloc(n));
    klsh::launch_kcount_emit(keys_, cnt_, ov, n, k_, val_, out->rep, out->cnt, s_,
                             hooks_.grid_cap);
    KLSH_HIP(hipGetLastError());
    std::vector<uint32_t> hcnt(n);
    if (n) KLSH_HIP(hipMemcpyAsync(hcnt.data(), out->cnt, n * 4ull, hipMemcpyDeviceToHost, s_));
    if (keep_val) {
      keep_val->resize(n);
      if (n) KLSH_HIP(hipMemcpyAsync(keep_val->data(), val_, n * 8ull, hipMemcpyDeviceToHost, s_));
    }
    KLSH_HIP(hipStreamSynchronize(s_));
    float cov = 0.0f;
    for (uint32_t i = 0; i < n; ++i) cov += log((double)hcnt[i]);
    out->coverage = cov;
    st_.listed += n;
    if (keep_cnt) keep_cnt->swap(hcnt);
    return KLSH_OK;
  }
};

}  // namespace

extern "C" int klsh_kcount_listing(klsh_ctx* ctx, int sample, uint64_t* kmc_values,
                                   uint32_t* counts, uint64_t* n) {
  if (!ctx || !n) return set_error(KLSH_E_ARG, "null argument");
  const klsh::KcountHooks& h = ctx->kcount;
  if (sample < 0 || (size_t)sample >= h.values.size())
    return set_error(KLSH_E_ARG, "klsh_kcount_listing: no kept listing of that sample");
  const std::vector<uint64_t>& v = h.values[sample];
  const uint64_t room = *n;
  *n = v.size();
  if (!kmc_values && !counts) return KLSH_OK;
  if (room < v.size()) return set_error(KLSH_E_RANGE, "klsh_kcount_listing: output too small");
  if (kmc_values && !v.empty()) memcpy(kmc_values, v.data(), v.size() * 8);
  if (counts && !v.empty()) memcpy(counts, h.counts[sample].data(), v.size() * 4);
  return KLSH_OK;
}

namespace {

// klsh_count_khtable (db_names == nullptr) and klsh_count_kmc: every sample counted and listed,
// its database written while its values are still on the device, then (table) the table build.
int count_run(klsh_ctx* ctx, const char* const* fastq_paths, const char* const* db_names,
              int n_samples, int k, int count_min, const char* out_dir, bool table,
              klsh_kcount_stats* st, klsh_kmcdb_stats* dst) {
  if (!ctx || !fastq_paths || n_samples <= 0) return set_error(KLSH_E_ARG, "bad argument");
  if (k < 1 || k > 32) return set_error(KLSH_E_RANGE, "k must be in [1, 32] (Kmer::MAX_K)");
  const double t_start = now_ms();
  if (st && st->struct_size != sizeof(klsh_kcount_stats))
    return set_error(KLSH_E_ARG, "klsh_kcount_stats.struct_size != sizeof: built against another klsh.h");
  if (dst && dst->struct_size != sizeof(klsh_kmcdb_stats))
    return set_error(KLSH_E_ARG, "klsh_kmcdb_stats.struct_size != sizeof: built against another klsh.h");
  klsh_kcount_stats local{};
  local.struct_size = sizeof(local);
  klsh_kmcdb_stats dlocal{};
  dlocal.struct_size = sizeof(dlocal);
  klsh::KcountHooks& hooks = ctx->kcount;  // test hooks; what this call reaches
  klsh::KmcHooks& bhooks = ctx->kmc;
  hooks.batches = hooks.rehashes = hooks.peak_slots = 0;
  hooks.db_chunks = 0;
  hooks.db_prefix_used = -1;
  klsh::FastqChunks::begin_call(ctx);
  hooks.values.clear();
  hooks.counts.clear();
  bhooks.decode_launches = 0;
  bhooks.high_sort = 0;
  bhooks.first.clear();
  for (int j = 0; j < n_samples; ++j) {  // a missing file fails before any device work
    FILE* f = fastq_paths[j] ? fopen(fastq_paths[j], "rb") : nullptr;
    if (!f)
      return set_error(KLSH_E_ARG, fastq_paths[j] ? (std::string("cannot open ") + fastq_paths[j]).c_str()
                                                  : "null FASTQ path");
    fclose(f);
  }
  if (db_names) {  // and so does a database that could not be written
    if (hooks.db_prefix >= 0 && !db_prefix_ok(k, hooks.db_prefix))
      return set_error(KLSH_E_ARG, "kcount_db_prefix: not a prefix length of this k (p <= min(k, 15), "
                                   "(k - p) % 4 == 0)");
    for (int j = 0; j < n_samples; ++j) {
      if (!db_names[j]) return set_error(KLSH_E_ARG, "null database name");
      for (int i = 0; i < j; ++i)
        if (!strcmp(db_names[i], db_names[j]))
          return set_error(KLSH_E_ARG, (std::string("database named twice: ") + db_names[j]).c_str());
    }
    for (int j = 0; j < n_samples; ++j)
      for (const char* ext : {".kmc_pre", ".kmc_suf"}) {
        const std::string path = std::string(db_names[j]) + ext;
        FILE* old = fopen(path.c_str(), "rb");  // a file the probe creates does not stay
        if (old) fclose(old);
        FILE* f = fopen(path.c_str(), "ab");
        if (!f) return set_error(KLSH_E_ARG, ("cannot write " + path).c_str());
        fclose(f);
        if (!old) (void)remove(path.c_str());
      }
  }
  if (hipSetDevice(ctx->device) != hipSuccess) return set_error(KLSH_E_HIP, "hipSetDevice");
  int rc;
  {
    ListingSource src;
    src.ls.resize(n_samples);
    if (hooks.keep_listing) {
      hooks.values.resize(n_samples);
      hooks.counts.resize(n_samples);
    }
    {
      const uint32_t cmin = (uint32_t)(count_min < 1 ? 1 : count_min);
      Counter counter(ctx, k, cmin, local);
      DbWriter writer(ctx, k, cmin, dlocal);
      rc = counter.init();
      if (rc == KLSH_OK && db_names) rc = writer.init();
      for (int j = 0; j < n_samples && rc == KLSH_OK; ++j) {
        Listing& l = src.ls[j];
        rc = counter.sample(fastq_paths[j], &l, hooks.keep_listing ? &hooks.values[j] : nullptr,
                            hooks.keep_listing ? &hooks.counts[j] : nullptr);
        if (rc == KLSH_OK && db_names) rc = writer.write(db_names[j], counter.values(), l.cnt, l.n);
        if (!table) {  // nothing reads the listing again
          l.rep.reset();
          l.cnt.reset();
        }
      }
    }  // the sample table is freed before the union's
    if (rc == KLSH_OK && table) {
      klsh_khtable_stats bst{};
      bst.struct_size = sizeof(bst);
      rc = klsh::khtable_run(ctx, src, n_samples, k, out_dir, &bst);
      local.kmap_size = bst.kmap_size;
      local.order_ms = bst.order_ms;
    }
    if (rc != KLSH_OK) {
      hooks.values.clear();
      hooks.counts.clear();
    }
  }
  local.total_ms = now_ms() - t_start;
  if (st) *st = local;
  if (dst) *dst = dlocal;
  return rc;
}

}  // namespace

extern "C" int klsh_count_khtable(klsh_ctx* ctx, const char* const* fastq_paths, int n_samples,
                                  int k, int count_min, const char* out_dir,
                                  klsh_kcount_stats* st) {
  return count_run(ctx, fastq_paths, nullptr, n_samples, k, count_min, out_dir, true, st, nullptr);
}

extern "C" int klsh_count_kmc(klsh_ctx* ctx, const char* const* fastq_paths,
                              const char* const* db_names, int n_samples, int k, int count_min,
                              const char* out_dir, klsh_kcount_stats* st, klsh_kmcdb_stats* dst) {
  if (!db_names && !out_dir) return set_error(KLSH_E_ARG, "neither databases nor a table asked for");
  return count_run(ctx, fastq_paths, db_names, n_samples, k, count_min, out_dir, out_dir != nullptr,
                   st, dst);
}
