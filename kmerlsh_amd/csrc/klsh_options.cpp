// klsh_set_option / klsh_get_option (include/klsh.h) from one table: an entry per name with its
// getter and, unless the name is read-only, its setter.  Results never depend on an option,
// except that "stop_after" stops early.
#include <string.h>

#include "klsh_ctx.h"

namespace {

struct Option {
  const char* name;
  int64_t (*get)(klsh_ctx*);
  int (*set)(klsh_ctx*, int64_t);  // null: read-only
};

int out_of_range(const char* name, const char* range) {
  return fail(KLSH_E_ARG, std::string(name) + " must be " + range);
}
// launch sizes (0 = the default): unsigned 32-bit, bounded so no grid overflows
int grid(const char* name, int64_t v) {
  return v < 0 || v > (1 << 20) ? out_of_range(name, "in [0, 2^20]") : 0;
}
int zero_or_one(const char* name, int64_t v) {
  return v != 0 && v != 1 ? out_of_range(name, "0 or 1") : 0;
}
int at_least_zero(const char* name, int64_t v) { return v < 0 ? out_of_range(name, ">= 0") : 0; }

// An entry's getter and setter as captureless lambdas over (klsh_ctx* c, int64_t v).
#define GET(expr) [](klsh_ctx* c) -> int64_t { return (int64_t)(expr); }
#define SET(...) [](klsh_ctx* c, int64_t v) -> int { __VA_ARGS__ }
// check(name, v) guards the assignment of v, converted by `conv`, to c->field
#define CHECKED(name, check, field, conv) \
  {name, GET(c->field), SET(if (int e = check(name, v)) return e; c->field = conv; return 0;)}
#define FLAG(name, field) {name, GET(c->field), SET(c->field = v != 0; return 0;)}  // any non-zero: on
#define GRID(name, field) CHECKED(name, grid, field, (uint32_t)v)
#define BOOL01(name, field) CHECKED(name, zero_or_one, field, v != 0)
#define COUNT(name, field) CHECKED(name, at_least_zero, field, (uint64_t)v)
// stored inverted: the field switches the default off
#define INVERTED01(name, field)  \
  {name, GET(c->field ? 0 : 1), \
   SET(if (int e = zero_or_one(name, v)) return e; c->field = v ? 0u : 1u; return 0;)}
#define READONLY(name, expr) {name, GET(expr), nullptr}

const Option kOptions[] = {
    COUNT("shard_min_rows", shard_min_rows),
    FLAG("phase_timing", phase_timing),
    FLAG("kernel_timing", kernel_timing),
    FLAG("tail_batch", tail_batch),
    FLAG("huge_fold", mp.huge_fold_always),
    FLAG("tail_local", tail_local),
    BOOL01("result_device", result_device),
    BOOL01("hyperplane_async", hyperplane_async),
    COUNT("hyperplane_window", hyperplane_window),
    {"progress", GET(c->progress), SET(
        if (v < 0 || v > INT32_MAX) return out_of_range("progress", ">= 0");
        c->progress = (int)v;
        return 0;)},
    {"stop_after", GET(c->stop_after), SET(
        if (v < 0 || v > INT32_MAX) return out_of_range("stop_after", "in [0, 2^31)");
        c->stop_after = (int)v;
        return 0;)},
    {"projection", GET(c->pp.variant), SET(
        if (v != klsh::kProjAuto && v != klsh::kProjPacked)
          return out_of_range("projection", "0 (default) or 1 (exact packed chains)");
        KLSH_HIP(hipSetDevice(c->device));
        c->pp.variant = (uint32_t)v;
        return c->apply_projection_variant();)},
    {"wide_gram", GET(c->mp.wide_gram), SET(
        if (v != 0 && v != 8 && v != 16 && v != 32 && v != 64)
          return out_of_range("wide_gram", "0, 8, 16, 32 or 64");
        c->mp.wide_gram = (uint32_t)v;
        return 0;)},
    INVERTED01("wide_unrolled", pp.wide_rolled),
    INVERTED01("h16_bound", pp.v.h16_cs),
    // MergePlan::long_off: 0 = on (option value 1), 1 = off (0), 4 = 4
    {"long_runs", GET(c->mp.long_off == 1u ? 0 : c->mp.long_off == 0u ? 1 : c->mp.long_off), SET(
        if (v != 0 && v != 1 && v != 4) return out_of_range("long_runs", "0, 1 or 4");
        c->mp.long_off = v == 1 ? 0u : v == 0 ? 1u : 4u;
        KLSH_HIP(hipSetDevice(c->device));
        return c->cap_slots ? c->ensure_long(c->cap_slots, c->d) : 0;)},
    {"comm_timeout_s", GET(c->comm_timeout_s), SET(
        if (v <= 0) return out_of_range("comm_timeout_s", "> 0");
        c->comm_timeout_s = (double)v;
        if (c->comm) c->comm->timeout_s = (double)v;
        return 0;)},
    COUNT("kmc_chunk_records", kmc.chunk_records),
    {"kmc_ordinal_base", GET(c->kmc.ordinal_base), SET(
        if (v < 0 || v > (1ll << 48)) return out_of_range("kmc_ordinal_base", "in [0, 2^48]");
        c->kmc.ordinal_base = (uint64_t)v;
        return 0;)},
    {"kmc_keep_first", GET(c->kmc.keep_first), SET(
        if (!v) std::vector<uint64_t>().swap(c->kmc.first);
        c->kmc.keep_first = v != 0;
        return 0;)},
    READONLY("kmc_decode_launches", c->kmc.decode_launches),
    READONLY("kmc_high_sort", c->kmc.high_sort),
    READONLY("extract_window", klsh::kCheckWindow),
    COUNT("kcount_batch_reads", kcount.batch_reads),
    {"kcount_table_slots", GET(c->kcount.table_slots), SET(
        if (v != 0 && (v < 1024 || v > (1ll << 32) || (v & (v - 1))))
          return out_of_range("kcount_table_slots", "0 or a power of two in [1024, 2^32]");
        c->kcount.table_slots = (uint64_t)v;
        return 0;)},
    {"kcount_keep_listing", GET(c->kcount.keep_listing), SET(
        if (!v) {
          std::vector<std::vector<uint64_t>>().swap(c->kcount.values);
          std::vector<std::vector<uint32_t>>().swap(c->kcount.counts);
        }
        c->kcount.keep_listing = v != 0;
        return 0;)},
    READONLY("kcount_batches", c->kcount.batches),
    READONLY("kcount_rehashes", c->kcount.rehashes),
    READONLY("kcount_peak_slots", c->kcount.peak_slots),
    READONLY("kcount_window", klsh::kKcountWindow),
    {"kcount_db_prefix", GET(c->kcount.db_prefix), SET(
        if (v < -1 || v > 15) return out_of_range("kcount_db_prefix", "in [-1, 15]");
        c->kcount.db_prefix = (int)v;
        return 0;)},
    COUNT("kcount_db_chunk_records", kcount.db_chunk_records),
    READONLY("kcount_db_chunks", c->kcount.db_chunks),
    READONLY("kcount_db_prefix_used", c->kcount.db_prefix_used),
    {"save_chunk_bytes", GET(c->save.chunk_bytes), SET(
        if (v != 0 && (v < 32 || v > (1ll << 40)))
          return out_of_range("save_chunk_bytes", "0 or in [32, 2^40]");
        c->save.chunk_bytes = (uint64_t)v;
        return 0;)},
    {"save_offset_base", GET(c->save.offset_base), SET(
        if (v < 0 || v > (1ll << 48)) return out_of_range("save_offset_base", "in [0, 2^48]");
        c->save.offset_base = (uint64_t)v;
        return 0;)},
    {"diff_chunk_bytes", GET(c->diff.chunk_bytes), SET(
        if (v != 0 && (v < 32 || v > (1ll << 40)))
          return out_of_range("diff_chunk_bytes", "0 or in [32, 2^40]");
        c->diff.chunk_bytes = (uint64_t)v;
        return 0;)},
    READONLY("diff_tile_bytes", klsh::kDiffTile),
    {"fastq_parse", GET(c->fastq.parse), SET(
        if (v < 0 || v > 2) return out_of_range("fastq_parse", "0 (auto), 1 (host) or 2 (device only)");
        c->fastq.parse = (int)v;
        return 0;)},
    // (positions inside a chunk are 32-bit)
    {"fastq_chunk_bytes", GET(c->fastq.chunk_bytes), SET(
        if (v != 0 && (v < 64 || v > (1ll << 31)))
          return out_of_range("fastq_chunk_bytes", "0 or in [64, 2^31]");
        c->fastq.chunk_bytes = (uint64_t)v;
        return 0;)},
    READONLY("fastq_device_chunks", c->fastq.device_chunks),
    READONLY("fastq_device_reads", c->fastq.device_reads),
    READONLY("fastq_host_reads", c->fastq.host_reads),
    READONLY("fastq_takeover_at", c->fastq.takeover_at),
    READONLY("fastq_parse_us", c->fastq.parse_ms * 1000.0),
    READONLY("fastq_read_us", c->fastq.read_ms * 1000.0),
    READONLY("fastq_tile", klsh::kFqTile),
    READONLY("save_chunks", c->save.chunks),
    READONLY("save_ids_uploaded", c->save.ids_uploaded),
    GRID("h16_grid", pp.h16_grid),
    GRID("h16_segcap", pp.segcap),
    GRID("wide_grid", pp.wide_grid),
    GRID("fix_grid", pp.fix_grid),
    GRID("small_grid", mp.small_grid),
    GRID("tail_big_groups", mp.tail_nbig),
    GRID("tail_small_groups", mp.tail_nsmall),
    GRID("wide_group_grid", mp.wide_group_grid),
    GRID("small_screen_grid", mp.screen_grid),
    // (modes B and K keep a copy: their sources and sample tables are built over KmcHooks /
    // KcountHooks alone, without the context)
    {"grid_cap", GET(c->grid_cap), SET(
        if (int e = grid("grid_cap", v)) return e;
        c->grid_cap = c->kmc.grid_cap = c->kcount.grid_cap = (uint32_t)v;
        return 0;)},
    // capped at the largest size the one-launch merge's parity is pinned at (2^22: C2's
    // iterations of 2^21..2^22 positions, test_mid_local_sort's 2.6M rows); above it, runs over
    // 896 rows at d = 16 / 32 would walk in huge_runs instead of k_merge_long, which no test
    // covers.  Reads back resolved (0 = the default).
    {"tail_merge_rows", GET(klsh::tail_merge_max(c->mp)), SET(
        if (v < 0 || v > (1 << 22)) return out_of_range("tail_merge_rows", "in [0, 2^22]");
        c->mp.tail_max = (uint32_t)v;
        return 0;)},
    CHECKED("small_screen", zero_or_one, mp.small_screen, (uint32_t)v),
    BOOL01("hip_events", hip_events),
    CHECKED("tail_screen", zero_or_one, mp.tail_screen, (uint32_t)v),
    GRID("tail_screen_grid", mp.tail_screen_grid),
    CHECKED("tail_big_screen", zero_or_one, mp.tail_big_screen, (uint32_t)v),
    READONLY("result_rounds", c->result_rounds),
    READONLY("result_rank_us", c->result_rank_us),
    READONLY("member_nodes", c->loaded ? c->members : 0),
    READONLY("fp16_image", c->rows.xh != nullptr),
    READONLY("last_hash_kernel", c->last_hash_kernel),
    READONLY("last_hash_variant", c->last_hash_variant),
    READONLY("last_hash_close_pairs", c->last_hash_close),
    READONLY("tail_local_iters", c->tail_local_iters),
};

const Option* find_option(const char* name) {
  for (const Option& o : kOptions)
    if (strcmp(o.name, name) == 0) return &o;
  return nullptr;
}

}  // namespace

extern "C" {

int klsh_set_option(klsh_ctx* ctx, const char* name, int64_t value) {
  if (!ctx || !name) return fail(KLSH_E_ARG, "null argument");
  const Option* o = find_option(name);
  if (!o || !o->set) return fail(KLSH_E_ARG, std::string("unknown option ") + name);
  return o->set(ctx, value);
}

int klsh_get_option(klsh_ctx* ctx, const char* name, int64_t* value) {
  if (!ctx || !name || !value) return fail(KLSH_E_ARG, "null argument");
  const Option* o = find_option(name);
  if (!o) return fail(KLSH_E_ARG, std::string("unknown option ") + name);
  *value = o->get(ctx);
  return 0;
}

}  // extern "C"
