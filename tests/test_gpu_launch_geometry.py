"""Strided kernels at grids that give every workgroup several trips.

Almost every kernel of the engine is persistent or grid-stride: a workgroup (or wave) takes item
blockIdx.x, then blockIdx.x + gridDim.x, and between trips it reuses LDS layouts, per-wave
buffers, per-workgroup fix-up segments and, in k_merge_long, a bit matrix in global memory.  At
the sizes the rest of the suite uses, the default grids are at least as large as the work, so a
kernel that is right on its first item and wrong on its second passes everything else.
include/klsh.h promises of the launch-size options that results never depend on them; this file
holds that claim: every case forces a grid of 1, 2 or 3 workgroups (the options of klsh.h, and
"grid_cap" for the launches that have none of their own) and compares, by bits, with the oracle
or the model — never with a default-grid run of the engine.

Each test first proves from the reference alone, on the CPU, that its geometry forces a second
trip (more runs, tiles, reads or records than the grid takes at once), and fails if it does not.
"""
import math

import numpy as np
import pytest

import klsh_oracle_e as oe  # (oracle/ is on sys.path via conftest)
import test_gpu_sharded as sharded
import test_mode_b as tb
import test_mode_e as te
import test_mode_k as tk
import test_mode_k_db as tdb
from row_state import (LADDER_CALL, LADDER_SHAPES, adversarial_rows, check, check_state,
                       ladder_reference, options)
from test_mode_b import dbs  # noqa: F401  (module-scoped fixtures of the mode tests)
from test_mode_k import cases  # noqa: F401
from test_mode_k_db import cases as db_cases  # noqa: F401

pytestmark = pytest.mark.gpu

BIG = 1000000   # bucket_size_threshold: no run is oversize
NESTED = 700    # runs over 700 rows go through nestedCluster
PER_CLASS = {"tail_merge_rows": 1}
PROJ_1 = {"h16_grid": 1, "wide_grid": 1, "fix_grid": 1}  # the loop's projection on one workgroup

# ------------------------------------------------------------- preconditions, from the oracle ---
CLASS_HI = [64, 128, 192, 384, 896]  # run classes 0..5: 2..64, 65..128, ..., 385..896, longer
BIG_CLASSES = (1, 2, 3, 4, 5)
_runs = {}


def first_iteration_runs(oracle, d, special=False):
    """Lengths of the runs of 2+ equal keys in the first iteration of the ladder loop at width d:
    the oracle's hyperplanes (seed 777, counter 3, floor(log2 n) of them) and keys."""
    if (d, special) not in _runs:
        n = LADDER_SHAPES[d]
        rows = ladder_reference(oracle, n, d, BIG, special=special)[0][0]
        _, _, seed, counter = LADDER_CALL
        w, _ = oracle.table(seed, counter, int(math.floor(math.log2(n))), d)
        _, lengths = np.unique(oracle.keys(rows, w), return_counts=True)
        _runs[d, special] = lengths[lengths >= 2]
    return _runs[d, special]


def class_counts(lengths, bthr=BIG):
    """Runs per class among the runs of at most bthr rows (longer ones are nested)."""
    lengths = lengths[lengths <= bthr]
    return np.bincount(np.searchsorted(CLASS_HI, lengths), minlength=6)


def require_second_trip(oracle, d, opts, bthr=BIG, special=False):
    """Fails unless, in the first iteration, every launch that `opts` shrinks has more items than
    workgroups (or waves) — from the oracle's keys alone."""
    lengths = first_iteration_runs(oracle, d, special)
    cnt = class_counts(lengths, bthr)
    what = f"d={d} bthr={bthr} special={special} {opts}: runs per class {cnt.tolist()}"
    if bthr < BIG:
        assert (lengths > bthr).sum() >= 1, what  # the nested path is taken at all
    per_class = opts.get("tail_merge_rows") == 1 or d not in (8, 16, 32, 64)
    if not per_class:
        if "tail_big_groups" in opts:
            # one index space over the five big classes: with g workgroups, more than g runs in
            # every class means a workgroup walks every LDS layout, each after another run
            g = opts["tail_big_groups"]
            assert all(cnt[c] > g for c in BIG_CLASSES if CLASS_HI[c - 1] < bthr), what
        if "tail_small_groups" in opts:  # four waves per small-run workgroup
            assert cnt[0] > 4 * opts["tail_small_groups"], what
        if "tail_screen_grid" in opts and d in (32, 64) and opts.get("tail_screen", 1):
            # one wave: its LDS buffer of passed runs (256, flushed when 64 more might not fit)
            # fills past the flush mark only with more than 192 runs
            assert opts["tail_screen_grid"] == 1 and cnt[0] > 192, what
        return
    if "grid_cap" in opts:
        g = opts["grid_cap"]
        covered = [c for c in BIG_CLASSES if CLASS_HI[c - 1] < bthr]
        if "long_runs" in opts:  # the case is about the two lists k_merge_long / k_merge_huge walk
            covered = [c for c in covered if c >= 4]
        assert covered and all(cnt[c] > g for c in covered), what
    if "small_grid" in opts:
        assert opts["small_grid"] == 1 and cnt[0] > 1, what
    if "small_screen_grid" in opts and d in (32, 64):
        assert opts["small_screen_grid"] == 1 and cnt[0] > 192, what  # the mid-loop flush()
    if "wide_group_grid" in opts:
        # per class of 2, 3-4, 5-8, ... 33-64 rows: one wave takes 32, 16, 8, 4, 2, 1 runs a trip
        assert opts["wide_group_grid"] == 1, what
        small = lengths[lengths <= 64]
        sub = np.bincount(np.searchsorted([2, 4, 8, 16, 32], small), minlength=6)
        assert all(sub[c] > (32 >> c) for c in range(6)), (what, sub.tolist())


def require_projection_trips(d, n):
    """The loop's projection on one workgroup: 256 rows a trip at d = 16, 32, 64 (k_project_h16),
    192 above 64 (k_project_mfma_wide: six waves of 32 rows)."""
    tile = 256 if d in (16, 32, 64) else 192
    assert n > 3 * tile and n % tile, (d, n)


def run_ladder(engine, oracle, d, opts, bthr=BIG, special=False):
    """The ladder loop under `opts`: trace, counter, result and row state against the oracle."""
    require_second_trip(oracle, d, opts, bthr, special)
    if "h16_grid" in opts or "wide_grid" in opts:
        require_projection_trips(d, LADDER_SHAPES[d])
    n = LADDER_SHAPES[d]
    (rows, off, ids), want = ladder_reference(oracle, n, d, bthr, special=special)
    min_sim, iters, seed, counter = LADDER_CALL
    with options(engine, **opts):
        for k, v in opts.items():
            assert engine.get_option(k) == v, k
        engine.load_rows(rows, off, ids)
        trace, c, _ = engine.cluster(min_sim, iters, bthr, seed, counter)
        assert np.array_equal(trace, want[3]) and c == want[4], (d, opts, trace, want[3])
        assert trace[-1] < trace[0]
        check(engine, want, f"ladder n={n} d={d} bthr={bthr} special={special} {opts}")


def ids_of(cases_):
    return [" ".join(f"{k}={v}" for k, v in c.items()) if isinstance(c, dict) else str(c)
            for c in cases_]


# ------------------------------------------------------- (a) the loop, one-launch merge ---------
TAIL_SETS = [{"tail_big_groups": 1}, {"tail_big_groups": 2},
             {"tail_small_groups": 1, "tail_screen_grid": 1},
             {"tail_big_groups": 1, "tail_small_groups": 1, "tail_screen_grid": 1}]


@pytest.mark.parametrize("opts", TAIL_SETS, ids=ids_of(TAIL_SETS))
@pytest.mark.parametrize("d", [64, 32, 16, 8])
def test_loop_one_launch_merge(engine, oracle, d, opts):
    """k_merge_tail with one or two big-run workgroups (one workgroup walks huge -> 896 -> 384 ->
    192 -> 128, every LDS layout after another), one small-run workgroup, a one-wave screen."""
    run_ladder(engine, oracle, d, opts)


@pytest.mark.parametrize("screen", ["tail_big_screen", "tail_screen"])
@pytest.mark.parametrize("opts", TAIL_SETS, ids=ids_of(TAIL_SETS))
@pytest.mark.parametrize("d", [64, 32])
def test_loop_one_launch_merge_without_screens(engine, oracle, d, opts, screen):
    run_ladder(engine, oracle, d, {**opts, screen: 0})


ALL_TAIL = TAIL_SETS[3]


@pytest.mark.parametrize("d", [64, 32, 16, 8])
def test_loop_one_launch_merge_and_projection(engine, oracle, d):
    """The same with the loop's projection on one workgroup."""
    run_ladder(engine, oracle, d, {**ALL_TAIL, **PROJ_1})


@pytest.mark.parametrize("d", [64, 16])
def test_loop_one_launch_merge_nested(engine, oracle, d):
    run_ladder(engine, oracle, d, ALL_TAIL, bthr=NESTED)


@pytest.mark.parametrize("d", [64, 32])
def test_loop_one_launch_merge_special_rows(engine, oracle, d):
    run_ladder(engine, oracle, d, ALL_TAIL, special=True)


# ------------------------------------------------------- (b) the loop, per-class launches -------
def per_class_sets(d):
    sets = [{"grid_cap": 1}, {"grid_cap": 2}, {"small_grid": 1, "small_screen_grid": 1},
            {"grid_cap": 1, "small_grid": 1, "small_screen_grid": 1, **PROJ_1}]
    if d in (13, 100, 512):
        sets += [{"wide_group_grid": 1}, {"grid_cap": 1, "wide_group_grid": 1}]
    if d in (16, 32):  # both of k_merge_long's lists in one workgroup; k_merge_huge
        sets += [{"grid_cap": 1, "long_runs": lr} for lr in (4, 1, 0)]
    if d in (64, 512):  # the 385..896 class, then huge_runs, in the same workgroup
        sets += [{"grid_cap": 1, "huge_fold": 1}]
    if d == 512:
        sets += [{"grid_cap": 1, "wide_group_grid": 1, "wide_gram": g} for g in (8, 0)]
    return [(d, s) for s in sets]


PER_CLASS_CASES = [c for d in LADDER_SHAPES for c in per_class_sets(d)]


@pytest.mark.parametrize("d,opts", PER_CLASS_CASES,
                         ids=[f"d{d} " + i for (d, _), i in
                              zip(PER_CLASS_CASES, ids_of([o for _, o in PER_CLASS_CASES]))])
def test_loop_per_class_launches(engine, oracle, d, opts):
    """k_merge_big / k_merge_big_wide / k_merge_huge / k_merge_long on one or two workgroups,
    k_merge_small and k_small_screen on one wave, the wide-row group merges on one wave."""
    run_ladder(engine, oracle, d, {**PER_CLASS, **opts})


ALL_PER_CLASS = {**PER_CLASS, "grid_cap": 1, "small_grid": 1, "small_screen_grid": 1,
                 "wide_group_grid": 1}


@pytest.mark.parametrize("d", [64, 32, 8, 100, 512])
def test_loop_per_class_launches_nested(engine, oracle, d):
    run_ladder(engine, oracle, d, ALL_PER_CLASS, bthr=NESTED)


@pytest.mark.parametrize("d", [64, 32, 16, 100])
def test_loop_per_class_launches_special_rows(engine, oracle, d):
    run_ladder(engine, oracle, d, ALL_PER_CLASS, special=True)


# ----------------------------------------------------------------------- (c) projection ---------
PROJ_N = 4000  # 15.6 tiles of 256 rows, 20.8 of 192: a partial last tile either way


def hash_case(engine, oracle, d, h, opts, kernel):
    from kmerlsh_amd import _native

    require_projection_trips(d, PROJ_N)
    w, _ = _native.hyperplanes(7 + d, 0, h, d)
    rows = adversarial_rows(np.random.default_rng(11 + d + h), PROJ_N, d, w)
    want = oracle.keys(rows, w)
    with options(engine, **opts):
        got = engine.hash_keys(rows, w)
        assert engine.get_option("last_hash_kernel") == kernel
        close = engine.get_option("last_hash_close_pairs")
    assert np.array_equal(got, want), (d, h, opts)
    assert close > 0
    return rows, w, close


@pytest.mark.parametrize("d,h,segcap", [(64, 23, 0), (32, 18, 0), (16, 9, 0), (64, 23, 3)])
def test_projection_h16_one_workgroup(engine, oracle, d, h, segcap):
    """k_project_h16: one workgroup takes every tile, its fix-up segment collects the close calls
    of all of them; with a segment of 3 entries it overflows across tiles (settled in place)."""
    hash_case(engine, oracle, d, h, {"h16_grid": 1, "h16_segcap": segcap}, 1)


WIDE_SETS = [{"wide_grid": 1}, {"fix_grid": 1}, {"wide_grid": 1, "fix_grid": 1}]
WIDE_CASES = [(d, h, o) for d, h in [(512, 20), (100, 31), (136, 31)] for o in WIDE_SETS]
WIDE_CASES += [(512, 20, {**o, "wide_unrolled": 0}) for o in WIDE_SETS]  # the generic screen


@pytest.mark.parametrize("d,h,opts", WIDE_CASES,
                         ids=[f"d{d} " + i for (d, _, _), i in
                              zip(WIDE_CASES, ids_of([o for _, _, o in WIDE_CASES]))])
def test_projection_wide_one_workgroup(engine, oracle, d, h, opts):
    """k_project_mfma_wide and k_project_fix on one workgroup each."""
    rows, w, close = hash_case(engine, oracle, d, h, opts, 2)
    if "fix_grid" in opts:
        # k_project_fix takes 256 listed pairs a trip.  From the reference: a pair whose exact
        # sum is below 2^-20 T, T = sum |x_k w_k|, cannot be called by the screen — its own sum is
        # within a few 2^-22 T of the exact one (fp16x3 split, f32 accumulation), far inside the
        # bound of wide_eps(d) T >= 2^-15 T — so each is listed
        x, v = rows.astype(np.float64), w.astype(np.float64)
        with np.errstate(all="ignore"):
            s, t = x @ v.T, np.abs(x) @ np.abs(v).T
            sure = int((np.isfinite(t) & (t > 0) & (np.abs(s) < t * 2.0 ** -20)).sum())
        assert sure > 3 * 256, sure
        assert close >= sure, (close, sure)


# --------------------------------------------------------------------------- (d) mode K ---------
# listings of more than 256 * cap records: k_kcount_hi / k_kcount_emit and the table build's
# emit kernels take a second trip (k21: 1007..1065 records a sample, k31: 478..511, sat: 167..172)
LISTING_TRIPS = {("k21", 1), ("k21", 3), ("k31", 1)}


def require_mode_k_trips(c, case, cap, batch_reads=0):
    reads = [len(s) for s in c.info["seqs"]]
    per_batch = min(reads) if not batch_reads else min(min(reads), batch_reads)
    assert per_batch > 4 * cap, (case, reads)  # k_kcount_reads: four waves, a read each, per trip
    # (the hash tables have at least 1024 slots: k_kcount_collect, k_kcount_rehash and
    # k_kmc_collect take four trips or more per workgroup below a grid of 4)
    assert cap < 4
    if (case, cap) in LISTING_TRIPS:
        assert max(len(ls) for ls in c.listings) > 256 * cap, case


def check_mode_k(engine, c, case, out, **kw):
    fx = tk.fixtures()[case]
    st, files, listings, first = tk.count(engine, c, out, **kw)
    assert st["kmap_size"] == fx["kmap"]
    assert files == c.oracle_files()
    tk.assert_listings(c, listings)
    assert np.array_equal(first, np.array(c.oracle("first")[0], np.uint64))
    tk.assert_stats(c, st)
    return st


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("case", ["k21", "sat", "k31"])
def test_mode_k_capped_grids(engine, cases, case, cap, tmp_path):  # noqa: F811
    c = cases(case)
    require_mode_k_trips(c, case, cap)
    with options(engine, grid_cap=cap):
        check_mode_k(engine, c, case, tmp_path)


@pytest.mark.parametrize("case", ["k21", "k31"])
def test_mode_k_capped_grid_table_growth(engine, cases, case, tmp_path):  # noqa: F811
    """Tables that start at 1024 slots and batches of 16 reads: k_kcount_rehash strides over
    several table sizes on one workgroup."""
    c = cases(case)
    require_mode_k_trips(c, case, 1, batch_reads=16)
    # from the model: a table is kept at most half full and never shrinks between samples, so
    # one that starts at 1024 slots has doubled at least ceil(log2(2 m / 1024)) times after a
    # sample of m distinct k-mers
    distinct = [len(tk.kc.count_occurrences(ss, c.k)) for ss in c.info["seqs"]]
    need = max(0, math.ceil(math.log2(2 * max(distinct) / 1024)))
    assert need >= 2, distinct
    with options(engine, grid_cap=1):
        st = check_mode_k(engine, c, case, tmp_path, table_slots=1024, batch_reads=16)
        assert st["rehashes"] >= need, (st["rehashes"], need)
        assert st["batches"] == sum(-(-len(ss) // 16) for ss in c.info["seqs"])


@pytest.mark.parametrize("chunk", [0, 257])
def test_mode_k_databases_capped_grid(engine, db_cases, chunk, tmp_path):  # noqa: F811
    """k_kmcdb_pack (an LDS tile and two barriers per trip, a partial last tile) and k_kmcdb_lut
    on one workgroup: the databases equal the model writer's byte for byte."""
    c = db_cases("k21")
    assert all(n > 512 and n % 256 for n in c.sizes), c.sizes
    p = tdb.kc.PREFIX[c.k]
    assert 4 ** p > 256  # k_kmcdb_lut: 256 prefixes a trip
    with options(engine, grid_cap=1), tdb.db_hooks(engine, prefix=p, chunk=chunk):
        st, dst = engine.count_kmc(c.fastq, c.names(tmp_path), c.k, c.count_min, str(tmp_path))
        assert engine.get_option("kcount_db_prefix_used") == p
    c.assert_dbs(tmp_path, p)
    assert dst["records"] == sum(c.sizes) == st["listed"]
    assert dst["chunks"] == sum(-(-n // (chunk or 1 << 22)) for n in c.sizes)
    assert st["kmap_size"] == tdb.fixtures()["k21"]["kmap"]


# --------------------------------------------------------------------------- (e) mode B ---------
# KMC1 k > 16, KMC2 k > 16, KMC2 k <= 16, KMC1 k <= 16
@pytest.mark.parametrize("case", ["b21", "b31", "e_k12win2", "e_k13win"])
def test_mode_b_capped_grid(engine, dbs, case, tmp_path):  # noqa: F811
    """k_kmc_decode, k_kmc_union, k_kmc_count, k_kmc_collect and the emit kernels on one
    workgroup: the reference's files and the oracle's first-appearance list."""
    _, info, totals = dbs(case)
    version = (tb.ki.CASES.get(case) or tb.ki.EDGE_CASES[case])["version"]
    assert (version, info["k"] > 16) == {"b21": (0, True), "b31": (0x200, True),
                                         "e_k12win2": (0x200, False),
                                         "e_k13win": (0, False)}[case]
    assert min(totals) > 256 and tb.fixtures()[case]["kmap"] > 256, totals
    with options(engine, grid_cap=1):
        tb.check_build(engine, dbs, case, tmp_path)


# --------------------------------------------------------------------------- (f) mode E ---------
@pytest.mark.parametrize("k", [21, 32])
def test_mode_e_capped_grid(engine, k):
    """k_kset_insert and k_check_reads on one workgroup (the inputs of
    test_check_reads_vs_oracle): 256 k-mers and four reads a trip."""
    from kmerlsh_amd import _native

    rng = np.random.default_rng(100 + k)
    src = rng.choice(list(b"ACGT"), size=20000).astype(np.uint8).tobytes()
    kset = np.unique(oe.canonical_kmers(src[:12000], k))
    kset = np.concatenate([kset, rng.integers(0, 2**63, size=500, dtype=np.uint64)])
    reads = te.random_reads(rng, 600, src, k)
    assert len(kset) > 3 * 256 and len(kset) % 256 and len(reads) > 3 * 4
    with options(engine, grid_cap=1):
        ks = _native.KmerSet(engine, kset)
        try:
            for vote in (0.5, 0.0, 0.99):
                hits, flags = ks.check_reads(reads, k, vote)
                oh, of = oe.check_reads(reads, kset, k, vote)
                assert np.array_equal(hits, oh), vote
                assert np.array_equal(flags, of), vote
        finally:
            ks.close()


# -------------------------------------------------------------------------- (g) sharded ---------
def test_sharded_capped_grid(oracle):
    """Two ranks, every iteration sharded, grid_cap = 1 on both: the per-class merges of each
    rank's key range, k_bin_hist, k_delta_pack and k_delta_apply on one workgroup."""
    d, opts = 64, {**PER_CLASS, "grid_cap": 1}
    # the ranks split the buckets between them: more than two runs per class leave one rank
    # with at least two; the histogram and the deltas stride over 256 keys / words a trip
    cnt = class_counts(first_iteration_runs(oracle, d))
    assert all(cnt[c] > 2 for c in BIG_CLASSES), cnt
    data, want = ladder_reference(oracle, LADDER_SHAPES[d], d, BIG)
    min_sim, iters, seed, counter = LADDER_CALL
    states = []
    outs, results = sharded.run_group(2, sharded.ladder_load(data, opts),
                                      [(min_sim, iters, BIG, seed, counter)], states=states)
    for r in range(2):
        what = f"rank {r} of 2, d={d} {opts}"
        assert outs[r][0][2]["world"] == 2
        sharded.assert_same(outs[r], results[r], [(want[3], want[4], None)], want[:3])
        check_state(states[r], results[r][0], results[r][1], what)


def test_grid_cap_option(engine):
    """Settable, readable, [0, 2^20], 0 = off."""
    from kmerlsh_amd import _native

    assert engine.get_option("grid_cap") == 0
    for v in (1, 1 << 20, 0):
        engine.set_option("grid_cap", v)
        assert engine.get_option("grid_cap") == v
    for v in (-1, (1 << 20) + 1):
        with pytest.raises(_native.KlshError):
            engine.set_option("grid_cap", v)
    assert engine.get_option("grid_cap") == 0
