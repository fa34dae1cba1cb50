"""The sharded multi-GPU loop against the single-GPU engine and the reference.

RCCL refuses two ranks on one device, so the sharded path is exercised here through the
in-process group (klsh_comm_init_local): W contexts on the one GPU, each driven by its own host
thread, exchanging through the same Comm interface RCCL implements.  Everything but the
transport is the product code path.  Bar: bit-exact — N_t trace, rng counter, survivor order,
member lists and centroid bits equal the single-GPU call (and the reference's goldens).
"""
import threading

import numpy as np
import pytest

from conftest import golden
from row_state import (LADDER_CALL, LADDER_SHAPES, assert_row_state, check_state, clustered,
                       ladder_reference, options)

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


def run_group(world, load, calls, shard_min_rows=0, states=None):
    """Create `world` engines on device 0, load each with load(eng), bind them into one group,
    run the klsh_cluster calls (list of argument tuples) on every rank concurrently.  Returns
    per-rank lists of (trace, counter, stats) and the per-rank results.  shard_min_rows = 0
    keeps every iteration sharded; larger values switch to the replicated tail below it.
    states (a list): receives every rank's row_state() after the calls — its replica's cached
    nrm, cnt, fp16 image, pad and member links."""
    from kmerlsh_amd import _native

    engines = [_native.Engine(0) for _ in range(world)]
    try:
        for e in engines:
            load(e)
            e.set_option("shard_min_rows", shard_min_rows)
        _native.comm_init_local(engines)
        for r, e in enumerate(engines):
            assert e.comm_info() == (r, world)
        outs = [None] * world
        errs = []

        def work(r):
            try:
                res = []
                counter = None
                for (ms, it, bthr, seed, c0) in calls:
                    c = c0 if counter is None or c0 is not None else counter
                    trace, counter, st = engines[r].cluster(ms, it, bthr, seed, c)
                    res.append((trace, counter, st))
                outs[r] = res
            except Exception as ex:  # surfaced below
                errs.append((r, ex))

        ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=600)
        assert not any(t.is_alive() for t in ts), "sharded call hung"
        assert not errs, errs
        results = [e.result() for e in engines]
        if states is not None:
            states.extend(e.row_state() for e in engines)
        return outs, results
    finally:
        for e in engines:
            e.close()


def single(engine, load, calls):
    load(engine)
    res = []
    counter = None
    for (ms, it, bthr, seed, c0) in calls:
        c = c0 if counter is None or c0 is not None else counter
        trace, counter, st = engine.cluster(ms, it, bthr, seed, c)
        res.append((trace, counter, st))
    return res, engine.result()


def assert_same(a_res, a_out, b_res, b_out):
    for (ta, ca, _), (tb, cb, _) in zip(a_res, b_res):
        assert np.array_equal(ta, tb)
        assert ca == cb
    ra, oa, ia = a_out
    rb, ob, ib = b_out
    assert np.array_equal(oa, ob)
    assert np.array_equal(ia, ib)
    assert same_bits(ra, rb)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["cluster_d16", "cluster_d64", "cluster_d12", "cluster_nested",
                                  "cluster_nested_small"])
def test_sharded_matches_reference(world, name):
    z = golden(name + ".npz")
    calls = [(float(z["min_sim"]), int(z["iters"]), int(z["bthr"]), int(z["seed"]), 0)]
    outs, results = run_group(world, lambda e: e.load_rows(z["rows"]), calls)
    for r in range(world):
        trace, _, st = outs[r][0]
        assert st["world"] == world
        assert np.array_equal(trace, z["trace"]), r
        rows, off, ids = results[r]
        assert np.array_equal(off, z["out_off"]) and np.array_equal(ids, z["out_ids"]), r
        assert same_bits(rows, z["out_rows"]), r


def test_sharded_weighted_matches_reference():
    z = golden("cluster_weighted.npz")
    calls = [(float(z["min_sim"]), int(z["iters"]), int(z["bthr"]), int(z["seed"]), 0)]
    outs, results = run_group(2, lambda e: e.load_rows(z["rows"], z["in_off"], z["in_ids"]), calls)
    for r in range(2):
        assert np.array_equal(outs[r][0][0], z["trace"])
        rows, off, ids = results[r]
        assert np.array_equal(off, z["out_off"]) and np.array_equal(ids, z["out_ids"])
        assert same_bits(rows, z["out_rows"])


@pytest.mark.parametrize("world,n,d,groups,iters,bthr", [
    (2, 200000, 64, 4000, 12, 1000000),
    (4, 200000, 64, 4000, 12, 1000000),
    (3, 100000, 32, 500, 8, 1000000),
    (2, 60000, 20, 300, 6, 1000000),     # generic kernels
    (4, 50000, 16, 3, 3, 5000),          # nested buckets on several ranks every iteration
    (8, 3000, 8, 40, 6, 1000000),        # more ranks than some key ranges have rows
    (2, 6000, 1000, 300, 6, 1000000),    # wide rows past the wide screen's 752 columns
])
def test_sharded_random_vs_single(engine, world, n, d, groups, iters, bthr):
    rng = np.random.default_rng(n + d + world)
    rows = clustered(rng, n, d, groups, 0.05)
    calls = [(0.8, iters, bthr, 777, 3)]
    ref = single(engine, lambda e: e.load_rows(rows), calls)
    outs, results = run_group(world, lambda e: e.load_rows(rows), calls)
    for r in range(world):
        assert_same(outs[r], results[r], *ref)


def test_sharded_negative_min_similarity_vs_single(engine):
    """min_similarity = -0.5: the threshold walks below 0, where the merge decider leaves its fast
    regime (no certified screens) — sharded in every iteration, against the single-GPU call."""
    rng = np.random.default_rng(32 + 2)
    rows = clustered(rng, 20000, 32, 2000, 0.5)
    calls = [(-0.5, 12, 1000000, 777, 3)]
    ref = single(engine, lambda e: e.load_rows(rows), calls)
    trace = ref[0][0][0]
    assert trace[-1] < trace[0]  # it merged
    outs, results = run_group(2, lambda e: e.load_rows(rows), calls)
    for r in range(2):
        assert_same(outs[r], results[r], *ref)


def test_sharded_hip_events_vs_single(engine):
    """Option hip_events on every rank (event pairs around each projection): the same result, and
    every projection launch timed."""
    rng = np.random.default_rng(64 + 2)
    rows = clustered(rng, 60000, 64, 1500, 0.05)
    calls = [(0.8, 10, 1000000, 777, 3)]
    ref = single(engine, lambda e: e.load_rows(rows), calls)

    def load(e):
        e.load_rows(rows)
        e.set_option("hip_events", 1)

    outs, results = run_group(2, load, calls)
    for r in range(2):
        assert_same(outs[r], results[r], *ref)
        st = outs[r][0][2]
        assert st["project_timed_launches"] == st["project_launches"] > 0


@pytest.mark.parametrize("world,switch", [(2, 150000), (3, 120000), (4, 1 << 19)])
def test_sharded_then_replicated_tail_vs_single(engine, world, switch):
    """The crossover: sharded while N_t >= switch, then every rank runs the rest on its replica."""
    rng = np.random.default_rng(world * 7 + 1)
    rows = clustered(rng, 200000, 64, 30000, 0.05)
    calls = [(0.8, 15, 1000000, 777, 3)]
    ref = single(engine, lambda e: e.load_rows(rows), calls)
    assert ref[0][0][0][0] >= switch or switch > 200000  # the run starts sharded unless above n
    outs, results = run_group(world, lambda e: e.load_rows(rows), calls, shard_min_rows=switch)
    for r in range(world):
        assert_same(outs[r], results[r], *ref)


def test_sharded_mode_c_two_calls_vs_single(engine):
    """Init pass + main loop (two calls carrying the rng counter), mode-C rows from synth."""
    from kmerlsh_amd import _native

    n, d = 300000, 64
    counts, cov = _native.synth_counts(n, d, seed=21)
    v_kmers = (cov.astype(np.float32) / np.float32(n)).astype(np.float32)
    calls = [(0.8, 1, 100000, 12345, 0), (0.8, 25, 1000000, 12345, None)]
    ref = single(engine, lambda e: e.load_counts(counts, v_kmers), calls)
    outs, results = run_group(2, lambda e: e.load_counts(counts, v_kmers), calls)
    for r in range(2):
        assert_same(outs[r], results[r], *ref)


def test_sharded_empty_and_single_row():
    calls = [(0.8, 3, 10, 1, 0)]
    outs, _ = run_group(2, lambda e: e.load_rows(np.zeros((0, 8), np.float32)), calls)
    assert [list(o[0][0]) for o in outs] == [[0, 0, 0]] * 2
    outs, res = run_group(3, lambda e: e.load_rows(np.ones((1, 8), np.float32)), calls)
    assert [list(o[0][0]) for o in outs] == [[1, 1, 1]] * 3
    assert all(r[0].shape == (1, 8) for r in res)


def test_rccl_single_rank_group_vs_single(engine):
    """The RCCL backend itself (a one-rank communicator: its allgather, broadcast-based
    allgather-v, all-to-all self copy and min all-reduce) driving the sharded loop."""
    from kmerlsh_amd import _native

    rng = np.random.default_rng(11)
    rows = clustered(rng, 100000, 64, 2000, 0.05)
    calls = [(0.8, 10, 1000000, 5, 0)]
    ref = single(engine, lambda e: e.load_rows(rows), calls)
    eng = _native.Engine(0)
    try:
        eng.load_rows(rows)
        eng.comm_init(0, 1, _native.comm_unique_id())
        eng.set_option("shard_min_rows", 0)
        trace, counter, st = eng.cluster(*calls[0])
        assert st["world"] == 1 and st["comm_ms"] > 0.0
        assert_same([(trace, counter, st)], eng.result(), *ref)
    finally:
        eng.close()


def test_sharded_failure_aborts_the_group():
    """A rank that fails (here: nothing loaded) aborts the group: the other rank's collectives
    return an error instead of waiting for it forever, and the group stays unusable."""
    from kmerlsh_amd import _native

    rng = np.random.default_rng(5)
    rows = clustered(rng, 20000, 16, 500, 0.05)
    engines = [_native.Engine(0) for _ in range(2)]
    try:
        engines[0].load_rows(rows)
        for e in engines:
            e.set_option("shard_min_rows", 0)
        _native.comm_init_local(engines)
        errs = [None, None]

        def work(r):
            try:
                engines[r].cluster(0.8, 5, 1000000, 3, 0)
            except _native.KlshError as ex:
                errs[r] = str(ex)

        ts = [threading.Thread(target=work, args=(r,)) for r in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in ts), "a rank hung after its peer failed"
        assert errs[1] and "before a load" in errs[1]
        assert errs[0] and "abort" in errs[0]
        with pytest.raises(_native.KlshError, match="aborted"):
            engines[0].cluster(0.8, 5, 1000000, 3, 0)
    finally:
        for e in engines:
            e.close()


# ---------------------------------------------------------------------------------------------
# Every merge class's delta listing and the replicas' state.  A sharded merge has two things to
# get right: the merge itself, and listing each slot it rewrote (append_slot / mark_dirty into
# DeltaSink::dlist, written separately in each kernel) — the only way the other ranks' replicas
# learn of it, through k_delta_apply, which is also the only writer of a replica's nrm, cnt, tail
# and fp16 image.  The cases below send runs of every class through the per-class launches (and
# k_merge_tail) at every width, sharded, and read every rank's cached state back.
def ladder_load(data, opts):
    def load(e):
        for k, v in opts.items():  # before the load: "projection" decides whether an image is kept
            e.set_option(k, v)
        e.load_rows(*data)
    return load


_single = {}


def ladder_single(engine, oracle, d, bthr, opts, min_sim=LADDER_CALL[0], special=False):
    """The single-GPU engine under the same options over ladder rows (once per session): its
    trace, counter and result against the oracle, its own row state, and the per-class statistics
    the sharded call does not fill."""
    key = (d, bthr, tuple(sorted(opts.items())), min_sim, special)
    if key not in _single:
        data, want = ladder_reference(oracle, LADDER_SHAPES[d], d, bthr, min_sim, special)
        _, iters, seed, counter = LADDER_CALL
        with options(engine, **opts):
            engine.load_rows(*data)
            trace, c, st = engine.cluster(min_sim, iters, bthr, seed, counter)
            got = engine.result()
            assert np.array_equal(trace, want[3]) and c == want[4]
            assert_same([(trace, c, st)], got, [(want[3], want[4], None)], want[:3])
            assert_row_state(engine, got[0], got[1], f"single GPU d={d} {opts}")
        _single[key] = ([(trace, c, st)], got)
    return _single[key]


def assert_reach(st, d, bthr, opts):
    """From the single-GPU statistics (key-range ownership never splits a bucket, so the ranks
    together walk the same runs): every class the case is there for had runs."""
    k = st["kern"]
    if opts.get("tail_merge_rows") == 1 or d not in (8, 16, 32, 64):  # the per-class launches
        for c in ("big128", "big192", "big384", "big896"):
            assert k[c]["runs"] > 0, c
        if k["screen"]["runs"] > 0:
            # screened iterations count the small runs under "screen" and leave small.runs at 0:
            # k_merge_small's reach is the rows of the runs the screen passed on to it
            assert k["small"]["rows"] > 0
        else:
            assert k["small"]["runs"] > 0
        assert (k["screen"]["launches"] == 0) == (opts.get("small_screen") == 0 or
                                                  opts.get("projection") == 1 or
                                                  d not in (32, 64))  # (its tiles need d >= 32)
    else:
        assert k["tail"]["runs"] > 0
    if bthr >= 1000000:
        assert k["huge"]["runs"] > 0
        assert st["nested_calls"] == 0
    else:
        assert st["nested_calls"] > 0  # runs over bthr: nestedCluster, on the ranks that own them


def check_sharded_ladder(engine, oracle, world, d, bthr, opts, min_sim=LADDER_CALL[0],
                         special=False):
    data, want = ladder_reference(oracle, LADDER_SHAPES[d], d, bthr, min_sim, special)
    ref = ladder_single(engine, oracle, d, bthr, opts, min_sim, special)
    assert_reach(ref[0][0][2], d, bthr, opts)
    _, iters, seed, counter = LADDER_CALL
    states = []
    outs, results = run_group(world, ladder_load(data, opts), [(min_sim, iters, bthr, seed, counter)],
                              states=states)
    for r in range(world):
        what = f"rank {r} of {world}, d={d} bthr={bthr} {opts}"
        assert outs[r][0][2]["world"] == world
        try:
            assert_same(outs[r], results[r], [(want[3], want[4], None)], want[:3])  # the oracle
            assert_same(outs[r], results[r], *ref)                                  # single GPU
        except AssertionError as ex:
            raise AssertionError(f"result differs: {what}") from ex
        check_state(states[r], results[r][0], results[r][1], what)


PER_CLASS = {"tail_merge_rows": 1}
OPTION_SETS = {
    "per_class": PER_CLASS,
    "long0": {**PER_CLASS, "long_runs": 0},
    "long1": {**PER_CLASS, "long_runs": 1},
    "huge_fold": {**PER_CLASS, "huge_fold": 1},
    "no_screen": {**PER_CLASS, "small_screen": 0},
    "packed": {"projection": 1},
    "default": {},
}


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("opts", list(OPTION_SETS))
@pytest.mark.parametrize("d", [64, 32, 16, 8])
def test_sharded_merge_classes_row_state(engine, oracle, d, opts, world):
    check_sharded_ladder(engine, oracle, world, d, 1000000, OPTION_SETS[opts])


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("d,opts", [(512, {"wide_gram": 8}), (512, {"wide_gram": 32}),
                                    (512, {"wide_gram": 0}), (13, {}), (100, {})])
def test_sharded_wide_rows_row_state(engine, oracle, d, opts, world):
    """d = 512 (the Gram group merges), the generic kernels at d = 13 and the chunked ones at 100:
    per-class launches in every iteration."""
    check_sharded_ladder(engine, oracle, world, d, 1000000, opts)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("d", [64, 32, 16, 8, 13, 100, 512])
def test_sharded_nested_row_state(engine, oracle, d, world):
    """bthr = 700: the oversize runs (nested hyperplanes) sit on some ranks and not on others."""
    check_sharded_ladder(engine, oracle, world, d, 700, PER_CLASS if d in (8, 16, 32, 64) else {})


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("d", [64, 32])
def test_sharded_special_rows_row_state(engine, oracle, d, world):
    """NaN, zero, x1e30, x1e-30, x1e5 (inf in the image) and x1e-9 (all-zero image) rows inside
    tight groups: rows the screens hand to the exact chains, and a replica's image of them."""
    check_sharded_ladder(engine, oracle, world, d, 1000000, PER_CLASS, special=True)


def test_sharded_negative_min_similarity_row_state(engine, oracle):
    """min_similarity = -0.5: the later iterations run the plain decider (s* <= 0)."""
    check_sharded_ladder(engine, oracle, 2, 32, 1000000, PER_CLASS, min_sim=-0.5)


# ----------------------------------------------------------------------- key-range edges -----
def check_sharded_vs_single(engine, world, rows, calls, must_merge=True):
    ref = single(engine, lambda e: e.load_rows(rows), calls)
    trace = ref[0][0][0]
    if must_merge:
        assert trace[-1] < trace[0] or ref[1][0].shape[0] < trace[0], list(trace)
    assert_row_state(engine, ref[1][0], ref[1][1], "single GPU")
    states = []
    outs, results = run_group(world, lambda e: e.load_rows(rows), calls, states=states)
    for r in range(world):
        assert_same(outs[r], results[r], *ref)
        check_state(states[r], results[r][0], results[r][1], f"rank {r} of {world}")
    return ref


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("d", [8, 64])
def test_sharded_fewer_bins_than_ranks(engine, d, world):
    """N = 2..17 rows: h = 1..4 hyperplanes, so 2..16 key bins — k_bin_split's branch for fewer
    than 16 bins, fewer bins than ranks, ranks that own nothing.  Two tight groups, so rows
    merge."""
    for n in (2, 3, 7, 15, 16, 17):
        rng = np.random.default_rng(n * 100 + d)
        centers = rng.normal(0, 1, size=(2, d)).astype(np.float32)
        label = np.arange(n) % 2 if n > 2 else np.zeros(n, int)
        rows = (centers[label] + rng.normal(0, 0.01, size=(n, d))).astype(np.float32)
        try:
            check_sharded_vs_single(engine, world, rows, [(0.8, 6, 1000000, 777, 3)])
        except AssertionError as ex:
            raise AssertionError(f"n={n}") from ex


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("bthr", [1000000, 1000])
def test_sharded_one_bin_holds_everything(engine, oracle, bthr, world):
    """3000 identical rows: every key equal, so one rank owns everything and the others receive 0
    pairs; with bthr = 1000 that rank alone runs the nested path."""
    rows = np.tile(np.random.default_rng(16).normal(0, 1, size=(1, 16)).astype(np.float32),
                   (3000, 1))
    calls = [(0.8, 3, bthr, 777, 3)]
    ref = check_sharded_vs_single(engine, world, rows, calls)
    want = oracle.cluster(rows, 0.8, 3, bthr, 777, 3)
    assert_same(*ref, [(want[3], want[4], None)], want[:3])
    assert (ref[0][0][2]["nested_calls"] > 0) == (bthr == 1000)


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_one_bin_holds_nearly_everything(engine, oracle, world):
    """5000 rows: two tight groups whose first-iteration keys differ only in the last (lowest)
    bit — 3900 and 1000 rows in two neighbouring bins — and 100 scattered rows that keep other
    bins non-empty: one rank's range is a single bin with most of the rows."""
    n, d = 5000, 64
    rng = np.random.default_rng(n + d)
    h = int(np.floor(np.log2(n)))
    w, _ = oracle.table(777, 3, h, d)
    a = rng.normal(0, 1, size=d)
    # b: the same side of every hyperplane but the last, the other side of that one
    t = w.astype(np.float64) @ a
    t[-1] = -t[-1]
    b = a + np.linalg.pinv(w.astype(np.float64)) @ (t - w.astype(np.float64) @ a)
    centers = np.stack([a, b])
    label = np.concatenate([np.zeros(3900, int), np.ones(1000, int)])
    rows = np.concatenate([centers[label] + rng.normal(0, 1e-4, size=(4900, d)),
                           rng.normal(0, 1, size=(100, d))]).astype(np.float32)
    rows = rows[rng.permutation(n)]
    keys = oracle.keys(rows, w)
    vals, cnt = np.unique(keys, return_counts=True)
    top = np.sort(cnt)[::-1]
    assert top[0] >= 3800 and top[1] >= 900 and len(vals) > 20
    big = vals[np.argsort(cnt)[::-1][:2]]
    assert int(big[0]) ^ int(big[1]) == 1  # they differ in the lowest bit only
    calls = [(0.8, 4, 1000000, 777, 3)]
    ref = check_sharded_vs_single(engine, world, rows, calls)
    want = oracle.cluster(rows, 0.8, 4, 1000000, 777, 3)
    assert_same(*ref, [(want[3], want[4], None)], want[:3])
