"""One queued iteration's bucket sort and run listing on chosen keys (klsh_tail_buckets).

Below 2^20 rows run_batched queues whole iterations: every kernel is launched for an upper bound
n_max and reads the real row count from a device word, and the stable bucket order with its run
lists comes from the top-9-bit partition + k_tail_local (path 1, keys of 10..19 bits) or from the
LSD passes + k_runs_count / k_runs_write<true> (path 0).  Whole clustering loops reach both only
with whatever keys LSH makes of Gaussian rows.  Here the keys are dealt by hand
(tests/bucket_model.py, whose claims tests/test_bucket_model.py checks without a GPU) and every
workspace starts dirty (the byte 0xA5), as it is in the loop.  DESIGN.md §3.4.

Every case states what its input holds before the engine runs, then for each path compares, by
bits: the permutation and the sorted keys of the live prefix with the model's stable order; every
entry at or past n_live with 0xA5A5A5A5 or the input at that position; the runs with their lists
and the seven run counters with the model's; and the two paths with each other.
"""
import numpy as np
import pytest

import bucket_model as bm
from row_state import check, clustered

pytestmark = pytest.mark.gpu


def sort_and_list(engine, keys, n_live, bits, bthr, what):
    """Both paths where the local one takes `bits`, path 0 alone elsewhere, against the model."""
    n_max = keys.size
    assert 1 <= n_live <= n_max < 1 << 20 and 0 <= bits <= 19
    assert bits == 0 and not keys[:n_live].any() or int(keys[:n_live].max()) < 1 << bits, what
    want = bm.expected(keys, n_live, bits, bthr)
    at = np.arange(n_live, n_max, dtype=np.uint32)
    got = {}
    for path in ((1, 0) if bm.local_ok(bits) else (0,)):
        ok, op, runs, ctr = engine.tail_buckets(keys, n_live, bits, bthr, path)
        tag = f"{what} path={path}"
        assert np.array_equal(op[:n_live], want["perm"]), tag
        assert np.array_equal(ok[:n_live], want["keys"]), tag
        # stale keys are neither counted, moved nor written over
        assert np.all((ok[n_live:] == bm.DIRTY) | (ok[n_live:] == keys[n_live:])), tag
        assert np.all((op[n_live:] == bm.DIRTY) | (op[n_live:] == at)), tag
        for name, g, w in zip(("starts", "lengths", "lists"), runs, want["runs"]):
            assert np.array_equal(g, w), f"{tag}: run {name}"
        assert ctr.tolist() == want["counters"].tolist(), f"{tag}: counters {ctr} {want['counters']}"
        got[path] = (ok[:n_live], op[:n_live]) + runs + (ctr,)
    if len(got) == 2:
        for a, b in zip(got[0], got[1]):
            assert np.array_equal(a, b), what
    return want


# ------------------------------------------------------------------------------ a: widths -----
@pytest.mark.parametrize("bits", range(20))
def test_every_width(engine, bits):
    """5000 uniform keys (two tiles) and 2^bits + 1 keys (every key value about once, one of
    them twice at least) at every key width: path 1 at 10..19 bits (lb = 1..10), path 0 at
    P = 1 and 2 passes of B = 8, 9 and 10 bits, and no pass at all for 0 bits."""
    for n in (5000, (1 << bits) + 1):
        assert n < 1 << 20
        keys = bm.uniform(n, bits, 100 * bits + (n == 5000))
        want = sort_and_list(engine, keys, n, bits, -1, f"bits={bits} n={n}")
        assert want["counters"][0] <= min(n, 1 << bits) and len(want["runs"][0]) >= 1


# ---------------------------------------------------- b: one top bucket holds everything -----
ONE_BUCKET_M = (1, 2, 255, 256, 257, 3840, 3841, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 70000)


@pytest.mark.parametrize("lb", [1, 5, 10])
@pytest.mark.parametrize("top", [0, 1, 255, 511])
def test_one_top_bucket_holds_everything(engine, top, lb):
    """All m keys in one of the 512 top buckets (the first two, a middle one, the last: `base` is
    0 or everything before), 511 workgroups with nothing to do: m at J = 1 | 2 and 15 | 16 keys
    per lane and either side of one, two and three 4096-key rounds (the run_[] carry, the reload
    branch), 18 rounds at 70000.  lb = 1: two digits, runs of m / 2; lb = 10: RAD = 1024, four
    digits per thread."""
    bits = bm.TOP_BITS + lb
    assert [bm.rounds(m) for m in ONE_BUCKET_M] == [1] * 9 + [2, 2, 2, 3, 4, 18]
    assert [bm.lanes_j(m) for m in ONE_BUCKET_M[:7]] == [1, 1, 1, 1, 2, 15, 16]
    for m in ONE_BUCKET_M:
        keys = bm.one_top_bucket(top, lb, m, 1000 * top + m)
        sizes = bm.top_sizes(keys, bits)
        assert sizes[top] == m and np.count_nonzero(sizes) == 1
        sort_and_list(engine, keys, m, bits, -1, f"top={top} lb={lb} m={m}")


@pytest.mark.parametrize("bthr,lst", [(-1, bm.HUGE_LIST), (100_000, bm.OVER_LIST)])
def test_all_keys_equal(engine, bthr, lst):
    """300 000 equal keys: one top bucket, one digit, 74 rounds in which all 64 lanes of every
    wave rank on that digit (the ballot rank, wc[wv][dig] read before its leader writes it) —
    one run, in the huge list or, over the threshold, in the oversize list."""
    n, bits = 300_000, 19
    keys = np.full(n, (255 << 10) | 0x2A5, np.uint32)
    assert bm.rounds(n) == 74 and bm.run_lengths(keys).tolist() == [n]
    want = sort_and_list(engine, keys, n, bits, bthr, f"all equal bthr={bthr}")
    assert want["runs"][2].tolist() == [lst]
    assert want["counters"].tolist() == [1, 0, 0, 0, 0, 0, n if lst == bm.HUGE_LIST else 0]


# ---------------------------------------------------------- c: bucket sizes dealt by hand -----
@pytest.mark.parametrize("bits", [10, 14, 19])
def test_bucket_sizes_dealt_by_hand(engine, bits):
    """Top bucket sizes 0, 1, 2, 3, 63, 64, 65 and 256 J - 1, 256 J, 256 J + 1 for J = 1..16
    once each, the other buckets empty or of 1..3 keys in turn, empty ones at both ends and on
    both sides of the largest: every J at its edges, and the `base` prefix over dtot with empty
    buckets next to full ones."""
    keys = bm.dealt(bits, bits)
    sizes, where, special = bm.dealt_sizes()
    assert np.array_equal(bm.top_sizes(keys, bits), sizes) and keys.size < 1 << 20
    big = int(np.argmax(sizes))
    assert sizes[big] == 4097 and not sizes[[0, 511, big - 1, big + 1]].any()
    assert {bm.lanes_j(m) for m in special if m} == set(range(1, 17))
    sort_and_list(engine, keys, keys.size, bits, -1, f"dealt bits={bits}")


# ---------------------------------------------------------------------- d: lane patterns -----
@pytest.mark.parametrize("kind", bm.LANE_PATTERNS)
@pytest.mark.parametrize("lb", [6, 10])
def test_lane_patterns(engine, lb, kind):
    """Unshuffled keys of one top bucket over four rounds, the low digit a function of the
    position: each digit once per RAD positions (every ballot group is one lane), one digit per
    64 consecutive positions (every group is the whole wave), one digit per 4096-key round
    (cnt[] + run_[] is the whole offset), two digits alternating from lane to lane."""
    m, bits, rad = 3 * bm.ROUND + 77, bm.TOP_BITS + lb, 1 << lb
    keys = bm.lane_pattern(kind, lb, m)
    low = (keys & np.uint32(rad - 1)).astype(np.int64)
    assert bm.rounds(m) == 4 and bm.top_sizes(keys, bits)[5] == m
    if kind == "ramp":
        assert np.array_equal(low, np.arange(m) % rad)
    elif kind == "wave_ramp":
        assert np.array_equal(low, (np.arange(m) // 64) % rad)
    elif kind == "round_blocks":
        assert np.unique(low).size == 4 and np.unique(low[:bm.ROUND]).size == 1
    else:
        assert np.unique(low).size == 2 and np.all(low[:-1] != low[1:])
    sort_and_list(engine, keys, m, bits, -1, f"{kind} lb={lb}")


# ------------------------------------------------------------------- e: run-class edges ------
@pytest.mark.parametrize("bthr", [-1, 0, 2, 64, 896, 4096])
@pytest.mark.parametrize("spread", [False, True])
def test_run_class_edges(engine, spread, bthr):
    """Digit counts exactly 1, 2, 3|4|5, 8|9, 16|17, 32|33, 64|65, 128|129, 192|193, 384|385,
    896|897 and bthr | bthr + 1, in one top bucket (the counts of one workgroup, one add per list)
    and one per top bucket (23 workgroups adding to the same counters): every list that the
    threshold leaves, and the oversize list for the rest."""
    for bits in (14, 19):
        keys, counts = bm.class_edges(bits, bthr, spread, bthr + 5)
        assert sorted(bm.run_lengths(keys).tolist()) == sorted(counts)
        assert set(bm.CLASS_EDGES) <= set(counts)
        if bthr >= 1:
            assert {bthr, bthr + 1} <= set(counts)
        assert np.count_nonzero(bm.top_sizes(keys, bits)) == (len(counts) if spread else 1)
        lists = set(range(11)) if bthr < 0 else {l for l in range(11) if bm.LIST_MIN_ROWS[l] <= bthr}
        assert bm.lists_present(keys, bthr) == (lists | {bm.OVER_LIST} if bthr >= 0 else lists)
        sort_and_list(engine, keys, keys.size, bits, bthr, f"edges bits={bits} bthr={bthr} {spread}")


# ----------------------------------------------------------------- f: worst-case lists -------
@pytest.mark.parametrize("lst,rows", list(enumerate(bm.LIST_MIN_ROWS)))
def test_worst_case_lists(engine, lst, rows):
    """Every run has the smallest length of its list, n just below 200 000 at 17 bits: the list
    holds n / rows entries, all that its capacity formula gives for n positions (+ 64)."""
    keys = bm.worst_case_list(rows, lst)
    n = keys.size
    assert n % rows == 0 and n + rows >= 200_000 > n
    assert set(bm.run_lengths(keys).tolist()) == {rows} and bm.lists_present(keys, -1) == {lst}
    assert bm.list_capacity(lst, n) - 64 == n // rows
    want = sort_and_list(engine, keys, n, 17, -1, f"worst case list {lst}")
    assert len(want["runs"][0]) == n // rows and set(want["runs"][2].tolist()) == {lst}


# ------------------------------------------------------ g: device count below the bound ------
@pytest.mark.parametrize("narrow", [True, False])
@pytest.mark.parametrize("n_max,n_live", bm.N_DEV_SHAPES)
def test_device_count_below_the_bound(engine, n_max, n_live, narrow):
    """Grids, tiles and the sort's passes for n_max, the count n_live on the device, a stale tail
    behind the live keys.  narrow: live keys of floor(log2 n_live) bits sorted with
    hb = floor(log2 n_max), as a chunk sized from an older N sorts them — the top digit uses a few
    of its 512 values, one at n_live = 1; otherwise keys of all hb bits."""
    keys, bits = bm.below_the_bound(n_max, n_live, narrow, n_max % 1000 + n_live)
    assert keys.size == n_max and bits == bm.floor_log2(n_max) and bm.local_ok(bits)
    assert int(keys[n_live:].min()) >= 1 << 31  # stale: never a live key, never 0xA5A5A5A5
    assert not np.any(keys[n_live:] == bm.DIRTY)
    if narrow:
        assert int(keys[:n_live].max()) < 1 << bm.floor_log2(n_live)
        used = np.count_nonzero(bm.top_sizes(keys[:n_live], bits))
        assert used <= max(1, 512 >> (bits - bm.floor_log2(n_live)))
    sort_and_list(engine, keys, n_live, bits, -1, f"n_max={n_max} n_live={n_live} narrow={narrow}")


# ------------------------------------------------------------- h: several calls in a row -----
def test_calls_of_different_shapes_in_a_row(engine, oracle):
    """Calls of different sizes, widths, thresholds and live counts on one context, then the
    engine's own state: a klsh_bucket_sort and a small klsh_cluster against the oracle."""
    shapes = [(300_000, 300_000, 19, -1), (4097, 1, 12, -1), (70_000, 1100, 16, 64),
              (1, 1, 10, -1), ((1 << 20) - 1, 600_000, 19, 2), (5000, 4097, 9, -1),
              (12_289, 12_289, 13, 896), (2, 2, 0, -1)]
    for i, (n_max, n_live, bits, bthr) in enumerate(shapes):
        keys = bm.with_stale_tail(bm.uniform(n_live, bits, i), n_max)
        sort_and_list(engine, keys, n_live, bits, bthr, f"call {i} {shapes[i]}")
    keys = bm.uniform(100_000, 17, 99)
    sk, perm = engine.bucket_sort(keys, 17)
    want = np.argsort(keys, kind="stable").astype(np.uint32)
    assert np.array_equal(perm, want) and np.array_equal(sk, keys[want])
    rows = clustered(np.random.default_rng(8), 3000, 16, 400, 0.05)
    res = oracle.cluster(rows, 0.8, 8, 1000000, 41, 9)
    assert res[0].shape[0] < 3000
    engine.load_rows(rows)
    trace, counter, _ = engine.cluster(0.8, 8, 1000000, 41, 9)
    assert np.array_equal(trace, res[3]) and counter == res[4]
    assert engine.get_option("tail_local_iters") == 8  # one chunk sized from 3000 rows: hb = 11
    check(engine, res, "after klsh_tail_buckets calls")
