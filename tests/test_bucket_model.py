"""tests/bucket_model.py against brute force, and every builder's claim about what it builds.

The GPU cases of test_gpu_tail_buckets.py are only as good as the model they compare with and the
inputs they name: here the model is checked against a plain Python loop on a few hundred keys,
and each builder against what its case says it holds (bucket sizes, rounds, lists present, totals
below 2^20).  No GPU.
"""
import numpy as np
import pytest

import bucket_model as bm


# ---------------------------------------------------------------------------- brute force -----
def brute_order(keys, n_live, bits):
    """Buckets filled in position order, read in key order (merge_hashtable)."""
    table = {}
    for i in range(n_live):
        table.setdefault(int(keys[i]) & ((1 << bits) - 1), []).append(i)
    return [i for k in sorted(table) for i in table[k]]


def brute_list(b, thr):
    if thr >= 0 and b > thr:
        return 11
    for lst, top in enumerate((2, 4, 8, 16, 32, 64, 128, 192, 384, 896)):
        if b <= top:
            return lst
    return 10


def brute_runs(sorted_keys, thr):
    """(start, length, list) of every run of 2+ equal keys, and the seven counters."""
    runs, ctr, i, n = [], [0] * 7, 0, len(sorted_keys)
    while i < n:
        j = i
        while j < n and sorted_keys[j] == sorted_keys[i]:
            j += 1
        b = j - i
        ctr[0] += 1
        if b >= 2:
            lst = brute_list(b, thr)
            runs.append((i, b, lst))
            if lst < 6:
                ctr[1] += b
            elif lst < 11:
                ctr[2 + lst - 6] += b
        i = j
    return runs, ctr


@pytest.mark.parametrize("thr", [-1, 0, 1, 2, 3, 64, 100])
@pytest.mark.parametrize("n,bits,spread", [(1, 4, 1), (2, 1, 2), (300, 4, 16), (700, 10, 40),
                                           (900, 3, 3), (500, 12, 4096), (1400, 0, 1)])
def test_model_against_brute_force(n, bits, spread, thr):
    rng = np.random.default_rng(n + bits)
    n_live = max(1, n - n // 5)
    live = rng.integers(0, spread, n_live, dtype=np.uint64).astype(np.uint32)
    live &= np.uint32((1 << bits) - 1)
    keys = bm.with_stale_tail(live, n)
    want = bm.expected(keys, n_live, bits, thr)
    order = brute_order(keys, n_live, bits)
    assert list(want["perm"]) == order
    assert list(want["keys"]) == [int(keys[i]) for i in order]
    runs, ctr = brute_runs([int(k) for k in want["keys"]], thr)
    assert list(zip(*(a.tolist() for a in want["runs"]))) == runs
    assert want["counters"].tolist() == ctr
    assert want["runs"][0].dtype == want["runs"][1].dtype == np.uint32
    assert want["runs"][2].dtype == np.int32
    # the vectorised run listing is runs_reference
    for a, b in zip(bm.runs_of(want["keys"], thr), bm.runs_reference(want["keys"], thr)):
        assert np.array_equal(a, b) and a.dtype == b.dtype


def test_list_of_every_length_up_to_1000():
    for thr in (-1, 0, 2, 64, 896, 4096):
        lens = np.arange(2, 1001)
        assert bm.list_of(lens, thr).tolist() == [brute_list(int(b), thr) for b in lens]
    assert [brute_list(b, -1) for b in bm.LIST_MIN_ROWS] == list(range(11))
    assert [brute_list(b - 1, -1) for b in bm.LIST_MIN_ROWS[1:]] == list(range(10))


def test_stale_tail_is_never_a_live_key():
    keys = bm.with_stale_tail(np.zeros(3, np.uint32), (1 << 20) - 1)
    assert keys.size == (1 << 20) - 1 and keys.dtype == np.uint32
    assert keys[3] == 0xFFFFFFFF - 3 and keys[-1] == 0xFFFFFFFF - ((1 << 20) - 2)
    assert int(keys[3:].min()) >= 1 << 31 and not np.any(keys[3:] == bm.DIRTY)
    assert np.unique(keys[3:]).size == keys.size - 3


# ------------------------------------------------------------------------ builders' claims ----
@pytest.mark.parametrize("lb", [1, 5, 10])
@pytest.mark.parametrize("top", [0, 1, 255, 511])
def test_one_top_bucket(top, lb):
    bits = bm.TOP_BITS + lb
    for m in (1, 2, 255, 256, 257, 4097, 70000):
        keys = bm.one_top_bucket(top, lb, m, m)
        assert keys.size == m and keys.dtype == np.uint32 and int(keys.max()) < 1 << bits
        sizes = bm.top_sizes(keys, bits)
        assert sizes[top] == m and sizes.sum() == m
        if m >= 70000:
            assert np.unique(keys & np.uint32((1 << lb) - 1)).size == 1 << lb
    assert [bm.rounds(m) for m in (1, 4095, 4096, 4097, 8192, 8193, 12289, 70000)] == \
        [1, 1, 1, 2, 2, 3, 4, 18]
    assert [bm.lanes_j(m) for m in (1, 256, 257, 3840, 3841, 4096, 70000)] == [1, 1, 2, 15, 16, 16, 16]
    assert bm.rounds((1 << 20) - 1) == 256 and bm.rounds(300_000) == 74


def test_dealt_sizes():
    sizes, where, special = bm.dealt_sizes()
    assert sizes.size == 512 and len(special) == 55 and np.unique(special).size == 55
    assert sizes[where].tolist() == special.tolist()
    for j in range(1, 17):
        assert {256 * j - 1, 256 * j, 256 * j + 1} <= set(special.tolist())
    assert {0, 1, 2, 3, 63, 64, 65} <= set(special.tolist())
    big = int(np.argmax(sizes))
    assert sizes[big] == 4097 and sizes[big - 1] == 0 and sizes[big + 1] == 0
    assert sizes[0] == 0 and sizes[511] == 0
    rest = np.ones(512, bool)
    rest[where] = False
    rest[[0, 511, big - 1, big + 1]] = False
    assert set(sizes[rest & (np.arange(512) % 2 == 0)]) == {0}
    assert set(sizes[rest & (np.arange(512) % 2 == 1)]) == {1, 2, 3}
    # an empty bucket and a full one next to each other, both ways round
    pairs = set(zip(sizes[:-1] > 0, sizes[1:] > 0))
    assert (True, False) in pairs and (False, True) in pairs
    assert {bm.lanes_j(m) for m in special if m} == set(range(1, 17))
    assert {bm.rounds(m) for m in special if m} == {1, 2}
    assert sizes.sum() < 1 << 20


@pytest.mark.parametrize("bits", [10, 14, 19])
def test_dealt_keys(bits):
    keys = bm.dealt(bits, bits)
    sizes, _, _ = bm.dealt_sizes()
    assert keys.dtype == np.uint32 and int(keys.max()) < 1 << bits
    assert np.array_equal(bm.top_sizes(keys, bits), sizes)
    assert np.any(np.diff(keys.astype(np.int64)) < 0)  # shuffled: stability has work to do


@pytest.mark.parametrize("lb", [6, 10])
def test_lane_patterns(lb):
    rad, m, bits = 1 << lb, 3 * bm.ROUND + 77, bm.TOP_BITS + lb
    assert bm.rounds(m) == 4
    low = {}
    for kind in bm.LANE_PATTERNS:
        keys = bm.lane_pattern(kind, lb, m)
        assert keys.size == m and int(keys.max()) < 1 << bits
        assert bm.top_sizes(keys, bits)[5] == m
        low[kind] = (keys & np.uint32(rad - 1)).astype(np.int64)
    for r in range(0, m - rad, rad):   # each digit once per RAD positions
        assert np.unique(low["ramp"][r:r + rad]).size == rad
    waves = low["wave_ramp"][:m - m % 64].reshape(-1, 64)
    assert np.all(waves == waves[:, :1]) and np.all(np.diff(waves[:rad, 0]) == 1)
    blocks = [np.unique(low["round_blocks"][r:r + bm.ROUND]) for r in range(0, m, bm.ROUND)]
    assert all(b.size == 1 for b in blocks) and len({int(b[0]) for b in blocks}) == 4
    alt = low["alternate"]
    assert set(alt[0::2]) == {1} and set(alt[1::2]) == {rad - 2} and rad - 2 != 1


@pytest.mark.parametrize("thr", [-1, 0, 2, 64, 896, 4096])
@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("bits", [14, 19])
def test_class_edges(bits, spread, thr):
    keys, counts = bm.class_edges(bits, thr, spread, thr + 5)
    assert set(bm.CLASS_EDGES) <= set(counts)
    if thr >= 1:
        assert counts[-2:] == [thr, thr + 1]
    elif thr == 0:
        assert counts[-1] == 1 and len(counts) == len(bm.CLASS_EDGES) + 1
    assert keys.size == sum(counts) < 1 << 20 and int(keys.max()) < 1 << bits
    assert sorted(bm.run_lengths(keys).tolist()) == sorted(counts)
    tops = np.flatnonzero(bm.top_sizes(keys, bits))
    assert tops.size == (len(counts) if spread else 1)
    want = set(range(11)) if thr < 0 else {l for l in range(11) if bm.LIST_MIN_ROWS[l] <= thr}
    if thr >= 0:
        want.add(11)
    assert bm.lists_present(keys, thr) == want


@pytest.mark.parametrize("lst,rows", list(enumerate(bm.LIST_MIN_ROWS)))
def test_worst_case_list(lst, rows):
    keys = bm.worst_case_list(rows, lst)
    n = keys.size
    assert n % rows == 0 and n < 200_000 <= n + rows and int(keys.max()) < 1 << 17
    lens = bm.run_lengths(keys)
    assert lens.size == n // rows and set(lens.tolist()) == {rows}
    assert bm.lists_present(keys, -1) == {lst}
    # the list holds n / rows entries: all its capacity formula gives for n positions
    assert bm.list_capacity(lst, n) - 64 == n // rows


def test_list_capacity_is_the_engines():
    s = 200_000
    assert [bm.list_capacity(c, s) for c in range(6)] == [s // ((1 << c) + 1) + 64 for c in range(6)]
    assert [bm.list_capacity(l, s) for l in (6, 7, 8, 9, 10, 11)] == \
        [s // 65 + 64, s // 129 + 64, s // 193 + 64, s // 385 + 64, s // 897 + 64, s + 64]


@pytest.mark.parametrize("narrow", [True, False])
@pytest.mark.parametrize("n_max,n_live", bm.N_DEV_SHAPES)
def test_below_the_bound(n_max, n_live, narrow):
    keys, bits = bm.below_the_bound(n_max, n_live, narrow, n_live)
    assert keys.size == n_max < 1 << 20 and 1 <= n_live <= n_max and bits == bm.floor_log2(n_max)
    live_bits = bm.floor_log2(n_live) if narrow else bits
    assert int(keys[:n_live].max()) < 1 << live_bits
    assert np.array_equal(keys[n_live:], 0xFFFFFFFF - np.arange(n_live, n_max, dtype=np.int64))
    if bm.local_ok(bits) and narrow and n_live > 1:
        # the top digit of the sort uses only a few of its 512 values
        used = np.flatnonzero(bm.top_sizes(keys[:n_live], bits)).size
        assert used <= max(1, 512 >> (bits - live_bits))
    if n_live == 1:
        assert keys[0] == 0 or not narrow


def test_uniform_widths():
    for bits in range(20):
        keys = bm.uniform(5000, bits, bits)
        assert keys.dtype == np.uint32 and int(keys.max()) < 1 << bits
        if 1 <= bits <= 8:   # (5000 draws: every value of a narrow key turns up)
            assert np.unique(keys).size == 1 << bits
    assert bm.uniform((1 << 19) + 1, 19, 1).size < 1 << 20
    assert [bm.local_ok(b) for b in (0, 9, 10, 19, 20)] == [False, False, True, True, False]
