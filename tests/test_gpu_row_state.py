"""The row state every writer leaves behind: nrm, cnt, the fp16 image, tail, the zero pad.

The parity tests compare what klsh_result returns.  Inside one klsh_pcluster call the kernels
keep the norm in registers, so a wrong value written back to `nrm`, a stale fp16 image or a lost
`tail` changes no result bit of that call — only a later decision that happens to sit within
the error.  Every case here still compares the result with the oracle, and then reads the cached
state back (klsh_row_state) and compares it by bits with what the returned rows and offsets say
it must be (tests/row_state.py).  Weighted input (cnt > 1 at load) throughout, so a consensus
that took its weights from a stale `cnt` shows in the rows as well.
"""
import numpy as np
import pytest

import row_state
from row_state import (LADDER_CALL, LADDER_SHAPES, assert_row_state, check, ladder_reference,
                       options, same_state, spread_cached)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------ shapes ---------
SMALL_B = [2, 3, 5, 9, 17, 33, 64]
BIG_B = [65, 128, 129, 192, 193, 384, 385, 896]
SHAPES = ([(b, d) for d in (8, 16, 32, 64, 13, 512) for b in SMALL_B] +
          [(b, d) for d in (16, 32, 64) for b in BIG_B] +
          [(897, 32), (1537, 16), (4097, 32), (1200, 64), (1000, 8)] +
          [(40, 13), (300, 130), (1000, 70), (100, 512), (1200, 512)])
# two-pass only: survivor counts of the first pass (about 0.55 b) in the classes the table above
# leaves out of a kernel family — 129..192 everywhere, over 896 at d = 64, and 65..128, 193..384
# and over 896 for the wide rows
EXTRA_TWO_PASS = [(300, 64), (300, 32), (300, 16), (1800, 64), (200, 100), (500, 130), (1800, 70)]
TWO_PASS = [s for s in SHAPES if s[0] >= 9] + EXTRA_TWO_PASS


def option_sets(b, d):
    """The default, the per-class launches, and every option that selects another kernel for a
    run of b rows of width d."""
    sets = [{}, {"tail_merge_rows": 1}]
    image = d in (16, 32, 64)
    if image:
        sets += [{"projection": 1}, {"projection": 1, "tail_merge_rows": 1}]
        if b <= 64:
            sets += [{"small_screen": 0}, {"small_screen": 0, "tail_merge_rows": 1},
                     {"tail_screen": 0}]
        elif b <= 384:
            sets += [{"tail_big_screen": 0}]
    if d in (16, 32) and b >= 385:
        for lr in (4, 1, 0):
            sets += [{"long_runs": lr}, {"long_runs": lr, "tail_merge_rows": 1}]
    if b > 896:
        sets += [{"huge_fold": 1, "tail_merge_rows": 1}]
        if d in (16, 32):
            sets += [{"huge_fold": 1, "tail_merge_rows": 1, "long_runs": lr} for lr in (1, 0)]
    if d == 512:
        sets += [{"wide_gram": g} for g in (8, 32, 0)]
    return sets


_oracle_cache = {}


def pcluster_reference(oracle, b, d, thr, unit=False):
    """oracle.pcluster of spread(b, d) — weighted, or with unit weights — once per session."""
    key = (b, d, thr, unit)
    if key not in _oracle_cache:
        rows, off, ids = spread_cached(b, d)
        _oracle_cache[key] = oracle.pcluster(rows, thr) if unit else \
            oracle.pcluster(rows, thr, off, ids)
    return _oracle_cache[key]


# ---------------------------------------------------------------- (a) one weighted pass --------
@pytest.mark.parametrize("b,d", SHAPES)
def test_pcluster_weighted_row_state(engine, oracle, b, d):
    """One klsh_pcluster(0.9) over weighted rows on every merge path that takes a run of b rows:
    the result against the oracle, then the state each path wrote back."""
    rows, off, ids = spread_cached(b, d)
    want = pcluster_reference(oracle, b, d, 0.9)
    for opts in option_sets(b, d):
        with options(engine, **opts):
            engine.load_rows(rows, off, ids)
            engine.pcluster(0.9)
            check(engine, want, f"b={b} d={d} {opts}")


@pytest.mark.parametrize("b,d", SHAPES)
def test_pcluster_plain_decider_row_state(engine, oracle, b, d):
    """The same table with unit weights at thr = 0.0: the plain decider, where the certified
    screens stand aside and other branches of each kernel do the write-back."""
    rows, _, _ = spread_cached(b, d)
    want = pcluster_reference(oracle, b, d, 0.0, unit=True)
    for opts in option_sets(b, d):
        with options(engine, **opts):
            engine.load_rows(rows)
            engine.pcluster(0.0)
            check(engine, want, f"b={b} d={d} thr=0 {opts}")


# --------------------------------------------------------------------- (b) two passes ----------
def two_pass_reference(oracle, b, d):
    key = (b, d, "two")
    if key not in _oracle_cache:
        first = pcluster_reference(oracle, b, d, 0.95)
        second = oracle.pcluster(first[0], 0.85, first[1], first[2])
        _oracle_cache[key] = (first, second)
    return _oracle_cache[key]


@pytest.mark.parametrize("b,d", TWO_PASS)
def test_pcluster_two_passes_row_state(engine, oracle, b, d):
    """klsh_pcluster(0.95), then klsh_pcluster(0.85) on its survivors: the second pass computes
    with the nrm, cnt, tail and image the first one wrote back.  Both passes must merge (asserted
    from the oracle alone), or the second would prove nothing about the first's state."""
    rows, off, ids = spread_cached(b, d)
    first, second = two_pass_reference(oracle, b, d)
    s1, s2 = first[0].shape[0], second[0].shape[0]
    assert s1 < b and s2 < s1, (b, d, s1, s2)
    sets = option_sets(b, d)
    sets += [o for o in option_sets(s1, d) if o not in sets]  # the second pass's run has s1 rows
    for opts in sets:
        with options(engine, **opts):
            engine.load_rows(rows, off, ids)
            engine.pcluster(0.95)
            check(engine, first, f"b={b} d={d} pass 1 (s1={s1}) {opts}")
            engine.pcluster(0.85)
            check(engine, second, f"b={b} d={d} pass 2 (s1={s1} s2={s2}) {opts}")


def run_class(n):
    return next(i for i, hi in enumerate([64, 128, 192, 384, 896, 1 << 62]) if n <= hi)


def test_two_pass_second_runs_cover_every_class(oracle):
    """The second pass's run length is the first pass's survivor count s1: over the two-pass
    shapes it falls in every run class (2..64, 65..128, 129..192, 193..384, 385..896, longer) at
    least once per kernel family — d = 64, d = 16 / 32, wide rows."""
    family = {64: "d64", 16: "d16_32", 32: "d16_32"}
    seen = {"d64": set(), "d16_32": set(), "wide": set()}
    for b, d in TWO_PASS:
        if d == 8:
            continue
        s1 = two_pass_reference(oracle, b, d)[0][0].shape[0]
        seen[family.get(d, "wide")].add(run_class(s1))
    for fam, classes in seen.items():
        assert classes == set(range(6)), (fam, sorted(classes))


# ----------------------------------------------------------------------------- (c) loops -------
@pytest.mark.parametrize("opts", [{}, {"tail_merge_rows": 1}, {"tail_batch": 0}],
                         ids=["default", "per_class", "no_tail_batch"])
@pytest.mark.parametrize("bthr", [1000000, 700])
@pytest.mark.parametrize("d", [64, 32, 16, 8, 13, 100, 512])
def test_cluster_loop_row_state(engine, oracle, d, bthr, opts):
    """Six iterations over weighted ladder rows (runs of every class in the first iteration, a
    trace that keeps falling; bthr = 700: nested hyperplanes on the oversize runs): the state the
    loop leaves for the next call."""
    n = LADDER_SHAPES[d]
    (rows, off, ids), want = ladder_reference(oracle, n, d, bthr)
    min_sim, iters, seed, counter = LADDER_CALL
    with options(engine, **opts):
        engine.load_rows(rows, off, ids)
        trace, c, _ = engine.cluster(min_sim, iters, bthr, seed, counter)
        assert np.array_equal(trace, want[3]) and c == want[4]
        assert trace[-1] < trace[0]
        check(engine, want, f"ladder n={n} d={d} bthr={bthr} {opts}")


# ------------------------------------------------------------------- (d) the other writers -----
def special_rows(d):
    """Rows a writer can get wrong: NaN, +-0, past fp32's square range, below it, past fp16's
    range (inf in the image), fp16-subnormal scale, and the fp16 rounding edges."""
    rng = np.random.default_rng(1000 + d)
    rows = rng.normal(0, 1, size=(300, d)).astype(np.float32)
    rows[3, 1] = np.nan
    rows[4] = 0.0
    rows[5] = -0.0
    rows[6, ::2] = -0.0
    rows[7] *= np.float32(1e30)
    rows[8] *= np.float32(1e-30)
    rows[9, 2] = np.float32(7e4)
    rows[10] *= np.float32(1e5)
    rows[11] *= np.float32(1e-6)      # fp16 subnormals (below 6.1e-5)
    rows[12] *= np.float32(3e-8)      # around half of fp16's smallest subnormal (5.96e-8)
    rows[13] *= np.float32(1e-9)      # all-zero image of a nonzero row
    rows[14, :4] = [65504.0, 65519.996, 65520.0, -65520.0]   # the last finite fp16 / first inf
    rows[15, :4] = [2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -14]  # subnormal ties
    rows[16, :4] = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), np.inf]  # ties
    return rows


@pytest.mark.parametrize("d", [64, 32, 16, 8, 13, 100, 512])
@pytest.mark.parametrize("weighted", [False, True])
def test_load_rows_row_state(engine, d, weighted):
    """k_norms and k_shadow_build straight after a load, special rows included."""
    rows = special_rows(d)
    off, ids = row_state.weights(np.random.default_rng(d), rows.shape[0], 301)
    if weighted:
        engine.load_rows(rows, off, ids)
    else:
        engine.load_rows(rows)
        off, ids = np.arange(rows.shape[0] + 1, dtype=np.uint64), np.arange(rows.shape[0])
    st = check(engine, (rows, off, ids), f"load d={d} weighted={weighted}")
    assert (st["image"] is not None) == (d in (16, 32, 64))


@pytest.mark.parametrize("d", [13, 32, 64])
def test_load_counts_row_state(engine, oracle, d):
    """k_convert (mode C) on a batch that starts inside the matrix and is no multiple of 256, with
    rows on either side of the keep / drop edge sum(count) > 0.1 d and counts of 0 and 65535."""
    rng = np.random.default_rng(d)
    n_total, batch_offset, batch_size = 2000, 333, 1111
    counts = rng.poisson(3.0, size=(d, n_total)).astype(np.uint16)
    counts[:, rng.integers(0, n_total, 300)] = 0          # dropped rows
    edge = int(np.floor(0.1 * d))                         # sum == edge drops, edge + 1 keeps
    for k, total in enumerate([edge, edge + 1, max(edge - 1, 0), edge + 2, 0]):
        col = batch_offset + 10 + k
        counts[:, col] = 0
        counts[:total, col] = 1
    counts[:, batch_offset] = 65535
    counts[:, batch_offset + batch_size - 1] = 65535
    counts[0, batch_offset + 1] = 65535
    counts[1:, batch_offset + 1] = 0
    v_kmers = rng.uniform(0.5, 2.0, d).astype(np.float32)
    w_rows, w_ids = oracle.convert(counts, v_kmers, batch_offset, batch_size)
    kept = set(int(i) for i in w_ids)
    assert batch_offset + 11 in kept and batch_offset + 10 not in kept  # both sides of the edge
    assert 0 < len(w_ids) < batch_size
    engine.load_counts(counts, v_kmers, batch_offset, batch_size)
    off = np.arange(len(w_ids) + 1, dtype=np.uint64)
    check(engine, (w_rows, off, w_ids), f"load_counts d={d}")


@pytest.mark.parametrize("d", [64, 32, 13])
def test_restore_row_state(engine, d):
    """snapshot -> cluster -> restore: the state equals the state before the cluster call (the
    image is rebuilt, not snapshotted)."""
    n = 6000
    rows, off, ids = row_state.ladder(n, d)
    engine.load_rows(rows, off, ids)
    before = check(engine, (rows, off, ids), f"before d={d}")
    engine.snapshot()
    trace, _, _ = engine.cluster(0.8, 4, 1000000, 777, 3)
    assert trace[-1] < trace[0]
    got = engine.result()
    assert_row_state(engine, got[0], got[1], f"after cluster d={d}")
    engine.restore()
    after = check(engine, (rows, off, ids), f"restored d={d}")
    assert same_state(before, after)


@pytest.mark.parametrize("d", [64, 32, 16])
def test_projection_switch_row_state(engine, oracle, d):
    """projection 0 -> 1 -> 0 around two cluster calls on the same rows: the image is dropped,
    the merges of the second call do not keep it, and it is rebuilt from the merged rows; a third
    call then computes with it."""
    n = 20000
    rows, off, ids = row_state.ladder(n, d)
    calls = [(0.9, 2, 1000000, 777, 0), (0.85, 2, 1000000, 777, None), (0.8, 3, 1000000, 777, None)]
    want, counter = [], 0
    cur = (rows, off, ids)
    for ms, it, bthr, seed, _ in calls:
        o = oracle.cluster(cur[0], ms, it, bthr, seed, counter, cur[1], cur[2])
        want.append(o)
        cur, counter = o[:3], o[4]
    assert want[0][0].shape[0] < n
    assert want[2][0].shape[0] < want[1][0].shape[0] < want[0][0].shape[0]
    with options(engine, projection=0):
        engine.load_rows(rows, off, ids)
        counter = 0
        for k, (ms, it, bthr, seed, _) in enumerate(calls):
            engine.set_option("projection", 1 if k == 1 else 0)
            trace, counter, _ = engine.cluster(ms, it, bthr, seed, counter)
            assert np.array_equal(trace, want[k][3]) and counter == want[k][4]
            st = check(engine, want[k], f"d={d} call {k}")
            assert (st["image"] is None) == (k == 1)
            if k == 1:  # back on: rebuilt from the rows the packed-projection call merged
                engine.set_option("projection", 0)
                st = check(engine, want[k], f"d={d} image rebuilt")
                assert st["image"] is not None
