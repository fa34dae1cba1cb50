"""Every row width the engine accepts, d = 1 .. 4096: which projection kernel runs, and the merges.

klsh_hash_keys and klsh_load_rows take any d in [1, 4096].  The projection kernel depends on d and
on the iteration's h = floor(log2 n) (launch_project, klsh_kernels.hip):

  default variant   d = 8, 16, 32, 64        the register kernels (other files)
                    d > 64, h > 0            k_project_mfma_wide while its fragment table fits:
                                             ceil(d / 16) * 2048 + 128 <= 96 KB, i.e. d <= 752
                    else                     k_project_wide_pk while the hyperplanes fit in LDS,
                                             16 * dp * ceil(h / 4) <= 64 KB; else k_project_generic
  projection = 1    the last line alone

so 753 / 20, 1024 / 16, 2048 / 8 and 4096 / 4 are the last (d, h) of k_project_wide_pk under the
default variant, and dp = 512 / h <= 28 under projection = 1.  Part (a) pins that rule: the
expected kernel of every case is written out, read back through option "last_hash_variant", and
the keys are the oracle's bits.  Parts (b) and (c) run the wide-row merges (klsh_merge_wide.h,
huge_runs) at widths where a row is narrower than one staging chunk (d = 1..4: dp = 4, mostly
pad), one column past a chunk (65), no multiple of 32 (1000) and the maximum (4096), result and
row state against the oracle by bits; part (d) the refusals on either side of the range.
"""
import ctypes
import math

import numpy as np
import pytest
import torch  # (before the engine's first use of the device, as test_gpu_result_device.py)

from kmerlsh_amd import _native
from row_state import (LADDER_CALL, adversarial_rows, assert_same_result, check, clustered,
                       ladder_reference, options, weights)
from test_gpu_launch_geometry import BIG, NESTED, class_counts, ids_of

pytestmark = pytest.mark.gpu

PK, WIDE_PK, GENERIC = (_native.PROJ_VARIANT_PK, _native.PROJ_VARIANT_WIDE_PK,
                        _native.PROJ_VARIANT_GENERIC)
H16, MFMA_512, MFMA = (_native.PROJ_VARIANT_H16, _native.PROJ_VARIANT_MFMA_WIDE_512,
                       _native.PROJ_VARIANT_MFMA_WIDE)
# option "last_hash_kernel" of each: packed chains 0, fp16-image screen 1, wide screen 2
KERNEL_OF = {PK: 0, WIDE_PK: 0, GENERIC: 0, H16: 1, MFMA_512: 2, MFMA: 2}

# ----------------------------------------------------------- (a) the projection dispatch table ---
HASH_N = 3000  # 11.7 tiles of 256 rows, 15.6 of 192: a partial last tile either way
# d, h, option "projection", the kernel
DISPATCH = [
    (1, 1, 0, WIDE_PK), (2, 5, 0, WIDE_PK), (3, 7, 0, WIDE_PK), (4, 7, 0, WIDE_PK),
    (7, 9, 0, WIDE_PK), (17, 11, 0, WIDE_PK), (63, 31, 0, WIDE_PK),
    (65, 31, 0, MFMA), (80, 20, 0, MFMA), (128, 31, 0, MFMA), (513, 20, 0, MFMA),
    (752, 31, 0, MFMA),            # 47 k-steps: 96,384 B of fragments, the last width that fits
    (753, 20, 0, WIDE_PK),         # 16 * 756 * 5 = 60,480 B
    (753, 21, 0, GENERIC),         # 16 * 756 * 6 = 72,576 B
    (1024, 16, 0, WIDE_PK),        # 16 * 1024 * 4: exactly 64 KB
    (1024, 17, 0, GENERIC),
    (2048, 8, 0, WIDE_PK),         # 16 * 2048 * 2: exactly 64 KB
    (2048, 9, 0, GENERIC),
    (4096, 4, 0, WIDE_PK),         # 16 * 4096 * 1: exactly 64 KB
    (4096, 5, 0, GENERIC), (4096, 31, 0, GENERIC),
    (4095, 31, 0, GENERIC),        # dp = 4096, three columns in the remainder loop
    (65, 31, 1, WIDE_PK), (512, 28, 1, WIDE_PK),
    (512, 31, 1, WIDE_PK),         # 16 * 512 * 8: exactly 64 KB
    (516, 28, 1, WIDE_PK),         # 16 * 516 * 7 = 57,792 B
    (516, 29, 1, GENERIC),         # 16 * 516 * 8 = 66,048 B
]
assert sum(v == GENERIC for *_, v in DISPATCH) >= 5
_hash = {}


def hash_reference(oracle, d, h):
    """(adversarial rows, hyperplanes, the oracle's keys) of a (d, h), once per session."""
    if (d, h) not in _hash:
        w, _ = _native.hyperplanes(7 + d, 0, h, d)
        rows = adversarial_rows(np.random.default_rng(11 + d + h), HASH_N, d, w)
        want = oracle.keys(rows, w)
        for a in (rows, w, want):
            a.setflags(write=False)
        _hash[d, h] = (rows, w, want)
    return _hash[d, h]


def hash_case(engine, oracle, d, h, opts, variant):
    rows, w, want = hash_reference(oracle, d, h)
    with options(engine, **opts):
        got = engine.hash_keys(rows, w)
        seen = engine.get_option("last_hash_variant")
        kernel = engine.get_option("last_hash_kernel")
        close = engine.get_option("last_hash_close_pairs")
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (d, h, opts, seen, bad[:8], got[bad[:8]], want[bad[:8]])
    assert seen == variant, (d, h, opts, seen)
    assert kernel == KERNEL_OF[variant]
    if variant in (MFMA, MFMA_512):
        assert close > 0
    return rows, w, close


@pytest.mark.parametrize("d,h,projection,variant", DISPATCH,
                         ids=[f"d{d} h{h} projection={p}" for d, h, p, _ in DISPATCH])
def test_projection_dispatch(engine, oracle, d, h, projection, variant):
    hash_case(engine, oracle, d, h, {"projection": projection}, variant)


WIDE_SETS = [{"wide_grid": 1}, {"fix_grid": 1}, {"wide_grid": 1, "fix_grid": 1}]
TRIP_CASES = [(d, h, o) for d, h in [(65, 31), (752, 31)] for o in WIDE_SETS]


@pytest.mark.parametrize("d,h,opts", TRIP_CASES,
                         ids=[f"d{d} " + i for (d, _, _), i in
                              zip(TRIP_CASES, ids_of([o for _, _, o in TRIP_CASES]))])
def test_projection_rolled_screen_one_workgroup(engine, oracle, d, h, opts):
    """k_project_mfma_wide<0> at 5 and at 47 k-steps, and k_project_fix at those widths, on one
    workgroup each: 192 rows and 256 listed pairs a trip."""
    assert HASH_N > 3 * 192 and HASH_N % 192
    rows, w, close = hash_case(engine, oracle, d, h, opts, MFMA)
    if "fix_grid" in opts:
        # the pairs the screen cannot call, from the reference alone (as
        # test_projection_wide_one_workgroup): an exact sum below 2^-20 sum |x_k w_k| is far
        # inside the screen's bound of wide_eps(d) >= 2^-15 times that
        x, v = rows.astype(np.float64), w.astype(np.float64)
        with np.errstate(all="ignore"):
            s, t = x @ v.T, np.abs(x) @ np.abs(v).T
            sure = int((np.isfinite(t) & (t > 0) & (np.abs(s) < t * 2.0 ** -20)).sum())
        assert sure > 3 * 256, sure
        assert close >= sure, (close, sure)


# ------------------------------------------------------- (b) one bucket, every run class --------
MERGE_B = [2, 7, 33, 64, 100, 160, 300, 600, 1000]
MERGE_D = [1, 2, 3, 4, 65, 1000, 4096]
PLAIN_D = [3, 1000]  # also at thr = 0 and with the special rows
# seeds other than 0: found on the CPU so that every case merges without collapsing (below)
SEEDS = {(2, 1): 1, (2, 2): 2, (2, 3): 3, (7, 3): 1, (2, 4): 1, (2, 65): 1, (2, 1000): 4,
         (7, 1000): 1, (2, 4096): 1}
_bucket, _pcluster = {}, {}


def bucket(b, d, special=False):
    """One bucket of b weighted rows of the form of row_state.spread (groups of rows at sigma
    0.05..0.45 around their centers, member counts 1..300), at least two groups.
    special: rows with a NaN, all zero, x1e30 and x1e-30 (two each, so that pairs of them meet)."""
    if (b, d, special) not in _bucket:
        rng = np.random.default_rng([b, d, SEEDS.get((b, d), 0)])
        groups = max(2, b // 6)
        centers = rng.normal(0, 1, size=(groups, d)).astype(np.float32)
        sig = rng.uniform(0.05, 0.45, size=(b, 1))
        labels = rng.integers(0, groups, b)
        rows = (centers[labels] + rng.normal(0, 1, size=(b, d)) * sig).astype(np.float32)
        off, ids = weights(rng, b, 301)
        if special:
            rows[5, min(2, d - 1)] = np.nan
            rows[b // 2, 0] = np.nan
            rows[17] = 0.0
            rows[b // 2 + 9] = 0.0
            rows[[40, 41, b - 3]] *= np.float32(1e30)
            rows[[80, 81, b - 7]] *= np.float32(1e-30)
        for a in (rows, off, ids):
            a.setflags(write=False)
        _bucket[b, d, special] = (rows, off, ids)
    return _bucket[b, d, special]


def bucket_reference(oracle, b, d, thr, unit=False, special=False):
    """oracle.pcluster of the bucket, once per session; fails unless it merges (fewer survivors
    than rows) without collapsing (more than one survivor; b = 2 can only merge)."""
    key = (b, d, thr, unit, special)
    if key not in _pcluster:
        rows, off, ids = bucket(b, d, special)
        want = oracle.pcluster(rows, thr) if unit else oracle.pcluster(rows, thr, off, ids)
        s = want[0].shape[0]
        # (d = 1: every pair of rows of one sign merges, so two survivors are the most)
        assert s < b and (b == 2 or s >= 2), (b, d, thr, unit, special, s)
        _pcluster[key] = want
    return _pcluster[key]


@pytest.mark.parametrize("d", MERGE_D)
@pytest.mark.parametrize("b", MERGE_B)
def test_pcluster_widths(engine, oracle, b, d):
    """klsh_pcluster(0.9) over weighted rows: k_merge_group_wide<G> by its exact chains (b <= 64),
    k_merge_big_wide in its four classes (65..896), k_merge_huge<0> (1000)."""
    rows, off, ids = bucket(b, d)
    want = bucket_reference(oracle, b, d, 0.9)
    engine.load_rows(rows, off, ids)
    engine.pcluster(0.9)
    check(engine, want, f"b={b} d={d}")


@pytest.mark.parametrize("d", PLAIN_D)
@pytest.mark.parametrize("b", MERGE_B)
def test_pcluster_widths_plain_decider(engine, oracle, b, d):
    """The same with unit weights at thr = 0: the plain decider."""
    rows, _, _ = bucket(b, d)
    want = bucket_reference(oracle, b, d, 0.0, unit=True)
    engine.load_rows(rows)
    engine.pcluster(0.0)
    check(engine, want, f"b={b} d={d} thr=0")


@pytest.mark.parametrize("d", PLAIN_D)
def test_pcluster_widths_special_rows(engine, oracle, d):
    """A 300-row bucket with NaN, zero, x1e30 and x1e-30 rows in it."""
    rows, off, ids = bucket(300, d, special=True)
    want = bucket_reference(oracle, 300, d, 0.9, special=True)
    engine.load_rows(rows, off, ids)
    engine.pcluster(0.9)
    check(engine, want, f"b=300 d={d} special")


@pytest.mark.parametrize("fold", [0, 1], ids=["huge", "huge_fold"])
@pytest.mark.parametrize("d", [1000, 4096])
@pytest.mark.parametrize("b", [1000, 1500])
def test_pcluster_widths_huge_runs(engine, oracle, b, d, fold):
    """Runs over 896 rows: k_merge_huge<0> with the visited row in LDS (64 KB of slots and norms
    + 16 KB of row at d = 4096), and the same walk folded into k_merge_big_wide's 896 class."""
    rows, off, ids = bucket(b, d)
    want = bucket_reference(oracle, b, d, 0.9)
    with options(engine, huge_fold=fold, tail_merge_rows=1):
        engine.load_rows(rows, off, ids)
        engine.pcluster(0.9)
        check(engine, want, f"b={b} d={d} huge_fold={fold}")


# ------------------------------------------------------------------------ (c) the loop ----------
LOOP_N = 12000  # the smallest size tried; runs of every class at each of the widths below
_runs = {}


def first_iteration_runs(oracle, n, d):
    """Lengths of the runs of 2+ equal keys in the first iteration of the ladder loop."""
    if (n, d) not in _runs:
        rows = ladder_reference(oracle, n, d, BIG)[0][0]
        _, _, seed, counter = LADDER_CALL
        w, _ = oracle.table(seed, counter, int(math.floor(math.log2(n))), d)
        _, lengths = np.unique(oracle.keys(rows, w), return_counts=True)
        _runs[n, d] = lengths[lengths >= 2]
    return _runs[n, d]


@pytest.mark.parametrize("opts", [{}, {"tail_merge_rows": 1}, {"tail_batch": 0}],
                         ids=["default", "per_class", "no_tail_batch"])
@pytest.mark.parametrize("bthr", [BIG, NESTED])
@pytest.mark.parametrize("d", [3, 65, 1000])
def test_cluster_loop_widths(engine, oracle, d, bthr, opts):
    """Six iterations over the weighted ladder rows (test_cluster_loop_row_state at these widths):
    trace, counter, result and the row state the loop leaves."""
    n = LOOP_N
    lengths = first_iteration_runs(oracle, n, d)
    cnt = class_counts(lengths)
    assert (cnt >= 1).all(), (d, n, cnt.tolist())  # 2..64, 65..128, ..., 385..896, longer
    if bthr < BIG:
        assert (lengths > bthr).sum() >= 1  # the nested path is taken
    (rows, off, ids), want = ladder_reference(oracle, n, d, bthr)
    min_sim, iters, seed, counter = LADDER_CALL
    with options(engine, **opts):
        engine.load_rows(rows, off, ids)
        trace, c, _ = engine.cluster(min_sim, iters, bthr, seed, counter)
        assert np.array_equal(trace, want[3]) and c == want[4], (trace, want[3])
        assert trace[-1] < trace[0]
        check(engine, want, f"ladder n={n} d={d} bthr={bthr} {opts}")


def packed_kernel(d, h):
    """launch_project's choice past the wide screen: the hyperplanes in LDS while they fit."""
    dp = (d + 3) & ~3
    return WIDE_PK if 16 * dp * ((h + 3) // 4) <= 64 * 1024 else GENERIC


@pytest.mark.parametrize("d,n,groups,iters", [(2048, 1400, 500, 6), (4096, 60, 12, 5)])
def test_cluster_loop_crosses_projection_kernels(engine, oracle, d, n, groups, iters):
    """A loop whose h falls through k_project_wide_pk's limit (h <= 8 at d = 2048, <= 4 at 4096)
    inside one call: k_project_generic in its first iterations, k_project_wide_pk after."""
    rng = np.random.default_rng([d, n, 0])
    rows = clustered(rng, n, d, groups, 0.05)
    off, ids = weights(rng, n, 6)
    min_sim, _, seed, counter = LADDER_CALL
    want = oracle.cluster(rows, min_sim, iters, BIG, seed, counter, off, ids)
    hs = sorted({int(math.floor(math.log2(int(nt)))) for nt in want[3]}, reverse=True)
    seen = set()
    for h in hs:  # the kernel of every (d, h) of the loop, on 64 of its rows
        w, _ = _native.hyperplanes(7 + d, 0, h, d)
        assert np.array_equal(engine.hash_keys(rows[:64], w), oracle.keys(rows[:64], w)), (d, h)
        variant = engine.get_option("last_hash_variant")
        assert variant == packed_kernel(d, h), (d, h, variant)
        seen.add(variant)
    assert seen == {WIDE_PK, GENERIC}, (d, hs, seen)
    engine.load_rows(rows, off, ids)
    trace, c, _ = engine.cluster(min_sim, iters, BIG, seed, counter)
    assert np.array_equal(trace, want[3]) and c == want[4], (trace, want[3])
    assert trace[-1] < trace[0]
    check(engine, want, f"clustered n={n} d={d}")


# ----------------------------------------------------------------------- (d) the range ----------
def test_width_range():
    """d = 0 and d = 4097 are KLSH_E_RANGE at every entry point that takes a width, and load
    nothing; the context then takes the widest matrix and returns it unchanged."""
    E_RANGE = -6
    assert _native.ERRORS[E_RANGE] == "KLSH_E_RANGE"
    lib = _native.load_library()
    P = ctypes.c_void_p
    host = np.random.default_rng(4097).normal(0, 1, size=(16, 4100)).astype(np.float32)
    keys = np.zeros(16, np.uint32)
    with _native.Engine(0) as eng:
        dev = torch.from_numpy(host).to(f"cuda:{eng.device}")
        for d in (0, 4097):
            assert lib.klsh_load_rows(eng._ctx, P(host.ctypes.data), 16, d, None, None) == E_RANGE
            assert lib.klsh_load_rows_device(eng._ctx, P(dev.data_ptr()), 16, d, 4100,
                                             None) == E_RANGE
            assert lib.klsh_hash_keys(eng._ctx, P(host.ctypes.data), 16, d, P(host.ctypes.data),
                                      1, P(keys.ctypes.data)) == E_RANGE
            assert eng.get_option("last_hash_variant") == _native.PROJ_VARIANT_NONE
            with pytest.raises(_native.KlshError, match="KLSH_E_STATE"):
                eng.count()
        rows = np.ascontiguousarray(host[:, :4096])
        eng.load_rows(rows)
        assert eng.count() == (16, 16)
        assert_same_result(eng.result(), rows, np.arange(17), np.arange(16))
