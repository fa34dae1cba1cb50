"""k_project_h16's sign bound: eps T~ (T~ = |w_hi| . |x~|, option h16_bound = 1, the default)
against eps |w||x~| (h16_bound = 0).

Either bound only decides which (row, hyperplane) pairs the fp16 screen may call; the rest are
settled by the reference's sequential f32 chain, so the keys must equal the oracle's bit for bit
under both, on rows built to sit where the T bound differs most from the norm bound.  The count of
pairs left to the exact chains is checked from both sides against the two bounds evaluated in
float64: the T bound must call clearly more pairs than the norm bound, and no pair that
h16_eps . T cannot certify.
"""
import numpy as np
import pytest

from row_state import LADDER_CALL, adversarial_rows, assert_same_result, ladder, options

pytestmark = pytest.mark.gpu

BIG = 1000000  # bucket_size_threshold: no run is oversize


def h16_eps(d):
    """klsh_kernels.hip h16_eps: fp16 rounding of x, the w hi/lo residual, the MFMA's f32 sums,
    the reference chain's own rounding, with 1.5x headroom."""
    ks = (d + 15) // 16
    return 1.5 * (2.0 ** -11 + 2.0 ** -22 + (17 + 2 * ks) * 2.0 ** -23 + (d + 1) * 2.0 ** -24)


# ------------------------------------------------------------------------------- the rows ------
def spike_rows(rng, n, d, w):
    """T << |x||w|: one element 10^4 times the rest, where |w_jk| is smallest (j = i % h); every
    other row is then moved onto hyperplane j, so s is rounding noise under a small T."""
    h = w.shape[0]
    w64 = w.astype(np.float64)
    rows = rng.normal(0, 1, size=(n, d))
    for i in range(n):
        j = i % h
        k = int(np.argmin(np.abs(w64[j])))
        rows[i, k] = 1e4 * (1 if i % 4 < 2 else -1) * (1 + rng.random())
        if i % 2:
            rows[i] -= (rows[i] @ w64[j]) / (w64[j] @ w64[j]) * w64[j]
    return rows.astype(np.float32)


def ulp_rows(rng, n, d, w):
    """The sequential sum of hyperplane j is +0, -0 + 0, or what one ulp of one element leaves:
    x = w_l e_k - w_k e_l (two exact opposite products), with x_k moved by -1, 0 or +1 ulp, either
    sign of the row, alone or among elements too small to reach the sum's last bit."""
    h = w.shape[0]
    rows = np.zeros((n, d), np.float32)
    for i in range(n):
        j, k = i % h, (i * 7) % d
        l = (k + 1 + i % (d - 1)) % d
        if i % 5 == 4:
            rows[i] = (rng.normal(0, 1, d) * 1e-30).astype(np.float32)
        a, b = w[j, l], -w[j, k]
        step = (i // h) % 3 - 1
        if step:
            a = np.nextafter(a, np.float32(np.inf if step > 0 else -np.inf))
        rows[i, k], rows[i, l] = a, b
        if (i // (3 * h)) % 2:
            rows[i] = -rows[i]
    return rows


def mixed_rows(rng, n, d, w):
    """Mixed signs, T >> |s|: the row moved onto hyperplane j = i % h, then given back a component
    along it of 0, 10^-9 ... 10^-2 of |x||w|, either sign: both sides of either bound."""
    h = w.shape[0]
    w64 = w.astype(np.float64)
    rows = rng.normal(0, 1, size=(n, d)) * np.exp(rng.normal(0, 2, size=(n, 1)))
    scale = [0.0] + [10.0 ** -e for e in range(9, 1, -1)]
    for i in range(n):
        j = i % h
        ww = w64[j] @ w64[j]
        rows[i] -= (rows[i] @ w64[j]) / ww * w64[j]
        rel = scale[(i // h) % len(scale)] * (1 if (i // (h * len(scale))) % 2 else -1)
        rows[i] += rel * np.linalg.norm(rows[i]) / np.sqrt(ww) * w64[j]
    return rows.astype(np.float32)


def range_rows(rng, n, d, w):
    """Elements below fp16's normal range (image subnormal or 0), at and past its largest finite
    value (65504; from 65520 on the image is inf), zeros, NaN and inf, one to all of a row."""
    f = np.float32
    rows = rng.normal(0, 1, size=(n, d)).astype(np.float32)
    for i in range(n):
        r, kind, k = rows[i], i % 12, (i * 5) % d
        if kind == 0:
            r *= f(3e-5)                     # every element fp16-subnormal
        elif kind == 1:
            r[::2] *= f(1e-6)                # half of them
        elif kind == 2:
            r[k] = f(2.0 ** -25)             # one that rounds to 0 (a tie) in the image
        elif kind == 3:
            r[k] = f(65519.0)                # rounds to 65504
        elif kind == 4:
            r[k] = f(-65520.0)               # the first value that is inf in the image
        elif kind == 5:
            r[:] = np.where(rng.random(d) < 0.5, f(65504.0), f(-65504.0))
        elif kind == 6:
            r[rng.random(d) < 0.7] = 0.0
        elif kind == 7:
            r[k] = np.nan
        elif kind == 8:
            r[k] = f(np.inf) if i % 24 < 12 else f(-np.inf)
        elif kind == 9:
            r[k] = f(1e30)
        elif kind == 10:
            r *= f(1e-41)                    # f32 subnormal
        else:
            r[k], r[(k + 1) % d] = f(3e4), f(6e-8)  # one large, one fp16-subnormal
    return rows


KINDS = {"adversarial": adversarial_rows, "spike": spike_rows, "ulp": ulp_rows,
         "mixed": mixed_rows, "range": range_rows}
_cases = {}


def case(oracle, kind, n, d, h):
    """(rows, hyperplanes, the oracle's keys), computed once and shared by both bounds."""
    from kmerlsh_amd import _native

    key = (kind, n, d, h)
    if key not in _cases:
        w, _ = _native.hyperplanes(31 + d, 2, h, d)
        rows = KINDS[kind](np.random.default_rng(1000 * d + 10 * h + n % 7), n, d, w)
        want = oracle.keys(rows, w)
        for a in (rows, w, want):
            a.setflags(write=False)
        _cases[key] = (rows, w, want)
    return _cases[key]


# ----------------------------------------------------------------------------- bit parity ------
@pytest.mark.parametrize("bound", [1, 0])
@pytest.mark.parametrize("n", [4000, 257])
@pytest.mark.parametrize("h", [1, 17, 31])
@pytest.mark.parametrize("d", [16, 32, 64])
def test_keys_bit_equal_under_both_bounds(engine, oracle, d, h, n, bound):
    """n = 257: one full workgroup of 256 rows and one row of the next."""
    with options(engine, h16_bound=bound):
        assert engine.get_option("h16_bound") == bound
        for kind in KINDS:
            rows, w, want = case(oracle, kind, n, d, h)
            got = engine.hash_keys(rows, w)
            assert engine.get_option("last_hash_kernel") == 1, kind
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (kind, d, h, n, bound, bad[:8], got[bad[:8]], want[bad[:8]])
    assert engine.get_option("h16_bound") == 1  # the default


@pytest.mark.parametrize("segcap", [1, 3])
@pytest.mark.parametrize("d,h", [(64, 23), (32, 17), (16, 12)])
def test_full_segment_entries_carry_the_slot(engine, oracle, d, h, segcap):
    """One workgroup, a fix-up segment of 1 or 3 entries: the listed rows are settled from the
    slot in their entry, the rest in place, under the T bound."""
    with options(engine, h16_bound=1, h16_grid=1, h16_segcap=segcap):
        for kind in ("adversarial", "mixed"):
            rows, w, want = case(oracle, kind, 4000, d, h)
            assert np.array_equal(engine.hash_keys(rows, w), want), (kind, d, h, segcap)
            assert engine.get_option("last_hash_close_pairs") > segcap


# -------------------------------------------------------------------------- effectiveness ------
def test_close_calls_between_the_two_bounds(engine, oracle):
    """Gaussian rows, d = 64, h = 22: the pairs left to the exact chains against the pairs each
    bound cannot certify in float64.  At most 0.8 c_cs (the model: 0.63 c_cs; the slack is the
    (1 + 2^-9) factors and the absolute term), so the test does not pass by sending everything to
    the exact chains; at least 0.9 c_T, since a screen that calls pairs the derivation cannot
    certify is wrong even where the keys happen to match; and the norm bound's own count within
    10 % of c_cs under h16_bound = 0."""
    from kmerlsh_amd import _native

    n, d, h = 20000, 64, 22
    rows = np.random.default_rng(64022).normal(0, 1, size=(n, d)).astype(np.float32)
    w, _ = _native.hyperplanes(22, 0, h, d)
    x64, w64 = rows.astype(np.float64), w.astype(np.float64)
    s = np.abs(x64 @ w64.T)
    eps = h16_eps(d)
    c_cs = int((s <= eps * np.outer(np.linalg.norm(x64, axis=1), np.linalg.norm(w64, axis=1))).sum())
    c_t = int((s <= eps * (np.abs(x64) @ np.abs(w64).T)).sum())
    want = oracle.keys(rows, w)
    close = {}
    for bound in (1, 0):
        with options(engine, h16_bound=bound):
            assert np.array_equal(engine.hash_keys(rows, w), want), bound
            close[bound] = engine.get_option("last_hash_close_pairs")
    print(f"pairs {n * h}: c_cs {c_cs} c_T {c_t} close(T) {close[1]} close(norm) {close[0]}")
    assert close[1] <= 0.8 * c_cs, (close, c_cs, c_t)
    assert close[1] >= 0.9 * c_t, (close, c_cs, c_t)
    assert 0.9 * c_cs <= close[0] <= 1.1 * c_cs, (close, c_cs, c_t)


# ---------------------------------------------------------------------------- queued path ------
def test_queued_tail_same_loop_fewer_fixups(engine, oracle):
    """A loop small enough for the queued tail (n and h read on the device): the same trace, rng
    counter and result under either bound (and the oracle's), fewer pairs settled by the exact
    chains under the T bound."""
    rows, off, ids = ladder(3000, 64)
    min_sim, iters, seed, counter = LADDER_CALL
    want = oracle.cluster(rows, min_sim, iters, BIG, seed, counter, off, ids)
    got = {}
    for bound in (1, 0):
        with options(engine, h16_bound=bound):
            engine.load_rows(rows, off, ids)
            trace, c, st = engine.cluster(min_sim, iters, BIG, seed, counter)
            got[bound] = (trace, c, st, engine.result())
        assert st["project_timed_launches"] < st["project_launches"], st  # queued iterations ran
    (t1, c1, st1, r1), (t0, c0, st0, r0) = got[1], got[0]
    assert np.array_equal(t1, t0) and c1 == c0
    assert_same_result(r1, *r0)
    assert np.array_equal(t1, want[3]) and c1 == want[4]
    assert_same_result(r1, *want[:3])
    print(f"proj_fix_pairs: T bound {st1['proj_fix_pairs']}, norm bound {st0['proj_fix_pairs']}")
    assert 0 < st1["proj_fix_pairs"] < st0["proj_fix_pairs"]
