"""The per-slot state the engine caches beside the rows, derived from what klsh_result returned.

klsh_result shows the fp32 rows and member lists of the live slots.  The engine also keeps, per
slot, the sequential fp32 sum of squares (every later cosine test reads it), the member count
(the weights of every later consensus), the fp16 row image (the certified screens' input, whose
error bounds assume image == fp16(x)), the tail of the member chain (links the next merge) and
the zero pad of columns d..dp.  Each merge kernel, the loaders, the restore, the projection
switch and the sharded delta apply write that state in their own code; `assert_row_state` reads
it back through the klsh_row_state hook and compares it, by bits, with what the returned rows and
offsets say it must be.  No tolerances: a cache that is off by one ulp is a wrong cache.

Also here: the seeded inputs of the state tests ("spread" single-bucket rows, "ladder" loop rows),
the projection tests' adversarial rows, the result comparison and the options context manager,
shared by test_gpu_parity.py, test_gpu_row_state.py, test_gpu_sharded.py,
test_gpu_launch_geometry.py, test_gpu_widths.py and test_gpu_small_loops.py (the options context
manager by test_gpu_kmer_table.py too), and `clustered`,
the seeded group rows of the parity, sharded, width and small-loop tests (the one definition).
"""
import numpy as np


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


def assert_same_result(got, rows, off, ids):
    g_rows, g_off, g_ids = got
    assert np.array_equal(g_off, off)
    assert np.array_equal(g_ids, ids)
    assert same_bits(g_rows, rows)


def seq_norms(rows):
    """Sequential fp32 sum of squares of every row (the reference's distance.cc:33-34 loop):
    one column at a time, numpy rounding every multiply and every add to fp32."""
    x = np.ascontiguousarray(rows, np.float32)
    n2 = np.zeros(x.shape[0], np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for k in range(x.shape[1]):
            n2 = n2 + x[:, k] * x[:, k]
    return n2


def fp16_image(rows):
    """IEEE round-to-nearest-even fp16 bits of the rows (|x| >= 65520 -> inf)."""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(rows, np.float32).astype(np.float16).view(np.uint16)


def expected_state(rows, off):
    return {"nrm": seq_norms(rows), "cnt": np.diff(np.asarray(off, np.uint64)).astype(np.uint32),
            "image": fp16_image(rows)}


def _first_diff(eq):
    return tuple(int(v) for v in np.argwhere(~eq)[0])


def assert_row_state(engine, rows, off, what=""):
    """The engine's cached state of the live rows against (rows, off) = engine.result()[:2]
    (check_state).  Returns the state read."""
    return check_state(engine.row_state(), rows, off, what)


def check_state(st, rows, off, what=""):
    """A row_state() reading against the rows and offsets klsh_result returned with it: nrm and
    image bits equal (an element NaN on both sides counts as equal), cnt equal, the pad all +0,
    every member chain cnt nodes long and ending at its tail."""
    want = expected_state(rows, off)
    n = want["nrm"].shape[0]
    assert st["nrm"].shape == (n,) and st["cnt"].shape == (n,), what
    eq = (st["nrm"].view(np.uint32) == want["nrm"].view(np.uint32)) | \
         (np.isnan(st["nrm"]) & np.isnan(want["nrm"]))
    if not eq.all():
        i = _first_diff(eq)[0]
        raise AssertionError(f"{what}: nrm of live row {i}: cached {st['nrm'][i]!r} "
                             f"({int(st['nrm'].view(np.uint32)[i]):#x}), sequential sum "
                             f"{want['nrm'][i]!r} ({int(want['nrm'].view(np.uint32)[i]):#x}); "
                             f"{int((~eq).sum())} of {n} rows differ")
    assert np.array_equal(st["cnt"], want["cnt"]), \
        f"{what}: cnt differs at live row {_first_diff(st['cnt'] == want['cnt'])}"
    if st["image"] is not None:
        got, exp = st["image"], want["image"]
        assert got.shape == exp.shape, what
        eq = (got == exp) | (np.isnan(got.view(np.float16)) & np.isnan(exp.view(np.float16)))
        if not eq.all():
            i, k = _first_diff(eq)
            raise AssertionError(f"{what}: fp16 image of live row {i} column {k}: cached "
                                 f"{int(got[i, k]):#06x}, fp16(x) {int(exp[i, k]):#06x} "
                                 f"(x = {rows[i, k]!r}); {int((~eq).sum())} values differ")
    assert st["pad_nonzero"] == 0, f"{what}: {st['pad_nonzero']} pad words are not +0"
    assert st["bad_links"] == 0, f"{what}: {st['bad_links']} member chains do not match cnt / tail"
    return st


def check(engine, want, what):
    """Result against the oracle's (rows, off, ids), then the cached state against the result."""
    got = engine.result()
    try:
        assert_same_result(got, *want[:3])
    except AssertionError as ex:
        raise AssertionError(f"result differs: {what}") from ex
    return assert_row_state(engine, got[0], got[1], what)


def same_state(a, b):
    """Two row_state() readings equal by bits (the NaN payloads included)."""
    if (a["image"] is None) != (b["image"] is None):
        return False
    return (np.array_equal(a["nrm"].view(np.uint32), b["nrm"].view(np.uint32)) and
            np.array_equal(a["cnt"], b["cnt"]) and
            (a["image"] is None or np.array_equal(a["image"], b["image"])) and
            a["pad_nonzero"] == b["pad_nonzero"] and a["bad_links"] == b["bad_links"])


class options:
    """Engine options set for a block and restored to their previous values after it."""

    def __init__(self, engine, **kv):
        self.engine, self.kv, self.old = engine, kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = self.engine.get_option(k)
            self.engine.set_option(k, v)
        return self.engine

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.engine.set_option(k, v)
        return False


def weights(rng, n, hi):
    """Member counts 1..hi-1 per row, their offsets, and a permutation as the member ids."""
    cnt = rng.integers(1, hi, n)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    ids = rng.permutation(int(off[-1])).astype(np.uint64)
    return off, ids


def clustered(rng, n, d, groups, noise):
    """n rows around `groups` normal centers, each a center plus normal noise of that sigma."""
    centers = rng.normal(0, 1, size=(groups, d)).astype(np.float32)
    return (centers[rng.integers(0, groups, n)] +
            rng.normal(0, noise, size=(n, d)).astype(np.float32)).astype(np.float32)


def spread(b, d):
    """One bucket of b rows in max(1, b // 6) groups whose rows sit at very different distances
    from their center (sigma 0.05..0.45 per row), so that a threshold of 0.95 merges some of every
    group and 0.85 merges more: (rows, offsets, ids) with weights 1..300."""
    rng = np.random.default_rng(b * 19 + d)
    groups = max(1, b // 6)
    centers = rng.normal(0, 1, size=(groups, d)).astype(np.float32)
    sig = rng.uniform(0.05, 0.45, size=(b, 1))
    labels = rng.integers(0, groups, b)
    rows = (centers[labels] + rng.normal(0, 1, size=(b, d)) * sig).astype(np.float32)
    off, ids = weights(rng, b, 301)
    return rows, off, ids


_spread_cache = {}


def spread_cached(b, d):
    if (b, d) not in _spread_cache:
        _spread_cache[b, d] = spread(b, d)
    return _spread_cache[b, d]


LADDER_SIZES = [3, 20, 50, 100, 160, 300, 600, 1500]
# the loop shapes: the first iteration's keys (seed 777, counter 3) hold runs of every merge class
LADDER_SHAPES = {64: 60000, 32: 60000, 16: 40000, 8: 30000, 13: 30000, 100: 30000, 512: 20000}
LADDER_CALL = (0.8, 6, 777, 3)  # min_similarity, iterations, seed, counter (bthr per case)
_ladder_cache = {}


def ladder_reference(oracle, n, d, bthr, min_sim=LADDER_CALL[0], special=False):
    """(rows, off, ids) of ladder(n, d) and the oracle's (rows, off, ids, trace, counter) of the
    weighted loop over them; computed once per session, shared by every test, never written."""
    key = (n, d, bthr, min_sim, special)
    if key not in _ladder_cache:
        if (n, d, special) not in _ladder_cache:
            _ladder_cache[n, d, special] = ladder(n, d, special)
        rows, off, ids = _ladder_cache[n, d, special]
        _, iters, seed, counter = LADDER_CALL
        want = oracle.cluster(rows, min_sim, iters, bthr, seed, counter, off, ids)
        for a in (rows, off, ids) + tuple(want[:4]):
            a.setflags(write=False)
        _ladder_cache[key] = ((rows, off, ids), want)
    return _ladder_cache[key]


def ladder(n, d, special=False):
    """Loop rows whose groups come in every merge class's run length: group sizes cycle through
    LADDER_SIZES until they sum to n (the last one trimmed), tight (sigma 0.03) in even cycles and
    loose (0.3) in odd ones, shuffled: (rows, offsets, ids) with weights 1..5.
    special: rows of the first cycle's tight groups of 20..1500 rows (two per kind, of different
    groups) become NaN, zero, x1e30, x1e-30, x1e5 (inf in the fp16 image) and x1e-9 (all-zero
    image) — rows no screen can call, inside runs of every class."""
    rng = np.random.default_rng(n + d)
    sizes, sigma = [], []
    while sum(sizes) < n:
        i = len(sizes)
        sizes.append(min(LADDER_SIZES[i % len(LADDER_SIZES)], n - sum(sizes)))
        sigma.append(0.03 if (i // len(LADDER_SIZES)) % 2 == 0 else 0.3)
    centers = rng.normal(0, 1, size=(len(sizes), d)).astype(np.float32)
    label = np.repeat(np.arange(len(sizes)), sizes)
    sig = np.repeat(np.array(sigma), sizes)[:, None]
    rows = (centers[label] + rng.normal(0, 1, size=(n, d)) * sig).astype(np.float32)
    perm = rng.permutation(n)
    rows = rows[perm]
    off, ids = weights(rng, n, 6)
    if special:
        label = label[perm]
        for kind in range(12):
            i = np.flatnonzero(label == 1 + kind % 7)[kind]
            if kind % 6 == 0:
                rows[i, kind] = np.nan
            elif kind % 6 == 1:
                rows[i] = 0.0
            else:
                rows[i] *= np.float32([1e30, 1e-30, 1e5, 1e-9][kind % 6 - 2])
    return rows, off, ids


def adversarial_rows(rng, n, d, w):
    """Rows the certified projection screens cannot call, and rows that break the fp16 image:
    every third row projected onto hyperplane i % h (s is rounding noise around 0), rows whose
    sequential sum is exactly 0 for a hyperplane (x = w_l e_k - w_k e_l: the two products are
    exact negatives), zero / -0 / tiny / huge / NaN / inf rows, elements past fp16's range
    (>= 65520 -> inf in the image), fp16-subnormal rows and rows whose fp16 image is all zero
    while the f32 row is not, f32-subnormal rows."""
    h = w.shape[0]
    w64 = w.astype(np.float64)
    rows = rng.normal(0, 1, size=(n, d))
    for i in range(0, n, 3):
        j = i % h
        rows[i] -= (rows[i] @ w64[j]) / (w64[j] @ w64[j]) * w64[j]
    rows = rows.astype(np.float32)
    f = np.float32
    rows[1] = 0.0
    rows[4] *= f(1e-30)
    rows[7] *= f(1e30)
    rows[10, min(3, d - 1)] = np.nan  # (d < 4: the row's last column)
    rows[13] = -0.0
    for m, i in enumerate(range(2, min(n, 2 + 3 * h * 4), 3)):  # s == 0 exactly for hyperplane j
        j, k = m % h, (m * 7) % d
        l = (k + 1 + m % (d - 1)) % d if d > 1 else k
        if l == k:
            continue
        rows[i] = 0.0
        rows[i, k], rows[i, l] = w[j, l], -w[j, k]
        if m % 2:
            rows[i] *= f(-1)
    special = {
        16: lambda r: r.__setitem__(0, f(70000.0)),      # fp16 overflow: inf in the image
        19: lambda r: r.__setitem__(d - 1, f(65519.0)),  # rounds to 65504, finite
        22: lambda r: r.__imul__(f(1e-6)),               # fp16 subnormal image
        25: lambda r: r.__imul__(f(1e-9)),               # fp16 image all zero, f32 nonzero
        28: lambda r: r.__setitem__(slice(0, d // 2), r[: d // 2] * f(1e-9)),
        31: lambda r: r.__setitem__(slice(None), np.where(np.arange(d) % 2, f(-0.0), f(0.0))),
        34: lambda r: r.__setitem__(0, f(np.inf)),
        37: lambda r: r.__imul__(f(1e-40)),              # f32 subnormal
        40: lambda r: r.__setitem__(slice(None), f(65504.0)),
        43: lambda r: r.__setitem__(d // 2, f(-1e5)),
    }
    for i, fn in special.items():
        if i < n:
            fn(rows[i])
    return rows
