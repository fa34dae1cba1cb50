"""The loop where it is small: 2..4097 rows, calls longer than the ring, tiny bucket thresholds.

The production runs spend their last few hundred iterations in the queued tail (run_batched,
klsh_loop.cpp): the host is out of the loop, every kernel takes N_t and h_t = floor(log2 N_t) from
a device word, and only the published counters would tell the host about a mistake.  The rest of
the suite enters that tail at 600 rows or more, for 40 iterations at most, with bucket thresholds
no input ever reaches.  Here:

  A  every N in 2..130 and around 256, 512, 1024, 2048 and 4096 — below one tile, one wave and one
     group, where each kernel's partial tile is its whole input — at the queued widths and at
     d = 13 (host-driven, the wide kernels), under the options that pick another launch sequence;
  B  calls of 130 and 200 iterations: the ring of 64 slots reused, chunks sized from a published
     N, both sort paths of the tail and the switch between them, N_t down to 1 inside a chunk, and
     the call lengths at the chunk edges;
  C  bucket_size_threshold -1, 0, 1, 2, 3, 64 and one the loop falls below in mid-call: the
     reference's `size > threshold` at its sign and at runs of exactly `threshold` rows, hundreds
     of adjacent nested regions of 2..4 rows, the host-driven loop handing over to the queue.

Every case compares the trace, the RNG counter and the result with oracle.cluster by bits and then
reads the cached row state back (row_state.check).  What a case claims about its input (chunks
that merge, the sort path of each chunk, an N_t of 1 with iterations left, nested draws) is
asserted from the oracle's own output before the engine runs.
"""
import numpy as np
import pytest

from row_state import check, clustered, options, same_bits, weights

pytestmark = pytest.mark.gpu

SEED, COUNTER = 777, 3
NO_BTHR = 1000000
QUEUED_D = (8, 16, 32, 64)  # project_device_n_ok: the widths whose kernels read N on the device
CHUNK = 32                  # iterations per queued chunk (klsh_ctx::kRing / 2), two in flight
LOCAL_HB_MIN = 10           # tail_local_ok: a chunk of hb = 10..19 sorts through k_tail_local


def floor_log2(n):
    return int(n).bit_length() - 1


def host_iterations(trace, iters, bthr, d):
    """Iterations the host drives before the queue takes the rest (batch_eligible, default
    options): the first t with 2 <= N_t, N_t <= bthr unless bthr < 0, two or more iterations left,
    at a queued width.  Every size here is far below the 2^20 bound."""
    if d in QUEUED_D:
        for t in range(iters):
            n = int(trace[t])
            if n >= 2 and (bthr < 0 or n <= bthr) and iters - t >= 2:
                return t
    return iters


def run(engine, data, want, min_sim, iters, bthr, what, counter=COUNTER, load=True,
        local_iters=None, **opts):
    """One klsh_cluster call against the oracle's `want`: trace, counter, result bits, then the
    cached row state; with local_iters, the queued iterations that sorted through k_tail_local
    (option "tail_local_iters").  Returns the call's statistics."""
    rows, off, ids = data
    with options(engine, **opts):
        if load:
            if off is None:
                engine.load_rows(rows)
            else:
                engine.load_rows(rows, off, ids)
        trace, c, st = engine.cluster(min_sim, iters, bthr, SEED, counter)
        assert np.array_equal(trace, want[3]), f"trace differs: {what} {opts}\n{trace}\n{want[3]}"
        assert c == want[4], f"rng_counter {c}, oracle {want[4]}: {what} {opts}"
        check(engine, want, f"{what} {opts}")
        if local_iters is not None:
            got = engine.get_option("tail_local_iters")
            assert got == local_iters, f"tail_local_iters {got}, planned {local_iters}: {what} {opts}"
    return st


def same_run(a, b):
    """Two oracle.cluster outputs equal: rows by bits, lists, trace and counter."""
    return (same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and
            np.array_equal(a[3], b[3]) and a[4] == b[4])


# ------------------------------------------------------------------------ A: every small N ----
_small = {}


def small_rows(n, d):
    """Tight groups of about 8 rows (sigma 0.05), weights 1..5 at even n; at every third n >= 8 an
    all-zero row, a row with one NaN and a row of 3e38 (its sum of squares is inf) — rows 1, 3 and
    5, never row 0, which is the row a lane past n reads.  Read-only, once per session."""
    if (n, d) not in _small:
        rng = np.random.default_rng(100 * n + d)
        rows = clustered(rng, n, d, max(1, n // 8), 0.05)
        if n >= 8 and n % 3 == 0:
            rows[1] = 0.0
            rows[3, d // 2] = np.nan
            rows[5] = np.float32(3e38)
        off, ids = weights(rng, n, 6) if n % 2 == 0 else (None, None)
        for a in (rows, off, ids):
            if a is not None:
                a.setflags(write=False)
        _small[n, d] = (rows, off, ids)
    return _small[n, d]


A_BANDS = {"2..33": range(2, 34), "34..65": range(34, 66), "66..97": range(66, 98),
           "98..130": range(98, 131),
           "edges": [e + k for e in (256, 512, 1024, 2048, 4096) for k in (-1, 0, 1)]}
A_OPTIONS = [{}, {"tail_batch": 0}, {"tail_merge_rows": 1}, {"tail_local": 0}, {"projection": 1}]


@pytest.mark.parametrize("band", list(A_BANDS))
@pytest.mark.parametrize("d", [8, 16, 32, 64, 13])
def test_every_small_n(engine, oracle, d, band):
    """Twelve iterations at 0.8 over n rows, every n of the band: queued from the first iteration
    at d = 8, 16, 32, 64 (host-driven with tail_batch = 0 and with the per-class launches), the
    wide kernels at d = 13.  Every loop merges; the ones of 8 rows or fewer reach N_t = 1 with
    iterations left, which the queued kernels then run with h = 0."""
    for n in A_BANDS[band]:
        data = small_rows(n, d)
        want = oracle.cluster(data[0], 0.8, 12, NO_BTHR, SEED, COUNTER, data[1], data[2])
        assert want[0].shape[0] < n, (n, d, list(want[3]))
        if n <= 8:
            assert 1 in want[3][:-2], (n, d, list(want[3]))
        # one chunk sized from n: all twelve iterations sort locally from hb = 10 on
        assert len(want[3]) == 12
        planned = local_iterations(chunk_plan(want[3], want[0].shape[0], 12)) if d in QUEUED_D else 0
        assert planned == (12 if d in QUEUED_D and n >= 1024 else 0)
        for opts in A_OPTIONS:
            observed = {(): planned, ("tail_local",): 0, ("tail_batch",): 0}.get(tuple(opts))
            run(engine, data, want, 0.8, 12, NO_BTHR, f"n={n} d={d}", local_iters=observed, **opts)


# --------------------------------------------------------- B: calls longer than the ring ------
_long = {}


def long_rows(n, d):
    """Loose groups of about 6 rows (sigma 0.5): a trace that keeps falling for 100+ iterations."""
    if (n, d) not in _long:
        rows = clustered(np.random.default_rng(100 * n + d), n, d, n // 6, 0.5)
        rows.setflags(write=False)
        _long[n, d] = (rows, None, None)
    return _long[n, d]


def chunk_plan(trace, n_final, iters):
    """The queued chunks of a call that is queued from its first iteration (run_batched): per
    chunk, the N its grids and its sort were sized from — the call's first N for chunks 0 and 1,
    the N after chunk c - 2 for chunk c >= 2 — its hb = floor(log2 of that N), and how many of its
    iterations merged."""
    n_after = [int(v) for v in trace[1:]] + [int(n_final)]  # N after iteration t
    plan = []
    for c in range((iters + CHUNK - 1) // CHUNK):
        lo, hi = c * CHUNK, min(iters, (c + 1) * CHUNK)
        n_max = int(trace[0]) if c < 2 else n_after[(c - 1) * CHUNK - 1]
        merging = sum(1 for t in range(lo, hi) if n_after[t] < int(trace[t]))
        assert all(int(trace[t]) <= n_max for t in range(lo, hi))
        plan.append({"n_max": n_max, "hb": floor_log2(n_max), "merging": merging,
                     "count": hi - lo})
    return plan


def local_iterations(plan):
    """The iterations of a fully queued call that sort through k_tail_local under the default
    options (option "tail_local_iters"): every iteration of the chunks with hb >= 10."""
    return sum(c["count"] for c in plan if c["hb"] >= LOCAL_HB_MIN)


def local_chunks(n, d, iters):
    """How many leading chunks of the B calls sort through k_tail_local (hb >= 10) before the
    call falls to the one-pass radix sort: none at 600 rows, chunks 0 and 1 (sized from the
    call's first N) at 1500 and 3000, and chunk 2 as well where 3000 rows are still 1024 or more
    after chunk 0."""
    if n == 600:
        return 0
    return 3 if (n, iters) == (3000, 130) and d != 8 else 2


B_CALLS = [(130, 0.3), (200, -1.0)]
# (200, -1.0) reaches N_t = 1 with iterations left here; at d = 8 the larger inputs end at 1 or 2
COLLAPSE = [(n, d) for n in (600, 1500, 3000) for d in (16, 32, 64)] + [(600, 8)]


@pytest.mark.parametrize("iters,min_sim", B_CALLS)
@pytest.mark.parametrize("d", [8, 16, 32, 64])
@pytest.mark.parametrize("n", [600, 1500, 3000])
def test_calls_longer_than_the_ring(engine, oracle, n, d, iters, min_sim):
    """130 iterations down to 0.3 and 200 down to -1.0 (the plain decider from threshold 0 on):
    five and seven chunks, so every ring slot is written two or three times, chunks 2.. are sized
    from a published N, and the 1500- and 3000-row calls change from k_tail_local to the one-pass
    radix sort on the way.  The second call collapses to one row and goes on."""
    data = long_rows(n, d)
    want = oracle.cluster(data[0], min_sim, iters, NO_BTHR, SEED, COUNTER)
    trace = want[3]
    plan = chunk_plan(trace, want[0].shape[0], iters)
    assert len(plan) == (5 if iters == 130 else 7)
    assert sum(1 for c in plan if c["merging"]) >= 3, plan
    k = local_chunks(n, d, iters)
    assert [c["hb"] >= LOCAL_HB_MIN for c in plan] == [True] * k + [False] * (len(plan) - k), plan
    if (n, d, iters) == (3000, 16, 130):
        assert [c["n_max"] for c in plan[:4]] == [3000, 3000, 1187, 406], plan
    if iters == 200:
        hs = {floor_log2(v) for v in trace}
        assert {1, 2} <= hs, sorted(hs)
        ones = [t for t in range(iters) if trace[t] == 1]
        assert bool(ones and ones[0] <= iters - 3) == ((n, d) in COLLAPSE), (ones[:1], n, d)
        # at d = 64 a whole chunk is sized from N = 1: hb = 0, no sort pass, grids of one tile
        assert (plan[-1]["hb"] == 0) == (d == 64), plan
    what = f"n={n} d={d} iters={iters} min_sim={min_sim}"
    # the sort path of every chunk is observed, not inferred: the engine counts the iterations
    # it queued with the local sort
    observed = local_iterations(plan)
    assert observed == sum(c["count"] for c in plan[:k]) == k * CHUNK
    st = run(engine, data, want, min_sim, iters, NO_BTHR, what, local_iters=observed, hip_events=1)
    assert st["iterations"] == st["project_launches"] == iters
    assert st["project_timed_launches"] == 0  # every iteration was queued
    st = run(engine, data, want, min_sim, iters, NO_BTHR, what, local_iters=0, hip_events=1,
             tail_local=0)
    assert st["project_timed_launches"] == 0
    st = run(engine, data, want, min_sim, iters, NO_BTHR, what, local_iters=0, hip_events=1,
             tail_batch=0)
    assert st["project_timed_launches"] == iters  # every iteration host-driven and timed


@pytest.mark.parametrize("iters", [1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 97])
@pytest.mark.parametrize("d", [16, 64])
def test_call_lengths_at_the_chunk_edges(engine, oracle, d, iters):
    """Calls that end on, one before and one after a chunk's last iteration, the ring's last slot
    and the third chunk's — and calls of 1, 2 and 3 iterations: the queue takes a call with two
    or more iterations left, so a call of one is host-driven."""
    n = 1500
    data = long_rows(n, d)
    want = oracle.cluster(data[0], 0.3, iters, NO_BTHR, SEED, COUNTER)
    assert len(want[3]) == iters
    if iters >= 2:
        assert want[0].shape[0] < n
    host = host_iterations(want[3], iters, NO_BTHR, d)
    assert host == (1 if iters == 1 else 0)
    what = f"n={n} d={d} iters={iters}"
    st = run(engine, data, want, 0.3, iters, NO_BTHR, what, hip_events=1)
    assert st["iterations"] == iters and st["project_timed_launches"] == host
    run(engine, data, want, 0.3, iters, NO_BTHR, what)


@pytest.mark.parametrize("d", [16, 64])
def test_long_call_small_hyperplane_window(engine, oracle, d):
    """hyperplane_window = 7 under a queued call of 130 iterations: predraw_hyperplanes draws
    the option's 7 rows, run_batched needs iterations * h_0 = 130 * 10 resident before its first
    launch and extends the window to them at once.  (Nothing reports the window's size: the
    evidence is the run's bit parity, every queued projection reading rows past the first 7.)"""
    n, iters, window = 1500, 130, 7
    data = long_rows(n, d)
    want = oracle.cluster(data[0], 0.3, iters, NO_BTHR, SEED, COUNTER)
    assert host_iterations(want[3], iters, NO_BTHR, d) == 0  # queued from the first iteration
    assert iters * floor_log2(n) > window and floor_log2(n) > window  # iteration 0 alone needs more
    st = run(engine, data, want, 0.3, iters, NO_BTHR, f"n={n} d={d} window 7",
             hyperplane_window=window, hip_events=1)
    assert st["project_timed_launches"] == 0


@pytest.mark.parametrize("n,d", [(1500, 16), (600, 32)])
def test_two_long_calls_back_to_back(engine, oracle, n, d):
    """A second call of 70 iterations on the state the first one left, without a reload, from the
    first's counter: it starts below 64 rows (below one wave), is queued from its first iteration,
    turns the ring again and collapses to one row."""
    data = long_rows(n, d)
    first = oracle.cluster(data[0], 0.3, 130, NO_BTHR, SEED, COUNTER)
    n1 = first[0].shape[0]
    assert 2 <= n1 < 64, n1
    second = oracle.cluster(first[0], -1.0, 70, NO_BTHR, SEED, first[4], first[1], first[2])
    assert second[3][0] == n1 and second[0].shape[0] == 1
    assert 1 in second[3][:-2], list(second[3])
    for opts in ({}, {"tail_local": 0}):
        st = run(engine, data, first, 0.3, 130, NO_BTHR, f"n={n} d={d} call 1", hip_events=1,
                 **opts)
        assert st["project_timed_launches"] == 0
        st = run(engine, data, second, -1.0, 70, NO_BTHR, f"n={n} d={d} call 2",
                 counter=first[4], load=False, hip_events=1, **opts)
        assert st["project_timed_launches"] == 0 and st["n_final"] == 1


# ------------------------------------------------- C: tiny and signed bucket thresholds -------
C_N = list(range(2, 10)) + [63, 64, 65, 130, 257, 1023, 1024, 1025]
C_ITERS = 70


def nested_draws(want):
    """Hyperplanes an oracle run drew for nested buckets: the counter advances by h_t per
    iteration and by floor(log2 size) per nested bucket (cluster.cc:194, :203 and :98)."""
    return int(want[4]) - COUNTER - sum(floor_log2(v) for v in want[3])


@pytest.mark.parametrize("n", C_N)
@pytest.mark.parametrize("d", [16, 64, 13])
def test_tiny_and_signed_bucket_thresholds(engine, oracle, d, n):
    """70 iterations at 0.8 under bucket_size_threshold -1, 0, 1, 2, 3, 64 and N_3 of the
    unnested run.  The reference nests a bucket when `size_t size > int threshold`
    (cluster.cc:286): -1 converts to SIZE_MAX and nests nothing, 0 and 1 nest every bucket of two
    rows or more, 2 and 3 leave the buckets of exactly 2 and 3 rows alone.  A bucket of more than
    b rows needs n > b, so a threshold of n or more changes nothing; below n, these tight groups
    always have one, and the nested draws show in the counter.  With a threshold the loop falls
    to in mid-call, the host-driven iterations (nested ones among them) hand over to the queue."""
    data = small_rows(n, d)
    rows, off, ids = data

    def oracle_run(bthr):
        return oracle.cluster(rows, 0.8, C_ITERS, bthr, SEED, COUNTER, off, ids)

    plain = oracle_run(NO_BTHR)
    want = {b: oracle_run(b) for b in (-1, 0, 1, 2, 3, 64)}
    n3 = int(plain[3][3])
    if n3 not in want:
        want[n3] = oracle_run(n3)
    assert same_run(want[-1], plain)
    assert same_run(want[0], want[1])
    for b in (0, 1, 2, 3):
        if n > b:
            assert want[b][4] > plain[4], (b, want[b][4], plain[4])
        else:
            assert same_run(want[b], plain), b
    if d in QUEUED_D and n >= 9:  # (8 rows or fewer are one row by then)
        assert 2 <= n3 < n
        assert 1 <= host_iterations(want[n3][3], C_ITERS, n3, d) <= 3, list(want[n3][3][:5])
    if d in QUEUED_D and n == 9:
        # the hand-over right behind nested work: iteration 0 is the only host-driven one, and it
        # drew nested hyperplanes (its queued projection was discarded and redone)
        assert host_iterations(want[n3][3], C_ITERS, n3, d) == 1 and nested_draws(want[n3]) > 0
    for b, w in want.items():
        what = f"n={n} d={d} bthr={b}"
        draws = nested_draws(w)
        assert (draws > 0) == (w[4] > plain[4]), (what, draws, w[4], plain[4])
        st = run(engine, data, w, 0.8, C_ITERS, b, what)
        assert (st["nested_calls"] > 0) == (w[4] > plain[4]), (what, st["nested_calls"], w[4])
        assert st["hyperplanes"] == w[4] - COUNTER
        host = host_iterations(w[3], C_ITERS, b, d)
        if 0 < host < C_ITERS:  # host-driven, then queued: only the host's projections are timed
            st = run(engine, data, w, 0.8, C_ITERS, b, what, hip_events=1)
            assert st["project_timed_launches"] == host, (what, st["project_timed_launches"])
