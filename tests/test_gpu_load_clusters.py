"""klsh_load_clusters_device (Engine.load_clusters): rows that already have member lists, loaded
from device memory — the inverse of klsh_result_device.

The state it leaves must be the one klsh_load_rows leaves for the same rows and lists, with the
nodes numbered the caller's way: result() by bits, the cached row state (row_state.check), the
device result in the caller's nodes (result_expect.check_device), and loops on it against the
oracle.  The two passes work per entry over tiles of 256, so the edge cases put list starts and
ends on and beside multiples of 256, one list over several tiles, windows with offsets[0] != 0,
nodes no list holds, and launches of one to three workgroups.  Every refusal must leave the
previous load as it was.
"""
import ctypes

import numpy as np
import pytest
import torch

import result_expect as rx
import row_state
from row_state import LADDER_CALL, check, ladder_reference, options

pytestmark = pytest.mark.gpu

SEED, COUNTER = 777, 3
BTHR = 1000000
E_ARG, E_STATE, E_RANGE = -1, -4, -6


def dev_of(engine):
    return f"cuda:{engine.device}"


def dev_u32(engine, a):
    """A host integer array as an int32 device tensor (the same bits as uint32 below 2^31)."""
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(dev_of(engine))


def as_i64(t):
    """A uint32 device tensor as int64 (values below 2^31), for arithmetic on the device."""
    return t.view(torch.int32).to(torch.int64)


def strided_rows(engine, rows):
    """The rows as a column slice of a wider device tensor: row stride d + 11, the start not
    16-byte aligned."""
    n, d = rows.shape
    wide = np.full((n, d + 11), np.float32(7.5))
    wide[:, 3:3 + d] = rows
    t = torch.from_numpy(wide).to(dev_of(engine))[:, 3:3 + d]
    assert t.stride() == (d + 11, 1) and t.data_ptr() % 16 != 0
    return t


def distinct_ids(rng, count):
    ids = np.unique(rng.integers(0, 1 << 63, 2 * count + 16, dtype=np.uint64))
    assert ids.size >= count
    return rng.permutation(ids)[:count]


def permuted_nodes(rng, m, spare):
    """m listed nodes and `spare` unlisted ones out of M = m + spare, and distinct ids by node."""
    perm = rng.permutation(m + spare).astype(np.uint32)
    return perm[:m], np.sort(perm[m:]), distinct_ids(rng, m + spare)


def load_and_check(engine, rows, off, nodes, ids_by_node, what, strided=False):
    """Load (rows, off, nodes) through the device into a new node space of ids_by_node.size nodes
    and check every view of the state against the host-side meaning of the same lists.  nodes
    None: entry q is node q - off[0].  Returns (row state, device outputs)."""
    off = np.asarray(off, np.uint64)
    big_m = ids_by_node.size
    t = strided_rows(engine, rows) if strided else torch.from_numpy(rows).to(dev_of(engine))
    engine.load_clusters(t, dev_u32(engine, off), None if nodes is None else dev_u32(engine, nodes),
                         n_nodes=big_m, member_ids=ids_by_node)
    m = int(off[-1] - off[0])
    listed = (np.arange(m, dtype=np.uint32) if nodes is None
              else np.asarray(nodes)[int(off[0]):int(off[-1])])
    single = (rows, off - off[0], ids_by_node[listed])
    assert engine.count() == (rows.shape[0], m), what
    st = check(engine, single, what)
    got = rx.check_device(engine, single, ids_by_node, what)
    assert engine.get_option("member_nodes") == big_m, what
    unlisted = np.setdiff1d(np.arange(big_m), listed)
    assert np.array_equal(np.flatnonzero(got[3] == rx.NO_LABEL), unlisted), what
    return st, got


# ------------------------------------------------------------- 1. the host load's state -------
def case_rows(kind, n, d):
    if kind == "chain":
        rows = rx.chain_rows()[0]
        assert rows.shape == (n, d)
        return rows, rx.chain_weights(n)[0]
    rows, off, _ = row_state.ladder(n, d)
    return rows, off


@pytest.mark.parametrize("kind,n,d", [("chain", 2500, 16), ("ladder", 6000, 13),
                                      ("ladder", 6000, 64)])
def test_state_equals_host_load(engine, kind, n, d):
    """Lists of 1..5 nodes, the nodes a random permutation of M = m + 37 (37 in no list), ids by
    node distinct random uint64, the rows a strided misaligned slice: result, norms, counts, pad,
    image and chain links are the host load's, the device result speaks in the caller's nodes."""
    rows, off = case_rows(kind, n, d)
    rng = np.random.default_rng(1000 + n + d)
    m = int(off[-1])
    nodes, unlisted, ids_by_node = permuted_nodes(rng, m, 37)
    st, got = load_and_check(engine, rows, off, nodes, ids_by_node, f"{kind} n={n} d={d}", True)
    # (an fp16 image is kept at d = 16, 32, 64: of the ladder widths here, exactly at 64)
    assert (st["image"] is not None) == (d in (16, 32, 64))
    assert engine.get_option("result_rounds") == 3
    assert np.array_equal(np.flatnonzero(got[3] == rx.NO_LABEL), unlisted) and unlisted.size == 37
    assert np.array_equal(got[2], nodes)
    engine.load_rows(rows, off, ids_by_node[nodes])
    host = engine.row_state()
    assert row_state.same_state(st, host)


# ------------------------------------------------------------- 2. a loop on it ----------------
@pytest.mark.parametrize("n,d", [(40000, 16), (30000, 13)])
def test_loop_on_device_loaded_lists(engine, oracle, n, d):
    """The ladder references' inputs through the device, nodes permuted: six iterations give the
    oracle's trace, counter, result, row state and device result."""
    (rows, off, ids), want = ladder_reference(oracle, n, d, BTHR)
    min_sim, iters, seed, counter = LADDER_CALL
    m = ids.size
    nodes = np.random.default_rng(n + 7 * d).permutation(m).astype(np.uint32)
    ids_by_node = np.zeros(m, np.uint64)
    ids_by_node[nodes] = ids
    engine.load_clusters(strided_rows(engine, rows), dev_u32(engine, off), dev_u32(engine, nodes),
                         n_nodes=m, member_ids=ids_by_node)
    # (before the loop: a merge rewrites the link of the tail it appends to, and can mend a list)
    check(engine, (rows, off, ids), f"ladder n={n} d={d} loaded through the device")
    trace, c, _ = engine.cluster(min_sim, iters, BTHR, seed, counter)
    assert np.array_equal(trace, want[3]) and c == want[4]
    check(engine, want, f"ladder n={n} d={d} through the device")
    rx.check_device(engine, want, ids_by_node, f"ladder n={n} d={d} through the device")


# ------------------------------------------------------------- 3. round trips, keep mode ------
ROUND_N, ROUND_ITERS, ROUND_SIM = 6000, 3, 0.8
_round_cache = {}


def big_clusters(off):
    """The filter of variant (b) on host offsets: (row mask, entry mask) of the clusters with more
    than 5 members."""
    cnt = np.diff(off.astype(np.int64))
    keep = cnt > 5
    return keep, np.repeat(keep, cnt)


def window(n_out):
    """The rows [a, b) of variant (c): a = 257 and b = n_out - 3 where call 1 leaves that many
    rows (after one iteration: 966 rows at d = 16, 806 at d = 64).  Its three iterations leave 133
    and 34, so there the window starts a quarter in; either way offsets[a] != 0 and neither edge
    is a multiple of 256."""
    a, b = (257 if n_out > 2 * 257 else n_out // 4 + 1), n_out - 3
    assert 0 < a < b and a % 256 and b % 256
    return a, b


def round_reference(oracle, d, iters1=ROUND_ITERS):
    """The ladder rows, the oracle's first call on them (iters1 iterations), and its second call
    on the first's output whole, filtered and windowed; once per session."""
    if (d, iters1) not in _round_cache:
        rows, off, ids = row_state.ladder(ROUND_N, d)
        w1 = oracle.cluster(rows, ROUND_SIM, iters1, BTHR, SEED, COUNTER, off, ids)
        r1, o1, i1, _, c1 = w1
        second = lambda r, o, i: oracle.cluster(r, ROUND_SIM, ROUND_ITERS, BTHR, SEED, c1, o, i)
        keep, ent = big_clusters(o1)
        a, b = window(r1.shape[0])
        lo, hi = int(o1[a]), int(o1[b])
        filt = (r1[keep], np.concatenate([[0], np.cumsum(np.diff(o1.astype(np.int64))[keep])])
                .astype(np.uint64), i1[ent])
        win = (r1[a:b], o1[a:b + 1] - o1[a], i1[lo:hi])
        _round_cache[d, iters1] = {"in": (rows, off, ids), "w1": w1, "iters1": iters1,
                                   "whole": second(r1, o1, i1),
                                   "filter_in": filt, "filter": second(*filt),
                                   "window_in": win, "window": second(*win)}
    return _round_cache[d, iters1]


def first_call(engine, ref):
    """Call 1 on the engine; its device result."""
    rows, off, ids = ref["in"]
    w1 = ref["w1"]
    engine.load_rows(rows, off, ids)
    trace, c, _ = engine.cluster(ROUND_SIM, ref["iters1"], BTHR, SEED, COUNTER)
    assert np.array_equal(trace, w1[3]) and c == w1[4]
    assert w1[0].shape[0] < ROUND_N  # call 1 merges
    return engine.result_device(), c


def second_call(engine, ref, which, c1, what):
    """Call 2 from call 1's counter against the oracle's second result: by bits, then the row
    state and the device result in the nodes of the FIRST load."""
    want = ref[which]
    n_in = ref[which + "_in"][0].shape[0] if which != "whole" else ref["w1"][0].shape[0]
    assert want[0].shape[0] < n_in, what  # call 2 merges
    trace, c, _ = engine.cluster(ROUND_SIM, ROUND_ITERS, BTHR, SEED, c1)
    assert np.array_equal(trace, want[3]) and c == want[4], what
    row_state.assert_same_result(engine.result(), *want[:3])
    check(engine, want, what)
    return rx.check_device(engine, want, ref["in"][2], what)


@pytest.mark.parametrize("d,iters1", [(16, 3), (64, 3), (16, 1), (64, 1)])
def test_round_trip_whole(engine, oracle, d, iters1):
    """(a) result_device() straight back in: nothing changes, and the second call is the
    oracle's.  (After a first call of one iteration lists start on multiples of 256 entries.)"""
    ref = round_reference(oracle, d, iters1)
    what = f"d={d}, call 1 of {iters1}, whole"
    (r, o, nd, _), c1 = first_call(engine, ref)
    engine.load_clusters(r, o, nd)
    check(engine, ref["w1"], what)
    rx.check_device(engine, ref["w1"], ref["in"][2], what)
    got = second_call(engine, ref, "whole", c1, what + ", second call")
    assert not (got[3] == rx.NO_LABEL).any()


@pytest.mark.parametrize("d,iters1", [(16, 3), (64, 3), (64, 1)])
def test_round_trip_filtered(engine, oracle, d, iters1):
    """(b) only the clusters with more than 5 members go back in, masks and offsets built on the
    device; the dropped clusters' nodes have no label afterwards.  (After a first call of one
    iteration at d = 64 a kept list starts on a multiple of 256 entries.)"""
    ref = round_reference(oracle, d, iters1)
    (r, o, nd, _), c1 = first_call(engine, ref)
    cnt = as_i64(o).diff()
    keep = cnt > 5
    ent = torch.repeat_interleave(keep, cnt)
    off2 = torch.cat([cnt.new_zeros(1), cnt[keep].cumsum(0)]).to(torch.int32)
    h_keep, h_ent = big_clusters(ref["w1"][1])
    assert 0 < h_keep.sum() < h_keep.size and np.array_equal(keep.cpu().numpy(), h_keep)
    engine.load_clusters(r[keep], off2, nd.view(torch.int32)[ent])
    check(engine, ref["filter_in"], f"d={d}, call 1 of {iters1}, filtered")
    got = second_call(engine, ref, "filter", c1, f"d={d}, call 1 of {iters1}, filtered, second call")
    dropped = rx.expected(ref["w1"], ref["in"][2])[1][~h_ent]
    assert dropped.size and np.array_equal(np.flatnonzero(got[3] == rx.NO_LABEL), np.sort(dropped))


@pytest.mark.parametrize("d,iters1", [(16, 3), (64, 3), (16, 1), (64, 1)])
def test_round_trip_window(engine, oracle, d, iters1):
    """(c) rows [a, b) with offsets[a .. b] against the WHOLE node array: offsets[0] != 0, neither
    edge a multiple of 256 (window()).  The state is the host load's of the same slice, before
    and after the second call.  After a first call of one iteration a = 257, and lists start on
    multiples of 256 entries inside the window."""
    ref = round_reference(oracle, d, iters1)
    what = f"d={d}, call 1 of {iters1}, window"
    win = ref["window_in"]
    engine.load_rows(*win)
    host = engine.row_state()
    (r, o, nd, _), c1 = first_call(engine, ref)
    a, b = window(r.shape[0])
    lo, hi = int(ref["w1"][1][a]), int(ref["w1"][1][b])
    assert lo > 0 and lo % 256 and hi % 256 and (a == 257) == (iters1 == 1)
    engine.load_clusters(r[a:b], o[a:b + 1], nd)
    st = check(engine, win, what)
    assert row_state.same_state(st, host)
    assert engine.count() == (b - a, hi - lo)
    got = second_call(engine, ref, "window", c1, what + ", second call")
    outside = np.concatenate([ref["w1"][2][:lo], ref["w1"][2][hi:]])
    node_of = np.argsort(ref["in"][2])  # (the loaded ids are a permutation: id -> node)
    assert np.array_equal(np.flatnonzero(got[3] == rx.NO_LABEL),
                          np.sort(node_of[outside.astype(np.int64)]))


# ------------------------------------------------------------- 4. two engines joined ----------
def test_two_engines_joined(engine, oracle):
    """Two engines cluster 3000 rows each; rows, offsets and nodes are concatenated on the device
    into a node space of n1 + n2 and clustered again: the reference's init pass in miniature,
    against the oracle run on the concatenation of its own two outputs."""
    from kmerlsh_amd import _native

    d, n1, n2 = 16, 3000, 3000
    x = row_state.ladder(n1 + n2, d)[0]
    x1, x2 = x[:n1], x[n1:]
    call = lambda r, c, o=None, i=None: oracle.cluster(r, ROUND_SIM, ROUND_ITERS, BTHR, SEED, c, o, i)
    w1, w2 = call(x1, COUNTER), call(x2, COUNTER)
    assert w1[0].shape[0] < n1 and w2[0].shape[0] < n2
    m1 = int(w1[1][-1])
    assert m1 == n1
    joined = (np.vstack([w1[0], w2[0]]), np.concatenate([w1[1], w2[1][1:] + np.uint64(m1)]),
              np.concatenate([w1[2], w2[2] + np.uint64(n1)]))
    want = call(joined[0], w1[4], joined[1], joined[2])
    assert want[0].shape[0] < joined[0].shape[0]

    with _native.Engine(engine.device) as other:
        engine.load_rows(x1)
        other.load_rows(x2)
        for e, w in ((engine, w1), (other, w2)):
            trace, c, _ = e.cluster(ROUND_SIM, ROUND_ITERS, BTHR, SEED, COUNTER)
            assert np.array_equal(trace, w[3]) and c == w[4]
        r1, o1, nd1, _ = engine.result_device()
        r2, o2, nd2, _ = other.result_device()
        rows = torch.cat([r1, r2])
        off = torch.cat([as_i64(o1), as_i64(o2)[1:] + m1]).to(torch.int32)
        nodes = torch.cat([as_i64(nd1), as_i64(nd2) + n1]).to(torch.int32)
    engine.load_clusters(rows, off, nodes, n_nodes=n1 + n2)
    ids = np.arange(n1 + n2, dtype=np.uint64)
    check(engine, joined, "joined, loaded")
    rx.check_device(engine, joined, ids, "joined, loaded")
    trace, c, _ = engine.cluster(ROUND_SIM, ROUND_ITERS, BTHR, SEED, w1[4])
    assert np.array_equal(trace, want[3]) and c == want[4]
    check(engine, want, "joined, clustered")
    rx.check_device(engine, want, ids, "joined, clustered")


# ------------------------------------------------------------- 5. edges of the two passes -----
EDGES = {
    # name: (offsets, nodes given, spare nodes)
    "one row, one entry": ([0, 1], True, 0),
    "one row, 2049 entries": ([0, 2049], True, 0),
    "one row, 2049 entries, m < M": ([0, 2049], True, 5),
    "tile edges": ([0, 100, 256, 512, 513, 600, 768, 1024, 1025], True, 5),
    "tile edges, m = M": ([0, 100, 256, 512, 513, 600, 768, 1024, 1025], True, 0),
    "no node array": ([0, 100, 256, 512, 513, 600], False, 0),
    "no node array, window, m < M": ([7, 9, 263, 519, 520, 775], False, 6),
    "window into a longer node array": ([255, 256, 300, 512, 1024, 1100], True, 3),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edges(engine, name):
    """Lists that start and end on multiples of 256 entries (the link pass decides from the start
    map alone whether entry q + 1 continues entry q's list), one list over several tiles, a
    one-entry list, windows with offsets[0] != 0, with and without a node array, m = M and m < M."""
    off, given, spare = EDGES[name]
    off = np.asarray(off, np.uint64)
    n, m = off.size - 1, int(off[-1] - off[0])
    rng = np.random.default_rng(40 + n + m)
    rows = rng.normal(0, 1, size=(n, 16)).astype(np.float32)
    if given:  # an array of off[n] entries: what lies before off[0] belongs to other rows
        total = int(off[-1])
        perm = rng.permutation(total + spare).astype(np.uint32)
        nodes, ids_by_node = perm[:total], distinct_ids(rng, total + spare)
    else:
        nodes, ids_by_node = None, distinct_ids(rng, m + spare)
    st, got = load_and_check(engine, rows, off, nodes, ids_by_node, name)
    assert np.array_equal(st["cnt"], np.diff(off.astype(np.int64)))


def test_empty_load(engine):
    """n = 0 with a node space of 5: no rows, no members, five unlabelled nodes."""
    rows = torch.zeros((0, 16), dtype=torch.float32, device=dev_of(engine))
    engine.load_clusters(rows, dev_u32(engine, [0]), None, n_nodes=5)
    assert engine.count() == (0, 0)
    assert engine.get_option("member_nodes") == 5
    labels = engine.labels()
    assert labels.size == 5 and (labels == rx.NO_LABEL).all()
    assert [tuple(t.shape) for t in engine.result_device()] == [(0, 16), (1,), (0,), (5,)]


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_grid_cap(engine, oracle, cap):
    """Both passes at 1, 2 and 3 workgroups over the reloaded weighted chains (ten tiles of 256
    entries and more, lists of over 1000 nodes): several trips per workgroup, the same outputs."""
    (rows, off, ids), want = rx.chain_reference(oracle, len(rx.CHAIN_SIZES), True)
    assert -(-ids.size // 256) >= 10 and 10 // cap >= 3
    assert int(np.diff(want[1].astype(np.int64)).max()) > 1000
    engine.load_rows(rows, off, ids)
    engine.pcluster(rx.CHAIN_THR)
    r, o, nd, _ = engine.result_device()
    engine.load_clusters(r, o, nd)
    base_state = check(engine, want, "chains reloaded, uncapped")
    base = rx.check_device(engine, want, ids, "chains reloaded, uncapped")
    with options(engine, grid_cap=cap):
        engine.load_clusters(r, o, nd)
        state = check(engine, want, f"chains reloaded, grid_cap={cap}")
        got = rx.check_device(engine, want, ids, f"chains reloaded, grid_cap={cap}")
    assert row_state.same_state(base_state, state)
    assert all(np.array_equal(a, b) for a, b in zip(base, got))


# ------------------------------------------------------------- 6. refusals --------------------
class Refusals:
    """Raw calls of klsh_load_clusters_device on an engine that holds a clustered state; after
    every refusal count() and result() must return what they returned before."""

    def __init__(self, engine, oracle):
        from kmerlsh_amd import _native

        self.native, self.lib, self.engine = _native, _native.load_library(), engine
        ref = round_reference(oracle, 16)
        first_call(engine, ref)
        self.before = (engine.count(), engine.result(), engine.labels())
        rng = np.random.default_rng(61)
        self.n, self.d = 1000, 16
        self.rows = rng.normal(0, 1, size=(self.n, self.d)).astype(np.float32)
        self.off = row_state.weights(rng, self.n, 6)[0].astype(np.uint32)
        self.m = int(self.off[-1])
        self.big_m = self.m + 9
        self.nodes = rng.permutation(self.big_m)[:self.m].astype(np.uint32)
        self.keep = []  # device tensors stay alive until the call returns

    def dev(self, a):
        a = np.ascontiguousarray(a)
        a = a.view(np.int32) if a.dtype == np.uint32 else a
        t = torch.from_numpy(a).to(dev_of(self.engine))
        self.keep.append(t)
        return ctypes.c_void_p(t.data_ptr())

    @staticmethod
    def host(a):
        return ctypes.c_void_p(a.ctypes.data)

    def call(self, rows=None, off=None, nodes=None, d=None, stride=None, n_nodes=None, ids=None):
        P = ctypes.c_void_p
        d = self.d if d is None else d
        rc = self.lib.klsh_load_clusters_device(
            self.engine._ctx, self.dev(self.rows) if rows is None else rows, self.n, d,
            self.d if stride is None else stride,
            self.dev(self.off) if off is None else off,
            self.dev(self.nodes) if nodes is None else nodes,
            self.big_m if n_nodes is None else n_nodes,
            None if ids is None else P(ids.ctypes.data))
        torch.cuda.synchronize()
        return rc, self.lib.klsh_last_error().decode()

    def refused(self, code, text, **kw):
        rc, msg = self.call(**kw)
        assert rc == code, (rc, msg, kw.keys())
        for part in ([text] if isinstance(text, str) else text):
            assert part in msg, (msg, part)
        count, (rows, off, ids), labels = self.before
        assert self.engine.count() == count, msg
        row_state.assert_same_result(self.engine.result(), rows, off, ids)
        assert np.array_equal(self.engine.labels(), labels), msg


def test_refused_arguments(engine, oracle):
    """Pointers that are not device memory, a stride below d, d outside [1, 4096], member ids in
    keep mode: refused, the clustered state untouched.  Then the unchanged arguments load."""
    t = Refusals(engine, oracle)
    t.refused(E_ARG, "d_rows", rows=t.host(t.rows))
    t.refused(E_ARG, "d_member_offsets", off=t.host(t.off))
    t.refused(E_ARG, "d_member_nodes", nodes=t.host(t.nodes))
    t.refused(E_ARG, "row_stride", stride=t.d - 1)
    t.refused(E_RANGE, "d must be", d=0)
    t.refused(E_RANGE, "d must be", d=4097, stride=4097)
    t.refused(E_ARG, "member_ids", n_nodes=0, ids=np.arange(t.big_m, dtype=np.uint64))
    rc, msg = t.call()
    assert rc == 0, msg
    assert engine.count() == (t.n, t.m) and engine.get_option("member_nodes") == t.big_m


def test_refused_lists(engine, oracle):
    """Offsets that do not strictly increase, nodes out of range or listed twice, more entries
    than nodes: refused with the smallest offending row or entry named, whatever else is wrong
    further on, the clustered state untouched."""
    t = Refusals(engine, oracle)
    off = t.off.copy()
    off[701] = off[700] - 1  # row 700 decreases (row 701 grows again)
    off[901] = off[900] - 1
    t.refused(E_ARG, ["strictly increasing", "row 700 "], off=t.dev(off))
    off = t.off.copy()
    off[501] = off[500]
    t.refused(E_ARG, ["strictly increasing", "row 500 "], off=t.dev(off))
    off = t.off.copy()
    off[1] = off[0]  # (the first row, and a later one)
    off[501] = off[500]
    t.refused(E_ARG, "row 0 ", off=t.dev(off))

    m = t.m
    nodes = t.nodes.copy()
    nodes[1234] = t.big_m
    nodes[2000] = t.big_m + 5
    t.refused(E_ARG, ["entry 1234 ", f"node {t.big_m},"], nodes=t.dev(nodes))
    nodes = t.nodes.copy()
    nodes[m - 2] = nodes[3]
    t.refused(E_ARG, [f"entry {m - 2} ", "twice", "first at entry 3)"], nodes=t.dev(nodes))
    nodes = t.nodes.copy()
    nodes[778] = nodes[777]
    t.refused(E_ARG, ["entry 778 ", "twice", "first at entry 777)"], nodes=t.dev(nodes))
    nodes[m - 2] = nodes[3]  # both repeats: the smaller entry is named
    t.refused(E_ARG, ["entry 778 ", "twice"], nodes=t.dev(nodes))
    nodes[300] = nodes[1]
    nodes[400] = nodes[1]  # three entries of one node: the second of them
    t.refused(E_ARG, ["entry 300 ", "first at entry 1)"], nodes=t.dev(nodes))
    nodes[200] = t.big_m  # a node out of range before every repeat
    t.refused(E_ARG, ["entry 200 ", "not below"], nodes=t.dev(nodes))

    t.refused(E_ARG, "more than", n_nodes=m - 1)  # m = M + 1
    # the window of a longer node array: the caller's index is named
    shift = 50
    nodes = np.concatenate([np.zeros(shift, np.uint32), t.nodes])
    nodes[shift + 11] = nodes[shift + 10]
    t.refused(E_ARG, f"entry {shift + 11} ", off=t.dev(t.off + np.uint32(shift)), nodes=t.dev(nodes))


def test_keep_mode_needs_a_load(engine):
    """n_nodes = 0 on a fresh engine is KLSH_E_STATE; Engine.load_rows still refuses member
    offsets with a device tensor, in the words it always used."""
    from kmerlsh_amd import _native

    lib = _native.load_library()
    rows = torch.zeros((4, 16), dtype=torch.float32, device=dev_of(engine))
    off = dev_u32(engine, [0, 1, 2, 3, 4])
    P = ctypes.c_void_p
    with _native.Engine(engine.device) as fresh:
        assert lib.klsh_load_clusters_device(fresh._ctx, P(rows.data_ptr()), 4, 16, 16,
                                             P(off.data_ptr()), None, 0, None) == E_STATE
        with pytest.raises(_native.KlshError, match="KLSH_E_STATE"):
            fresh.count()
        with pytest.raises(_native.KlshError, match="KLSH_E_STATE"):
            fresh.load_clusters(rows, off)
        fresh.load_clusters(rows, off, n_nodes=4)
        assert fresh.count() == (4, 4)
        fresh.load_clusters(rows[:2], off[2:], dev_u32(engine, [0, 1, 2, 3]))  # keep: nodes 2, 3
        assert fresh.count() == (2, 2)
        assert np.array_equal(fresh.labels(), np.array([rx.NO_LABEL, rx.NO_LABEL, 0, 1], np.uint32))
        assert np.array_equal(fresh.result()[2], [2, 3])
    with pytest.raises(_native.KlshError, match="singleton rows"):
        engine.load_rows(rows, member_offsets=np.arange(5))
