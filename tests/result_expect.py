"""What the device-side result (klsh_result_device, klsh_labels, option "result_device") must be,
derived from the oracle's (rows, offsets, ids) alone — never from the engine.

Nodes number the loaded members in load order, so with `loaded_ids` the member ids as they were
loaded, the node of an id is its position there; labels are the oracle's row index of every
listed id, scattered to those nodes, KLSH_NO_LABEL everywhere else.

Also here: the inputs of the chain-length cases (groups of collinear rows on distinct axes, whose
one klsh_pcluster(0.9) pass chains each group into one list), shared by the GPU tests and the CPU
test that pins what the oracle makes of them.
"""
import numpy as np

import row_state

NO_LABEL = 0xFFFFFFFF
# list lengths on both sides of every power of two up to 2^10: ceil(log2) = 0, 1, 2, 2, 3, 3, 4, ...
CHAIN_SIZES = [1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 65, 128, 129, 1024, 1025]
CHAIN_D = 16
CHAIN_THR = 0.9


def rounds(max_cnt):
    """ceil(log2(max_cnt)), 0 for lists of at most one node: the ranking rounds of a result."""
    return int(max_cnt - 1).bit_length() if max_cnt > 1 else 0


_chain_cache = {}


def chain_rows(n_groups=len(CHAIN_SIZES)):
    """The first n_groups groups: row k of group g is e_g (1 + 0.37 g)(1 + 0.25 k), the rows
    shuffled with a fixed seed.  Returns (rows, group of each row)."""
    if n_groups not in _chain_cache:
        sizes = CHAIN_SIZES[:n_groups]
        n = sum(sizes)
        rows = np.zeros((n, CHAIN_D), np.float32)
        group = np.repeat(np.arange(n_groups), sizes)
        k = np.concatenate([np.arange(s) for s in sizes])
        rows[np.arange(n), group] = ((1 + 0.37 * group) * (1 + 0.25 * k)).astype(np.float32)
        perm = np.random.default_rng(20250 + n_groups).permutation(n)
        rows, group = rows[perm], group[perm]
        rows.setflags(write=False)
        _chain_cache[n_groups] = (rows, group)
    return _chain_cache[n_groups]


def chain_weights(n):
    """Member lists of 1..5 ids per row and a permutation as the ids (row_state.weights)."""
    return row_state.weights(np.random.default_rng(77 + n), n, 6)


_chain_want = {}


def chain_reference(oracle, n_groups, weighted):
    """(rows, off, ids as loaded) and the oracle's p_cluster of them; once per session."""
    key = (n_groups, weighted)
    if key not in _chain_want:
        rows, _ = chain_rows(n_groups)
        n = rows.shape[0]
        if weighted:
            off, ids = chain_weights(n)
            want = oracle.pcluster(rows, CHAIN_THR, off, ids)
        else:
            off, ids = np.arange(n + 1, dtype=np.uint64), np.arange(n, dtype=np.uint64)
            want = oracle.pcluster(rows, CHAIN_THR)
        _chain_want[key] = ((rows, off, ids), want)
    return _chain_want[key]


def expected(want, loaded_ids):
    """(offsets uint32, nodes uint32, labels uint32, rounds) of the oracle result want[:3] for
    members loaded as loaded_ids (distinct)."""
    _, off, ids = want[:3]
    loaded_ids = np.asarray(loaded_ids, np.uint64)
    m = loaded_ids.size
    by_id = np.argsort(loaded_ids, kind="stable")
    at = np.searchsorted(loaded_ids[by_id], ids)
    assert at.size == 0 or (at.max() < m and np.array_equal(loaded_ids[by_id][at], ids))
    nodes = by_id[at].astype(np.uint32)
    assert np.unique(nodes).size == nodes.size
    cnt = np.diff(off.astype(np.int64))
    labels = np.full(m, NO_LABEL, np.uint32)
    labels[nodes] = np.repeat(np.arange(cnt.size, dtype=np.uint32), cnt)
    return off.astype(np.uint32), nodes, labels, rounds(int(cnt.max()) if cnt.size else 0)


def check_device(engine, want, loaded_ids, what):
    """Every device-side output of the engine's current state against the oracle result `want`:
    result_device() (rows by bits, offsets, nodes, labels), the rounds it took, labels(), and
    count() / result() under option result_device = 1.  Returns the device outputs as numpy."""
    off, nodes, labels, r = expected(want, loaded_ids)
    got = [t.cpu().numpy() for t in engine.result_device()]
    assert engine.get_option("member_nodes") == labels.size, what
    assert engine.get_option("result_rounds") == r, (what, engine.get_option("result_rounds"), r)
    assert got[0].shape == want[0].shape and row_state.same_bits(got[0], want[0]), what
    assert got[1].dtype == np.uint32 and np.array_equal(got[1], off), what
    assert got[2].dtype == np.uint32 and np.array_equal(got[2], nodes), what
    assert got[3].dtype == np.uint32 and np.array_equal(got[3], labels), what
    host_labels = engine.labels()
    assert host_labels.dtype == np.uint32 and np.array_equal(host_labels, labels), what
    with row_state.options(engine, result_device=1):
        assert engine.count() == (want[0].shape[0], int(off[-1])), what
        row_state.assert_same_result(engine.result(), *want[:3])
    assert engine.get_option("result_device") == 0
    return got
