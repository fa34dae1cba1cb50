"""The result on the device: klsh_result_device, klsh_labels, klsh_load_rows_device and option
"result_device" against the oracle (tests/result_expect.py derives offsets, nodes and labels from
the oracle's lists; rows are compared by bits).

The member lists are flattened by list ranking in R = ceil(log2(longest list)) rounds of pointer
jumping over two buffers used in turn, so the cases pin R on both sides of every power of two
(one round too few breaks the longest lists of 2^(R-1) + 2 .. 2^R nodes), both buffer parities,
R = 0, lists
the loop interleaved over thousands of nodes, launches of one to three workgroups, nodes no live
row owns, rows loaded from a strided device tensor, and a sharded rank's replica.
"""
import ctypes
import threading

import numpy as np
import pytest
import torch

import result_expect as rx
import row_state
from row_state import LADDER_CALL, check, ladder_reference, options

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------- 1. chain lengths ---------------
@pytest.mark.parametrize("n_groups,want_rounds", [(2, 1), (3, 2), (5, 3), (7, 4), (15, 11),
                                                  (4, 2), (6, 3), (8, 4), (10, 6), (12, 7), (14, 10)])
def test_chain_lengths_singletons(engine, oracle, n_groups, want_rounds):
    """Prefixes of the size list, loaded as singletons: the longest list has 2, 3, 5, 9 and 1025
    nodes, so the ranking takes 1, 2, 3, 4 and 11 rounds; then the prefixes whose longest list
    has 4, 8, 16, 64, 128 and 1024 nodes — a list of 2^r nodes is the one that needs all r
    rounds (its first node is 2^r - 1 links from the end, and r - 1 rounds reach 2^(r-1))."""
    (rows, _, ids), want = rx.chain_reference(oracle, n_groups, False)
    assert rx.expected(want, ids)[3] == want_rounds
    engine.load_rows(rows)
    engine.pcluster(rx.CHAIN_THR)
    rx.check_device(engine, want, ids, f"chains of {rx.CHAIN_SIZES[:n_groups]}")
    assert engine.get_option("result_rounds") == want_rounds


@pytest.mark.parametrize("weighted", [False, True])
def test_no_pass_takes_zero_rounds(engine, weighted):
    """Straight after a load: singletons need no round at all (the init alone ranks them), lists
    of 1..5 loaded ids need 3."""
    rows, _ = rx.chain_rows()
    n = rows.shape[0]
    if weighted:
        off, ids = rx.chain_weights(n)
        engine.load_rows(rows, off, ids)
    else:
        off, ids = np.arange(n + 1, dtype=np.uint64), np.arange(n, dtype=np.uint64)
        engine.load_rows(rows)
    rx.check_device(engine, (rows, off, ids), ids, f"loaded, weighted={weighted}")
    assert engine.get_option("result_rounds") == (3 if weighted else 0)


def test_chain_lengths_weighted(engine, oracle):
    """The 15 groups loaded with lists of 1..5 permuted ids per row: nodes are positions in the
    loaded id list, not ids, and the lists are a few thousand nodes long."""
    (rows, off, ids), want = rx.chain_reference(oracle, len(rx.CHAIN_SIZES), True)
    assert rx.expected(want, ids)[3] >= 11
    engine.load_rows(rows, off, ids)
    engine.pcluster(rx.CHAIN_THR)
    rx.check_device(engine, want, ids, "weighted chains")


# ------------------------------------------------------------- 2. loop-made chains ------------
LADDERS = [(40000, 16), (30000, 13)]


@pytest.mark.parametrize("bthr", [1000000, 5000])
@pytest.mark.parametrize("n,d", LADDERS)
def test_loop_made_chains(engine, oracle, n, d, bthr):
    """Six weighted iterations: lists of thousands of nodes interleaved by real merges (d = 13:
    the row gather skips the pad).  Also right after the load, where the offsets scan has a tile
    per 2048 of the n live rows."""
    (rows, off, ids), want = ladder_reference(oracle, n, d, bthr)
    min_sim, iters, seed, counter = LADDER_CALL
    engine.load_rows(rows, off, ids)
    rx.check_device(engine, (rows, off, ids), ids, f"ladder n={n} d={d} loaded")
    trace, c, _ = engine.cluster(min_sim, iters, bthr, seed, counter)
    assert np.array_equal(trace, want[3]) and c == want[4]
    assert int(np.diff(want[1].astype(np.int64)).max()) > 2048
    rx.check_device(engine, want, ids, f"ladder n={n} d={d} bthr={bthr}")


# ------------------------------------------------------------- 3. capped grids ----------------
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_grid_cap(engine, oracle, cap):
    """Every launch at 1, 2 and 3 workgroups: each workgroup takes several trips over the nodes
    (256 per trip) and over the offsets scan's tiles, and the outputs do not change."""
    (rows, off, ids), want = rx.chain_reference(oracle, len(rx.CHAIN_SIZES), True)
    assert rows.shape[0] == 2500 and -(-rows.shape[0] // 256) == 10  # the singleton nodes' tiles
    assert -(-ids.size // 256) >= 10 and 10 // cap >= 3
    engine.load_rows(rows, off, ids)
    engine.pcluster(rx.CHAIN_THR)
    base = rx.check_device(engine, want, ids, "chains, uncapped")
    with options(engine, grid_cap=cap):
        got = rx.check_device(engine, want, ids, f"chains, grid_cap={cap}")
    assert all(np.array_equal(a, b) for a, b in zip(base, got))

    n, d = LADDERS[0]
    (rows, off, ids), want = ladder_reference(oracle, n, d, 1000000)
    min_sim, iters, seed, counter = LADDER_CALL
    assert -(-n // 2048) >= 3 * cap  # offsets tiles of the loaded state
    with options(engine, grid_cap=cap):
        engine.load_rows(rows, off, ids)
        rx.check_device(engine, (rows, off, ids), ids, f"ladder loaded, grid_cap={cap}")
        engine.cluster(min_sim, iters, 1000000, seed, counter)
        rx.check_device(engine, want, ids, f"ladder, grid_cap={cap}")


# ------------------------------------------------------------- 4. dropped rows ----------------
def test_dropped_rows_have_no_label(engine, oracle):
    """klsh_load_counts drops the rows with sum(count) <= 0.1 d: their nodes exist (node k is
    batch row k) and no live row owns them — right after the load and after three iterations."""
    rng = np.random.default_rng(8)
    d, n_total, batch_offset, batch_size = 8, 5600, 333, 5000
    profile = rng.uniform(1.0, 40.0, size=(60, d))
    counts = rng.poisson(profile[rng.integers(0, 60, n_total)].T).astype(np.uint16)
    counts[:, rng.integers(0, n_total, 700)] = 0
    v_kmers = rng.uniform(0.5, 2.0, d).astype(np.float32)
    w_rows, w_ids = oracle.convert(counts, v_kmers, batch_offset, batch_size)
    kept = w_ids.astype(np.int64) - batch_offset
    dropped = np.setdiff1d(np.arange(batch_size), kept)
    assert 100 < dropped.size < batch_size - 2048
    loaded_ids = batch_offset + np.arange(batch_size, dtype=np.uint64)
    off = np.arange(len(w_ids) + 1, dtype=np.uint64)

    engine.load_counts(counts, v_kmers, batch_offset, batch_size)
    got = rx.check_device(engine, (w_rows, off, w_ids), loaded_ids, "load_counts")
    assert np.array_equal(np.flatnonzero(got[3] == rx.NO_LABEL), dropped)
    assert np.array_equal(got[2], kept)

    want = oracle.cluster(w_rows, 0.8, 3, 1000000, 777, 3, off, w_ids)
    assert want[3][-1] < want[3][0]
    trace, c, _ = engine.cluster(0.8, 3, 1000000, 777, 3)
    assert np.array_equal(trace, want[3]) and c == want[4]
    got = rx.check_device(engine, want, loaded_ids, "load_counts + 3 iterations")
    assert np.array_equal(np.flatnonzero(got[3] == rx.NO_LABEL), dropped)


# ------------------------------------------------------------- 5. device load -----------------
@pytest.mark.parametrize("d", [13, 64])
def test_load_rows_from_device_tensor(engine, oracle, d):
    """A column slice of a wider GPU tensor (row stride > d, start not 16-byte aligned): the
    state equals what klsh_load_rows leaves — norms, image, pad, chains — and a loop on it
    equals the oracle's."""
    n = 6000
    rows = row_state.ladder(n, d)[0]
    wide = np.full((n, d + 11), np.float32(7.5))
    wide[:, 3:3 + d] = rows
    t = torch.from_numpy(wide).to(f"cuda:{engine.device}")[:, 3:3 + d]
    assert t.stride() == (d + 11, 1) and t.data_ptr() % 16 != 0
    engine.load_rows(t)
    ids = np.arange(n, dtype=np.uint64)
    single = (rows, np.arange(n + 1, dtype=np.uint64), ids)
    st = check(engine, single, f"device load d={d}")
    assert (st["image"] is not None) == (d == 64)
    rx.check_device(engine, single, ids, f"device load d={d}")
    want = oracle.cluster(rows, 0.8, 3, 1000000, 777, 3)
    assert want[3][-1] < want[3][0]
    trace, c, _ = engine.cluster(0.8, 3, 1000000, 777, 3)
    assert np.array_equal(trace, want[3]) and c == want[4]
    check(engine, want, f"device load d={d} + 3 iterations")
    rx.check_device(engine, want, ids, f"device load d={d} + 3 iterations")
    # member ids of the caller's
    my_ids = (ids * 3 + 5).astype(np.uint64)
    engine.load_rows(t, member_ids=my_ids)
    assert np.array_equal(engine.result()[2], my_ids)


def test_load_rows_device_arguments():
    """A host pointer, a CPU tensor's memory and a row stride below d are KLSH_E_ARG and load
    nothing; n = 0 is a valid load; a CPU tensor through Engine.load_rows goes the numpy way."""
    from kmerlsh_amd import _native

    lib = _native.load_library()
    rows = np.random.default_rng(5).normal(0, 1, size=(300, 16)).astype(np.float32)
    with _native.Engine(0) as eng:
        dev = torch.from_numpy(rows).to(f"cuda:{eng.device}")
        cpu = torch.from_numpy(rows)
        P = ctypes.c_void_p
        for ptr, stride in [(P(rows.ctypes.data), 16), (P(cpu.data_ptr()), 16),
                            (P(dev.data_ptr()), 15)]:
            assert lib.klsh_load_rows_device(eng._ctx, ptr, 300, 16, stride, None) == -1  # E_ARG
            with pytest.raises(_native.KlshError, match="KLSH_E_STATE"):
                eng.count()
        host_out = np.zeros(300, np.uint32)
        eng.load_rows(dev)
        assert lib.klsh_result_device(eng._ctx, None, None, None, P(host_out.ctypes.data)) == -1
        assert eng.count() == (300, 300)
        assert lib.klsh_load_rows_device(eng._ctx, None, 0, 16, 16, None) == 0
        assert eng.count() == (0, 0)
        out = eng.result_device()
        assert [tuple(t.shape) for t in out] == [(0, 16), (1,), (0,), (0,)]
        assert int(out[1][0].item()) == 0 and eng.labels().size == 0
        eng.load_rows(cpu)
        assert eng.count() == (300, 300)
        row_state.assert_same_result(eng.result(), rows, np.arange(301), np.arange(300))
        with pytest.raises(_native.KlshError):
            eng.load_rows(dev.to(torch.float64))


# ------------------------------------------------------------- 6. sharded replica -------------
def test_sharded_rank_result_device(engine, oracle):
    """W = 2 in-process ranks over a ladder case: each rank's result_device() equals the oracle's
    and the single-GPU engine's."""
    from kmerlsh_amd import _native

    n, d = LADDERS[0]
    (rows, off, ids), want = ladder_reference(oracle, n, d, 1000000)
    min_sim, iters, seed, counter = LADDER_CALL
    engine.load_rows(rows, off, ids)
    engine.cluster(min_sim, iters, 1000000, seed, counter)
    base = rx.check_device(engine, want, ids, "single GPU")
    engines = [_native.Engine(0) for _ in range(2)]
    try:
        for e in engines:
            e.load_rows(rows, off, ids)
            e.set_option("shard_min_rows", 0)
        _native.comm_init_local(engines)
        errs = []

        def work(r):
            try:
                trace, c, st = engines[r].cluster(min_sim, iters, 1000000, seed, counter)
                assert st["world"] == 2 and np.array_equal(trace, want[3]) and c == want[4]
            except Exception as ex:  # surfaced below
                errs.append((r, ex))

        ts = [threading.Thread(target=work, args=(r,)) for r in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=600)
        assert not any(t.is_alive() for t in ts), "sharded call hung"
        assert not errs, errs
        for r, e in enumerate(engines):
            got = rx.check_device(e, want, ids, f"rank {r}")
            assert all(np.array_equal(a, b) for a, b in zip(base, got))
    finally:
        for e in engines:
            e.close()
