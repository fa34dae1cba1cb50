"""klsh_save_clusters (Engine.save_clusters): the reference's two cluster files, formatted and
written from the device.

Unless a case names another expectation, both files are compared byte for byte with
kmerlsh_amd.io.save_result / save_binary of engine.result() — the slow Python writers that
tests/test_save_expect.py ties to the reference's own IOMat::SaveResult / SaveBinary.  The cases:
every digit count of a uint64, the seeded reference CLI's md5s, the ignore_small edge on both
sides, list starts and row counts on the kernels' tile edges, lists interleaved by real merges,
every chunk size around the text's length (a chunk edge inside a token, a row larger than a
chunk), text positions past 2^32, launches of one to three workgroups, the state left untouched,
the refusals, and a sharded rank's replica.
"""
import ctypes
import hashlib
import json
import os
import sys
import threading

import numpy as np
import pytest
import torch

import result_expect as rx
import row_state
from conftest import GOLDEN, golden
from kmerlsh_amd import _native, io
from row_state import LADDER_CALL, ladder_reference, options

sys.path.insert(0, GOLDEN)
import kat_inputs  # noqa: E402

pytestmark = pytest.mark.gpu


def expected_files(tmp_path, result, ignore_small):
    rows, off, ids = result[:3]
    io.save_result(str(tmp_path / "want.clust"), off, ids, ignore_small)
    io.save_binary(str(tmp_path / "want"), np.ascontiguousarray(rows), off, ignore_small)
    return (tmp_path / "want.clust").read_bytes(), (tmp_path / "want").read_bytes()


def save(engine, tmp_path, ignore_small=5, name="got"):
    """(text bytes, binary bytes, stats) of one save_clusters call."""
    clust, binary = tmp_path / (name + ".clust"), tmp_path / name
    st = engine.save_clusters(clust, binary, ignore_small)
    assert st["chunks"] == engine.get_option("save_chunks")
    text, rows = clust.read_bytes(), binary.read_bytes()
    assert st["text_bytes"] == len(text) and st["bin_bytes"] == len(rows)
    assert st["clusters_written"] == text.count(b"\n") and st["members_written"] == text.count(b"\t")
    assert len(rows) == st["clusters_written"] * 4 * engine.d
    return text, rows, st


def check_save(engine, tmp_path, ignore_small, what, want=None):
    """A save of the engine's state against the Python writers over `want` (default: result())."""
    want = engine.result() if want is None else want
    text, rows = expected_files(tmp_path, want, ignore_small)
    got = save(engine, tmp_path, ignore_small)
    assert got[0] == text, f"{what}: text differs (ignore_small={ignore_small})"
    assert got[1] == rows, f"{what}: binary differs (ignore_small={ignore_small})"
    assert got[2]["clusters"] == want[0].shape[0], what
    return got


def direct_lists(sizes, d, seed):
    """Rows with member lists of the given sizes and a permutation as ids."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ids = rng.permutation(int(off[-1])).astype(np.uint64)
    rows = rng.normal(0, 1, size=(len(sizes), d)).astype(np.float32)
    return rows, off, ids


# ------------------------------------------------------------- 1. digits ----------------------
def test_digits_reference_bytes(engine, tmp_path):
    """The fixture's lists (ids of 1..20 digits, both sides of every power of ten) loaded with
    their ids: the reference's own bytes at ignore_small = 0, their lines filtered by header at 5."""
    z = golden("save_digits.npz")
    engine.load_rows(z["rows"], z["off"], z["ids"])
    text, rows, st = save(engine, tmp_path, 0)
    assert text == z["clust"].tobytes() and rows == z["binary"].tobytes()
    assert engine.get_option("save_ids_uploaded") == 1
    assert st["clusters"] == 6 and st["clusters_written"] == 6 and st["members_written"] == 62
    lines = z["clust"].tobytes().split(b"\n")[:-1]
    keep = [int(ln.split(b"\t")[0]) > 5 for ln in lines]
    text, rows, st = save(engine, tmp_path, 5)
    assert text == b"".join(ln + b"\n" for ln, k in zip(lines, keep) if k)
    assert rows == np.frombuffer(z["binary"].tobytes(), "<f4").reshape(-1, 3)[np.array(keep)].tobytes()
    assert st["clusters_written"] == 4 and engine.get_option("save_ids_uploaded") == 1


def test_digits_load_counts_ids_not_uploaded(engine, tmp_path):
    """klsh_load_counts defines id = batch_offset + node: 40 rows whose ids cross 10^5, formatted
    from the node numbers with no id upload."""
    rng = np.random.default_rng(11)
    d, n_total, batch_offset, batch_size = 8, 100040, 99990, 40
    counts = rng.integers(1, 50, size=(d, n_total)).astype(np.uint16)
    counts[:, batch_offset + 7] = 0  # a dropped row: its node is in no list
    v_kmers = rng.uniform(0.5, 2.0, d).astype(np.float32)
    engine.load_counts(counts, v_kmers, batch_offset, batch_size)
    want = engine.result()
    assert want[0].shape[0] == 39 and int(want[2].min()) == 99990 and int(want[2].max()) == 100029
    text, _, _ = check_save(engine, tmp_path, 0, "load_counts", want)
    assert engine.get_option("save_ids_uploaded") == 0
    assert b"1\t99999\n1\t100000\n" in text and b"\t99997\n" not in text
    engine.load_rows(want[0])  # member_ids = None: id = node
    check_save(engine, tmp_path, 0, "load_rows without ids")
    assert engine.get_option("save_ids_uploaded") == 0


# ------------------------------------------------------------- 2. KAT -------------------------
@pytest.mark.parametrize("kat", ["katF", "katG", "katN"])
def test_kat_md5(engine, kat, tmp_path):
    """The mode-C pipeline through the library: the md5s of the seeded reference CLI's files."""
    with open(os.path.join(GOLDEN, "kat_md5.json")) as f:
        ref = json.load(f)[kat]
    kat_inputs.write_kat(kat, str(tmp_path))
    d = io.count_lines(str(tmp_path / "a.txt")) + io.count_lines(str(tmp_path / "b.txt"))
    kmap, v_kmers = io.read_count_log(str(tmp_path / "kmer_count.log"), d)
    counts = np.fromfile(tmp_path / "kmer_count.bin", "<u2").reshape(d, kmap)
    engine.load_counts(counts, v_kmers)
    t0, c, _ = engine.cluster(0.8, 1, 100000, 12345, 0)
    t1, c, _ = engine.cluster(0.8, 10, 1000000, 12345, c)
    assert [int(v) for v in t0] + [int(v) for v in t1] == ref["trace"]
    text, rows, _ = save(engine, tmp_path, 5, "clustering_result.txt")
    assert hashlib.md5(rows).hexdigest() == ref["md5"]["clustering_result.txt"]
    assert hashlib.md5(text).hexdigest() == ref["md5"]["clustering_result.txt.clust"]
    assert engine.get_option("save_ids_uploaded") == 0


# ------------------------------------------------------------- 3. ignore_small edges ----------
EDGE_SIZES = [1, 5, 6, 7, 10, 1025, 2049, 6, 5, 1, 2049, 7]


@pytest.mark.parametrize("ignore_small", [0, 5, 6, 2048, 2049, 2 ** 31 - 1])
def test_ignore_small_edges(engine, tmp_path, ignore_small):
    """Lists of 1, 5, 6, 7, 10 (a two-digit header), 1025 and 2049 members (one row over several
    256-entry tiles) at thresholds on both sides of them; nothing kept: two empty files."""
    rows, off, ids = direct_lists(EDGE_SIZES, 8, 3)
    engine.load_rows(rows, off, ids)
    text, binary, st = check_save(engine, tmp_path, ignore_small, "edges", (rows, off, ids))
    kept = sum(1 for s in EDGE_SIZES if s > ignore_small)
    assert st["clusters_written"] == kept
    if kept == 0:
        assert text == b"" and binary == b"" and st["chunks"] == 0
        assert (tmp_path / "got.clust").exists() and (tmp_path / "got").exists()


def test_no_rows_gives_empty_files(engine, tmp_path):
    engine.load_rows(np.zeros((0, 8), np.float32))
    text, binary, st = save(engine, tmp_path, 5)
    assert text == b"" and binary == b"" and st["chunks"] == 0 and st["clusters"] == 0


# ------------------------------------------------------------- 4. tile edges ------------------
def tile_case(kind, n):
    if kind == "six":  # list starts on multiples of 256 entries (every 768 entries)
        return direct_lists([6] * n, 8, n)
    return direct_lists([5 + (i & 1) for i in range(n)], 8, n)  # the keep scan's 2048-row tile


@pytest.mark.parametrize("kind,n", [("six", 255), ("six", 256), ("six", 257),
                                    ("alt", 2047), ("alt", 2048), ("alt", 2049)])
def test_tile_edges(engine, tmp_path, kind, n):
    rows, off, ids = tile_case(kind, n)
    engine.load_rows(rows, off, ids)
    _, _, st = check_save(engine, tmp_path, 5, f"{kind} {n}", (rows, off, ids))
    assert st["clusters_written"] == (n if kind == "six" else n // 2)


# ------------------------------------------------------------- 5. interleaved lists -----------
@pytest.mark.parametrize("weighted", [False, True])
def test_chain_lists(engine, oracle, tmp_path, weighted):
    """15 lists of 1..1025 nodes chained by one p_cluster pass, plain and with lists of permuted
    ids per loaded row."""
    (rows, off, ids), want = rx.chain_reference(oracle, len(rx.CHAIN_SIZES), weighted)
    engine.load_rows(rows, off, ids) if weighted else engine.load_rows(rows)
    engine.pcluster(rx.CHAIN_THR)
    for ignore_small in (0, 5):
        check_save(engine, tmp_path, ignore_small, f"chains weighted={weighted}", want)
    assert engine.get_option("save_ids_uploaded") == (1 if weighted else 0)


LADDERS = [(40000, 16), (30000, 13)]


def ladder_state(engine, oracle, n, d):
    (rows, off, ids), want = ladder_reference(oracle, n, d, 1000000)
    min_sim, all_iters, seed, counter = LADDER_CALL
    engine.load_rows(rows, off, ids)
    trace, c, _ = engine.cluster(min_sim, all_iters, 1000000, seed, counter)
    assert np.array_equal(trace, want[3]) and c == want[4]
    return want


@pytest.mark.parametrize("n,d", LADDERS)
def test_loop_made_lists(engine, oracle, tmp_path, n, d):
    """Six weighted iterations: thousands of lists interleaved by real merges (d = 13: the row
    gather skips the pad), against the oracle's lists."""
    want = ladder_state(engine, oracle, n, d)
    check_save(engine, tmp_path, 5, f"ladder n={n} d={d}", want)


def test_unlisted_nodes_are_never_written(engine, oracle, tmp_path):
    """result_device() filtered to the lists of more than 5 members and loaded back in keep mode:
    saved with ignore_small = 0 it is the unfiltered state's file at 5; the nodes of the lists
    left out are in no live row and appear nowhere."""
    n, d = LADDERS[0]
    want = ladder_state(engine, oracle, n, d)
    full = check_save(engine, tmp_path, 5, "ladder", want)
    rows, off, nodes, _ = engine.result_device()
    off64 = off.view(torch.int32).to(torch.int64)
    cnt = off64[1:] - off64[:-1]
    keep = cnt > 5
    assert 0 < int(keep.sum()) < keep.numel()
    new_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=cnt.device),
                         torch.cumsum(cnt[keep], 0)]).to(torch.int32)
    new_nodes = nodes.view(torch.int32)[torch.repeat_interleave(keep, cnt)].contiguous()
    engine.load_clusters(rows[keep].contiguous(), new_off, new_nodes)
    assert engine.get_option("member_nodes") > int(new_off[-1].item())
    got = check_save(engine, tmp_path, 0, "kept lists")
    assert got[0] == full[0] and got[1] == full[1]
    assert engine.get_option("save_ids_uploaded") == 1


# ------------------------------------------------------------- 6. chunks ----------------------
def chain_state(engine, oracle):
    (rows, off, ids), want = rx.chain_reference(oracle, len(rx.CHAIN_SIZES), True)
    engine.load_rows(rows, off, ids)
    engine.pcluster(rx.CHAIN_THR)
    return want


def n_chunks(text_len, kept_rows, d, chunk):
    """ceil(L / chunk) text windows; the binary file in whole rows, one per chunk at least."""
    per = max(1, chunk // (4 * d))
    return -(-text_len // chunk) + -(-kept_rows // per)


def test_chunk_sizes(engine, oracle, tmp_path):
    """The chain state at every chunk size around the text's length L, down to 32 bytes (chunk
    edges inside tokens; a 64-byte row per chunk), and with the text's positions starting just
    below 2^32 and at 2^40: the same files, in the chunks the rule gives."""
    want = chain_state(engine, oracle)
    text, rows = expected_files(tmp_path, want, 5)
    L, kept = len(text), text.count(b"\n")
    assert L > 8192 and kept >= 10
    base = save(engine, tmp_path, 5)
    assert base[0] == text and base[1] == rows and base[2]["chunks"] == 2
    for chunk in (32, 33, 257, 4096, L - 1, L, L + 1):
        with options(engine, save_chunk_bytes=chunk):
            got = save(engine, tmp_path, 5)
        assert got[0] == text and got[1] == rows, f"chunk {chunk}"
        assert got[2]["chunks"] == n_chunks(L, kept, rx.CHAIN_D, chunk), f"chunk {chunk}"
    assert engine.get_option("save_chunk_bytes") == 0
    for pos in (2 ** 32 - L // 2, 2 ** 40):
        for chunk in (0, 257):
            with options(engine, save_offset_base=pos, save_chunk_bytes=chunk):
                got = save(engine, tmp_path, 5)
            assert got[0] == text and got[1] == rows, f"offset base {pos} chunk {chunk}"
    assert engine.get_option("save_offset_base") == 0
    for name, bad in (("save_chunk_bytes", 31), ("save_chunk_bytes", -1),
                      ("save_offset_base", -1), ("save_offset_base", 2 ** 48 + 1)):
        with pytest.raises(_native.KlshError, match="KLSH_E_ARG"):
            engine.set_option(name, bad)


def test_row_larger_than_chunk(engine, tmp_path):
    """d = 100 at 32-byte chunks: every 400-byte row is a chunk of its own."""
    sizes = [6, 3, 9, 12, 7, 5, 30] * 7
    rows, off, ids = direct_lists(sizes, 100, 100)
    engine.load_rows(rows, off, ids)
    text, binary = expected_files(tmp_path, (rows, off, ids), 5)
    with options(engine, save_chunk_bytes=32):
        got = save(engine, tmp_path, 5)
    assert got[0] == text and got[1] == binary
    assert got[2]["chunks"] == n_chunks(len(text), 35, 100, 32) == -(-len(text) // 32) + 35


# ------------------------------------------------------------- 7. capped grids ----------------
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_grid_cap(engine, oracle, tmp_path, cap):
    """Every launch at 1, 2 and 3 workgroups: each takes several trips over the entries (256 a
    trip) and, where the state has the rows for it, over the keep scan's tiles."""
    rows, off, ids = tile_case("alt", 2049)
    assert rows.shape[0] > 3 * 256 and ids.size > 3 * 256 * cap
    engine.load_rows(rows, off, ids)
    with options(engine, grid_cap=cap):
        check_save(engine, tmp_path, 5, f"alt 2049, grid_cap={cap}", (rows, off, ids))

    # the ladder as loaded (40000 rows: 20 tiles of the keep scan) and after its six iterations
    # (a few hundred rows are left by then, so only its entries take several trips)
    n, d = LADDERS[0]
    (rows, off, ids), _ = ladder_reference(oracle, n, d, 1000000)
    assert -(-n // 2048) >= 3 * cap and ids.size > 3 * 256 * cap
    engine.load_rows(rows, off, ids)
    with options(engine, grid_cap=cap):
        check_save(engine, tmp_path, 3, f"ladder loaded, grid_cap={cap}", (rows, off, ids))
    want = ladder_state(engine, oracle, n, d)
    assert want[2].size > 3 * 256 * cap
    with options(engine, grid_cap=cap, save_chunk_bytes=4096):
        check_save(engine, tmp_path, 5, f"ladder, grid_cap={cap}", want)

    want = chain_state(engine, oracle)
    assert want[2].size > 3 * 256 * cap
    with options(engine, grid_cap=cap):
        check_save(engine, tmp_path, 5, f"chains, grid_cap={cap}", want)


# ------------------------------------------------------------- 8. state untouched -------------
def test_save_leaves_the_state(engine, oracle, tmp_path):
    """Three iterations, a save, three more: trace, counter and result equal the oracle's two
    calls, and the cached row state passes before and after the save, bit for bit the same."""
    rows, off, ids = row_state.ladder(12000, 16)
    w1 = oracle.cluster(rows, 0.8, 3, 1000000, 777, 3, off, ids)
    w2 = oracle.cluster(w1[0], 0.8, 3, 1000000, 777, w1[4], w1[1], w1[2])
    assert w2[3][-1] < w1[3][-1] < w1[3][0]
    engine.load_rows(rows, off, ids)
    trace, c, _ = engine.cluster(0.8, 3, 1000000, 777, 3)
    assert np.array_equal(trace, w1[3]) and c == w1[4]
    before = row_state.check(engine, w1, "before the save")
    check_save(engine, tmp_path, 5, "3 iterations", w1)
    after = row_state.check(engine, w1, "after the save")
    assert row_state.same_state(before, after)
    trace, c, _ = engine.cluster(0.8, 3, 1000000, 777, c)
    assert np.array_equal(trace, w2[3]) and c == w2[4]
    row_state.check(engine, w2, "3 more iterations")
    check_save(engine, tmp_path, 5, "6 iterations", w2)


# ------------------------------------------------------------- 9. refusals --------------------
def test_refusals(engine, oracle, tmp_path):
    """Argument errors and unwritable paths are refused before anything is touched: no file is
    created, a file that was there keeps its bytes, and the result is what it was."""
    want = chain_state(engine, oracle)
    old = tmp_path / "old"
    old.write_bytes(b"keep me")
    fresh, missing = tmp_path / "fresh", tmp_path / "no_such_dir" / "x"
    for args in [(old, fresh, -1), (None, None, 5), (missing, old, 5), (old, missing, 5),
                 (fresh, missing, 5), (missing, None, 5), (None, missing, 5)]:
        with pytest.raises(_native.KlshError, match="KLSH_E_ARG"):
            engine.save_clusters(*args)
        assert old.read_bytes() == b"keep me" and not fresh.exists() and not missing.parent.exists()
    lib = _native.load_library()
    st = _native.KlshSaveStats()
    st.struct_size -= 8
    assert lib.klsh_save_clusters(engine._ctx, os.fspath(old).encode(), None, 5,
                                  ctypes.byref(st)) == -1
    assert old.read_bytes() == b"keep me"
    with _native.Engine(0) as empty:
        with pytest.raises(_native.KlshError, match="KLSH_E_STATE"):
            empty.save_clusters(fresh, None, 5)
    assert not fresh.exists()
    row_state.assert_same_result(engine.result(), *want[:3])
    # one file alone
    text, rows = expected_files(tmp_path, want, 5)
    st = engine.save_clusters(fresh, None, 5)
    assert fresh.read_bytes() == text and st["bin_bytes"] == 0 and st["text_bytes"] == len(text)
    st = engine.save_clusters(None, old, 5)
    assert old.read_bytes() == rows and st["text_bytes"] == 0 and st["bin_bytes"] == len(rows)


# ------------------------------------------------------------- 10. sharded replica ------------
def test_sharded_rank_saves_its_replica(engine, oracle, tmp_path):
    """W = 2 in-process ranks after a three-iteration sharded call: each rank's files equal the
    single-GPU engine's."""
    n, d = LADDERS[0]
    (rows, off, ids), _ = ladder_reference(oracle, n, d, 1000000)
    engine.load_rows(rows, off, ids)
    trace1, c1, _ = engine.cluster(0.8, 3, 1000000, 777, 3)
    base = check_save(engine, tmp_path, 5, "single GPU")
    engines = [_native.Engine(0) for _ in range(2)]
    try:
        for e in engines:
            e.load_rows(rows, off, ids)
            e.set_option("shard_min_rows", 0)
        _native.comm_init_local(engines)
        errs = []

        def work(r):
            try:
                trace, c, st = engines[r].cluster(0.8, 3, 1000000, 777, 3)
                assert st["world"] == 2 and np.array_equal(trace, trace1) and c == c1
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
            got = save(e, tmp_path, 5, f"rank{r}")
            assert got[0] == base[0] and got[1] == base[1], f"rank {r}"
    finally:
        for e in engines:
            e.close()
