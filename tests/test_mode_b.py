"""Mode B: the k-mer table built from KMC databases.

CPU: the oracle (oracle/klsh_oracle_b.py) reproduces the reference CLI's own outputs byte for byte
(tests/golden/mode_b.json: kmer_count.log verbatim and the md5s of kmer_set.hex / kmer_count.bin,
rows in the reference's libcuckoo table order), and the product's host replay of that table
(klsh_cuckoo_order, no GPU) gives the oracle's order, up to a table loaded to 95.6 % ("bl_fill").
GPU: klsh_build_khtable writes the reference's three files byte for byte, over every record
layout the listing accepts (kmc_inputs.EDGE_CASES).  The files barely react to a wrong
first-appearance order (on b21, swapping two neighbours of that list changes none of the 7687
rows), so the list itself (klsh_khtable_first) is compared with the oracle's; the many-chunk
stream and the ordinals past 2^32, which no database of test size reaches by itself, are reached
through the test options "kmc_chunk_records" and "kmc_ordinal_base", and every such test asserts
from "kmc_decode_launches" / "kmc_high_sort" that it did reach them.
"""
import contextlib
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN

import klsh_oracle_b as ob  # noqa: E402

sys.path.insert(0, GOLDEN)
import kmc_inputs as ki  # noqa: E402
from make_golden_b import row_digest  # noqa: E402

CASES = sorted(ki.CASES)
EDGE = sorted(ki.EDGE_CASES)
ALL_CASES = CASES + ["bl_fill"] + EDGE


def fixtures():
    with open(os.path.join(GOLDEN, "mode_b.json")) as f:
        return json.load(f)


def write(case, path):
    return (ki.write_big_case if case in ki.BIG_CASES else ki.write_edge_case
            if case in ki.EDGE_CASES else ki.write_case)(str(path), case)


def rows_md5(reps, counts):
    """md5s of kmer_set.hex and kmer_count.bin as the reference writes them from these rows."""
    hx = hashlib.md5(np.ascontiguousarray(reps, "<u8").tobytes()).hexdigest()
    bn = hashlib.md5(np.ascontiguousarray(counts, "<u2").tobytes()).hexdigest()
    return hx, bn


@pytest.mark.parametrize("case", ALL_CASES)
def test_oracle_mode_b_matches_reference(case, tmp_path):
    """KMC1 and KMC2 (3 signature bins) layouts, min_count filtering (the all-A k-mer the
    reference then adds), 65535 saturation, databases listing both strands, and a 501K-k-mer
    table at 95.6 % load: the oracle's rows are the reference's files byte for byte."""
    info = write(case, tmp_path)
    fx = fixtures()[case]
    reps, counts, log = ob.build_khtable([str(tmp_path / n) for n in info["names"]], info["k"])
    reps = np.array(reps, np.uint64)
    assert log == fx["log"]
    assert len(reps) == fx["kmap"]
    assert rows_md5(reps, counts) == (fx["hex_md5"], fx["bin_md5"])
    assert row_digest(reps, counts) == fx["rows_md5"]
    assert int((counts == 65535).sum()) == fx["saturated"]
    assert (0 in reps) == fx["has_zero_kmer"]


@pytest.mark.parametrize("case", ALL_CASES)
def test_host_cuckoo_order_matches_oracle(case, tmp_path):
    """The product's host replay of the reference's libcuckoo inserts (klsh_cuckoo_order, no GPU)
    orders the first-appearance rows exactly as the oracle does."""
    from kmerlsh_amd import _native

    info = write(case, tmp_path)
    first, _, _ = ob.build_khtable([str(tmp_path / n) for n in info["names"]], info["k"],
                                   order="first")
    idx, hp = ob.cuckoo_order(first, info["k"])
    mine, mhp = _native.cuckoo_order(np.array(first, np.uint64), info["k"])
    assert mhp == hp == 16
    assert np.array_equal(mine, np.array(idx, np.uint32))


def test_cuckoo_order_grows_like_a_sequential_table():
    """Past 2^16 x 8 slots the table doubles; the reference re-inserts from several threads (its
    order is then not reproducible run to run), the product as those threads would one after
    another — the same as the oracle's sequential restatement."""
    from kmerlsh_amd import _native

    rng = np.random.default_rng(5)
    reps = np.unique(rng.integers(0, 1 << 62, 530_000, dtype=np.uint64))
    rng.shuffle(reps)
    idx, hp = ob.cuckoo_order(list(reps), 31)
    mine, mhp = _native.cuckoo_order(reps, 31)
    assert hp == mhp == 17
    assert np.array_equal(mine, np.array(idx, np.uint32))


def test_edge_fixtures_reach_what_they_are_for():
    """From the reference's recorded output alone: the edge databases filter, saturate and add the
    all-A k-mer where they are meant to (make_golden_b.check_edge_conditions)."""
    fx = fixtures()
    assert fx["e_allfilt"]["kmap"] == 1 and fx["e_allfilt"]["log"] == "1\t0.000000\t0.000000"
    assert fx["e_empty"]["log"].split("\t")[1] == "0.000000"
    for case in ("e_k13win", "e_k12win2"):
        assert fx[case]["has_zero_kmer"], case
    for case in ("e_k5p1", "e_k9p9", "e_k4p4"):
        assert fx[case]["saturated"] > 0, case
    assert fx["e_k1p1"]["kmap"] == 2


def assert_fixture(case, st, out):
    """klsh_build_khtable's three files in `out` are the reference's, byte for byte."""
    fx = fixtures()[case]
    assert st["kmap_size"] == fx["kmap"]
    with open(os.path.join(out, "kmer_count.log")) as f:
        assert f.read() == fx["log"]
    for name, key in (("kmer_set.hex", "hex_md5"), ("kmer_count.bin", "bin_md5")):
        with open(os.path.join(out, name), "rb") as f:
            assert hashlib.md5(f.read()).hexdigest() == fx[key], name


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL_CASES)
def test_build_khtable_matches_reference(engine, case, tmp_path):
    info = write(case, tmp_path)
    st = engine.build_khtable([str(tmp_path / n) for n in info["names"]], info["k"], str(tmp_path))
    assert_fixture(case, st, tmp_path)


# ------------------------------------------------------------ the paths no small database takes
@pytest.fixture(scope="module")
def dbs(tmp_path_factory):
    """case -> (directory, info, per-sample record totals): each database is written once."""
    from kmerlsh_amd import _native

    cache = {}

    def get(case):
        if case not in cache:
            d = tmp_path_factory.mktemp(case)
            info = write(case, d)
            totals = [_native.kmc_info(str(d / n))[1] for n in info["names"]]
            cache[case] = (d, info, totals)
        return cache[case]

    return get


_oracle_first = {}


def oracle_first(dbs, case):
    """(the oracle's first-appearance list, the records it lists), once per case."""
    if case not in _oracle_first:
        d, info, _ = dbs(case)
        names = [str(d / n) for n in info["names"]]
        first, _, _ = ob.build_khtable(names, info["k"], order="first")
        listed = sum(len(ob.read_kmc(n)[1]) for n in names)
        _oracle_first[case] = (np.array(first, np.uint64), listed)
    return _oracle_first[case]


@contextlib.contextmanager
def kmc_hooks(engine, chunk=0, base=0):
    engine.set_option("kmc_chunk_records", chunk)
    engine.set_option("kmc_ordinal_base", base)
    engine.set_option("kmc_keep_first", 1)
    try:
        yield
    finally:
        for name in ("kmc_chunk_records", "kmc_ordinal_base", "kmc_keep_first"):
            engine.set_option(name, 0)


def build(engine, dbs, case, out, chunk=0, base=0, directory=None):
    """(stats, first-appearance list, pass 1's decode launches, whether the high words were
    sorted) of one klsh_build_khtable call under the test options."""
    d, info, _ = dbs(case)
    d = directory or d
    with kmc_hooks(engine, chunk, base):
        st = engine.build_khtable([str(d / n) for n in info["names"]], info["k"], str(out))
        return (st, engine.khtable_first(), engine.get_option("kmc_decode_launches"),
                engine.get_option("kmc_high_sort"))


def check_build(engine, dbs, case, out, chunk=0, base=0, first=True):
    """One build under the test options: the reference's files, the oracle's first-appearance
    list and record count, one decode launch per chunk, the high-word sort exactly when an
    ordinal needs it."""
    _, info, totals = dbs(case)
    st, mine, launches, high = build(engine, dbs, case, out, chunk, base)
    assert_fixture(case, st, out)
    assert st["records"] == 2 * sum(totals)  # records streamed: both passes read every file
    if first:
        want, listed = oracle_first(dbs, case)
        assert st["records_listed"] == listed
        assert np.array_equal(mine, want)
    per = chunk or (64 << 20)  # the default chunk holds far more records than any test database
    assert launches == sum(-(-t // per) for t in totals)
    assert high == int(base + sum(totals) + len(totals) >= 1 << 32)
    return st, mine, launches


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES + EDGE)
def test_first_appearance_list_matches_oracle(engine, dbs, case, tmp_path):
    """The list the libcuckoo replay is fed — distinct canonical k-mers by first (sample, record)
    ordinal, the all-A k-mer of a filtered sample after its records — equals the oracle's on every
    layout: one chunk per sample, no high words."""
    _, _, totals = dbs(case)
    _, _, launches = check_build(engine, dbs, case, tmp_path)
    assert launches == sum(t > 0 for t in totals)


def chunk_cases():
    out = [("e_k4p0", 1)] + [("b21", c) for c in (64, 257, 1000, "total-1", "total", "total+1")]
    return out + [("b31", 257), ("e_k13win", 257), ("e_k12win2", 257)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,chunk", chunk_cases())
def test_chunked_stream_matches_one_chunk(engine, dbs, case, chunk, tmp_path):
    """The .kmc_suf streams read `chunk` records at a time (a production database's 64 MB chunks,
    at test size): the LUT search on absolute record indices (KMC2: across bins), ordinals that
    carry the chunk's first record, the count of listed records summed over chunks and the
    all-A k-mer's ordinal after them give the same files, list and counts as one chunk."""
    _, _, totals = dbs(case)
    if isinstance(chunk, str):  # around sample 0's record count
        chunk = totals[0] + {"total-1": -1, "total": 0, "total+1": 1}[chunk]
    one = tmp_path / "one"
    one.mkdir()
    st1, first1, _ = check_build(engine, dbs, case, one)
    st, first, launches = check_build(engine, dbs, case, tmp_path, chunk=chunk)
    assert st["records_listed"] == st1["records_listed"]
    assert np.array_equal(first, first1)
    for name in ("kmer_set.hex", "kmer_count.bin", "kmer_count.log"):
        assert (tmp_path / name).read_bytes() == (one / name).read_bytes(), name
    assert launches > sum(t > 0 for t in totals)  # more than one chunk somewhere: not the old path


def base_cases():
    return [("2^32-1000", 0), ("2^32-total0-1", 0), ("2^32", 0), ("2^33+2^32-500", 0),
            ("2^32-1000", 257)]


@pytest.mark.gpu
@pytest.mark.parametrize("base,chunk", base_cases())
def test_ordinals_past_2_32(engine, dbs, base, chunk, tmp_path):
    """b21 with its ordinals started near 2^32 (a production run of more than 4.29 G records):
    the boundary inside sample 0, sample 1 starting exactly at 2^32, every high word equal, two
    high bits, and the boundary inside a chunked sample.  The high-word sort runs (asserted) and
    files and list are those of base 0."""
    _, _, totals = dbs("b21")
    base = {"2^32-1000": (1 << 32) - 1000, "2^32-total0-1": (1 << 32) - (totals[0] + 1),
            "2^32": 1 << 32, "2^33+2^32-500": (1 << 33) + (1 << 32) - 500}[base]
    assert totals[0] > 1000  # the boundary does fall inside sample 0
    zero = tmp_path / "zero"
    zero.mkdir()
    _, first0, _ = check_build(engine, dbs, "b21", zero)
    assert engine.get_option("kmc_high_sort") == 0
    _, first, _ = check_build(engine, dbs, "b21", tmp_path, chunk=chunk, base=base)
    assert engine.get_option("kmc_high_sort") == 1
    assert np.array_equal(first, first0)
    for name in ("kmer_set.hex", "kmer_count.bin", "kmer_count.log"):
        assert (tmp_path / name).read_bytes() == (zero / name).read_bytes(), name


@pytest.mark.gpu
def test_ordinals_past_2_32_loaded_table(engine, dbs, tmp_path):
    """bl_fill (a libcuckoo table at 95.6 % load: its bytes follow the insertion order closely)
    with the 2^32 boundary 100000 records into sample 0, against the reference's files."""
    check_build(engine, dbs, "bl_fill", tmp_path, base=(1 << 32) - 100000, first=False)
    assert engine.get_option("kmc_high_sort") == 1


@pytest.mark.gpu
def test_builds_share_one_context(engine, oracle, dbs, tmp_path):
    """Two rows, thousands, one: three builds in a row on one context each match their fixture,
    and the Cluster() path afterwards computes what it did before (nothing of a build stays in
    the context)."""
    for case in ("e_k1p1", "b32", "e_allfilt"):
        out = tmp_path / case
        out.mkdir()
        check_build(engine, dbs, case, out)
    rng = np.random.default_rng(17)
    centres = rng.random((8, 16), dtype=np.float32) * 100
    rows = (np.repeat(centres, 8, axis=0) + rng.random((64, 16), dtype=np.float32)).astype(np.float32)
    want = oracle.pcluster(rows, 0.9)
    assert want[0].shape[0] < 64  # it does merge
    engine.load_rows(rows)
    engine.pcluster(0.9)
    g_rows, g_off, g_ids = engine.result()
    assert np.array_equal(g_off, want[1]) and np.array_equal(g_ids, want[2])
    assert np.array_equal(g_rows.view(np.uint32), np.ascontiguousarray(want[0], np.float32).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("cut", ["one record", "mid record"])
def test_short_suffix_file_is_an_error_and_leaves_the_context_usable(engine, dbs, cut, tmp_path):
    """Sample 1's .kmc_suf ends one record early / in the middle of its last record; with 257-record
    chunks the call has processed sample 0 and most of sample 1 on the device when it finds out.
    It returns the "short file" error, and the next build on the same context is right."""
    from kmerlsh_amd import _native

    d, info, totals = dbs("b21")
    bad = tmp_path / "bad"
    shutil.copytree(d, bad)
    rec = (info["k"] - info["p"]) // 4 + info["counter_size"]
    keep = 4 + (totals[1] - 1) * rec + (0 if cut == "one record" else rec // 2)
    with open(bad / (info["names"][1] + ".kmc_suf"), "r+b") as f:
        f.truncate(keep)
    with pytest.raises(_native.KlshError, match="short file"):
        build(engine, dbs, "b21", tmp_path, chunk=257, directory=bad)
    assert engine.get_option("kmc_decode_launches") > -(-totals[0] // 257)  # sample 1 was under way
    check_build(engine, dbs, "b21", tmp_path)


@pytest.mark.gpu
def test_wrong_k_fails_before_device_work(engine, dbs, tmp_path):
    from kmerlsh_amd import _native

    d, info, _ = dbs("b21")
    with pytest.raises(_native.KlshError, match="differs from -K"):
        engine.build_khtable([str(d / n) for n in info["names"]], info["k"] + 1, str(tmp_path))
    assert engine.get_option("kmc_decode_launches") == 0
    assert not os.path.exists(tmp_path / "kmer_set.hex")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["e_k32p0", "e_k13win"])
def test_cli_mode_b_edge_layouts(case, tmp_path):
    """kmerLSH -M B --only writes the reference's bytes on k = 32 / p = 0 and on a count window."""
    from kmerlsh_amd import _native

    write(case, tmp_path)
    fx = fixtures()[case]
    args = [a for a in ki.cli_args(case) if a not in ("-T", "1")]
    subprocess.run([_native.CLI_PATH] + args, cwd=tmp_path, check=True, capture_output=True,
                   timeout=300)
    assert_fixture(case, {"kmap_size": fx["kmap"]}, tmp_path)


@pytest.mark.gpu
def test_cli_mode_b_then_cluster(tmp_path):
    """kmerLSH -M B --only, then -M C --only on its output (the B -> C hand-off)."""
    from kmerlsh_amd import _native

    ki.write_case(str(tmp_path), "b21")
    fx = fixtures()["b21"]
    args = [a for a in ki.cli_args("b21") if a not in ("-T", "1")]
    subprocess.run([_native.CLI_PATH] + args, cwd=tmp_path, check=True, capture_output=True,
                   timeout=300)
    with open(tmp_path / "kmer_count.log") as f:
        assert f.read() == fx["log"]
    subprocess.run([_native.CLI_PATH, "-a", "a.txt", "-b", "b.txt", "-I", "5", "-M", "C", "--only"],
                   cwd=tmp_path, check=True, capture_output=True, timeout=300)
    assert os.path.getsize(tmp_path / "clustering_result.txt") > 0
