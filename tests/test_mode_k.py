"""Mode K: the k-mer table counted from FASTQ files on the GPU (klsh_count_khtable).

The expectation has two halves.  Per sample, the listing: a plain dictionary counter
(tests/golden/kcount_inputs.py) of what `kmc -k<K> -r -cs65535 -ci<C>` lists, in the order of a
KMC1-layout database.  Across samples, mode B on those listings: the model's listings written
as KMC1 databases, and the reference CLI's own files from them (tests/golden/mode_k.json, made by
make_golden_k.py).
CPU: the oracle over the model's databases reproduces mode_k.json; the fixtures contain what they
are named for; the model's FASTQ parser reads what the project's reader reads.
GPU: klsh_count_khtable writes the fixture's files, byte for byte what klsh_build_khtable writes
from the model's databases; the files barely react to a wrong listing order, so
the per-sample listings (klsh_kcount_listing) and the first-appearance list are compared
themselves; batches of 1, 7 and 64 reads, a table grown from 1024 slots and reads built around
the kernel's LDS window give the same output.
"""
import contextlib
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN

import klsh_oracle_b as ob  # noqa: E402

sys.path.insert(0, GOLDEN)
import kcount_inputs as kc  # noqa: E402
import kmc_inputs as ki  # noqa: E402
from make_golden_b import row_digest  # noqa: E402

CASES = list(kc.CASES)
FILES = ("kmer_set.hex", "kmer_count.bin", "kmer_count.log")


def fixtures():
    with open(os.path.join(GOLDEN, "mode_k.json")) as f:
        return json.load(f)


class Case:
    """One case written once: FASTQ files, the model's listings and databases, the oracle's
    table over them."""

    def __init__(self, d, info):
        self.dir, self.info = d, info
        self.k, self.count_min = info["k"], info["count_min"]
        self.fastq = [str(d / n) for n in info["fastq"]]
        self.dbs, self.listings = kc.write_model_dbs(str(d), info)
        self._oracle = {}

    def oracle(self, order="reference"):
        if order not in self._oracle:
            self._oracle[order] = ob.build_khtable(self.dbs, self.k, order=order)
        return self._oracle[order]

    def oracle_files(self):
        reps, counts, log = self.oracle()
        return (np.array(reps, "<u8").tobytes(), np.ascontiguousarray(counts, "<u2").tobytes(),
                log.encode())


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    cache = {}

    def get(case, W=None):
        if case not in cache:
            d = tmp_path_factory.mktemp(case)
            info = kc.write_win_case(str(d), W) if case == "win" else kc.write_case(str(d), case)
            cache[case] = Case(d, info)
        return cache[case]

    return get


# ------------------------------------------------------------------------------------ CPU ---
@pytest.mark.parametrize("case", CASES)
def test_oracle_over_model_matches_reference(cases, case):
    """The mode-B oracle over the model's databases gives the files the reference CLI wrote from
    them, and the listings are the recorded ones."""
    c, fx = cases(case), fixtures()[case]
    reps, counts, log = c.oracle()
    assert log == fx["log"] and len(reps) == fx["kmap"]
    hx, bn, _ = c.oracle_files()
    assert (hashlib.md5(hx).hexdigest(), hashlib.md5(bn).hexdigest()) == (fx["hex_md5"], fx["bin_md5"])
    assert row_digest(np.array(reps, np.uint64), counts) == fx["rows_md5"]
    assert [dict(n=len(ls), md5=kc.listing_md5(ls)) for ls in c.listings] == fx["listings"]


def test_fixtures_reach_what_they_are_for(cases):
    """From the model alone: each case contains what it is named for."""
    sat = cases("sat")
    occ = kc.count_occurrences(sat.info["seqs"][0], sat.k)
    assert 65535 in occ.values() and 65536 in occ.values() and max(occ.values()) > 65536
    assert occ["A" * sat.k] > 65536  # the poly-A read, with the poly-T read's windows
    assert sum(n == 65535 for _, n in sat.listings[0]) == 3

    filt = cases("filt")
    occs = [kc.count_occurrences(s, filt.k) for s in filt.info["seqs"]]
    listed = [dict(ls) for ls in filt.listings]
    assert any(0 < occs[0][w] < filt.count_min for w in listed[1])  # filtered in 0, listed in 1
    assert occs[2] and not listed[2]  # every k-mer of sample 2 is filtered
    assert not occs[3] and os.path.getsize(filt.fastq[3]) == 0  # an empty file
    assert fixtures()["filt"]["log"].split("\t")[3:] == ["0.000000", "0.000000"]

    k4 = cases("k4")
    occ = kc.count_occurrences(k4.info["seqs"][0], 4)
    assert occ["ACGT"] >= 2 and occ["AATT"] >= 2  # palindromes: one occurrence per window
    assert kc.count_occurrences(["ACGTACGT"], 4)["ACGT"] == 2

    # the listing's order by a 2k-bit value: at k = 16 the one sort uses all 32 bits, at k = 17 the
    # low words alone do not order the listing (the pass over the high words is needed)
    for name in ("k16", "k17"):
        for ls in cases(name).listings:
            vals = [ki.kmer_value(w) for w, _ in ls]
            lows = [v & 0xFFFFFFFF for v in vals]
            assert vals == sorted(vals) and len(vals) > 300
            if name == "k16":
                assert max(vals) >> 31 == 1
            else:
                assert max(vals) >> 32 == 3 and lows != sorted(lows)

    k21 = cases("k21")
    seqs = [s for ss in k21.info["seqs"] for s in ss]
    assert any(s.startswith("N") for s in seqs) and any(s.endswith("N") for s in seqs)
    assert any("NNNN" in s for s in seqs) and any(s != s.upper() for s in seqs)
    assert any(len(s) == 21 for s in seqs) and any(0 < len(s) < 21 for s in seqs) and "" in seqs
    windows = sum(max(0, len(s) - 20) for s in k21.info["seqs"][0])
    assert sum(kc.count_occurrences(k21.info["seqs"][0], 21).values()) < windows  # N-broken windows
    fwd = {s[p:p + 21] for s in seqs for p in range(len(s) - 20)}
    fwd = {w for w in fwd if not w.strip("ACGT")}
    assert any(ki.revcomp(w) in fwd for w in fwd if w != ki.revcomp(w))  # both strands seen
    assert any(n.endswith(".gz") for n in k21.info["fastq"])


@pytest.mark.parametrize("case", CASES)
def test_model_reads_what_the_project_reader_reads(cases, case):
    """The model's FASTQ parser and klsh_fastq_next (host only) agree on every record, gzip,
    CRLF, multi-line and empty ones included; both give the sequences that were written."""
    from kmerlsh_amd import _native

    c = cases(case)
    for path, want in zip(c.fastq, c.info["seqs"]):
        assert kc.read_sequences(path) == want
        assert [r[1].decode() for r in _native.fastq_records(path)] == want


# ------------------------------------------------------------------------------------ GPU ---
@contextlib.contextmanager
def hooks(engine, batch_reads=0, table_slots=0):
    engine.set_option("kcount_batch_reads", batch_reads)
    engine.set_option("kcount_table_slots", table_slots)
    engine.set_option("kcount_keep_listing", 1)
    engine.set_option("kmc_keep_first", 1)
    try:
        yield
    finally:
        for name in ("kcount_batch_reads", "kcount_table_slots", "kcount_keep_listing",
                     "kmc_keep_first"):
            engine.set_option(name, 0)


def count(engine, c, out, **kw):
    """(stats, the three files' bytes, per-sample listings, first-appearance list) of one call."""
    with hooks(engine, **kw):
        st = engine.count_khtable(c.fastq, c.k, c.count_min, str(out))
        listings = [engine.kcount_listing(j) for j in range(len(c.fastq))]
        first = engine.khtable_first()
    return st, tuple((out / n).read_bytes() for n in FILES), listings, first


def assert_listings(c, listings):
    for j, (vals, cnts) in enumerate(listings):
        want = c.listings[j]
        assert np.array_equal(vals, np.array([ki.kmer_value(w) for w, _ in want], np.uint64)), j
        assert np.array_equal(cnts, np.array([n for _, n in want], np.uint32)), j


def assert_stats(c, st):
    seqs = [s for ss in c.info["seqs"] for s in ss]
    assert st["reads"] == len(seqs) and st["bases"] == sum(len(s) for s in seqs)
    occs = [kc.count_occurrences(ss, c.k) for ss in c.info["seqs"]]
    assert st["positions"] == sum(sum(o.values()) for o in occs)
    assert st["distinct"] == sum(len(o) for o in occs)
    assert st["listed"] == sum(len(ls) for ls in c.listings)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_count_khtable_matches_reference(engine, cases, case, tmp_path):
    c, fx = cases(case), fixtures()[case]
    st, files, _, _ = count(engine, c, tmp_path)
    assert st["kmap_size"] == fx["kmap"]
    assert files[2].decode() == fx["log"]
    assert (hashlib.md5(files[0]).hexdigest(), hashlib.md5(files[1]).hexdigest()) == (fx["hex_md5"], fx["bin_md5"])
    assert_stats(c, st)
    b = tmp_path / "b"
    b.mkdir()
    engine.build_khtable(c.dbs, c.k, str(b))
    assert files == tuple((b / n).read_bytes() for n in FILES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_listing_matches_model(engine, cases, case, tmp_path):
    c = cases(case)
    _, _, listings, _ = count(engine, c, tmp_path)
    assert_listings(c, listings)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_first_appearance_matches_oracle(engine, cases, case, tmp_path):
    c = cases(case)
    _, _, _, first = count(engine, c, tmp_path)
    assert np.array_equal(first, np.array(c.oracle("first")[0], np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("count_min", [0, -3, 1, 4])
def test_count_min(engine, cases, count_min, tmp_path):
    """count_min below 1 is 1 (every k-mer listed); above, the listing thins as the model's."""
    c = cases("k5")
    with hooks(engine):
        st = engine.count_khtable(c.fastq, c.k, count_min, str(tmp_path))
        got = [engine.kcount_listing(j) for j in range(len(c.fastq))]
    want = [kc.listing_of(kc.count_occurrences(ss, c.k), count_min) for ss in c.info["seqs"]]
    assert st["listed"] == sum(len(w) for w in want)
    assert st["listed"] == st["distinct"] if count_min <= 1 else st["listed"] < st["distinct"]
    for (vals, cnts), w in zip(got, want):
        assert np.array_equal(vals, np.array([ki.kmer_value(x) for x, _ in w], np.uint64))
        assert np.array_equal(cnts, np.array([n for _, n in w], np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["k21", "sat"])
@pytest.mark.parametrize("batch", [1, 7, 64])
def test_batches_match_one_batch(engine, cases, case, batch, tmp_path):
    c = cases(case)
    one = tmp_path / "one"
    one.mkdir()
    st1, files1, listings1, first1 = count(engine, c, one)
    assert engine.get_option("kcount_batches") == sum(1 for ss in c.info["seqs"] if ss)
    st, files, listings, first = count(engine, c, tmp_path, batch_reads=batch)
    assert engine.get_option("kcount_batches") == st["batches"] == sum(
        -(-len(ss) // batch) for ss in c.info["seqs"])
    assert files == files1 == c.oracle_files()
    assert np.array_equal(first, first1)
    assert_listings(c, listings)
    assert_stats(c, st)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["k21", "k31"])
def test_table_growth(engine, cases, case, tmp_path):
    c = cases(case)
    big = tmp_path / "default"
    big.mkdir()
    _, files0, _, first0 = count(engine, c, big)
    assert engine.get_option("kcount_rehashes") == 0
    st, files, listings, first = count(engine, c, tmp_path, table_slots=1024, batch_reads=16)
    assert engine.get_option("kcount_rehashes") == st["rehashes"] >= 2
    assert files == files0 == c.oracle_files()
    assert np.array_equal(first, first0)
    assert_listings(c, listings)
    assert_stats(c, st)


@pytest.mark.gpu
def test_window_edges(engine, cases, tmp_path):
    """Reads one position short of the kernel's LDS window, exactly one window, one position into
    the second and into the third, clean and with an N at the window's last position, the next
    one, and the last base the first window stages."""
    W = engine.get_option("kcount_window")
    assert W >= 64
    c = cases("win", W)
    st, files, listings, first = count(engine, c, tmp_path)
    assert files == c.oracle_files()
    assert_listings(c, listings)
    assert_stats(c, st)
    assert np.array_equal(first, np.array(c.oracle("first")[0], np.uint64))


@pytest.mark.gpu
def test_errors_leave_the_context_usable(engine, cases, tmp_path):
    from kmerlsh_amd import _native

    c = cases("k21")
    with pytest.raises(_native.KlshError, match="cannot open"):
        engine.count_khtable(c.fastq[:2] + [str(tmp_path / "missing.fq")], c.k, 2, str(tmp_path))
    assert engine.get_option("kcount_batches") == 0  # failed before any device work
    assert not os.path.exists(tmp_path / "kmer_set.hex")
    for k in (0, 33):
        with pytest.raises(_native.KlshError, match=r"k must be in \[1, 32\]"):
            engine.count_khtable(c.fastq, k, 2, str(tmp_path))
    with pytest.raises(_native.KlshError):
        engine.kcount_listing(0)  # nothing kept by a failed call

    # a truncated gzip ends that file where the project's reader ends it
    gz = c.fastq[1]
    assert gz.endswith(".gz")
    cut = tmp_path / "cut.fq.gz"
    with open(gz, "rb") as f:
        data = f.read()
    cut.write_bytes(data[:len(data) * 2 // 3])
    got = [r[1].decode() for r in _native.fastq_records(str(cut))]
    assert 0 < len(got) < len(c.info["seqs"][1])
    with hooks(engine):
        st = engine.count_khtable([str(cut)], c.k, 1, str(tmp_path))
        vals, cnts = engine.kcount_listing(0)
    want = kc.listing_of(kc.count_occurrences(got, c.k), 1)
    assert st["reads"] == len(got)
    assert np.array_equal(vals, np.array([ki.kmer_value(w) for w, _ in want], np.uint64))
    assert np.array_equal(cnts, np.array([n for _, n in want], np.uint32))

    # and the context still builds b21
    info = ki.write_case(str(tmp_path), "b21")
    st = engine.build_khtable([str(tmp_path / n) for n in info["names"]], info["k"], str(tmp_path))
    with open(os.path.join(GOLDEN, "mode_b.json")) as f:
        fx = json.load(f)["b21"]
    assert st["kmap_size"] == fx["kmap"]
    assert (tmp_path / "kmer_count.log").read_text() == fx["log"]
    assert hashlib.md5((tmp_path / "kmer_set.hex").read_bytes()).hexdigest() == fx["hex_md5"]
    assert hashlib.md5((tmp_path / "kmer_count.bin").read_bytes()).hexdigest() == fx["bin_md5"]


@pytest.mark.gpu
def test_missing_second_sample_leaves_the_context_usable(engine, cases, tmp_path):
    """klsh_count_kmc whose second sample's FASTQ is missing fails on the host ("cannot open"),
    writes nothing, and the next call on the same context writes k5's files."""
    from kmerlsh_amd import _native

    c, fx = cases("k5"), fixtures()["k5"]
    bad, good = tmp_path / "bad", tmp_path / "good"
    bad.mkdir()
    good.mkdir()
    paths = [c.fastq[0], str(tmp_path / "missing.fq")] + c.fastq[2:]
    with pytest.raises(_native.KlshError, match="cannot open"):
        engine.count_kmc(paths, [str(bad / ("s%d" % j)) for j in range(len(paths))], c.k,
                         c.count_min, str(bad))
    assert not any(bad.iterdir())
    dbs = [str(good / ("s%d" % j)) for j in range(len(c.fastq))]
    st, dst = engine.count_kmc(c.fastq, dbs, c.k, c.count_min, str(good))
    assert st["kmap_size"] == fx["kmap"] and dst["databases"] == len(dbs)
    assert (good / "kmer_count.log").read_text() == fx["log"]
    assert hashlib.md5((good / "kmer_set.hex").read_bytes()).hexdigest() == fx["hex_md5"]
    assert hashlib.md5((good / "kmer_count.bin").read_bytes()).hexdigest() == fx["bin_md5"]


@pytest.mark.gpu
def test_cli_mode_k_only(cases):
    """kmerLSH -M K --only -C 3 on k31 writes the fixture's files and stops."""
    from kmerlsh_amd import _native

    c, fx = cases("k31"), fixtures()["k31"]
    assert c.count_min == 3
    subprocess.run([_native.CLI_PATH] + kc.cli_args(c.info, "K"), cwd=c.dir, check=True,
                   capture_output=True, timeout=300)
    assert (c.dir / "kmer_count.log").read_text() == fx["log"]
    assert hashlib.md5((c.dir / "kmer_set.hex").read_bytes()).hexdigest() == fx["hex_md5"]
    assert hashlib.md5((c.dir / "kmer_count.bin").read_bytes()).hexdigest() == fx["bin_md5"]
    assert not os.path.exists(c.dir / "clustering_result.txt")


@pytest.mark.gpu
@pytest.mark.parametrize("mode_flag", [["-M", "K"], []])
def test_cli_mode_k_through_extraction(mode_flag, tmp_path):
    """-M K, and no -M at all (the reference's default), run from FASTQ files through clustering
    and extraction with the outputs of -M B on the model's databases under the same seed."""
    from kmerlsh_amd import _native

    outs = {}
    for run, flags in (("k", mode_flag), ("b", ["-M", "B"])):
        d = tmp_path / run
        d.mkdir()
        info = kc.write_case(str(d), "k21")
        kc.write_model_dbs(str(d), info)
        args = ["-a", "a.txt", "-b", "b.txt", "-o", "A", "-p", "B", "-K", "21", "-C", "2", "-I", "3",
                "-S", "5", "-P", "0.5", "-V", "0.1", "--seed", "7"] + flags
        subprocess.run([_native.CLI_PATH] + args, cwd=d, check=True, capture_output=True, timeout=300)
        names = sorted(n for n in os.listdir(d) if n.startswith(("kmer_", "clustering_result", "A_", "B_")))
        outs[run] = {n: (d / n).read_bytes() for n in names}
    assert set(outs["k"]) == set(outs["b"])
    assert {"kmer_set.hex", "clustering_result.txt", "clustering_result.txt.clust", "A_s0.fq",
            "B_s5.fq"} <= set(outs["k"])
    assert outs["k"] == outs["b"]
    assert len(outs["k"]["clustering_result.txt"]) > 0
