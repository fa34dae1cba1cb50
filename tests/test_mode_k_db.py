"""Mode K's databases: each sample's listing written from the GPU as a KMC1-layout database
(klsh_count_kmc, Engine.count_kmc, kmerLSH --kmc-db / --kmc-db-only).

The expectation is the model writer of the fixtures (tests/golden/kmc_inputs.write_db over the
dictionary counter's listings, kcount_inputs.write_model_dbs): the files the reference CLI read
to make tests/golden/mode_k.json.  The product's .kmc_pre / .kmc_suf must equal them byte for
byte: at the fixtures' prefix lengths, at the prefix length the size rule picks, at the edges of
the prefix range, and whatever the chunk size.  Then the hand-off the databases exist for: mode
B over the written databases gives the table mode K gives.
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

sys.path.insert(0, GOLDEN)
import kcount_inputs as kc  # noqa: E402
import kmc_inputs as ki  # noqa: E402

CASES = list(kc.CASES)
FILES = ("kmer_set.hex", "kmer_count.bin", "kmer_count.log")
EXTS = (".kmc_pre", ".kmc_suf")


def fixtures():
    with open(os.path.join(GOLDEN, "mode_k.json")) as f:
        return json.load(f)


def same_file(a, b, block=1 << 24):
    """Byte equality of two files without holding either (a 4^13-entry LUT is 512 MB)."""
    if os.path.getsize(a) != os.path.getsize(b):
        return False
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x, y = fa.read(block), fb.read(block)
            if x != y:
                return False
            if not x:
                return True


class Case:
    """One case written once: the FASTQ files and the model's listings; the model's databases
    per (sample, prefix length), written when first asked for."""

    def __init__(self, d, name):
        self.dir, self.name = d, name
        self.info = kc.write_case(str(d), name)
        self.k, self.count_min = self.info["k"], self.info["count_min"]
        self.fastq = [str(d / n) for n in self.info["fastq"]]
        self.listings = [kc.count_listing(f, self.k, self.count_min) for f in self.fastq]
        self.sizes = [len(ls) for ls in self.listings]
        self._model = {}

    def model(self, j, p):
        """Path (no extension) of sample j's model database at prefix length p."""
        if (j, p) not in self._model:
            d = self.dir / ("model_p%d" % p)
            d.mkdir(exist_ok=True)
            path = str(d / ("db%d" % j))
            ki.write_db(path, self.k, self.listings[j], 0, p, 2, max(self.count_min, 1), 65535)
            self._model[(j, p)] = path
        return self._model[(j, p)]

    def names(self, d, samples=None):
        return [str(d / ("db%d" % j)) for j in (range(len(self.fastq)) if samples is None else samples)]

    def assert_dbs(self, d, prefix, samples=None):
        """The databases under d equal the model's; prefix: one p or one per sample."""
        for j in range(len(self.fastq)) if samples is None else samples:
            p = prefix[j] if isinstance(prefix, (list, tuple)) else prefix
            for ext in EXTS:
                assert same_file(str(d / ("db%d" % j)) + ext, self.model(j, p) + ext), (j, p, ext)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = Case(tmp_path_factory.mktemp(case), case)
        return cache[case]

    return get


@contextlib.contextmanager
def db_hooks(engine, prefix=-1, chunk=0, keep_first=0):
    engine.set_option("kcount_db_prefix", prefix)
    engine.set_option("kcount_db_chunk_records", chunk)
    engine.set_option("kmc_keep_first", keep_first)
    try:
        yield
    finally:
        engine.set_option("kcount_db_prefix", -1)
        engine.set_option("kcount_db_chunk_records", 0)
        engine.set_option("kmc_keep_first", 0)


def no_db_files(d):
    return not [n for n in os.listdir(d) if n.endswith(EXTS)]


# ------------------------------------------------------------------------------------ CPU ---
def test_prefix_length_is_the_size_rule():
    """kmc_prefix_length against a brute force of the rule written out here: the legal p with the
    fewest bytes in both files, the smaller p on a tie; n = 0 gives the smallest legal p."""
    from kmerlsh_amd.io import kmc_prefix_length

    for k in range(1, 33):
        legal = [p for p in range(0, min(k, 15) + 1) if (k - p) % 4 == 0]
        assert legal
        for n in (0, 1, 10 ** 3, 10 ** 6, 10 ** 8, 2 ** 31):
            best, best_bytes = None, None
            for p in legal:  # ascending: a tie keeps the smaller p
                size = 8 * 4 ** p + n * ((k - p) // 4 + 2)
                if best is None or size < best_bytes:
                    best, best_bytes = p, size
            got = kmc_prefix_length(k, n)
            assert got == best, (k, n)
            assert got <= min(k, 15) and (k - got) % 4 == 0
        assert kmc_prefix_length(k, 0) == legal[0] == k % 4
    # the rule does move: a large listing pays for a longer table
    assert kmc_prefix_length(31, 10 ** 3) == 3 and kmc_prefix_length(31, 10 ** 8) == 11


def test_library_exports_count_kmc():
    import ctypes

    from kmerlsh_amd import _native

    lib = _native.load_library()
    assert hasattr(lib, "klsh_count_kmc") and "klsh_count_kmc" in _native.EXPORTED
    assert lib.klsh_abi_version() == 3 == _native.ABI_VERSION
    # five uint64, two uint32, two doubles (include/klsh.h klsh_kmcdb_stats)
    assert ctypes.sizeof(_native.KlshKmcdbStats) == 64
    assert callable(_native.Engine.count_kmc)


# ------------------------------------------------------------------------------------ GPU ---
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_databases_equal_the_model_at_the_fixture_prefix(engine, cases, case, tmp_path):
    """Byte for byte the files write_model_dbs writes, which the reference CLI consumed for
    mode_k.json (filt: an empty listing and an empty file among them)."""
    c = cases(case)
    p = kc.PREFIX[c.k]
    with db_hooks(engine, prefix=p):
        st, dst = engine.count_kmc(c.fastq, c.names(tmp_path), c.k, c.count_min, str(tmp_path))
        assert engine.get_option("kcount_db_prefix_used") == p
    m = tmp_path / "m"
    m.mkdir()
    for n in c.info["fastq"]:
        os.symlink(c.dir / n, m / n)
    kc.write_model_dbs(str(m), c.info)
    for j in range(len(c.fastq)):
        for ext in EXTS:
            assert same_file(str(tmp_path / ("db%d" % j)) + ext, str(m / ("db%d" % j)) + ext)
    assert dst["databases"] == len(c.fastq) and dst["records"] == sum(c.sizes) == st["listed"]
    assert dst["bytes"] == sum(os.path.getsize(n + e) for n in c.names(tmp_path) for e in EXTS)
    assert dst["prefix_len_min"] == dst["prefix_len_max"] == p
    assert st["kmap_size"] == fixtures()[case]["kmap"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_automatic_prefix(engine, cases, case, tmp_path):
    from kmerlsh_amd.io import kmc_prefix_length

    c = cases(case)
    ps = [kmc_prefix_length(c.k, n) for n in c.sizes]
    with db_hooks(engine):
        _, dst = engine.count_kmc(c.fastq, c.names(tmp_path), c.k, c.count_min, None)
        assert engine.get_option("kcount_db_prefix_used") == ps[-1]
    c.assert_dbs(tmp_path, ps)
    assert (dst["prefix_len_min"], dst["prefix_len_max"]) == (min(ps), max(ps))


# k31 at p = 15 would be a 2^30-entry LUT (8 GB per file): p = 11 and p = 7 stand in for it.  From
# 4^12 entries on (128 MB; k21 at p = 13 is 512 MB) only sample 0 is written, so that the test
# stays within seconds: the edge is the prefix length, not the sample.
EDGES = [("k4", 0), ("k4", 4), ("k5", 5), ("k1", 1), ("k32", 0), ("k32", 12), ("k21", 1),
         ("k21", 13), ("k31", 11), ("k31", 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,p", EDGES)
def test_prefix_edges(engine, cases, case, p, tmp_path):
    c = cases(case)
    samples = [0] if p >= 12 else list(range(len(c.fastq)))
    try:
        with db_hooks(engine, prefix=p):
            _, dst = engine.count_kmc([c.fastq[j] for j in samples], c.names(tmp_path, samples), c.k,
                                      c.count_min, None)
        c.assert_dbs(tmp_path, p, samples)
        assert dst["prefix_len_min"] == dst["prefix_len_max"] == p
        rec = (c.k - p) // 4 + 2
        assert dst["bytes"] == sum(8 * 4 ** p + 60 + rec * c.sizes[j] for j in samples)
    finally:
        if p >= 12:  # the large tables do not stay behind
            for path in c.names(tmp_path, samples) + [c.model(j, p) for j in samples]:
                for ext in EXTS:
                    if os.path.exists(path + ext):
                        os.remove(path + ext)
            for j in samples:
                del c._model[(j, p)]


@pytest.mark.gpu
def test_illegal_prefix_is_refused(engine, cases, tmp_path):
    from kmerlsh_amd import _native

    c = cases("k21")
    with db_hooks(engine, prefix=10):  # (21 - 10) % 4 != 0
        with pytest.raises(_native.KlshError, match="KLSH_E_ARG.*kcount_db_prefix"):
            engine.count_kmc(c.fastq, c.names(tmp_path), c.k, c.count_min, None)
        assert engine.get_option("kcount_batches") == 0  # refused before any device work
    assert no_db_files(tmp_path)
    with pytest.raises(_native.KlshError):
        engine.set_option("kcount_db_prefix", 16)
    with db_hooks(engine, prefix=9):
        engine.count_kmc(c.fastq, c.names(tmp_path), c.k, c.count_min, None)
    c.assert_dbs(tmp_path, 9)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["k21", "sat"])
@pytest.mark.parametrize("chunk", [1, 7, 257])
def test_chunks_match_one_chunk(engine, cases, case, chunk, tmp_path):
    c = cases(case)
    p = kc.PREFIX[c.k]
    one = tmp_path / "one"
    one.mkdir()
    with db_hooks(engine, prefix=p):
        _, dst1 = engine.count_kmc(c.fastq, c.names(one), c.k, c.count_min, None)
        assert engine.get_option("kcount_db_chunks") == dst1["chunks"] == sum(n > 0 for n in c.sizes)
    with db_hooks(engine, prefix=p, chunk=chunk):
        _, dst = engine.count_kmc(c.fastq, c.names(tmp_path), c.k, c.count_min, None)
        chunks = engine.get_option("kcount_db_chunks")
    want = sum(-(-n // chunk) for n in c.sizes)
    # the many-chunk path, with a chunk that starts past the first one; sat's listings (167 and
    # 172 records) fit one chunk of 257: there the hook must change nothing
    if (case, chunk) == ("sat", 257):
        assert want == dst1["chunks"]
    else:
        assert max(c.sizes) > 2 * chunk and want > 2 * dst1["chunks"]
    assert chunks == dst["chunks"] == want
    for j in range(len(c.fastq)):
        for ext in EXTS:
            assert same_file(str(tmp_path / ("db%d" % j)) + ext, str(one / ("db%d" % j)) + ext)
    c.assert_dbs(tmp_path, p)
    assert dst["bytes"] == dst1["bytes"] and dst["records"] == dst1["records"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_round_trip_through_mode_b(engine, cases, case, tmp_path):
    """Mode K's table, and mode B's over the databases mode K wrote: the same three files, the
    fixture's digests, the same first-appearance list."""
    c, fx = cases(case), fixtures()[case]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    names = c.names(tmp_path)
    with db_hooks(engine, keep_first=1):
        st, _ = engine.count_kmc(c.fastq, names, c.k, c.count_min, str(a))
        first_k = engine.khtable_first()
        stb = engine.build_khtable(names, c.k, str(b))
        first_b = engine.khtable_first()
    files = tuple((a / n).read_bytes() for n in FILES)
    assert files == tuple((b / n).read_bytes() for n in FILES)
    assert st["kmap_size"] == stb["kmap_size"] == fx["kmap"]
    assert files[2].decode() == fx["log"]
    assert (hashlib.md5(files[0]).hexdigest(), hashlib.md5(files[1]).hexdigest()) == (fx["hex_md5"], fx["bin_md5"])
    assert np.array_equal(first_k, first_b) and len(first_k) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["k21", "filt"])
def test_databases_only(engine, cases, case, tmp_path, monkeypatch):
    c = cases(case)
    p = kc.PREFIX[c.k]
    cwd = tmp_path / "cwd"
    cwd.mkdir()
    monkeypatch.chdir(cwd)  # where a table would go if one were written after all
    with db_hooks(engine, prefix=p):
        st, dst = engine.count_kmc(c.fastq, c.names(tmp_path), c.k, c.count_min, None)
    c.assert_dbs(tmp_path, p)
    assert os.listdir(cwd) == []
    assert sorted(os.listdir(tmp_path)) == sorted(
        ["cwd"] + ["db%d%s" % (j, e) for j in range(len(c.fastq)) for e in EXTS])
    assert st["kmap_size"] == 0 and st["order_ms"] == 0.0
    assert st["listed"] == dst["records"] == sum(c.sizes) and dst["databases"] == len(c.fastq)
    assert st["reads"] == sum(len(s) for s in c.info["seqs"])


@pytest.mark.gpu
def test_no_database_names_is_count_khtable(engine, cases, tmp_path):
    c = cases("k21")
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    st0 = engine.count_khtable(c.fastq, c.k, c.count_min, str(a))
    st, dst = engine.count_kmc(c.fastq, None, c.k, c.count_min, str(b))
    assert sorted(os.listdir(b)) == sorted(FILES)
    assert tuple((a / n).read_bytes() for n in FILES) == tuple((b / n).read_bytes() for n in FILES)
    timed = [n for n in st if n.endswith("_ms")]
    assert {n: v for n, v in st.items() if n not in timed} == {n: v for n, v in st0.items() if n not in timed}
    assert all(v == 0 for v in dst.values())
    assert engine.get_option("kcount_db_chunks") == 0
    assert engine.get_option("kcount_db_prefix_used") == -1


@pytest.mark.gpu
def test_saturated_counters(engine, cases, tmp_path):
    """sat: the poly-A k-mer (65560 occurrences) and the two (AC)-repeat k-mers (65536 and 65535)
    carry the counter bytes FF FF; nothing else does."""
    c = cases("sat")
    with db_hooks(engine, prefix=1):  # 5 suffix bytes: the low 40 bits of the value
        engine.count_kmc(c.fastq[:1], c.names(tmp_path, [0]), c.k, c.count_min, None)
    data = (tmp_path / "db0.kmc_suf").read_bytes()
    assert data[:4] == data[-4:] == b"KMCS"
    rec = (c.k - 1) // 4 + 2
    assert len(data) == 8 + rec * c.sizes[0]
    recs = [data[4 + i * rec: 4 + (i + 1) * rec] for i in range(c.sizes[0])]
    words = [w for w, _ in c.listings[0]]
    ac = ("AC" * c.k)[:c.k]
    ca = ("CA" * c.k)[:c.k]
    sat = sorted({"A" * c.k, min(ac, ki.revcomp(ac)), min(ca, ki.revcomp(ca))})
    assert len(sat) == 3
    for w in sat:
        r = recs[words.index(w)]
        assert r[:5] == (ki.kmer_value(w) & ((1 << 40) - 1)).to_bytes(5, "big")
        assert r[5:] == b"\xff\xff"
    assert sum(r[5:] == b"\xff\xff" for r in recs) == 3
    for r, (w, n) in zip(recs, c.listings[0]):
        assert int.from_bytes(r[5:], "little") == n


@pytest.mark.gpu
def test_errors_leave_no_partial_database_and_a_usable_context(engine, cases, tmp_path):
    from kmerlsh_amd import _native

    c = cases("k21")
    p = kc.PREFIX[c.k]
    good = c.names(tmp_path)

    def still_counts():
        d = tmp_path / ("ok%d" % len(os.listdir(tmp_path)))
        d.mkdir()
        with db_hooks(engine, prefix=p):
            st, _ = engine.count_kmc(c.fastq, c.names(d), c.k, c.count_min, str(d))
        c.assert_dbs(d, p)
        assert st["kmap_size"] == fixtures()["k21"]["kmap"]
        assert hashlib.md5((d / "kmer_set.hex").read_bytes()).hexdigest() == fixtures()["k21"]["hex_md5"]

    bad = [
        (good[:3] + [str(tmp_path / "missing" / "db3")] + good[4:], str(tmp_path), "cannot write"),
        (good[:2] + [None] + good[3:], str(tmp_path), "null database name"),
        (good[:4] + [good[1]] + good[5:], str(tmp_path), "named twice"),
        (None, None, "neither"),
    ]
    for names, out_dir, what in bad:
        with pytest.raises(_native.KlshError, match="KLSH_E_ARG.*" + what):
            engine.count_kmc(c.fastq, names, c.k, c.count_min, out_dir)
        assert no_db_files(tmp_path), what  # sample 0's files included
        assert not os.path.exists(tmp_path / "kmer_set.hex")
        still_counts()
    # a database that exists is not removed by a call that fails before it is rewritten
    with db_hooks(engine, prefix=p):
        engine.count_kmc(c.fastq, good, c.k, c.count_min, None)
    with pytest.raises(_native.KlshError, match="named twice"):
        engine.count_kmc(c.fastq, good[:5] + [good[0]], c.k, c.count_min, None)
    c.assert_dbs(tmp_path, p)


def run_cli(args, cwd, check=True):
    from kmerlsh_amd import _native

    return subprocess.run([_native.CLI_PATH] + args, cwd=cwd, check=check, capture_output=True,
                          timeout=300)


@pytest.mark.gpu
def test_cli_kmc_db_then_mode_b(tmp_path):
    """-M K --only --kmc-db writes the table and db<j>; -M B --only on those databases rewrites
    the table byte for byte: the reference's K -> B hand-off."""
    from kmerlsh_amd.io import kmc_prefix_length

    fx = fixtures()["k31"]
    info = kc.write_case(str(tmp_path), "k31")
    run_cli(kc.cli_args(info, "K") + ["--kmc-db"], tmp_path)
    files = {n: (tmp_path / n).read_bytes() for n in FILES}
    assert files["kmer_count.log"].decode() == fx["log"]
    assert hashlib.md5(files["kmer_set.hex"]).hexdigest() == fx["hex_md5"]
    assert hashlib.md5(files["kmer_count.bin"]).hexdigest() == fx["bin_md5"]
    m = tmp_path / "model"
    m.mkdir()
    for j, name in enumerate(info["fastq"]):
        listing = kc.count_listing(str(tmp_path / name), info["k"], info["count_min"])
        ki.write_db(str(m / ("db%d" % j)), info["k"], listing, 0,
                    kmc_prefix_length(info["k"], len(listing)), 2, info["count_min"], 65535)
        for ext in EXTS:
            assert same_file(str(tmp_path / ("db%d" % j)) + ext, str(m / ("db%d" % j)) + ext)
    for n in FILES:
        os.remove(tmp_path / n)
    run_cli(kc.cli_args(info, "B"), tmp_path)
    assert {n: (tmp_path / n).read_bytes() for n in FILES} == files


@pytest.mark.gpu
def test_cli_kmc_db_only_and_usage(tmp_path):
    info = kc.write_case(str(tmp_path), "k5")
    dbs = sorted("db%d%s" % (j, e) for j in range(info["d"]) for e in EXTS)
    # plain -M K --only: the table, no database
    run_cli(kc.cli_args(info, "K"), tmp_path)
    assert all(os.path.exists(tmp_path / n) for n in FILES) and no_db_files(tmp_path)
    for n in FILES:
        os.remove(tmp_path / n)
    # --kmc-db-only: the databases, no table
    run_cli(kc.cli_args(info, "K") + ["--kmc-db-only"], tmp_path)
    assert sorted(n for n in os.listdir(tmp_path) if n.endswith(EXTS)) == dbs
    assert not any(os.path.exists(tmp_path / n) for n in FILES)
    # anywhere else it is a usage error, before anything runs
    for args in (kc.cli_args(info, "C") + ["--kmc-db-only"],
                 [a for a in kc.cli_args(info, "K") if a != "--only"] + ["--kmc-db-only"],
                 kc.cli_args(info, "K") + ["--kmc-db", "--kmc-db-only"]):
        r = run_cli(args, tmp_path, check=False)
        assert r.returncode == 2 and b"--kmc-db-only" in r.stderr
        assert not any(os.path.exists(tmp_path / n) for n in FILES)
