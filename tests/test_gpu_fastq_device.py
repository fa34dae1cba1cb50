"""Modes E and K over the device FASTQ parser: klsh_extract_fastq,
klsh_count_khtable and klsh_count_kmc give the same bytes and the same statistics whether the host
reader parses the file (option fastq_parse 1), the device parses it in one chunk (0), or in dozens
of chunks (0 with a small fastq_chunk_bytes) — with chunk ends inside each of a record's four
lines and exactly on a record's end; the host reader takes over where the grammar says so, and
fastq_parse 2 refuses exactly there.
"""
import contextlib
import gzip
import re

import numpy as np
import pytest

import fastq_model as fm
import klsh_oracle_e as oe
from kmerlsh_amd import _native

pytestmark = pytest.mark.gpu

K = 21
FILES = ("kmer_set.hex", "kmer_count.bin", "kmer_count.log")
E_STATS = ("reads", "bases", "reads_tested", "kmers_checked", "reads_extracted", "abnormal")
K_STATS = ("kmap_size", "reads", "bases", "positions", "distinct", "listed")
K_BATCH_STATS = ("batches", "rehashes")
K_BATCH_OPTIONS = ("kcount_batches", "kcount_rehashes", "kcount_peak_slots")
FASTQ_RO = ("fastq_device_chunks", "fastq_device_reads", "fastq_host_reads", "fastq_takeover_at")
NEVER = -1  # fastq_takeover_at: all ones


def make_records(seed, n):
    """n records: reads from a common source (so the vote selects some and k-mers repeat), N and
    lowercase and junk bases, reads of k + 9 and k + 10, empty sequences, names with '+' and '>',
    '+' lines with and without text, qualities that begin with '@' and '+'."""
    rng = np.random.default_rng(seed)
    src = rng.choice(list(b"ACGT"), size=6000).astype(np.uint8).tobytes()
    recs = []
    for i in range(n):
        u = i % 16
        ln = K + 9 if u == 0 else K + 10 if u == 1 else 0 if u == 2 and i % 160 == 2 else int(rng.integers(25, 220))
        a = int(rng.integers(0, len(src) - 220))
        s = bytearray(src[a:a + ln] if u % 3 else rng.choice(list(b"ACGT"), size=ln).astype(np.uint8).tobytes())
        for q in rng.integers(0, max(ln, 1), size=ln // 50):
            s[q] = int(rng.choice(list(b"NnacgtXY.")))
        q = bytearray(fm.quals(ln, i))
        if ln and u == 5:
            q[0] = ord("@")
        if ln and u == 6:
            q[0] = ord("+")
        name = b"r%d a+b>c %d" % (i, seed)
        recs.append(fm.record(name, bytes(s), bytes(q), b"+" + (name if u % 4 == 0 else b"")))
    return src, recs


def chunk_sizes(recs, near):
    """Chunk sizes whose first chunk ends inside L0, L1, L2, L3 of a record near offset `near`,
    and exactly on that record's end; each larger than every record."""
    ends = np.cumsum([len(r) for r in recs])
    j = int(np.searchsorted(ends, near))
    while recs[j].count(b"\n") != 4 or len(recs[j].split(b"\n")[2]) < 3 or len(recs[j].split(b"\n")[1]) < 3:
        j += 1
    s = int(ends[j - 1])
    l0, l1, l2, l3 = recs[j].split(b"\n")[:4]
    sizes = {"L0": s + 2, "L1": s + len(l0) + 1 + 2, "L2": s + len(l0) + len(l1) + 2 + 2,
             "L3": s + len(l0) + len(l1) + len(l2) + 3 + 2, "record end": int(ends[j])}
    text = b"".join(recs)
    starts = fm.parse(text)["line_starts"]
    for label, c in sizes.items():
        line = int(np.searchsorted(starts, c - 1, side="right")) - 1  # of the chunk's last byte
        assert line % 4 == {"L0": 0, "L1": 1, "L2": 2, "L3": 3, "record end": 3}[label], label
        assert (text[c - 1] == 10) == (label == "record end") and c > max(map(len, recs)), label
    return sizes


@contextlib.contextmanager
def options(engine, **kw):
    before = {name: engine.get_option(name) for name in kw}
    try:
        for name, v in kw.items():
            engine.set_option(name, v)
        yield
    finally:
        for name, v in before.items():
            engine.set_option(name, v)


def ro(engine):
    return {name: engine.get_option(name) for name in FASTQ_RO}


@pytest.fixture(scope="module")
def sample():
    src, recs = make_records(1, 3000)
    kset = np.unique(oe.canonical_kmers(src[:3500], K))
    return src, recs, kset


def test_default_is_documented(engine):
    """The shipped default and the options' ranges."""
    assert engine.get_option("fastq_parse") == 0
    assert engine.get_option("fastq_chunk_bytes") == 0 and engine.get_option("fastq_tile") == fm.TILE
    for name, bad in (("fastq_parse", 3), ("fastq_parse", -1), ("fastq_chunk_bytes", 63),
                      ("fastq_chunk_bytes", (1 << 31) + 1)):
        with pytest.raises(_native.KlshError, match="KLSH_E_ARG: " + name + " must be"):
            engine.set_option(name, bad)
    with pytest.raises(_native.KlshError, match="unknown option"):
        engine.set_option("fastq_device_reads", 1)


# ------------------------------------------------------------------------------- mode E --------
def extract(engine, ks, path, out, vote=0.3, **kw):
    with options(engine, **kw):
        st = ks.extract_fastq(str(path), str(out), K, vote)
        return st, out.read_bytes(), ro(engine)


def test_extract_three_ways(engine, sample, tmp_path):
    src, recs, kset = sample
    path = tmp_path / "in.fastq"
    path.write_bytes(b"".join(recs))
    ks = _native.KmerSet(engine, kset)
    try:
        st1, out1, ro1 = extract(engine, ks, path, tmp_path / "o1", fastq_parse=1)
        assert ro1 == dict(fastq_device_chunks=0, fastq_device_reads=0, fastq_host_reads=len(recs),
                           fastq_takeover_at=0)
        # the expected bytes, from the model's records and the oracle's vote
        m = fm.parse(b"".join(recs))
        _, flags = oe.check_reads([s for _, s, _ in m["records"]], kset, K, 0.3)
        want = b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n"
                        for (n, s, q), f in zip(m["records"], flags) if f)
        assert out1 == want and 0 < st1["reads_extracted"] == int(flags.sum()) < len(recs)
        assert st1["abnormal"] == sum(1 for _, s, _ in m["records"] if not s) > 0
        st0, out0, ro0 = extract(engine, ks, path, tmp_path / "o0", fastq_parse=0)
        assert out0 == out1 and [st0[f] for f in E_STATS] == [st1[f] for f in E_STATS]
        assert ro0 == dict(fastq_device_chunks=1, fastq_device_reads=len(recs), fastq_host_reads=0,
                           fastq_takeover_at=NEVER)
        assert engine.get_option("fastq_parse_us") > 0
        for label, c in chunk_sizes(recs, 20000).items():
            stc, outc, roc = extract(engine, ks, path, tmp_path / "oc", fastq_parse=0, fastq_chunk_bytes=c)
            assert outc == out1 and [stc[f] for f in E_STATS] == [st1[f] for f in E_STATS], label
            assert roc["fastq_device_chunks"] >= 24 and roc["fastq_takeover_at"] == NEVER, label
            assert roc["fastq_device_reads"] == len(recs) and roc["fastq_host_reads"] == 0, label
        # device only: nothing to refuse in this file
        st2, out2, _ = extract(engine, ks, path, tmp_path / "o2", fastq_parse=2, fastq_chunk_bytes=30000)
        assert out2 == out1
    finally:
        ks.close()


def test_extract_takeover(engine, sample, tmp_path):
    """A file whose 1500th record is multi-line: the device parses the chunks before the one that
    holds it, the host reader the rest; fastq_parse 2 refuses, naming that chunk's offset, and the
    context is usable afterwards."""
    src, recs, kset = sample
    recs = list(recs)
    n, s, q = fm.parse(recs[1500])["records"][0]
    recs[1500] = b"@" + n + b"\n" + s[:10] + b"\n" + s[10:] + b"\n+\n" + q + b"\n"
    text = b"".join(recs)
    path = tmp_path / "in.fastq"
    path.write_bytes(text)
    bad_at = len(b"".join(recs[:1500]))
    c = 30000
    # the chunk starts, by the chunk rule, from the model
    off, starts = 0, []
    while True:
        starts.append(off)
        m = fm.parse(text[off:off + c])
        if m["consumed"] == 0:
            break
        off += m["consumed"]
    assert starts[-1] <= bad_at < starts[-1] + c and len(starts) > 5
    ks = _native.KmerSet(engine, kset)
    try:
        st1, out1, _ = extract(engine, ks, path, tmp_path / "o1", fastq_parse=1)
        stc, outc, roc = extract(engine, ks, path, tmp_path / "oc", fastq_parse=0, fastq_chunk_bytes=c)
        assert outc == out1 and [stc[f] for f in E_STATS] == [st1[f] for f in E_STATS]
        assert roc["fastq_takeover_at"] == starts[-1] and roc["fastq_device_chunks"] == len(starts) - 1
        assert roc["fastq_device_reads"] + roc["fastq_host_reads"] == st1["reads"] == len(recs)
        assert 0 < roc["fastq_device_reads"] < len(recs)
        with pytest.raises(_native.KlshError, match=r"KLSH_E_ARG: .*take over at offset %d$" % starts[-1]):
            extract(engine, ks, path, tmp_path / "o2", fastq_parse=2, fastq_chunk_bytes=c)
        st0, out0, ro0 = extract(engine, ks, path, tmp_path / "o0", fastq_parse=0)  # one chunk: all host
        assert out0 == out1 and ro0["fastq_device_chunks"] == 0 and ro0["fastq_takeover_at"] == 0
    finally:
        ks.close()


def test_extract_host_only_inputs(engine, sample, tmp_path):
    """gzip, CRLF and a chunk smaller than the first record: no device chunk.  No final newline
    and a truncated last record: the host reader's records (test_mode_e holds it to read_fastq)."""
    src, recs, kset = sample
    recs = recs[:400]
    text = b"".join(recs)
    ks = _native.KmerSet(engine, kset)
    try:
        def both(name, data, **kw):
            p = tmp_path / name
            p.write_bytes(data)
            st1, out1, _ = extract(engine, ks, p, tmp_path / "o1", fastq_parse=1)
            st0, out0, ro0 = extract(engine, ks, p, tmp_path / "o0", fastq_parse=0, **kw)
            assert out0 == out1 and [st0[f] for f in E_STATS] == [st1[f] for f in E_STATS], name
            assert ro0["fastq_device_reads"] + ro0["fastq_host_reads"] == st1["reads"], name
            return st1, ro0

        st, r = both("a.fastq.gz", gzip.compress(text))
        assert r["fastq_device_chunks"] == 0 and r["fastq_takeover_at"] == 0 and st["reads"] == 400
        with pytest.raises(_native.KlshError, match="KLSH_E_ARG: .*gzip.*offset 0$"):
            extract(engine, ks, tmp_path / "a.fastq.gz", tmp_path / "o2", fastq_parse=2)
        st, r = both("crlf.fastq", text.replace(b"\n", b"\r\n"))
        assert r["fastq_device_chunks"] == 0 and r["fastq_takeover_at"] == 0 and st["reads"] == 400
        st, r = both("small_chunk.fastq", fm.record(b"long", fm.bases(300)) + text, fastq_chunk_bytes=64)
        assert r["fastq_device_chunks"] == 0 and r["fastq_takeover_at"] == 0 and st["reads"] == 401
        st, r = both("no_final_newline.fastq", text[:-1], fastq_chunk_bytes=9000)
        assert r["fastq_device_chunks"] > 5 and r["fastq_takeover_at"] == len(b"".join(recs[:399]))
        assert st["reads"] == 400 and r["fastq_host_reads"] == 1
        st, r = both("truncated.fastq", text[:-20], fastq_chunk_bytes=9000)
        assert st["reads"] == 399 and r["fastq_host_reads"] == 0 and r["fastq_device_reads"] == 399
        assert r["fastq_takeover_at"] == len(b"".join(recs[:399]))
        st, r = both("empty.fastq", b"")
        assert st["reads"] == 0 and r["fastq_takeover_at"] == NEVER
    finally:
        ks.close()


# ------------------------------------------------------------------------------- mode K --------
def count(engine, paths, out, dbs=None, **kw):
    out.mkdir(exist_ok=True)
    with options(engine, kcount_keep_listing=1, **kw):
        if dbs is None:
            st = engine.count_khtable([str(p) for p in paths], K, 2, str(out))
        else:
            st, _ = engine.count_kmc([str(p) for p in paths], [str(d) for d in dbs], K, 2, str(out))
        listings = [engine.kcount_listing(j) for j in range(len(paths))]
        batch = {name: engine.get_option(name) for name in K_BATCH_OPTIONS}
        files = [(out / n).read_bytes() for n in FILES]
        if dbs is not None:
            files += [(d.parent / (d.name + ext)).read_bytes() for d in dbs for ext in (".kmc_pre", ".kmc_suf")]
        return st, files, listings, batch, ro(engine)


def same_listings(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("with_dbs", [False, True])
def test_count_three_ways(engine, tmp_path, with_dbs):
    samples = [make_records(11, 2500)[1], make_records(12, 1800)[1]]
    paths = []
    for j, recs in enumerate(samples):
        paths.append(tmp_path / ("s%d.fastq" % j))
        paths[-1].write_bytes(b"".join(recs))
    total = sum(map(len, samples))
    dbs = lambda tag: [tmp_path / ("db_%s_%d" % (tag, j)) for j in range(2)] if with_dbs else None
    hooks = dict(kcount_batch_reads=700, kcount_table_slots=1024)  # several launches and rehashes
    st1, f1, l1, b1, ro1 = count(engine, paths, tmp_path / "t1", dbs("1"), fastq_parse=1, **hooks)
    assert ro1["fastq_device_chunks"] == 0 and ro1["fastq_host_reads"] == total
    assert st1["reads"] == total and b1["kcount_rehashes"] > 0
    assert b1["kcount_batches"] == sum(-(-len(r) // 700) for r in samples)
    st0, f0, l0, b0, ro0 = count(engine, paths, tmp_path / "t0", dbs("0"), fastq_parse=0, **hooks)
    assert f0 == f1 and same_listings(l0, l1)
    assert [st0[f] for f in K_STATS + K_BATCH_STATS] == [st1[f] for f in K_STATS + K_BATCH_STATS]
    assert b0 == b1  # one chunk per file: the host path's launches, rehashes and peak
    assert ro0 == dict(fastq_device_chunks=2, fastq_device_reads=total, fastq_host_reads=0,
                       fastq_takeover_at=NEVER)
    for label, c in chunk_sizes(samples[0], 15000).items():
        stc, fc, lc, bc, roc = count(engine, paths, tmp_path / "tc", dbs("c"), fastq_parse=0,
                                     fastq_chunk_bytes=c, **hooks)
        assert fc == f1 and same_listings(lc, l1), label
        assert [stc[f] for f in K_STATS] == [st1[f] for f in K_STATS], label
        assert roc["fastq_device_chunks"] >= 40 and roc["fastq_device_reads"] == total, label
        assert roc["fastq_host_reads"] == 0 and roc["fastq_takeover_at"] == NEVER, label
        if with_dbs:
            break  # (the chunk ends inside every line: once, with the table alone)


def test_count_takeover_and_refusal(engine, tmp_path):
    """Mode K over a file that turns irregular: device chunks, then the host reader; fastq_parse 2
    refuses it, and the context counts on afterwards."""
    recs = make_records(21, 1200)[1]
    n, s, q = fm.parse(recs[700])["records"][0]
    recs[700] = b"@" + n + b"\r\n" + s + b"\r\n+\r\n" + q + b"\r\n"
    path = tmp_path / "s.fastq"
    path.write_bytes(b"".join(recs) + b"@last\nACGTACGTACGTACGTACGTACGTACGT")  # and no quality at the end
    hooks = dict(kcount_batch_reads=500)
    st1, f1, l1, _, _ = count(engine, [path], tmp_path / "t1", fastq_parse=1, **hooks)
    assert st1["reads"] == 1201
    stc, fc, lc, _, roc = count(engine, [path], tmp_path / "tc", fastq_parse=0, fastq_chunk_bytes=20000, **hooks)
    assert fc == f1 and same_listings(lc, l1) and [stc[f] for f in K_STATS] == [st1[f] for f in K_STATS]
    assert roc["fastq_device_chunks"] > 3 and 0 < roc["fastq_device_reads"] <= 700
    assert roc["fastq_device_reads"] + roc["fastq_host_reads"] == 1201
    assert roc["fastq_takeover_at"] <= len(b"".join(recs[:700])) < roc["fastq_takeover_at"] + 20000
    with pytest.raises(_native.KlshError) as err:
        count(engine, [path], tmp_path / "t2", fastq_parse=2, fastq_chunk_bytes=20000, **hooks)
    assert re.search(r"KLSH_E_ARG: .*take over at offset %d$" % roc["fastq_takeover_at"], str(err.value))
    st0, f0, l0, _, ro0 = count(engine, [path], tmp_path / "t0", fastq_parse=0, fastq_chunk_bytes=20000, **hooks)
    assert f0 == f1 and ro0 == roc


def test_extract_from_a_fifo(engine, sample, tmp_path):
    """A path that is not a regular file (a FIFO here; a process substitution or /dev/stdin alike)
    has no size and takes no positioned reads: the host reader reads it from its first byte, plain
    or gzip, as it always did; fastq_parse 2 refuses it without opening it."""
    import os
    import threading

    src, recs, kset = sample
    recs = recs[:500]
    text = b"".join(recs)
    plain = tmp_path / "in.fastq"
    plain.write_bytes(text)
    fifo = tmp_path / "in.fifo"
    os.mkfifo(fifo)
    ks = _native.KmerSet(engine, kset)
    try:
        st1, out1, _ = extract(engine, ks, plain, tmp_path / "o1", fastq_parse=1)
        assert st1["reads"] == 500 and 0 < st1["reads_extracted"] < 500
        with pytest.raises(_native.KlshError, match="KLSH_E_ARG: .*not a regular file.*offset 0$"):
            extract(engine, ks, fifo, tmp_path / "o2", fastq_parse=2)  # (no writer: it must not block)
        for data in (text, gzip.compress(text)):
            def feed():
                with open(fifo, "wb") as f:
                    f.write(data)

            t = threading.Thread(target=feed)
            t.start()
            try:
                st0, out0, ro0 = extract(engine, ks, fifo, tmp_path / "o0", fastq_parse=0)
            finally:
                t.join(timeout=30)
            assert not t.is_alive()
            assert out0 == out1 and [st0[f] for f in E_STATS] == [st1[f] for f in E_STATS]
            assert ro0 == dict(fastq_device_chunks=0, fastq_device_reads=0, fastq_host_reads=500,
                               fastq_takeover_at=0)
    finally:
        ks.close()
