"""The host FASTQ reader of modes E and K under AddressSanitizer + UndefinedBehaviorSanitizer (CPU
only): `make -C kmerlsh_amd/csrc fastq_reader` builds tests/cpp/fastq_reader_main.cpp over
kmerlsh_amd/csrc/klsh_fastq_reader.h and zlib — a stand-alone program, nothing is loaded into
Python.  It opens a file at a byte offset, as the host takeover of the device parser does
(DESIGN.md §16), and prints the records it reads; they are compared with the oracle's
read_fastq on the file's suffix from that offset.  Any sanitizer report aborts: exit 0 = clean.
"""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import fastq_model as fm
import klsh_oracle_e as oe

DRIVER = os.path.join(ROOT, "kmerlsh_amd", "build_asan", "fastq_reader_main")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def driver():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kmerlsh_amd", "csrc"), "fastq_reader"],
                   check=True, capture_output=True, timeout=600)
    return DRIVER


def run(driver, per, pairs):
    args = [driver, str(per)]
    for path, off in pairs:
        args += [str(path), str(off)]
    p = subprocess.run(args, env=ENV, capture_output=True, text=True, timeout=300)
    report = "AddressSanitizer" in p.stderr or "runtime error" in p.stderr or "LeakSanitizer" in p.stderr
    assert p.returncode == 0 and not report, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def hexf(b):
    return b.hex() if b else "-"


def expected(tmp_path, path, text, off):
    suffix = tmp_path / "suffix.fastq"
    suffix.write_bytes(text[off:])
    recs = oe.read_fastq(str(suffix))
    body = "".join("%s %s %s\n" % (hexf(n), hexf(s), hexf(q)) for n, s, q in recs)
    return "file %s offset %d\n%srecords %d\n" % (path, off, body, len(recs))


def check(driver, tmp_path, cases, pers=(1, 3, 1 << 18)):
    """cases: [(text, [offsets])]"""
    pairs, want = [], ""
    for i, (text, offsets) in enumerate(cases):
        p = tmp_path / ("f%d.fastq" % i)
        p.write_bytes(text)
        for off in offsets:
            pairs.append((p, off))
            want += expected(tmp_path, p, text, off)
    for per in pers:
        assert run(driver, per, pairs) == want, per


def test_regular_texts_at_record_boundaries(driver, tmp_path):
    cases = []
    for label, text in fm.regular_texts():
        s = fm.parse(text)["line_starts"][::4]
        cases.append((text, sorted({0, s[len(s) // 2], s[-1]})))
    check(driver, tmp_path, cases)


def test_irregular_texts_from_the_chunk_start(driver, tmp_path):
    """The takeover: the reader starts at a record boundary before the irregularity and reads the
    rest of the file by the reference's rules (CR, multi-line sequences, '>' headers, truncation)."""
    cases = []
    for label, text, at in fm.irregular_texts():
        m = fm.parse(text)
        s = m["line_starts"]
        cases.append((text, sorted({0, s[4 * (m["first_bad"] // 2)], s[4 * m["first_bad"]]})))
    check(driver, tmp_path, cases)


def test_junk_and_truncation(driver, tmp_path):
    good = fm.filler(200)
    texts = [b"", b"\n", b"@", b"@n", b"@n\n", b"@n\nAC", b"@n\nAC\n+", b"@n\nAC\n+\nI", b"junk\n" + good,
             good + b"@n\nAC\xffGT\n+\nIIII\n" + good, good + b">fa\nACGT\nACGT\n>fb\nAC\n",
             good + b"@n\nACGT\n+\nII\n@m\nAC\n+\nII\n", good[:-1], good + b"\n\n\n", good + b"@x\nAC\n+\nI\xffI\n"]
    check(driver, tmp_path, [(t, [0] + ([200] if len(t) > 200 else [])) for t in texts])
    out = run(driver, 8, [(tmp_path / "no_such_file", 0)])
    assert out == "file %s unreadable\n" % (tmp_path / "no_such_file")


def test_offsets_across_the_read_buffer(driver, tmp_path):
    """A file of several read buffers (1 MB each), opened before, at and after a buffer edge."""
    rng = np.random.default_rng(5)
    recs = []
    for i in range(9000):
        n = int(rng.integers(100, 160))
        recs.append(fm.record(b"r%d" % i, fm.bases(n, i), fm.quals(n, i)))
    text = b"".join(recs)
    assert len(text) > 2 * (1 << 20)
    ends = np.cumsum([len(r) for r in recs])
    edge = int(ends[np.searchsorted(ends, 1 << 20)])
    check(driver, tmp_path, [(text, [0, int(ends[10]), edge, int(ends[-2])])], pers=(1 << 18,))


def test_gzip_from_the_start(driver, tmp_path):
    text = fm.filler(5000) + b"@n\r\nACGT\r\n+\r\nIIII\r\n"
    p = tmp_path / "z.fastq.gz"
    with gzip.open(p, "wb") as f:
        f.write(text)
    plain = tmp_path / "z.fastq"
    plain.write_bytes(text)
    recs = oe.read_fastq(str(plain))
    body = "".join("%s %s %s\n" % (hexf(n), hexf(s), hexf(q)) for n, s, q in recs)
    assert run(driver, 64, [(p, 0)]) == "file %s offset 0\n%srecords %d\n" % (p, body, len(recs))
