"""The host parser of klsh_diff_ksets under AddressSanitizer + UndefinedBehaviorSanitizer (CPU
only): `make -C kmerlsh_amd/csrc clust_parse` builds tests/cpp/clust_parse_main.cpp over
kmerlsh_amd/csrc/klsh_clust_parse.h — a stand-alone program, nothing is loaded into Python.  It
parses files in blocks of a given size and prints what it parsed; every print is compared with
tests/clust_model.py (which test_clust_model.py holds to libc's strtol).  Any sanitizer report
aborts: exit 0 = clean.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import clust_model as cm
from test_clust_model import corner_strings, random_regular_text

DRIVER = os.path.join(ROOT, "kmerlsh_amd", "build_asan", "clust_parse_main")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def driver():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kmerlsh_amd", "csrc"), "clust_parse"],
                   check=True, capture_output=True, timeout=600)
    return DRIVER


def run(driver, block, keep_ids, paths):
    p = subprocess.run([driver, str(block), "1" if keep_ids else "0"] + [str(x) for x in paths],
                       env=ENV, capture_output=True, text=True, timeout=300)
    report = "AddressSanitizer" in p.stderr or "runtime error" in p.stderr or "LeakSanitizer" in p.stderr
    assert p.returncode == 0 and not report, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def expected(path, text, keep_ids=True):
    m = cm.parse(text, want_ids=keep_ids)
    irr = cm.irregular_at(text)
    total = min(sum(m["counts"]), 2**64 - 1)  # (the program prints its saturating 64-bit sum)
    head = "file %s lines %d entries %d range %d irregular_at %d\n" % (
        path, len(m["counts"]), total, m["range"], -1 if irr is None else irr)
    if m["range"]:
        return head
    body = []
    for c, n in enumerate(m["counts"]):
        ids = m["ids"][m["offsets"][c]:m["offsets"][c + 1]] if keep_ids else []
        body.append(" ".join(str(v) for v in [n] + ids) + "\n")
    return head + "".join(body)


def check(driver, tmp_path, texts, blocks, keep_ids=True):
    paths = []
    for i, t in enumerate(texts):
        p = tmp_path / ("t%d.clust" % i)
        p.write_bytes(t)
        paths.append(str(p))
    want = "".join(expected(p, t, keep_ids) for p, t in zip(paths, texts))
    for block in blocks:
        assert run(driver, block, keep_ids, paths) == want, block


def small_counts(s: bytes) -> bytes:
    """A corner string as a line whose declared count is small: the string follows a count of 3,
    so its signs, overflows and junk land in the id chain (and stop it) instead of sizing it."""
    return b"3 " + s


def test_corner_files(driver, tmp_path):
    """The corner strings of test_clust_model as id chains and as whole lines of their own (the
    ones whose own first token would declare 2^32 entries or more are `range`), at block sizes
    that cut every line."""
    corners = [s for s in corner_strings() if b"\n" not in s]
    texts = [b"\n".join(small_counts(s) for s in corners) + b"\n",
             b"\n".join(small_counts(s) for s in corners)]
    for s in corners:
        texts.append(s)
        texts.append(s + b"\n2 1 2\n")
    texts += [b"", b"\n", b"\n\n", b"0", b"0\n", b"5", b"2 7\n\n\n1 9", b"\x00", b"\x00\n1 4\n",
              b"1 4\x00 5\n2 6 7\n", b"3\t10\n", b"2\t10\t20\t30\t40\n", b"0\t5\n"]
    got_range = sum(cm.parse(t, want_ids=False)["range"] for t in texts)
    got_irr = sum(cm.irregular_at(t) is not None for t in texts)
    assert got_range > 10 and got_irr > 30 and len(texts) - got_irr > 30
    check(driver, tmp_path, texts, blocks=(1, 2, 3, 7, 64, 1 << 20))


def test_random_byte_soup(driver, tmp_path):
    """Random bytes from an alphabet rich in digits, blanks, newlines, signs, NUL and high bytes,
    each line led by a small count; regular random texts too."""
    rng = np.random.default_rng(3)
    alphabet = np.frombuffer(b"0123456789 0123456789\t\v\f\r\n\n+-xA\x00\x80\xff", np.uint8)
    texts = []
    for i in range(60):
        soup = alphabet[rng.integers(0, alphabet.size, size=int(rng.integers(0, 300)))].tobytes()
        texts.append(b"\n".join(b"%d " % int(rng.integers(0, 9)) + ln for ln in soup.split(b"\n")))
    for i in range(30):
        texts.append(random_regular_text(rng, int(rng.integers(0, 30))))
    assert sum(cm.irregular_at(t) is None for t in texts) >= 30
    check(driver, tmp_path, texts, blocks=(1, 5, 16, 4096))


def test_block_edges(driver, tmp_path):
    """A newline, a token's first and last digit, a sign and a NUL at every position around a
    block edge: blocks of 16 bytes, the byte of interest at offsets 14 to 17 and 30 to 33."""
    texts = []
    for at in list(range(13, 19)) + list(range(29, 35)):
        pad = b"1" + b" " * (at - 1)  # a declared count of 1, blanks up to `at`
        texts.append(pad + b"\n2 5 6\n")            # newline at `at`
        texts.append(pad + b"12345\n2 5 6\n")       # a token starting at `at`
        texts.append(pad[:at - 4] + b"12345\n3 5")  # a token ending at `at`, no final newline
        texts.append(pad + b"-7\n1 8\n")            # a sign at `at`
        texts.append(pad + b"\x007\n1 8\n")         # a NUL at `at`
        texts.append(pad + b"9" * 19 + b"\n")       # an over-long run starting at `at`
    check(driver, tmp_path, texts, blocks=(16, 15, 17, 1, 1 << 16))


def test_truncated_and_empty_files(driver, tmp_path):
    full = b"3\t10\t20\t30\n2\t7\t8\n5\t1\t2\t3\t4\t5\n"
    texts = [full[:n] for n in range(len(full) + 1)]
    check(driver, tmp_path, texts, blocks=(4, 1 << 20))
    out = run(driver, 8, True, [tmp_path / "no_such_file"])
    assert out == "file %s unreadable\n" % (tmp_path / "no_such_file")


def test_saturating_count_sum(driver, tmp_path):
    """2^32 - 1 declared entries parse when no ids are kept; 2^32, counts that would wrap a 64-bit
    sum, and 18-digit counts are `range`: nothing is allocated for them (the sanitizer's allocator
    would refuse a 32 GB vector), and lines after the one that crossed the limit still count."""
    quarter = b"".join(b"%d\n" % (2**30) for _ in range(3))
    ok = quarter + b"%d 7\n" % (2**30 - 1)
    assert not cm.parse(ok, want_ids=False)["range"]
    check(driver, tmp_path, [ok], blocks=(5, 1 << 20), keep_ids=False)
    over = [quarter + b"%d 7\n" % (2**30) + b"1 2\n0\n", b"-1\n-1\n2\n", b"4294967296\n",
            b"999999999999999999 1\n" * 40, b"1 2\n9223372036854775807\n9223372036854775807\n3\n"]
    assert all(cm.parse(t, want_ids=False)["range"] for t in over)
    check(driver, tmp_path, over, blocks=(3, 1 << 20), keep_ids=True)
    check(driver, tmp_path, over, blocks=(1 << 20,), keep_ids=False)
