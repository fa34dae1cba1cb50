"""tests/clust_model.py tied down (CPU): the model of the reference's <F>.clust reader that the
host parser (test_clust_host.py) and the device parser (test_gpu_diff_ksets.py) are held to.

Three ways: its strtol against libc's own through ctypes, over corner and random strings; its parse
against the oracle's read_cluster_all on the three mode_e_inputs cases (clean text, where splitting
on whitespace and the strtol chain agree); its grammar against hand-written expectations.
"""
import ctypes
import ctypes.util
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

import clust_model as cm
import klsh_oracle_e as oe  # noqa: E402  (oracle/ is on sys.path via conftest)

sys.path.insert(0, GOLDEN)
import mode_e_inputs as mi  # noqa: E402

_libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
_libc.strtol.restype = ctypes.c_long
_libc.strtol.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]


def libc_strtol(s: bytes, pos: int):
    buf = ctypes.create_string_buffer(s)  # (NUL-terminated)
    base = ctypes.addressof(buf)
    end = ctypes.c_void_p(0)
    v = _libc.strtol(base + pos, ctypes.byref(end), 10)
    return int(v), int(end.value) - base


def corner_strings():
    out = [b"", b"0", b"7", b"-7", b"+7", b"+-7", b"-+7", b"- 7", b"--7", b"+", b"-", b" ", b"x",
           b"12x", b"12 x", b"x12", b"0x10", b"00012", b"1e5", b"1.5", b"\t\n\v\f\r 42",
           b"42\t\n\v\f\r ", b"4 2", b"\x0042", b"4\x002", b"\xff1", b"1\xff", b"\x801", b"1_000"]
    for nd in (17, 18, 19, 20, 21, 40):
        for lead in (b"1", b"9", b"0"):
            out.append(lead * nd)
            out.append(b"-" + lead * nd)
            out.append(b" " + lead * nd + b" 5")
    for v in (cm.LONG_MAX - 1, cm.LONG_MAX, cm.LONG_MAX + 1, 10**18 - 1, 10**18, 10**19,
              -cm.LONG_MIN - 1, -cm.LONG_MIN, -cm.LONG_MIN + 1):
        out.append(b"%d" % v)
        out.append(b"-%d" % v)
        out.append(b"+%d" % v)
        out.append(b"\r%d\r" % v)
    for sp in b" \t\n\v\f\r":
        out.append(bytes([sp]) + b"5")
        out.append(b"5" + bytes([sp]) + b"6")
        out.append(bytes([sp, sp]) + b"-5" + bytes([sp]))
    return out


def random_strings(n, seed):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"0123456789 0123456789\t\v\f\r\n+-xA\x00\x80\xff", np.uint8)
    out = []
    for _ in range(n):
        ln = int(rng.integers(0, 40))
        out.append(alphabet[rng.integers(0, alphabet.size, size=ln)].tobytes())
    return out


def test_strtol_matches_libc():
    """The model's strtol gives libc's value and end pointer from every start position of a few
    thousand strings: signs, 17- to 40-digit runs, LONG_MAX +- 1 and LONG_MIN +- 1, all six space
    bytes, NUL, letters after digits, bytes of 128 and above."""
    cases = corner_strings() + random_strings(3000, 1)
    assert len(cases) > 3000
    seen_clamp = seen_none = 0
    for s in cases:
        z = s.find(b"\0")
        c_str = s if z < 0 else s[:z]
        for pos in range(len(c_str) + 1):
            got, want = cm.strtol(c_str, pos), libc_strtol(s, pos)
            assert got == want, (s, pos, got, want)
            seen_clamp += want[0] in (cm.LONG_MAX, cm.LONG_MIN)
            seen_none += want[1] == pos
    assert seen_clamp > 50 and seen_none > 1000


def test_parse_line_is_the_reference_chain():
    """Hand-written lines: declared count against tokens held, zero fill, ignored tokens, signs, a
    NUL that ends the C string, a token that stops the chain."""
    U = cm.U64
    for line, n, ids in [
        (b"3\t10\t20\t30", 3, [10, 20, 30]),
        (b"3\t10", 3, [10, 0]),                # short: the failed strtol stores a 0 and ends it
        (b"2\t10\t20\t30\t40", 2, [10, 20]),   # tokens past n are ignored
        (b"0\t5", 0, []),
        (b"", 0, []),
        (b" \t ", 0, []),
        (b"0003 007 08 9", 3, [7, 8, 9]),
        (b"2 \r\v\f 5  \t6\r", 2, [5, 6]),
        (b"2 5x 6", 2, [5, 0]),                # 'x' converts nothing: one 0 is stored, then it ends
        (b"3 5 -6 7", 3, [5, U - 6, 7]),
        (b"-1", U - 1, [0]),
        (b"2 5\x006", 2, [5, 0]),              # strtol sees "2 5"
        (b"x 5", 0, []),
        (b"2 999999999999999999 1000000000000000000", 2, [10**18 - 1, 10**18]),
        (b"1 99999999999999999999", 1, [cm.LONG_MAX]),
    ]:
        assert cm.parse_line(line) == (n, ids), line


def test_lines_are_getlines():
    assert cm.lines_of(b"") == []
    assert cm.lines_of(b"\n") == [b""]
    assert cm.lines_of(b"1") == [b"1"]
    assert cm.lines_of(b"1\n") == [b"1"]
    assert cm.lines_of(b"1\n\n") == [b"1", b""]
    assert cm.lines_of(b"\n\n2") == [b"", b"", b"2"]
    assert cm.lines_of(b"1\r\n2") == [b"1\r", b"2"]


def test_irregular_at_by_hand():
    nine = b"9" * 18
    for text, want in [
        (b"", None), (b"\n", None), (b"3\t1\t2\t3\n", None), (b" \t\v\f\r\n0", None),
        (nine, None), (nine + b"\n" + nine, None), (b"1 " + nine + b" 2\n", None),
        (b"x", 0), (b"1x", 1), (b"12\n-3\n", 3), (b"1\n2+\n", 3), (b"12\x00", 2), (b"\x80", 0),
        (b"1 2\xff", 3), (b"1\x0b2", None), (b"1\x0e2", 1), (b"1\x082", 1), (b"1\x1f2", 1),
        (nine + b"9", 0),                       # 19 digits: the run's first digit
        (b"5\n" + nine + b"0 7\n", 2),
        (b"5\n" + b"0" * 30, 2),                # leading zeros count: strtol is not asked
        (b"a" + nine + b"9", 0),                # two: the smaller offset
        (nine + b"9 a", 0), (b"1 a " + nine + b"9", 2), (b"12 " + nine + b"9 a", 3),
    ]:
        assert cm.irregular_at(text) == want, text


def random_regular_text(rng, n_lines: int) -> bytes:
    """Lines of a regular text: empty, blank-only, or a small declared count (leading zeros at
    times) and 0 to 8 further tokens of up to 18 digits, between random blanks."""
    blanks = [b" ", b"\t", b"\v", b"\f", b"\r", b"  ", b"\t \r"]
    lines = []
    for _ in range(n_lines):
        u = int(rng.integers(0, 10))
        if u == 0:
            lines.append(b"")
            continue
        if u == 1:
            lines.append(blanks[int(rng.integers(0, len(blanks)))])
            continue
        toks = [b"0" * int(rng.integers(0, 3)) + b"%d" % int(rng.integers(0, 6))]
        for _ in range(int(rng.integers(0, 9))):
            toks.append(b"%d" % int(rng.integers(0, 10 ** int(rng.integers(1, 19)))))
        line = b"" if rng.integers(0, 4) else blanks[int(rng.integers(0, len(blanks)))]
        for t in toks:
            line += t + blanks[int(rng.integers(0, len(blanks)))]
        lines.append(line if rng.integers(0, 3) else line.rstrip())
    text = b"\n".join(lines)
    return text + (b"\n" if rng.integers(0, 2) else b"")


def test_regular_text_is_a_function_of_digit_runs():
    """On regular text the strtol chain equals the statement on digit runs the kernels implement:
    random regular texts with every blank byte, empty and blank-only lines, leading zeros, short
    and long lines, with and without a final newline."""
    rng = np.random.default_rng(2)
    short = long_ = empty = 0
    for it in range(300):
        text = random_regular_text(rng, int(rng.integers(0, 12)))
        assert cm.irregular_at(text) is None, text
        m = cm.parse(text)
        counts, offsets, ids = cm.parse_regular(text)
        assert (m["counts"], m["offsets"], m["ids"]) == (counts, offsets, ids), text
        for ln, n in zip(cm.lines_of(text), counts):
            t = cm.tokens_of(ln)
            short += n > max(len(t) - 1, 0)
            long_ += len(t) - 1 > n
            empty += not t
    assert short > 20 and long_ > 20 and empty > 20


@pytest.mark.parametrize("case", sorted(mi.CASES))
def test_parse_matches_oracle_on_mode_e_cases(case, tmp_path):
    c = mi.CASES[case]
    mi.write_case(str(tmp_path), case)
    path = os.path.join(str(tmp_path), "clustering_result.txt")
    _, id_lists = oe.read_cluster_all(path, c["n1"] + c["n2"])
    with open(path + ".clust", "rb") as f:
        text = f.read()
    assert cm.irregular_at(text) is None
    m = cm.parse(text)
    assert m["counts"] == [len(x) for x in id_lists]
    assert m["ids"] == [int(i) for x in id_lists for i in x]
    assert (m["counts"], m["offsets"], m["ids"]) == cm.parse_regular(text)


def test_range_is_a_saturating_sum():
    """2^32 - 1 declared entries parse (no ids asked for); 2^32, and counts that would wrap a
    64-bit sum, are `range`."""
    lines = b"".join(b"%d\n" % (2**30) for _ in range(3))
    m = cm.parse(lines + b"%d 7\n" % (2**30 - 1), want_ids=False)
    assert not m["range"] and m["entries"] == 2**32 - 1 and m["offsets"][-1] == 2**32 - 1
    m = cm.parse(lines + b"%d 7\n" % (2**30), want_ids=False)
    assert m["range"] and m["entries"] == 2**32 and m["offsets"] is None
    m = cm.parse(b"-1\n-1\n2\n", want_ids=False)  # 2^64 - 1 twice: wraps unless saturating
    assert m["range"] and m["entries"] == 2**32
    m = cm.parse(b"999999999999999999 1\n" * 40, want_ids=False)
    assert m["range"]


def test_select_and_capacity():
    a, b, ra, rb = cm.select([2, 3, 1], [0, 2, 5, 6], [1, 9, 1, 2, 0, 4], [1, 2, 0], kmap=9)
    assert (a, b, ra, rb) == ([1], [0, 1, 2], [1], [0, 2])
    assert [cm.kset_slots(n) for n in (0, 512, 513, 1024, 1025)] == [1024, 1024, 2048, 2048, 4096]
