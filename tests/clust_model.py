"""The reference's reader of <F>.clust restated over bytes, and the grammar of a REGULAR text
(DESIGN.md §15).  The model the parsers of klsh_diff_ksets are held to.

IOMat::ReadClusterAll (io/ioMatrix.cc:48-119) takes the text line by line (std::getline) and runs a
strtol chain over each line: the first strtol gives n, the declared member count; up to n further
strtol results are the ids; the ones a short line does not hold stay 0; tokens past n are ignored.
The oracle's read_cluster_all splits on whitespace, which agrees with that only on clean text; this
module follows strtol itself (C locale, base 10): leading isspace bytes, an optional sign, digits,
the value clamped to [LONG_MIN, LONG_MAX], nothing converted when no digit follows.
"""
from __future__ import annotations

LONG_MAX = 2**63 - 1
LONG_MIN = -(2**63)
U64 = 2**64
MAX_ENTRIES = 2**32          # the declared counts must sum to less
MAX_DIGITS = 18              # a longer digit run could reach LONG_MAX: the text is irregular
SPACES = frozenset(b" \t\n\v\f\r")        # isspace in the C locale
BLANKS = frozenset(b" \t\v\f\r")          # the five other than the newline
DIGITS = frozenset(b"0123456789")


def strtol(buf: bytes, pos: int = 0) -> tuple[int, int]:
    """strtol(buf + pos, &end, 10) on a NUL-terminated buffer: (value, end).  end == pos when
    nothing was converted.  `buf` is read up to its first NUL byte at or after pos, or its end."""
    n = len(buf)
    i = pos
    while i < n and buf[i] != 0 and buf[i] in SPACES:
        i += 1
    neg = False
    if i < n and buf[i] in b"+-":
        neg = buf[i] == 0x2D
        i += 1
    start = i
    v = 0
    while i < n and buf[i] in DIGITS:
        v = v * 10 + (buf[i] - 0x30)
        i += 1
    if i == start:
        return 0, pos
    v = -v if neg else v
    return max(LONG_MIN, min(LONG_MAX, v)), i


def lines_of(text: bytes) -> list[bytes]:
    """std::getline's lines: an unterminated, non-empty last line counts; the empty text has none."""
    parts = text.split(b"\n")
    last = parts.pop()
    if last:
        parts.append(last)
    return parts


def parse_line(line: bytes) -> tuple[int, list[int]]:
    """(n as the uint64 the reference sizes its vector with, the entries the chain stores — at most
    n: each strtol result, the 0 of the first strtol that converts nothing included, after which
    the chain ends; the caller fills the rest with 0)."""
    z = line.find(b"\0")
    s = line if z < 0 else line[:z]  # strtol reads a C string
    v, e = strtol(s, 0)
    n = v % U64
    ids, p = [], 0
    while p != e and len(ids) < n:
        p = e
        v, e = strtol(s, p)
        ids.append(v % U64)
    return n, ids


def parse(text: bytes, want_ids: bool = True):
    """The whole text: dict(counts, offsets, ids, entries, range).  entries is the saturating sum
    of the declared counts clamped at 2^32; from there on `range` is True and offsets / ids are
    None (the library refuses with KLSH_E_RANGE before allocating anything of that size)."""
    counts, per_line = [], []
    for line in lines_of(text):
        n, ids = parse_line(line) if want_ids else (parse_line_count(line), None)
        counts.append(n)
        per_line.append(ids)
    total = sum(counts)
    if total >= MAX_ENTRIES:
        return dict(counts=counts, offsets=None, ids=None, entries=MAX_ENTRIES, range=True)
    offsets, flat = [0], []
    for n, ids in zip(counts, per_line):
        offsets.append(offsets[-1] + n)
        if want_ids:
            flat.extend(ids + [0] * (n - len(ids)))
    return dict(counts=counts, offsets=offsets, ids=flat if want_ids else None, entries=total,
                range=False)


def parse_line_count(line: bytes) -> int:
    z = line.find(b"\0")
    return strtol(line if z < 0 else line[:z], 0)[0] % U64


def irregular_at(text: bytes):
    """The smallest offset that makes the text irregular: a byte that is no digit, no newline and
    none of the five blanks, or the first digit of a run of more than MAX_DIGITS digits.  None for a
    regular text."""
    best = None
    run = 0
    for i, c in enumerate(text):
        if c in DIGITS:
            run += 1
            if run == MAX_DIGITS + 1:
                best = i - MAX_DIGITS if best is None else min(best, i - MAX_DIGITS)
            continue
        run = 0
        if c != 0x0A and c not in BLANKS and best is None:
            best = i
    return best


def tokens_of(line: bytes) -> list[int]:
    """The maximal digit runs of a line of a regular text, as values."""
    out, cur = [], None
    for c in line:
        if c in DIGITS:
            cur = (cur or 0) * 10 + (c - 0x30)
        elif cur is not None:
            out.append(cur)
            cur = None
    if cur is not None:
        out.append(cur)
    return out


def parse_regular(text: bytes):
    """What the kernels compute on a regular text, stated on digit runs alone: per line, n = the
    first token (0 without one), entry j = token 1 + j, 0 past the line's tokens.  test_clust_model
    holds this equal to parse() on every regular text it sees."""
    assert irregular_at(text) is None
    counts, offsets, ids = [], [0], []
    for line in lines_of(text):
        t = tokens_of(line)
        n = t[0] if t else 0
        counts.append(n)
        offsets.append(offsets[-1] + n)
        if offsets[-1] < MAX_ENTRIES:
            ids.extend((t[1 + j] if 1 + j < len(t) else 0) for j in range(n))
    return counts, offsets, ids


def select(counts, offsets, ids, groups, kmap: int):
    """The marks of the two sets (app/kmerLSH.cc:541-585): the ids < kmap of group-1 clusters mark
    A, of group-2 clusters B; row i goes to A if marked A, else to B if marked B.
    Returns (sorted ids marked A, sorted ids marked B, rows of A, rows of B)."""
    a, b = set(), set()
    for c, g in enumerate(groups):
        if g not in (1, 2):
            continue
        dst = a if g == 1 else b
        for q in range(offsets[c], offsets[c + 1]):
            if ids[q] < kmap:
                dst.add(ids[q])
    rows_a = sorted(a)
    rows_b = sorted(b - a)
    return sorted(a), sorted(b), rows_a, rows_b


def kset_slots(n: int) -> int:
    """klsh_kset_create's capacity for n keys: a power of two, at least 1024 and at least 2 n."""
    cap = 1024
    while cap < 2 * n:
        cap *= 2
    return cap
