"""The regular FASTQ grammar of the device parser in Python, and the builders of
the test texts.  test_fastq_model.py holds it to the oracle's kseq restatement
(oracle/klsh_oracle_e.py::read_fastq); the GPU tests hold the kernels to it.

A chunk starts at a record boundary.  Lines are split at "\\n"; record r is lines 4r .. 4r + 3; the
complete records are the newlines // 4 first.  parse() returns

    n            complete records
    line_starts  4 n + 1 offsets: each line's first byte, then the end of the last complete record
    irregular_at the smallest offset that makes a complete record irregular, None if none does
    first_bad    the record that offset lies in (None if none)
    consumed     line_starts[4 n] when every complete record is regular, else 0
    records      [(name, seq, qual)] of the complete records when regular, else of those before
                 first_bad
"""

AT, PLUS, GT, NL = 64, 43, 62, 10


def l1_ok(c):
    return 33 <= c <= 126 and c not in (AT, PLUS, GT)


def l3_ok(c):
    return 33 <= c <= 127


def parse(text: bytes) -> dict:
    nls = [i for i, c in enumerate(text) if c == NL]
    n = len(nls) // 4
    starts = [0] + [p + 1 for p in nls[:4 * n]]
    bad = []  # every offending offset

    for r in range(n):
        s = starts[4 * r:4 * r + 5]
        lines = [text[s[j]:s[j + 1] - 1] for j in range(4)]
        # L0: the line's first byte (its newline, if it is empty) must be '@'
        if text[s[0]] != AT:
            bad.append(s[0])
        bad += [s[1] + i for i, c in enumerate(lines[1]) if not l1_ok(c)]
        if text[s[2]] != PLUS:
            bad.append(s[2])
        bad += [s[2] + i for i, c in enumerate(lines[2]) if i > 0 and c >= 0x80]
        bad += [s[3] + i for i, c in enumerate(lines[3]) if not l3_ok(c)]
        if len(lines[1]) != len(lines[3]):
            # the newline that came too early, or the first byte too many
            bad.append(s[3] + min(len(lines[1]), len(lines[3])))
    irregular_at = min(bad) if bad else None
    first_bad = None
    if bad:
        first_bad = max(r for r in range(n) if starts[4 * r] <= irregular_at)
    good = n if first_bad is None else first_bad
    records = []
    for r in range(good):
        s = starts[4 * r:4 * r + 5]
        records.append((text[s[0] + 1:s[1] - 1], text[s[1]:s[2] - 1], text[s[3]:s[4] - 1]))
    return dict(n=n, line_starts=starts, irregular_at=irregular_at, first_bad=first_bad,
                consumed=starts[4 * n] if not bad else 0, records=records)


def seq_arrays(records):
    """(seq_off list, packed sequences) as the parser leaves them"""
    off = [0]
    for _, s, _ in records:
        off.append(off[-1] + len(s))
    return off, b"".join(s for _, s, _ in records)


# ---------------------------------------------------------------------------- builders ---------
def record(name: bytes, seq: bytes, qual: bytes = None, plus: bytes = b"+") -> bytes:
    if qual is None:
        qual = b"I" * len(seq)
    return b"@" + name + b"\n" + seq + b"\n" + plus + b"\n" + qual + b"\n"


def bases(n: int, salt: int = 0) -> bytes:
    return bytes(b"ACGT"[(i * 7 + salt + i // 5) & 3] for i in range(n))


def quals(n: int, salt: int = 0) -> bytes:
    return bytes(33 + (i * 11 + salt) % 94 for i in range(n))


def filler(total: int, tag: int = 0) -> bytes:
    """Regular records of exactly `total` bytes (total >= 8, or 0): short ones, the last stretched."""
    if total == 0:
        return b""
    assert total >= 8, total
    out = []
    left = total
    i = 0
    while left:
        # a record of name length a and sequence length b takes a + 2 b + 6 bytes (a bare '+' line)
        size = 47 if left >= 47 + 8 else left
        b = (size - 6) // 2
        a = size - 6 - 2 * b
        out.append(record(b"n" * a, bases(b, tag + i), quals(b, tag + i)))
        assert len(out[-1]) == size
        left -= size
        i += 1
    return b"".join(out)


def newline_at(pos: int, kind: int, tag: int = 0) -> bytes:
    """A regular text whose line of kind `kind` (0..3) ends with its newline at offset `pos`, with
    records before and after it."""
    # the record holding that line: name 3, sequence 9, '+x', quality 9
    name, seq, plus, qual = b"nam", bases(9, tag), b"+x", quals(9, tag)
    rec = record(name, seq, qual, plus)
    ends = [len(b"@" + name), len(b"@" + name + b"\n" + seq),
            len(b"@" + name + b"\n" + seq + b"\n" + plus), len(rec) - 1]
    before = pos - ends[kind]
    assert before == 0 or before >= 8, before
    text = filler(before, tag) + rec + filler(60, tag + 1)
    assert text[pos] == NL
    return text


def line_start_at(pos: int, kind: int, tag: int = 0) -> bytes:
    """... whose line of kind `kind` starts at offset `pos`"""
    return newline_at(pos - 1, (kind + 3) % 4, tag) if kind else filler(pos, tag) + filler(60, tag + 1)


TILE = 4096  # the parser's tile (read-only option "fastq_tile"; the GPU tests check it is this)


def regular_texts(T: int = TILE):
    """[(label, text)]: regular complete records (a partial tail where the label says so), the
    edges at chosen offsets around the tile size T."""
    out = []
    for kind in range(4):
        for pos in (T - 1, T, T + 1):
            out.append(("newline of L%d at %d" % (kind, pos), newline_at(pos, kind, kind)))
    # one record's lines over three tiles and more: L0 across the first edge, L1 and L3 a tile long
    out.append(("record over tiles", filler(T - 10) + record(b"x" * 20, bases(T, 3), quals(T, 5)) + filler(50)))
    for shift in range(16):  # a line start at every byte of a lane's 16, each kind in turn
        for kind in range(4):
            out.append(("L%d starts at lane byte %d" % (kind, shift),
                        line_start_at(T + 160 + shift, kind, shift)))
    out.append(("L3 begins with @", filler(40) + record(b"q", b"ACGT", b"@II+") + filler(40)))
    out.append(("L3 begins with +", filler(40) + record(b"q", b"ACGT", b"+II@") + filler(40)))
    out.append(("L0 holds + > and high bytes", record(b"a+b>c@d\x80\xff\x00 e\r", b"ACGTN") + filler(40)))
    out.append(("L2 holds text", record(b"n", b"ACGTNacgtn.-*", None, b"+n some text\x7f\x01") + filler(40)))
    out.append(("quality 33 and 127", record(b"n", b"ACG", b"!\x7f~")))
    out.append(("empty sequence alone", record(b"e", b"")))
    out.append(("empty name and sequence", record(b"", b"")))
    out.append(("empty sequences among others",
                filler(40) + record(b"e1", b"") + filler(40) + record(b"e2", b"") + record(b"e3", b"") + filler(16)))
    out.append(("one record", record(b"only", bases(31))))
    for n in (1, 15, 16, 17, 5000):
        out.append(("sequence of %d" % n, filler(24) + record(b"s%d" % n, bases(n, n), quals(n, n)) + filler(24)))
    out.append(("empty text", b""))
    # partial tails: nothing of them is consumed
    whole = record(b"tail", bases(12), quals(12), b"+tail")
    cuts = [len(b"@tail\n"), len(b"@tail\n") + 13, len(b"@tail\n") + 13 + 6]
    out.append(("1 line only", whole[:cuts[0]]))
    out.append(("2 lines only", whole[:cuts[1]]))
    out.append(("3 lines only", whole[:cuts[2]]))
    out.append(("4 lines, no final newline", whole[:-1]))
    for label, cut in (("L0", 3), ("L0's newline", cuts[0]), ("L1", cuts[0] + 5), ("L1's newline", cuts[1]),
                       ("L2", cuts[1] + 2), ("L2's newline", cuts[2]), ("L3", cuts[2] + 4),
                       ("L3 without its newline", len(whole) - 1), ("L3's newline", len(whole))):
        out.append(("text ends in " + label, filler(100) + whole[:cut]))
    return out


def irregular_kinds():
    """[(label, the bad record's bytes, the offset inside them that is reported)]"""
    return [
        ("CR before newline", b"@n\r\nACGT\r\n+\r\nIIII\r\n", 8),
        ("two-line sequence", b"@n\nACGT\nACGT\n+\nIIIIIIII\n", 8),
        ("> header", b">n\nACGT\n+\nIIII\n", 0),
        ("+ inside L1", b"@n\nAC+T\n+\nIIII\n", 5),
        ("@ inside L1", b"@n\nAC@T\n+\nIIII\n", 5),
        ("space inside L1", b"@n\nAC T\n+\nIIII\n", 5),
        ("0xFF inside L2", b"@n\nACGT\n+a\xffb\nIIII\n", 10),
        ("L3 one byte short", b"@n\nACGT\n+\nIII\n", 13),
        ("L3 one byte long", b"@n\nACGT\n+\nIIIII\n", 14),
        ("byte 128 in L3", b"@n\nACGT\n+\nII\x80I\n", 12),
        ("blank line between records", b"\n@n\nACGT\n+\nIIII\n", 0),
    ]


def irregular_kinds_by_label():
    return [(label, (bad, at)) for label, bad, at in irregular_kinds()]


def irregular_texts(T: int = TILE):
    """[(label, text, irregular_at)]: each kind in the first record, in a record that straddles a
    tile edge, and in the last complete record."""
    out = []
    for label, bad, at in irregular_kinds():
        out.append((label + ", first record", bad + filler(200), at))
        out.append((label + ", across a tile edge", filler(T - 4) + bad + filler(200), T - 4 + at))
        out.append((label + ", last record", filler(T + 300) + bad, T + 300 + at))
    return out
