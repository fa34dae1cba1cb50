"""The device FASTQ parser alone (klsh_parse_fastq): the kernels (path 0) against
the grammar's model (tests/fastq_model.py, which test_fastq_model.py holds to the oracle's reader)
AND against the host reader over the same bytes (path 1), field by field.  The texts are built
from the parser's tile size so that every edge is chosen: newlines and line starts around a tile
edge and at every byte of a lane's 16, records over several tiles, every irregular kind in the
first record, across a tile edge and in the last complete record.  Everything runs at grid_cap 1,
2 and 3 too, where every workgroup makes several trips.
"""
import numpy as np
import pytest

import fastq_model as fm
from kmerlsh_amd import _native

pytestmark = pytest.mark.gpu

GRIDS = (0, 1, 2, 3)
_host = {}


@pytest.fixture(scope="module")
def T(engine):
    t = engine.get_option("fastq_tile")
    assert t == fm.TILE  # (the model test's edges are the kernels')
    return t


@pytest.fixture(params=GRIDS)
def eng(request, engine):
    engine.set_option("grid_cap", request.param)
    yield engine
    engine.set_option("grid_cap", 0)


def host(engine, text):
    """path 1, once per text"""
    if text not in _host:
        _host[text] = _native.parse_fastq(engine, text, path=1, seq_capacity=len(text))
    return _host[text]


def check_regular(engine, label, text):
    m = fm.parse(text)
    d = _native.parse_fastq(engine, text, path=0, seq_capacity=len(text))
    n = m["n"]
    off, seq = fm.seq_arrays(m["records"])
    assert d["irregular_at"] is None, label
    assert d["n_records"] == n and d["consumed"] == m["consumed"], label
    if n:
        assert d["line_starts"].tolist() == m["line_starts"], label
    assert d["seq_off"].tolist() == off and d["seq"] == seq, label
    # the host reader over the same bytes: the same records, and at most the one it makes of a tail
    h = host(engine, text)
    assert h["n_records"] in (n, n + 1), label
    assert h["seq_off"][:n + 1].tolist() == off and h["seq"][:off[-1]] == seq, label
    if n:
        assert h["line_starts"][:4 * n + 1].tolist() == d["line_starts"].tolist(), label
    if m["consumed"] == len(text):
        assert h["n_records"] == n and h["consumed"] == d["consumed"], label


def test_regular_texts(eng, T):
    texts = fm.regular_texts(T)
    assert max(len(t) for _, t in texts) < (1 << 20)
    for label, text in texts:
        check_regular(eng, label, text)


def test_irregular_texts(eng, T):
    for label, text, at in fm.irregular_texts(T):
        m = fm.parse(text)
        d = _native.parse_fastq(eng, text, path=0, seq_capacity=len(text))
        assert d["irregular_at"] == at == m["irregular_at"], label
        assert d["n_records"] == 0 and d["consumed"] == 0, label
        # what the reader makes of the records before the bad one is the model's
        h = host(eng, text)
        off, seq = fm.seq_arrays(m["records"])
        fb = m["first_bad"]
        assert h["n_records"] >= fb, label
        assert h["seq_off"][:fb + 1].tolist() == off and h["seq"][:off[-1]] == seq, label


def test_several_irregularities_report_the_smallest(eng, T):
    """Offenders in many tiles and lanes: the smallest offset wins whichever workgroup finds it."""
    bad = dict(fm.irregular_kinds_by_label())
    parts, want = [fm.filler(3 * T + 111)], None
    for i, label in enumerate(("L3 one byte long", "space inside L1", "byte 128 in L3", "0xFF inside L2")):
        rec, at = bad[label]
        if want is None:
            want = len(b"".join(parts)) + at
        parts += [rec, fm.filler(2 * T + 40 + i)]
    text = b"".join(parts)
    d = _native.parse_fastq(eng, text, path=0, seq_capacity=len(text))
    assert d["irregular_at"] == want == fm.parse(text)["irregular_at"]
    # a length mismatch and a bad byte in one record: whichever comes first
    for rec, at in ((b"@n\nAC T\n+\nII\n", 5), (b"@n\nACGT\n+\nI\x80\n", 11), (b"@n\nACGT\n+\n\x80IIII\n", 10)):
        text = fm.filler(T - 6) + rec + fm.filler(100)
        d = _native.parse_fastq(eng, text, path=0, seq_capacity=len(text))
        assert d["irregular_at"] == T - 6 + at == fm.parse(text)["irregular_at"], rec


def test_random_records_over_many_tiles(eng, T):
    """Random regular records from the whole of each line's class, 40 tiles of them, with a
    partial record behind."""
    rng = np.random.default_rng(161)
    l0 = np.array([c for c in range(256) if c != 10], np.uint8)
    l1 = np.array([c for c in range(33, 127) if c not in (62, 43, 64)], np.uint8)
    l2 = np.array([c for c in range(128) if c != 10], np.uint8)
    l3 = np.arange(33, 128, dtype=np.uint8)
    draw = lambda a, n: a[rng.integers(0, a.size, size=n)].tobytes()
    recs = []
    while sum(map(len, recs)) < 40 * T:
        n = int(rng.integers(0, 300))
        recs.append(fm.record(draw(l0, int(rng.integers(0, 40))), draw(l1, n), draw(l3, n),
                              b"+" + draw(l2, int(rng.integers(0, 8)))))
    text = b"".join(recs) + recs[0][:-3]
    check_regular(eng, "random", text)


def test_size_query_and_capacity(engine):
    text = fm.filler(500) + b"@partial\nAC"
    q = _native.parse_fastq(engine, text, path=0)  # NULL arrays first, then arrays of those sizes
    m = fm.parse(text)
    assert q["n_records"] == m["n"] and q["seq"] == fm.seq_arrays(m["records"])[1]
    assert _native.parse_fastq(engine, text, path=1)["n_records"] == m["n"] + 1
    for path in (0, 1):
        with pytest.raises(_native.KlshError, match="KLSH_E_RANGE"):
            _native.parse_fastq(engine, text, path=path, seq_capacity=len(q["seq"]) - 1)
    with pytest.raises(_native.KlshError, match="KLSH_E_ARG"):
        _native.parse_fastq(engine, text, path=2)
    assert _native.parse_fastq(engine, text, path=0, seq_capacity=len(q["seq"]))["seq"] == q["seq"]


def test_trailing_lines_are_no_record(eng, T):
    """n complete records and one, two or three lines more: exactly n records, consumed exactly
    their end (a parser that counts one record too many would read line starts nobody wrote)."""
    head = fm.filler(T + 321)
    n = fm.parse(head)["n"]
    tail = fm.record(b"tail", fm.bases(12), fm.quals(12), b"+t")
    lines = tail.split(b"\n")
    for extra in (1, 2, 3):
        text = head + b"\n".join(lines[:extra]) + b"\n"
        d = _native.parse_fastq(eng, text, path=0, seq_capacity=len(text))
        assert d["n_records"] == n and d["consumed"] == len(head), extra
        assert d["irregular_at"] is None and len(d["line_starts"]) == 4 * n + 1, extra
        assert d["seq_off"].size == n + 1 and len(d["seq"]) == int(d["seq_off"][-1]), extra
