"""The regular FASTQ grammar (tests/fastq_model.py) against the oracle's restatement
of the reference's kseq reader (oracle/klsh_oracle_e.py::read_fastq): what the model calls the
complete regular records of a chunk is what the reader reads from those bytes, so a device parser
that equals the model equals the reader.  No GPU.
"""
import numpy as np

import fastq_model as fm
import klsh_oracle_e as oe

T = fm.TILE


def reader(tmp_path, text):
    p = tmp_path / "t.fastq"
    p.write_bytes(text)
    return oe.read_fastq(str(p))


def test_regular_prefix_is_what_the_reader_reads(tmp_path):
    """For every regular text, read_fastq on text[:consumed] gives the model's records."""
    texts = fm.regular_texts(T)
    assert len(texts) > 100
    for label, text in texts:
        m = fm.parse(text)
        assert m["irregular_at"] is None, label
        assert m["consumed"] == m["line_starts"][-1] <= len(text), label
        assert len(m["records"]) == m["n"], label
        assert reader(tmp_path, text[:m["consumed"]]) == m["records"], label


def test_irregular_prefix_still_agrees(tmp_path):
    """For every irregular text, the records before the first bad one are the reader's of those
    bytes, the reported offset lies inside the first bad record and is the builder's."""
    for label, text, at in fm.irregular_texts(T):
        m = fm.parse(text)
        assert m["irregular_at"] == at, label
        assert m["consumed"] == 0 and m["first_bad"] is not None, label
        s = m["line_starts"]
        lo = s[4 * m["first_bad"]]
        assert lo <= at < s[4 * m["first_bad"] + 4], label
        assert len(m["records"]) == m["first_bad"], label
        assert reader(tmp_path, text[:lo]) == m["records"], label


def test_random_regular_records(tmp_path):
    """Random regular records from the whole of each line's class."""
    rng = np.random.default_rng(16)
    l0 = bytes(c for c in range(256) if c != 10)
    l1 = bytes(c for c in range(33, 127) if c not in (62, 43, 64))
    l2 = bytes(c for c in range(128) if c != 10)
    l3 = bytes(range(33, 128))

    def draw(alphabet, n):
        a = np.frombuffer(alphabet, np.uint8)
        return a[rng.integers(0, a.size, size=n)].tobytes()

    recs = []
    for _ in range(300):
        n = int(rng.integers(0, 40))
        recs.append(fm.record(draw(l0, int(rng.integers(0, 20))), draw(l1, n), draw(l3, n),
                              b"+" + draw(l2, int(rng.integers(0, 6)))))
    text = b"".join(recs)
    m = fm.parse(text)
    assert m["irregular_at"] is None and m["n"] == 300 and m["consumed"] == len(text)
    assert reader(tmp_path, text) == m["records"]
    # and with a partial record behind them
    m2 = fm.parse(text + recs[0][:-1])
    assert m2["consumed"] == len(text) and m2["records"] == m["records"]


def test_builders_deliver_their_edges():
    for kind in range(4):
        for pos in (T - 1, T, T + 1):
            text = fm.newline_at(pos, kind)
            m = fm.parse(text)
            nl = [s - 1 for s in m["line_starts"][1:]]
            assert pos in nl and nl.index(pos) % 4 == kind
    for shift in range(16):
        for kind in range(4):
            m = fm.parse(fm.line_start_at(T + 160 + shift, kind))
            s = m["line_starts"]
            assert (T + 160 + shift) in s and s.index(T + 160 + shift) % 4 == kind
            assert (T + 160 + shift) % 16 == shift
    by = dict(fm.regular_texts(T))
    m = fm.parse(by["record over tiles"])
    r = next(i for i in range(m["n"]) if m["line_starts"][4 * i + 4] - m["line_starts"][4 * i] > 2 * T)
    s = m["line_starts"][4 * r:4 * r + 5]
    assert s[0] // T == 0 and s[1] // T == 1 and s[2] // T == 2 and s[3] // T == 2 and s[4] // T >= 3
    for n in (1, 15, 16, 17, 5000):
        assert n in [len(q) for _, q, _ in fm.parse(by["sequence of %d" % n])["records"]]
    assert fm.parse(by["L3 begins with @"])["records"][1][2][:1] == b"@"
    assert fm.parse(by["L3 begins with +"])["records"][1][2][:1] == b"+"
    for label in ("1 line only", "2 lines only", "3 lines only", "4 lines, no final newline", "empty text"):
        m = fm.parse(by[label])
        assert m["n"] == 0 and m["consumed"] == 0 and m["irregular_at"] is None, label
    for label, text in fm.regular_texts(T):
        if label.startswith("text ends in "):
            m = fm.parse(text)
            want = len(text) if label.endswith("L3's newline") else 100
            assert m["consumed"] == want, label
    assert [len(r[1]) for r in fm.parse(by["empty sequences among others"])["records"]].count(0) == 3
    # the irregular kinds sit where their labels say
    for label, text, at in fm.irregular_texts(T):
        if "across a tile edge" in label:
            m = fm.parse(text)
            s = m["line_starts"]
            assert s[4 * m["first_bad"]] < T <= s[4 * m["first_bad"] + 4], label
        if "last record" in label:
            m = fm.parse(text)
            assert m["first_bad"] == m["n"] - 1, label
        if "first record" in label:
            assert fm.parse(text)["first_bad"] == 0, label
