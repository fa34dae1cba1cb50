"""klsh_diff_ksets and klsh_parse_clust: the first half of mode E on the device.

The reference for every parse is tests/clust_model.py (the strtol chain restated over bytes, tied
to libc's strtol by test_clust_model.py); the reference for the sets is KmerSet(engine, k) built
from the model's selection.  Each case first asserts from the model and the text alone that it
reaches what it names, then compares what the device gives.  T = option "diff_tile_bytes".
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import clust_model as cm
import row_state
from conftest import GOLDEN
from kmerlsh_amd import _native, extract
from row_state import LADDER_CALL, ladder_reference, options

import klsh_oracle_e as oe  # noqa: E402  (oracle/ is on sys.path via conftest)

sys.path.insert(0, GOLDEN)
import mode_e_inputs as mi  # noqa: E402

pytestmark = pytest.mark.gpu

NINES = b"9" * 18  # 10^18 - 1: the largest token of a regular text


@pytest.fixture(scope="module")
def T(engine):
    t = engine.get_option("diff_tile_bytes")
    assert t == 256 * 16
    return t


def prefix(n: int) -> bytes:
    """A regular text of exactly n >= 2 bytes that ends with a newline: "1 7" lines, then one line
    "0", blanks, newline."""
    body = b"1 7\n" * ((n - 2) // 4)
    rest = n - len(body)
    return body + b"0" + b" " * (rest - 2) + b"\n"


def parse_all(engine, text):
    """The text through paths 2, 0 and 1 (arrays included)."""
    return {p: _native.parse_clust(engine, text, p) for p in (2, 0, 1)}


def check_regular(engine, text, what):
    """A regular text: paths 0 and 2 run the kernels, every path gives the model's arrays, and
    paths 1 and 2 agree byte for byte."""
    assert cm.irregular_at(text) is None, what
    counts, offsets, ids = cm.parse_regular(text)
    got = parse_all(engine, text)
    for p, r in got.items():
        assert r["path_used"] == (1 if p == 1 else 0), (what, p)
        assert r["irregular_at"] is None, (what, p)
        assert r["n_lines"] == len(counts) and r["n_ids"] == len(ids), (what, p)
        assert r["counts"].tolist() == counts, (what, p)
        assert r["offsets"].tolist() == offsets, (what, p)
        assert r["ids"].tolist() == ids, (what, p)
    for k in ("counts", "offsets", "ids"):
        assert got[1][k].tobytes() == got[2][k].tobytes(), (what, k)
    return counts, offsets, ids


# ------------------------------------------------------------------ 1. tile edges --------------
def test_digit_runs_around_the_tile_edge(engine, T):
    """An 18-digit run starting at every offset from T - 18 to T + 1: ending on the edge, straddling
    it by every split, starting on it and after it; the run is an id and, in a second text, the
    line's declared count's neighbour."""
    for s in range(T - 18, T + 2):
        text = prefix(s - 2) + b"2 " + NINES + b" 5\n1 3\n"
        assert text[s - 1:s] == b" " and text[s:s + 18] == NINES and text[s + 18:s + 19] == b" "
        if T - 18 < s < T:
            assert s < T < s + 18  # straddles
        counts, _, ids = check_regular(engine, text, f"run at {s}")
        assert counts[-2:] == [2, 1] and ids[-3:] == [10**18 - 1, 5, 3]
    # shorter runs whose last digit is the tile's last byte, and whose first is its first
    for nd in (1, 2, 17):
        for s in (T - nd, T):
            text = prefix(s - 2) + b"1 " + b"123456789012345678"[:nd] + b"\n1 3"
            assert text[s:s + nd].isdigit() and not text[s - 1:s].isdigit()
            check_regular(engine, text, f"{nd} digits at {s}")


def test_newlines_and_empty_lines_on_the_edge(engine, T):
    cases = {
        "newline at T-1": prefix(T) + b"2 8 9\n",
        "newline at T": prefix(T + 1) + b"2 8 9\n",
        "empty lines at T-1, T, T+1": prefix(T - 1) + b"\n\n\n2 8 9\n",
        "blank-only line over the edge": prefix(T - 2) + b" \t\r \n2 8 9\n",
        "blank-only lines at the edge": prefix(T - 1) + b" \n\t\n2 8 9\n",
        "a count at T-1, its id at T+1": prefix(T - 1) + b"1 8\n",
        "a two-digit count over the edge": prefix(T - 1) + b"12 8\n",
    }
    assert cases["newline at T-1"][T - 1] == 10 and cases["newline at T"][T] == 10
    t = cases["empty lines at T-1, T, T+1"]
    assert t[T - 2:T + 2] == b"\n\n\n\n"
    t = cases["blank-only line over the edge"]
    assert t[T - 3] == 10 and t[T - 2:T + 2] == b" \t\r " and t[T + 2] == 10
    assert cases["a two-digit count over the edge"][T - 1:T + 1] == b"12"
    for what, text in cases.items():
        counts, _, _ = check_regular(engine, text, what)
        assert 0 in counts


def test_text_sizes(engine, T):
    """Texts of T - 1, T, T + 1 and 3T + 1 bytes, with and without a final newline; the empty
    text (0 lines), "\\n", one line."""
    for n in (T - 1, T, T + 1, 3 * T + 1):
        text = prefix(n)
        assert len(text) == n
        check_regular(engine, text, f"{n} bytes")
        text = prefix(n - 5) + b"2 9 4"
        assert len(text) == n and text[-1:] != b"\n"
        counts, _, ids = check_regular(engine, text, f"{n} bytes, no final newline")
        assert counts[-1] == 2 and ids[-2:] == [9, 4]
    for text, lines in ((b"", 0), (b"\n", 1), (b"3 1 2 3", 1), (b"3 1 2 3\n", 1), (b"7", 1),
                        (b"\n\n", 2), (b" ", 1), (b"0", 1)):
        assert len(cm.lines_of(text)) == lines
        counts, _, _ = check_regular(engine, text, repr(text))
        assert len(counts) == lines


# ------------------------------------------------------------------ 2. counts against tokens ---
def test_counts_against_tokens(engine, T):
    text = (b"3\t10\n"                      # declares more than it holds: two zeros
            b"2\t10\t20\t30\t40\n"          # declares fewer: 30 and 40 are ignored
            b"0\t5\n"                       # declares none
            b"4\n"                          # holds none: four zeros
            b"2 " + NINES + b" " + NINES + b"\n"
            b"0003 007 08 00000000000000009\n"
            b"2 \r\v\f 5  \t6\r\n"
            b"\r\n"
            b"1\r\n")
    counts, offsets, ids = check_regular(engine, text, "counts against tokens")
    assert counts == [3, 2, 0, 4, 2, 3, 2, 0, 1]
    assert ids == [10, 0, 0, 10, 20, 0, 0, 0, 0, 10**18 - 1, 10**18 - 1, 7, 8, 9, 5, 6, 0]
    # the same lines pushed over a tile edge, and many short lines: zero fills across tiles of
    # entries (256 a tile) and of lines
    long_text = prefix(T - 7) + text * 3 + b"300\n" + b"2 1\n" * 600
    counts, offsets, ids = check_regular(engine, long_text, "over the edge")
    assert offsets[-1] > 3 * 256 and len(counts) > 2 * 256 and ids.count(0) > 900


def test_declared_sum_limits(engine):
    """2^32 - 1 declared entries pass a size query on every path; 2^32, and 18-digit counts whose
    plain 64-bit sum would wrap to 0, are KLSH_E_RANGE on every path — the counts spread over
    lines so that nothing near that size is ever requested."""
    quarter = b"".join(b"%d\n" % (2**30) for _ in range(3))
    under = quarter + b"%d 7\n" % (2**30 - 1)
    m = cm.parse(under, want_ids=False)
    assert not m["range"] and m["entries"] == 2**32 - 1
    for p in (2, 0, 1):
        r = _native.parse_clust(engine, under, p, ids=False)
        assert (r["n_lines"], r["n_ids"], r["path_used"]) == (4, 2**32 - 1, 1 if p == 1 else 0)
    wrap = b"999999999999999999\n" * 18 + b"446744073709551634\n"
    assert sum(cm.parse(wrap, want_ids=False)["counts"]) == 2**64
    over = [quarter + b"%d 7\n" % (2**30), wrap, b"999999999999999999 1\n" * 40,
            b"4294967296\n", b"1 2\n" * 300 + b"4294967000\n"]
    for text in over:
        assert cm.irregular_at(text) is None and cm.parse(text, want_ids=False)["range"]
        for p in (2, 0, 1):
            with pytest.raises(_native.KlshError, match="KLSH_E_RANGE"):
                _native.parse_clust(engine, text, p)
    check_regular(engine, b"2 1 2\n", "after the refusals")


# ------------------------------------------------------------------ 3. irregular texts ---------
def check_irregular(engine, text, at, what):
    assert cm.irregular_at(text) == at, what
    m = cm.parse(text)
    assert not m["range"]
    with pytest.raises(_native.KlshError, match="KLSH_E_ARG"):
        _native.parse_clust(engine, text, 2)
    for p in (0, 1):
        r = _native.parse_clust(engine, text, p)
        assert r["path_used"] == 1 and r["irregular_at"] == at, (what, p)
        assert r["counts"].tolist() == m["counts"], (what, p)
        assert r["offsets"].tolist() == m["offsets"], (what, p)
        assert r["ids"].tolist() == m["ids"], (what, p)


def test_irregular_texts_take_the_host_parser(engine, T):
    base = prefix(T - 3) + b"2 5 6\n" * 3 + prefix(T) + b"1 9\n"
    assert len(base) > 2 * T and cm.irregular_at(base) is None
    n = len(base)
    for bad in (b"-", b"x", b"\x00", b"\xff", b"+", b"\x0e"):
        for at in (0, T - 1, T, n - 1):
            text = base[:at] + bad + base[at + 1:]
            check_irregular(engine, text, at, f"{bad!r} at {at}")
    # a 19-digit run that straddles the edge: its first digit's offset; 18 digits there are regular
    s = T - 10
    text = prefix(s - 2) + b"1 " + b"1234567890123456789" + b"\n1 3\n"
    assert text[s:s + 19].isdigit() and not text[s + 19:s + 20].isdigit() and s < T < s + 19
    check_irregular(engine, text, s, "19 digits over the edge")
    check_regular(engine, prefix(s - 2) + b"1 " + NINES + b"\n1 3\n", "18 digits over the edge")
    text = prefix(s - 2) + b"1 " + b"0" * 40 + b"\n"
    check_irregular(engine, text, s, "40 zeros")
    # two irregularities in different tiles, and a run against a byte: the smaller offset wins
    two = base[:100] + b"x" + base[101:T + 50] + b"-" + base[T + 51:]
    check_irregular(engine, two, 100, "two bytes")
    two = base[:T + 50] + b"-" + base[T + 51:]
    two = prefix(200) + b"1 " + b"7" * 25 + b"\n" + two
    check_irregular(engine, two, 202, "a run before a byte")
    two = base[:T + 50] + b"-" + base[T + 51:] + b"1 " + b"7" * 25 + b"\n"
    check_irregular(engine, two, T + 50, "a byte before a run")


# ------------------------------------------------------------------ 4. round trip --------------
def round_trip(engine, tmp_path, want, what):
    rows, off, ids = [np.asarray(x) for x in want[:3]]
    sizes = np.diff(off.astype(np.int64))
    for ignore_small in (0, 5):
        keep = sizes > ignore_small
        assert 0 < keep.sum() and (ignore_small == 0 or keep.sum() < keep.size), what
        clust = tmp_path / f"rt{ignore_small}.clust"
        engine.save_clusters(clust, None, ignore_small)
        text = clust.read_bytes()
        r = _native.parse_clust(engine, text, 2)
        want_ids = np.concatenate([ids[off[i]:off[i + 1]] for i in np.nonzero(keep)[0]])
        assert r["counts"].tolist() == sizes[keep].tolist(), what
        assert np.array_equal(r["offsets"], np.concatenate([[0], np.cumsum(sizes[keep])])), what
        assert np.array_equal(r["ids"], want_ids.astype(np.uint64)), what


def test_round_trip_of_saved_clusters(engine, oracle, tmp_path):
    """What klsh_save_clusters writes comes back through the kernels as klsh_result's offsets and
    ids of the kept rows: lists loaded directly (sizes around 5, one of 3000) and the lists six loop
    iterations make."""
    rng = np.random.default_rng(9)
    sizes = [6, 3, 9, 1, 12, 7, 5, 30, 3000, 2, 6] * 9
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ids = rng.permutation(int(off[-1])).astype(np.uint64) * np.uint64(1000003)
    rows = rng.normal(0, 1, size=(len(sizes), 8)).astype(np.float32)
    engine.load_rows(rows, off, ids)
    round_trip(engine, tmp_path, engine.result(), "direct lists")
    n, d = 40000, 16
    (rows, off, ids), want = ladder_reference(oracle, n, d, 1000000)
    min_sim, iters, seed, counter = LADDER_CALL
    engine.load_rows(rows, off, ids)
    trace, c, _ = engine.cluster(min_sim, iters, 1000000, seed, counter)
    assert np.array_equal(trace, want[3]) and c == want[4]
    round_trip(engine, tmp_path, want, "loop-made lists")


# ------------------------------------------------------------------ 5. the sets ----------------
def model_sets(dirpath, n1, n2, pval, size_thresh, kmap, name="clustering_result.txt"):
    """The model's selection for the files of a case: (ids A, ids B, k1, k2, kmers)."""
    path = os.path.join(dirpath, name)
    with open(path + ".clust", "rb") as f:
        text = f.read()
    m = cm.parse(text)
    d = n1 + n2
    vals = np.fromfile(path, np.float32)
    vals = vals[:len(m["counts"]) * d].reshape(len(m["counts"]), d)
    # (the oracle's test looks at a list's length alone: lists of the declared lengths)
    lists = [m["ids"][m["offsets"][c]:m["offsets"][c + 1]] for c in range(len(m["counts"]))]
    groups = oe.wrs_groups(vals, lists, n1, n2, pval, size_thresh)
    a, b, rows_a, rows_b = cm.select(m["counts"], m["offsets"], m["ids"], groups, kmap)
    kmers = np.fromfile(os.path.join(dirpath, "kmer_set.hex"), np.uint64, count=kmap)
    return dict(a=a, b=b, rows_a=rows_a, rows_b=rows_b, k1=kmers[rows_a], k2=kmers[rows_b],
                kmers=kmers, groups=np.asarray(groups), m=m, text=text)


def occupancy(kset, keys):
    """(table slots, the sorted occupied slots reached from `keys`, which keys are present)."""
    slots, n_slots = kset.find(keys)
    present = slots != np.uint64(2**64 - 1)
    return n_slots, np.unique(slots[present]), present


def check_sets(engine, got_a, got_b, st, ms, reads, k, vote):
    for got, keys, rows, what in ((got_a, ms["k1"], ms["rows_a"], "A"), (got_b, ms["k2"], ms["rows_b"], "B")):
        ref = _native.KmerSet(engine, keys)
        g, r = occupancy(got, ms["kmers"]), occupancy(ref, ms["kmers"])
        assert g[0] == r[0] == cm.kset_slots(len(rows)), what
        assert np.array_equal(g[1], r[1]), what
        assert np.array_equal(g[2], r[2]), what
        # unselected rows absent (the all-ones image is never held by either)
        sel = np.zeros(ms["kmers"].size, bool)
        sel[rows] = True
        sel &= ms["kmers"] != np.uint64(2**64 - 1)
        assert np.array_equal(g[2], sel), what
        if reads:
            gh, rh = got.check_reads(reads, k, vote), ref.check_reads(reads, k, vote)
            assert np.array_equal(gh[0], rh[0]) and np.array_equal(gh[1], rh[1]), what
        ref.close()
    assert (st["ids_a"], st["ids_b"]) == (len(ms["a"]), len(ms["b"]))
    assert (st["kmers_a"], st["kmers_b"]) == (len(ms["rows_a"]), len(ms["rows_b"]))
    assert st["clusters"] == len(ms["m"]["counts"]) and st["entries"] == len(ms["m"]["ids"])
    assert st["clusters_a"] == int((ms["groups"] == 1).sum())
    assert st["clusters_b"] == int((ms["groups"] == 2).sum())
    assert st["text_bytes"] == len(ms["text"])


@pytest.mark.parametrize("case", sorted(mi.CASES))
def test_sets_of_mode_e_cases(engine, tmp_path, case):
    c = mi.CASES[case]
    info = mi.write_case(str(tmp_path), case)
    with open(os.path.join(GOLDEN, "mode_e.json")) as f:
        fx = json.load(f)[case]
    ms = model_sets(str(tmp_path), c["n1"], c["n2"], c["pval"], c["size_thresh"], info["kmap"])
    assert [len(ms["a"]), len(ms["b"])] == fx["differential"] and min(fx["differential"]) > 0
    reads = [s for _, s, _ in oe.read_fastq(os.path.join(str(tmp_path), info["samples1"][1]))][:200]
    reads += [s for _, s, _ in oe.read_fastq(os.path.join(str(tmp_path), info["samples2"][0]))][:200]
    a, b, st = extract.differential_ksets(
        engine, c["n1"], c["n2"], c["pval"], c["size_thresh"], info["kmap"],
        os.path.join(str(tmp_path), "clustering_result.txt"), os.path.join(str(tmp_path), "kmer_set.hex"))
    assert st["parse_path"] == 0 and [st["ids_a"], st["ids_b"]] == fx["differential"]
    check_sets(engine, a, b, st, ms, reads, c["k"], c["vote"])
    hits = a.check_reads(reads, c["k"], c["vote"])[0]
    assert hits.max() > 0
    a.close()
    b.close()


N1 = N2 = 4
SIZE_THRESH = 3
PVAL = 0.01
ROW_A = [10.0, 10.5, 9.5, 10.25, 1.0, 1.5, 0.5, 1.25]   # first half above the second: group 1
ROW_B = ROW_A[4:] + ROW_A[:4]                           # group 2
ROW_0 = [1.0, 2.0, 3.0, 4.0, 1.0, 2.0, 3.0, 4.0]        # neither


def chunks(ids, size):
    out = [ids[i:i + size] for i in range(0, len(ids), size)]
    if len(out) > 1 and len(out[-1]) <= SIZE_THRESH:  # (a cluster that small would not be tested)
        last = out.pop()
        out[-1] = out[-1] + last
    return out


def write_constructed(dirpath, na, nb, irregular=False):
    """Files whose selection is na rows for A and nb rows for B (see the test below).  Returns
    the kmap."""
    kmap = na + nb + 50
    spare = list(range(na + nb, kmap))  # rows nothing may select
    lines, rows = [], []

    def cluster(row, declared, ids):
        lines.append(b"%d" % declared + b"".join(b"\t%d" % i for i in ids) + b"\n")
        rows.append(row)

    a_ids = list(range(1, na + 1))
    for part in chunks(a_ids, 37):
        cluster(ROW_A, len(part), part)
    if na:  # ids at or above kmap, in a group-1 cluster
        cluster(ROW_A, 5, [kmap, kmap + 7, 10**18 - 1, 1, 2])
    if nb:
        b_rows = list(range(na + 1, na + nb))           # nb - 1 rows; row 0 comes from a zero fill
        both = a_ids[:5]                                 # in both groups: A wins
        parts = chunks(b_rows + both, 41)
        for i, part in enumerate(parts):
            if i == 0:  # the short line: declares one more than it holds, the fill is id 0
                cluster(ROW_B, len(part) + 1, part)
            elif i == 1:  # declares fewer than it holds: the ignored tokens select nothing
                cluster(ROW_B, len(part), part + spare[:3])
            else:
                cluster(ROW_B, len(part), part)
        cluster(ROW_B, 4, [kmap + 1, 2 * kmap, na + 1 if nb > 1 else kmap, kmap])
    # clusters of exactly size_thresh members are not tested, whatever their rows say
    cluster(ROW_A, SIZE_THRESH, spare[3:3 + SIZE_THRESH])
    cluster(ROW_B, SIZE_THRESH, spare[6:6 + SIZE_THRESH])
    cluster(ROW_B, SIZE_THRESH, [0, 0, 0] if nb == 0 else spare[9:12])
    cluster(ROW_0, 20, spare[12:32])   # tested, in neither group
    cluster(ROW_A, 0, [])              # an empty cluster
    if irregular:
        lines[0] = lines[0].replace(b"\t", b"\t+", 1)
    with open(os.path.join(dirpath, "cr"), "wb") as f:
        f.write(np.asarray(rows, np.float32).tobytes())
    with open(os.path.join(dirpath, "cr.clust"), "wb") as f:
        f.write(b"".join(lines))
    kmers = (np.arange(1, kmap + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    assert np.unique(kmers).size == kmap and (kmers != np.uint64(2**64 - 1)).all()
    kmers.tofile(os.path.join(dirpath, "kmer_set.hex"))
    return kmap


def run_constructed(engine, dirpath, kmap):
    return _native.diff_ksets(engine, os.path.join(dirpath, "cr"), os.path.join(dirpath, "kmer_set.hex"),
                              kmap, N1, N2, PVAL, SIZE_THRESH)


@pytest.mark.parametrize("na,nb", [(512, 513), (513, 1025), (1025, 0), (0, 512), (1024, 1024)])
def test_sets_constructed(engine, tmp_path, na, nb):
    """Selections of exactly na and nb rows, across the capacity rule's steps (512 -> 1024 slots,
    513 -> 2048, 1025 -> 4096): ids in both groups (A wins), ids at or above kmap, a group-2 short
    line whose zero fill selects row 0, lines that hold more than they declare, clusters of exactly
    size_thresh members, an empty cluster, an empty group."""
    kmap = write_constructed(str(tmp_path), na, nb)
    ms = model_sets(str(tmp_path), N1, N2, PVAL, SIZE_THRESH, kmap, "cr")
    assert cm.irregular_at(ms["text"]) is None
    assert (len(ms["rows_a"]), len(ms["rows_b"])) == (na, nb)
    assert ((ms["groups"] == 1).any(), (ms["groups"] == 2).any()) == (na > 0, nb > 0)
    if na and nb:
        assert set(ms["a"]) & set(ms["b"]) and len(ms["b"]) > nb  # ids in both groups
    if nb:
        assert 0 in ms["rows_b"]  # and no line holds a token 0: the fill alone selects row 0
        assert all(0 not in cm.tokens_of(ln)[1:] for ln in cm.lines_of(ms["text"]))
    assert max(ms["m"]["ids"]) >= kmap
    counts = ms["m"]["counts"]
    assert counts.count(SIZE_THRESH) >= 3 and (ms["groups"][np.array(counts) == SIZE_THRESH] == 0).all()
    assert {cm.kset_slots(na), cm.kset_slots(nb)} <= {1024, 2048, 4096}
    a, b, st = run_constructed(engine, str(tmp_path), kmap)
    assert st["parse_path"] == 0 and st["tested"] == sum(c > SIZE_THRESH for c in counts)
    check_sets(engine, a, b, st, ms, None, 0, 0.0)
    a.close()
    b.close()


def test_sets_from_an_irregular_text(engine, tmp_path):
    """One '+' in the text: the whole file takes the host parser, and the sets are the model's."""
    kmap = write_constructed(str(tmp_path), 600, 300, irregular=True)
    ms = model_sets(str(tmp_path), N1, N2, PVAL, SIZE_THRESH, kmap, "cr")
    assert cm.irregular_at(ms["text"]) is not None and (len(ms["rows_a"]), len(ms["rows_b"])) == (600, 300)
    a, b, st = run_constructed(engine, str(tmp_path), kmap)
    assert st["parse_path"] == 1
    check_sets(engine, a, b, st, ms, None, 0, 0.0)
    a.close()
    b.close()


# ------------------------------------------------------------------ 6. chunks and grids --------
COUNTERS = ("clusters", "entries", "text_bytes", "tokens", "tested", "clusters_a", "clusters_b",
            "ids_a", "ids_b", "kmers_a", "kmers_b", "parse_path")


def test_chunks_and_grids_change_nothing(engine, tmp_path, T):
    """A text of more than 7 tiles and a kmap of two dozen insert trips at one workgroup: upload
    chunks of 32, T - 1, T + 1 and the text's length, launches of 1 to 3 workgroups — the same
    statistics and the same tables as the default run, which are the model's."""
    kmap = write_constructed(str(tmp_path), 3200, 3100)
    ms = model_sets(str(tmp_path), N1, N2, PVAL, SIZE_THRESH, kmap, "cr")
    L = len(ms["text"])
    assert L >= 7 * T and kmap > 20 * 256 and len(ms["m"]["ids"]) > 20 * 256
    a, b, st = run_constructed(engine, str(tmp_path), kmap)
    check_sets(engine, a, b, st, ms, None, 0, 0.0)
    base = (occupancy(a, ms["kmers"]), occupancy(b, ms["kmers"]), [st[k] for k in COUNTERS])
    a.close()
    b.close()
    runs = [dict(diff_chunk_bytes=c) for c in (32, T - 1, T + 1, L)]
    runs += [dict(grid_cap=g) for g in (1, 2, 3)] + [dict(grid_cap=2, diff_chunk_bytes=4097)]
    for kv in runs:
        with options(engine, **kv):
            a, b, st = run_constructed(engine, str(tmp_path), kmap)
            r = _native.parse_clust(engine, ms["text"], 2)
        got = (occupancy(a, ms["kmers"]), occupancy(b, ms["kmers"]), [st[k] for k in COUNTERS])
        for x, y in zip(base[:2], got[:2]):
            assert x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]), kv
        assert base[2] == got[2], kv
        assert r["ids"].tolist() == ms["m"]["ids"] and r["counts"].tolist() == ms["m"]["counts"], kv
        a.close()
        b.close()
    assert engine.get_option("diff_chunk_bytes") == 0 and engine.get_option("grid_cap") == 0
    for bad in (31, -1):
        with pytest.raises(_native.KlshError, match="KLSH_E_ARG"):
            engine.set_option("diff_chunk_bytes", bad)
    with pytest.raises(_native.KlshError, match="KLSH_E_ARG"):
        engine.set_option("diff_tile_bytes", 4096)


# ------------------------------------------------------------------ 7. state and refusals ------
def raw_call(engine, clust, kmers, kmap, n1=N1, n2=N2, stats="ok", null=None):
    """klsh_diff_ksets through ctypes: (return code, set A, set B) with the out-pointers preset."""
    lib = engine._lib
    a, b = ctypes.c_void_p(1), ctypes.c_void_p(1)
    st = _native.KlshDiffStats()
    if stats == "wrong size":
        st.struct_size -= 8
    args = [engine._ctx, os.fsencode(clust), os.fsencode(kmers), kmap, n1, n2, ctypes.c_float(PVAL),
            SIZE_THRESH, ctypes.byref(a), ctypes.byref(b), None if stats is None else ctypes.byref(st)]
    if null is not None:
        args[null] = None
    rc = lib.klsh_diff_ksets(*args)
    return rc, a.value, b.value


def test_state_untouched_and_refusals(engine, tmp_path):
    """A loaded, clustered context reads the same bytes from klsh_result and klsh_row_state before
    and after the calls; every refusal leaves both out-pointers NULL and the context usable."""
    rows, off, ids = row_state.ladder(6000, 16)
    engine.load_rows(rows, off, ids)
    engine.cluster(0.8, 2, 1000000, 777, 3)
    before, state_before = engine.result(), engine.row_state()
    d = str(tmp_path)
    kmap = write_constructed(d, 300, 200)
    cr, ks = os.path.join(d, "cr"), os.path.join(d, "kmer_set.hex")
    good = raw_call(engine, cr, ks, kmap)
    assert good[0] == 0 and good[1] and good[2]
    for h in good[1:]:
        engine._lib.klsh_kset_destroy(h)

    os.mkdir(os.path.join(d, "r"))
    # a rows file of 4 clusters and a text that declares 2^32 entries; three rows against the
    # good text's lines
    np.zeros((4, N1 + N2), np.float32).tofile(os.path.join(d, "r", "cr"))
    with open(os.path.join(d, "r", "cr.clust"), "wb") as f:
        f.write(b"".join(b"%d 1\n" % (2**30) for _ in range(4)))
    with open(os.path.join(d, "cr3"), "wb") as f:
        f.write(open(cr, "rb").read()[:3 * 4 * (N1 + N2)])
    os.link(cr + ".clust", os.path.join(d, "cr3.clust"))
    E_ARG, E_RANGE = -1, -6
    refusals = [
        ("null ctx", E_ARG, dict(null=0)), ("null clust_path", E_ARG, dict(null=1)),
        ("null kmer_set_path", E_ARG, dict(null=2)), ("null set_b", E_ARG, dict(null=9)),
        ("n1 < 0", E_ARG, dict(n1=-1)), ("n2 < 0", E_ARG, dict(n2=-1)),
        ("struct_size", E_ARG, dict(stats="wrong size")),
        ("no rows file", E_ARG, dict(clust=os.path.join(d, "missing"))),
        ("no text", E_ARG, dict(clust=ks)),  # kmer_set.hex.clust does not exist
        ("no kmer_set", E_ARG, dict(kmers=os.path.join(d, "missing.hex"))),
        ("a directory", E_ARG, dict(kmers=d)),
        ("short kmer_set", E_ARG, dict(kmap=kmap + 1)),
        ("line count", E_ARG, dict(clust=os.path.join(d, "cr3"))),
        ("2^32 entries", E_RANGE, dict(clust=os.path.join(d, "r", "cr"))),
    ]
    for what, code, kv in refusals:
        args = dict(clust=cr, kmers=ks, kmap=kmap)
        args.update(kv)
        rc, a, b = raw_call(engine, **args)
        assert rc == code, what
        if kv.get("null") != 9:
            assert a is None, what
        assert b is None or kv.get("null") == 9, what
        assert engine._lib.klsh_last_error(), what
        rc, a, b = raw_call(engine, cr, ks, kmap, stats=None)  # a good call follows every refusal
        assert rc == 0 and a and b, what
        engine._lib.klsh_kset_destroy(a)
        engine._lib.klsh_kset_destroy(b)

    after, state_after = engine.result(), engine.row_state()
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(before, after))
    assert row_state.same_state(state_before, state_after)
    row_state.check_state(state_after, after[0], after[1], "after the calls")
