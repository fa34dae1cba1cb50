"""The k-mer table of modes E, B and K at chosen slots ("What chance did not reach").

Every other key in the suite is a random or genome-derived k-mer: its chain is a few slots long
and almost never wraps from the table's last slot to slot 0.  Here the keys are searched for by
their home slot (tests/ktab_model.py): hundreds of keys homed on the table's last slots, so that
one chain runs across the wrap for ~500 slots; a 400-slot chain in the middle; five keys alone on
the first and last lanes of a wave.  Mode E's table is read back slot by slot (klsh_kset_find /
KmerSet.find) and compared with a linear-probing model, whose set of occupied slots no insertion
order changes; modes K and B are compared through their listings, first-appearance lists and
files, and prove the table sizes they ran in from their counters.  Also here: the vote kernel's
2048-position LDS window with set k-mers planted on both sides of every window edge, and the
float vote at exact ties (hits / positions == vote must not extract).

Each case asserts what it reaches from the model or the oracle alone (CPU tests, and again at the
head of the GPU test) before any device output is compared.
"""
import functools
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN

import klsh_oracle_b as ob  # noqa: E402
import klsh_oracle_e as oe  # noqa: E402

sys.path.insert(0, GOLDEN)
import kcount_inputs as kc  # noqa: E402
import kmc_inputs as ki  # noqa: E402
import mode_e_inputs as mi  # noqa: E402

import ktab_model as tm  # noqa: E402
from row_state import options  # noqa: E402

U = np.uint64
EMPTY = tm.EMPTY
KS = (32, 21)
EDGE_HOMES = (0, 63, 64, 127, 1023)  # first / last lane of waves 0 and 1, the table's last slot
FILES = ("kmer_set.hex", "kmer_count.bin", "kmer_count.log")


def frozen(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------ the key sets, once each ---
@functools.lru_cache(maxsize=None)
def wrap_keys(k, enc):
    """812 keys homed on slots 1020..1023 of 1024: [:512] the members, [512:] 300 absent ones."""
    return frozen(tm.search(k, enc, 812, seed=1000 + k, slots=1024, homes=range(1020, 1024)))


@functools.lru_cache(maxsize=None)
def inside_keys(k):
    """300 absent keys whose home slot lies inside the wrapped chain (0..500)."""
    return frozen(tm.search(k, "image", 300, seed=2000 + k, slots=1024, homes=range(0, 501)))


@functools.lru_cache(maxsize=None)
def low_keys(k, enc, bits, n):
    """n keys whose hash has its low `bits` bits all ones."""
    return frozen(tm.search(k, enc, n, seed=3000 + k + bits, low_bits=bits))


@functools.lru_cache(maxsize=None)
def chain_keys(k):
    """500 keys homed at slot 100 of 1024: [:400] the members, [400:] 100 absent ones."""
    return frozen(tm.search(k, "image", 500, seed=4000 + k, slots=1024, homes=(100,)))


@functools.lru_cache(maxsize=None)
def edge_keys(k, enc):
    return frozen(tm.search_homes_in_order(k, enc, EDGE_HOMES, 1024, seed=5000 + k))


# ------------------------------------------------------------------------ the helper itself ---
def scalar_hash(x):
    m = (1 << 64) - 1
    x ^= x >> 33
    x = x * 0xFF51AFD7ED558CCD & m
    x ^= x >> 33
    x = x * 0xC4CEB9FE1A85EC53 & m
    return x ^ (x >> 33)


def test_hash_matches_scalar_integers():
    rng = np.random.default_rng(1)
    keys = np.concatenate([rng.integers(0, 1 << 63, 500, dtype=np.uint64) << U(1),
                           np.array([0, 1, EMPTY, EMPTY - 1, 1 << 63], np.uint64)])
    assert tm.ktab_hash(keys).tolist() == [scalar_hash(int(x)) for x in keys]
    assert int(tm.ktab_hash(np.array([0], np.uint64))[0]) == 0  # key 0: home slot 0 everywhere


@pytest.mark.parametrize("k", [1, 4, 5, 11, 16, 17, 21, 31, 32])
def test_canonical_forms_match_scalar_oracles(k):
    """The vectorised encodings against the scalar ones of the fixtures and the oracle."""
    rng = np.random.default_rng(k)
    v = (rng.integers(0, 1 << 63, 300, dtype=np.uint64) << U(1) |
         rng.integers(0, 2, 300, dtype=np.uint64)) & tm.kmer_mask(k)
    v[:3] = [0, int(tm.kmer_mask(k)), 1]  # all-A, all-T
    ints = [int(x) for x in v]
    assert tm.revcomp(v, k).tolist() == [mi.twin(x, k) for x in ints]
    assert tm.image_rep(v, k).tolist() == [mi.rep(x, k) for x in ints]
    assert tm.image_rep(v, k).tolist() == [ob.canonical(x, k) for x in ints]
    assert tm.value_image(v, k).tolist() == [ob.image(x, k) for x in ints]
    strings = [tm.value_string(x, k) for x in ints]
    assert [ki.kmer_value(s) for s in strings] == ints
    assert tm.kmc_canonical(v, k).tolist() == [
        min(ki.kmer_value(s), ki.kmer_value(mi.revcomp(s))) for s in strings]
    assert [mi.fwd_value(tm.image_string(x, k), k) for x in ints] == ints
    # a canonical form is its own canonical form, and never all ones
    for enc in ("image", "kmc"):
        c = tm.canonical(v, k, enc)
        assert np.array_equal(tm.canonical(c, k, enc), c) and (c != U(EMPTY)).all()


def test_model_is_plain_linear_probing_and_its_set_ignores_the_order():
    rng = np.random.default_rng(3)
    for slots, n in ((1024, 512), (1024, 100), (2048, 1000)):
        keys = np.unique(rng.integers(0, 1 << 62, n, dtype=np.uint64))
        if slots == 2048:  # most of them into one cluster
            keys = np.concatenate([keys[:200], low_keys(32, "image", 11, 513)])
        tab = {}
        for key, h in zip(keys.tolist(), (tm.ktab_hash(keys) & U(slots - 1)).tolist()):
            while h in tab:
                h = (h + 1) & (slots - 1)
            tab[h] = key
        m = tm.Model(keys, slots)
        assert {int(s): int(key) for s, key in zip(m.slot_of, m.keys)} == tab
        occ, home, wrapped, longest = tm.model(rng.permutation(keys), slots)
        assert occ.tolist() == sorted(tab) and wrapped == m.wrapped
        assert m.in_cluster(m.keys, m.slot_of).all()
        free = sorted(set(range(slots)) - set(tab))
        for h, e in zip(m.home[:50].tolist(), m.cluster_end(m.home[:50]).tolist()):
            assert e == next((f for f in free if f >= h), free[0])


def test_search_gives_what_it_was_asked_for():
    for k, enc in ((32, "image"), (21, "image"), (32, "kmc"), (21, "kmc")):
        w = wrap_keys(k, enc)
        assert len(set(w.tolist())) == 812 and (w <= tm.kmer_mask(k)).all()
        assert np.array_equal(tm.canonical(w, k, enc), w)
        assert set((tm.ktab_hash(w) & U(1023)).tolist()) <= {1020, 1021, 1022, 1023}
        lo = low_keys(k, enc, 12, 1200)
        assert len(set(lo.tolist())) == 1200 and (lo <= tm.kmer_mask(k)).all()
        assert ((tm.ktab_hash(lo) & U(4095)) == U(4095)).all()
        assert (tm.ktab_hash(edge_keys(k, enc)) & U(1023)).tolist() == list(EDGE_HOMES)


# ================================================================================== mode E ===
E_CASES = ("wrap", "one_more", "dups", "chain", "edges")


@functools.lru_cache(maxsize=None)
def e_case(name, k):
    """(the entries klsh_kset_create gets, absent keys, the model of the table they make), with
    the case's reach asserted from the model alone."""
    none = np.zeros(0, np.uint64)
    if name == "wrap":  # exactly half load, one chain across the wrap
        w = wrap_keys(k, "image")
        entries, absent = w[:512], np.concatenate([w[512:], inside_keys(k)])
        m = tm.Model(entries, tm.slots_for(len(entries)))
        assert m.slots == 1024 and m.wrapped >= 500 and m.longest >= 500
        # every absent key's lookup walks the chain to its end: across the wrap from the last
        # slots, or from a home inside the chain
        home = (tm.ktab_hash(absent) & U(1023)).astype(np.int64)
        end = m.cluster_end(home)
        assert (end[:300] < home[:300]).all() and (m.absent_probes(absent[:300]) >= 500).all()
        assert m.occupied[home[300:]].all() and (end[300:] > home[300:]).all()
    elif name == "one_more":  # 513 entries: the next table size
        entries, absent = low_keys(k, "image", 11, 513), none
        m = tm.Model(entries, tm.slots_for(len(entries)))
        assert m.slots == 2048 and (m.home == 2047).all() and m.wrapped == 512
    elif name == "dups":  # every key four times, the empty mark and key 0 among them
        # 511 keys: with the two special entries n = 2046 <= 2048, so the table has 4096 slots
        d = low_keys(k, "image", 12, 1200)[:511]
        entries = np.concatenate([np.repeat(d, 4), np.array([EMPTY, 0], np.uint64)])
        entries = np.random.default_rng(k).permutation(entries)
        absent = low_keys(k, "image", 12, 1200)[511:811]
        m = tm.Model(entries, tm.slots_for(len(entries)))
        assert m.slots == 4096 and len(m.keys) == 512 and m.wrapped >= 500 and m.longest >= 500
        assert 0 in m.keys.tolist() and EMPTY not in m.keys.tolist()
        assert (m.absent_probes(absent) >= 500).all()
    elif name == "chain":  # a long chain away from the end
        c = chain_keys(k)
        entries, absent = c[:400], c[400:]
        m = tm.Model(entries, tm.slots_for(len(entries)))
        assert m.slots == 1024 and m.wrapped == 0 and m.longest >= 400
        assert (m.absent_probes(absent) == 401).all()
    else:  # no collisions: wave edges
        entries, absent = edge_keys(k, "image"), none
        m = tm.Model(entries, tm.slots_for(len(entries)))
        assert m.slots == 1024 and m.slot_of.tolist() == list(EDGE_HOMES) and m.longest == 1
    return frozen(entries), frozen(absent), m


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", E_CASES)
def test_mode_e_cases_reach_their_slots(name, k):
    entries, absent, m = e_case(name, k)
    assert (entries[entries != U(EMPTY)] <= tm.kmer_mask(k)).all()
    assert not set(absent.tolist()) & set(entries.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", E_CASES)
def test_mode_e_table_at_chosen_slots(engine, name, k):
    """k_kset_insert's table, read back with klsh_kset_find: every member has a slot of its own,
    the occupied slots are the model's, every slot lies between its key's home and its cluster's
    end, and absent keys — each walking the chain to its first empty slot — come back absent."""
    from kmerlsh_amd import _native

    entries, absent, m = e_case(name, k)
    ks = _native.KmerSet(engine, entries)
    try:
        slots, n_slots = ks.find(m.keys)
        assert n_slots == m.slots
        assert (slots != U(EMPTY)).all()
        assert len(np.unique(slots)) == len(slots)
        assert np.array_equal(np.sort(slots.astype(np.int64)), m.occupied_set())
        assert m.in_cluster(m.keys, slots).all()
        if name == "edges":
            assert slots.tolist() == list(EDGE_HOMES)
        with options(engine, grid_cap=1):  # k_kset_find on one workgroup: 256 keys a trip
            again, _ = ks.find(m.keys)
        assert np.array_equal(again, slots)
        # the entries as they were given: duplicates share their key's slot, all ones has none
        where = dict(zip(m.keys.tolist(), slots.tolist()))
        got, _ = ks.find(entries)
        assert got.tolist() == [where.get(e, EMPTY) for e in entries.tolist()]
        if len(absent):
            got, _ = ks.find(absent)
            assert (got == U(EMPTY)).all()
    finally:
        ks.close()


@pytest.mark.gpu
def test_kset_find_arguments(engine):
    from kmerlsh_amd import _native

    ks = _native.KmerSet(engine, np.zeros(0, np.uint64))
    try:
        got, n_slots = ks.find(np.zeros(0, np.uint64))
        assert got.size == 0 and n_slots == 1024
        got, _ = ks.find(np.array([0, EMPTY, 5], np.uint64))
        assert (got == U(EMPTY)).all()
        lib = engine._lib
        assert lib.klsh_kset_find(engine._ctx, None, None, 0, None, None) == -1  # KLSH_E_ARG
        assert lib.klsh_kset_find(engine._ctx, ks._set, None, 3, None, None) == -1
    finally:
        ks.close()


@functools.lru_cache(maxsize=None)
def key_reads(name, k):
    """One read per member and per absent key of a case: the key's k bases, then 10 filler bases,
    redrawn until the oracle counts exactly 1 hit (members) or 0 (absent keys)."""
    entries, absent, m = e_case(name, k)
    keys = np.concatenate([m.keys, absent])
    want = np.concatenate([np.ones(len(m.keys), np.uint32), np.zeros(len(absent), np.uint32)])
    rng = np.random.default_rng(7000 + k)

    def filler():
        return rng.choice(list(b"ACGT"), size=10).astype(np.uint8).tobytes()

    reads = [tm.image_string(key, k).encode() + filler() for key in keys.tolist()]
    for _ in range(20):
        hits, _ = oe.check_reads(reads, entries, k, 0.0)
        bad = np.flatnonzero(hits != want)
        if not len(bad):
            break
        for i in bad.tolist():
            reads[i] = reads[i][:k] + filler()
    assert np.array_equal(hits, want)
    return reads, want


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["wrap", "chain"])
def test_key_reads_hit_once_or_never(name, k):
    reads, want = key_reads(name, k)
    assert all(len(r) == k + 10 for r in reads) and 0 < int(want.sum()) < len(want)


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["wrap", "chain"])
def test_mode_e_reads_at_chosen_slots(engine, name, k):
    """The same tables through k_check_reads (ktab_find<false>): a read per member and per absent
    key, whose lookups walk the long chains; 1 / 11 > 0.05 extracts the members' reads only."""
    from kmerlsh_amd import _native

    entries, _, _ = e_case(name, k)
    reads, want = key_reads(name, k)
    ks = _native.KmerSet(engine, entries)
    try:
        for vote in (0.0, 0.05):
            hits, flags = ks.check_reads(reads, k, vote)
            oh, of = oe.check_reads(reads, entries, k, vote)
            assert np.array_equal(oh, want) and np.array_equal(of, (want > 0).astype(np.uint8))
            assert np.array_equal(hits, oh), vote
            assert np.array_equal(flags, of), vote
    finally:
        ks.close()


# ================================================================================== mode K ===
K_CASES = ("half", "again", "grown", "edges")


def strand(v, k, other):
    s = tm.value_string(v, k)
    return mi.revcomp(s) if other else s


@functools.lru_cache(maxsize=None)
def k_case(name, k):
    """(the reads of the one sample, the rehashes and peak table the growth rule gives, the
    expected listing), with the case's reach asserted from the model alone."""
    rng = np.random.default_rng(8000 + k)
    if name == "half":  # half full, never grown
        keys = wrap_keys(k, "kmc")[:512]
        seqs = [strand(v, k, False) for v in keys.tolist()]
        m = tm.Model(keys, 1024)
        assert m.wrapped >= 500 and m.longest >= 500
    elif name == "again":  # keys that are already there, met from the other strand
        keys = wrap_keys(k, "kmc")[:256]
        seqs = [strand(v, k, False) for v in keys.tolist()] + \
               [strand(v, k, True) for v in keys.tolist()]
        m = tm.Model(keys, 1024)
        assert m.wrapped >= 250 and m.longest >= 250
    elif name == "grown":  # one chain from the last slot of the 1024-, 2048- and 4096-slot table
        keys = low_keys(k, "kmc", 12, 1200)
        times = rng.integers(1, 4, len(keys))
        seqs = [strand(v, k, rng.integers(0, 2)) for v, t in zip(keys.tolist(), times.tolist())
                for _ in range(t)]
        seqs = [seqs[i] for i in rng.permutation(len(seqs))]
        for slots in (1024, 2048, 4096):
            assert ((tm.ktab_hash(keys) & U(slots - 1)) == U(slots - 1)).all()
        m = tm.Model(keys, 4096)
        assert m.wrapped == len(keys) - 1 and m.longest == len(keys)
    else:  # the collect's wave edges: counts 1..5
        keys = edge_keys(k, "kmc")
        seqs = [strand(v, k, (i + t) & 1) for i, v in enumerate(keys.tolist()) for t in range(i + 1)]
        m = tm.Model(keys, 1024)
        assert m.slot_of.tolist() == list(EDGE_HOMES)
    # grow() (klsh_kcount.cpp): before a batch, the table doubles until occupied + the batch's
    # windows <= slots / 2; a read of k bases is one window
    cap, rehashes, seen = 1024, 0, set()
    for b in range(0, len(seqs), 64):
        batch = seqs[b:b + 64]
        while len(seen) + len(batch) > cap // 2:
            cap, rehashes = cap * 2, rehashes + 1
        seen |= set(kc.count_occurrences(batch, k))
    occ = kc.count_occurrences(seqs, k)
    assert sorted(ki.kmer_value(w) for w in occ) == sorted(keys.tolist())  # canonical, all there
    return seqs, rehashes, cap, kc.listing_of(occ, 1)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", K_CASES)
def test_mode_k_cases_reach_their_tables(name, k):
    seqs, rehashes, peak, listing = k_case(name, k)
    assert all(len(s) == k for s in seqs)
    counts = [n for _, n in listing]
    want = {"half": (512, 0, 1024, [1]), "again": (512, 0, 1024, [2]),
            "grown": (len(seqs), 2, 4096, [1, 2, 3]), "edges": (15, 0, 1024, [1, 2, 3, 4, 5])}
    assert (len(seqs), rehashes, peak, sorted(set(counts))) == want[name]
    if name == "edges":  # count i + 1 on the key homed at EDGE_HOMES[i]
        by_value = dict((ki.kmer_value(w), n) for w, n in listing)
        assert [by_value[v] for v in edge_keys(k, "kmc").tolist()] == [1, 2, 3, 4, 5]


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", K_CASES)
def test_mode_k_table_at_chosen_slots(engine, name, k, tmp_path):
    """k_kcount_reads (ktab_claim_read), k_kcount_rehash and k_ktab_collect<ByValue> on a table
    whose chain wraps: the listing is the model's, and rehashes / peak slots are what the growth
    rule gives, so the case ran in the table sizes it was built for."""
    seqs, rehashes, peak, listing = k_case(name, k)
    path = str(tmp_path / "s0.fq")
    kc.write_fastq(path, seqs, "r0")
    with options(engine, kcount_table_slots=1024, kcount_batch_reads=64, kcount_keep_listing=1):
        st = engine.count_khtable([path], k, 1, str(tmp_path))
        vals, cnts = engine.kcount_listing(0)
        assert engine.get_option("kcount_rehashes") == st["rehashes"] == rehashes
        assert engine.get_option("kcount_peak_slots") == peak
        assert engine.get_option("kcount_batches") == -(-len(seqs) // 64)
    assert st["reads"] == st["positions"] == len(seqs) and st["distinct"] == len(listing)
    assert np.array_equal(vals, np.array([ki.kmer_value(w) for w, _ in listing], np.uint64))
    assert np.array_equal(cnts, np.array([n for _, n in listing], np.uint32))


# ================================================================================== mode B ===
B_CASES = ("wrap", "long", "edges")
B_PREFIX = {32: 0, 21: 5}  # LUT prefix symbols: (k - p) % 4 == 0


@functools.lru_cache(maxsize=None)
def b_case(name, k):
    """(per sample: [(k-mer string, count)], the distinct reps), with the case's reach asserted
    from the model alone.  A rep's record is listed on either strand."""
    rng = np.random.default_rng(9000 + k)

    def records(reps):
        return [(tm.image_string(r, k) if i & 1 else mi.revcomp(tm.image_string(r, k)),
                 int(rng.integers(1, 200))) for i, r in enumerate(reps.tolist())]

    if name == "wrap":  # one chain across the wrap of 1024 slots; 128 rows shared
        reps = wrap_keys(k, "image")[:382]
        samples = [records(reps[:255]), records(np.concatenate([reps[:128], reps[255:]]))]
        slots, m = 1024, tm.Model(reps, 1024)
        assert len(m.keys) == 382 and m.wrapped >= 370
    elif name == "long":  # one chain from the last slot of 4096
        reps = low_keys(k, "image", 12, 1200)[:1000]
        samples = [records(reps[0:400]), records(reps[300:700]), records(reps[600:1000])]
        slots, m = 4096, tm.Model(reps, 4096)
        assert (m.home == 4095).all() and m.wrapped == 999 and m.longest == 1000
    else:
        reps = edge_keys(k, "image")
        samples = [records(reps), records(reps[1:4])]
        slots, m = 1024, tm.Model(reps, 1024)
        assert m.slot_of.tolist() == list(EDGE_HOMES)
    # the table's size (klsh_kmc.cpp): 1024 slots, doubled until 2 (records + samples) fit
    assert tm.slots_for(sum(len(s) for s in samples) + len(samples)) == slots
    for recs in samples:  # the records' reps are the chosen keys, by the oracle's scalar forms
        got = [ob.canonical(ob.image(ki.kmer_value(s), k), k) for s, _ in recs[:40]]
        assert set(got) <= set(reps.tolist())
    return samples, reps


@pytest.fixture(scope="module")
def b_dbs(tmp_path_factory):
    """(name, k) -> (database paths, the oracle's first-appearance list, its three files)."""
    cache = {}

    def get(name, k):
        if (name, k) not in cache:
            samples, reps = b_case(name, k)
            d = tmp_path_factory.mktemp("%s%d" % (name, k))
            names = []
            for j, recs in enumerate(samples):
                names.append(str(d / ("db%d" % j)))
                ki.write_db(names[-1], k, recs, 0, B_PREFIX[k], 2, 1, 65535)
            first, fcounts, _ = ob.build_khtable(names, k, order="first")
            rows, counts, log = ob.build_khtable(names, k)
            files = (np.array(rows, "<u8").tobytes(),
                     np.ascontiguousarray(counts, "<u2").tobytes(), log.encode())
            cache[name, k] = (names, np.array(first, np.uint64), fcounts, files)
        return cache[name, k]

    return get


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", B_CASES)
def test_mode_b_cases_reach_their_tables(b_dbs, name, k):
    samples, reps = b_case(name, k)
    names, first, fcounts, files = b_dbs(name, k)
    assert sorted(first.tolist()) == sorted(reps.tolist())  # no filtered sample: no all-A row
    assert [len(s) for s in samples] == {"wrap": [255, 255], "long": [400] * 3,
                                         "edges": [5, 3]}[name]
    if name == "wrap":  # the shared rows carry both samples' counts
        both = (fcounts[0] > 0) & (fcounts[1] > 0)
        assert int(both.sum()) == 128 and (fcounts[0][both] != fcounts[1][both]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name,chunk", [("wrap", 0), ("long", 0), ("long", 100), ("edges", 0)])
def test_mode_b_table_at_chosen_slots(engine, b_dbs, name, chunk, k, tmp_path):
    """k_kmc_union (ktab_claim), k_kmc_count (ktab_find<true>) and k_ktab_collect<ByFirst> on a
    chain across the wrap: first-appearance list and files are the oracle's; in 100-record chunks
    later launches meet keys that are already there."""
    samples, _ = b_case(name, k)
    names, first, _, files = b_dbs(name, k)
    with options(engine, kmc_keep_first=1, kmc_chunk_records=chunk):
        st = engine.build_khtable(names, k, str(tmp_path))
        mine = engine.khtable_first()
        launches = engine.get_option("kmc_decode_launches")
    assert launches == sum(-(-len(s) // (chunk or len(s))) for s in samples)
    assert st["kmap_size"] == len(first) and st["records_listed"] == sum(len(s) for s in samples)
    assert np.array_equal(mine, first)
    assert tuple((tmp_path / n).read_bytes() for n in FILES) == files


# ============================================================== mode E: the LDS window's edges ===
WINDOW_KS = (11, 21, 32)


@functools.lru_cache(maxsize=None)
def window_case(k, W):
    """(reads of W - 1 .. 3 W + 1 k-mer positions, the set: their canonical k-mers at positions 0,
    W - 2, W - 1, W, W + 1 and the last one, the planted positions per read); reads redrawn until
    the oracle counts exactly the planted positions in each."""
    rng = np.random.default_rng(6000 + k)
    nposs = (W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 3 * W + 1)
    planted = [sorted({p for p in (0, W - 2, W - 1, W, W + 1, n - 1) if 0 <= p < n})
               for n in nposs]

    def draw(n):
        return rng.choice(list(b"ACGT"), size=n + k - 1).astype(np.uint8).tobytes()

    reads = [draw(n) for n in nposs]
    for _ in range(50):
        kset = np.unique(np.concatenate([oe.canonical_kmers(r, k)[p]
                                         for r, p in zip(reads, planted)]))
        hits, _ = oe.check_reads(reads, kset, k, 0.0)
        bad = [j for j, p in enumerate(planted) if hits[j] != len(p)]
        if not bad:
            break
        for j in bad:
            reads[j] = draw(nposs[j])
    assert not bad
    return reads, frozen(kset), planted


def mixed_reads(k, reads):
    """The long reads inside 200 short ones (random, and slices of the long reads around their
    planted positions), so that a wave goes from a long read to short ones and back."""
    rng = np.random.default_rng(6500 + k)
    out = []
    for i in range(200):
        n = int(rng.integers(k + 10, k + 120))
        if i % 3 == 0:
            src = reads[i % len(reads)]
            a = int(rng.integers(0, len(src) - n))
            out.append(src[a:a + n])
        else:
            out.append(rng.choice(list(b"ACGT"), size=n).astype(np.uint8).tobytes())
    at = [3 + 29 * j for j in range(len(reads))]
    for j, r in zip(at, reads):
        out.insert(j, r)
    return out, at


@pytest.mark.parametrize("k", WINDOW_KS)
def test_window_reads_hold_only_their_planted_kmers(k):
    W = 2048
    reads, kset, planted = window_case(k, W)
    assert [len(r) - k + 1 for r in reads] == [W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1,
                                               3 * W + 1]
    assert [len(p) for p in planted] == [2, 3, 4, 6, 6, 6, 6]
    assert planted[0] == [0, W - 2] and planted[2] == [0, W - 2, W - 1, W]
    mixed, at = mixed_reads(k, reads)
    assert [mixed[j] for j in at] == reads and len(mixed) == 207


@pytest.mark.gpu
@pytest.mark.parametrize("k", WINDOW_KS)
def test_mode_e_window_edges(engine, k):
    """Set k-mers on the last position of one LDS window of k_check_reads and the first of the
    next, at read lengths one short of, exactly at and one past one, two and three windows."""
    from kmerlsh_amd import _native

    W = engine.get_option("extract_window")
    assert W >= 64
    reads, kset, planted = window_case(k, W)
    mixed, at = mixed_reads(k, reads)
    ks = _native.KmerSet(engine, kset)
    try:
        for vote in (0.0, 0.001):
            oh, of = oe.check_reads(reads, kset, k, vote)
            assert oh.tolist() == [len(p) for p in planted]
            hits, flags = ks.check_reads(reads, k, vote)
            assert np.array_equal(hits, oh) and np.array_equal(flags, of), vote
            mh, mf = oe.check_reads(mixed, kset, k, vote)
            assert mh[at].tolist() == oh.tolist()
            hits, flags = ks.check_reads(mixed, k, vote)
            assert np.array_equal(hits, mh) and np.array_equal(flags, mf), vote
    finally:
        ks.close()


# =============================================================================== vote ties ===
VOTE_KS = (1, 21, 32)
F = np.float32
VOTES = [F(0.5), F(1) / F(3), F(2) / F(3), F(0.1), F(0.7), F(0.9), F(1.0), F(0.0)]


@functools.lru_cache(maxsize=None)
def vote_grid(k):
    """Reads with exactly m hits in n windows against the set {all-A}, n = 11..60, m = 0..n:
    k - 1 + m A's, then n - m bases drawn from C and G (a window holding a C or G is not all-A,
    and neither is its twin, which holds a G or C)."""
    rng = np.random.default_rng(500 + k)
    reads, m_of, n_of = [], [], []
    for n in range(11, 61):
        for m in range(n + 1):
            tail = rng.choice(list(b"CG"), size=n - m).astype(np.uint8).tobytes()
            reads.append(b"A" * (k - 1 + m) + tail)
            m_of.append(m)
            n_of.append(n)
    m_of, n_of = np.array(m_of, np.uint32), np.array(n_of, np.uint32)
    hits, _ = oe.check_reads(reads, np.array([0], np.uint64), k, 0.0)
    assert np.array_equal(hits, m_of)  # from the oracle alone
    return reads, frozen(m_of), frozen(n_of)


@pytest.mark.parametrize("k", VOTE_KS)
def test_vote_grid_holds_exact_ties(k):
    reads, m_of, n_of = vote_grid(k)
    assert all(len(r) - k + 1 == n for r, n in zip(reads, n_of.tolist()))
    ratio = m_of.astype(F) / n_of.astype(F)
    assert ratio.dtype == F
    for vote in VOTES:
        assert (ratio == vote).any()  # (0.0 too: m = 0)
    assert ((ratio == F(0.0)) == (m_of == 0)).all()
    tie = (m_of == 14) & (n_of == 20)
    assert tie.sum() == 1 and ratio[tie][0] == F(0.7)
    # 7/10 and 9/10: the float quotient lies below the real ratio, so a comparison in double
    # against the float vote would extract these reads
    for num, den, m, n in ((7, 10, 14, 20), (9, 10, 18, 20)):
        q = F(m) / F(n)
        assert Fraction(float(q)) < Fraction(num, den) and q == F(num / den)
        assert float(m) / float(n) > float(q)


@pytest.mark.gpu
@pytest.mark.parametrize("k", VOTE_KS)
def test_vote_ties_do_not_extract(engine, k):
    """(float)hits / (float)positions > vote at every vote of the list and one ulp to either side:
    an exact tie does not extract, one ulp below does."""
    from kmerlsh_amd import _native

    reads, m_of, n_of = vote_grid(k)
    ratio = m_of.astype(F) / n_of.astype(F)
    ks = _native.KmerSet(engine, np.array([0, int(tm.image_rep(tm.kmer_mask(k), k))], np.uint64))
    try:
        for v in VOTES:
            for vote in (np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))):
                assert vote.dtype == F
                hits, flags = ks.check_reads(reads, k, float(vote))
                assert np.array_equal(hits, m_of)
                want = (ratio > vote).astype(np.uint8)
                assert np.array_equal(flags, want), (float(vote), np.flatnonzero(flags != want)[:5])
    finally:
        ks.close()
