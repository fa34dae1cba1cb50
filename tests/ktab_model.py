"""The k-mer table of modes E, B and K (kmerlsh_amd/csrc/klsh_kmer.h) as a CPU model, and keys
chosen by where they land in it.  TEST INFRASTRUCTURE ONLY.

The device table has `slots` 64-bit slots (a power of two), a key's home slot is the low bits of
the murmur3 finalizer of the key, and a key sits in the first slot at or cyclically after its home
that was free when it came.  With insertions only, the SET of occupied slots does not depend on
the insertion order (each cluster is filled from the homes that fall into it, whoever comes
first), so `model` predicts that set for whatever order the device's CAS operations resolve in;
which key sits in which slot of a cluster does depend on the order and is not predicted.

The murmur3 finalizer is cheap to search forwards: `search` draws random k-mers from a seeded
generator, takes their canonical form in the encoding asked for, and keeps those whose home slot
(or whose low hash bits) are the chosen ones.

Encodings (klsh_kmer.h): "image" = the reference Kmer's 8-byte image, base i at bits 2i, canonical
= the smaller in memcmp order of the image and its twin (the keys of modes E and B); "kmc" = the
KMC value, base 0 in the most significant of its 2k bits, canonical = the numerically smaller of
the value and its reverse complement's value (the keys of mode K).
"""
import numpy as np

U = np.uint64
EMPTY = 0xFFFFFFFFFFFFFFFF  # an empty slot; "absent" in KmerSet.find


def ktab_hash(keys):
    """The murmur3 finalizer (klsh_kmer.h kmer_hash) of uint64 keys, wrapping arithmetic."""
    k = np.array(keys, dtype=np.uint64, copy=True).reshape(-1)
    k ^= k >> U(33)
    k *= U(0xFF51AFD7ED558CCD)
    k ^= k >> U(33)
    k *= U(0xC4CEB9FE1A85EC53)
    k ^= k >> U(33)
    return k


def kmer_mask(k):
    return U(EMPTY) if k == 32 else U((1 << (2 * k)) - 1)


def reverse_bases(v, k):
    """The k bases of v (bits [0, 2k)) in reverse order, either encoding."""
    x = np.asarray(v, np.uint64)
    m2, m4 = U(0x3333333333333333), U(0x0F0F0F0F0F0F0F0F)
    x = ((x >> U(2)) & m2) | ((x & m2) << U(2))
    x = ((x >> U(4)) & m4) | ((x & m4) << U(4))
    return x.byteswap() >> U(64 - 2 * k)


def revcomp(v, k):
    """The reverse complement's word, either encoding (Kmer::twin on images)."""
    return reverse_bases(~np.asarray(v, np.uint64) & kmer_mask(k), k)


def image_rep(img, k):
    """(km < twin) ? km : twin with operator< = memcmp of the 8 bytes, on images."""
    img = np.asarray(img, np.uint64)
    tw = revcomp(img, k)
    return np.where(img.byteswap() < tw.byteswap(), img, tw)


def kmc_canonical(v, k):
    """KMC's canonical k-mer: the smaller of the value and its reverse complement's value."""
    v = np.asarray(v, np.uint64)
    return np.minimum(v, revcomp(v, k))


def value_image(v, k):
    """KMC value <-> Kmer image (the same k bases, the other way round)."""
    return reverse_bases(v, k)


def canonical(v, k, encoding):
    return {"image": image_rep, "kmc": kmc_canonical}[encoding](v, k)


def image_string(img, k):
    """The bases of one image, base 0 first."""
    return "".join("ACGT"[(int(img) >> (2 * i)) & 3] for i in range(k))


def value_string(v, k):
    """The bases of one KMC value, base 0 first."""
    return "".join("ACGT"[(int(v) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def slots_for(n):
    """The slots of a table made for n entries: 1024, doubled until 2n fit."""
    cap = 1024
    while cap < 2 * n:
        cap <<= 1
    return cap


def search(k, encoding, n, seed, slots=None, homes=None, low_bits=None, batch=1 << 19):
    """n distinct canonical keys of length k in `encoding`, in the order a seeded generator gives
    them, whose home slot in a table of `slots` slots is one of `homes`, or whose hash has its
    low `low_bits` bits all ones (their home is then the last slot of every table of up to
    2^low_bits slots).  Never 0 (hash 0: the one key whose home is slot 0 in every table) and
    never all ones."""
    assert (homes is None) != (low_bits is None)
    rng = np.random.default_rng(seed)
    if homes is not None:
        want = np.zeros(slots, bool)
        want[np.asarray(list(homes), np.int64)] = True
    out, seen = [], set()
    for _ in range(400):
        v = rng.integers(0, 1 << 63, size=batch, dtype=np.uint64) << U(1) | \
            rng.integers(0, 2, size=batch, dtype=np.uint64)
        c = canonical(v & kmer_mask(k), k, encoding)
        h = ktab_hash(c)
        if homes is not None:
            ok = want[(h & U(slots - 1)).astype(np.int64)]
        else:
            ok = (h & U((1 << low_bits) - 1)) == U((1 << low_bits) - 1)
        for key in c[ok].tolist():
            if key not in seen and key != 0 and key != EMPTY:
                seen.add(key)
                out.append(key)
                if len(out) == n:
                    return np.array(out, np.uint64)
    raise AssertionError("search: %d of %d keys found" % (len(out), n))


def search_homes_in_order(k, encoding, homes, slots, seed):
    """One key per entry of `homes`, key i with home slot homes[i]."""
    pool = search(k, encoding, 40 * len(homes), seed, slots=slots, homes=homes)
    home = (ktab_hash(pool) & U(slots - 1)).astype(np.int64)
    return np.array([pool[np.flatnonzero(home == h)[0]] for h in homes], np.uint64)


class Model:
    """Linear probing of the distinct keys (all ones skipped) in the order given."""

    def __init__(self, keys, slots):
        keys = np.asarray(keys, np.uint64)
        _, first = np.unique(keys, return_index=True)
        keys = keys[np.sort(first)]
        self.keys = keys[keys != U(EMPTY)]
        self.slots = slots
        mask = slots - 1
        self.home = (ktab_hash(self.keys) & U(mask)).astype(np.int64)
        nxt = list(range(slots))  # nxt[s]: a slot at or after s that may be free (path-compressed)
        slot_of = np.zeros(len(self.keys), np.int64)
        assert 2 * len(self.keys) <= slots
        for i, h in enumerate(self.home.tolist()):
            s, path = h, []
            while nxt[s] != s:
                path.append(s)
                s = nxt[s]
            nxt[s] = (s + 1) & mask
            for p in path:
                nxt[p] = nxt[s]
            slot_of[i] = s
        self.slot_of = slot_of
        self.occupied = np.zeros(slots, bool)
        self.occupied[slot_of] = True
        self.probes = ((slot_of - self.home) & mask) + 1
        self.wrapped = int((slot_of < self.home).sum())
        self.longest = int(self.probes.max()) if len(self.keys) else 0

    def occupied_set(self):
        return np.flatnonzero(self.occupied)

    def cluster_end(self, home):
        """The first free slot at or cyclically after each home slot."""
        free = np.flatnonzero(~self.occupied)
        home = np.asarray(home, np.int64)
        i = np.searchsorted(free, home)
        return np.where(i < len(free), free[np.minimum(i, len(free) - 1)], free[0])

    def in_cluster(self, keys, slot):
        """Whether each key's slot lies in the cyclic interval from its home to its cluster's
        end (the only slots linear probing can give it)."""
        mask = self.slots - 1
        home = (ktab_hash(keys) & U(mask)).astype(np.int64)
        end = self.cluster_end(home)
        return ((np.asarray(slot, np.int64) - home) & mask) < ((end - home) & mask)

    def absent_probes(self, keys):
        """Slots a lookup of each (absent) key reads: from its home to the first free slot."""
        mask = self.slots - 1
        home = (ktab_hash(keys) & U(mask)).astype(np.int64)
        return ((self.cluster_end(home) - home) & mask) + 1


def model(keys, slots):
    """(occupied slots ascending, each distinct key's home slot, keys that end below their home
    slot (wrapped), the longest probe) of linear probing."""
    m = Model(keys, slots)
    return m.occupied_set(), m.home, m.wrapped, m.longest
