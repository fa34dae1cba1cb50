"""FASTQ inputs and the counting model for mode-K fixtures (TEST INFRASTRUCTURE ONLY).

`write_case(dir, case)` writes one FASTQ file per sample (drawn from a splitmix64 stream:
byte-reproducible anywhere, written at test time) and a.txt / b.txt ("<fastq> <kmc db name>"
lines, serving -M K by their first column and -M B by their second).

The model is what `kmc -k<K> -r -cs65535 -ci<C>` lists for such a file, in the order of a
KMC1-layout database: `count_listing(path, k, count_min)` -> [(k-mer string, count)], a plain
dictionary counter that shares nothing with the kernels.  A C G T a c g t are bases, any other
character breaks the read; every window of k bases is one occurrence of the smaller of the window
and its reverse complement (plain string order = KMC value order); a k-mer is listed with
min(occurrences, 65535) from count_min occurrences on, ascending.  `write_model_dbs` writes each
sample's listing as a KMC1 database (kmc_inputs.write_db) for the reference CLI's and the
oracle's mode B.
"""
from __future__ import annotations

import gzip
import hashlib
import os

from kmc_inputs import write_db
from mode_e_inputs import SplitMix, revcomp

# lut_prefix_length per k: (k - p) % 4 == 0
PREFIX = {1: 1, 4: 0, 5: 1, 16: 8, 17: 9, 21: 9, 31: 11, 32: 12}

CASES = {
    # 3 + 3 samples from shared genomes, both strands, reads of 60..150 bases; lower case, N at the
    # first / last base and in runs, reads shorter than k and of exactly k, an empty record, one
    # gzip sample, one with multi-line records, one with CRLF
    "k21": dict(k=21, count_min=2, n1=3, n2=3, genomes=3, glen=400, reads=110, rlen=(60, 150),
                seed=401, gz=(1,), crlf=(4,), multiline=(2,)),
    "k31": dict(k=31, count_min=3, n1=2, n2=2, genomes=2, glen=300, reads=140, rlen=(60, 150),
                seed=409, gz=(), crlf=(), multiline=(1,)),
    # the 64-bit mask edge; every k-mer listed
    "k32": dict(k=32, count_min=1, n1=1, n2=1, genomes=2, glen=300, reads=60, rlen=(60, 150),
                seed=419, gz=(0,), crlf=(), multiline=()),
    # one-byte Kmer images; k = 4 with the palindromes ACGT and AATT
    "k1": dict(k=1, count_min=2, n1=1, n2=1, genomes=1, glen=60, reads=12, rlen=(1, 20), seed=421,
               gz=(), crlf=(1,), multiline=()),
    "k4": dict(k=4, count_min=2, n1=2, n2=1, genomes=2, glen=120, reads=40, rlen=(4, 60), seed=431,
               gz=(), crlf=(), multiline=(), extra=("ACGTACGTACGT", "AATTAATT", "acgtNAATT")),
    "k5": dict(k=5, count_min=2, n1=1, n2=2, genomes=2, glen=150, reads=50, rlen=(5, 70), seed=433,
               gz=(2,), crlf=(), multiline=(0,)),
    # the edge of the listing's order by a 2k-bit value: k = 16 is one sort over exactly 32 bits,
    # k = 17 adds the pass over the values' high words, 2 bits wide
    "k16": dict(k=16, count_min=2, n1=1, n2=1, genomes=2, glen=200, reads=150, rlen=(16, 80),
                seed=457, gz=(), crlf=(), multiline=()),
    "k17": dict(k=17, count_min=2, n1=1, n2=1, genomes=2, glen=200, reads=150, rlen=(17, 80),
                seed=461, gz=(), crlf=(), multiline=()),
    # saturation: see _sat_samples
    "sat": dict(k=21, count_min=2, n1=1, n2=1, genomes=1, glen=200, reads=30, rlen=(60, 120),
                seed=439, gz=(), crlf=(), multiline=()),
    # the count_min filter across samples: see _filt_samples
    "filt": dict(k=21, count_min=3, n1=2, n2=2, seed=443, gz=(), crlf=(), multiline=()),
}
# reads built from the kernel's own LDS window W (option "kcount_window"): see win_samples
WIN = dict(k=21, count_min=1, n1=1, n2=1, seed=449, gz=(), crlf=(), multiline=())


def _random_seq(rng: SplitMix, n: int) -> str:
    return "".join("ACGT"[rng.below(4)] for _ in range(n))


def _genome_samples(c: dict) -> list:
    k = c["k"]
    rng = SplitMix(c["seed"])
    genomes = [_random_seq(rng, c["glen"]) for _ in range(c["genomes"])]
    lo, hi = c["rlen"]
    samples = []
    for j in range(c["n1"] + c["n2"]):
        recs = []
        for r in range(c["reads"]):
            g = genomes[rng.below(len(genomes))]
            ln = min(lo + rng.below(hi - lo + 1), len(g))
            p = rng.below(len(g) - ln + 1)
            s = g[p:p + ln]
            if rng.below(2):
                s = revcomp(s)
            s = list(s)
            for q in range(len(s)):
                u = rng.below(1000)
                if u < 5:
                    s[q] = "ACGT"[rng.below(4)]
                elif u < 8:
                    s[q] = "N"
                elif u < 30:
                    s[q] = s[q].lower()
            s = "".join(s)
            m = r % 23
            if m == 3:
                s = "N" + s[1:]                      # N at position 0
            elif m == 5:
                s = s[:-1] + "N"                     # N at the last position
            elif m == 7 and len(s) > 8:
                s = s[:len(s) // 2] + "NNNN" + s[len(s) // 2 + 4:]  # a run of N
            elif m == 11:
                s = s[:k - 1]                        # shorter than k: no window
            elif m == 13:
                s = s[:k]                            # exactly k: one window
            recs.append(s)
            if r == 9:
                recs.append("")                      # an empty record
        if j == 0:
            recs += list(c.get("extra", ()))
        samples.append(recs)
    return samples


def _sat_samples(c: dict) -> list:
    """Sample 0: a poly-A read of 65535 + 20 windows and a poly-T read of 5 (the same canonical
    k-mer: 65560 occurrences); an (AC)-repeat read whose 2 x 65535 windows alternate between two
    k-mers (65535 each), and one more read of exactly k bringing the first of them to 65536."""
    k = c["k"]
    s0 = ["A" * (65535 + 20 + k - 1), "T" * (k + 4), ("AC" * (65535 + k))[:2 * 65535 + k - 1],
          ("AC" * k)[:k]]
    rest = _genome_samples(c)
    return [s0 + rest[0], rest[1] + ["a" * (k + 9), ("CA" * k)[:k + 3]]]


def _filt_samples(c: dict) -> list:
    """Sample 0 lists read A's k-mers (3 copies) and has read B's twice (below count_min = 3);
    sample 1 lists B's (3 copies) and has A once; sample 2 has every k-mer once (an empty
    listing); sample 3 is an empty file."""
    rng = SplitMix(c["seed"])
    a, b, g2 = _random_seq(rng, 100), _random_seq(rng, 60), _random_seq(rng, 150)
    return [[a, b, revcomp(a), b, a], [b, a, revcomp(b), b], [g2], None]


def win_samples(W: int) -> list:
    """Reads of W + k - 2, W + k - 1, W + k and 2W + k bases (W - 1, W, W + 1 and 2W + 1 k-mer
    positions: one short of a window, exactly one, one into the second, one into the third): of
    each length one clean and one with a single N at base W - 1, W and W + k - 1 (the last window
    position's first base, the next window's, and the last base of the first window's last k-mer).
    Sample 1 holds the reverse complements of the clean ones."""
    k = WIN["k"]
    rng = SplitMix(WIN["seed"])
    s0, s1 = [], []
    for ln in (W + k - 2, W + k - 1, W + k, 2 * W + k):
        clean = _random_seq(rng, ln)
        s0.append(clean)
        s1.append(revcomp(clean))
        for at in (W - 1, W, W + k - 1):
            s = _random_seq(rng, ln)
            if at < ln:
                s = s[:at] + "N" + s[at + 1:]
            s0.append(s)
    return [s0, s1]


def write_fastq(path: str, seqs, tag: str, crlf: bool = False, multiline: bool = False) -> None:
    recs = []
    for i, s in enumerate(seqs):
        q = "I" * len(s)
        if multiline and i % 5 == 0 and len(s) > 30:
            recs.append("@%s_%d\n%s\n%s\n+\n%s\n%s\n" % (tag, i, s[:30], s[30:], q[:25], q[25:]))
        else:
            recs.append("@%s_%d len=%d\n%s\n+\n%s\n" % (tag, i, len(s), s, q))
    text = "".join(recs)
    if crlf:
        text = text.replace("\n", "\r\n")
    if path.endswith(".gz"):
        with gzip.GzipFile(path, "wb", mtime=0) as f:
            f.write(text.encode())
    else:
        with open(path, "w", newline="") as f:
            f.write(text)


def write_samples(dirpath: str, c: dict, samples) -> dict:
    names = []
    for j, seqs in enumerate(samples):
        name = "s%d.fq" % j + (".gz" if j in c["gz"] else "")
        write_fastq(os.path.join(dirpath, name), seqs or [], "r%d" % j, j in c["crlf"],
                    j in c["multiline"])
        names.append(name)
    n1 = c["n1"]
    with open(os.path.join(dirpath, "a.txt"), "w") as f:
        f.write("".join("%s db%d\n" % (names[j], j) for j in range(n1)))
    with open(os.path.join(dirpath, "b.txt"), "w") as f:
        f.write("".join("%s db%d\n" % (names[j], j) for j in range(n1, len(names))))
    return dict(c, d=len(names), fastq=names, seqs=[list(s or []) for s in samples])


def write_case(dirpath: str, case: str) -> dict:
    c = CASES[case]
    samples = (_sat_samples(c) if case == "sat" else _filt_samples(c) if case == "filt"
               else _genome_samples(c))
    return write_samples(dirpath, c, samples)


def write_win_case(dirpath: str, W: int) -> dict:
    return write_samples(dirpath, WIN, win_samples(W))


# ------------------------------------------------------------------------------- the model ---
def read_sequences(path: str) -> list:
    """The sequences of the FASTQ files written above (records of '@' header, sequence lines,
    '+' line, as many quality characters as bases)."""
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        lines = [ln.strip() for ln in f.read().decode("ascii").split("\n")]
    seqs, i = [], 0
    while i < len(lines):
        if not lines[i].startswith("@"):
            i += 1
            continue
        i += 1
        seq = ""
        while i < len(lines) and not lines[i].startswith("+"):
            seq += lines[i]
            i += 1
        i += 1
        q = 0
        while i < len(lines) and q < len(seq):
            q += len(lines[i])
            i += 1
        seqs.append(seq)
    return seqs


def count_occurrences(seqs, k: int) -> dict:
    occ = {}
    for s in seqs:
        s = s.upper()
        for p in range(len(s) - k + 1):
            w = s[p:p + k]
            if w.strip("ACGT"):
                continue  # a break inside the window
            w = min(w, revcomp(w))
            occ[w] = occ.get(w, 0) + 1
    return occ


def listing_of(occ: dict, count_min: int) -> list:
    return [(w, min(n, 65535)) for w, n in sorted(occ.items()) if n >= max(count_min, 1)]


def count_listing(fastq_path: str, k: int, count_min: int) -> list:
    return listing_of(count_occurrences(read_sequences(fastq_path), k), count_min)


def listing_md5(listing) -> str:
    return hashlib.md5("".join("%s\t%d\n" % wc for wc in listing).encode()).hexdigest()


def write_model_dbs(dirpath: str, info: dict) -> list:
    """(database paths, listings): sample j's listing as KMC1 database db<j>, 2-byte counters."""
    k, cm = info["k"], max(info["count_min"], 1)
    paths, listings = [], []
    for j, name in enumerate(info["fastq"]):
        listing = count_listing(os.path.join(dirpath, name), k, cm)
        path = os.path.join(dirpath, "db%d" % j)
        write_db(path, k, listing, 0, PREFIX[k], 2, cm, 65535)
        paths.append(path)
        listings.append(listing)
    return paths, listings


def cli_args(info: dict, mode: str) -> list:
    return ["-a", "a.txt", "-b", "b.txt", "-o", "A", "-p", "B", "-K", str(info["k"]), "-C",
            str(info["count_min"]), "-M", mode, "--only", "--verbose"]
