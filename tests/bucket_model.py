"""A plain numpy model of one queued iteration's bucket order and run lists, and the inputs that
put chosen sizes at chosen places (tests/test_gpu_tail_buckets.py).

The engine sorts the live keys stably by their low `bits` bits (merge_hashtable's bucket order,
cluster.cc:15-30) and lists every run of two or more equal keys by its length class.  Below 2^20
rows it does so in one of two ways (run_batched): a partition by the top 9 key bits followed by
one LDS counting sort per top bucket over the remaining lb = bits - 9 bits (k_tail_local), or LSD
passes followed by the run kernels.  The model knows nothing of either; the builders know the
first one's geometry (top bucket = key >> lb, 256 lanes with J = ceil(m / 256) keys each up to
16, rounds of 4096 keys) so that a test can say where its keys land.

A key is (top << lb) | low.  Every builder returns keys below 2^bits; `with_stale_tail` appends
what a queued iteration leaves behind its live keys.
"""
import numpy as np

TOP_BITS = 9                # kTailTopBits
TOPS = 1 << TOP_BITS
LANES = 256                 # k_tail_local's workgroup
ROUND = 16 * LANES          # keys of one of its rounds at most (kItems = 16 per lane)
BIG_ROWS = (128, 192, 384, 896)
SMALL_LISTS, HUGE_LIST, OVER_LIST = 6, 10, 11
DIRTY = np.uint32(0xA5A5A5A5)   # what klsh_tail_buckets fills its workspaces with
# the smallest run of every list 0..10 and the capacity divisor of that list (klsh_ctx::alloc:
# group_class_capacity, s/65, s/129, s/193, s/385, s/897, each + 64)
LIST_MIN_ROWS = (2, 3, 5, 9, 17, 33, 65, 129, 193, 385, 897)
CLASS_EDGES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 192, 193, 384, 385, 896, 897)


def floor_log2(n):
    return int(n).bit_length() - 1


def local_ok(bits):
    """tail_local_ok for n_max < 2^20: the widths the local path takes."""
    return TOP_BITS < bits <= 19


# ------------------------------------------------------------------------------ the model -----
def stable_order(keys, n_live, bits):
    """Positions of keys[:n_live] in the stable order of their low `bits` bits."""
    mask = np.uint32((1 << bits) - 1)
    return np.argsort(keys[:n_live] & mask, kind="stable").astype(np.uint32)


def runs_reference(keys, bucket_thr):
    """Runs of equal keys (the buckets merge_hashtable fills, cluster.cc:15-30) of 2+ rows with the
    merge step's list: size class by length, > bucket_thr = nestedCluster (cluster.cc:286)."""
    n = keys.size
    heads = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]])) if n else np.zeros(0, int)
    lens = np.diff(np.concatenate([heads, [n]]))
    keep = lens >= 2
    heads, lens = heads[keep], lens[keep]
    lists = np.empty(lens.size, np.int32)
    for i, b in enumerate(lens):
        if bucket_thr >= 0 and b > bucket_thr:
            lists[i] = 11
        elif b > 896:
            lists[i] = 10
        elif b > 64:
            lists[i] = 6 + int(np.searchsorted([128, 192, 384, 896], b))
        else:
            lists[i] = int(np.searchsorted([2, 4, 8, 16, 32, 64], b))
    return heads.astype(np.uint32), lens.astype(np.uint32), lists


def list_of(lens, bucket_thr):
    """runs_reference's list of a run of each length in `lens` (2 or more), without the loop."""
    lens = np.asarray(lens, np.int64)
    edges = np.array([2, 4, 8, 16, 32, 64, 128, 192, 384, 896])
    lists = np.searchsorted(edges, lens).astype(np.int32)   # 0..9, 10 past 896
    if bucket_thr >= 0:
        lists[lens > bucket_thr] = OVER_LIST
    return lists


def runs_of(sorted_keys, bucket_thr):
    """runs_reference, vectorised: (starts, lengths, lists) of the runs of 2+ equal keys."""
    n = sorted_keys.size
    heads = np.flatnonzero(np.concatenate([[True], sorted_keys[1:] != sorted_keys[:-1]]))
    lens = np.diff(np.concatenate([heads, [n]]))
    keep = lens >= 2
    return (heads[keep].astype(np.uint32), lens[keep].astype(np.uint32),
            list_of(lens[keep], bucket_thr))


def counters_of(sorted_keys, bucket_thr):
    """The seven run counters beside the lists: heads (every run, those of one key too), the rows
    in runs of lists 0..5, in each of lists 6..9, and in list 10.  Oversize runs are in none."""
    heads = int(np.count_nonzero(sorted_keys[1:] != sorted_keys[:-1])) + 1
    _, lens, lists = runs_of(sorted_keys, bucket_thr)
    lens = lens.astype(np.int64)
    rows = [int(lens[lists < SMALL_LISTS].sum())]
    rows += [int(lens[lists == SMALL_LISTS + c].sum()) for c in range(len(BIG_ROWS))]
    rows.append(int(lens[lists == HUGE_LIST].sum()))
    return np.array([heads] + rows, np.uint32)


def expected(keys, n_live, bits, bucket_thr):
    """What klsh_tail_buckets must return for the live keys: the permutation, the sorted keys,
    the runs in start order and the counters."""
    perm = stable_order(keys, n_live, bits)
    sk = keys[:n_live][perm]
    masked = sk & np.uint32((1 << bits) - 1)
    return {"perm": perm, "keys": sk, "runs": runs_of(masked, bucket_thr),
            "counters": counters_of(masked, bucket_thr)}


# --------------------------------------------------------------------- what an input holds -----
def top_sizes(keys, bits):
    """Keys per top bucket (512 of them) of keys below 2^bits, bits 10..19."""
    return np.bincount(keys >> np.uint32(bits - TOP_BITS), minlength=TOPS)


def rounds(m):
    """4096-key rounds k_tail_local spends on a top bucket of m keys."""
    return -(-int(m) // ROUND)


def lanes_j(m):
    """J: the keys per lane of a round."""
    return min(16, -(-int(m) // LANES))


def run_lengths(keys):
    """The length of every run of equal keys, singletons included, in key order."""
    return np.unique(keys, return_counts=True)[1]


def lists_present(keys, bucket_thr):
    lens = run_lengths(keys)
    return set(int(l) for l in list_of(lens[lens >= 2], bucket_thr))


def with_stale_tail(live, n_max):
    """`live` followed by n_max - live.size stale keys 0xFFFFFFFF - i (i: the position), which
    cannot pass for a live key of 19 bits or fewer."""
    tail = np.uint32(0xFFFFFFFF) - np.arange(live.size, n_max, dtype=np.uint32)
    return np.concatenate([live.astype(np.uint32), tail])


def shuffled(keys, seed):
    return keys[np.random.default_rng(seed).permutation(keys.size)]


# -------------------------------------------------------------------------------- builders -----
def uniform(n, bits, seed):
    """n keys uniform over bits bits."""
    return np.random.default_rng(seed).integers(0, 1 << bits, n, dtype=np.uint64).astype(np.uint32)


def one_top_bucket(top, lb, m, seed):
    """m keys of TOP_BITS + lb bits, all in top bucket `top`, their low bits uniform."""
    low = np.random.default_rng(seed).integers(0, 1 << lb, m, dtype=np.uint64).astype(np.uint32)
    return np.uint32(top << lb) | low


def dealt_sizes():
    """A size for each of the 512 top buckets: 0, 1, 2, 3, 63, 64, 65 and 256 J - 1, 256 J,
    256 J + 1 for J = 1..16 once each, at buckets 2, 11, 20, ...; every other bucket alternates
    between empty (even) and 1, 2 or 3 keys (odd); buckets 0 and 511 and the two beside the
    largest bucket are empty."""
    special = [0, 1, 2, 3, 63, 64, 65] + [256 * j + k for j in range(1, 17) for k in (-1, 0, 1)]
    sizes = np.array([0 if d % 2 == 0 else 1 + (d // 2) % 3 for d in range(TOPS)], np.int64)
    where = 2 + 9 * np.arange(len(special))
    sizes[where] = special
    big = int(where[int(np.argmax(special))])
    sizes[[0, TOPS - 1, big - 1, big + 1]] = 0
    return sizes, where, np.array(special)


def dealt(bits, seed):
    """Keys whose top buckets have dealt_sizes(), low bits uniform, positions shuffled."""
    sizes, _, _ = dealt_sizes()
    lb = bits - TOP_BITS
    rng = np.random.default_rng(seed)
    top = np.repeat(np.arange(TOPS, dtype=np.uint32), sizes)
    low = rng.integers(0, 1 << lb, top.size, dtype=np.uint64).astype(np.uint32)
    return shuffled((top << np.uint32(lb)) | low, seed + 1)


LANE_PATTERNS = ("ramp", "wave_ramp", "round_blocks", "alternate")


def lane_pattern(kind, lb, m, top=5):
    """m keys of one top bucket in position order (no shuffle), low bits by position i:
    ramp          i % RAD: each digit once per RAD positions
    wave_ramp     (i // 64) % RAD: all 64 lanes of a wave step on one digit
    round_blocks  one digit for a whole 4096-key round, another for the next
    alternate     two digits alternating from lane to lane."""
    rad = 1 << lb
    i = np.arange(m, dtype=np.int64)
    if kind == "ramp":
        low = i % rad
    elif kind == "wave_ramp":
        low = (i // 64) % rad
    elif kind == "round_blocks":
        low = (7 + 3 * (i // ROUND)) % rad
    elif kind == "alternate":
        low = np.where(i % 2 == 0, 1, rad - 2)
    else:
        raise ValueError(kind)
    return (np.uint32(top << lb) | low.astype(np.uint32)).astype(np.uint32)


def edge_counts(bucket_thr):
    """The run lengths at every class edge, and bucket_thr | bucket_thr + 1 where positive."""
    counts = list(CLASS_EDGES)
    counts += [c for c in (bucket_thr, bucket_thr + 1) if c >= 1]
    return counts


def class_edges(bits, bucket_thr, spread, seed):
    """One key per entry of edge_counts, repeated that often, shuffled.  spread = False: all in top
    bucket 3 with low digits 0, 1, 2, ... (bits 14 or more: 32 digits hold them); True: key j in
    top bucket 23 j + 1, its low digit j mod 2^lb."""
    counts = edge_counts(bucket_thr)
    lb = bits - TOP_BITS
    j = np.arange(len(counts), dtype=np.uint32)
    if spread:
        vals = ((23 * j + 1) << np.uint32(lb)) | (j & np.uint32((1 << lb) - 1))
    else:
        vals = np.uint32(3 << lb) | j
    return shuffled(np.repeat(vals.astype(np.uint32), counts), seed), counts


def worst_case_list(rows, seed, bits=17, below=200_000):
    """Every run has exactly `rows` keys (an entry of LIST_MIN_ROWS, the smallest run of its
    list), n the largest multiple of `rows` below `below`: n / rows runs in one list."""
    runs = (below - 1) // rows
    vals = (np.arange(runs, dtype=np.uint64) * ((1 << bits) // runs)).astype(np.uint32)
    return shuffled(np.repeat(vals, rows), seed)


def list_capacity(lst, s):
    """Entries the engine allocates for list `lst` over s positions."""
    if lst == OVER_LIST:
        return s + 64
    return s // LIST_MIN_ROWS[lst] + 64


N_DEV_SHAPES = [(4097, 1), (5000, 2), (5000, 4096), (5000, 4097), (70_000, 1100), (600_000, 4096),
                ((1 << 20) - 1, 1500), ((1 << 20) - 1, (1 << 20) - 2)]


def below_the_bound(n_max, n_live, narrow, seed):
    """n_live uniform keys followed by a stale tail up to n_max, to be sorted on
    floor(log2 n_max) bits.  narrow: the live keys have floor(log2 n_live) bits, as a queued
    iteration's do; otherwise all the bits of the sort."""
    bits = floor_log2(n_max)
    live = uniform(n_live, floor_log2(n_live) if narrow else bits, seed)
    return with_stale_tail(live, n_max), bits
