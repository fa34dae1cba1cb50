"""ctypes binding of the C-ABI engine library (include/klsh.h -> kmerlsh_amd/lib/libklsh.so).

The library is built in-tree by ``__graft_entry__.build()`` (``make -C kmerlsh_amd/csrc``).
There is no fallback: if the library is missing, or no gfx950 device is visible, every entry point
raises.  Loading the library itself needs no GPU (the symbol checks in tests/ run on CPU).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# KLSH_LIB overrides the library path (A/B runs of engine builds; the default is the in-tree build)
LIB_PATH = os.environ.get("KLSH_LIB") or os.path.join(_HERE, "lib", "libklsh.so")
CLI_PATH = os.path.join(_HERE, "bin", "kmerLSH")

KLSH_OK = 0
ERRORS = {
    -1: "KLSH_E_ARG",
    -2: "KLSH_E_HIP",
    -3: "KLSH_E_NOMEM",
    -4: "KLSH_E_STATE",
    -5: "KLSH_E_NODEVICE",
    -6: "KLSH_E_RANGE",
}

# Every symbol include/klsh.h declares (tests/test_native_lib.py checks the .so exports them).
EXPORTED = (
    "klsh_create", "klsh_destroy", "klsh_last_error", "klsh_version", "klsh_abi_version",
    "klsh_load_rows",
    "klsh_load_counts", "klsh_snapshot", "klsh_restore", "klsh_cluster", "klsh_count",
    "klsh_result", "klsh_hash_keys", "klsh_bucket_sort", "klsh_pcluster", "klsh_hyperplanes", "klsh_fp_selftest",
    "klsh_synth_counts", "klsh_comm_unique_id", "klsh_comm_init", "klsh_comm_init_local",
    "klsh_comm_info", "klsh_set_option", "klsh_get_option", "klsh_wrs", "klsh_ttest2", "klsh_fastq_open",
    "klsh_fastq_next", "klsh_fastq_close", "klsh_kset_create", "klsh_kset_destroy",
    "klsh_check_reads", "klsh_extract_fastq", "klsh_build_khtable", "klsh_cuckoo_order",
    "klsh_kmc_info", "klsh_khtable_first", "klsh_bucket_runs", "klsh_row_state",
    "klsh_count_khtable", "klsh_kcount_listing", "klsh_count_kmc",
    "klsh_load_rows_device", "klsh_result_device", "klsh_labels",
    "klsh_load_clusters_device", "klsh_save_clusters", "klsh_kset_find", "klsh_tail_buckets",
    "klsh_diff_ksets", "klsh_parse_clust", "klsh_parse_fastq",
)


# include/klsh.h KLSH_ABI_VERSION (the structs below mirror that header)
ABI_VERSION = 3
# klsh_stats.kern indices (include/klsh.h KLSH_K_*); "merge" is a phase (KLSH_K_MERGE)
KERNEL_CLASSES = ("project", "sort", "runs", "small", "big128", "big192", "big384", "big896",
                  "huge", "tail", "compact", "screen", "merge")
KCLASSES = 13
# option "last_hash_variant" (klsh_internal.h ProjVariant): the kernel klsh_hash_keys launched
PROJ_VARIANT_NONE = -1
PROJ_VARIANT_PK = 0             # k_project_pk<D>
PROJ_VARIANT_WIDE_PK = 1        # k_project_wide_pk
PROJ_VARIANT_GENERIC = 2        # k_project_generic
PROJ_VARIANT_H16 = 3            # k_project_h16<D>
PROJ_VARIANT_MFMA_WIDE_512 = 4  # k_project_mfma_wide<512> + k_project_fix
PROJ_VARIANT_MFMA_WIDE = 5      # k_project_mfma_wide<0> + k_project_fix


class KlshKstat(ctypes.Structure):
    _fields_ = [
        ("ms", ctypes.c_double),
        ("launches", ctypes.c_uint64),
        ("rows", ctypes.c_uint64),
        ("runs", ctypes.c_uint64),
    ]


class _Sized(ctypes.Structure):
    """A statistics struct whose leading struct_size field the caller fills in."""

    def __init__(self):
        super().__init__()
        self.struct_size = ctypes.sizeof(self)

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


class KlshStats(_Sized):
    _fields_ = [
        ("struct_size", ctypes.c_uint64),
        ("iterations", ctypes.c_uint64),
        ("sum_rows", ctypes.c_uint64),
        ("sum_merges", ctypes.c_uint64),
        ("sum_proj_bits", ctypes.c_uint64),
        ("nested_calls", ctypes.c_uint64),
        ("hyperplanes", ctypes.c_uint64),
        ("n_final", ctypes.c_uint64),
        ("project_launches", ctypes.c_uint64),
        ("project_timed_launches", ctypes.c_uint64),
        ("wall_ms", ctypes.c_double),
        ("project_ms", ctypes.c_double),
        ("sort_ms", ctypes.c_double),
        ("merge_ms", ctypes.c_double),
        ("compact_ms", ctypes.c_double),
        ("host_ms", ctypes.c_double),
        ("comm_ms", ctypes.c_double),
        ("world", ctypes.c_uint64),
        ("small_ms", ctypes.c_double),
        ("small_launches", ctypes.c_uint64),
        ("small_rows", ctypes.c_uint64),
        ("small_iter_merges", ctypes.c_uint64),
        ("kern", KlshKstat * KCLASSES),
        ("proj_fix_pairs", ctypes.c_uint64),
    ]

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("kern", "struct_size")}
        d["kern"] = {name: {f: getattr(self.kern[i], f) for f, _ in KlshKstat._fields_}
                     for i, name in enumerate(KERNEL_CLASSES)}
        return d


class KlshExtractStats(_Sized):
    _fields_ = [
        ("struct_size", ctypes.c_uint64),
        ("reads", ctypes.c_uint64),
        ("bases", ctypes.c_uint64),
        ("reads_tested", ctypes.c_uint64),
        ("kmers_checked", ctypes.c_uint64),
        ("reads_extracted", ctypes.c_uint64),
        ("abnormal", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double),
        ("parse_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
    ]


class KlshKcountStats(_Sized):
    _fields_ = [
        ("struct_size", ctypes.c_uint64),
        ("kmap_size", ctypes.c_uint64),
        ("reads", ctypes.c_uint64),
        ("bases", ctypes.c_uint64),
        ("positions", ctypes.c_uint64),
        ("distinct", ctypes.c_uint64),
        ("listed", ctypes.c_uint64),
        ("batches", ctypes.c_uint64),
        ("rehashes", ctypes.c_uint64),
        ("kernel_ms", ctypes.c_double),
        ("parse_ms", ctypes.c_double),
        ("order_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
    ]


class KlshKmcdbStats(_Sized):
    _fields_ = [
        ("struct_size", ctypes.c_uint64),
        ("databases", ctypes.c_uint64),
        ("records", ctypes.c_uint64),
        ("bytes", ctypes.c_uint64),
        ("chunks", ctypes.c_uint64),
        ("prefix_len_min", ctypes.c_uint32),
        ("prefix_len_max", ctypes.c_uint32),
        ("pack_ms", ctypes.c_double),
        ("write_ms", ctypes.c_double),
    ]


class KlshSaveStats(_Sized):
    _fields_ = [
        ("struct_size", ctypes.c_uint64),
        ("clusters", ctypes.c_uint64),
        ("clusters_written", ctypes.c_uint64),
        ("members_written", ctypes.c_uint64),
        ("text_bytes", ctypes.c_uint64),
        ("bin_bytes", ctypes.c_uint64),
        ("chunks", ctypes.c_uint64),
        ("rank_ms", ctypes.c_double),
        ("format_ms", ctypes.c_double),
        ("write_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
    ]


class KlshDiffStats(_Sized):
    _fields_ = [
        ("struct_size", ctypes.c_uint64),
        ("clusters", ctypes.c_uint64),
        ("entries", ctypes.c_uint64),
        ("text_bytes", ctypes.c_uint64),
        ("tokens", ctypes.c_uint64),
        ("tested", ctypes.c_uint64),
        ("clusters_a", ctypes.c_uint64),
        ("clusters_b", ctypes.c_uint64),
        ("ids_a", ctypes.c_uint64),
        ("ids_b", ctypes.c_uint64),
        ("kmers_a", ctypes.c_uint64),
        ("kmers_b", ctypes.c_uint64),
        ("parse_path", ctypes.c_uint64),
        ("read_ms", ctypes.c_double),
        ("parse_ms", ctypes.c_double),
        ("wrs_ms", ctypes.c_double),
        ("select_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
    ]


class KlshKhtableStats(_Sized):
    _fields_ = [
        ("struct_size", ctypes.c_uint64),
        ("kmap_size", ctypes.c_uint64),
        ("records", ctypes.c_uint64),
        ("records_listed", ctypes.c_uint64),
        ("io_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("order_ms", ctypes.c_double),
    ]


class KlshError(RuntimeError):
    pass


_lib = None

_P = ctypes.c_void_p
_u64p = ctypes.POINTER(ctypes.c_uint64)


def load_library() -> ctypes.CDLL:
    """Load libklsh.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KlshError(
            f"{LIB_PATH} is missing: the gfx950 engine has no CPU fallback; "
            "build it with `python -c 'import __graft_entry__ as g; g.build()'`"
        )
    lib = ctypes.CDLL(LIB_PATH)
    sig = {
        "klsh_create": (_P, [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
        "klsh_destroy": (None, [_P]),
        "klsh_last_error": (ctypes.c_char_p, []),
        "klsh_version": (ctypes.c_char_p, []),
        "klsh_abi_version": (ctypes.c_int, []),
        "klsh_load_rows": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_int, _P, _P]),
        "klsh_load_rows_device": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_int,
                                                 ctypes.c_uint64, _P]),
        "klsh_load_clusters_device": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_int,
                                                     ctypes.c_uint64, _P, _P, ctypes.c_uint64, _P]),
        "klsh_result_device": (ctypes.c_int, [_P, _P, _P, _P, _P]),
        "klsh_labels": (ctypes.c_int, [_P, _P]),
        "klsh_save_clusters": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int,
                                              _P]),
        "klsh_load_counts": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_uint64,
                                            ctypes.c_uint64, ctypes.c_int, _P]),
        "klsh_snapshot": (ctypes.c_int, [_P]),
        "klsh_restore": (ctypes.c_int, [_P]),
        "klsh_cluster": (ctypes.c_int, [_P, ctypes.c_float, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_uint32, _u64p, _P, _P]),
        "klsh_count": (ctypes.c_int, [_P, _u64p, _u64p]),
        "klsh_result": (ctypes.c_int, [_P, _P, _P, _P]),
        "klsh_hash_keys": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_int, _P,
                                          ctypes.c_int, _P]),
        "klsh_bucket_sort": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_int, _P, _P]),
        "klsh_pcluster": (ctypes.c_int, [_P, ctypes.c_float]),
        "klsh_row_state": (ctypes.c_int, [_P, _P, _P, _P, _u64p, _u64p]),
        "klsh_bucket_runs": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_int, _u64p, _P, _P,
                                            _P]),
        "klsh_tail_buckets": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, _P, _P, _u64p, _P, _P, _P,
                                             _P]),
        "klsh_hyperplanes": (ctypes.c_int, [ctypes.c_uint32, _u64p, ctypes.c_int,
                                            ctypes.c_int, _P]),
        "klsh_fp_selftest": (ctypes.c_int, [_P, _P, _P, ctypes.c_uint64, _P, _P]),
        "klsh_synth_counts": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64,
                                             ctypes.c_uint64, ctypes.c_int, _P, _P]),
        "klsh_comm_unique_id": (ctypes.c_int, [_P]),
        "klsh_comm_init": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P]),
        "klsh_comm_init_local": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]),
        "klsh_comm_info": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(ctypes.c_int)]),
        "klsh_set_option": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_int64]),
        "klsh_get_option": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]),
        "klsh_wrs": (ctypes.c_int, [_P, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, _P,
                                    ctypes.c_float, ctypes.c_int, _P]),
        "klsh_ttest2": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P]),
        "klsh_fastq_open": (_P, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]),
        "klsh_fastq_next": (ctypes.c_int64, [_P, ctypes.c_uint64] + [ctypes.POINTER(_P)] * 6),
        "klsh_fastq_close": (None, [_P]),
        "klsh_kset_create": (_P, [_P, _P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int)]),
        "klsh_kset_destroy": (None, [_P]),
        "klsh_check_reads": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_uint64, ctypes.c_int,
                                            ctypes.c_float, _P, _P]),
        "klsh_kset_find": (ctypes.c_int, [_P, _P, _P, ctypes.c_uint64, _P, _u64p]),
        "klsh_extract_fastq": (ctypes.c_int, [_P, _P, ctypes.c_char_p, ctypes.c_char_p,
                                              ctypes.c_int, ctypes.c_float, _P]),
        "klsh_diff_ksets": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                           ctypes.POINTER(_P), ctypes.POINTER(_P), _P]),
        "klsh_parse_clust": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_int, _u64p, _P, _P,
                                            _P, _u64p, _u64p, ctypes.POINTER(ctypes.c_int)]),
        "klsh_parse_fastq": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.c_int, _u64p, _P, _P, _P,
                                            _u64p, _u64p, _u64p]),
        "klsh_build_khtable": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int,
                                              ctypes.c_int, ctypes.c_char_p, _P]),
        "klsh_cuckoo_order": (ctypes.c_int, [_P, ctypes.c_uint64, ctypes.c_int, _P]),
        "klsh_kmc_info": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), _u64p, _u64p]),
        "klsh_khtable_first": (ctypes.c_int, [_P, _P, _u64p]),
        "klsh_count_khtable": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_char_p, _P]),
        "klsh_kcount_listing": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, _u64p]),
        "klsh_count_kmc": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_char_p),
                                          ctypes.POINTER(ctypes.c_char_p), ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_char_p, _P, _P]),
    }
    for name, (res, args) in sig.items():
        if os.environ.get("KLSH_LIB") and not hasattr(lib, name):
            continue  # an A/B build of an older engine: entry points it predates stay unbound
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    # every library is checked, the KLSH_LIB ones (diagnostics / A/B builds, the likeliest to be
    # stale) too; KLSH_ABI_ANY=1 turns the refusal into a warning for an older A/B build, whose
    # calls with statistics structs then fail on their struct_size check instead
    if hasattr(lib, "klsh_abi_version") and lib.klsh_abi_version() != ABI_VERSION:
        msg = (f"{os.environ.get('KLSH_LIB') or LIB_PATH}: ABI version {lib.klsh_abi_version()}, "
               f"this binding mirrors {ABI_VERSION}: rebuild the library")
        if os.environ.get("KLSH_ABI_ANY") != "1":
            raise KlshError(msg)
        import warnings

        warnings.warn(msg)
    _lib = lib
    return lib


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _torch_if_tensor(x):
    """The torch module if x is a torch tensor, else None.  torch is never imported here: an
    object can only be a tensor if its creator imported torch already."""
    import sys

    torch = sys.modules.get("torch")
    return torch if torch is not None and isinstance(x, torch.Tensor) else None


def _check(rc: int, what: str) -> None:
    if rc != KLSH_OK:
        msg = load_library().klsh_last_error().decode(errors="replace")
        raise KlshError(f"{what} failed: {ERRORS.get(rc, rc)}: {msg}")


def hyperplanes(seed: int, counter: int, h: int, d: int) -> tuple[np.ndarray, int]:
    """LSH::generateHashTable under the seeding convention (host; no GPU needed)."""
    lib = load_library()
    out = np.zeros((max(h, 0), d), dtype=np.float32)
    c = ctypes.c_uint64(counter)
    _check(lib.klsh_hyperplanes(seed, ctypes.byref(c), h, d, _ptr(out)), "klsh_hyperplanes")
    return out, c.value


def comm_unique_id() -> bytes:
    """128-byte RCCL id for klsh_comm_init (create on rank 0, ship to the others)."""
    lib = load_library()
    buf = (ctypes.c_uint8 * 128)()
    _check(lib.klsh_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p)), "klsh_comm_unique_id")
    return bytes(buf)


def comm_init_local(engines) -> None:
    """Bind Engines into one in-process sharded group (each must then run on its own thread)."""
    lib = load_library()
    arr = (ctypes.c_void_p * len(engines))(*[e._ctx for e in engines])
    _check(lib.klsh_comm_init_local(arr, len(engines)), "klsh_comm_init_local")


def cuckoo_order(images: np.ndarray, k: int) -> tuple[np.ndarray, int]:
    """The reference's libcuckoo table order of distinct k-mer images inserted in the given order
    (host): (index of each table element in iteration order, final hash power)."""
    lib = load_library()
    im = np.ascontiguousarray(images, np.uint64)
    out = np.zeros(im.size, np.uint32)
    hp = lib.klsh_cuckoo_order(_ptr(im), im.size, k, _ptr(out))
    if hp < 0:
        _check(hp, "klsh_cuckoo_order")
    return out, int(hp)


def kmc_info(name: str) -> tuple[int, int, int]:
    """The host parse of <name>.kmc_pre (no GPU needed): (k, total records, LUT entries)."""
    lib = load_library()
    k = ctypes.c_int(0)
    total = ctypes.c_uint64(0)
    lut = ctypes.c_uint64(0)
    _check(lib.klsh_kmc_info(name.encode(), ctypes.byref(k), ctypes.byref(total), ctypes.byref(lut)),
           "klsh_kmc_info")
    return k.value, total.value, lut.value


def synth_counts(n: int, d: int, seed: int, genomes: int = 0, threads: int = 0):
    """klsh-synth v1 (host): sample-major (d, n) uint16 counts and per-sample coverage."""
    lib = load_library()
    counts = np.empty((d, n), dtype=np.uint16)
    cov = np.empty(d, dtype=np.float64)
    _check(lib.klsh_synth_counts(n, d, seed, genomes, threads, _ptr(counts), _ptr(cov)),
           "klsh_synth_counts")
    return counts, cov


def ttest2(x: np.ndarray, y: np.ndarray) -> tuple[float, float, float]:
    """alglib::studentttest2 as AB::WRS calls it (host restatement): (both, left, right) tails."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float64)
    y = np.ascontiguousarray(y, np.float64)
    out = np.zeros(3, np.float64)
    base = out.ctypes.data
    _check(lib.klsh_ttest2(_ptr(x), x.size, _ptr(y), y.size, base, base + 8, base + 16),
           "klsh_ttest2")
    return float(out[0]), float(out[1]), float(out[2])


def wrs(centroids: np.ndarray, member_counts: np.ndarray, n1: int, n2: int, pvalue_thresh: float,
        size_thresh: int) -> np.ndarray:
    """AB::WRS over every cluster (host): uint8 group per cluster, 1 = group A, 2 = group B."""
    lib = load_library()
    c = np.ascontiguousarray(centroids, np.float32).reshape(-1, n1 + n2) if n1 + n2 else \
        np.zeros((len(member_counts), 0), np.float32)
    mc = np.ascontiguousarray(member_counts, np.uint64)
    g = np.zeros(mc.size, np.uint8)
    _check(lib.klsh_wrs(_ptr(c), mc.size, n1, n2, _ptr(mc), ctypes.c_float(pvalue_thresh),
                        int(size_thresh), _ptr(g)), "klsh_wrs")
    return g


def fastq_records(path: str, batch: int = 1 << 16):
    """Every record of a FASTQ(.gz) as the reference's FastqFile/kseq reads it (host):
    a list of (name, seq, qual) byte strings."""
    lib = load_library()
    err = ctypes.c_int(0)
    f = lib.klsh_fastq_open(path.encode(), ctypes.byref(err))
    if not f:
        _check(err.value or -1, "klsh_fastq_open")
    out = []
    try:
        while True:
            ptrs = [_P() for _ in range(6)]
            n = lib.klsh_fastq_next(f, batch, *[ctypes.byref(p) for p in ptrs])
            if n < 0:
                _check(int(n), "klsh_fastq_next")
            if n == 0:
                break
            offs = [np.ctypeslib.as_array(ctypes.cast(ptrs[i], ctypes.POINTER(ctypes.c_uint64)),
                                          shape=(n + 1,)).copy() for i in (1, 3, 5)]
            blobs = [ctypes.string_at(ptrs[i], int(o[-1])) if o[-1] else b""
                     for i, o in zip((0, 2, 4), offs)]
            so, no, qo = offs
            sb, nb, qb = blobs
            for r in range(n):
                out.append((nb[no[r]:no[r + 1]], sb[so[r]:so[r + 1]], qb[qo[r]:qo[r + 1]]))
    finally:
        lib.klsh_fastq_close(f)
    return out


class KmerSet:
    """A differential k-mer set on an Engine's device (``klsh_kset``)."""

    def __init__(self, engine: "Engine", kmers: np.ndarray):
        self._lib = engine._lib
        self.engine = engine
        k = np.ascontiguousarray(kmers, np.uint64)
        err = ctypes.c_int(0)
        self._set = self._lib.klsh_kset_create(engine._ctx, _ptr(k), k.size, ctypes.byref(err))
        if not self._set:
            _check(err.value or -2, "klsh_kset_create")
        self.size = k.size

    @classmethod
    def adopt(cls, engine: "Engine", handle, size: int) -> "KmerSet":
        """A set around a ``klsh_kset*`` the library made on `engine` (``klsh_diff_ksets``); the
        object owns the handle from here on.  `size`: the keys it was built from."""
        ks = cls.__new__(cls)  # (no klsh_kset_create: the library made the set)
        ks._lib, ks.engine = engine._lib, engine
        ks._set = handle
        ks.size = int(size)
        return ks

    def close(self) -> None:
        if getattr(self, "_set", None):
            self._lib.klsh_kset_destroy(self._set)
            self._set = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check_reads(self, seqs, k: int, kmer_vote: float):
        """IOFQ::CheckRead on the GPU: (hits uint32, flags uint8) per read (bytes sequences)."""
        blob = b"".join(seqs)
        off = np.zeros(len(seqs) + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
        buf = np.frombuffer(blob + b"\0", np.uint8)
        hits = np.zeros(len(seqs), np.uint32)
        flags = np.zeros(len(seqs), np.uint8)
        _check(self._lib.klsh_check_reads(self.engine._ctx, self._set, _ptr(buf), _ptr(off),
                                          len(seqs), k, ctypes.c_float(kmer_vote), _ptr(hits),
                                          _ptr(flags)), "klsh_check_reads")
        return hits, flags

    def find(self, keys: np.ndarray) -> tuple[np.ndarray, int]:
        """Where the set's table keeps each key (``klsh_kset_find``, a test hook): (slot per key as
        uint64, all ones = absent; the table's slot count)."""
        k = np.ascontiguousarray(keys, np.uint64)
        slots = np.zeros(k.size, np.uint64)
        n_slots = ctypes.c_uint64(0)
        _check(self._lib.klsh_kset_find(self.engine._ctx, self._set, _ptr(k), k.size, _ptr(slots),
                                        ctypes.byref(n_slots)), "klsh_kset_find")
        return slots, int(n_slots.value)

    def extract_fastq(self, in_path: str, out_path: str, k: int, kmer_vote: float) -> dict:
        """IOFQ::ReadExtract for one sample (host parse + GPU vote + writer)."""
        st = KlshExtractStats()
        _check(self._lib.klsh_extract_fastq(self.engine._ctx, self._set, in_path.encode(),
                                            out_path.encode(), k, ctypes.c_float(kmer_vote),
                                            ctypes.byref(st)), "klsh_extract_fastq")
        return st.as_dict()


def diff_ksets(engine: "Engine", clust_path: str, kmer_set_path: str, kmap: int, n1: int, n2: int,
               pval: float, size_thresh: int) -> tuple[KmerSet, KmerSet, dict]:
    """The cluster files <clust_path> / <clust_path>.clust to the two differential k-mer sets
    (``klsh_diff_ksets``): (set A, set B, statistics)."""
    lib = engine._lib
    a, b = _P(), _P()
    st = KlshDiffStats()
    _check(lib.klsh_diff_ksets(engine._ctx, os.fsencode(clust_path), os.fsencode(kmer_set_path),
                               int(kmap), int(n1), int(n2), ctypes.c_float(pval), int(size_thresh),
                               ctypes.byref(a), ctypes.byref(b), ctypes.byref(st)),
           "klsh_diff_ksets")
    return (KmerSet.adopt(engine, a.value, st.kmers_a), KmerSet.adopt(engine, b.value, st.kmers_b),
            st.as_dict())


def parse_clust(engine: "Engine", text: bytes, path: int = 0, ids: bool = True) -> dict:
    """``klsh_parse_clust`` (a test hook): the text of a .clust file parsed by the kernels
    (path 2), the host parser (1) or whichever ``klsh_diff_ksets`` would take (0).  Returns
    n_lines, n_ids, irregular_at (None if the text is regular), path_used and, with `ids`, counts,
    offsets and ids (uint64 arrays); without, the size query alone."""
    lib = engine._lib
    buf = np.frombuffer(bytes(text) + b"\0", np.uint8)
    n_lines, n_ids, irr = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    used = ctypes.c_int(-1)

    def call(counts, offsets, idv):
        _check(lib.klsh_parse_clust(engine._ctx, _ptr(buf), len(text), int(path),
                                    ctypes.byref(n_lines), _ptr(counts), _ptr(offsets), _ptr(idv),
                                    ctypes.byref(n_ids), ctypes.byref(irr), ctypes.byref(used)),
               "klsh_parse_clust")

    call(None, None, None)
    out = {}
    if ids:
        nl, ni = n_lines.value, n_ids.value  # (one entry at least: no empty array's NULL pointer)
        counts, offsets, idv = (np.zeros(max(n, 1), np.uint64) for n in (nl, nl + 1, ni))
        call(counts, offsets, idv)
        out.update(counts=counts[:nl], offsets=offsets[:nl + 1], ids=idv[:ni])
    out.update(n_lines=int(n_lines.value), n_ids=int(n_ids.value), path_used=int(used.value),
               irregular_at=None if irr.value == 2**64 - 1 else int(irr.value))
    return out


def parse_fastq(engine: "Engine", data: bytes, path: int = 0, seq_capacity: int | None = None) -> dict:
    """``klsh_parse_fastq`` (a test hook): one chunk of plain FASTQ parsed by the kernels (path 0)
    or read by the host reader (path 1).  Returns n_records, line_starts (uint32, 4 n + 1), seq_off
    (uint64, n + 1), seq (bytes), consumed and irregular_at (None if nothing is irregular).
    seq_capacity: None = a size query (NULL arrays) and then the call with arrays of those sizes;
    a number = one call with a sequence buffer of that many bytes and offset arrays for as many
    records as the data can hold."""
    lib = engine._lib
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
    n, cap, used, irr = (ctypes.c_uint64(0) for _ in range(4))

    def call(lines, off, seq):
        _check(lib.klsh_parse_fastq(engine._ctx, _ptr(buf), len(data), int(path), ctypes.byref(n),
                                    _ptr(lines), _ptr(off), _ptr(seq), ctypes.byref(cap),
                                    ctypes.byref(used), ctypes.byref(irr)), "klsh_parse_fastq")

    if seq_capacity is None:
        call(None, None, None)
        nr, nb = n.value, cap.value
    else:  # (the reader reads a record per header line at most, and one without any)
        nr, nb = bytes(data).count(b"\n") + 1, int(seq_capacity)
    # (one entry more: no empty array's NULL pointer)
    lines, off, seq = np.zeros(4 * nr + 1, np.uint32), np.zeros(nr + 1, np.uint64), np.zeros(nb + 1, np.uint8)
    cap.value = nb
    call(lines, off, seq)
    nr, nb = n.value, cap.value
    return dict(n_records=int(nr), line_starts=lines[:4 * nr + 1], seq_off=off[:nr + 1],
                seq=seq[:nb].tobytes(), consumed=int(used.value),
                irregular_at=None if irr.value == 2**64 - 1 else int(irr.value))


class Engine:
    """One device context (``klsh_ctx``)."""

    def __init__(self, device: int = 0):
        lib = load_library()
        err = ctypes.c_int(0)
        self._ctx = lib.klsh_create(device, ctypes.byref(err))
        if not self._ctx:
            _check(err.value or -2, "klsh_create")
        self._lib = lib
        self.device = device
        self.d = 0

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.klsh_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- loading
    def load_rows(self, rows, member_offsets: np.ndarray | None = None,
                  member_ids: np.ndarray | None = None) -> None:
        """Rows as a numpy array, or as a torch tensor (float32, 2-D, last-dimension stride 1, any
        row stride >= d): one on this engine's GPU is read where it is (klsh_load_rows_device,
        every row a singleton), a CPU tensor goes the numpy way, any other device raises."""
        torch = _torch_if_tensor(rows)
        if torch is not None:
            if rows.device.type == "cpu":
                rows = rows.detach().numpy()
            else:
                return self._load_rows_tensor(torch, rows, member_offsets, member_ids)
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        n, d = rows.shape
        mo = None if member_offsets is None else np.ascontiguousarray(member_offsets, np.uint64)
        mi = None if member_ids is None else np.ascontiguousarray(member_ids, np.uint64)
        _check(self._lib.klsh_load_rows(self._ctx, _ptr(rows), n, d, _ptr(mo), _ptr(mi)),
               "klsh_load_rows")
        self.d = d

    def _torch_device(self, torch):
        return torch.device("cuda", self.device)

    def _load_rows_tensor(self, torch, rows, member_offsets, member_ids) -> None:
        if rows.device != self._torch_device(torch):
            raise KlshError(f"load_rows: the tensor is on {rows.device}, this engine on "
                            f"{self._torch_device(torch)}")
        if member_offsets is not None:
            raise KlshError("load_rows: a device tensor is loaded as singleton rows "
                            "(member_offsets must be None)")
        if rows.dtype != torch.float32 or rows.dim() != 2:
            raise KlshError("load_rows: the tensor must be float32 and 2-D")
        n, d = rows.shape
        if (d > 1 and rows.stride(1) != 1) or (n > 1 and rows.stride(0) < d):
            raise KlshError("load_rows: the tensor needs last-dimension stride 1 and a row "
                            f"stride >= d (strides {tuple(rows.stride())})")
        stride = rows.stride(0) if n > 1 else d
        mi = None if member_ids is None else np.ascontiguousarray(member_ids, np.uint64)
        if mi is not None and mi.size != n:
            raise KlshError("load_rows: one member id per row")
        torch.cuda.current_stream(rows.device).synchronize()  # the caller's writes are complete
        _check(self._lib.klsh_load_rows_device(self._ctx, ctypes.c_void_p(rows.data_ptr()), n, d,
                                               stride, _ptr(mi)), "klsh_load_rows_device")
        self.d = d

    def load_clusters(self, rows, member_offsets, member_nodes=None, n_nodes: int | None = None,
                      member_ids: np.ndarray | None = None) -> None:
        """Rows with their member lists, all on this engine's GPU (``klsh_load_clusters_device``):
        rows as in load_rows (float32, 2-D, last-dimension stride 1, row stride >= d),
        member_offsets (n + 1) and member_nodes (or None: entry q is node q - offsets[0]) 1-D
        contiguous uint32 or int32 tensors; row i holds nodes[offsets[i]:offsets[i + 1]], so a
        slice ``off[a:b + 1]`` goes with the whole node tensor.  n_nodes=None keeps the node
        space and the ids of the current load (the round trip of result_device()); n_nodes=M
        starts a new one, member_ids (numpy uint64 on the host, M entries, or None = k) its
        ids."""
        torch = _torch_if_tensor(rows)
        if torch is None:
            raise KlshError("load_clusters: rows must be a torch tensor on the engine's GPU")
        dev = self._torch_device(torch)
        if rows.device != dev:
            raise KlshError(f"load_clusters: the tensor is on {rows.device}, this engine on {dev}")
        if rows.dtype != torch.float32 or rows.dim() != 2:
            raise KlshError("load_clusters: the rows must be float32 and 2-D")
        n, d = rows.shape
        if (d > 1 and rows.stride(1) != 1) or (n > 1 and rows.stride(0) < d):
            raise KlshError("load_clusters: the rows need last-dimension stride 1 and a row "
                            f"stride >= d (strides {tuple(rows.stride())})")
        stride = rows.stride(0) if n > 1 else d
        for name, t in (("member_offsets", member_offsets), ("member_nodes", member_nodes)):
            if t is None and name == "member_nodes":
                continue
            if (_torch_if_tensor(t) is None or t.device != dev or t.dim() != 1 or
                    not t.is_contiguous() or t.dtype not in (torch.uint32, torch.int32)):
                raise KlshError(f"load_clusters: {name} must be a 1-D contiguous uint32 or int32 "
                                f"tensor on {dev}")
        if member_offsets.numel() != n + 1:
            raise KlshError("load_clusters: member_offsets needs one entry per row and one more")
        if n_nodes is None and member_ids is not None:
            raise KlshError("load_clusters: member_ids belong to a new node space (give n_nodes)")
        if n_nodes is not None and n_nodes <= 0:
            raise KlshError("load_clusters: n_nodes must be positive (None keeps the loaded nodes)")
        mi = None if member_ids is None else np.ascontiguousarray(member_ids, np.uint64)
        if mi is not None and mi.size != n_nodes:
            raise KlshError("load_clusters: one member id per node")

        def p(t):
            return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

        torch.cuda.current_stream(dev).synchronize()  # the caller's writes are complete
        _check(self._lib.klsh_load_clusters_device(self._ctx, p(rows), n, d, stride,
                                                   p(member_offsets), p(member_nodes),
                                                   n_nodes or 0, _ptr(mi)),
               "klsh_load_clusters_device")
        self.d = d

    def load_counts(self, counts: np.ndarray, v_kmers: np.ndarray, batch_offset: int = 0,
                    batch_size: int | None = None) -> None:
        counts = np.ascontiguousarray(counts, dtype=np.uint16)
        d, n_total = counts.shape
        if batch_size is None:
            batch_size = n_total - batch_offset
        vk = np.ascontiguousarray(v_kmers, dtype=np.float32)
        _check(self._lib.klsh_load_counts(self._ctx, _ptr(counts), n_total, batch_offset,
                                          batch_size, d, _ptr(vk)), "klsh_load_counts")
        self.d = d

    def comm_init(self, rank: int, world: int, uid: bytes) -> None:
        """Join the RCCL group `uid` as `rank` of `world` (one process per GPU)."""
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        _check(self._lib.klsh_comm_init(self._ctx, rank, world, ctypes.cast(buf, ctypes.c_void_p)),
               "klsh_comm_init")

    def set_option(self, name: str, value: int) -> None:
        _check(self._lib.klsh_set_option(self._ctx, name.encode(), int(value)), "klsh_set_option")

    def get_option(self, name: str) -> int:
        v = ctypes.c_int64(0)
        _check(self._lib.klsh_get_option(self._ctx, name.encode(), ctypes.byref(v)),
               "klsh_get_option")
        return v.value

    def comm_info(self) -> tuple[int, int]:
        r = ctypes.c_int(0)
        w = ctypes.c_int(1)
        _check(self._lib.klsh_comm_info(self._ctx, ctypes.byref(r), ctypes.byref(w)),
               "klsh_comm_info")
        return r.value, w.value

    def snapshot(self) -> None:
        _check(self._lib.klsh_snapshot(self._ctx), "klsh_snapshot")

    def restore(self) -> None:
        _check(self._lib.klsh_restore(self._ctx), "klsh_restore")

    # ---- hot path
    def cluster(self, min_similarity: float, iterations: int, bucket_size_threshold: int,
                seed: int = 12345, counter: int = 0):
        """Returns (trace of N_t, new rng counter, stats dict)."""
        c = ctypes.c_uint64(counter)
        trace = np.zeros(max(iterations, 1), dtype=np.uint64)
        st = KlshStats()
        _check(self._lib.klsh_cluster(self._ctx, ctypes.c_float(min_similarity), iterations,
                                      bucket_size_threshold, seed, ctypes.byref(c), _ptr(trace),
                                      ctypes.byref(st)), "klsh_cluster")
        return trace[: st.iterations], c.value, st.as_dict()

    def build_khtable(self, kmc_names, k: int, out_dir: str = "") -> dict:
        """Mode B: kmer_set.hex / kmer_count.bin / kmer_count.log from KMC databases."""
        arr = (ctypes.c_char_p * len(kmc_names))(*[n.encode() for n in kmc_names])
        st = KlshKhtableStats()
        _check(self._lib.klsh_build_khtable(self._ctx, arr, len(kmc_names), k, out_dir.encode(),
                                            ctypes.byref(st)), "klsh_build_khtable")
        return st.as_dict()

    def count_khtable(self, fastq_paths, k: int, count_min: int = 2, out_dir: str = "") -> dict:
        """Mode K: kmer_set.hex / kmer_count.bin / kmer_count.log from one FASTQ file per sample
        (k-mers counted on the GPU, listed from count_min occurrences on)."""
        arr = (ctypes.c_char_p * len(fastq_paths))(*[os.fspath(n).encode() for n in fastq_paths])
        st = KlshKcountStats()
        _check(self._lib.klsh_count_khtable(self._ctx, arr, len(fastq_paths), k, count_min,
                                            os.fspath(out_dir).encode(), ctypes.byref(st)),
               "klsh_count_khtable")
        return st.as_dict()

    def count_kmc(self, fastq_paths, db_names, k: int, count_min: int = 2,
                  out_dir=None) -> tuple[dict, dict]:
        """Mode K with its databases: sample j's listing written as the KMC database
        db_names[j] (.kmc_pre / .kmc_suf, what build_khtable reads), and, unless out_dir is None,
        the three table files in out_dir as count_khtable writes them.  db_names None: only the
        table.  Returns (counting statistics, database statistics)."""
        arr = (ctypes.c_char_p * len(fastq_paths))(*[os.fspath(n).encode() for n in fastq_paths])
        dbs = None
        if db_names is not None:
            if len(db_names) != len(fastq_paths):
                raise ValueError("one database name per FASTQ file")
            # None stays a NULL entry (the library refuses it)
            dbs = (ctypes.c_char_p * len(db_names))(
                *[None if n is None else os.fspath(n).encode() for n in db_names])
        st, dst = KlshKcountStats(), KlshKmcdbStats()
        _check(self._lib.klsh_count_kmc(self._ctx, arr, dbs, len(fastq_paths), k, count_min,
                                        None if out_dir is None else os.fspath(out_dir).encode(),
                                        ctypes.byref(st), ctypes.byref(dst)), "klsh_count_kmc")
        return st.as_dict(), dst.as_dict()

    def kcount_listing(self, sample: int) -> tuple[np.ndarray, np.ndarray]:
        """Sample `sample`'s listing of the last count_khtable made with option
        "kcount_keep_listing" on (a test hook): (KMC values ascending, counts)."""
        n = ctypes.c_uint64(0)
        _check(self._lib.klsh_kcount_listing(self._ctx, sample, None, None, ctypes.byref(n)),
               "klsh_kcount_listing")
        vals, cnts = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint32)
        _check(self._lib.klsh_kcount_listing(self._ctx, sample, _ptr(vals), _ptr(cnts),
                                             ctypes.byref(n)), "klsh_kcount_listing")
        return vals, cnts

    def khtable_first(self) -> np.ndarray:
        """The first-appearance list of the last build_khtable made with option "kmc_keep_first"
        on (a test hook): distinct canonical k-mer images by first (sample, record) ordinal."""
        n = ctypes.c_uint64(0)
        _check(self._lib.klsh_khtable_first(self._ctx, None, ctypes.byref(n)), "klsh_khtable_first")
        out = np.zeros(n.value, np.uint64)
        _check(self._lib.klsh_khtable_first(self._ctx, _ptr(out), ctypes.byref(n)),
               "klsh_khtable_first")
        return out

    def pcluster(self, thr: float) -> None:
        _check(self._lib.klsh_pcluster(self._ctx, ctypes.c_float(thr)), "klsh_pcluster")

    def hash_keys(self, rows: np.ndarray, table: np.ndarray) -> np.ndarray:
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        table = np.ascontiguousarray(table, dtype=np.float32)
        n, d = rows.shape
        h = table.shape[0]
        keys = np.zeros(n, dtype=np.uint32)
        _check(self._lib.klsh_hash_keys(self._ctx, _ptr(rows), n, d, _ptr(table), h,
                                        _ptr(keys)), "klsh_hash_keys")
        return keys

    def bucket_sort(self, keys: np.ndarray, bits: int):
        """merge_hashtable's stable bucket order on the GPU: (sorted keys, permutation)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        out = np.zeros_like(keys)
        perm = np.zeros_like(keys)
        _check(self._lib.klsh_bucket_sort(self._ctx, _ptr(keys), keys.size, bits, _ptr(out),
                                          _ptr(perm)), "klsh_bucket_sort")
        return out, perm

    def bucket_runs(self, sorted_keys: np.ndarray, bucket_thr: int):
        """The merge step's runs of equal sorted keys: (starts, lengths, lists), start order."""
        k = np.ascontiguousarray(sorted_keys, dtype=np.uint32)
        cap = k.size // 2 + 1
        st = np.zeros(cap, np.uint32)
        ln = np.zeros(cap, np.uint32)
        li = np.zeros(cap, np.int32)
        nr = ctypes.c_uint64(cap)
        _check(self._lib.klsh_bucket_runs(self._ctx, _ptr(k), k.size, int(bucket_thr),
                                          ctypes.byref(nr), _ptr(st), _ptr(ln), _ptr(li)),
               "klsh_bucket_runs")
        m = nr.value
        return st[:m], ln[:m], li[:m]

    def tail_buckets(self, keys: np.ndarray, n_live: int, bits: int, bucket_thr: int, path: int):
        """One queued iteration's sort and run listing on caller keys (klsh_tail_buckets): grids
        for keys.size, the count n_live on the device, path 1 = k_tail_local, 0 = LSD + run
        kernels.  Returns (keys, perm) of all keys.size entries, (starts, lengths, lists) in start
        order and the seven counters (heads, small rows, rows of lists 6..9, huge rows)."""
        k = np.ascontiguousarray(keys, dtype=np.uint32)
        out = np.zeros_like(k)
        perm = np.zeros_like(k)
        cap = k.size + 1  # (a threshold of 0 lists the runs of one row as oversize)
        st = np.zeros(cap, np.uint32)
        ln = np.zeros(cap, np.uint32)
        li = np.zeros(cap, np.int32)
        ctr = np.zeros(7, np.uint32)
        nr = ctypes.c_uint64(cap)
        _check(self._lib.klsh_tail_buckets(self._ctx, _ptr(k), k.size, int(n_live), int(bits),
                                           int(bucket_thr), int(path), _ptr(out), _ptr(perm),
                                           ctypes.byref(nr), _ptr(st), _ptr(ln), _ptr(li),
                                           _ptr(ctr)), "klsh_tail_buckets")
        m = nr.value
        return out, perm, (st[:m], ln[:m], li[:m]), ctr

    def fp_selftest(self, a: np.ndarray, b: np.ndarray):
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        s = np.zeros_like(a)
        q = np.zeros_like(a)
        _check(self._lib.klsh_fp_selftest(self._ctx, _ptr(a), _ptr(b), a.size, _ptr(s), _ptr(q)),
               "klsh_fp_selftest")
        return s, q

    # ---- results
    def count(self) -> tuple[int, int]:
        n = ctypes.c_uint64(0)
        m = ctypes.c_uint64(0)
        _check(self._lib.klsh_count(self._ctx, ctypes.byref(n), ctypes.byref(m)), "klsh_count")
        return n.value, m.value

    def result(self):
        """(rows (n, d) float32, member_offsets (n+1,) uint64, member_ids (m,) uint64)."""
        n, m = self.count()
        rows = np.zeros((n, self.d), dtype=np.float32)
        off = np.zeros(n + 1, dtype=np.uint64)
        ids = np.zeros(m, dtype=np.uint64)
        _check(self._lib.klsh_result(self._ctx, _ptr(rows), _ptr(off), _ptr(ids)),
               "klsh_result")
        return rows, off, ids

    def result_device(self):
        """The result left on this engine's GPU, as torch tensors (``klsh_result_device``):
        (rows (n, d) float32, member_offsets (n+1,) uint32, member_nodes (m,) uint32, labels (M,)
        uint32).  Nodes number the loaded members in load order; labels[k] is the row of node k,
        0xFFFFFFFF for a node no live row holds (include/klsh.h)."""
        import torch

        dev = self._torch_device(torch)
        n = ctypes.c_uint64(0)
        _check(self._lib.klsh_count(self._ctx, ctypes.byref(n), None), "klsh_count")
        n, big_m = n.value, self.get_option("member_nodes")
        rows = torch.empty((n, self.d), dtype=torch.float32, device=dev)
        off = torch.empty(n + 1, dtype=torch.uint32, device=dev)
        nodes = torch.empty(big_m, dtype=torch.uint32, device=dev)  # (the live members: <= M)
        labels = torch.empty(big_m, dtype=torch.uint32, device=dev)
        # the engine writes on its own stream: nothing queued on torch's may still use this memory
        torch.cuda.current_stream(dev).synchronize()

        def p(t):
            return ctypes.c_void_p(t.data_ptr()) if t.numel() else None

        _check(self._lib.klsh_result_device(self._ctx, p(rows), p(off), p(nodes), p(labels)),
               "klsh_result_device")
        return rows, off, nodes[: int(off[-1].item())], labels

    def save_clusters(self, clust_path, bin_path=None, ignore_small: int = 5) -> dict:
        """The reference's two cluster files written from the device (``klsh_save_clusters``):
        clust_path gets a text line "count<TAB>id..." per live row with more than ignore_small
        members, bin_path those rows' float32 values; either may be None.  Returns the call's
        statistics (include/klsh.h klsh_save_stats)."""
        st = KlshSaveStats()
        _check(self._lib.klsh_save_clusters(
            self._ctx, None if clust_path is None else os.fspath(clust_path).encode(),
            None if bin_path is None else os.fspath(bin_path).encode(), int(ignore_small),
            ctypes.byref(st)), "klsh_save_clusters")
        return st.as_dict()

    def labels(self) -> np.ndarray:
        """labels[k] = the result row whose member list holds node k (``klsh_labels``), uint32,
        0xFFFFFFFF for a node no live row holds."""
        out = np.zeros(self.get_option("member_nodes"), dtype=np.uint32)
        _check(self._lib.klsh_labels(self._ctx, _ptr(out)), "klsh_labels")
        return out

    def row_state(self) -> dict:
        """The cached per-slot state of the live rows, in result() order (``klsh_row_state``):
        nrm (n,) float32, cnt (n,) uint32, image (n, d) uint16 fp16 bits or None when no image is
        kept, and the host-computed counters pad_nonzero and bad_links."""
        n, _ = self.count()
        nrm = np.zeros(n, dtype=np.float32)
        cnt = np.zeros(n, dtype=np.uint32)
        image = np.zeros((n, self.d), dtype=np.uint16) if self.get_option("fp16_image") else None
        pad = ctypes.c_uint64(0)
        bad = ctypes.c_uint64(0)
        _check(self._lib.klsh_row_state(self._ctx, _ptr(nrm), _ptr(cnt), _ptr(image),
                                        ctypes.byref(pad), ctypes.byref(bad)), "klsh_row_state")
        return {"nrm": nrm, "cnt": cnt, "image": image, "pad_nonzero": pad.value,
                "bad_links": bad.value}
