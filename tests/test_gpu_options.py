"""klsh_set_option / klsh_get_option: every name, its default, its range and its message.

The tables below were recorded from the library as it was before the options moved into one
table (the two if-chains of the single-file host engine), on a context with nothing loaded; the
test passes unchanged against that library and against the table.  Each settable name has its
default, one accepted value with what reads back afterwards, and, where a range exists, one
refused value with its message.  The context is this module's own, so the session's engines keep
their options.
"""
import re

import pytest

from kmerlsh_amd import _native

pytestmark = pytest.mark.gpu

GRID = r"%s must be in \[0, 2\^20\]"
ZERO_ONE = r"%s must be 0 or 1"
AT_LEAST_0 = r"%s must be >= 0"

# name: (default, accepted value, its read-back, refused value or None, message pattern or None)
SETTABLE = {
    "shard_min_rows": (1 << 21, 12345, 12345, -1, AT_LEAST_0),
    # flags: any non-zero value switches them on
    "phase_timing": (0, 5, 1, None, None),
    "kernel_timing": (1, 0, 0, None, None),
    "tail_batch": (1, 0, 0, None, None),
    "huge_fold": (0, 3, 1, None, None),
    "tail_local": (1, 0, 0, None, None),
    "kmc_keep_first": (0, 9, 1, None, None),
    "kcount_keep_listing": (0, 9, 1, None, None),
    "result_device": (0, 1, 1, 2, ZERO_ONE),
    "hyperplane_async": (1, 0, 0, 2, ZERO_ONE),
    "hyperplane_window": (0, 4096, 4096, -1, AT_LEAST_0),
    "progress": (0, 25, 25, 1 << 31, AT_LEAST_0),
    "stop_after": (0, 3, 3, -1, r"%s must be in \[0, 2\^31\)"),
    # (nothing is loaded: neither setter has anything to allocate or rebuild)
    "projection": (0, 1, 1, 2, r"%s must be 0 \(default\) or 1 \(exact packed chains\)"),
    "long_runs": (4, 0, 0, 2, r"%s must be 0, 1 or 4"),
    "wide_gram": (32, 16, 16, 7, r"%s must be 0, 8, 16, 32 or 64"),
    "wide_unrolled": (1, 0, 0, 2, ZERO_ONE),
    "h16_bound": (1, 0, 0, 2, ZERO_ONE),
    "comm_timeout_s": (600, 30, 30, 0, r"%s must be > 0"),
    "kmc_chunk_records": (0, 1000, 1000, -1, AT_LEAST_0),
    "kmc_ordinal_base": (0, 77, 77, (1 << 48) + 1, r"%s must be in \[0, 2\^48\]"),
    "kcount_batch_reads": (0, 100, 100, -1, AT_LEAST_0),
    "kcount_table_slots": (0, 2048, 2048, 1000,
                           r"%s must be 0 or a power of two in \[1024, 2\^32\]"),
    "kcount_db_prefix": (-1, 5, 5, 16, r"%s must be in \[-1, 15\]"),
    "kcount_db_chunk_records": (0, 1000, 1000, -1, AT_LEAST_0),
    "h16_grid": (0, 3, 3, (1 << 20) + 1, GRID),
    "h16_segcap": (0, 3, 3, -1, GRID),
    "wide_grid": (0, 3, 3, (1 << 20) + 1, GRID),
    "fix_grid": (0, 3, 3, -1, GRID),
    "small_grid": (0, 3, 3, (1 << 20) + 1, GRID),
    "tail_big_groups": (0, 3, 3, -1, GRID),
    "tail_small_groups": (0, 3, 3, (1 << 20) + 1, GRID),
    "wide_group_grid": (0, 3, 3, -1, GRID),
    "small_screen_grid": (0, 3, 3, (1 << 20) + 1, GRID),
    "grid_cap": (0, 3, 3, (1 << 20) + 1, GRID),
    "tail_screen_grid": (0, 3, 3, -1, GRID),
    # reads back resolved: 0 (the default) as the size it stands for
    "tail_merge_rows": (1 << 22, 4096, 4096, (1 << 22) + 1, r"%s must be in \[0, 2\^22\]"),
    "tail_screen": (1, 0, 0, 2, ZERO_ONE),
    "tail_big_screen": (1, 0, 0, 2, ZERO_ONE),
    "hip_events": (0, 1, 1, 2, ZERO_ONE),
    "small_screen": (1, 0, 0, 2, ZERO_ONE),
}

# name: its value on a fresh context
READ_ONLY = {
    "kmc_decode_launches": 0, "kmc_high_sort": 0, "kcount_batches": 0, "kcount_rehashes": 0,
    "kcount_peak_slots": 0, "kcount_window": 2048, "kcount_db_chunks": 0,
    "kcount_db_prefix_used": -1, "result_rounds": 0, "result_rank_us": 0, "member_nodes": 0,
    "fp16_image": 0, "last_hash_kernel": -1, "last_hash_close_pairs": 0,
    "last_hash_variant": -1, "extract_window": 2048, "tail_local_iters": 0,
}


@pytest.fixture(scope="module")
def eng():
    with _native.Engine(0) as e:
        yield e


def refused(eng, name, value, pattern):
    with pytest.raises(_native.KlshError) as err:
        eng.set_option(name, value)
    assert re.search(r"KLSH_E_ARG: " + pattern + "$", str(err.value)), str(err.value)


def test_tables_are_complete():
    assert len(SETTABLE) == 41 and len(READ_ONLY) == 17 and not set(SETTABLE) & set(READ_ONLY)


def test_defaults(eng):
    got = {name: eng.get_option(name) for name in SETTABLE}
    assert got == {name: row[0] for name, row in SETTABLE.items()}


@pytest.mark.parametrize("name", sorted(SETTABLE))
def test_round_trip(eng, name):
    default, value, readback, bad, message = SETTABLE[name]
    assert value != default and readback != default
    eng.set_option(name, value)
    assert eng.get_option(name) == readback
    if bad is not None:
        refused(eng, name, bad, message % name)
        assert eng.get_option(name) == readback  # a refused value changes nothing
    eng.set_option(name, default)
    assert eng.get_option(name) == default


@pytest.mark.parametrize("name", sorted(READ_ONLY))
def test_read_only(eng, name):
    assert eng.get_option(name) == READ_ONLY[name]
    refused(eng, name, 1, "unknown option " + name)
    assert eng.get_option(name) == READ_ONLY[name]


def test_unknown_name(eng):
    refused(eng, "no_such_option", 1, "unknown option no_such_option")
    with pytest.raises(_native.KlshError, match="KLSH_E_ARG: unknown option no_such_option$"):
        eng.get_option("no_such_option")


def test_grid_cap_reads_back_what_was_set(eng):
    for value in (7, 1 << 20, 0):
        eng.set_option("grid_cap", value)
        assert eng.get_option("grid_cap") == value


def test_long_runs_values(eng):
    for value in (0, 1, 4):
        eng.set_option("long_runs", value)
        assert eng.get_option("long_runs") == value


def test_tail_merge_rows_zero_is_the_default_size(eng):
    eng.set_option("tail_merge_rows", 4096)
    eng.set_option("tail_merge_rows", 0)
    assert eng.get_option("tail_merge_rows") == SETTABLE["tail_merge_rows"][0]
