"""bench.py --dump-outputs on CPU: the files it writes for a result larger than its caps are
float32 / float64, stay below 64 MB in all, and are the same from call to call."""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_sampled_and_repeatable(tmp_path):
    n, d, m = 20_000, 512, 700_000  # rows 41 MB > DUMP_ROW_BYTES, ids > DUMP_MAX_INTS
    rng = np.random.default_rng(3)
    rows = rng.random((n, d), dtype=np.float32)
    off = np.linspace(0, m, n + 1).astype(np.uint64)
    ids = rng.permutation(m).astype(np.uint64)
    trace = np.arange(500, 0, -1, dtype=np.uint64)
    dumps = []
    for name in ("a", "b"):
        out = tmp_path / name
        total = bench.dump_outputs(str(out), trace, (1 << 40) + 7, lambda: (rows, off, ids))
        files = {p.name: np.load(p) for p in sorted(out.iterdir())}
        assert total <= 64_000_000 and sum(os.path.getsize(p) for p in out.iterdir()) <= 64_000_000
        dumps.append(files)
    a, b = dumps
    assert set(a) == {"trace.npy", "counter.npy", "rows.npy", "rows_index.npy", "member_offsets.npy",
                      "member_ids.npy", "member_ids_index.npy"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert np.array_equal(a["trace.npy"], trace.astype(np.float64))
    assert a["counter.npy"][0] == (1 << 40) + 7
    assert np.array_equal(a["member_offsets.npy"], off.astype(np.float64))  # below its cap: whole
    at = a["rows_index.npy"].astype(np.int64)
    assert at.size == bench.DUMP_ROW_BYTES // (4 * d) and np.all(np.diff(at) > 0)
    assert np.array_equal(a["rows.npy"], rows[at])
    at = a["member_ids_index.npy"].astype(np.int64)
    assert at.size == bench.DUMP_MAX_INTS
    assert np.array_equal(a["member_ids.npy"], ids[at].astype(np.float64))
