"""The expectation of the klsh_save_clusters tests, tied to the reference's own writers.

tests/golden/save_digits.npz holds lists of ids with every digit count of a uint64 (on both sides
of every power of ten) and the bytes IOMat::SaveResult / IOMat::SaveBinary made of them at
ignore_small = 0 (tests/golden/make_golden_save.py).  kmerlsh_amd.io.save_result / save_binary,
the independent expectation of tests/test_gpu_save_clusters.py, must reproduce those bytes, and
their ignore_small filter must be the filter of those lines by their header.
"""
import numpy as np

from conftest import golden
from kmerlsh_amd import io


def _files(tmp_path, z, ignore_small):
    io.save_result(str(tmp_path / "t.clust"), z["off"], z["ids"], ignore_small)
    io.save_binary(str(tmp_path / "t"), z["rows"], z["off"], ignore_small)
    return (tmp_path / "t.clust").read_bytes(), (tmp_path / "t").read_bytes()


def test_python_writers_reproduce_reference_bytes(tmp_path):
    z = golden("save_digits.npz")
    sizes = np.diff(z["off"].astype(np.int64)).tolist()
    assert sizes[:5] == [1, 5, 6, 10, 21] and z["ids"].size == 62 and z["rows"].shape[1] == 3
    digits = {len(str(int(v))) for v in z["ids"].tolist()}
    assert digits == set(range(1, 21)) and int(z["ids"].max()) == 2 ** 64 - 1
    clust, binary = _files(tmp_path, z, 0)
    assert clust == z["clust"].tobytes()
    assert binary == z["binary"].tobytes()


def test_ignore_small_filters_lines_by_header(tmp_path):
    z = golden("save_digits.npz")
    lines = z["clust"].tobytes().split(b"\n")
    assert lines[-1] == b"" and len(lines) - 1 == z["rows"].shape[0]
    keep = [int(ln.split(b"\t")[0]) > 5 for ln in lines[:-1]]
    assert keep == [False, False, True, True, True, True]
    clust, binary = _files(tmp_path, z, 5)
    assert clust == b"".join(ln + b"\n" for ln, k in zip(lines[:-1], keep) if k)
    rows = np.frombuffer(z["binary"].tobytes(), "<f4").reshape(-1, 3)
    assert binary == rows[np.array(keep)].tobytes()
