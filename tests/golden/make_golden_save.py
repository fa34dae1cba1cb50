"""Generate tests/golden/save_digits.npz from the REFERENCE's own writers.

`oracle/_ref/ref_harness cluster_w ROWS OFF IDS N D 0.8 0 1000000 OUT` runs zero iterations of
Cluster, so it writes the lists it was given through IOMat::SaveResult / IOMat::SaveBinary
(io/ioMatrix.cc:265-294, 322-351) with ignore_small = 0.  The ids cover every digit count of a
uint64 on both sides: 0, 10^k - 1, 10^k, 10^k + 1 for k = 1..19, 2^32 - 1, 2^32, 2^63, 2^64 - 1,
in lists of 1, 5, 6, 10, 21 and the rest, at d = 3.  Stored: the inputs and the two files' bytes.
Needs the reference build (`make -C oracle ref`); the fixture it writes is committed.

    python tests/golden/make_golden_save.py
"""
from __future__ import annotations

import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
ENV = dict(os.environ, OMP_THREAD_LIMIT="1", OMP_NUM_THREADS="1", KLSH_SEED="12345")

LISTS = [1, 5, 6, 10, 21]  # then the rest


def digit_ids() -> np.ndarray:
    ids = [0]
    for k in range(1, 20):
        ids += [10 ** k - 1, 10 ** k, 10 ** k + 1]
    ids += [2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1]
    assert len(set(ids)) == len(ids) == 62
    # a fixed shuffle, so that neighbours in a list differ in length
    perm = np.random.default_rng(62).permutation(len(ids))
    return np.array(ids, dtype=np.uint64)[perm]


def main() -> None:
    ids = digit_ids()
    sizes = LISTS + [ids.size - sum(LISTS)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n, d = len(sizes), 3
    rows = (np.arange(n * d, dtype=np.float32).reshape(n, d) * np.float32(0.37) -
            np.float32(2.5)).astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "rows.f32")
        rows.astype("<f4").tofile(src)
        off.astype("<u8").tofile(src + ".off")
        ids.astype("<u8").tofile(src + ".ids")
        out = os.path.join(tmp, "out")
        subprocess.run([HARNESS, "cluster_w", src, src + ".off", src + ".ids", str(n), str(d), "0.8",
                        "0", "1000000", out], env=ENV, check=True, capture_output=True)
        with open(out + ".clust", "rb") as f:
            clust = np.frombuffer(f.read(), dtype=np.uint8)
        with open(out, "rb") as f:
            binary = np.frombuffer(f.read(), dtype=np.uint8)
    assert clust.size and binary.size == 4 * n * d
    np.savez_compressed(os.path.join(HERE, "save_digits.npz"), rows=rows, off=off, ids=ids,
                        clust=clust, binary=binary)
    print(f"save_digits.npz: {n} lists, {ids.size} ids, {clust.size} text bytes, "
          f"{binary.size} binary bytes")


if __name__ == "__main__":
    main()
