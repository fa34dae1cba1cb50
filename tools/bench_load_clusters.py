"""What reloading a clustered state costs at C2 (synthetic 10M x 64, M = 10M nodes; DESIGN.md
§13.6): the device load against the host path it replaces, in one process.

The state is C2's after its loop, its lists interleaved over the 10M nodes by the merges.  Median
of `--runs` wall-clock runs after one warm run each, the device idle before each:
  device  klsh_load_clusters_device of result_device()'s own rows, offsets and nodes (n_nodes = 0)
  host    klsh_result into preallocated host arrays, then klsh_load_rows of them
klsh_load_rows renumbers the nodes in list order, which would make the next run's host walk
sequential, so every host run starts from the loop's own numbering, put back (untimed) by a device
load.  Also given: the host path on the renumbered state it leaves.  One JSON line at the end.
    python tools/bench_load_clusters.py [--n 10000000] [--d 64] [--iters 500] [--runs 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmerlsh_amd import _native  # noqa: E402
from kmerlsh_amd.io import v_kmers_from_coverage  # noqa: E402


def timed_ms(fn, runs, before=lambda: None):
    before()
    fn()  # warm: allocations, first launches
    out = []
    for _ in range(runs):
        before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(out), 3), [round(v, 3) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    counts, cov = _native.synth_counts(a.n, a.d, seed=11)
    out = {"n": a.n, "d": a.d, "iters": a.iters, "runs": a.runs}
    with _native.Engine(0) as eng:
        eng.load_counts(counts, v_kmers_from_coverage(cov, a.n))
        del counts
        _, c0, _ = eng.cluster(0.80, 1, 100_000, 12345, 0)
        eng.cluster(0.80, a.iters, 1_000_000, 12345, c0)
        n, m = eng.count()
        out.update(rows=n, members=m, nodes=eng.get_option("member_nodes"))
        want = eng.result()
        d_rows, d_off, d_nodes, _ = eng.result_device()

        out["device_ms"], out["device_runs"] = timed_ms(
            lambda: eng.load_clusters(d_rows, d_off, d_nodes), a.runs)
        got = eng.result()
        assert all(np.array_equal(x, y) for x, y in zip(got[1:], want[1:]))
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))

        rows = np.zeros((n, a.d), np.float32)
        off, ids = np.zeros(n + 1, np.uint64), np.zeros(m, np.uint64)
        lib, ctx, p = eng._lib, eng._ctx, _native._ptr
        parts = {"result": [], "load": []}

        def host_path():
            t0 = time.perf_counter()
            assert lib.klsh_result(ctx, p(rows), p(off), p(ids)) == 0
            t1 = time.perf_counter()
            assert lib.klsh_load_rows(ctx, p(rows), n, a.d, p(off), p(ids)) == 0
            parts["result"].append(1e3 * (t1 - t0))
            parts["load"].append(1e3 * (time.perf_counter() - t1))

        def loop_numbering():  # (klsh_load_counts numbered the ids as the nodes: id k = node k)
            eng.load_clusters(d_rows, d_off, d_nodes, n_nodes=out["nodes"])

        def split(name):
            out[name + "_result_ms"] = round(statistics.median(parts["result"][1:]), 3)
            out[name + "_load_rows_ms"] = round(statistics.median(parts["load"][1:]), 3)
            parts["result"].clear(), parts["load"].clear()

        out["host_ms"], out["host_runs"] = timed_ms(host_path, a.runs, loop_numbering)
        split("host")
        out["host_renumbered_ms"], _ = timed_ms(host_path, a.runs)
        split("host_renumbered")
        got = eng.result()
        assert all(np.array_equal(x, y) for x, y in zip(got[1:], want[1:]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
