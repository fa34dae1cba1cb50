"""What the step after the loop costs at C2 (synthetic 10M x 64): the host result path against
the device one, and the host load against the device load.

After 1 iteration (the init pass) and after the full loop, median of `--runs` wall-clock runs,
the device idle before each:
  host    klsh_count + klsh_result with option result_device = 0 (the walk on the host)
  dev     the same calls with result_device = 1 (offsets + list ranking on the GPU, ids on the host)
  device  klsh_result_device alone, into preallocated device buffers
each with the rows (centroids copied out) and for the member lists alone; then klsh_load_rows
against klsh_load_rows_device for the converted matrix.  One JSON line at the end.
    python tools/bench_result.py [--n 10000000] [--d 64] [--iters 500] [--runs 5]
"""
import argparse
import ctypes
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


def median_ms(fn, runs):
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(out), 3)


def time_results(eng, runs):
    """The three result paths on the engine's current state."""
    lib, ctx = eng._lib, eng._ctx
    n, m = eng.count()
    big_m = eng.get_option("member_nodes")
    rows = np.zeros((n, eng.d), np.float32)
    off, ids = np.zeros(n + 1, np.uint64), np.zeros(m, np.uint64)
    dev = torch.device("cuda", eng.device)
    d_rows = torch.zeros((n, eng.d), dtype=torch.float32, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.uint32, device=dev)
    d_nodes = torch.zeros(max(m, 1), dtype=torch.uint32, device=dev)
    d_labels = torch.zeros(max(big_m, 1), dtype=torch.uint32, device=dev)
    P = ctypes.c_void_p
    nn, mm = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def host_call(with_rows):
        def run():
            assert lib.klsh_count(ctx, ctypes.byref(nn), ctypes.byref(mm)) == 0
            assert lib.klsh_result(ctx, _native._ptr(rows) if with_rows else None,
                                   _native._ptr(off), _native._ptr(ids)) == 0
        return run

    def device_call(with_rows):
        def run():
            assert lib.klsh_result_device(ctx, P(d_rows.data_ptr()) if with_rows else None,
                                          P(d_off.data_ptr()), P(d_nodes.data_ptr()),
                                          P(d_labels.data_ptr())) == 0
        return run

    res = {"rows": n, "members": m, "nodes": big_m}
    for mode, name in ((0, "host"), (1, "dev")):
        eng.set_option("result_device", mode)
        res[name + "_ms"] = median_ms(host_call(True), runs)
        res[name + "_lists_ms"] = median_ms(host_call(False), runs)
        if mode == 0:
            want = (off.copy(), ids.copy())
        else:
            assert np.array_equal(off, want[0]) and np.array_equal(ids, want[1])
    eng.set_option("result_device", 0)
    res["device_ms"] = median_ms(device_call(True), runs)
    res["device_lists_ms"] = median_ms(device_call(False), runs)
    res["rounds"] = eng.get_option("result_rounds")
    res["rank_us"] = eng.get_option("result_rank_us")
    res["round_us"] = round(res["rank_us"] / res["rounds"], 1) if res["rounds"] else 0.0
    assert np.array_equal(d_off.cpu().numpy(), want[0].astype(np.uint32))
    return res


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
        matrix = eng.result()[0]  # the converted rows: the matrix of the load comparison
        _, c0, _ = eng.cluster(0.80, 1, 100_000, 12345, 0)
        out["after_1"] = time_results(eng, a.runs)
        print(json.dumps(out["after_1"]), flush=True)
        t0 = time.perf_counter()
        eng.cluster(0.80, a.iters, 1_000_000, 12345, c0)
        out["loop_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        out["after_loop"] = time_results(eng, a.runs)
        print(json.dumps(out["after_loop"]), flush=True)
        d_matrix = torch.from_numpy(matrix).to(f"cuda:{eng.device}")
        out["load_rows_ms"] = median_ms(lambda: eng.load_rows(matrix), a.runs)
        out["load_rows_device_ms"] = median_ms(lambda: eng.load_rows(d_matrix), a.runs)
        out["load_rows_n"] = int(matrix.shape[0])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
