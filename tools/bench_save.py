"""What writing the cluster files costs at C2 (synthetic 10M x 64, M = 10M nodes).

In one process, on C2's state after its loop (one warm run, then the median of `--runs` wall-clock
runs, the device idle before each; the files go to `--dir`, a tmpfs directory by default):
  save    klsh_save_clusters (both files, ignore_small = 5) with its statistics' breakdown
  result  klsh_count + klsh_result alone: the host walk the command line used to finish before it
          formatted a byte
and the two files are checked once against kmerlsh_amd.io's writers over that result.

With `--cli A B` also the whole command line, `-M C --only -I <iters>` on C2's count files
(io.write_count_files in `--dir`): binaries A and B alternating, `--cli-runs` runs each, wall clock
of the process, both outputs compared.  B's runs are then placed against A's window (A's min..max
widened by its own spread on each side).  One JSON line at the end.
    python tools/bench_save.py [--n 10000000] [--d 64] [--iters 500] [--runs 5] [--cli A B]
"""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmerlsh_amd import _native, io  # noqa: E402


def log(msg):
    print(f"[bench_save] {msg}", file=sys.stderr, flush=True)


def timed_ms(fn, runs):
    fn()  # warm: allocations, first launches
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(out), 3), [round(v, 3) for v in out]


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def cli_ab(work, counts, cov, iters, clis, runs):
    io.write_count_files(work, counts, cov)
    clis = [os.path.abspath(c) for c in clis]  # (they run in `work`)
    out = {"cli": clis, "cli_secs": [[], []], "cli_md5": [None, None]}
    for _ in range(runs):
        for k, cli in enumerate(clis):
            t0 = time.perf_counter()
            subprocess.run([cli, "-a", "a.txt", "-b", "b.txt", "-I", str(iters), "-M", "C", "--only",
                            "--seed", "12345"], cwd=work, check=True, capture_output=True,
                           timeout=600)
            out["cli_secs"][k].append(round(time.perf_counter() - t0, 3))
            log(f"{cli}: {out['cli_secs'][k][-1]} s")
            sums = [md5(os.path.join(work, f)) for f in ("clustering_result.txt",
                                                         "clustering_result.txt.clust")]
            assert out["cli_md5"][k] in (None, sums), "a binary's outputs changed between runs"
            out["cli_md5"][k] = sums
    a, b = out["cli_secs"]
    spread = max(a) - min(a)
    out["cli_window"] = [round(min(a) - spread, 3), round(max(a) + spread, 3)]
    out["cli_b_within"] = max(b) <= out["cli_window"][1]
    out["cli_same_files"] = out["cli_md5"][0] == out["cli_md5"][1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--cli", nargs=2, metavar=("A", "B"))
    ap.add_argument("--cli-runs", type=int, default=3)
    a = ap.parse_args()
    work = tempfile.mkdtemp(prefix="klsh_save_", dir=a.dir)
    try:
        counts, cov = _native.synth_counts(a.n, a.d, seed=11)
        out = {"n": a.n, "d": a.d, "iters": a.iters, "runs": a.runs}
        clust, binary = os.path.join(work, "out.clust"), os.path.join(work, "out")
        with _native.Engine(0) as eng:
            eng.load_counts(counts, io.v_kmers_from_coverage(cov, a.n))
            _, c0, _ = eng.cluster(0.80, 1, 100_000, 12345, 0)
            t0 = time.perf_counter()
            eng.cluster(0.80, a.iters, 1_000_000, 12345, c0)
            out["loop_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            n, m = eng.count()
            out.update(rows=n, members=m)
            stats = []
            out["save_ms"], out["save_runs"] = timed_ms(
                lambda: stats.append(eng.save_clusters(clust, binary, 5)), a.runs)
            for key in ("rank_ms", "format_ms", "write_ms", "total_ms"):
                out["save_" + key] = round(statistics.median(s[key] for s in stats[1:]), 3)
            out.update({k: stats[-1][k] for k in ("clusters_written", "members_written",
                                                  "text_bytes", "bin_bytes", "chunks")})
            out["ids_uploaded"] = eng.get_option("save_ids_uploaded")
            log(f"save {out['save_ms']} ms {out['save_runs']}")
            got = md5(clust), md5(binary)
            res = {}
            out["result_ms"], out["result_runs"] = timed_ms(
                lambda: res.update(last=eng.result()), a.runs)
            rows, off, ids = res["last"]
            log(f"result {out['result_ms']} ms; checking the files against the Python writers")
            del res
            io.save_result(clust, off, ids, 5)
            io.save_binary(binary, rows, off, 5)
            out["same_as_python_writers"] = got == (md5(clust), md5(binary))
        if a.cli:
            out.update(cli_ab(work, counts, cov, a.iters, a.cli, a.cli_runs))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
