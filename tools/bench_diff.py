"""What the first half of mode E costs at C2 (synthetic 10M x 64, M = 10M nodes).

C2's state after its loop is saved with klsh_save_clusters (ignore_small = 5) into `--dir` (a tmpfs
directory by default) beside a kmer_set.hex of n distinct images and a kmer_count.log.  Then, in
one process (one warm run, then the median of `--runs` wall-clock runs, the device idle before
each):
  diff    klsh_diff_ksets alone, with its statistics' read / parse / wrs / select breakdown
  host    the same call with the host parser forced: the same files, one '+' written in front of
          the first id (strtol reads the same numbers; the text is irregular)
and the two calls' statistics and table occupancy are compared once.

With `--cli A B` also the whole process `kmerLSH -M E --only`, one tiny FASTQ listed for every
sample of both groups: binaries A and B alternating, `--cli-runs` runs each, wall clock of the
process, their printed id counts and output files compared.  B's runs are then placed against A's
window (A's min..max widened by its own spread on each side).  One JSON line at the end.
    python tools/bench_diff.py [--n 10000000] [--d 64] [--iters 500] [--runs 5] [--cli A B]
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

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmerlsh_amd import _native, io  # noqa: E402

PVAL, SIZE_THRESH = 0.25, 5  # every saved cluster is tested; about half of them pick a group
COUNTERS = ("clusters", "entries", "tokens", "tested", "clusters_a", "clusters_b", "ids_a", "ids_b",
            "kmers_a", "kmers_b")


def log(msg):
    print(f"[bench_diff] {msg}", file=sys.stderr, flush=True)


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


def occupied(kset, probe):
    """(table slots, which of the probe keys the set holds): a key's own slot depends on the order
    the colliding claims landed in, its presence does not."""
    slots, n_slots = kset.find(probe)
    return n_slots, slots != np.uint64(2**64 - 1)


def cli_ab(work, d, clis, runs):
    """-M E --only in `work`: d / 2 samples a group, all of them one tiny FASTQ."""
    with open(os.path.join(work, "tiny.fq"), "w") as f:
        f.write("@r0\n" + "ACGT" * 20 + "\n+\n" + "I" * 80 + "\n")
    for name in ("a.txt", "b.txt"):
        with open(os.path.join(work, name), "w") as f:
            f.write("tiny.fq k0\n" * (d // 2))
    clis = [os.path.abspath(c) for c in clis]  # (they run in `work`)
    out = {"cli": clis, "cli_secs": [[], []], "cli_out": [None, None]}
    for _ in range(runs):
        for k, cli in enumerate(clis):
            t0 = time.perf_counter()
            p = subprocess.run([cli, "-a", "a.txt", "-b", "b.txt", "-o", "A", "-p", "B", "-K", "21",
                                "-M", "E", "--only", "-S", str(SIZE_THRESH), "-P", str(PVAL),
                                "-F", "clustering_result.txt", "--verbose"],
                               cwd=work, check=True, capture_output=True, text=True, timeout=1200)
            out["cli_secs"][k].append(round(time.perf_counter() - t0, 3))
            log(f"{cli}: {out['cli_secs'][k][-1]} s")
            said = [ln for ln in p.stdout.splitlines() if "# of differential" in ln]
            said += [md5(os.path.join(work, f)) for f in ("A_tiny.fq", "B_tiny.fq")]
            assert out["cli_out"][k] in (None, said), "a binary's outputs changed between runs"
            out["cli_out"][k] = said
    a, b = out["cli_secs"]
    spread = max(a) - min(a)
    out["cli_window"] = [round(min(a) - spread, 3), round(max(a) + spread, 3)]
    out["cli_b_within"] = max(b) <= out["cli_window"][1]
    out["cli_b_below"] = max(b) < out["cli_window"][0]
    out["cli_same_output"] = out["cli_out"][0] == out["cli_out"][1]
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
    work = tempfile.mkdtemp(prefix="klsh_diff_", dir=a.dir)
    try:
        counts, cov = _native.synth_counts(a.n, a.d, seed=11)
        out = {"n": a.n, "d": a.d, "iters": a.iters, "runs": a.runs}
        rows_path = os.path.join(work, "clustering_result.txt")
        kmers_path = os.path.join(work, "kmer_set.hex")
        n1 = a.d // 2
        with _native.Engine(0) as eng:
            eng.load_counts(counts, io.v_kmers_from_coverage(cov, a.n))
            _, c0, _ = eng.cluster(0.80, 1, 100_000, 12345, 0)
            eng.cluster(0.80, a.iters, 1_000_000, 12345, c0)
            st = eng.save_clusters(rows_path + ".clust", rows_path, 5)
            out.update(clusters=st["clusters_written"], members=st["members_written"],
                       text_bytes=st["text_bytes"])
            del counts
            kmers = np.arange(1, a.n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
            kmers.tofile(kmers_path)
            with open(os.path.join(work, "kmer_count.log"), "w") as f:
                f.write("%d" % a.n + "".join("\t%f" % 1000.0 for _ in range(a.d)))
            probe = kmers[:: max(1, a.n // 200_000)].copy()
            del kmers

            def call(path, keep):
                sa, sb, s = _native.diff_ksets(eng, path, kmers_path, a.n, n1, a.d - n1, PVAL,
                                               SIZE_THRESH)
                keep.append((s, occupied(sa, probe), occupied(sb, probe)))
                sa.close()
                sb.close()

            dev = []
            out["diff_ms"], out["diff_runs"] = timed_ms(lambda: call(rows_path, dev), a.runs)
            for key in ("read_ms", "parse_ms", "wrs_ms", "select_ms", "total_ms"):
                out["diff_" + key] = round(statistics.median(s[0][key] for s in dev[1:]), 3)
            out.update({k: dev[-1][0][k] for k in COUNTERS})
            out["diff_parse_path"] = dev[-1][0]["parse_path"]
            log(f"diff {out['diff_ms']} ms {out['diff_runs']}")

            # the forced host path: the same rows, the text with one '+' before its first id
            host_rows = os.path.join(work, "host_result.txt")
            os.link(rows_path, host_rows)
            with open(rows_path + ".clust", "rb") as f, open(host_rows + ".clust", "wb") as g:
                head = f.read(1 << 16)
                g.write(head.replace(b"\t", b"\t+", 1))
                shutil.copyfileobj(f, g, 1 << 24)
            host = []
            out["host_ms"], out["host_runs"] = timed_ms(lambda: call(host_rows, host), a.runs)
            for key in ("read_ms", "parse_ms", "wrs_ms", "select_ms", "total_ms"):
                out["host_" + key] = round(statistics.median(s[0][key] for s in host[1:]), 3)
            out["host_parse_path"] = host[-1][0]["parse_path"]
            log(f"host {out['host_ms']} ms {out['host_runs']}")
            same = all(dev[-1][0][k] == host[-1][0][k] for k in COUNTERS if k != "tokens")
            for x, y in zip(dev[-1][1:], host[-1][1:]):
                same = same and x[0] == y[0] and np.array_equal(x[1], y[1])
            out["host_same_sets"] = bool(same)
            os.remove(host_rows)
            os.remove(host_rows + ".clust")
        if a.cli:
            out.update(cli_ab(work, a.d, a.cli, a.cli_runs))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
