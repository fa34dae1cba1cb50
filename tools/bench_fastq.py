"""Modes E and K with the host FASTQ reader against the device parser, and
against another build of the engine, interleaved.

  python tools/bench_fastq.py --data DIR [--make] [--rounds 5] [--other LIB] [--reads 2000000]
                              [--kreads 1000000] [--log FILE]

--make writes the workloads of DESIGN.md §10 / §12 into DIR once: mode E's 2 x 10^6 random 150-bp
reads (a third drawn from the sequence the 4 x 10^6-k-mer set was cut from), plain and (a quarter
of them) gzip, and mode K's two samples of 10^6 reads, plain and (a quarter) gzip.  Then `rounds`
rounds; each runs every (mode, input) once per variant, in turn, each in a process of its own (one
warm-up call, one timed call):

  other       the library --other names (KLSH_LIB; e.g. the parent commit's build), if given
  host        this tree's library, fastq_parse 1
  device      this tree's library, fastq_parse 0 (plain inputs only: gzip never reaches the device)

One JSON line per run (wall_ms around the timed call, the call's statistics, the fastq_* options),
appended to --log too, and a table of medians and spreads at the end.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

K, VOTE, COUNT_MIN = 31, 0.5, 2
FASTQ_OPTIONS = ("fastq_parse", "fastq_device_chunks", "fastq_device_reads", "fastq_host_reads",
                 "fastq_takeover_at", "fastq_parse_us", "fastq_read_us")
INPUTS = {"E": ("e_plain", "e_gzip"), "K": ("k_plain", "k_gzip")}


def make(data: str, n_reads: int, n_kset: int, k_reads: int, k_genome: int) -> None:
    from bench_modes import _write_reads, canonical_np

    os.makedirs(data, exist_ok=True)
    rng = np.random.default_rng(3)
    src = rng.integers(0, 4, size=n_kset + K, dtype=np.uint8)
    np.save(os.path.join(data, "kset.npy"), np.unique(canonical_np(src, K)))
    L = 150
    starts = rng.integers(0, src.size - L, size=n_reads)
    rand = rng.integers(0, 4, size=(n_reads, L), dtype=np.uint8)
    from_src = (np.arange(n_reads) % 3) == 0
    rand[from_src] = src[starts[from_src, None] + np.arange(L)[None, :]]
    seq = np.frombuffer(b"ACGT", np.uint8)[rand]
    _write_reads(os.path.join(data, "e_plain.fq"), seq)
    _write_reads(os.path.join(data, "e_gzip.fq.gz"), seq[:n_reads // 4], gz=True)
    rng = np.random.default_rng(7)
    pool = rng.integers(0, 4, size=k_genome, dtype=np.uint8)
    for j in range(2):
        starts = rng.integers(0, pool.size - L, size=k_reads)
        codes = pool[starts[:, None] + np.arange(L)[None, :]]
        flip = rng.integers(0, 2, size=k_reads).astype(bool)
        codes[flip] = 3 - codes[flip, ::-1]
        err = rng.random(codes.shape) < 0.01
        codes[err] = rng.integers(0, 4, size=int(err.sum()), dtype=np.uint8)
        seq = np.frombuffer(b"ACGT", np.uint8)[codes]
        _write_reads(os.path.join(data, "k_plain%d.fq" % j), seq)
        _write_reads(os.path.join(data, "k_gzip%d.fq.gz" % j), seq[:k_reads // 4], gz=True)


def worker(data: str, mode: str, inp: str, parse: int, label: str) -> None:
    """One process: a warm-up call and the timed call."""
    from kmerlsh_amd import _native

    out = os.path.join(data, "out_%d" % os.getpid())
    os.makedirs(out, exist_ok=True)
    with _native.Engine(0) as eng:
        try:
            eng.set_option("fastq_parse", parse)
        except _native.KlshError:
            pass  # a build from before the option: the host reader is all it has
        if mode == "E":
            path = os.path.join(data, "e_plain.fq" if inp == "e_plain" else "e_gzip.fq.gz")
            ks = _native.KmerSet(eng, np.load(os.path.join(data, "kset.npy")))
            run = lambda: ks.extract_fastq(path, os.path.join(out, "out.fq"), K, VOTE)
        else:
            paths = [os.path.join(data, ("k_plain%d.fq" if inp == "k_plain" else "k_gzip%d.fq.gz") % j)
                     for j in range(2)]
            run = lambda: eng.count_khtable(paths, K, COUNT_MIN, out)
        run()
        t = time.perf_counter()
        st = run()
        wall = (time.perf_counter() - t) * 1e3
        opts = {}
        for name in FASTQ_OPTIONS:
            try:
                opts[name] = eng.get_option(name)
            except _native.KlshError:
                opts[name] = None
        if mode == "E":
            ks.close()
    digest = hashlib.md5()
    for f in sorted(os.listdir(out)):  # (faster and different is not faster: the variants' outputs are compared)
        with open(os.path.join(out, f), "rb") as fh:
            while True:
                block = fh.read(1 << 24)
                if not block:
                    break
                digest.update(block)
        os.remove(os.path.join(out, f))
    os.rmdir(out)
    print(json.dumps({"variant": label, "mode": mode, "input": inp, "wall_ms": wall, "output_md5": digest.hexdigest(),
                      **st, **opts}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", required=True)
    ap.add_argument("--make", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--other", default=None, help="another build's libklsh.so, run beside this tree's")
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--kset", type=int, default=4000000)
    ap.add_argument("--kreads", type=int, default=1000000)
    ap.add_argument("--kgenome", type=int, default=4000000)
    ap.add_argument("--log", default=None)
    ap.add_argument("--worker", nargs=4, metavar=("MODE", "INPUT", "PARSE", "LABEL"), default=None)
    a = ap.parse_args()
    if a.worker:
        worker(a.data, a.worker[0], a.worker[1], int(a.worker[2]), a.worker[3])
        return
    if a.make:
        make(a.data, a.reads, a.kset, a.kreads, a.kgenome)
    rows = []
    for r in range(a.rounds):
        for mode in ("E", "K"):
            for inp in INPUTS[mode]:
                variants = ([("other", 1, a.other)] if a.other else []) + [("host", 1, None)]
                if inp.endswith("plain"):
                    variants.append(("device", 0, None))
                for label, parse, lib in variants:
                    env = dict(os.environ)
                    env.pop("KLSH_LIB", None)
                    if lib:
                        env.update(KLSH_LIB=lib, KLSH_ABI_ANY="1")
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--data", a.data, "--worker",
                                        mode, inp, str(parse), label], env=env, capture_output=True,
                                       text=True, timeout=600)
                    line = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
                    if p.returncode != 0 or not line.startswith("{"):
                        print("run failed:", label, mode, inp, p.stderr[-2000:], flush=True)
                        sys.exit(1)
                    row = dict(json.loads(line), round=r)
                    rows.append(row)
                    text = json.dumps(row)
                    print(text, flush=True)
                    if a.log:
                        with open(a.log, "a") as f:
                            f.write(text + "\n")
    for mode in ("E", "K"):
        for inp in INPUTS[mode]:
            outs = {x["output_md5"] for x in rows if (x["mode"], x["input"]) == (mode, inp)}
            if len(outs) > 1:
                print("OUTPUTS DIFFER:", mode, inp, outs, flush=True)
                sys.exit(1)
    lines = ["every variant of a (mode, input) wrote the same bytes",
             "mode input    variant  median_wall_ms  min..max  (spread)  parse_ms  kernel_ms  fastq_parse_us  fastq_read_us"]
    for mode in ("E", "K"):
        for inp in INPUTS[mode]:
            for label in ("other", "host", "device"):
                sel = [x for x in rows if (x["mode"], x["input"], x["variant"]) == (mode, inp, label)]
                if not sel:
                    continue
                w = sorted(x["wall_ms"] for x in sel)
                med = lambda key: float(np.median([x[key] for x in sel if x.get(key) is not None] or [0]))
                lines.append("%-4s %-8s %-7s %9.1f  %8.1f..%-8.1f (%6.1f)  %8.1f  %8.1f  %10.0f  %10.0f" % (
                    mode, inp, label, float(np.median(w)), w[0], w[-1], w[-1] - w[0], med("parse_ms"),
                    med("kernel_ms"), med("fastq_parse_us"), med("fastq_read_us")))
    print("\n".join(lines), flush=True)
    if a.log:
        with open(a.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
