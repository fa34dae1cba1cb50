"""Generate the threshold-domain fixtures in tests/golden/ from the REFERENCE itself.

make_golden.py pins the reference at thresholds 0.7 .. 0.95; the product takes any float (-N is
read with atof, and the loop walks the threshold from 0.95 to min_similarity), so these fixtures
cover the rest: thresholds at and below 0, tiny, at and either side of 1, infinite, NaN, and
min_similarity values that take the loop below 0 or up past 1.  Its own seeded RNG stream (adding
the cases to make_golden.py would redraw every existing fixture).

    python tests/golden/make_golden_thr.py

pcluster_thr_<b>x<d>.npz: rows and thr[k]; pcluster_thr_<b>x<d>_ref.npz: per threshold k the
reference's off_k / ids_k and its output rows, stored only for the survivors with more than one
member (midx_k, mrows_k): a survivor that never merged is its input row bit for bit (checked
here), which load_pcluster_thr puts back.  (Two files and no unmerged rows: 40 x 512 floats and
nine outputs of up to 40 rows would not fit the size of the largest pcluster_*.npz otherwise.)
cluster_thr_*.npz: the layout of cluster_*.npz.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

F = np.float32
PCLUSTER_THR_SHAPES = [(64, 64), (200, 32), (40, 512), (33, 13)]
PCLUSTER_THR = [0.0, -0.25, 1e-30, 0.05, float(np.nextafter(F(1), F(0))), 1.0,
                float(np.nextafter(F(1), F(2))), float("inf"), float("nan")]
CLUSTER_THR_CASES = {
    "cluster_thr_neg_d32": dict(n=3000, d=32, groups=300, noise=0.3, min_sim=-0.5, iters=12,
                                bthr=1000000, seed=101),
    "cluster_thr_zero_d64": dict(n=3000, d=64, groups=60, noise=0.3, min_sim=0.0, iters=12,
                                 bthr=1000000, seed=102),
    "cluster_thr_nested_d16": dict(n=2000, d=16, groups=2, noise=0.3, min_sim=0.3, iters=10,
                                   bthr=300, seed=103),
    "cluster_thr_rising_d13": dict(n=3000, d=13, groups=300, noise=0.3, min_sim=0.97, iters=10,
                                   bthr=1000000, seed=104),
    "cluster_thr_over1_d16": dict(n=2000, d=16, groups=200, noise=0.3, min_sim=1.3, iters=10,
                                  bthr=1000000, seed=105),
}


def pcluster_thr_name(b, d, ref=False):
    return f"pcluster_thr_{b}x{d}{'_ref' if ref else ''}.npz"


def load_pcluster_thr(b, d):
    """rows and [(thr, out_rows, out_off, out_ids)] of one pcluster_thr fixture."""
    zin = np.load(os.path.join(HERE, pcluster_thr_name(b, d)), allow_pickle=False)
    z = np.load(os.path.join(HERE, pcluster_thr_name(b, d, ref=True)), allow_pickle=False)
    rows, cases = zin["rows"], []
    for k, thr in enumerate(zin["thr"]):
        off, ids = z[f"off_{k}"], z[f"ids_{k}"]
        out = rows[ids[off[:-1]].astype(np.int64)].copy()  # each survivor's first member ...
        out[z[f"midx_{k}"]] = z[f"mrows_{k}"]              # ... but for the merged ones
        cases.append((float(thr), out, off, ids))
    return rows, cases


def threshold_rows(rng, b, d, groups, nan_row=True):
    """One run for the merge test over the whole threshold domain: clustered rows (noise 0.3) with
    special rows written over them, alternately at the back and at the front of the run (so each
    kind is met as current row and as candidate), their sources being rows left plain:
    x2 copy, zero row (0/0: never merges), negated copy (cos = -1), exact copy, a pair with
    disjoint supports (dot exactly +0), a row orthogonalised against its source in f64 and then
    cast (cos = rounding noise around 0), x3 copy, for b >= 32 a NaN row (nan_row), then the list
    again on other sources, up to max(8, b / 8) special rows (at most 40).  Runs under 9 rows take
    the first b - 1 kinds."""
    f = np.float32
    centers = rng.normal(0, 1, size=(groups, d)).astype(np.float32)
    rows = (centers[rng.integers(0, groups, b)] +
            rng.normal(0, 0.3, size=(b, d)).astype(np.float32)).astype(np.float32)
    kinds = ["x2", "zero", "neg", "copy", "disj_a", "disj_b", "orth", "x3", "nan"]
    want = min(b - 1, max(8, min(b // 8, 40)))
    todo = []
    while len(todo) < want:
        for kd in kinds:
            if len(todo) < want and not (kd == "nan" and (b < 32 or not nan_row or "nan" in todo)):
                todo.append(kd)
    # destinations: b-1, 1, b-2, 2, ...; every other row stays plain
    dst = [(b - 1 - i // 2) if i % 2 == 0 else (1 + i // 2) for i in range(len(todo))]
    plain = [i for i in range(b) if i not in set(dst)]
    half = d // 2
    for m, (kd, t) in enumerate(zip(todo, dst)):
        # a plain source on the other side of the run
        src = plain[(m // 2) % len(plain)] if t >= b // 2 else plain[-1 - (m // 2) % len(plain)]
        if kd == "x2":
            rows[t] = rows[src] * f(2)
        elif kd == "x3":
            rows[t] = rows[src] * f(3)
        elif kd == "neg":
            rows[t] = -rows[src]
        elif kd == "copy":
            rows[t] = rows[src]
        elif kd == "zero":
            rows[t] = 0.0
        elif kd == "nan":
            rows[t, d // 3] = np.nan
        elif kd == "disj_a":
            rows[t, half:] = 0.0
        elif kd == "disj_b":
            rows[t, :half] = 0.0
        else:  # orth
            u = rows[src].astype(np.float64)
            v = rng.normal(0, 1, size=d)
            rows[t] = (v - (v @ u) / (u @ u) * u).astype(np.float32)
    return rows


def main():
    from make_golden import HARNESS, clustered_rows, harness_cluster, parse_clust, run

    if not os.path.exists(HARNESS):
        sys.exit("build the reference first: make -C oracle ref")
    rng = np.random.default_rng(20261019)
    with tempfile.TemporaryDirectory() as tmp:
        for b, d in PCLUSTER_THR_SHAPES:
            rows = threshold_rows(rng, b, d, max(2, b // 4), nan_row=False)
            src = os.path.join(tmp, "p.f32")
            rows.astype("<f4").tofile(src)
            thrs = np.array(PCLUSTER_THR, np.float32)
            np.savez_compressed(os.path.join(HERE, pcluster_thr_name(b, d)), rows=rows, thr=thrs)
            out = {}
            for k, thr in enumerate(thrs):
                prefix = os.path.join(tmp, "p")
                run([HARNESS, "pcluster", src, str(b), str(d), repr(float(thr)), prefix])
                out_rows = np.fromfile(prefix, dtype="<f4").reshape(-1, d)
                off, ids = parse_clust(prefix + ".clust")
                single = np.diff(off.astype(np.int64)) == 1
                first = ids[off[:-1]].astype(np.int64)
                assert np.array_equal(out_rows[single].view(np.uint32),
                                      rows[first[single]].view(np.uint32))
                midx = np.flatnonzero(~single).astype(np.uint32)
                out.update({f"off_{k}": off, f"ids_{k}": ids, f"midx_{k}": midx,
                            f"mrows_{k}": out_rows[midx]})
                print(f"pcluster {b}x{d} thr {float(thr)!r}: {out_rows.shape[0]} survivors")
            np.savez_compressed(os.path.join(HERE, pcluster_thr_name(b, d, ref=True)), **out)
        for name, c in CLUSTER_THR_CASES.items():
            rows = clustered_rows(rng, c["n"], c["d"], c["groups"], c["noise"])
            out_rows, off, ids, trace = harness_cluster(tmp, rows, c["min_sim"], c["iters"],
                                                        c["bthr"], c["seed"])
            np.savez_compressed(os.path.join(HERE, name + ".npz"), rows=rows,
                                min_sim=np.float32(c["min_sim"]), iters=np.int32(c["iters"]),
                                bthr=np.int32(c["bthr"]), seed=np.uint32(c["seed"]),
                                out_rows=out_rows, out_off=off, out_ids=ids, trace=trace)
            print(name, "trace", trace.tolist())
    print("threshold fixtures written to", HERE)


if __name__ == "__main__":
    main()
