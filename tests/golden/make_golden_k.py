"""Mode-K golden fixtures, tied to files the reference itself wrote (TEST INFRASTRUCTURE ONLY).

Needs oracle/_ref/kmerLSH_seeded (`make -C oracle ref`, this container only).  For every case of
kcount_inputs.CASES the counting model's listings are written as KMC1 databases and the
reference CLI runs `-M B --only -T 1` on them, the way make_golden_b.py does for mode B;
tests/golden/mode_k.json keeps kmer_count.log verbatim, the md5 of the reference's kmer_set.hex
and kmer_count.bin, the order-free row digest, and per sample the listing's length and md5.
(The "win" case depends on the counting kernel's LDS window: its expectation is computed by
the model and the oracle at test time.)

    python tests/golden/make_golden_k.py
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import kcount_inputs as kc  # noqa: E402
import klsh_oracle_b as ob  # noqa: E402
from make_golden_b import row_digest  # noqa: E402

REF_CLI = os.path.join(ROOT, "oracle", "_ref", "kmerLSH_seeded")


def main() -> None:
    if not os.path.exists(REF_CLI):
        sys.exit("build the reference first: make -C oracle ref")
    out = {}
    for case in kc.CASES:
        with tempfile.TemporaryDirectory() as tmp:
            info = kc.write_case(tmp, case)
            _, listings = kc.write_model_dbs(tmp, info)
            subprocess.run([REF_CLI] + kc.cli_args(info, "B") + ["-T", "1"], cwd=tmp, check=True,
                           capture_output=True, env=dict(os.environ, OMP_THREAD_LIMIT="1"))
            reps, counts, log = ob.read_outputs(tmp, info["d"])
            md5f = lambda n: hashlib.md5(open(os.path.join(tmp, n), "rb").read()).hexdigest()  # noqa: E731
            out[case] = dict(kmap=int(len(reps)), log=log, rows_md5=row_digest(reps, counts),
                             hex_md5=md5f("kmer_set.hex"), bin_md5=md5f("kmer_count.bin"),
                             listings=[dict(n=len(ls), md5=kc.listing_md5(ls)) for ls in listings])
    with open(os.path.join(HERE, "mode_k.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote mode_k.json:", {c: v["kmap"] for c, v in out.items()})


if __name__ == "__main__":
    main()
