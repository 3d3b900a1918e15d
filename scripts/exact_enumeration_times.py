"""Times of the exact enumeration (gml_model_exact) on one connected component: a dense pairwise model with fields on sb spins
(sb (sb + 1) / 2 terms: 820 at sb = 40), log Z with all means and pairs (one window of queries), and log Z alone.

Every measurement is a fresh child process under its own time limit: a warm-up call on a 12-spin model (loads the code object), then
one timed call.  The call returns after its stream is synchronised, so the host clock around it is the time of the enumeration plus
the uploads and the download of a few kilobytes.  The driver prints the median of --repeats children per size as one JSON line, and
stops at the first child that fails.

    python scripts/exact_enumeration_times.py --sizes 24 30 36 40 --repeats 3"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dense_pairwise(sb, seed=0):
    rng = np.random.default_rng(seed)
    terms = {(i,): float(rng.normal(scale=0.1)) for i in range(1, sb + 1)}
    terms.update({(i, j): float(rng.normal(scale=0.5 / np.sqrt(sb))) for i in range(1, sb + 1) for j in range(i + 1, sb + 1)})
    return terms


def child(sb, pairs):
    import gml_amd as gml
    gml._lib.model_exact(dense_pairwise(12), 12, pairs=True)
    terms = dense_pairwise(sb)
    t0 = time.perf_counter()
    log_z, m, C, _ = gml._lib.model_exact(terms, sb, pairs=pairs)
    dt = time.perf_counter() - t0
    assert np.isfinite(log_z) and np.isfinite(m).all()
    print(json.dumps({"sb": sb, "terms": len(terms), "pairs": pairs, "seconds": dt, "log_z": log_z}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[24, 30, 36, 40])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--no-pairs", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.child, not args.no_pairs)
    for sb in args.sizes:
        for pairs in (True, False):
            times, log_z = [], None
            for _ in range(args.repeats):
                cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(sb)]
                r = subprocess.run(cmd + ([] if pairs else ["--no-pairs"]), capture_output=True, text=True)
                if r.returncode != 0:
                    print(json.dumps({"sb": sb, "pairs": pairs, "failed": r.returncode, "stderr": r.stderr[-400:]}), flush=True)
                    return 1
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                times.append(rec["seconds"])
                log_z = rec["log_z"]
            print(json.dumps({"sb": sb, "terms": sb * (sb + 1) // 2, "pairs": pairs, "median_s": statistics.median(times), "all_s": times,
                              "log_z": log_z}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
