"""Times of exact variable elimination (gml_model_elim) on sparse models in one connected component.

Per model: the plan (width, work = sum_t 2^|scope_t|, stored = sum_t 2^|F_t|, and the host time of gml_model_elim_plan), the
whole-call time of log Z alone and of log Z with all means and term expectations, and the achieved rate on the bytes the step kernels
must move: a forward step reads alpha_{t-1} and writes alpha_t, 16 x stored bytes for the pass (split launches not counted); the
backward step reads alpha_{t-1} and beta_t and writes beta_{t-1}, 24 x stored more.  Models: a 16 x 16 lattice, Chimera C4, a 24 x 24
lattice (log Z only: its forward tables are beyond the 2^32 entries the moments may store) and a tree of 16 384 spins in which every
spin hangs from one of the 8 before it (a uniform random recursive tree of that size grows hubs: its greedy order has width 857).
Then the 5 x 8 lattice beside gml_model_exact on the same model, and the AIS estimate of the 8 x 8 lattice beside the exact value.

One process: a warm-up call on a small model (loads the code object), then --repeats timed calls per case, each of which returns
after its stream is synchronised; the median is printed as one JSON line per case.

    python scripts/elim_times.py --repeats 3"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _elim_reference as R  # noqa: E402  (the models of the tests)


def timed(fn, repeats):
    out, secs = None, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t0)
    return out, statistics.median(secs), secs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true", help="leave out the 24 x 24 lattice and the 40-spin enumeration")
    args = ap.parse_args()
    import gml_amd as gml
    lib = gml._lib
    lib.model_elim(*R.lattice(4, 4))
    models = [("lattice_16x16", R.lattice(16, 16), True), ("chimera_4", R.chimera(4), True), ("tree_16384", R.tree(16384, back=8), True)]
    if not args.skip_large:
        models.insert(2, ("lattice_24x24", R.lattice(24, 24), False))
    for name, (terms, n), moments in models:
        (_, width, work, stored), plan_s, _ = timed(lambda: lib.model_elim_plan(terms, n), args.repeats)
        rec = {"model": name, "n": n, "terms": len(terms), "width": width, "work": work, "stored": stored, "plan_s": plan_s}
        (log_z, _, _), secs, all_s = timed(lambda: lib.model_elim(terms, n, mean=False, texp=False), args.repeats)
        rec.update(log_z=log_z, logz_s=secs, logz_all_s=all_s, logz_GBps=16 * stored / secs / 1e9)
        if moments:
            (lz, m, e), secs, all_s = timed(lambda: lib.model_elim(terms, n), args.repeats)
            assert lz == log_z and np.isfinite(m).all() and np.isfinite(e).all()
            rec.update(moments_s=secs, moments_all_s=all_s, moments_GBps=40 * stored / secs / 1e9)
        print(json.dumps(rec), flush=True)
    if not args.skip_large:
        terms, n = R.lattice(5, 8)
        (log_z, m, e), elim_s, _ = timed(lambda: lib.model_elim(terms, n), args.repeats)
        (xz, xm, _, xe), exact_s, _ = timed(lambda: lib.model_exact(terms, n, queries=terms, pairs=False), 1)
        print(json.dumps({"model": "lattice_5x8", "n": n, "elim_s": elim_s, "model_exact_s": exact_s, "log_z": log_z, "log_z_exact": xz,
                          "max_diff_means": float(np.abs(m - xm).max()), "max_diff_terms": float(np.abs(e - xe).max())}), flush=True)
    terms, n = R.lattice(8, 8)
    log_z = lib.model_elim(terms, n, mean=False, texp=False)[0]
    ais, ais_s, _ = timed(lambda: gml.log_partition(terms, gml.AIS(), seed=1), 1)
    print(json.dumps({"model": "lattice_8x8", "log_z": log_z, "ais_log_z": ais.log_z, "ais_stderr": ais.stderr, "ais_minus_exact": ais.log_z - log_z,
                      "ais_s": ais_s}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
