"""Times of the selecting enumerations beside the summing ones.

Model path (gml_model_best_states): one connected component, the dense pairwise model with fields of exact_enumeration_times.py on sb
spins, k = 1 and k = 256, beside gml_model_exact's "log Z alone" on the same component in the same run; and the worst case of the
selection, fields of -2.0 on every spin with weak pairs, whose energies ascend with the state so that every chunk enters the list.
Conditional path (gml_conditional_mode): the uniform case of cond_exact_times.py (dense pairwise, n = 1024, 524 800 terms, K rows, h
hidden spins) without log_p (no exponential), with log_p, and gml_conditional_exact with all three outputs beside them.

Every measurement is a fresh child process under its own time limit: a warm-up call of the same entry point on a small problem (loads
the code object), then one timed call, which returns after its stream is synchronised, so the host clock around it is the time of the
call.  The driver prints the median of --repeats children per case as one JSON line, and stops at the first child that fails.

    python scripts/best_states_times.py --sizes 24 30 36 40 --repeats 3"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.cond_exact_times import dense_pairwise as dense_pairwise_arrays, ptr, rows  # noqa: E402
from scripts.exact_enumeration_times import dense_pairwise  # noqa: E402

COND = [(12, 10000), (16, 10000), (20, 10000)]  # (h, K)


def ascending(sb, seed=7):
    rng = np.random.default_rng(seed)
    terms = {(i,): -2.0 for i in range(1, sb + 1)}
    terms.update({(i, j): float(rng.normal(scale=0.05)) for i in range(1, sb + 1) for j in range(i + 1, sb + 1)})
    return terms


def child_model(sb, what, model):
    import gml_amd as gml
    make = ascending if model == "ascending" else dense_pairwise
    k = {"best1": 1, "best256": 256}.get(what)
    call = (lambda t, n: gml._lib.model_exact(t, n, pairs=False)[0]) if k is None else (lambda t, n: gml._lib.model_best_states(t, n, k)[1][0])
    call(make(12), 12)
    terms = make(sb)
    t0 = time.perf_counter()
    value = call(terms, sb)
    dt = time.perf_counter() - t0
    assert np.isfinite(value)
    print(json.dumps({"case": what, "model": model, "sb": sb, "terms": len(terms), "seconds": dt, "value": float(value)}), flush=True)


def child_cond(h, K, what):
    import gml_amd as gml
    L = gml._lib.lib()
    n = 1024
    keys, wts = dense_pairwise_arrays(n)
    hidden = np.zeros(n, dtype=np.uint8)
    hidden[np.random.default_rng(1).permutation(n)[:h]] = 1

    def call(ev):
        K = ev.K
        lp = np.zeros(K)
        t0 = time.perf_counter()
        if what == "exact":
            means, lw = np.zeros((h, K)), np.zeros(K)
            rc = L.gml_conditional_exact(ptr(keys), 2, ptr(wts), len(wts), n, ev._h, ptr(hidden), ptr(means), ptr(lw), ptr(lp))
            value = lw[0]
        else:
            st, en = np.zeros((h, K), dtype=np.int8), np.zeros(K)
            rc = L.gml_conditional_mode(ptr(keys), 2, ptr(wts), len(wts), n, ev._h, ptr(hidden), ptr(st), ptr(en),
                                        ptr(lp) if what == "mode_log_p" else None)
            value = en[0]
        dt = time.perf_counter() - t0
        assert rc == 0, L.gml_last_error().decode()
        split = np.zeros(3)
        L.gml_test_cond_exact_times(ptr(split))
        return dt, split.tolist(), float(value)

    with gml.Problem(spins=rows(64, n, 2)) as warm:
        call(warm)
    with gml.Problem(spins=rows(K, n, 3)) as ev:
        dt, split, value = call(ev)
    print(json.dumps({"case": what, "n": n, "terms": len(wts), "h": h, "K": K, "seconds": dt, "host_s": split[0], "slabs_s": split[1],
                      "value": value}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[24, 30, 36])
    ap.add_argument("--ascending", type=int, default=30, help="sb of the ascending-energy model (0: leave it out)")
    ap.add_argument("--no-cond", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds a child may take")
    ap.add_argument("--child", choices=["model", "cond"])
    ap.add_argument("--what", default="logz")
    ap.add_argument("--model", default="dense")
    ap.add_argument("--sb", type=int, default=24)
    ap.add_argument("--h", type=int, default=12)
    ap.add_argument("--K", type=int, default=10000)
    args = ap.parse_args()
    if args.child == "model":
        return child_model(args.sb, args.what, args.model)
    if args.child == "cond":
        return child_cond(args.h, args.K, args.what)
    cases = [["--child", "model", "--sb", str(sb), "--what", what] for sb in args.sizes for what in ("logz", "best1", "best256")]
    if args.ascending:
        cases += [["--child", "model", "--model", "ascending", "--sb", str(args.ascending), "--what", what]
                  for what in ("logz", "best1", "best256")]
    if not args.no_cond:
        cases += [["--child", "cond", "--h", str(h), "--K", str(K), "--what", what] for h, K in COND
                  for what in ("exact", "mode_log_p", "mode")]
    for case in cases:
        recs = []
        for _ in range(args.repeats):
            r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__)] + case, capture_output=True,
                               text=True)
            if r.returncode != 0:
                print(json.dumps({"case": case, "failed": r.returncode, "stderr": r.stderr[-400:]}), flush=True)
                return 1
            recs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        out = dict(recs[0])
        for key in ("seconds", "host_s", "slabs_s"):
            if key in out:
                out[key] = statistics.median(rec[key] for rec in recs)
        out["all_s"] = [rec["seconds"] for rec in recs]
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
