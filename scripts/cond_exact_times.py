"""Times of exact conditional inference (gml_conditional_exact, gml_conditional_exact_masked).

Uniform case: a dense pairwise model with fields on n = 1024 spins (524 800 terms), K evidence rows, the first h spins of a fixed random
order hidden in every row; all three outputs.  Beside the time: states per second (K 2^h / seconds), and the time gml_conditional_means
takes on the same rows at the default sampler (GlauberTermChains(): one replica, 200 sweeps of burn-in, one recorded sample).
Masked case: dense pairwise on n = 64, K = 4096 rows, every entry missing with probability 0.1; beside the time the number of distinct
hidden sets and the host's share of the call (checks, download and grouping of the mask's bits, one plan per distinct set), which the
library reports through gml_test_cond_exact_times.

Every measurement is a fresh child process under its own time limit: a warm-up call of each entry point on 64 rows (loads the code
objects), then one timed call, which returns after its stream is synchronised, so the host clock around it is the time of the call.
The term arrays are built before the clock starts.  The driver prints the median of --repeats children per case as one JSON line, and
stops at the first child that fails.

    python scripts/cond_exact_times.py --repeats 3"""
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

UNIFORM = [(1, 10000), (8, 10000), (12, 10000), (16, 10000), (20, 10000), (24, 256)]  # (h, K)


def dense_pairwise(n, seed=0):
    """(keys int32 [T, 2], weights [T]): fields, then the pairs i < j"""
    rng = np.random.default_rng(seed)
    i, j = np.triu_indices(n, 1)
    keys = np.concatenate([np.stack([np.arange(n), np.full(n, -1)], axis=1), np.stack([i, j], axis=1)]).astype(np.int32)
    wts = np.concatenate([rng.normal(scale=0.1, size=n), rng.normal(scale=0.5 / np.sqrt(n), size=len(i))])
    return np.ascontiguousarray(keys), wts


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def rows(K, n, seed):
    return np.where(np.random.default_rng(seed).random((K, n)) < 0.5, -1, 1).astype(np.int8)


def exact_call(L, keys, wts, n, ev, hidden=None, mask=None):
    """one call with all three outputs: (seconds, [host, slabs, total] seconds as the library saw them, log_w)"""
    K = ev.K
    means, lw, lp = np.zeros(((int(hidden.sum()) if mask is None else n), K)), np.zeros(K), np.zeros(K)
    t0 = time.perf_counter()
    if mask is None:
        rc = L.gml_conditional_exact(ptr(keys), keys.shape[1], ptr(wts), len(wts), n, ev._h, ptr(hidden), ptr(means), ptr(lw), ptr(lp))
    else:
        rc = L.gml_conditional_exact_masked(ptr(keys), keys.shape[1], ptr(wts), len(wts), n, ev._h, mask._h, ptr(means), ptr(lw), ptr(lp))
    dt = time.perf_counter() - t0
    assert rc == 0, L.gml_last_error().decode()
    assert np.isfinite(means).all() and np.isfinite(lw).all() and np.isfinite(lp).all()
    split = np.zeros(3)
    L.gml_test_cond_exact_times(ptr(split))
    return dt, split.tolist(), lw


def child_uniform(h, K):
    import gml_amd as gml
    L = gml._lib.lib()
    n = 1024
    keys, wts = dense_pairwise(n)
    hidden = np.zeros(n, dtype=np.uint8)
    hidden[np.random.default_rng(1).permutation(n)[:h]] = 1
    sampler = gml.GlauberTermChains()
    chain_args = (1, sampler.samples_per_chain, sampler.burn_in, sampler.thin, 0)
    with gml.Problem(spins=rows(64, n, 2)) as warm:
        exact_call(L, keys, wts, n, warm, hidden)
        assert L.gml_conditional_means(ptr(keys), 2, ptr(wts), len(wts), n, warm._h, ptr(hidden), *chain_args, ptr(np.zeros((h, 64)))) == 0
    with gml.Problem(spins=rows(K, n, 3)) as ev:
        dt, split, lw = exact_call(L, keys, wts, n, ev, hidden)
        cm = np.zeros((h, K))
        t0 = time.perf_counter()
        rc = L.gml_conditional_means(ptr(keys), 2, ptr(wts), len(wts), n, ev._h, ptr(hidden), *chain_args, ptr(cm))
        chain_dt = time.perf_counter() - t0
        assert rc == 0, L.gml_last_error().decode()
    print(json.dumps({"case": "uniform", "n": n, "terms": len(wts), "h": h, "K": K, "seconds": dt, "host_s": split[0], "slabs_s": split[1],
                      "states_per_s": K * 2.0 ** h / dt, "chain_seconds": chain_dt, "log_w0": float(lw[0])}), flush=True)


def child_masked():
    import gml_amd as gml
    L = gml._lib.lib()
    n, K = 64, 4096
    keys, wts = dense_pairwise(n)
    missing = np.random.default_rng(4).random((K, n)) < 0.1
    patterns = len({r.tobytes() for r in np.packbits(missing, axis=1)})
    with gml.Problem(spins=rows(64, n, 2)) as warm, gml.Problem(spins=np.where(missing[:64], -1, 1).astype(np.int8)) as wm:
        exact_call(L, keys, wts, n, warm, mask=wm)
    with gml.Problem(spins=rows(K, n, 3)) as ev, gml.Problem(spins=np.where(missing, -1, 1).astype(np.int8)) as mk:
        dt, split, lw = exact_call(L, keys, wts, n, ev, mask=mk)
    print(json.dumps({"case": "masked", "n": n, "terms": len(wts), "K": K, "patterns": patterns, "most_holes": int(missing.sum(axis=1).max()),
                      "states": float(np.sum(2.0 ** missing.sum(axis=1))), "seconds": dt, "host_s": split[0], "slabs_s": split[1],
                      "host_share": split[0] / split[2], "log_w0": float(lw[0])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds a child may take")
    ap.add_argument("--child", choices=["uniform", "masked"])
    ap.add_argument("--h", type=int, default=1)
    ap.add_argument("--K", type=int, default=10000)
    args = ap.parse_args()
    if args.child == "uniform":
        return child_uniform(args.h, args.K)
    if args.child == "masked":
        return child_masked()
    cases = [["--child", "uniform", "--h", str(h), "--K", str(K)] for h, K in UNIFORM] + [["--child", "masked"]]
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
        for key in ("seconds", "host_s", "slabs_s", "states_per_s", "chain_seconds", "host_share"):
            if key in out:
                out[key] = statistics.median(rec[key] for rec in recs)
        out["all_s"] = [rec["seconds"] for rec in recs]
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
