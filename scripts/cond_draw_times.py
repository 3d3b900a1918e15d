"""Times of exact draws of hidden spins (gml_conditional_draw) beside what they stand next to.

The uniform case of scripts/cond_exact_times.py: a dense pairwise model with fields on n = 1024 spins (524 800 terms), K = 10^4 evidence
rows, the first h spins of a fixed random order hidden in every row.  Per h, in ONE process: gml_conditional_draw at replicas 1, 2 and
8, each with and without log_p; gml_conditional_mode without log_p (the kernel the draws were built from); the masked chains
(gml_problem_create_mcmc_terms_masked on a mask handle whose rows all hide the same h spins) at ImputationEM's default sampler (10 sweeps
of burn-in, one recorded sample); gml_conditional_means at the default sampler (200 sweeps of burn-in).  Beside every time of an exact
call: the part the library spent in its slabs (upload, launch, drain), from gml_test_cond_exact_times, and for the draws the ratio of
those slabs PER REPLICA to the slabs of the mode call.

Every measurement is a fresh child process under its own time limit: a warm-up call of each entry point on 64 rows (loads the code
objects), then one timed call each, which returns after its stream is synchronised, so the host clock around it is the time of the call.
The term arrays are built before the clock starts.  The driver prints the median of --repeats children per h as one JSON line, and stops
at the first child that fails.

    python scripts/cond_draw_times.py --repeats 3"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cond_exact_times import dense_pairwise, ptr, rows  # noqa: E402

HIDDEN = (12, 16, 20)
REPLICAS = (1, 2, 8)
N, K = 1024, 10000


def split_of(L):
    split = np.zeros(3)
    L.gml_test_cond_exact_times(ptr(split))
    return split.tolist()


def draw_call(L, keys, wts, ev, hidden, replicas, log_p, seed=7):
    """(seconds, slabs seconds) of one gml_conditional_draw with states and energy, and log_p if asked for"""
    chains = ev.K * replicas
    st, en = np.zeros((int(hidden.sum()), chains), dtype=np.int8), np.zeros(chains)
    lp = np.zeros(chains) if log_p else None
    t0 = time.perf_counter()
    rc = L.gml_conditional_draw(ptr(keys), 2, ptr(wts), len(wts), N, ev._h, ptr(hidden), replicas, seed, ptr(st), ptr(en),
                                None if lp is None else ptr(lp))
    dt = time.perf_counter() - t0
    assert rc == 0, L.gml_last_error().decode()
    assert np.all(np.abs(st) == 1) and np.isfinite(en).all() and (lp is None or np.all(lp <= 0))
    return dt, split_of(L)[1]


def mode_call(L, keys, wts, ev, hidden):
    st, en = np.zeros((int(hidden.sum()), ev.K), dtype=np.int8), np.zeros(ev.K)
    t0 = time.perf_counter()
    rc = L.gml_conditional_mode(ptr(keys), 2, ptr(wts), len(wts), N, ev._h, ptr(hidden), ptr(st), ptr(en), None)
    dt = time.perf_counter() - t0
    assert rc == 0, L.gml_last_error().decode()
    return dt, split_of(L)[1]


def chains_call(L, keys, wts, ev, mask, sampler):
    """seconds of the masked chains at `sampler`, one replica: the handle made, synchronised and destroyed outside the clock"""
    h = C.c_void_p()
    t0 = time.perf_counter()
    rc = L.gml_problem_create_mcmc_terms_masked(ptr(keys), 2, ptr(wts), len(wts), N, ev._h, mask._h, 1, sampler.samples_per_chain,
                                                sampler.burn_in, sampler.thin, 7, 2, 0, N, C.byref(h))
    dt = time.perf_counter() - t0
    assert rc == 0, L.gml_last_error().decode()
    L.gml_problem_destroy(h)
    return dt


def means_call(L, keys, wts, ev, hidden, sampler):
    out = np.zeros((int(hidden.sum()), ev.K))
    t0 = time.perf_counter()
    rc = L.gml_conditional_means(ptr(keys), 2, ptr(wts), len(wts), N, ev._h, ptr(hidden), 1, sampler.samples_per_chain, sampler.burn_in,
                                 sampler.thin, 7, ptr(out))
    dt = time.perf_counter() - t0
    assert rc == 0, L.gml_last_error().decode()
    return dt


def child(h):
    import gml_amd as gml
    L = gml._lib.lib()
    keys, wts = dense_pairwise(N)
    hidden = np.zeros(N, dtype=np.uint8)
    hidden[np.random.default_rng(1).permutation(N)[:h]] = 1
    em_sampler, default_sampler = gml.ImputationEM().sampler, gml.GlauberTermChains()

    def mask_of(rows_):
        return gml.Problem(spins=np.where(hidden[None, :] != 0, -1, 1).astype(np.int8).repeat(rows_, axis=0))

    with gml.Problem(spins=rows(64, N, 2)) as warm, mask_of(64) as wm:
        draw_call(L, keys, wts, warm, hidden, 2, True)
        draw_call(L, keys, wts, warm, hidden, 2, False)
        mode_call(L, keys, wts, warm, hidden)
        chains_call(L, keys, wts, warm, wm, em_sampler)
        means_call(L, keys, wts, warm, hidden, default_sampler)
    out = {"n": N, "terms": len(wts), "h": h, "K": K}
    with gml.Problem(spins=rows(K, N, 3)) as ev, mask_of(K) as mk:
        out["mode_s"], out["mode_slabs_s"] = mode_call(L, keys, wts, ev, hidden)
        for r in REPLICAS:
            for log_p in (False, True):
                tag = f"draw_r{r}_{'logp' if log_p else 'only'}"
                out[tag + "_s"], out[tag + "_slabs_s"] = draw_call(L, keys, wts, ev, hidden, r, log_p)
                out[tag + "_slabs_per_replica_over_mode"] = out[tag + "_slabs_s"] / r / out["mode_slabs_s"]
        out["masked_chains_em_sampler_s"] = chains_call(L, keys, wts, ev, mk, em_sampler)
        out["means_default_sampler_s"] = means_call(L, keys, wts, ev, hidden, default_sampler)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=180, help="seconds a child may take")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--h", type=int, default=12)
    ap.add_argument("--hidden", type=int, nargs="+", default=list(HIDDEN), help="the numbers of hidden spins to time")
    args = ap.parse_args()
    if args.child:
        return child(args.h)
    for h in args.hidden:
        recs = []
        for _ in range(args.repeats):
            r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--h", str(h)],
                               capture_output=True, text=True)
            if r.returncode != 0:
                print(json.dumps({"h": h, "failed": r.returncode, "stderr": r.stderr[-400:]}), flush=True)
                return 1
            recs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        out = {key: (statistics.median(rec[key] for rec in recs) if isinstance(val, float) else val) for key, val in recs[0].items()}
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
