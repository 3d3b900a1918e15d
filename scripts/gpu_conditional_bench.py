"""Per lane-sweep time of k_cond_chains on the three models of gpu_term_chains_bench.py -- (a) the 64 x 64 periodic lattice with
fields, (b) sparse order 3 with n = 1024, (c) dense pairwise with n = 1024 -- at 65 536 lanes, one process, the runs interleaved:
  H = n     every spin hidden, against the unchanged k_term_chains (the yardstick) on the same build;
  H = n/8   a fixed random hidden set, the full walk (gml_test_cond_split(0)) against the split of the field into a per-chain
            constant and a live part (gml_test_cond_split(2): wherever a record allows it) and against the default
            (gml_test_cond_split(1): the host's rule picks one of the two).  A sweep here visits the H hidden spins only.
A per lane-sweep time is the difference of two runs that differ only in their sweep count, divided by the extra lane-sweeps, so
record building, uploads, the start pass and the handle cancel; the median of REPS such differences, and their spread (max - min).
Then the wall time of conditional_means on model (c): 100 000 evidence rows, 32 hidden spins, 100 sweeps.  Prints one line per
measurement (JSON)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gml_amd as gml  # noqa: E402
from gml_amd import _lib  # noqa: E402
from gpu_term_chains_bench import dense, lattice, sparse3, wall  # noqa: E402

LANES, REPS = 65536, 5


def emit(**kw):
    print(json.dumps(kw), flush=True)


def rows(K, n, seed=0):
    return np.where(np.random.default_rng(seed).random((K, n)) < 0.5, -1, 1).astype(np.int8)


def split_hook():
    f = _lib.lib().gml_test_cond_split
    f.argtypes, f.restype = [C.c_int], C.c_int
    return f


def summary(per):
    return ({k: [round(x, 3) for x in v] for k, v in per.items()}, {k: float(np.median(v)) for k, v in per.items()},
            {k: float(max(v) - min(v)) for k, v in per.items()})


def interleaved(runs, sweeps, lane_sweeps):
    """runs: {name: f(sweeps) -> wall seconds}; ns per lane-sweep of every run, REPS times, interleaved"""
    s1, s2 = sweeps
    for run in runs.values():  # warm-up (library, code objects, allocator)
        run(s1)
    per = {k: [] for k in runs}
    for _ in range(REPS):
        for key, run in runs.items():
            t1, t2 = run(s1), run(s2)
            per[key].append((t2 - t1) / (lane_sweeps * (s2 - s1)) * 1e9)
    return per


def compare(name, terms, n, sweeps):
    order = max(2, max(len(k) for k in terms))
    split = split_hook()
    with gml.Problem(spins=rows(LANES, n)) as ev:
        def cond(hidden, on):
            def run(s):
                split(on)
                try:
                    return wall(lambda: _lib.conditional_chains(terms, n, ev, hidden, 1, 1, s, 1, seed=1, order=order))
                finally:
                    split(1)
            return run
        plain = lambda s: wall(lambda: gml.Problem(terms=terms, n=n, num_samples=LANES, mcmc_sweeps=s, mcmc_thin=1, seed=1, order=order))  # noqa: E731
        per = interleaved({"k_term_chains": plain, "k_cond_chains": cond(np.arange(n), 1)}, sweeps, LANES)
        runs, med, spread = summary(per)
        emit(model=name, n=n, hidden=n, lanes=LANES, sweeps=list(sweeps), reps=REPS, ns_per_lane_sweep=runs, median_ns_per_lane_sweep=med,
             spread_ns=spread, ratio_cond_over_plain=med["k_cond_chains"] / med["k_term_chains"])
        hidden = np.sort(np.random.default_rng(1).choice(n, n // 8, replace=False))
        wide = (sweeps[0] * 8, sweeps[1] * 8)  # (a sweep over n / 8 spins: about the same wall time as above)
        per = interleaved({"full_walk": cond(hidden, 0), "split": cond(hidden, 2), "default": cond(hidden, 1)}, wide, LANES)
        runs, med, spread = summary(per)
        emit(model=name, n=n, hidden=int(len(hidden)), lanes=LANES, sweeps=list(wide), reps=REPS, ns_per_lane_sweep=runs,
             median_ns_per_lane_sweep=med, spread_ns=spread, ratio_split_over_full=med["split"] / med["full_walk"],
             ratio_default_over_full=med["default"] / med["full_walk"])


def whole_call():
    _, terms, n = dense()
    split = split_hook()
    hidden = [int(i) + 1 for i in np.sort(np.random.default_rng(2).choice(n, 32, replace=False))]
    sampler = gml.GlauberTermChains(burn_in=100, thin=1, samples_per_chain=1)
    with gml.Problem(spins=rows(100000, n)) as ev:
        gml.conditional_means(terms, ev, hidden, gml.GlauberTermChains(burn_in=2, thin=1), seed=0)  # warm-up
        for on in (1, 0):  # (the default takes the split here; 0: the full walk)
            split(on)
            try:
                walls = []
                for _ in range(REPS):
                    t0 = time.perf_counter()
                    cm = gml.conditional_means(terms, ev, hidden, sampler, seed=1)
                    walls.append(time.perf_counter() - t0)
            finally:
                split(1)
            emit(model="(c) dense pairwise", n=n, call="conditional_means(terms, evidence [100000 rows], 32 hidden, burn_in=100)",
                 split=bool(on), wall_s=[round(w, 4) for w in walls], median_wall_s=float(np.median(walls)),
                 mean_abs_mean=float(np.abs(cm.means).mean()))


def main():
    which = sys.argv[1:] or ["a", "b", "c", "call"]
    if "a" in which:
        compare("(a) 64 x 64 periodic lattice + fields", *lattice(), (10, 210))
    if "b" in which:
        compare("(b) sparse order 3", *sparse3(), (10, 410))
    if "c" in which:
        _, terms, n = dense()
        compare("(c) dense pairwise", terms, n, (2, 22))
    if "call" in which:
        whole_call()


if __name__ == "__main__":
    main()
