"""Per lane-sweep time of k_ais_chains (one sweep per step on a linear schedule) next to the unchanged k_term_chains -- the same
65 536 lanes, one process, the runs interleaved -- on the three models of gpu_term_chains_bench.py:
  (a) the 64 x 64 periodic lattice with fields, (b) sparse order 3 with n = 1024, (c) dense pairwise with n = 1024.
A per lane-sweep time is the difference of two runs that differ only in their sweep count, divided by the extra lane-sweeps, so
record building, uploads and the start-energy pass cancel; the median of REPS such differences per kernel, and the ratio of the two
medians.  Then the wall time of log_partition on model (b) with 4096 chains x 1000 steps.  Prints one line per measurement (JSON)."""
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


def ais_wall(terms, n, steps):
    t0 = time.perf_counter()
    _lib.log_partition_ais(terms, n, LANES, np.linspace(0.0, 1.0, steps + 1), 1, seed=1)
    return time.perf_counter() - t0


def compare(name, terms, n, sweeps):
    order = max(2, max(len(k) for k in terms))
    plain = lambda s: wall(lambda: gml.Problem(terms=terms, n=n, num_samples=LANES, mcmc_sweeps=s, mcmc_thin=1, seed=1, order=order))  # noqa: E731
    ais = lambda s: ais_wall(terms, n, s)  # noqa: E731
    s1, s2 = sweeps
    for run in (plain, ais):  # warm-up (library, code objects, allocator)
        run(s1)
    per = {"k_term_chains": [], "k_ais_chains": []}
    for _ in range(REPS):
        for key, run in (("k_term_chains", plain), ("k_ais_chains", ais)):
            t1, t2 = run(s1), run(s2)
            per[key].append((t2 - t1) / (LANES * (s2 - s1)) * 1e9)
    med = {k: float(np.median(v)) for k, v in per.items()}
    emit(model=name, n=n, lanes=LANES, sweeps_per_step=1, sweeps=list(sweeps), reps=REPS,
         ns_per_lane_sweep={k: [round(x, 3) for x in v] for k, v in per.items()}, median_ns_per_lane_sweep=med,
         ratio_ais_over_plain=med["k_ais_chains"] / med["k_term_chains"])


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
        terms, n = sparse3()
        method = gml.AIS(4096, 1000)
        gml.log_partition(terms, gml.AIS(256, 10), seed=0)  # warm-up
        walls = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            est = gml.log_partition(terms, method, seed=1)
            walls.append(time.perf_counter() - t0)
        emit(model="(b) sparse order 3", n=n, call="log_partition(terms, AIS(4096, 1000), seed=1)", wall_s=[round(w, 4) for w in walls],
             median_wall_s=float(np.median(walls)), log_z=est.log_z, stderr=est.stderr, ess=est.ess)


if __name__ == "__main__":
    main()
