"""Per lane-sweep time of k_tempered_chains (8 rungs per ladder, swap_every = 1: 8192 ladders) next to the unchanged k_term_chains
(65 536 chains) -- the same 65 536 lanes, one process, the runs interleaved -- on the three models of gpu_term_chains_bench.py:
  (a) the 64 x 64 periodic lattice with fields, (b) sparse order 3 with n = 1024, (c) dense pairwise with n = 1024.
A per lane-sweep time is the difference of two runs that differ only in their sweep count, divided by the extra lane-sweeps, so
handle building and uploads cancel; the median of REPS such differences per kernel, and the ratio of the two medians.  Then the
wall time of the sampling call of the two-well distribution test (tests/test_gpu_tempered.py: 16 spins, 16 384 ladders of 8, 300
sweeps).  Prints one line per measurement (JSON)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gml_amd as gml  # noqa: E402
from gpu_term_chains_bench import dense, lattice, sparse3, wall  # noqa: E402

LANES, R, REPS = 65536, 8, 5


def emit(**kw):
    print(json.dumps(kw), flush=True)


def compare(name, terms, n, sweeps):
    order = max(2, max(len(k) for k in terms))
    betas = gml.TemperedTermChains(replicas=R, beta_min=0.1).betas
    plain = lambda s: gml.Problem(terms=terms, n=n, num_samples=LANES, mcmc_sweeps=s, mcmc_thin=1, seed=1, order=order)  # noqa: E731
    tempered = lambda s: gml.Problem(terms=terms, n=n, num_samples=LANES // R, mcmc_sweeps=s, mcmc_thin=1, mcmc_betas=betas,  # noqa: E731
                                     mcmc_swap_every=1, seed=1, order=order)
    s1, s2 = sweeps
    for make in (plain, tempered):  # warm-up (library, code objects, allocator)
        wall(lambda: make(s1))
    per = {"k_term_chains": [], "k_tempered_chains": []}
    for _ in range(REPS):
        for key, make in (("k_term_chains", plain), ("k_tempered_chains", tempered)):
            t1, t2 = wall(lambda: make(s1)), wall(lambda: make(s2))
            per[key].append((t2 - t1) / (LANES * (s2 - s1)) * 1e9)
    med = {k: float(np.median(v)) for k, v in per.items()}
    emit(model=name, n=n, lanes=LANES, replicas=R, swap_every=1, sweeps=list(sweeps), reps=REPS,
         ns_per_lane_sweep={k: [round(x, 3) for x in v] for k, v in per.items()}, median_ns_per_lane_sweep=med,
         ratio_tempered_over_plain=med["k_tempered_chains"] / med["k_term_chains"])


def bimodal_16():
    terms = {(i + 1, j + 1): 0.35 for i in range(16) for j in range(i + 1, 16)}
    rng = np.random.default_rng(6)
    for _ in range(12):
        terms[tuple(int(v) for v in np.sort(rng.choice(16, 3, replace=False)) + 1)] = float(rng.normal(scale=0.2))
    for i in range(16):
        terms[(i + 1,)] = float(rng.normal(scale=0.03) + 0.02)
    return terms


def main():
    which = sys.argv[1:] or ["a", "b", "c", "test"]
    if "a" in which:
        compare("(a) 64 x 64 periodic lattice + fields", *lattice(), (10, 210))
    if "b" in which:
        compare("(b) sparse order 3", *sparse3(), (10, 410))
    if "c" in which:
        _, terms, n = dense()
        compare("(c) dense pairwise", terms, n, (2, 22))
    if "test" in which:
        terms = bimodal_16()
        sampler = gml.TemperedTermChains(burn_in=300, thin=1, samples_per_chain=1, replicas=8, beta_min=0.1)
        gml.sample(terms, 1024, sampler=sampler, seed=0)  # warm-up
        walls = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            gml.sample(terms, 16384, sampler=sampler, seed=1)
            walls.append(time.perf_counter() - t0)
        emit(model="two wells, 16 spins", call="sample(terms, 16384, TemperedTermChains(300, 1, 1, replicas=8, beta_min=0.1))",
             wall_s=[round(w, 4) for w in walls], median_wall_s=float(np.median(walls)), swap_rates=sampler.swap_rates.tolist())


if __name__ == "__main__":
    main()
