"""Per chain-sweep time of the term-list Glauber kernels at 65 536 chains: k_glauber (one sample per chain, Problem(terms=...,
mcmc_sweeps=S)) and k_term_chains (exact integer fields, Problem(terms=..., mcmc_sweeps=S, mcmc_thin=1)), on
  (a) a 64 x 64 periodic lattice with fields (n = 4096),
  (b) a sparse order-3 model, n = 1024, about 12 three-body and 4 two-body incidences per spin,
  (c) the dense n = 1024 pairwise model of gpu_mcmc_chains_bench.py, also with k_mcmc_chains (Problem(model=..., burn_in=S));
then the wall time of 2^20 samples of (b) held on the device (Problem(), no host histogram): GlauberTermChains(200, 10, 16)
next to Glauber(200).
A per chain-sweep time is the difference of two runs that differ only in their sweep count, divided by the extra chain-sweeps,
so handle building and uploads cancel.  Prints one line per measurement (JSON)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gml_amd as gml  # noqa: E402

CHAINS = 65536


def lattice(L=64, seed=0):
    rng = np.random.default_rng(seed)
    idx = lambda x, y: (x % L) * L + (y % L) + 1  # noqa: E731
    terms = {}
    for x in range(L):
        for y in range(L):
            terms[(idx(x, y), idx(x + 1, y))] = 0.4 * rng.choice([-1.0, 1.0])
            terms[(idx(x, y), idx(x, y + 1))] = 0.4 * rng.choice([-1.0, 1.0])
    for i in range(L * L):
        terms[(i + 1,)] = rng.normal(scale=0.2)
    return terms, L * L


def sparse3(n=1024, seed=0):
    # 4 three-body terms per spin give it 12 incidences, 2 two-body terms 4
    rng = np.random.default_rng(seed)
    terms = {}
    for _ in range(4 * n):
        terms[tuple(int(v) for v in np.sort(rng.choice(n, 3, replace=False)) + 1)] = float(rng.normal(scale=0.25))
    for _ in range(2 * n):
        terms[tuple(int(v) for v in np.sort(rng.choice(n, 2, replace=False)) + 1)] = float(rng.normal(scale=0.25))
    for i in range(n):
        terms[(i + 1,)] = float(rng.normal(scale=0.2))
    return terms, n


def dense(n=1024, seed=0):
    rng = np.random.default_rng(seed)
    J = np.triu(rng.normal(scale=1.0 / np.sqrt(n), size=(n, n)), 1)
    J = J + J.T
    J[np.diag_indices(n)] = rng.normal(scale=0.2, size=n)
    terms = {(i + 1, j + 1): J[i, j] for i in range(n) for j in range(i + 1, n)}
    terms.update({(i + 1,): J[i, i] for i in range(n)})
    return J, terms, n


def wall(make):
    t0 = time.perf_counter()
    with make() as p:
        p.K  # noqa: B018
    return time.perf_counter() - t0


def per_sweep(make, chains, s1, s2):
    wall(lambda: make(s1))  # warm-up (library, code objects, allocator)
    t1, t2 = wall(lambda: make(s1)), wall(lambda: make(s2))
    return (t2 - t1) / (chains * (s2 - s1)), t1, t2


def emit(**kw):
    print(json.dumps(kw), flush=True)


def engines(name, terms, n, glauber_sweeps, chain_sweeps):
    order = max(2, max(len(k) for k in terms))
    ps, t1, t2 = per_sweep(lambda s: gml.Problem(terms=terms, n=n, num_samples=CHAINS, mcmc_sweeps=s, seed=1, order=order), CHAINS,
                           *glauber_sweeps)
    emit(model=name, engine="k_glauber (term list)", n=n, chains=CHAINS, sweeps=list(glauber_sweeps), wall_s=[t1, t2],
         ns_per_chain_sweep=ps * 1e9)
    ps, t1, t2 = per_sweep(lambda s: gml.Problem(terms=terms, n=n, num_samples=CHAINS, mcmc_sweeps=s, mcmc_thin=1, seed=1, order=order),
                           CHAINS, *chain_sweeps)
    emit(model=name, engine="k_term_chains (exact integer fields)", n=n, chains=CHAINS, sweeps=list(chain_sweeps), wall_s=[t1, t2],
         ns_per_chain_sweep=ps * 1e9)


def main():
    which = sys.argv[1:] or ["a", "b", "c", "million"]
    if "a" in which:
        terms, n = lattice()
        engines("(a) 64 x 64 periodic lattice + fields", terms, n, (2, 6), (10, 410))
    if "b" in which:
        terms, n = sparse3()
        engines("(b) sparse order 3", terms, n, (2, 6), (10, 410))
    if "c" in which:
        J, terms, n = dense()
        engines("(c) dense pairwise", terms, n, (1, 2), (2, 42))
        ps, t1, t2 = per_sweep(lambda s: gml.Problem(model=J, num_samples=CHAINS, burn_in=s, thin=1, seed=1), CHAINS, 10, 50)
        emit(model="(c) dense pairwise", engine="k_mcmc_chains (int8 MFMA)", n=n, chains=CHAINS, sweeps=[10, 50], wall_s=[t1, t2],
             ns_per_chain_sweep=ps * 1e9)
    if "million" in which:
        terms, n = sparse3()
        N = 65536 * 16
        wall(lambda: gml.Problem(terms=terms, n=n, num_samples=65536, mcmc_sweeps=2, mcmc_thin=1, seed=0, order=3))  # warm-up
        t = wall(lambda: gml.Problem(terms=terms, n=n, num_samples=N, mcmc_sweeps=200, mcmc_thin=10, mcmc_samples_per_chain=16, seed=1,
                                     order=3))
        emit(model="(b) sparse order 3", sampler="GlauberTermChains(200, 10, 16)", n=n, samples=N, chains=N // 16,
             chain_sweeps=(N // 16) * 350, wall_s=t)
        t = wall(lambda: gml.Problem(terms=terms, n=n, num_samples=N, mcmc_sweeps=200, seed=1, order=3))
        emit(model="(b) sparse order 3", sampler="Glauber(200)", n=n, samples=N, chains=N, chain_sweeps=N * 200, wall_s=t)

if __name__ == "__main__":
    main()
