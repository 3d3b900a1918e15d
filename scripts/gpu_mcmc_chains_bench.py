"""Per chain-sweep time of the two Glauber engines on a dense n = 1024 model with couplings on all pairs: the term-list
kernel (k_glauber, Problem(terms=..., mcmc_sweeps=S)) and the int8 matrix-core kernel (k_mcmc_chains, Problem(model=...,
burn_in=S)); then the matrix-core kernel at 10^6 samples (thinned, and as 10^6 chains x 200 sweeps) and at n = 4096.
A per chain-sweep time is the difference of two runs that differ only in their sweep count, divided by the extra chain-sweeps,
so handle building and uploads cancel.  Prints one line per measurement (JSON)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gml_amd as gml  # noqa: E402


def dense(n, seed=0):
    rng = np.random.default_rng(seed)
    J = np.triu(rng.normal(scale=1.0 / np.sqrt(n), size=(n, n)), 1)
    J = J + J.T
    J[np.diag_indices(n)] = rng.normal(scale=0.2, size=n)
    return J


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


def main():
    which = sys.argv[1:] or ["glauber", "chains", "million", "n4096"]
    J = dense(1024)
    if "glauber" in which:
        terms = {(i + 1, j + 1): J[i, j] for i in range(1024) for j in range(i + 1, 1024)}
        terms.update({(i + 1,): J[i, i] for i in range(1024)})
        ch = 16384
        ps, t1, t2 = per_sweep(lambda s: gml.Problem(terms=terms, n=1024, num_samples=ch, mcmc_sweeps=s, seed=1), ch, 2, 6)
        emit(engine="k_glauber (term list)", n=1024, chains=ch, sweeps=[2, 6], wall_s=[t1, t2], ns_per_chain_sweep=ps * 1e9)
    if "chains" in which:
        for ch in (16384, 65536):
            ps, t1, t2 = per_sweep(lambda s: gml.Problem(model=J, num_samples=ch, burn_in=s, thin=1, seed=1), ch, 10, 50)
            emit(engine="k_mcmc_chains (int8 MFMA)", n=1024, chains=ch, sweeps=[10, 50], wall_s=[t1, t2], ns_per_chain_sweep=ps * 1e9)
    if "million" in which:
        for ch, spc in ((65536, 16), (1000000, 1)):
            t = wall(lambda: gml.Problem(model=J, num_samples=ch * spc, burn_in=200, thin=10, samples_per_chain=spc, seed=1))
            sweeps = 200 + (spc - 1) * 10
            emit(engine="k_mcmc_chains (int8 MFMA)", n=1024, chains=ch, samples_per_chain=spc, burn_in=200, thin=10, samples=ch * spc,
                 chain_sweeps=ch * sweeps, wall_s=t)
    if "n4096" in which:
        J4 = dense(4096, 1)
        ch = 16384
        ps, t1, t2 = per_sweep(lambda s: gml.Problem(model=J4, num_samples=ch, burn_in=s, thin=1, seed=1), ch, 2, 6)
        emit(engine="k_mcmc_chains (int8 MFMA)", n=4096, chains=ch, sweeps=[2, 6], wall_s=[t1, t2], ns_per_chain_sweep=ps * 1e9)


if __name__ == "__main__":
    main()
