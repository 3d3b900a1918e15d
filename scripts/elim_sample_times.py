"""Times of exact draws by backward sampling on the elimination's tables (gml_problem_create_sampled_elim), beside the route such
models took before: GlauberTermChains(burn_in=200), one recorded sample per chain, at the same N on the same model.

Per model: the plan (width, stored), the number of forward launches the walk covers, and the whole-call time of each sampler -- from
the call of _lib.Problem(...) to its return, which is after the stream is synchronised and the handle is built (the forward pass, the
walk and the packing of the N rows for the draws; burn-in, recording and packing for the chains).  Models: the 16 x 16 lattice and
Chimera C4 at N = 1e6, the 16 384-spin width-6 tree at N = 65 536 (the models of scripts/elim_times.py).  The chains' draws are
correlated with their start and with the model's wells; the times say what each route costs, not that the two give the same thing.

One process: a warm-up call of each sampler on a small model (loads the code objects), then --repeats timed calls per case; the
median is printed as one JSON line per case.

    python scripts/elim_sample_times.py --repeats 3 [--model lattice_16x16]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _elim_reference as R  # noqa: E402  (the models of the tests)

MODELS = {
    "lattice_16x16": (lambda: R.lattice(16, 16), 1000000),
    "chimera_4": (lambda: R.chimera(4), 1000000),
    "tree_16384": (lambda: R.tree(16384, back=8), 65536),
}


def timed(make, repeats):
    secs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        p = make()
        secs.append(time.perf_counter() - t0)
        K = p.K
        p.close()
    return K, statistics.median(secs), secs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--model", choices=sorted(MODELS), action="append", help="only these (default: all three)")
    args = ap.parse_args()
    import gml_amd as gml
    lib = gml._lib
    small, ns = R.lattice(4, 4)
    lib.Problem(terms=small, n=ns, num_samples=256, elim=True).close()
    lib.Problem(terms=small, n=ns, num_samples=256, mcmc_sweeps=10, mcmc_thin=1).close()
    for name in args.model or list(MODELS):
        make, N = MODELS[name]
        terms, n = make()
        _, width, _, stored = lib.model_elim_plan(terms, n)
        rec = {"model": name, "n": n, "terms": len(terms), "width": width, "stored": stored, "N": N}
        K, secs, all_s = timed(lambda: lib.Problem(terms=terms, n=n, num_samples=N, seed=1, elim=True), args.repeats)
        assert K == N
        rec.update(elim_s=secs, elim_all_s=all_s, elim_samples_per_s=N / secs)
        K, secs, all_s = timed(lambda: lib.Problem(terms=terms, n=n, num_samples=N, seed=1, mcmc_sweeps=200, mcmc_thin=10,
                                                   mcmc_samples_per_chain=1), args.repeats)
        assert K == N
        rec.update(chains_s=secs, chains_all_s=all_s, chains_over_elim=secs / rec["elim_s"])
        print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
