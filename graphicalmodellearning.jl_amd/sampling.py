"""sample(model, N): host mirror of the reference's sampler front door (src/sampling.jl:90-106) on top of
the on-device exact sampler (gml_problem_create_sampled / _sampled_terms).  Any interaction order; every
connected component of the term hypergraph must have at most 22 spins (the reference enumerates all 2^n
states of the whole model, which limits it to n ~ 25).  Beyond that, Markov chains on the device: Glauber (one sample per
chain), GlauberChains (long thinned chains of dense pairwise models), GlauberTermChains (long thinned chains of any term
list) and TemperedTermChains (replica exchange on those, for models with more than one deep well).  Sparse models of any size --
lattices, Chimera graphs, trees, l1 solutions -- need no chain: Elimination() (the class of likelihood.py) draws exactly and
independently by backward sampling on the tables of variable elimination (gml_problem_create_sampled_elim)."""
import numpy as np

from . import _lib
from .factor_graph import FactorGraph


class GMSampler:  # sampling.jl:7
    pass


class Gibbs(GMSampler):  # sampling.jl:9  (the reference's "Gibbs" sampler is exact enumeration, as is this one)
    pass


class Glauber(GMSampler):
    """Not in the reference: N independent heat-bath chains of `sweeps` sweeps on the device, for models whose
    connected components exceed the 22 spins exact enumeration can handle (gml_problem_create_mcmc_terms)."""

    def __init__(self, sweeps=200):
        self.sweeps = int(sweeps)


class GlauberChains(GMSampler):
    """Not in the reference: long heat-bath chains of a PAIRWISE model on the int8 matrix cores
    (gml_problem_create_mcmc_chains): N // samples_per_chain chains, each burnt in for `burn_in` sweeps and then recorded
    every `thin` sweeps, samples_per_chain times.  Its cost is n^2 per chain-sweep whatever the density, so it serves dense
    models (SK-type glasses, learned models) at the sizes learn() handles; sparse and multi-body models go to GlauberTermChains."""

    def __init__(self, burn_in=200, thin=10, samples_per_chain=1):
        self.burn_in, self.thin, self.samples_per_chain = int(burn_in), int(thin), int(samples_per_chain)


class GlauberTermChains(GMSampler):
    """Not in the reference: long heat-bath chains of ANY term list (any order up to 8, any sparsity; n <= 16384)
    (gml_problem_create_mcmc_terms_chains): N // samples_per_chain chains, each burnt in for `burn_in` sweeps and then recorded
    every `thin` sweeps, samples_per_chain times.  Couplings are quantised per spin to 2^-38 of its largest one and the fields
    summed exactly, so the draws depend only on the model, the seed and these three numbers; on a pairwise model they are the
    draws of GlauberChains, bit for bit.  Its cost per chain-sweep follows the number of incidences (sparse models, lattices,
    multi-body models learned by multiRISE / ISODUS)."""

    def __init__(self, burn_in=200, thin=10, samples_per_chain=1):
        self.burn_in, self.thin, self.samples_per_chain = int(burn_in), int(thin), int(samples_per_chain)


class TemperedTermChains(GMSampler):
    """Not in the reference: replica exchange (parallel tempering) on the chains of GlauberTermChains
    (gml_problem_create_mcmc_terms_tempered), for models with more than one deep well -- a ferromagnet below its transition, a glass
    at low temperature, a sharply learned model -- where a single-temperature chain stays in the well it started in.
    N // samples_per_chain ladders of `replicas` chains (1, 2, 4 .. 64) at the inverse temperatures `betas` (non-increasing, the first
    positive; default: geometric from 1 down to beta_min); neighbouring rungs try to exchange their states every `swap_every`
    sweeps; the rung at betas[0] is recorded.  After sample(), swap_rates holds accepts / attempts per neighbouring pair (of the last
    replicate): a rate near 0 asks for more rungs or a larger beta_min between those two."""

    def __init__(self, burn_in=200, thin=10, samples_per_chain=1, replicas=8, beta_min=0.1, betas=None, swap_every=1):
        self.burn_in, self.thin, self.samples_per_chain = int(burn_in), int(thin), int(samples_per_chain)
        self.swap_every = int(swap_every)
        if betas is not None:
            self.betas = [float(b) for b in betas]
        else:
            R = int(replicas)
            if R < 1:
                raise ValueError(f"replicas must be at least 1 (given {replicas})")
            self.betas = [float(beta_min) ** (r / (R - 1)) for r in range(R)] if R > 1 else [1.0]
        self.replicas = len(self.betas)
        self.swap_rates = None


def _problem_args(model):
    """Keyword arguments of _lib.Problem for a model: matrix (order <= 2, :98-99) or term list (:100-101)."""
    if isinstance(model, FactorGraph):
        if model.alphabet != "spin":
            raise ValueError(f"sampling is only supported for spin FactorGraphs, given alphabet {model.alphabet}")  # :97
        if model.order <= 2:
            return {"model": model.to_matrix()}
        return {"terms": model.terms, "n": model.varible_count, "order": model.order}
    if isinstance(model, dict):
        return {"terms": model, "order": max(2, max(len(k) for k in model))}
    return {"model": np.asarray(model, dtype=np.float64)}


def _term_list_args(model, args):
    """The arguments of a pairwise model as a term list: the chains of Glauber and GlauberTermChains run on term lists."""
    if "model" not in args:
        return args
    fg = model if isinstance(model, FactorGraph) else FactorGraph(np.asarray(model, dtype=np.float64))
    return {"terms": fg.terms, "n": fg.varible_count, "order": 2}


def _check_whole_chains(number_sample, sampler):
    if int(number_sample) % sampler.samples_per_chain != 0:
        raise ValueError(f"the number of samples ({number_sample}) must be a multiple of samples_per_chain "
                         f"({sampler.samples_per_chain})")


def sample(model, number_sample, replicates=None, sampler=None, *, seed=0, device=0):
    """sample(gm, N) -> histogram matrix [count, s_1..s_n], one row per observed configuration
    (sampling.jl:52-54); sample(gm, N, replicates) -> list of such matrices (:91).  sampler: None or Gibbs() for exact enumeration, one
    of the chain samplers above, or an Elimination for exact draws of a sparse model (planned on the host first: ValueError where the
    order is wider than its max_width)."""
    from .likelihood import Elimination, _check_elimination  # (likelihood.py imports this module)
    args = _problem_args(model)
    if isinstance(sampler, GlauberChains):
        if "model" not in args:
            raise ValueError("GlauberChains samples pairwise models (order <= 2) only; use Glauber for multi-body models")
        _check_whole_chains(number_sample, sampler)
        args.update(burn_in=sampler.burn_in, thin=sampler.thin, samples_per_chain=sampler.samples_per_chain)
    elif isinstance(sampler, GlauberTermChains):
        args = _term_list_args(model, args)
        _check_whole_chains(number_sample, sampler)
        args.update(mcmc_sweeps=sampler.burn_in, mcmc_thin=sampler.thin, mcmc_samples_per_chain=sampler.samples_per_chain)
    elif isinstance(sampler, TemperedTermChains):
        args = _term_list_args(model, args)
        _check_whole_chains(number_sample, sampler)
        args.update(mcmc_sweeps=sampler.burn_in, mcmc_thin=sampler.thin, mcmc_samples_per_chain=sampler.samples_per_chain,
                    mcmc_betas=sampler.betas, mcmc_swap_every=sampler.swap_every)
    elif isinstance(sampler, Glauber):
        args = _term_list_args(model, args)
        args["mcmc_sweeps"] = sampler.sweeps
    elif isinstance(sampler, Elimination):
        args = _term_list_args(model, args)
        _check_elimination(sampler, args["terms"], args.get("n"))
        args.update(elim=True, elim_order=sampler.order)
    reps = 1 if replicates is None else int(replicates)
    nspins = args["model"].shape[0] if "model" in args else args["n"] if "n" in args else max(max(k) for k in args["terms"] if len(k))
    out = []
    for b in range(reps):
        kw = dict(num_samples=int(number_sample), seed=int(seed) + 7919 * b, device=device, **args)
        if nspins <= 64 and int(number_sample) < 2 ** 31:
            # countmap (sampling.jl:52) on the device: the draws are sorted and run-length encoded there; only the distinct
            # configurations and their counts come back
            with _lib.Problem(histogram=True, **kw) as p:
                states, counts, swaps = p.spins(), p.counts(), p.swap_counts
            order = np.lexsort(states.T[::-1])  # rows in the order np.unique would give them
            states, counts = states[order], counts[order]
        else:
            with _lib.Problem(**kw) as p:
                spins, swaps = p.spins(), p.swap_counts
            states, counts = np.unique(spins, axis=0, return_counts=True)
        if isinstance(sampler, TemperedTermChains):
            # (a pair without a swap round -- swap_every above the sweep count -- has no rate: NaN)
            sampler.swap_rates = np.divide(swaps[1], swaps[0], out=np.full(swaps.shape[1], np.nan), where=swaps[0] > 0)
        out.append(np.concatenate([np.rint(counts)[:, None].astype(np.int64), states.astype(np.int64)], axis=1))
    return out[0] if replicates is None else out
