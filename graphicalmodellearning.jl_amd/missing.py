"""learn_missing(samples, formulation, method, em): learn() for data with holes, by stochastic-imputation EM.

Every iteration completes the data under the current model -- the missing entries of a row are drawn from the model's conditional
distribution given the row's observed entries, by the per-row masked chains (gml_problem_create_mcmc_terms_masked) -- and learns on
the completed handle, started from the previous solution.  With ImputationEM(method=Exact()) the draws are exact instead: every row's
missing entries are enumerated (gml_conditional_draw_masked, at most 24 per row), so the completions come from p(missing | observed)
itself and no burn-in has to be guessed.  Iteration 0 completes under the empty model: coin flips, the baseline that
shrinks every coupling towards zero.

What the estimator is.  Data completed from p_theta*(missing | observed) are distributed as p_theta*, so the true model is a fixed
point of the iteration for any consistent M-step, RISE included.  That holds for entries missing at random: whether an entry is
missing may depend on what the row shows, not on the value the hole hides.  What it is not: the iterates are random (each imputation
is a draw), there is no convergence test -- `trace` is there to be looked at -- and nothing here models missingness that depends on
the hidden value."""
from dataclasses import dataclass, field
from importlib import import_module

import numpy as np

from . import _lib, inference
from .factor_graph import FactorGraph, TermArray
from .formulations import HIP, NLP, RISE, GMLFormulation, GMLMethod, multiRISE
from .likelihood import Exact
from .sampling import GlauberTermChains

_learn = import_module(".learn", __package__)  # (the module: the package binds the name `learn` to the function)

@dataclass
class ImputationEM:
    """iterations: imputations and solves, the coin-flip one included; replicas: completions of every row per iteration (all of them
    go into the solve); sampler: the GlauberTermChains of one imputation -- short by default, since every chain starts from the
    row's observed spins and the model changes little between iterations; method: None for those chains, or an Exact -- every
    imputation is then an exact draw by enumeration of each row's missing spins (at most method.max_hidden <= 24 per row) and the
    sampler plays no part."""
    iterations: int = 20
    replicas: int = 2
    sampler: GlauberTermChains = field(default_factory=lambda: GlauberTermChains(burn_in=10, thin=1, samples_per_chain=1))
    method: Exact = None


@dataclass
class EMStep:
    """One iteration: the model learned on its completed data (what learn() returns), the largest change of any solved parameter from
    the previous iteration's rows (iteration 0: from zero), and the solver's iteration count."""
    model: object
    change: float
    solver_iterations: int


@dataclass
class MissingDataResult:
    """model: learn()'s result for the last iterate; trace: one EMStep per iteration."""
    model: object
    trace: list


def _open_hip(values, missing, order, device):
    """the data as the two resident handles of the masked chains (inference._Holes), entered"""
    return inference._Holes(values, missing, order, device).__enter__()


def _impute_hip(holes, model, sampler, replicas, seed, order):
    """a handle of the completed rows under `model`"""
    return holes.chains(model, sampler, replicas, seed, False, order=order)


def _impute_exact_hip(holes, model, replicas, seed, order):
    """a handle of the rows completed by exact draws under `model`"""
    return holes.draws(model, replicas, seed, order=order)


def _solve_hip(prob, formulation, x0, method):
    """the rows of all nodes on the completed handle, started from x0 (None: from zero): (rows, stats)"""
    out, _, st = prob.learn(_learn._form_name(formulation), formulation.regularizer, x0=x0, tol=method.tol, max_iter=method.max_iter,
                            precision=method.precision, max_working=method.max_working, max_add=method.max_add, verbose=method.verbose,
                            hess_samples=method.hess_samples, polish=method.polish)
    return out, st


def _model_of_rows(rows, formulation, n, order, device):
    """learn()'s result assembly: the symmetrised (or not) matrix of a pairwise formulation, the FactorGraph of multiRISE"""
    if isinstance(formulation, multiRISE):
        weights = _learn._assemble_terms_hip(rows, n, order, bool(formulation.symmetrization), device)
        terms = TermArray(n, order, bool(formulation.symmetrization), weights)
        return FactorGraph(order, n, "spin", terms.to_dict() if len(terms) <= _learn.DICT_TERMS_MAX else terms)
    R = np.array(rows)
    return _learn._symmetrize_hip(R, device) if formulation.symmetrization else R


def _largest(model):
    if isinstance(model, FactorGraph):
        t = model.terms
        w = np.asarray(t.weights if hasattr(t, "weights") else list(t.values()), dtype=np.float64)
        return float(np.abs(w).max()) if w.size else 0.0
    return float(np.abs(np.asarray(model)).max())


def learn_missing(samples, formulation=None, method=None, em=None, seed=0):
    """learn() for a K x (1+n) histogram matrix whose spin entries are -1, +1 or 0 = missing (counts: positive integers, a row of count c
    is c samples).  formulation: as learn (default RISE()); pairwise formulations and multiRISE both go through.  method: a HIP (NLP
    and None: HIP()); its solver options apply to every solve; one process, one GPU, all nodes.  em: an ImputationEM.

    Iteration t = 0 .. em.iterations - 1 imputes with seed + t -- under the empty model at t = 0, under the model of iteration t - 1
    after -- then solves on the completed handle from the previous rows and closes it.  The evidence and mask handles stay open
    throughout.  Data without a single hole are handed to learn() as they are: the result is exactly learn(samples, formulation,
    method), after one pass.  Returns a MissingDataResult."""
    formulation = RISE() if formulation is None else formulation
    method_given = HIP() if method is None else method
    em = ImputationEM() if em is None else em
    if not isinstance(formulation, GMLFormulation):
        raise TypeError(f"no method matching learn_missing(::Array, ::{type(formulation).__name__}, ...)")
    if not isinstance(method_given, GMLMethod):
        raise TypeError(f"no method matching learn_missing(..., ::{type(method_given).__name__})")
    method = HIP() if isinstance(method_given, NLP) else method_given
    if method.devices is not None or method.distributed or method.node_range is not None:
        raise ValueError("learn_missing: the completed data are ONE handle over all nodes: one process, one GPU, no devices, distributed or node_range")
    if method.structure is not None or method.refit is not None or method.stderr:
        raise ValueError("learn_missing: structure, refit and stderr are not carried through the iterations")
    if not isinstance(em, ImputationEM):
        raise TypeError(f"em is an ImputationEM, not {type(em).__name__}")
    if int(em.iterations) < 1 or int(em.replicas) < 1:
        raise ValueError(f"ImputationEM: iterations and replicas must be at least 1 (given {em.iterations}, {em.replicas})")
    if em.method is not None and not isinstance(em.method, Exact):
        raise TypeError(f"ImputationEM: method is None (chains) or an Exact, not {type(em.method).__name__}")
    sampler = None if em.method is not None else inference._sampler(em.sampler)
    values, missing = inference._missing_rows(samples)
    if em.method is not None:
        inference._check_holes(missing, em.method.max_hidden)  # (refused before a handle is opened)
    if not missing.any():
        model = _learn.learn(samples, formulation, method_given)
        its = int((method_given.stats if hasattr(method_given, "stats") else {}).get("iterations", 0) or 0)
        return MissingDataResult(model, [EMStep(model, _largest(model), its)])
    n = values.shape[1]
    order = int(formulation.interaction_order) if isinstance(formulation, multiRISE) else 2
    device = 0 if method.device is None else int(method.device)
    # (module attributes, looked up per call: the host tests substitute the steps, as with _local_solve_hip in learn.py)
    open_, impute, impute_exact, solve, assemble = _open_hip, _impute_hip, _impute_exact_hip, _solve_hip, _model_of_rows
    trace, rows, model = [], None, {(1,): 0.0}  # the empty model: every field is 0, every update a coin flip
    holes = open_(values, missing, order, device)
    try:
        for t in range(int(em.iterations)):
            if em.method is not None:
                completed = impute_exact(holes, model, int(em.replicas), int(seed) + t, order)
            else:
                completed = impute(holes, model, sampler, int(em.replicas), int(seed) + t, order)
            try:
                new, st = solve(completed, formulation, rows, method)
            finally:
                if hasattr(completed, "close"):
                    completed.close()
            new = np.asarray(new)
            change = float(np.abs(new - (0.0 if rows is None else rows)).max())
            rows, model = new, assemble(new, formulation, n, order, device)
            trace.append(EMStep(model, change, int((st or {}).get("iterations", 0))))
    finally:
        holes.__exit__(None, None, None)
    return MissingDataResult(model, trace)
