"""learn_missing without a GPU: the device steps (the two handles, the masked chains, the solve, the symmetrisation) are substituted by the
numpy restatement of the masked chains (_masked_reference.py, vectorised over chains) and the CPU oracle's solve; gml.learn_missing
itself runs.  What is checked: the estimator on the case of _learn_missing_cases.py (it beats complete-case learning and coin-flip
imputation, and the bound written there), the trace, the seeds and warm starts handed on, data without holes, the argument errors."""
import importlib

import numpy as np
import pytest

import gml_amd as gml
import _learn_missing_cases as Cs
from _masked_reference import masked
from _sampler_reference import exact_draws
from oracle import oracle as O

missing_module = importlib.import_module("gml_amd.missing")
learn_module = importlib.import_module("gml_amd.learn")
inference = gml.inference


class HostHoles:
    def __init__(self, values, missing):
        self.values, self.missing, self.closed = values, missing, False

    def __exit__(self, *a):
        self.closed = True


class HostSteps:
    """the substituted steps, recording what learn_missing hands them"""

    def __init__(self):
        self.imputes, self.solves, self.holes = [], [], None

    def open(self, values, missing, order, device):
        assert self.holes is None  # opened once, kept across the iterations
        perm = inference._mask_order(missing)  # (the order the device runs the rows in: the same chains, draw for draw)
        self.holes = HostHoles(values[perm], missing[perm])
        return self.holes

    def impute(self, holes, model, sampler, replicas, seed, order):
        assert holes is self.holes and not holes.closed
        terms = inference._term_list_args(model, inference._problem_args(model))["terms"]
        n = holes.values.shape[1]
        states, _ = masked(terms, n, holes.values, holes.missing, replicas, sampler.samples_per_chain, sampler.burn_in, sampler.thin, seed)
        self.imputes.append((model, seed, states))
        return states

    def solve(self, completed, formulation, x0, method):
        x, _, st = O.learn_pair_fast(None, completed, type(formulation).__name__, c=formulation.regularizer, tol=method.tol)
        self.solves.append((None if x0 is None else np.array(x0), x))
        return x, st


def oracle_local_solve(samples, formulation, method, order, node_range, device, **kw):
    assert not {k: v for k, v in kw.items() if v is not None}
    Rm, kkt, _ = O.learn_pair(samples, type(formulation).__name__, c=formulation.regularizer, symmetrize=False)
    return Rm[node_range[0]:node_range[1]], kkt[node_range[0]:node_range[1]], {"iterations": 7}


def run_host(steps, *args, **kw):
    old = (missing_module._open_hip, missing_module._impute_hip, missing_module._solve_hip, learn_module._local_solve_hip,
           learn_module._symmetrize_hip)
    missing_module._open_hip, missing_module._impute_hip, missing_module._solve_hip = steps.open, steps.impute, steps.solve
    learn_module._local_solve_hip = oracle_local_solve
    learn_module._symmetrize_hip = lambda Rm, device: 0.5 * (Rm + Rm.T)
    try:
        return gml.learn_missing(*args, **kw)
    finally:
        (missing_module._open_hip, missing_module._impute_hip, missing_module._solve_hip, learn_module._local_solve_hip,
         learn_module._symmetrize_hip) = old


def host_errors(seed):
    """(e_full, e_cc, e_0, e_em, steps, result) of the host loop at one seed"""
    terms, truth = Cs.true_terms()
    spins, _ = exact_draws(terms, Cs.N, Cs.DRAWS, seed)
    holes, full, complete = Cs.with_holes(spins, seed)
    e_full = Cs.error(O.learn_pair(full, "RISE", c=0.4, symmetrize=True)[0], truth)
    e_cc = Cs.error(O.learn_pair(complete, "RISE", c=0.4, symmetrize=True)[0], truth)
    steps = HostSteps()
    res = run_host(steps, holes, gml.RISE(), gml.HIP(tol=1e-9), seed=seed)
    return e_full, e_cc, Cs.error(res.trace[0].model, truth), Cs.error(res.model, truth), steps, res


@pytest.fixture(scope="module")
def run0():
    return host_errors(0)


def test_em_beats_complete_cases_and_coin_flips(run0):
    """host loop, seed 0: e_full 0.0330, e_cc 0.1248, e_0 0.4145, e_em 0.0554 (bound 0.0722)"""
    e_full, e_cc, e_0, e_em, _, _ = run0
    print(f"e_full {e_full:.4f}  e_cc {e_cc:.4f}  e_0 {e_0:.4f}  e_em {e_em:.4f}  bound {Cs.BOUND}")
    assert e_em < e_cc and e_em < e_0
    assert e_em < Cs.BOUND


def test_trace_seeds_and_warm_starts(run0):
    _, _, _, _, steps, res = run0
    assert len(res.trace) == 20 and len(steps.imputes) == len(steps.solves) == 20 and steps.holes.closed
    assert steps.imputes[0][0] == {(1,): 0.0} and [s for _, s, _ in steps.imputes] == list(range(20))  # seed + t
    assert all(st.shape == (2 * Cs.DRAWS, Cs.N) for _, _, st in steps.imputes)  # two completions of every row
    assert steps.solves[0][0] is None
    for t in range(1, 20):
        assert np.array_equal(steps.solves[t][0], steps.solves[t - 1][1])  # started from the previous rows
        assert steps.imputes[t][0] is res.trace[t - 1].model  # imputed under the previous model
        assert res.trace[t].change == np.abs(steps.solves[t][1] - steps.solves[t - 1][1]).max()
    assert res.trace[0].change == np.abs(steps.solves[0][1]).max()
    assert res.model is res.trace[-1].model and np.array_equal(res.model, 0.5 * (steps.solves[-1][1] + steps.solves[-1][1].T))
    assert all(s.solver_iterations > 0 for s in res.trace)
    # every completion keeps the observed entries
    values, missing = steps.holes.values, steps.holes.missing
    for _, _, st in steps.imputes[::7]:
        for block in st.reshape(2, Cs.DRAWS, Cs.N):
            assert np.array_equal(block[~missing], values[~missing])


def test_data_without_holes_is_learn(run0):
    terms, _ = Cs.true_terms()
    spins, _ = exact_draws(terms, Cs.N, 500, 3)
    _, full, _ = Cs.with_holes(spins, 3)

    class Boom(HostSteps):
        def open(self, *a):
            raise AssertionError("data without holes must not reach the chains")

    method = gml.HIP(tol=1e-9)
    res = run_host(Boom(), full, gml.RISE(0.3, True), method)
    rows = O.learn_pair(full, "RISE", c=0.3, symmetrize=False)[0]
    want = 0.5 * (rows + rows.T)
    assert np.array_equal(res.model, want) and len(res.trace) == 1 and res.trace[0].model is res.model
    assert res.trace[0].solver_iterations == 7 and res.trace[0].change == np.abs(want).max()


def test_argument_errors_before_the_library_loads():
    good = np.array([[1, 1, 0, -1], [2, -1, 1, 0]])

    class Boom(HostSteps):
        def open(self, *a):
            raise AssertionError("an argument error must come before a handle is opened")

    for kw, exc, what in ((dict(formulation=3), TypeError, "no method matching"), (dict(method=3), TypeError, "no method matching"),
                          (dict(em=3), TypeError, "ImputationEM"), (dict(em=gml.ImputationEM(iterations=0)), ValueError, "at least 1"),
                          (dict(em=gml.ImputationEM(replicas=0)), ValueError, "at least 1"),
                          (dict(em=gml.ImputationEM(sampler=gml.Glauber())), ValueError, "GlauberTermChains"),
                          (dict(method=gml.HIP(devices=[0, 1])), ValueError, "one process"),
                          (dict(method=gml.HIP(node_range=(0, 1))), ValueError, "one process"),
                          (dict(method=gml.HIP(refit=0.1)), ValueError, "not carried")):
        with pytest.raises(exc, match=what):
            run_host(Boom(), good, **kw)
    for bad, what in ((np.array([[1, 1, 2, -1]]), "0 = missing"), (np.array([[0.5, 1, 0, -1]]), "positive integers")):
        with pytest.raises(ValueError, match=what):
            run_host(Boom(), bad)
    em = gml.ImputationEM()
    assert (em.iterations, em.replicas, em.sampler.burn_in, em.sampler.thin, em.sampler.samples_per_chain) == (20, 2, 10, 1, 1)
