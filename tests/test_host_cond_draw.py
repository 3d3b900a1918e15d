"""gml_conditional_draw and gml_conditional_draw_masked without a GPU: the numpy restatement of the rule (_cond_draw_reference.py) against
an independent formulation (plain probabilities of every state against the frequencies of many chains), the exports, the argument checks
that precede all device work, the ABI version, the front doors' own refusals, and learn_missing with ImputationEM(method=Exact())
through substituted steps (the exact draws by the numpy restatement, the CPU oracle's solve)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import gml_amd as gml
import _learn_missing_cases as Cs
import test_host_learn_missing as H
from _best_reference import cond_model
from _cond_draw_reference import (codes_of, cond_draw_masked, cond_draw_masked_grouped, cond_draw_rows, draw_of, gumbel, row_energies,
                                  state_probabilities)
from _conditional_reference import random_rows
from _exact_reference import LD
from _mcmc_chains_reference import u01
from _sampler_reference import exact_draws
from oracle import oracle as O

SO = os.path.join(os.path.dirname(os.path.abspath(gml._lib.__file__)), "libgml_hip.so")
missing_module = importlib.import_module("gml_amd.missing")
inference = gml.inference


# ---- the reference against a second formulation ---------------------------------------------------------------------------------------
def plain_probabilities(terms, row, hidden):
    """P(hidden state | visible spins) with nothing shared with the reference: every completed row's energy as the plain float64 sum of
    w prod s over the terms as given, normalised"""
    E = []
    for s in range(1 << len(hidden)):
        x = np.array(row, dtype=np.float64)
        for j, i in enumerate(hidden):
            x[i] = -1.0 if (s >> j) & 1 else 1.0
        E.append(sum(w * np.prod([x[v - 1] for v in key]) for key, w in terms.items()))
    p = np.exp(np.array(E) - max(E))
    return p / p.sum()


def test_draw_frequencies_follow_the_plain_probabilities():
    """20000 chains on one row, 3 hidden spins: chi-square of the reference's draws against probabilities formed without it, below 24.32
    (the 0.999 quantile at 7 degrees of freedom); the softmax of the reference's own energies agrees with them to rounding"""
    n, hidden = 6, [1, 2, 4]
    terms = cond_model(n, seed=9, triples=3)
    row = random_rows(1, n, 4)[0]
    p = plain_probabilities(terms, row, hidden)
    assert float(np.abs(state_probabilities(terms, row, hidden) - p).max()) < 1e-14
    E, log_w = row_energies(terms, row, hidden)
    draws = np.array([draw_of(E, log_w, 3, c)[0] for c in range(20000)])
    counts = np.bincount(draws, minlength=8)
    chi2 = float(((counts - 20000 * p) ** 2 / (20000 * p)).sum())
    print(f"chi-square {chi2:.2f}, smallest expected count {20000 * p.min():.0f}")
    assert 20000 * p.min() > 50 and chi2 < 24.32


def test_the_rule_in_detail():
    n, hidden = 6, [0, 3, 5]
    terms = cond_model(n, seed=9, triples=3)
    rows = random_rows(5, n, 1)
    st, en, lp, gap = cond_draw_rows(terms, n, rows, hidden, 2, 11)
    assert st.shape == (10, 3) and np.all(gap > 0)
    for c in range(10):  # chain r K + k is replica r of row k: stream c, counter s, key = E - log(-log u)
        E, log_w = row_energies(terms, rows[c % 5], hidden)
        u = u01(11, c, np.arange(8, dtype=np.uint64)).astype(LD)
        key = E - np.log(-np.log(u))
        s = int(np.argmax(key))
        assert codes_of(st[c:c + 1])[0] == s and en[c] == E[s] and lp[c] == E[s] - log_w  # the UNPERTURBED energy
        assert np.array_equal(gumbel(11, c, 8), -np.log(-np.log(u)))
    with np.errstate(divide="ignore"):
        assert -np.log(-np.log(LD(0.0))) == -np.inf  # u = 0 can never win
    assert float(-np.log(-np.log(LD(1.0) - LD(2.0) ** -53))) < 36.75  # the largest perturbation


def test_masked_reference_forms_agree():
    terms = cond_model(8, seed=3, triples=3)
    terms[()] = 0.3
    ev = random_rows(60, 8, 2)
    mask = np.random.default_rng(1).random(ev.shape) < 0.4
    mask[::7] = False  # (rows without a hole)
    a = cond_draw_masked(terms, 8, ev, mask, 3, 5)
    assert np.array_equal(a[0], cond_draw_masked_grouped(terms, 8, ev, mask, 3, 5)) and a[3].min() > 1e-9
    none = ~mask.any(axis=1)
    assert none.any() and np.all(a[2][np.tile(none, 3)] == 0) and np.all(np.isinf(a[3][np.tile(none, 3)]))  # no hole: the row, log_p 0
    # a hidden spin in no term is a coin flip: both values occur
    free = {(1, 2): 0.4, (3,): 0.2}
    st = cond_draw_rows(free, 4, np.ones((64, 4), dtype=np.int8), [1, 3], 1, 0)[0]
    assert set(st[:, 1].tolist()) == {-1, 1}


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def test_exports():
    for name in ("conditional_draw", "conditional_draw_masked"):
        assert hasattr(gml._lib, name)
    assert hasattr(missing_module, "_impute_exact_hip") and hasattr(inference._Holes, "draws")
    assert gml.ImputationEM().method is None and isinstance(gml.ImputationEM(method=gml.Exact()).method, gml.Exact)


def test_front_door_refusals_before_a_handle_is_opened(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("an argument error must come before a handle is opened")

    monkeypatch.setattr(gml._lib.Problem, "__init__", boom)
    monkeypatch.setattr(gml._lib, "conditional_draw", boom)
    monkeypatch.setattr(gml._lib, "conditional_draw_masked", boom)
    chain = {(i, i + 1): 0.3 for i in range(1, 7)}
    ev = np.ones((2, 8))
    holes = np.array([[1, 0, 0, 0, 1, 1, 1, 1]])
    with pytest.raises(ValueError, match="no sampler"):
        gml.conditional_sample(chain, ev, [1, 2], gml.GlauberTermChains(), method=gml.Exact())
    with pytest.raises(ValueError, match="no sampler"):
        gml.impute_sample(chain, holes, gml.GlauberTermChains(), method=gml.Exact())
    with pytest.raises(ValueError, match="max_hidden = 2"):
        gml.conditional_sample(chain, ev, [1, 2, 3], method=gml.Exact(max_hidden=2))
    with pytest.raises(ValueError, match="a row lacks 3 spins"):
        gml.impute_sample(chain, holes, method=gml.Exact(max_hidden=2))
    with pytest.raises(ValueError, match="at least 1"):
        gml.conditional_sample(chain, ev, [1, 2], replicas=0, method=gml.Exact())
    with pytest.raises(ValueError, match="at least 1"):
        gml.impute_sample(chain, holes, replicas=0, method=gml.Exact())
    with pytest.raises(ValueError, match="None .chains. or an Exact"):
        gml.conditional_sample(chain, ev, [1, 2], method="exact")
    with pytest.raises(ValueError, match="0 = missing"):
        gml.impute_sample(chain, np.array([[1, 2, 0, 0, 1, 1, 1, 1]]), method=gml.Exact())


def test_method_none_takes_the_chains_as_before(monkeypatch):
    calls = []

    def run(model, evidence, hidden, sampler, replicas, seed, means):
        calls.append((model, evidence, hidden, sampler, replicas, seed, means))
        return ("handle", None, None, None)

    monkeypatch.setattr(inference, "_run", run)
    sampler, model, ev = gml.GlauberTermChains(burn_in=3), {(1, 2): 0.5}, np.ones((2, 3))
    assert gml.conditional_sample(model, ev, [1], sampler, replicas=2, seed=5) == "handle"
    assert gml.conditional_sample(model, ev, [1], sampler, replicas=2, seed=5, method=None) == "handle"
    assert calls == [(model, ev, [1], sampler, 2, 5, False)] * 2

    class Holes:
        K, n, inverse = 1, 2, np.array([0])
        made = []

        def __init__(self, values, missing):
            Holes.made.append(self)

        def __enter__(self):
            return self

        def __exit__(self, *a):
            pass

        def draws(self, *a, **k):
            raise AssertionError("method=None draws nothing exactly")

        def chains(self, model, sampler, replicas, seed, means):
            self.args = (model, sampler, replicas, seed, means)

            class Q:
                order = 2

                def spins(self):
                    return np.ones((2, 2), dtype=np.int8)

                def __enter__(self):
                    return self

                def __exit__(self, *a):
                    pass

            return Q()

    monkeypatch.setattr(inference, "_Holes", Holes)
    monkeypatch.setattr(gml._lib, "Problem", lambda spins, order: ("built", spins.shape, order))
    assert gml.impute_sample(model, np.array([[1, 0, 1]]), sampler, replicas=2, seed=5) == ("built", (2, 2), 2)
    assert Holes.made[-1].args == (model, sampler, 2, 5, False)


# ---- the C entry points ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(SO)
    p = C.c_void_p
    for f in (L.gml_conditional_draw, L.gml_conditional_draw_masked):
        f.argtypes = [p, C.c_int, p, C.c_int64, C.c_int64, p, p, C.c_int, C.c_uint64, p, p, p]
    L.gml_last_error.restype = C.c_char_p
    return L


KEYS = np.array([[0, 1, -1], [1, 2, 0], [2, -1, -1]], dtype=np.int32)  # (1,2), (2,3,1), (3,) 0-based
WTS = np.array([0.3, -0.2, 0.5])


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_exported_and_abi_version(cdll):
    for name in ("gml_conditional_draw", "gml_conditional_draw_masked", "gml_conditional_mode", "gml_conditional_exact"):
        assert hasattr(cdll, name)
    assert cdll.gml_abi_version() == 6  # functions were added: nothing that exists changed


def test_conditional_draw_einval_before_device_work(cdll):
    """the order of gml_conditional_mode with replicas < 1 after "states is NULL": all of it before the evidence handle is looked at"""
    hidden, st = np.array([1, 0, 0], dtype=np.uint8), np.zeros(6, dtype=np.int8)
    for f, second in ((cdll.gml_conditional_draw, _ptr(hidden)), (cdll.gml_conditional_draw_masked, None)):
        for replicas in (1, 0):
            assert f(_ptr(KEYS), 3, _ptr(WTS), 3, 3, None, second, replicas, 7, None, None, None) == 1
            assert "states is NULL" in cdll.gml_last_error().decode()
        for replicas in (0, -2):
            assert f(_ptr(KEYS), 3, _ptr(WTS), 3, 3, None, second, replicas, 7, _ptr(st), None, None) == 1
            msg = cdll.gml_last_error().decode()
            assert "replicas" in msg and "HIP" not in msg, msg
        assert f(_ptr(KEYS), 3, _ptr(WTS), 3, 3, None, second, 2, 7, _ptr(st), None, None) == 1
        assert "evidence is NULL" in cdll.gml_last_error().decode()


# ---- learn_missing with exact draws, through substituted steps ------------------------------------------------------------------------
class ExactSteps(H.HostSteps):
    """the steps of test_host_learn_missing.py with the exact completion in the place of the chains"""

    def impute(self, *a):
        raise AssertionError("ImputationEM(method=Exact()) runs no chain")

    def impute_exact(self, holes, model, replicas, seed, order):
        assert holes is self.holes and not holes.closed
        terms = inference._term_list_args(model, inference._problem_args(model))["terms"]
        states = cond_draw_masked_grouped(terms, holes.values.shape[1], holes.values, holes.missing, replicas, seed)
        self.imputes.append((model, seed, states))
        return states


def run_host(steps, *args, **kw):
    old = missing_module._impute_exact_hip
    missing_module._impute_exact_hip = steps.impute_exact
    try:
        return H.run_host(steps, *args, **kw)
    finally:
        missing_module._impute_exact_hip = old


def host_errors(seed):
    """(e_full, e_cc, e_0, e_em, steps, result) of the host loop with exact draws at one seed"""
    terms, truth = Cs.true_terms()
    spins, _ = exact_draws(terms, Cs.N, Cs.DRAWS, seed)
    holes, full, complete = Cs.with_holes(spins, seed)
    e_full = Cs.error(O.learn_pair(full, "RISE", c=0.4, symmetrize=True)[0], truth)
    e_cc = Cs.error(O.learn_pair(complete, "RISE", c=0.4, symmetrize=True)[0], truth)
    steps = ExactSteps()
    res = run_host(steps, holes, gml.RISE(), gml.HIP(tol=1e-9), gml.ImputationEM(method=gml.Exact()), seed=seed)
    return e_full, e_cc, Cs.error(res.trace[0].model, truth), Cs.error(res.model, truth), steps, res


@pytest.fixture(scope="module")
def run0():
    return host_errors(0)


def test_exact_em_beats_complete_cases_and_coin_flips(run0):
    """host loop with exact draws, seed 0: e_full 0.0330, e_cc 0.1248, e_0 0.4105, e_em 0.0528 (bound 0.0722, tests/test_gpu_learn_missing_exact.py has the table of seeds 0 .. 4)"""
    e_full, e_cc, e_0, e_em, _, _ = run0
    print(f"e_full {e_full:.4f}  e_cc {e_cc:.4f}  e_0 {e_0:.4f}  e_em {e_em:.4f}  bound {Cs.BOUND}")
    assert e_em < e_cc and e_em < e_0
    assert e_em < Cs.BOUND


def test_exact_em_seeds_models_and_observed_entries(run0):
    _, _, _, _, steps, res = run0
    assert len(res.trace) == 20 and len(steps.imputes) == len(steps.solves) == 20 and steps.holes.closed
    assert steps.imputes[0][0] == {(1,): 0.0} and [s for _, s, _ in steps.imputes] == list(range(20))  # seed + t
    assert all(st.shape == (2 * Cs.DRAWS, Cs.N) for _, _, st in steps.imputes)  # two completions of every row
    for t in range(1, 20):
        assert np.array_equal(steps.solves[t][0], steps.solves[t - 1][1])  # started from the previous rows
        assert steps.imputes[t][0] is res.trace[t - 1].model  # completed under the previous model
    values, missing = steps.holes.values, steps.holes.missing
    for _, _, st in steps.imputes[::7]:
        for block in st.reshape(2, Cs.DRAWS, Cs.N):
            assert np.array_equal(block[~missing], values[~missing])
    # iteration 0 completes under the empty model: coin flips
    first = steps.imputes[0][2][:Cs.DRAWS][missing]
    assert abs(float((first == 1).mean()) - 0.5) < 0.01


def test_exact_em_argument_errors_before_a_handle_is_opened():
    good = np.array([[1, 1, 0, 0, 0, -1], [2, -1, 1, 0, 1, 1]])

    class Boom(ExactSteps):
        def open(self, *a):
            raise AssertionError("an argument error must come before a handle is opened")

    with pytest.raises(ValueError, match="a row lacks 3 spins"):
        run_host(Boom(), good, em=gml.ImputationEM(method=gml.Exact(max_hidden=2)))
    with pytest.raises(TypeError, match="an Exact"):
        run_host(Boom(), good, em=gml.ImputationEM(method="exact"))
    # the sampler plays no part with an Exact: one the chains would refuse is not looked at
    steps = ExactSteps()
    res = run_host(steps, good, em=gml.ImputationEM(iterations=2, replicas=1, sampler=gml.Glauber(), method=gml.Exact()))
    assert len(res.trace) == 2 and [s for _, s, _ in steps.imputes] == [0, 1]
