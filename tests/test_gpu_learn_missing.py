"""learn_missing on the device, through the front door: the case and the bound of _learn_missing_cases.py (the bound comes from the host
loop, not from this code; the device run is not bit-equal to that loop, since solver differences at 1e-9 flip imputed spins), data
without holes, the trace, and the handles it opens."""
import numpy as np
import pytest

import gml_amd as gml
from gml_amd import _lib
import _learn_missing_cases as Cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case():
    terms, truth = Cs.true_terms()
    with gml.Problem(terms=terms, n=Cs.N, num_samples=Cs.DRAWS, seed=0) as p:  # the exact sampler
        spins = p.spins()
    return truth, Cs.with_holes(spins, 0)


def test_em_beats_complete_cases_and_coin_flips(case):
    """device, seed 0: the four errors are printed; the host loop at the same seed gives e_full 0.0330, e_cc 0.1248, e_0 0.4145, e_em 0.0554"""
    import torch
    truth, (holes, full, complete) = case
    method = gml.HIP(tol=1e-9)
    e_full = Cs.error(gml.learn(full, gml.RISE(), method), truth)
    e_cc = Cs.error(gml.learn(complete, gml.RISE(), method), truth)
    gml.learn_missing(holes, gml.RISE(), method, gml.ImputationEM(iterations=2), seed=0)  # (first use: code objects, the allocator)
    torch.cuda.synchronize()
    _lib.trim_cache()
    free0 = torch.cuda.mem_get_info()[0]
    res = gml.learn_missing(holes, gml.RISE(), method, seed=0)
    _lib.trim_cache()
    free1 = torch.cuda.mem_get_info()[0]
    e_0, e_em = Cs.error(res.trace[0].model, truth), Cs.error(res.model, truth)
    print(f"e_full {e_full:.4f}  e_cc {e_cc:.4f}  e_0 {e_0:.4f}  e_em {e_em:.4f}  bound {Cs.BOUND}")
    print("trace:", " ".join(f"{Cs.error(s.model, truth):.3f}" for s in res.trace))
    print("free bytes before / after:", free0, free1)
    assert len(res.trace) == 20 and res.model is res.trace[-1].model
    assert all(s.solver_iterations > 0 and s.change > 0 for s in res.trace)
    assert e_em < e_cc and e_em < e_0
    assert e_em < Cs.BOUND
    assert free1 == free0  # every handle is closed


def test_data_without_holes_is_learn(case):
    _, (_, full, _) = case
    for form in (gml.RISE(0.3, True), gml.logRISE(0.8, False)):
        want = gml.learn(full[:2000], form, gml.HIP(tol=1e-9))
        res = gml.learn_missing(full[:2000], form, gml.HIP(tol=1e-9))
        assert np.array_equal(res.model, want) and len(res.trace) == 1


def test_multirise_goes_through(case):
    _, (holes, _, _) = case
    em = gml.ImputationEM(iterations=3, replicas=1)
    res = gml.learn_missing(holes[:3000], gml.multiRISE(0.4, True, 3), gml.HIP(tol=1e-8), em, seed=1)
    assert len(res.trace) == 3 and isinstance(res.model, gml.FactorGraph) and res.model.order == 3
    assert all(isinstance(s.model, gml.FactorGraph) and np.isfinite(s.change) and s.change > 0 for s in res.trace)
    # the ring's couplings (+-0.6) keep their signs through the order-3 route: imputation noise shrinks a coupling, it does not turn it
    assert all(np.sign(res.model[k]) == np.sign(w) for k, w in Cs.true_terms()[0].items() if len(k) == 2)
