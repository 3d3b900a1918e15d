"""learn_missing with exact imputation on the device, through the front door: ImputationEM(method=Exact()) on the case of
_learn_missing_cases.py at seed 0 -- every iteration completes the data by exact draws of each row's missing entries
(gml_conditional_draw_masked), no chain.

The bound is Cs.BOUND = 0.0722, which _learn_missing_cases.py derives from the host loop of the CHAIN imputation.  The same host loop with
the numpy exact draws (tests/_cond_draw_reference.py) and the CPU oracle's solve (tests/test_host_cond_draw.py: host_errors), the seed
setting the draws, the mask and the imputations alike, the rows in the order the front door runs them in:

    seed   e_full    e_cc     e_0      e_em
    0      0.0330    0.1248   0.4105   0.0528
    1      0.0314    0.1009   0.4097   0.0461
    2      0.0472    0.1026   0.4097   0.0447
    3      0.0336    0.0940   0.4100   0.0455
    4      0.0289    0.1281   0.4208   0.0473

No e_em exceeds 0.0722 (the formula on this table, sqrt(0.0528 x 0.0940) = 0.0705, would be a little tighter; the bound of the case is
kept as it stands).  Neither number comes from the device code.  The device run is not bit-equal to the host loop: solver differences
at 1e-9 move a key across a gap now and then."""
import numpy as np
import pytest

import gml_amd as gml
from gml_amd import _lib
import _learn_missing_cases as Cs

pytestmark = pytest.mark.gpu


def test_exact_em_beats_complete_cases_and_coin_flips():
    """device, seed 0: the four errors are printed; the host loop with exact draws gives e_full 0.0330, e_cc 0.1248, e_0 0.4105, e_em 0.0528"""
    import torch
    terms, truth = Cs.true_terms()
    with gml.Problem(terms=terms, n=Cs.N, num_samples=Cs.DRAWS, seed=0) as p:  # the exact sampler
        spins = p.spins()
    holes, full, complete = Cs.with_holes(spins, 0)
    method = gml.HIP(tol=1e-9)
    e_cc = Cs.error(gml.learn(complete, gml.RISE(), method), truth)
    gml.learn_missing(holes, gml.RISE(), method, gml.ImputationEM(iterations=2, method=gml.Exact()), seed=0)  # (first use: code objects)
    torch.cuda.synchronize()
    _lib.trim_cache()
    free0 = torch.cuda.mem_get_info()[0]
    res = gml.learn_missing(holes, gml.RISE(), method, gml.ImputationEM(method=gml.Exact()), seed=0)
    _lib.trim_cache()
    free1 = torch.cuda.mem_get_info()[0]
    e_0, e_em = Cs.error(res.trace[0].model, truth), Cs.error(res.model, truth)
    print(f"e_cc {e_cc:.4f}  e_0 {e_0:.4f}  e_em {e_em:.4f}  bound {Cs.BOUND}")
    print("trace:", " ".join(f"{Cs.error(s.model, truth):.3f}" for s in res.trace))
    print("free bytes before / after:", free0, free1)
    assert len(res.trace) == 20 and res.model is res.trace[-1].model
    assert all(s.solver_iterations > 0 and s.change > 0 for s in res.trace)
    assert e_em < e_cc and e_em < e_0
    assert e_em < Cs.BOUND
    assert free1 == free0  # every handle is closed
