"""gml_problem_create_sampled_elim without a GPU: the symbol and the ABI version, every refusal in its stated order before any device
work, and the Python front door -- sample(model, N, sampler=Elimination()) -- with the device step substituted by the host model of
the draws (tests/_elim_draw_reference.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

import gml_amd as gml
import _elim_draw_reference as D
import _elim_reference as R

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")
EINVAL, EHIP, EUNSUPPORTED = 1, 3, 5


@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(SO)
    p, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    L.gml_problem_create_sampled_elim.argtypes = [p, i32, p, i64, i64, i64, C.c_uint64, p, i32, i32, i64, i64, i32, p]
    L.gml_problem_destroy.argtypes = [p]
    L.gml_problem_destroy.restype = None
    L.gml_last_error.restype = C.c_char_p
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


KEYS = np.array([[0, 1, -1], [1, 2, 0], [2, -1, -1]], dtype=np.int32)
WTS = np.array([0.3, -0.2, 0.5])


def _draw(L, keys=KEYS, wts=WTS, n=3, N=8, order=None, histogram=0, porder=3, node0=0, node1=None, stride=None, nterms=None,
          null_keys=False, null_wts=False, null_out=False):
    keys, wts = np.ascontiguousarray(keys, dtype=np.int32), np.ascontiguousarray(wts, dtype=np.float64)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    h = C.c_void_p()
    rc = L.gml_problem_create_sampled_elim(None if null_keys else _ptr(keys), keys.shape[1] if stride is None else stride,
                                           None if null_wts else _ptr(wts), len(wts) if nterms is None else nterms, n, N, 7, _ptr(order),
                                           histogram, porder, node0, n if node1 is None else node1, 0, None if null_out else C.byref(h))
    msg = L.gml_last_error().decode()
    if h.value:
        L.gml_problem_destroy(h)
    return rc, msg


def _pairs(edges):
    keys = np.array(edges, dtype=np.int32)
    return keys, np.full(len(keys), 0.01)


def _dense(n):
    return _pairs([[a, b] for a in range(n) for b in range(a + 1, n)])


def _chain(n):
    return _pairs([[a, a + 1] for a in range(n - 1)])


def _lattice(r, c):
    return _pairs([[i * c + j, i * c + j + 1] for i in range(r) for j in range(c - 1)] + [[i * c + j, (i + 1) * c + j] for i in range(r - 1) for j in range(c)])


def test_symbol_and_abi_version(cdll):
    assert cdll.gml_abi_version() == 6 and gml._lib.GML_ABI_VERSION == 6  # a function only: no struct or argument list changed
    assert hasattr(cdll, "gml_problem_create_sampled_elim")
    text = open(os.path.join(ROOT, "include", "gml.h")).read()
    assert "#define GML_ABI_VERSION 6" in text and "int gml_problem_create_sampled_elim(" in text


BAD = {
    "null_out": dict(null_out=True), "null_keys": dict(null_keys=True), "null_weights": dict(null_wts=True), "stride0": dict(stride=0),
    "nterms_negative": dict(nterms=-1), "n0": dict(n=0), "spin_high": dict(keys=[[0, 3, -1], [1, 2, 0], [2, -1, -1]]),
    "nan": dict(wts=[0.3, np.nan, 0.5]), "porder0": dict(porder=0), "porder9": dict(porder=9), "node_range": dict(node0=2, node1=2),
    "node1_high": dict(node1=4), "N0": dict(N=0), "N_negative": dict(N=-3), "order_repeats": dict(order=[0, 1, 1]),
    "order_high": dict(order=[0, 1, 3]), "order_negative": dict(order=[0, -1, 2]),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_einval_before_device_work(cdll, case):
    rc, msg = _draw(cdll, **BAD[case])
    assert rc == EINVAL and "HIP" not in msg, (case, rc, msg)
    if case.startswith("order"):
        assert "permutation" in msg
    if case.startswith("N"):
        assert "N must" in msg


def test_refusals_in_their_order(cdll):
    # width 31 ...
    keys, wts = _dense(31)
    rc, msg = _draw(cdll, keys=keys, wts=wts, n=31, porder=2)
    assert rc == EUNSUPPORTED and "width 31" in msg and "limited to 30" in msg and "HIP" not in msg, (rc, msg)
    # ... after every bad argument: N = 0, a non-permutation, the handle's arguments
    assert _draw(cdll, keys=keys, wts=wts, n=31, porder=2, N=0)[0] == EINVAL
    assert _draw(cdll, keys=keys, wts=wts, n=31, porder=2, order=[0] * 31)[0] == EINVAL
    assert _draw(cdll, keys=keys, wts=wts, n=31, porder=0)[0] == EINVAL
    # ... and before everything else that is unsupported: with histogram and 65 spins it is still the width
    keys65 = np.concatenate([keys, [[31 + a, 32 + a] for a in range(33)]]).astype(np.int32)
    rc, msg = _draw(cdll, keys=keys65, wts=np.full(len(keys65), 0.01), n=65, porder=2, histogram=1)
    assert rc == EUNSUPPORTED and "width 31" in msg, (rc, msg)
    # the kept entries: a 24 x 24 lattice has width 25 and keeps about 576 x 2^24 > 2^32 entries
    keys, wts = _lattice(24, 24)
    rc, msg = _draw(cdll, keys=keys, wts=wts, n=576, porder=2)
    assert rc == EUNSUPPORTED and "2^32" in msg and "kept" in msg and "HIP" not in msg, (rc, msg)
    # ... before n > 16384 and the histogram's limits
    rc, msg = _draw(cdll, keys=keys, wts=wts, n=20000, porder=2, histogram=1)
    assert rc == EUNSUPPORTED and "2^32" in msg, (rc, msg)
    # n > 16384, before the histogram's limits
    keys, wts = _chain(16385)
    for hist in (0, 1):
        rc, msg = _draw(cdll, keys=keys, wts=wts, n=16385, porder=2, histogram=hist)
        assert rc == EUNSUPPORTED and "16384" in msg and "HIP" not in msg, (rc, msg)
    # the histogram: n = 65, and N = 2^31
    keys, wts = _chain(65)
    rc, msg = _draw(cdll, keys=keys, wts=wts, n=65, porder=2, histogram=1)
    assert rc == EUNSUPPORTED and "n <= 64" in msg and "HIP" not in msg, (rc, msg)
    rc, msg = _draw(cdll, N=2 ** 31, histogram=1)
    assert rc == EUNSUPPORTED and "2^31" in msg and "HIP" not in msg, (rc, msg)


def test_valid_arguments_reach_the_device_lookup(cdll):
    """past every refusal the device is looked for last: without one GML_EHIP, with one the handle is made"""
    import torch
    keys, wts = _chain(65)
    for kw in (dict(), dict(order=[2, 0, 1]), dict(histogram=1), dict(keys=keys, wts=wts, n=65, porder=2)):
        rc, msg = _draw(cdll, **kw)
        if torch.cuda.is_available():
            assert rc == 0, (rc, msg)
        else:
            assert rc == EHIP and "no HIP device" in msg, (rc, msg)


# ---- the Python front door, the device step substituted ------------------------------------------------------------------------------
class FakeProblem:
    """_lib.Problem(terms=..., elim=True) answered by the host model of the draws"""
    calls = []

    def __init__(self, *, terms, n=None, num_samples, seed, elim, elim_order=None, histogram=False, order=2, device=0):
        assert elim is True
        keys, wts, _, n = gml._lib.term_arrays(terms, n)
        model = {tuple(int(v) + 1 for v in k if v >= 0): float(w) for k, w in zip(keys, wts)}
        FakeProblem.calls.append(dict(n=int(n), N=num_samples, seed=seed, order=elim_order, histogram=histogram, porder=order))
        states = D.draw(model, int(n), num_samples, seed, elim_order)[0]
        self._states, self._counts = np.unique(states, axis=0, return_counts=True) if histogram else (states, np.ones(len(states)))
        self.swap_counts = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def spins(self):
        return self._states

    def counts(self):
        return self._counts.astype(np.float64)


@pytest.fixture()
def substituted(monkeypatch):
    FakeProblem.calls = []
    monkeypatch.setattr(gml._lib, "Problem", FakeProblem)
    return FakeProblem.calls


def _check_histogram(hist, n, N):
    assert hist.shape[1] == n + 1 and hist[:, 0].sum() == N and set(np.unique(hist[:, 1:])) <= {-1, 1}
    assert len(np.unique(hist[:, 1:], axis=0)) == len(hist)
    assert np.array_equal(hist[:, 1:], hist[np.lexsort(hist[:, 1:].T[::-1]), 1:])  # rows in the order np.unique gives them


def test_sample_of_a_dict_a_factor_graph_and_a_matrix(substituted):
    terms, n = R.lattice(3, 3, seed=4)
    hist = gml.sample(terms, 2000, sampler=gml.Elimination(), seed=5)
    _check_histogram(hist, n, 2000)
    assert substituted[-1] == dict(n=n, N=2000, seed=5, order=None, histogram=True, porder=2)
    # a FactorGraph of order 3 keeps its terms; the caller's order is passed on, 1-based
    ladder, n3 = R.triples_ladder(8, seed=1)
    perm = np.random.default_rng(1).permutation(n3) + 1
    fg = gml.FactorGraph(3, n3, terms=ladder)
    _check_histogram(gml.sample(fg, 1000, sampler=gml.Elimination(order=perm)), n3, 1000)
    assert substituted[-1]["porder"] == 3 and substituted[-1]["order"].tolist() == perm.tolist()
    # a pairwise matrix (fields on the diagonal) goes through the term list of its FactorGraph
    A = np.zeros((n, n))
    for k, w in terms.items():
        A[k[0] - 1, k[-1] - 1] = A[k[-1] - 1, k[0] - 1] = w
    hist_m = gml.sample(A, 2000, sampler=gml.Elimination(), seed=5)
    _check_histogram(hist_m, n, 2000)
    assert substituted[-1]["n"] == n and substituted[-1]["histogram"] is True
    # replicates: a list, one seed each
    reps = gml.sample(terms, 500, 3, sampler=gml.Elimination(), seed=5)
    assert len(reps) == 3 and [c["seed"] for c in substituted[-3:]] == [5, 5 + 7919, 5 + 2 * 7919]
    for h in reps:
        _check_histogram(h, n, 500)


def test_more_than_64_spins_come_back_through_unique(substituted):
    terms, n = R.tree(70, seed=2)
    hist = gml.sample(terms, 300, sampler=gml.Elimination())
    _check_histogram(hist, n, 300)
    assert substituted[-1]["histogram"] is False


def test_max_width_refuses_before_the_device_step(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device step was reached")

    monkeypatch.setattr(gml._lib, "Problem", boom)
    terms, n = R.lattice(8, 8)  # (greedy width 9)
    with pytest.raises(ValueError, match="width 9, above max_width = 8"):
        gml.sample(terms, 100, sampler=gml.Elimination(max_width=8))
    perm = np.random.default_rng(0).permutation(n) + 1
    width = gml._lib.model_elim_plan(terms, n, perm)[1]
    assert width > 10
    with pytest.raises(ValueError, match=f"width {width}, above max_width = 10"):
        gml.sample(terms, 100, sampler=gml.Elimination(max_width=10, order=perm))


def test_problem_refuses_elim_with_other_routes():
    with pytest.raises(gml.GMLError, match="elim"):
        gml._lib.Problem(model=np.eye(3), num_samples=10, elim=True)
    with pytest.raises(gml.GMLError, match="elim"):
        gml._lib.Problem(terms={(1, 2): 0.3}, num_samples=10, elim_order=[1, 2])
    with pytest.raises(gml.GMLError, match="mcmc_"):
        gml._lib.Problem(terms={(1, 2): 0.3}, num_samples=10, elim=True, mcmc_sweeps=10)
    with pytest.raises(gml.GMLError, match="each of the 2 spins"):
        gml._lib.Problem(terms={(1, 2): 0.3}, n=2, num_samples=10, elim=True, elim_order=[1, 2, 3])
