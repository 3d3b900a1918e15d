"""gml_problem_create_mcmc_terms_chains without a GPU: exported, every GML_EINVAL / GML_EUNSUPPORTED case rejected before any device
work, the GlauberTermChains / Problem argument errors.  The numpy restatement of the chain is checked for its invariants."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

import gml_amd as gml
from _mcmc_chains_reference import quantise
from _term_chains_reference import chains as ref_chains, quantise_spins

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")


@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(SO)
    L.gml_problem_create_mcmc_terms_chains.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                                       C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int,
                                                       C.POINTER(C.c_void_p)]
    L.gml_problem_destroy.argtypes = [C.c_void_p]
    L.gml_last_error.restype = C.c_char_p
    return L


KEYS = np.array([[0, 1, -1], [1, 2, 0], [2, -1, -1]], dtype=np.int32)  # (1,2), (2,3,1), (3,) 0-based
WTS = np.array([0.3, -0.2, 0.5])


def _call(L, keys=KEYS, wts=WTS, n=3, chains=8, spc=2, burn_in=3, thin=2, histogram=0, order=3, node0=0, node1=None, stride=None,
          null_keys=False, null_wts=False):
    keys = np.ascontiguousarray(keys, dtype=np.int32)
    wts = np.ascontiguousarray(wts, dtype=np.float64)
    h = C.c_void_p()
    rc = L.gml_problem_create_mcmc_terms_chains(None if null_keys else keys.ctypes.data_as(C.c_void_p),
                                                keys.shape[1] if stride is None else stride,
                                                None if null_wts else wts.ctypes.data_as(C.c_void_p), len(wts), n, chains, spc,
                                                burn_in, thin, 1, histogram, order, node0, n if node1 is None else node1, 0,
                                                C.byref(h))
    msg = L.gml_last_error().decode()
    if h.value:
        L.gml_problem_destroy(h)
    return rc, msg


def test_exported(cdll):
    assert hasattr(cdll, "gml_problem_create_mcmc_terms_chains") and hasattr(cdll, "gml_test_term_chains_tile")


EINVAL = {
    "null_keys": dict(null_keys=True), "null_weights": dict(null_wts=True), "stride0": dict(stride=0),
    "spin_high": dict(keys=[[0, 3, -1], [1, 2, 0], [2, -1, -1]]), "spin_low": dict(keys=[[0, -2, -1], [1, 2, 0], [2, -1, -1]]),
    "nan": dict(wts=[0.3, np.nan, 0.5]), "inf": dict(wts=[0.3, -0.2, -np.inf]),
    "chains": dict(chains=0), "spc": dict(spc=0), "burn_in": dict(burn_in=0), "thin": dict(thin=0),
    "sweeps_overflow": dict(burn_in=2 ** 31 - 1, spc=2, thin=1), "samples_overflow": dict(chains=2 ** 40, spc=2),
    "order0": dict(order=0), "order9": dict(order=9), "node0": dict(node0=-1), "node1": dict(node1=4),
    "empty_range": dict(node0=2, node1=2), "n0": dict(n=0),
}


@pytest.mark.parametrize("case", sorted(EINVAL))
def test_einval_before_device_work(cdll, case):
    rc, msg = _call(cdll, **EINVAL[case])
    assert rc == 1, (case, rc, msg)  # GML_EINVAL, not GML_EHIP: nothing reached the device
    assert "HIP" not in msg


def test_limits_named_before_device_work(cdll):
    rc, msg = _call(cdll, n=16385)
    assert rc == 5 and "n <= 16384" in msg, msg  # GML_EUNSUPPORTED
    rc, msg = _call(cdll, n=65, histogram=1)
    assert rc == 5 and "n <= 64" in msg, msg
    nine = np.arange(9, dtype=np.int32)[None, :]
    rc, msg = _call(cdll, keys=nine, wts=[0.1], n=9)
    assert rc == 5 and "at most 8" in msg, msg
    # a spin named twice cancels: 10 slots, 8 distinct spins after cancellation, is within the limit (zero weights are skipped)
    rc, msg = _call(cdll, keys=np.array([[0, 1, 2, 3, 4, 5, 6, 7, 8, 8]], dtype=np.int32), wts=[0.1], n=9)
    assert rc != 5, msg
    rc, msg = _call(cdll, keys=nine, wts=[0.0], n=9)
    assert rc != 5, msg


def test_incidence_limit_named_before_device_work(cdll):
    K = 1 << 24
    keys = np.zeros((K, 2), dtype=np.int32)
    keys[:, 1] = 1
    rc, msg = _call(cdll, keys=keys, wts=np.full(K, 1e-3), n=2)
    assert rc == 5 and "2^24" in msg, msg


def test_python_layer_errors_and_defaults():
    terms = {(1, 2, 3): 0.5, (1,): 0.1, (2, 3): -0.2}
    with pytest.raises(ValueError, match="multiple of samples_per_chain"):
        gml.sample(terms, 10, sampler=gml.GlauberTermChains(samples_per_chain=4))
    with pytest.raises(ValueError, match="pairwise"):  # GlauberChains keeps refusing multi-body models
        gml.sample(terms, 16, sampler=gml.GlauberChains())
    with pytest.raises(gml.GMLError, match="multiple of mcmc_samples_per_chain"):
        gml.Problem(terms=terms, n=3, num_samples=10, mcmc_sweeps=5, mcmc_samples_per_chain=4)
    with pytest.raises(gml.GMLError, match="mcmc_sweeps"):
        gml.Problem(terms=terms, n=3, num_samples=10, mcmc_thin=2)
    for kw in (dict(model=np.zeros((3, 3))), dict(spins=np.ones((4, 3), dtype=np.int8)), dict(samples=np.ones((4, 4)))):
        with pytest.raises(gml.GMLError, match="terms="):
            gml.Problem(num_samples=10, mcmc_sweeps=5, mcmc_thin=1, **kw)
    with pytest.raises(gml.GMLError, match="model="):  # the keywords of GlauberChains keep their meaning
        gml.Problem(terms={(1, 2): 0.1}, n=2, num_samples=10, burn_in=3)
    s = gml.GlauberTermChains()
    assert (s.burn_in, s.thin, s.samples_per_chain) == (200, 10, 1) and isinstance(s, gml.GMSampler)
    assert {"Glauber", "GlauberChains", "GlauberTermChains"} <= set(gml.__all__)


def _dense(n, seed):
    rng = np.random.default_rng(seed)
    A = np.triu(rng.normal(scale=0.4, size=(n, n)), 1)
    A = A + A.T
    A[np.diag_indices(n)] = rng.normal(scale=0.3, size=n)
    A[0, 1] = A[1, 0] = 0.0  # a zero coupling (skipped term)
    return A


def _pair_terms(A):
    n = A.shape[0]
    terms = [((i + 1, j + 1), A[i, j]) for i in range(n) for j in range(i + 1, n)]
    return terms + [((i + 1,), A[i, i]) for i in range(n)]


def test_pairwise_quantisation_is_the_row_rule():
    A = _dense(9, 1)
    q, sig = quantise(A)
    for i, (a, s, qe) in enumerate(quantise_spins(_pair_terms(A), 9)):
        assert a == A[i, i] and s == sig[i]
        got = np.zeros(9, dtype=np.int64)
        for v, (j,) in qe:
            got[j] = v
        assert np.array_equal(got, q[i])


def test_cancelled_key_is_a_field():
    base = [((1, 2, 3), 0.4), ((2, 4), -0.3), ((3, 4), 0.2), ((1, 4), 0.25)]
    a = ref_chains(base + [((1, 1, 2), 0.7)], 4, 300, 2, 4, 2, seed=5)
    b = ref_chains(base + [((2,), 0.7)], 4, 300, 2, 4, 2, seed=5)
    assert np.array_equal(a, b)
    assert quantise_spins([((1, 1, 2), 0.7)], 2)[1][0] == 0.7


def test_restatement_ignores_the_order_of_coupling_terms():
    rng = np.random.default_rng(3)
    n = 12
    terms = [((int(i), int(j), int(k)), float(rng.normal(scale=0.3)))
             for i, j, k in (rng.choice(n, 3, replace=False) + 1 for _ in range(30))]
    terms += [((int(i), int(j)), float(rng.normal(scale=0.3))) for i, j in (rng.choice(n, 2, replace=False) + 1 for _ in range(20))]
    fields = [((i + 1,), float(rng.normal(scale=0.2))) for i in range(n)]
    a = ref_chains(terms + fields, n, 200, 3, 5, 2, seed=9)
    perm = [terms[t] for t in rng.permutation(len(terms))]
    b = ref_chains(fields[:5] + perm + fields[5:], n, 200, 3, 5, 2, seed=9)
    assert np.array_equal(a, b)


def test_restatement_rows_per_sample():
    terms = {(1, 2, 3): 0.5, (2, 3): -0.3, (1, 4): 0.2, (3,): 0.1}
    a = ref_chains(terms, 4, 50, 3, 4, 3, seed=2)
    assert a.shape == (150, 4)
    for t in range(3):
        assert np.array_equal(a[50 * t:50 * (t + 1)], ref_chains(terms, 4, 50, 1, 4 + 3 * t, 1, seed=2))
