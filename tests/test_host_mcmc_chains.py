"""gml_problem_create_mcmc_chains without a GPU: exported, every GML_EINVAL case rejected before any device work, and the
GlauberChains / sample argument errors.  The numpy restatement of the chain is checked against itself for its invariants."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

import gml_amd as gml
from _mcmc_chains_reference import chains as ref_chains, quantise, u01

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")


@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(SO)
    L.gml_problem_create_mcmc_chains.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_uint64, C.c_int,
                                                 C.c_int, C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]
    L.gml_last_error.restype = C.c_char_p
    return L


def _call(L, m, n=None, chains=8, spc=2, burn_in=3, thin=2, histogram=0, order=2, node0=0, node1=None):
    m = np.ascontiguousarray(m, dtype=np.float64)
    n = m.shape[0] if n is None else n
    h = C.c_void_p()
    rc = L.gml_problem_create_mcmc_chains(m.ctypes.data_as(C.c_void_p), n, chains, spc, burn_in, thin, 1, histogram, order, node0,
                                          n if node1 is None else node1, 0, C.byref(h))
    return rc, L.gml_last_error().decode()


def test_exported(cdll):
    assert hasattr(cdll, "gml_problem_create_mcmc_chains")


@pytest.mark.parametrize("case", ["asym", "nan", "inf", "chains", "spc", "burn_in", "thin", "order0", "order9", "node0", "node1",
                                  "empty_range", "n0"])
def test_einval_before_device_work(cdll, case):
    m = np.array([[0.1, 0.3, 0.0], [0.3, 0.0, -0.2], [0.0, -0.2, 0.5]])
    kw = {}
    if case == "asym":
        m[0, 1] = 0.31
    elif case == "nan":
        m[2, 2] = np.nan
    elif case == "inf":
        m[1, 2] = m[2, 1] = np.inf
    elif case in ("chains", "spc", "burn_in", "thin"):
        kw[case] = 0
    elif case == "order0":
        kw["order"] = 0
    elif case == "order9":
        kw["order"] = 9
    elif case == "node0":
        kw["node0"] = -1
    elif case == "node1":
        kw["node1"] = 4
    elif case == "empty_range":
        kw.update(node0=2, node1=2)
    elif case == "n0":
        kw["n"] = 0
    rc, msg = _call(cdll, m, **kw)
    assert rc == 1, (case, rc, msg)  # GML_EINVAL, not GML_EHIP: nothing reached the device
    assert "HIP" not in msg


def test_limits_named_before_device_work(cdll):
    rc, msg = _call(cdll, np.zeros((70, 70)), histogram=1)
    assert rc == 5 and "n <= 64" in msg  # GML_EUNSUPPORTED
    rc, msg = _call(cdll, np.zeros((16385, 16385), dtype=np.float64))
    assert rc == 5 and "n <= 16384" in msg


def test_sampler_errors():
    with pytest.raises(ValueError, match="multiple of samples_per_chain"):
        gml.sample(np.zeros((4, 4)), 10, sampler=gml.GlauberChains(samples_per_chain=4))
    with pytest.raises(ValueError, match="pairwise"):
        gml.sample({(1, 2, 3): 0.5, (1,): 0.1}, 16, sampler=gml.GlauberChains())
    s = gml.GlauberChains()
    assert (s.burn_in, s.thin, s.samples_per_chain) == (200, 10, 1)
    assert "GlauberChains" in gml.__all__ and isinstance(s, gml.GMSampler)


def test_problem_keywords_checked_on_the_host():
    with pytest.raises(gml.GMLError, match="multiple of samples_per_chain"):
        gml.Problem(model=np.zeros((4, 4)), num_samples=10, samples_per_chain=4)
    with pytest.raises(gml.GMLError, match="model="):
        gml.Problem(terms={(1, 2): 0.1}, n=2, num_samples=10, burn_in=3)


def test_reference_hash_and_quantisation():
    # u01 is the samplers' splitmix64 counter hash: a value computed by hand for (seed 0, stream 0, k 0)
    z = (0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) % 2 ** 64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    z ^= z >> 31
    assert u01(0, 0, [0])[0] == (z >> 11) / 2.0 ** 53
    A = np.array([[0.5, 0.75, -0.1], [0.75, 0.0, 1e-3], [-0.1, 1e-3, -2.0]])
    q, sig = quantise(A)
    assert np.all(np.diag(q) == 0) and np.abs(q).max() <= 2 ** 38
    assert np.allclose(q * sig[:, None], A - np.diag(np.diag(A)), rtol=0, atol=np.abs(A).max() * 2.0 ** -38)
    assert sig[0] == 2.0 ** (0 - 38) and sig[1] == 2.0 ** (0 - 38)  # 0.75 < 2^0
    # the restatement: recorded rows for t = 0 .. spc-1; spc = 1 equals the first block of a longer run
    a = ref_chains(A, 5, 3, 2, 2, seed=3)
    b = ref_chains(A, 5, 1, 2, 1, seed=3)
    assert a.shape == (15, 3) and np.array_equal(a[:5], b)
