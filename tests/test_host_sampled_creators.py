"""gml_problem_create_sampled_terms, _mcmc_terms and _sampled_hist without a GPU: every GML_EINVAL / GML_EUNSUPPORTED case is
rejected before the device lookup, so a bad argument never reads as a missing GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")
GML_OK, GML_EINVAL, GML_EHIP, GML_EUNSUPPORTED = 0, 1, 3, 5

_HEAD = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_uint64]  # keys, stride, weights, nterms, n, N, seed
_TAIL = [C.c_int, C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]  # order, node0, node1, device, out


@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(SO)
    L.gml_problem_create_sampled_terms.argtypes = _HEAD + _TAIL
    L.gml_problem_create_mcmc_terms.argtypes = _HEAD + [C.c_int] + _TAIL  # + sweeps
    L.gml_problem_create_sampled_hist.argtypes = _HEAD + [C.c_int] + _TAIL  # + mcmc_sweeps (0: the exact sampler)
    L.gml_problem_destroy.argtypes = [C.c_void_p]
    L.gml_last_error.restype = C.c_char_p
    return L


KEYS = np.array([[0, 1, -1], [1, 2, 0], [2, -1, -1]], dtype=np.int32)  # (1,2), (2,3,1), (3,) 0-based
WTS = np.array([0.3, -0.2, 0.5])

# entry point -> (symbol, the sweeps argument it takes or None)
ENTRIES = {
    "sampled_terms": ("gml_problem_create_sampled_terms", None),
    "mcmc_terms": ("gml_problem_create_mcmc_terms", 5),
    "hist_exact": ("gml_problem_create_sampled_hist", 0),
    "hist_mcmc": ("gml_problem_create_sampled_hist", 5),
}


def _call(L, entry, keys=KEYS, wts=WTS, n=3, N=16, order=3, node0=0, node1=None, stride=None, null_keys=False, null_wts=False,
          sweeps=None):
    symbol, default_sweeps = ENTRIES[entry]
    keys = np.ascontiguousarray(keys, dtype=np.int32)
    wts = np.ascontiguousarray(wts, dtype=np.float64)
    h = C.c_void_p()
    args = [None if null_keys else keys.ctypes.data_as(C.c_void_p), keys.shape[1] if stride is None else stride,
            None if null_wts else wts.ctypes.data_as(C.c_void_p), len(wts), n, N, 1]
    if default_sweeps is not None:
        args.append(default_sweeps if sweeps is None else sweeps)
    rc = getattr(L, symbol)(*args, order, node0, n if node1 is None else node1, 0, C.byref(h))
    msg = L.gml_last_error().decode()
    if h.value:
        L.gml_problem_destroy(h)
    return rc, msg


EINVAL = {
    "null_keys": dict(null_keys=True), "null_weights": dict(null_wts=True), "stride0": dict(stride=0),
    "spin_high": dict(keys=[[0, 3, -1], [1, 2, 0], [2, -1, -1]]), "spin_low": dict(keys=[[0, -2, -1], [1, 2, 0], [2, -1, -1]]),
    "nan": dict(wts=[0.3, np.nan, 0.5]), "inf": dict(wts=[0.3, -0.2, -np.inf]),
    "order0": dict(order=0), "order9": dict(order=9), "node0": dict(node0=-1), "node1": dict(node1=4),
    "empty_range": dict(node0=2, node1=2), "n0": dict(n=0), "N0": dict(N=0),
}


@pytest.mark.parametrize("case", sorted(EINVAL))
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_einval_before_device_work(cdll, entry, case):
    rc, msg = _call(cdll, entry, **EINVAL[case])
    assert rc == GML_EINVAL, (entry, case, rc, msg)  # not GML_EHIP: nothing reached the device
    assert "HIP" not in msg


def test_sweeps_must_be_positive(cdll):
    rc, msg = _call(cdll, "mcmc_terms", sweeps=0)  # (in _sampled_hist, 0 sweeps select the exact sampler)
    assert rc == GML_EINVAL and "HIP" not in msg, (rc, msg)
    rc, msg = _call(cdll, "mcmc_terms", sweeps=-1)
    assert rc == GML_EINVAL and "HIP" not in msg, (rc, msg)


@pytest.mark.parametrize("entry", ["hist_exact", "hist_mcmc"])
def test_histogram_limit_named_before_device_work(cdll, entry):
    rc, msg = _call(cdll, entry, n=65)
    assert rc == GML_EUNSUPPORTED and "n <= 64" in msg and "HIP" not in msg, (rc, msg)


@pytest.mark.parametrize("entry", ["sampled_terms", "hist_exact"])
def test_component_limit_named_before_device_work(cdll, entry):
    chain = np.array([[i, i + 1] for i in range(22)], dtype=np.int32)  # 23 spins in one connected component
    rc, msg = _call(cdll, entry, keys=chain, wts=np.full(22, 0.1), n=23, order=2)
    assert rc == GML_EUNSUPPORTED and "23 spins" in msg and "22" in msg and "HIP" not in msg, (rc, msg)
    # 22 spins are within the limit, and zero-weight terms do not connect: only the device lookup can refuse these
    rc, msg = _call(cdll, entry, keys=chain[:21], wts=np.full(21, 0.1), n=22, order=2, N=4)
    assert rc in (GML_OK, GML_EHIP), (rc, msg)
    wts = np.full(22, 0.1)
    wts[11] = 0.0
    rc, msg = _call(cdll, entry, keys=chain, wts=wts, n=23, order=2, N=4)
    assert rc in (GML_OK, GML_EHIP), (rc, msg)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_valid_arguments_reach_the_device_lookup(cdll, entry):
    rc, msg = _call(cdll, entry)
    assert rc in (GML_OK, GML_EHIP), (entry, rc, msg)
    if rc == GML_EHIP:
        assert "no HIP device" in msg
    rc, msg = _call(cdll, entry, keys=np.zeros((0, 2), dtype=np.int32), wts=np.zeros(0), null_keys=True, null_wts=True)
    assert rc in (GML_OK, GML_EHIP), (entry, rc, msg)  # an empty term list may come with NULL pointers
