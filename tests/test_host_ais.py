"""gml_log_partition_ais without a GPU.  The numpy restatement of the contract (_ais_reference.py) is held to what it must be: with one
step it is the plain term chain, its tracked energy is the energy of its final state, an all-zero model gives n log 2 exactly, and on
three models small enough to enumerate the estimate lies within five of its own standard errors of the exact log Z -- with a
standard error small enough for that to mean something, and a one-step control that misses.  Then the AIS class, and the C entry
point: every GML_EINVAL / GML_EUNSUPPORTED case rejected before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

import gml_amd as gml
from _ais_reference import ais, energies, exact_log_z, lattice, sparse_model, summary
from _tempered_reference import bimodal_16
from _term_chains_reference import chains as ref_chains

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")


MODELS = {
    "bimodal_16": lambda: (bimodal_16(), 16),
    "lattice_4x4": lambda: (lattice(4, 0.4, 0.2, 1), 16),
    "sparse_n18": lambda: (sparse_model(18, 6, 3, 0.3, 2), 18),
}
_cache = {}


def estimate(name):
    """(log_z, stderr, ess, exact) of 4096 chains, 300 linear steps, one sweep per step, seed 1: computed once per model"""
    if name not in _cache:
        terms, n = MODELS[name]()
        logw, _, _ = ais(terms, n, 4096, np.linspace(0.0, 1.0, 301), 1, seed=1)
        _cache[name] = summary(logw, n) + (exact_log_z(terms, n),)
    return _cache[name]


def test_one_step_is_the_plain_chain():
    terms = sparse_model(12, 6, 3, 0.3, 3)
    for k in (1, 4):
        _, _, states = ais(terms, 12, 200, [0.0, 1.0], k, seed=9)
        assert np.array_equal(states, ref_chains(terms, 12, 200, 1, k, 1, seed=9))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_tracked_energy_is_the_energy_of_the_final_state(name):
    terms, n = MODELS[name]()
    betas = [0.0, 0.2, 0.1, 0.5, 0.5, 1.0]
    logw, E, states = ais(terms, n, 300, betas, 3, seed=4)
    drift = np.abs(E - energies(terms, states)).max()
    print(f"{name}: largest |tracked E - E(final state)| = {drift:.2e}")  # (from the 2^-38 quantisation: at most 7e-10 here)
    assert drift < 1e-8
    # the start energy on its own state (one sweep at beta = 0 follows it); a schedule of zeros weighs nothing
    logw0, E0, s0 = ais(terms, n, 300, [0.0, 0.0], 1, seed=4)
    assert np.all(logw0 == 0.0) and np.abs(E0 - energies(terms, s0)).max() < 1e-8


def test_all_zero_model():
    terms = {(1, 2): 0.0, (2, 3, 4): 0.0, (5,): 0.0}
    logw, E, _ = ais(terms, 5, 64, np.linspace(0.0, 1.0, 11), 1, seed=2)
    log_z, se, ess = summary(logw, 5)
    assert np.all(logw == 0.0) and np.all(E == 0.0)
    assert log_z == 5 * np.log(2.0) and se == 0.0 and ess == 64.0
    assert summary(np.array([-3.25]), 7) == (7 * np.log(2.0) + -3.25 + 0.0, 0.0, 1.0)  # one chain: no standard error


@pytest.mark.parametrize("name", sorted(MODELS))
def test_accuracy_against_enumeration(name):
    log_z, se, ess, exact = estimate(name)
    print(f"{name}: log Z = {log_z:.6f}, exact {exact:.6f}, error {log_z - exact:+.4f}, stderr {se:.4f}, ess {ess:.0f}")
    assert abs(log_z - exact) < 5 * se


@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_accuracy_bound_means_something(name):
    assert estimate(name)[1] < 0.02


def test_naive_control_one_step_misses():
    terms, n = MODELS["bimodal_16"]()
    logw, _, _ = ais(terms, n, 4096, [0.0, 1.0], 1, seed=1)
    log_z, se, ess = summary(logw, n)
    exact = estimate("bimodal_16")[3]
    print(f"one step: log Z = {log_z:.4f}, exact {exact:.4f}, ess {ess:.2f}")
    assert abs(log_z - exact) > 1.0


def test_ais_class():
    m = gml.AIS()
    assert (m.chains, m.steps, m.sweeps_per_step) == (4096, 1000, 1)
    assert np.array_equal(m.betas, np.linspace(0.0, 1.0, 1001)) and m.betas[0] == 0.0 and m.betas[-1] == 1.0
    m = gml.AIS(4096, 300)
    assert (m.chains, m.steps) == (4096, 300) and len(m.betas) == 301
    m = gml.AIS(chains=10, sweeps_per_step=2, betas=(0, 0.5, 0.25, 0.7))
    assert (m.chains, m.steps, m.sweeps_per_step) == (10, 3, 2) and m.betas.tolist() == [0.0, 0.5, 0.25, 0.7]
    for bad in ([0.1, 1.0], [0.0], [], [0.0, np.nan], [0.0, -0.5, 1.0], [0.0, np.inf]):
        with pytest.raises(ValueError, match="betas"):
            gml.AIS(betas=bad)
    for kw in (dict(chains=0), dict(sweeps_per_step=0), dict(steps=0)):
        with pytest.raises(ValueError):
            gml.AIS(**kw)
    with pytest.raises(ValueError, match="AIS"):
        gml.log_partition({(1, 2): 0.3}, gml.Glauber())
    assert {"AIS", "log_partition", "log_likelihood"} <= set(gml.__all__)


# ---- the C entry point ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(SO)
    L.gml_log_partition_ais.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int,
                                        C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gml_last_error.restype = C.c_char_p
    return L


KEYS = np.array([[0, 1, -1], [1, 2, 0], [2, -1, -1]], dtype=np.int32)  # (1,2), (2,3,1), (3,) 0-based
WTS = np.array([0.3, -0.2, 0.5])


def _call(L, keys=KEYS, wts=WTS, n=3, chains=8, betas=(0.0, 0.5, 1.0), nbetas=None, sps=1, stride=None, nterms=None, null_keys=False,
          null_wts=False, null_betas=False, null_logw=False, outputs=True):
    keys = np.ascontiguousarray(keys, dtype=np.int32)
    wts = np.ascontiguousarray(wts, dtype=np.float64)
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    room = min(max(chains, 1), 64)  # (a rejected call writes nothing)
    logw, en, sp, res = np.zeros(room), np.zeros(room), np.zeros((room, max(n, 1)), dtype=np.int8), np.zeros(3)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = L.gml_log_partition_ais(None if null_keys else ptr(keys), keys.shape[1] if stride is None else stride,
                                 None if null_wts else ptr(wts), len(wts) if nterms is None else nterms, n, chains,
                                 None if null_betas else ptr(betas), len(betas) if nbetas is None else nbetas, sps, 1, 0,
                                 None if null_logw else ptr(logw), ptr(en) if outputs else None, ptr(sp) if outputs else None,
                                 ptr(res) if outputs else None)
    return rc, L.gml_last_error().decode()


def test_exported(cdll):
    assert hasattr(cdll, "gml_log_partition_ais")


EINVAL = {
    "null_keys": dict(null_keys=True), "null_weights": dict(null_wts=True), "null_betas": dict(null_betas=True),
    "null_log_weights": dict(null_logw=True),
    # what check_term_pointers / check_term_values reject
    "stride0": dict(stride=0), "nterms_negative": dict(nterms=-1), "spin_high": dict(keys=[[0, 3, -1], [1, 2, 0], [2, -1, -1]]),
    "spin_low": dict(keys=[[0, -2, -1], [1, 2, 0], [2, -1, -1]]), "nan": dict(wts=[0.3, np.nan, 0.5]), "inf": dict(wts=[0.3, -0.2, -np.inf]),
    "n0": dict(n=0),
    "chains0": dict(chains=0), "chains_negative": dict(chains=-5), "chains_above_2_31": dict(chains=2 ** 31 + 1),
    "nbetas1": dict(betas=(0.0,)), "nbetas0": dict(nbetas=0), "beta0_positive": dict(betas=(0.1, 1.0)),
    "beta_negative": dict(betas=(0.0, -0.1, 1.0)), "beta_nan": dict(betas=(0.0, np.nan)), "beta_inf": dict(betas=(0.0, np.inf)),
    "sps0": dict(sps=0), "sps_negative": dict(sps=-1), "sweeps_overflow": dict(betas=np.linspace(0.0, 1.0, 3), sps=2 ** 30),
}


@pytest.mark.parametrize("case", sorted(EINVAL))
def test_einval_before_device_work(cdll, case):
    rc, msg = _call(cdll, **EINVAL[case])
    assert rc == 1, (case, rc, msg)  # GML_EINVAL, not GML_EHIP: nothing reached the device
    assert "HIP" not in msg


def test_limits_named_before_device_work(cdll):
    rc, msg = _call(cdll, n=16385)
    assert rc == 5 and "n <= 16384" in msg and "HIP" not in msg, msg  # GML_EUNSUPPORTED
    nine = np.arange(9, dtype=np.int32)[None, :]
    rc, msg = _call(cdll, keys=nine, wts=[0.1], n=9)
    assert rc == 5 and "at most 8" in msg and "HIP" not in msg, msg


def test_incidence_limit_named_before_device_work(cdll):
    K = 1 << 24
    keys = np.zeros((K, 2), dtype=np.int32)
    keys[:, 1] = 1
    rc, msg = _call(cdll, keys=keys, wts=np.full(K, 1e-3), n=2)
    assert rc == 5 and "2^24" in msg and "HIP" not in msg, msg


@pytest.mark.parametrize("kw", [dict(), dict(outputs=False), dict(betas=(0.0, 0.7, 0.3, 0.3, 2.0), sps=3), dict(betas=(0.0, 0.0))],
                         ids=["plain", "optional_outputs_null", "non_monotone", "zeros"])
def test_valid_arguments_reach_the_device_lookup(cdll, kw):
    rc, msg = _call(cdll, **kw)
    assert rc in (0, 3), (rc, msg)  # GML_OK on a GPU, else GML_EHIP: the device is looked for last
    if rc == 3:
        assert "no HIP device" in msg
