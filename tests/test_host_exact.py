"""gml_model_exact without a GPU.  The brute-force restatement of the contract (_exact_reference.py) is held to closed forms -- independent
spins, the open chain -- and to its own rules (components, cancellation, the empty key); then the C entry point: every GML_EINVAL /
GML_EUNSUPPORTED case rejected before any device work; then the Exact class, the exports and the unchanged error of log_partition."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

import gml_amd as gml
from _exact_reference import ExactModel, LD, chain_corr, chain_log_z, chain_model, components, dense_model, independent_log_z, reduce_key

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")
EPS = 1e-17  # np.longdouble here has a 64-bit mantissa; sums over 2^14 states of probabilities <= 1 stay far below this scale x 2^14


def test_longdouble_is_wider_than_double():
    assert np.finfo(LD).eps < 2e-19  # (the reference is only a yardstick for FP64 where it is)


def test_reference_independent_spins():
    h = np.random.default_rng(1).normal(size=11)
    ref = ExactModel({(i + 1,): float(h[i]) for i in range(11)}, 11)
    assert len(ref.comp) == 11
    assert abs(ref.log_z - independent_log_z(h)) < 1e-16 * 11
    assert np.abs(ref.mean - np.tanh(h.astype(LD))).max() < 1e-17 * 16
    C2 = ref.corr
    assert abs(C2[2, 7] - np.tanh(LD(h[2])) * np.tanh(LD(h[7]))) < 1e-17 * 16 and C2[4, 4] == 1


def test_reference_open_chain():
    terms, J = chain_model(list(range(1, 15)), seed=2)
    ref = ExactModel(terms, 14)
    assert len(ref.comp) == 1
    assert abs(ref.log_z - chain_log_z(J)) < 1e-16 * 14
    assert np.abs(ref.mean).max() < 1e-17 * 2 ** 4
    assert np.abs(ref.corr - chain_corr(J)).max() < 1e-17 * 2 ** 4


def test_reference_rules():
    assert reduce_key((3, 1, 3, 2, 1, 1)) == (1, 2) and reduce_key((4, 4)) == () and reduce_key(()) == ()
    terms = {(1, 2): 0.4, (2, 3, 3): -0.2, (4, 5): 0.0, (5, 6, 5, 7): 0.3, (): 0.25, (8, 8): -0.5, (9,): 0.0}
    assert components(terms, 10) == [[1, 2], [3], [4], [5], [6, 7], [8], [9], [10]]
    ref = ExactModel(terms, 10)
    # spins 1-2: a pair with a field on 2 ((2, 3, 3) reduces to (2,)); 6-7 a pair; 3, 4, 5, 8, 9, 10 free; constants 0.25 - 0.5
    want = (np.log(LD(4)) + np.log(np.cosh(LD(0.4))) + np.log(np.cosh(LD(-0.2)))) + (np.log(LD(4)) + np.log(np.cosh(LD(0.3)))) \
        + 6 * np.log(LD(2)) + LD(0.25) - LD(0.5)
    assert abs(ref.log_z - want) < 1e-17 * 64
    assert abs(ref.expectation((6, 7)) - np.tanh(LD(0.3))) < 1e-18 * 8
    assert ref.expectation(()) == 1 and ref.expectation((3, 3)) == 1 and ref.expectation((3,)) == 0 and ref.expectation((1, 6)) == 0
    # a key across two components is the product of its restrictions
    assert ref.expectation((1, 2, 6, 7, 1)) == ref.expectation((2,)) * ref.expectation((6, 7))


def test_reference_agrees_with_itself_across_a_split():
    # two components held as one model and as two
    a, b = dense_model([1, 2, 3, 4, 5], 3), dense_model([6, 7, 8], 4)
    whole, ra, rb = ExactModel({**a, **b}, 8), ExactModel(a, 5), ExactModel({tuple(v - 5 for v in k): w for k, w in b.items()}, 3)
    assert abs(whole.log_z - (ra.log_z + rb.log_z)) < 1e-17 * 16
    assert abs(whole.expectation((2, 4, 7)) - ra.expectation((2, 4)) * rb.expectation((2,))) < 1e-18 * 8


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def test_exact_class_and_exports():
    assert gml.Exact().max_spins == 40 and gml.Exact(24).max_spins == 24 and gml.Exact(max_spins=1).max_spins == 1
    for bad in (0, 41, -3):
        with pytest.raises(ValueError, match="max_spins"):
            gml.Exact(bad)
    assert {"Exact", "exact_moments", "AIS", "log_partition", "log_likelihood"} <= set(gml.__all__)
    assert gml.exact_moments is gml.likelihood.exact_moments and gml.Exact is gml.likelihood.Exact
    assert hasattr(gml._lib, "model_exact")


def test_max_spins_refuses_before_the_library_is_called():
    chain, _ = chain_model(list(range(1, 8)), seed=5)
    with pytest.raises(ValueError, match="max_spins = 6"):
        gml.log_partition(chain, gml.Exact(6))
    with pytest.raises(ValueError, match="max_spins = 3"):
        gml.exact_moments(chain, method=gml.Exact(3))


def test_another_method_is_still_refused_with_the_text_that_names_ais():
    with pytest.raises(ValueError, match="AIS"):
        gml.log_partition({(1, 2): 0.3}, gml.Glauber())
    with pytest.raises(ValueError, match="takes an AIS method, given int"):
        gml.log_partition({(1, 2): 0.3}, 7)


# ---- the C entry point ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(SO)
    L.gml_model_exact.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gml_last_error.restype = C.c_char_p
    return L


KEYS = np.array([[0, 1, -1], [1, 2, 0], [2, -1, -1]], dtype=np.int32)  # (1,2), (2,3,1), (3,) 0-based
WTS = np.array([0.3, -0.2, 0.5])
QKEYS = np.array([[0, 2], [1, 1], [-1, -1]], dtype=np.int32)


def _call(L, keys=KEYS, wts=WTS, n=3, qkeys=QKEYS, stride=None, nterms=None, qstride=None, nq=None, null_keys=False, null_wts=False,
          null_logz=False, null_qkeys=False, null_qexp=False, outputs=True):
    keys = np.ascontiguousarray(keys, dtype=np.int32)
    wts = np.ascontiguousarray(wts, dtype=np.float64)
    qkeys = np.ascontiguousarray(qkeys, dtype=np.int32)
    nn = max(n, 1)
    logz, mean, corr, qexp = np.zeros(1), np.zeros(nn), np.zeros((nn, nn)), np.zeros(max(len(qkeys), 1))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = L.gml_model_exact(None if null_keys else ptr(keys), keys.shape[1] if stride is None else stride, None if null_wts else ptr(wts),
                           len(wts) if nterms is None else nterms, n, None if null_qkeys else ptr(qkeys),
                           qkeys.shape[1] if qstride is None else qstride, len(qkeys) if nq is None else nq, 0,
                           None if null_logz else ptr(logz), ptr(mean) if outputs else None, ptr(corr) if outputs else None,
                           None if null_qexp else ptr(qexp))
    return rc, L.gml_last_error().decode()


def test_exported(cdll):
    assert hasattr(cdll, "gml_model_exact") and hasattr(cdll, "gml_test_exact_chunk_bits")


EINVAL = {
    "null_log_z": dict(null_logz=True), "null_keys": dict(null_keys=True), "null_weights": dict(null_wts=True),
    "stride0": dict(stride=0), "stride_negative": dict(stride=-2), "nterms_negative": dict(nterms=-1),
    "spin_high": dict(keys=[[0, 3, -1], [1, 2, 0], [2, -1, -1]]), "spin_low": dict(keys=[[0, -2, -1], [1, 2, 0], [2, -1, -1]]),
    "nan": dict(wts=[0.3, np.nan, 0.5]), "inf": dict(wts=[0.3, -0.2, -np.inf]), "n0": dict(n=0), "n_negative": dict(n=-4),
    "nq_negative": dict(nq=-1), "null_qkeys": dict(null_qkeys=True), "null_qexp": dict(null_qexp=True), "qstride0": dict(qstride=0),
    "query_spin_high": dict(qkeys=[[0, 3]]), "query_spin_low": dict(qkeys=[[-2, 1]]),
}


@pytest.mark.parametrize("case", sorted(EINVAL))
def test_einval_before_device_work(cdll, case):
    rc, msg = _call(cdll, **EINVAL[case])
    assert rc == 1, (case, rc, msg)  # GML_EINVAL, not GML_EHIP: nothing reached the device
    assert "HIP" not in msg


def _chain_keys(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)], axis=1).astype(np.int32)


def test_component_limit_named_before_device_work(cdll):
    rc, msg = _call(cdll, keys=_chain_keys(41), wts=np.full(40, 0.1), n=41)
    assert rc == 5 and "41 spins" in msg and "limited to 40" in msg and "HIP" not in msg, msg  # GML_EUNSUPPORTED
    # the limit is per component: the same chain cut by a zero weight in the middle (a zero weight joins nothing) is not refused
    w = np.full(40, 0.1)
    w[20] = 0.0
    rc, msg = _call(cdll, keys=_chain_keys(41), wts=w, n=41, nq=0, null_qkeys=True, null_qexp=True, outputs=False)
    assert rc in (0, 3) and (rc == 0 or "no HIP device" in msg), (rc, msg)


def test_chunk_bits_hook_range(cdll):
    assert cdll.gml_test_exact_chunk_bits(13) == -1 and cdll.gml_test_exact_chunk_bits(-1) == -1
    assert cdll.gml_test_exact_chunk_bits(4) == 0 and cdll.gml_test_exact_chunk_bits(0) == 4 and cdll.gml_test_exact_chunk_bits(0) == 0


@pytest.mark.parametrize("kw", [dict(), dict(outputs=False), dict(nq=0, null_qkeys=True, null_qexp=True),
                                dict(keys=np.zeros((0, 2), dtype=np.int32), wts=[], null_keys=True, null_wts=True)],
                         ids=["plain", "optional_outputs_null", "no_queries", "no_terms"])
def test_valid_arguments_reach_the_device_lookup(cdll, kw):
    rc, msg = _call(cdll, **kw)
    assert rc in (0, 3), (rc, msg)  # GML_OK on a GPU, else GML_EHIP: the device is looked for last
    if rc == 3:
        assert "no HIP device" in msg
