"""gml_model_best_states and gml_conditional_mode without a GPU.  The brute-force restatement (_best_reference.py) is held to itself
-- components with the merge against the whole model -- and to a closed form; the conditions the device tests rest on (every gap among
the reference's best k + 1 energies above 1e-9) are checked on the reference alone; the Python surface and every refusal of the C entry
points that precedes device work are checked here too."""
import ctypes as C
import os

import numpy as np
import pytest

import gml_amd as gml
from conftest import ROOT
from _best_reference import (MODELS, best_states, best_states_whole, chain_best_energies, cond_mode, reference, smallest_gap, spins_of,
                             code_of)
from _exact_reference import LD, chain_model, dense_model

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")
GAP = 1e-9


# ---- the reference against itself ---------------------------------------------------------------------------------------------------
def several_components(case):
    """(terms, n <= 16) of 2 to 4 components, spins in no term among them"""
    if case == 0:  # two components and two free spins (3 and 12)
        terms = dense_model([1, 5, 9, 11], seed=1, extra=2)
        terms.update(dense_model([2, 4, 6, 7, 8, 10], seed=2, extra=3))
        return terms, 12
    if case == 1:  # three components, the empty key, a cancelled spin, a zero weight that joins nothing; free: 16
        terms = dense_model(range(1, 8), seed=3, extra=4)
        terms.update(dense_model([8, 10, 12, 14], seed=4, extra=1))
        terms.update(chain_model([9, 11, 13, 15], seed=5)[0])
        terms.update({(): 0.4, (2, 2, 3): 0.3, (7, 8): 0.0})
        return terms, 16
    terms = {(1,): 0.3, (2, 3): -0.45, (4, 5): 0.2, (4,): -0.1, (6, 7): 0.35, (7,): 0.05}  # four components, free: 8
    return terms, 8


@pytest.mark.parametrize("case", [0, 1, 2])
@pytest.mark.parametrize("k", [1, 7, 64, 256, 300])
def test_components_with_merge_equal_the_whole_model(case, k):
    terms, n = several_components(case)
    a, b = best_states(terms, n, k), best_states_whole(terms, n, k)
    assert len(a) == len(b) == min(k, 1 << n)
    assert [s for _, s in a] == [s for _, s in b]  # (a free spin ties exactly: +1, the lower number, first)
    assert max(abs(ea - eb) for (ea, _), (eb, _) in zip(a, b)) < 1e-17


def test_more_states_asked_for_than_there_are():
    terms = {(1, 2): 0.3, (3,): -0.2}
    got = best_states(terms, 3, 256)
    assert len(got) == 8 and sorted(s for _, s in got) == list(range(8))
    assert [s for _, s in got[:2]] == [0b100, 0b111]  # spin 3 down, spins 1 and 2 aligned: (+, +) before (-, -)


def test_open_chain_closed_form():
    terms, J = chain_model(list(range(1, 17)), seed=16)
    got = best_states_whole(terms, 16, 64)
    want = chain_best_energies(J, 64)
    assert max(abs(e - w) for (e, _), w in zip(got, want)) < 1e-16 * 16
    for a in range(0, 64, 2):  # the pair s, -s: the same energy, s (spin 16 up) first
        assert got[a][0] == got[a + 1][0] and got[a][1] < got[a + 1][1] and got[a][1] ^ got[a + 1][1] == (1 << 16) - 1


def test_codes_and_spins_round_trip():
    codes = [0, 1, 0b1010, (1 << 50) - 1, 1 << 49]
    assert code_of(spins_of(codes, 50)) == codes and spins_of([0b10], 3).tolist() == [[1, -1, 1]]


# ---- the conditions of the device tests, on the reference alone ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(set(MODELS) - {"components"}))
def test_gaps_of_the_device_tests_models(name):
    _, n, best = reference(name)
    assert len(best) == min(257, 1 << n) and smallest_gap(best) > GAP, smallest_gap(best)


def test_components_model_ties_are_exact():
    # 13 spins in no term: the best 257 are the best state of the others under the 257 lowest settings of the free spins
    _, n, best = reference("components")
    assert n == 50 and len(best) == 257 and all(e == best[0][0] for e, _ in best)
    assert [s for _, s in best] == sorted(s for _, s in best)


def test_chain_gaps_between_pairs():
    _, J = chain_model(list(range(1, 25)), seed=24)
    e = chain_best_energies(J, 66)
    assert np.all(e[0:64:2] == e[1:64:2]) and float(np.min(e[1:65:2] - e[2:66:2])) > GAP


def test_conditional_mode_of_one_row():
    # two hidden spins tied to a visible one and to each other: the mode follows the stronger bond; a hidden spin in no term is +1
    terms = {(1, 2): 1.0, (2, 3): 0.5, (1, 4): -0.25}
    st, e, lp, gap = cond_mode(terms, 5, np.array([-1, 1, 1, 1, 1]), [1, 2, 4])
    assert st.tolist() == [-1, -1, 1] and abs(e - LD(1.75)) < 1e-18 and gap == 0.0 and lp < 0  # (the free spin ties; +1 wins)


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def test_exports():
    assert {"most_probable_states", "conditional_mode", "impute_mode"} <= set(gml.__all__)
    assert gml.most_probable_states is gml.likelihood.most_probable_states
    assert gml.conditional_mode is gml.inference.conditional_mode and gml.impute_mode is gml.inference.impute_mode
    for name in ("model_best_states", "conditional_mode", "conditional_mode_masked"):
        assert hasattr(gml._lib, name)


def test_python_refusals_before_the_library_is_called():
    chain, _ = chain_model(list(range(1, 8)), seed=5)
    with pytest.raises(ValueError, match="max_spins = 6"):
        gml.most_probable_states(chain, method=gml.Exact(6))
    with pytest.raises(ValueError, match="max_hidden = 2"):
        gml.conditional_mode(chain, np.ones((1, 8)), [1, 2, 3], method=gml.Exact(max_hidden=2))
    with pytest.raises(ValueError, match="a row lacks 3 spins"):
        gml.impute_mode(chain, np.array([[1, 0, 0, 0, 1, 1, 1, 1]]), method=gml.Exact(max_hidden=2))
    with pytest.raises(ValueError, match="0 = missing"):
        gml.impute_mode(chain, np.array([[1, 2, 0, 0, 1, 1, 1, 1]]))


# ---- the C entry points ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(SO)
    p = C.c_void_p
    L.gml_model_best_states.argtypes = [p, C.c_int, p, C.c_int64, C.c_int64, C.c_int64, C.c_int, p, p, p]
    for f in (L.gml_conditional_mode, L.gml_conditional_mode_masked):
        f.argtypes = [p, C.c_int, p, C.c_int64, C.c_int64, p, p, p, p, p]
    L.gml_last_error.restype = C.c_char_p
    return L


KEYS = np.array([[0, 1, -1], [1, 2, 0], [2, -1, -1]], dtype=np.int32)  # (1,2), (2,3,1), (3,) 0-based
WTS = np.array([0.3, -0.2, 0.5])


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _best(L, keys=KEYS, wts=WTS, n=3, k=1, stride=None, nterms=None, null=()):
    keys = np.ascontiguousarray(keys, dtype=np.int32)
    wts = np.ascontiguousarray(wts, dtype=np.float64)
    found, states, energies = np.zeros(1, dtype=np.int64), np.zeros((256, max(n, 1)), dtype=np.int8), np.zeros(256)
    arg = lambda name, a: None if name in null else _ptr(a)  # noqa: E731
    rc = L.gml_model_best_states(arg("keys", keys), keys.shape[1] if stride is None else stride, arg("weights", wts),
                                 len(wts) if nterms is None else nterms, n, k, 0, arg("found", found), arg("states", states),
                                 arg("energies", energies))
    return rc, L.gml_last_error().decode()


def _chain_keys(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)], axis=1).astype(np.int32)


def test_exported(cdll):
    for name in ("gml_model_best_states", "gml_conditional_mode", "gml_conditional_mode_masked"):
        assert hasattr(cdll, name)


EINVAL = {
    "null_keys": dict(null=("keys",)), "null_weights": dict(null=("weights",)), "stride0": dict(stride=0), "nterms_negative": dict(nterms=-1),
    "n0": dict(n=0), "spin_high": dict(keys=[[0, 3, -1], [1, 2, 0], [2, -1, -1]]), "spin_low": dict(keys=[[0, -2, -1], [1, 2, 0], [2, -1, -1]]),
    "nan": dict(wts=[0.3, np.nan, 0.5]), "k0": dict(k=0), "k_negative": dict(k=-3), "null_found": dict(null=("found",)),
    "null_states": dict(null=("states",)), "null_energies": dict(null=("energies",)),
}


@pytest.mark.parametrize("case", sorted(EINVAL))
def test_best_states_einval_before_device_work(cdll, case):
    rc, msg = _best(cdll, **EINVAL[case])
    assert rc == 1, (case, rc, msg)  # GML_EINVAL, not GML_EHIP: nothing reached the device
    assert "HIP" not in msg


def test_best_states_refusals_in_the_stated_order(cdll):
    chain41 = dict(keys=_chain_keys(41), wts=np.full(40, 0.1), n=41)
    # the term list's values come before k; k < 1 before the outputs; both before the limits; k's limit before the component's
    rc, msg = _best(cdll, wts=[0.3, np.inf, 0.5], k=0)
    assert rc == 1 and "finite" in msg, msg
    rc, msg = _best(cdll, k=0, null=("found",))
    assert rc == 1 and "k must be at least 1" in msg, msg
    rc, msg = _best(cdll, k=0, **chain41)
    assert rc == 1 and "k must be at least 1" in msg, msg
    rc, msg = _best(cdll, k=257, null=("states",))
    assert rc == 1 and "NULL" in msg, msg
    rc, msg = _best(cdll, k=257)
    assert rc == 5 and "257" in msg and "256" in msg and "HIP" not in msg, msg  # GML_EUNSUPPORTED, the limit named
    rc, msg = _best(cdll, k=257, **chain41)
    assert rc == 5 and "256" in msg, msg
    rc, msg = _best(cdll, k=256, **chain41)
    assert rc == 5 and "41 spins" in msg and "limited to 40" in msg and "HIP" not in msg, msg
    # the limit is per component: the same chain cut by a zero weight is not refused, and k = 256 is not
    w = np.full(40, 0.1)
    w[20] = 0.0
    rc, msg = _best(cdll, keys=_chain_keys(41), wts=w, n=41, k=256)
    assert rc in (0, 3) and (rc == 0 or "no HIP device" in msg), (rc, msg)


def test_conditional_mode_einval_before_device_work(cdll):
    hidden, st = np.array([1, 0, 0], dtype=np.uint8), np.zeros(3, dtype=np.int8)
    for f, second in ((cdll.gml_conditional_mode, _ptr(hidden)), (cdll.gml_conditional_mode_masked, None)):
        # states NULL takes the place of "all three outputs NULL", before the evidence is looked at
        assert f(_ptr(KEYS), 3, _ptr(WTS), 3, 3, None, second, None, None, None) == 1
        assert "states is NULL" in cdll.gml_last_error().decode()
        assert f(_ptr(KEYS), 3, _ptr(WTS), 3, 3, None, second, _ptr(st), None, None) == 1
        assert "evidence is NULL" in cdll.gml_last_error().decode()
