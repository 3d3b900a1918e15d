"""The per-row masked conditional chains without a GPU.  The numpy restatement of the rule (_masked_reference.py) is held to what it
must be: with one mask shared by every row it is the fixed-mask restatement, observed columns never move, one hidden spin per row gives
tanh of its field, and on a model small enough to enumerate the sampled configurations and the Rao-Blackwellised means agree with the
exact conditional distribution of every row's own hidden set.  Then the C entry points' checks that need no device, the header, and
the Python front door's refusals, count expansion and row order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import gml_amd as gml
from _ais_reference import sparse_model
from _conditional_reference import closed_form_bound, conditional, exact_field, random_rows
from _masked_reference import ENUM, check_enumeration, enum_model, mask_rows, masked, random_mask

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")


def model33():
    return sparse_model(33, 6, 4, 0.3, 4), 33


def test_shared_mask_is_the_fixed_mask_chain():
    terms, n = model33()
    ev = random_rows(70, n, 0)
    hid = [0, 5, 31, 32]
    mask = np.zeros((70, n), dtype=bool)
    mask[:, hid] = True
    states, means = masked(terms, n, ev, mask, 2, 3, 5, 2, seed=11)
    ref_states, ref_means = conditional(terms, n, ev, hid, 2, 3, 5, 2, seed=11)
    assert np.array_equal(states, ref_states)
    assert np.array_equal(means[:, hid], ref_means)
    vis = [i for i in range(n) if i not in hid]
    assert np.array_equal(means[:, vis], np.tile(ev[:, vis].astype(np.float64), (2, 1)))


def test_observed_entries_equal_the_evidence():
    terms, n = model33()
    ev = random_rows(70, n, 0)
    mask = random_mask(70, n, 0.3, 1)
    mask[3], mask[4] = False, True  # a row without a hole, a row that is all holes
    states, means = masked(terms, n, ev, mask, 2, 3, 5, 2, seed=11)
    assert states.shape == (70 * 2 * 3, n) and means.shape == (140, n)
    for block in states.reshape(3 * 2, 70, n):  # (t, r): every recorded row of every replica
        assert np.array_equal(block[~mask], ev[~mask])
        assert np.array_equal(block[3], ev[3])  # a row with no hidden spin comes back as it is
    assert any(not np.array_equal(block[mask], ev[mask]) for block in states.reshape(6, 70, n))
    both = np.tile(mask, (2, 1))
    assert np.array_equal(means[~both], np.tile(ev, (2, 1))[~both].astype(np.float64))
    assert np.abs(means[both]).max() < 1.0
    # the hidden entries of the evidence play no part
    other = np.where(mask, -ev, ev)
    s2, m2 = masked(terms, n, other, mask, 2, 3, 5, 2, seed=11)
    assert np.array_equal(states, s2) and np.array_equal(means, m2)


def test_one_hidden_spin_per_row_is_tanh_of_its_field():
    terms, n = model33()
    K = 70
    ev = random_rows(K, n, 0)
    which = np.arange(K) * 7 % n  # a different spin in neighbouring rows; 0, 32 and the word boundary among them
    mask = np.zeros((K, n), dtype=bool)
    mask[np.arange(K), which] = True
    want = np.tanh([exact_field(terms, n, ev[k], int(which[k])) for k in range(K)])
    bound = np.array([closed_form_bound(terms, n, int(i)) for i in which])
    for spc, burn_in, thin in ((1, 1, 1), (3, 5, 2), (4, 2, 7)):
        _, means = masked(terms, n, ev, mask, 1, spc, burn_in, thin, seed=11)
        err = np.abs(means[np.arange(K), which] - want)
        print(f"spc {spc}: max |mean - tanh h| = {err.max():.2e}, bounds from {bound.min():.2e}")
        assert np.all(err <= bound)


def test_enumeration():
    """at seed 3 the worst cell z-score is 3.27, the worst mean z-score 2.09; the bound is 6"""
    terms, ev, mask = enum_model()
    assert mask.sum(axis=1).min() >= 2 and mask.sum(axis=1).max() <= 5 and len({tuple(r) for r in mask}) == ENUM["K"]
    states, means = masked(terms, ENUM["n"], ev, mask, ENUM["replicas"], 1, ENUM["burn_in"], 1, seed=ENUM["seed"])
    zc, zm = check_enumeration(terms, ev, mask, states, means)
    print(f"worst cell z-score {zc:.2f}, worst mean z-score {zm:.2f}")


# ---- the C entry points ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(SO)
    p, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.gml_problem_create_mcmc_terms_masked.argtypes = [p, i32, p, i64, i64, p, p, i32, i64, i32, i32, C.c_uint64, i32, i64, i64, C.POINTER(p)]
    L.gml_conditional_means_masked.argtypes = [p, i32, p, i64, i64, p, p, i32, i64, i32, i32, C.c_uint64, p]
    L.gml_test_problem_stub.argtypes = [i64, i64, i32, i64, i64, C.POINTER(p)]
    L.gml_problem_destroy.argtypes = [p]
    L.gml_problem_destroy.restype = None
    L.gml_last_error.restype = C.c_char_p
    return L


KEYS = np.array([[0, 1, -1], [1, 2, 0], [2, -1, -1]], dtype=np.int32)
WTS = np.array([0.3, -0.2, 0.5])


def make_stub(cdll, n):
    """a handle of n spins that holds sizes only: enough for the checks that come before any device work"""
    h = C.c_void_p()
    assert cdll.gml_test_problem_stub(n, n, 2, 0, n, C.byref(h)) == 0
    return h


@pytest.fixture()
def stubs(cdll):
    hs = [make_stub(cdll, 3), make_stub(cdll, 3), make_stub(cdll, 4)]
    yield hs
    for h in hs:
        cdll.gml_problem_destroy(h)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def creator(cdll, evidence, mask, out, n=3):
    return cdll.gml_problem_create_mcmc_terms_masked(ptr(KEYS), 3, ptr(WTS), 3, n, evidence, mask, 1, 1, 5, 1, 0, 2, 0, n, out)


def the_means(cdll, evidence, mask, means, n=3):
    return cdll.gml_conditional_means_masked(ptr(KEYS), 3, ptr(WTS), 3, n, evidence, mask, 1, 1, 5, 1, 0, means)


@pytest.mark.parametrize("case", ["evidence", "mask", "out"])
def test_null_arguments_of_the_creator(cdll, stubs, case):
    out = C.c_void_p()
    rc = creator(cdll, None if case == "evidence" else stubs[0], None if case == "mask" else stubs[1], None if case == "out" else C.byref(out))
    msg = cdll.gml_last_error().decode()
    assert rc == 1 and "HIP" not in msg and "NULL" in msg, (rc, msg)  # GML_EINVAL
    assert not out.value


@pytest.mark.parametrize("case", ["evidence", "mask", "means"])
def test_null_arguments_of_the_means(cdll, stubs, case):
    means = np.zeros(8)
    rc = the_means(cdll, None if case == "evidence" else stubs[0], None if case == "mask" else stubs[1], None if case == "means" else ptr(means))
    msg = cdll.gml_last_error().decode()
    assert rc == 1 and "HIP" not in msg and "NULL" in msg, (rc, msg)
    assert np.all(means == 0.0)


def test_mismatched_handles(cdll, stubs):
    out, means = C.c_void_p(), np.zeros(16)
    for rc in (creator(cdll, stubs[0], stubs[2], C.byref(out)), the_means(cdll, stubs[0], stubs[2], ptr(means))):
        msg = cdll.gml_last_error().decode()
        assert rc == 1 and "mask handle" in msg and "differs" in msg, (rc, msg)
    # n against the evidence comes first, as in the fixed-mask entry points
    assert creator(cdll, stubs[2], stubs[0], C.byref(out), n=3) == 1 and "evidence handle's 4 spins" in cdll.gml_last_error().decode()
    # matching stubs get past both checks: the next one (no rows: no chains) answers
    assert creator(cdll, stubs[0], stubs[1], C.byref(out)) == 1 and "at least 1" in cdll.gml_last_error().decode()
    assert not out.value and np.all(means == 0.0)


def test_header_and_bindings():
    text = open(os.path.join(ROOT, "include", "gml.h")).read()
    assert "#define GML_ABI_VERSION 6" in text and gml._lib.GML_ABI_VERSION == 6  # functions only
    for name in ("gml_problem_create_mcmc_terms_masked", "gml_conditional_means_masked"):
        assert re.search(r"\bint " + name + r"\(", text), name
    assert gml.inference.impute is gml.impute and hasattr(gml._lib, "conditional_chains_masked")
    assert {"impute", "impute_sample", "Imputation", "learn_missing", "ImputationEM"} <= set(gml.__all__)


# ---- the front door ----------------------------------------------------------------------------------------------------------
def test_front_door_refusals_before_a_handle_is_opened():
    model = {(1, 2): 0.3, (3,): 0.1}
    good = np.array([[2, 1, 0, 1], [1, -1, -1, 0]])
    for f in (gml.impute, gml.impute_sample):
        for bad, what in ((np.array([[1, 1, 2, 1]]), "-1, \\+1 or 0"), (np.array([[1.0, 1, 0.5, 1]]), "-1, \\+1 or 0"),
                          (np.array([[1.0, 1, np.nan, 1]]), "-1, \\+1 or 0"), (np.array([[0, 1, 0, 1]]), "positive integers"),
                          (np.array([[1.5, 1, 0, 1]]), "positive integers"), (np.array([[-1, 1, 0, 1]]), "positive integers"),
                          (np.array([1, 1, 0, 1]), "histogram matrix")):
            with pytest.raises(ValueError, match=what):
                f(model, bad)
        with pytest.raises(ValueError, match="GlauberTermChains"):
            f(model, good, gml.Glauber())
        with pytest.raises(ValueError, match="replicas"):
            f(model, good, replicas=0)


def test_count_expansion_and_row_order():
    from gml_amd.inference import _missing_rows
    hist = np.array([[2, 1, 0, -1], [1, -1, -1, 1], [3, 0, 0, 0]])
    values, missing = _missing_rows(hist)
    assert values.dtype == np.int8 and missing.dtype == bool
    assert np.array_equal(missing, np.array([[0, 1, 0], [0, 1, 0], [0, 0, 0], [1, 1, 1], [1, 1, 1], [1, 1, 1]], dtype=bool))
    assert np.array_equal(values, np.array([[1, 1, -1], [1, 1, -1], [-1, -1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1]]))
    v2, m2 = _missing_rows(hist.astype(np.float64))
    assert np.array_equal(values, v2) and np.array_equal(missing, m2)
    assert np.array_equal(mask_rows(missing)[0], [1, -1, 1])
    # the order the rows run in on the device: stable, by packed mask with spin 0 the most significant bit
    from gml_amd.inference import _Holes, _mask_order
    m = np.array([[0, 1, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0], [1, 1, 1], [0, 0, 0], [0, 0, 1]], dtype=bool)
    assert _mask_order(m).tolist() == [2, 5, 6, 0, 3, 1, 4]
    wide = np.zeros((3, 70), dtype=bool)
    wide[0, 69] = wide[1, 8] = wide[2, 7] = True  # (beyond one byte and one word: spin 7 before spin 8 before spin 69)
    assert _mask_order(wide).tolist() == [0, 1, 2]
    h = _Holes(np.arange(21, dtype=np.int8).reshape(7, 3), m)
    assert np.array_equal(h.missing, m[h.perm]) and np.array_equal(h.values[h.inverse], np.arange(21).reshape(7, 3))
