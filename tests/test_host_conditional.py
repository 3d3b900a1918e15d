"""The conditional chains without a GPU.  The numpy restatement of the rule (_conditional_reference.py, always the full walk) is held
to what it must be: with every spin hidden it is the plain term chain, visible columns never move, one hidden spin gives tanh of its
field whatever the chain's length, and on a model small enough to enumerate both the sampled configurations and the Rao-Blackwellised
means agree with the exact conditional distribution.  Then the C entry points' checks that need no device, the header, and the
Python front door's handling of `hidden`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import gml_amd as gml
from _ais_reference import sparse_model
from _conditional_reference import ENUM, check_enumeration, closed_form_bound, conditional, enum_model, exact_field, random_rows
from _term_chains_reference import chains as ref_chains

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")


def model33():
    return sparse_model(33, 6, 4, 0.3, 4), 33


def test_all_hidden_is_the_term_chain():
    terms, n = model33()
    states, means = conditional(terms, n, random_rows(70, n, 0), range(n), 1, 3, 5, 2, seed=11)
    assert np.array_equal(states, ref_chains(terms, n, 70, 3, 5, 2, seed=11))
    assert means.shape == (70, n) and np.abs(means).max() < 1.0


def test_visible_columns_equal_the_evidence():
    terms, n = model33()
    ev = random_rows(70, n, 0)
    hid = [0, 5, 31, 32]
    states, means = conditional(terms, n, ev, hid, 2, 3, 5, 2, seed=11)
    vis = [i for i in range(n) if i not in hid]
    assert states.shape == (70 * 2 * 3, n) and means.shape == (140, 4)
    for block in states.reshape(3 * 2, 70, n):  # (t, r): every recorded row of every replica
        assert np.array_equal(block[:, vis], ev[:, vis])
    assert any(not np.array_equal(block[:, hid], ev[:, hid]) for block in states.reshape(6, 70, n))


@pytest.mark.parametrize("i", [0, 17, 32])
def test_one_hidden_spin_is_tanh_of_its_field(i):
    terms, n = model33()
    ev = random_rows(70, n, 0)
    want = np.tanh([exact_field(terms, n, row, i) for row in ev])
    bound = closed_form_bound(terms, n, i)
    for spc, burn_in, thin in ((1, 1, 1), (3, 5, 2), (4, 2, 7)):
        _, means = conditional(terms, n, ev, [i], 1, spc, burn_in, thin, seed=11)
        err = np.abs(means[:, 0] - want).max()
        print(f"spin {i}, spc {spc}: max |mean - tanh h| = {err:.2e}, bound {bound:.2e}")
        assert err <= bound


def test_enumeration():
    terms, ev = enum_model()
    states, means = conditional(terms, ENUM["n"], ev, ENUM["hidden"], ENUM["replicas"], 1, ENUM["burn_in"], 1, seed=ENUM["seed"])
    zc, zm = check_enumeration(terms, ev, states, means)
    print(f"worst cell z-score {zc:.2f}, worst mean z-score {zm:.2f}")


# ---- the C entry points ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(SO)
    p, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.gml_problem_create_mcmc_terms_conditional.argtypes = [p, i32, p, i64, i64, p, p, i32, i64, i32, i32, C.c_uint64, i32, i64, i64, C.POINTER(p)]
    L.gml_conditional_means.argtypes = [p, i32, p, i64, i64, p, p, i32, i64, i32, i32, C.c_uint64, p]
    L.gml_test_problem_stub.argtypes = [i64, i64, i32, i64, i64, C.POINTER(p)]
    L.gml_problem_destroy.argtypes = [p]
    L.gml_problem_destroy.restype = None
    L.gml_last_error.restype = C.c_char_p
    return L


KEYS = np.array([[0, 1, -1], [1, 2, 0], [2, -1, -1]], dtype=np.int32)
WTS = np.array([0.3, -0.2, 0.5])


@pytest.fixture()
def stub(cdll):
    """a handle of 3 spins that holds sizes only: enough for the checks that come before any device work"""
    h = C.c_void_p()
    assert cdll.gml_test_problem_stub(3, 3, 2, 0, 3, C.byref(h)) == 0
    yield h
    cdll.gml_problem_destroy(h)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("case", ["evidence", "hidden", "out"])
def test_null_arguments_of_the_creator(cdll, stub, case):
    mask = np.array([1, 0, 0], dtype=np.uint8)
    out = C.c_void_p()
    rc = cdll.gml_problem_create_mcmc_terms_conditional(ptr(KEYS), 3, ptr(WTS), 3, 3, None if case == "evidence" else stub,
                                                        None if case == "hidden" else ptr(mask), 1, 1, 5, 1, 0, 2, 0, 3,
                                                        None if case == "out" else C.byref(out))
    msg = cdll.gml_last_error().decode()
    assert rc == 1 and "HIP" not in msg and "NULL" in msg, (rc, msg)  # GML_EINVAL
    assert not out.value


@pytest.mark.parametrize("case", ["evidence", "hidden", "means"])
def test_null_arguments_of_the_means(cdll, stub, case):
    mask = np.array([1, 0, 0], dtype=np.uint8)
    means = np.zeros(8)
    rc = cdll.gml_conditional_means(ptr(KEYS), 3, ptr(WTS), 3, 3, None if case == "evidence" else stub,
                                    None if case == "hidden" else ptr(mask), 1, 1, 5, 1, 0, None if case == "means" else ptr(means))
    msg = cdll.gml_last_error().decode()
    assert rc == 1 and "HIP" not in msg and "NULL" in msg, (rc, msg)
    assert np.all(means == 0.0)


def test_header_and_bindings():
    text = open(os.path.join(ROOT, "include", "gml.h")).read()
    assert "#define GML_ABI_VERSION 6" in text and gml._lib.GML_ABI_VERSION == 6  # functions only
    for name in ("gml_problem_create_mcmc_terms_conditional", "gml_conditional_means"):
        assert re.search(r"\bint " + name + r"\(", text), name
    assert gml.inference.conditional_means is gml.conditional_means
    assert {"conditional_sample", "conditional_means", "predictive_check"} <= set(gml.__all__)
    assert hasattr(gml._lib, "conditional_chains")
    julia = open(os.path.join(ROOT, "graphicalmodellearning.jl_amd", "julia", "GraphicalModelLearningHIP.jl")).read()
    assert ":gml_conditional_means" in julia


def test_hidden_is_one_based_and_checked():
    from gml_amd.inference import _hidden_spins
    assert _hidden_spins([3, 1, 10], 10) == [1, 3, 10]  # 1-based, like FactorGraph keys; n itself is a spin, 0 is not
    model = {(1, 2): 0.3, (3,): 0.1}
    hist = np.array([[2, 1, -1, 1], [1, -1, -1, 1]])
    for bad, what in (([], "no spin"), ([0], "numbered from 1"), ([4], "numbered from 1"), ([2, 2], "twice")):
        with pytest.raises(ValueError, match=what):
            _hidden_spins(bad, 3)
        for f in (gml.conditional_means, gml.conditional_sample, gml.predictive_check):
            with pytest.raises(ValueError, match=what):  # refused before the evidence is opened: no device needed
                f(model, hist, bad)
    with pytest.raises(ValueError, match="GlauberTermChains"):
        gml.conditional_means(model, hist, [1], gml.Glauber())
    with pytest.raises(ValueError, match="replicas"):
        gml.conditional_means(model, hist, [1], replicas=0)
