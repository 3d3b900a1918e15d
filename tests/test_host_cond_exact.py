"""Exact conditional inference without a GPU.  The brute-force restatement (_cond_exact_reference.py) is held to what it must be: one
hidden spin is tanh of its field, independent hidden spins factorise, with every spin hidden it is the model's own log Z and means
(_exact_reference.py), and on the enumeration case of the conditional chains it agrees with their yardstick
(_conditional_reference.exact_conditional).  Then the header and the bindings, every refusal of the two C entry points that is
reachable with size-only stub handles -- code and message, two faults at a time to pin the order -- and the Python front door's
ValueErrors, which all come before a handle is opened."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import gml_amd as gml
from _ais_reference import sparse_model
from _cond_exact_reference import cond_exact, cond_exact_masked, cond_exact_rows, energy, tol
from _conditional_reference import ENUM, enum_model, exact_conditional, exact_field, random_rows
from _exact_reference import LD, ExactModel

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")
EINVAL, EUNSUPPORTED = 1, gml._lib.GML_EUNSUPPORTED


# ---- the reference against closed forms -------------------------------------------------------------------------------------------
def test_one_hidden_spin_is_tanh_of_its_field():
    n = 33
    terms = sparse_model(n, 6, 4, 0.3, 4)
    terms[(5, 5, 9)] = 0.4  # a spin named twice cancels
    ev = random_rows(20, n, 0)
    for k, i in enumerate(np.arange(20) * 7 % n):
        means, log_w, log_p = cond_exact(terms, n, ev[k], [int(i)])
        field = exact_field(terms, n, ev[k], int(i))
        assert abs(float(means[0]) - np.tanh(field)) <= 1e-15
        assert abs(float(log_p) - np.log((1 + ev[k, i] * np.tanh(field)) / 2)) <= 1e-14
        up = ev[k].copy()
        up[i] = 1
        assert abs(float(log_w - (energy(terms, up) - field) - np.log(2 * np.cosh(LD(field))))) <= tol(terms)


def test_independent_hidden_spins_factorise():
    # the hidden spins 0, 3, 7 couple to visible spins only
    n, hid = 9, [0, 3, 7]
    terms = {(1,): 0.3, (1, 2): -0.4, (1, 3, 6): 0.25, (4, 5): 0.7, (4,): -0.1, (8, 9, 2, 3): -0.35, (2, 3): 0.2, (5, 6, 7): 0.15, (): 0.05}
    for row in random_rows(6, n, 2):
        means, log_w, log_p = cond_exact(terms, n, row, hid)
        fields = np.array([exact_field(terms, n, row, i) for i in hid], dtype=LD)
        assert np.abs(means - np.tanh(fields)).max() <= 1e-15  # (the fields are FP64 sums)
        base = row.copy()
        base[hid] = 1
        const = energy(terms, base) - fields.sum()
        assert abs(log_w - const - np.sum(np.log(2 * np.cosh(fields)))) <= 1e-14
        assert abs(log_p - np.sum(np.log((1 + row[hid] * np.tanh(fields)) / 2))) <= 1e-14


def test_all_hidden_is_the_model_itself():
    n = 10
    terms = sparse_model(n, 4, 3, 0.4, 9)
    terms.update({(): -0.3, (2, 2): 0.2, (3, 4): 0.0})
    ref = ExactModel(terms, n)
    for row in random_rows(3, n, 5):
        means, log_w, log_p = cond_exact(terms, n, row, range(n))
        assert abs(log_w - ref.log_z) <= 1e-16 and np.abs(means - ref.mean).max() <= 1e-16
        assert abs(log_p - (energy(terms, row) - ref.log_z)) <= 1e-16


def test_agrees_with_the_yardstick_of_the_conditional_chains():
    terms, ev = enum_model()
    n, hid = ENUM["n"], ENUM["hidden"]
    means, _, log_p = cond_exact_rows(terms, n, ev, hid)
    for k in range(ENUM["K"]):
        p, mag = exact_conditional(terms, n, ev[k], hid)
        held = sum(1 << a for a, i in enumerate(hid) if ev[k, i] < 0)
        assert np.abs(means[k] - mag).max() <= 1e-14 and abs(float(log_p[k]) - np.log(p[held])) <= 1e-13


def test_masked_reference_rows_are_the_uniform_ones():
    terms, ev = enum_model()
    mask = np.zeros(ev.shape, dtype=bool)
    mask[:, ENUM["hidden"]] = True
    mask[2] = False
    means, log_w, log_p = cond_exact_masked(terms, ENUM["n"], ev, mask)
    m, lw, lp = cond_exact_rows(terms, ENUM["n"], ev, ENUM["hidden"])
    keep = np.arange(len(ev)) != 2
    assert np.array_equal(means[keep][:, ENUM["hidden"]], m[keep]) and np.array_equal(log_w[keep], lw[keep]) and np.array_equal(log_p[keep], lp[keep])
    assert np.array_equal(means[2], ev[2].astype(LD)) and log_w[2] == energy(terms, ev[2]) and log_p[2] == 0


# ---- the header and the bindings --------------------------------------------------------------------------------------------------
def test_header_and_bindings():
    text = open(os.path.join(ROOT, "include", "gml.h")).read()
    assert "#define GML_ABI_VERSION 6" in text and gml._lib.GML_ABI_VERSION == 6  # functions only
    for name in ("gml_conditional_exact", "gml_conditional_exact_masked"):
        assert re.search(r"\bint " + name + r"\(", text), name
    assert hasattr(gml._lib, "conditional_exact") and hasattr(gml._lib, "conditional_exact_masked")
    assert gml.observed_log_likelihood is gml.likelihood.observed_log_likelihood and "observed_log_likelihood" in gml.__all__
    assert gml.Exact().max_hidden == 24 and gml.Exact().max_spins == 40
    fields = {f for f in gml.ConditionalMeans.__dataclass_fields__}
    assert {"log_w", "log_p"} <= fields and "joint_log_loss" in gml.PredictiveCheck.__dataclass_fields__


# ---- the C entry points' refusals -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    try:
        import torch  # noqa: F401  (as _lib.lib(): one HIP runtime for both, whichever loads first)
    except Exception:
        pass
    L = C.CDLL(SO)
    p, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.gml_conditional_exact.argtypes = [p, i32, p, i64, i64, p, p, p, p, p]
    L.gml_conditional_exact_masked.argtypes = [p, i32, p, i64, i64, p, p, p, p, p]
    L.gml_test_problem_stub.argtypes = [i64, i64, i32, i64, i64, C.POINTER(p)]
    L.gml_problem_destroy.argtypes = [p]
    L.gml_problem_destroy.restype = None
    L.gml_last_error.restype = C.c_char_p
    return L


@pytest.fixture(scope="module")
def stub(cdll):
    """stub(n, role): a handle of n spins that holds sizes only, one per (n, role)"""
    made = {}

    def get(n, role="evidence"):
        if (n, role) not in made:
            h = C.c_void_p()
            assert cdll.gml_test_problem_stub(n, n, 2, 0, n, C.byref(h)) == 0
            made[n, role] = h
        return made[n, role]

    yield get
    for h in made.values():
        cdll.gml_problem_destroy(h)


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


GOOD = (np.array([[0, 1, -1], [1, 2, 0], [2, -1, -1]], dtype=np.int32), np.array([0.3, -0.2, 0.5]))
NONFINITE = (GOOD[0], np.array([0.3, np.inf, 0.5]))
OUT_OF_RANGE = (np.array([[0, 1, -1], [1, 7, 0], [2, -1, -1]], dtype=np.int32), GOOD[1])
NINE = (np.array([list(range(9)), [0, 1] + [-1] * 7], dtype=np.int32), np.array([0.1, 0.2]))  # a term of nine distinct spins
NINE_ZERO = (NINE[0], np.array([0.0, 0.2]))  # ... of weight zero: it joins nothing
EIGHT_OF_TEN = (np.array([list(range(8)) + [3, 3]], dtype=np.int32), np.array([0.1]))  # ten slots, eight distinct spins after cancellation
# every key of one to three of 20 spins: 1350 distinct hidden parts when all 20 are hidden, 231 when spins 0 .. 9 are
SUBSETS_OF_20 = [c + (-1,) * (9 - len(c)) for r in (1, 2, 3) for c in itertools.combinations(range(20), r)]
SUBSETS_OF_20 = (np.array(SUBSETS_OF_20, dtype=np.int32), np.full(len(SUBSETS_OF_20), 0.01))


def hidden_of(n, spins):
    h = np.zeros(n, dtype=np.uint8)
    h[list(spins)] = 1
    return h


def uniform(cdll, stub, terms=GOOD, n=3, hidden=(0,), ev_n=None, evidence=True, outs=(1, 1, 1), keys=True, stride=None, nterms=None):
    k, w = terms
    buf = [np.zeros(64) if o else None for o in outs]
    hid = None if hidden is None else hidden_of(n, hidden)
    rc = cdll.gml_conditional_exact(ptr(k) if keys else None, k.shape[1] if stride is None else stride, ptr(w), len(w) if nterms is None else nterms,
                                    n, stub(n if ev_n is None else ev_n) if evidence else None, ptr(hid), *[ptr(b) for b in buf])
    assert all(b is None or np.all(b == 0.0) for b in buf)  # a refused call writes nothing
    return rc, cdll.gml_last_error().decode()


def masked(cdll, stub, terms=GOOD, n=3, mask_n=None, ev_n=None, evidence=True, mask=True, outs=(1, 1, 1), keys=True):
    k, w = terms
    buf = [np.zeros(64) if o else None for o in outs]
    ev = stub(n if ev_n is None else ev_n) if evidence else None
    mk = stub(n if mask_n is None else mask_n, "mask") if mask else None
    rc = cdll.gml_conditional_exact_masked(ptr(k) if keys else None, k.shape[1], ptr(w), len(w), n, ev, mk, *[ptr(b) for b in buf])
    assert all(b is None or np.all(b == 0.0) for b in buf)
    return rc, cdll.gml_last_error().decode()


# every refusal of gml_conditional_exact in its order: (arguments, code, text); entry i carries the fault of entry i + 1 as well
UNIFORM_ORDER = [
    (dict(outs=(0, 0, 0), evidence=False), EINVAL, "means, log_w and log_p are all NULL"),
    (dict(evidence=False, hidden=None), EINVAL, "evidence is NULL"),
    (dict(hidden=None, keys=False), EINVAL, "hidden is NULL"),
    (dict(keys=False, ev_n=4), EINVAL, "NULL or malformed term list"),
    (dict(ev_n=4, hidden=()), EINVAL, "evidence handle's 4 spins"),
    (dict(hidden=(), terms=NONFINITE), EINVAL, "no spin is hidden"),
    (dict(terms=NONFINITE, n=16385, hidden=(0,)), EINVAL, "weight of term 1 is not finite"),
    (dict(n=16385, hidden=range(25)), EUNSUPPORTED, "n <= 16384"),
    (dict(n=40, hidden=range(25), terms=NINE), EUNSUPPORTED, "25 spins are hidden.*at most 24"),
    (dict(n=40, hidden=range(11), terms=NINE), EUNSUPPORTED, "term 0 names 9 distinct spins.*at most 8"),
]


@pytest.mark.parametrize("case", range(len(UNIFORM_ORDER)), ids=[c[2][:28] for c in UNIFORM_ORDER])
def test_refusals_of_the_uniform_form_in_order(cdll, stub, case):
    args, code, text = UNIFORM_ORDER[case]
    rc, msg = uniform(cdll, stub, **args)
    assert rc == code and re.search(text, msg) and "HIP" not in msg, (rc, msg)


def test_further_refusals_of_the_uniform_form(cdll, stub):
    for args, code, text in [
        (dict(terms=OUT_OF_RANGE), EINVAL, "term 1 names spin 7 outside"),
        (dict(stride=0), EINVAL, "NULL or malformed term list"),
        (dict(nterms=-1), EINVAL, "NULL or malformed term list"),
        (dict(n=20, hidden=range(20), terms=SUBSETS_OF_20), EUNSUPPORTED, "1350 distinct hidden parts.*at most 1024"),
        # the nine-spin term before the hidden parts
        (dict(n=20, hidden=range(20), terms=(np.concatenate([SUBSETS_OF_20[0], NINE[0][:1]]), np.concatenate([SUBSETS_OF_20[1], NINE[1][:1]]))),
         EUNSUPPORTED, "term 1350 names 9 distinct spins"),
    ]:
        rc, msg = uniform(cdll, stub, **args)
        assert rc == code and re.search(text, msg) and "HIP" not in msg, (args.keys(), rc, msg)
    # each single output is enough to get past the first check
    for outs in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        rc, msg = uniform(cdll, stub, outs=outs, hidden=())
        assert rc == EINVAL and "no spin is hidden" in msg
    # what the limits accept is not refused by them: a zero weight joins nothing, a spin named twice cancels, 24 hidden spins and
    # n = 16384 pass (the call then goes on to look for the device, which the stubs do not have: any answer but these refusals)
    for args in (dict(n=40, hidden=range(24), terms=NINE_ZERO), dict(n=16384, hidden=range(24)), dict(n=10, hidden=(3,), terms=EIGHT_OF_TEN),
                 dict(n=20, hidden=range(10), terms=SUBSETS_OF_20)):
        rc, msg = uniform(cdll, stub, **args)
        assert not re.search("distinct spins|are hidden|n <= 16384|hidden parts|NULL|not finite|outside", msg) or rc == 0, (rc, msg)


MASKED_ORDER = [
    (dict(outs=(0, 0, 0), evidence=False), EINVAL, "means, log_w and log_p are all NULL"),
    (dict(evidence=False, mask=False), EINVAL, "evidence is NULL"),
    (dict(mask=False, keys=False), EINVAL, "mask is NULL"),
    (dict(keys=False, ev_n=4), EINVAL, "NULL or malformed term list"),
    (dict(ev_n=4, mask_n=3), EINVAL, "evidence handle's 4 spins"),
    (dict(mask_n=4, terms=OUT_OF_RANGE), EINVAL, "the mask handle \\(n = 4.*differs from the evidence handle \\(n = 3"),
    (dict(terms=NONFINITE, n=16385), EINVAL, "weight of term 1 is not finite"),
    (dict(n=16385, terms=NINE), EUNSUPPORTED, "n <= 16384"),
    (dict(n=40, terms=NINE), EUNSUPPORTED, "term 0 names 9 distinct spins.*at most 8"),
]


@pytest.mark.parametrize("case", range(len(MASKED_ORDER)), ids=[c[2][:28] for c in MASKED_ORDER])
def test_refusals_of_the_masked_form_in_order(cdll, stub, case):
    args, code, text = MASKED_ORDER[case]
    rc, msg = masked(cdll, stub, **args)
    assert rc == code and re.search(text, msg) and "HIP" not in msg, (rc, msg)


# ---- the front door ---------------------------------------------------------------------------------------------------------------
def test_front_door_refusals_before_a_handle_is_opened():
    model = {(1, 2): 0.3, (3,): 0.1, (2, 3): -0.2}
    ev = np.array([[2, 1, -1, 1], [1, -1, -1, 1]])
    holes = np.array([[2, 1, 0, 1], [1, -1, 0, 0]])
    for kw in (dict(max_hidden=0), dict(max_hidden=25), dict(max_spins=41)):
        with pytest.raises(ValueError, match="must lie in"):
            gml.Exact(**kw)
    for f, data, extra in ((gml.conditional_means, ev, ([1],)), (gml.predictive_check, ev, ([1],)), (gml.impute, holes, ())):
        with pytest.raises(ValueError, match="no sampler"):
            f(model, data, *extra, gml.GlauberTermChains(), method=gml.Exact())
        with pytest.raises(ValueError, match="replicas=1"):
            f(model, data, *extra, replicas=2, method=gml.Exact())
        with pytest.raises(ValueError, match="seed=0"):
            f(model, data, *extra, seed=1, method=gml.Exact())
        with pytest.raises(ValueError, match="or an Exact"):
            f(model, data, *extra, method=gml.AIS())
    for f in (gml.conditional_means, gml.predictive_check):
        with pytest.raises(ValueError, match="2 spins are hidden: more than max_hidden = 1"):
            f(model, ev, [1, 3], method=gml.Exact(max_hidden=1))
        with pytest.raises(ValueError, match="names no spin"):
            f(model, ev, [], method=gml.Exact())
    with pytest.raises(ValueError, match="a row lacks 2 spins: more than max_hidden = 1"):
        gml.impute(model, holes, method=gml.Exact(max_hidden=1))
    with pytest.raises(ValueError, match="a row lacks 2 spins: more than max_hidden = 1"):
        gml.observed_log_likelihood(holes, model, gml.Exact(max_hidden=1))
    wide = np.concatenate([np.ones((1, 1)), np.zeros((1, 30))], axis=1)
    with pytest.raises(ValueError, match="a row lacks 30 spins: more than max_hidden = 24"):
        gml.observed_log_likelihood(wide, {(1, 30): 0.1}, log_z=0.0)
    for bad, what in ((np.array([[1, 1, 2, 1]]), "-1, \\+1 or 0"), (np.array([[1.5, 1, 0, 1]]), "positive integers"),
                      (np.array([1, 1, 0, 1]), "histogram matrix")):
        with pytest.raises(ValueError, match=what):
            gml.observed_log_likelihood(bad, model, log_z=0.0)
        with pytest.raises(ValueError, match=what):
            gml.impute(model, bad, method=gml.Exact())
