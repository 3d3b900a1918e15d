"""gml_model_elim_plan and gml_model_elim without a GPU.  The independent sum-product of _elim_reference.py is held to brute force
(_exact_reference.ExactModel); the library's planner -- order, width, work, stored -- is compared with `==` against the rule restated
in Python; the refusals come in their stated order before any device work; then the Python front door with the device step
substituted, the exports and the ABI version."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

import gml_amd as gml
import _elim_reference as R
from _exact_reference import ExactModel, LD

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")


# ---- the reference against brute force ---------------------------------------------------------------------------------------------
BRUTE = {
    "lattice_4x4": lambda: R.lattice(4, 4, seed=3),
    "ladder_14": lambda: R.triples_ladder(14, seed=2),
    "cylinder_3x6": lambda: R.lattice(3, 6, seed=5, periodic=True),
    "order5": R.order5,
    "mixed_conventions": R.mixed_conventions,
}


@pytest.mark.parametrize("case", sorted(BRUTE))
def test_reference_against_brute_force(case):
    terms, n = BRUTE[case]()
    if case != "mixed_conventions":
        terms = {**terms, (): 0.37}
    ref, brute = R.SumProduct(terms, n), ExactModel(terms, n)
    assert abs(ref.log_z - brute.log_z) < 1e-17 * 64
    assert np.abs(ref.mean - brute.mean).max() < 1e-17
    want = np.array([brute.expectation(k) for k in terms], dtype=LD)
    seen = ~np.isnan(ref.texp)
    assert np.abs(ref.texp - want)[seen].max() < 1e-17
    # NaN exactly where the contract says so: a zero weight over two or more spins
    assert [k for k, s in zip(terms, seen) if not s] == [k for k, w in terms.items() if w == 0.0 and len(R.reduce_key(k)) > 1]


def test_reference_rules_on_the_mixed_model():
    terms, n = R.mixed_conventions()
    ref = R.SumProduct(terms, n)
    keys = list(terms)
    assert ref.texp[keys.index(())] == 1 and ref.texp[keys.index((3, 3))] == 1      # the empty key, a key that cancels
    assert ref.texp[keys.index((2,))] == ref.mean[1] and np.isnan(ref.texp[keys.index((1, 7))])  # zero weights: one spin, two
    assert ref.mean[8] == 0                                                         # the isolated spin
    assert abs(ref.texp[keys.index((2, 2, 4))] - ref.mean[3]) < 1e-18              # a duplicated spin cancels


def test_bound_of_the_8x8_lattice():
    assert 2e-12 < R.bound(*R.lattice(8, 8)) < 8e-12  # (the figure checked by hand: about 4e-12)


# ---- the planner ---------------------------------------------------------------------------------------------------------------------
PLANS = {  # the model and the width of its greedy order
    "lattice_8x8": (lambda: R.lattice(8, 8), 9),
    "lattice_16x16": (lambda: R.lattice(16, 16), 17),
    "lattice_6x40": (lambda: R.lattice(6, 40), 7),
    "chimera_2": (lambda: R.chimera(2), 12),
    "chimera_3": (lambda: R.chimera(3), 16),
    "chimera_4": (lambda: R.chimera(4), 20),
    "tree_200": (lambda: R.tree(200), 12),
    "regular3_60": (lambda: R.regular3(60), 13),
    "regular3_100": (lambda: R.regular3(100), 21),
    "ladder_64": (lambda: R.triples_ladder(64), 3),
    "mixed_conventions": (R.mixed_conventions, 4),
    "tree_16384": (lambda: R.tree(16384, back=8), 6),
}


@pytest.mark.parametrize("case", sorted(PLANS))
def test_plan_equals_the_python_rule(case):
    make, width = PLANS[case]
    terms, n = make()
    order, w, work, stored = gml._lib.model_elim_plan(terms, n)
    seq, w0, work0, stored0 = R.plan(terms, n)
    assert w == w0 == width
    assert order.tolist() == seq and work == work0 and stored == stored0
    assert sorted(seq) == list(range(1, n + 1))


@pytest.mark.parametrize("case", ["lattice_8x8", "mixed_conventions", "tree_200"])
def test_plan_of_a_callers_permutation(case):
    terms, n = PLANS[case][0]()
    perm = np.random.default_rng(11).permutation(n) + 1
    order, w, work, stored = gml._lib.model_elim_plan(terms, n, perm)
    seq, w0, work0, stored0 = R.plan(terms, n, perm)
    assert order.tolist() == seq and (w, work, stored) == (w0, work0, stored0)
    # the natural order of a lattice: one row of frontier
    if case == "lattice_8x8":
        assert gml._lib.model_elim_plan(terms, n, np.arange(1, n + 1))[1] == 9
        assert order.tolist() == perm.tolist()  # one component: the permutation as given


def test_plan_never_refuses_a_wide_model():
    dense = {(a, b): 0.01 for a in range(1, 46) for b in range(a + 1, 46)}
    order, w, work, stored = gml._lib.model_elim_plan(dense, 45)
    assert w == 45 and order.tolist() == list(range(1, 46)) and work == sum(2.0 ** k for k in range(1, 46))


# ---- the C entry points: refusals before any device work ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(SO)
    p = C.c_void_p
    L.gml_model_elim_plan.argtypes = [p, C.c_int, p, C.c_int64, C.c_int64, p, p, p, p, p]
    L.gml_model_elim.argtypes = [p, C.c_int, p, C.c_int64, C.c_int64, p, C.c_int, p, p, p]
    L.gml_last_error.restype = C.c_char_p
    return L


KEYS = np.array([[0, 1, -1], [1, 2, 0], [2, -1, -1]], dtype=np.int32)
WTS = np.array([0.3, -0.2, 0.5])


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _elim(L, keys=KEYS, wts=WTS, n=3, order=None, stride=None, nterms=None, null_keys=False, null_wts=False, null_logz=False, moments=True):
    keys, wts = np.ascontiguousarray(keys, dtype=np.int32), np.ascontiguousarray(wts, dtype=np.float64)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    logz, mean, texp = np.zeros(1), np.zeros(max(n, 1)), np.zeros(max(len(wts), 1))
    rc = L.gml_model_elim(None if null_keys else _ptr(keys), keys.shape[1] if stride is None else stride, None if null_wts else _ptr(wts),
                          len(wts) if nterms is None else nterms, n, _ptr(order), 0, None if null_logz else _ptr(logz),
                          _ptr(mean) if moments else None, _ptr(texp) if moments else None)
    return rc, L.gml_last_error().decode()


EINVAL = {
    "null_log_z": dict(null_logz=True), "null_keys": dict(null_keys=True), "null_weights": dict(null_wts=True), "stride0": dict(stride=0),
    "nterms_negative": dict(nterms=-1), "n0": dict(n=0), "spin_high": dict(keys=[[0, 3, -1], [1, 2, 0], [2, -1, -1]]),
    "nan": dict(wts=[0.3, np.nan, 0.5]), "order_repeats": dict(order=[0, 1, 1]), "order_high": dict(order=[0, 1, 3]),
    "order_negative": dict(order=[0, -1, 2]),
}


@pytest.mark.parametrize("case", sorted(EINVAL))
def test_einval_before_device_work(cdll, case):
    rc, msg = _elim(cdll, **EINVAL[case])
    assert rc == 1 and "HIP" not in msg, (case, rc, msg)
    if case.startswith("order"):
        assert "permutation" in msg


def test_plan_rejects_bad_arguments_too(cdll):
    bad = np.array([0, 0, 2], dtype=np.int32)
    assert cdll.gml_model_elim_plan(_ptr(KEYS), 3, _ptr(WTS), 3, 3, _ptr(bad), None, None, None, None) == 1
    assert cdll.gml_model_elim_plan(_ptr(KEYS), 0, _ptr(WTS), 3, 3, None, None, None, None, None) == 1
    assert cdll.gml_model_elim_plan(_ptr(KEYS), 3, _ptr(WTS), 3, 3, None, None, None, None, None) == 0  # every output is optional


def _dense(n):
    keys = np.array([[a, b] for a in range(n) for b in range(a + 1, n)], dtype=np.int32)
    return keys, np.full(len(keys), 0.01)


def test_refusals_in_their_order(cdll):
    keys, wts = _dense(45)
    rc, msg = _elim(cdll, keys=keys, wts=wts, n=45)
    assert rc == 5 and "width 45" in msg and "limited to 30" in msg and "HIP" not in msg, (rc, msg)  # GML_EUNSUPPORTED, no device needed
    # a bad argument comes before the width ...
    assert _elim(cdll, keys=keys, wts=wts, n=45, order=[0] * 45)[0] == 1
    assert _elim(cdll, keys=keys, wts=wts, n=45, null_logz=True)[0] == 1
    # ... the width before the store of the moments, and log Z alone never stores: nine dense blocks of 30 spins have width 30 and
    # keep about 2^30 forward entries each, 9 x 2^30 > 2^32
    n = 30
    kk, shift = _dense(n)[0], []
    for r in range(9):
        shift.append(kk + r * n)
    keys9 = np.concatenate(shift)
    rc, msg = _elim(cdll, keys=keys9, wts=np.full(len(keys9), 0.01), n=9 * n)
    assert rc == 5 and "2^32" in msg and "HIP" not in msg, (rc, msg)
    import torch
    if not torch.cuda.is_available():  # (with a device the call would run nine width-30 components)
        rc, msg = _elim(cdll, keys=keys9, wts=np.full(len(keys9), 0.01), n=9 * n, moments=False)
        assert rc == 3 and "no HIP device" in msg, (rc, msg)  # past every refusal: the device is looked for last


def test_valid_arguments_reach_the_device_lookup(cdll):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the calls would succeed (tests/test_gpu_elim.py holds their results)")
    for kw in (dict(), dict(moments=False), dict(order=[2, 0, 1])):
        rc, msg = _elim(cdll, **kw)
        assert rc == 3 and "no HIP device" in msg, (rc, msg)


# ---- the Python front door, the device step substituted ------------------------------------------------------------------------------
@pytest.fixture()
def substituted(monkeypatch):
    """_lib.model_elim answered by the reference; the plan stays the library's (host only)"""
    calls = []

    def model_elim(terms, n, order=None, mean=True, texp=True, device=0):
        keys, wts, _, n = gml._lib.term_arrays(terms, n)
        model = {tuple(int(v) + 1 for v in k if v >= 0): float(w) for k, w in zip(keys, wts)}
        assert len(model) == len(wts)
        ref = R.SumProduct(model, int(n))
        calls.append(dict(order=order, mean=mean, texp=texp))
        return float(ref.log_z), ref.mean.astype(float) if mean else None, ref.texp.astype(float) if texp else None

    monkeypatch.setattr(gml._lib, "model_elim", model_elim)
    return calls


def test_elimination_class_and_exports():
    assert gml.Elimination().max_width == 26 and gml.Elimination(30).max_width == 30 and gml.Elimination().order is None
    for bad in (0, 31, -2):
        with pytest.raises(ValueError, match="max_width"):
            gml.Elimination(bad)
    assert {"Elimination", "model_term_moments"} <= set(gml.__all__)
    assert gml.Elimination is gml.likelihood.Elimination and gml.model_term_moments is gml.likelihood.model_term_moments
    assert hasattr(gml._lib, "model_elim") and hasattr(gml._lib, "model_elim_plan")


def test_log_partition_through_the_front_door(substituted):
    terms, n = R.lattice(4, 4, seed=3)
    brute = ExactModel(terms, n)
    lp = gml.log_partition(terms, gml.Elimination())
    assert abs(lp.log_z - float(brute.log_z)) < 1e-14 and lp.stderr == 0.0 and np.isnan(lp.ess) and len(lp.log_weights) == 0
    assert substituted == [dict(order=None, mean=False, texp=False)]
    perm = np.random.default_rng(3).permutation(n) + 1
    gml.log_partition(terms, gml.Elimination(order=perm))
    assert substituted[-1]["order"].tolist() == perm.tolist()


def test_max_width_refuses_before_the_device_step(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device step was reached")

    monkeypatch.setattr(gml._lib, "model_elim", boom)
    terms, n = R.lattice(8, 8)
    with pytest.raises(ValueError, match="width 9, above max_width = 8"):
        gml.log_partition(terms, gml.Elimination(8))
    with pytest.raises(ValueError, match="max_width = 5"):
        gml.model_term_moments(terms, gml.Elimination(5))
    with pytest.raises(ValueError, match="width 5, above max_width = 2"):
        gml.most_probable_states(R.lattice(4, 4)[0], log_prob=True, method=gml.Elimination(2))


def test_model_term_moments_through_the_front_door(substituted):
    terms, n = R.mixed_conventions()
    m, e = gml.model_term_moments(terms, gml.Elimination())
    brute = ExactModel(terms, n)
    assert len(m) == 8  # (a dict names no spin 9: the isolated one is not part of it)
    assert np.abs(m - brute.mean.astype(float)[:8]).max() < 1e-15
    want = np.array([float(brute.expectation(k)) for k in terms])
    seen = ~np.isnan(e)
    assert np.abs(e - want)[seen].max() < 1e-15 and (~seen).sum() == 1
    assert substituted == [dict(order=None, mean=True, texp=True)]
    with pytest.raises(ValueError, match="Exact or Elimination"):
        gml.model_term_moments(terms, gml.AIS())


def test_model_term_moments_of_an_array_backed_model(substituted, monkeypatch):
    """a learned model holds its terms as one weight array over every key up to its order (factor_graph.TermArray), most of them
    zero: the library gets the non-zero ones, and the result comes back at full length with NaN at the zero weights"""
    from gml_amd.factor_graph import FactorGraph, TermArray
    n = 6
    count = gml._lib.terms_count(n, 2, True)
    blank = TermArray(n, 2, True, np.zeros(count))
    w = np.zeros(count)
    model = {(1,): 0.2, (4,): -0.3, (1, 2): 0.5, (2, 3): -0.4, (3, 4): 0.3, (5, 6): 0.6}
    for k, v in model.items():
        w[blank.rank(k)] = v
    fg = FactorGraph(2, n, terms=TermArray(n, 2, True, w))
    brute = ExactModel(model, n)
    keys = list(fg.terms)
    assert len(keys) == count == 21
    m, e = gml.model_term_moments(fg, gml.Elimination())
    assert len(e) == count and np.abs(m - brute.mean.astype(float)).max() < 1e-15
    for t, k in enumerate(keys):
        if k in model:
            assert abs(e[t] - float(brute.expectation(k))) < 1e-15, k
        else:
            assert np.isnan(e[t]), k
    # Exact(): the model's own keys as queries, every one answered (the device step substituted by brute force)
    def model_exact(terms, n, queries=None, pairs=True, device=0):
        return float(brute.log_z), brute.mean.astype(float), None, np.array([float(brute.expectation(k)) for k in queries])

    monkeypatch.setattr(gml._lib, "model_exact", model_exact)
    m2, e2 = gml.model_term_moments(fg)
    assert len(e2) == count and not np.isnan(e2).any()
    assert all(e2[t] == e[t] or np.isnan(e[t]) or abs(e2[t] - e[t]) < 1e-15 for t in range(count))
    assert e2[keys.index((1, 5))] == float(brute.mean[0] * brute.mean[4])  # a key across components, which only Exact() answers


def test_other_methods_are_refused_as_before():
    with pytest.raises(ValueError, match="takes an AIS method, given int"):
        gml.log_partition({(1, 2): 0.3}, 7)


def test_abi_version_is_still_6(cdll):
    assert cdll.gml_abi_version() == 6 and gml._lib.GML_ABI_VERSION == 6
    assert hasattr(cdll, "gml_model_elim") and hasattr(cdll, "gml_model_elim_plan")
