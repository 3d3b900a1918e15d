"""gml_stderr without a GPU: the dense numpy model of the sandwich covariance (tests/_sandwich_reference.py) against finite
differences of the oracle's gradients, against an explicit per-sample loop and against the scatter of replicated estimates; the
argument errors of the C entry point, decided before any device work."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import _sandwich_reference as SW
import gml_amd as gml
from conftest import MODELS, ROOT, load_csv
from oracle import oracle as O

_lib = gml._lib
GML_EINVAL = 1
FORMS = ["RISE", "logRISE", "RPLE"]


def fixture_rows(name):
    s = load_csv(f"{name}_samples.csv")
    return s, s[:, 0].copy(), s[:, 1:].copy()


# ---- 1. A is the Hessian of the oracle's objective --------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["c", "mvt"])
def test_A_equals_a_central_difference_of_the_oracle_gradients(name, form):
    s, counts, spins = fixture_rows(name)
    n = spins.shape[1]
    rng = np.random.default_rng(3)
    h = 1e-5
    for u in (0, n - 1):
        x = rng.normal(scale=0.3, size=n)
        A, _, g, _, _ = SW.sandwich(form, counts, spins, u, x, np.arange(n))
        _, g0 = O.objgrad_nodes(form, counts, spins, [u], x)
        assert np.abs(g - g0[0]).max() <= 1e-12 * max(1.0, np.abs(g0).max())
        fd = np.zeros((n, n))
        for j in range(n):
            e = np.zeros(n)
            e[j] = h
            fd[:, j] = (O.objgrad_nodes(form, counts, spins, [u], x + e)[1][0] - O.objgrad_nodes(form, counts, spins, [u], x - e)[1][0]) / (2 * h)
        # step^2 x a curvature of order 1 x a safety factor
        assert np.abs(A - fd).max() <= 1e-6 * np.abs(A).max(), (name, form, u, np.abs(A - fd).max())


# ---- 2. B is the weighted covariance of the per-sample scores --------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_B_equals_the_covariance_of_scores_formed_sample_by_sample(form):
    _, counts, spins = fixture_rows("c")
    n = spins.shape[1]
    u, support = 1, [0, 1, 3]
    x = np.array([0.3, -0.2, 0.0, 0.25])
    _, B, g, _, _ = SW.sandwich(form, counts, spins, u, x, support)
    M = counts.sum()
    stat = np.array([[spins[k, u] * (1.0 if j == u else spins[k, j]) for j in support] for k in range(len(counts))])
    e = [np.exp(-sum(x[j] * stat[k, i] for i, j in enumerate(support))) for k in range(len(counts))]
    Z = sum(counts[k] / M * e[k] for k in range(len(counts)))
    gb = -sum(counts[k] / M * e[k] * stat[k] for k in range(len(counts))) / Z
    psis = []
    for k in range(len(counts)):
        if form == "RISE":
            psis.append(-e[k] * stat[k])
        elif form == "logRISE":
            psis.append(-(e[k] / Z) * (stat[k] + gb))
        else:
            a = sum(x[j] * stat[k, i] for i, j in enumerate(support))
            psis.append(-2.0 * (1.0 - 1.0 / (1.0 + np.exp(-2.0 * a))) * stat[k])
    mean = sum(counts[k] / M * psis[k] for k in range(len(counts)))
    cov = sum(counts[k] / M * np.outer(psis[k] - mean, psis[k] - mean) for k in range(len(counts)))
    assert np.abs(B - cov).max() <= 1e-14 * max(1.0, np.abs(cov).max())
    if form != "logRISE":
        assert np.abs(g - mean).max() <= 1e-15
    else:
        assert np.abs(mean).max() <= 1e-15 and np.abs(g - gb).max() <= 1e-15


# ---- 3. the predicted standard error is the scatter of replicated estimates -----------------------------------------------------------
def newton(form, counts, spins, u, support, x0=None, tol=1e-13):
    """unpenalised minimiser of node u's objective on `support` (damped Newton on the reference's own A and g)"""
    n = spins.shape[1]
    x = np.zeros(n) if x0 is None else x0.copy()
    for _ in range(100):
        A, _, g, _, _ = SW.sandwich(form, counts, spins, u, x, support)
        if np.abs(g).max() < tol:
            break
        step = np.linalg.solve(A, g)
        t = min(1.0, 1.0 / max(np.abs(step).max(), 1e-300))  # (no step longer than 1 in any coordinate)
        x[support] -= t * step
    return x


def test_replicates_scatter_as_predicted():
    """400 replicates of N = 4000 draws from model `c` with fields, node 0 on the full support: empirical sd / mean predicted se within
    1 +- 0.15 (the sd of 400 draws scatters by 1 / sqrt(2 x 399) = 3.5 %: about 4.2 sigma) for every parameter and formulation"""
    J = MODELS["c"].copy()
    np.fill_diagonal(J, [0.15, -0.1, 0.2, -0.05])
    n = 4
    states = np.array(list(itertools.product([-1.0, 1.0], repeat=n)))
    energy = np.array([sum(J[i, j] * s[i] * s[j] for i in range(n) for j in range(i + 1, n)) + sum(J[i, i] * s[i] for i in range(n)) for s in states])
    prob = np.exp(energy)
    prob /= prob.sum()
    rng = np.random.default_rng(0)
    support = np.arange(n)
    est = {f: [] for f in FORMS}
    pred = {f: [] for f in FORMS}
    for _ in range(400):
        counts = rng.multinomial(4000, prob).astype(np.float64)
        for form in FORMS:
            x = newton(form, counts, states, 0, support)
            est[form].append(x)
            pred[form].append(SW.sandwich(form, counts, states, 0, x, support)[3])
    for form in FORMS:
        ratio = np.std(np.array(est[form]), axis=0, ddof=1) / np.mean(np.array(pred[form]), axis=0)
        print(form, "empirical sd / predicted se:", ratio)
        assert np.all(np.abs(ratio - 1.0) <= 0.15), (form, ratio)
    # the unpenalised RISE and logRISE optima coincide: grad log Z = 0 <=> grad Z = 0
    assert np.abs(np.array(est["RISE"]) - np.array(est["logRISE"])).max() <= 1e-10


# ---- 4. RISE and logRISE agree at the common optimum -----------------------------------------------------------------------------------
def test_rise_and_logrise_se_agree_at_the_rise_optimum():
    _, counts, spins = fixture_rows("c")
    n = spins.shape[1]
    for u in range(n):
        x = newton("RISE", counts, spins, u, np.arange(n), tol=1e-15)
        se_r = SW.sandwich("RISE", counts, spins, u, x, np.arange(n))[3]
        se_l = SW.sandwich("logRISE", counts, spins, u, x, np.arange(n))[3]
        assert np.abs(se_r - se_l).max() <= 1e-10 * se_r.max(), (u, se_r, se_l)


# ---- 5. the C entry point: declared, exported, argument errors before any device work -------------------------------------------------
def test_entry_point_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gml.h")).read(), flags=re.S)
    L = _lib.lib()
    assert re.search(r"\bint gml_stderr\s*\(", text) and hasattr(L, "gml_stderr") and hasattr(L, "gml_test_sandwich_grams")
    consts = dict(re.findall(r"#define (GML_SE_\w+) (\d+)", text))
    assert {k: int(v) for k, v in consts.items()} == {"GML_SE_OK": 0, "GML_SE_SINGULAR": 1, "GML_SE_TOO_LARGE": 2}
    assert int(re.search(r"#define GML_ABI_VERSION (\d+)", text).group(1)) == 6  # functions only: no struct or argument list changed


@pytest.fixture()
def stub():
    """a handle that holds sizes only (n = 4 pairwise, rows 1..3): enough for everything gml_stderr checks before it needs a device"""
    L = _lib.lib()
    L.gml_test_problem_stub.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert L.gml_test_problem_stub(4, 4, 2, 1, 4, C.byref(h)) == 0
    yield h
    L.gml_problem_destroy(h)


BAD = np.ones((3, 4), dtype=np.uint8)
BAD[2, 1] = 3
NONFINITE = np.zeros((3, 4))
NONFINITE[1, 2] = np.inf
EINVAL_CASES = {
    "x NULL": (dict(x=None), "NULL"), "se NULL": (dict(se=None), "NULL"), "ld < P": (dict(ld=3), "leading dimension"),
    "ld_s < P": (dict(ld_s=3), "leading dimension"), "formulation 3": (dict(form=3), "formulation"),
    "formulation -1": (dict(form=-1), "formulation"), "structure byte 3": (dict(S=BAD), "row 2, slot 1"),
    "x not finite": (dict(x=NONFINITE), "row 1, slot 2"), "x nan": (dict(x=np.full((3, 4), np.nan)), "row 0, slot 0"),
}


@pytest.mark.parametrize("case", sorted(EINVAL_CASES))
def test_stderr_rejects_bad_arguments_before_any_device_work(stub, case):
    L = _lib.lib()
    a = dict(form=0, x=np.zeros((3, 4)), ld=4, S=np.ones((3, 4), dtype=np.uint8), ld_s=4, se=np.zeros((3, 4)))
    change, text = EINVAL_CASES[case]
    a.update(change)
    status = np.zeros(3, dtype=np.int32)
    rc = L.gml_stderr(stub, a["form"], _lib._ptr(a["x"]), a["ld"], _lib._ptr(a["S"]), a["ld_s"], _lib._ptr(a["se"]), _lib._ptr(status), None)
    msg = L.gml_last_error().decode()
    assert rc == GML_EINVAL, (case, rc, msg)  # not GML_EHIP: nothing reached the device
    assert text in msg, (case, msg)


def test_stderr_rejects_a_null_handle_and_the_front_door_its_restrictions():
    L = _lib.lib()
    z = np.zeros((3, 3))
    assert L.gml_stderr(None, 0, _lib._ptr(z), 3, None, 0, _lib._ptr(z), None, None) == GML_EINVAL
    hist = np.concatenate([np.ones((8, 1)), np.array(list(itertools.product([-1.0, 1.0], repeat=3)))], axis=1)
    for bad in (dict(devices=[0, 1]), dict(distributed=True), dict(node_range=(0, 2))):
        with pytest.raises(ValueError, match="stderr"):
            gml.learn(hist, gml.RISE(), gml.HIP(stderr=True, **bad))
    assert gml.HIP().stderr is False
