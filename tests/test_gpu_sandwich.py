"""gml_stderr on the GPU against the dense numpy model (tests/_sandwich_reference.py): the Grams and the gradient as the finish
kernel's factorisation receives them (test hook), the standard errors, the contract cases of include/gml.h, the front door.

Inputs: iid +-1 spins, integer counts from {0, 1, 2, 3} (zero counts present), x random on the support with sum |x| = 2; the
reference's cond2(A) <= 100 is asserted before anything is compared (measured <= 6.5 on these shapes)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import _sandwich_reference as SW
import gml_amd as gml
from conftest import GOLDEN

_lib = gml._lib
pytestmark = pytest.mark.gpu
FORMS = ["RISE", "logRISE", "RPLE"]
# (n, m, K): tile edges at 16, 32 and 128, the cap, K that is no multiple of 32, 64 or 512
SHAPES = [(40, 1, 8), (40, 15, 513), (40, 16, 1037), (40, 17, 1037), (40, 33, 1037), (200, 128, 2085), (200, 129, 2085), (320, 300, 4133),
          (520, 512, 4133)]
NROWS = 2  # local rows per handle: node 0 with its field in the support, node 1 without


@functools.lru_cache(maxsize=None)
def inputs(n, m, K, uniform=False, l1=2.0):
    rng = np.random.default_rng(1000 * n + m + K)
    spins = (2 * rng.integers(0, 2, size=(K, n)) - 1).astype(np.int8)
    counts = np.ones(K) if uniform else rng.integers(0, 4, size=K).astype(np.float64)
    if not uniform:
        counts[0], counts[-1] = 0.0, 3.0
    S = np.zeros((NROWS, n), dtype=np.uint8)
    x = np.zeros((NROWS, n))
    for r in range(NROWS):
        others = np.array([j for j in range(n) if j != r])
        sup = np.sort(np.concatenate([[r], rng.choice(others, m - 1, replace=False)]) if r == 0 else rng.choice(others, m, replace=False))
        S[r, sup] = gml.FREE
        v = rng.normal(size=m)
        x[r, sup] = l1 * v / np.abs(v).sum()
    return counts, spins, S, x


@functools.lru_cache(maxsize=None)
def reference(n, m, K, form, uniform=False, l1=2.0):
    """[(support, A, B, g, se)] of the local rows; computed once, shared by the tests"""
    counts, spins, S, x = inputs(n, m, K, uniform, l1)
    out = []
    for r in range(NROWS):
        sup = np.flatnonzero(S[r])
        A, B, g, se, cond = SW.sandwich(form, counts, spins, r, x[r], sup)
        assert cond <= 100.0, (n, m, K, form, r, cond)
        out.append((sup, A, B, g, se))
    return out


def grams(prob, form, x, S, rows, cap):
    L = _lib.lib()
    L.gml_test_sandwich_grams.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    nr = len(rows)
    lists, msz = np.zeros((nr, cap), dtype=np.int32), np.zeros(nr, dtype=np.int32)
    A, B, g = np.zeros((nr, cap, cap)), np.zeros((nr, cap, cap)), np.zeros((nr, cap))
    _lib.check(L.gml_test_sandwich_grams(prob._h, _lib.FORMULATION_IDS[form], _lib._ptr(x), x.shape[1], _lib._ptr(S), S.shape[1], nr, _lib._ptr(rows),
                                         cap, _lib._ptr(lists), _lib._ptr(msz), _lib._ptr(A), _lib._ptr(B), _lib._ptr(g)))
    return lists, msz, A, B, g


def check_case(n, m, K, form, uniform=False, l1=2.0):
    counts, spins, S, x = inputs(n, m, K, uniform, l1)
    ref = reference(n, m, K, form, uniform, l1)
    with _lib.Problem(counts=None if uniform else counts, spins=spins, node_range=(0, NROWS)) as prob:
        lists, msz, A, B, g = grams(prob, form, x, S, np.arange(NROWS), m)
        se, status = prob.stderr(form, x, structure=S)
    for r, (sup, A0, B0, g0, se0) in enumerate(ref):
        assert msz[r] == m and np.array_equal(lists[r], sup)
        for name, got, want in (("A", A[r], A0), ("B", B[r], B0), ("g", g[r], g0)):
            err = np.abs(got - want).max() / np.abs(want).max()
            print(f"{(n, m, K)} {form} row {r} {name}: {err:.2e}")
            assert err <= 1e-12, (name, r, err)
        assert status[r] == 0
        err = np.abs(se[r, sup] - se0).max() / se0.max()
        print(f"{(n, m, K)} {form} row {r} se: {err:.2e}")
        assert err <= 1e-9, (r, err)  # (2 cond + 1) x 1e-12 <= 2e-10 at cond <= 100, with a 5x margin
        off = np.ones(n, dtype=bool)
        off[sup] = False
        assert np.all(se[r, off] == 0.0)


# ---- 1 + 2. Grams through the hook, and se, against the reference ----------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-m%d-K%d" % s)
def test_grams_and_se_match_the_reference(shape, form):
    check_case(*shape, form)


@pytest.mark.parametrize("form", FORMS)
def test_uniform_counts(form):
    check_case(40, 17, 1037, form, uniform=True)


def test_weights_spread_over_many_orders_of_magnitude():
    check_case(40, 16, 1037, "RISE", l1=8.0)  # exp(-a) over e^16, the same relative tolerance


# ---- 3. contract cases --------------------------------------------------------------------------------------------------------------------
def test_host_and_device_pointers_give_the_same_bits():
    import torch
    counts, spins, S, x = inputs(40, 17, 1037)
    with _lib.Problem(counts=counts, spins=spins, node_range=(0, NROWS)) as prob:
        se, status = prob.stderr("RISE", x, structure=S)
        dx, dS = torch.from_numpy(x).cuda(), torch.from_numpy(S).cuda()
        dse = torch.full((NROWS, 40), 7.0, dtype=torch.float64, device="cuda")
        st2 = np.zeros(NROWS, dtype=np.int32)
        torch.cuda.synchronize()
        _lib.check(_lib.lib().gml_stderr(prob._h, 0, C.c_void_p(dx.data_ptr()), 40, C.c_void_p(dS.data_ptr()), 40, C.c_void_p(dse.data_ptr()),
                                         _lib._ptr(st2), None))
        assert np.array_equal(dse.cpu().numpy(), se) and np.array_equal(st2, status)
        # mixed: device x, host structure and se
        se3 = np.zeros_like(se)
        _lib.check(_lib.lib().gml_stderr(prob._h, 0, C.c_void_p(dx.data_ptr()), 40, _lib._ptr(S), 40, _lib._ptr(se3), None, None))
        assert np.array_equal(se3, se)


def test_a_node_shard_equals_the_rows_of_the_full_handle():
    n, K = 24, 1037
    rng = np.random.default_rng(5)
    spins = (2 * rng.integers(0, 2, size=(K, n)) - 1).astype(np.int8)
    counts = rng.integers(0, 4, size=K).astype(np.float64)
    x = rng.normal(scale=0.1, size=(n, n)) * (rng.random((n, n)) < 0.4)
    with _lib.Problem(counts=counts, spins=spins) as full:
        se_full, st_full = full.stderr("logRISE", x)  # the reference's structure: the field free, non-zero couplings in the support
    with _lib.Problem(counts=counts, spins=spins, node_range=(7, 19)) as shard:
        se_sh, st_sh = shard.stderr("logRISE", x[7:19])
    assert np.array_equal(se_sh, se_full[7:19]) and np.array_equal(st_sh, st_full[7:19])
    for u in (0, 7, 23):
        sup = np.flatnonzero((x[u] != 0) | (np.arange(n) == u))
        se0 = SW.sandwich("logRISE", counts, spins, u, x[u], sup)[3]
        assert np.abs(se_full[u, sup] - se0).max() <= 1e-9 * se0.max()
        assert np.count_nonzero(se_full[u]) == len(sup)


def test_order_three_with_mixed_kinds():
    n, K, order = 12, 1037, 3
    rng = np.random.default_rng(7)
    spins = (2 * rng.integers(0, 2, size=(K, n)) - 1).astype(np.int8)
    counts = rng.integers(0, 4, size=K).astype(np.float64)
    with _lib.Problem(counts=counts, spins=spins, order=order, node_range=(3, 6)) as prob:
        P = prob.P
        assert P == 67
        S = rng.integers(0, 3, size=(3, P)).astype(np.uint8)
        x = rng.normal(scale=0.05, size=(3, P)) * (S != gml.EXCLUDED) * (rng.random((3, P)) < 0.7)
        S[1, 0] = gml.EXCLUDED  # row 1: no field
        x[1, 0] = 0.0
        se, status = prob.stderr("RISE", x, structure=S)
        for r in range(3):
            keys = [tuple(int(v) for v in k) for k in prob.multi_keys_array(3 + r)]
            sup = np.flatnonzero((S[r] == gml.FREE) | ((S[r] == gml.PENALISED) & (x[r] != 0)))
            _, _, _, se0, cond = SW.sandwich("RISE", counts, spins, 3 + r, x[r], sup, keys=keys)
            assert cond <= 100.0 and status[r] == 0
            assert np.abs(se[r, sup] - se0).max() <= 1e-9 * se0.max()
            assert np.count_nonzero(se[r]) == len(sup)
        assert se[1, 0] == 0.0


def test_empty_rows_oversized_and_singular_supports():
    n, K = 520, 1037
    rng = np.random.default_rng(11)
    spins = (2 * rng.integers(0, 2, size=(K, n)) - 1).astype(np.int8)
    spins[:, 6] = spins[:, 5]  # two identical spin columns
    counts = rng.integers(0, 4, size=K).astype(np.float64)
    S = np.zeros((4, n), dtype=np.uint8)
    x = np.zeros((4, n))
    S[0, :513] = gml.FREE                    # row 0: 513 entries, the first size above the cap of 512
    S[1, [1, 5, 6, 9]] = gml.FREE            # row 1: a duplicated statistic
    x[1, [1, 5, 6, 9]] = [0.1, 0.2, -0.1, 0.3]
    S[2, [0, 2, 5, 40]] = [gml.PENALISED, gml.FREE, gml.PENALISED, gml.PENALISED]  # row 2: regular (slot 0 penalised at x = 0: outside)
    x[2, [2, 5, 40]] = [0.2, -0.3, 0.4]
    S[3, 7] = gml.PENALISED                  # row 3: empty support (its one parameter is penalised and zero)
    with _lib.Problem(counts=counts, spins=spins, node_range=(0, 4)) as prob:
        se, status = prob.stderr("RPLE", x, structure=S)
        assert list(status) == [2, 1, 0, 0]
        assert np.all(np.isnan(se[0, :513])) and np.all(se[0, 513:] == 0.0)
        assert np.all(np.isnan(se[1, [1, 5, 6, 9]])) and np.count_nonzero(np.nan_to_num(se[1], nan=1.0)) == 4
        sup = np.array([2, 5, 40])
        se0 = SW.sandwich("RPLE", counts, spins, 2, x[2], sup)[3]
        assert np.abs(se[2, sup] - se0).max() <= 1e-9 * se0.max() and np.count_nonzero(se[2]) == 3
        assert np.all(se[3] == 0.0)
        # a non-zero x at an excluded slot: GML_EINVAL naming row and slot
        x[2, 17] = 0.5
        with pytest.raises(gml.GMLError, match="row 2, slot 17") as e:
            prob.stderr("RPLE", x, structure=S)
        assert e.value.code == 1


# ---- 4. the front door ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("c", "RISE"), ("mvt", "logRISE"), ("mvt", "RPLE")])
def test_front_door(name, form):
    samples = np.loadtxt(os.path.join(GOLDEN, f"{name}_samples.csv"), delimiter=",")
    F = {"RISE": gml.RISE, "logRISE": gml.logRISE, "RPLE": gml.RPLE}[form]
    c = F().regularizer
    n = samples.shape[1] - 1
    m = gml.HIP(refit=0.05, stderr=True)
    rows = gml.learn(samples, F(c, False), m)  # without symmetrisation: the refit rows themselves
    se, status = m.stats["stderr"], m.stats["stderr_status"]
    assert se.shape == (n, n) and np.all(status == 0) and "stderr_sym_bound" not in m.stats
    for u in range(n):
        sup = np.flatnonzero((rows[u] != 0) | (np.arange(n) == u))
        se0 = SW.sandwich(form, samples[:, 0], samples[:, 1:], u, rows[u], sup)[3]
        assert np.abs(se[u, sup] - se0).max() <= 1e-9 * se0.max(), (u, se[u, sup], se0)
        assert np.array_equal(np.flatnonzero(se[u]), sup)
    assert np.array_equal(m.stats["z"], np.divide(rows, se, out=np.zeros_like(rows), where=se > 0))
    ms = gml.HIP(refit=0.05, stderr=True)
    gml.learn(samples, F(c, True), ms)  # the same solves, then symmetrised
    assert np.array_equal(ms.stats["stderr"], se) and np.array_equal(ms.stats["z"], m.stats["z"])
    assert np.array_equal(ms.stats["stderr_sym_bound"], 0.5 * (se + se.T))
    assert np.array_equal(np.diag(ms.stats["stderr_sym_bound"]), np.diag(se))
    # a plain call: the fused route as before, no stderr key
    plain = gml.HIP()
    got = gml.learn(samples, F(c, True), plain)
    with _lib.Problem(samples) as prob:
        want = prob.learn(form, c, matrix=True)[0]
    assert np.array_equal(got, want) and "stderr" not in plain.stats and "z" not in plain.stats
