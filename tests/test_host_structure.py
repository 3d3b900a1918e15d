"""Structured learn, host side: the numpy restatement of the two structure builders (tests/_structure_reference.py) against a
brute-force dict implementation, the three C entry points (declared, exported, every GML_EINVAL case decided before any device work)
and the argument errors of the Python layer.  No GPU needed."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import _structure_reference as SR
import gml_amd as gml
from conftest import ROOT
from oracle import oracle as O

_lib = gml._lib
GML_OK, GML_EINVAL, GML_EHIP = 0, 1, 3
RULES = ["row", "mean", "all", "any"]


# ---- the reference against a brute-force implementation ------------------------------------------------------------------------------
def brute_tables(n, order):
    """{(u, frozenset of the other spins): slot} from the oracle's key lists (pairwise: the slot layout of the C ABI)"""
    slot = {}
    for u in range(n):
        if order == 2:
            for j in range(n):
                slot[(u, frozenset() if j == u else frozenset([j]))] = j
        else:
            for j, k in enumerate(O.multi_keys(n, order, u)):
                assert k[0] == u
                slot[(u, frozenset(k[1:]))] = j
    return slot


def brute_from_rows(rows, n, order, thr, rule, keep, drop, field):
    slot = brute_tables(n, order)
    S = np.full(rows.shape, 255, dtype=np.uint8)
    kept = 0
    for (u, rest), j in slot.items():
        if not rest:
            S[u, j] = field
            continue
        key = sorted(rest | {u})
        vals = [float(rows[v, slot[(v, frozenset(key) - {v})]]) for v in key]
        if rule == "row":
            k = abs(float(rows[u, j])) >= thr
        elif rule == "mean":
            k = abs(sum(vals[1:], vals[0]) / len(vals)) >= thr
        elif rule == "all":
            k = sum(abs(v) >= thr for v in vals) == len(vals)  # (a NaN counts as below)
        else:
            k = sum(abs(v) >= thr for v in vals) > 0
        S[u, j] = keep if k else drop
        kept += bool(k)
    return S, kept


@pytest.mark.parametrize("order", [2, 3, 4])
def test_reference_slot_order_is_the_reference_key_order(order):
    n = 5
    for u in range(n):
        want = O.multi_keys(n, order, u)
        got = SR.node_keys(n, order, u)
        if order == 2:  # the pairwise layout of the C ABI: slot j <-> spin j, slot u = the field
            assert got == [(u,) if j == u else (u, j) for j in range(n)] and sorted(got) == sorted(want)
        else:
            assert got == want
    assert SR.params_per_node(n, order) == _lib.params_per_node(n, order)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("order", [2, 3, 4])
def test_reference_from_rows_equals_brute_force(order, rule):
    n = 5
    rng = np.random.default_rng(10 * order + RULES.index(rule))
    rows = rng.normal(size=(n, SR.params_per_node(n, order)))
    rows[1, 2] = np.nan  # compares false: dropped (with its whole key under mean / all; alone under row)
    for thr in (0.0, float(np.nanmedian(np.abs(rows)))):
        got, kept = SR.structure_from_rows(rows, n, order, thr, rule, keep=2, drop=0, field=1)
        want, kept_b = brute_from_rows(rows, n, order, thr, rule, 2, 0, 1)
        assert np.array_equal(got, want) and kept == kept_b == int((got == 2).sum())
    assert got[1, 2] == 0 or rule == "any"


@pytest.mark.parametrize("order", [2, 3, 4])
def test_reference_from_keys_equals_brute_force(order):
    n = 5
    slot = brute_tables(n, order)
    rng = np.random.default_rng(order)
    keys = [tuple(int(v) for v in rng.choice(n, size=int(rng.integers(1, order + 1)), replace=False)) for _ in range(12)]
    keys += keys[:3]  # duplicates are harmless
    got = SR.structure_from_keys(keys, n, order, listed=2, other=0, field=1)
    want = np.zeros_like(got)
    for (u, rest), j in slot.items():
        listed = any(set(k) == rest | {u} for k in keys)
        want[u, j] = 2 if listed else (1 if not rest else 0)
    assert np.array_equal(got, want)


# ---- the C entry points ---------------------------------------------------------------------------------------------------------------
def test_three_entry_points_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gml.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ("gml_learn_structured", "gml_structure_from_rows", "gml_structure_from_keys"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert hasattr(L, name), name
    consts = dict(re.findall(r"#define (GML_(?:PARAM|RULE)_\w+) (\d+)", text))
    assert {k: int(v) for k, v in consts.items()} == {"GML_PARAM_EXCLUDED": 0, "GML_PARAM_FREE": 1, "GML_PARAM_PENALISED": 2, "GML_RULE_ROW": 0,
                                                       "GML_RULE_MEAN": 1, "GML_RULE_ALL": 2, "GML_RULE_ANY": 3}
    assert (gml.EXCLUDED, gml.FREE, gml.PENALISED) == (0, 1, 2) and _lib.RULES == {"row": 0, "mean": 1, "all": 2, "any": 3}
    assert int(re.search(r"#define GML_ABI_VERSION (\d+)", text).group(1)) == 6  # no struct or argument list changed


def from_rows(rows, ld, n, order, rule, thr, keep, drop, field, S, ld_s, kept=None):
    L = _lib.lib()
    rc = L.gml_structure_from_rows(None if rows is None else _lib._ptr(rows), ld, n, order, rule, thr, keep, drop, field, 0,
                                   None if S is None else _lib._ptr(S), ld_s, kept)
    return rc, L.gml_last_error().decode()


def from_keys(keys, stride, nterms, n, order, listed, other, field, S, ld_s):
    L = _lib.lib()
    rc = L.gml_structure_from_keys(None if keys is None else _lib._ptr(keys), stride, nterms, n, order, listed, other, field, 0,
                                   None if S is None else _lib._ptr(S), ld_s)
    return rc, L.gml_last_error().decode()


ROWS_CASES = {
    "rows NULL": dict(rows=None), "structure NULL": dict(S=None), "order 0": dict(order=0), "rule -1": dict(rule=-1), "rule 4": dict(rule=4),
    "keep 3": dict(keep=3), "drop -1": dict(drop=-1), "field 7": dict(field=7), "threshold negative": dict(thr=-0.1),
    "threshold nan": dict(thr=float("nan")), "threshold inf": dict(thr=float("inf")), "ld < P": dict(ld=6), "ld_s < P": dict(ld_s=6), "n 0": dict(n=0),
}


@pytest.mark.parametrize("case", sorted(ROWS_CASES))
def test_from_rows_rejects_bad_arguments_before_any_device_work(case):
    n, order = 4, 3
    P = SR.params_per_node(n, order)  # 7
    a = dict(rows=np.zeros((n, P)), ld=P, n=n, order=order, rule=1, thr=0.1, keep=1, drop=0, field=1, S=np.zeros((n, P), dtype=np.uint8), ld_s=P)
    a.update(ROWS_CASES[case])
    rc, msg = from_rows(**a)
    assert rc == GML_EINVAL, (case, rc, msg)  # not GML_EHIP: nothing reached the device
    assert msg


KEYS_CASES = {
    "structure NULL": (dict(S=None), "NULL"), "keys NULL": (dict(keys=None), "NULL"), "stride 0": (dict(stride=0), "key_stride"),
    "nterms negative": (dict(nterms=-1), "nterms"), "listed 3": (dict(listed=3), "kinds"), "other 9": (dict(other=9), "kinds"),
    "field -1": (dict(field=-1), "kinds"), "ld_s < P": (dict(ld_s=6), "leading dimension"), "order 0": (dict(order=0), "order"),
    "spin out of range": (dict(keys=np.array([[0, 1, -1], [1, 4, -1]], dtype=np.int32)), "term 1 names spin 4"),
    "spin below -1": (dict(keys=np.array([[0, 1, -1], [-2, 1, -1]], dtype=np.int32)), "term 1 names spin -2"),
    "spin twice": (dict(keys=np.array([[0, 1, -1], [2, -1, 2]], dtype=np.int32)), "term 1 names spin 2 twice"),
    "key longer than the order": (dict(keys=np.array([[0, 1, 2, 3], [0, 1, -1, -1]], dtype=np.int32), stride=4), "term 0 has 4 spins"),
    "empty key": (dict(keys=np.array([[0, 1, -1], [-1, -1, -1]], dtype=np.int32)), "term 1 names no spin"),
}


@pytest.mark.parametrize("case", sorted(KEYS_CASES))
def test_from_keys_rejects_bad_arguments_before_any_device_work(case):
    n, order = 4, 3
    P = SR.params_per_node(n, order)
    a = dict(keys=np.array([[0, 1, -1], [2, -1, -1]], dtype=np.int32), stride=3, nterms=2, n=n, order=order, listed=2, other=0, field=1,
             S=np.zeros((n, P), dtype=np.uint8), ld_s=P)
    change, text = KEYS_CASES[case]
    a.update(change)
    rc, msg = from_keys(**a)
    assert rc == GML_EINVAL, (case, rc, msg)
    assert text in msg, (case, msg)


def test_learn_structured_rejects_a_null_handle():
    L = _lib.lib()
    S = np.ones((3, 3), dtype=np.uint8)
    out = np.zeros((3, 3))
    assert L.gml_learn_structured(None, 0, 0.4, None, _lib._ptr(S), 3, None, _lib._ptr(out), None, None) == GML_EINVAL


def test_valid_arguments_reach_the_device_or_fail_loudly():
    # without a GPU: GML_EHIP, never a host fallback; with one: the reference's bytes
    n, order = 4, 3
    P = SR.params_per_node(n, order)
    rows = np.random.default_rng(0).normal(size=(n, P))
    S = np.zeros((n, P), dtype=np.uint8)
    kept = C.c_int64(-1)
    rc, msg = from_rows(rows, P, n, order, 1, 0.5, 1, 0, 1, S, P, C.byref(kept))
    assert rc in (GML_OK, GML_EHIP), (rc, msg)
    if rc == GML_OK:
        want, k = SR.structure_from_rows(rows, n, order, 0.5, "mean", 1, 0, 1)
        assert np.array_equal(S, want) and kept.value == k
    keys = np.array([[0, 1, -1], [2, -1, -1], [3, 1, 0]], dtype=np.int32)
    rc2, msg = from_keys(keys, 3, 3, n, order, 2, 0, 1, S, P)
    assert rc2 == rc, (rc2, msg)
    if rc2 == GML_OK:
        assert np.array_equal(S, SR.structure_from_keys([(0, 1), (2,), (3, 1, 0)], n, order, 2, 0, 1))
    else:
        with pytest.raises(gml.GMLError) as e:
            gml.structure_from_rows(rows, n, order, 0.5)
        assert e.value.code == GML_EHIP


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------
def handle_without_device(n=4, node_range=(0, 4)):
    """a Problem whose attributes are set by hand: what learn() checks before it calls the library needs no handle"""
    p = _lib.Problem.__new__(_lib.Problem)
    p._h, p.n, p.P, p.order = None, n, n, 2
    p.node0, p.node1 = node_range
    return p


def test_problem_learn_checks_the_structure_argument():
    p = handle_without_device(4, (1, 4))
    good = np.ones((3, 4), dtype=np.uint8)
    for bad in (np.ones((4, 4), dtype=np.uint8), np.ones((3, 5), dtype=np.uint8), np.ones(12, dtype=np.uint8),  # shape
                np.ones((3, 4), dtype=np.int64), np.ones((3, 4), dtype=np.float64), np.ones((3, 4), dtype=bool)):  # dtype
        with pytest.raises(gml.GMLError, match="structure is") as e:
            p.learn("RISE", 0.4, structure=bad)
        assert e.value.code == GML_EINVAL
    for other in (dict(terms=True), dict(matrix=True), dict(matrix=False)):
        with pytest.raises(gml.GMLError, match="cannot be combined") as e:
            p.learn("RISE", 0.4, structure=good, **other)
        assert e.value.code == GML_EINVAL
    with pytest.raises(gml.GMLError, match="x0 has shape"):  # x0 combines with structure, and is still checked
        p.learn("RISE", 0.4, structure=good, x0=np.zeros((4, 4)))
    with pytest.raises(gml.GMLError, match="unknown rule"):
        gml.structure_from_rows(np.zeros((4, 4)), 4, 2, 0.1, rule="median")
    with pytest.raises(gml.GMLError, match="rows of all 4 nodes"):
        gml.structure_from_rows(np.zeros((3, 4)), 4, 2, 0.1)
    with pytest.raises(gml.GMLError, match="numbered from 1"):
        gml.structure_from_keys([(0, 1)], 4, 2)


def test_front_door_argument_errors():
    hist = np.concatenate([np.ones((8, 1)), np.array(list(itertools.product([-1.0, 1.0], repeat=3)))], axis=1)
    S = np.ones((3, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="devices"):
        gml.learn(hist, gml.RISE(), gml.HIP(devices=[0, 1], structure=S))
    with pytest.raises(ValueError, match="refit"):
        gml.learn(hist, gml.RISE(), gml.HIP(refit=0.1, distributed=True))
    with pytest.raises(ValueError, match="refit"):
        gml.learn(hist, gml.RISE(), gml.HIP(refit=0.1, devices=[0, 1]))
    with pytest.raises(ValueError, match="refit"):
        gml.learn(hist, gml.RISE(), gml.HIP(refit=0.1, node_range=(0, 2)))
    with pytest.raises(ValueError, match="refit"):
        gml.learn(hist, gml.RISE(), gml.HIP(refit=-0.1))
    with pytest.raises(ValueError, match="refit_rule"):
        gml.learn(hist, gml.RISE(), gml.HIP(refit=0.1, refit_rule="median"))
    for bad in (np.ones((2, 3), dtype=np.uint8), np.ones((3, 3), dtype=np.int32), np.ones(9, dtype=np.uint8)):
        with pytest.raises(gml.GMLError, match="HIP: structure is") as e:
            gml.learn(hist, gml.RISE(), gml.HIP(structure=bad))
        assert e.value.code == GML_EINVAL


def test_hip_defaults_are_unchanged():
    m = gml.HIP()
    assert (m.structure, m.refit, m.refit_rule) == (None, None, None)
    assert (m.tol, m.precision, m.device, m.devices, m.max_iter, m.max_working, m.max_add, m.hess_samples, m.polish, m.verbose, m.distributed,
            m.node_range) == (1e-9, "auto", None, None, 100, 512, 64, 0, True, 0, False, None)
    assert gml.HIP(1e-8, "i8x") == gml.HIP(tol=1e-8, precision="i8x")  # the positional order of the existing fields stands
