"""gml_problem_moments / gml_problem_term_moments without a GPU: the numpy reference against brute force and hand-computed values,
the symbols, the argument checks that need no device, and the Python key normalisation."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_csv

import gml_amd as gml
from _moments_reference import moments as ref_moments, split_histogram, term_sums as ref_term_sums

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")
_lib = gml._lib


@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(SO)
    L.gml_problem_moments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.gml_problem_term_moments.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
    L.gml_last_error.restype = C.c_char_p
    return L


def test_reference_against_brute_force():
    rng = np.random.default_rng(5)
    K, n = 7, 5
    S = rng.choice([-1, 1], size=(K, n))
    c = rng.integers(0, 1000, size=K)
    s1, s2 = ref_moments(S, c)
    for i in range(n):
        assert s1[i] == sum(int(c[k]) * int(S[k, i]) for k in range(K))
        for j in range(n):
            assert s2[i, j] == sum(int(c[k]) * int(S[k, i]) * int(S[k, j]) for k in range(K))
    keys = [(), (0,), (1, 3), (0, 2, 4), (0, 1, 2, 3, 4), (2, 2), (1, 3, 1), (4, -1, -1)]
    got = ref_term_sums(S, c, keys)
    for t, key in enumerate(keys):
        want = 0
        for k in range(K):
            v = int(c[k])
            for i in key:
                if i >= 0:
                    v *= int(S[k, i])
            want += v
        assert got[t] == want
    assert got[0] == c.sum() and got[5] == c.sum() and got[6] == s1[3] and got[7] == s1[4]


def test_reference_on_golden_a():
    # tests/golden/a_samples.csv, rows (count, s1, s2, s3):
    #   211725 ---, 77620 --+, 94788 +-+, 115717 -++, 95346 -+-, 211198 +++, 77625 ++-, 115981 +--
    S, c = split_histogram(load_csv("a_samples.csv"))
    s1, s2 = ref_moments(S, c)
    M = 211725 + 77620 + 94788 + 115717 + 95346 + 211198 + 77625 + 115981
    assert M == 1000000
    assert s1.tolist() == [-211725 - 77620 + 94788 - 115717 - 95346 + 211198 + 77625 + 115981,
                           -211725 - 77620 - 94788 + 115717 + 95346 + 211198 + 77625 - 115981,
                           -211725 + 77620 + 94788 + 115717 - 95346 + 211198 - 77625 - 115981]
    assert s1.tolist() == [-816, -228, -1354]
    s12 = 211725 + 77620 - 94788 - 115717 - 95346 + 211198 + 77625 - 115981
    s13 = 211725 - 77620 + 94788 - 115717 + 95346 + 211198 - 77625 - 115981
    s23 = 211725 - 77620 - 94788 + 115717 - 95346 + 211198 - 77625 + 115981
    assert s2.tolist() == [[M, s12, s13], [s12, M, s23], [s13, s23, M]]
    s123 = -211725 + 77620 - 94788 - 115717 + 95346 + 211198 - 77625 + 115981
    assert ref_term_sums(S, c, [(0, 1, 2), ()]).tolist() == [s123, M]


def test_reference_refuses_sums_beyond_2_53():
    with pytest.raises(AssertionError):
        ref_moments(np.ones((2, 1)), np.array([2.0 ** 52, 2.0 ** 52]))
    with pytest.raises(AssertionError):
        ref_moments(np.ones((2, 1)), np.array([1.5, 1.0]))


def test_declared_and_exported(cdll):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gml.h")).read(), flags=re.S)
    for name in ("gml_problem_moments", "gml_problem_term_moments"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(cdll, name), name
    assert "#define GML_ABI_VERSION 6" in text


def test_null_arguments_are_einval_without_a_gpu(cdll):
    buf = np.zeros(4, dtype=np.int64)
    keys = np.zeros((1, 2), dtype=np.int32)
    pb, pk = buf.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p)
    assert cdll.gml_problem_moments(None, pb, None) == _lib.GML_EINVAL
    assert b"NULL" in cdll.gml_last_error()
    assert cdll.gml_problem_term_moments(None, pk, 2, 1, pb) == _lib.GML_EINVAL
    assert cdll.gml_problem_term_moments(None, None, 2, 1, pb) == _lib.GML_EINVAL


def test_key_windows_from_dict_list_and_factor_graph():
    want = np.array([[0, 1, -1], [2, -1, -1], [3, 3, 0], [-1, -1, -1]], dtype=np.int32)
    as_dict = {(1, 2): 0.5, (3,): 0.1, (4, 4, 1): -1.0, (): 2.0}
    for terms in (as_dict, list(as_dict), gml.FactorGraph(3, 4, "spin", {(1, 2): 0.5, (3,): 0.1, (1, 2, 4): 1.0})):
        (keys,) = list(_lib.moment_key_windows(terms))
        assert keys.dtype == np.int32 and keys.flags.c_contiguous
        if isinstance(terms, gml.FactorGraph):
            assert keys.tolist() == [[0, 1, -1], [2, -1, -1], [0, 1, 3]]
        else:
            assert np.array_equal(keys, want)
    (keys,) = list(_lib.moment_key_windows([()]))  # the empty key alone: one unused slot
    assert keys.tolist() == [[-1]]
    assert list(_lib.moment_key_windows([])) == []
    with pytest.raises(gml.GMLError):
        list(_lib.moment_key_windows([(0, 1)]))


def test_key_windows_of_a_term_array():
    n, order = 6, 3
    count = _lib.terms_count(n, order, True)
    ta = gml.factor_graph.TermArray(n, order, True, np.zeros(count))
    wins = list(_lib.moment_key_windows(ta, chunk=16))
    assert [len(w) for w in wins] == [16] * (count // 16) + ([count % 16] if count % 16 else [])
    keys = np.concatenate(wins)
    want = [k for q in range(1, order + 1) for k in itertools.combinations(range(n), q)]
    assert [tuple(int(v) for v in row if v >= 0) for row in keys] == want
    assert keys.min() == -1 and keys.dtype == np.int32
