"""gml_problem_fold_sizes / gml_problem_split without a GPU: the numpy model of the split (tests/_split_reference.py) against its
own definition, the symbols, the header, and the argument checks that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import gml_amd as gml
import _split_reference as R
from _mcmc_chains_reference import u01

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")
_lib = gml._lib


@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(SO)
    L.gml_problem_fold_sizes.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p]
    L.gml_problem_split.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_void_p]
    L.gml_last_error.restype = C.c_char_p
    return L


def random_case(seed, K=40, n=7):
    rng = np.random.default_rng(seed)
    S = rng.choice([-1, 1], size=(K, n)).astype(np.int8)
    c = rng.integers(0, 9, size=K).astype(np.float64)
    c[3] = 500
    return S, c


def test_unit_definition_by_hand():
    # the definition, unit by unit, in Python integers and floats
    seed, nfolds = 12345, 5
    lab = R.unit_folds(200, nfolds, seed)
    for g in range(200):
        z = (seed + 0x9E3779B97F4A7C15 * (g + 1) + 0xD1B54A32D192ED03 * (R.FOLD_STREAM + 1)) % 2 ** 64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
        z ^= z >> 31
        u = (z >> 11) / 9007199254740992.0
        assert lab[g] == min(nfolds - 1, int(nfolds * u))
    assert R.FOLD_STREAM == 0x8000000000000000


def test_fold_stream_is_not_a_sampler_stream():
    # the samplers count streams up from 0: the same (seed, counter) gives other draws there
    k = np.arange(1000, dtype=np.uint64)
    for stream in (0, 1, 2, 1000):
        assert not np.any(u01(7, stream, k) == u01(7, R.FOLD_STREAM, k))


@pytest.mark.parametrize("nfolds", [2, 5, 64])
def test_parts_partition_the_source(nfolds):
    S, c = random_case(1)
    sizes = R.fold_sizes(c, nfolds, seed=3)
    assert sizes.sum() == c.sum() and len(sizes) == nfolds
    for fold in (0, nfolds - 1):
        held = R.new_counts(c, nfolds, fold, 3, False)
        train = R.new_counts(c, nfolds, fold, 3, True)
        assert np.array_equal(held + train, c.astype(np.int64))
        assert held.sum() == sizes[fold]
        rows, cn, bits, Kn = R.split(S, c, nfolds, fold, 3, True)
        assert Kn == len(rows) == np.count_nonzero(train) and np.array_equal(cn, train[rows])
        assert np.array_equal(R.unpack_bits(bits, Kn), S[rows])
        assert bits.shape == (S.shape[1], (Kn + 1023) // 1024 * 32)


def test_same_seed_same_split_other_seed_other_split():
    S, c = random_case(2)
    a = R.new_counts(c, 5, 1, 11, False)
    assert np.array_equal(a, R.new_counts(c, 5, 1, 11, False))
    assert not np.array_equal(a, R.new_counts(c, 5, 1, 12, False))


def test_fold_never_reaches_nfolds():
    # u01 < 1, and the min() covers nfolds * u rounding up to nfolds: the largest u01 value there is
    umax = (2 ** 53 - 1) / 2 ** 53
    for nfolds in range(2, 65):
        assert min(nfolds - 1, int(np.floor(nfolds * umax))) == nfolds - 1
    for seed in (0, 1, 2 ** 63, 2 ** 64 - 1):
        for nfolds in (2, 3, 64):
            lab = R.unit_folds(20000, nfolds, seed)
            assert lab.min() >= 0 and lab.max() == nfolds - 1
    assert u01(5, R.FOLD_STREAM, np.arange(100000, dtype=np.uint64)).max() < 1.0


def test_pack_roundtrip_and_zero_padding():
    rng = np.random.default_rng(4)
    for K in (1, 31, 33, 1025):
        S = rng.choice([-1, 1], size=(K, 3)).astype(np.int8)
        bits = R.pack_bits(S)
        assert np.array_equal(R.unpack_bits(bits, K), S)
        full = ((bits[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(3, -1)
        assert not full[:, K:].any()


def test_declared_and_exported(cdll):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gml.h")).read(), flags=re.S)
    for name in ("gml_problem_fold_sizes", "gml_problem_split"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(cdll, name), name
    assert "#define GML_ABI_VERSION 6" in text
    assert _lib.GML_ABI_VERSION == 6
    rng_h = open(os.path.join(ROOT, "graphicalmodellearning.jl_amd", "csrc", "gml_rng.h")).read()
    assert re.search(r"kU01FoldStream\s*=\s*0x8000000000000000ull", rng_h)


def test_null_arguments_are_einval_without_a_gpu(cdll):
    sizes = np.zeros(64, dtype=np.int64)
    out = C.c_void_p()
    assert cdll.gml_problem_fold_sizes(None, 5, 0, sizes.ctypes.data_as(C.c_void_p)) == _lib.GML_EINVAL
    assert b"NULL" in cdll.gml_last_error()
    assert cdll.gml_problem_split(None, 5, 0, 0, 0, C.byref(out)) == _lib.GML_EINVAL
    assert b"NULL" in cdll.gml_last_error()
    assert out.value is None


def test_python_surface():
    assert callable(gml.Problem.split) and callable(gml.Problem.fold_sizes) and callable(gml.Problem._from_handle)
    assert gml.learn_path is gml.path.learn_path and "learn_path" in gml.__all__ and "PathResult" in gml.__all__
