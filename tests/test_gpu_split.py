"""gml_problem_fold_sizes / gml_problem_split on the device against the numpy model (tests/_split_reference.py): sign bits, counts,
K and M of both parts compared with `==` at every edge of the kernels' tiling; the empty part; independence from the source; and a
split handle against the packed handle of the same rows, bit for bit through learn and objgrad."""
import numpy as np
import pytest

import gml_amd as gml
import _split_reference as R

pytestmark = pytest.mark.gpu
_lib = gml._lib
synthetic = __import__("importlib").import_module("gml_amd.synthetic")

KS = [1, 31, 33, 64, 65, 513, 1500]  # a partial word, a partial wave, more than one 512-block of padding
NS = [1, 3, 33, 70]                  # (70 > 64: nothing key-based can stand in)
FOLDS = [2, 5, 64]
PATTERNS = ["ones", "threes", "mixed"]


def make_counts(pattern, K, rng):
    if pattern == "ones":
        return np.ones(K)
    if pattern == "threes":
        return np.full(K, 3.0)
    c = rng.integers(0, 4, size=K).astype(np.float64)  # zeros in the source, and ones and twos that a split empties
    c[rng.integers(0, K)] = 100000.0                   # one row whose units the lanes of a wave stride over
    return c


def check_part(src, S, c, nfolds, fold, seed, complement):
    rows, cn, bits, Kn = R.split(S, c, nfolds, fold, seed, complement)
    if Kn == 0:
        with pytest.raises(gml.GMLError) as e:
            src.split(nfolds, fold, seed=seed, complement=complement)
        assert e.value.code == _lib.GML_EINVAL and "fold" in str(e.value)
        return 0
    with src.split(nfolds, fold, seed=seed, complement=complement) as q:
        assert (q.K, q.n, q.M, q.order, q.node0, q.node1) == (Kn, src.n, cn.sum(), src.order, src.node0, src.node1)
        assert np.array_equal(q.counts(), cn)
        got = q.sign_bits()
        assert got.shape == bits.shape and np.array_equal(got, bits)  # (the bits of the rows >= K' are zero in both)
    return int(cn.sum())


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("K", KS)
def test_split_matches_the_numpy_model(K, n, pattern):
    rng = np.random.default_rng(1000 * K + 10 * n + len(pattern))
    S = rng.choice([-1, 1], size=(K, n)).astype(np.int8)
    c = make_counts(pattern, K, rng)
    seed = int(rng.integers(0, 2 ** 62))
    with gml.Problem(spins=S, counts=c) as src:
        for nfolds in FOLDS:
            sizes = src.fold_sizes(nfolds, seed=seed)
            assert sizes.dtype == np.int64 and np.array_equal(sizes, R.fold_sizes(c, nfolds, seed)) and sizes.sum() == c.sum()
            for fold in (0, nfolds - 1):
                held = check_part(src, S, c, nfolds, fold, seed, False)
                train = check_part(src, S, c, nfolds, fold, seed, True)
                assert held == sizes[fold] and held + train == c.sum()


def test_empty_part_is_einval():
    with gml.Problem(spins=np.array([[1]], dtype=np.int8), counts=np.ones(1)) as src:
        sizes = src.fold_sizes(2, seed=9)
        assert sorted(sizes.tolist()) == [0, 1]
        codes = []
        for fold in (0, 1):
            try:
                with src.split(2, fold, seed=9) as q:
                    assert (q.K, q.M) == (1, 1.0) and sizes[fold] == 1
                codes.append(0)
            except gml.GMLError as e:
                assert "fold %d" % fold in str(e) and sizes[fold] == 0
                codes.append(e.code)
        assert sorted(codes) == [0, _lib.GML_EINVAL]


def test_argument_errors():
    S = np.array([[1, -1], [-1, -1], [1, 1]], dtype=np.int8)
    with gml.Problem(spins=S, counts=np.array([2.0, 1.0, 4.0])) as src:
        for nfolds, fold in ((1, 0), (65, 0), (0, 0), (5, 5), (5, -1)):
            with pytest.raises(gml.GMLError) as e:
                src.split(nfolds, fold)
            assert e.value.code == _lib.GML_EINVAL
        for nfolds in (1, 65):
            with pytest.raises(gml.GMLError) as e:
                src.fold_sizes(nfolds)
            assert e.value.code == _lib.GML_EINVAL
        assert _lib.lib().gml_problem_split(src._h, 5, 0, 0, 0, None) == _lib.GML_EINVAL
        assert _lib.lib().gml_problem_fold_sizes(src._h, 5, 0, None) == _lib.GML_EINVAL
    with gml.Problem(spins=S, counts=np.array([2.0, 1.5, 4.0])) as frac:
        for call in (lambda: frac.split(2, 0), lambda: frac.fold_sizes(2)):
            with pytest.raises(gml.GMLError) as e:
                call()
            assert e.value.code == _lib.GML_EUNSUPPORTED
        with pytest.raises(gml.GMLError) as e:  # the argument checks come first
            frac.split(2, 2)
        assert e.value.code == _lib.GML_EINVAL
    with gml.Problem(spins=S, counts=np.array([2.0 ** 40, 1.0, 4.0])) as big:
        with pytest.raises(gml.GMLError) as e:
            big.split(2, 0)
        assert e.value.code == _lib.GML_EUNSUPPORTED


def test_split_handle_outlives_its_source():
    rng = np.random.default_rng(3)
    S = rng.choice([-1, 1], size=(700, 5)).astype(np.int8)
    c = rng.integers(1, 5, size=700).astype(np.float64)
    src = gml.Problem(spins=S, counts=c, node_range=(1, 4))
    q = src.split(3, 1, seed=5, complement=True)
    src.close()
    _lib.trim_cache()
    rows, cn, bits, Kn = R.split(S, c, 3, 1, 5, True)
    with q:
        assert (q.node0, q.node1) == (1, 4)
        assert np.array_equal(q.sign_bits(), bits) and np.array_equal(q.counts(), cn) and np.array_equal(q.spins(), S[rows])
        out, kkt, _ = q.learn("RISE", 0.3)
        assert out.shape == (3, 5) and kkt.max() < 1e-8


@pytest.fixture(scope="module")
def ising():
    spins, _ = synthetic.block_ising(n=16, K=3000, seed=2)
    return spins


@pytest.fixture(scope="module")
def ising_parts(ising):
    """both parts of fold 2 of 5 as (split handle, packed handle of the numpy model), open for the module"""
    S = ising
    K = S.shape[0]
    src = gml.Problem(spins=S)
    pairs = []
    for complement in (True, False):
        rows, cn, bits, Kn = R.split(S, np.ones(K), 5, 2, 77, complement)
        pairs.append((src.split(5, 2, seed=77, complement=complement), gml.Problem(packed=(bits, cn, Kn))))
    src.close()
    yield pairs
    for q, ref in pairs:
        q.close(), ref.close()


@pytest.mark.parametrize("form,c", [("RISE", 0.4), ("RPLE", 0.2)])
def test_split_handle_equals_packed_handle_learn(ising_parts, form, c):
    for q, ref in ising_parts:
        a, b = q.learn(form, c), ref.learn(form, c)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("form", ["RISE", "RPLE"])
def test_split_handle_equals_packed_handle_objgrad(ising_parts, form):
    """Same handle contents, same library calls: objective and gradient bit for bit.  (Operator calls under precision "auto" take
    the FP64-grade int8 pass, whose sums are all integers -- RPLE's objective included: two words per row, gml_kernels_i8w.hip.)"""
    n = ising_parts[0][0].n
    theta = np.random.default_rng(1).normal(scale=0.2, size=(n, n))
    for q, ref in ising_parts:
        fa, ga = q.objgrad(form, np.arange(n), theta)
        fb, gb = ref.objgrad(form, np.arange(n), theta)
        print(f"{form}: max |f - f'| = {np.abs(fa - fb).max():.3e}, max |g - g'| = {np.abs(ga - gb).max():.3e}")
        assert np.array_equal(ga, gb)
        assert np.array_equal(fa, fb)


def test_split_handle_equals_packed_handle_multibody():
    rng = np.random.default_rng(8)
    K, n = 2000, 8
    S = rng.choice([-1, 1], size=(K, n)).astype(np.int8)
    S[:, 3] = S[:, 0] * S[:, 1] * np.where(rng.random(K) < 0.8, 1, -1)  # a three-body term to find
    c = rng.integers(1, 4, size=K).astype(np.float64)
    rows, cn, bits, Kn = R.split(S, c, 4, 3, 21, True)
    with gml.Problem(spins=S, counts=c, order=3) as src:
        with src.split(4, 3, seed=21, complement=True) as q, gml.Problem(packed=(bits, cn, Kn), order=3) as ref:
            assert q.P == ref.P and q.order == 3
            a, b = q.learn("multiRISE", 0.4), ref.learn("multiRISE", 0.4)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            theta = rng.normal(scale=0.1, size=(n, q.P))
            fa, ga = q.objgrad("multiRISE", np.arange(n), theta)
            fb, gb = ref.objgrad("multiRISE", np.arange(n), theta)
            assert np.array_equal(fa, fb) and np.array_equal(ga, gb)
