"""Interaction orders 5 to 8 above the pass: the solver against the oracle's own solutions, the front door, the standard errors,
the term moments and the public Hessian-vector product, at the smallest shapes where a key of four to seven spins besides the
node's own exists.  (The pass itself, the layout and the bit images at these orders: test_gpu_f64_pass_exact.py,
test_gpu_i8_pass_exact.py, test_gpu_i8_pack_state.py; assembly and structure kernels: test_gpu_terms.py, test_gpu_structure.py.)

Samples for the solves are histograms over the 2^n states of a model with true terms of every size up to the order
(tests/_high_order_cases.py): 1e6 draws, so lambda = c sqrt(log(n^2 / 0.05) / M) is about 5.5e-4 at c = 0.2 and about half of a
node's parameters are non-zero at the optimum; c = 0 leaves every parameter non-zero.  (n, order) as the shapes of
tests/_f64_pass_reference.py: H5 (11, 5) P = 386, H6 (10, 6) P = 382, H8 (9, 8) P = 255, E7 (7, 8) P = 64 with all 128 states present,
E3 (3, 8) P = 4; H7 (12, 7) P = 1486 > 512 takes learn's matrix-free branch and has no oracle solve (a dense one at that P is too
slow): its rows are certified by the KKT residual of the oracle's gradient at c = 2 (lambda = 5.6e-3, a sparse optimum).
Tolerances are those of test_gpu_parity.test_multirise_order3_solutions_match_oracle_midsize and
test_gpu_fullsize._assert_solution_parity."""
import functools

import numpy as np
import pytest

import _high_order_cases as H
import _f64_pass_reference as F
import _sandwich_reference as SW
import gml_amd as gml
from oracle import oracle as O
from test_gpu_moments import ref_term_sums

pytestmark = pytest.mark.gpu
EXACT = ("f64", "i8w")
PRECS = ["f64", "i8w", "i8x"]


@functools.lru_cache(maxsize=None)
def data(name):
    spins, counts, terms = H.histogram(name)
    return spins, counts, terms, H.hist_array(spins, counts)


@functools.lru_cache(maxsize=None)
def oracle_rows(name, c):
    order = F.SHAPES[name][1]
    rows, kkt = O.learn_multi_rows(data(name)[3], c=c, order=order, tol=1e-11)
    assert kkt.max() <= 1e-10
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# the solver
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", [0.2, 0.0])
@pytest.mark.parametrize("name", ["H5", "H6", "H8", "E7", "E3"])
def test_learn_matches_the_oracle_solutions(name, c, prec):
    n, order = F.SHAPES[name][:2]
    spins, counts, terms, _ = data(name)
    ref = oracle_rows(name, c)
    if name == "E7":
        assert len(spins) == 128 and (counts > 0).all()  # every state present: at c = 0 the optimum is finite and unique
    if c == 0.0:
        assert (ref != 0).all()
    else:
        assert max(len(k) for k in terms) == min(order, n) and (ref != 0).any()
    with gml.Problem(spins=spins, counts=counts, order=order) as p:
        assert p.P == ref.shape[1]
        out, kkt, st = p.learn("RISE", c, tol=1e-10 if prec in EXACT else 1e-9, precision=prec, max_iter=200)
    fro = np.linalg.norm(out - ref) / np.linalg.norm(ref)
    mx = np.abs(out - ref).max() / np.abs(ref).max()
    print(f"{name} order {order}, c = {c}, {prec}: rel-Frobenius {fro:.2e}, max-abs / max {mx:.2e}, non-zeros per node "
          f"{(ref != 0).sum(1).mean():.1f} of {ref.shape[1]}, max kkt {kkt.max():.1e}")
    assert st["not_converged"] == 0
    assert fro <= 1e-6 and mx <= 1e-6
    if c > 0:
        assert ((out == 0) == (ref == 0)).all()  # the same exact-zero pattern
    # the true terms of the largest size are recovered in the rows of their members (a key of `order` spins, or of all n)
    top = max(terms, key=len)
    for u in top:
        j = O.multi_keys(n, order, u).index((u,) + tuple(i for i in top if i != u))
        assert abs(out[u, j] - terms[top]) <= 0.05, (top, u, out[u, j], terms[top])


@pytest.mark.parametrize("prec", PRECS)
def test_learn_matrix_free_order7_is_certified_by_the_oracle_gradient(prec):
    name, c = "H7", 2.0
    n, order = F.SHAPES[name][:2]
    spins, counts, terms, hist = data(name)
    lam = O.lam(c, n, counts.sum())
    with gml.Problem(spins=spins, counts=counts, order=order) as p:
        assert p.P == 1486 > 512
        out, kkt, st = p.learn("RISE", c, tol=1e-10 if prec in EXACT else 1e-9, precision=prec, max_iter=200)
    assert st["not_converged"] == 0
    worst = 0.0
    for u in range(n):
        keys = O.multi_keys(n, order, u)
        fld = next(j for j, k in enumerate(keys) if len(k) == 1)
        _, g = O.objgrad_multi(hist, order, u, out[u])
        worst = max(worst, O.kkt_residual(out[u], g, lam, fld))
    nnz = (out != 0).sum(axis=1)
    print(f"H7 order 7, c = {c}, {prec}: KKT residual by the oracle's gradient {worst:.2e}, non-zeros per node {nnz.min()} .. {nnz.max()} of {p.P}")
    assert worst <= 5e-9
    assert 1 <= nnz.min() and nnz.max() < 1486 // 2  # a sparse optimum that is not empty
    top = max(terms, key=len)  # the 7-spin terms are there
    for u in top:
        j = O.multi_keys(n, order, u).index((u,) + tuple(i for i in top if i != u))
        assert abs(out[u, j] - terms[top]) <= 0.1 and out[u, j] * terms[top] > 0  # (lambda = 5.6e-3 shrinks them a little)


@pytest.mark.parametrize("sym", [True, False])
@pytest.mark.parametrize("name", ["H8", "E3"])
def test_front_door_matches_the_oracle(name, sym):
    n, order = F.SHAPES[name][:2]
    hist = data(name)[3]
    for c in (0.2, 0.0):
        fg = gml.learn(hist, gml.multiRISE(c, sym, order), gml.HIP(tol=1e-11))
        rec, _ = O.learn_multi(hist, c=c, symmetrize=sym, order=order)
        assert set(fg.keys()) == set(rec.keys())
        assert max(abs(fg[k] - v) for k, v in rec.items()) <= 1e-8


# ---------------------------------------------------------------------------------------------------------------------------
# around the solve
# ---------------------------------------------------------------------------------------------------------------------------
def _iid(n, K, seed):
    rng = np.random.default_rng(seed)
    spins = (2 * rng.integers(0, 2, size=(K, n)) - 1).astype(np.int8)
    return rng, spins


@pytest.mark.parametrize("order,P_want", [(5, 163), (6, 219)])
def test_stderr_orders_five_and_six_with_mixed_kinds(order, P_want):
    """n = 9, orders 5 and 6 (P = 163, 219: keys of up to four and five spins besides the node's own), rows of the nodes 2 .. 5, every
    kind in every row, the last key (the largest) in every support"""
    n, K = 9, 2053
    rng, spins = _iid(n, K, 21)
    counts = rng.integers(0, 4, size=K).astype(np.float64)
    with gml.Problem(counts=counts, spins=spins, order=order, node_range=(2, 6)) as prob:
        P = prob.P
        assert P == P_want
        S = rng.choice(np.array([gml.EXCLUDED, gml.FREE, gml.PENALISED], dtype=np.uint8), p=[0.7, 0.1, 0.2], size=(4, P))
        x = rng.normal(scale=0.05, size=(4, P)) * (S != gml.EXCLUDED) * (rng.random((4, P)) < 0.7)
        S[1, 0] = gml.EXCLUDED  # row 1: no field
        x[1, 0] = 0.0
        S[:, P - 1] = gml.FREE  # the last key, of `order` spins, is in every support
        S[:, 1] = gml.FREE  # and so is a pair
        se, status = prob.stderr("RISE", x, structure=S)
        for r in range(4):
            keys = O.multi_keys(n, order, 2 + r)
            assert [tuple(int(v) for v in k if v >= 0) for k in prob.multi_keys_array(2 + r)] == keys
            sup = np.flatnonzero((S[r] == gml.FREE) | ((S[r] == gml.PENALISED) & (x[r] != 0)))
            assert len(sup) >= 20 and {len(keys[j]) for j in sup} >= set(range(2, order + 1))
            _, _, _, se0, cond = SW.sandwich("RISE", counts, spins, 2 + r, x[r], sup, keys=keys)
            assert cond <= 100.0 and status[r] == 0, (r, cond, status[r])
            assert np.abs(se[r, sup] - se0).max() <= 1e-9 * se0.max()
            assert np.count_nonzero(se[r]) == len(sup)
        assert se[1, 0] == 0.0


@pytest.mark.parametrize("weighted", [False, True])
def test_term_moments_of_five_to_eight_spins(weighted):
    n, K = 12, 3001
    rng, S = _iid(n, K, 23 + weighted)
    c = rng.integers(1, 1000, size=K).astype(np.float64) if weighted else np.ones(K)
    keys = [tuple(int(i) for i in rng.choice(n, size=q, replace=False)) for q in (5, 6, 7, 8) for _ in range(40)]
    keys += [(0, 1, 2, 3, 4, 5, 6, 7), (4, 5, 6, 7, 8, 9, 10, 11), (1, 3, 5, 7, 9, 3, 11), (2, 2, 4, 6, 8, 10, 0, 1), (7, 6, 5, 4, 3, 2, 1, 7)]
    want = ref_term_sums(S, c, keys)
    with gml.Problem(spins=S, counts=c if weighted else None) as p:
        got = p.term_moments([tuple(i + 1 for i in k) for k in keys], raw=True)
    assert np.array_equal(got, want)
    # (a spin named twice cancels: the seven-slot key with 3 twice is the five-spin term without it)
    assert want[-3] == ref_term_sums(S, c, [(1, 5, 7, 9, 11)])[0] and want[-3] != ref_term_sums(S, c, [(1, 3, 5, 7, 9, 11)])[0]


def _dense_hessian(form, counts, spins, keys, theta):
    """Hess f_u(theta) from the statistics of the keys in numpy float64"""
    s = spins.astype(np.float64)
    stat = np.stack([s[:, list(k)].prod(axis=1) for k in keys], axis=1)
    w = counts / counts.sum()
    E = stat @ theta
    if form == "RPLE":
        sg = 1.0 / (1.0 + np.exp(2.0 * E))
        return (stat * (4.0 * w * sg * (1.0 - sg))[:, None]).T @ stat
    e = w * np.exp(-E)
    Hm = (stat * e[:, None]).T @ stat
    if form == "logRISE":
        Z = e.sum()
        g = -(stat * e[:, None]).sum(0) / Z
        Hm = Hm / Z - np.outer(g, g)
    return Hm


@pytest.mark.parametrize("form", ["RISE", "logRISE", "RPLE"])
def test_hessvec_order_five_against_a_dense_numpy_hessian(form):
    """the GEMM form of the product (the sparse form declines keys of more than two other spins): n = 9, order 5, P = 163"""
    n, K, order = 9, 1531, 5
    rng, spins = _iid(n, K, 25)
    counts = 1.0 + (np.arange(K) % 4)
    nodes = np.array([0, 4, 8, 4, 3], dtype=np.int64)
    with gml.Problem(counts=counts, spins=spins, order=order) as p:
        P = p.P
        theta = rng.normal(scale=0.1, size=(len(nodes), P))
        vec = rng.normal(size=(len(nodes), P))
        want = np.stack([_dense_hessian(form, counts, spins, O.multi_keys(n, order, int(u)), theta[a]) @ vec[a] for a, u in enumerate(nodes)])
        scale = np.abs(want).max()
        hv64 = p.hessvec(form, nodes, theta, vec, precision="f64")
        hv8 = p.hessvec(form, nodes, theta, vec, precision="i8x")
    e64, e8 = np.abs(hv64 - want).max() / scale, np.abs(hv8 - want).max() / scale
    print(f"order 5 hessvec {form}: f64 {e64:.2e}, i8x {e8:.2e} of the largest entry")
    assert e64 <= 1e-12
    assert e8 <= 2e-7
