"""Annealed importance sampling on the device (gml_log_partition_ais / log_partition / log_likelihood): log weights, energies and
final states bit for bit against the numpy restatement; independent of chain tile, term order and chain count; one step is the plain
term chain of k_term_chains; the host summary; and the front door against enumeration on a model with two wells."""
import ctypes as C

import numpy as np
import pytest

import gml_amd as gml
from gml_amd import _lib
from _high_order_cases import wide_terms
from _ais_reference import ais, exact_log_z, lattice, sparse_model, summary
from _tempered_reference import bimodal_16

pytestmark = pytest.mark.gpu

SCHEDULE = [0.0, 0.1, 0.3, 0.2, 0.2, 0.5, 0.9, 0.7]  # 7 steps: not monotone, one value repeated, the last beta is 0.7


def run(terms, n, chains, betas, sps, seed):
    """(result, log_weights, energies, spins) of the C entry point"""
    return _lib.log_partition_ais(terms, n, chains, betas, sps, seed=seed, return_states=True)


def order4_with_cancellations(n, seed):
    rng = np.random.default_rng(seed)
    terms = sparse_model(n, 3, 2, 0.25, seed, order=4)
    for _ in range(n // 2):  # keys naming a spin twice: (i, i, j, k) is the pair (j, k), (i, i, j) the field of j
        i, j, k = (int(v) for v in rng.choice(n, 3, replace=False) + 1)
        terms[(i, i, j, k)] = float(rng.normal(scale=0.3))
        terms[(i, j, i)] = float(rng.normal(scale=0.3))
    return terms


def two_8_spin_terms():
    terms = sparse_model(20, 3, 2, 0.3, 5)
    terms[(1, 3, 5, 7, 9, 11, 13, 15)] = 0.6
    terms[(20, 2, 18, 4, 16, 6, 14, 9)] = -0.45
    return terms


# the five models of the tempered tests, and one whose terms reach the kernel's largest arity
CASES = {
    "lattice_16x16": lambda: (lattice(16, 0.4, 0.2, 1), 256),
    "order3_n40": lambda: (sparse_model(40, 6, 3, 0.3, 2), 40),
    "order4_cancelled_n30": lambda: (order4_with_cancellations(30, 3), 30),
    "n1": lambda: ({(1,): 0.3}, 1),
    "n33": lambda: (sparse_model(33, 6, 4, 0.3, 4), 33),
    "two_8_spin_terms_n20": lambda: (two_8_spin_terms(), 20),
    "orders_5_to_8_cancelled_n12": lambda: (wide_terms(12, 5), 12),  # terms of 5 to 8 spins, some through keys that name a spin twice
}


def assert_same(got, ref):
    _, logw, en, spins = got
    assert np.array_equal(spins, ref[2])
    assert np.array_equal(en, ref[1]), np.abs(en - ref[1]).max()
    assert np.array_equal(logw, ref[0]), np.abs(logw - ref[0]).max()


@pytest.mark.parametrize("sps", [1, 3])
@pytest.mark.parametrize("case", sorted(CASES))
def test_bit_for_bit_against_the_restatement(case, sps):
    terms, n = CASES[case]()
    chains = 2003  # the last tile and the last wave are partly empty
    got = run(terms, n, chains, SCHEDULE, sps, seed=11)
    assert_same(got, ais(terms, n, chains, SCHEDULE, sps, seed=11))
    assert got[1].shape == (chains,) and got[3].shape == (chains, n) and set(np.unique(got[3])) <= {-1, 1}


def test_bit_for_bit_large_sparse():
    n = 4096
    terms = sparse_model(n, 4, 2, 0.3, n)
    assert_same(run(terms, n, 130, [0.0, 0.4, 1.0], 1, seed=5), ais(terms, n, 130, [0.0, 0.4, 1.0], 1, seed=5))


def test_every_chain_tile_gives_the_same_bits():
    L = _lib.lib()
    L.gml_test_term_chains_tile.argtypes = [C.c_int]
    L.gml_test_term_chains_tile.restype = C.c_int
    terms = sparse_model(300, 6, 3, 0.3, 8)
    got = {}
    try:
        for T in (64, 128, 256):
            assert L.gml_test_term_chains_tile(T) in (0, 64, 128, 256)
            got[T] = run(terms, 300, 2003, SCHEDULE, 2, seed=3)
    finally:
        L.gml_test_term_chains_tile(0)
    free = run(terms, 300, 2003, SCHEDULE, 2, seed=3)
    for other in (got[128], got[256], free):
        assert all(np.array_equal(a, b) for a, b in zip(got[64], other))
    assert np.unique(got[64][1]).size > 1000  # (the weights are not trivially equal)


def test_independent_of_chain_count_seed_and_term_order():
    terms = sparse_model(70, 6, 3, 0.3, 7)
    a = run(terms, 70, 700, SCHEDULE, 2, seed=17)
    b = run(terms, 70, 150, SCHEDULE, 2, seed=17)
    assert all(np.array_equal(x[:150], y) for x, y in zip(a[1:], b[1:]))
    other = run(terms, 70, 150, SCHEDULE, 2, seed=18)
    assert not np.array_equal(other[3], b[3]) and not np.array_equal(other[1], b[1])
    # the same model with its terms shuffled (one field term per spin: a_i is an ordered FP64 sum) gives the same bits
    items = list(terms.items())
    perm = np.random.default_rng(1).permutation(len(items))
    d = run(dict(items[t] for t in perm), 70, 150, SCHEDULE, 2, seed=17)
    assert all(np.array_equal(x, y) for x, y in zip(b, d))


@pytest.mark.parametrize("k", [1, 12])
def test_one_step_is_the_term_chain_kernel(k):
    terms = sparse_model(70, 6, 3, 0.3, 7)
    with gml.Problem(terms=terms, n=70, num_samples=1100, mcmc_sweeps=k, mcmc_samples_per_chain=1, seed=17, order=3) as p:
        plain = p.spins()
    assert np.array_equal(run(terms, 70, 1100, [0.0, 1.0], k, seed=17)[3], plain)


def test_result_is_the_summary_of_the_log_weights():
    terms, n = CASES["order3_n40"]()
    for chains in (2003, 1):
        result, logw, _, _ = run(terms, n, chains, np.linspace(0.0, 1.0, 21), 1, seed=2)
        ref = summary(logw, n)
        assert np.allclose(result, ref, rtol=1e-12, atol=0.0), (result, ref)
    assert result[1] == 0.0 and result[2] == 1.0  # one chain
    result, logw, en, _ = run({(1, 2): 0.0, (2, 3, 4): 0.0, (5,): 0.0}, 5, 64, np.linspace(0.0, 1.0, 11), 1, seed=2)
    assert np.all(logw == 0.0) and np.all(en == 0.0) and result.tolist() == [5 * np.log(2.0), 0.0, 64.0]


@pytest.fixture(scope="module")
def bimodal():
    """the model with two wells, its exact log Z, and the restatement at the front-door test's shape"""
    terms = bimodal_16()
    logw, _, _ = ais(terms, 16, 4096, np.linspace(0.0, 1.0, 301), 1, seed=1)
    return terms, exact_log_z(terms, 16), logw, summary(logw, 16)


def test_front_door_against_enumeration(bimodal):
    terms, exact, ref_logw, (ref_log_z, ref_se, _) = bimodal
    est = gml.log_partition(terms, gml.AIS(4096, 300), seed=1)
    print(f"log Z = {est.log_z:.6f} +- {est.stderr:.4f} (ess {est.ess:.0f}); exact {exact:.6f}; the restatement's {ref_log_z:.6f} +- {ref_se:.4f}")
    assert abs(est.log_z - exact) < 5 * ref_se
    assert np.array_equal(est.log_weights, ref_logw) and est.energies is None and est.spins is None
    fg = gml.FactorGraph(3, 16, "spin", dict(terms))
    again = gml.log_partition(fg, gml.AIS(4096, 300), seed=1, return_states=True)
    assert again.log_z == est.log_z and again.spins.shape == (4096, 16) and again.energies.shape == (4096,)
    # a pairwise model as a matrix (fields on the diagonal) and as its term list
    pair = lattice(4, 0.4, 0.2, 1)
    small = gml.AIS(500, 20)
    assert gml.log_partition(gml.FactorGraph(pair).to_matrix(), small, seed=2).log_z == gml.log_partition(pair, small, seed=2).log_z


def test_log_likelihood(bimodal):
    terms, exact, _, _ = bimodal
    hist = gml.sample(terms, 20000, seed=3)  # exact draws
    method = gml.AIS(4096, 300)
    ll = gml.log_likelihood(hist, terms, method, seed=1)
    rows = hist[:, 1:].astype(np.float64)
    data = sum(w * float(np.dot(hist[:, 0], np.prod(rows[:, [i - 1 for i in k]], axis=1))) for k, w in terms.items()) / 20000
    assert abs(ll.data_term - data) <= 1e-12 * abs(data), (ll.data_term, data)
    assert ll.mean == ll.data_term - ll.log_z and ll.total == 20000 * ll.mean
    est = gml.log_partition(terms, method, seed=1)
    assert (ll.log_z, ll.stderr) == (est.log_z, est.stderr)
    # the model the data came from explains them better than the same model without its couplings
    flat = {k: (w if len(k) == 1 else 0.0) for k, w in terms.items()}
    ll0 = gml.log_likelihood(hist, flat, method, seed=1)
    print(f"log-likelihood per sample: true model {ll.mean:.4f} (log Z {ll.log_z:.4f} +- {ll.stderr:.4f}), couplings zeroed {ll0.mean:.4f} "
          f"(log Z {ll0.log_z:.4f} +- {ll0.stderr:.4f}); exact log Z {exact:.4f}")
    assert ll.mean - ll0.mean > 10 * np.hypot(ll.stderr, ll0.stderr)
    # a Problem, and an estimate reused across data sets
    with gml.Problem(hist, order=3) as p:
        reused = gml.log_likelihood(p, terms, log_z=est)
        assert reused == ll
        parts = []
        for complement in (False, True):  # a held-out fold and its training part share the estimate; their totals add up
            with p.split(5, 0, seed=1, complement=complement) as q:
                parts.append(gml.log_likelihood(q, terms, log_z=est))
                assert parts[-1].log_z == est.log_z and parts[-1].total == q.M * parts[-1].mean
    assert abs(parts[0].total + parts[1].total - ll.total) <= 1e-9 * abs(ll.total)
    plain = gml.log_likelihood(hist, terms, log_z=exact)
    assert plain.log_z == exact and np.isnan(plain.stderr) and plain.data_term == ll.data_term


def test_device_memory_returns():
    import torch
    terms = sparse_model(300, 6, 3, 0.3, 8)
    run(terms, 300, 70000, [0.0, 0.5, 1.0], 1, seed=1)
    torch.cuda.synchronize()
    _lib.trim_cache()
    free0 = torch.cuda.mem_get_info()[0]
    first = run(terms, 300, 70000, [0.0, 0.5, 1.0], 1, seed=1)
    for _ in range(19):
        again = run(terms, 300, 70000, [0.0, 0.5, 1.0], 1, seed=1)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    _lib.trim_cache()
    free1 = torch.cuda.mem_get_info()[0]
    print("free bytes before / after:", free0, free1)
    assert free1 == free0
