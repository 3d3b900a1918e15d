"""Replica-exchange chains of any term list (gml_problem_create_mcmc_terms_tempered / TemperedTermChains): samples and swap counts
bit for bit against the numpy restatement, one rung at beta = 1 against GlauberTermChains, independent of ladder count, chain tile
and term order, and the right distribution on a model with two wells where the plain chains stay in the well they started in."""
import ctypes as C
import time

import numpy as np
import pytest

import gml_amd as gml
from gml_amd import _lib
from _high_order_cases import wide_terms
from _tempered_reference import bimodal_16, exact_moments, tempered

pytestmark = pytest.mark.gpu


def run(terms, n, ladders, spc, burn_in, thin, betas, swap_every, seed, histogram=False, order=None):
    order = max(2, max(len(k) for k in terms)) if order is None else order  # (the handle's order is the learner's, not the sampler's)
    N = ladders * spc
    with gml.Problem(terms=terms, n=n, num_samples=N, mcmc_sweeps=burn_in, mcmc_thin=thin, mcmc_samples_per_chain=spc,
                     mcmc_betas=betas, mcmc_swap_every=swap_every, seed=seed, order=order, histogram=histogram) as p:
        assert p.swap_counts.shape == (2, len(betas) - 1) and p.swap_counts.dtype == np.int64
        if not histogram:
            assert (p.K, p.n, p.M) == (N, n, float(N))
            return p.spins(), p.swap_counts
        return p.spins(), p.counts(), p.M


def ladder(R, beta_min=0.1):
    return gml.TemperedTermChains(replicas=R, beta_min=beta_min).betas


# the models of CASES in test_gpu_term_chains.py
def lattice(L, J, h, seed):
    rng = np.random.default_rng(seed)
    idx = lambda x, y: (x % L) * L + (y % L) + 1  # noqa: E731
    terms = {}
    for x in range(L):
        for y in range(L):
            terms[(idx(x, y), idx(x + 1, y))] = J * rng.choice([-1.0, 1.0])
            terms[(idx(x, y), idx(x, y + 1))] = J * rng.choice([-1.0, 1.0])
    for i in range(L * L):
        terms[(i + 1,)] = rng.normal(scale=h)
    return terms


def sparse_model(n, n3, n2, scale, seed, order=3, fields=True):
    """about n3 order-`order` and n2 pairwise terms per spin, random spins, N(0, scale^2) weights"""
    rng = np.random.default_rng(seed)
    terms = {}
    for _ in range(n * n3 // order):
        terms[tuple(int(v) for v in rng.choice(n, order, replace=False) + 1)] = float(rng.normal(scale=scale))
    for _ in range(n * n2 // 2):
        terms[tuple(int(v) for v in rng.choice(n, 2, replace=False) + 1)] = float(rng.normal(scale=scale))
    if fields:
        for i in range(n):
            terms[(i + 1,)] = float(rng.normal(scale=0.2))
    return terms


def order4_with_cancellations(n, seed):
    rng = np.random.default_rng(seed)
    terms = sparse_model(n, 3, 2, 0.25, seed, order=4)
    for _ in range(n // 2):  # keys naming a spin twice: (i, i, j, k) is the pair (j, k), (i, i, j) the field of j
        i, j, k = (int(v) for v in rng.choice(n, 3, replace=False) + 1)
        terms[(i, i, j, k)] = float(rng.normal(scale=0.3))
        terms[(i, j, i)] = float(rng.normal(scale=0.3))
    return terms


CASES = {
    "lattice_16x16": lambda: (lattice(16, 0.4, 0.2, 1), 256),
    "order3_n40": lambda: (sparse_model(40, 6, 3, 0.3, 2), 40),
    "order4_cancelled_n30": lambda: (order4_with_cancellations(30, 3), 30),
    "n1": lambda: ({(1,): 0.3}, 1),
    "n33": lambda: (sparse_model(33, 6, 4, 0.3, 4), 33),
    # terms of 5 to 8 spins, some through keys that name a spin twice; the handle is one of order 8 (n = 12: 3301 statistics columns)
    "orders_5_to_8_cancelled_n12": lambda: (wide_terms(12, 5), 12),
}
LADDERS = {2: 1001, 8: 251, 64: 37}  # about 2000 lanes; the last tile is partly empty (at R = 64 only for tiles above 64 lanes)


@pytest.mark.parametrize("swap_every", [1, 3])
@pytest.mark.parametrize("R", [2, 8, 64])
@pytest.mark.parametrize("case", sorted(CASES))
def test_bit_for_bit_against_the_restatement(case, R, swap_every):
    terms, n = CASES[case]()
    got, counts = run(terms, n, LADDERS[R], 3, 5, 2, ladder(R), swap_every, seed=11)
    ref, ref_counts = tempered(terms, n, LADDERS[R], 3, 5, 2, ladder(R), swap_every, seed=11)
    assert np.array_equal(counts, ref_counts), (counts, ref_counts)
    assert np.array_equal(got, ref)


def test_bit_for_bit_large_sparse():
    n, R, ladders = 4096, 8, 9
    terms = sparse_model(n, 4, 2, 0.3, n)
    got, counts = run(terms, n, ladders, 2, 2, 2, ladder(R, 0.5), 1, seed=5, order=2)  # (order 2: see test_gpu_term_chains.py)
    ref, ref_counts = tempered(terms, n, ladders, 2, 2, 2, ladder(R, 0.5), 1, seed=5)
    assert np.array_equal(counts, ref_counts), (counts, ref_counts)
    assert np.array_equal(got, ref)


def test_one_rung_at_beta_one_is_glauber_term_chains():
    terms = sparse_model(70, 6, 3, 0.3, 7)
    with gml.Problem(terms=terms, n=70, num_samples=3 * 1100, mcmc_sweeps=12, mcmc_thin=3, mcmc_samples_per_chain=3, seed=17, order=3) as p:
        plain = p.spins()
        assert p.swap_counts is None
    got, counts = run(terms, 70, 1100, 3, 12, 3, [1.0], 1, seed=17)
    assert counts.shape == (2, 0)
    assert np.array_equal(got, plain)


def test_independent_of_ladder_count_seed_and_term_order():
    terms = sparse_model(70, 6, 3, 0.3, 7)
    betas = ladder(8)
    a, _ = run(terms, 70, 700, 1, 12, 1, betas, 1, seed=17)
    b, cb = run(terms, 70, 150, 1, 12, 1, betas, 1, seed=17)
    assert np.array_equal(a[:150], b)
    assert not np.array_equal(run(terms, 70, 150, 1, 12, 1, betas, 1, seed=18)[0], b)
    c, cc = run(terms, 70, 150, 4, 12, 3, betas, 2, seed=17)
    # the same model with its terms shuffled (one field term per spin: a_i is an ordered FP64 sum) gives the same bits
    items = list(terms.items())
    perm = np.random.default_rng(1).permutation(len(items))
    d, cd = run(dict(items[t] for t in perm), 70, 150, 4, 12, 3, betas, 2, seed=17)
    assert np.array_equal(c, d) and np.array_equal(cc, cd)


def test_every_chain_tile_gives_the_same_bits():
    L = _lib.lib()
    L.gml_test_term_chains_tile.argtypes = [C.c_int]
    L.gml_test_term_chains_tile.restype = C.c_int
    terms = sparse_model(300, 6, 3, 0.3, 8)
    betas = ladder(16)
    got = {}
    try:
        for T in (64, 128, 256):
            assert L.gml_test_term_chains_tile(T) in (0, 64, 128, 256)
            got[T] = run(terms, 300, 139, 3, 4, 2, betas, 1, seed=3)
    finally:
        L.gml_test_term_chains_tile(0)
    free = run(terms, 300, 139, 3, 4, 2, betas, 1, seed=3)
    for other in (got[128], got[256], free):
        assert np.array_equal(got[64][0], other[0]) and np.array_equal(got[64][1], other[1])
    assert got[64][1][0].min() > 0


def test_whole_ladder_per_wave_with_empty_ladders_in_the_last_tile():
    # R = 64: a ladder is a whole wave, so only a forced tile of 128 or 256 lanes leaves waves of ladders that do not exist
    L = _lib.lib()
    L.gml_test_term_chains_tile.argtypes = [C.c_int]
    L.gml_test_term_chains_tile.restype = C.c_int
    terms = sparse_model(40, 6, 3, 0.3, 2)
    ref, ref_counts = tempered(terms, 40, 37, 3, 5, 2, ladder(64), 1, seed=11)
    try:
        for T in (128, 256):
            L.gml_test_term_chains_tile(T)
            got, counts = run(terms, 40, 37, 3, 5, 2, ladder(64), 1, seed=11)
            assert np.array_equal(counts, ref_counts), (T, counts, ref_counts)
            assert np.array_equal(got, ref)
    finally:
        L.gml_test_term_chains_tile(0)


def test_no_swap_round_gives_no_rate():
    import warnings
    terms = sparse_model(20, 6, 3, 0.3, 9)
    sampler = gml.TemperedTermChains(burn_in=4, thin=1, samples_per_chain=1, replicas=4, swap_every=5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        gml.sample(terms, 100, sampler=sampler, seed=0)
    assert sampler.swap_rates.shape == (3,) and np.isnan(sampler.swap_rates).all()


def test_equal_betas_accept_every_attempt():
    terms = sparse_model(40, 6, 3, 0.3, 2)
    ladders, sweeps = 300, 9
    _, counts = run(terms, 40, ladders, 1, sweeps, 1, [0.8] * 8, 1, seed=4)
    assert np.array_equal(counts[0], counts[1])
    assert counts[0].tolist() == [ladders * ((sweeps + 1) // 2 if r % 2 == 0 else sweeps // 2) for r in range(7)]


def test_histogram_flag():
    terms = sparse_model(20, 6, 3, 0.3, 9)
    betas = ladder(4, 0.3)
    spins, counts0 = run(terms, 20, 10000, 3, 20, 2, betas, 1, seed=4)
    states, counts, M = run(terms, 20, 10000, 3, 20, 2, betas, 1, seed=4, histogram=True)
    assert M == 30000.0 and counts.sum() == 30000
    u, c = np.unique(spins, axis=0, return_counts=True)
    order = np.lexsort(states.T[::-1])
    assert np.array_equal(states[order], u) and np.array_equal(np.rint(counts[order]).astype(int), c)
    with pytest.raises(gml.GMLError, match="n <= 64"):
        run(sparse_model(70, 3, 2, 0.3, 1), 70, 100, 1, 2, 1, betas, 1, seed=0, histogram=True)


def moments_of(hist, N):
    s = hist[:, 1:].astype(float)
    w = hist[:, 0] / N
    return w @ s, (s * w[:, None]).T @ s


def test_distribution_two_wells_against_the_plain_chains():
    terms = bimodal_16()
    ppos, mag0, corr0 = exact_moments(terms, 16)
    assert abs(ppos - 0.893) < 1e-3 and np.abs(mag0 - 0.786).max() < 0.02, (ppos, mag0)
    N = 16384
    sampler = gml.TemperedTermChains(burn_in=300, thin=1, samples_per_chain=1, replicas=8, beta_min=0.1)
    t0 = time.perf_counter()
    hist = gml.sample(terms, N, sampler=sampler, seed=1)
    wall = time.perf_counter() - t0
    assert hist[:, 0].sum() == N
    mag, corr = moments_of(hist, N)
    bound = 6 / np.sqrt(N)  # a +-1 product has variance at most 1: six standard deviations at the least
    err_m, err_c = np.abs(mag - mag0).max(), np.abs(corr - corr0).max()
    print(f"tempered, {N} ladders of 8: max error of a magnetisation {err_m:.4f}, of a pair correlation {err_c:.4f} (bound {bound:.4f}); "
          f"swap rates {np.round(sampler.swap_rates, 3).tolist()}; sample() took {wall:.3f} s")
    assert err_m < bound and err_c < bound
    assert sampler.swap_rates.shape == (7,) and (sampler.swap_rates > 0).all() and (sampler.swap_rates < 1).all()
    # the control: the single-temperature chains stay in the well they started in, half of them in the wrong one
    plain = gml.sample(terms, N, sampler=gml.GlauberTermChains(burn_in=300, thin=1, samples_per_chain=1), seed=1)
    miss = np.abs(moments_of(plain, N)[0] - mag0).max()
    print(f"plain Glauber chains, same model and sweeps: max error of a magnetisation {miss:.4f}")
    assert miss > 0.3


def test_distribution_two_wells_thinned():
    terms = bimodal_16()
    _, mag0, corr0 = exact_moments(terms, 16)
    ladders = 4096
    sampler = gml.TemperedTermChains(burn_in=300, thin=25, samples_per_chain=4, replicas=8, beta_min=0.1)
    hist = gml.sample(terms, 4 * ladders, sampler=sampler, seed=2)
    mag, corr = moments_of(hist, 4 * ladders)
    bound = 6 / np.sqrt(ladders)  # 4 correlated samples per ladder: the effective sample size is at least the ladder count
    err_m, err_c = np.abs(mag - mag0).max(), np.abs(corr - corr0).max()
    print(f"tempered, {ladders} ladders x 4 samples: max error of a magnetisation {err_m:.4f}, of a pair correlation {err_c:.4f} "
          f"(bound {bound:.4f})")
    assert err_m < bound and err_c < bound
