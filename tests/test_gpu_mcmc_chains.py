"""Glauber chains of dense pairwise models on the int8 matrix cores (gml_problem_create_mcmc_chains / GlauberChains): bit for
bit against the numpy restatement, the same chain as the term-list kernel, independent of the chain tile, the right
distribution, and learn -> sample -> re-learn at a size exact enumeration cannot reach."""
import numpy as np
import pytest

import gml_amd as gml
from _mcmc_chains_reference import chains as ref_chains

pytestmark = pytest.mark.gpu


def dense_model(n, scale, field, seed):
    rng = np.random.default_rng(seed)
    J = rng.normal(scale=scale, size=(n, n))
    J = np.triu(J, 1)
    J = J + J.T
    J[np.diag_indices(n)] = rng.normal(scale=field, size=n)
    return J


def chain_spins(J, N, spc, burn_in, thin, seed):
    with gml.Problem(model=J, num_samples=N, burn_in=burn_in, thin=thin, samples_per_chain=spc, seed=seed) as p:
        assert (p.K, p.n, p.M) == (N, J.shape[0], float(N))
        return p.spins()


@pytest.mark.parametrize("n,nch,burn_in", [(1, 3000, 5), (33, 3000, 8), (100, 2000, 10), (257, 1000, 6)])
def test_bit_for_bit_against_the_restatement(n, nch, burn_in):
    J = dense_model(n, 0.6 / np.sqrt(n), 0.3, seed=n)
    got = chain_spins(J, nch * 4, 4, burn_in, 3, seed=11)
    ref = ref_chains(J, nch, 4, burn_in, 3, seed=11)
    assert np.array_equal(got, ref)


def test_bit_for_bit_at_n_4096():
    n = 4096
    J = dense_model(n, 1.0 / np.sqrt(n), 0.2, seed=4)
    got = chain_spins(J, 64, 1, 2, 1, seed=5)
    assert np.array_equal(got, ref_chains(J, 64, 1, 2, 1, seed=5))


def test_same_chain_as_the_term_list_kernel():
    n, N = 96, 8192
    J = dense_model(n, 0.8 / np.sqrt(n), 0.3, seed=21)
    got = chain_spins(J, N, 1, 30, 1, seed=8)
    terms = {(i + 1, j + 1): J[i, j] for i in range(n) for j in range(i + 1, n)}
    terms.update({(i + 1,): J[i, i] for i in range(n)})
    with gml.Problem(terms=terms, n=n, num_samples=N, seed=8, mcmc_sweeps=30) as p:
        ref = p.spins()
    agree = np.mean(np.all(got == ref, axis=1))
    assert agree >= 0.99, agree


def test_independent_of_tiling_and_seeded():
    J = dense_model(70, 0.1, 0.3, seed=3)
    a = chain_spins(J, 5000, 1, 12, 1, seed=17)
    b = chain_spins(J, 1000, 1, 12, 1, seed=17)
    assert np.array_equal(a[:1000], b)
    assert np.array_equal(chain_spins(J, 1000, 1, 12, 1, seed=17), b)
    assert not np.array_equal(chain_spins(J, 1000, 1, 12, 1, seed=18), b)
    # spc > 1: row t * chains + c, with the rows of t = 0 those of a one-sample run
    c = chain_spins(J, 4000, 4, 12, 3, seed=17)
    assert np.array_equal(c[:1000], b)


def exact_probabilities(m):  # as in test_gpu_sampler.py (weigh_proba, sampling.jl:26-30)
    n = m.shape[0]
    states = ((np.arange(2 ** n)[:, None] >> np.arange(n)) & 1) * 2 - 1
    sf = states.astype(float)
    A = m - np.diag(np.diag(m))
    en = 0.5 * ((sf @ A) * sf).sum(1) + sf @ np.diag(m)
    p = np.exp(en - en.max())
    return states, p / p.sum()


def test_distribution_one_sample_per_chain():
    J = dense_model(12, 0.25, 0.3, seed=6)
    N = 400000
    hist = gml.sample(J, N, sampler=gml.GlauberChains(burn_in=60, thin=1, samples_per_chain=1), seed=1)
    assert hist[:, 0].sum() == N
    states, p = exact_probabilities(J)
    lookup = {tuple(s): pi for s, pi in zip(states, p)}
    seen = set()
    for row in hist:
        expect = lookup[tuple(row[1:])] * N
        assert abs(row[0] - expect) <= 6 * np.sqrt(expect) + 1  # 6 sigma of the binomial count
        seen.add(tuple(row[1:]))
    for s, pi in lookup.items():  # the states never drawn must be rare ones
        if s not in seen:
            assert pi * N <= 40


def test_distribution_thinned_chains():
    J = dense_model(12, 0.25, 0.3, seed=6)
    N = 400000
    hist = gml.sample(J, N, sampler=gml.GlauberChains(burn_in=60, thin=5, samples_per_chain=8), seed=2)
    states, p = exact_probabilities(J)
    s = hist[:, 1:].astype(float)
    w = hist[:, 0] / N
    mag, corr = w @ s, (s * w[:, None]).T @ s
    mag0, corr0 = p @ states, (states * p[:, None]).T @ states
    # 8 correlated samples per chain: the effective sample size is at least the 50 000 chains, sd <= 1 / sqrt(5e4) = 0.0045
    assert np.abs(mag - mag0).max() < 0.02, np.abs(mag - mag0).max()
    assert np.abs(corr - corr0).max() < 0.02, np.abs(corr - corr0).max()


def test_learn_sample_relearn_dense_128():
    n, N = 128, 200000
    J = dense_model(n, 0.05, 0.1, seed=12)
    hist = gml.sample(J, N, sampler=gml.GlauberChains(burn_in=200, thin=10, samples_per_chain=4), seed=3)
    assert hist[:, 0].sum() == N
    learned = gml.learn(hist, gml.RISE(0.02, True), gml.HIP())
    err = np.abs(learned - J).max()
    print(f"learn -> sample -> re-learn, dense n = 128: max |J_learned - J| = {err:.4f}")
    assert err < 0.03, err  # first measured run (MI355X): 0.0129


def test_histogram_flag():
    J = dense_model(20, 0.2, 0.2, seed=9)
    kw = dict(model=J, num_samples=30000, burn_in=20, thin=2, samples_per_chain=3, seed=4)
    with gml.Problem(**kw) as p:
        spins = p.spins()
    with gml.Problem(histogram=True, **kw) as p:
        states, counts = p.spins(), p.counts()
        assert p.M == 30000.0
    assert counts.sum() == 30000
    u, c = np.unique(spins, axis=0, return_counts=True)
    order = np.lexsort(states.T[::-1])
    assert np.array_equal(states[order], u) and np.array_equal(np.rint(counts[order]).astype(int), c)
    with pytest.raises(gml.GMLError, match="n <= 64"):
        gml.Problem(model=dense_model(70, 0.1, 0.1, seed=1), num_samples=100, burn_in=2, histogram=True)
