"""The host model of the elimination's draws (tests/_elim_draw_reference.py) held to brute force and to the independent sum-product,
and the seeds of tests/test_gpu_elim_draw.py vetted on the CPU: at every case and seed used there, no sample's u total comes nearer
to a running sum than 1000 tau total, tau = 4 bound(terms, n) + 1e-13 -- the elimination's own derived error, which bounds how far the
device's x_c, and hence its p_c / total, can sit from the host model's.  That is what lets the GPU test demand plain equality."""
import numpy as np
import pytest

import _elim_draw_reference as D
import _elim_reference as R
from _exact_reference import ExactModel

CASES = D.draw_cases()


def chi2_quantile_999(df):
    """the 0.999 quantile of chi-square with df degrees of freedom (scipy if present, otherwise Wilson-Hilferty)"""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(0.999, df))
    except ImportError:
        z = 3.090232306167813  # the 0.999 quantile of the standard normal
        return df * (1.0 - 2.0 / (9.0 * df) + z * np.sqrt(2.0 / (9.0 * df))) ** 3


def test_draws_of_a_2x3_lattice_against_brute_force():
    terms, n = R.lattice(2, 3, seed=1)
    N, seed = 65536, 1
    states, _, _ = D.draw(terms, n, N, seed)
    # the 64 probabilities by plain enumeration, bit i of a state set <=> spin i + 1 is -1
    all_states = np.array([[-1 if s >> i & 1 else 1 for i in range(n)] for s in range(1 << n)], dtype=np.int8)
    e = D.energy(terms, all_states)
    prob = np.exp(e - e.max())
    prob /= prob.sum()
    seen = np.bincount(((states < 0).astype(np.int64) << np.arange(n)).sum(axis=1), minlength=1 << n)
    chi2 = float((((seen - N * prob) ** 2) / (N * prob)).sum())
    limit = chi2_quantile_999(63)
    print(f"2 x 3 lattice, N = {N}, seed {seed}: chi-square {chi2:.1f} at 63 degrees of freedom (limit {limit:.1f})")
    assert (N * prob).min() > 5 and chi2 < limit


@pytest.mark.parametrize("case", ["lattice_4x4", "ladder_14", "complete_7", "mixed_conventions", "lattice_4x4_permuted"])
def test_walk_probability_telescopes(case):
    """sum of log(p_c / total) along a walk = E(s) - log Z of the independent sum-product, within bound(); the walk does not cover the
    free spin of the mixed model (a factor 1/2 of its own), and the empty key's weight is in E and in log Z alike"""
    terms, n, order, seed, _ = CASES[case]
    states, _, logp = D.draw(terms, n, 512, seed, order)
    ref = R.SumProduct(terms, n)
    nfree = len(D.launch_list(terms, n, order)[1])
    want = D.energy(terms, states) - float(ref.log_z) + nfree * np.log(2.0)
    err = np.abs(logp - want).max()
    print(f"{case}: max |sum log p - (E - log Z)| = {err:.1e} (bound {R.bound(terms, n):.1e})")
    assert err <= R.bound(terms, n)


def test_against_brute_force_marginals_with_more_than_one_component():
    terms, n = R.mixed_conventions()
    states, _, _ = D.draw(terms, n, 65536, 3)
    brute = ExactModel(terms, n)
    mean = brute.mean.astype(float)
    z = np.abs(states.mean(axis=0) - mean) / np.sqrt((1 - mean ** 2) / 65536)
    assert z.max() < 5, z


@pytest.mark.parametrize("case", sorted(CASES))
def test_gaps_at_the_seeds_of_the_gpu_test(case):
    terms, n, order, seed, N = CASES[case]
    _, gap, _ = D.draw(terms, n, N, seed, order)
    tau = 4 * R.bound(terms, n) + 1e-13
    print(f"{case}: seed {seed}, N = {N}: smallest gap {gap.min():.2e} = {gap.min() / tau:.0f} tau")
    assert gap.min() >= 1000 * tau


def test_seed_of_the_8x8_statistics():
    """the GPU test holds 65 536 device draws of the 8 x 8 lattice to exact moments at z < 5: here the host model's draws at that seed"""
    terms, n, order, seed, N = CASES["lattice_8x8"]
    states = D.draw(terms, n, N, seed, order)[0].astype(np.float64)
    ref = R.SumProduct(terms, n)
    got = np.concatenate([states.mean(axis=0), [np.prod(states[:, [v - 1 for v in k]], axis=1).mean() for k in terms]])
    exact = np.concatenate([ref.mean, ref.texp]).astype(float)
    z = np.abs(got - exact) / np.sqrt((1 - exact ** 2) / N)
    print(f"8 x 8 lattice, seed {seed}: largest z over {len(z)} quantities = {z.max():.2f}")
    assert len(z) == 240 and z.max() < 5


def test_seed_of_the_ferromagnet():
    terms, n, order, seed, N = CASES["ferromagnet_6x6"]
    mag = D.draw(terms, n, N, seed, order)[0].astype(np.int64).sum(axis=1)
    up, down, zero = int((mag > 0).sum()), int((mag < 0).sum()), int((mag == 0).sum())
    print(f"ferromagnet 6 x 6, seed {seed}: {up} up, {down} down, {zero} rows of magnetisation 0")
    assert abs(up - (up + down) / 2) <= 5 * np.sqrt((up + down) / 4)
