"""The exact block sampler (gml_sampler.hip: k_block_energies, k_block_cdf, k_block_draw, and their host half in gml_sampled.cpp), the
FP64 Glauber kernel k_glauber and the device histogram (gml_dedupe.hip), draw for draw against tests/_sampler_reference.py.
The cases live in tests/_sampler_cases.py; tests/test_host_sampler_reference.py proves on the reference alone that none of their
random numbers lies within the device's rounding of a decision edge (exact sampler: margin > B_cdf, Glauber: margin > 2^-45), so every
comparison here is np.array_equal with nothing excluded."""
import ctypes as C

import numpy as np
import pytest

import gml_amd as gml
from gml_amd import _lib
import _sampler_cases as cases
import _sampler_reference as R
from test_host_pack import numpy_pack

pytestmark = pytest.mark.gpu


def _hook():
    L = _lib.lib()
    L.gml_test_block_sampler.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    return L.gml_test_block_sampler


def run_block(name, N, seed, block):
    sb, masks, wts, members, n, _, _ = cases.block_model(name)
    en, cdf = np.full(1 << sb, np.nan), np.full(1 << sb, np.nan)
    S = np.full((N, n), 7, dtype=np.int8)
    _lib.check(_hook()(_lib._ptr(masks), _lib._ptr(wts), len(wts), sb, _lib._ptr(members), N, n, seed, block, _lib._ptr(en), _lib._ptr(cdf),
                       _lib._ptr(S)))
    return en, cdf, S


# ------------------------------------------------------------------------------------------
# a. the three kernels on one block
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.BLOCK_MODELS))
def test_block_kernels_against_the_reference(name):
    """en within en_bound, cdf within cdf_bound (derived in _sampler_cases.py) of the np.longdouble reference; cdf non-decreasing
    and ending at exactly 1; the draws are the inversion of the device's own cdf (k_block_draw alone) and the reference's draws
    (all three kernels); spins outside `members` stay 0."""
    sb, masks, wts, members, n, en0, cdf0 = cases.block_model(name)
    nt, sumw = len(wts), float(np.abs(wts).sum())
    ns = 1 << sb
    outside = np.setdiff1d(np.arange(n), members)
    for N, seed, block in cases.BLOCK_RUNS:
        en, cdf, S = run_block(name, N, seed, block)
        e_en, e_cdf = float(np.abs(en - en0).max()), float(np.abs(cdf - cdf0).max())
        b_en, b_cdf = cases.en_bound(nt, sumw), cases.cdf_bound(sb, nt, sumw)
        print(f"{name} sb={sb} nt={nt} N={N} block={block}: en measured / bound = {e_en / b_en if b_en else e_en:.3g}, "
              f"cdf measured / bound = {e_cdf / b_cdf:.3g}")
        assert e_en <= b_en and e_cdf <= b_cdf
        assert np.all(np.diff(cdf) >= 0) and cdf[-1] == 1.0
        u = R.u01(seed, block, np.arange(N, dtype=np.uint64))
        st = np.minimum(np.searchsorted(cdf, u, side="right"), ns - 1)  # the first index with cdf > u
        own = np.zeros((N, n), dtype=np.int8)
        own[:, members] = np.where((st[:, None] >> np.arange(sb)) & 1, 1, -1)
        assert np.array_equal(S, own)
        p = np.diff(np.concatenate([[0.0], cdf]))
        assert np.all(p[st] > 0)  # a state of probability zero is never drawn
        want, _ = cases.block_draws(name, N, seed, block)
        assert np.array_equal(S, want)
        assert not S[:, outside].any() and np.all(np.abs(S[:, members]) == 1)


def test_a_tie_goes_to_the_upper_state():
    """u = 0.5 exactly on the CDF (0.5, 1.0) of an isolated spin (cases.TIE_SEED): the first state whose cdf > u is state 1"""
    en, cdf, S = run_block("isolated_sb1", cases.TIE_N, cases.TIE_SEED, cases.TIE_BLOCK)
    assert en.tolist() == [0.0, 0.0] and cdf.tolist() == [0.5, 1.0]
    want, _ = cases.block_draws("isolated_sb1", cases.TIE_N, cases.TIE_SEED, cases.TIE_BLOCK)
    assert want[cases.TIE_K].tolist() == [0, 1, 0, 0] and np.array_equal(S, want)
    ref, _ = R.exact_draws({(1,): 0.0}, 4, cases.TIE_N, cases.TIE_SEED)  # four isolated spins: spin 3 is block 3
    with gml.Problem(terms={(1,): 0.0}, n=4, num_samples=cases.TIE_N, seed=cases.TIE_SEED) as p:
        got = p.spins()
    assert got[cases.TIE_K, 3] == 1 and np.array_equal(got, ref)


# ------------------------------------------------------------------------------------------
# b. the front door of the exact sampler
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", cases.SEEDS)
@pytest.mark.parametrize("name", sorted(cases.EXACT_CASES))
def test_exact_sampler_draw_for_draw(name, seed):
    terms, n, N, want, _, _ = cases.exact_case(name, seed)
    with gml.Problem(terms=terms, n=n, num_samples=N, seed=seed) as p:
        assert (p.K, p.n, p.M) == (N, n, float(N))
        got = p.spins()
        assert np.array_equal(p.sign_bits(), numpy_pack(want))
    assert np.array_equal(got, want)
    if name == "twins":  # the same terms twice: two streams, not one
        assert not np.array_equal(got[:, :4], got[:, 4:])


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_matrix_route_lists_its_terms_row_by_row(seed):
    # gml_problem_create_sampled turns the matrix into terms row by row with j <= i ((j, i): A_ij for j < i, (i): A_ii), zeros
    # skipped -- cases.matrix_terms; the order of the terms is the order of the FP64 energy sum
    _, n, N, want, _, _ = cases.exact_case("golden_c", seed)
    with gml.Problem(model=cases.MODELS["c"], num_samples=N, seed=seed) as p:
        assert np.array_equal(p.spins(), want)
    _, n, N, want, _, _ = cases.exact_case("blocks64", seed)
    with gml.Problem(model=cases.blocks64_matrix(), num_samples=N, seed=seed) as p:
        assert np.array_equal(p.spins(), want)


# ------------------------------------------------------------------------------------------
# c. k_glauber
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", cases.SEEDS)
@pytest.mark.parametrize("name", sorted(cases.GLAUBER_CASES))
def test_glauber_draw_for_draw(name, seed):
    terms, n, N, sweeps, want, _ = cases.glauber_case(name, seed)
    with gml.Problem(terms=terms, n=n, num_samples=N, mcmc_sweeps=sweeps, seed=seed) as p:
        assert (p.K, p.n, p.M) == (N, n, float(N))
        got, bits = p.spins(), p.sign_bits()
    assert np.array_equal(got, want)
    assert np.array_equal(bits, numpy_pack(want))  # the padding chains of the spin-major output (Np = round_up(N, 256)) stay zero


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_glauber_equals_the_term_chain_kernel_on_dyadic_weights(seed):
    # weights that are multiples of 2^-8: the FP64 field sum and the integer field of k_term_chains are both exact
    terms, n, N, sweeps, want, _ = cases.glauber_case("dyadic33", seed)
    with gml.Problem(terms=terms, n=n, num_samples=N, mcmc_sweeps=sweeps, mcmc_thin=1, mcmc_samples_per_chain=1, seed=seed) as p:
        assert np.array_equal(p.spins(), want)


# ------------------------------------------------------------------------------------------
# d. histogram handles: sample-major draws (exact) and spin-major draws (Glauber)
# ------------------------------------------------------------------------------------------
def check_histogram(p, want, N):
    rows, counts = R.histogram(want)
    assert p.M == float(N) and p.K == len(rows)
    got, cnt = p.spins(), p.counts()
    assert np.array_equal(got, rows) and np.array_equal(cnt, counts.astype(np.float64)) and cnt.sum() == N
    assert np.array_equal(p.sign_bits(), numpy_pack(got))


@pytest.mark.parametrize("seed", cases.SEEDS)
@pytest.mark.parametrize("name", cases.HIST_EXACT)
def test_histogram_of_exact_draws(name, seed):
    terms, n, N, want, _, _ = cases.exact_case(name, seed)
    with gml.Problem(terms=terms, n=n, num_samples=N, seed=seed, histogram=True) as p:
        check_histogram(p, want, N)


@pytest.mark.parametrize("seed", cases.SEEDS)
@pytest.mark.parametrize("name", cases.HIST_GLAUBER)
def test_histogram_of_glauber_draws(name, seed):
    terms, n, N, sweeps, want, _ = cases.glauber_case(name, seed)
    with gml.Problem(terms=terms, n=n, num_samples=N, mcmc_sweeps=sweeps, seed=seed, histogram=True) as p:
        check_histogram(p, want, N)
