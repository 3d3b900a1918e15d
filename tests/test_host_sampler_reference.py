"""The numpy restatement of the exact sampler and of the FP64 Glauber chains (tests/_sampler_reference.py), held to something of its
own -- and the margin rule of tests/test_gpu_sampler_exact.py: for every case of that file, no random number lies closer to a decision
edge than the device's rounding can move the edge, so the GPU tests compare draw for draw without an exclusion.  No GPU needed."""
import itertools

import numpy as np
import pytest

import _sampler_cases as cases
import _sampler_reference as R
from _term_chains_reference import chains as term_chains
from conftest import MODELS


def test_blocks_interleaved_components_cancelled_keys_zero_weights_and_isolated_spins():
    terms = [((1, 4), 0.5), ((4, 7), -0.2), ((2, 5, 8), 0.3), ((5,), 0.1),
             ((1, 2), 0.0),          # zero weight: joins nothing
             ((3, 3, 2, 8), 0.7),    # 3 cancels: the pair (2, 8); 3 stays alone
             ((6, 6), 0.4), ((), 0.9), ((0, -1), 0.3),  # empty after cancellation, empty, unused slots only: dropped
             ((7, 1, 4, 4), -0.6)]   # 4 cancels: the pair (7, 1), listed in the key's order
    got = R.blocks(terms, 9)
    assert [b[0] for b in got] == [[0, 3, 6], [1, 4, 7], [2], [5], [8]]  # numbered by their smallest spin, spins ascending
    assert got[0][1].tolist() == [0b011, 0b110, 0b101] and got[0][2].tolist() == [0.5, -0.2, -0.6]
    assert got[1][1].tolist() == [0b111, 0b010, 0b101] and got[1][2].tolist() == [0.3, 0.1, 0.7]
    for b in got[2:]:
        assert len(b[1]) == 0 and len(b[2]) == 0
    assert got[0][1].dtype == np.uint32 and got[0][2].dtype == np.float64


def test_block_energies_against_the_direct_product_sum():
    rng = np.random.default_rng(0)
    sb = 6
    keys = [c for k in (1, 2, 3, 4) for c in itertools.combinations(range(sb), k)]
    wts = rng.normal(scale=0.5, size=len(keys))
    masks = np.array([sum(1 << i for i in k) for k in keys], dtype=np.uint32)
    en = R.block_energies(masks, wts, sb)
    assert en.dtype == np.longdouble and en.shape == (64,)
    for state in range(64):
        s = [1 if (state >> i) & 1 else -1 for i in range(sb)]
        want = sum(np.longdouble(w) * int(np.prod([s[i] for i in k])) for k, w in zip(keys, wts))
        assert abs(en[state] - want) <= 1e-15


def test_cdf_and_exact_draws_follow_the_exact_probabilities():
    m = MODELS["c"]
    terms = cases.matrix_terms(m)
    N = 200000
    S, margin = R.exact_draws(terms, 4, N, seed=5)
    states = ((np.arange(16)[:, None] >> np.arange(4)) & 1) * 2 - 1
    sf = states.astype(float)
    en = 0.5 * ((sf @ (m - np.diag(np.diag(m)))) * sf).sum(1) + sf @ np.diag(m)  # weigh_proba of the pairwise form
    p = np.exp(en - en.max())
    p /= p.sum()
    (spins, masks, wts), = R.blocks(terms, 4)
    cdf = R.block_cdf(R.block_energies(masks, wts, 4))
    assert cdf[-1] == 1 and np.all(np.diff(cdf) > 0) and np.abs(np.diff(np.concatenate([[0], cdf])) - p).max() <= 1e-15
    emp = np.bincount(((S > 0) * (1 << np.arange(4))).sum(1), minlength=16)
    assert np.all(np.abs(emp - N * p) <= 6 * np.sqrt(N * p * (1 - p)))
    assert 0 < margin < 1


def test_draw_states_takes_the_first_state_above_u_and_reports_the_margin():
    cdf = np.array([0.25, 0.25, 0.75, 1.0], dtype=np.longdouble)  # state 1 has probability zero
    st, margin = R.draw_states(cdf, 5000, 7, 2)
    u = R.u01(7, 2, np.arange(5000, dtype=np.uint64))
    assert np.array_equal(st, np.where(u < 0.25, 0, np.where(u < 0.75, 2, 3))) and 1 not in st
    edges = np.array([0.0, 0.25, 0.75, 1.0])
    assert margin == pytest.approx(np.abs(u[:, None] - edges).min(), abs=1e-18)


@pytest.mark.parametrize("seed", cases.SEEDS)
def test_glauber_equals_the_term_chain_restatement_on_dyadic_weights(seed):
    # multiples of 2^-8 below 1: the FP64 field sum of `glauber` and a_i + sigma_i * (integer sum) of the term chains are both
    # exact, so the two texts of "the same chain" must agree bit for bit
    terms, n, N, sweeps, S, _ = cases.glauber_case("dyadic33", seed)
    assert all(w * 256 == np.rint(w * 256) and abs(w) < 1 for w in terms.values())
    assert np.array_equal(S, term_chains(terms, n, N, 1, sweeps, 1, seed))


def test_histogram_orders_by_unsigned_key():
    S = np.ones((6, 64), dtype=np.int8)
    S[0, 63] = -1
    S[1, 0] = S[4, 0] = -1
    S[2, 62] = -1
    S[5, 63] = S[5, 0] = -1
    rows, counts = R.histogram(S)
    assert counts.dtype == np.int64 and counts.tolist() == [1, 2, 1, 1, 1]
    assert np.array_equal(rows, S[[3, 1, 2, 0, 5]])


# ------------------------------------------------------------------------------------------
# The margin conditions of the GPU cases.  A case that fails here gets another seed of its model or other weights in
# _sampler_cases.py; the GPU test never gets an exclusion list.
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.BLOCK_MODELS))
def test_margin_of_the_block_cases(name):
    sb, masks, wts, members, n, en, cdf = cases.block_model(name)
    assert sorted(members) == list(range(1, 3 * sb, 3)) and n == 3 * sb + 1 and (sb == 1 or np.any(np.diff(members) != 3))
    bound = cases.cdf_bound(sb, len(wts), float(np.abs(wts).sum()))
    for N, seed, block in cases.BLOCK_RUNS:
        _, margin = cases.block_draws(name, N, seed, block)
        print(f"{name} N={N} seed={seed} block={block}: margin {margin:.3e}, B_cdf {bound:.3e}")
        assert margin > bound


def test_the_block_cases_are_the_shapes_they_claim():
    nts = {name: len(cases.block_model(name)[2]) for name in cases.BLOCK_MODELS}
    assert nts["isolated_sb1"] == 0 and nts["field_sb1"] == 1 and nts["subsets_sb13"] == 1092 and nts["chain_sb22"] == 43
    masks = cases.block_model("wide_sb12")[1]
    assert sorted({bin(int(m)).count("1") for m in masks}) == [1, 5, 6, 7, 8]
    sb, _, _, _, _, en, cdf = cases.block_model("steep_sb10")
    p = np.diff(np.concatenate([[0], cdf]))
    assert np.count_nonzero(p == 0) >= 2 ** 10 - 2 ** 6  # flat runs: states whose probability underflows


def test_the_tie_case_draws_exactly_one_half_once():
    u = R.u01(cases.TIE_SEED, cases.TIE_BLOCK, np.arange(cases.TIE_N, dtype=np.uint64))
    assert u[cases.TIE_K] == 0.5 and np.count_nonzero(u == 0.5) == 1
    sb, _, _, _, _, _, cdf = cases.block_model("isolated_sb1")
    assert cdf.tolist() == [0.5, 1.0]  # exact on the device too: the edge does not move, so the margin rule has nothing to guard
    st, _ = R.draw_states(cdf, cases.TIE_N, cases.TIE_SEED, cases.TIE_BLOCK)
    assert st[cases.TIE_K] == 1  # cdf[0] > u is false at u = 0.5
    assert np.abs(np.delete(u, cases.TIE_K) - 0.5).min() > 1e-6
    # four isolated spins through the front door: spin 3 is block 3
    S, _ = R.exact_draws({(1,): 0.0}, 4, cases.TIE_N, cases.TIE_SEED)
    assert S[cases.TIE_K, 3] == 1


@pytest.mark.parametrize("seed", cases.SEEDS)
@pytest.mark.parametrize("name", sorted(cases.EXACT_CASES))
def test_margin_of_the_front_door_cases(name, seed):
    terms, n, N, S, margin, bound = cases.exact_case(name, seed)
    print(f"{name} seed={seed}: margin {margin:.3e}, B_cdf {bound:.3e}")
    assert margin > bound and set(np.unique(S)) <= {-1, 1}
    sizes = sorted(len(b[0]) for b in R.blocks(terms, n))
    if name == "interleaved29":
        assert sizes == [1, 1, 1, 5, 9, 12]
    if name == "blocks64":
        assert sizes == [16] * 4
        rows, counts = R.histogram(S)
        assert np.any(rows[:, 63] == -1) and len(rows) % 32 != 0  # bit 63 of a key, and a ragged last sign word
    if name == "twins":
        assert sizes == [4, 4] and not np.array_equal(S[:, :4], S[:, 4:])
    if name == "wide19":
        assert sizes == [1, 6, 12]
        (_, masks, _), = [b for b in R.blocks(terms, n) if len(b[0]) == 12]
        bits = sorted({bin(int(m)).count("1") for m in masks})
        assert bits == [1, 5, 6, 7, 8] and any(len(set(k)) < len(k) for k in terms)


@pytest.mark.parametrize("seed", cases.SEEDS)
@pytest.mark.parametrize("name", sorted(cases.GLAUBER_CASES))
def test_margin_of_the_glauber_cases(name, seed):
    terms, n, N, sweeps, S, margin = cases.glauber_case(name, seed)
    print(f"{name} seed={seed}: margin {margin:.3e}")
    assert margin > 2.0 ** -45  # far above the few-ulp error of the device's exp in pup
    if name == "sparse33":
        inc = R.incidences(list(terms.items()), n)
        assert inc[7] == [] and inc[21] == [] and any(len(set(k)) < len(k) for k in terms)
    if name == "wide24":
        inc = R.incidences(list(terms.items()), n)
        assert {len(set(k)) for k in terms} >= {5, 6, 7, 8} and any(len(set(k)) < len(k) for k in terms) and all(inc)
    if name == "ring64":
        rows, _ = R.histogram(S)
        assert np.any(rows[:, 63] == -1) and len(rows) % 32 != 0
