"""gml_conditional_exact and gml_conditional_exact_masked on the device: exact conditional means, log sum exp(E) and the conditional
log-probability of the held values by enumeration of every row's hidden spins, against brute force in np.longdouble
(tests/_cond_exact_reference.py), against gml_model_exact, against the conditional chains where one spin is hidden, and bit for bit
where the contract says so.
Tolerance of log_w, log_p, every mean and the Python aggregates: 1e-12 max(1, sum_t |w_t|), absolute -- the project's tolerance of the
exact enumerations (tests/test_gpu_exact.py): the a-priori error is about (12 + log2 T) 2^-53 sum|w| from the energies plus about
1e-13 from the sums."""
import itertools

import numpy as np
import pytest

import gml_amd as gml
from _ais_reference import sparse_model
from _cond_exact_reference import cond_exact_masked, cond_exact_rows, energy, tol
from _conditional_reference import closed_form_bound, exact_field, random_rows
from _exact_reference import LD

pytestmark = pytest.mark.gpu
_lib = gml._lib

K70 = 70  # rows: the row words 0 to 2, the last partial


def uniform(terms, n, ev, hidden, **kw):
    """(means [K, h], log_w [K], log_p [K]) of gml_conditional_exact; hidden 0-based"""
    with gml.Problem(spins=np.ascontiguousarray(ev, dtype=np.int8)) as p:
        m, lw, lp = _lib.conditional_exact(terms, n, p, hidden, **kw)
    return (None if m is None else m.T.copy()), lw, lp


def masked(terms, n, ev, mask, **kw):
    """(means [K, n], log_w [K], log_p [K]) of gml_conditional_exact_masked; mask bool [K, n]"""
    with gml.Problem(spins=np.ascontiguousarray(ev, dtype=np.int8)) as e:
        with gml.Problem(spins=np.where(mask, -1, 1).astype(np.int8)) as q:
            m, lw, lp = _lib.conditional_exact_masked(terms, n, e, q, **kw)
    return (None if m is None else m.T.copy()), lw, lp


def errors(got, want):
    return tuple(float(np.abs(g - w).max()) for g, w in zip(got, want))


def check_uniform(terms, n, ev, hidden, what):
    got = uniform(terms, n, ev, hidden)
    want = cond_exact_rows(terms, n, ev, hidden)
    errs = errors(got, want)
    print(f"{what}: n = {n}, K = {len(ev)}, h = {len(hidden)}, sum|w| = {tol(terms) / 1e-12:.1f}; errors: means {errs[0]:.1e}, log_w {errs[1]:.1e}, "
          f"log_p {errs[2]:.1e}; tolerance {tol(terms):.1e}")
    assert all(np.isfinite(g).all() for g in got)
    assert max(errs) <= tol(terms), errs
    return got


def multi_body_model(n, seed):
    """sparse terms of orders 1 to 4"""
    terms = sparse_model(n, 3, 2, 0.3, seed, order=3)
    terms.update(sparse_model(n, 2, 0, 0.3, seed + 1, order=4, fields=False))
    return terms


def spread_hidden(n, h, seed):
    return sorted(int(i) for i in np.random.default_rng(seed).choice(n, h, replace=False))


# 1. against brute force: one spin, a partial chunk, exactly one chunk, the first with a high bit, sixteen chunks
@pytest.mark.parametrize("h", [1, 5, 12, 13, 16])
def test_against_brute_force(h):
    n = 40
    check_uniform(multi_body_model(n, 20 + h), n, random_rows(K70, n, h), spread_hidden(n, h, 100 + h), "multi-body")


def test_every_rule_of_the_term_list():
    # a spin named twice, a zero weight, the empty key, visible-only terms and hidden-only terms
    n, hidden = 12, [1, 4, 5, 9]
    terms = {(2, 5): 0.3, (2, 2, 5): -0.45, (2, 6): 0.0, (): 0.7, (1, 3): 0.25, (7, 8, 11): -0.2, (12,): 0.15, (2, 5, 6, 10): 0.35, (6,): -0.3,
             (10, 10): 0.1, (5, 6, 6): 0.2, (1, 2, 3, 4, 5, 6, 7, 8): 0.05, (6, 10): -0.4, (3, 3, 4, 4): -0.6}
    check_uniform(terms, n, random_rows(K70, n, 3), hidden, "term rules")


# 2. spins on the edges of the row words; every singleton's coefficient has 64 terms and more: items and partial sums
def test_dense_pairwise_70():
    n = 70
    rng = np.random.default_rng(70)
    terms = {(i + 1, j + 1): float(rng.normal(scale=0.1)) for i in range(n) for j in range(i + 1, n)}
    terms.update({(i + 1,): float(rng.normal(scale=0.2)) for i in range(n)})
    check_uniform(terms, n, random_rows(K70, n, 70), [0, 31, 32, 63, 64, 69], "dense pairwise")


def test_dense_pairwise_300():
    # n above 256: the gather of the row's bits takes a second round, hidden spins on both sides of it; 45 000 terms without a hidden
    # spin: the items double from 16 terms until the partial sums fit
    n = 300
    rng = np.random.default_rng(300)
    terms = {(i + 1, j + 1): float(rng.normal(scale=0.05)) for i in range(n) for j in range(i + 1, n)}
    terms.update({(i + 1,): float(rng.normal(scale=0.2)) for i in range(n)})
    check_uniform(terms, n, random_rows(5, n, 300), [0, 255, 256, 257, 299], "dense pairwise")


def test_terms_of_one_visible_spin():
    # no term has two visible spins: one 16-bit slot per term
    n, hidden = 7, [0, 1, 2]
    terms = {(1, 4): 0.3, (2, 5): -0.4, (3, 6): 0.5, (4,): 0.2, (7,): -0.3, (1, 2): 0.25, (1, 2, 3): -0.15, (2, 3, 7): 0.35, (3,): 0.1}
    check_uniform(terms, n, random_rows(K70, n, 7), hidden, "one visible spin")


# 3. the chunk hook
def test_chunk_width_invariance():
    n, h = 30, 12
    terms, ev, hidden = multi_body_model(n, 3), random_rows(K70, n, 12), spread_hidden(n, h, 5)
    got = {}
    try:
        for c in (4, 8, 12):
            assert _lib.lib().gml_test_exact_chunk_bits(c) >= 0
            got[c] = check_uniform(terms, n, ev, hidden, f"chunk bits {c}")
    finally:
        _lib.lib().gml_test_exact_chunk_bits(0)
    for c in (4, 8):
        assert max(errors(got[c], got[12])) <= 2 * tol(terms)


def test_more_chunks_than_one_accumulator_takes():
    # 19 hidden spins at 8 chunk bits: 2048 chunks, the first accumulator folds into the second twice
    n, h = 24, 19
    terms = multi_body_model(n, 19)
    try:
        assert _lib.lib().gml_test_exact_chunk_bits(8) >= 0
        check_uniform(terms, n, random_rows(2, n, 19), spread_hidden(n, h, 19), "chunk bits 8")
    finally:
        _lib.lib().gml_test_exact_chunk_bits(0)


# 4. range: neither a shift by sum|w| nor an unshifted exp would do
@pytest.mark.parametrize("J", [-150.0, 150.0])
def test_range(J):
    n = 8
    terms = {k: J for k in itertools.combinations(range(1, 7), 2)}
    terms.update({(1, 7): 0.4, (6, 8): -0.3, (7, 8): 0.2, (3, 7, 8): 0.1})
    check_uniform(terms, n, random_rows(K70, n, 6), list(range(6)), f"K6 at J = {J}")


# 5. ties to gml_model_exact
def test_all_hidden_is_the_model():
    n = 10
    terms = multi_body_model(n, 10)
    terms[()] = -0.4
    log_z, mean, _, _ = _lib.model_exact(terms, n, pairs=False)
    m, lw, lp = uniform(terms, n, random_rows(K70, n, 10), list(range(n)))
    assert np.abs(lw - log_z).max() <= tol(terms) and np.abs(m - mean).max() <= tol(terms)
    assert np.all(lw == lw[0]) and np.all(m == m[0])  # every row: the same bits
    want = np.array([float(energy(terms, r)) for r in random_rows(K70, n, 10)]) - log_z
    assert np.abs(lp - want).max() <= 2 * tol(terms)


def test_marginalising_the_visible_spins_gives_the_model():
    n, vis = 10, [2, 3, 6, 8]
    hidden = [i for i in range(n) if i not in vis]
    terms = multi_body_model(n, 11)
    ev = np.ones((16, n), dtype=np.int8)
    ev[:, vis] = np.where((np.arange(16)[:, None] >> np.arange(4)) & 1, -1, 1)
    log_z, mean, _, _ = _lib.model_exact(terms, n, pairs=False)
    m, lw, _ = uniform(terms, n, ev, hidden)
    assert abs(float(np.log(np.sum(np.exp(lw.astype(LD) - lw.max()))) + lw.max()) - log_z) <= tol(terms)
    P = np.exp(lw - log_z)
    assert abs(P.sum() - 1.0) <= 16 * tol(terms)
    assert np.abs(P @ m - mean[hidden]).max() <= tol(terms)
    assert np.abs(P @ ev[:, vis].astype(np.float64) - mean[vis]).max() <= tol(terms)


# 6. tie to the chains: with one hidden spin the Rao-Blackwellised mean is tanh of the quantised field
def test_one_hidden_spin_against_the_chains():
    n, i = 33, 32
    terms = sparse_model(n, 6, 4, 0.3, 4)
    ev = random_rows(K70, n, 0)
    with gml.Problem(spins=ev) as p:
        chain = _lib.conditional_chains(terms, n, p, [i], 1, 1, 1, 1, 0, means=True)[0]
        exact = _lib.conditional_exact(terms, n, p, [i])[0][0]
    want = np.tanh([exact_field(terms, n, r, i) for r in ev])
    assert np.abs(exact - want).max() <= tol(terms)
    assert np.abs(exact - chain).max() <= closed_form_bound(terms, n, i) + tol(terms)


# 7. a hidden set per row
def mixed_case():
    n = 12
    terms = multi_body_model(n, 12)
    ev = random_rows(K70, n, 7)
    mask = np.random.default_rng(8).random((K70, n)) < 0.25
    mask[3] = False                       # a row with no holes
    mask[4] = True                        # a row with every spin hidden
    mask[5], mask[66] = mask[40], mask[40]  # equal patterns far apart
    return terms, n, ev, mask


def test_masked_against_brute_force():
    terms, n, ev, mask = mixed_case()
    got = masked(terms, n, ev, mask)
    want = cond_exact_masked(terms, n, ev, mask)
    errs = errors(got, want)
    print(f"masked: {len({tuple(r) for r in mask})} patterns in {K70} rows; errors: means {errs[0]:.1e}, log_w {errs[1]:.1e}, log_p {errs[2]:.1e}")
    assert max(errs) <= tol(terms), errs
    m, lw, lp = got
    assert np.array_equal(m[~mask], ev[~mask].astype(np.float64))  # an observed entry holds its evidence value
    assert np.array_equal(m[3], ev[3].astype(np.float64)) and abs(lw[3] - float(energy(terms, ev[3]))) <= tol(terms) and lp[3] == 0.0
    log_z, mean, _, _ = _lib.model_exact(terms, n, pairs=False)
    assert abs(lw[4] - log_z) <= tol(terms) and np.abs(m[4] - mean).max() <= tol(terms)
    # rows 5, 40 and 66 share a pattern: each the uniform form's bits of its own row
    hid = np.flatnonzero(mask[40])
    um, ulw, ulp = uniform(terms, n, ev, hid)
    for k in (5, 40, 66):
        assert np.array_equal(m[k, hid], um[k]) and lw[k] == ulw[k] and lp[k] == ulp[k]


def test_uniform_mask_is_the_unmasked_call_bit_for_bit():
    n, hid = 40, [0, 7, 31, 32, 39]
    terms, ev = multi_body_model(n, 21), random_rows(K70, n, 9)
    mask = np.zeros((K70, n), dtype=bool)
    mask[:, hid] = True
    m, lw, lp = masked(terms, n, ev, mask)
    um, ulw, ulp = uniform(terms, n, ev, hid)
    assert np.array_equal(m[:, hid], um) and np.array_equal(lw, ulw) and np.array_equal(lp, ulp)


def test_permuting_the_rows_permutes_the_outputs():
    terms, n, ev, mask = mixed_case()
    perm = np.random.default_rng(1).permutation(K70)
    a, b = masked(terms, n, ev, mask), masked(terms, n, ev[perm], mask[perm])
    assert all(np.array_equal(x[perm], y) for x, y in zip(a, b))


def test_a_row_with_25_holes_is_refused_by_name():
    n = 30
    terms = {(i + 1, i + 2): 0.1 for i in range(n - 1)}
    mask = np.zeros((5, n), dtype=bool)
    mask[1, :24], mask[3, :25], mask[4, :26] = True, True, True
    with pytest.raises(gml.GMLError, match="row 3 hides 25 spins.*at most 24"):
        masked(terms, n, random_rows(5, n, 1), mask)
    with pytest.raises(gml.GMLError, match="25 spins are hidden.*at most 24"):
        uniform(terms, n, random_rows(5, n, 1), list(range(25)))


def test_24_hidden_spins():
    # one row, ten terms: 2^24 states in 4096 chunks, the reference in 64 blocks
    n = 26
    rng = np.random.default_rng(24)
    terms = {tuple(int(v) + 1 for v in rng.choice(n, size=k, replace=False)): float(rng.normal(scale=0.5)) for k in (1, 1, 2, 2, 2, 2, 3, 3, 4, 2)}
    mask = np.zeros((1, n), dtype=bool)
    mask[0, [i for i in range(n) if i not in (5, 20)]] = True
    ev = random_rows(1, n, 24)
    got = masked(terms, n, ev, mask)
    want = cond_exact_masked(terms, n, ev, mask)
    errs = errors(got, want)
    print(f"h = 24: errors: means {errs[0]:.1e}, log_w {errs[1]:.1e}, log_p {errs[2]:.1e}; tolerance {tol(terms):.1e}")
    assert max(errs) <= tol(terms), errs


# 8. the result of a row is a function of the model, the row and its hidden set
def test_reproducible_bits():
    n, h = 40, 13
    terms, ev, hidden = multi_body_model(n, 33), random_rows(K70, n, 13), spread_hidden(n, h, 113)
    a, b = uniform(terms, n, ev, hidden), uniform(terms, n, ev, hidden)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for k in (0, 37, 69):
        one = uniform(terms, n, ev[k:k + 1], hidden)
        assert all(np.array_equal(x[k:k + 1], y) for x, y in zip(a, one))
    only = uniform(terms, n, ev, hidden, means=False, log_p=False)
    assert only[0] is None and only[2] is None and np.array_equal(only[1], a[1])


# 9. the front door
def front_door_case():
    n = 8
    terms = multi_body_model(n, 44)
    rng = np.random.default_rng(45)
    data = np.concatenate([rng.integers(1, 6, size=(20, 1)), rng.choice([-1, 1], size=(20, n))], axis=1).astype(np.float64)
    return terms, n, data


def test_front_door_conditional_means_and_predictive_check():
    terms, n, data = front_door_case()
    hidden = [2, 5, 8]  # 1-based
    rows = data[:, 1:].astype(np.int8)
    want = cond_exact_rows(terms, n, rows, [i - 1 for i in hidden])
    cm = gml.conditional_means(terms, data, hidden, method=gml.Exact())
    assert cm.hidden == hidden and np.array_equal(cm.counts, data[:, 0]) and cm.per_replica.shape == (1, 20, 3)
    assert np.all(cm.stderr == 0.0) and np.array_equal(cm.per_replica[0], cm.means)
    assert max(errors((cm.means, cm.log_w, cm.log_p), want)) <= tol(terms)
    pc = gml.predictive_check(terms, data, hidden, method=gml.Exact())
    w = data[:, 0] / data[:, 0].sum()
    truth = rows[:, [i - 1 for i in hidden]].astype(np.float64)
    assert np.array_equal(pc.means.means, cm.means)
    assert abs(pc.joint_log_loss - float(-(w.astype(LD) @ want[2]))) <= tol(terms)
    assert np.abs(pc.log_loss - (w @ -np.log((1 + truth * want[0].astype(np.float64)) / 2))).max() <= 10 * tol(terms)
    assert np.array_equal(pc.accuracy, w @ (np.where(want[0] >= 0, 1.0, -1.0) == truth))
    chains = gml.predictive_check(terms, data, hidden)
    assert chains.joint_log_loss is None and chains.means.log_w is None and chains.means.log_p is None  # method=None: as before


def test_front_door_impute_and_observed_log_likelihood():
    terms, n, data = front_door_case()
    full = gml.observed_log_likelihood(data, terms, gml.Exact())
    ll = gml.log_likelihood(data, terms, gml.Exact())
    assert abs(full.mean - ll.mean) <= tol(terms) and full.log_z == ll.log_z and abs(full.data_term - ll.data_term) <= tol(terms)
    holes = data.copy()
    missing = np.random.default_rng(46).random((20, n)) < 0.3
    missing[0], missing[1] = False, True
    holes[:, 1:][missing] = 0
    got = gml.observed_log_likelihood(holes, terms, gml.Exact())
    # brute-force marginalisation: log P(x_O) = log sum over the completions of exp(E) - log Z, all in long double
    states = np.where((np.arange(1 << n)[:, None] >> np.arange(n)) & 1, -1, 1).astype(np.int8)
    E = np.array([energy(terms, s) for s in states], dtype=LD)
    log_z = np.log(np.sum(np.exp(E - E.max()))) + E.max()
    want = LD(0)
    for k in range(20):
        fits = np.all((states == holes[k, 1:]) | missing[k], axis=1)
        want += LD(holes[k, 0]) * (np.log(np.sum(np.exp(E[fits] - E.max()))) + E.max() - log_z)
    want /= holes[:, 0].sum()
    print(f"observed log-likelihood {got.mean!r}, brute force {float(want)!r}")
    assert abs(got.mean - want) <= tol(terms) and abs(got.total - want * holes[:, 0].sum()) <= tol(terms) * holes[:, 0].sum()
    # impute: a row of count c becomes c rows
    imp = gml.impute(terms, holes, method=gml.Exact())
    reps = np.repeat(np.arange(20), holes[:, 0].astype(int))
    ref = cond_exact_masked(terms, n, np.where(missing, 1, data[:, 1:]).astype(np.int8), missing)[0][reps]
    assert imp.means.shape == (len(reps), n) and np.array_equal(imp.missing, missing[reps]) and np.all(imp.stderr == 0.0)
    assert np.abs(imp.means - ref).max() <= tol(terms)
    assert np.array_equal(imp.means[~imp.missing], data[:, 1:][reps][~imp.missing])
