"""gml_conditional_draw and gml_conditional_draw_masked on the device: exact draws of every row's hidden spins by Gumbel-max over the
row's enumeration, against the numpy restatement of the rule in np.longdouble (tests/_cond_draw_reference.py), byte for byte where the
contract says so, and as a distribution against the brute-force probabilities.
Tolerances: the states EQUAL to the reference's; energy and log_p within 1e-12 max(1, sum_t |w_t|), the tolerance of the exact
enumerations.  Equal states are a condition, not a measurement: every test asserts on the reference that each chain's gap between its
best and second-best key exceeds 1e-9 (the device's energies are within 1e-12 sum|w| of the reference's and its two logarithms within
a few ulps of a number below 37), and excludes no chain.  Smallest gaps of the reference at seed 7, replicas 3:
h = 1 (K = 200) 2.0e-2, h = 5 (200) 1.3e-3, h = 12 (64) 4.0e-3, h = 13 (32) 1.6e-4, h = 16 (8) 8.3e-3."""
import numpy as np
import pytest

import gml_amd as gml
from _best_reference import cond_model
from _cond_draw_reference import codes_of, cond_draw_masked, cond_draw_rows, state_probabilities
from _cond_exact_reference import tol
from _conditional_reference import random_rows

pytestmark = pytest.mark.gpu
_lib = gml._lib
GAP = 1e-9
N = 16
SEED, REPLICAS = 7, 3
ROWS = {1: 200, 5: 200, 12: 64, 13: 32, 16: 8}  # rows per number of hidden spins: the reference walks 2^h states per chain
RB = 8  # kCondDrawBatch (gml_dev.h): the replicas of a row that one job draws
U01_STREAM = 0xD1B54A32D192ED03  # kU01Stream (gml_rng.h)
_cache = {}


def uniform(terms, n, ev, hidden, replicas=REPLICAS, seed=SEED, **kw):
    """(states [K replicas, h], energy, log_p) of gml_conditional_draw; hidden 0-based"""
    with gml.Problem(spins=np.ascontiguousarray(ev, dtype=np.int8)) as p:
        st, en, lp = _lib.conditional_draw(terms, n, p, hidden, replicas, seed, **kw)
    return st.T.copy(), en, lp


def masked(terms, n, ev, mask, replicas=REPLICAS, seed=SEED, **kw):
    """(completed [K replicas, n], energy, log_p) of gml_conditional_draw_masked; mask bool [K, n]"""
    with gml.Problem(spins=np.ascontiguousarray(ev, dtype=np.int8)) as e:
        with gml.Problem(spins=np.where(mask, -1, 1).astype(np.int8)) as q:
            st, en, lp = _lib.conditional_draw_masked(terms, n, e, q, replicas, seed, **kw)
    return st.T.copy(), en, lp


def case(h):
    """(terms, evidence rows, hidden, the reference's (states, energy, log_p, gap)) of the dense 16-spin model at h hidden spins, once"""
    if h not in _cache:
        terms = cond_model()
        ev = random_rows(ROWS[h], N, h)
        hidden = sorted(int(i) for i in np.random.default_rng(100 + h).choice(N, h, replace=False))
        _cache[h] = (terms, ev, hidden, cond_draw_rows(terms, N, ev, hidden, REPLICAS, SEED))
    return _cache[h]


def check(got, want, terms, what):
    st, en, lp, gap = want
    assert gap.min() > GAP  # the condition: no chain's draw is ambiguous
    errs = (float(np.abs(got[1] - en).max()), float(np.abs(got[2] - lp).max()))
    print(f"{what}: chains = {len(en)}, smallest gap {gap.min():.1e}; errors: energy {errs[0]:.1e}, log_p {errs[1]:.1e}; "
          f"tolerance {tol(terms):.1e}")
    assert np.array_equal(got[0], st)
    assert max(errs) <= tol(terms), errs


# 1. against brute force: one spin, a partial chunk, exactly one chunk, the first with a high bit, sixteen chunks
@pytest.mark.parametrize("h", [1, 5, 12, 13, 16])
def test_against_brute_force(h):
    terms, ev, hidden, want = case(h)
    check(uniform(terms, N, ev, hidden), want, terms, f"h = {h}")


# 2. batching changes nothing: 2 RB + 1 replicas of K rows (three jobs a row, the last of one replica) are the bytes of one replica of
# the evidence tiled that many times -- chain r K + k of the first is row r K + k of the second, chain r K + k again
@pytest.mark.parametrize("h", [5, 13])
def test_batching_changes_nothing(h):
    terms, ev, hidden, _ = case(h)
    ev = ev[:24]
    R = 2 * RB + 1
    a = uniform(terms, N, ev, hidden, replicas=R)
    b = uniform(terms, N, np.tile(ev, (R, 1)), hidden, replicas=1)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()
    st, en, lp = uniform(terms, N, ev, hidden, replicas=R, log_p=False)
    assert lp is None and st.tobytes() == a[0].tobytes() and en.tobytes() == a[1].tobytes()
    st, en, lp = uniform(terms, N, ev, hidden, replicas=R, energy=False, log_p=False)
    assert en is None and lp is None and st.tobytes() == a[0].tobytes()
    again = uniform(terms, N, ev, hidden, replicas=R)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, again))  # the same bytes on every call


# 3. log_p is the sums' own: every row moved to hold its draw, gml_conditional_exact's log_p of the held values is the draw's, bit for bit
@pytest.mark.parametrize("h", [5, 13])
def test_log_p_is_the_sums_own(h):
    terms, ev, hidden, _ = case(h)
    K = len(ev)
    st, en, lp = uniform(terms, N, ev, hidden)
    moved = np.tile(ev, (REPLICAS, 1))
    moved[:, hidden] = st  # row r K + k holds the draw of chain r K + k (the visible spins, and so log_w, are unchanged)
    with gml.Problem(spins=moved) as p:
        _, lw, held = _lib.conditional_exact(terms, N, p, hidden)
    assert np.array_equal(held, lp) and np.array_equal(en - lw, lp)
    assert np.array_equal(lw[:K], lw[K:2 * K])


# 4. the per-row form
def test_uniform_mask_is_the_unmasked_call():
    terms, ev, hidden, _ = case(5)
    mask = np.zeros(ev.shape, dtype=bool)
    mask[:, hidden] = True
    visible = [i for i in range(N) if i not in hidden]
    for kw in (dict(), dict(log_p=False)):
        a = uniform(terms, N, ev, hidden, **kw)
        b = masked(terms, N, ev, mask, **kw)
        assert b[0][:, hidden].tobytes() == a[0].tobytes() and b[1].tobytes() == a[1].tobytes()
        assert (a[2] is None and b[2] is None) or b[2].tobytes() == a[2].tobytes()
        assert np.array_equal(b[0][:, visible], np.tile(ev[:, visible], (REPLICAS, 1)))


def ragged_case():
    """(terms, rows, mask): a different hidden set per row, 0 to 9 holes, some rows without any"""
    terms = cond_model()
    rng = np.random.default_rng(77)
    ev = random_rows(90, N, 77)
    mask = np.zeros(ev.shape, dtype=bool)
    for k in range(len(ev)):
        mask[k, rng.choice(N, size=k % 10, replace=False)] = True
    return terms, ev, mask


def test_a_hidden_set_per_row():
    terms, ev, mask = ragged_case()
    want = cond_draw_masked(terms, N, ev, mask, REPLICAS, SEED)
    holes = np.tile(mask.any(axis=1), REPLICAS)
    assert (~holes).sum() == 9 * REPLICAS and want[3].min() > GAP
    got = masked(terms, N, ev, mask)
    assert np.array_equal(got[0], want[0])
    errs = (float(np.abs(got[1] - want[1]).max()), float(np.abs(got[2] - want[2]).max()))
    print(f"a hidden set per row: smallest gap {want[3].min():.1e}; errors: energy {errs[0]:.1e}, log_p {errs[1]:.1e}; "
          f"tolerance {tol(terms):.1e}")
    assert max(errs) <= tol(terms)
    # a row without holes: itself, its own energy, probability 1
    assert np.array_equal(got[0][~holes], np.tile(ev, (REPLICAS, 1))[~holes]) and np.all(got[2][~holes] == 0.0)


def test_permuted_rows_with_their_chain_numbers():
    """A chain's result is a function of (row, hidden set, seed, c), and c is the row's PLACE, r K + k: permuted rows get other chains.
    Two ways to hold c fixed.  (a) The permuted call against the reference run with the chain numbers of the places.  (b) u01 hashes
    seed + kU01Step (s + 1) + kU01Stream (c + 1): chain 0 of seed + kU01Stream c is chain c of seed.  So row k of the whole call,
    replicas = 1, is the one-row call on that row at seed + kU01Stream k, byte for byte, whatever rows stood beside it."""
    terms, ev, mask = ragged_case()
    K = len(ev)
    perm = np.random.default_rng(5).permutation(K)
    whole = masked(terms, N, ev, mask, replicas=1)
    b = masked(terms, N, ev[perm], mask[perm], replicas=1)
    want = cond_draw_masked(terms, N, ev[perm], mask[perm], 1, SEED, chains=np.arange(K))
    assert want[3].min() > GAP and np.array_equal(b[0], want[0]) and float(np.abs(b[1] - want[1]).max()) <= tol(terms)
    for k in (0, 9, 17, 38, 59, 89):  # 0, 9, 7, 8, 9, 9 holes
        alone = masked(terms, N, ev[k:k + 1], mask[k:k + 1], replicas=1, seed=(SEED + U01_STREAM * k) % 2 ** 64)
        for x, y in zip(whole, alone):
            assert x[k:k + 1].tobytes() == y.tobytes()


def test_too_many_holes_are_refused_by_row():
    terms = {(i, i + 1): 0.2 for i in range(1, 30)}
    ev = random_rows(3, 30, 1)
    mask = np.zeros(ev.shape, dtype=bool)
    mask[1, :25] = True
    mask[0, :24] = True
    with pytest.raises(gml.GMLError, match="row 1 hides 25 spins"):
        masked(terms, 30, ev, mask)


# 5. the chunk hook: 13 hidden spins at 8 chunk bits, 32 chunks per row
def test_chunk_hook():
    terms, ev, hidden, want = case(13)
    assert want[3].min() > GAP
    try:
        assert _lib.lib().gml_test_exact_chunk_bits(8) >= 0
        for kw in (dict(), dict(log_p=False)):
            got = uniform(terms, N, ev, hidden, **kw)
            assert np.array_equal(got[0], want[0]) and float(np.abs(got[1] - want[1]).max()) <= tol(terms)
            assert got[2] is None or float(np.abs(got[2] - want[2]).max()) <= tol(terms)
    finally:
        _lib.lib().gml_test_exact_chunk_bits(0)


# 6. it is the right distribution: 4096 draws of 3 hidden spins of one row against the brute-force probabilities
def test_chi_square_against_the_probabilities():
    """The reference alone gives chi-square 6.4 at this seed (smallest expected count 82, smallest gap 1.3e-4); the device's states
    equal the reference's, so it gives the same count.  24.32: the 0.999 quantile of chi-square at 7 degrees of freedom."""
    terms = {k: 0.4 * w for k, w in cond_model().items()}
    row = random_rows(1, N, 53)[0]
    hidden = sorted(int(i) for i in np.random.default_rng(103).choice(N, 3, replace=False))
    ev = np.tile(row, (256, 1))
    st, en, lp = uniform(terms, N, ev, hidden, replicas=16)
    want = cond_draw_rows(terms, N, ev, hidden, 16, SEED)
    assert want[3].min() > GAP and np.array_equal(st, want[0])
    p = state_probabilities(terms, row, hidden)
    counts = np.bincount(codes_of(st), minlength=8)
    chi2 = float(((counts - 4096 * p) ** 2 / (4096 * p)).sum())
    print(f"chi-square {chi2:.2f} (7 degrees of freedom), smallest expected count {4096 * p.min():.0f}, smallest gap {want[3].min():.1e}")
    assert counts.sum() == 4096 and chi2 < 24.32
    assert float(np.abs(lp - np.log(p)[codes_of(st)]).max()) <= 1e-12 + tol(terms)


def test_hidden_spin_in_no_term_is_a_coin_flip():
    terms = {(1, 2): 0.4, (2, 3): -0.3, (3,): 0.2, (1, 5): 0.25}
    ev = -np.ones((40, 6), dtype=np.int8)  # (the evidence holds -1 on the free spins: what it holds there plays no part)
    ev[:, :3] = random_rows(40, 3, 3)
    for hidden in ([1, 3, 5], [3], [0, 1, 2, 3, 4, 5]):
        st, en, lp = uniform(terms, 6, ev, hidden)
        want = cond_draw_rows(terms, 6, ev, hidden, REPLICAS, SEED)
        assert want[3].min() > GAP and np.array_equal(st, want[0])
        for i in (3, 5):  # spins 4 and 6 (1-based) are in no term
            if i in hidden:
                col = st[:, hidden.index(i)]
                assert (col == 1).any() and (col == -1).any()
        assert float(np.abs(en - want[1]).max()) <= tol(terms) and float(np.abs(lp - want[2]).max()) <= tol(terms)


def test_refusals():
    terms, ev, hidden, _ = case(5)
    with pytest.raises(gml.GMLError, match="replicas"):
        uniform(terms, N, ev, hidden, replicas=0)
    with pytest.raises(gml.GMLError, match="no spin is hidden"):
        uniform(terms, N, ev, [])


# 7. the front doors
def test_conditional_sample_exact():
    terms, ev, hidden, _ = case(5)
    ev = ev[:40]
    st, _, _ = uniform(terms, N, ev, hidden, replicas=2, seed=11)
    samples = np.hstack([np.ones((len(ev), 1)), ev])
    with gml.conditional_sample(terms, samples, [i + 1 for i in hidden], replicas=2, seed=11, method=gml.Exact()) as q:
        rows, counts = q.spins(), q.counts()
    want = np.tile(ev, (2, 1))
    want[:, hidden] = st
    assert rows.shape == (80, N) and np.all(counts == 1) and np.array_equal(rows, want)
    with gml.Problem(spins=ev) as p:  # an open handle as evidence
        with gml.conditional_sample(terms, p, [i + 1 for i in hidden], replicas=2, seed=11, method=gml.Exact()) as q:
            assert np.array_equal(q.spins(), want)


def test_impute_sample_exact():
    terms, ev, mask = ragged_case()
    samples = np.hstack([np.ones((len(ev), 1)), np.where(mask, 0, ev)])
    with gml.impute_sample(terms, samples, replicas=2, seed=11, method=gml.Exact()) as q:
        rows, counts = q.spins(), q.counts()
    # the chains are numbered in the order of the packed masks: the _lib call on the rows in that order, put back
    perm = gml.inference._mask_order(mask)
    st, _, _ = masked(terms, N, ev[perm], mask[perm], replicas=2, seed=11)
    want = st.reshape(2, len(ev), N)[:, np.argsort(perm)].reshape(-1, N)
    assert rows.shape == (180, N) and np.all(counts == 1) and np.array_equal(rows, want)
    assert np.array_equal(rows[np.tile(~mask, (2, 1))], np.tile(ev, (2, 1))[np.tile(~mask, (2, 1))])
    ref = cond_draw_masked(terms, N, ev[perm], mask[perm], 2, 11)
    assert ref[3].min() > GAP and np.array_equal(st, ref[0])
