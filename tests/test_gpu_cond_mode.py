"""gml_conditional_mode and gml_conditional_mode_masked on the device: every row's most probable joint state of its hidden spins, its
energy and its conditional log-probability, against brute force in np.longdouble (tests/_best_reference.py on top of
tests/_cond_exact_reference.py), and bit for bit against gml_conditional_exact where the contract says so.
Tolerances: the states EQUAL to the reference's; energy and log_p within 1e-12 max(1, sum_t |w_t|), the project's tolerance of the exact
enumerations.  Equal states are a condition, not a measurement: every test asserts on the reference that each row's gap between its
best and second-best energy exceeds 1e-9 (where a test is about an exact tie, it says so)."""
import numpy as np
import pytest

import gml_amd as gml
from _best_reference import cond_mode_masked, cond_mode_rows, cond_model
from _cond_exact_reference import cond_exact_rows, tol
from _conditional_reference import random_rows

pytestmark = pytest.mark.gpu
_lib = gml._lib
GAP = 1e-9
N = 16
ROWS = {1: 200, 5: 200, 12: 200, 13: 64, 16: 32}  # rows per number of hidden spins: the reference walks 2^h states per row
_cache = {}


def uniform(terms, n, ev, hidden, **kw):
    """(states [K, h], energy [K], log_p [K]) of gml_conditional_mode; hidden 0-based"""
    with gml.Problem(spins=np.ascontiguousarray(ev, dtype=np.int8)) as p:
        st, en, lp = _lib.conditional_mode(terms, n, p, hidden, **kw)
    return st.T.copy(), en, lp


def masked(terms, n, ev, mask, **kw):
    """(completed [K, n], energy [K], log_p [K]) of gml_conditional_mode_masked; mask bool [K, n]"""
    with gml.Problem(spins=np.ascontiguousarray(ev, dtype=np.int8)) as e:
        with gml.Problem(spins=np.where(mask, -1, 1).astype(np.int8)) as q:
            st, en, lp = _lib.conditional_mode_masked(terms, n, e, q, **kw)
    return st.T.copy(), en, lp


def case(h):
    """(terms, evidence rows, hidden, the reference's (states, energy, log_p, gap)) of the dense 16-spin model at h hidden spins, once"""
    if h not in _cache:
        terms = cond_model()
        ev = random_rows(ROWS[h], N, h)
        hidden = sorted(int(i) for i in np.random.default_rng(100 + h).choice(N, h, replace=False))
        _cache[h] = (terms, ev, hidden, cond_mode_rows(terms, N, ev, hidden))
    return _cache[h]


def check(got, want, terms, what):
    st, en, lp, gap = want
    assert gap.min() > GAP  # the condition: no row's mode is ambiguous
    errs = (float(np.abs(got[1] - en).max()), float(np.abs(got[2] - lp).max()))
    print(f"{what}: K = {len(en)}, smallest gap {gap.min():.1e}; errors: energy {errs[0]:.1e}, log_p {errs[1]:.1e}; tolerance {tol(terms):.1e}")
    assert np.array_equal(got[0], st)
    assert max(errs) <= tol(terms), errs


# against brute force: one spin, a partial chunk, exactly one chunk, the first with a high bit, sixteen chunks
@pytest.mark.parametrize("h", [1, 5, 12, 13, 16])
def test_against_brute_force(h):
    terms, ev, hidden, want = case(h)
    check(uniform(terms, N, ev, hidden), want, terms, f"h = {h}")


# 1. log_p against gml_conditional_exact: never below the held values' own, and the same bits where the held values are the mode
@pytest.mark.parametrize("h", [5, 13])
def test_log_p_against_the_held_values(h):
    terms, ev, hidden, _ = case(h)
    st, _, lp = uniform(terms, N, ev, hidden)
    with gml.Problem(spins=ev) as p:
        _, lw, held = _lib.conditional_exact(terms, N, p, hidden)
    assert np.all(lp >= held)
    is_mode = np.all(ev[:, hidden] == st, axis=1)
    assert np.array_equal(lp[is_mode], held[is_mode]) and np.all(lp[~is_mode] > held[~is_mode])
    moved = ev.copy()
    moved[:, hidden] = st  # every row now holds its mode (the visible spins, and so the mode, are unchanged)
    with gml.Problem(spins=moved) as p:
        _, lw2, held2 = _lib.conditional_exact(terms, N, p, hidden)
    assert np.array_equal(lw2, lw) and np.array_equal(held2, lp)


# 2. what is asked for changes nothing else; without log_p the kernel takes no exponential and gives the same states
@pytest.mark.parametrize("h", [5, 13])
def test_outputs_are_independent(h):
    terms, ev, hidden, _ = case(h)
    full = uniform(terms, N, ev, hidden)
    st, en, lp = uniform(terms, N, ev, hidden, energy=False)
    assert en is None and np.array_equal(lp, full[2]) and np.array_equal(st, full[0])
    st, en, lp = uniform(terms, N, ev, hidden, log_p=False)
    assert lp is None and np.array_equal(st, full[0]) and np.array_equal(en, full[1])
    st, en, lp = uniform(terms, N, ev, hidden, energy=False, log_p=False)
    assert en is None and lp is None and np.array_equal(st, full[0])


# 3. the per-row form
def test_uniform_mask_is_the_unmasked_call():
    terms, ev, hidden, _ = case(5)
    a = uniform(terms, N, ev, hidden)
    mask = np.zeros(ev.shape, dtype=bool)
    mask[:, hidden] = True
    for kw in (dict(), dict(log_p=False)):
        a = uniform(terms, N, ev, hidden, **kw)
        b = masked(terms, N, ev, mask, **kw)
        assert np.array_equal(b[0][:, hidden], a[0]) and np.array_equal(b[1], a[1])
        assert (a[2] is None and b[2] is None) or np.array_equal(b[2], a[2])
        visible = [i for i in range(N) if i not in hidden]
        assert np.array_equal(b[0][:, visible], ev[:, visible])


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
    want = cond_mode_masked(terms, N, ev, mask)
    holes = mask.any(axis=1)
    assert (~holes).sum() == 9 and want[3][holes].min() > GAP
    got = masked(terms, N, ev, mask)
    assert np.array_equal(got[0], want[0])
    errs = (float(np.abs(got[1] - want[1]).max()), float(np.abs(got[2] - want[2]).max()))
    print(f"a hidden set per row: errors: energy {errs[0]:.1e}, log_p {errs[1]:.1e}; tolerance {tol(terms):.1e}")
    assert max(errs) <= tol(terms)
    assert np.array_equal(got[0][~holes], ev[~holes]) and np.all(got[2][~holes] == 0.0)  # a row without holes: itself, probability 1


def test_permuted_rows_permute_the_results():
    terms, ev, mask = ragged_case()
    perm = np.random.default_rng(5).permutation(len(ev))
    a, b = masked(terms, N, ev, mask), masked(terms, N, ev[perm], mask[perm])
    for x, y in zip(a, b):
        assert np.array_equal(x[perm], y)


def test_too_many_holes_are_refused_by_row():
    terms = {(i, i + 1): 0.2 for i in range(1, 30)}
    ev = random_rows(3, 30, 1)
    mask = np.zeros(ev.shape, dtype=bool)
    mask[1, :25] = True
    mask[0, :24] = True
    with pytest.raises(gml.GMLError, match="row 1 hides 25 spins"):
        masked(terms, 30, ev, mask)


# 4. the joint mode is not the spin-by-spin decision
def test_mode_differs_from_the_signs_of_the_means():
    n, hidden = 8, [0, 2, 3, 5, 6]
    terms, ev = cond_model(n, seed=1000, triples=4), random_rows(16, n, 0)
    st, en, lp, gap = cond_mode_rows(terms, n, ev, hidden)
    means = cond_exact_rows(terms, n, ev, hidden)[0]
    differ = [k for k in range(len(ev)) if not np.array_equal(np.where(means[k] >= 0, 1, -1), st[k])]
    assert differ and gap.min() > GAP and float(np.abs(means).min()) > 1e-6  # on the reference: some rows differ, none is a toss-up
    got = uniform(terms, n, ev, hidden)
    check(got, (st, en, lp, gap), terms, "mode against marginals")
    res = gml.conditional_means(terms, np.hstack([np.ones((len(ev), 1)), ev]), [i + 1 for i in hidden], method=gml.Exact())
    assert [k for k in range(len(ev)) if not np.array_equal(np.where(res.means[k] >= 0, 1, -1), got[0][k])] == differ
    mode = gml.conditional_mode(terms, np.hstack([np.ones((len(ev), 1)), ev]), [i + 1 for i in hidden])
    assert isinstance(mode, gml.ConditionalMode) and np.array_equal(mode.states, got[0]) and np.array_equal(mode.log_p, got[2])
    assert mode.hidden == [i + 1 for i in hidden] and np.array_equal(mode.energy, got[1])


# 5. an exact tie goes to the lower state: a hidden spin in no term comes out +1
def test_hidden_spin_in_no_term_is_plus_one():
    terms = {(1, 2): 0.4, (2, 3): -0.3, (3,): 0.2, (1, 5): 0.25}
    ev = -np.ones((40, 6), dtype=np.int8)  # (the evidence holds -1 on the free spins: what it holds there plays no part)
    ev[:, :3] = random_rows(40, 3, 3)
    for hidden in ([1, 3, 5], [3], [0, 1, 2, 3, 4, 5]):
        st, en, lp = uniform(terms, 6, ev, hidden)
        want = cond_mode_rows(terms, 6, ev, hidden)
        assert np.array_equal(st, want[0]) and np.all(st[:, [hidden.index(i) for i in (3, 5) if i in hidden]] == 1)
        assert float(np.abs(en - want[1]).max()) <= tol(terms) and float(np.abs(lp - want[2]).max()) <= tol(terms)


# 6. the chunk hook: 13 hidden spins at 8 chunk bits, 32 chunks per row
def test_chunk_hook():
    terms, ev, hidden, want = case(13)
    try:
        assert _lib.lib().gml_test_exact_chunk_bits(8) >= 0
        for kw in (dict(), dict(log_p=False)):
            got = uniform(terms, N, ev, hidden, **kw)
            assert np.array_equal(got[0], want[0]) and float(np.abs(got[1] - want[1]).max()) <= tol(terms)
            assert got[2] is None or float(np.abs(got[2] - want[2]).max()) <= tol(terms)
    finally:
        _lib.lib().gml_test_exact_chunk_bits(0)


# 7. the front door for data with holes
def test_impute_mode():
    terms, ev, mask = ragged_case()
    samples = np.hstack([np.ones((len(ev), 1)), np.where(mask, 0, ev)])
    res = gml.impute_mode(terms, samples)
    want = cond_mode_masked(terms, N, ev, mask)
    assert isinstance(res, gml.ImputedMode) and res.completed.dtype == np.int8 and np.array_equal(res.missing, mask)
    assert np.array_equal(res.completed[~mask], ev[~mask]) and np.array_equal(res.completed, want[0])
    assert float(np.abs(res.energy - want[1]).max()) <= tol(terms) and float(np.abs(res.log_p - want[2]).max()) <= tol(terms)
