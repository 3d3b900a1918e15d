"""gml_problem_create_sampled_elim on the device: exact draws of sparse models by backward sampling on the elimination's tables.

Draw for draw: the rows of the handle `==` the rows of the numpy host model (tests/_elim_draw_reference.py), every row of every
case.  Plain equality is a fair demand because tests/test_host_elim_draw_reference.py has checked, on the CPU, that at these seeds no
sample's u total comes nearer to a running sum than 1000 (4 B + 1e-13) total, B the elimination's derived error bound: the device's
tables differ from the host model's by far less, so both make the same picks.

Then what does not lean on the host model of the draws: the rows are a pure function of (model, order, seed, k); 65 536 draws of the
8 x 8 lattice have the means and term expectations gml_model_elim computes; the draws of a stiff chain are ground states and a
ferromagnet below its transition comes out in both wells equally -- the two models a single-temperature chain gets wrong."""
import numpy as np
import pytest

import gml_amd as gml
import _elim_draw_reference as D
import _elim_reference as R

pytestmark = pytest.mark.gpu
_lib = gml._lib

CASES = D.draw_cases()
EQUAL = ["lattice_4x4", "ladder_14", "chimera_2", "order5", "mixed_conventions", "field_free_tree_200", "complete_7",
         "lattice_4x4_perturbed", "lattice_4x4_permuted"]
_host = {}


def host(case, N=None):
    """the host model's rows of a case, computed once and shared"""
    terms, n, order, seed, N0 = CASES[case]
    if case not in _host:
        _host[case] = D.draw(terms, n, N0, seed, order)[0]
    return _host[case][:N0 if N is None else N]


def device(case, N=None, seed=None, **kw):
    terms, n, order, seed0, N0 = CASES[case]
    return _lib.Problem(terms=terms, n=n, num_samples=N0 if N is None else N, seed=seed0 if seed is None else seed, elim=True,
                        elim_order=order, order=max(2, max(len(k) for k in terms)), **kw)


# ---- 1. draw for draw ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EQUAL)
def test_rows_equal_the_host_model(case):
    want = host(case)
    with device(case) as p:
        got = p.spins()
        assert (p.K, p.M) == (len(want), float(len(want))) and np.array_equal(p.counts(), np.ones(len(want)))
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).any(axis=1).sum())} of {len(want)} rows differ"


def test_the_cases_have_the_shapes_they_are_there_for():
    shape = {case: [len(L["rbit"]) for L in D.launch_list(*CASES[case][:3])[0]] for case in EQUAL}
    assert shape["complete_7"][-3:] == [3, 3, 1]                                   # tables between the launches of one step
    assert 0 in shape["lattice_4x4_permuted"] and 0 in shape["field_free_tree_200"]  # introduce-only launches
    assert D.launch_list(*CASES["mixed_conventions"][:3])[1] == [9]                 # a spin in no term
    assert all({1, 2, 3} <= set(shape[c]) for c in ("lattice_4x4", "chimera_2"))


# ---- 2. a pure function of (model, order, seed, k) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["chimera_2", "mixed_conventions"])
def test_same_arguments_same_bytes(case):
    with device(case) as a, device(case) as b:
        assert a.sign_bits().tobytes() == b.sign_bits().tobytes()  # (gml_problem_get_sign_bits)


@pytest.mark.parametrize("case", ["chimera_2", "mixed_conventions", "lattice_4x4_permuted"])
def test_rows_do_not_depend_on_N_or_on_the_histogram(case):
    want = host(case)
    with device(case, N=1000) as p:
        assert np.array_equal(p.spins(), want[:1000])
    if CASES[case][1] <= 64:
        with device(case, histogram=True) as p:
            states, counts = p.spins(), p.counts()
        assert p.M == len(want) and counts.sum() == len(want) and len(states) == len(np.unique(states, axis=0))
        rows, mult = np.unique(want, axis=0, return_counts=True)
        o1, o2 = np.lexsort(states.T[::-1]), np.lexsort(rows.T[::-1])
        assert np.array_equal(states[o1], rows[o2]) and np.array_equal(counts[o1], mult[o2])


def test_two_seeds_differ():
    with device("lattice_4x4") as a, device("lattice_4x4", seed=CASES["lattice_4x4"][3] + 1) as b:
        assert (a.spins() != b.spins()).any(axis=1).mean() > 0.9


# ---- 3. the right distribution, independently of the host model of draws ----------------------------------------------------------
def test_moments_of_the_8x8_lattice():
    """64 spins in one component: the enumerating sampler refuses it.  z = |sample mean - exact| / sqrt((1 - exact^2) / N) of the 64
    means and the 176 term expectations against gml_model_elim, all below 5 (the seed vetted on the host model's draws)."""
    terms, n, order, seed, N = CASES["lattice_8x8"]
    with pytest.raises(_lib.GMLError):
        _lib.Problem(terms=terms, n=n, num_samples=16, seed=1)
    _, mean, texp = _lib.model_elim(terms, n)
    with device("lattice_8x8") as p:
        m, _ = p.moments(pairs=False)
        e = p.term_moments(terms)
    exact, got = np.concatenate([mean, texp]), np.concatenate([m, e])
    z = np.abs(got - exact) / np.sqrt((1.0 - exact ** 2) / N)
    print(f"8 x 8 lattice, N = {N}: largest z over {len(z)} quantities = {z.max():.2f}")
    assert len(z) == 240 and z.max() < 5.0


# ---- 4. where chains fail ---------------------------------------------------------------------------------------------------------------
def test_stiff_chain_draws_are_ground_states():
    """fields and couplings of +-150: every state but the most probable ones has probability below e^-300.  The largest energy by
    dynamic programming along the chain (multiples of 150: exact in FP64)."""
    terms, n = R.stiff_chain()
    best = {s: terms[(1,)] * s for s in (1, -1)}
    for v in range(2, n + 1):
        best = {s: terms[(v,)] * s + max(best[q] + terms[(v - 1, v)] * q * s for q in (1, -1)) for s in (1, -1)}
    with _lib.Problem(terms=terms, n=n, num_samples=4096, seed=5, elim=True) as p:
        rows = p.spins()
    assert np.array_equal(D.energy(terms, rows), np.full(4096, max(best.values())))


def test_ferromagnet_is_drawn_in_both_wells():
    """a field-free 6 x 6 ferromagnet at J = 1: P(s) = P(-s) exactly, so the rows of positive total magnetisation are Binomial(N', 1/2)
    among the N' rows whose magnetisation is not 0.  Within 5 standard deviations."""
    terms, n, order, seed, N = CASES["ferromagnet_6x6"]
    with device("ferromagnet_6x6") as p:
        mag = p.spins().astype(np.int64).sum(axis=1)
    up, down, zero = int((mag > 0).sum()), int((mag < 0).sum()), int((mag == 0).sum())
    print(f"ferromagnet 6 x 6: {up} up, {down} down, {zero} with magnetisation 0; mean |m| = {np.abs(mag).mean() / n:.3f}")
    assert abs(up - (up + down) / 2) <= 5 * np.sqrt((up + down) / 4)
    assert np.abs(mag).mean() / n > 0.9  # (deep in the ordered phase: each row sits in one well)


# ---- 5. the front door ---------------------------------------------------------------------------------------------------------------
def test_sample_returns_the_rows_of_the_handle_and_learn_runs_on_it():
    terms, n = R.lattice(8, 8)
    hist = gml.sample(terms, 4096, sampler=gml.Elimination(), seed=3)
    with _lib.Problem(terms=terms, n=n, num_samples=4096, seed=3, elim=True) as p:
        rows, mult = np.unique(p.spins(), axis=0, return_counts=True)
        assert hist[:, 0].sum() == 4096 and np.array_equal(hist[:, 1:], rows) and np.array_equal(hist[:, 0], mult)
        out, kkt, stats = p.learn("RISE", 0.2)  # the handle is a handle like any other: learn() runs on it
    assert out.shape[0] == n and np.isfinite(out).all() and np.abs(out).max() > 0.05
