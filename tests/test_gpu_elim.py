"""gml_model_elim on the device: exact log Z, means and term expectations by variable elimination, against the independent
np.longdouble sum-product of tests/_elim_reference.py (bucket elimination in a min-degree order with its adjoint pass).

The bound is derived, not measured.  L = sum |w| + n ln 2 bounds every log entry; a step adds at most T_t + 1 roundings from phi_t and
about four from max / exp / log / add, each of at most 2^-53 L: B = 2^-53 (T + 4 n) L for log Z, and 4 B + 1e-13 for means and term
expectations (the exponent of p_t carries three such errors, plus the sums).  Every case prints its measured errors before it asserts.

The models cover growth steps (lattices, Chimera), retire-only launches and retirements of more than three spins at once (the last
step of every wide component), slot reuse (one spin in, one out: lattices) and compaction (trees, the 3-regular graph); the models
without a field on every spin add introduce steps without terms and steps that neither apply a term nor retire a spin, where the
backward pass has nothing to sum and still has to hand beta on, and the forty islands many components in one call."""
import numpy as np
import pytest

import gml_amd as gml
import _elim_reference as R
from _exact_reference import LD, abs_weight

pytestmark = pytest.mark.gpu
_lib = gml._lib

CASES = {
    "lattice_4x4": lambda: R.lattice(4, 4, seed=3),
    "lattice_8x8": lambda: R.lattice(8, 8),
    "cylinder_3x6": lambda: R.lattice(3, 6, seed=5, periodic=True),
    "chimera_2": lambda: R.chimera(2),
    "chimera_3": lambda: R.chimera(3),    # width 16: tables of many workgroups, sums folded across them
    "regular3_60": lambda: R.regular3(60),
    "tree_200": lambda: R.tree(200),
    "ladder_64": lambda: R.triples_ladder(64),
    "order5": R.order5,
    "stiff_chain_60": R.stiff_chain,     # fields and couplings of +-150
    "mixed_conventions": R.mixed_conventions,
    "triples_only_12": R.triples_only,   # steps with no term and no retiring spin: nothing to sum backward, beta still handed on
    "islands_40": R.islands,             # 40 components and 10 free spins in one call: one upload, one set of tables, one sync
    "field_free_tree_40": lambda: R.tree(40, seed=6, field=False),
    "field_free_lattice_4x5": lambda: R.lattice(4, 5, seed=8, field=False),
}
_cache = {}


def reference(case):
    """(terms, n, the reference, B), computed once and shared"""
    if case not in _cache:
        terms, n = CASES[case]()
        _cache[case] = (terms, n, R.SumProduct(terms, n), R.bound(terms, n))
    return _cache[case]


def errors(got, ref):
    log_z, m, e = got
    seen = ~np.isnan(ref.texp)
    assert np.array_equal(np.isnan(e), ~seen)  # NaN exactly where the contract says so
    return float(abs(log_z - ref.log_z)), float(np.abs(m - ref.mean).max()), float(np.abs(e - ref.texp)[seen].max())


def shuffled_order(terms, n, seed):
    """another valid order: the greedy one with every second pair of consecutive steps swapped at random (a swap widens a scope by
    at most one spin; a wholly random order of a lattice is as wide as the lattice is large)"""
    order = _lib.model_elim_plan(terms, n)[0].copy()
    for i in np.flatnonzero(np.random.default_rng(seed).integers(0, 2, size=n // 2)):
        order[[2 * i, 2 * i + 1]] = order[[2 * i + 1, 2 * i]]
    return order


@pytest.mark.parametrize("case", sorted(CASES))
def test_against_the_reference(case):
    terms, n, ref, B = reference(case)
    _, width, work, stored = _lib.model_elim_plan(terms, n)
    got = _lib.model_elim(terms, n)
    dz, dm, de = errors(got, ref)
    print(f"{case}: n = {n}, T = {len(terms)}, width {width}, work {work:.3g}, log Z = {got[0]:.12f}; errors: log Z {dz:.1e} (B = {B:.1e}), "
          f"means {dm:.1e}, terms {de:.1e} (4 B + 1e-13 = {4 * B + 1e-13:.1e})")
    assert dz <= B and dm <= 4 * B + 1e-13 and de <= 4 * B + 1e-13
    # log Z alone (two tables taking turns, nothing stored) is the same forward pass: the same bits
    assert _lib.model_elim(terms, n, mean=False, texp=False)[0] == got[0]


@pytest.mark.parametrize("case", sorted(CASES))
def test_orders_agree(case):
    terms, n, ref, B = reference(case)
    greedy = _lib.model_elim(terms, n)
    orders = {"shuffled": shuffled_order(terms, n, seed=5)}
    if _lib.model_elim_plan(terms, n, np.arange(1, n + 1))[1] <= 20:
        orders["natural"] = np.arange(1, n + 1)
    for name, order in orders.items():
        width = _lib.model_elim_plan(terms, n, order)[1]
        assert width <= 20, (name, width)
        got = _lib.model_elim(terms, n, order)
        dz, dm, de = errors(got, ref)
        print(f"{case} / {name}: width {width}; errors: log Z {dz:.1e}, means {dm:.1e}, terms {de:.1e}")
        assert dz <= B and dm <= 4 * B + 1e-13 and de <= 4 * B + 1e-13
        seen = ~np.isnan(got[2])
        assert abs(got[0] - greedy[0]) <= 2 * B
        assert np.abs(got[1] - greedy[1]).max() <= 2 * (4 * B + 1e-13)
        assert np.abs(got[2] - greedy[2])[seen].max() <= 2 * (4 * B + 1e-13)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("case", ["triples_only_12", "field_free_tree_40", "field_free_lattice_4x5", "regular3_60"])
def test_really_permuted_orders(case, seed):
    """A wholly random permutation (for the 60-spin graph: the perturbed greedy order, which has steps of this kind too) of a model
    without fields: spins enter with no processed neighbour, so there are introduce steps without terms, steps that neither apply a
    term nor retire a spin (no quantity to sum backward), growth well beyond the greedy width and retirements of several spins."""
    terms, n, ref, B = reference(case)
    order = shuffled_order(terms, n, seed=9) if case == "regular3_60" else np.random.default_rng(seed).permutation(n) + 1
    seq, width, _, _ = _lib.model_elim_plan(terms, n, order)
    assert width <= 24, width
    # the shapes this test is about are there: restated from the order, the steps that apply no term and retire no spin
    adj = R.neighbours(terms, n)
    pos = {v: t for t, v in enumerate(seq)}
    last = {v: max([pos[v]] + [pos[u] for u in adj[v]]) for v in seq}
    applied = {max(pos[v] for v in R.reduce_key(k)) for k, w in terms.items() if w != 0.0 and R.reduce_key(k)}
    idle = [t for t in range(n) if t not in applied and t not in last.values()]
    got = _lib.model_elim(terms, n, order)
    dz, dm, de = errors(got, ref)
    print(f"{case} / permutation {seed}: width {width}, {len(idle)} steps without quantities; errors: log Z {dz:.1e}, means {dm:.1e}, "
          f"terms {de:.1e} (B = {B:.1e})")
    assert len(idle) > 0
    assert dz <= B and dm <= 4 * B + 1e-13 and de <= 4 * B + 1e-13


@pytest.mark.parametrize("case", ["chimera_3", "tree_200", "mixed_conventions"])
def test_same_arguments_same_bytes(case):
    terms, n, _, _ = reference(case)
    order = shuffled_order(terms, n, seed=9)
    for o in (None, order):
        a, b = _lib.model_elim(terms, n, o), _lib.model_elim(terms, n, o)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_field_free_tree_closed_forms():
    terms, n = R.tree(150, seed=4, field=False)
    J = np.array(list(terms.values()), dtype=LD)
    log_z, m, e = _lib.model_elim(terms, n)
    B = R.bound(terms, n)
    want = n * np.log(LD(2)) + np.sum(np.log(np.cosh(J)))
    print(f"field-free tree: log Z error {float(abs(log_z - want)):.1e} (B = {B:.1e}), means {np.abs(m).max():.1e}, "
          f"edges {float(np.abs(e - np.tanh(J)).max()):.1e}")
    assert abs(log_z - want) <= B
    assert np.abs(m).max() <= 4 * B + 1e-13 and np.abs(e - np.tanh(J)).max() <= 4 * B + 1e-13


def test_chimera_2_against_the_enumeration():
    terms, n, ref, B = reference("chimera_2")
    log_z, m, e = _lib.model_elim(terms, n)
    xz, xm, _, xe = _lib.model_exact(terms, n, queries=terms, pairs=False)
    tol = 1e-12 * max(1.0, abs_weight(terms))  # (the enumeration's own tolerance, tests/test_gpu_exact.py)
    assert abs(log_z - xz) <= B + tol
    assert np.abs(m - xm).max() <= 4 * B + 1e-13 + tol and np.abs(e - xe).max() <= 4 * B + 1e-13 + tol


def _data(n, seed, rows=300):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(1, 5, size=(rows, 1)), rng.choice([-1, 1], size=(rows, n))], axis=1).astype(np.float64)


def test_log_likelihood_equals_exact_on_chimera_2():
    terms, n, ref, B = reference("chimera_2")
    data = _data(n, 1)
    a, b = gml.log_likelihood(data, terms, gml.Elimination()), gml.log_likelihood(data, terms, gml.Exact())
    tol = 1e-12 * max(1.0, abs_weight(terms))
    assert a.data_term == b.data_term and a.stderr == 0.0
    assert abs(a.log_z - b.log_z) <= B + tol and abs(a.mean - b.mean) <= B + tol + 1e-15 * abs(a.data_term)
    assert gml.log_partition(terms, gml.Elimination()).log_z == a.log_z
    mp = gml.most_probable_states(terms, 2, log_prob=True, method=gml.Elimination())
    assert np.array_equal(mp.log_p, mp.energy - a.log_z)


def test_log_likelihood_of_the_8x8_lattice():
    terms, n, ref, B = reference("lattice_8x8")  # 64 spins in one component: Exact() refuses it
    with pytest.raises(_lib.GMLError):
        gml.log_partition(terms, gml.Exact())
    ll = gml.log_likelihood(_data(n, 2), terms, gml.Elimination())
    want = LD(ll.data_term) - ref.log_z
    assert abs(ll.mean - want) <= B + 2.0 ** -52 * abs(float(want)) and ll.stderr == 0.0
    assert abs(gml.observed_log_likelihood(_data(n, 2), terms, gml.Elimination()).log_z - ref.log_z) <= B


def test_model_term_moments_both_ways_on_chimera_2():
    terms, n, ref, B = reference("chimera_2")
    (m1, e1), (m2, e2) = gml.model_term_moments(terms, gml.Elimination()), gml.model_term_moments(terms)
    tol = 1e-12 * max(1.0, abs_weight(terms))
    assert len(e1) == len(e2) == len(terms)
    assert np.abs(m1 - ref.mean).max() <= 4 * B + 1e-13 and np.abs(e1 - ref.texp).max() <= 4 * B + 1e-13
    assert np.abs(m2 - ref.mean).max() <= tol and np.abs(e2 - ref.texp).max() <= tol
