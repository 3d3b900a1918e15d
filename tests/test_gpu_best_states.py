"""gml_model_best_states on the device: the k most probable states by streaming enumeration and selection, against brute force in
np.longdouble (tests/_best_reference.py) and against a closed form.
Tolerances: found exact; the states EQUAL to the reference's; every energy within 1e-12 max(1, sum_t |w_t|), the project's tolerance of
the exact enumerations (tests/test_gpu_exact.py).  Equal states are a condition, not a measurement: every test asserts on the reference
that the gaps among its best k + 1 energies exceed 1e-9 (exact ties -- a spin in no term, the pair s and -s of a model of even terms --
are decided by the tie rule instead, and are asserted to be exact)."""
import numpy as np
import pytest

import gml_amd as gml
from _best_reference import (best_states, chain_best_energies, code_of, reference, smallest_gap, spins_of)
from _exact_reference import LD, abs_weight, chain_model

pytestmark = pytest.mark.gpu
_lib = gml._lib
GAP = 1e-9


def tol(terms):
    return 1e-12 * max(1.0, abs_weight(terms))


class chunk_bits:
    """the test hook's chunk width for the body, the default again afterwards"""

    def __init__(self, c):
        self.c = c

    def __enter__(self):
        assert _lib.lib().gml_test_exact_chunk_bits(self.c) >= 0

    def __exit__(self, *a):
        _lib.lib().gml_test_exact_chunk_bits(0)


def check(name, k, what):
    """the device's k best of the model `name` against the reference's; returns (states, energies)"""
    terms, n, best = reference(name)
    want = best[:k]
    assert smallest_gap(best[:k + 1]) > GAP  # the condition: no ambiguity within the reference's best k + 1
    states, energies = _lib.model_best_states(terms, n, k)
    err = float(np.abs(energies - np.array([e for e, _ in want], dtype=LD)).max()) if len(energies) == len(want) else np.inf
    print(f"{what}: n = {n}, k = {k}, found = {len(energies)}, sum|w| = {abs_weight(terms):.1f}, smallest gap {smallest_gap(best[:k + 1]):.1e}, "
          f"energy error {err:.1e}; tolerance {tol(terms):.1e}")
    assert len(energies) == len(states) == len(want) == min(k, 1 << n)
    assert code_of(states) == [s for _, s in want]
    assert err <= tol(terms)
    return states, energies


# 1. against brute force: a partial chunk (1, 3, 11), exactly one chunk (12), two chunks (13), 64 chunks (18); k above 2^n at sb = 1, 3
@pytest.mark.parametrize("k", [1, 8, 64, 256])
@pytest.mark.parametrize("sb", [1, 3, 11, 12, 13, 18])
def test_against_brute_force(sb, k):
    check(f"two{sb}", k, "default chunk")


# 2. the chunk hook
@pytest.mark.parametrize("k", [1, 256])
def test_many_groups_and_chunks_per_group(k):
    # 18 spins at 4 chunk bits: 1024 groups of 16 chunks of 16 states, the cut over 1024 k candidates
    with chunk_bits(4):
        check("two18", k, "chunk bits 4")


@pytest.mark.parametrize("k", [1, 64])
def test_chunk_width_invariance(k):
    got = {}
    for c in (4, 8, 0):
        with chunk_bits(c):
            got[c] = check("ten", k, f"chunk bits {c or 'default'}")
    for c in (4, 8):
        assert np.array_equal(got[c][0], got[0][0])


# 3. degenerate pairs: a 24-spin open chain without fields at 2 chunk bits, 4096 chunks per group
def test_chain_pairs_against_closed_form():
    terms, J = chain_model(list(range(1, 25)), seed=24)
    want = chain_best_energies(J, 66)
    assert np.all(want[0:64:2] == want[1:64:2]) and float(np.min(want[1:65:2] - want[2:66:2])) > GAP
    with chunk_bits(2):
        states, energies = _lib.model_best_states(terms, 24, 64)
    err = float(np.abs(energies - want[:64]).max())
    print(f"24-spin chain, chunk bits 2, k = 64: energy error {err:.1e}; tolerance {tol(terms):.1e}")
    assert len(energies) == 64 and err <= tol(terms)
    codes = code_of(states)
    for a in range(0, 64, 2):  # s and -s: both there, bit-equal energies, in state order
        assert energies[a] == energies[a + 1] and codes[a] < codes[a + 1] and codes[a] ^ codes[a + 1] == (1 << 24) - 1
    # the states themselves: every bond satisfied but the subset whose sum is the energy's deficit
    e_of = np.array([sum(w * states[r, i - 1] * states[r, j - 1] for (i, j), w in terms.items()) for r in range(64)])
    assert float(np.abs(e_of - want[:64]).max()) <= tol(terms)


# 4. energies that ascend with the state: every chunk qualifies (16 states a chunk, 8 chunks a group)
def test_every_chunk_qualifies():
    with chunk_bits(4):
        check("ascending", 256, "ascending energies, chunk bits 4")


# 5. components: 1, 3, 13 and 20 spins and 13 spins in no term; the free spins' exact ties come out in state order
def test_components_and_free_spins():
    terms, n, best = reference("components")
    assert all(e == best[0][0] for e, _ in best)  # (2^13 exact ties at the top: the order is the tie rule's alone)
    states, energies = _lib.model_best_states(terms, n, 64)
    codes = code_of(states)
    assert codes == [s for _, s in best[:64]] and codes == sorted(codes)
    assert np.all(energies == energies[0]) and abs(energies[0] - best[0][0]) <= tol(terms)


def test_components_without_ties():
    # components of 13, 3 and 1 spins and no free spin: the merge's order of the sums against the reference's
    check("merged", 64, "three components")


# 6. determinism
@pytest.mark.parametrize("k", [1, 256])
def test_two_calls_give_the_same_bytes(k):
    terms, n, _ = reference("two13")
    a, b = _lib.model_best_states(terms, n, k), _lib.model_best_states(terms, n, k)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# 7. consistency with the summing enumerator
def test_log_p_against_log_z():
    terms, n, best = reference("ten")
    log_z = _lib.model_exact(terms, n, pairs=False)[0]
    res = gml.most_probable_states(terms, 256, log_prob=True)
    assert len(res.energy) == 256 and res.log_p[0] == res.energy[0] - log_z and np.array_equal(res.log_p, res.energy - log_z)
    assert np.all(res.log_p <= 0.0)
    terms, n, best = reference("eight", 256)
    res = gml.most_probable_states(terms, 256, log_prob=True)
    total = float(np.exp(res.log_p.astype(LD)).sum())
    print(f"8 spins, all 256 states: sum exp(log_p) - 1 = {total - 1:.1e}; tolerance {tol(terms):.1e}")
    assert len(res.energy) == 256 and abs(total - 1.0) <= tol(terms) and np.all(res.log_p <= 0.0)
    assert sorted(code_of(res.states)) == list(range(256))


# 8. the front door
def test_front_door():
    terms, n, best = reference("two11")
    states, energies = _lib.model_best_states(terms, n, 8)
    for model in (terms, gml.FactorGraph(terms)):
        res = gml.most_probable_states(model, 8)
        assert isinstance(res, gml.MostProbable) and res.log_p is None
        assert np.array_equal(res.states, states) and np.array_equal(res.energy, energies)
    one = gml.most_probable_states(terms)
    assert one.states.shape == (1, n) and np.array_equal(one.states[0], spins_of([best[0][1]], n)[0])
