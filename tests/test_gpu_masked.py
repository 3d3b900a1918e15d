"""The per-row masked conditional chains on the device (gml_problem_create_mcmc_terms_masked, gml_conditional_means_masked, the front door
of inference.py): states bit for bit and means to 1e-13 against the numpy restatement (_masked_reference.py); a shared mask against the
fixed-mask entry points bit for bit; independent of the chain tile; the closed form for one hidden spin per row; enumeration; the front
door; errors and memory.  Shapes: word tails (n = 33, 70, 1), a row without a hole and a row of holes only, waves whose unions have
whole zero words and differ from wave to wave, rows across the 1024-row padding of the sign bits, arities 1 to 7, the largest n."""
import ctypes as C

import numpy as np
import pytest

import gml_amd as gml
from gml_amd import _lib
from _ais_reference import lattice, sparse_model
from _conditional_reference import closed_form_bound, exact_field, random_rows
from _high_order_cases import wide_terms
from _masked_reference import ENUM, check_enumeration, enum_model, mask_rows, masked, random_mask

pytestmark = pytest.mark.gpu


class Handles:
    """evidence and mask as two open handles"""

    def __init__(self, ev, mask, **kw):
        self.ev, self.mask, self.kw = ev, mask, kw

    def __enter__(self):
        self.p = gml.Problem(spins=self.ev, **self.kw)
        self.m = gml.Problem(spins=mask_rows(self.mask), **self.kw)
        return self.p, self.m

    def __exit__(self, *a):
        self.m.close()
        self.p.close()


def run_on(p, m, terms, n, replicas, spc, burn_in, thin, seed, node_range=None):
    """(states int8 [chains spc, n], means [chains, n]) of the two C entry points on open handles"""
    with _lib.conditional_chains_masked(terms, n, p, m, replicas, spc, burn_in, thin, seed, node_range=node_range) as q:
        states = q.spins()
        assert (q.K, q.M) == (p.K * replicas * spc, p.K * replicas * spc) and np.all(q.counts() == 1.0)
    means = _lib.conditional_chains_masked(terms, n, p, m, replicas, spc, burn_in, thin, seed, means=True)
    return states, means.T


def device_run(terms, n, ev, mask, replicas, spc, burn_in, thin, seed):
    with Handles(ev, mask) as (p, m):
        return run_on(p, m, terms, n, replicas, spc, burn_in, thin, seed)


def assert_matches_restatement(terms, n, ev, mask, replicas, spc, burn_in, thin, seed):
    states, means = device_run(terms, n, ev, mask, replicas, spc, burn_in, thin, seed)
    ref_states, ref_means = masked(terms, n, ev, mask, replicas, spc, burn_in, thin, seed)
    assert np.array_equal(states, ref_states)
    err = np.abs(means - ref_means).max()
    print(f"max |means - restatement| = {err:.2e}")
    # two exp implementations differ by a few ulp of a value <= 1: three orders of margin; the states themselves are equal
    assert means.shape == ref_means.shape and err < 1e-13
    assert np.array_equal(means[~np.tile(mask, (replicas, 1))], ref_means[~np.tile(mask, (replicas, 1))])  # observed: exactly +-1


def mask_n33():
    mask = random_mask(70, 33, 0.3, 1)
    mask[3], mask[4] = False, True  # a row with nothing hidden, a row with everything hidden
    return mask


def mask_two_waves():
    """130 rows of 70 spins: rows 0 .. 63 (the first wave) hide spins of word 0 only, the others spins of word 2 only"""
    rng = np.random.default_rng(2)
    mask = np.zeros((130, 70), dtype=bool)
    mask[:64, :32] = rng.random((64, 32)) < 0.2
    mask[64:, 64:] = rng.random((66, 6)) < 0.5
    return mask


CASES = {
    "n33_independent_masks": lambda: (sparse_model(33, 6, 4, 0.3, 4), 33, 70, mask_n33(), 2, 3, 5, 2),
    "n70_two_waves_words_0_and_2": lambda: (sparse_model(70, 6, 3, 0.3, 7), 70, 130, mask_two_waves(), 1, 2, 4, 2),
    "lattice_16x16_1100_rows": lambda: (lattice(16, 0.4, 0.2, 1), 256, 1100, random_mask(1100, 256, 0.1, 3), 1, 2, 4, 2),
    "orders_5_to_8_cancelled_n12": lambda: (wide_terms(12, 5), 12, 65, random_mask(65, 12, 0.4, 4), 2, 2, 3, 2),
    "n1": lambda: ({(1,): 0.3}, 1, 3, np.array([[True], [False], [True]]), 2, 2, 2, 1),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_bit_for_bit_against_the_restatement(case):
    terms, n, K, mask, replicas, spc, burn_in, thin = CASES[case]()
    assert mask.shape == (K, n)
    assert_matches_restatement(terms, n, random_rows(K, n, 0), mask, replicas, spc, burn_in, thin, seed=11)


def test_the_largest_n():
    """n = 8192: state and mask of 64 chains fill the kernel's whole LDS budget"""
    n = 8192
    terms = {(1, 4096): 0.4, (4096, 8192): -0.3, (1, 33, 8192): 0.2, (1,): 0.1, (8192,): -0.2, (4096,): 0.05}
    ev = random_rows(3, n, 0)
    mask = np.zeros((3, n), dtype=bool)
    mask[0, [0, 8191]] = mask[1, [4095]] = mask[2, [0, 32, 4095, 8191]] = True
    with Handles(ev, mask, node_range=(0, 1)) as (p, m):
        states, means = run_on(p, m, terms, n, 2, 2, 2, 1, seed=5, node_range=(0, 1))
    ref_states, ref_means = masked(terms, n, ev, mask, 2, 2, 2, 1, seed=5)
    assert np.array_equal(states, ref_states) and np.abs(means - ref_means).max() < 1e-13


def hook(name):
    f = getattr(_lib.lib(), name)
    f.argtypes, f.restype = [C.c_int], C.c_int
    return f


def test_every_chain_tile_gives_the_same_bits():
    tile = hook("gml_test_term_chains_tile")
    terms, n, K = sparse_model(300, 6, 3, 0.3, 8), 300, 1100
    mask = random_mask(K, n, 0.25, 6)
    got = {}
    with Handles(random_rows(K, n, 0), mask) as (p, m):
        try:
            for T in (64, 128, 256):
                assert tile(T) in (0, 64, 128, 256)
                got[T] = run_on(p, m, terms, n, 3, 2, 3, 2, seed=3)
        finally:
            tile(0)
        got[0] = run_on(p, m, terms, n, 3, 2, 3, 2, seed=3)
    for T in (128, 256, 0):
        assert np.array_equal(got[64][0], got[T][0]) and np.array_equal(got[64][1], got[T][1])
    assert np.unique(got[64][1]).size > 1000  # (the means are not trivially equal)


@pytest.mark.parametrize("split", [0, 2])
def test_shared_mask_is_the_fixed_mask_entry_points(split):
    """every row of the mask the same vector: states and means of gml_problem_create_mcmc_terms_conditional / gml_conditional_means with
    that vector, array_equal on both, whether those split the field into a per-chain constant and a live part or not"""
    set_split = hook("gml_test_cond_split")
    terms, n, K = sparse_model(70, 6, 3, 0.3, 7), 70, 130
    hid = [0, 7, 31, 32, 33, 64, 69]
    mask = np.zeros((K, n), dtype=bool)
    mask[:, hid] = True
    ev = random_rows(K, n, 0)
    with Handles(ev, mask) as (p, m):
        states, means = run_on(p, m, terms, n, 2, 3, 4, 2, seed=9)
        try:
            assert set_split(split) in (0, 1, 2)
            with _lib.conditional_chains(terms, n, p, hid, 2, 3, 4, 2, 9) as q:
                fixed_states = q.spins()
            fixed_means = _lib.conditional_chains(terms, n, p, hid, 2, 3, 4, 2, 9, means=True).T
        finally:
            set_split(1)
    vis = [i for i in range(n) if i not in hid]
    assert np.array_equal(states, fixed_states)
    assert np.array_equal(means[:, hid], fixed_means)
    assert np.array_equal(means[:, vis], np.tile(ev[:, vis].astype(np.float64), (2, 1)))
    assert np.unique(fixed_means).size > 500


def test_one_hidden_spin_per_row_is_tanh_of_its_field():
    terms, n, K = sparse_model(33, 6, 4, 0.3, 4), 33, 70
    ev = random_rows(K, n, 0)
    which = np.arange(K) * 7 % n
    mask = np.zeros((K, n), dtype=bool)
    mask[np.arange(K), which] = True
    want = np.tanh([exact_field(terms, n, ev[k], int(which[k])) for k in range(K)])
    bound = np.array([closed_form_bound(terms, n, int(i)) for i in which])
    with Handles(ev, mask) as (p, m):
        for spc, burn_in, thin in ((1, 1, 1), (3, 5, 2), (4, 2, 7)):
            _, means = run_on(p, m, terms, n, 1, spc, burn_in, thin, seed=11)
            err = np.abs(means[np.arange(K), which] - want)
            print(f"spc {spc}: max |mean - tanh h| = {err.max():.2e}, bounds from {bound.min():.2e}")
            assert np.all(err <= bound)


def test_enumeration():
    terms, ev, mask = enum_model()
    states, means = device_run(terms, ENUM["n"], ev, mask, ENUM["replicas"], 1, ENUM["burn_in"], 1, seed=ENUM["seed"])
    zc, zm = check_enumeration(terms, ev, mask, states, means)
    print(f"worst cell z-score {zc:.2f}, worst mean z-score {zm:.2f}")


def test_front_door():
    terms, ev, mask = enum_model()
    n, K = ENUM["n"], ENUM["K"]
    sampler = gml.GlauberTermChains(burn_in=40, thin=1, samples_per_chain=1)
    counts = np.array([1, 2, 1, 3, 1, 1])
    hist = np.concatenate([counts[:, None], np.where(mask, 0, ev).astype(np.int64)], axis=1)
    rows = np.repeat(np.arange(K), counts)  # the expanded rows, in the caller's order
    from gml_amd.inference import _mask_order
    perm = _mask_order(mask[rows])  # the order the device runs them in: chain r 9 + j is expanded row perm[j]
    inverse = np.argsort(perm)
    assert sorted(perm) == list(range(9)) and not np.array_equal(perm, np.arange(9))
    im = gml.impute(terms, hist, sampler, replicas=5, seed=3)
    assert im.means.shape == im.stderr.shape == im.missing.shape == (9, n) and np.array_equal(im.missing, mask[rows])
    assert np.array_equal(im.means[~im.missing], ev[rows][~im.missing].astype(np.float64)) and np.all(im.stderr[~im.missing] == 0.0)
    assert np.abs(im.means[im.missing]).max() < 1.0 and (im.stderr[im.missing] > 0).any()
    ref_states, ref_means = masked(terms, n, ev[rows][perm], mask[rows][perm], 5, 1, 40, 1, seed=3)
    ref_means = ref_means.reshape(5, 9, n)[:, inverse]  # back in the caller's order
    assert np.abs(im.means - ref_means.mean(axis=0)).max() < 1e-13
    one = gml.impute(gml.FactorGraph(3, n, "spin", dict(terms)), hist, sampler, seed=3)
    assert np.isnan(one.stderr[one.missing]).all() and np.all(one.stderr[~one.missing] == 0.0)
    assert np.abs(one.means - ref_means[0]).max() < 1e-13
    with gml.impute_sample(terms, hist, sampler, replicas=5, seed=3) as q:
        assert (q.K, q.n) == (45, n) and np.all(q.counts() == 1.0)
        assert np.array_equal(q.spins().reshape(5, 9, n), ref_states.reshape(5, 9, n)[:, inverse])


EV_N = 12


def bad_call(code, match, terms=None, n=EV_N, means=False, mask_shape=(5, EV_N), **kw):
    terms = {(1, 2): 0.3, (3, 4, 5): -0.2, (6,): 0.1} if terms is None else terms
    args = dict(replicas=1, samples_per_chain=1, burn_in=2, thin=1)
    args.update(kw)
    with gml.Problem(spins=random_rows(5, EV_N, 0)) as p, gml.Problem(spins=mask_rows(random_mask(*mask_shape, 0.3, 1))) as m:
        with pytest.raises(gml.GMLError, match=match) as e:
            _lib.conditional_chains_masked(terms, n, p, m, seed=1, means=means, **args)
    assert e.value.code == code, (e.value.code, str(e.value))


@pytest.mark.parametrize("means", [False, True], ids=["creator", "means"])
def test_errors(means):
    EINVAL, EUNSUPPORTED = _lib.GML_EINVAL, _lib.GML_EUNSUPPORTED
    bad_call(EINVAL, "mask handle", mask_shape=(6, EV_N), means=means)  # another K
    bad_call(EINVAL, "mask handle", mask_shape=(5, EV_N + 1), means=means)  # another n
    bad_call(EINVAL, "differs from the evidence", n=EV_N + 1, means=means)
    bad_call(EINVAL, "replicas", replicas=0, means=means)
    bad_call(EINVAL, "at least 1", samples_per_chain=0, means=means)
    bad_call(EINVAL, "at least 1", burn_in=0, means=means)
    bad_call(EINVAL, "at least 1", thin=0, means=means)
    bad_call(EINVAL, "2\\^31 - 1 sweeps", samples_per_chain=2 ** 20, thin=2 ** 12, means=means)
    bad_call(EINVAL, "too large", samples_per_chain=2 ** 40, means=means)
    bad_call(EINVAL, "not finite", terms={(1, 2): np.nan}, means=means)
    bad_call(EUNSUPPORTED, "at most 8", terms={tuple(range(1, 10)): 0.1}, means=means)


# Two faults at once, on handles with rows: the checks that follow the chain arguments (term values, n limit, the masked tile,
# incidence limits), which a size-only stub cannot reach (tests/test_host_chain_refusal_order.py has the ones before).  Each case names
# two neighbours of the sequence; the answers were recorded from the library before the host half of the family moved to its own file.
NINE = {tuple(range(1, 10)): 0.1}
BIG_N = 20000  # above the chain kernels' 16384 spins, and so above the masked kernel's 8192 too
TWO_FAULTS = {
    "thin 0 + non-finite weight": dict(terms={(1, 2): np.nan}, n=EV_N, thin=0),
    "non-finite weight + n above the masked tile": dict(terms={(1, 2): np.nan}, n=8193),
    "key out of range + n above the limit": dict(terms={(1, BIG_N + 5): 0.3}, n=BIG_N),
    "n above the limit and the masked tile": dict(terms={(1, 2): 0.3}, n=BIG_N),
    "n above the limit + nine distinct spins": dict(terms=NINE, n=BIG_N),
    "n above the masked tile + nine distinct spins": dict(terms=NINE, n=8193),
}
EXPECTED_TWO_FAULTS = {
    'key out of range + n above the limit':
        (1, 'libgml_hip error 1: term 0 names spin 20004 outside [0,20000)'),
    'n above the limit + nine distinct spins':
        (5, 'libgml_hip error 5: the term-list chain kernel supports n <= 16384 spins (n = 20000)'),
    'n above the limit and the masked tile':
        (5, 'libgml_hip error 5: the term-list chain kernel supports n <= 16384 spins (n = 20000)'),
    'n above the masked tile + nine distinct spins':
        (5, 'libgml_hip error 5: the per-row masked chain kernel supports n <= 8192 spins (n = 8193)'),
    'non-finite weight + n above the masked tile':
        (1, 'libgml_hip error 1: weight of term 0 is not finite'),
    'thin 0 + non-finite weight':
        (1, 'libgml_hip error 1: chains, samples_per_chain, burn_in and thin must be at least 1'),
}


def refusal(terms, n, means, **kw):
    """(code, text) of the refusal on an evidence and a mask handle of 3 rows of n spins"""
    args = dict(replicas=1, samples_per_chain=1, burn_in=2, thin=1)
    args.update(kw)
    ones = np.ones((3, n), dtype=np.int8)
    with gml.Problem(spins=ones, node_range=(0, 1)) as p, gml.Problem(spins=-ones, node_range=(0, 1)) as m:
        with pytest.raises(gml.GMLError) as e:
            _lib.conditional_chains_masked(terms, n, p, m, seed=1, means=means, **args)
    return e.value.code, str(e.value)


@pytest.mark.parametrize("means", [False, True], ids=["creator", "means"])
@pytest.mark.parametrize("case", sorted(TWO_FAULTS))
def test_order_of_refusals_past_the_chain_arguments(case, means):
    kw = dict(TWO_FAULTS[case])
    got = refusal(kw.pop("terms"), kw.pop("n"), means, **kw)
    print(case, "->", got)
    assert got == EXPECTED_TWO_FAULTS[case]


def test_spin_limit_named():
    n = 8193  # one spin past the state and mask words of 64 chains that fit the kernel's LDS budget
    ones = np.ones((2, n), dtype=np.int8)
    with gml.Problem(spins=ones, node_range=(0, 1)) as p, gml.Problem(spins=ones, node_range=(0, 1)) as m:
        for means in (False, True):
            with pytest.raises(gml.GMLError, match="n <= 8192") as e:
                _lib.conditional_chains_masked({(1, 2): 0.3}, n, p, m, means=means)
            assert e.value.code == _lib.GML_EUNSUPPORTED


def test_device_memory_returns():
    import torch
    terms, n = sparse_model(300, 6, 3, 0.3, 8), 300
    with Handles(random_rows(3000, n, 0), random_mask(3000, n, 0.2, 2)) as (p, m):
        first = run_on(p, m, terms, n, 4, 1, 2, 1, seed=1)
        torch.cuda.synchronize()
        _lib.trim_cache()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(20):
            again = run_on(p, m, terms, n, 4, 1, 2, 1, seed=1)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
        _lib.trim_cache()
        free1 = torch.cuda.mem_get_info()[0]
    print("free bytes before / after:", free0, free1)
    assert free1 == free0
