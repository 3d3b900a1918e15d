"""The conditional chains on the device (gml_problem_create_mcmc_terms_conditional, gml_conditional_means, the front door of
inference.py): states bit for bit and means to 1e-13 against the numpy restatement (always the full walk); every spin hidden against
the plain term-chain sampler; visible columns; independent of the chain tile, of the split of the field into a per-chain constant and
a live part, of the number of evidence rows and of the term order; the closed form for one hidden spin; enumeration; the front door;
errors and memory.  Shapes: word tails (n = 33, 12, 1), a partial wave and more than one tile, evidence rows across the 1024-row
padding of the sign bits, hidden spins in several state words, arities 1 to 7."""
import ctypes as C

import numpy as np
import pytest

import gml_amd as gml
from gml_amd import _lib
from _ais_reference import lattice, sparse_model
from _conditional_reference import (ENUM, check_enumeration, closed_form_bound, conditional, enum_model, exact_conditional, exact_field,
                                    random_rows)
from _high_order_cases import wide_terms

pytestmark = pytest.mark.gpu


def device_run(terms, n, evidence, hidden, replicas, spc, burn_in, thin, seed):
    """(states int8 [chains spc, n], means [chains, H]) of the two C entry points; evidence int8 [K, n] or an open Problem"""
    p = evidence if isinstance(evidence, gml.Problem) else gml.Problem(spins=evidence)
    try:
        with _lib.conditional_chains(terms, n, p, hidden, replicas, spc, burn_in, thin, seed) as q:
            states = q.spins()
            assert (q.K, q.M) == (p.K * replicas * spc, p.K * replicas * spc) and np.all(q.counts() == 1.0)
        means = _lib.conditional_chains(terms, n, p, hidden, replicas, spc, burn_in, thin, seed, means=True)
    finally:
        if p is not evidence:
            p.close()
    return states, means.T


def assert_matches_restatement(terms, n, ev, hidden, replicas, spc, burn_in, thin, seed):
    states, means = device_run(terms, n, ev, hidden, replicas, spc, burn_in, thin, seed)
    ref_states, ref_means = conditional(terms, n, ev, hidden, replicas, spc, burn_in, thin, seed)
    assert np.array_equal(states, ref_states)
    err = np.abs(means - ref_means).max()
    print(f"max |means - restatement| = {err:.2e}")
    # two exp implementations differ by a few ulp of a value <= 1: three orders of margin; the states themselves are equal
    assert means.shape == ref_means.shape and err < 1e-13


CASES = {
    "n33_four_hidden": lambda: (sparse_model(33, 6, 4, 0.3, 4), 33, 70, [0, 5, 31, 32], 2, 3, 5, 2),
    "lattice_16x16_every_third": lambda: (lattice(16, 0.4, 0.2, 1), 256, 1100, list(range(0, 256, 3)), 1, 2, 4, 2),
    "orders_5_to_8_cancelled_n12": lambda: (wide_terms(12, 5), 12, 65, [2, 3, 7], 2, 2, 3, 2),
    "n1": lambda: ({(1,): 0.3}, 1, 3, [0], 2, 2, 2, 1),
    "n33_all_but_one_hidden": lambda: (sparse_model(33, 6, 4, 0.3, 4), 33, 70, [i for i in range(33) if i != 16], 1, 2, 3, 2),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_bit_for_bit_against_the_restatement(case):
    terms, n, K, hidden, replicas, spc, burn_in, thin = CASES[case]()
    assert_matches_restatement(terms, n, random_rows(K, n, 0), hidden, replicas, spc, burn_in, thin, seed=11)


def test_counts_of_the_evidence_are_ignored():
    terms, n = sparse_model(33, 6, 4, 0.3, 4), 33
    rows = np.unique(random_rows(70, n, 0), axis=0)
    hist = np.concatenate([np.arange(2, 2 + len(rows))[:, None], rows.astype(np.int64)], axis=1)
    with gml.Problem(hist) as p:
        ev = p.spins()
        assert p.M > p.K and sorted(map(tuple, ev)) == sorted(map(tuple, rows))
        states, means = device_run(terms, n, p, [0, 5, 31, 32], 2, 3, 5, 2, seed=11)
    ref_states, ref_means = conditional(terms, n, ev, [0, 5, 31, 32], 2, 3, 5, 2, seed=11)
    assert np.array_equal(states, ref_states) and np.abs(means - ref_means).max() < 1e-13


def test_all_hidden_is_the_term_chain_sampler():
    terms, n, K, R = sparse_model(70, 6, 3, 0.3, 7), 70, 130, 3
    states, _ = device_run(terms, n, random_rows(K, n, 0), list(range(n)), R, 2, 6, 3, seed=17)
    with gml.Problem(terms=terms, n=n, num_samples=K * R * 2, mcmc_sweeps=6, mcmc_thin=3, mcmc_samples_per_chain=2, seed=17, order=3) as p:
        assert np.array_equal(states, p.spins())


def test_visible_columns_equal_the_evidence():
    terms, n, K, R, spc = sparse_model(70, 6, 3, 0.3, 7), 70, 130, 3, 2
    hid = [0, 31, 32, 64, 69]
    vis = [i for i in range(n) if i not in hid]
    ev = random_rows(K, n, 0)
    states, _ = device_run(terms, n, ev, hid, R, spc, 4, 2, seed=5)
    blocks = states.reshape(spc * R, K, n)  # (t, r)
    for block in blocks:
        assert np.array_equal(block[:, vis], ev[:, vis])
    assert not np.array_equal(blocks[0][:, hid], blocks[1][:, hid])  # the replicas are chains of their own


def hook(name):
    f = getattr(_lib.lib(), name)
    f.argtypes, f.restype = [C.c_int], C.c_int
    return f


def test_every_chain_tile_gives_the_same_bits():
    tile = hook("gml_test_term_chains_tile")
    terms, n, K = sparse_model(300, 6, 3, 0.3, 8), 300, 1100
    hid = list(range(1, n, 4))
    got = {}
    with gml.Problem(spins=random_rows(K, n, 0)) as p:
        try:
            for T in (64, 128, 256):
                assert tile(T) in (0, 64, 128, 256)
                got[T] = device_run(terms, n, p, hid, 3, 2, 3, 2, seed=3)
        finally:
            tile(0)
        got[0] = device_run(terms, n, p, hid, 3, 2, 3, 2, seed=3)
    for T in (128, 256, 0):
        assert np.array_equal(got[64][0], got[T][0]) and np.array_equal(got[64][1], got[T][1])
    assert np.unique(got[64][1]).size > 1000  # (the means are not trivially equal)


def dense_pairwise(n, seed):
    rng = np.random.default_rng(seed)
    terms = {(i + 1, j + 1): float(rng.normal(scale=1.0 / np.sqrt(n))) for i in range(n) for j in range(i + 1, n)}
    terms.update({(i + 1,): float(rng.normal(scale=0.2)) for i in range(n)})
    return terms


SPLIT_CASES = {
    # every record of a hidden spin names one other spin: const where that spin is visible, live where it is hidden
    "dense_pairwise_n70_9_hidden": lambda: (dense_pairwise(70, 2), 70, [3, 8, 30, 31, 32, 33, 50, 64, 69]),
    # order 3: records with two visible others (const), one hidden and one visible other, two hidden others (both live)
    "order3_n40_half_hidden": lambda: (sparse_model(40, 6, 3, 0.3, 2), 40, list(range(0, 40, 2))),
}


@pytest.mark.parametrize("case", sorted(SPLIT_CASES))
def test_split_of_the_field_gives_the_same_bits_as_the_full_walk(case):
    split = hook("gml_test_cond_split")
    terms, n, hid = SPLIT_CASES[case]()
    got = {}
    with gml.Problem(spins=random_rows(1100, n, 0)) as p:
        try:
            for on in (0, 1, 2):  # never, by the host's rule (the default), wherever a record allows it
                assert split(on) in (0, 1, 2)
                got[on] = device_run(terms, n, p, hid, 2, 3, 4, 2, seed=9)
        finally:
            split(1)
    for on in (1, 2):
        assert np.array_equal(got[0][0], got[on][0]) and np.array_equal(got[0][1], got[on][1])
    ref_states, ref_means = conditional(terms, n, random_rows(1100, n, 0), hid, 2, 3, 4, 2, seed=9)
    assert np.array_equal(got[2][0], ref_states) and np.abs(got[2][1] - ref_means).max() < 1e-13


def test_prefix_of_the_rows_and_term_order():
    terms, n, hid = sparse_model(70, 6, 3, 0.3, 7), 70, [0, 7, 31, 32, 33, 69]
    ev = random_rows(130, n, 0)
    full = device_run(terms, n, ev, hid, 1, 2, 4, 2, seed=17)
    part = device_run(terms, n, ev[:64], hid, 1, 2, 4, 2, seed=17)
    assert np.array_equal(full[0].reshape(2, 130, n)[:, :64], part[0].reshape(2, 64, n))
    assert np.array_equal(full[1][:64], part[1])
    # the same model with its terms shuffled (one field term per spin: a_i is an ordered FP64 sum) gives the same bits
    items = list(terms.items())
    perm = np.random.default_rng(1).permutation(len(items))
    other = device_run(dict(items[t] for t in perm), n, ev, hid, 1, 2, 4, 2, seed=17)
    assert np.array_equal(full[0], other[0]) and np.array_equal(full[1], other[1])


@pytest.mark.parametrize("i", [0, 17, 32])
def test_one_hidden_spin_is_tanh_of_its_field(i):
    terms, n = sparse_model(33, 6, 4, 0.3, 4), 33
    ev = random_rows(70, n, 0)
    want = np.tanh([exact_field(terms, n, row, i) for row in ev])
    bound = closed_form_bound(terms, n, i)
    for spc, burn_in, thin in ((1, 1, 1), (3, 5, 2), (4, 2, 7)):
        _, means = device_run(terms, n, ev, [i], 1, spc, burn_in, thin, seed=11)
        err = np.abs(means[:, 0] - want).max()
        print(f"spin {i}, spc {spc}: max |mean - tanh h| = {err:.2e}, bound {bound:.2e}")
        assert err <= bound


def test_enumeration():
    terms, ev = enum_model()
    states, means = device_run(terms, ENUM["n"], ev, ENUM["hidden"], ENUM["replicas"], 1, ENUM["burn_in"], 1, seed=ENUM["seed"])
    zc, zm = check_enumeration(terms, ev, states, means)
    print(f"worst cell z-score {zc:.2f}, worst mean z-score {zm:.2f}")


def test_front_door():
    terms, ev = enum_model()
    n, hid1 = ENUM["n"], [i + 1 for i in ENUM["hidden"]]
    sampler = gml.GlauberTermChains(burn_in=40, thin=1, samples_per_chain=1)
    hist = np.concatenate([np.arange(1, 7)[:, None], ev.astype(np.int64)], axis=1)
    cm = gml.conditional_means(terms, hist, hid1[::-1], sampler, replicas=5, seed=3)  # (any order in: ascending out)
    assert cm.means.shape == cm.stderr.shape == (6, 4) and cm.per_replica.shape == (5, 6, 4) and cm.hidden == hid1
    assert np.array_equal(cm.means, cm.per_replica.mean(axis=0))
    # (a hidden spin whose other spins are all visible has the same mean in every replica: its standard error is 0)
    assert np.array_equal(cm.stderr, cm.per_replica.std(axis=0, ddof=1) / np.sqrt(5)) and (cm.stderr > 0).any()
    assert sorted(cm.counts.tolist()) == [1, 2, 3, 4, 5, 6]
    one = gml.conditional_means(gml.FactorGraph(3, n, "spin", dict(terms)), hist, hid1, sampler, seed=3)
    assert np.isnan(one.stderr).all() and np.array_equal(one.means, cm.per_replica[0])
    # samples against Rao-Blackwellised means on a one-row evidence: the mean is E[s | the rest] of the very update that drew s, so
    # Var(s - mean) = Var(s) - Var(mean) <= 1 - m^2 with m the exact magnetisation: 6 sigma of the sample average bound the difference
    R = ENUM["replicas"]
    row = np.concatenate([[1], ev[0].astype(np.int64)])[None, :]
    with gml.conditional_sample(terms, row, hid1, sampler, replicas=R, seed=3) as q:
        assert (q.K, q.n) == (R, n)
        m, _ = q.moments(pairs=False)
    rb = gml.conditional_means(terms, row, hid1, sampler, replicas=R, seed=3)
    _, mag = exact_conditional(terms, n, ev[0], ENUM["hidden"])
    vis = [i for i in range(n) if i not in ENUM["hidden"]]
    assert np.array_equal(m[vis], ev[0][vis].astype(np.float64))
    z = np.abs(m[ENUM["hidden"]] - rb.means[0]) / np.sqrt((1 - mag ** 2) / R)
    print("sample moments against Rao-Blackwellised means, z:", z)
    assert z.max() < 6
    assert np.all(np.abs(rb.means[0] - mag) < 6 * rb.stderr[0])


def test_predictive_check_with_one_hidden_spin_is_deterministic():
    terms, n, i = sparse_model(33, 6, 4, 0.3, 4), 33, 17
    rows = np.unique(random_rows(200, n, 3), axis=0)
    counts = np.random.default_rng(4).integers(1, 9, size=len(rows))
    hist = np.concatenate([counts[:, None], rows.astype(np.int64)], axis=1)
    with gml.Problem(hist) as p:
        pc = gml.predictive_check(terms, p, [i + 1], gml.GlauberTermChains(burn_in=3, thin=2, samples_per_chain=2))
        data, w = p.spins(), p.counts() / p.M
    mean = np.tanh([exact_field(terms, n, row, i) for row in data])  # (the hidden spin's own value plays no part in its field)
    truth = data[:, i].astype(np.float64)
    accuracy = w @ (np.where(mean >= 0, 1.0, -1.0) == truth)
    log_loss = w @ -np.log((1 + truth * mean) / 2)
    print(f"accuracy {pc.accuracy[0]:.6f} (numpy {accuracy:.6f}), log-loss {pc.log_loss[0]:.12f} (numpy {log_loss:.12f})")
    assert pc.hidden == [i + 1] and pc.accuracy.shape == pc.log_loss.shape == (1,)
    assert pc.accuracy[0] == accuracy and abs(pc.log_loss[0] - log_loss) < 1e-9
    again = gml.predictive_check(terms, hist, [i + 1], gml.GlauberTermChains(burn_in=1, thin=1))  # a matrix: opened and closed
    assert again.accuracy[0] == accuracy and abs(again.log_loss[0] - log_loss) < 1e-9


EV_N = 12


def bad_call(code, match, terms=None, n=EV_N, hidden=(1, 5), means=False, **kw):
    terms = {(1, 2): 0.3, (3, 4, 5): -0.2, (6,): 0.1} if terms is None else terms
    args = dict(replicas=1, samples_per_chain=1, burn_in=2, thin=1)
    args.update(kw)
    with gml.Problem(spins=random_rows(5, EV_N, 0)) as p:
        with pytest.raises(gml.GMLError, match=match) as e:
            _lib.conditional_chains(terms, n, p, list(hidden), seed=1, means=means, **args)
    assert e.value.code == code, (e.value.code, str(e.value))


@pytest.mark.parametrize("means", [False, True], ids=["creator", "means"])
def test_errors(means):
    EINVAL, EUNSUPPORTED = _lib.GML_EINVAL, _lib.GML_EUNSUPPORTED
    bad_call(EINVAL, "no spin is hidden", hidden=(), means=means)
    bad_call(EINVAL, "differs from the evidence", n=EV_N + 1, means=means)
    bad_call(EINVAL, "replicas", replicas=0, means=means)
    bad_call(EINVAL, "at least 1", samples_per_chain=0, means=means)
    bad_call(EINVAL, "at least 1", burn_in=0, means=means)
    bad_call(EINVAL, "at least 1", thin=0, means=means)
    bad_call(EINVAL, "2\\^31 - 1 sweeps", samples_per_chain=2 ** 20, thin=2 ** 12, means=means)
    bad_call(EINVAL, "too large", samples_per_chain=2 ** 40, means=means)
    bad_call(EINVAL, "not finite", terms={(1, 2): np.nan}, means=means)
    bad_call(EUNSUPPORTED, "at most 8", terms={tuple(range(1, 10)): 0.1}, means=means)
    if not means:
        with gml.Problem(spins=random_rows(5, EV_N, 0)) as p:
            with pytest.raises(gml.GMLError, match="node") as e:
                _lib.conditional_chains({(1, 2): 0.3}, EV_N, p, [1], node_range=(3, 2))
        assert e.value.code == EINVAL


# Two faults at once, on handles with rows: the checks that follow the chain arguments (no hidden spin, term values, n limit, incidence
# limits), which a size-only stub cannot reach (tests/test_host_chain_refusal_order.py has the ones before).  Each case names two
# neighbours of the sequence; the answers were recorded from the library before the host half of the family moved to its own file.
NINE = {tuple(range(1, 10)): 0.1}
BIG_N = 20000  # above the kernels' 16384 spins
TWO_FAULTS = {
    "thin 0 + no hidden spin": dict(terms={(1, 2): 0.3}, n=EV_N, hidden=(), thin=0),
    "no hidden spin + non-finite weight": dict(terms={(1, 2): np.nan}, n=EV_N, hidden=()),
    "no hidden spin + nine distinct spins": dict(terms=NINE, n=EV_N, hidden=()),
    "non-finite weight + n above the limit": dict(terms={(1, 2): np.nan}, n=BIG_N, hidden=(1, 5)),
    "key out of range + n above the limit": dict(terms={(1, BIG_N + 5): 0.3}, n=BIG_N, hidden=(1, 5)),
    "n above the limit + nine distinct spins": dict(terms=NINE, n=BIG_N, hidden=(1, 5)),
}
EXPECTED_TWO_FAULTS = {
    'key out of range + n above the limit':
        (1, 'libgml_hip error 1: term 0 names spin 20004 outside [0,20000)'),
    'n above the limit + nine distinct spins':
        (5, 'libgml_hip error 5: the term-list chain kernel supports n <= 16384 spins (n = 20000)'),
    'no hidden spin + nine distinct spins':
        (1, 'libgml_hip error 1: no spin is hidden'),
    'no hidden spin + non-finite weight':
        (1, 'libgml_hip error 1: no spin is hidden'),
    'non-finite weight + n above the limit':
        (1, 'libgml_hip error 1: weight of term 0 is not finite'),
    'thin 0 + no hidden spin':
        (1, 'libgml_hip error 1: chains, samples_per_chain, burn_in and thin must be at least 1'),
}


def refusal(call, terms, n, second, means, **kw):
    """(code, text) of the refusal of call(terms, n, evidence, second(n), ...) on an evidence handle of 3 rows of n spins"""
    args = dict(replicas=1, samples_per_chain=1, burn_in=2, thin=1)
    args.update(kw)
    with gml.Problem(spins=np.ones((3, n), dtype=np.int8), node_range=(0, 1)) as p:
        with pytest.raises(gml.GMLError) as e:
            call(terms, n, p, second, seed=1, means=means, **args)
    return e.value.code, str(e.value)


@pytest.mark.parametrize("means", [False, True], ids=["creator", "means"])
@pytest.mark.parametrize("case", sorted(TWO_FAULTS))
def test_order_of_refusals_past_the_chain_arguments(case, means):
    kw = dict(TWO_FAULTS[case])
    got = refusal(_lib.conditional_chains, kw.pop("terms"), kw.pop("n"), list(kw.pop("hidden")), means, **kw)
    print(case, "->", got)
    assert got == EXPECTED_TWO_FAULTS[case]


def test_spin_limit_named():
    n = 16385
    with gml.Problem(spins=np.ones((2, n), dtype=np.int8), node_range=(0, 1)) as p:
        for means in (False, True):
            with pytest.raises(gml.GMLError, match="n <= 16384") as e:
                _lib.conditional_chains({(1, 2): 0.3}, n, p, [0], means=means)
            assert e.value.code == _lib.GML_EUNSUPPORTED


def test_incidence_limit_named():
    K = 1 << 24

    class Pairs:  # 2^24 copies of the pair (1, 2) as an array-backed term list (term_arrays takes keys_array / weights)
        weights, varible_count, order = np.full(K, 1e-3), EV_N, 2

        def __len__(self):
            return K

        def keys_array(self, first, count):
            return np.tile(np.array([[1, 2]], dtype=np.int32), (count, 1))

    with gml.Problem(spins=random_rows(5, EV_N, 0)) as p:
        with pytest.raises(gml.GMLError, match="2\\^24") as e:
            _lib.conditional_chains(Pairs(), EV_N, p, [0], means=True)
    assert e.value.code == _lib.GML_EUNSUPPORTED


def test_device_memory_returns():
    import torch
    terms, n = sparse_model(300, 6, 3, 0.3, 8), 300
    hid = list(range(0, n, 5))
    with gml.Problem(spins=random_rows(7000, n, 0)) as p:
        first = device_run(terms, n, p, hid, 10, 1, 2, 1, seed=1)
        torch.cuda.synchronize()
        _lib.trim_cache()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(20):
            again = device_run(terms, n, p, hid, 10, 1, 2, 1, seed=1)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
        _lib.trim_cache()
        free1 = torch.cuda.mem_get_info()[0]
    print("free bytes before / after:", free0, free1)
    assert free1 == free0
