"""gml_problem_create_mcmc_terms_tempered without a GPU: exported, every GML_EINVAL / GML_EUNSUPPORTED case rejected before any device
work, the TemperedTermChains / Problem argument errors and defaults.  The numpy restatement of the ladder is checked for its
invariants and, on a model with two wells, against exact enumeration: the rule is right, not merely matched."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

import gml_amd as gml
from _term_chains_reference import chains as ref_chains
from _tempered_reference import bimodal_16, exact_moments, tempered

SO = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "libgml_hip.so")


@pytest.fixture(scope="module")
def cdll():
    if not os.path.exists(SO):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(SO)
    L.gml_problem_create_mcmc_terms_tempered.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                                         C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int,
                                                         C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    L.gml_problem_destroy.argtypes = [C.c_void_p]
    L.gml_last_error.restype = C.c_char_p
    return L


KEYS = np.array([[0, 1, -1], [1, 2, 0], [2, -1, -1]], dtype=np.int32)  # (1,2), (2,3,1), (3,) 0-based
WTS = np.array([0.3, -0.2, 0.5])


def _call(L, keys=KEYS, wts=WTS, n=3, ladders=8, spc=2, burn_in=3, thin=2, betas=(1.0, 0.5), replicas=None, swap_every=1, histogram=0,
          order=3, node0=0, node1=None, stride=None, null_keys=False, null_wts=False, null_betas=False):
    keys = np.ascontiguousarray(keys, dtype=np.int32)
    wts = np.ascontiguousarray(wts, dtype=np.float64)
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    R = len(betas) if replicas is None else replicas
    counts = np.zeros((2, 64), dtype=np.int64)
    h = C.c_void_p()
    rc = L.gml_problem_create_mcmc_terms_tempered(None if null_keys else keys.ctypes.data_as(C.c_void_p),
                                                  keys.shape[1] if stride is None else stride,
                                                  None if null_wts else wts.ctypes.data_as(C.c_void_p), len(wts), n, ladders, spc,
                                                  burn_in, thin, None if null_betas else betas.ctypes.data_as(C.c_void_p), R,
                                                  swap_every, 1, histogram, order, node0, n if node1 is None else node1, 0,
                                                  counts.ctypes.data_as(C.c_void_p), C.byref(h))
    msg = L.gml_last_error().decode()
    if h.value:
        L.gml_problem_destroy(h)
    return rc, msg


def test_exported(cdll):
    assert hasattr(cdll, "gml_problem_create_mcmc_terms_tempered")


EINVAL = {
    # what gml_problem_create_mcmc_terms_chains rejects, ladders in the place of chains
    "null_keys": dict(null_keys=True), "null_weights": dict(null_wts=True), "stride0": dict(stride=0),
    "spin_high": dict(keys=[[0, 3, -1], [1, 2, 0], [2, -1, -1]]), "spin_low": dict(keys=[[0, -2, -1], [1, 2, 0], [2, -1, -1]]),
    "nan": dict(wts=[0.3, np.nan, 0.5]), "inf": dict(wts=[0.3, -0.2, -np.inf]),
    "ladders": dict(ladders=0), "spc": dict(spc=0), "burn_in": dict(burn_in=0), "thin": dict(thin=0),
    "sweeps_overflow": dict(burn_in=2 ** 31 - 1, spc=2, thin=1), "samples_overflow": dict(ladders=2 ** 40, spc=2),
    "order0": dict(order=0), "order9": dict(order=9), "node0": dict(node0=-1), "node1": dict(node1=4),
    "empty_range": dict(node0=2, node1=2), "n0": dict(n=0),
    # the ladder
    "null_betas": dict(null_betas=True), "replicas0": dict(replicas=0), "replicas3": dict(betas=(1.0, 0.5, 0.2)),
    "replicas128": dict(betas=np.linspace(1.0, 0.1, 128)), "replicas_negative": dict(replicas=-2),
    "beta_nan": dict(betas=(1.0, np.nan)), "beta_inf": dict(betas=(np.inf, 1.0)), "beta_negative": dict(betas=(1.0, -0.1)),
    "beta_increasing": dict(betas=(1.0, 0.3, 0.5, 0.1)), "beta0_zero": dict(betas=(0.0, 0.0)), "beta0_zero_single": dict(betas=(0.0,)),
    "swap_every0": dict(swap_every=0), "swap_every_negative": dict(swap_every=-1),
    "lanes_overflow": dict(ladders=2 ** 40, spc=1, betas=(1.0, 0.5)),
}


@pytest.mark.parametrize("case", sorted(EINVAL))
def test_einval_before_device_work(cdll, case):
    rc, msg = _call(cdll, **EINVAL[case])
    assert rc == 1, (case, rc, msg)  # GML_EINVAL, not GML_EHIP: nothing reached the device
    assert "HIP" not in msg


def test_limits_named_before_device_work(cdll):
    rc, msg = _call(cdll, n=16385)
    assert rc == 5 and "n <= 16384" in msg and "HIP" not in msg, msg  # GML_EUNSUPPORTED
    rc, msg = _call(cdll, n=65, histogram=1)
    assert rc == 5 and "n <= 64" in msg and "HIP" not in msg, msg
    nine = np.arange(9, dtype=np.int32)[None, :]
    rc, msg = _call(cdll, keys=nine, wts=[0.1], n=9)
    assert rc == 5 and "at most 8" in msg and "HIP" not in msg, msg
    rc, msg = _call(cdll, keys=nine, wts=[0.0], n=9)  # zero weights are skipped
    assert rc != 5, msg
    for betas in ((1.0,), (2.0, 2.0), (1.0, 0.0), tuple(np.linspace(1.0, 0.0, 64))):  # equal betas and a last beta of 0 are ladders
        rc, msg = _call(cdll, betas=betas)
        assert rc not in (1, 5), (betas, rc, msg)


def test_incidence_limit_named_before_device_work(cdll):
    K = 1 << 24
    keys = np.zeros((K, 2), dtype=np.int32)
    keys[:, 1] = 1
    rc, msg = _call(cdll, keys=keys, wts=np.full(K, 1e-3), n=2)
    assert rc == 5 and "2^24" in msg and "HIP" not in msg, msg


def test_python_layer_errors_and_defaults():
    terms = {(1, 2, 3): 0.5, (1,): 0.1, (2, 3): -0.2}
    with pytest.raises(ValueError, match="multiple of samples_per_chain"):
        gml.sample(terms, 10, sampler=gml.TemperedTermChains(samples_per_chain=4))
    with pytest.raises(gml.GMLError, match="multiple of mcmc_samples_per_chain"):
        gml.Problem(terms=terms, n=3, num_samples=10, mcmc_sweeps=5, mcmc_samples_per_chain=4, mcmc_betas=[1.0, 0.5])
    with pytest.raises(gml.GMLError, match="mcmc_sweeps"):
        gml.Problem(terms=terms, n=3, num_samples=10, mcmc_betas=[1.0, 0.5])
    for kw in (dict(model=np.zeros((3, 3))), dict(spins=np.ones((4, 3), dtype=np.int8)), dict(samples=np.ones((4, 4)))):
        with pytest.raises(gml.GMLError, match="terms="):
            gml.Problem(num_samples=10, mcmc_sweeps=5, mcmc_betas=[1.0, 0.5], **kw)
    for bad in ([1.0, 0.5, 0.2], [0.5, 1.0], [0.0, 0.0], [1.0, float("nan")]):  # the library's own check, before any device work
        with pytest.raises(gml.GMLError) as e:
            gml.Problem(terms=terms, n=3, num_samples=10, mcmc_sweeps=5, mcmc_betas=bad)
        assert e.value.code == 1 and "HIP" not in str(e.value)
    with pytest.raises(gml.GMLError, match="swap_every"):
        gml.Problem(terms=terms, n=3, num_samples=10, mcmc_sweeps=5, mcmc_betas=[1.0, 0.5], mcmc_swap_every=0)
    s = gml.TemperedTermChains()
    assert (s.burn_in, s.thin, s.samples_per_chain, s.replicas, s.swap_every) == (200, 10, 1, 8, 1) and isinstance(s, gml.GMSampler)
    assert s.betas == [0.1 ** (r / 7) for r in range(8)] and s.betas[0] == 1.0 and s.swap_rates is None
    assert gml.TemperedTermChains(replicas=1).betas == [1.0]
    assert gml.TemperedTermChains(replicas=4, beta_min=0.2).betas == [0.2 ** (r / 3) for r in range(4)]
    s = gml.TemperedTermChains(betas=(2.0, 1.0), swap_every=3)
    assert s.betas == [2.0, 1.0] and s.replicas == 2 and s.swap_every == 3
    assert "TemperedTermChains" in gml.__all__


def _model(n, seed):
    rng = np.random.default_rng(seed)
    terms = [((int(i), int(j), int(k)), float(rng.normal(scale=0.3)))
             for i, j, k in (rng.choice(n, 3, replace=False) + 1 for _ in range(30))]
    terms += [((int(i), int(j)), float(rng.normal(scale=0.3))) for i, j in (rng.choice(n, 2, replace=False) + 1 for _ in range(20))]
    fields = [((i + 1,), float(rng.normal(scale=0.2))) for i in range(n)]
    return terms, fields


def test_one_rung_at_beta_one_is_the_plain_chain():
    terms, fields = _model(12, 3)
    got, counts = tempered(terms + fields, 12, 200, 3, 5, 2, [1.0], 1, seed=9)
    assert counts.shape == (2, 0)
    assert np.array_equal(got, ref_chains(terms + fields, 12, 200, 3, 5, 2, seed=9))


@pytest.mark.parametrize("swap_every", [1, 3])
def test_equal_betas_accept_every_attempt_and_attempts_follow_the_parity(swap_every):
    terms, fields = _model(12, 4)
    R, ladders, burn_in, thin, spc = 8, 37, 7, 3, 4
    _, counts = tempered(terms + fields, 12, ladders, spc, burn_in, thin, [0.7] * R, swap_every, seed=2)
    assert np.array_equal(counts[0], counts[1]) and counts[0].min() > 0
    _, counts = tempered(terms + fields, 12, ladders, spc, burn_in, thin, np.linspace(1.0, 0.0, R), swap_every, seed=2)
    rounds = (burn_in + (spc - 1) * thin) // swap_every  # round m = 1 .. rounds pairs the rungs r = m - 1 (mod 2)
    per_parity = [(rounds + 1) // 2, rounds // 2]
    assert counts[0].tolist() == [ladders * per_parity[r % 2] for r in range(R - 1)]
    assert (counts[1] <= counts[0]).all() and counts[1].sum() < counts[0].sum()


def test_restatement_ignores_the_order_of_coupling_terms():
    terms, fields = _model(12, 5)
    a = tempered(terms + fields, 12, 50, 3, 5, 2, [1.0, 0.6, 0.3, 0.1], 2, seed=9)
    perm = [terms[t] for t in np.random.default_rng(1).permutation(len(terms))]
    b = tempered(fields[:5] + perm + fields[5:], 12, 50, 3, 5, 2, [1.0, 0.6, 0.3, 0.1], 2, seed=9)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_first_ladders_do_not_depend_on_the_ladder_count():
    terms, fields = _model(12, 6)
    a, _ = tempered(terms + fields, 12, 40, 1, 6, 1, [1.0, 0.5], 1, seed=3)
    b, _ = tempered(terms + fields, 12, 15, 1, 6, 1, [1.0, 0.5], 1, seed=3)
    assert np.array_equal(a[:15], b)


def test_restatement_equilibrates_the_two_wells():
    terms = bimodal_16()
    ppos, mag0, corr0 = exact_moments(terms, 16)
    assert abs(ppos - 0.893) < 1e-3 and np.abs(mag0 - 0.786).max() < 0.02, (ppos, mag0)
    ladders = 2048
    s = gml.TemperedTermChains(burn_in=300, thin=1, samples_per_chain=1, replicas=8, beta_min=0.1)
    got, counts = tempered(terms, 16, ladders, 1, s.burn_in, s.thin, s.betas, s.swap_every, seed=1)
    x = got.astype(np.float64)
    bound = 6 / np.sqrt(ladders)  # a +-1 product has variance at most 1: six standard deviations at the least
    err_m, err_c = np.abs(x.mean(axis=0) - mag0).max(), np.abs(x.T @ x / ladders - corr0).max()
    print(f"restatement, {ladders} ladders: max error of a magnetisation {err_m:.4f}, of a pair correlation {err_c:.4f}, bound {bound:.4f}")
    assert err_m < bound and err_c < bound
    rates = counts[1] / counts[0]
    assert (rates > 0).all() and (rates < 1).all(), rates
