"""learn_path on the device: the loss table against an explicit loop over packed handles built from the numpy split
(tests/_split_reference.py), the final model against learn() at the chosen c, and what a cross-validated path must show on data with
structure -- the selected model beats the empty one, the support shrinks as c grows."""
import numpy as np
import pytest

import gml_amd as gml
import _split_reference as R

pytestmark = pytest.mark.gpu
synthetic = __import__("importlib").import_module("gml_amd.synthetic")

FOLDS, SEED = 4, 5
# lambda = c sqrt(log(n^2 / 0.05) / M) and every gradient entry at zero couplings is a correlation, at most 1 in magnitude: with n = 16
# and M = 3000 training samples lambda(25) = 1.33 >= 1 leaves every coupling at zero (the empty model)
CS = [25.0, 1.0, 0.4, 0.1, 0.02, 0.0]


@pytest.fixture(scope="module")
def data():
    spins, _ = synthetic.block_ising(n=16, K=4000, seed=0)
    return spins, np.concatenate([np.ones((len(spins), 1)), spins.astype(np.float64)], axis=1)


@pytest.fixture(scope="module")
def result(data):
    method = gml.HIP()
    return gml.learn_path(data[1], gml.RISE(0.4, True), CS, method, folds=FOLDS, seed=SEED), method


def test_loss_equals_the_explicit_loop(data, result):
    spins, _ = data
    res, _ = result
    K, n = spins.shape
    assert np.array_equal(res.cs, np.array(CS))
    loss = np.zeros((len(CS), FOLDS))
    supp = np.zeros((len(CS), FOLDS), dtype=np.int64)
    for f in range(FOLDS):
        _, tc, tb, tK = R.split(spins, np.ones(K), FOLDS, f, SEED, True)
        _, hc, hb, hK = R.split(spins, np.ones(K), FOLDS, f, SEED, False)
        with gml.Problem(packed=(tb, tc, tK)) as train, gml.Problem(packed=(hb, hc, hK)) as held:
            x = None
            for a, c in enumerate(CS):
                x, _, _ = train.learn("RISE", c, x0=x)
                loss[a, f] = held.objgrad("RISE", np.arange(n), x, want_grad=False)[0].sum()
                supp[a, f] = np.count_nonzero(x[~np.eye(n, dtype=bool)])
    assert np.array_equal(res.loss, loss)
    assert np.array_equal(res.support, supp)
    assert np.array_equal(res.mean, loss.mean(axis=1)) and np.array_equal(res.se, loss.std(axis=1, ddof=1) / np.sqrt(FOLDS))
    assert np.array_equal(res.stats["fold_sizes"], R.fold_sizes(np.ones(K), FOLDS, SEED))


def test_model_is_learn_at_the_chosen_c(data, result):
    res, method = result
    assert res.c == res.c_min == res.cs[int(np.argmin(res.mean))] and res.c_1se >= res.c_min
    assert np.array_equal(res.model, gml.learn(data[1], gml.RISE(res.c, True), gml.HIP()))
    assert method.stats["kkt"].shape == (16,)  # (the method carries the final solve's statistics, as after learn)


def test_selected_model_beats_the_empty_one(result):
    res, _ = result
    assert np.all(res.support[0] == 0)  # the largest c: no coupling survives, on any fold
    assert res.mean[int(np.argmin(res.mean))] < res.mean[0]
    assert res.c_min < res.cs[0]


def test_support_shrinks_as_c_grows(result):
    res, _ = result
    assert np.all(np.diff(res.support, axis=0) >= 0)  # (cs descend along axis 0)
    assert res.support[-1].max() <= 16 * 15
