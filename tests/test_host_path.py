"""learn_path without a GPU: the four device steps (open / split / solve / score) and learn()'s node solver are substituted by the
numpy split (tests/_split_reference.py) and the CPU oracle on the golden c_samples.csv; what is checked is the orchestration -- the
order of the path, the warm starts, the loss table, the selection rules, the argument errors."""
import importlib

import numpy as np
import pytest

import gml_amd as gml
import _split_reference as R
from conftest import load_csv
from oracle import oracle as O

path_module = importlib.import_module("gml_amd.path")
learn_module = importlib.import_module("gml_amd.learn")

CS = [0.05, 0.8, 0.2, 3.0]  # (given unsorted on purpose)
FOLDS, SEED = 3, 17


class HostPart:
    def __init__(self, counts, spins):
        self.counts, self.spins, self.n = np.asarray(counts, dtype=np.float64), np.asarray(spins, dtype=np.int8), spins.shape[1]
        self.closed = False

    def fold_sizes(self, folds, seed=0):
        return R.fold_sizes(self.counts, folds, seed)

    def close(self):
        self.closed = True


class Recorder:
    """the substituted steps, recording what learn_path hands them"""

    def __init__(self, score_override=None):
        self.solves, self.parts, self.score_override = [], [], score_override

    def open(self, samples, order, device):
        counts, spins = O.split_histogram(samples)
        self.root = HostPart(counts, spins)
        return self.root

    def split(self, prob, folds, fold, seed):
        out = []
        for complement in (True, False):
            rows, cn, _, Kn = R.split(prob.spins, prob.counts, folds, fold, seed, complement)
            assert Kn > 0
            out.append(HostPart(cn, prob.spins[rows]))
        self.parts.append((fold, out[0], out[1]))
        return tuple(out)

    def solve(self, train, formulation, c, x0, method, structure):
        name = type(formulation).__name__
        x, _, st = O.learn_nodes_fast(train.counts, train.spins, np.arange(train.n), name, c=c, tol=method.tol)
        self.solves.append((train, c, None if x0 is None else np.array(x0), x))
        return x, st

    def score(self, held, score, rows):
        if self.score_override is not None:
            return self.score_override(held, rows)
        f, _ = O.objgrad_nodes(type(score).__name__, held.counts, held.spins, np.arange(held.n), rows, want_grad=False)
        return float(f.sum())


def oracle_local_solve(samples, formulation, method, order, node_range, device, **kw):
    assert not {k: v for k, v in kw.items() if v is not None}
    name = type(formulation).__name__
    Rm, kkt, _ = O.learn_pair(samples, name, c=formulation.regularizer, symmetrize=False)
    return Rm[node_range[0]:node_range[1]], kkt[node_range[0]:node_range[1]], {}


def run_path(rec, *args, **kw):
    old = (path_module._open_hip, path_module._split_hip, path_module._solve_hip, path_module._score_hip,
           learn_module._local_solve_hip, learn_module._symmetrize_hip)
    path_module._open_hip, path_module._split_hip, path_module._solve_hip, path_module._score_hip = rec.open, rec.split, rec.solve, rec.score
    learn_module._local_solve_hip, learn_module._symmetrize_hip = oracle_local_solve, lambda Rm, device: 0.5 * (Rm + Rm.T)
    try:
        return gml.learn_path(*args, **kw)
    finally:
        (path_module._open_hip, path_module._split_hip, path_module._solve_hip, path_module._score_hip,
         learn_module._local_solve_hip, learn_module._symmetrize_hip) = old


@pytest.fixture(scope="module")
def samples():
    return load_csv("c_samples.csv")


@pytest.fixture(scope="module")
def rise_run(samples):
    rec = Recorder()
    res = run_path(rec, samples, gml.RISE(0.4, True), CS, gml.HIP(tol=1e-9), folds=FOLDS, seed=SEED)
    return rec, res


def test_path_is_descending_and_warm_started(rise_run):
    rec, res = rise_run
    want = np.sort(np.array(CS))[::-1]
    assert np.array_equal(res.cs, want)
    assert len(rec.solves) == FOLDS * len(CS)
    for f in range(FOLDS):
        chunk = rec.solves[f * len(CS):(f + 1) * len(CS)]
        assert [c for _, c, _, _ in chunk] == want.tolist()
        assert all(t is rec.parts[f][1] for t, _, _, _ in chunk)  # every solve of the fold on its training part
        assert chunk[0][2] is None
        for a in range(1, len(CS)):
            assert np.array_equal(chunk[a][2], chunk[a - 1][3])  # x0 = the previous solution
    assert all(tr.closed and he.closed for _, tr, he in rec.parts) and rec.root.closed


def test_loss_table_and_selection_against_numpy(rise_run, samples):
    rec, res = rise_run
    counts, spins = O.split_histogram(samples)
    n = spins.shape[1]
    cs = np.sort(np.array(CS))[::-1]
    loss = np.zeros((len(cs), FOLDS))
    supp = np.zeros((len(cs), FOLDS), dtype=np.int64)
    for f in range(FOLDS):
        tr_rows, tr_c, _, _ = R.split(spins, counts, FOLDS, f, SEED, True)
        he_rows, he_c, _, _ = R.split(spins, counts, FOLDS, f, SEED, False)
        for a, c in enumerate(cs):
            x, _, _ = O.learn_nodes_fast(tr_c, spins[tr_rows], np.arange(n), "RISE", c=c, tol=1e-9)
            loss[a, f] = O.objgrad_nodes("RISE", he_c, spins[he_rows], np.arange(n), x, want_grad=False)[0].sum()
            supp[a, f] = np.count_nonzero(x[~np.eye(n, dtype=bool)])
    assert np.array_equal(res.loss, loss) and np.array_equal(res.support, supp)
    mean = loss.mean(axis=1)
    se = loss.std(axis=1, ddof=1) / np.sqrt(FOLDS)
    assert np.array_equal(res.mean, mean) and np.array_equal(res.se, se)
    i = int(np.argmin(mean))
    assert res.c_min == cs[i] and res.c == res.c_min
    assert res.c_1se == max(c for c, m in zip(cs, mean) if m <= mean[i] + se[i])
    assert res.c_1se >= res.c_min
    assert np.array_equal(res.stats["fold_sizes"], R.fold_sizes(counts, FOLDS, SEED)) and res.stats["fold_sizes"].sum() == counts.sum()
    assert res.stats["iterations"].shape == (len(cs), FOLDS)
    assert all(res.stats[k] >= 0 for k in ("split_s", "solve_s", "score_s"))
    # the final model: learn() at the chosen c, verbatim
    want = O.learn_pair(samples, "RISE", c=res.c, symmetrize=False)[0]
    assert np.array_equal(res.model, 0.5 * (want + want.T))


def test_rule_1se_and_other_score(samples):
    rec = Recorder()
    res = run_path(rec, samples, gml.logRISE(0.8, False), [1.0, 0.1], gml.HIP(), folds=2, seed=1, score=gml.RPLE(), rule="1se")
    assert res.c == res.c_1se
    counts, spins = O.split_histogram(samples)
    _, tr, he = rec.parts[0]
    x = rec.solves[0][3]
    assert res.loss[0, 0] == O.objgrad_nodes("RPLE", he.counts, he.spins, np.arange(he.n), x, want_grad=False)[0].sum()
    want = O.learn_pair(samples, "logRISE", c=res.c, symmetrize=False)[0]
    assert np.array_equal(res.model, want)  # (symmetrization False: the rows as solved)


def test_ties_go_to_the_larger_c(samples):
    res = run_path(Recorder(score_override=lambda held, rows: 1.0), samples, gml.RISE(), [0.1, 0.2, 0.3], gml.HIP(), folds=2)
    assert res.c_min == 0.3 and res.c_1se == 0.3 and res.c == 0.3 and np.array_equal(res.se, np.zeros(3))
    cs = np.array([4.0, 3.0, 2.0, 1.0])
    loss = np.array([[5.0, 5.0], [1.0, 3.0], [2.0, 2.0], [1.5, 2.5]])  # means 5, 2, 2, 2; se 0, 1, 0, 0.5
    mean, se, c_min, c_1se, c = path_module.select_c(cs, loss, "min")
    assert (c_min, c_1se, c) == (3.0, 3.0, 3.0) and mean.tolist() == [5.0, 2.0, 2.0, 2.0]
    loss = np.array([[2.5, 3.5], [2.0, 2.0], [1.0, 2.0], [3.0, 3.0]])  # means 3, 2, 1.5, 3; se at the minimum 0.5
    assert path_module.select_c(cs, loss, "1se")[2:] == (2.0, 3.0, 3.0)


def test_argument_errors_before_the_library_loads(samples):
    def boom(*a, **k):
        raise AssertionError("a device step ran")
    rec = Recorder()
    rec.open = boom
    bad = [dict(method=gml.HIP(devices=[0, 1])), dict(method=gml.HIP(distributed=True)), dict(method=gml.HIP(node_range=(0, 2))),
           dict(folds=1), dict(folds=65), dict(folds=2.5), dict(cs=[]), dict(cs=[0.1, -0.2]), dict(cs=[0.1, np.inf]), dict(cs=[np.nan]),
           dict(rule="best"), dict(method=gml.HIP(precision="f16"))]
    for kw in bad:
        args = dict(cs=[0.2, 0.1], method=gml.HIP(), folds=3)
        args.update(kw)
        with pytest.raises(ValueError):
            run_path(rec, samples, gml.RISE(), args.pop("cs"), args.pop("method"), **args)
    with pytest.raises(TypeError):
        run_path(rec, samples, "RISE", [0.1])
    with pytest.raises(TypeError):
        run_path(rec, samples, gml.RISE(), [0.1], gml.HIP(), score="RPLE")
    with pytest.raises(ValueError):
        run_path(rec, np.zeros(5), gml.RISE(), [0.1])
