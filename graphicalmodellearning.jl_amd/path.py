"""learn_path(samples, formulation, cs, method): the regulariser chosen by K-fold cross-validation over a warm-started path.

The folds are cut on the device (Problem.split: the handle's sign bits are compacted in HBM, nothing is downloaded or re-packed);
the rest is orchestration over calls that exist: Problem.learn(x0=...) down the path on each training part,
Problem.objgrad(want_grad=False) on the held-out part, and learn() itself, verbatim, at the chosen c."""
import time
from dataclasses import dataclass, field, replace

import numpy as np

from . import _lib
from .formulations import HIP, NLP, RISE, GMLFormulation, GMLMethod, multiRISE
from .learn import _form_name, learn


@dataclass
class PathResult:
    """What learn_path returns.  cs: the regularisers, descending.  loss [len(cs), folds]: the held-out loss of every solve (the
    score formulation's smooth objective on the held-out part, summed over the nodes; a per-sample mean, comparable across folds),
    mean its average over the folds, se = std(ddof=1) / sqrt(folds).  support [len(cs), folds]: non-zero non-field entries of the
    solved rows.  c_min: the c of the smallest mean (ties: the larger c); c_1se: the largest c whose mean is within one se (the
    se at c_min) of the smallest; c: the one `rule` chose; model: learn(samples, formulation at c, method).  stats: "iterations"
    [len(cs), folds], "fold_sizes", and the wall-clock seconds "split_s", "solve_s", "score_s", "final_s"."""
    cs: np.ndarray
    loss: np.ndarray
    mean: np.ndarray
    se: np.ndarray
    support: np.ndarray
    c_min: float
    c_1se: float
    c: float
    model: object
    stats: dict = field(default_factory=dict)


def _open_hip(samples, order, device):
    """one handle over all nodes"""
    return _lib.Problem(samples, order=order, device=device)


def _split_hip(prob, folds, fold, seed):
    """(training part, held-out part) of fold `fold`: two new handles, split on the device"""
    return prob.split(folds, fold, seed=seed, complement=True), prob.split(folds, fold, seed=seed, complement=False)


def _solve_hip(train, formulation, c, x0, method, structure):
    """the rows of all nodes on the training part at regulariser c, started from x0 (None: from zero): (rows, stats)"""
    out, _, st = train.learn(_form_name(formulation), c, x0=x0, structure=structure, tol=method.tol, max_iter=method.max_iter,
                             precision=method.precision, max_working=method.max_working, max_add=method.max_add, verbose=method.verbose,
                             hess_samples=method.hess_samples, polish=method.polish)
    return out, st


def _score_hip(held, score, rows):
    """the held-out loss: the score formulation's smooth objective of the rows on the held-out part, summed over the nodes"""
    f, _ = held.objgrad(_form_name(score), np.arange(held.n), rows, want_grad=False)
    return float(f.sum())


def _field_mask(n, P, order):
    """True at the field slot of every row: slot u of node u for pairwise rows (:162), slot 0 for multi-body rows (:94-104)"""
    m = np.zeros((n, P), dtype=bool)
    if order == 2:
        m[np.arange(n), np.arange(n)] = True
    else:
        m[:, 0] = True
    return m


def select_c(cs, loss, rule="min"):
    """(mean, se, c_min, c_1se, c) of a loss table [len(cs), folds] over descending cs -- the selection rules of PathResult"""
    cs, loss = np.asarray(cs, dtype=np.float64), np.asarray(loss, dtype=np.float64)
    folds = loss.shape[1]
    mean = loss.mean(axis=1)
    se = loss.std(axis=1, ddof=1) / np.sqrt(folds)
    i_min = int(np.argmin(mean))  # cs descend: the first of equal means is the larger c
    i_1se = int(np.flatnonzero(mean <= mean[i_min] + se[i_min])[0])
    c_min, c_1se = float(cs[i_min]), float(cs[i_1se])
    return mean, se, c_min, c_1se, (c_min if rule == "min" else c_1se)


def learn_path(samples, formulation=None, cs=(), method=None, *, folds=5, seed=0, score=None, rule="min"):
    """Cross-validated regularisation path: learn() with the regulariser chosen among `cs` by `folds`-fold cross-validation.

    One handle is built over all nodes and split into folds on the device (Problem.split with `seed`).  On every training part the
    `cs` are solved in descending order, each solve started from the previous solution (method's tol / precision / max_iter / ... and
    method.structure apply to every solve); after each solve the held-out loss is the smooth objective of `score` -- None: the
    training formulation's own; or any formulation instance, e.g. RPLE() for the held-out conditional log-likelihood -- on the
    held-out part, summed over the nodes.  The final model is learn(samples, formulation with regularizer = the chosen c, method),
    called verbatim: method.refit / method.stderr apply to it and to nothing else.  rule: "min" (smallest mean loss; ties go to the
    larger c) or "1se" (the largest c within one standard error of it).  Works for every formulation learn takes.

    One process, one GPU, all nodes: method.devices, method.distributed and method.node_range raise ValueError.

    Caveat: the folds are drawn per SAMPLE.  A handle recorded from thinned chains with several samples per chain has
    autocorrelated rows, which land in different folds: the held-out part is then not independent of the training part and the
    held-out loss is optimistic.  Blocked (per-chain) folds are not implemented.

    Returns a PathResult."""
    if formulation is None:
        formulation = RISE()
    if method is None:
        method = HIP()
    if not isinstance(formulation, GMLFormulation):
        raise TypeError(f"no method matching learn_path(::Array, ::{type(formulation).__name__}, ...)")
    if not isinstance(method, GMLMethod):
        raise TypeError(f"no method matching learn_path(..., ::{type(method).__name__})")
    if score is not None and not isinstance(score, GMLFormulation):
        raise TypeError(f"score is a formulation instance or None, not {type(score).__name__}")
    method_given = method
    if isinstance(method, NLP):
        method = HIP()  # (as learn does)
    # (everything below is checked before the library loads)
    if method.devices is not None or method.distributed or method.node_range is not None:
        raise ValueError("learn_path: the folds are cut from ONE handle over all nodes: one process, one GPU, no devices, distributed or node_range")
    if isinstance(folds, bool) or int(folds) != folds or not 2 <= int(folds) <= 64:
        raise ValueError(f"learn_path: folds must be an integer in [2, 64], not {folds!r}")
    if rule not in ("min", "1se"):
        raise ValueError(f"learn_path: unknown rule {rule!r} (use 'min' or '1se')")
    cs = np.sort(np.asarray(list(cs), dtype=np.float64).ravel())[::-1].copy()
    if cs.size == 0 or not np.all(np.isfinite(cs)) or np.any(cs < 0):
        raise ValueError("learn_path: cs must be a non-empty list of finite regularisers >= 0")
    if method.precision not in _lib.PRECISIONS:
        raise ValueError(f"HIP: unknown precision {method.precision!r} (use 'auto', 'i8x', 'i8w' or 'f64')")
    samples = np.asarray(samples)
    if samples.ndim != 2 or samples.shape[1] < 2:
        raise ValueError("samples must be a K x (1+n) histogram matrix")
    folds, seed = int(folds), int(seed)
    n = samples.shape[1] - 1
    order = int(formulation.interaction_order) if isinstance(formulation, multiRISE) else 2
    score_form = formulation if score is None else score
    if (int(score_form.interaction_order) if isinstance(score_form, multiRISE) else 2) != order:
        raise ValueError("learn_path: score must read the rows the formulation solves: the same interaction order")
    structure = None
    if method.structure is not None:
        structure = np.asarray(method.structure)
        if structure.dtype != np.uint8 or structure.ndim != 2 or structure.shape[0] != n:
            raise _lib.GMLError(_lib.GML_EINVAL, f"HIP: structure is {structure.dtype} {structure.shape}, the problem takes uint8 ({n}, P)")
        structure = np.ascontiguousarray(structure)
    # (module attributes, looked up per call: the host tests substitute the four steps, as with _local_solve_hip in learn.py)
    open_, split, solve, score_fn = _open_hip, _split_hip, _solve_hip, _score_hip
    device = 0 if method.device is None else int(method.device)

    loss = np.zeros((len(cs), folds))
    support = np.zeros((len(cs), folds), dtype=np.int64)
    iters = np.zeros((len(cs), folds), dtype=np.int64)
    t_split = t_solve = t_score = 0.0
    prob = open_(samples, order, device)
    try:
        fold_sizes = np.asarray(prob.fold_sizes(folds, seed=seed), dtype=np.int64)
        for f in range(folds):
            t0 = time.perf_counter()
            train, held = split(prob, folds, f, seed)
            t_split += time.perf_counter() - t0
            try:
                x = None
                for a, c in enumerate(cs):
                    t0 = time.perf_counter()
                    x, st = solve(train, formulation, float(c), x, method, structure)
                    t1 = time.perf_counter()
                    loss[a, f] = score_fn(held, score_form, x)
                    t_score += time.perf_counter() - t1
                    t_solve += t1 - t0
                    xa = np.asarray(x)
                    support[a, f] = int(np.count_nonzero(xa[~_field_mask(xa.shape[0], xa.shape[1], order)]))
                    iters[a, f] = int((st or {}).get("iterations", 0))
            finally:
                for q in (train, held):
                    if hasattr(q, "close"):
                        q.close()
    finally:
        if hasattr(prob, "close"):
            prob.close()
    mean, se, c_min, c_1se, c = select_c(cs, loss, rule)
    t0 = time.perf_counter()
    model = learn(samples, replace(formulation, regularizer=c), method_given)
    stats = {"iterations": iters, "fold_sizes": fold_sizes, "split_s": t_split, "solve_s": t_solve, "score_s": t_score,
             "final_s": time.perf_counter() - t0}
    return PathResult(cs=cs, loss=loss, mean=mean, se=se, support=support, c_min=c_min, c_1se=c_1se, c=c, model=model, stats=stats)
