"""Conditional inference with a model: given some spins of a sample, what are the others?

conditional_sample / conditional_means run Glauber chains on the device that start from the rows of the evidence and hold the observed
spins fixed (gml_problem_create_mcmc_terms_conditional, gml_conditional_means: the term-list chains of GlauberTermChains, swept over
the hidden spins only).  A conditional mean is Rao-Blackwellised: not the average of the sampled spin but of 2 pup - 1, the
conditional expectation of the spin given all the others at the moment it was updated -- the same expectation with less variance,
and exact (no sampling at all) when one spin is hidden.  predictive_check hides the same spins in every row of a data set and scores
the predictions against the values the data hold: held-out predictive accuracy, the check of a fit that neither a
pseudo-likelihood nor an AIS likelihood gives.

impute / impute_sample are the same two for data with holes, where every row lacks its own set of spins (0 in the histogram matrix):
the hidden set is read per row from a second resident handle (gml_conditional_means_masked, gml_problem_create_mcmc_terms_masked).
missing.learn_missing builds stochastic-imputation EM on them.

With method=Exact() conditional_means, impute and predictive_check use no chain: every row's hidden spins are enumerated on the device
(gml_conditional_exact, gml_conditional_exact_masked; at most 24 hidden spins per row, any n), with the model's weights as they are
(the chains quantise them).  The exact path also gives what no chain can: log_p, the joint conditional log-probability of the values a
row holds on its hidden spins, and log_w, from which likelihood.observed_log_likelihood scores data with holes.  conditional_sample and
impute_sample with method=Exact() draw exactly, with no burn-in to guess: the same enumeration on energies perturbed by Gumbel noise
(gml_conditional_draw, gml_conditional_draw_masked); replicas and seed keep their meaning there."""
from dataclasses import dataclass

import numpy as np

from . import _lib
from .likelihood import Exact
from .sampling import GlauberTermChains, _problem_args, _term_list_args


@dataclass
class ConditionalMeans:
    """means [K, H]: E[s_i | the visible spins of row k] for the hidden spins i (ascending), averaged over the replicas; stderr [K, H]:
    the standard deviation over replicas / sqrt(replicas), NaN for one replica; per_replica [replicas, K, H]; hidden: the H hidden spins,
    1-based, ascending; counts [K]: the counts of the evidence rows.  From method=Exact(): the exact means, stderr 0.0, per_replica
    [1, K, H], and log_w [K] = log sum over the hidden spins of exp(E) (log P(visible spins of row k) = log_w[k] - log Z), log_p [K] =
    log P(the values row k holds on the hidden spins | its visible spins); both None from the chains."""
    means: np.ndarray
    stderr: np.ndarray
    per_replica: np.ndarray
    hidden: list
    counts: np.ndarray
    log_w: np.ndarray = None
    log_p: np.ndarray = None


@dataclass
class PredictiveCheck:
    """Per hidden spin (1-based, ascending): accuracy, the count-weighted share of rows whose hidden value is sign(mean) (a mean of
    exactly 0 predicts +1), and log_loss, the count-weighted mean of -log p with p = (1 + s mean) / 2 the probability given to the
    value s the data hold.  means: the ConditionalMeans behind them.  joint_log_loss (method=Exact() only, else None): the
    count-weighted mean of -log P(all held-out values of the row | its visible spins), the joint that the per-spin losses do not give."""
    hidden: list
    accuracy: np.ndarray
    log_loss: np.ndarray
    means: ConditionalMeans
    joint_log_loss: float = None


def _hidden_spins(hidden, n):
    """the hidden spins as a sorted list of 1-based ints; empty, out-of-range and repeated entries are refused"""
    spins = [int(i) for i in hidden]
    if not spins:
        raise ValueError("hidden names no spin")
    if min(spins) < 1 or max(spins) > int(n):
        raise ValueError(f"hidden spins are numbered from 1 to n = {int(n)} (given {spins})")
    if len(set(spins)) != len(spins):
        raise ValueError(f"hidden names a spin twice (given {spins})")
    return sorted(spins)


def _sampler(sampler):
    sampler = GlauberTermChains() if sampler is None else sampler
    if not isinstance(sampler, GlauberTermChains):
        raise ValueError(f"conditional inference takes a GlauberTermChains sampler, given {type(sampler).__name__}")
    return sampler


class _Evidence:
    """the evidence as an open Problem: the caller's own, or one opened from a histogram matrix and closed on exit"""

    def __init__(self, evidence):
        self.given = isinstance(evidence, _lib.Problem)
        self.p, self.matrix = (evidence, None) if self.given else (None, np.asarray(evidence))
        if not self.given and (self.matrix.ndim != 2 or self.matrix.shape[1] < 2):
            raise ValueError("evidence must be an open Problem or a K x (1+n) histogram matrix")
        self.n = evidence.n if self.given else self.matrix.shape[1] - 1

    def __enter__(self):
        if not self.given:
            self.p = _lib.Problem(self.matrix)
        return self.p

    def __exit__(self, *a):
        if not self.given:
            self.p.close()


def _exact_method(method, sampler, replicas, seed):
    """method=None: the chains.  An Exact: no chain runs, so a sampler, replicas and a seed are refused rather than ignored."""
    if method is None:
        return None
    if not isinstance(method, Exact):
        raise ValueError(f"conditional inference takes method=None (chains) or an Exact, given {type(method).__name__}")
    if sampler is not None or int(replicas) != 1 or int(seed) != 0:
        raise ValueError("method=Exact() enumerates: it takes no sampler, replicas=1 and seed=0")
    return method


def _draw_method(method, sampler, replicas):
    """method=None: the chains.  An Exact: exact draws by enumeration -- no chain runs, so a sampler is refused rather than ignored;
    replicas and seed keep their meaning."""
    if method is None:
        return None
    if not isinstance(method, Exact):
        raise ValueError(f"conditional sampling takes method=None (chains) or an Exact, given {type(method).__name__}")
    if sampler is not None:
        raise ValueError("method=Exact() draws by enumeration: it takes no sampler")
    if int(replicas) < 1:
        raise ValueError(f"replicas must be at least 1 (given {replicas})")
    return method


def _model_terms(model):
    """(the model's term list, a model without a term as the chains take it; its interaction order)"""
    args = _term_list_args(model, _problem_args(model))
    return (args["terms"] if len(args["terms"]) else {(1,): 0.0}), args.get("order", 2)


def _run(model, evidence, hidden, sampler, replicas, seed, means):
    sampler = _sampler(sampler)
    if int(replicas) < 1:
        raise ValueError(f"replicas must be at least 1 (given {replicas})")
    ev = _Evidence(evidence)
    spins = _hidden_spins(hidden, ev.n)
    args = _term_list_args(model, _problem_args(model))
    with ev as p:
        out = _lib.conditional_chains(args["terms"], ev.n, p, np.asarray(spins) - 1, int(replicas), sampler.samples_per_chain,
                                      sampler.burn_in, sampler.thin, seed, means=means, order=args.get("order", 2))
        return out, spins, (p.counts() if means else None), p.K


def conditional_sample(model, evidence, hidden, sampler=None, *, replicas=1, seed=0, method=None):
    """Samples of the hidden spins (1-based, like FactorGraph keys) given the visible spins of every row of `evidence` (an open Problem or
    a K x (1+n) histogram matrix; its counts play no part).  model: a FactorGraph, a {1-based key tuple: weight} dict or a matrix with the
    fields on its diagonal; sampler: a GlauberTermChains (burn_in, thin, samples_per_chain).  Returns a Problem on the evidence's device
    with K replicas samples_per_chain rows of count 1: row (t replicas + r) K + k is sample t of replica r of evidence row k, its
    visible spins those of the evidence.
    method=Exact(): exact draws by enumeration of the hidden spins (gml_conditional_draw; at most method.max_hidden <= 24 of them), no
    chain and no sampler.  The result has K replicas rows of count 1, row r K + k the draw of replica r of evidence row k (chain
    r K + k of the seed); it is built through the host."""
    if _draw_method(method, sampler, replicas) is None:
        return _run(model, evidence, hidden, sampler, replicas, seed, False)[0]
    ev = _Evidence(evidence)
    spins = _hidden_spins(hidden, ev.n)
    if len(spins) > method.max_hidden:  # (refused before a handle is opened)
        raise ValueError(f"{len(spins)} spins are hidden: more than max_hidden = {method.max_hidden}")
    terms, order = _model_terms(model)
    hid = np.asarray(spins) - 1
    with ev as p:
        st = _lib.conditional_draw(terms, ev.n, p, hid, int(replicas), seed, energy=False, log_p=False)[0]
        rows = np.tile(p.spins(), (int(replicas), 1))
    rows[:, hid] = st.T
    return _lib.Problem(spins=rows, order=order)


def conditional_means(model, evidence, hidden, sampler=None, *, replicas=1, seed=0, method=None):
    """Rao-Blackwellised conditional means of the hidden spins given the visible spins of every evidence row; arguments as
    conditional_sample.  No handle is made.  Returns a ConditionalMeans (columns: the hidden spins in ascending order).
    method=Exact(): the exact means by enumeration of the hidden spins (at most method.max_hidden <= 24 of them), with log_w and log_p;
    no sampler, replicas or seed then."""
    if _exact_method(method, sampler, replicas, seed) is not None:
        ev = _Evidence(evidence)
        spins = _hidden_spins(hidden, ev.n)
        if len(spins) > method.max_hidden:  # (refused before a handle is opened)
            raise ValueError(f"{len(spins)} spins are hidden: more than max_hidden = {method.max_hidden}")
        args = _term_list_args(model, _problem_args(model))
        terms = args["terms"] if len(args["terms"]) else {(1,): 0.0}  # (a model without a term, as the chains take it)
        with ev as p:
            m, log_w, log_p = _lib.conditional_exact(terms, ev.n, p, np.asarray(spins) - 1)
            counts = p.counts()
        means = np.ascontiguousarray(m.T)
        return ConditionalMeans(means, np.zeros_like(means), means[None].copy(), spins, counts, log_w, log_p)
    raw, spins, counts, K = _run(model, evidence, hidden, sampler, replicas, seed, True)
    R = int(replicas)
    per = np.ascontiguousarray(raw.reshape(len(spins), R, K).transpose(1, 2, 0))  # [H][r K + k] -> [r][k][a]
    if R > 1:
        stderr = per.std(axis=0, ddof=1) / np.sqrt(R)
    else:
        stderr = np.full(per.shape[1:], np.nan)
    return ConditionalMeans(per.mean(axis=0), stderr, per, spins, counts)


@dataclass
class Imputation:
    """means [K', n]: E[s_i | the observed spins of row k] where row k lacks spin i, averaged over the replicas, and the observed value
    (+-1) where it does not; stderr [K', n]: the standard deviation over replicas / sqrt(replicas) -- 0 for an observed entry, NaN for
    one replica; missing [K', n] bool.  K' rows: the rows of the given matrix, one of count c expanded into c consecutive rows."""
    means: np.ndarray
    stderr: np.ndarray
    missing: np.ndarray


def _parse_holes(samples):
    """(counts [K], spins [K, n], missing bool [K, n]) of a K x (1+n) histogram matrix whose spin entries are in {-1, 0, +1}, 0 =
    missing.  Counts that are not positive integers and any other spin entry are refused."""
    s = np.asarray(samples)
    if s.ndim != 2 or s.shape[1] < 2:
        raise ValueError("samples must be a K x (1+n) histogram matrix")
    counts, spins = s[:, 0], s[:, 1:]
    if not np.all(np.isfinite(counts)) or np.any(counts < 1) or np.any(counts != np.floor(counts)):
        raise ValueError("the counts of data with missing entries must be positive integers (a row of count c is expanded into c rows)")
    if not np.all((spins == -1) | (spins == 0) | (spins == 1)):
        raise ValueError("the spin entries of data with missing entries must be -1, +1 or 0 (0 = missing)")
    return counts, spins, spins == 0


def _missing_rows(samples):
    """(values int8 [K', n] with +1 in place of a hole, missing bool [K', n]) of a histogram matrix as _parse_holes takes it.  A row of
    count c becomes c consecutive rows: every original sample has its own holes to fill."""
    counts, spins, missing = _parse_holes(samples)
    rows = np.repeat(np.arange(len(counts)), counts.astype(np.int64))
    missing = missing[rows]
    return np.where(missing, 1, spins[rows]).astype(np.int8), missing


def _check_holes(missing, max_hidden):
    most = int(missing.sum(axis=1).max()) if missing.size else 0
    if most > max_hidden:
        raise ValueError(f"a row lacks {most} spins: more than max_hidden = {max_hidden}")


def _mask_order(missing):
    """the stable order of the rows by their packed masks (spin 0 the most significant bit): rows that lack the same spins become
    neighbours, and a wave of 64 chains sweeps the union of what its rows lack"""
    return np.lexsort(np.packbits(missing, axis=1).T[::-1])


class _Holes:
    """data with holes as two open handles of the same rows: `evidence` (a hole holds +1, which plays no part) and `mask` (-1 = missing);
    closed on exit.  The handles hold the rows in the order of _mask_order (row j of the handles is the caller's row perm[j], and
    caller's row i is handle row inverse[i]); the chains are numbered in that order, r K + j, and so are their random streams."""

    def __init__(self, values, missing, order=2, device=0):
        self.perm = _mask_order(missing)
        self.inverse = np.argsort(self.perm)
        self.values, self.missing, self.order, self.device = values[self.perm], missing[self.perm], int(order), int(device)
        self.K, self.n = values.shape
        self.evidence = self.mask = None

    def __enter__(self):
        self.evidence = _lib.Problem(spins=self.values, order=self.order, device=self.device)
        try:
            self.mask = _lib.Problem(spins=np.where(self.missing, -1, 1).astype(np.int8), device=self.device)
        except Exception:
            self.evidence.close()
            raise
        return self

    def __exit__(self, *a):
        for p in (self.mask, self.evidence):
            if p is not None:
                p.close()

    def chains(self, model, sampler, replicas, seed, means, order=None):
        """_lib.conditional_chains_masked of `model` on the two handles: rows in the handles' order"""
        args = _term_list_args(model, _problem_args(model))
        terms = args["terms"] if len(args["terms"]) else {(1,): 0.0}  # (a model without a term: every update is a coin flip)
        return _lib.conditional_chains_masked(terms, self.n, self.evidence, self.mask, int(replicas), sampler.samples_per_chain,
                                              sampler.burn_in, sampler.thin, seed, means=means,
                                              order=args.get("order", 2) if order is None else order)


    def draws(self, model, replicas, seed, order=None):
        """a handle of the K replicas exact draws of `model` on the two handles (_lib.conditional_draw_masked), rows in the handles'
        order: row r K + j completes handle row j, from chain r K + j; built through the host"""
        terms, model_order = _model_terms(model)
        st = _lib.conditional_draw_masked(terms, self.n, self.evidence, self.mask, int(replicas), seed, energy=False, log_p=False)[0]
        return _lib.Problem(spins=np.ascontiguousarray(st.T), order=model_order if order is None else order, device=self.device)


def _exact_holes(model, values, missing, device=0, means=True, log_w=True, log_p=True):
    """_lib.conditional_exact_masked of `model` on data with holes (values int8 [K, n], missing bool [K, n]): (means [K, n], log_w [K],
    log_p [K]) in the caller's row order, None for what was not asked for"""
    with _Holes(values, missing, device=device) as holes:
        args = _term_list_args(model, _problem_args(model))
        terms = args["terms"] if len(args["terms"]) else {(1,): 0.0}
        m, lw, lp = _lib.conditional_exact_masked(terms, holes.n, holes.evidence, holes.mask, means=means, log_w=log_w, log_p=log_p)
        inv = holes.inverse
    return (None if m is None else np.ascontiguousarray(m.T[inv]), None if lw is None else lw[inv], None if lp is None else lp[inv])


@dataclass
class ConditionalMode:
    """states int8 [K, H]: every evidence row's most probable JOINT state of the hidden spins given its visible ones (equal energies:
    the hidden spins read as a binary number, the first at bit 0, -1 a set bit -- the lower number, so a hidden spin in no term is +1);
    energy [K]: E_k of that state, the row's constant included; log_p [K] = log P(x_H = states[k] | x_O); hidden: the H hidden spins,
    1-based, ascending; counts [K]: the counts of the evidence rows."""
    states: np.ndarray
    energy: np.ndarray
    log_p: np.ndarray
    hidden: list
    counts: np.ndarray


def conditional_mode(model, evidence, hidden, *, method=None):
    """The most probable joint completion of the hidden spins of every evidence row, by enumeration on the device
    (gml_conditional_mode): model, evidence, hidden as conditional_means takes them; method: an Exact whose max_hidden (<= 24) bounds
    the hidden spins.  Not the signs of the conditional means, which decide spin by spin.  Returns a ConditionalMode."""
    method = Exact() if method is None else _exact_method(method, None, 1, 0)
    ev = _Evidence(evidence)
    spins = _hidden_spins(hidden, ev.n)
    if len(spins) > method.max_hidden:  # (refused before a handle is opened)
        raise ValueError(f"{len(spins)} spins are hidden: more than max_hidden = {method.max_hidden}")
    args = _term_list_args(model, _problem_args(model))
    terms = args["terms"] if len(args["terms"]) else {(1,): 0.0}  # (a model without a term, as the chains take it)
    with ev as p:
        st, energy, log_p = _lib.conditional_mode(terms, ev.n, p, np.asarray(spins) - 1)
        counts = p.counts()
    return ConditionalMode(np.ascontiguousarray(st.T), energy, log_p, spins, counts)


@dataclass
class ImputedMode:
    """completed int8 [K', n]: every row with its missing entries filled by their most probable JOINT values given the observed ones
    (an observed entry keeps its value); energy [K'] and log_p [K'] of that completion as in ConditionalMode (a row without holes:
    its own energy and 0.0); missing [K', n] bool.  K' rows as in Imputation."""
    completed: np.ndarray
    energy: np.ndarray
    log_p: np.ndarray
    missing: np.ndarray


def impute_mode(model, samples, *, method=None):
    """The most probable joint completion of every row of data with holes (`samples` as impute takes it), by enumeration of the row's
    missing spins on the device (gml_conditional_mode_masked; at most method.max_hidden <= 24 per row).  Returns an ImputedMode, its rows
    in the caller's order."""
    method = Exact() if method is None else _exact_method(method, None, 1, 0)
    values, missing = _missing_rows(samples)
    _check_holes(missing, method.max_hidden)  # (refused before a handle is opened)
    with _Holes(values, missing) as holes:
        args = _term_list_args(model, _problem_args(model))
        terms = args["terms"] if len(args["terms"]) else {(1,): 0.0}
        st, energy, log_p = _lib.conditional_mode_masked(terms, holes.n, holes.evidence, holes.mask)
        inv = holes.inverse
    return ImputedMode(np.ascontiguousarray(st.T[inv]), energy[inv], log_p[inv], missing)


def _impute_args(samples, sampler, replicas):
    sampler = _sampler(sampler)
    if int(replicas) < 1:
        raise ValueError(f"replicas must be at least 1 (given {replicas})")
    return sampler, _missing_rows(samples)  # (refused before a handle is opened)


def impute_sample(model, samples, sampler=None, *, replicas=1, seed=0, method=None):
    """Completions of data with holes: `samples` is a K x (1+n) histogram matrix whose spin entries are -1, +1 or 0 = missing (counts:
    positive integers; a row of count c stands for c samples, each completed on its own).  Every row keeps its observed spins and has
    its missing ones drawn from the model's conditional distribution given them, by Glauber chains whose hidden set is the row's own
    (gml_problem_create_mcmc_terms_masked).  model, sampler as conditional_sample.  Returns a Problem of K' replicas samples_per_chain rows
    of count 1, K' the number of expanded rows: row (t replicas + r) K' + k is sample t of replica r of expanded row k, in the caller's
    order.  On the device the rows run in the stable order of their packed masks, so that the 64 chains of a wave lack similar spins;
    chain numbers, and so the random streams, follow that order, and the completed rows are put back into the caller's order through
    the host (learn_missing, which does not care about the order, skips that).
    method=Exact(): every row's missing spins are drawn exactly, by enumeration (gml_conditional_draw_masked; at most
    method.max_hidden <= 24 per row), no chain and no sampler: K' replicas rows, row r K' + k the draw of replica r of expanded row k in
    the caller's order.  The chains are numbered as above: chain r K' + j is replica r of the j-th row in the order of the packed
    masks, and so are the random streams."""
    if _draw_method(method, sampler, replicas) is not None:
        values, missing = _missing_rows(samples)
        _check_holes(missing, method.max_hidden)  # (refused before a handle is opened)
        with _Holes(values, missing) as holes:
            with holes.draws(model, replicas, seed) as q:
                states, order = q.spins(), q.order
        states = states.reshape(-1, holes.K, holes.n)[:, holes.inverse].reshape(-1, holes.n)
        return _lib.Problem(spins=states, order=order)
    sampler, (values, missing) = _impute_args(samples, sampler, replicas)
    with _Holes(values, missing) as holes:
        with holes.chains(model, sampler, replicas, seed, False) as q:
            states, order = q.spins(), q.order
    states = states.reshape(-1, holes.K, holes.n)[:, holes.inverse].reshape(-1, holes.n)
    return _lib.Problem(spins=states, order=order)


def impute(model, samples, sampler=None, *, replicas=1, seed=0, method=None):
    """Rao-Blackwellised conditional means of the missing entries of `samples` (as impute_sample) given the observed entries of the
    same row (gml_conditional_means_masked).  No handle is returned.  Returns an Imputation, its rows in the caller's order.
    method=Exact(): the exact means by enumeration of every row's missing spins (gml_conditional_exact_masked; at most
    method.max_hidden <= 24 per row), stderr 0.0; no sampler, replicas or seed then."""
    if _exact_method(method, sampler, replicas, seed) is not None:
        values, missing = _missing_rows(samples)
        _check_holes(missing, method.max_hidden)  # (refused before a handle is opened)
        means = _exact_holes(model, values, missing, log_w=False, log_p=False)[0]
        return Imputation(means, np.zeros_like(means), missing)
    sampler, (values, missing) = _impute_args(samples, sampler, replicas)
    with _Holes(values, missing) as holes:
        raw = holes.chains(model, sampler, replicas, seed, True)
    R, (K, n) = int(replicas), values.shape
    per = raw.reshape(n, R, K).transpose(1, 2, 0)[:, holes.inverse]  # [n][r K + j] -> [r][k][i]
    if R > 1:
        stderr = per.std(axis=0, ddof=1) / np.sqrt(R)
    else:
        stderr = np.where(missing, np.nan, 0.0)
    return Imputation(per.mean(axis=0), stderr, missing)


def predictive_check(model, data, hidden, sampler=None, *, replicas=1, seed=0, method=None):
    """Hide the spins `hidden` in every row of `data` (an open Problem or a histogram matrix), predict them from the others under
    `model`, and compare with the values the data hold.  Returns a PredictiveCheck.  It says how well each hidden spin is predicted
    from the rest under the model; with several hidden spins each is predicted with the others hidden too (their joint uncertainty is
    averaged over), and it says nothing about spins that were never hidden.  method=Exact(): exact means instead of chains, and
    joint_log_loss, the loss of the joint prediction of a row's hidden spins."""
    ev = _Evidence(data)
    spins = _hidden_spins(hidden, ev.n)  # (refused before the data are opened)
    if _exact_method(method, sampler, replicas, seed) is not None and len(spins) > method.max_hidden:
        raise ValueError(f"{len(spins)} spins are hidden: more than max_hidden = {method.max_hidden}")
    with ev as p:
        cm = conditional_means(model, p, hidden, sampler, replicas=replicas, seed=seed, method=method)
        truth = p.spins()[:, np.asarray(cm.hidden) - 1].astype(np.float64)
    w = cm.counts / cm.counts.sum()
    predicted = np.where(cm.means >= 0.0, 1.0, -1.0)
    accuracy = w @ (predicted == truth)
    prob = np.maximum((1.0 + truth * cm.means) / 2.0, np.finfo(np.float64).tiny)
    joint = None if cm.log_p is None else float(-(w @ cm.log_p))
    return PredictiveCheck(cm.hidden, accuracy, w @ (-np.log(prob)), cm, joint)
