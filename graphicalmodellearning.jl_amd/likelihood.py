"""log_partition(model) and log_likelihood(data, model): how well a model explains data.

(1/M) sum_k c_k log P(s_k) = sum_t w_t <prod_{i in t} s_i>_data - log Z.  The first part is exact (Problem.term_moments: integer
sums on the device); log Z is estimated by annealed importance sampling on the device (gml_log_partition_ais: the term-list chains
walked from beta = 0 to beta = 1 with a running weight).  AIS is unbiased for Z, hence biased low for log Z: the likelihood is an
optimistic one, and the standard error does not see a well that no chain found (include/gml.h).  Where every connected component of
the model has at most 40 spins, Exact() gives log Z itself (gml_model_exact: enumeration on the device), and exact_moments the
model's own means, correlations and term expectations: the model-side twin of moments(samples).  Where the model is sparse --
a lattice, a Chimera graph, a tree, an l1 solution of thousands of spins in one component -- Elimination() gives the exact log Z by
variable elimination (gml_model_elim: the cost follows the width of an elimination order, not the number of spins), and
model_term_moments the model's own sufficient statistics to hold against Problem.term_moments."""
from dataclasses import dataclass

import numpy as np

from . import _lib
from .sampling import _problem_args, _term_list_args


class AIS:
    """Annealed importance sampling: `chains` chains, each walked along the inverse temperatures `betas` with `sweeps_per_step`
    sweeps at each.  betas=None: `steps` equal steps from 0 to 1, np.linspace(0, 1, steps + 1).  A given schedule starts at 0, has at
    least two values, all finite and >= 0; it need not be monotone, and its last value is the beta whose log Z is estimated."""

    def __init__(self, chains=4096, steps=1000, sweeps_per_step=1, betas=None):
        self.chains, self.sweeps_per_step = int(chains), int(sweeps_per_step)
        if self.chains < 1 or self.sweeps_per_step < 1:
            raise ValueError(f"chains and sweeps_per_step must be at least 1 (given {chains}, {sweeps_per_step})")
        if betas is None:
            if int(steps) < 1:
                raise ValueError(f"steps must be at least 1 (given {steps})")
            self.betas = np.linspace(0.0, 1.0, int(steps) + 1)
        else:
            self.betas = np.array(betas, dtype=np.float64).ravel()
            if len(self.betas) < 2 or self.betas[0] != 0.0 or not np.isfinite(self.betas).all() or (self.betas < 0.0).any():
                raise ValueError("betas must start at 0, have at least two values and be finite and non-negative")
        self.steps = len(self.betas) - 1


class Exact:
    """Exact enumeration on the device.  For log Z and the model's moments (gml_model_exact): every connected component of the model's
    term hypergraph has at most `max_spins` spins, itself at most 40 (the library's limit; a component of sb spins costs one pass over
    its 2^sb states).  For conditional inference (gml_conditional_exact: conditional_means, impute, predictive_check,
    observed_log_likelihood): every row hides at most `max_hidden` spins, itself at most 24 (a row of h hidden spins costs 2^h states)."""

    def __init__(self, max_spins=40, max_hidden=24):
        self.max_spins, self.max_hidden = int(max_spins), int(max_hidden)
        if not 1 <= self.max_spins <= 40:
            raise ValueError(f"max_spins must lie in [1, 40] (given {max_spins})")
        if not 1 <= self.max_hidden <= 24:
            raise ValueError(f"max_hidden must lie in [1, 24] (given {max_hidden})")


class Elimination:
    """Exact variable elimination on the device (gml_model_elim) for log Z, the means and the model's own term expectations: any
    number of spins, as long as the elimination order has width (the largest scope of a step) at most `max_width`, itself at most 30
    (the library's limit; a step of scope k costs 2^k table entries).  order: a permutation of the 1-based spins, or None for the
    library's greedy order.  The width is planned on the host (gml_model_elim_plan), so a model too wide is refused before any
    device work."""

    def __init__(self, max_width=26, order=None):
        self.max_width = int(max_width)
        if not 1 <= self.max_width <= 30:
            raise ValueError(f"max_width must lie in [1, 30] (given {max_width})")
        self.order = None if order is None else np.asarray(order, dtype=np.int64).ravel()


@dataclass
class LogPartition:
    """log_z: the estimate; stderr: its delta-method standard error; ess: the effective sample size of the chains' weights (near 1:
    the schedule is too short); log_weights [chains].  energies [chains] and spins [chains, n] (the chains' final states and their
    energies) with return_states, else None.  From Exact(): log_z is exact, stderr 0.0, ess NaN, log_weights empty."""
    log_z: float
    stderr: float
    ess: float
    log_weights: np.ndarray
    energies: np.ndarray = None
    spins: np.ndarray = None


@dataclass
class LogLikelihood:
    """mean: the log-likelihood per sample, data_term - log_z; total = M mean; data_term = sum_t w_t <prod s>_data (exact sums);
    log_z and stderr: the estimate of log Z used and its standard error (NaN for a log_z given as a plain number)."""
    mean: float
    total: float
    data_term: float
    log_z: float
    stderr: float


def _model_terms(model):
    """(terms, n) of a FactorGraph, a term dict or a matrix: the term list the chains run on (n None: the largest spin named)"""
    args = _term_list_args(model, _problem_args(model))
    return args["terms"], args.get("n")


def _largest_component(terms, n):
    """the size of the largest connected component of the term hypergraph, by the library's rules (a spin named twice cancels, a
    zero weight joins nothing)"""
    keys, wts, _, n = _lib.term_arrays(terms, n)
    parent = list(range(int(n)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for key, w in zip(keys.tolist(), wts.tolist()):
        sp = [v for v in set(key) if v >= 0 and key.count(v) % 2 == 1]
        if w != 0.0:
            for v in sp[1:]:
                parent[find(v)] = find(sp[0])
    return int(np.bincount([find(i) for i in range(int(n))]).max())


def _check_exact(method, terms, n):
    if method.max_spins < 40 and _largest_component(terms, n) > method.max_spins:
        raise ValueError(f"a connected component of the model has more than max_spins = {method.max_spins} spins")


def _check_elimination(method, terms, n):
    width = _lib.model_elim_plan(terms, n, method.order)[1]
    if width > method.max_width:
        raise ValueError(f"the elimination order has width {width}, above max_width = {method.max_width}")


def log_partition(model, method=None, *, seed=0, device=0, return_states=False):
    """log Z of `model` (a FactorGraph, a {1-based key tuple: weight} dict or a matrix with the fields on its diagonal) by annealed
    importance sampling on the device; method: an AIS (default AIS()), an Exact for the exact value by enumeration, or an Elimination
    for the exact value by variable elimination (seed and return_states play no part in the exact ones).  Returns a LogPartition."""
    method = AIS() if method is None else method
    if not isinstance(method, (AIS, Exact, Elimination)):
        raise ValueError(f"log_partition takes an AIS method, given {type(method).__name__}")
    terms, n = _model_terms(model)
    if isinstance(method, Elimination):
        _check_elimination(method, terms, n)
        log_z = _lib.model_elim(terms, n, method.order, mean=False, texp=False, device=device)[0]
        return LogPartition(log_z, 0.0, float("nan"), np.zeros(0))
    if isinstance(method, Exact):
        _check_exact(method, terms, n)
        log_z = _lib.model_exact(terms, n, pairs=False, device=device)[0]
        return LogPartition(log_z, 0.0, float("nan"), np.zeros(0))
    result, logw, energies, spins = _lib.log_partition_ais(terms, n, method.chains, method.betas, method.sweeps_per_step, seed=seed,
                                                           device=device, return_states=return_states)
    return LogPartition(float(result[0]), float(result[1]), float(result[2]), logw, energies, spins)


def log_likelihood(data, model, method=None, *, log_z=None, seed=0, device=0):
    """The log-likelihood of `data` (a K x (1+n) histogram matrix as learn() takes, or an open Problem) under `model`.  log_z: a
    LogPartition (or a number) to reuse across data sets -- the folds of Problem.split, say; None: log_partition(model, method).
    Handles with fractional counts are refused by term_moments, whose error comes through unchanged.  Returns a LogLikelihood."""
    terms, _ = _model_terms(model)
    w = np.ascontiguousarray(terms.weights if hasattr(terms, "keys_array") else list(terms.values()), dtype=np.float64)
    if isinstance(data, _lib.Problem):
        sums, M = data.term_moments(terms, raw=True), data.M
    else:
        with _lib.Problem(data, device=device) as p:
            sums, M = p.term_moments(terms, raw=True), p.M
    data_term = float(np.dot(w, sums.astype(np.float64))) / M
    if log_z is None:
        log_z = log_partition(model, method, seed=seed, device=device)
    lz, se = (log_z.log_z, log_z.stderr) if isinstance(log_z, LogPartition) else (float(log_z), float("nan"))
    mean = data_term - lz
    return LogLikelihood(mean, M * mean, data_term, lz, se)


def observed_log_likelihood(data, model, method=None, *, log_z=None, seed=0, device=0):
    """The log-likelihood of data with holes: `data` is a K x (1+n) histogram matrix whose spin entries are -1, +1 or 0 = missing, as
    impute takes it (counts: positive integers), every row hiding at most 24 spins.  A row contributes log P(x_O), the marginal
    probability of what it observes: log sum over its missing spins of exp(E), by enumeration on the device
    (gml_conditional_exact_masked: exact, whatever `method` is), minus log Z.  log_z and method (an AIS, an Elimination, or an Exact
    whose max_hidden also bounds the holes of a row) as in log_likelihood.  Returns a LogLikelihood whose data_term is the count-weighted mean of
    log sum exp(E); on data without holes it equals log_likelihood."""
    from . import inference  # (inference imports this module)

    max_hidden = method.max_hidden if isinstance(method, Exact) else 24
    counts, spins, missing = inference._parse_holes(data)
    inference._check_holes(missing, max_hidden)  # (refused before a handle is opened)
    _, log_w, _ = inference._exact_holes(model, np.where(missing, 1, spins).astype(np.int8), missing, device=device, means=False, log_p=False)
    M = float(counts.sum())
    data_term = float(np.dot(counts.astype(np.float64), log_w)) / M
    if log_z is None:
        log_z = log_partition(model, method, seed=seed, device=device)
    lz, se = (log_z.log_z, log_z.stderr) if isinstance(log_z, LogPartition) else (float(log_z), float("nan"))
    mean = data_term - lz
    return LogLikelihood(mean, M * mean, data_term, lz, se)


def exact_moments(model, terms=None, pairs=True, device=0, method=None):
    """The model's own moments by enumeration on the device (gml_model_exact; components of at most 40 spins): (m [n], C [n, n]) --
    the magnetisations <s_i> and pair correlations <s_i s_j> under `model`, shaped as Problem.moments returns them (pairs=False: C is
    None).  With terms= (what Problem.term_moments takes for keys): the expectation of every listed term, in the caller's order.  The
    model-side twin of moments(samples).  method: an Exact whose max_spins refuses larger components."""
    mterms, n = _model_terms(model)
    _check_exact(Exact() if method is None else method, mterms, n)
    if terms is not None:
        return _lib.model_exact(mterms, n, queries=terms, pairs=False, device=device)[3]
    _, m, corr, _ = _lib.model_exact(mterms, n, pairs=pairs, device=device)
    return m, corr


@dataclass
class MostProbable:
    """states int8 [found, n]: the found = min(k, 2^n) most probable states of the model, +-1, by energy descending, equal energies in
    state order (spin i at bit i - 1, -1 a set bit, read as a binary number); energy [found]: E(s) = sum_t w_t prod_{i in t} s_i;
    log_p [found] = energy - log Z with log_prob=True, else None."""
    states: np.ndarray
    energy: np.ndarray
    log_p: np.ndarray = None


def most_probable_states(model, k=1, *, log_prob=False, device=0, method=None):
    """The k most probable states of `model` (as log_partition takes it), certified by enumeration on the device
    (gml_model_best_states): 1 <= k <= 256, components of at most 40 spins (method: an Exact whose max_spins refuses larger ones).
    log_prob=True adds their log-probabilities at the price of one exact log Z: by enumeration (gml_model_exact), or with
    method=Elimination() by variable elimination (the states themselves are enumerated either way).  Returns a MostProbable."""
    terms, n = _model_terms(model)
    if isinstance(method, Elimination):
        if log_prob:
            _check_elimination(method, terms, n)
    else:
        _check_exact(Exact() if method is None else method, terms, n)
    states, energy = _lib.model_best_states(terms, n, k, device=device)
    if not log_prob:
        return MostProbable(states, energy, None)
    if isinstance(method, Elimination):
        log_z = _lib.model_elim(terms, n, method.order, mean=False, texp=False, device=device)[0]
    else:
        log_z = _lib.model_exact(terms, n, pairs=False, device=device)[0]
    return MostProbable(states, energy, energy - log_z)


def model_term_moments(model, method=None, device=0):
    """The model's own sufficient statistics: (m [n], e [number of terms]) -- the means <s_i> and the expectation <prod_{i in t} s_i>
    of every term of `model` under the model itself, the terms in the model's own order: the model-side twin of
    Problem.term_moments(model.terms).  method: an Exact (the default: gml_model_exact with the model's terms as queries; components
    of at most 40 spins) or an Elimination (gml_model_elim: sparse models of any size; a term of weight zero over two or more spins
    gives NaN there)."""
    method = Exact() if method is None else method
    if not isinstance(method, (Exact, Elimination)):
        raise ValueError(f"model_term_moments takes an Exact or Elimination method, given {type(method).__name__}")
    terms, n = _model_terms(model)
    if isinstance(method, Elimination):
        _check_elimination(method, terms, n)
        _, m, e = _lib.model_elim(terms, n, method.order, device=device)
        if hasattr(terms, "keys_array"):  # (an array-backed model goes to the library without its zero weights: NaN, as above)
            nz = np.flatnonzero(terms.weights != 0.0)
            full = np.full(len(terms), np.nan)
            full[nz] = e[:len(nz)]
            e = full
        return m, e
    _check_exact(method, terms, n)
    _, m, _, e = _lib.model_exact(terms, n, queries=terms, pairs=False, device=device)
    return m, e
