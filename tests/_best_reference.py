"""numpy restatement of gml_model_best_states and gml_conditional_mode (include/gml.h) by brute force in np.longdouble.
The k best states of a model: per connected component of at most 20 spins every state is listed, its energy is the plain sum over the
component's terms (as Component of _exact_reference.py forms it), and the best k are taken by (energy descending, state ascending).
The components' lists -- a spin in no term is a component of two states of energy 0 -- are merged in pairs: all sums of two lists,
the best k of them by the same rule on the joint state.  The empty key is a constant of every energy.
The tie rule, stated once: a state is the number whose bit i - 1 is set iff spin i (1-based) is -1; of two states with equal energies
the smaller number comes first.  (Numbers compare from their highest bit, i.e. from the highest spin down.)
The conditional mode of a row: the hidden state of largest E_k(s_H) (the energies of _cond_exact_reference.py, all terms, the row's
constant included), equal energies to the lower local state (bit j <-> the j-th hidden spin, ascending).
Models are {1-based key tuple: weight} dicts."""
import numpy as np

from _cond_exact_reference import _parity, row_coefficients
from _exact_reference import LD, MAX_SPINS, chain_model, components, dense_model, reduce_key


def _energies(nspins, cterms):
    """the energies of all 2^nspins states over local bits; cterms: (local mask, weight) pairs"""
    states = np.arange(1 << nspins, dtype=np.uint32)
    E = np.zeros(len(states), dtype=LD)
    for mask, w in cterms:
        E += np.where(_parity(states & np.uint32(mask)), -LD(w), LD(w))
    return E


def _take_best(E, codes, k):
    """the best k of (E[a], codes[a]) by (energy descending, code ascending): a list of (energy, code)"""
    at = len(E) - min(k, len(E))
    cand = np.flatnonzero(E >= np.partition(E, at)[at])  # (everything at or above the k-th largest energy, ties included)
    order = sorted(cand.tolist(), key=lambda a: (-E[a], codes[a]))
    return [(E[a], int(codes[a])) for a in order[:k]]


def component_best(spins, cterms, k):
    """the best min(k, 2^sb) states of one component: (energy, global code); cterms: (reduced 1-based key, weight) of this component"""
    assert len(spins) <= MAX_SPINS, len(spins)
    local = {v: i for i, v in enumerate(spins)}
    E = _energies(len(spins), [(sum(1 << local[v] for v in key), w) for key, w in cterms])
    best = _take_best(E, np.arange(len(E)), k)
    return [(e, sum(1 << (spins[i] - 1) for i in range(len(spins)) if (s >> i) & 1)) for e, s in best]


def merge_best(A, B, k):
    """the best k sums of two lists over disjoint spins, by (sum descending, joint code ascending)"""
    sums = [(ea + eb, sa | sb) for ea, sa in A for eb, sb in B]
    sums.sort(key=lambda p: (-p[0], p[1]))
    return sums[:k]


def best_states(terms, n, k):
    """the min(k, 2^n) best states of the model: a list of (energy long double, code), component by component with the merge"""
    blocks = components(terms, n)
    of = {v: b for b, blk in enumerate(blocks) for v in blk}
    cterms = [[] for _ in blocks]
    const = LD(0)
    for key, w in terms.items():
        sp = reduce_key(key)
        if w == 0.0:
            continue
        if not sp:
            const += LD(w)
        else:
            cterms[of[sp[0]]].append((sp, w))
    out = [(const, 0)]
    for blk, ct in zip(blocks, cterms):
        out = merge_best(out, component_best(blk, ct, k), k)
    return out


def best_states_whole(terms, n, k):
    """the same by brute force over all 2^n states of the whole model (n <= 20), no components, no merge"""
    cterms = [(sum(1 << (v - 1) for v in reduce_key(key)), w) for key, w in terms.items() if w != 0.0]
    E = _energies(n, cterms)
    return _take_best(E, np.arange(len(E)), k)


def spins_of(codes, n):
    """int8 [len(codes), n] of +-1"""
    return np.array([[-1 if (c >> i) & 1 else 1 for i in range(n)] for c in codes], dtype=np.int8).reshape(len(codes), n)


def code_of(states):
    """the codes of int8 [r, n] rows of +-1"""
    return [sum(1 << i for i, s in enumerate(row) if s < 0) for row in np.asarray(states)]


def smallest_gap(best):
    """the smallest difference of neighbouring energies of a best-first list (inf for fewer than two)"""
    e = np.array([b[0] for b in best], dtype=LD)
    return float(np.min(e[:-1] - e[1:])) if len(e) > 1 else float("inf")


def chain_best_energies(J, k):
    """the k largest energies of an open chain without fields: sum|J| - 2 (the subset sums of |J| in ascending order), each twice (s
    and -s); long double [k].  len(J) <= 24."""
    a = np.sort(np.abs(np.asarray(J, dtype=LD)))
    # the k / 2 smallest subset sums: grow the list bond by bond, keep the smallest
    sums = np.zeros(1, dtype=LD)
    for x in a:
        sums = np.sort(np.concatenate([sums, sums + x]))[:(k + 1) // 2]
    return np.repeat(a.sum() - 2 * sums, 2)[:k]


# ---- the conditional mode -----------------------------------------------------------------------------------------------------------
def cond_mode(terms, n, row, hidden):
    """(state int8 [h] of +-1, the hidden spins ascending; energy; log_p; gap = best - second-best energy, inf for h = 0) of one row,
    long double; h <= 20"""
    hid = sorted(int(i) for i in hidden)
    h = len(hid)
    coef = row_coefficients(terms, np.asarray(row), hid)
    E = _energies(h, list(coef.items()))
    best = int(np.argmax(E))  # (the first maximum: the lower local state)
    m = E[best]
    log_w = m + np.log(np.exp(E - m).sum())
    rest = np.delete(E, best)
    gap = float(m - rest.max()) if len(rest) else float("inf")
    return np.array([-1 if (best >> j) & 1 else 1 for j in range(h)], dtype=np.int8), m, m - log_w, gap


def cond_mode_rows(terms, n, rows, hidden):
    """every row under one hidden set: (states int8 [K, h], energy [K], log_p [K], gap [K])"""
    out = [cond_mode(terms, n, r, hidden) for r in np.asarray(rows)]
    return (np.array([o[0] for o in out], dtype=np.int8).reshape(len(out), len(list(hidden))), np.array([o[1] for o in out], dtype=LD),
            np.array([o[2] for o in out], dtype=LD), np.array([o[3] for o in out]))


def cond_mode_masked(terms, n, rows, mask):
    """every row under its own hidden set mask[k] (bool [K, n]): (completed int8 [K, n], energy [K], log_p [K], gap [K])"""
    rows, mask = np.asarray(rows), np.asarray(mask, dtype=bool)
    done = rows.astype(np.int8).copy()
    energy, log_p, gap = np.zeros(len(rows), dtype=LD), np.zeros(len(rows), dtype=LD), np.zeros(len(rows))
    for k, r in enumerate(rows):
        hid = np.flatnonzero(mask[k])
        st, energy[k], log_p[k], gap[k] = cond_mode(terms, n, r, hid)
        done[k, hid] = st
    return done, energy, log_p, gap


# ---- the models of the tests, and their references computed once ---------------------------------------------------------------------
def two_component_model(sb):
    """(terms, n): a dense component on spins 1 .. sb with fields and 8 longer terms, a second one on the two spins after it (the
    family of tests/test_gpu_exact.py, restated)"""
    terms = dense_model(range(1, sb + 1), seed=100 + sb, extra=8)
    terms.update({(sb + 1, sb + 2): 0.35, (sb + 1,): -0.2, (sb + 2,): 0.15})
    return terms, sb + 2


def ascending_model(sb=13, seed=7):
    """(terms, n): fields of -2.0 on every spin and weak random pairs: the energies rise with the state's number of set bits, so every
    chunk of an enumeration in state order beats the ones before it"""
    rng = np.random.default_rng(seed)
    terms = {(i,): -2.0 for i in range(1, sb + 1)}
    terms.update({(i, j): float(rng.normal(scale=0.05)) for i in range(1, sb + 1) for j in range(i + 1, sb + 1)})
    return terms, sb


def components_model():
    """(terms, n = 50): components of 1, 3, 13 and 20 spins, 13 spins in no term, a zero weight, the empty key and a cancelled key (the
    model of test_components in tests/test_gpu_exact.py, restated)"""
    terms = {(7,): 0.6}
    terms.update(dense_model([2, 9, 30], seed=31, extra=1))
    terms.update(dense_model(range(10, 23), seed=32, extra=6))
    terms.update(chain_model(list(range(31, 51)), seed=33)[0])
    rng = np.random.default_rng(34)
    terms.update({(v,): float(rng.normal(scale=0.2)) for v in range(31, 51, 3)})
    terms.update({(31, 40, 50): 0.25, (33, 35, 44, 47): -0.3, (32, 36, 41, 45, 49): 0.2})
    terms[(7, 10)] = 0.0
    terms[()] = -0.75
    terms[(3, 3)] = 0.5
    return terms, 50


def cond_model(n=16, seed=16, triples=12):
    """dense pairwise terms with fields on n spins and a few terms of order 3"""
    rng = np.random.default_rng(seed)
    terms = {(i,): float(rng.normal(scale=0.3)) for i in range(1, n + 1)}
    terms.update({(i, j): float(rng.normal(scale=0.3)) for i in range(1, n + 1) for j in range(i + 1, n + 1)})
    for _ in range(triples):
        terms[tuple(int(v) + 1 for v in sorted(rng.choice(n, size=3, replace=False)))] = float(rng.normal(scale=0.3))
    return terms


def merged_model():
    """(terms, n = 17): components of 13, 3 and 1 spins, no spin without a term"""
    terms = dense_model(range(1, 14), seed=32, extra=6)
    terms.update(dense_model([14, 15, 16], seed=31, extra=1))
    terms[(17,)] = 0.6
    return terms, 17


MODELS = {f"two{sb}": (lambda sb=sb: two_component_model(sb)) for sb in (1, 3, 11, 12, 13, 18)}
MODELS.update(ten=lambda: (dense_model(range(1, 11), seed=110, extra=8), 10), eight=lambda: (dense_model(range(1, 9), seed=108), 8),
              ascending=ascending_model, components=components_model, merged=merged_model)
_cache = {}


def reference(name, k=257):
    """(terms, n, the best min(k, 2^n) states of MODELS[name] as best_states gives them), computed once per (name, k)"""
    if (name, k) not in _cache:
        terms, n = MODELS[name]()
        _cache[(name, k)] = (terms, n, best_states(terms, n, k))
    return _cache[(name, k)]
