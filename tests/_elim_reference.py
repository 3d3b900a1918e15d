"""Restatements of gml_model_elim_plan and gml_model_elim (include/gml.h) for the tests.

plan(): the planner's rule in Python -- neighbours, the greedy order, frontier sizes, width, work and stored -- to be compared with
`==` against the library.

SumProduct: an independent exact answer in np.longdouble.  Not the frontier recursion: bucket elimination over explicit factor arrays
(one log table per term, one unit table per spin) in a min-degree order, followed by the adjoint pass of that computation -- the
derivative of log Z with respect to every entry of every factor is that factor's marginal, which gives the means and the term
expectations.  The rules of the contract are restated by _exact_reference.reduce_key: a spin named twice cancels, a zero weight
joins nothing, an empty key adds its weight to log Z, a spin in no term gives ln 2 and mean 0.

bound(): the a-priori error bound of the device's FP64 recursion.  Models are {1-based key tuple: weight} dicts."""
import numpy as np

from _exact_reference import reduce_key

LD = np.longdouble


# ---- the planner's rule ----------------------------------------------------------------------------------------------------------
def neighbours(terms, n):
    """adj[v] (1-based; adj[0] unused): the spins that share a term of non-zero weight with v, after cancellation"""
    adj = [set() for _ in range(n + 1)]
    for key, w in terms.items():
        if w == 0.0:
            continue
        sp = reduce_key(key)
        for a in sp:
            adj[a].update(b for b in sp if b != a)
    return adj


def greedy(adj, n):
    """Components in the order of their smallest spin; a component starts at its lowest spin; then the unprocessed spin next to the
    frontier whose step leaves the smallest frontier after retiring, the lowest index among equals."""
    left = [len(a) for a in adj]  # unprocessed neighbours
    done = [False] * (n + 1)
    frontier, cand, seq = set(), set(), []
    lowest = 1
    while len(seq) < n:
        if cand:
            def after(c):
                retire = sum(1 for u in adj[c] if u in frontier and left[u] == 1) + (1 if left[c] == 0 else 0)
                return len(frontier) + 1 - retire
            v = min(sorted(cand), key=after)  # (min keeps the first, i.e. lowest, of equal scores)
        else:
            while done[lowest]:
                lowest += 1
            v = lowest
        seq.append(v)
        done[v] = True
        cand.discard(v)
        frontier.add(v)
        for u in adj[v]:
            left[u] -= 1
            if not done[u]:
                cand.add(u)
        frontier = {u for u in frontier if left[u] > 0}
    return seq


def by_component(adj, n, order):
    """a caller's permutation, component by component (the components in the order of their smallest spin)"""
    comp, ncomp = [None] * (n + 1), 0
    for i in range(1, n + 1):
        if comp[i] is None:
            comp[i], stack = ncomp, [i]
            while stack:
                for w in adj[stack.pop()]:
                    if comp[w] is None:
                        comp[w] = ncomp
                        stack.append(w)
            ncomp += 1
    parts = [[] for _ in range(ncomp)]
    for v in order:
        parts[comp[v]].append(v)
    return [v for part in parts for v in part]


def plan(terms, n, order=None):
    """(order [n] 1-based, width, work, stored) as gml_model_elim_plan defines them"""
    adj = neighbours(terms, n)
    seq = greedy(adj, n) if order is None else by_component(adj, n, [int(v) for v in order])
    pos = {v: t for t, v in enumerate(seq)}
    last = {v: max([pos[v]] + [pos[u] for u in adj[v]]) for v in seq}
    retiring = [0] * n
    for v in seq:
        retiring[last[v]] += 1
    F, width, work, stored = 0, 0, 0.0, 0.0
    for t in range(n):
        width = max(width, F + 1)
        work += 2.0 ** (F + 1)
        F += 1 - retiring[t]
        stored += 2.0 ** F
    return seq, width, work, stored


# ---- the independent sum-product ----------------------------------------------------------------------------------------------------
def _lse(a, axis):
    m = a.max(axis=axis, keepdims=True)
    return m + np.log(np.exp(a - m).sum(axis=axis, keepdims=True))


def _signs(k):
    """[2] * k table of prod s, index 0 = +1, index 1 = -1"""
    out = np.ones((), dtype=LD)
    for _ in range(k):
        out = np.multiply.outer(out, np.array([1, -1], dtype=LD))
    return out


def _min_degree(factors, n):
    adj = [set() for _ in range(n + 1)]
    for vs, _ in factors:
        for a in vs:
            adj[a].update(b for b in vs if b != a)
    todo, order = set(range(1, n + 1)), []
    while todo:
        v = min(todo, key=lambda u: (len(adj[u]), u))
        for a in adj[v]:
            adj[a].discard(v)
            adj[a].update(b for b in adj[v] if b != a)
        todo.discard(v)
        order.append(v)
    return order


class SumProduct:
    """log_z, mean [n], texp [number of terms, in the dict's order] of a model; all np.longdouble.  texp follows the contract of
    gml_model_elim: 1 for an empty or cancelled key; for a zero weight the spin's mean if one spin is left, else NaN."""

    def __init__(self, terms, n):
        items = [(reduce_key(k), w) for k, w in terms.items()]
        self.log_z = LD(0)
        factors, owner = [], []  # (vars ascending, log table); owner: ("term", index) or ("spin", v)
        for t, (sp, w) in enumerate(items):
            if not sp:
                self.log_z += LD(w)
            elif w != 0.0:
                factors.append((sp, LD(w) * _signs(len(sp))))
                owner.append(("term", t))
        for v in range(1, n + 1):
            factors.append(((v,), np.zeros(2, dtype=LD)))
            owner.append(("spin", v))
        nf = len(factors)
        order = _min_degree(factors, n)
        live = list(range(nf))
        buckets = []
        for v in order:
            mine = [f for f in live if v in factors[f][0]]
            live = [f for f in live if v not in factors[f][0]]
            allv = tuple(sorted(set().union(*[factors[f][0] for f in mine])))
            J = np.zeros((1,) * len(allv), dtype=LD)
            for f in mine:
                J = J + factors[f][1].reshape([2 if u in factors[f][0] else 1 for u in allv])
            ax = allv.index(v)
            m = _lse(J, ax)
            outv = tuple(u for u in allv if u != v)
            factors.append((outv, m.reshape((2,) * len(outv))))
            buckets.append((allv, ax, J, m, mine, len(factors) - 1))
            if outv:
                live.append(len(factors) - 1)
            else:
                self.log_z += m.reshape(())
        # the adjoint pass: d log Z / d (entry of a log table) = the marginal probability of that entry
        adj = [None] * len(factors)
        for allv, ax, J, m, mine, msg in reversed(buckets):
            am = np.ones((1,) * len(allv), dtype=LD) if adj[msg] is None else \
                adj[msg].reshape([2 if (u != allv[ax]) else 1 for u in allv])
            aJ = am * np.exp(J - m)
            for f in mine:
                drop = tuple(i for i, u in enumerate(allv) if u not in factors[f][0])
                adj[f] = aJ.sum(axis=drop).reshape((2,) * len(factors[f][0]))
        self.mean = np.zeros(n, dtype=LD)
        got = {}
        for f in range(nf):
            kind, what = owner[f]
            if kind == "spin":
                self.mean[what - 1] = adj[f][0] - adj[f][1]
            else:
                got[what] = (adj[f] * _signs(len(factors[f][0]))).sum()
        self.texp = np.array([LD(1) if not sp else got[t] if t in got else self.mean[sp[0] - 1] if len(sp) == 1 else LD(np.nan)
                              for t, (sp, w) in enumerate(items)], dtype=LD)


def bound(terms, n):
    """B = 2^-53 (T + 4 n) L for log Z, L = sum |w| + n ln 2 bounding every log entry: a step adds at most T_t + 1 roundings from phi_t
    and about four from max / exp / log / add, each of at most 2^-53 L.  Means and term expectations: 4 B + 1e-13 (the exponent of
    p_t carries three such errors, plus the sums)."""
    L = sum(abs(w) for w in terms.values()) + n * np.log(2.0)
    return 2.0 ** -53 * (len(terms) + 4 * n) * L


# ---- the models of the tests -----------------------------------------------------------------------------------------------------
def lattice(r, c, seed=0, field=True, periodic=False, scale=0.6):
    """r x c square lattice, row-major 1-based spins; periodic: the rows close into rings (a cylinder)"""
    rng = np.random.default_rng(seed)
    t = {}
    idx = lambda i, j: i * c + j + 1  # noqa: E731
    for i in range(r):
        for j in range(c):
            if j + 1 < c:
                t[(idx(i, j), idx(i, j + 1))] = float(rng.uniform(-scale, scale))
            elif periodic and c > 2:
                t[(idx(i, 0), idx(i, j))] = float(rng.uniform(-scale, scale))
            if i + 1 < r:
                t[(idx(i, j), idx(i + 1, j))] = float(rng.uniform(-scale, scale))
            if field:
                t[(idx(i, j),)] = float(rng.uniform(-0.2, 0.2))
    return t, r * c


def chimera(m, seed=0):
    """Chimera C_m: m x m cells of K_{4,4}; side 0 couples down the column of cells, side 1 along the row"""
    rng = np.random.default_rng(seed)
    t = {}
    q = lambda i, j, s, k: ((i * m + j) * 2 + s) * 4 + k + 1  # noqa: E731
    for i in range(m):
        for j in range(m):
            for a in range(4):
                for b in range(4):
                    t[(q(i, j, 0, a), q(i, j, 1, b))] = float(rng.uniform(-0.5, 0.5))
                if i + 1 < m:
                    t[(q(i, j, 0, a), q(i + 1, j, 0, a))] = float(rng.uniform(-0.5, 0.5))
                if j + 1 < m:
                    t[(q(i, j, 1, a), q(i, j + 1, 1, a))] = float(rng.uniform(-0.5, 0.5))
    for v in range(1, 8 * m * m + 1):
        t[(v,)] = float(rng.uniform(-0.1, 0.1))
    return t, 8 * m * m


def tree(n, seed=0, field=True, back=None):
    """a random recursive tree: spin v hangs from a uniformly drawn earlier spin; back: from one of the `back` spins before it (a
    uniform tree grows hubs, and the frontier of the greedy order with them: width 857 at n = 16384, against 6 with back=8)"""
    rng = np.random.default_rng(seed)
    t = {}
    for v in range(2, n + 1):
        t[(int(rng.integers(1 if back is None else max(1, v - back), v)), v)] = float(rng.uniform(-0.8, 0.8))
    if field:
        for v in range(1, n + 1):
            t[(v,)] = float(rng.uniform(-0.3, 0.3))
    return t, n


def triples_ladder(n, seed=0):
    """a chain with the three-body terms (v, v+1, v+2), the pairs (v, v+1) and fields"""
    rng = np.random.default_rng(seed)
    t = {}
    for v in range(1, n - 1):
        t[(v, v + 1, v + 2)] = float(rng.uniform(-0.5, 0.5))
    for v in range(1, n):
        t[(v, v + 1)] = float(rng.uniform(-0.5, 0.5))
    for v in range(1, n + 1):
        t[(v,)] = float(rng.uniform(-0.2, 0.2))
    return t, n


def regular3(n, seed=0):
    """a random simple 3-regular graph (pairing model, redrawn until simple), no fields"""
    rng = np.random.default_rng(seed)
    while True:
        p = rng.permutation(np.repeat(np.arange(1, n + 1), 3)).reshape(-1, 2)
        if all(a != b for a, b in p) and len({(min(a, b), max(a, b)) for a, b in p}) == len(p):
            break
    return {(int(min(a, b)), int(max(a, b))): float(rng.uniform(-0.5, 0.5)) for a, b in p}, n


def triples_only(n=12, seed=0):
    """three-body terms (v, v+1, v+2) alone and a single field on spin 1: under the greedy order every second step applies no term
    and retires no spin, so its backward step has nothing to sum and still has to hand beta on"""
    rng = np.random.default_rng(seed)
    t = {(v, v + 1, v + 2): float(rng.uniform(-0.9, 0.9)) for v in range(1, n - 1)}
    t[(1,)] = 0.3
    return t, n


def islands(count=40, seed=0):
    """`count` components of 2 to 5 spins each -- a closed ring of pairs (a chain for two spins), one term over the whole island
    where it has three or more, a field on its first spin -- with a spin in no term after every fourth: many components in one call"""
    rng = np.random.default_rng(seed)
    t, v = {}, 1
    for c in range(count):
        size = 2 + c % 4
        sp = list(range(v, v + size))
        for a in range(size if size > 2 else 1):
            t[tuple(sorted((sp[a], sp[(a + 1) % size])))] = float(rng.uniform(-0.8, 0.8))
        if size > 2:
            t[tuple(sp)] = float(rng.uniform(-0.5, 0.5))
        t[(sp[0],)] = float(rng.uniform(-0.4, 0.4))
        v += size + (1 if c % 4 == 3 else 0)
    return t, v - 1


def order5(seed=0):
    """a 12-spin ring of pairs with fields and one order-5 term across it"""
    rng = np.random.default_rng(seed)
    t = {(v, v % 12 + 1) if v < 12 else (1, 12): float(rng.uniform(-0.7, 0.7)) for v in range(1, 13)}
    t[(2, 4, 7, 9, 11)] = 0.9
    t[(3, 6, 10)] = -0.4
    for v in range(1, 13):
        t[(v,)] = float(rng.uniform(-0.3, 0.3))
    return t, 12


def stiff_chain(n=60, seed=0):
    """an open chain whose fields and couplings are all +-150"""
    rng = np.random.default_rng(seed)
    t = {(v, v + 1): float(rng.choice([-150.0, 150.0])) for v in range(1, n)}
    for v in range(1, n + 1):
        t[(v,)] = float(rng.choice([-150.0, 150.0]))
    return t, n


def mixed_conventions():
    """a duplicated spin, an empty key, a key that cancels to nothing, zero weights (one spin, and two), an isolated spin (9) and two
    components ({1, 2, 3, 4} and {5, 6, 7, 8}); n = 9"""
    return {(1, 2): 0.4, (2, 3): -0.3, (3, 4, 4, 1): 0.25, (1, 2, 3): 0.2, (2, 2, 4): -0.15, (): 0.37, (3, 3): 0.11, (2,): 0.0,
            (1, 7): 0.0, (5, 6): 0.5, (6, 7): -0.45, (7, 8): 0.35, (5, 8): 0.3, (5, 6, 7, 8): -0.2, (6,): 0.1, (4, 3): 0.05}, 9
