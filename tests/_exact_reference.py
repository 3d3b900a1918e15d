"""numpy restatement of gml_model_exact (include/gml.h) by brute force in np.longdouble, for components of at most 20 spins: every
state of a component is listed, its energy is the plain sum over the terms, and an expectation is the plain sum of the probabilities
with the key's sign.  The rules of the contract are here too: a spin named twice cancels, a zero weight joins nothing, an empty key
adds its weight to log Z, a spin in no term gives ln 2, log Z adds over the connected components and expectations multiply.
Models are {1-based key tuple: weight} dicts; queries are 1-based key tuples."""
import numpy as np

LD = np.longdouble
MAX_SPINS = 20


def reduce_key(key):
    """the distinct spins of a key after cancellation, ascending"""
    out = []
    for v in key:
        v = int(v)
        if v in out:
            out.remove(v)
        else:
            out.append(v)
    return tuple(sorted(out))


def components(terms, n):
    """the connected components of the term hypergraph as ascending lists of 1-based spins, in the order of their smallest spin"""
    parent = list(range(n + 1))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for key, w in terms.items():
        sp = reduce_key(key)
        if w != 0.0:
            for v in sp[1:]:
                parent[find(v)] = find(sp[0])
    blocks = {}
    for i in range(1, n + 1):
        blocks.setdefault(find(i), []).append(i)
    return sorted(blocks.values())


class Component:
    """one component enumerated: log_z and the probabilities of its 2^sb states (bit i set <=> its i-th spin is -1)"""

    def __init__(self, spins, cterms):
        assert len(spins) <= MAX_SPINS, len(spins)
        self.spins = list(spins)
        self.local = {v: i for i, v in enumerate(self.spins)}
        self._seen = {}
        states = np.arange(1 << len(spins), dtype=np.uint32)
        self.down = [((states >> i) & 1).astype(bool) for i in range(len(spins))]
        E = np.zeros(len(states), dtype=LD)
        for key, w in cterms:
            E += np.where(self.negative(key), -LD(w), LD(w))
        m = E.max()
        p = np.exp(E - m)
        Z = p.sum()
        self.log_z = m + np.log(Z)
        self.p = p / Z

    def negative(self, key):
        """where the product of the key's spins (reduced, 1-based, all of this component) is -1"""
        neg = np.zeros(1 << len(self.spins), dtype=bool)
        for v in key:
            neg ^= self.down[self.local[v]]
        return neg

    def expectation(self, key):
        """of a reduced key of this component: the sum of p with the key's sign, 1 - 2 sum_{product = -1} p (kept once computed)"""
        if key not in self._seen:
            self._seen[key] = LD(1) - 2 * self.p[self.negative(key)].sum() if key else LD(1)
        return self._seen[key]


class ExactModel:
    """log_z, mean [n], corr [n, n] of a model, and expectation(key) of any key; all np.longdouble"""

    def __init__(self, terms, n):
        self.n = n
        self.log_z = LD(0)
        blocks = components(terms, n)
        self.of = {v: b for b, blk in enumerate(blocks) for v in blk}
        cterms = [[] for _ in blocks]
        for key, w in terms.items():
            sp = reduce_key(key)
            if not sp:
                self.log_z += LD(w)  # the empty key (a zero weight adds nothing)
            elif w != 0.0:
                cterms[self.of[sp[0]]].append((sp, w))
        self.comp = [Component(blk, ct) for blk, ct in zip(blocks, cterms)]
        for c in self.comp:
            self.log_z += c.log_z  # (a spin in no term: one state of each sign at energy 0, ln 2)
        self.mean = np.array([self.expectation((i,)) for i in range(1, n + 1)], dtype=LD)

    def expectation(self, key):
        """the product over the components of the expectations of the key's restrictions; the empty key gives 1"""
        parts = {}
        for v in reduce_key(key):
            parts.setdefault(self.of[v], []).append(v)
        out = LD(1)
        for b in sorted(parts):
            out *= self.comp[b].expectation(tuple(parts[b]))
        return out

    @property
    def corr(self):
        C = np.ones((self.n, self.n), dtype=LD)
        for i in range(self.n):
            for j in range(i + 1, self.n):
                C[i, j] = C[j, i] = self.expectation((i + 1, j + 1))
        return C


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
def independent_log_z(h):
    """log Z = sum_i ln(2 cosh h_i) of independent spins with fields h"""
    h = np.asarray(h, dtype=LD)
    return np.sum(np.log(2 * np.cosh(h)))


def chain_log_z(J):
    """log Z = n ln 2 + sum_k ln cosh J_k of an open chain of n = len(J) + 1 spins without fields"""
    J = np.asarray(J, dtype=LD)
    return (len(J) + 1) * np.log(LD(2)) + np.sum(np.log(np.cosh(J)))


def chain_corr(J):
    """<s_i s_j> = prod_{i <= k < j} tanh J_k of that chain: [n, n]"""
    t = np.tanh(np.asarray(J, dtype=LD))
    n = len(t) + 1
    C = np.ones((n, n), dtype=LD)
    for i in range(n):
        for j in range(i + 1, n):
            C[i, j] = C[j, i] = np.prod(t[i:j])
    return C


# ---- the models of the tests -----------------------------------------------------------------------------------------------------
def dense_model(spins, seed, scale=0.3, extra=4):
    """random dense pairwise terms plus fields plus `extra` terms of orders 3 to 6 (as far as the spins reach) on the 1-based `spins`"""
    rng = np.random.default_rng(seed)
    spins = list(spins)
    terms = {(v,): float(rng.normal(scale=scale)) for v in spins}
    for a in range(len(spins)):
        for b in range(a + 1, len(spins)):
            terms[(spins[a], spins[b])] = float(rng.normal(scale=scale))
    for e in range(extra):
        k = 3 + e % 4
        if k <= len(spins):
            terms[tuple(int(v) for v in sorted(rng.choice(spins, size=k, replace=False)))] = float(rng.normal(scale=scale))
    return terms


def chain_model(spins, seed, scale=0.5):
    """an open chain without fields along the 1-based `spins`: (terms, J)"""
    rng = np.random.default_rng(seed)
    J = rng.normal(scale=scale, size=len(spins) - 1)
    return {(spins[k], spins[k + 1]): float(J[k]) for k in range(len(J))}, J


def abs_weight(terms):
    return float(sum(abs(w) for w in terms.values()))
