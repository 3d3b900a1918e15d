"""Host model of gml_problem_create_sampled_elim (include/gml.h) in numpy FP64, written from the header's contract: the plan of
_elim_reference.plan, the slot rule and the launch list restated, the forward tables, and every sample's backward walk as the
contract words it.  It shares no code with the library.  Models are {1-based key tuple: weight} dicts.

The forward tables use the device's expression and order -- phi summed from 0.0 in the caller's term order, x = in + phi, the sum of
exp(x - max) in candidate order -- so they differ from the device's by the roundings of exp and log alone, which the elimination's
derived bound covers (_elim_reference.bound).  draw() therefore also returns, per sample, the smallest gap of its walk: over the
launches, |u total - the nearest running sum| / total.  Where every gap is far above that bound, the device has to make the same
picks, and its rows can be held to these with `==`."""
import numpy as np

from _elim_reference import neighbours, plan, reduce_key
from _mcmc_chains_reference import u01

MAX_RETIRE = 3
FREE_STREAM = 1 << 62


def retire(cur, now):
    """The slot rule.  cur[p]: the spin at bit p; now: the positions that go, ascending.  The survivors below the new size keep their
    bit, the others fill the freed bits in ascending order.  Returns the new list of spins by bit."""
    k2 = len(cur) - len(now)
    late = [cur[p] for p in range(k2, len(cur)) if p not in now]  # the survivors that have to move, ascending
    return [cur[p] if p not in now else late.pop(0) for p in range(k2)]


def launch_list(terms, n, order=None):
    """(launches, free): the forward launches of the whole call in their numbering -- the components in the order of their smallest
    spin, each one's launches in forward order -- and the spins in no term.  A launch: kin, the scope's spins by bit, the retiring
    bits (positions in the scope as this launch sees it, ascending) with their spins, the output's spins by bit, the masks and weights
    of the step's terms (first launch of a step only), and `last`: it is the last launch of its component."""
    seq, _, _, _ = plan(terms, n, order)
    adj = neighbours(terms, n)
    pos = {v: t for t, v in enumerate(seq)}
    last = {v: max([pos[v]] + [pos[u] for u in adj[v]]) for v in seq}
    step_terms = [[] for _ in range(n)]
    for key, w in terms.items():
        sp = reduce_key(key)
        if w != 0.0 and sp:
            step_terms[max(pos[v] for v in sp)].append((sp, float(w)))
    launches, free, cur = [], [], []
    for t, v in enumerate(seq):
        if not cur and last[v] == t and not step_terms[t]:
            free.append(v)
            continue
        kin = len(cur)
        cur = cur + [v]
        scope = list(cur)
        masks = [sum(1 << scope.index(u) for u in sp) for sp, _ in step_terms[t]]
        todo = [u for u in scope if last[u] == t]  # in ascending scope position
        first = True
        while first or todo:
            now = sorted(cur.index(u) for u in todo[:MAX_RETIRE])
            todo = todo[MAX_RETIRE:]
            nxt = retire(cur, now)
            launches.append(dict(kin=kin if first else len(cur), scope=list(cur), rbit=now, rspin=[cur[p] for p in now], out=nxt,
                                 masks=masks if first else [], weights=[w for _, w in step_terms[t]] if first else [], last=False))
            cur, first = nxt, False
        launches[-1]["last"] = not cur
    return launches, free


def _parity(x):
    x = x.copy()
    for s in (16, 8, 4, 2, 1):
        x ^= x >> s
    return x & 1


def _scope_of(L, j):
    """the scope state whose surviving bits are those of output index j (array), the retiring bits 0"""
    s = np.zeros_like(j)
    for b, u in enumerate(L["out"]):
        s |= ((j >> b) & 1) << L["scope"].index(u)
    return s


def forward(launches):
    """adds to every launch X [2^|scope|]: x(s) = in[s & inmask] + phi(s) over the launch's scope, and returns nothing; the output
    table of a launch is the input of the next, the first launch of a component reads alpha_0 = [0.0]"""
    table = np.zeros(1)
    for L in launches:
        k = len(L["scope"])
        s = np.arange(1 << k, dtype=np.int64)
        phi = np.zeros(1 << k)
        for m, w in zip(L["masks"], L["weights"]):
            phi += np.where(_parity(s & m) == 1, -w, w)
        L["X"] = table[s & ((1 << L["kin"]) - 1)] + phi
        base = _scope_of(L, np.arange(1 << len(L["out"]), dtype=np.int64))
        r = len(L["rbit"])
        if r == 0:
            table = L["X"][base]
        else:
            x = np.stack([L["X"][base | _bits(L, c)] for c in range(1 << r)])
            m = x.max(axis=0)
            total = np.zeros_like(m)
            for c in range(1 << r):
                total = total + np.exp(x[c] - m)
            table = m + np.log(total)
        if L["last"]:
            assert table.shape == (1,)
            table = np.zeros(1)


def _bits(L, c):
    return sum(1 << p for i, p in enumerate(L["rbit"]) if c >> i & 1)


def draw(terms, n, N, seed, order=None):
    """(states int8 [N, n], gap [N], logp [N]): the draws of gml_problem_create_sampled_elim, every sample's smallest gap and
    the sum of log(p_c / total) along its walk (which telescopes to E(s) - log Z)"""
    launches, free = launch_list(terms, n, order)
    forward(launches)
    k = np.arange(N, dtype=np.uint64)
    states = np.zeros((N, n), dtype=np.int8)
    gap, logp = np.full(N, np.inf), np.zeros(N)
    j = np.zeros(N, dtype=np.int64)
    for l in range(len(launches) - 1, -1, -1):
        L = launches[l]
        if L["last"]:
            assert not j.any()  # the walk arrives at a component's last launch with index 0
        base, r = _scope_of(L, j), len(L["rbit"])
        inmask = (1 << L["kin"]) - 1
        if r == 0:
            j = base & inmask
            continue
        x = np.stack([L["X"][base | _bits(L, c)] for c in range(1 << r)])
        p = np.exp(x - x.max(axis=0))
        run = np.zeros_like(p)
        total = np.zeros(N)
        for c in range(1 << r):
            total = total + p[c]
            run[c] = total
        target = u01(seed, l, k) * total
        over = run > target
        pick = np.where(over.any(axis=0), over.argmax(axis=0), (1 << r) - 1)  # the smallest c that exceeds; the last if none does
        gap = np.minimum(gap, np.abs(run - target).min(axis=0) / total)
        logp += np.log(p[pick, np.arange(N)] / total)
        nxt = base.copy()
        for i, (pbit, u) in enumerate(zip(L["rbit"], L["rspin"])):
            minus = (pick >> i) & 1
            states[:, u - 1] = np.where(minus == 1, -1, 1)
            nxt |= minus << pbit
        j = nxt & inmask
    for v in free:
        states[:, v - 1] = np.where(u01(seed, FREE_STREAM + v - 1, k) < 0.5, 1, -1)
    assert (states != 0).all()
    return states, gap, logp


def energy(terms, states):
    """E(s) = sum_t w_t prod_{i in t} s_i per row, FP64 in the dict's order"""
    e = np.zeros(len(states))
    for key, w in terms.items():
        sp = reduce_key(key)
        e += w * (np.prod(states[:, [v - 1 for v in sp]].astype(np.float64), axis=1) if sp else 1.0)
    return e


# ---- the models and cases of the tests ---------------------------------------------------------------------------------------------
def complete(n=7, seed=0):
    """the complete graph K_n with fields: the last step retires all n spins at once (n = 7: launches of 3, 3 and 1 spins, the only
    shape here with tables between the launches of one step)"""
    rng = np.random.default_rng(seed)
    t = {(a, b): float(rng.uniform(-0.6, 0.6)) for a in range(1, n + 1) for b in range(a + 1, n + 1)}
    for v in range(1, n + 1):
        t[(v,)] = float(rng.uniform(-0.3, 0.3))
    return t, n


def ferromagnet(r=6, c=6, J=1.0):
    """a field-free r x c lattice with every coupling J: P(s) = P(-s) exactly"""
    from _elim_reference import lattice
    t, n = lattice(r, c, field=False)
    return {k: J for k in t}, n


def perturbed_greedy(terms, n, seed):
    """the greedy order with every second pair of consecutive steps swapped at random (a swap widens a scope by at most one spin)"""
    order = np.array(plan(terms, n)[0])
    for i in np.flatnonzero(np.random.default_rng(seed).integers(0, 2, size=n // 2)):
        order[[2 * i, 2 * i + 1]] = order[[2 * i + 1, 2 * i]]
    return order


def draw_cases():
    """name -> (terms, n, order or None, seed, N): every case whose rows the device is held to with `==`, and the cases whose seed
    the host model has vetted (tests/test_host_elim_draw_reference.py: the gaps, the statistics at that seed)"""
    import _elim_reference as R
    l44 = R.lattice(4, 4, seed=3)
    cases = {
        "lattice_4x4": (*l44, None, 11, 4096),
        "ladder_14": (*R.triples_ladder(14, seed=2), None, 12, 4096),
        "chimera_2": (*R.chimera(2), None, 13, 4096),
        "order5": (*R.order5(), None, 14, 4096),
        "mixed_conventions": (*R.mixed_conventions(), None, 15, 4096),
        "field_free_tree_200": (*R.tree(200, seed=6, field=False), None, 16, 4096),
        "complete_7": (*complete(7), None, 17, 4096),
        "lattice_4x4_perturbed": (*l44, perturbed_greedy(*l44, seed=5), 18, 4096),
        "lattice_4x4_permuted": (*l44, np.random.default_rng(2).permutation(16) + 1, 19, 4096),
        "lattice_8x8": (*R.lattice(8, 8), None, 20, 65536),
        "ferromagnet_6x6": (*ferromagnet(), None, 21, 4096),
    }
    return cases
