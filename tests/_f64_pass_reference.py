"""Host model of the FP64 pass (k_fwd_f64 and k_bwd_f64, csrc/gml_kernels_f64gemm.hip) in np.longdouble, written from the kernels'
comments; it imports and calls nothing compiled from them.  The design matrix in internal column order comes from
tests/_i8_pack_reference.py (stat_keys, stat_bits), to which tests/test_gpu_i8_pack_state.py holds the device's Xb and Xtb images;
a parameter's column is found by looking the other spins of its key up in stat_keys, at any interaction order (Shape.colidx).
tests/test_host_f64_pass_reference.py holds this file to a brute-force triple loop; tests/test_gpu_f64_pass_exact.py holds the
device to it.

For a row r with node u (rowcol), the constant column cconst and the weights w (0 on the padding samples), x the +-1 statistics
(+1 on the padding samples and beyond the Qf statistics columns), s the node's own spin (+1 on the padding samples):
  A_k = sum_{c < Qf} theta_c x_kc + theta_cconst,   E_k = s_k A_k
  RISE, logRISE (Z):  e_k = w_k exp(-E_k),              V_k = -e_k s_k
  RPLE:               e_k = w_k log(1 + exp(-2 E_k)),   V_k = -2 w_k sigma(-2 E_k) s_k,   sigma(t) = 1 / (1 + exp(-t))
  f = sum_k e_k
  products (Theta holds the direction p, V the objective pass's V_old):  V_k = h_k A_k,  h = h' = -V_old s (RISE, logRISE),
      h = 2 h' (1 - h' / 2w) (RPLE; 0 where w = 0)
  G_c = sum_k V_k x_kc (c < Qf),   G_cconst = sum_k V_k,   every other column 0
  rows with rowcol < 0 keep their V.

Error bounds, per element, u = 2^-53 (all follow from the code; EXP_ULPS is the one measured constant).  They are FIRST-ORDER bounds:
the factors are added, so the cross terms of products such as (1 + expm1 B_E)(1 + EXP_ULPS u)(1 + u) - 1 -- of the order of u^2 and
u B_E, below 1e-27 of the element here -- are left out, as are the 1 / (1 - n u) factors of the sums other than E's:
  E:   B_E = m u sum_c |theta_c| / (1 - m u), m = the row's non-zero entries (constant column included): m additions, each rounded
       once, in any order -- the products with +-1 are exact and adding a zero product is exact.
  V, exp forms:  |V| (expm1(B_E) + (EXP_ULPS + 1) u): the energy's error through exp, exp itself, the product with w.  (-e s is exact.)
  V, RPLE:       |V| (expm1(2 B_E) + (EXP_ULPS + 3) u): sg = 1 / (1 + exp(2 E)) -- 2 E exact, exp, the sum (a relative error d of
                 exp(2E) is at most d of 1 + exp(2E)), the division; -2 w is exact, its product with sg is rounded, the one with s is not.
  e, RPLE:       t = -2 E.  t <= 0: sp = log1p(exp(t)): a relative error d of y = exp(t) is at most d of log1p(y)
                 (y / (1 + y) <= log1p(y)), so  e (expm1(2 B_E) + (2 EXP_ULPS + 1) u)  with log1p's own error and the product with w.
                 t > 0: sp = t + l, l = log1p(exp(-t)): t carries 2 B_E absolutely, l as above, the sum and the product one rounding
                 each:  w (2 B_E + l (expm1(2 B_E) + 2 EXP_ULPS u)) + 2 u e.
  f:   the sum of the element bounds + (8 + 4 + Kp / 128) u sum_k e_k: eight adds per lane, four shuffles, one atomic per
       128-sample wave.
  G given the device's own V (the cut):  (kchunk + nsplit) u sum_k |V_k| per column below Qf;  (kchunk / 4 + 2 + nsplit) u sum_k |V_k|
       for the constant column (a lane adds every fourth 8-sample run of its chunk, two shuffles, one atomic per chunk); kchunk and
       nsplit as launch_bwd_f64 computes them (bwd_plan).
  products given the device's V_old:  h' = -V_old s is exact.  |h| |A| u + (|h| B_A + e_h |A| + e_h B_A) (1 + u) with B_A the bound
       B_E of the direction's row and e_h = 0 (RISE, logRISE) or u (2 |h'| + |h|) (RPLE: the division, the difference, the product).
The model's own error: the +-1 sums are exact float64 GEMMs of 26-bit pieces (pm1_dot: 2^-79 of a column's largest entry per
term), everything else is np.longdouble (2^-64): below a thousandth of any bound above.

EXP_ULPS: the relative error, in units of u, allowed to the device library's double exp (and log1p).  Measured on the dyadic
cases of tests/test_gpu_f64_pass_exact.py, where E is exact and V differs from this model by exp and one product only: the worst
|V_dev - V| / (u |V|) - 1 seen over RISE and logRISE on all shapes is recorded in HISTORY.md (section 17: 0.982 on an MI355X); the
constant is twice that, and not less than 2: 2.  The dyadic cases re-assert it on every run."""
import numpy as np

import _i8_pack_reference as R

LD = np.longdouble
U = 2.0 ** -53
EXP_ULPS = 2.0
FORM_ID = {"RISE": 0, "logRISE": 1, "RPLE": 2}


# ---------------------------------------------------------------------------------------------------------------------------
# exact +-1 GEMM
# ---------------------------------------------------------------------------------------------------------------------------
def pm1_dot(X, A):
    """X (+-1 float64 [k, m], m < 2^27) @ A ([m, F]) in np.longdouble: A is cut per column into three 26-bit pieces whose float64
    GEMMs with X are integer sums below 2^53, so what is lost is 2^-79 of the column's largest entry per term"""
    A = np.asarray(A, dtype=LD)
    mx = np.abs(A).max(axis=0) if A.shape[0] else np.zeros(A.shape[1], dtype=LD)
    ex = np.frexp(np.where(mx > 0, mx, 1).astype(np.float64))[1]
    s = np.ldexp(LD(1), ex + 1).astype(LD)  # (+ 1: the float64 rounding of mx may round up across a power of two)
    y = A / s
    out = np.zeros((X.shape[0], A.shape[1]), dtype=LD)
    for sh in (26, 52, 78):
        piece = np.round(y * LD(2.0) ** sh) / LD(2.0) ** sh
        out += (X @ piece.astype(np.float64)).astype(LD)
        y = y - piece
    return out * s


# ---------------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------------
def counts_pow2(K, seed, zeros=0):
    """integer counts floor(10^U(0, 3)) rescaled so that their total M is a power of two (w_k = c_k / M is then dyadic), `zeros` of
    them zero"""
    rng = np.random.default_rng(seed)
    c = np.floor(10 ** rng.uniform(0, 3, size=K))
    M = 1 << int(np.round(np.log2(c.sum())))
    c = np.maximum(1.0, np.floor(c * (M / c.sum())))
    order = np.argsort(-c, kind="stable")
    d = int(M - c.sum())
    while d:
        idx = order[:min(abs(d), K)]
        idx = idx[c[idx] + np.sign(d) >= 1]
        c[idx] += np.sign(d)
        d -= int(np.sign(d)) * len(idx)
    if zeros:
        z = rng.choice(np.arange(K), size=zeros, replace=False)
        z = z[z != order[0]]
        c[order[0]] += c[z].sum()
        c[z] = 0.0
    assert c.sum() == M and (c >= 0).all()
    return c, M


def _row_list(n, count, seed):
    rng = np.random.default_rng(seed)
    rest = rng.choice(np.arange(n), size=count - 4, replace=True)
    return np.concatenate([[0, n - 1, 3, 3], rest]).astype(np.int64)  # node 0, node n - 1, a repeated node


#        n, order, K, rows (None: all nodes), zero counts, seed
SHAPES = {"S1": (5, 2, 37, None, 0, 1), "S2": (70, 2, 700, 45, 2, 2), "S3": (100, 2, 4500, None, 3, 3), "S4": (48, 3, 1100, 40, 2, 4),
          "S5": (40, 2, 6200, None, 0, 5), "T2": (4, 2, 11, None, 1, 6), "T3": (4, 3, 11, None, 0, 7),  # (T2, T3: the host test's)
          # orders 5 to 8: keys of four to seven spins besides the node's own, and an order above n (keys that are mostly -1)
          "H5": (11, 5, 1500, None, 2, 8), "H6": (10, 6, 1100, None, 2, 9), "H7": (12, 7, 700, None, 1, 10), "H8": (9, 8, 2100, None, 2, 11),
          "E7": (7, 8, 300, None, 1, 12), "E3": (3, 8, 40, None, 1, 13), "T5": (5, 5, 13, None, 0, 14)}  # (T5: the host test's)
HIGH = ["H5", "H6", "H7", "H8", "E7", "E3"]


def closed_form_column(n, rest, cconst):
    """the column of the statistic of the spins `rest` (ascending, at most two) in closed form: what Shape.column computed before it
    looked the key up in stat_keys; tests/test_host_f64_pass_reference.py holds the lookup to it at orders 2 and 3"""
    if not rest:
        return cconst
    if len(rest) == 1:
        return rest[0]
    a, b = rest
    return n + a * n - a * (a + 1) // 2 + (b - a - 1)


class Shape:
    """One problem of tests/test_gpu_f64_pass_exact.py on the host: spins, dyadic weights, the +-1 design matrix in internal
    column order, the node's own spins, the row list."""

    def __init__(self, name, multi_keys=None):
        self.name = name
        self.n, self.order, self.K, nrows, zeros, seed = SHAPES[name]
        n, K = self.n, self.K
        rng = np.random.default_rng(100 + seed)
        self.spins = np.where(rng.random((K, n)) < 0.5, 1, -1).astype(np.int8)
        self.counts, self.M = counts_pow2(K, seed, zeros)
        self.nodes = np.arange(n, dtype=np.int64) if nrows is None else _row_list(n, nrows, seed)
        self.R = len(self.nodes)
        self.Rp = (self.R + 31) // 32 * 32
        self.Kp = (K + 1023) // 1024 * 1024
        self.keys = R.stat_keys(n, self.order)
        self.Qf = len(self.keys)
        self.Qfp = (self.Qf + 63) // 64 * 64
        self.cconst, self.Qp = self.Qfp, self.Qfp + 64
        self.w = np.zeros(self.Kp)
        self.w[:K] = self.counts / self.M
        bits = R.stat_bits(self.spins, self.keys, self.Qf, self.Kp)
        self.X = 1.0 - 2.0 * bits.astype(np.float64)  # [Qf][Kp], +1 on the padding samples
        sb = np.ones((n, self.Kp))
        sb[:, :K] = self.spins.T
        self.S = sb[self.nodes]  # [R][Kp] the rows' own spins
        self.real = np.arange(self.Kp) < K
        self.colidx = {tuple(int(i) for i in k if i >= 0): c for c, k in enumerate(self.keys)}  # sorted key -> column, any order
        if self.order == 2:
            self.P = n
        else:
            self.pkeys = {int(u): multi_keys(n, self.order, int(u)) for u in set(self.nodes.tolist())}
            self.P = len(self.pkeys[int(self.nodes[0])])
        self.ld_rows = np.arange(self.R)  # the rows the long-double comparisons cover: all of them, on every shape

    def column(self, u, j):
        """internal column of parameter j (reference order) of node u"""
        if self.order == 2:
            return self.cconst if j == u else j
        rest = tuple(sorted(i for i in self.pkeys[u][j] if i != u))
        return self.colidx[rest] if rest else self.cconst

    def cols(self, u):
        return np.array([self.column(int(u), j) for j in range(self.P)])

    def internal(self, th):
        """the rows th [R][P] (reference order) in the internal column layout [R][Qp]"""
        out = np.zeros((self.R, self.Qp))
        for r, u in enumerate(self.nodes):
            out[r, self.cols(u)] = th[r]
        return out

    def ref_stats(self, u):
        """the statistics of node u in the reference's parameter order, from the spins alone: float64 +-1 [K][P]"""
        S = self.spins.astype(np.float64)
        if self.order == 2:
            X = S * S[:, [u]]
            X[:, u] = S[:, u]
            return X
        X = np.ones((self.K, self.P))
        for j, key in enumerate(self.pkeys[u]):
            for i in key:
                X[:, j] *= S[:, i]
        return X


def bwd_plan(Kp, Qf, ngroups):
    """(nsplit, kchunk) of launch_bwd_f64: about two rounds of workgroups over 256 CUs, chunks of at least 2048 samples, rounded
    up to 64"""
    gx = max((Qf + 1023) // 1024, 1)
    nsplit = (512 + gx * ngroups - 1) // (gx * ngroups)
    nsplit = max(1, min(nsplit, max(Kp // 2048, 1)))
    kchunk = (Kp + nsplit - 1) // nsplit
    kchunk = (kchunk + 63) // 64 * 64
    return (Kp + kchunk - 1) // kchunk, kchunk


# ---------------------------------------------------------------------------------------------------------------------------
# the pass
# ---------------------------------------------------------------------------------------------------------------------------
def bound_E(TH, Qf, cconst):
    """B_E per row of the internal-layout rows TH [R][Qp]"""
    a = np.concatenate([TH[:, :Qf], TH[:, cconst:cconst + 1]], axis=1)
    m = (a != 0).sum(axis=1).astype(LD)
    return m * U * np.abs(a).astype(LD).sum(axis=1) / (1 - m * U)


def energies(sh, TH, rows):
    """A [len(rows)][Kp] of the internal-layout rows TH[rows]"""
    return pm1_dot(np.ascontiguousarray(sh.X.T), TH[rows, :sh.Qf].T).T + TH[rows, sh.cconst].astype(LD)[:, None]


def forward(form, A, s, w, BE, exp_ulps=EXP_ULPS):
    """V, e and their bounds [rows][Kp] from the energies' A, the rows' own spins s, the weights w and B_E [rows]"""
    E = s * A
    w = w.astype(LD)[None, :]
    BE = np.asarray(BE, dtype=LD)[:, None]
    if form != "RPLE":
        e = w * np.exp(-E)
        V = -e * s
        rel = np.expm1(BE) + (exp_ulps + 1) * U
        return dict(E=E, V=V, e=e, bV=np.abs(V) * rel, be=e * rel)
    t = -2 * E
    l = np.log1p(np.exp(-np.abs(t)))
    sp = np.where(t > 0, t + l, l)
    e = w * sp
    V = -2 * w / (1 + np.exp(2 * E)) * s
    d = np.expm1(2 * BE)
    be = np.where(t > 0, w * (2 * BE + l * (d + 2 * exp_ulps * U)) + 2 * U * e, e * (d + (2 * exp_ulps + 1) * U))
    return dict(E=E, V=V, e=e, bV=np.abs(V) * (d + (exp_ulps + 3) * U), be=be)


def f_of(o, Kp):
    """f and its bound per row"""
    es = o["e"].sum(axis=1)
    return es, o["be"].sum(axis=1) + (8 + 4 + Kp / 128) * U * es


def product(form, Vold, A, s, w, BA):
    """V of a product pass and its bound from the device's V_old [rows][Kp] (float64), the direction's A and B_A [rows]"""
    hp = (-Vold * s).astype(LD)  # exact
    BA = np.asarray(BA, dtype=LD)[:, None]
    if form == "RPLE":
        w2 = (2 * w).astype(LD)[None, :]
        pos = w2 > 0
        h = np.where(pos, 2 * hp * (1 - hp / np.where(pos, w2, 1)), 0)
        eh = np.where(pos, U * (2 * np.abs(hp) + np.abs(h)), 0)
    else:
        h, eh = hp, 0
    V = h * A
    ah, aA = np.abs(h), np.abs(A)
    return V, ah * aA * U + (ah * BA + eh * aA + eh * BA) * (1 + U)


def backward(sh, V, plan):
    """G [rows][Qp] and its bound from the device's V [rows][Kp] (float64)"""
    nsplit, kchunk = plan
    G = np.zeros((len(V), sh.Qp), dtype=LD)
    B = np.zeros((len(V), sh.Qp), dtype=LD)
    G[:, :sh.Qf] = pm1_dot(sh.X, V.T).T
    G[:, sh.cconst] = V.astype(LD).sum(axis=1)
    sa = np.abs(V).astype(LD).sum(axis=1)
    B[:, :sh.Qf] = ((kchunk + nsplit) * U * sa)[:, None]
    B[:, sh.cconst] = (kchunk / 4 + 2 + nsplit) * U * sa
    return G, B


def ratio(dev, mod, bnd):
    """max |dev - mod| / bnd over all elements; an element with bound 0 must be equal (inf otherwise), and so must a non-finite one"""
    dev = np.asarray(dev)
    if not np.isfinite(dev).all():
        return float("inf")
    d = np.abs(dev.astype(LD) - mod)
    bnd = np.broadcast_to(np.asarray(bnd, dtype=LD), d.shape)
    z = bnd == 0
    if (d[z] != 0).any():
        return float("inf")
    return float((d[~z] / bnd[~z]).max()) if (~z).any() else 0.0


def check_untouched(V_after, V_before, Rrows):
    """rows Rrows .. of V (rowcol < 0, and the groups no pass listed) keep their bits"""
    a, b = np.ascontiguousarray(V_after[Rrows:]), np.ascontiguousarray(V_before[Rrows:])
    return np.array_equal(a.view(np.int64), b.view(np.int64))


# ---------------------------------------------------------------------------------------------------------------------------
# theta families (reference order [R][P])
# ---------------------------------------------------------------------------------------------------------------------------
def thetas(sh, fam, form):
    rng = np.random.default_rng(sh.P + 7 * len(fam))
    R_, P = sh.R, sh.P
    if fam == "zero":
        return np.zeros((R_, P))
    if fam == "dyadic":  # multiples of 2^-8, |theta| <= 4: every partial sum of E is exact
        return np.clip(np.rint(rng.normal(scale=0.3, size=(R_, P)) * 256), -1024, 1024) / 256
    if fam == "dense":
        return rng.normal(scale=0.3, size=(R_, P))
    if fam == "big":  # sum |theta| = 40
        th = rng.normal(size=(R_, P))
        return th * (40.0 / np.abs(th).sum(axis=1, keepdims=True))
    if fam == "sparse":  # one or two entries: the field alone, the last parameter alone, parameter 0 and another, two others
        th = np.zeros((R_, P))
        mags = (0.5, 3.0, 20.0) if form == "RPLE" else (0.5, 3.0, 9.0)  # (RPLE: |E| up to 39.5, both softplus branches)
        for r, u in enumerate(sh.nodes):
            fld = int(u) if sh.order == 2 else next(j for j, k in enumerate(sh.pkeys[int(u)]) if len(k) == 1)
            a = mags[r % 3] * (-1.0) ** (r // 3)
            kind = r % 4
            if kind == 0:
                th[r, fld] = a
            elif kind == 1:
                th[r, P - 1 if fld != P - 1 else P - 2] = a
            else:
                j1, j2 = (int(v) for v in rng.choice(np.arange(1, P), size=2, replace=False))
                th[r, 0 if kind == 2 else j1] = a
                th[r, j2] = 0.95 * a
        return th
    raise KeyError(fam)


def padding_case(sh, value, far=7):
    """dense rows with every entry of row `far` at `value`: the padding samples of that row have E = P value"""
    th = np.random.default_rng(sh.P + 11).normal(scale=0.3, size=(sh.R, sh.P))
    th[far, :] = value
    return th, far


def direction(sh):
    """dense dyadic directions: multiples of 2^-6, |p| <= 2"""
    return np.random.default_rng(sh.P + 1).integers(-128, 129, size=(sh.R, sh.P)) / 64.0


# ---------------------------------------------------------------------------------------------------------------------------
# the exact (integer) cases
# ---------------------------------------------------------------------------------------------------------------------------
def exact_product(sh, pint):
    """theta = 0 and the directions pint [R][Qp] (internal layout): h = w exactly in every form, so V = w A and G = X^T diag(w) X p
    are sums of integers over 64 M.  float64 GEMMs of integers below 2^53 (exact_preconditions): exact in any order."""
    A = pint[:, :sh.Qf] @ sh.X + pint[:, [sh.cconst]]
    V = sh.w[None, :] * A
    G = np.zeros((sh.R, sh.Qp))
    G[:, :sh.Qf] = V @ sh.X.T
    G[:, sh.cconst] = V.sum(axis=1)
    return V, G


def exact_preconditions(sh, p_ref, th_dyadic):
    """In Python integers: every partial sum of the exact cases fits in 53 bits, whatever the order.  A in units of 2^-6: |A| <=
    sum |64 p|; V = c A in units of 2^-6 / M; any partial sum of a column of G is at most sum_k c_k |64 A_k|; the dyadic energies in
    units of 2^-8.  Returns the largest of them."""
    worst = 0
    for r, u in enumerate(sh.nodes):
        p64 = [int(v) for v in np.rint(p_ref[r] * 64)]
        assert all(abs(v) <= 128 for v in p64) and np.array_equal(np.array(p64) / 64.0, p_ref[r])
        sa = sum(abs(v) for v in p64)
        X = sh.ref_stats(int(u)).astype(np.int64)
        A64 = X @ np.array(p64, dtype=np.int64)
        g = sum(int(c) * abs(int(a)) for c, a in zip(sh.counts, A64))
        t256 = [int(v) for v in np.rint(th_dyadic[r] * 256)]
        assert all(abs(v) <= 1024 for v in t256) and np.array_equal(np.array(t256) / 256.0, th_dyadic[r])
        worst = max(worst, sa, g, max(int(c) for c in sh.counts) * sa, sum(abs(v) for v in t256))
    assert sh.M & (sh.M - 1) == 0 and int(sum(int(c) for c in sh.counts)) == sh.M
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# the public path: the reference's parameter order, from the spins alone
# ---------------------------------------------------------------------------------------------------------------------------
def public_reference(sh, form, th, rows, plan, exp_ulps=EXP_ULPS):
    """f, g [rows][P] of objgrad and their bounds: the element bounds above carried through the sums (no cut at V here), and for
    logRISE the log and the division (u each)"""
    nsplit, kchunk = plan
    f, bf = np.zeros(len(rows), dtype=LD), np.zeros(len(rows), dtype=LD)
    g, bg = np.zeros((len(rows), sh.P), dtype=LD), np.zeros((len(rows), sh.P), dtype=LD)
    w = sh.w[:sh.K]
    for i, r in enumerate(rows):
        u = int(sh.nodes[r])
        X = sh.ref_stats(u)
        t = th[r]
        m = LD(np.count_nonzero(t))
        BE = m * U * np.abs(t).astype(LD).sum() / (1 - m * U)
        E = pm1_dot(X, t[:, None])[:, 0]
        o = forward(form, E[None, :], np.ones((1, sh.K)), w, [BE], exp_ulps)  # (x already carries the node's spin: s = 1)
        fs, bfs = f_of(o, sh.Kp)
        V = o["V"][0]
        gs = pm1_dot(np.ascontiguousarray(X.T), V[:, None])[:, 0]
        sa = np.abs(V).sum()
        fld = u if sh.order == 2 else next(j for j, k in enumerate(sh.pkeys[u]) if len(k) == 1)
        bgs = np.full(sh.P, o["bV"][0].sum() + (kchunk + nsplit) * U * sa, dtype=LD)
        bgs[fld] = o["bV"][0].sum() + (kchunk / 4 + 2 + nsplit) * U * sa
        if form == "logRISE":
            f[i], bf[i] = np.log(fs[0]), -np.log1p(-bfs[0] / fs[0]) + U * np.abs(np.log(fs[0]))
            g[i] = gs / fs[0]
            bg[i] = (bgs + np.abs(g[i]) * bfs[0]) / (fs[0] - bfs[0]) + U * np.abs(g[i])
        else:
            f[i], bf[i], g[i], bg[i] = fs[0], bfs[0], gs, bgs
    return f, bf, g, bg


def public_hessvec_logrise(sh, th, pd, rows, plan, exp_ulps=EXP_ULPS, exact_E=False):
    """Hess log Z p = Hess Z p / Z - g (g . p), g = grad Z / Z, of the public hessvec at f64 for logRISE, in the reference's parameter
    order, with first-order bounds carried through both passes and the host finish:
      U_k = e_k A_k, A = x . p:  the device multiplies its own e (off by be) with its own A (off by B_A) and rounds once:
          bU = e |A| u + (e B_A + be |A| + be B_A) (1 + u);   (Hess Z p)_j = sum_k U_k x_kj: sum bU + the backward bound on sum |U|
      gv = sum_j g_j p_j:  sum bg_j |p_j| + (P + 1) u sum |g_j p_j|  (a product and an addition per term)
      t1 = (Hess Z p)_j / Z:  (bH + |t1| bZ) / (Z - bZ) + u |t1|;   t2 = g_j gv:  bg |gv| + |g_j| bgv + bg bgv + u |t2|;   the difference: u |t1 - t2|.
    exact_E: theta and p are dyadic and every partial sum of E and A is exact (B_E = B_A = 0)"""
    nsplit, kchunk = plan
    hv, bhv = np.zeros((len(rows), sh.P), dtype=LD), np.zeros((len(rows), sh.P), dtype=LD)
    w = sh.w[:sh.K]
    for i, r in enumerate(rows):
        u = int(sh.nodes[r])
        X = sh.ref_stats(u)
        XT = np.ascontiguousarray(X.T)
        t, p = th[r], pd[r]
        m, mp = LD(np.count_nonzero(t)), LD(np.count_nonzero(p))
        BE = m * U * np.abs(t).astype(LD).sum() / (1 - m * U)
        BA = mp * U * np.abs(p).astype(LD).sum() / (1 - mp * U)
        if exact_E:
            BE = BA = LD(0)
        o = forward("RISE", pm1_dot(X, t[:, None])[:, 0][None, :], np.ones((1, sh.K)), w, [BE], exp_ulps)
        Z, bZ = (v[0] for v in f_of(o, sh.Kp))
        e, be = o["e"][0], o["be"][0]
        fld = u if sh.order == 2 else next(j for j, k in enumerate(sh.pkeys[u]) if len(k) == 1)
        back = np.full(sh.P, (kchunk + nsplit) * U, dtype=LD)
        back[fld] = (kchunk / 4 + 2 + nsplit) * U
        gZ = pm1_dot(XT, (-e)[:, None])[:, 0]
        bgZ = be.sum() + back * e.sum()
        g = gZ / Z
        bg = (bgZ + np.abs(g) * bZ) / (Z - bZ) + U * np.abs(g)
        A = pm1_dot(X, p[:, None])[:, 0]
        Uk = e * A
        bU = e * np.abs(A) * U + (e * BA + be * np.abs(A) + be * BA) * (1 + U)
        H = pm1_dot(XT, Uk[:, None])[:, 0]
        bH = bU.sum() + back * np.abs(Uk).sum()
        gv = (g * p).sum()
        bgv = (bg * np.abs(p)).sum() + (sh.P + 1) * U * np.abs(g * p).sum()
        t1, t2 = H / Z, g * gv
        b1 = (bH + np.abs(t1) * bZ) / (Z - bZ) + U * np.abs(t1)
        b2 = bg * np.abs(gv) + np.abs(g) * bgv + bg * bgv + U * np.abs(t2)
        hv[i], bhv[i] = t1 - t2, b1 + b2 + U * np.abs(t1 - t2)
    return hv, bhv


def brute(sh_n, spins, counts, M, u, th_ref, keys, form):
    """triple loop in np.longdouble scalars: f and g of one node in the reference's parameter order (keys: the spins of each statistic)"""
    K = len(spins)
    f, g = LD(0), [LD(0)] * len(keys)
    for k in range(K):
        x = []
        for key in keys:
            v = 1
            for i in key:
                v *= int(spins[k][i])
            x.append(v)
        E = LD(0)
        for j, xv in enumerate(x):
            E += LD(th_ref[j]) * xv
        w = LD(counts[k]) / LD(M)
        if form == "RPLE":
            f += w * np.log1p(np.exp(-2 * E))
            v = -2 * w / (1 + np.exp(2 * E))
        else:
            f += w * np.exp(-E)
            v = -w * np.exp(-E)
        for j, xv in enumerate(x):
            g[j] = g[j] + v * xv
    return f, np.array(g, dtype=LD)


def pair_keys(n, u):
    return [(u,) if j == u else tuple(sorted((u, j))) for j in range(n)]
