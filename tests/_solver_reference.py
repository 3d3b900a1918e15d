"""Host model of the solver's device kernels (csrc/gml_solver.hip) and of the direction phase around the batched solve
(csrc/gml_newton_solve.hip), written from the comments above the kernels and from the textbook definitions.  Numpy only; nothing of the
code under test is imported.  One row at a time: the tests loop over rows.

Arithmetic: float64 where the kernel's result is one rounding (g +- lambda, x - xprev, lambda |x|); math.fsum / np.longdouble wherever
the kernel sums, so that a sum of this model is the exact sum of the kernel's terms (fsum) or carries a thousand times less rounding
(longdouble).  Every function that sums also returns the sum of the absolute terms where a test needs it for its tolerance."""
import math

import numpy as np

LD = np.longdouble


# ---- k_select -----------------------------------------------------------------------------------------------------------------------
def pseudo_grad(x, g, lam):
    """Minimum-norm element of the subdifferential of f + lam |x| in one coordinate: g + lam sign(x) off zero; at zero the element of
    [g - lam, g + lam] closest to 0.  Arrays or scalars; lam may be an array (0 on the unpenalised columns)."""
    x, g, lam = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64), np.asarray(lam, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        at0 = np.where(g + lam < 0, g + lam, np.where(g - lam > 0, g - lam, 0.0))
        pg = np.where(x > 0, g + lam, np.where(x < 0, g - lam, at0))
    return np.where(lam == 0, g, pg)


def f32_pattern(a):
    """bit pattern of float32(|a|): monotone in |a| as an unsigned integer"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32).view(np.uint32)


def admission_threshold(patterns, max_add):
    """Threshold on the float32 patterns of the violators' |pg| that admits at most max_add of them -- unless the class of equal
    patterns at the cut is all there is to admit: one above the pattern of the (max_add + 1)-th largest violator if any violator
    reaches that, else that violator's own pattern (the whole tie class gets in).  Called only with more than max_add violators."""
    v = np.sort(np.asarray(patterns, dtype=np.uint64))[::-1]
    assert len(v) > max_add >= 0
    p = int(v[max_add])
    return p + 1 if (v >= p + 1).any() else p


def effective_max_add(max_add, nsupp, nviol, capW):
    """twice as many for a row with violators by the thousand; then as many as fill the working set up to whole 32-entry tiles, as long
    as at least half of max_add still get in"""
    if nviol > 16 * capW:
        max_add *= 2
    full = (nsupp + max_add) // 32 * 32
    if full - nsupp >= max_add // 2:
        max_add = full - nsupp
    return max_add


def select_row(x, g, kind, lam, max_add, capW, capP, viol_frac, best):
    """k_select on one row.  Returns a dict: pg (after the matrix-free cut), l1, l1_abs, worst, worstW, nsupp, nviol, m, thr, addv,
    F / gF / pgF (length capP with the padding; None for a matrix-free row), better (the best-iterate rule), best."""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    Qp = len(x)
    par = kind != 0
    l = np.where(kind == 2, lam, 0.0)
    pg = np.where(par, pseudo_grad(x, g, l), 0.0)
    terms = (l * np.abs(x))[par]
    l1 = math.fsum(terms)
    a = np.abs(pg)
    supp = par & ((x != 0) | (kind == 1))
    viol = par & ~supp & (pg != 0)
    nan = np.isnan(a[par]).any()
    worst = math.inf if nan else float(np.max(a[par], initial=0.0))  # a NaN gradient is an infinite residual
    worstW = float(np.fmax.reduce(a[supp], initial=0.0))             # (over the support: a NaN there is passed over)
    nsupp, nviol = int(supp.sum()), int(viol.sum())
    addv = not (worstW > worst * 0.999999 and worstW > 0 and nsupp > 1)
    max_add = effective_max_add(max_add, nsupp, nviol, capW)
    pat = f32_pattern(pg)
    thr = 0
    if addv and nviol > max_add and nsupp <= capW:
        thr = admission_threshold(pat[viol], max_add)
    if nsupp <= capW:
        inW = supp | (viol & (pat >= thr) & addv)
        m = int(inW.sum())
    else:
        inW, m = supp, nsupp
    out = dict(l1=l1, l1_abs=math.fsum(np.abs(terms)), worst=worst, worstW=worstW, nsupp=nsupp, nviol=nviol, thr=thr, addv=addv,
               max_add=max_add, F=None, gF=None, pgF=None)
    if m > capW:  # matrix-free: W = every column with x != 0 or pg != 0 after the cut
        pg = pg.copy()
        if viol_frac > 0 and nviol * 16 > nsupp:
            z = (kind == 2) & (x == 0)
            cut = viol_frac * float(np.fmax.reduce(np.abs(pg[z]), initial=0.0))
            pg[z & (np.abs(pg) < cut)] = 0.0
        m = -int((par & ((x != 0) | (pg != 0))).sum())
    else:
        cols = np.flatnonzero(inW)
        F = np.full(capP, Qp - 1, dtype=np.int32)
        gF = np.zeros(capP)
        pgF = np.zeros(capP)
        F[:m], gF[:m], pgF[:m] = cols, g[cols], pg[cols]
        out.update(F=F, gF=gF, pgF=pgF)
    better = worst < best
    out.update(pg=pg, m=m, better=better, best=worst if better else best)
    return out


# ---- k_trial / k_back ---------------------------------------------------------------------------------------------------------------
def trial_row(x, d, pg, kind, lam, al):
    """Projected trial point xt = P(x + al d) of one row and its scalars; when the projected step is no descent direction (dd >= 0)
    only the clipping is taken.  Returns a dict: xt, dd, stepn, l1t and the sums of absolute terms dd_abs, and the margins of the branch
    decisions: clip_margin = min over the clip tests of |v| / (|x| + |al d|) (inf where v is exactly 0 or nothing is tested),
    fallback (bool), dd_first (the dd that chose the branch) and dd_first_abs."""
    x, d, pg = (np.asarray(v, dtype=np.float64) for v in (x, d, pg))
    mv = (kind != 0) & (d != 0)
    step = al * d
    v = np.where(mv, x + step, x)
    pen = mv & (kind == 2) & (lam > 0)
    xi = np.where(x != 0, np.sign(x), np.where(pg < 0, 1.0, -1.0))
    size = np.abs(x) + np.abs(step)
    rel = np.abs(v[pen]) / size[pen]
    clip_margin = float(np.min(rel[rel > 0], initial=math.inf))
    clipped = pen & (v * xi < 0)
    xt = np.where(clipped, 0.0, v)
    t = (pg * (xt - x))[mv]
    dd_first, dd_first_abs = math.fsum(t), math.fsum(np.abs(t))
    fallback = not dd_first < 0
    if fallback:
        cross = (kind == 2) & (lam > 0) & (x != 0) & (d != 0) & ((x + step) * x < 0)
        xt = np.where(cross, 0.0, x)
        t = (pg * (0.0 - x))[cross]
        mv = cross
    sn = np.abs(xt - x)[mv]
    l1 = (lam * np.abs(xt))[kind == 2]
    return dict(xt=xt, clipped=(clipped if not fallback else cross), dd=math.fsum(t), dd_abs=math.fsum(np.abs(t)), stepn=math.fsum(sn),
                l1t=math.fsum(l1), clip_margin=clip_margin, fallback=fallback, dd_first=dd_first, dd_first_abs=dd_first_abs, nterms=int(mv.sum()))


def back_row(x, xt, gt, kind, lam):
    """F'(xt; x - xt): the directional derivative of F = f + lam |.|_1 at xt towards x.  Returns (back, sum of |terms|, terms)."""
    x, xt, gt = (np.asarray(v, dtype=np.float64) for v in (x, xt, gt))
    sc = x - xt
    on = (sc != 0) & (kind != 0)
    gl = gt * sc
    pen = lam * np.where(xt != 0, np.sign(xt) * sc, np.abs(sc))
    terms = np.concatenate([gl[on], pen[on & (kind == 2)]])
    return math.fsum(terms), math.fsum(np.abs(terms)), int(on.sum())


# ---- k_secant: the state machine and the BFGS correction ---------------------------------------------------------------------------
class SecantState:
    """State of one row between iterations: previous working set, x and g on it, the last (at most two) pairs, oldest first."""

    def __init__(self, cap, fill=0.0, ifill=0):
        self.Fprev = np.full(cap, ifill, dtype=np.int32)
        self.mprev = 0
        self.xprev = np.full(cap, fill)
        self.gprev = np.full(cap, fill)
        self.S = np.full((2, cap), fill)
        self.Y = np.full((2, cap), fill)
        self.npairs = 0

    def step(self, F, xF, gF, ynoise):
        """One call of k_secant with working set F (its length is m), x and g on it.  Returns the scalars of the acceptance test
        (None when m == 0, or when the working set changed)."""
        m = len(F)
        if m == 0:
            return None
        same = m == self.mprev and (self.Fprev[:m] == F).all()
        n = self.npairs if same else 0
        s = np.asarray(xF, dtype=np.float64) - self.xprev[:m]
        y = np.asarray(gF, dtype=np.float64) - self.gprev[:m]
        sl, yl = s.astype(LD), y.astype(LD)
        ss, yy, ys, ymax = float(sl @ sl), float(yl @ yl), float(sl @ yl), float(np.abs(y).max())
        self.xprev[:m], self.gprev[:m], self.Fprev[:m] = xF, gF, F
        info = None
        if same:
            ratio = ys / math.sqrt(ss * yy) if ss > 0 and yy > 0 else 0.0
            info = dict(ss=ss, yy=yy, ys=ys, ymax=ymax, ratio=ratio)
            if ss > 0 and ys > 1e-4 * math.sqrt(ss * yy) and ymax > ynoise:
                if n == 2:
                    self.S[0, :m], self.Y[0, :m] = self.S[1, :m], self.Y[1, :m]
                    n = 1
                self.S[n, :m], self.Y[n, :m] = s, y
                n += 1
        self.npairs, self.mprev = n, m
        return info

    def pairs(self, m):
        return [(self.S[l, :m].copy(), self.Y[l, :m].copy()) for l in range(self.npairs)]


U = 2.0 ** -53  # unit roundoff of float64


def gamma(n):
    """the constant of the standard error bound of an n-term float64 inner product (Higham, Accuracy and Stability, Lemma 3.1)"""
    return n * U / (1 - n * U)


def bfgs(B, pairs, Babs=None, dtype=LD):
    """B <- B - (B s)(B s)^T / (s^T B s) + y y^T / (y^T s) for the pairs in order (oldest first); a pair with s^T B s <= 0 or
    y^T s <= 0 is skipped.  Returns (B', dB): B' in `dtype`; dB = an entry-wise bound on |float64 evaluation - B'| for an evaluation
    that forms every inner product in float64 in any order (derivation: tests/test_gpu_newton_solve.py, test_secant_*).  Babs bounds
    the absolute values of what B itself was added up from (default |B|)."""
    B = np.array(B, dtype=dtype)
    m = len(B)
    Babs = np.abs(B) if Babs is None else np.array(Babs, dtype=dtype)
    dB = np.zeros_like(B)
    for s, y in pairs:
        s, y = s.astype(dtype), y.astype(dtype)
        sa, ya = np.abs(s), np.abs(y)
        v = B @ s
        sBs, ys = s @ v, s @ y
        if not (sBs > 0 and ys > 0):
            continue
        va = Babs @ sa                           # sum of the absolute terms of v
        dv = dB @ sa + gamma(m + 3) * va         # the error of v: the input's, and the inner product's
        dsBs = sa @ dv + gamma(m + 1) * (sa @ va)
        dys = gamma(m + 1) * (sa @ ya)
        lo_sBs, lo_ys = sBs - dsBs, ys - dys
        assert lo_sBs > 0 and lo_ys > 0
        vv, yyt = np.outer(np.abs(v), np.abs(v)), np.outer(ya, ya)
        e2 = (np.outer(dv, np.abs(v)) + np.outer(np.abs(v), dv) + np.outer(dv, dv)) / lo_sBs + vv * dsBs / (sBs * lo_sBs) + 4 * U * vv / lo_sBs
        e1 = yyt * dys / (ys * lo_ys) + 4 * U * yyt / lo_ys
        B = B + np.outer(y, y) / ys - np.outer(v, v) / sBs
        Babs = Babs + yyt / ys + np.outer(va, va) / sBs
        dB = dB + e1 + e2 + 3 * U * Babs
    return B, dB


def corrected_block(H, g, s1, s2, pairs, dtype=LD):
    """What k_secant leaves in the block: H' with s1 H' - s2 g g^T = bfgs(s1 H - s2 g g^T).  Returns (H', B', dH): dH bounds the
    entry-wise distance of a float64 evaluation from H'."""
    H = np.array(H, dtype=dtype)
    gg = s2 * np.outer(g.astype(dtype), g.astype(dtype))
    B, dB = bfgs(s1 * H - gg, pairs, s1 * np.abs(H) + np.abs(gg), dtype)
    return (B + gg) / s1, B, dB / s1 + 2 * U * np.abs(H)


# ---- the solve with fixed entries and the orthant faces ------------------------------------------------------------------------------
def solve_fixed(B, pg, fx, dfx):
    """d = dfx on the fixed entries; B_ff d_f = -pg_f - B_fx dfx_x on the free ones"""
    B = np.asarray(B, dtype=np.float64)
    d = np.where(fx, dfx, 0.0)
    fr = ~fx
    if fr.any():
        d[fr] = np.linalg.solve(B[np.ix_(fr, fr)], -pg[fr] - B[np.ix_(fr, fx)] @ dfx[fx])
    return d


def face_candidates(x, d, pg, kind, free):
    """Entries of `free` whose step leaves the orthant face of the iterate (a zero one moving with its pseudo-gradient, a non-zero one
    past zero), where the projection puts them, their share mass of total = sum |pg d|, and the margins of the two sign tests."""
    pen = free & (kind == 2)
    t0, t1 = d * pg, (x + d) * x
    cand = pen & np.where(x == 0, t0 > 0, t1 < 0)
    fixed = np.where(x == 0, 0.0, -x)
    mass = math.fsum(np.abs(pg * (d - fixed))[cand])
    total = math.fsum(np.abs(pg * d)[free])
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(x == 0, np.abs(t0) / (np.abs(d) * np.abs(pg)), np.abs(t1) / ((np.abs(x) + np.abs(d)) * np.abs(x)))
        dmar = np.where(x == 0, np.abs(d) / np.abs(d).max(), np.abs(x + d) / (np.abs(x) + np.abs(d)))
    margin = float(np.min(np.minimum(rel, dmar)[pen], initial=math.inf))
    return cand, fixed, mass, total, margin


def solve_faces(B, pg, x, kind, share, rounds, fix=None, dfix=None):
    """The direction of one Cholesky row: the solve, then at most `rounds` re-solves with the candidates fixed, each only when they
    carry more than `share` of the predicted decrease.  B is the (corrected) matrix on both sides of every re-solve.
    Returns (d, log); log has one entry per face test: dict(n, mass, total, margin, again)."""
    m = len(pg)
    fx = np.zeros(m, dtype=bool) if fix is None else np.asarray(fix, dtype=bool).copy()
    dfx = np.zeros(m) if dfix is None else np.where(fx, dfix, 0.0)
    log = []
    face = 0
    while True:
        d = solve_fixed(B, pg, fx, dfx)
        if face >= rounds:
            break
        cand, fixed, mass, total, margin = face_candidates(x, d, pg, kind, ~fx)
        again = bool(cand.any()) and mass > share * total
        signs = np.where(x == 0, d * pg, (x + d) * x)[~fx & (kind == 2)]  # (the values whose signs pick the candidates)
        log.append(dict(n=int(cand.sum()), mass=mass, total=total, margin=margin, again=again, signs=signs))
        if not again:
            break
        fx |= cand
        dfx = np.where(cand, fixed, dfx)
        face += 1
    return d, log


# ---- the matrix-free Newton-CG of one row -------------------------------------------------------------------------------------------
class Pcg:
    """Preconditioned CG on W = {c: parameter, x_c != 0 or pg_c != 0} of B = s1 Hd - s2 g g^T, B d = -pg, preconditioned by the
    inverses of the diagonal blocks of T consecutive entries of W in column order.  The blocks of the original W stay when faces
    shrink W (the mask Wm): z is masked instead.  All arithmetic in `dtype`.

    The products can come from outside (the cut the tests make at the device's own recorded products): step(hp) / update(hp) and
    faces(hd) take Hd @ p and Hd @ d as given, and Minv -- one inverted block per tile, [T][T] or larger with the tile in the leading
    corner -- replaces the inverses of Hd's blocks; Hd may then be None.  With the products it would form itself, the bits are the same."""

    def __init__(self, Hd, s1, s2, x, pg, g, kind, T, dtype=np.float64, Minv=None):
        self.dt = dtype
        self.Hd, self.s1, self.s2 = None if Hd is None else np.asarray(Hd, dtype=dtype), dtype(s1), dtype(s2)
        self.x, self.pg, self.g, self.kind = x, np.asarray(pg, dtype=dtype), np.asarray(g, dtype=dtype), kind
        Qp = len(x)
        inW = (kind != 0) & ((x != 0) | (pg != 0))
        self.W = np.flatnonzero(inW)
        self.tiles = [self.W[a:a + T] for a in range(0, len(self.W), T)]
        self.Minv = [] if Minv is None else [np.asarray(Mi, dtype=dtype)[:len(t), :len(t)] for t, Mi in zip(self.tiles, Minv)]
        for t in (self.tiles if Minv is None else []):
            A = self.s1 * self.Hd[np.ix_(t, t)] - self.s2 * np.outer(self.g[t], self.g[t])
            self.Minv.append(np.asarray(np.linalg.inv(A.astype(np.float64)), dtype=dtype) if dtype is np.float64 else _inv_ld(A))
        self.Wm = inW.copy()
        self.r = np.where(inW, -self.pg, dtype(0))
        self.d, self.z, self.p = (np.zeros(Qp, dtype=dtype) for _ in range(3))
        self.rs = self.rs0 = self.r @ self.r
        self.pHp = self.rz = dtype(0)
        self.apply()
        self.direction(True)

    def B(self):
        return self.s1 * self.Hd - self.s2 * np.outer(self.g, self.g)

    def apply(self):
        for t, Mi in zip(self.tiles, self.Minv):
            self.z[t] = Mi @ self.r[t]

    def direction(self, first):
        rzo = self.rz
        w = self.W[self.Wm[self.W]]
        self.rz = self.r[w] @ self.z[w]
        be = self.rz / rzo if (not first and rzo > 0) else self.dt(0)
        self.p[self.W] = np.where(self.Wm[self.W], self.z[self.W] + (0 if first else be * self.p[self.W]), 0)

    def step(self, hp=None):
        self.update(hp)
        self.advance()

    def update(self, hp=None, pHp=None):
        """k_pcg_step: d, r and the scalars pHp, rs (rz is still the one the step length was taken from).  pHp: the step length is taken
        from this value instead of the model's own sum, which stays in pHp_own (a cut after the kernel's first reduction)"""
        hp = self.Hd @ self.p if hp is None else np.asarray(hp, dtype=self.dt)
        gp = self.g[self.W] @ self.p[self.W] if self.s2 != 0 else self.dt(0)
        h = np.where(self.Wm, self.s1 * hp - self.s2 * self.g * gp, 0)
        self.pHp_own = self.p[self.W] @ h[self.W]
        self.pHp = self.pHp_own if pHp is None else self.dt(pHp)
        al = self.rz / self.pHp if self.pHp > 0 else self.dt(0)
        self.d[self.W] += al * self.p[self.W]
        self.r[self.W] -= al * h[self.W]
        self.rs = self.r[self.W] @ self.r[self.W]

    def advance(self):
        """the preconditioner and the next direction (a row that stays live)"""
        self.apply()
        self.direction(False)

    def faces(self, hd=None):
        """k_pcg_faces, then the residual of the shrunk system (k_pcg_resid) and the first direction.  Returns dict(n, mass, total, margin)."""
        d64 = self.d.astype(np.float64)
        pg64 = self.pg.astype(np.float64)
        cand, fixed, mass, total, margin = face_candidates(self.x, d64, pg64, self.kind, self.Wm.copy())
        self.d = np.where(cand, fixed.astype(self.dt), self.d)
        self.Wm &= ~cand
        hd = self.Hd @ self.d if hd is None else (hd(self.d) if callable(hd) else np.asarray(hd, dtype=self.dt))
        gd = self.g @ self.d if self.s2 != 0 else self.dt(0)
        self.r = np.where(self.Wm, -self.pg - (self.s1 * hd - self.s2 * self.g * gd), 0)
        self.rs = self.r @ self.r
        self.pHp = self.rz = self.dt(0)
        self.apply()
        self.direction(True)
        return dict(n=int(cand.sum()), mass=mass, total=total, margin=margin, cand=cand)


def _inv_ld(A):
    """inverse of a symmetric positive definite matrix in longdouble: the float64 inverse and two Newton-Schulz refinements"""
    X = np.linalg.inv(A.astype(np.float64)).astype(LD)
    I = np.eye(len(A), dtype=LD)
    for _ in range(2):
        X = X + X @ (I - A @ X)
    return X
