"""The solver's device kernels (csrc/gml_solver.hip), one by one, against the host model of tests/_solver_reference.py: k_select (the
pseudo-gradient, the KKT residual the solver stops on, the working set), k_trial / k_back (the projected line search), and the vector
kernels of the matrix-free Newton-CG.  The hooks (csrc/gml_testhooks.cpp) run the launchers as gml_solver.cpp calls them on arrays given
here; every output array goes in filled with a sentinel, so what a kernel must not touch is checked too."""
import ctypes as C
import math

import numpy as np
import pytest

import _solver_reference as M
from gml_amd import _lib

pytestmark = pytest.mark.gpu

SEL = np.dtype([("l1", "f8"), ("worst", "f8"), ("worstW", "f8"), ("m", "i4"), ("nsupp", "i4"), ("nviol", "i4"), ("pad", "i4")])
TRI = np.dtype([("dd", "f8"), ("stepn", "f8"), ("l1t", "f8"), ("back", "f8")])
CGS = np.dtype([("rs", "f8"), ("rs0", "f8"), ("pHp", "f8"), ("rz", "f8")])
FAC = np.dtype([("nfixed", "i4"), ("pad", "i4"), ("mass", "f8"), ("total", "f8")])
SENT = -777.25  # sentinel of the float outputs
QPS = [64, 255, 256, 257, 2048, 2049, 4352]
ROWS = np.array([4, 0, 5, 2, 1], dtype=np.int32)  # of R = 6: permuted, row 3 left out
P = _lib._ptr


def call(name, *args):
    """a hook by name: arrays as pointers (None: NULL), Python floats as double, np.int64 as int64_t, other integers as int"""
    fn = getattr(_lib.lib(), name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p if (a is None or isinstance(a, C.c_void_p)) else C.c_double if isinstance(a, float) else C.c_int64 if isinstance(a, np.int64)
                   else C.c_int for a in args]
    _lib.check(fn(*[int(a) if isinstance(a, (np.integer, int)) else a for a in args]))


# ---- k_select -----------------------------------------------------------------------------------------------------------------------
def make_row(rng, Qp, lam, nfree, nsupport, viol, holes=True, resid=1e-3, big=None, nan=False):
    """One row: kinds 0 / 1 / 2 mixed (nfree free columns, a tenth of the others excluded), x != 0 on nsupport penalised columns with a
    pseudo-gradient of size resid there, the given pseudo-gradients `viol` on as many zero columns as fit, no violation elsewhere."""
    kind = np.full(Qp, 2, dtype=np.uint8)
    if holes:
        kind[rng.random(Qp) < 0.1] = 0
    kind[rng.choice(Qp, nfree, replace=False)] = 1
    x = np.zeros(Qp)
    g = np.where(lam > 0, rng.uniform(-0.9, 0.9, Qp) * lam, 0.0)  # |g| < lam at zero: no violation
    pen = rng.permutation(np.flatnonzero(kind == 2))
    ns = min(nsupport, len(pen) - 4)
    nv = min(len(viol), len(pen) - ns)
    sup, vio = pen[:ns], pen[ns:ns + nv]
    x[sup] = rng.choice([-1.0, 1.0], ns) * rng.uniform(0.05, 1.0, ns)
    g[sup] = -lam * np.sign(x[sup]) + rng.uniform(-1, 1, ns) * resid
    g[kind == 1] = rng.uniform(-1, 1, nfree) * resid
    v = np.asarray(viol[:nv], dtype=np.float64)
    g[vio] = v + lam * np.sign(v)
    if big is not None:
        g[sup[0]] = big
    if nan:
        g[sup[1]] = np.nan
    x[kind == 0] = rng.normal(size=int((kind == 0).sum()))  # excluded columns: ignored whatever they hold
    g[kind == 0] = rng.normal(size=int((kind == 0).sum())) * 10
    return x, g, kind


def distinct(rng, n, lo=0.05, hi=1.0):
    """n pseudo-gradients of distinct sizes (distinct as float32 too), random signs"""
    return rng.permutation(lo + (hi - lo) * (np.arange(n) + 0.5) / max(n, 1)) * rng.choice([-1.0, 1.0], n)


def select_rows(rng, scen, Qp, lam, max_add, capW):
    eff = lambda nsupp: M.effective_max_add(max_add, nsupp, 0, capW)
    if scen == "A":
        nf2, ns2 = (3, 5) if capW > 8 else (1, 1)  # (a support that leaves room for violators below capW)
        ties = np.concatenate([distinct(rng, max(eff(nf2 + ns2) - 2, 0), 0.5, 1.0), [0.3, -0.3, 0.3, 0.3], distinct(rng, 3, 0.05, 0.2)])
        cls = np.where(np.arange(eff(3) + 3) % 2 == 0, 1.0, 1.0 + 1e-12) * rng.choice([-1.0, 1.0], eff(3) + 3)
        big_supp = capW + 4 if capW + 40 < Qp else 12
        return {0: make_row(rng, Qp, lam, 1, 0, distinct(rng, eff(1)), holes=Qp > 64),        # X = 0; nviol = max_add: no search
                1: make_row(rng, Qp, lam, 1, 0, distinct(rng, eff(1) + 1), holes=Qp > 64),    # one more: the smallest stays out
                2: make_row(rng, Qp, lam, nf2, ns2, ties),                                         # equal |pg| straddling the cut
                4: make_row(rng, Qp, lam, 1, 2, np.concatenate([cls, distinct(rng, 5, 0.05, 0.2)])),  # the largest class is the cut
                5: make_row(rng, Qp, lam, 2, big_supp, distinct(rng, 3))}                      # a support above capW
    many = 16 * capW + 1
    return {0: make_row(rng, Qp, lam, 2, 4, distinct(rng, 10), big=5.0),                       # the support's residual dominates
            1: make_row(rng, Qp, lam, 1, 3, distinct(rng, 3), nan=True),                       # a NaN gradient on the support
            2: make_row(rng, Qp, lam, 1, 2, distinct(rng, many if many < Qp // 2 else Qp // 2)),  # violators by the hundred
            4: make_row(rng, Qp, lam, 1, 40, distinct(rng, 2)),                                # few violators next to a large support
            5: make_row(rng, Qp, lam, 3, Qp, distinct(rng, 2))}                                # a dense iterate


@pytest.mark.parametrize("scen,lam,viol_frac", [("A", 0.25, 0.0), ("A", 0.0, 0.5), ("B", 0.25, 0.5), ("B", 0.25, 0.0)])
@pytest.mark.parametrize("capW", [8, 512])
@pytest.mark.parametrize("max_add", [5, 64])
@pytest.mark.parametrize("Qp", QPS)
def test_select_matches_the_host_model(Qp, max_add, capW, scen, lam, viol_frac):
    """k_select: PG, the scalars, the working set with its padding and the best iterate are exact; l1 is within Qp 2^-53 of the exact
    sum of its terms.  Rows of the scenarios above in a permuted row list; the row left out keeps its sentinels."""
    rng = np.random.default_rng(Qp * 131 + max_add * 7 + capW + (scen == "B") + int(4 * lam))
    R, capP = 6, capW
    rows = select_rows(rng, scen, Qp, lam, max_add, capW)
    X, G, kind = rng.normal(size=(R, Qp)), rng.normal(size=(R, Qp)), np.full((R, Qp), 2, dtype=np.uint8)
    for r, (x, g, k) in rows.items():
        X[r], G[r], kind[r] = x, g, k
    best0 = np.array([math.inf, 1e-9, math.inf, 0.5, 1e-9, math.inf])  # above and below the rows' residuals
    want = {r: M.select_row(X[r], G[r], kind[r], lam, max_add, capW, capP, viol_frac, best0[r]) for r in ROWS}
    # what the scenarios are there for
    if scen == "A":
        assert want[0]["nsupp"] == 1 and want[0]["thr"] == 0 and (want[1]["thr"] > 0 or Qp == 64)
        assert want[5]["nsupp"] <= capW or want[5]["m"] == -int((kind[5] != 0).sum() - (((X[5] == 0) & (want[5]["pg"] == 0))[kind[5] != 0]).sum())
        if want[2]["m"] >= 0 and (Qp > 64 or max_add == 5):  # the tie class at the cut stays out as a whole, the largest class gets in as a whole
            assert want[2]["thr"] > 0 and want[2]["m"] == want[2]["nsupp"] + want[2]["max_add"] - 2
        assert abs(want[4]["m"]) >= want[4]["nsupp"] + want[4]["max_add"] + 3 or Qp == 64
    else:
        assert not want[0]["addv"] and want[1]["worst"] == math.inf and not want[1]["better"] and want[4]["nviol"] * 16 <= want[4]["nsupp"]
    PG, Xbest = np.full((R, Qp), SENT), np.full((R, Qp), SENT)
    F, gF, pgF = np.full((R, capP), -5, dtype=np.int32), np.full((R, capP), SENT), np.full((R, capP), SENT)
    out = np.zeros(R, dtype=SEL)
    out["l1"], out["m"] = SENT, -5
    best = best0.copy()
    call("gml_test_solver_select", R, np.int64(Qp), len(ROWS), P(ROWS), P(X), P(G), P(kind), float(lam), max_add, capW, capP, float(viol_frac), P(PG),
         P(F), P(gF), P(pgF), P(out), P(best), P(Xbest), 0)
    assert (PG[3] == SENT).all() and (Xbest[3] == SENT).all() and (F[3] == -5).all() and (gF[3] == SENT).all() and (pgF[3] == SENT).all()
    assert out[3]["l1"] == SENT and out[3]["m"] == -5 and best[3] == best0[3]
    for r in ROWS:
        w, o = want[r], out[r]
        print(f"row {r}: m {o['m']} (model {w['m']}) nsupp {o['nsupp']} nviol {o['nviol']} worst {o['worst']:.6g} ({w['worst']:.6g}) thr {w['thr']:#x}"
              f" l1 - model {o['l1'] - w['l1']:.3g}")
        assert np.array_equal(PG[r], w["pg"], equal_nan=True), (r, np.flatnonzero(~((PG[r] == w["pg"]) | np.isnan(w["pg"]))))
        assert (o["worst"], o["worstW"], o["nsupp"], o["nviol"], o["m"], o["pad"]) == (w["worst"], w["worstW"], w["nsupp"], w["nviol"], w["m"], 0), r
        assert abs(o["l1"] - w["l1"]) <= Qp * 2.0 ** -53 * w["l1"], r
        if w["m"] >= 0:
            assert (F[r] == w["F"]).all() and np.array_equal(gF[r], w["gF"], equal_nan=True) and np.array_equal(pgF[r], w["pgF"], equal_nan=True), r
        else:  # matrix-free: nothing is gathered
            assert (F[r] == -5).all() and (gF[r] == SENT).all() and (pgF[r] == SENT).all(), r
        assert best[r] == w["best"] and (Xbest[r] == (X[r] if w["better"] else SENT)).all(), r
    assert {bool(want[r]["better"]) for r in ROWS} == {True, False}
    if capW == 8 and Qp >= 255:
        assert any(want[r]["m"] < 0 for r in ROWS)


# ---- k_trial / k_back ---------------------------------------------------------------------------------------------------------------
def grid(a):
    return np.round(np.asarray(a) * 1024) / 1024  # multiples of 2^-10: x + alpha d is exact for the alphas below, fused or not


def trial_rows(rng, Qp, lam):
    R = 6
    kind = np.full((R, Qp), 2, dtype=np.uint8)
    kind[rng.random((R, Qp)) < 0.1] = 0
    for r in range(R):
        kind[r, rng.choice(Qp, 3, replace=False)] = 1
    X = np.where(rng.random((R, Qp)) < 0.4, grid(rng.normal(size=(R, Qp))), 0.0)
    PG = np.where(rng.random((R, Qp)) < 0.8, grid(rng.normal(size=(R, Qp))), 0.0)
    # a descent direction with noise: zero coordinates move with and against -pg, non-zero ones cross zero or not
    D = np.where(rng.random((R, Qp)) < 0.7, grid(-PG * rng.uniform(0.5, 3.0, (R, Qp)) + rng.normal(size=(R, Qp)) * 0.4), 0.0)
    cross = rng.random((R, Qp)) < 0.1
    D = np.where(cross & (X != 0), -3.0 * X, D)
    D[kind == 0] = 1.5  # ignored
    pen = np.flatnonzero(kind[0] == 2)
    X[0, pen[0]], D[0, pen[0]], PG[0, pen[0]] = 0.5, -0.5, 0.25  # lands exactly on zero at alpha = 1
    # row 4: the clipped coordinates climb (pg against x) and the rest hardly moves: the projected step is no descent direction
    X[4], D[4], PG[4] = 0.0, 0.0, grid(rng.normal(size=Qp))
    c = np.flatnonzero(kind[4] == 2)[:6]
    X[4, c], D[4, c], PG[4, c] = 1.0, -3.0, -2.0
    c2 = np.flatnonzero(kind[4] == 2)[6:12]
    D[4, c2], PG[4, c2] = 2.0 ** -10, -1.0
    D[5] = 0.0  # no direction at all
    alpha = np.array([1.0, 0.5, 1 / 64, 1.0, 1.0, 0.5])
    return X, D, PG, kind, alpha


@pytest.mark.parametrize("with_stepn", [False, True])
@pytest.mark.parametrize("lam", [0.0, 0.3])
@pytest.mark.parametrize("Qp", QPS)
def test_trial_and_back_match_the_host_model(Qp, lam, with_stepn):
    """k_trial, then k_back with a given gradient at the trial points.  Xt within 2^-52 (|x| + |alpha d|) (the compiler may fuse
    x + alpha d) and exactly 0 where clipped; dd, stepn, l1t, back within n 2^-53 sum |terms| of the exact sums.  The model's branch
    decisions have margin (asserted), so rounding cannot choose a branch; k_back leaves dd, stepn and l1t as they were."""
    rng = np.random.default_rng(Qp + int(10 * lam))
    R = 6
    X, D, PG, kind, alpha = trial_rows(rng, Qp, lam)
    Gt = rng.normal(size=(R, Qp))
    want = {r: M.trial_row(X[r], D[r], PG[r], kind[r], lam, alpha[r]) for r in ROWS}
    for r in ROWS:
        w = want[r]
        assert w["clip_margin"] >= 1e-9
        assert w["dd_first"] == 0.0 or abs(w["dd_first"]) >= 1e-6 * w["dd_first_abs"], (r, w["dd_first"], w["dd_first_abs"])
    assert want[4]["fallback"] and want[5]["fallback"] and want[5]["dd"] == 0 and not want[0]["fallback"] and not want[2]["fallback"]
    if lam > 0:
        assert want[4]["dd"] > 0 and want[4]["clipped"].sum() == 6 and want[0]["clipped"].sum() > 0
        z = (X[0] == 0) & (kind[0] == 2) & (D[0] != 0)
        assert (want[0]["xt"][z] != 0).any() and (want[0]["clipped"][z]).any()  # zero coordinates: some move, some are held
    Xt = np.full((R, Qp), SENT)
    out = np.full(R, SENT, dtype=TRI)
    stepn = np.full(R, SENT) if with_stepn else None
    args = lambda gt: (R, np.int64(Qp), len(ROWS), P(ROWS), P(X), P(D), P(PG), P(kind), float(lam), P(alpha), P(Xt), P(out), P(stepn), P(gt), 0)
    call("gml_test_solver_trial", *args(None))
    first = out.copy()
    assert (Xt[3] == SENT).all() and out[3] == np.full(1, SENT, dtype=TRI)[0] and (stepn is None or stepn[3] == SENT)
    for r in ROWS:
        w, o = want[r], out[r]
        n, u = max(w["nterms"], 1), 2.0 ** -53
        print(f"row {r}: dd {o['dd']:.17g} - model {o['dd'] - w['dd']:.3g} (allowed {n * u * w['dd_abs']:.3g}); stepn - model {o['stepn'] - w['stepn']:.3g};"
              f" l1t - model {o['l1t'] - w['l1t']:.3g}; fallback {w['fallback']}")
        assert (np.abs(Xt[r] - w["xt"]) <= 2.0 ** -52 * (np.abs(X[r]) + np.abs(alpha[r] * D[r]))).all() and (Xt[r][w["clipped"]] == 0).all(), r
        assert (Xt[r][kind[r] == 0] == X[r][kind[r] == 0]).all()
        assert abs(o["dd"] - w["dd"]) <= n * u * w["dd_abs"] and abs(o["stepn"] - w["stepn"]) <= n * u * w["stepn"], r
        assert abs(o["l1t"] - w["l1t"]) <= Qp * u * w["l1t"] and o["back"] == 0.0, r
        assert stepn is None or stepn[r] == o["stepn"]
    if with_stepn:  # again, with k_back behind it
        call("gml_test_solver_trial", *args(Gt))
        for r in ROWS:
            b, babs, n = M.back_row(X[r], Xt[r], Gt[r], kind[r], lam)
            print(f"row {r}: back {out[r]['back']:.17g} - model {out[r]['back'] - b:.3g} (allowed {2 * max(n, 1) * 2.0 ** -53 * babs:.3g})")
            assert abs(out[r]["back"] - b) <= 2 * max(n, 1) * 2.0 ** -53 * babs, r  # (two terms per coordinate)
            assert (out[r]["dd"], out[r]["stepn"], out[r]["l1t"]) == (first[r]["dd"], first[r]["stepn"], first[r]["l1t"])
        assert out[3]["back"] == SENT


# ---- the matrix-free Newton-CG ------------------------------------------------------------------------------------------------------
PCG_QP, PCG_R = 700, 3


def pcg_problem(T, s1v, s2):
    """Three rows of 700 columns with |W| = 513, 4 T and 600: +-1 outer-product Hessians (as the other solve tests use), in the units
    the kernels read (Hd = (A + s2 g g^T) / s1)."""
    rng = np.random.default_rng(T + int(10 * s1v) + int(s2))
    Qp, R = PCG_QP, PCG_R
    nW = [513, 4 * T, 600]
    Hd = np.zeros((R, Qp, Qp)); X = np.zeros((R, Qp)); PG = np.zeros((R, Qp)); G = np.zeros((R, Qp)); kind = np.zeros((R, Qp), dtype=np.uint8)
    s1 = np.array([s1v, 1.0, s1v if s1v != 1.0 else 0.4])
    for r in range(R):
        Xs = rng.choice([-1.0, 1.0], size=(4 * Qp, Qp))
        A = (Xs * rng.random(4 * Qp)[:, None]).T @ Xs / (4 * Qp)
        G[r] = rng.normal(size=Qp) * 0.05
        Hd[r] = (A + s2 * np.outer(G[r], G[r])) / s1[r]
        kind[r] = 2
        kind[r, rng.choice(Qp, 30, replace=False)] = 0
        kind[r, rng.choice(np.flatnonzero(kind[r]), 2, replace=False)] = 1
        w = rng.choice(np.flatnonzero(kind[r]), nW[r], replace=False)
        nz = w[: nW[r] // 2]
        X[r, nz] = rng.choice([-1.0, 1.0], len(nz)) * rng.uniform(0.02, 0.2, len(nz))
        PG[r, w] = rng.normal(size=nW[r]) * 0.1
        PG[r, w[-20:]] = 0.0
        X[r, w[-20:]] = 0.05  # in W through x alone
        X[r, kind[r] == 0] = 1.0  # excluded columns: never in W
    return Hd, s1, X, PG, G, kind, nW


def run_pcg(T, prob, s2, live, nsteps, faces=0, nsteps2=0):
    Hd, s1, X, PG, G, kind, nW = prob
    R, Qp = PCG_R, PCG_QP
    rows = np.array([2, 0, 1], dtype=np.int32)
    tcap = R * ((Qp + T - 1) // T)
    FV, gV = np.full(tcap * T, -9, dtype=np.int32), np.full(tcap * T, SENT)
    D, Rv, Zv, Pv = (np.full((R, Qp), SENT) for _ in range(4))
    Wm = np.full((R, Qp), 9, dtype=np.uint8)
    cg, fo = np.full(R, SENT, dtype=CGS), np.zeros(R, dtype=FAC)
    fo["nfixed"] = -5
    lv = np.asarray(live, dtype=np.int32)
    call("gml_test_pcg", R, np.int64(Qp), T, len(rows), P(rows), P(Hd), P(s1), float(s2), P(X), P(PG), P(G), P(kind), P(lv), nsteps, faces, nsteps2,
         P(FV), P(gV), P(D), P(Rv), P(Zv), P(Pv), P(Wm), P(cg), P(fo), 0)
    return dict(rows=rows, FV=FV, gV=gV, D=D, Rv=Rv, Zv=Zv, Pv=Pv, Wm=Wm, cg=cg, fo=fo)


def models(T, prob, s2, r, nsteps, dtype):
    Hd, s1, X, PG, G, kind, nW = prob
    cg = M.Pcg(Hd[r], s1[r], s2, X[r], PG[r], G[r], kind[r], T, dtype)
    for _ in range(nsteps):
        cg.step()
    return cg


def spread_ok(got, m64, mld, nW, what):
    """the device within 16 x the distance of the float64 model from the longdouble model + |W| 2^-53 scale; returns the two distances"""
    ref = np.asarray(mld, dtype=np.float64)
    delta = float(np.abs(np.asarray(m64, dtype=np.float64) - ref).max())
    dist = float(np.abs(np.asarray(got) - ref).max())
    scale = float(np.abs(ref).max())
    assert dist <= 16 * delta + nW * 2.0 ** -53 * scale, (what, dist, delta, scale)
    return delta, dist


@pytest.mark.parametrize("s2", [0.0, 1.0])
@pytest.mark.parametrize("s1v", [1.0, 0.4])
@pytest.mark.parametrize("T", [64, 128])
def test_pcg_kernels_match_the_host_model(T, s1v, s2):
    """k_cg_tiles, k_pcg_init, k_pcg_dir, k_pcg_step with the tile preconditioner between them, state by state.

    Exact: FV / gV with their padding, Wm, and Rv, D, Pv after the initialisation (Zv and the first Pv are the preconditioner's product:
    to rounding).  After 1, 2 and 6 steps D, Rv, Pv and the CgState scalars lie within 16 delta_k + |W| 2^-53 scale of the longdouble
    model, delta_k = the distance of the same model run in float64 (the rounding spread of the algorithm on this input; 16 for the
    kernels' tree reductions against the model's sequential sums).  Row 1 is not live: its Zv stays untouched.
    Observed on an MI355X (T = 64, s1 = 0.4, s2 = 1, row 2; delta_k / the device's distance): D after 1, 2, 6 steps 3.3e-16 / 4.4e-16,
    5.0e-16 / 2.9e-16, 1.0e-15 / 2.2e-16; Rv 2.4e-16 / 2.4e-16, 1.8e-16 / 1.2e-16, 2.0e-17 / 1.3e-17; Pv 4.8e-16 / 4.7e-16, 3.6e-16 / 2.7e-16,
    4.3e-17 / 2.3e-17; the first Pv (the preconditioner alone) 2.8e-16 / 4.4e-16: the device stays below 2 delta_k."""
    prob = pcg_problem(T, s1v, s2)
    Hd, s1, X, PG, G, kind, nW = prob
    live = [1, 0, 1]
    for nsteps in (0, 1, 2, 6):
        got = run_pcg(T, prob, s2, live, nsteps)
        tile0 = 0
        for r in got["rows"]:
            inW = (kind[r] != 0) & ((X[r] != 0) | (PG[r] != 0))
            W = np.flatnonzero(inW)
            assert len(W) == nW[r]
            ntr = -(-len(W) // T)
            fv, gv = got["FV"][tile0 * T:(tile0 + ntr) * T], got["gV"][tile0 * T:(tile0 + ntr) * T]
            assert (fv[:len(W)] == W).all() and (fv[len(W):] == PCG_QP - 1).all() and (gv[:len(W)] == G[r][W]).all() and (gv[len(W):] == 0).all()
            tile0 += ntr
            assert (got["Wm"][r] == inW).all()
            if not live[r]:  # initialised, never stepped, Zv as k_pcg_init left it
                assert (got["Zv"][r] == 0).all() and (got["D"][r] == 0).all() and (got["Rv"][r] == np.where(inW, -PG[r], 0.0)).all()
                assert got["cg"][r]["rz"] == 0 and got["cg"][r]["pHp"] == 0
                continue
            m64, mld = models(T, prob, s2, r, nsteps, np.float64), models(T, prob, s2, r, nsteps, np.longdouble)
            if nsteps == 0:
                assert (got["Rv"][r] == np.where(inW, -PG[r], 0.0)).all() and (got["D"][r] == 0).all()
                assert (got["Pv"][r] == got["Zv"][r]).all() and (got["Zv"][r][~inW] == 0).all() and got["cg"][r]["pHp"] == 0
                assert got["cg"][r]["rs"] == got["cg"][r]["rs0"] and abs(got["cg"][r]["rs"] - float(mld.rs)) <= nW[r] * 2.0 ** -53 * float(mld.rs)
            for name, a, b in (("D", m64.d, mld.d), ("Rv", m64.r, mld.r), ("Pv", m64.p, mld.p)):
                delta, dist = spread_ok(got[name][r], a, b, nW[r], (name, r, nsteps))
                print(f"T {T} s1 {s1[r]} s2 {s2} row {r} step {nsteps} {name}: delta_k {delta:.3g}, device - model {dist:.3g}")
                assert (got[name][r][~inW] == 0).all()
            for name in ("rs", "rs0", "pHp", "rz"):
                a, b = float(getattr(m64, name)), float(getattr(mld, name))
                assert abs(got["cg"][r][name] - b) <= 16 * abs(a - b) + 4 * nW[r] * 2.0 ** -53 * abs(b), (name, r, nsteps, got["cg"][r][name], b)
        assert (got["FV"][tile0 * T:] == -9).all() and (got["gV"][tile0 * T:] == SENT).all()


@pytest.mark.parametrize("s2", [0.0, 1.0])
@pytest.mark.parametrize("T", [64, 128])
def test_pcg_converges_and_resolves_on_the_faces(T, s2):
    """Enough steps: rs / rs0 < 1e-20 and D = the direct solve on W to 1e-9 scale.  Then k_pcg_faces (nfixed, Wm and D at the fixed
    entries exact, mass and total to the sum bound), k_pcg_resid (Rv, rs against the model) and a second run of steps, which ends at the
    reduced solve B_ff d_f = -pg_f - B_fx d_x."""
    prob = pcg_problem(T, 0.4, s2)
    Hd, s1, X, PG, G, kind, nW = prob
    live = [1, 1, 1]
    nst = 60
    conv = run_pcg(T, prob, s2, live, nst)
    res = run_pcg(T, prob, s2, live, nst, faces=1, nsteps2=0)
    fin = run_pcg(T, prob, s2, live, nst, faces=1, nsteps2=nst)
    for r in range(PCG_R):
        B = s1[r] * Hd[r] - s2 * np.outer(G[r], G[r])
        W = np.flatnonzero((kind[r] != 0) & ((X[r] != 0) | (PG[r] != 0)))
        want = np.linalg.solve(B[np.ix_(W, W)], -PG[r][W])
        scale = np.abs(want).max()
        print(f"row {r}: rs/rs0 {conv['cg'][r]['rs'] / conv['cg'][r]['rs0']:.3g}, |D - solve| / scale {np.abs(conv['D'][r][W] - want).max() / scale:.3g}")
        assert conv["cg"][r]["rs"] < 1e-20 * conv["cg"][r]["rs0"] and np.abs(conv["D"][r][W] - want).max() <= 1e-9 * scale
        # the faces, from the device's own converged D (the model's candidates need margin against its 1e-9)
        inW = np.zeros(PCG_QP, dtype=bool)
        inW[W] = True
        cand, fixed, mass, total, margin = M.face_candidates(X[r], conv["D"][r], PG[r], kind[r], inW)
        assert margin >= 1e-6 and cand.sum() > 0, (r, margin)
        fo = res["fo"][r]
        assert fo["nfixed"] == cand.sum() and fo["pad"] == 0 and (res["Wm"][r] == (inW & ~cand)).all()
        assert (res["D"][r][cand] == fixed[cand]).all() and (res["D"][r][~cand] == conv["D"][r][~cand]).all()
        assert abs(fo["mass"] - mass) <= nW[r] * 2.0 ** -53 * mass and abs(fo["total"] - total) <= nW[r] * 2.0 ** -53 * total
        # the residual of the shrunk system
        d = res["D"][r].astype(np.longdouble)
        rv = np.where(res["Wm"][r] != 0, -PG[r] - (B.astype(np.longdouble) @ d), 0).astype(np.float64)
        tol = 8 * PCG_QP * 2.0 ** -53 * (np.abs(B) @ np.abs(res["D"][r]) + np.abs(PG[r])).max()
        assert np.abs(res["Rv"][r] - rv).max() <= tol, (r, np.abs(res["Rv"][r] - rv).max(), tol)
        rs = float(rv.astype(np.longdouble) @ rv.astype(np.longdouble))
        assert abs(res["cg"][r]["rs"] - rs) <= 1e-9 * rs and res["cg"][r]["pHp"] == 0 and res["cg"][r]["rs0"] == conv["cg"][r]["rs0"]
        # the second solve
        fr, fx = np.flatnonzero(res["Wm"][r]), np.flatnonzero(cand)
        want2 = np.linalg.solve(B[np.ix_(fr, fr)], -PG[r][fr] - B[np.ix_(fr, fx)] @ fixed[fx])
        print(f"row {r}: {cand.sum()} fixed, mass / total {mass / total:.3g}, |D - reduced solve| / scale {np.abs(fin['D'][r][fr] - want2).max() / np.abs(want2).max():.3g}")
        assert np.abs(fin["D"][r][fr] - want2).max() <= 1e-9 * np.abs(want2).max() and (fin["D"][r][fx] == fixed[fx]).all()
        assert (fin["Wm"][r] == res["Wm"][r]).all()
