"""The batched Newton solve of the direction phase (k_newton_chol: A d = -pg on ragged symmetric positive definite blocks, one
workgroup per row, blocked right-looking Cholesky with panels of 32) against numpy: one panel, partial last panels, sizes around
every multiple of 32 and 64 up to 512, mixed sizes in one launch; with and without the logRISE rank-one term."""
import ctypes as C

import numpy as np
import pytest

from gml_amd import _lib

pytestmark = pytest.mark.gpu


def solve(blocks, pg, s2=0.0, g=None):
    L = _lib.lib()
    L.gml_test_newton_solve.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_int]
    R, cap = blocks.shape[0], blocks.shape[1]
    ms = np.array([b for b in pg[1]], dtype=np.int32)
    out = np.zeros((R, cap))
    _lib.check(L.gml_test_newton_solve(R, _lib._ptr(ms), cap, _lib._ptr(np.ascontiguousarray(blocks)), _lib._ptr(np.ascontiguousarray(pg[0])),
                                       float(s2), _lib._ptr(g), _lib._ptr(out), 0))
    return out


@pytest.mark.parametrize("sizes", [[1, 5, 31, 32, 33, 63, 64], [65, 90, 96, 127, 128], [129, 160, 191, 192, 193, 200, 224, 255, 256],
                                   [257, 300, 384, 511, 512], [7, 64, 100, 128, 150, 200, 256, 300, 512]])
@pytest.mark.parametrize("logrise", [False, True])
def test_batched_newton_solve_matches_numpy(sizes, logrise):
    rng = np.random.default_rng(sum(sizes))
    cap = 512
    R = len(sizes)
    blocks = np.zeros((R, cap, cap))
    pg = np.zeros((R, cap))
    g = np.zeros((R, cap)) if logrise else None
    want = []
    for r, m in enumerate(sizes):
        X = rng.choice([-1.0, 1.0], size=(4 * m + 50, m))  # a Hessian-like block: weighted +-1 outer products
        h = rng.random(4 * m + 50)
        A = (X * h[:, None]).T @ X / len(h)
        gg = rng.normal(size=m) * 0.1 if logrise else np.zeros(m)
        blocks[r, :m, :m] = A + (np.outer(gg, gg) if logrise else 0.0)  # so that A_eff = H - g g^T stays positive definite
        pg[r, :m] = rng.normal(size=m)
        if logrise:
            g[r, :m] = gg
        want.append(np.linalg.solve(A, -pg[r, :m]))
    got = solve(blocks, (pg, sizes), s2=1.0 if logrise else 0.0, g=g)
    for r, m in enumerate(sizes):
        scale = np.abs(want[r]).max()
        assert np.abs(got[r, :m] - want[r]).max() <= 1e-9 * scale, (m, np.abs(got[r, :m] - want[r]).max() / scale)


@pytest.mark.parametrize("T", [64, 128])
@pytest.mark.parametrize("logrise", [False, True])
def test_tile_preconditioner_matches_numpy(T, logrise):
    """The block-diagonal preconditioner of the matrix-free rows (launch_tile_inverse + launch_tile_apply): full and partial tiles, a
    tile of one entry, and a tile that is not positive definite (two identical statistics), which must fall back to its diagonal."""
    L = _lib.lib()
    L.gml_test_tile_precond.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    rng = np.random.default_rng(T + logrise)
    sizes = [T, T, T - 1, T // 2 + 3, 1, 17, T]
    nt = len(sizes)
    tiles = np.zeros((nt, T, T))
    g = np.zeros((nt, T))
    r = rng.normal(size=(nt, T))
    s1, s2 = 0.7, (1.0 if logrise else 0.0)
    want = []
    for t, m in enumerate(sizes):
        X = rng.choice([-1.0, 1.0], size=(6 * m + 40, m))
        if t == nt - 1:
            X[:, 5] = X[:, 9]  # duplicate statistic: singular block
        h = rng.random(len(X))
        H = (X * h[:, None]).T @ X / len(h)
        gg = rng.normal(size=m) * 0.05 if logrise else np.zeros(m)
        tiles[t, :m, :m] = H / s1 + (np.outer(gg, gg) / s1 if logrise else 0.0)  # so that s1 H - s2 g g^T = the SPD matrix above
        tiles[t, m:, m:] = np.eye(T - m) * 3.0  # padding entries (the kernels must not touch them)
        g[t, :m] = gg
        A = s1 * tiles[t, :m, :m] - s2 * np.outer(gg, gg)
        want.append(r[t, :m] / np.diag(A) if t == nt - 1 else np.linalg.solve(A, r[t, :m]))
    z = np.zeros((nt, T))
    ms = np.array(sizes, dtype=np.int32)
    _lib.check(L.gml_test_tile_precond(T, nt, _lib._ptr(ms), _lib._ptr(np.ascontiguousarray(tiles)), s1, s2, _lib._ptr(g), _lib._ptr(r), _lib._ptr(z), 0))
    for t, m in enumerate(sizes):
        if t == nt - 1:  # ridge-regularised inverse or the diagonal: either way a finite, symmetric positive definite action
            assert np.isfinite(z[t]).all() and r[t, :m] @ z[t, :m] > 0
            continue
        scale = np.abs(want[t]).max()
        assert np.abs(z[t, :m] - want[t]).max() <= 1e-9 * scale, (t, m, np.abs(z[t, :m] - want[t]).max() / scale)
        assert (z[t, m:] == 0).all()


@pytest.mark.parametrize("logrise", [False, True])
def test_newton_resolve_with_fixed_entries_matches_numpy(logrise):
    """The orthant-face re-solve of the Cholesky rows (k_newton_chol with fix / dfix): fixed entries keep their prescribed step, the
    others solve A_ff d_f = -pg_f - A_fx dfix_x."""
    L = _lib.lib()
    L.gml_test_newton_solve_fixed.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_int]
    rng = np.random.default_rng(5 + logrise)
    sizes = [3, 33, 64, 100, 190, 257, 512]
    cap, R = 512, len(sizes)
    blocks = np.zeros((R, cap, cap)); pg = np.zeros((R, cap)); g = np.zeros((R, cap)) if logrise else None
    fix = np.zeros((R, cap), dtype=np.uint8); dfix = np.zeros((R, cap))
    want = []
    for r, m in enumerate(sizes):
        X = rng.choice([-1.0, 1.0], size=(4 * m + 50, m)); h = rng.random(len(X))
        A = (X * h[:, None]).T @ X / len(h)
        gg = rng.normal(size=m) * 0.1 if logrise else np.zeros(m)
        blocks[r, :m, :m] = A + np.outer(gg, gg)
        pg[r, :m] = rng.normal(size=m)
        if logrise:
            g[r, :m] = gg
        fx = rng.random(m) < 0.2
        fx[0] = True  # (at least one fixed, and one with a non-zero step)
        fix[r, :m] = fx
        dfix[r, :m] = np.where(fx, np.where(rng.random(m) < 0.5, 0.0, rng.normal(size=m) * 0.01), 0.0)
        dfix[r, 0] = 0.02
        d = dfix[r, :m].copy()
        fr = ~fx
        if fr.any():
            d[fr] = np.linalg.solve(A[np.ix_(fr, fr)], -pg[r, :m][fr] - A[np.ix_(fr, fx)] @ dfix[r, :m][fx])
        want.append(d)
    out = np.zeros((R, cap))
    ms = np.array(sizes, dtype=np.int32)
    _lib.check(L.gml_test_newton_solve_fixed(R, _lib._ptr(ms), cap, _lib._ptr(blocks), _lib._ptr(pg), 1.0 if logrise else 0.0, _lib._ptr(g),
                                             _lib._ptr(fix), _lib._ptr(dfix), _lib._ptr(out), 0))
    for r, m in enumerate(sizes):
        scale = np.abs(want[r]).max()
        assert np.abs(out[r, :m] - want[r]).max() <= 1e-9 * scale, (m, np.abs(out[r, :m] - want[r]).max() / scale)


# ---- gml_learn_warm: the same optimum from any starting point, in fewer iterations from a near one ----------------------------------
@pytest.mark.parametrize("form,c", [("RISE", 0.4), ("logRISE", 0.8), ("RPLE", 0.2)])
@pytest.mark.parametrize("prec", ["i8x", "i8w", "f64"])
def test_warm_start_reaches_the_cold_optimum(form, c, prec):
    import gml_amd as gml
    synthetic = __import__("importlib").import_module("gml_amd.synthetic")
    n, K = 96, 40000
    J = synthetic.block_ising_model(n, block=16, seed=4)
    with gml.Problem(model=J, num_samples=K, seed=1) as p:
        cold, kc, sc = p.learn(form, c, tol=1e-10, precision=prec)
        # from the optimum itself: the certifying pass, at most a polishing step
        again, ka, sa = p.learn(form, c, tol=1e-10, precision=prec, x0=cold)
        # (i8x at this tolerance ends on the FP64 path, below the noise floor of its own gradient: its restart re-enters that phase)
        assert sa["iterations"] <= (2 if prec != "i8x" else sc["iterations"]) and ka.max() <= 1e-10 and np.abs(again - cold).max() <= 2e-9
        # a regularisation path: 2c -> c from the previous solution
        far, _, sf = p.learn(form, 2 * c, tol=1e-10, precision=prec)
        warm, kw, sw = p.learn(form, c, tol=1e-10, precision=prec, x0=far)
        assert kw.max() <= 1e-10 and np.abs(warm - cold).max() <= 2e-9 and sw["iterations"] <= sc["iterations"]
        assert ((warm != 0) == (cold != 0)).all()
        # from a dense random point (every coordinate starts off its optimum, most of them off zero)
        rnd = np.random.default_rng(0).normal(scale=0.05, size=cold.shape)
        w2, k2, s2 = p.learn(form, c, tol=1e-10, precision=prec, x0=rnd)
        assert k2.max() <= 1e-10 and np.abs(w2 - cold).max() <= 2e-9
        bad = cold.copy()
        bad[3, 7] = np.nan
        with pytest.raises(gml.GMLError, match="non-finite"):
            p.learn(form, c, tol=1e-10, precision=prec, x0=bad)
        with pytest.raises(gml.GMLError, match="shape"):
            p.learn(form, c, tol=1e-10, precision=prec, x0=cold[:5])


def test_warm_start_multibody_and_node_shard():
    import gml_amd as gml
    synthetic = __import__("importlib").import_module("gml_amd.synthetic")
    n, K = 24, 30000
    terms = synthetic.block_multibody_terms(n, block=12, seed=7)
    with gml.Problem(terms=terms, n=n, num_samples=K, seed=2, order=3, node_range=(5, 17)) as p:
        cold, kc, sc = p.learn("RISE", 0.5, tol=1e-10)
        far, _, _ = p.learn("RISE", 1.0, tol=1e-6)
        warm, kw, sw = p.learn("RISE", 0.5, tol=1e-10, x0=far)
        assert cold.shape == (12, p.P) and kw.max() <= 1e-10 and np.abs(warm - cold).max() <= 2e-9
        again, ka, sa = p.learn("RISE", 0.5, tol=1e-10, x0=cold)
        assert sa["iterations"] <= 2 and np.abs(again - cold).max() <= 2e-9


# ---- the direction phase of the Cholesky rows, as Solver::newton_blocks runs it: k_secant, the solve with the secant pairs and the
# ---- orthant faces inside, k_scatter_dir (gml_test_newton_direction) against tests/_solver_reference.py -----------------------------
import _solver_reference as M  # noqa: E402

CAP, DQP, DSENT = 512, 600, -777.25


class DirState:
    """the secant state of R rows as the hook takes and returns it"""
    NAMES = ("Fprev", "mprev", "npairs", "xprev", "gprev", "S", "Y")

    def __init__(self, R):
        self.Fprev = np.full((R, CAP), -1, dtype=np.int32)
        self.mprev, self.npairs = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
        self.xprev, self.gprev = np.full((R, CAP), DSENT), np.full((R, CAP), DSENT)
        self.S, self.Y = np.full((2, R, CAP), DSENT), np.full((2, R, CAP), DSENT)

    def snapshot(self):
        return [getattr(self, n).copy() for n in self.NAMES]

    def restore(self, snap):
        for n, a in zip(self.NAMES, snap):
            setattr(self, n, a.copy())

    def assert_equals(self, model, tag):
        for r, st in enumerate(model):
            assert (self.Fprev[r] == st.Fprev).all() and self.mprev[r] == st.mprev and self.npairs[r] == st.npairs, (tag, r, self.npairs[r], st.npairs)
            assert (self.xprev[r] == st.xprev).all() and (self.gprev[r] == st.gprev).all(), (tag, r)
            assert (self.S[:, r] == st.S).all() and (self.Y[:, r] == st.Y).all(), (tag, r)


def direction(rows, m, F, blocks, gF, pgF, s1, s2, X, kind, st, secant=1, apply_above=128, pairs=1, ynoise=None, faces=0, share=0.05, rounds=0,
              fix=None, dfix=None):
    """gml_test_newton_direction; returns (corrected blocks, dsol, Sdiag, D); st (DirState) is updated in place"""
    L = _lib.lib()
    V, I, D_ = C.c_void_p, C.c_int, C.c_double
    L.gml_test_newton_direction.argtypes = [I, I, C.c_int64, I, V, V, V, V, V, V, V, D_, V, V, I, I, I, V, V, V, V, V, V, V, V, I, D_, I, V, V, V, V, V, I]
    R = len(m)
    rows, m, F = np.asarray(rows, dtype=np.int32), np.asarray(m, dtype=np.int32), np.ascontiguousarray(F, dtype=np.int32)
    out = np.ascontiguousarray(blocks).copy()
    dsol, Sdiag, D = np.full((R, CAP), DSENT), np.full(R, DSENT), np.full((R, DQP), DSENT)
    yn = np.zeros(R) if ynoise is None else np.asarray(ynoise, dtype=np.float64)
    p = _lib._ptr
    _lib.check(L.gml_test_newton_direction(R, CAP, DQP, len(rows), p(rows), p(m), p(F), p(out), p(gF), p(pgF), p(np.asarray(s1, dtype=np.float64)), float(s2),
                                           p(X), p(kind), secant, apply_above, pairs, p(yn), p(st.Fprev), p(st.mprev), p(st.xprev), p(st.gprev), p(st.S),
                                           p(st.Y), p(st.npairs), faces, float(share), rounds, p(fix), p(dfix), p(dsol), p(Sdiag), p(D), 0))
    return out, dsol, Sdiag, D


def check_scatter(rows, m, F, dsol, D):
    """k_scatter_dir: D = dsol on F, zero off it (where the sentinel was), all zero for m = 0; rows not listed keep the sentinel"""
    for r in range(len(m)):
        if r not in rows:
            assert (D[r] == DSENT).all()
            continue
        want = np.zeros(DQP)
        want[F[r, :m[r]]] = dsol[r, :m[r]]
        assert (D[r] == want).all(), r


def pd_block(rng, m, extra=1.0):
    """a Hessian-like block (weighted +-1 outer products) plus a multiple of the identity"""
    Xs = rng.choice([-1.0, 1.0], size=(4 * m + 50, m))
    B = (Xs * rng.random(len(Xs))[:, None]).T @ Xs / len(Xs) + extra * np.eye(m)
    return (B + B.T) / 2  # (symmetric to the last bit: the kernels read the lower triangle only)


SIZES = [1, 5, 33, 100, 128, 129, 200, 512, 0]


@pytest.mark.parametrize("s2", [0.0, 1.0])
def test_secant_state_and_corrected_direction(s2):
    """A sequence of calls on rows of 1 .. 512 entries (and one of none) whose gradients come from a true quadratic g = A x + b while
    the block holds B = A + a perturbation, in the kernels' units (H = (B + s2 g g^T) / s1, s1 in {1, 0.37, 25} by row): no pair, one,
    two, the oldest dropped, three rejected pairs (s = 0, y orthogonal to s, ymax below the noise) with the old ones still applied, and
    a reset by one changed column at equal size.  After every call the secant state equals the model's exactly.

    Every call with pairs is run twice from the same state: with k_secant correcting every block in global memory (apply_above = 0; the
    solve gets no pairs) and as the solver runs it (apply_above = 128: the solve kernel corrects the smaller blocks in LDS).  The blocks
    k_secant returns are held to the model entry-wise; both runs' dsol to numpy's solve of the corrected matrix (1e-9 scale, as the
    tests above), Sdiag to its last diagonal entry.

    The entry-wise bound (M.bfgs): a float64 inner product of n terms is within gamma_n sum |terms| of the exact one (gamma_n =
    n u / (1 - n u)).  With dB the bound carried in, v = B s has error dv <= dB |s| + gamma_{m+3} (Babs |s|) (Babs: s1 |H| + s2 |g||g|^T,
    the scaling and the rank-one term are the three extra operations); s.v has d(sBs) <= |s|.dv + gamma_{m+1} |s|.(Babs |s|), y.s has
    d(ys) <= gamma_{m+1} |s|.|y|.  A quotient a b / c with errors da, db, dc is off by at most (da |b| + |a| db + da db) / (c - dc) +
    |a b| dc / (c (c - dc)) + 4 u |a b| / (c - dc) (two products, the reciprocal, the sum); that is e2 for v v^T / sBs and e1 for
    y y^T / ys, and dB grows by e1 + e2 + 3 u Babs per pair.  In H's units the bound is dB / s1 + 2 u |H|.  The inputs keep it below
    1e-10 max |B| (asserted)."""
    rng = np.random.default_rng(11 + int(s2))
    R = len(SIZES)
    rows = np.array([3, 8, 0, 7, 5, 1, 2, 6, 4], dtype=np.int32)
    s1 = np.array([[1.0, 0.37, 25.0][r % 3] for r in range(R)])
    kind = np.full((R, DQP), 2, dtype=np.uint8)
    A, Bm, b, F = [], [], [], np.full((R, CAP), DQP - 1, dtype=np.int32)
    for r, m in enumerate(SIZES):
        A.append(pd_block(rng, m))
        Bm.append(A[r] + 0.3 * pd_block(rng, m, 0.0))  # what the sub-sampled block would be: not the true Hessian
        b.append(rng.normal(size=m) * 0.1)  # (a gradient of the size logRISE sees: the rank-one term stays a correction)
        F[r, :m] = np.sort(rng.choice(DQP - 1, m, replace=False))
    st, model = DirState(R), [M.SecantState(CAP, fill=DSENT, ifill=-1) for _ in range(R)]

    def run(tag, xs, gs=None, ynoise=0.0, both=True):
        X = rng.normal(size=(R, DQP))
        gF, pgF, blocks = np.zeros((R, CAP)), np.zeros((R, CAP)), np.zeros((R, CAP, CAP))
        for r, m in enumerate(SIZES):
            X[r, F[r, :m]] = xs[r]
            gF[r, :m] = A[r] @ xs[r] + b[r] if gs is None else gs[r]
            pgF[r, :m] = gF[r, :m] + rng.normal(size=m) * 0.01
            blocks[r, :m, :m] = (Bm[r] + s2 * np.outer(gF[r, :m], gF[r, :m])) / s1[r]
        infos = [model[r].step(F[r, :m], xs[r], gF[r, :m], ynoise) for r, m in enumerate(SIZES)]
        for r, info in enumerate(infos):
            if info is not None and info["ss"] > 0 and info["yy"] > 0:  # no pair is decided by rounding
                assert not 0.9e-4 <= info["ratio"] <= 1.1e-4, (tag, r, info["ratio"])
        want = []
        for r, m in enumerate(SIZES):
            Hc, Bc, dH = M.corrected_block(blocks[r, :m, :m], gF[r, :m], s1[r], s2, model[r].pairs(m))
            if m:
                assert float(dH.max()) * s1[r] <= 1e-10 * float(np.abs(Bc).max()), (tag, m, float(dH.max()))
            want.append((Hc.astype(np.float64), Bc.astype(np.float64), dH.astype(np.float64)))
        before = st.snapshot()
        for name, above, prs in [("solver", 128, 1)] + ([("global", 0, 0)] if both else []):
            st.restore(before)
            blk, dsol, Sd, D = direction(rows, SIZES, F, blocks, gF, pgF, s1, s2, X, kind, st, apply_above=above, pairs=prs, ynoise=np.full(R, ynoise))
            st.assert_equals(model, (tag, name))
            check_scatter(rows, SIZES, F, dsol, D)
            for r, m in enumerate(SIZES):
                if m == 0:
                    assert (dsol[r] == DSENT).all() and Sd[r] == DSENT
                    continue
                Hc, Bc, dH = want[r]
                corrected = m > above
                ref = Hc if corrected else blocks[r, :m, :m]
                err = np.abs(blk[r, :m, :m] - ref)
                assert (err <= (dH if corrected else 0.0)).all(), (tag, name, m, float(err.max()), float(np.max(dH)))
                d = np.linalg.solve(Bc, -pgF[r, :m])
                scale = np.abs(d).max()
                assert np.abs(dsol[r, :m] - d).max() <= 1e-9 * scale, (tag, name, m, np.abs(dsol[r, :m] - d).max() / scale)
                tol = s1[r] * dH[-1, -1] + 8 * M.U * (s1[r] * abs(Hc[-1, -1]) + s2 * gF[r, m - 1] ** 2)  # (the entry's bound, and forming it)
                assert abs(Sd[r] - Bc[m - 1, m - 1]) <= tol, (tag, name, m, Sd[r] - Bc[m - 1, m - 1], tol)
                assert (dsol[r, m:] == DSENT).all()
        return infos

    xs = [[rng.normal(size=m) * 0.1 for m in SIZES] for _ in range(5)]
    run("first call: no previous set", xs[0], both=False)
    assert all(s.npairs == 0 for s in model)
    run("one pair", xs[1])
    assert all(s.npairs == 1 for s in model[:-1])
    run("two pairs", xs[2])
    run("the oldest dropped", xs[3])
    assert all(s.npairs == 2 for s in model[:-1]) and model[-1].npairs == 0 and model[-1].mprev == 0
    keep = [s.S.copy() for s in model]
    run("s = 0", xs[3])
    # y orthogonal to s: g moves within the plane orthogonal to the step
    gs = []
    for r, m in enumerate(SIZES):
        s_ = xs[4][r] - xs[3][r]
        y = rng.normal(size=m) * 0.1
        y -= s_ * (y @ s_) / max(s_ @ s_, 1e-300)
        gs.append(A[r] @ xs[3][r] + b[r] + y)
    infos = run("y orthogonal to s", xs[4], gs=gs)
    assert all(abs(i["ratio"]) < 1e-12 for i in infos[:-1])
    run("ymax below the noise", xs[0], ynoise=1e3)
    assert all(s.npairs == 2 for s in model[:-1]) and all((s.S == k).all() for s, k in zip(model, keep))
    for r, m in enumerate(SIZES):  # one column changed at equal size: the pairs are dropped
        if m:
            F[r, m - 1] = DQP - 1
    run("one column changed", xs[1], both=False)
    assert all(s.npairs == 0 for s in model)
    run("a pair again", xs[2])
    assert all(s.npairs == 1 for s in model[:-1])


def face_row(seed, m, s2, with_pairs, calm=False):
    """One row for the face tests: a block, a true quadratic for its pairs, an iterate with zeros and non-zeros so that some entries of
    the Newton step leave the orthant face.  Returns dict(H, g, pg, x, kind, pairs, B): B the (corrected) matrix in float64."""
    rng = np.random.default_rng(seed)
    Z = rng.normal(size=(4 * m + 50, m)) + 0.7 * rng.normal(size=(4 * m + 50, 3)) @ rng.normal(size=(3, m))  # correlated statistics
    Xs = np.sign(Z)
    B0 = (Xs * rng.random(len(Xs))[:, None]).T @ Xs / len(Xs) + 0.02 * np.eye(m)
    B0 = (B0 + B0.T) / 2
    A = B0 + 0.3 * pd_block(rng, m, 0.0)
    g = rng.normal(size=m) * 0.1
    pg = rng.normal(size=m)
    pairs = []
    if with_pairs:
        for _ in range(2):
            s = rng.normal(size=m) * 0.1
            pairs.append((s, A @ s))
    s1 = [1.0, 0.37, 25.0][seed % 3]
    H = (B0 + s2 * np.outer(g, g)) / s1
    _, Bc, _ = M.corrected_block(H, g, s1, s2, pairs)
    Bc = Bc.astype(np.float64)
    d0 = np.linalg.solve(Bc, -pg)
    u = rng.random(m)
    # zeros (a step along pg leaves the face), non-zeros the step crosses (x = -d/2 or so), non-zeros it stops just short of (a
    # re-solve may push them over) and non-zeros it moves away from zero
    lim = 0.4 + 0.02 * (seed % 7)
    x = np.where(u < 0.4, 0.0, np.where(u < lim, -d0 * rng.uniform(0.3, 0.7, m),
                                        np.where(u < lim + 0.3, -d0 * rng.uniform(1.02, 1.3, m), np.sign(d0) * rng.uniform(0.5, 2.0, m))))
    if calm:  # hardly anything leaves the face: a few zeros, everything else moves away from zero
        x = np.where(u < 0.1, 0.0, np.sign(d0) * rng.uniform(0.5, 2.0, m))
    kind = np.where(rng.random(m) < 0.1, 1, 2).astype(np.uint8)
    return dict(H=H, g=g, pg=pg, x=x, kind=kind, pairs=pairs, B=Bc, s1=s1)


def stage_rows(rowsdata, s2, with_pairs, seed):
    """the hook's arrays for a list of face_row-like dicts (None: a row of no entries): working sets at random columns, the iterate on
    them, and -- with pairs -- a secant state that holds the rows' two pairs and meets a zero step, so that k_secant keeps them and
    applies them to the larger blocks while the solve kernel applies them to the smaller ones"""
    rng = np.random.default_rng(seed)
    R = len(rowsdata)
    m = np.array([0 if d is None else len(d["pg"]) for d in rowsdata], dtype=np.int32)
    F = np.full((R, CAP), DQP - 1, dtype=np.int32)
    X, kind = rng.normal(size=(R, DQP)), np.full((R, DQP), 2, dtype=np.uint8)
    gF, pgF, blocks, s1 = np.zeros((R, CAP)), np.zeros((R, CAP)), np.zeros((R, CAP, CAP)), np.ones(R)
    st = DirState(R)
    for r, d in enumerate(rowsdata):
        if d is None:
            continue
        k = m[r]
        F[r, :k] = np.sort(rng.choice(DQP, k, replace=False))
        X[r, F[r, :k]], kind[r, F[r, :k]] = d["x"], d["kind"]
        gF[r, :k], pgF[r, :k], blocks[r, :k, :k], s1[r] = d["g"], d["pg"], d["H"], d["s1"]
        if with_pairs:
            st.Fprev[r, :k], st.mprev[r], st.npairs[r] = F[r, :k], k, len(d["pairs"])
            st.xprev[r, :k], st.gprev[r, :k] = d["x"], d["g"]
            for l, (s, y) in enumerate(d["pairs"]):
                st.S[l, r, :k], st.Y[l, r, :k] = s, y
    return m, F, X, kind, gF, pgF, blocks, s1, st


FACE_SHARE = 1e-3
# seeds of face_row by (pairs, m): re-solves once, twice, never (a calm row) at FACE_SHARE and two rounds -- asserted on the model below
FACE_SEEDS = {(False, 100): (0, 3, 3), (False, 200): (8, 1, 1), (True, 100): (0, 2, 3), (True, 200): (1, 0, 1)}


@pytest.mark.parametrize("with_pairs", [False, True])
@pytest.mark.parametrize("s2", [0.0, 1.0])
def test_orthant_faces_inside_the_solve(s2, with_pairs):
    """The face detection of the solve kernels (NewtonFaces), in LDS (100 entries) and on the global block (200): which entries are
    fixed, when a re-solve is triggered, and that both sides of a re-solve use the corrected matrix.  Per size one row that re-solves
    once, one that re-solves twice (rounds = 2) and one whose candidates stay below the share; all again with rounds = 0.  The model's
    decisions have margin (asserted): a candidate's sign tests are at least 1e-5 away from zero relative to their factors, mass / total
    at least 10 % away from the share.  Result: 1e-9 scale against the model."""
    data, patterns = [], []
    for m in (100, 200):
        once, twice, never = FACE_SEEDS[(with_pairs, m)]
        data += [face_row(once, m, s2, with_pairs), face_row(twice, m, s2, with_pairs), face_row(never, m, s2, with_pairs, calm=True)]
        patterns += [[True, False], [True, True], [False]]
    data.insert(2, None)  # a row of no entries between them
    patterns.insert(2, None)
    m, F, X, kind, gF, pgF, blocks, s1, st0 = stage_rows(data, s2, with_pairs, 5)
    rows = np.array([6, 0, 3, 5, 1, 4, 2], dtype=np.int32)
    want = {}
    for r, d in enumerate(data):
        if d is None:
            continue
        dd, log = M.solve_faces(d["B"], d["pg"], d["x"], d["kind"], FACE_SHARE, 2)
        assert [e["again"] for e in log] == patterns[r], (r, log)
        for e in log:
            assert e["n"] > 0 and e["margin"] >= 1e-5 and abs(e["mass"] / e["total"] / FACE_SHARE - 1) >= 0.1, (r, e)
        d0, _ = M.solve_faces(d["B"], d["pg"], d["x"], d["kind"], FACE_SHARE, 0)
        assert patterns[r] == [False] or np.abs(dd - d0).max() > 1e-3 * np.abs(d0).max()  # a re-solve is no detail
        want[r] = {2: dd, 0: d0}
    for rounds in (2, 0):
        st = DirState(len(data))
        st.restore(st0.snapshot())
        blk, dsol, Sd, D = direction(rows, m, F, blocks, gF, pgF, s1, s2, X, kind, st, secant=int(with_pairs), apply_above=128, pairs=int(with_pairs),
                                     faces=1, share=FACE_SHARE, rounds=rounds)
        check_scatter(rows, m, F, dsol, D)
        assert (st.npairs == st0.npairs).all() and (st.S == st0.S).all()
        for r, w in want.items():
            scale = np.abs(w[rounds]).max()
            err = np.abs(dsol[r, :m[r]] - w[rounds]).max()
            print(f"m {m[r]} rounds {rounds} pattern {patterns[r]}: |d - model| / scale {err / scale:.3g}")
            assert err <= 1e-9 * scale, (r, m[r], rounds, err / scale)


@pytest.mark.parametrize("s2", [0.0, 1.0])
def test_ridge_restart_with_secant_pairs(s2):
    """A block with a duplicated statistic (singular; its pairs, gradient and right-hand side share the duplication, so the corrected
    matrix is singular too and the system stays consistent) at 100 entries (the LDS kernel: reloads the block, applies the pairs again)
    and at 200, next to well-conditioned rows.  The singular rows give a finite descent step -- what the tile test asserts -- that
    solves the CORRECTED system (residual below 1e-6 of the right-hand side: Cholesky is backward stable whatever the ridge, and the
    null vector of the matrix does not show in the residual); their neighbours match numpy to 1e-9 scale."""
    rng = np.random.default_rng(21 + int(s2))
    data = []
    for m, sing in ((100, True), (60, False), (200, True), (150, False), (128, False)):
        def block(extra):
            Xs = rng.choice([-1.0, 1.0], size=(4 * m + 50, m))
            if sing:
                Xs[:, 9] = Xs[:, 5]
            B = (Xs * rng.random(len(Xs))[:, None]).T @ Xs / len(Xs) + (0.0 if sing else extra) * np.eye(m)
            return (B + B.T) / 2
        B0 = block(0.5)
        A = B0 + 0.3 * block(0.0)
        g, pg = rng.normal(size=m) * 0.1, rng.normal(size=m)
        if sing:
            g[9], pg[9] = g[5], pg[5]
        pairs = []
        for _ in range(2):
            s = rng.normal(size=m) * 0.1
            pairs.append((s, A @ s))
        s1 = [0.37, 1.0, 25.0][len(data) % 3]
        H = (B0 + s2 * np.outer(g, g)) / s1
        _, Bc, _ = M.corrected_block(H, g, s1, s2, pairs)
        Bc = Bc.astype(np.float64)
        if sing:
            assert (H[5] == H[9]).all() and all(y[5] == y[9] for _, y in pairs) and np.abs(Bc[5] - Bc[9]).max() <= 1e-14
            assert np.abs(Bc - (s1 * H - s2 * np.outer(g, g))).max() > 1e-3  # the correction is no detail
        data.append(dict(H=H, g=g, pg=pg, x=rng.normal(size=m), kind=np.full(m, 2, dtype=np.uint8), pairs=pairs, B=Bc, s1=s1, sing=sing))
    m, F, X, kind, gF, pgF, blocks, s1, st = stage_rows(data, s2, True, 6)
    rows = np.array([2, 4, 0, 3, 1], dtype=np.int32)
    blk, dsol, Sd, D = direction(rows, m, F, blocks, gF, pgF, s1, s2, X, kind, st, secant=1, apply_above=128, pairs=1)
    check_scatter(rows, m, F, dsol, D)
    for r, d in enumerate(data):
        got = dsol[r, :m[r]]
        if d["sing"]:
            res = np.abs(d["B"] @ got + d["pg"]).max() / np.abs(d["pg"]).max()
            print(f"singular row of {m[r]}: max |d| {np.abs(got).max():.3g}, pg.d {d['pg'] @ got:.3g}, residual of the corrected system {res:.3g}")
            assert np.isfinite(got).all() and d["pg"] @ got < 0
            assert res <= 1e-6
        else:
            want = np.linalg.solve(d["B"], -d["pg"])
            assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (r, m[r])
