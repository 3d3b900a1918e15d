"""The host model of the solver's kernels (tests/_solver_reference.py) against independent mathematics: there is no host header to
compile the model against, so each piece is held to its textbook definition by brute force.  No GPU."""
import itertools
import math

import numpy as np
import pytest

import _solver_reference as M


def test_pseudo_gradient_is_the_minimum_norm_subgradient():
    grid = [-2.0, -1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0, 2.0]
    for x, g, lam in itertools.product([-1.5, -1e-300, 0.0, 1e-300, 0.7], grid, [0.0, 0.5, 1.0]):
        # the subdifferential of g x + lam |x| at x: g + lam [-1, 1] at zero, g + lam sign(x) elsewhere; sampled densely
        ts = np.linspace(-1.0, 1.0, 4001) if x == 0 else np.array([np.sign(x)])
        sub = g + lam * ts
        want = sub[np.argmin(np.abs(sub))]
        assert M.pseudo_grad(x, g, lam) == pytest.approx(want, abs=1e-12), (x, g, lam)
    # vectorised with a per-column lambda, and the unpenalised column
    pg = M.pseudo_grad(np.array([0.0, 0.0, 1.0]), np.array([0.3, 0.3, 0.3]), np.array([0.0, 0.5, 0.5]))
    assert (pg == np.array([0.3, 0.0, 0.8])).all()


def brute_threshold(pat, max_add):
    """the bisection's answer by definition: the largest hi = lo + 1 with count(v >= lo) > max_add >= count(v >= hi); the class at lo
    when nothing lies above it"""
    vals = sorted(set(int(p) for p in pat))
    for lo in reversed(vals):
        if sum(int(p) >= lo for p in pat) > max_add:
            hi = lo + 1
            return hi if any(int(p) >= hi for p in pat) else lo
    raise AssertionError


def test_admission_threshold_equals_a_brute_force_sort():
    rng = np.random.default_rng(0)
    for trial in range(300):
        n = int(rng.integers(2, 40))
        vals = rng.choice(rng.random(int(rng.integers(1, 6))) + 0.1, size=n) if trial % 2 else rng.random(n) + 1e-3  # with ties / without
        if trial % 5 == 0:
            vals[: n // 2] = 1.0 + 1e-12 * rng.random(n // 2)  # equal to float32 resolution: one class
        pat = M.f32_pattern(vals)
        max_add = int(rng.integers(0, n))
        thr = M.admission_threshold(pat, max_add)
        assert thr == brute_threshold(pat, max_add)
        admitted = int((pat >= thr).sum())
        srt = np.sort(pat)[::-1]
        if srt[0] > srt[max_add]:  # something above the cut: at most max_add, and every one of them above the (max_add + 1)-th
            assert 0 < admitted <= max_add and (pat[pat >= thr] > srt[max_add]).all()
        else:  # the largest class straddles the cut: all of it
            assert admitted == int((pat == srt[0]).sum()) > max_add
    assert M.f32_pattern(1.0) == M.f32_pattern(1.0 + 1e-12) and M.f32_pattern(1.0) < M.f32_pattern(1.0 + 1e-6)


def test_select_row_working_set_and_scalars():
    kind = np.array([1, 2, 2, 0, 2, 2, 2, 2], dtype=np.uint8)
    x = np.array([0.0, 0.5, 0.0, 9.0, 0.0, 0.0, -0.25, 0.0])
    g = np.array([0.01, -0.1, 0.9, 5.0, -0.7, 0.3, 0.1, 0.05])
    o = M.select_row(x, g, kind, 0.1, 1, 8, 8, 0.0, best=1.0)
    # pg: field g; support g + lam sign x; zeros shrink by lam; the excluded column contributes nothing
    assert np.allclose(o["pg"], [0.01, 0.0, 0.8, 0.0, -0.6, 0.2, 0.0, 0.0])
    assert (o["nsupp"], o["nviol"], o["m"]) == (3, 3, 4) and o["F"].tolist() == [0, 1, 2, 6, 7, 7, 7, 7]
    assert o["worst"] == pytest.approx(0.8) and o["worstW"] == pytest.approx(0.01) and o["l1"] == pytest.approx(0.075)
    assert o["better"] and o["best"] == o["worst"]
    # the support residual dominates: nothing is admitted
    g2 = g.copy()
    g2[1] = -3.0
    o = M.select_row(x, g2, kind, 0.1, 1, 8, 8, 0.0, best=0.5)
    assert not o["addv"] and o["m"] == 3 and not o["better"] and o["best"] == 0.5
    # a working set above capW: matrix-free, m = -|W|, the cut drops the small violators
    o = M.select_row(x, g, kind, 0.1, 8, 3, 8, 0.5, best=1.0)
    assert o["m"] == -5 and o["F"] is None and o["pg"][5] == 0.0 and o["pg"][4] == pytest.approx(-0.6)
    assert M.select_row(x, g, kind, 0.1, 8, 3, 8, 0.0, best=1.0)["m"] == -6
    # tile rounding and the doubling
    assert M.effective_max_add(64, 1, 100, 512) == 63 and M.effective_max_add(64, 40, 100, 512) == 56
    assert M.effective_max_add(5, 1, 100, 512) == 5 and M.effective_max_add(5, 1, 129, 8) == 10 and M.effective_max_add(64, 1, 129, 8) == 127
    # NaN: an infinite residual, never the best iterate
    g3 = g.copy()
    g3[1] = np.nan
    o = M.select_row(x, g3, kind, 0.1, 1, 8, 8, 0.0, best=1.0)
    assert o["worst"] == math.inf and not o["better"]


def spd(rng, m, cond=30.0):
    Q, _ = np.linalg.qr(rng.normal(size=(m, m)))
    return (Q * np.geomspace(1.0, cond, m)) @ Q.T


def test_bfgs_secant_equation_definiteness_and_recursion():
    rng = np.random.default_rng(1)
    for m in (1, 2, 7, 40):
        A = spd(rng, m)
        B0 = spd(rng, m)
        pairs = []
        for _ in range(2):
            s = rng.normal(size=m)
            pairs.append((s, A @ s))  # pairs of a true SPD quadratic
        B2, dB = M.bfgs(B0, pairs)
        s, y = pairs[-1]
        assert np.abs(B2.astype(np.float64) @ s - y).max() <= 1e-12 * np.abs(y).max()  # B+ s_last = y_last
        assert np.linalg.eigvalsh(B2.astype(np.float64)).min() > 0
        B64, _ = M.bfgs(B0, pairs, dtype=np.float64)  # the bound covers a float64 evaluation
        assert (np.abs(B64 - B2) <= dB).all() and dB.max() <= 1e-11 * np.abs(B0).max()
        # oldest first == the recursive formula applied twice
        B1 = B0 - np.outer(B0 @ pairs[0][0], B0 @ pairs[0][0]) / (pairs[0][0] @ B0 @ pairs[0][0]) + np.outer(pairs[0][1], pairs[0][1]) / (pairs[0][1] @ pairs[0][0])
        Br = B1 - np.outer(B1 @ s, B1 @ s) / (s @ B1 @ s) + np.outer(y, y) / (y @ s)
        assert np.abs(B2.astype(np.float64) - Br).max() <= 1e-11 * np.abs(Br).max()
        # a pair with y.s <= 0 is skipped
        assert (M.bfgs(B0, [(s, -y)])[0] == B0.astype(M.LD)).all()
        # the block form: s1 H' - s2 g g^T is the corrected matrix
        g = rng.normal(size=m) * 0.1
        H = (B0 + np.outer(g, g)) / 0.37
        Hc, Bc, _ = M.corrected_block(H, g, 0.37, 1.0, pairs)
        assert np.abs((0.37 * Hc - np.outer(g, g) - B2).astype(np.float64)).max() <= 1e-13 * np.abs(B0).max()


def test_secant_state_machine():
    st = M.SecantState(6, fill=7.0, ifill=-1)
    F = np.array([1, 4, 5], dtype=np.int32)
    A = np.diag([1.0, 2.0, 3.0])
    xs = [np.array([0.1, 0.2, 0.3]), np.array([0.2, 0.1, 0.3]), np.array([0.3, 0.3, 0.1]), np.array([0.0, 0.1, 0.2]), np.array([0.5, 0.1, 0.2])]
    assert st.step(F, xs[0], A @ xs[0], 0.0) is None and st.npairs == 0 and st.mprev == 3  # first call: no previous set
    for k in (1, 2):
        assert st.step(F, xs[k], A @ xs[k], 0.0) is not None and st.npairs == k
    first = st.S[1, :3].copy()
    st.step(F, xs[3], A @ xs[3], 0.0)  # a third pair: the oldest goes
    assert st.npairs == 2 and (st.S[0, :3] == first).all() and (st.S[1, :3] == xs[3] - xs[2]).all() and (st.S[:, 3:] == 7.0).all()
    st.step(F, xs[3], A @ xs[3], 0.0)  # s = 0: rejected, the old pairs stay
    assert st.npairs == 2
    st.step(F, xs[4], A @ xs[4], 10.0)  # below the noise: rejected
    assert st.npairs == 2
    st.step(np.array([1, 3, 5], dtype=np.int32), xs[4], A @ xs[4], 0.0)  # another set of the same size: reset
    assert st.npairs == 0 and st.Fprev[:3].tolist() == [1, 3, 5]
    assert st.step(np.array([], dtype=np.int32), [], [], 0.0) is None and st.mprev == 3  # m = 0: untouched


def test_trial_and_back_on_a_convex_quadratic():
    rng = np.random.default_rng(2)
    n, lam = 12, 0.3
    A = spd(rng, n)
    b = rng.normal(size=n)
    kind = np.array([1] + [2] * (n - 2) + [0], dtype=np.uint8)
    pen = kind == 2

    def Fobj(x):
        return 0.5 * x @ A @ x + b @ x + lam * np.abs(x[pen]).sum()

    worse = better = 0
    for it in range(200):
        x = np.where(rng.random(n) < 0.5, 0.0, rng.normal(size=n))
        x[-1] = 0.0
        g = A @ x + b
        pg = M.pseudo_grad(x, g, np.where(pen, lam, 0.0)) * (kind != 0)
        d = np.where(kind != 0, -pg * rng.random(n) * 2.0 + rng.normal(size=n) * 0.3, 5.0)  # (the excluded column's d is ignored)
        al = [1.0, 0.5, 1 / 64][it % 3]
        t = M.trial_row(x, d, pg, kind, lam, al)
        xt = t["xt"]
        assert xt[-1] == 0.0 and (np.sign(xt[pen]) * np.sign(x[pen]) >= 0).all()  # same orthant
        assert t["dd"] == pytest.approx(pg @ (xt - x), abs=1e-12) and t["stepn"] == pytest.approx(np.abs(xt - x).sum(), abs=1e-12)
        assert t["l1t"] == pytest.approx(lam * np.abs(xt[pen]).sum(), abs=1e-12) and t["dd"] <= 0
        back, _, _ = M.back_row(x, xt, A @ xt + b, kind, lam)
        # back = the one-sided derivative of F at xt towards x
        h = 1e-7
        fd = (Fobj(xt + h * (x - xt)) - Fobj(xt)) / h
        assert back == pytest.approx(fd, abs=1e-5 * (1 + abs(back)))
        if back >= 0:  # convexity: the trial is no worse
            assert Fobj(xt) <= Fobj(x) + 1e-12
            better += 1
        else:
            worse += 1
    assert better > 20 and worse > 20
    # exactly on zero: clipped neither way, xt = 0; the fallback takes only the clipping
    t = M.trial_row(np.array([0.5]), np.array([-0.5]), np.array([1.0]), np.array([2], dtype=np.uint8), 0.1, 1.0)
    assert t["xt"][0] == 0.0 and not t["fallback"] and t["clip_margin"] == math.inf
    x = np.array([1.0, 0.0]); d = np.array([-2.0, -1.0]); pg = np.array([-1.0, -1.0])
    t = M.trial_row(x, d, pg, np.array([2, 2], dtype=np.uint8), 0.1, 1.0)  # the first is clipped; the second moves with pg: dd = +1 + 0 >= 0
    assert t["fallback"] and t["xt"].tolist() == [0.0, 0.0] and t["dd"] == 1.0 and t["stepn"] == 1.0


def test_face_loop_reaches_the_hand_worked_solution():
    # minimise 1/2 d^T B d + pg^T d from x = (1, 0, 0.5) on the orthant of x (second coordinate: free sign, against its pg)
    B = np.array([[2.0, 1.8, 0.0], [1.8, 2.0, 0.0], [0.0, 0.0, 1.0]])
    pg = np.array([3.0, -1.0, 0.1])
    x = np.array([1.0, 0.0, 0.5])
    kind = np.array([2, 2, 2], dtype=np.uint8)
    d0, log0 = M.solve_faces(B, pg, x, kind, 0.05, 0)
    assert np.allclose(d0, np.linalg.solve(B, -pg)) and log0 == []
    assert x[0] + d0[0] < 0  # the unconstrained step crosses zero in the first coordinate
    d1, log1 = M.solve_faces(B, pg, x, kind, 0.05, 2)
    # by hand: d_0 = -1 fixed; 2 d_1 = 1 - 1.8 (-1) -> d_1 = 1.4; d_2 = -0.1
    assert np.allclose(d1, [-1.0, 1.4, -0.1]) and [e["again"] for e in log1] == [True, False] and log1[0]["n"] == 1
    # below the share: the unconstrained solution stays
    d2, log2 = M.solve_faces(B, pg, x, kind, 0.99, 2)
    assert np.allclose(d2, d0) and [e["again"] for e in log2] == [False]
    # the result is the minimiser over the face: every feasible perturbation raises the model
    q = lambda d: 0.5 * d @ B @ d + pg @ d
    rng = np.random.default_rng(3)
    for _ in range(200):
        e = d1 + rng.normal(size=3) * 0.05
        e[0] = max(e[0], -1.0)
        assert q(e) >= q(d1) - 1e-12


@pytest.mark.parametrize("s2", [0.0, 1.0])
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_pcg_reaches_the_direct_solve_also_after_faces(s2, dtype):
    rng = np.random.default_rng(4)
    Qp, T, s1 = 90, 16, 0.4
    Xs = rng.choice([-1.0, 1.0], size=(600, Qp))
    g = rng.normal(size=Qp) * 0.05
    Hd = ((Xs * rng.random(600)[:, None]).T @ Xs / 600 + s2 * np.outer(g, g)) / s1
    kind = np.full(Qp, 2, dtype=np.uint8)
    kind[0], kind[5:8] = 1, 0
    x = np.where(rng.random(Qp) < 0.5, rng.normal(size=Qp) * 0.05, 0.0)
    pg = np.where(rng.random(Qp) < 0.9, rng.normal(size=Qp), 0.0) * (kind != 0)
    cg = M.Pcg(Hd, s1, s2, x, pg, g, kind, T, dtype)
    W = cg.W
    assert (np.diff(W) > 0).all() and not np.isin([5, 6, 7], W).any() and all(len(t) == T for t in cg.tiles[:-1])
    for _ in range(60):
        cg.step()
    B = (s1 * Hd - s2 * np.outer(g, g))
    want = np.linalg.solve(B[np.ix_(W, W)], -pg[W])
    assert float(cg.rs / cg.rs0) < 1e-20 and np.abs(cg.d[W].astype(np.float64) - want).max() <= 1e-9 * np.abs(want).max()
    assert (cg.d[np.setdiff1d(np.arange(Qp), W)] == 0).all()
    f = cg.faces()
    assert f["n"] > 0 and 0 < f["mass"] <= f["total"] * (1 + 1e-12) + f["mass"]
    fixed = f["cand"]
    assert (cg.d[fixed & (x == 0)] == 0).all() and (cg.d[fixed] == -x[fixed]).all() and not cg.Wm[fixed].any()
    for _ in range(60):
        cg.step()
    fr = np.flatnonzero(cg.Wm)
    fx = np.flatnonzero(fixed)
    want = np.linalg.solve(B[np.ix_(fr, fr)], -pg[fr] - B[np.ix_(fr, fx)] @ cg.d[fx].astype(np.float64))
    assert np.abs(cg.d[fr].astype(np.float64) - want).max() <= 1e-9 * np.abs(want).max()
    assert (cg.d[fx].astype(np.float64) == -x[fx]).all()
