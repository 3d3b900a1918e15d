"""tests/_f64_pass_reference.py, the host model tests/test_gpu_f64_pass_exact.py holds the FP64 pass to, on the CPU: against a
brute-force triple loop on tiny problems; against deliberately wrong results, which it must notice; against a plain float64
evaluation of the same sums in numpy's order, which must stay inside its bounds; and the preconditions of the exact cases in
integer arithmetic."""
import numpy as np
import pytest

import _f64_pass_reference as F
from oracle import oracle as O

LD = np.longdouble
HAVE_LD = np.finfo(LD).nmant >= 63
need_ld = pytest.mark.skipif(not HAVE_LD, reason="np.longdouble is not the 80-bit x87 format here: the model needs 64-bit mantissas")
FORMS = ["RISE", "logRISE", "RPLE"]
GPU_SHAPES = ["S1", "S2", "S3", "S4", "S5"] + F.HIGH

_shapes = {}


def shape(name):
    if name not in _shapes:
        _shapes[name] = F.Shape(name, O.multi_keys)
    return _shapes[name]


def float64_pass(sh, form, TH):
    """the pass in plain float64, numpy's summation orders: V, f, G"""
    A = TH[:, :sh.Qf] @ sh.X + TH[:, [sh.cconst]]
    E = sh.S * A
    if form == "RPLE":
        t = -2.0 * E
        sp = np.where(t > 0, t + np.log1p(np.exp(-np.abs(t))), np.log1p(np.exp(-np.abs(t))))
        e = sh.w * sp
        V = -2.0 * sh.w * (1.0 / (1.0 + np.exp(2.0 * E))) * sh.S
    else:
        e = sh.w * np.exp(-E)
        V = -e * sh.S
    G = np.zeros((sh.R, sh.Qp))
    G[:, :sh.Qf] = V @ sh.X.T
    G[:, sh.cconst] = V.sum(axis=1)
    return V, e.sum(axis=1), G


@need_ld
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["T2", "T3", "T5"])
def test_model_matches_brute_force(name, form):
    """n = 4, K = 11 (pairwise and order 3) and n = 5, K = 13 at order 5 (every subset of the other four spins is a column): the
    internal-layout model and the reference-order sums against a triple loop in
    np.longdouble scalars"""
    sh = shape(name)
    th = np.random.default_rng(5).normal(scale=0.7, size=(sh.R, sh.P))
    TH = sh.internal(th)
    rows = np.arange(sh.R)
    o = F.forward(form, F.energies(sh, TH, rows), sh.S, sh.w, np.zeros(sh.R))
    fm, _ = F.f_of(o, sh.Kp)
    assert not o["V"][:, sh.K:].any() and not o["e"][:, sh.K:].any()  # (w = 0 on the padding)
    V64 = o["V"].astype(np.float64)
    G, _ = F.backward(sh, V64, (1, sh.Kp))
    fp, _, gp, _ = F.public_reference(sh, "RISE" if form == "logRISE" else form, th, rows, (1, sh.Kp))
    for r, u in enumerate(sh.nodes):
        u = int(u)
        keys = F.pair_keys(sh.n, u) if sh.order == 2 else sh.pkeys[u]
        f, g = F.brute(sh.n, sh.spins.tolist(), sh.counts.tolist(), sh.M, u, th[r].tolist(), keys, form)
        tol = LD(2.0) ** -58 * np.abs(o["V"][r]).sum()
        assert abs(fm[r] - f) <= LD(2.0) ** -58 * abs(f) and abs(fp[r] - f) <= LD(2.0) ** -58 * abs(f)
        assert np.abs(gp[r] - g).max() <= tol
        # (the model's G is that of the float64 V it was given: 2^-53 of sum |V| away)
        assert np.abs(G[r, sh.cols(u)] - g).max() <= F.U * np.abs(o["V"][r]).sum() + tol
        other = np.setdiff1d(np.arange(sh.Qp), sh.cols(u))
        assert not G[r, other[other >= sh.Qf]].any()


@need_ld
@pytest.mark.parametrize("form", FORMS)
def test_model_notices_wrong_results(form):
    sh = shape("S3")
    plan = F.bwd_plan(sh.Kp, sh.Qf, sh.Rp // 32)
    assert plan == (2, 2560)
    TH = sh.internal(F.thetas(sh, "dense", form))
    V, f, G = float64_pass(sh, form, TH)
    Gm, Bg = F.backward(sh, V, plan)
    assert F.ratio(G, Gm, Bg) <= 1.0
    bad = G.copy()
    bad[:, sh.cconst] = 0.0
    assert F.ratio(bad, Gm, Bg) > 1e6, "a dropped constant column"
    bad = G.copy()
    bad[:, :sh.Qf] = np.roll(G[:, :sh.Qf], 1, axis=1)
    assert F.ratio(bad, Gm, Bg) > 1e6, "a shifted column"
    bad = G.copy()
    bad[:, sh.Qf] = G[:, sh.Qf - 1]
    assert F.ratio(bad, Gm, Bg) == float("inf"), "a column beyond Qf written"
    Vc = np.zeros_like(V)
    Vc[:, plan[1]:] = V[:, plan[1]:]
    G2, _ = F.backward(sh, Vc, plan)
    assert F.ratio(G + G2.astype(np.float64), Gm, Bg) > 1e6, "a chunk counted twice"
    bad = G.copy()
    bad[:, sh.cconst] -= G2[:, sh.cconst].astype(np.float64)
    assert F.ratio(bad, Gm, Bg) > 1e6, "the row sums of the first chunk only"
    # V: one flipped spin, one sample with a value on the padding, the rows no pass lists
    o = F.forward(form, F.energies(sh, TH, np.arange(sh.R)), sh.S, sh.w, F.bound_E(TH, sh.Qf, sh.cconst))
    assert F.ratio(V, o["V"], o["bV"]) <= 1.0
    bad = V.copy()
    k = int(np.flatnonzero(sh.w > 0)[5])
    bad[3, k] = -bad[3, k]
    assert F.ratio(bad, o["V"], o["bV"]) > 1e6, "a flipped spin"
    bad = V.copy()
    bad[3, sh.K] = 1e-300
    assert F.ratio(bad, o["V"], o["bV"]) == float("inf"), "a padding sample with a value"
    bad = V * (1.0 + 2.0 ** -40)
    assert F.ratio(bad, o["V"], o["bV"]) > 1.0, "exp in a shorter format"
    before = np.random.default_rng(1).normal(size=(sh.Rp, sh.Kp))
    after = before.copy()
    after[:sh.R] = V
    assert F.check_untouched(after, before, sh.R)
    after[sh.R:] = -after[sh.R:]
    assert not F.check_untouched(after, before, sh.R), "a flipped sign on the padded rows"
    after[sh.R:] = 0.0
    assert not F.check_untouched(after, before, sh.R), "padded rows zeroed"


@need_ld
@pytest.mark.parametrize("fam", ["dyadic", "dense", "sparse", "big"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["S1", "S2", "S5"] + F.HIGH)
def test_float64_evaluation_stays_inside_the_bounds(name, form, fam):
    """numpy's float64 evaluation is one of the orders the bounds allow (its exp and log1p are within 1 ulp): V, f, G, the products
    and the reference-order sums.  H7 (P = 1486) is kept out of ONE sub-assertion, the sensitivity of logRISE's finish: the bound of
    gv = g . p grows with P, and a rank-one term off by 1e-9 is 0.26 of it there; every other shape keeps that assertion."""
    sh = shape(name)
    th = F.thetas(sh, fam, form)
    TH = sh.internal(th)
    rows = np.arange(sh.R)
    plan = F.bwd_plan(sh.Kp, sh.Qf, sh.Rp // 32)
    V, f, G = float64_pass(sh, form, TH)
    BE = np.zeros(sh.R, dtype=LD) if fam == "dyadic" else F.bound_E(TH, sh.Qf, sh.cconst)
    o = F.forward(form, F.energies(sh, TH, rows), sh.S, sh.w, BE)
    fm, bf = F.f_of(o, sh.Kp)
    Gm, Bg = F.backward(sh, V, plan)
    r = [F.ratio(V, o["V"], o["bV"]), F.ratio(f, fm, bf), F.ratio(G, Gm, Bg)]
    PD = sh.internal(np.random.default_rng(2).normal(scale=0.5, size=(sh.R, sh.P)))
    Ap = PD[:, :sh.Qf] @ sh.X + PD[:, [sh.cconst]]
    hp = -V * sh.S
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.where(sh.w > 0, 2.0 * hp * (1.0 - hp / (2.0 * sh.w)), 0.0) if form == "RPLE" else hp
    Vm, bV = F.product(form, V, F.energies(sh, PD, rows), sh.S, sh.w, F.bound_E(PD, sh.Qf, sh.cconst))
    r.append(F.ratio(h * Ap, Vm, bV))
    if form != "logRISE":
        fr, bfr, gr, bgr = F.public_reference(sh, form, th, rows, plan)
        g = np.stack([G[i, sh.cols(u)] for i, u in enumerate(sh.nodes)])
        r += [F.ratio(f, fr, bfr), F.ratio(g, gr, bgr)]
    else:
        fr, bfr, gr, bgr = F.public_reference(sh, form, th, rows, plan)
        g = np.stack([G[i, sh.cols(u)] for i, u in enumerate(sh.nodes)]) / f[:, None]
        r += [F.ratio(np.log(f), fr, bfr), F.ratio(g, gr, bgr)]
        # the public product of logRISE in float64: Hess Z p / Z - g (g . p), as the host finish forms it
        pd = np.random.default_rng(2).normal(scale=0.5, size=(sh.R, sh.P))
        G2 = np.zeros((sh.R, sh.Qp))
        G2[:, :sh.Qf] = (h * Ap) @ sh.X.T
        G2[:, sh.cconst] = (h * Ap).sum(axis=1)
        H = np.stack([G2[i, sh.cols(u)] for i, u in enumerate(sh.nodes)])
        hv = H / f[:, None] - g * (g * pd).sum(axis=1, keepdims=True)
        want, bound = F.public_hessvec_logrise(sh, th, pd, rows, plan)
        r.append(F.ratio(hv, want, bound))
        wrong = H / f[:, None] - g * (g * pd).sum(axis=1, keepdims=True) * (1 + 1e-9)
        if name != "H7":
            assert F.ratio(wrong, want, bound) > 1.0, "a finish off by 1e-9 of its rank-one term is noticed"
    print(f"{name} {form} {fam}: float64 / bound  V {r[0]:.3f}  f {r[1]:.3f}  G {r[2]:.3f}  product V {r[3]:.3f}  public f {r[4]:.3f}  g {r[5]:.3f}")
    assert max(r) <= 1.0, r


def test_bwd_plan_of_the_shapes():
    """what each shape is there to reach (launch_bwd_f64's arithmetic, restated)"""
    got = {n: F.bwd_plan(shape(n).Kp, shape(n).Qf, shape(n).Rp // 32) for n in GPU_SHAPES}
    assert got == {"S1": (1, 1024), "S2": (1, 1024), "S3": (2, 2560), "S4": (1, 2048), "S5": (3, 2432), "H5": (1, 2048), "H6": (1, 2048),
                   "H7": (1, 1024), "H8": (1, 3072), "E7": (1, 1024), "E3": (1, 1024)}, got
    s2, s4, s5 = shape("S2"), shape("S4"), shape("S5")
    assert (s2.R, s2.Rp, s2.Qfp // 64) == (45, 64, 2) and len(set(s2.nodes.tolist())) < s2.R
    assert s4.Qf > 1024 and (s4.Qf + 1023) // 1024 == 2 and s4.Qfp // 64 == 19
    assert s5.Kp - 2 * 2432 == 2304
    # orders 5 to 8: statistics columns, padded columns, parameters per node (the sizes each shape is there for)
    got = {n: (shape(n).Qf, shape(n).Qfp, shape(n).P) for n in F.HIGH}
    assert got == {"H5": (561, 576, 386), "H6": (637, 640, 382), "H7": (2509, 2560, 1486), "H8": (501, 512, 255), "E7": (127, 128, 64),
                   "E3": (7, 64, 4)}, got
    h7 = shape("H7")
    assert (h7.Qf + 1023) // 1024 == 3 and h7.Qfp // 64 == 40 and h7.P > 512 and shape("E7").Qf == 2 ** 7 - 1


@pytest.mark.parametrize("name", ["S4", "T3", "S1", "T2"])
def test_key_lookup_gives_the_closed_form_columns(name):
    """Shape.column looks a parameter's other spins up in stat_keys; at orders 2 and 3 that is the closed form it replaced: the spin
    itself, n + a n - a (a + 1) / 2 + (b - a - 1) for a pair a < b, the constant column for the field"""
    sh = shape(name)
    for u in sorted(set(sh.nodes.tolist())):
        keys = F.pair_keys(sh.n, u) if sh.order == 2 else sh.pkeys[u]
        want = [F.closed_form_column(sh.n, sorted(i for i in k if i != u), sh.cconst) for k in keys]
        assert sh.cols(u).tolist() == want, (name, u)
        assert [sh.colidx[tuple(sorted(i for i in k if i != u))] if len(k) > 1 else sh.cconst for k in keys] == want


@pytest.mark.parametrize("name", F.HIGH + ["T5"])
def test_columns_of_the_high_orders(name):
    """every parameter of a node is one distinct column: the constant column once, and each subset of the other spins up to
    order - 1 of them exactly once, at the index itertools.combinations gives it (by size, then lexicographically)"""
    import itertools
    sh = shape(name)
    subsets = [c for q in range(1, sh.order) for c in itertools.combinations(range(sh.n), q)]
    assert [tuple(int(i) for i in k if i >= 0) for k in sh.keys] == subsets and sh.keys.shape[1] == sh.order - 1
    for u in sorted(set(sh.nodes.tolist())):
        cols = sh.cols(u)
        assert len(set(cols.tolist())) == sh.P and (cols == sh.cconst).sum() == 1
        want = sorted(c for c, k in enumerate(subsets) if u not in k)
        assert sorted(c for c in cols.tolist() if c != sh.cconst) == want


@pytest.mark.parametrize("name", GPU_SHAPES)
def test_exact_cases_fit_53_bits(name):
    """every partial sum of every exact case, in Python integers"""
    sh = shape(name)
    worst = F.exact_preconditions(sh, F.direction(sh), F.thetas(sh, "dyadic", "RISE"))
    print(f"{name}: largest partial sum of an exact case 2^{np.log2(max(worst, 1)):.1f}")
    assert worst < 2 ** 53
    assert all(float(c) == int(c) and c < 2 ** 20 for c in sh.counts) and sh.counts.max() / max(1.0, sh.counts[sh.counts > 0].min()) >= 100


@need_ld
@pytest.mark.parametrize("value", [-7.5, -10.5])
@pytest.mark.parametrize("form", ["RISE", "logRISE"])
def test_padding_case_preconditions(form, value):
    """the far row's padding energy, the finite reference, and no real sample at the padding's energy"""
    sh = shape("S2")
    th, far = F.padding_case(sh, value)
    assert sh.Kp - sh.K == 324 and float(th[far].sum()) == 70 * value
    assert (70 * value < -709.8) == (value == -10.5)  # (-7.5, the value first proposed for this case, stays finite: exp(525))
    assert not (sh.spins == 1).all(axis=1).any()
    fr, bf, gr, bg = F.public_reference(sh, form, th, np.array([far, 0]), F.bwd_plan(sh.Kp, sh.Qf, sh.Rp // 32))
    for a in (fr, bf, gr, bg):
        assert np.isfinite(a.astype(np.float64)).all()
