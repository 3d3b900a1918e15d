"""The FP64 pass (k_fwd_f64, k_bwd_f64: csrc/gml_kernels_f64gemm.hip) cut at V and held on both sides to the host model
tests/_f64_pass_reference.py (itself held to brute force by tests/test_host_f64_pass_reference.py).  Passes run through
gml_test_i8_pass at GML_PREC_F64 (one objective pass, optionally one product pass, no log finish); V comes back through the copy-only
hook gml_test_f64_v, the internal-layout rows of Theta through gml_test_i8_pack_state, the internal-layout G and f through
gml_test_i8_gacc.

Shapes (tests/_f64_pass_reference.py: SHAPES; counts are integers over three decades whose total M is a power of two, so w_k is dyadic):
  S1  n = 5,   order 2, K = 37   (Kp 1024), all 5 rows:   one group, one column step, almost all padding
  S2  n = 70,  order 2, K = 700  (Kp 1024), 45 rows, shuffled with repeats: two column steps, a partial second group with inactive rows
  S3  n = 100, order 2, K = 4500 (Kp 5120), all rows:     split-K, two chunks of 2560 samples (equal at this Kp), a barrier inside each
  S4  n = 48,  order 3, K = 1100 (Kp 2048), 40 rows:      Qf = 1176 statistics columns: two backward column blocks, six waves of the
                                                          second leave at once beside two that reach the barriers; 19 forward column steps
  S5  n = 40,  order 2, K = 6200 (Kp 7168), all rows:     split-K with UNEQUAL chunks (2432, 2432, 2304): the smallest Kp that has them
Orders 5 to 8, all rows, iid spins (keys of four to seven spins besides the node's own: stat_word's XOR of up to seven rows of Sb, the
column walk of gml_node_cols up to q = 7):
  H5  n = 11, order 5, K = 1500 (Kp 2048): Qf = 561 -> 576 (15 padding columns, 9 column steps), P = 386
  H6  n = 10, order 6, K = 1100 (Kp 2048): Qf = 637 -> 640 (3 padding columns), P = 382
  H7  n = 12, order 7, K = 700  (Kp 1024): Qf = 2509 -> 2560 (40 column steps, a third 1024-column block in k_bwd_f64), P = 1486
  H8  n = 9,  order 8, K = 2100 (Kp 3072): Qf = 501 -> 512, P = 255: the largest order
  E7  n = 7,  order 8, K = 300:  order = n + 1: every non-empty subset is a column (127 -> 128), P = 64
  E3  n = 3,  order 8, K = 40:   order far above n: seven key slots, at most three used; Qf = 7 -> 64, P = 4
The long-double comparisons and the exact tests cover every row of every shape (S4's 40 rows in long double take about a second
per case on the host).

Exact (np.array_equal, no element excluded): theta = 0 (V = -w s, 0 on the padding; f = 1; G the integer sums); products at
theta = 0 with a dense dyadic direction through the hook in all three forms and through the public hessvec (RISE, RPLE): the new V and
every entry of G -- the constant column, the zeros beyond Qf -- are the integer model X^T diag(w) X p.
Bounds (every element; the derivations are in the model's docstring; each prints measured / bound): V, f, G given the device's V,
the products given the device's V_old, for RISE, logRISE (Z) and RPLE on the families dyadic (E exact: this measures EXP_ULPS), dense,
sparse, big; objgrad at f64 in the reference's parameter order against the spins and O.multi_keys; logRISE's public hessvec at f64,
whose finish Hess Z p / Z - g (g . p) is no integer sum, against the same long-double sums; and the padding case.

Figures of the run on an MI355X are in HISTORY.md."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _f64_pass_reference as F
import gml_amd as gml
from oracle import oracle as O
from test_gpu_i8_pack_state import State
from test_gpu_i8_pass_variants import i8_pass, need_ld

_lib = importlib.import_module("gml_amd._lib")
LD = np.longdouble
U = F.U
NAMES = ["S1", "S2", "S3", "S4", "S5"] + F.HIGH
FORMS = ["RISE", "logRISE", "RPLE"]
FAMILIES = ["dyadic", "dense", "sparse", "big"]

_shapes, _handles = {}, {}


def shape(name):
    if name not in _shapes:
        _shapes[name] = F.Shape(name, O.multi_keys)
    return _shapes[name]


@pytest.fixture(scope="module")
def handles():
    yield _handles
    for p in _handles.values():
        p.close()
    _handles.clear()


def handle(handles, name):
    if name not in handles:
        sh = shape(name)
        handles[name] = gml.Problem(spins=sh.spins, counts=sh.counts, order=sh.order)
    return handles[name]


def _hooks():
    L = _lib.lib()
    v = C.c_void_p
    L.gml_test_f64_v.argtypes = [v, v, v]
    L.gml_test_i8_gacc.argtypes = [v, v, v, v, v]
    return L


def read_v(p):
    L = _hooks()
    d = np.zeros(3, dtype=np.int64)
    _lib.check(L.gml_test_f64_v(p._h, _lib._ptr(d), None))
    V = np.zeros((int(d[0]), int(d[1])))
    if V.size:
        _lib.check(L.gml_test_f64_v(p._h, _lib._ptr(d), _lib._ptr(V)))
    return V, int(d[1]), int(d[2])


def read_gf(p):
    L = _hooks()
    d = np.zeros(8, dtype=np.int64)
    _lib.check(L.gml_test_i8_gacc(p._h, _lib._ptr(d), None, None, None))
    G, f = np.zeros((int(d[5]), int(d[6]))), np.zeros(int(d[5]))
    _lib.check(L.gml_test_i8_gacc(p._h, _lib._ptr(d), None, _lib._ptr(G), _lib._ptr(f)))
    return G, f


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


def run_pass(p, sh, form, th, vec=None):
    """one objective pass, or (vec) one objective and one product pass; what they left, with the checks every pass gets: the
    sizes, the rows Theta holds, V of the rows no pass lists, the padding samples, and the hook's own f and g against the workspace"""
    Vb, _, _ = read_v(p)
    out = i8_pass(p, form, "f64", sh.nodes, th, vec=vec, hv=1 if vec is not None else 0)
    V, Kp, K = read_v(p)
    G, f = read_gf(p)
    st = State(p)
    assert (Kp, K, st.Qf, st.Qfp, st.cconst, st.Qp) == (sh.Kp, sh.K, sh.Qf, sh.Qfp, sh.cconst, sh.Qp)
    assert len(V) >= sh.Rp and len(V) % 32 == 0 and len(G) >= sh.Rp
    assert np.array_equal(st.theta[:sh.R], sh.internal(th if vec is None else vec)), "the rows the pass read"
    if Vb.shape != V.shape:  # (the first pass of a handle sized V, zeroed)
        Vb = np.zeros_like(V)
    assert F.check_untouched(V, Vb, sh.R), "V of rows no pass listed was written"
    assert not V[:sh.R, sh.K:].any(), "a padding sample has a V"
    cols = [sh.cols(u) for u in sh.nodes]
    if vec is None:
        assert _bits(out["f"], f[:sh.R]), "f as returned"
        assert all(_bits(out["g"][r], G[r, cols[r]]) for r in range(sh.R)), "g as returned"
    else:
        assert all(_bits(out["hv"][r], G[r, cols[r]]) for r in range(sh.R)), "hv as returned"
    return dict(V=V, G=G, f=f, theta=st.theta[:sh.R].copy(), out=out)


def plan_of(sh, active_groups=None):
    """(nsplit, kchunk) of the backward launch.  launch_bwd_f64 takes the number of ACTIVE row groups; every pass of this file lists
    all R rows, so every group up to Rp / 32 is active (the one exception, `auto` in the padding case, asserts its own count)"""
    full = sh.Rp // 32
    assert full == (sh.R + 31) // 32 and (active_groups is None or 1 <= active_groups <= full)
    return F.bwd_plan(sh.Kp, sh.Qf, full if active_groups is None else active_groups)


def check_backward(tag, sh, res):
    rows = sh.ld_rows
    Gm, Bg = F.backward(sh, res["V"][rows], plan_of(sh))
    rg = F.ratio(res["G"][rows], Gm, Bg)
    sel = np.zeros(sh.Qp, dtype=bool)
    sel[sh.cconst] = True
    rc = F.ratio(res["G"][rows][:, sel], Gm[:, sel], Bg[:, sel])
    return rg, rc


# ---------------------------------------------------------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_theta_zero_is_exact(handles, name, form):
    """V = -w s bit for bit on the real samples (exp(0) = 1; RPLE: -2 w / (1 + 1) s) and 0 on the padding; f of the exp forms is
    sum w = 1; G is the integer sum -X^T (w s) over M"""
    sh, p = shape(name), handle(handles, name)
    res = run_pass(p, sh, form, np.zeros((sh.R, sh.P)))
    V = -sh.w[None, :] * sh.S
    assert np.array_equal(res["V"][:sh.R], V), np.argwhere(res["V"][:sh.R] != V)[:4].tolist()
    G = np.zeros((sh.R, sh.Qp))
    G[:, :sh.Qf] = V @ sh.X.T
    G[:, sh.cconst] = V.sum(axis=1)
    assert np.array_equal(res["G"][:sh.R], G), np.argwhere(res["G"][:sh.R] != G)[:4].tolist()
    if form != "RPLE":
        assert np.array_equal(res["f"][:sh.R], np.ones(sh.R))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_products_at_theta_zero_are_exact(handles, name, form):
    """h = w exactly at theta = 0 in every form, so with a direction in multiples of 2^-6 the new V and every entry of G are sums
    of integers over 64 M (tests/test_host_f64_pass_reference.py: below 2^53 in any order): every bit-to-column mapping of both
    kernels, the chunking and the row-sum path, with no tolerance"""
    sh, p = shape(name), handle(handles, name)
    pd = F.direction(sh)
    Vm, Gm = F.exact_product(sh, sh.internal(pd))
    res = run_pass(p, sh, form, np.zeros((sh.R, sh.P)), vec=pd)
    assert np.array_equal(res["V"][:sh.R], Vm), np.argwhere(res["V"][:sh.R] != Vm)[:4].tolist()
    assert np.array_equal(res["G"][:sh.R], Gm), np.argwhere(res["G"][:sh.R] != Gm)[:4].tolist()
    if form != "logRISE":  # (logRISE's public product has a finish: Hess Z v / Z - g (g . v))
        hv = p.hessvec(form, sh.nodes, np.zeros((sh.R, sh.P)), pd, precision="f64")
        want = np.stack([Gm[r, sh.cols(u)] for r, u in enumerate(sh.nodes)])
        assert np.array_equal(hv, want), np.argwhere(hv != want)[:4].tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# bounds, in the internal layout
# ---------------------------------------------------------------------------------------------------------------------------
@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_pass_within_the_model_bounds(handles, name, form, fam):
    sh, p = shape(name), handle(handles, name)
    th = F.thetas(sh, fam, form)
    rows = sh.ld_rows
    res = run_pass(p, sh, form, th)
    TH = res["theta"]
    BE = np.zeros(sh.R, dtype=LD) if fam == "dyadic" else F.bound_E(TH, sh.Qf, sh.cconst)  # (dyadic: every partial sum is exact)
    o = F.forward(form, F.energies(sh, TH, rows), sh.S[rows], sh.w, BE[rows])
    rv = F.ratio(res["V"][rows], o["V"], o["bV"])
    fm, bf = F.f_of(o, sh.Kp)
    rf = F.ratio(res["f"][rows], fm, bf)
    rg, rc = check_backward((name, form, fam), sh, res)
    msg = f"{name} {form} {fam}: measured / bound  V {rv:.3f}  f {rf:.3f}  G {rg:.3f}  G const {rc:.3f}  (max |E| {float(np.abs(o['E']).max()):.1f})"
    if fam == "dyadic":
        nz = o["V"] != 0
        ulps = float((np.abs(res["V"][rows].astype(LD) - o["V"])[nz] / (U * np.abs(o["V"][nz]))).max())
        msg += f"  |V_dev - V| / (u |V|) = {ulps:.3f}" + (f": exp alone {ulps - 1:.3f}" if form != "RPLE" else "")
        if form != "RPLE":  # (E exact: exp and one product; the model's constant is twice the worst seen, at least 2, and never above 4)
            assert 2.0 * (ulps - 1.0) <= 4.0, ("the device's exp is off by more than a constant may absorb: a finding", msg)
            assert F.EXP_ULPS >= max(2.0, 2.0 * (ulps - 1.0)), msg
    if form == "RPLE":
        t = -2 * o["E"][:, :sh.K]
        msg += f"  softplus branches t > 0: {int((t > 0).sum())}, t <= 0: {int((t <= 0).sum())}"
        if fam == "sparse":
            assert (t > 0).any() and (t <= 0).any() and float(np.abs(o["E"]).max()) >= 39.0
    # the products: forms 4 to 6 on the V this pass left
    pd = F.direction(sh) if fam == "dyadic" else np.random.default_rng(sh.P + 3).normal(scale=0.5, size=(sh.R, sh.P))
    res2 = run_pass(p, sh, form, th, vec=pd)
    PD = res2["theta"]
    BA = np.zeros(sh.R, dtype=LD) if fam == "dyadic" else F.bound_E(PD, sh.Qf, sh.cconst)
    Vm, bV = F.product(form, res["V"][rows], F.energies(sh, PD, rows), sh.S[rows], sh.w, BA[rows])
    rpv = F.ratio(res2["V"][rows], Vm, bV)
    rpg, rpc = check_backward((name, form, fam, "product"), sh, res2)
    print(msg + f"  product V {rpv:.3f}  product G {rpg:.3f}  product G const {rpc:.3f}")
    assert max(rv, rf, rg, rc, rpv, rpg, rpc) <= 1.0, msg


# ---------------------------------------------------------------------------------------------------------------------------
# the public path
# ---------------------------------------------------------------------------------------------------------------------------
def check_public(tag, sh, form, th, f, g, rows):
    fr, bf, gr, bg = F.public_reference(sh, form, th, rows, plan_of(sh))
    rf, rg = F.ratio(f[rows], fr, bf), F.ratio(g[rows], gr, bg)
    print(f"{tag}: measured / bound  f {rf:.3f}  g {rg:.3f}")
    return max(rf, rg)


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["dense", "sparse"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_objgrad_f64_in_reference_order(handles, name, form, fam):
    """the layout and the host finish as well: long-double sums over statistics built from the spins and O.multi_keys"""
    sh, p = shape(name), handle(handles, name)
    th = F.thetas(sh, fam, form)
    f, g = p.objgrad(form, sh.nodes, th, precision="f64")
    assert check_public(f"{name} {form} {fam} objgrad f64", sh, form, th, f, g, sh.ld_rows) <= 1.0


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["dyadic", "dense"])
@pytest.mark.parametrize("name", NAMES)
def test_hessvec_logrise_f64_in_reference_order(handles, name, fam):
    """logRISE's public product has a host finish (Hess Z p / Z - g (g . p)) that the exact tests cannot reach: both passes, the
    layout and the finish against long-double sums in the reference's order"""
    sh, p = shape(name), handle(handles, name)
    th = F.thetas(sh, fam, "logRISE")
    pd = F.direction(sh) if fam == "dyadic" else np.random.default_rng(sh.P + 3).normal(scale=0.5, size=(sh.R, sh.P))
    hv = p.hessvec("logRISE", sh.nodes, th, pd, precision="f64")
    want, bound = F.public_hessvec_logrise(sh, th, pd, sh.ld_rows, plan_of(sh), exact_E=fam == "dyadic")
    r = F.ratio(hv[sh.ld_rows], want, bound)
    print(f"{name} logRISE {fam} hessvec f64: measured / bound {r:.3f}")
    assert r <= 1.0, r


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("value", [-7.5, -10.5])
@pytest.mark.parametrize("form", ["RISE", "logRISE"])
def test_padding_samples_of_a_far_row(handles, form, value):
    """S2 (324 padding samples) with every entry of one row at `value`: the padding samples, whose statistics are all +1, have
    E = 70 value.  At -7.5 that is -525; at -10.5 it is -735, below -709.8 where exp(-E) overflows and w exp(-E) = 0 * inf.  The real
    samples have moderate energies: the reference is finite, and so must f and g be, at f64 and where `auto` sends such a row."""
    sh, p = shape("S2"), handle(handles, "S2")
    th, far = F.padding_case(sh, value)
    assert not (sh.spins == 1).all(axis=1).any()  # (no real sample shares the padding's energy)
    fr, bf, gr, bg = F.public_reference(sh, form, th, np.arange(sh.R), plan_of(sh))
    assert np.isfinite(fr.astype(np.float64)).all() and np.isfinite(gr.astype(np.float64)).all() and np.isfinite(bg.astype(np.float64)).all()
    # (auto hands the FP64 kernels the far row alone: one active group.  At Kp = 1024 the plan is the same for any number of groups)
    assert plan_of(sh, 1) == plan_of(sh) == (1, 1024)
    for prec in ("f64", "auto"):
        f, g = p.objgrad(form, sh.nodes, th, precision=prec)
        assert np.isfinite(f).all() and np.isfinite(g).all(), (prec, "rows with a non-finite f or g", np.flatnonzero(~np.isfinite(f)).tolist())
        # (auto sends the far row to the FP64 path and runs the others on the FP64-grade int8 limbs: all of them are held to these bounds)
        rf, rg = F.ratio(f, fr, bf), F.ratio(g, gr, bg)
        rows = np.array([far])
        print(f"S2 {form} padding case {value} {prec}: measured / bound  f {rf:.3f}  g {rg:.3f};  the far row alone  f {F.ratio(f[rows], fr[rows], bf[rows]):.3f}"
              f"  g {F.ratio(g[rows], gr[rows], bg[rows]):.3f}  (its f {f[far]:.3e})")
        assert max(rf, rg) <= 1.0, (prec, rf, rg)
