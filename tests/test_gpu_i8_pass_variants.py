"""Every form of the int8-limb pass (csrc/gml_i8_pass.hip) against an independent extended-precision statement of the same sums.

The public operator runs one form only (lf = 5, never coarse, full products).  The solver also runs reduced-limb, coarse,
objective-only and sub-sampled forms; here each of them runs once through the test hook gml_test_i8_pass (one objective pass,
optionally one Hessian-vector pass after it, no rescaled re-runs) and is compared with a plain numpy reference.

Reference.  Statistics x_k (products of +-1 spins, the reference's key order), weights w_k = c_k / M, energies E_k = x_k . theta.
f, the gradient and sum_k h_k (x_k . p) x_k are formed in np.longdouble (80-bit).  The +-1 GEMMs are exact: the real operand is cut
into 26-bit pieces whose float64 GEMMs with x are integer sums below 2^53.
  RISE / logRISE (raw: Z and grad Z):  f = sum w e^-E,  g = -sum w e^-E x,  h = w e^-E
  RPLE:  f = sum w log(1 + e^-2E),  g = -sum 2 w sig x,  h = 4 w sig (1 - sig),  sig = 1 / (1 + e^2E)
Products over ksub > 1 cover the configurations k with k mod kchunk < kpart.  The finalise step applies no weight to them.

Bounds (err is |device - reference| for f and for every gradient entry):
  * f64, and i8w on well-scaled rows: FTOL = 1e-12 relative to f.  i8w on the dense row (sum |theta| = 60): I8W_DYN_TOL = 3e-10.
  * every other form: 1e-13 |f| + 3.3 sqrt(K) tau unit + e + q.  The first three terms are the solver's noise model (gml_solver.cpp,
    "noise"): each V_k is rounded to a multiple of unit * tau with a dither, so the K errors add like a random walk.  unit = 1, or
    i8_coarse_unit (2^8 i8x, 2^24 i8w) for coarse passes.  e = EXP_ERR |f| for the i8x exp forms: their FP32 expm1 (vq_exp) has
    three roundings of ~2^-24 |r| each, |r| <= ln2/128, so exp is off by up to 3 * 2^-24 * ln2/128 / (1 - ln2/128) = 9.74e-10 of
    |V_k| (7.7e-10 seen in a CPU emulation of the instruction sequence) -- one error for all samples of an energy, so it adds up
    with f.  The clustered-energy test below puts a row at that worst case.  q bounds the quantisation of theta (k_quant_theta: sigma = 2^(ex - 8 LF + 2)
    per row; coarse i8w keeps the top four of seven planes, so the three dropped balanced digits add up to 128 * 65793 sigma per
    column).  With d = sum_c |theta_c - theta_q,c|: q = (e^d - 1) |f| for the exp forms and q = 2 d for RPLE (|dV/dE| <= w, sum w = 1).
  * products: 1e-13 |f| + 3.3 sqrt(Kpart) tau_hv + 3.3 sqrt(Kpart) c_h tau_V |p|_1 + d_p sum h.  tau_hv is the unit of the rounded
    products (hv = 1: 31 bits of tau_V |p|_1; hv = 2: 15 bits).  The third term is the dithered rounding of the curvature weights
    (c_h = 1 for the exp forms, 2 for RPLE, whose h is 2 a (1 - a / 2w) of a = |V|).  The last term is the quantisation of the
    direction at the product pass's lf.
  * range: max_k |V_k| <= (mmax + 1) i8_mmax_unit tau for every slot of every exp-form pass, V_k of the quantised theta: the reference
    at theta is allowed the factor e^d (1 + EXP_ERR) (this found the coarse i8w bound short by up to half a unit).  RPLE keeps no mmax, so there
    |V| <= 2 w_max = tau i8_vdiv.  The products have no mmax either: max_k |u_k| / tau_hv is held to the width of their planes.
Each case prints measured / bound.  Bounds are never loosened to make a case pass."""
import ctypes as C
import importlib

import numpy as np
import pytest

import gml_amd as gml
from conftest import load_csv
from oracle import oracle as O

_lib = importlib.import_module("gml_amd._lib")
LD = np.longdouble
HAVE_LD = np.finfo(LD).nmant >= 63
need_ld = pytest.mark.skipif(not HAVE_LD, reason="np.longdouble is not the 80-bit x87 format here: the reference needs 64-bit mantissas")

FORMS = ["RISE", "logRISE", "RPLE"]
FTOL = 1e-12
EXP_ERR = 1e-9  # relative error of exp(-E) in the i8x exp forms (vq_exp; gml_solver.cpp "noise" uses the same)
I8W_DYN_TOL = 3e-10
COARSE_UNIT = {False: 256.0, True: 16777216.0}  # i8_coarse_unit
MMAX_UNIT = {False: 1.0, True: 65536.0}          # i8_mmax_unit
VDIV = {False: 2130000000.0, True: 1.400e14}     # i8_vdiv


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
def _xdot(X, A):
    """X (+-1 float64 [k, m]) @ A (longdouble [m, F]) to ~2^-78 of max |A| per column: A cut into 26-bit pieces, each GEMM exact."""
    A = np.asarray(A, dtype=LD)
    mx = np.abs(A).max(axis=0)
    s = np.where(mx > 0, np.ldexp(LD(1), np.frexp(np.where(mx > 0, mx, 1).astype(np.float64))[1]), LD(1)).astype(LD)
    y = A / s
    out = np.zeros((X.shape[0], A.shape[1]), dtype=LD)
    for sh in (26, 52, 78):
        piece = np.round(y * LD(2.0) ** sh) / LD(2.0) ** sh
        out += (X @ piece.astype(np.float64)).astype(LD)
        y = y - piece
    return out * s


class Ref:
    """The statistics of one problem (spins and counts as the handle holds them) and the sums of the passes over them."""

    def __init__(self, spins, counts, order=2, keys=None):
        self.S = np.ascontiguousarray(spins, dtype=np.int8)
        self.K, self.n = self.S.shape
        c = np.ones(self.K) if counts is None else np.asarray(counts, dtype=np.float64)
        self.w = c.astype(LD) / c.astype(LD).sum()
        self.order, self.keys = order, keys  # keys(u): int32 [P, order], -1 = unused slot (order > 2)
        self.P = self.n if order == 2 else len(keys(0))
        self.chunk = max(256, (1 << 26) // (8 * self.P))  # host memory of one chunk of statistics: <= 64 MB (x a few temporaries)

    def stats(self, u, k0, k1):
        S = self.S[k0:k1]
        if self.order == 2:
            X = S.astype(np.float64) * S[:, [u]]
            X[:, u] = S[:, u]
            return X
        kk = self.keys(u)
        X = np.ones((k1 - k0, len(kk)))
        for j in range(kk.shape[1]):
            col = kk[:, j]
            X[:, col >= 0] *= S[:, col[col >= 0]]
        return X

    def run(self, nodes, jobs):
        """jobs: list of dicts {form, theta [R, P], vec [R, P] or None, keep: list of (kchunk, kpart) or []}.  Returns per job
        f [R], g [R, P], vmax [R] (largest |V|), and hv / hsum per keep entry (products and sum of the curvature weights)."""
        R, P = len(nodes), self.P
        out = [dict(f=np.zeros(R, LD), g=np.zeros((R, P), LD), vmax=np.zeros(R, LD),
                    hv=[np.zeros((R, P), LD) for _ in j["keep"]], hsum=[np.zeros(R, LD) for _ in j["keep"]],
                    umax=[np.zeros(R, LD) for _ in j["keep"]]) for j in jobs]
        for r, u in enumerate(nodes):
            A = np.stack([j["theta"][r] for j in jobs] + [j["vec"][r] for j in jobs if j["keep"]], axis=1)
            for k0 in range(0, self.K, self.chunk):
                k1 = min(self.K, k0 + self.chunk)
                X = self.stats(u, k0, k1)
                EA = _xdot(X, A)
                w = self.w[k0:k1]
                B, where = [], []
                iv = len(jobs)
                for a, j in enumerate(jobs):
                    E = EA[:, a]
                    if j["form"] == "RPLE":
                        E2 = 2 * E
                        sig = 1 / (1 + np.exp(E2))
                        fk = w * np.where(E2 < 0, -E2 + np.log1p(np.exp(E2)), np.log1p(np.exp(-E2)))
                        V = -2 * w * sig
                        h = 4 * w * sig * (1 - sig)
                    else:
                        fk = w * np.exp(-E)
                        V = -fk
                        h = fk
                    o = out[a]
                    o["f"][r] += fk.sum()
                    o["vmax"][r] = max(o["vmax"][r], np.abs(V).max())
                    B.append(V)
                    where.append((a, "g", None))
                    if j["keep"]:
                        t = EA[:, iv]
                        iv += 1
                        kidx = np.arange(k0, k1)
                        for e, (kc, kp) in enumerate(j["keep"]):
                            m = (kidx % kc) < kp
                            uk = np.where(m, h * t, 0)
                            B.append(uk)
                            where.append((a, "hv", e))
                            o["hsum"][e][r] += np.where(m, h, 0).sum()
                            o["umax"][e][r] = max(o["umax"][e][r], np.abs(uk).max())
                G = _xdot(np.ascontiguousarray(X.T), np.stack(B, axis=1))
                for col, (a, kind, e) in enumerate(where):
                    if kind == "g":
                        out[a]["g"][r] += G[:, col]
                    else:
                        out[a]["hv"][e][r] += G[:, col]
        return out


def quant_defect(theta, lf, coarse_wide=False):
    """sum_c |theta_c - its quantised value| per row, as k_quant_theta quantises (lf = 7: the i8w pass)"""
    theta = np.asarray(theta, dtype=np.float64)
    mx = np.abs(theta).max(axis=1)
    ex = np.where(mx > 0, np.frexp(np.where(mx > 0, mx, 1))[1], 0)
    sx = ex - (8 * lf - 2)
    if lf > 5:
        s1 = np.abs(theta).sum(axis=1)
        e1 = np.where(s1 > 0, np.frexp(np.where(s1 > 0, s1 * 1.0000001, 1))[1], 0)
        sx = np.maximum(sx, e1 - 61)
    sg = np.ldexp(1.0, sx)[:, None]
    d = np.abs(theta - np.rint(theta / sg) * sg).sum(axis=1)
    if coarse_wide:  # the three dropped balanced digits of every non-zero column: |.| <= 128 * (1 + 256 + 65536) sigma
        d = d + (theta != 0).sum(axis=1) * 128.0 * 65793.0 * sg[:, 0]
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the reference against the C oracle
# ---------------------------------------------------------------------------------------------------------------------------
@need_ld
@pytest.mark.parametrize("name", ["a", "b", "c", "mvt"])
def test_reference_matches_oracle_on_goldens(name):
    s = load_csv(f"{name}_samples.csv")
    counts, spins = O.split_histogram(s)
    K, n = spins.shape
    rng = np.random.default_rng(len(name))
    nodes = np.arange(n)
    theta = rng.normal(scale=0.4, size=(n, n))
    ref = Ref(spins, counts)
    res = ref.run(nodes, [dict(form=f, theta=theta, vec=None, keep=[]) for f in FORMS])
    for form, o in zip(FORMS, res):
        fo, go = O.objgrad_nodes(form, counts, spins, nodes, theta)
        f = o["f"] if form != "logRISE" else np.log(o["f"])
        g = o["g"] if form != "logRISE" else o["g"] / o["f"][:, None]
        err = max(np.abs(f - fo).max() / np.abs(fo).max(), (np.abs(g - go) / np.abs(fo)[:, None]).max())
        print(f"{name} {form}: reference vs oracle {float(err):.1e}")
        assert err <= 1e-13, (name, form, err)


@need_ld
def test_reference_matches_oracle_order3():
    n, K = 9, 700
    rng = np.random.default_rng(3)
    spins = np.where(rng.random((K, n)) < 0.6, 1, -1).astype(np.int8)
    counts = np.floor(10 ** rng.uniform(0, 3, size=K))
    nodes = np.array([0, 4, 8, 4])
    keys = {u: O.multi_keys(n, 3, u) for u in range(n)}
    P = len(keys[0])

    def karr(u):
        a = np.full((P, 3), -1, dtype=np.int32)
        for i, k in enumerate(keys[u]):
            a[i, :len(k)] = k
        return a

    theta = rng.normal(scale=0.1, size=(len(nodes), P))
    o = Ref(spins, counts, order=3, keys=karr).run(nodes, [dict(form="RISE", theta=theta, vec=None, keep=[])])[0]
    fo, go = O.objgrad_multi3_nodes(counts, spins, nodes, theta)
    err = max(np.abs(o["f"] - fo).max() / np.abs(fo).max(), (np.abs(o["g"] - go) / np.abs(fo)[:, None]).max())
    print(f"order 3 RISE: reference vs oracle {float(err):.1e}")
    assert err <= 1e-13, err


def test_exact_gemm_of_the_reference():
    # the split GEMM is exact where a plain float64 GEMM is not: +-1 times values 2^60 apart
    X = np.array([[1.0, -1.0, 1.0], [1.0, 1.0, -1.0]])
    A = np.array([[LD(2.0) ** 60], [LD(1.0)], [LD(2.0) ** -3]], dtype=LD)
    got = _xdot(X, A)[:, 0]
    want = np.array([LD(2.0) ** 60 - 1 + LD(2.0) ** -3, LD(2.0) ** 60 + 1 - LD(2.0) ** -3], dtype=LD)
    if HAVE_LD:
        assert np.array_equal(got, want)
    else:
        assert np.allclose(got.astype(np.float64), want.astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the pass forms through the test hook
# ---------------------------------------------------------------------------------------------------------------------------
def _hooks():
    L = _lib.lib()
    v, i64 = C.c_void_p, C.c_int64
    L.gml_test_i8_pass.argtypes = [v, C.c_int, C.c_int, i64, v, v, v, v, i64, v, v, v, v, v, v]
    L.gml_test_i8_instances.argtypes = [v, C.c_int, C.c_int]
    return L


def i8_pass(p, form, prec, nodes, theta, *, coarse=False, lf=0, want_grad=True, compact=True, zero_theta=False, tauovr=None, vec=None,
            hv=0, hv_lf=5, ksub=1, kchunk=0, kpart=0):
    L = _hooks()
    nodes = np.ascontiguousarray(nodes, dtype=np.int64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    R, P = theta.shape
    kn = np.array([coarse, lf, want_grad, compact, zero_theta, hv, hv_lf, ksub, kchunk, kpart, 0], dtype=np.int64)
    f, g, h = np.zeros(R), np.zeros((R, P)), np.zeros((R, P))
    slots, plan = np.zeros((2, R, 3)), np.zeros(2, dtype=np.int64)
    tv = None if tauovr is None else np.ascontiguousarray(tauovr, dtype=np.float64)
    vv = None if vec is None else np.ascontiguousarray(vec, dtype=np.float64)
    _lib.check(L.gml_test_i8_pass(p._h, _lib.FORMULATION_IDS[form], _lib.PRECISIONS[prec], R, _lib._ptr(nodes), _lib._ptr(theta),
                                  None if tv is None else _lib._ptr(tv), None if vv is None else _lib._ptr(vv), P, _lib._ptr(kn),
                                  _lib._ptr(f), _lib._ptr(g), _lib._ptr(h), _lib._ptr(slots), _lib._ptr(plan)))
    return dict(f=f, g=g if want_grad else None, hv=h if hv else None, s0=slots[0], s1=slots[1], plan=tuple(int(x) for x in plan))


def instances(reset=False):
    L = _hooks()
    out = np.zeros(8, dtype=np.uint64)
    nw = L.gml_test_i8_instances(_lib._ptr(out), 8, int(reset))
    bits = set()
    for b in range(64 * nw):
        if (int(out[b >> 6]) >> (b & 63)) & 1:
            bits.add(b)
    return bits


def fwd_bit(LF, FORM, WANTF, WIDE, COARSE, UNIW):  # the numbering of gml_i8.h (kI8InstBits)
    return (LF - 2) * 64 + {0: 0, 2: 1, 3: 2, 4: 3}[FORM] * 16 + WANTF * 8 + WIDE * 4 + COARSE * 2 + UNIW


def fwdw_bit(FORM, WANTF, WIDE, UNIW, COARSE):
    return 256 + (FORM == 2) * 16 + WANTF * 8 + WIDE * 4 + UNIW * 2 + COARSE


def bwd_bit(NL, pl0):
    return 288 + {2: 0, 3: 1, 4: 2, 6: 3}[NL] * 4 + {0: 0, 1: 1, 3: 2}[pl0]


def reachable_instances():
    """Every kernel instance i8_pass can launch.  Excluded combinations, and why:
      * coarse RPLE and coarse product passes: i8_pass forces coarse = false for them (gml_i8_pass.hip, `const bool coarse`), and the
        launchers instantiate COARSE only under FORM == 0 (launch_fwd4 / launch_fwd_w4);
      * LF = 2: products only (launch_fwd_i8, `case 2`); an objective pass has LF >= 3 (`if (LF < 3 && !hv) LF = 3`);
      * COARSE with LF != 4: a coarse pass runs four limbs (`coarse ? 4`) and launch_fwd4 instantiates COARSE only for LF == 4;
      * RPLE with WANTF = false: launch_fwd / launch_fwd_i8w run RPLE as <FORM 2, WANTF true> (f is its forward kernel's FP64 sum);
      * product passes never use the i8w format (`const bool wide = a.wide && !hv`) and always run WANTF = false;
      * i8w beyond 2^21 columns: refused (GML_EUNSUPPORTED), nothing is launched;
      * backward: planes (6, 0) and (3, 3) for i8w (the latter coarse), (3, 1) for coarse i8x, (4, 0) and, for hv = 2 products, (2, 0);
        the other NL / pl0 pairs exist only in the -DI8W_BWD33 build."""
    bits = set()
    for WIDE in (0, 1):
        for UNIW in (0, 1):
            for LF in (3, 4, 5):
                for FORM, WANTF in ((0, 0), (0, 1), (2, 1)):
                    bits.add(fwd_bit(LF, FORM, WANTF, WIDE, 0, UNIW))
            for WANTF in (0, 1):
                bits.add(fwd_bit(4, 0, WANTF, WIDE, 1, UNIW))
            for LF in (2, 3, 4, 5):
                for FORM in (3, 4):
                    bits.add(fwd_bit(LF, FORM, 0, WIDE, 0, UNIW))
            for FORM, WANTF in ((0, 0), (0, 1), (2, 1)):
                bits.add(fwdw_bit(FORM, WANTF, WIDE, UNIW, 0))
            for WANTF in (0, 1):
                bits.add(fwdw_bit(0, WANTF, WIDE, UNIW, 1))
    bits |= {bwd_bit(6, 0), bwd_bit(3, 3), bwd_bit(3, 1), bwd_bit(4, 0), bwd_bit(2, 0)}
    bits |= {304, 305, 306, 307}  # k_finalize_i8 (objective, products), k_finalize_i8w (full, coarse)
    return bits


def _rows(n, count, seed):
    rng = np.random.default_rng(seed)
    rest = rng.choice(np.arange(1, n - 1), size=count - 4, replace=count - 4 > n - 2)
    return np.concatenate([[0, n - 1, 3, 3], rest]).astype(np.int64)  # node 0, node n-1, a repeated node; two slot tiles


def _thetas(R, P, seed):
    rng = np.random.default_rng(seed)
    sparse = rng.normal(size=(R, P)) * (rng.random((R, P)) < 0.05)
    sparse[:, 0] += 0.01  # (no empty row)
    sparse *= 2.0 / np.abs(sparse).sum(axis=1, keepdims=True)  # sum |theta| = 2 whatever P
    dense = rng.normal(size=(R, P)) * (1.5 / P)
    dyn = rng.normal(size=(R, P))
    dyn *= 60.0 / np.abs(dyn).sum(axis=1, keepdims=True)
    return {"sparse": sparse, "dense": dense, "dyn": dyn, "zero": np.zeros((R, P))}


def _counts(K, seed):
    rng = np.random.default_rng(seed)
    c = np.floor(10 ** rng.uniform(0, 3, size=K))
    c[rng.random(K) < 0.03] = 0.0
    return c


# the objective forms: (label, precision, coarse, lf)
OBJ_FORMS = [("f64", "f64", False, 0), ("i8x/3", "i8x", False, 3), ("i8x/4", "i8x", False, 4), ("i8x/5", "i8x", False, 5),
             ("i8x/coarse", "i8x", True, 0), ("i8w", "i8w", False, 0), ("i8w/coarse", "i8w", True, 0)]
# the product passes after the i8x objective pass: (hv, lf, ksub)
HV_FORMS = [(1, 5, 1), (2, 2, 1), (1, 2, 4), (2, 5, 4), (1, 3, 1), (1, 4, 1), (2, 2, 4), (1, 5, 4)]
_seen = set()
_ran = set()  # the matrix tests that ran in this session (the coverage test needs all of them)
_worst = {}
_fails = []  # every case runs; the failures are listed together at the end of a test


def _expect(ok, what):
    if not ok:
        _fails.append(what)


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), float(ratio))


def _run_rescaled(p, form, prec, nodes, theta, **kw):
    """one pass, then -- as the operator does -- re-runs with tauovr = (mmax + 1) unit tau / vdiv while a row leaves more than 8 (i8w: 4)
    bits of its planes unused; every pass's slots are kept for the range check"""
    wide = prec == "i8w"
    out = i8_pass(p, form, prec, nodes, theta, **kw)
    passes = [out]
    if prec == "f64" or form == "RPLE":
        return out, passes
    mm_min = (1 << 27) if wide else (1 << 23)
    for _ in range(6):
        tau, mm = out["s0"][:, 1], out["s0"][:, 2]
        if (mm >= mm_min).all():
            break
        ovr = np.where(mm < mm_min, (mm + 1.0) * MMAX_UNIT[wide] * tau * (1.0 + 1e-12) / VDIV[wide], 0.0)
        out = i8_pass(p, form, prec, nodes, theta, tauovr=ovr, **kw)
        passes.append(out)
    return out, passes


def _check_range(tag, form, prec, passes, ref_vmax, d):
    wide = prec == "i8w"
    for q in passes:
        tau, mm = q["s0"][:, 1], q["s0"][:, 2]
        cap = tau * VDIV[wide] if form == "RPLE" else (mm + 1.0) * MMAX_UNIT[wide] * tau * np.exp(d) * (1.0 + EXP_ERR)
        ratio = (ref_vmax.astype(np.float64) / cap).max()
        _note(("range", prec, form), ratio)
        _expect(ratio <= 1.0, (tag, "range bound", ratio))


def _matrix(p, ref, nodes, label):
    """every objective form x formulation x theta family x want_grad, and the product passes, on one problem"""
    P, K = ref.P, ref.K
    thetas = _thetas(len(nodes), P, seed=P)
    vec = np.random.default_rng(P + 1).normal(size=(len(nodes), P)) * (np.random.default_rng(P + 2).random((len(nodes), P)) < 0.3)
    runs, keeps = [], {}
    for fam, th in thetas.items():
        for form in FORMS:
            for flabel, prec, coarse, lf in OBJ_FORMS:
                if coarse and form == "RPLE":
                    continue
                kw = dict(coarse=coarse, lf=lf)
                full, passes = _run_rescaled(p, form, prec, nodes, th, **kw)
                obj, obj_passes = _run_rescaled(p, form, prec, nodes, th, want_grad=False, **kw)
                again, _ = _run_rescaled(p, form, prec, nodes, th, **kw)
                dense, _ = _run_rescaled(p, form, prec, nodes, th, compact=False, **kw)
                tag = (label, fam, form, flabel)
                # same bits: two runs, compacted = dense, zero_theta = the GEMM at theta = 0
                atomic = prec == "f64" or form == "RPLE"  # (f an FP64 atomic sum: run-to-run spread)
                for other in (again, dense):
                    fs = np.abs(full["f"]).max()
                    if atomic:
                        _expect(np.abs(other["f"] - full["f"]).max() <= 1e-13 * fs, (tag, "same f"))
                    else:
                        _expect(np.array_equal(other["f"], full["f"]), (tag, "same f bits"))
                    if prec != "f64":
                        _expect(np.array_equal(other["g"], full["g"]), (tag, "same g bits"))
                    else:
                        _expect(np.abs(other["g"] - full["g"]).max() <= 1e-13 * fs, (tag, "same g"))
                if fam == "zero" and prec != "f64":
                    z, _ = _run_rescaled(p, form, prec, nodes, th, zero_theta=True, **kw)
                    zf = np.abs(z["f"] - full["f"]).max() <= 1e-13 * np.abs(full["f"]).max() if atomic else np.array_equal(z["f"], full["f"])
                    _expect(zf and np.array_equal(z["g"], full["g"]), (tag, "zero_theta bits"))
                # objective-only = with gradient: the same integer sum (coarse: of the same 23-bit magnitudes) -- or an FP64 atomic sum
                if atomic:
                    _expect(np.abs(obj["f"] - full["f"]).max() <= 1e-13 * np.abs(full["f"]).max(), (tag, "objective-only f"))
                else:
                    _expect(np.array_equal(obj["f"], full["f"]), (tag, "objective-only f bits"))
                runs.append((tag, form, prec, coarse, lf, th, full, obj, passes + obj_passes, (fam, form), None))
                keeps.setdefault((fam, form), [])
            if fam in ("sparse", "dense"):
                for hv, hlf, ksub in HV_FORMS:
                    out = i8_pass(p, form, "i8x", nodes, th, vec=vec, hv=hv, hv_lf=hlf, ksub=ksub)
                    runs.append(((label, fam, form, f"hv{hv}/lf{hlf}/ksub{ksub}"), form, "hv", hv, hlf, th, out, vec, None, (fam, form), out["plan"]))
                out = i8_pass(p, form, "f64", nodes, th, vec=vec, hv=1)
                runs.append(((label, fam, form, "hv f64"), form, "hv64", 1, 0, th, out, vec, None, (fam, form), (1, 1)))
    for run in runs:
        if run[10] is not None and run[10] not in keeps[run[9]]:
            keeps[run[9]].append(run[10])
    order = list(keeps)
    res = dict(zip(order, ref.run(nodes, [dict(form=form, theta=thetas[fam], vec=vec if keeps[(fam, form)] else None, keep=keeps[(fam, form)])
                                          for fam, form in order])))
    sq = np.sqrt(K)
    for run in runs:
        tag, form, prec = run[0], run[1], run[2]
        o = res[run[9]]
        f_ref = o["f"].astype(np.float64)
        if prec in ("hv", "hv64"):
            out, p_vec = run[6], run[7]
            hv_ref = o["hv"][keeps[run[9]].index(run[10])].astype(np.float64)
            err = np.abs(out["hv"] - hv_ref).max(axis=1)
            if prec == "hv64":
                bound = FTOL * np.abs(f_ref) * np.abs(p_vec).sum(axis=1)
            else:
                hv_, hlf = run[3], run[4]
                kc, kp = out["plan"]
                kpart = K if kc == 0 else (K // kc) * kp + min(K % kc, kp)
                tau_h, tau_v = out["s1"][:, 1], out["s0"][:, 1]
                ch = 2.0 if form == "RPLE" else 1.0
                p1 = np.abs(p_vec).sum(axis=1)
                dq = quant_defect(p_vec, hlf)
                bound = (1e-13 * np.abs(f_ref) + 3.3 * np.sqrt(kpart) * tau_h + 3.3 * np.sqrt(kpart) * ch * tau_v * p1
                         + dq * o["hsum"][keeps[run[9]].index(run[10])].astype(np.float64))
                umax = (o["umax"][keeps[run[9]].index(run[10])].astype(np.float64) / tau_h).max()
                _expect(umax <= (32639.0 if hv_ == 2 else 2.0 ** 31), (tag, "product range", umax))
            ratio = (err / bound).max()
            _note(("hv" if prec == "hv" else "hv64", form, tag[3]), ratio)
            _expect(ratio <= 1.0, (tag, "products", ratio))
            continue
        coarse, lf, th, full, obj, passes = run[3:9]
        wide = prec == "i8w"
        err = np.maximum(np.abs(full["f"] - f_ref), np.abs(full["g"] - o["g"].astype(np.float64)).max(axis=1))
        err = np.maximum(err, np.abs(obj["f"] - f_ref))
        d = quant_defect(th, 7 if wide else (4 if coarse else (lf or 5)), coarse_wide=wide and coarse)
        if prec == "f64" or (wide and not coarse):
            tol = I8W_DYN_TOL if (wide and tag[1] == "dyn") else FTOL
            bound = tol * np.abs(f_ref)
        else:
            tau = full["s0"][:, 1]
            unit = COARSE_UNIT[wide] if coarse else 1.0
            q = 2.0 * d if form == "RPLE" else np.expm1(d) * np.abs(f_ref)
            e = EXP_ERR * np.abs(f_ref) if (not wide and form != "RPLE") else 0.0
            bound = 1e-13 * np.abs(f_ref) + 3.3 * sq * tau * unit + e + q
        bound = np.maximum(bound, 1e-300)
        ratio = (err / bound).max()
        _note((prec + ("/coarse" if coarse else f"/lf{lf}" if prec == "i8x" else ""), form, tag[1]), ratio)
        _expect(ratio <= 1.0, (tag, "value", ratio, err.max()))
        if prec != "f64":
            _check_range(tag, form, prec, passes, o["vmax"], d)


def _report(label):
    for key in sorted(_worst, key=str):
        print(f"{label} worst measured/bound {key}: {_worst[key]:.3g}")
    _worst.clear()
    fails = list(_fails)
    _fails.clear()
    for f in fails[:200]:
        print("FAILED CASE", f)
    assert not fails, f"{len(fails)} cases failed (listed above)"


@pytest.fixture(scope="module")
def coverage():
    instances(reset=True)  # (the record is per process: earlier test files ran other instances)
    return _seen


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("uniform", [True, False])
def test_pass_forms_narrow(uniform, coverage):
    # (a) pairwise, n = 97, K = 10007 (not a multiple of 32, 256 or 1024: the UNIW padding guard and the Kp padding matter)
    n, K = 97, 10007
    rng = np.random.default_rng(7)
    spins = np.where(rng.random((K, n)) < 0.55, 1, -1).astype(np.int8)
    counts = None if uniform else _counts(K, 8)
    _ran.add(("narrow", uniform))
    with gml.Problem(spins=spins, counts=counts) as p:
        ref = Ref(p.spins(), p.counts())
        _matrix(p, ref, _rows(n, 45, 1), f"narrow uniform={uniform}")
    _seen.update(instances())
    _report(f"narrow uniform={uniform}")


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("uniform", [True, False])
def test_pass_forms_wide(uniform, coverage):
    # (b) order 3, n = 258: 33154 statistics columns (> 32768: the WIDE instances)
    n, K = 258, 3001
    rng = np.random.default_rng(9)
    spins = np.where(rng.random((K, n)) < 0.5, 1, -1).astype(np.int8)
    counts = None if uniform else _counts(K, 10)
    _ran.add(("wide", uniform))
    with gml.Problem(spins=spins, counts=counts, order=3) as p:
        assert p.P == 33154
        keys = {}

        def karr(u):
            if u not in keys:
                keys[u] = p.multi_keys_array(u)
            return keys[u]

        ref = Ref(p.spins(), p.counts(), order=3, keys=karr)
        _matrix(p, ref, _rows(n, 36, 2), f"wide uniform={uniform}")
    _seen.update(instances())
    _report(f"wide uniform={uniform}")


@need_ld
@pytest.mark.gpu
def test_pass_forms_beyond_2p24_configurations(coverage):
    # (c) K = 2^24 + 5 2^20 + 123 > 2^24: several sets of i32 accumulators (gplanes > 1) and the split-K clamp at 2^22; non-uniform
    # counts.  One form per width and one product pass, on a few rows (the reference is the expensive part here)
    n, K = 64, (1 << 24) + 5 * (1 << 20) + 123
    rng = np.random.default_rng(13)
    spins = (1 - 2 * rng.integers(0, 2, size=(K, n), dtype=np.int8)).astype(np.int8)
    counts = _counts(K, 14)
    nodes = np.array([0, 63, 17, 17], dtype=np.int64)
    th = np.random.default_rng(15).normal(size=(len(nodes), n)) * (1.5 / n)
    vec = np.random.default_rng(16).normal(size=(len(nodes), n))
    _ran.add(("beyond 2^24", None))
    with gml.Problem(spins=spins, counts=counts) as p:
        ref = Ref(spins, counts)
        del spins
        x = i8_pass(p, "RISE", "i8x", nodes, th, vec=vec, hv=1, hv_lf=5, ksub=1)
        w = i8_pass(p, "RISE", "i8w", nodes, th)
    o = ref.run(nodes, [dict(form="RISE", theta=th, vec=vec, keep=[x["plan"]]), dict(form="RISE", theta=th, vec=None, keep=[])])
    f_ref = o[0]["f"].astype(np.float64)
    ex = np.maximum(np.abs(x["f"] - f_ref), np.abs(x["g"] - o[0]["g"].astype(np.float64)).max(axis=1))
    bx = 1e-13 * f_ref + 3.3 * np.sqrt(K) * x["s0"][:, 1] + EXP_ERR * f_ref + np.expm1(quant_defect(th, 5)) * f_ref
    ew = np.maximum(np.abs(w["f"] - f_ref), np.abs(w["g"] - o[1]["g"].astype(np.float64)).max(axis=1))
    bw = FTOL * f_ref
    kc, kp = x["plan"]
    kpart = (K // kc) * kp + min(K % kc, kp)
    eh = np.abs(x["hv"] - o[0]["hv"][0].astype(np.float64)).max(axis=1)
    bh = (1e-13 * f_ref + 3.3 * np.sqrt(kpart) * x["s1"][:, 1] + 3.3 * np.sqrt(kpart) * x["s0"][:, 1] * np.abs(vec).sum(axis=1)
          + quant_defect(vec, 5) * o[0]["hsum"][0].astype(np.float64))
    print(f">2^24: plan {x['plan']}, measured/bound i8x {(ex / bx).max():.3g}, i8w {(ew / bw).max():.3g}, hv {(eh / bh).max():.3g}")
    assert kc <= (1 << 22)
    assert (ex <= bx).all() and (ew <= bw).all() and (eh <= bh).all()
    for q, wide, lf in ((x, False, 5), (w, True, 7)):
        cap = (q["s0"][:, 2] + 1.0) * MMAX_UNIT[wide] * q["s0"][:, 1] * np.exp(quant_defect(th, lf)) * (1.0 + EXP_ERR)
        assert (o[0]["vmax"].astype(np.float64) <= cap).all()
    _seen.update(instances())


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("skew", [False, True])
@pytest.mark.parametrize("form", ["RISE", "logRISE"])
def test_clustered_energies_meet_the_noise_model(form, skew):
    # A row whose only non-zero parameter is its local field has two energies, -+theta_u: every sample of a spin class shares one
    # error of vq_exp, so the error of f grows with f, not like a random walk.  Node 0 is +1 in 97 % of the samples (skew: those
    # carry 1000 times the count as well), and theta_u takes values where the FP32 expm1 errs most for that class (7e-10 of
    # exp(-theta_u) in a CPU emulation of the instruction sequence).  The 38-bit form (lf = 5) quantises these theta exactly
    # enough that the exp error dominates; the bound is the solver's noise model with e = EXP_ERR |f|.  (With 3.3e-10 |f| in its
    # place these rows measure up to 2x over; the ratio against that coefficient is printed for comparison.)
    n, K = 40, 10007
    rng = np.random.default_rng(21)
    spins = np.where(rng.random((K, n)) < 0.5, 1, -1).astype(np.int8)
    spins[:, 0] = np.where(rng.random(K) < 0.97, 1, -1)
    counts = np.where(spins[:, 0] > 0, 1000.0, 1.0) if skew else None
    field = np.array([0.01649, 0.038239, -0.015781, 0.059653, -0.02695, -0.0385])
    nodes = np.zeros(len(field), dtype=np.int64)
    th = np.zeros((len(field), n))
    th[:, 0] = field
    with gml.Problem(spins=spins, counts=counts) as p:
        ref = Ref(p.spins(), p.counts())
        out = i8_pass(p, form, "i8x", nodes, th)
    o = ref.run(nodes, [dict(form=form, theta=th, vec=None, keep=[])])[0]
    f_ref = o["f"].astype(np.float64)
    err = np.maximum(np.abs(out["f"] - f_ref), np.abs(out["g"] - o["g"].astype(np.float64)).max(axis=1))
    walk = 1e-13 * f_ref + 3.3 * np.sqrt(K) * out["s0"][:, 1] + np.expm1(quant_defect(th, 5)) * f_ref
    ratio, ratio_old = err / (walk + EXP_ERR * f_ref), err / (walk + 3.3e-10 * f_ref)
    print(f"clustered {form} skew={skew}: |err| / f", " ".join(f"{e:.2e}" for e in err / f_ref),
          f"| measured/bound {ratio.max():.3g} (against 3.3e-10 |f|: {ratio_old.max():.3g})")
    assert (ratio <= 1.0).all(), ratio


@need_ld
@pytest.mark.gpu
def test_every_reachable_instance_ran(coverage):
    # the record of the matrices above (pytest runs this file's tests in order, in one process) equals the list of reachable
    # instances; selected without them, there is nothing to compare
    if len(_ran) < 5:
        pytest.skip("needs the five matrix tests of this file (narrow, wide, beyond 2^24) in the same session")
    _seen.update(instances())
    want = reachable_instances()
    assert not (want - _seen), sorted(want - _seen)
    assert not (_seen - want), sorted(_seen - want)
