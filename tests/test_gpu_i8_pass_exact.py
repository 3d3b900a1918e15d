"""The objective passes of the int8-limb operator (k_fwd_i8, k_fwd_i8w, k_bwd_i8, k_finalize_i8, k_finalize_i8w), cut at the limb planes
Vq of V and held on both sides to the host model tests/_i8_pass_reference.py (itself held to brute force by
tests/test_host_i8_pass_reference.py).  Passes run through gml_test_i8_pass, one at a time; the device's Vq and slot sums come back
through gml_test_i8_pass_state, the operands (the internal-layout rows of Theta) through gml_test_i8_pack_state, the i32 accumulator
planes and the internal-layout G and f through gml_test_i8_gacc.  All three hooks only copy.

A.  Exact, given the device's own Vq: csum, csum2, asum, asum2 and (i8x) mmax are the model's integers; every Gacc entry is the model's
    sum_k v_l b, int32 for int32, for every slot of every tile that ran (the rows of unused slots multiply whatever their planes
    hold: the model multiplies the same bytes); G is the model's float64 bit for bit over all Qp columns of every active row -- the
    constant column, the zeros beyond Qf.  The rows of G of the unused slots are compared before and after each pass; this is a
    LIMITED check, not the sentinel the issue had in mind: the hooks are read-only and cannot plant one, the first pass of a handle
    has nothing to compare with, and rows that happen to hold zeros would not show a kernel that wrote zeros.  f of the exp forms is
    bit for bit, with and without the gradient.  RPLE's f is a sum of
    device FP64 terms, not a function of Vq: it stays with test_gpu_i8_pass_variants.py.  i8w's mmax comes from the un-rounded y: from
    Vq it is held to the interval the comment at k_fwd_i8w's tail derives, and to the formula's value for the model's own y where
    every y within its error bound gives the same high word.
B.  Forward, element by element: for every sample of every listed row the model gives y = (w_k / (unit tau_r)) F(E_k) + d(u, k) in
    np.longdouble (E exact from the integers of the quantised row and the sign bits; tau as the pass reports it) and the device's
    magnitude must be rint(y) wherever |y - nearest half-integer| > eps_k; elsewhere within 1 + ceil(eps_k) units.  The sign is -s.
    Padding samples and samples of count zero have every digit zero.
      eps_k = (e_exp + 2^-53 (ROUNDINGS + 2 |E_k|)) (y_k + 1),  ROUNDINGS = 3,  y_k the first term of y
    e_exp: the relative error of the device's F.  EXP_ERR = 1e-9 for the i8x exp forms (test_gpu_i8_pass_variants.py derives it: three
    FP32 roundings of ~2^-24 |r|, |r| <= ln2 / 128, in vq_exp's expm1); 1e-15 for i8w and for RPLE (exp_tab and the FP64 layers, as
    gml_i8.h states).  At E_k = 0 exactly the exp forms compute 1 exactly (n = 0, r = 0: the table entry 2^0 times 1 + 0), so e_exp = 0
    there: the zero family has no other energy.  The second term is the issue's "a few 2^-53 (1 + |E|)" written out: 1 / tau,
    w_k / tau and the final fma are rounded once each (ROUNDINGS 2^-53 relative to y); E_k is rounded to float64 once, an absolute error
    of 2^-53 |E| in the exponent, which is a relative error of 2^-53 |E| of exp(-E) -- and of twice that for RPLE, whose F is a
    function of 2 E: 2 |E| covers both.  The model's own longdouble error (2^-63 of the same terms) is below a thousandth of that.
    Never fitted.
    Condition (computed from the model alone, asserted here before the device is compared and by test_decidable_share_on_the_host
    without any GPU): at least DECIDABLE_CASE = 0.9 of a case's real samples and DECIDABLE_ROW = 0.5 of every row's are decidable.
    y_k reaches vdiv = 2.13e9 (1.4e14) at the top of a row's range, where eps_k is 2 units (0.2 units); theta families whose rows keep
    most samples there are scaled UP for that form (SCALE below: the bound exp(sum |theta|) that tau is derived from then leaves the
    typical sample lower in the planes).  SCALE: i8x exp forms, not coarse: sparse x 32 (its rows of one or two non-zero columns keep
    half their samples at the top whatever the scale; at x 32 the narrow problem with uniform counts has 0.917 per case and 0.504 in its
    worst row), dense x 4; i8w exp forms, not coarse: sparse x 2, dense x 2.  Everything else runs the families of _thetas as they are.
    DEVIATION from the condition, stated and not hidden: RPLE in the i8w format on UNIFORM counts cannot reach the caps and no scale of
    theta changes that.  y_k = vdiv (w_k / w_max) sig_k with vdiv = 1.4e14 and sig_k = 1 / (1 + exp(2 E_k)): at equal weights every
    sample with E_k < 0 sits within a factor two of the top of the 47-bit range, where the header's 1e-15 is 0.14 units, and scaling
    theta (either sign) only moves sig towards {0, 1} with half the samples on each side.  Computed shares per case / worst row on
    the narrow problem: sparse 0.783 / 0.743, dense 0.811 / 0.800, dyn 0.645 / 0.618, zero 0.813 / 0.813.  For these four cases
    (CAP_SHORTFALL) the caps are not asserted; their shares are printed and every element is still held by the rule above.  With
    counts (weights spread over three decades) the same form meets the caps (0.948 .. 0.974).  test_tauovr_rerun prints its share as
    well: a re-run exists to move a row's largest sample to the top of the range, and is not one of the matrix's cases.
C.  The device's f and G also stay within the bounds of test_gpu_i8_pass_variants.py against its 80-bit reference (Ref), on the same
    inputs; and gml_test_i8_instances shows that every forward, backward and finalise instance an objective pass can reach below
    32768 statistics columns ran.

Shapes: pairwise n = 97, K = 10007 (not a multiple of 32, 256 or 1024; Kp = 10240, five full split-K chunks of 2048), once with
uniform counts (the UNIW instances and their padding guard) and once with counts floor(10^U(0,3)), 3 % of them zero; rows
_rows(n, 45, seed): node 0, node n - 1, a repeated node, two slot tiles, the second partial.  Order 3 at n = 20: 210 statistics columns
(20 + 190), Qfp = 256, four 64-column steps, 46 padding columns; K = 4099 (Kp = 5120: three chunks of 2048, the last partial).
Order 6 at n = 10 (`order6`): 637 statistics columns (10 + 45 + 120 + 210 + 252), Qfp = 640, ten steps, keys of up to five spins
besides the node's own, P = 382; K = 4099, rows _rows(n, 45, 4).  The SCALE table and the caps are those of the other problems.
test_split_k_last_chunk_partial: pairwise n = 40, K = 2049 -- the smallest K whose backward launch has two chunks with the last one
partial: Kp = 3072 (K rounded up to 1024), plan kchunk = 2048 (i8_split_plan: two node tiles give nsplit = 256, ceil(Kp / 256) = 12 rounded
up to 256 samples, raised to the minimum chunk of 2048), chunks
[0, 2048) and [2048, 3072).  More than 2^24 configurations (gplanes > 1) are out of scope: their Vq read-back is gigabytes, and
test_pass_forms_beyond_2p24_configurations (test_gpu_i8_pass_variants.py) stays their guard.  Product (Hessian-vector) passes write
Uq, not Vq: test_gpu_i8_hv_exact.py cuts them there, beside test_gpu_i8_pass_variants.py and test_gpu_hv_sparse_direct.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _i8_pack_reference as R
import _i8_pass_reference as M
import gml_amd as gml
from oracle import oracle as O
from test_gpu_i8_pack_state import State
from test_gpu_i8_pass_variants import (COARSE_UNIT, EXP_ERR, FTOL, I8W_DYN_TOL, MMAX_UNIT, VDIV, Ref, _counts, _rows, _thetas, bwd_bit, fwd_bit,
                                       fwdw_bit, i8_pass, instances, need_ld, quant_defect)

_lib = importlib.import_module("gml_amd._lib")
LD = np.longdouble
ROUNDINGS = 3.0
EXP_WIDE = 1e-15
DECIDABLE_CASE, DECIDABLE_ROW = 0.9, 0.5
FAMILIES = ["sparse", "dense", "dyn", "zero"]
# (label, precision, coarse, lf)
OBJ_FORMS = [("i8x/3", "i8x", False, 3), ("i8x/4", "i8x", False, 4), ("i8x/5", "i8x", False, 5), ("i8x/coarse", "i8x", True, 0),
             ("i8w", "i8w", False, 0), ("i8w/coarse", "i8w", True, 0)]
CASES = [(form, fl) for form in ("RISE", "RPLE") for fl in OBJ_FORMS if not (fl[2] and form == "RPLE")]
PROBLEMS = ["narrow-uniform", "narrow-counts", "order3", "order6"]
# theta of a family times this, per (precision, exp form?, family), so that the decidable share meets the caps (docstring, B)
SCALE = {("i8x", True, False, "sparse"): 32.0, ("i8x", True, False, "dense"): 4.0, ("i8w", True, False, "sparse"): 2.0, ("i8w", True, False, "dense"): 2.0}


def _scale(prec, form, coarse, fam):
    return SCALE.get((prec, form != "RPLE", coarse, fam), 1.0)


def _cap_exempt(pb, prec, form, coarse, fam):
    """CAP_SHORTFALL (docstring, B: the one deviation from the condition): RPLE in the i8w format on uniform counts, every family"""
    return pb.counts is None and prec == "i8w" and form == "RPLE"


# ---------------------------------------------------------------------------------------------------------------------------
# problems, on the host
# ---------------------------------------------------------------------------------------------------------------------------
class Prob:
    def __init__(self, name):
        self.name = name
        if name.startswith("narrow"):
            self.n, self.K, self.order, seed = 97, 10007, 2, 7
            rng = np.random.default_rng(seed)
            self.spins = np.where(rng.random((self.K, self.n)) < 0.55, 1, -1).astype(np.int8)
            self.counts = None if name.endswith("uniform") else _counts(self.K, 8)
            self.nodes = _rows(self.n, 45, 1)
        elif name == "order3":
            self.n, self.K, self.order = 20, 4099, 3
            rng = np.random.default_rng(11)
            self.spins = np.where(rng.random((self.K, self.n)) < 0.5, 1, -1).astype(np.int8)
            self.counts = _counts(self.K, 12)
            self.nodes = _rows(self.n, 45, 3)
        elif name == "order6":  # keys of up to five spins besides the node's own: 637 statistics columns, Qfp = 640, ten steps
            self.n, self.K, self.order = 10, 4099, 6
            rng = np.random.default_rng(13)
            self.spins = np.where(rng.random((self.K, self.n)) < 0.5, 1, -1).astype(np.int8)
            self.counts = _counts(self.K, 14)
            self.nodes = _rows(self.n, 45, 4)
        else:
            self.n, self.K, self.order = 40, 2049, 2
            rng = np.random.default_rng(17)
            self.spins = np.where(rng.random((self.K, self.n)) < 0.5, 1, -1).astype(np.int8)
            self.counts = _counts(self.K, 18)
            self.nodes = _rows(self.n, 36, 5)
        n = self.n
        self.Kp = (self.K + 1023) // 1024 * 1024
        self.keys = R.stat_keys(n, self.order)
        self.Qf = len(self.keys)
        c = np.ones(self.K) if self.counts is None else self.counts
        self.w = np.zeros(self.Kp)
        self.w[:self.K] = c / c.sum()
        self.wmax = float(self.w.max())
        self.colidx = {tuple(int(i) for i in k if i >= 0): c for c, k in enumerate(self.keys)}  # sorted key -> column, any order
        self.pkeys = None if self.order == 2 else {int(u): O.multi_keys(n, self.order, int(u)) for u in set(self.nodes.tolist())}
        self.P = n if self.order == 2 else len(self.pkeys[int(self.nodes[0])])
        self._bits = {}
        self.sb = np.zeros((n, self.Kp), dtype=np.uint8)
        self.sb[:, :self.K] = (self.spins.T < 0)

    def bits(self, Qfp):
        if Qfp not in self._bits:
            b = R.stat_bits(self.spins, self.keys, Qfp, self.Kp)
            self._bits[Qfp] = (b, 1.0 - 2.0 * b.astype(np.float64))
        return self._bits[Qfp]

    def column(self, u, key):
        """internal column of the parameter of node u with the reference key `key` (which holds u): the statistic of the other spins;
        -1: the constant column"""
        rest = tuple(sorted(i for i in key if i != u))
        return self.colidx[rest] if rest else -1

    def internal(self, th, Qp, cconst):
        """the rows th [R][P] (reference order) in the internal column layout"""
        out = np.zeros((len(self.nodes), Qp))
        for r, u in enumerate(self.nodes):
            u = int(u)
            if self.order == 2:
                out[r, :self.n] = th[r]
                out[r, cconst] = th[r, u]
                out[r, u] = 0.0
            else:
                for p, key in enumerate(self.pkeys[u]):
                    c = self.column(u, key)
                    out[r, cconst if c < 0 else c] = th[r, p]
        return out

    def thetas(self, prec, form, coarse):
        th = _thetas(len(self.nodes), self.P, seed=self.P)
        return {fam: th[fam] * _scale(prec, form, coarse, fam) for fam in FAMILIES}


_probs = {}


def prob(name):
    if name not in _probs:
        _probs[name] = Prob(name)
    return _probs[name]


# ---------------------------------------------------------------------------------------------------------------------------
# B on the host: the model's elements, their error bounds, the decidable share
# ---------------------------------------------------------------------------------------------------------------------------
def eps_of(prec, form, o):
    e_exp = np.full(len(o["E"]), EXP_ERR if (prec == "i8x" and form != "RPLE") else EXP_WIDE)
    if form != "RPLE":
        e_exp[o["E"] == 0.0] = 0.0
    return (e_exp + 2.0 ** -53 * (ROUNDINGS + 2.0 * np.abs(o["E"]))) * (o["ymag"].astype(np.float64) + 1.0)


def model_rows(pb, prec, form, coarse, lf, theta_int, Qfp, cconst, tau):
    """forward_row of every listed row, with its eps and the decidable mask"""
    lbt = M.LBT[prec]
    bits, x = pb.bits(Qfp)
    rows = []
    for r, u in enumerate(pb.nodes):
        u = int(u)
        o = M.forward_row(form, lbt, coarse, lf, theta_int[r], Qfp, cconst, u, pb.sb[u], bits, pb.w, tau[r], pb.K, x)
        o["eps"] = eps_of(prec, form, o)
        # (a sample of count zero rounds the dither alone, exactly: decidable whatever its margin)
        o["dec"] = (o["margin"].astype(np.float64) > o["eps"]) | ~o["real"]
        rows.append(o)
    return rows


def shares(pb, rows):
    live = np.arange(pb.Kp) < pb.K
    per_row = np.array([o["dec"][live].mean() for o in rows])
    return float(np.mean([o["dec"][live] for o in rows])), float(per_row.min())


def host_tau(pb, prec, form, coarse, lf, theta_int, Qfp, cconst):
    """tau of a first pass (no tauovr) as tests/_i8_pack_reference.py states it"""
    lbt = M.LBT[prec]
    lfq = 7 if lbt == 6 else (4 if coarse else lf)
    out = []
    for r in range(len(pb.nodes)):
        sc = R.row_scalars(theta_int[r], Qfp, cconst, lfq)
        out.append(float(R.tau(sc["sabs"], sc["sx"], pb.wmax, form, lbt)))
    return np.array(out)


def test_key_lookup_gives_the_closed_form_columns():
    """Prob.column looks a parameter's other spins up in stat_keys; at order 3 that is the closed form it replaced"""
    pb = prob("order3")
    n = pb.n
    for u, keys in pb.pkeys.items():
        for key in keys:
            rest = sorted(i for i in key if i != u)
            want = -1 if not rest else rest[0] if len(rest) == 1 else n + rest[0] * n - rest[0] * (rest[0] + 1) // 2 + (rest[1] - rest[0] - 1)
            assert pb.column(u, key) == want, (u, key)
    p6 = prob("order6")
    assert (p6.Qf, p6.P, max(len(k) for k in p6.pkeys[0])) == (637, 382, 6)
    for u, keys in p6.pkeys.items():
        cols = [p6.column(u, k) for k in keys]
        assert len(set(cols)) == p6.P and cols.count(-1) == 1 and all(u not in p6.keys[c] for c in cols if c >= 0)


@need_ld
@pytest.mark.parametrize("name", PROBLEMS + ["splitk"])
def test_decidable_share_on_the_host(name):
    pb = prob(name)
    Qfp = (pb.Qf + 63) // 64 * 64
    cconst, Qp = Qfp, Qfp + 64
    cases = CASES if name != "splitk" else [("RISE", OBJ_FORMS[2]), ("RISE", OBJ_FORMS[4])]
    worst = {}
    for form, (flabel, prec, coarse, lf) in cases:
        th = pb.thetas(prec, form, coarse)
        for fam in (FAMILIES if name != "splitk" else ["dense"]):
            ti = pb.internal(th[fam], Qp, cconst)
            tau = host_tau(pb, prec, form, coarse, lf, ti, Qfp, cconst)
            case, row = shares(pb, model_rows(pb, prec, form, coarse, lf, ti, Qfp, cconst, tau))
            print(f"{name} {form} {flabel} {fam}: decidable share {case:.4f}, worst row {row:.4f}")
            if not _cap_exempt(pb, prec, form, coarse, fam):
                worst[(form, flabel, fam)] = (case, row)
    bad = {k: v for k, v in worst.items() if v[0] < DECIDABLE_CASE or v[1] < DECIDABLE_ROW}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: hooks
# ---------------------------------------------------------------------------------------------------------------------------
def _hooks():
    L = _lib.lib()
    v = C.c_void_p
    L.gml_test_i8_pass_state.argtypes = [v, v, v, v, v, v]
    L.gml_test_i8_gacc.argtypes = [v, v, v, v, v]
    return L


class PassState:
    """Vq, the slot sums, the accumulator planes and the internal-layout G and f as the last pass left them"""

    def __init__(self, p, want_g=True):
        L = _hooks()
        slots, planes, kp = C.c_int64(0), C.c_int(0), C.c_int64(0)
        _lib.check(L.gml_test_i8_pass_state(p._h, C.byref(slots), C.byref(planes), C.byref(kp), None, None))
        self.slots, self.lbt, self.Kp = int(slots.value), int(planes.value), int(kp.value)
        vq = np.zeros(self.slots * self.lbt * self.Kp, dtype=np.int8)
        sums = np.zeros((5, self.slots), dtype=np.int64)
        _lib.check(L.gml_test_i8_pass_state(p._h, C.byref(slots), C.byref(planes), C.byref(kp), _lib._ptr(vq), _lib._ptr(sums)))
        self.vq = vq
        self.planes = M.unpack_vq(vq, self.slots, self.Kp, self.lbt)
        self.csum, self.csum2, self.asum, self.asum2, self.mmax = sums
        d = np.zeros(8, dtype=np.int64)
        _lib.check(L.gml_test_i8_gacc(p._h, _lib._ptr(d), None, None, None))
        self.gplanes, self.stride, self.Qfp, gslots, glbt, self.ws_rows, self.Qp, _ = (int(x) for x in d)
        assert (gslots, glbt) == (self.slots, self.lbt) and self.stride == self.slots * self.lbt * self.Qfp
        g = np.zeros(self.gplanes * self.stride, dtype=np.int32)
        self.G = np.zeros((self.ws_rows, self.Qp)) if want_g else None
        self.F = np.zeros(self.ws_rows)
        _lib.check(L.gml_test_i8_gacc(p._h, _lib._ptr(d), _lib._ptr(g), None if self.G is None else _lib._ptr(self.G), _lib._ptr(self.F)))
        assert self.gplanes == 1  # (docstring: more than 2^24 configurations are out of scope)
        self.gacc = M.gacc_rows(g, self.slots, self.lbt, self.Qfp)


def read_G(p):
    L = _hooks()
    d = np.zeros(8, dtype=np.int64)
    _lib.check(L.gml_test_i8_gacc(p._h, _lib._ptr(d), None, None, None))
    G = np.zeros((int(d[5]), int(d[6])))
    if G.size:
        _lib.check(L.gml_test_i8_gacc(p._h, _lib._ptr(d), None, _lib._ptr(G), None))
    return G


_handles = {}


@pytest.fixture(scope="module")
def handles():
    instances(reset=True)  # (the record is per process: earlier test files ran other instances)
    yield _handles
    for p in _handles.values():
        p.close()
    _handles.clear()


def handle(handles, name):
    if name not in handles:
        pb = prob(name)
        handles[name] = gml.Problem(spins=pb.spins, counts=pb.counts, order=pb.order)
    return handles[name]


_refs = {}
_seen = set()
_ran = set()
_worst = {}


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# ---------------------------------------------------------------------------------------------------------------------------
# A: everything behind Vq
# ---------------------------------------------------------------------------------------------------------------------------
def check_behind_vq(tag, pb, ps, out, G_before, tau, form, coarse, want_grad, Qf, cconst):
    """ps: PassState after the pass; out: what gml_test_i8_pass returned; G_before: the workspace's G before the pass"""
    R_, lbt = len(pb.nodes), ps.lbt
    Rp = (R_ + 31) // 32 * 32
    exp_form = form != "RPLE"
    planes = ps.planes[:Rp]
    s = M.slot_sums(planes, coarse, exp_form, not want_grad)
    act = slice(0, R_)
    assert np.array_equal(ps.csum[act], s["csum"][act]), (tag, "csum")
    assert np.array_equal(ps.csum2[act], s["csum2"][act]), (tag, "csum2")
    if s["asum"] is not None:
        assert np.array_equal(ps.asum[act], s["asum"][act]), (tag, "asum")
        assert np.array_equal(ps.asum2[act], s["asum2"][act]), (tag, "asum2")
    if lbt == 4:
        assert np.array_equal(ps.mmax[act], s["mmax"][act]), (tag, "mmax")
    else:
        for r in range(R_):
            lo, hi = s["mmax"][r]
            assert lo <= ps.mmax[r] <= hi, (tag, "mmax outside the interval of its planes", r, int(ps.mmax[r]), lo, hi)
    assert np.array_equal(out["s0"][:, 2], ps.mmax[act].astype(np.float64)) and np.array_equal(out["s0"][:, 1], tau[act]), (tag, "slot results")
    rowcol = np.full(Rp, -1, dtype=np.int64)
    rowcol[:R_] = pb.nodes
    f_dev = ps.F[:R_]
    if want_grad:
        bits, _ = pb.bits(ps.Qfp)
        g = M.backward(planes, bits, coarse)
        bad = np.argwhere(ps.gacc[:Rp] != g)
        assert not len(bad), (tag, "Gacc [slot, plane, column]", bad[:4].tolist(), len(bad))
        G, f = M.finalize(lbt, coarse, tau, s, g, rowcol, Qf, ps.Qp, cconst, True, exp_form)
        assert _same_bits(ps.G[:R_], G[:R_]), (tag, "G", np.argwhere(ps.G[:R_] != G[:R_])[:4].tolist())
        assert _same_bits(ps.G[R_:], G_before[R_:]), (tag, "rows of unused slots were written")
    else:
        _, f = M.finalize(lbt, coarse, tau, s, None, rowcol, Qf, ps.Qp, cconst, False, exp_form)
    if exp_form:
        assert _same_bits(f_dev, f[:R_]), (tag, "f", f_dev[:3], f[:3])
        assert _same_bits(out["f"], f[:R_]) and _same_bits(out["s0"][:, 0], f[:R_]), (tag, "f as returned")
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# B: the elements of Vq
# ---------------------------------------------------------------------------------------------------------------------------
def check_elements(tag, pb, ps, rows, coarse, exp_form):
    lbt = ps.lbt
    live = np.arange(pb.Kp) < pb.K
    worst, nund = 0, 0
    val = M.value_of(M.live_planes(ps.planes[:len(rows)], coarse))
    for r, o in enumerate(rows):
        v = val[r]
        assert not np.any(v % o["unit"]), (tag, "digits below the coarse unit", r)
        assert not np.any(v[~o["real"]]), (tag, "a padding or zero-count sample has a digit", r, np.flatnonzero(v[~o["real"]])[:4].tolist())
        if coarse:
            assert not ps.planes[r, M.COARSE_PL0[lbt] - 1].any(), (tag, "the zero plane of a coarse pass", r)
        mag = np.abs(v) // o["unit"]
        assert np.array_equal(v, o["sign"] * mag * o["unit"]), (tag, "sign", r, np.flatnonzero(v != o["sign"] * mag * o["unit"])[:4].tolist())
        diff = np.abs(mag - o["mag"])
        dec = o["dec"]
        bad = np.flatnonzero(dec & (diff != 0))
        assert not len(bad), (tag, "decidable elements differ: slot", r, "samples", bad[:4].tolist(), "device", mag[bad[:4]].tolist(), "model",
                              o["mag"][bad[:4]].tolist(), "margin", o["margin"][bad[:4]].astype(float).tolist(), "eps", o["eps"][bad[:4]].tolist())
        und = ~dec
        bad = np.flatnonzero(und & (diff > 1 + np.ceil(o["eps"])))
        assert not len(bad), (tag, "undecidable elements off by more than 1 + ceil(eps): slot", r, bad[:4].tolist(), diff[bad[:4]].tolist())
        worst = max(worst, int(diff.max()))
        nund += int((und & live).sum())
        if lbt == 6 and exp_form:  # mmax for the model's own y, where every y inside its bound gives the same value
            yy = o["y"].astype(np.float64)
            sel = o["real"] if pb.counts is None else np.ones(len(yy), dtype=bool)
            lo = float(np.max(np.where(sel, yy - o["eps"] - 1e-6, 0.0)))
            hi = float(np.max(np.where(sel, yy + o["eps"] + 1e-6, 0.0)))
            a, b = M.mmax_wide_of_y(max(lo, 0.0) * 4294967296.0, coarse), M.mmax_wide_of_y(hi * 4294967296.0, coarse)
            if a == b:
                assert int(ps.mmax[r]) == a, (tag, "mmax for the model's y", r, int(ps.mmax[r]), a)
    return worst, nund


# ---------------------------------------------------------------------------------------------------------------------------
# C: the 80-bit reference, with the bounds of test_gpu_i8_pass_variants.py
# ---------------------------------------------------------------------------------------------------------------------------
def reference(p, pb, name, form, th_key, th):
    key = (name, form, th_key)
    if key not in _refs:
        if pb.order == 2:
            ref = Ref(pb.spins, pb.counts)
        else:
            keys = {}

            def karr(u):
                if u not in keys:
                    keys[u] = p.multi_keys_array(u)
                return keys[u]

            ref = Ref(pb.spins, pb.counts, order=pb.order, keys=karr)
        _refs[key] = ref.run(pb.nodes, [dict(form=form, theta=th, vec=None, keep=[])])[0]
    return _refs[key]


def check_reference(tag, pb, o, form, prec, coarse, lf, fam, th, full, obj):
    wide = prec == "i8w"
    f_ref = o["f"].astype(np.float64)
    err = np.maximum(np.abs(full["f"] - f_ref), np.abs(full["g"] - o["g"].astype(np.float64)).max(axis=1))
    err = np.maximum(err, np.abs(obj["f"] - f_ref))
    d = quant_defect(th, 7 if wide else (4 if coarse else (lf or 5)), coarse_wide=wide and coarse)
    tau = full["s0"][:, 1]
    unit = COARSE_UNIT[wide] if coarse else 1.0
    q = 2.0 * d if form == "RPLE" else np.expm1(d) * np.abs(f_ref)
    e = EXP_ERR * np.abs(f_ref) if (not wide and form != "RPLE") else 0.0
    bound = 1e-13 * np.abs(f_ref) + 3.3 * np.sqrt(pb.K) * tau * unit + e + q  # the solver's noise model: any single pass
    if wide and not coarse:
        # that file's relative bound holds for the pass the operator ends on: no row leaves more than four bits of its planes unused
        # (RPLE never does).  Here a pass runs once at the bound's own tau: the rows that would be re-run keep the noise model.
        settled = (full["s0"][:, 2] >= float(1 << 27)) | (form == "RPLE")
        bound = np.where(settled, (I8W_DYN_TOL if fam == "dyn" else FTOL) * np.abs(f_ref), bound)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    assert ratio <= 1.0, (tag, "the bound of test_gpu_i8_pass_variants.py against the 80-bit reference", ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------
# the matrix
# ---------------------------------------------------------------------------------------------------------------------------
def run_case(handles, name, form, flabel, prec, coarse, lf, families, variants=True):
    pb = prob(name)
    p = handle(handles, name)
    exp_form = form != "RPLE"
    thetas = pb.thetas(prec, form, coarse)
    kw = dict(coarse=coarse, lf=lf)
    for fam in families:
        th = thetas[fam]
        tag = (name, form, flabel, fam)
        G0 = read_G(p)
        full = i8_pass(p, form, prec, pb.nodes, th, **kw)
        st = State(p)
        ps = PassState(p)
        Qfp, Qf, cconst, Qp = st.Qfp, st.Qf, st.cconst, st.Qp
        R_ = len(pb.nodes)
        assert (st.Kp, st.K, Qf) == (pb.Kp, pb.K, pb.Qf) and ps.Qfp == Qfp and ps.Qp == Qp
        ti = pb.internal(th, Qp, cconst)
        assert np.array_equal(st.theta[:R_], ti), (tag, "the rows the pass read")
        tau = st.tau[:(R_ + 31) // 32 * 32].copy()
        if G0.shape != ps.G.shape:  # (the first pass of a handle sized the workspace)
            G0 = ps.G.copy()
            G0[:R_] = 0.0
        # B: the model first, its decidable share, then the device
        rows = model_rows(pb, prec, form, coarse, lf, st.theta[:R_], Qfp, cconst, tau)
        case, row = shares(pb, rows)
        if not _cap_exempt(pb, prec, form, coarse, fam):
            assert case >= DECIDABLE_CASE and row >= DECIDABLE_ROW, (tag, "decidable share", case, row)
        worst, nund = check_elements(tag, pb, ps, rows, coarse, exp_form)
        print(f"{name} {form} {flabel} {fam}: decidable share {case:.4f} (worst row {row:.4f}), worst |device - model| {worst} units, "
              f"{nund} undecidable elements")
        # A on the pass with the gradient
        check_behind_vq(tag, pb, ps, full, G0, tau, form, coarse, True, Qf, cconst)
        # the other forms of the same pass: the same planes, byte for byte (B carries over), and A on each
        vq_full, G1 = ps.vq, ps.G
        runs = [("objective only", dict(want_grad=False))]
        if variants:
            runs += [("not compacted", dict(compact=False)), ("not compacted, objective only", dict(compact=False, want_grad=False))]
            if fam == "zero":
                runs += [("zero_theta", dict(zero_theta=True)), ("zero_theta, objective only", dict(zero_theta=True, want_grad=False))]
        obj = None
        for what, extra in runs:
            out = i8_pass(p, form, prec, pb.nodes, th, **kw, **extra)
            ps2 = PassState(p)
            assert np.array_equal(State(p).tau[:R_], tau[:R_]), (tag, what, "tau")
            live = M.live_planes(ps2.planes[:R_], coarse)
            assert np.array_equal(live, M.live_planes(M.unpack_vq(vq_full, ps.slots, ps.Kp, ps.lbt)[:R_], coarse)), (tag, what, "Vq differs")
            wg = extra.get("want_grad", True)
            check_behind_vq(tag + (what,), pb, ps2, out, G1, tau, form, coarse, wg, Qf, cconst)
            if not wg:
                assert _same_bits(ps2.G, G1), (tag, what, "an objective-only pass wrote G")
                if exp_form:
                    # (equal as numbers: a row whose V all round to zero -- dyn at the bound's own tau -- has f = -tau * 0 = -0.0 with
                    # the gradient and tau * 0 = +0.0 without; each is the model's bit pattern)
                    assert np.array_equal(out["f"], full["f"]), (tag, what, "f with and without the gradient")
            else:
                G1 = ps2.G
            if what == "objective only":
                obj = out
        # C
        o = reference(p, pb, name, form, (fam, _scale(prec, form, coarse, fam)), th)
        ratio = check_reference(tag, pb, o, form, prec, coarse, lf, fam, th, full, obj)
        _worst[tag] = (case, row, worst, ratio)
    _seen.update(instances())


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("form,flabel,prec,coarse,lf", [(f, *fl) for f, fl in CASES], ids=[f"{f}-{fl[0]}" for f, fl in CASES])
@pytest.mark.parametrize("name", PROBLEMS)
def test_pass_exact(handles, name, form, flabel, prec, coarse, lf):
    _ran.add((name, form, flabel))  # (registered first: a case that fails still counts as run, and the coverage test below then fails too)
    run_case(handles, name, form, flabel, prec, coarse, lf, FAMILIES)


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["i8x", "i8w"])
def test_tauovr_rerun(handles, prec):
    """Rescaled re-runs as the operator makes them (test_gpu_i8_pass_variants._run_rescaled): the dyn family leaves far more than 8 (i8w: 4)
    bits of the planes unused at the tau of its bound, so tau is imposed from the last pass's mmax until no row does.  A and B on
    the pass the loop ends on, as for any pass; its decidable share is printed, not capped (docstring, B): the re-runs move each
    row's largest sample to the top of the range."""
    name, form = "narrow-counts", "RISE"
    pb, p = prob(name), handle(handles, name)
    wide = prec == "i8w"
    th = _thetas(len(pb.nodes), pb.P, seed=pb.P)["dyn"]
    R_ = len(pb.nodes)
    mm_min = (1 << 27) if wide else (1 << 23)
    out = i8_pass(p, form, prec, pb.nodes, th)
    reruns = 0
    for _ in range(6):
        tau0, mm = out["s0"][:, 1], out["s0"][:, 2]
        if (mm >= mm_min).all():
            break
        ovr = np.where(mm < mm_min, (mm + 1.0) * MMAX_UNIT[wide] * tau0 * (1.0 + 1e-12) / VDIV[wide], 0.0)
        G0 = read_G(p)
        out = i8_pass(p, form, prec, pb.nodes, th, tauovr=ovr)
        reruns += 1
        tau = State(p).tau[:(R_ + 31) // 32 * 32].copy()
        assert (tau[:R_][mm < mm_min] < tau0[mm < mm_min]).all() and np.array_equal(tau[:R_][mm >= mm_min], tau0[mm >= mm_min])
    assert reruns >= 1 and (out["s0"][:, 2] >= mm_min).all(), (reruns, out["s0"][:, 2].min())
    st, ps = State(p), PassState(p)
    rows = model_rows(pb, prec, form, False, 5, st.theta[:R_], st.Qfp, st.cconst, tau)
    case, row = shares(pb, rows)
    tag = (name, form, prec, "tauovr")
    worst, nund = check_elements(tag, pb, ps, rows, False, True)
    print(f"tauovr re-run {prec} ({reruns} re-runs): decidable share {case:.4f} (worst row {row:.4f}), worst |device - model| {worst} units, "
          f"{nund} undecidable")
    check_behind_vq(tag, pb, ps, out, G0, tau, form, False, True, st.Qf, st.cconst)


@need_ld
@pytest.mark.gpu
def test_split_k_last_chunk_partial(handles):
    """Pairwise n = 40, K = 2049: Kp = 3072, plan kchunk = kpart = 2048 -- two split-K chunks, [0, 2048) and the partial [2048, 3072).
    The smallest K that gives it: Kp is K rounded up to 1024 and a chunk is never below 2048 samples, so Kp = 2048 is one chunk."""
    name = "splitk"
    pb, p = prob(name), handle(handles, name)
    th = _thetas(len(pb.nodes), pb.P, seed=pb.P)["dense"]
    vec = np.random.default_rng(19).normal(size=th.shape)
    plan = i8_pass(p, "RISE", "i8x", pb.nodes, th, vec=vec, hv=1, hv_lf=5, ksub=1)["plan"]  # (the plan comes back with a product pass)
    assert plan == (2048, 2048) and pb.Kp == 3072 and pb.Kp % plan[0] != 0 and -(-pb.Kp // plan[0]) == 2, (plan, pb.Kp)
    for form, (flabel, prec, coarse, lf) in [("RISE", OBJ_FORMS[2]), ("RISE", OBJ_FORMS[4])]:
        run_case(handles, name, form, flabel, prec, coarse, lf, ["dense"], variants=False)


@need_ld
@pytest.mark.gpu
def test_every_objective_instance_ran(handles):
    """the record of the matrix above (this file's tests, in order, in one process) holds every forward, backward and finalise
    instance an objective pass reaches below 32768 statistics columns, and no other"""
    if len(_ran) < len(PROBLEMS) * len(CASES):
        pytest.skip("needs the whole matrix of this file in the same session")
    want = set()
    for UNIW in (0, 1):
        for LF in (3, 4, 5):
            for FORM, WANTF in ((0, 0), (0, 1), (2, 1)):
                want.add(fwd_bit(LF, FORM, WANTF, 0, 0, UNIW))
        for WANTF in (0, 1):
            want.add(fwd_bit(4, 0, WANTF, 0, 1, UNIW))
            want.add(fwdw_bit(0, WANTF, 0, UNIW, 1))
        for FORM, WANTF in ((0, 0), (0, 1), (2, 1)):
            want.add(fwdw_bit(FORM, WANTF, 0, UNIW, 0))
    want |= {bwd_bit(6, 0), bwd_bit(3, 3), bwd_bit(3, 1), bwd_bit(4, 0), 304, 306, 307}
    hv = {fwd_bit(5, 3, 0, 0, 0, 0), 305}  # the product pass test_split_k_last_chunk_partial ran for its plan
    assert not (want - _seen), sorted(want - _seen)
    assert not (_seen - want - hv), sorted(_seen - want - hv)
    for tag in sorted(_worst):
        case, row, worst, ratio = _worst[tag]
        print(f"{' '.join(tag)}: decidable {case:.4f} / row {row:.4f}, worst |device - model| {worst}, against the 80-bit bound {ratio:.3g}")
