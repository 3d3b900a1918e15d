"""What the pack layer of the int8-limb passes leaves on the device (csrc/gml_i8_pack.hip, k_zero_pass, i8_pass), read back through
the test hook gml_test_i8_pack_state and held, bit for bit, to the host model tests/_i8_pack_reference.py: the three bit images
(Xb, Xtb, a tile's Xc), the digit planes of Theta (plain, and on signed column pairs), sigma / qconst / qconst2 / qpair, the marks
of the tiles that keep plain planes, the compact column lists -- and which of the fast paths a pass took.  The other int8 suites
show that the fast paths change no bit of f and G; a pass that silently swept every tile densely over all columns would pass them.

Every comparison is exact (np.array_equal on integers, bytes and bits) except tau, the one floating-point value: it is held to
B (1 + 1e-12) / vdiv formed in np.longdouble from the model's integer sum |q|, within TAU_ULPS = 4 ulp (the device's FP64 exp and
two roundings); each test prints measured / bound.  Every test first asserts, on the model's own prediction, that its case is not
vacuous (the marks hold a 0 and a 1, the step counts hold -1, 0, 1 and 2, ...).

Passes run through gml_test_i8_pass (one pass, no rescaled re-runs) unless a test says otherwise.  Pairwise handles: parameter i of
node u's row is column i, the field (i = u) is the constant column, so column u of the row is zero.

Edge entries (big = nextafter(0.125, 0): q = 2^54 - 2 at sigma = 2^-57), U = 0x01010101010101, a pair runs on seven digits inside
[-128 U, 127 U]:
  (a) +big, +big   alpha = 2^55 - 4 > 127 U: the tile keeps plain planes
  (b) +big, -big   alpha = 0, beta = 2^55 - 4: outside through the difference alone
  (c) -big, -big   alpha = -2^55 + 4 > -128 U: stays paired, digits [4, 0, 0, 0, 0, 0, -128]
  (d) q with q' = 127 U - 1 - q: the largest sum a pair of these rows can have inside (q' is even and below 2^54, so q' 2^-57 is an
      exact double); q' + 2 gives 127 U + 1, the smallest outside.  At sigma = 2^-57 with one entry at 2^54 - 2 every sum here is
      even and 127 U is odd: 127 U itself cannot be hit, its two sides can."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import _f64_pass_reference as F
import _i8_pack_reference as R
import gml_amd as gml
from oracle import oracle as O

_lib = importlib.import_module("gml_amd._lib")
pytestmark = pytest.mark.gpu
LD = np.longdouble
NO_COMPACT, NO_PAIRS = 6, 9  # gml_solver.h: GML_TUNE_NO_COMPACT, GML_TUNE_NO_PAIRS
TAU_ULPS = 4
FTOL = GTOL = 1e-12  # tests/test_gpu_i8w_pairs.py
BIG = float(np.nextafter(0.125, 0.0))
QBIG = 2 ** 54 - 2
_tau_worst = [0.0]


# ---------------------------------------------------------------------------------------------------------------------------
# the hooks
# ---------------------------------------------------------------------------------------------------------------------------
def _hooks():
    L = _lib.lib()
    v, i64 = C.c_void_p, C.c_int64
    L.gml_test_i8_pass.argtypes = [v, C.c_int, C.c_int, i64, v, v, v, v, i64, v, v, v, v, v, v]
    L.gml_test_i8_pack_state.argtypes = [v, i64, v, v]
    L.gml_test_tune.restype = C.c_double
    L.gml_test_tune.argtypes = [C.c_int, C.c_double]
    return L


def i8_pass(p, form, prec, nodes, theta, *, coarse=False, lf=0, want_grad=True, compact=True, vec=None, hv=0, hv_lf=5):
    L = _hooks()
    nodes = np.ascontiguousarray(nodes, dtype=np.int64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    Rn, P = theta.shape
    kn = np.array([coarse, lf, want_grad, compact, 0, hv, hv_lf, 1, 0, 0, 0], dtype=np.int64)
    f, g, h = np.zeros(Rn), np.zeros((Rn, P)), np.zeros((Rn, P))
    slots, plan = np.zeros((2, Rn, 3)), np.zeros(2, dtype=np.int64)
    vv = None if vec is None else np.ascontiguousarray(vec, dtype=np.float64)
    _lib.check(L.gml_test_i8_pass(p._h, _lib.FORMULATION_IDS[form], _lib.PRECISIONS[prec], Rn, _lib._ptr(nodes), _lib._ptr(theta), None,
                                  None if vv is None else _lib._ptr(vv), P, _lib._ptr(kn), _lib._ptr(f), _lib._ptr(g), _lib._ptr(h),
                                  _lib._ptr(slots), _lib._ptr(plan)))
    return f, g


class State:
    """the arrays of gml_test_i8_pack_state"""

    def __init__(self, p, xc_tile=0):
        L = _hooks()
        d = np.zeros(20, dtype=np.int64)
        _lib.check(L.gml_test_i8_pack_state(p._h, 0, _lib._ptr(d), None))
        (self.slots, self.lf_buf, self.lf, paired, compact, self.csteps, self.Qp, self.Qfp, self.Qf, self.cconst, self.Kp, self.K, tqb, xbb,
         xtbb, xcb, self.ws_rows, self.has_marks, self.hv_lf, _) = (int(x) for x in d)
        self.paired, self.compact = bool(paired), bool(compact)
        nt, cs = self.slots // 32, max(self.csteps, 0)
        self.tq = np.zeros(tqb, dtype=np.int8)
        self.tdense = np.full(nt, -7, dtype=np.int32)
        self.cnk = np.full(nt, -7, dtype=np.int32)
        self.cmap = np.full((nt, cs * 64), -7, dtype=np.int32)
        self.sigma, self.tau = np.zeros(self.slots), np.zeros(self.slots)
        self.qconst, self.qconst2, self.qpair = (np.zeros(self.slots, dtype=np.int64) for _ in range(3))
        self.theta = np.zeros((self.ws_rows, self.Qp))
        self.xb = np.zeros(xbb // 4, dtype=np.uint32)
        self.xtb = np.zeros(xtbb // 4, dtype=np.uint32)
        self.xc = np.zeros(xcb // 4, dtype=np.uint32)
        arrs = [self.tq, self.tdense, self.cnk, self.cmap, self.sigma, self.tau, self.qconst, self.qconst2, self.qpair, self.theta, self.xb,
                self.xtb, self.xc]
        ptrs = (C.c_void_p * 13)(*[a.ctypes.data if a.size else None for a in arrs])
        _lib.check(L.gml_test_i8_pack_state(p._h, int(xc_tile), _lib._ptr(d), ptrs))
        if self.lf:
            self.tq = self.tq.reshape(nt, self.Qfp // 64, self.lf, 32, 64)

    def row_image(self, slot, steps):
        """the bytes of a slot in its tile's image: int8 [steps][LF][64]"""
        return self.tq[slot // 32, :steps, :, slot % 32, :]


class tune:
    def __init__(self, knob, value=1.0):
        self.knob, self.value = knob, value

    def __enter__(self):
        _hooks().gml_test_tune(self.knob, self.value)

    def __exit__(self, *a):
        _hooks().gml_test_tune(self.knob, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# problems and rows
# ---------------------------------------------------------------------------------------------------------------------------
def _problem(n, K, weighted, seed, order=2):
    rng = np.random.default_rng(seed)
    spins = rng.choice(np.array([-1, 1], dtype=np.int8), size=(K, n))
    counts = 1.0 + (np.arange(K) % 3) if weighted else None
    return spins, counts


def _hist(spins, counts):
    c = np.ones(len(spins)) if counts is None else counts
    return np.concatenate([c[:, None], spins.astype(np.float64)], axis=1)


def _wmax(counts, K):
    c = np.ones(K) if counts is None else counts
    return float((c / c.sum()).max())


def internal(nodes, th, Qp, cconst):
    """pairwise rows in the internal column layout: parameter i is column i, the field of node u the constant column"""
    out = np.zeros((len(nodes), Qp))
    out[:, :th.shape[1]] = th
    for r, u in enumerate(nodes):
        out[r, cconst] = th[r, u]
        out[r, u] = 0.0
    return out


def _check_tau(st, slot, sc, wmax, form, planes_v):
    want = R.tau(sc["sabs"], sc["sx"], wmax, form, planes_v)
    err = abs(LD(st.tau[slot]) - want) / want
    ratio = float(err / (TAU_ULPS * LD(2.0) ** -52))
    _tau_worst[0] = max(_tau_worst[0], ratio)
    return ratio


def _report_tau(label):
    print(f"{label}: tau worst measured/bound = {_tau_worst[0]:.3g} (bound {TAU_ULPS} ulp)")
    worst, _tau_worst[0] = _tau_worst[0], 0.0
    assert worst <= 1.0, f"tau off by {worst:.3g} x {TAU_ULPS} ulp"


def check_pass(st, nrows, th_int, LF, *, pairs, compact, wmax, form, wide, what, rows=None, marks=True, images=True):
    """the state of the handle against the model's prediction of one objective pass over the slots 0 .. nrows with the
    internal-layout rows th_int; returns the prediction.  rows: the slots to compare (default: every active one)"""
    Rp = (nrows + 31) // 32 * 32
    assert st.lf == LF and st.paired == pairs and st.compact == compact, (what, st.lf, st.paired, st.compact)
    assert np.array_equal(st.theta[:nrows], th_int), (what, "the rows the pass read")
    theta = st.theta[:Rp]  # (inactive slots: whatever an earlier pass left there; the model must not look at them)
    active = np.arange(Rp) < nrows
    pred = R.predict_pass(theta, active, st.Qfp, st.cconst, LF, pairs, compact)
    for t in range(Rp // 32):
        if compact:
            assert st.csteps == pred["csteps"] > 0, (what, st.csteps)
            nk = pred["cnk"][t]
            assert st.cnk[t] == nk, (what, "cnk", t, int(st.cnk[t]), nk)
            if nk > 0:
                assert np.array_equal(st.cmap[t, :nk * 64], pred["cmap"][t]), (what, "cmap", t)
        if pairs and marks:
            assert st.tdense[t] == pred["mark"][t], (what, "mark", t, int(st.tdense[t]), pred["mark"][t])
    for s in (range(nrows) if rows is None else rows):
        sc, img = pred["scalars"][s], pred["image"][s]
        if images:
            got = st.row_image(s, img.shape[0])
            if not np.array_equal(got, img):
                dec = R.decode_image(np.ascontiguousarray(got), pred["paired"][s // 32])
                bad = np.argwhere(got != img)[:4].tolist()
                raise AssertionError((what, "digit planes of slot", s, "paired" if pred["paired"][s // 32] else "plain", "first [step, plane, byte]", bad,
                                      "decodes" if dec is not None else "does not decode"))
        assert st.sigma[s] == sc["sigma"], (what, "sigma", s, st.sigma[s], sc["sigma"])
        assert st.qconst[s] == sc["qconst"], (what, "qconst", s)
        if LF > 5:
            assert st.qconst2[s] == sc["qconst2"], (what, "qconst2", s)
            assert st.qpair[s] == sc["qpair"], (what, "qpair", s)
        _check_tau(st, s, sc, wmax, form, 6 if wide else 4)
    return pred


# ---------------------------------------------------------------------------------------------------------------------------
# 1. bit images
# ---------------------------------------------------------------------------------------------------------------------------
def test_bit_images_pairwise():
    """n = 128, K = 300 (Kp = 1024: padding samples), weighted counts; Xc of a compacted tile after an i8w pass"""
    n, K = 128, 300
    spins, counts = _problem(n, K, True, 31)
    rng = np.random.default_rng(32)
    with gml.Problem(spins=spins, counts=counts) as p:
        assert np.array_equal(p.spins(), spins)
        nodes = np.arange(96, 128, dtype=np.int64)
        th = np.zeros((32, n))
        cols = np.sort(rng.choice(96, size=37, replace=False))
        for r in range(32):
            th[r, cols] = rng.normal(scale=0.01, size=len(cols)) * (rng.random(len(cols)) < 0.6)
        th[0, cols] = 0.01
        i8_pass(p, "RISE", "i8w", nodes, th)
        st = State(p, xc_tile=0)
        assert (st.Kp, st.Qfp, st.Qf, st.K) == (1024, 128, 128, 300)
        B = R.stat_bits(spins, R.stat_keys(n, 2), st.Qfp, st.Kp)
        assert 0 < B[:, :K].mean() < 1 and not B[:, K:].any()
        assert np.array_equal(st.xb, R.xb_image(B, st.Kp, st.Qfp)), "Xb"
        assert np.array_equal(st.xtb, R.xtb_image(B, st.Kp, st.Qfp)), "Xtb"
        pred = check_pass(st, 32, internal(nodes, th, st.Qp, st.cconst), 7, pairs=True, compact=True, wmax=_wmax(counts, K), form="RISE",
                          wide=True, what="pairwise")
        assert pred["cnk"][0] == 1 and pred["cmap"][0][:37].tolist() == cols.tolist() and (pred["cmap"][0][37:] == -1).all()
        want = R.xc_image(B, st.Kp, 1, pred["cmap"][0])
        assert want.any() and np.array_equal(st.xc[:want.size], want), "Xc"
    _report_tau("bit images, pairwise")


def test_bit_images_order3():
    """n = 12, order 3: 12 + 66 = 78 statistics in two steps, keys with unused slots, 50 padding columns"""
    n, K = 12, 200
    spins, _ = _problem(n, K, False, 33)
    rng = np.random.default_rng(34)
    with gml.Problem(spins=spins, order=3) as p:
        assert p.P == 1 + 11 + 55
        nodes = np.array([0, 5, 11, 5], dtype=np.int64)
        th = rng.normal(scale=0.01, size=(4, p.P)) * (rng.random((4, p.P)) < 0.15)
        th[:, 0] = 0.02
        i8_pass(p, "RISE", "i8w", nodes, th)
        st = State(p, xc_tile=0)
        assert (st.Kp, st.Qfp, st.Qf) == (1024, 128, 78)
        keys = R.stat_keys(n, 3)
        assert (keys[:12, 1] == -1).all() and (keys[12:] >= 0).all()
        B = R.stat_bits(spins, keys, st.Qfp, st.Kp)
        assert B[:78, :K].any() and not B[78:].any()
        assert np.array_equal(st.xb, R.xb_image(B, st.Kp, st.Qfp)), "Xb"
        assert np.array_equal(st.xtb, R.xtb_image(B, st.Kp, st.Qfp)), "Xtb"
        # the rows as the pass read them: the same values, spread over the columns of each node
        for r in range(4):
            assert sorted(st.theta[r][st.theta[r] != 0].tolist()) == sorted(th[r][th[r] != 0].tolist())
            assert st.theta[r, st.cconst] == 0.02 and not st.theta[r, 78:128].any()
        pred = check_pass(st, 4, st.theta[:4].copy(), 7, pairs=True, compact=True, wmax=1.0 / K, form="RISE", wide=True, what="order 3")
        nk, cm = pred["cnk"][0], pred["cmap"][0]
        assert nk == 1 and 10 < (cm >= 0).sum() <= 64 and (cm < 78).all()
        want = R.xc_image(B, st.Kp, 1, cm)
        assert want.any() and np.array_equal(st.xc[:want.size], want), "Xc"
    _report_tau("bit images, order 3")


@pytest.mark.parametrize("name", F.HIGH)
def test_layout_keys_and_bit_images_orders_5_to_8(name):
    """The shapes H5 .. H8, E7, E3 of tests/_f64_pass_reference.py (orders 5 to 8; E7, E3: an order above n): P and every node's keys
    against the oracle's, then Sb, Xb and Xtb -- padding columns and padding samples included -- against the images of
    stat_bits over stat_keys (itertools.combinations by size): a statistic's bit is the XOR of up to seven rows of Sb."""
    sh = F.Shape(name, O.multi_keys)
    n, order = sh.n, sh.order
    with gml.Problem(spins=sh.spins, counts=sh.counts, order=order) as p:
        assert p.P == sh.P == len(O.multi_keys(n, order, 0))
        for u in range(n):
            ka = p.multi_keys_array(u)
            want = O.multi_keys(n, order, u)
            assert ka.shape == (sh.P, order)
            assert [tuple(int(v) for v in row if v >= 0) for row in ka] == want, (name, u)
            assert all((row[len(k):] == -1).all() and (row[:len(k)] >= 0).all() for row, k in zip(ka, want)), (name, u, "unused slots")
        assert np.array_equal(p.spins(), sh.spins)
        sb = np.zeros((n, sh.Kp // 32), dtype=np.uint32)
        neg = np.zeros((n, sh.Kp), dtype=np.uint32)
        neg[:, :sh.K] = sh.spins.T < 0
        for b in range(32):
            sb |= neg[:, b::32] << np.uint32(b)
        assert np.array_equal(p.sign_bits(), sb), "Sb"  # (bit b of word w: sample 32 w + b; the padding samples are zero bits)
        th = np.random.default_rng(50).normal(scale=0.01, size=(n, sh.P))
        i8_pass(p, "RISE", "i8w", np.arange(n, dtype=np.int64), th)
        st = State(p)
        assert (st.Kp, st.K, st.Qf, st.Qfp, st.cconst, st.Qp) == (sh.Kp, sh.K, sh.Qf, sh.Qfp, sh.cconst, sh.Qp)
        assert sh.keys.shape == (sh.Qf, order - 1) and (sh.keys[-1] >= 0).sum() == min(order - 1, n)
        B = R.stat_bits(sh.spins, sh.keys, st.Qfp, st.Kp)
        assert B[:sh.Qf, :sh.K].any(axis=1).all() and not B[sh.Qf:].any() and not B[:, sh.K:].any()
        assert np.array_equal(st.xb, R.xb_image(B, st.Kp, st.Qfp)), "Xb"
        assert np.array_equal(st.xtb, R.xtb_image(B, st.Kp, st.Qfp)), "Xtb"
        assert np.array_equal(st.theta[:n], sh.internal(th)), "the rows the pass read: gml_node_cols against the key lookup"


# ---------------------------------------------------------------------------------------------------------------------------
# 2. planes and scalars, plain
# ---------------------------------------------------------------------------------------------------------------------------
PLAIN_FORMS = [("i8x", 5, False, False), ("i8x", 4, False, False), ("i8x", 3, False, False), ("i8x", 0, True, False), ("i8w", 0, False, True),
               ("i8w", 0, True, False)]  # (precision, lf, coarse, GML_TUNE_NO_PAIRS)


@pytest.mark.parametrize("prec,lf,coarse,nopairs", PLAIN_FORMS)
def test_plain_planes_and_scalars(prec, lf, coarse, nopairs):
    """40 rows (a full tile and one with inactive rows), n = 128: normal rows, a wide one, an all-zero row, and a row whose 128 entries
    are all `big`: sum |theta| * 1.0000001 = 16.0000016 > 2^4, so seven planes take sigma = 2^-56 where max |theta| alone gives 2^-57
    (a pairwise row of 128 spins has no 129th entry; the sum is 1e-7 above the power of two, the device's rounding of it 1e-14)"""
    n, K = 128, 256
    spins, counts = _problem(n, K, True, 35)
    rng = np.random.default_rng(36)
    wide = prec == "i8w"
    LF = 7 if wide else (4 if coarse else lf)
    with gml.Problem(spins=spins, counts=counts) as p:
        nodes = np.arange(40, dtype=np.int64)
        th = rng.normal(scale=0.02, size=(40, n))
        th[4] = 0.0
        th[6] = BIG
        th[35] = rng.normal(scale=0.5, size=n)
        with tune(NO_PAIRS, 1.0 if nopairs else 0.0):
            i8_pass(p, "RISE", prec, nodes, th, coarse=coarse, lf=lf, compact=False)
        st = State(p)
        ti = internal(nodes, th, st.Qp, st.cconst)
        sx6, margin = R.sigma_exponent(ti[6], st.Qfp, st.cconst, LF)
        assert sx6 == (-56 if wide else -3 - (8 * LF - 2)) and (margin > 1e-8 or not wide), (sx6, margin)
        assert R.sigma_exponent(ti[4], st.Qfp, st.cconst, LF)[0] == -(8 * LF - 2)
        check_pass(st, 40, ti, LF, pairs=False, compact=False, wmax=_wmax(counts, K), form="RISE", wide=wide, what=(prec, lf, coarse))
        assert st.hv_lf == 0 and (st.has_marks == 1) == wide
    _report_tau(f"plain planes {prec} lf={lf} coarse={coarse}")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. planes and marks, paired
# ---------------------------------------------------------------------------------------------------------------------------
def _pair_cols(step, h, m):
    return 64 * step + R.pair_col(h, m, 0), 64 * step + R.pair_col(h, m, 1)


A_COLS = _pair_cols(2, 1, 5)  # case (a): lane half 1, pair 5, third step
QD = R.PAIR_MAX - 1 - QBIG     # case (d)


def _edge(th, row, case):
    if case == "a":
        th[row, list(A_COLS)] = BIG
    elif case == "b":
        c0, c1 = _pair_cols(1, 0, 15)
        th[row, c0], th[row, c1] = BIG, -BIG
    elif case == "c":
        th[row, list(_pair_cols(0, 1, 0))] = -BIG
    else:
        c0, c1 = _pair_cols(2, 0, 7)
        qd = QD + (2 if case == "d_out" else 0)
        th[row, c0], th[row, c1] = BIG, math.ldexp(float(qd), -57)
        assert qd % 2 == 0 and qd < 2 ** 54 and int(math.ldexp(th[row, c1], 57)) == qd


PAIRED_CASES = {"a+c+d_in": ([(3, "c"), (5, "d_in"), (40, "a")], [0, 1]), "b": ([(7, "b"), (33, "c"), (34, "d_in")], [1, 0]),
                "d_out": ([(9, "d_out")], [1, 0])}


@pytest.mark.parametrize("case", list(PAIRED_CASES))
def test_paired_planes_and_marks(case):
    """i8w, RISE and RPLE, n = 192 (three steps), 64 rows on a background of normal(0.001): the marks per tile, every row's image
    (alpha, beta per pair in unmarked tiles, plain digits in marked ones), the scalars, and f, G of the rows with the edge entries"""
    n, K = 192, 256
    spins, counts = _problem(n, K, True, 37)
    s = _hist(spins, counts)
    rng = np.random.default_rng(38)
    assert A_COLS == (153, 157) and R.pair_in_range(QBIG, QD) and not R.pair_in_range(QBIG, QD + 2) and QBIG + QD == R.PAIR_MAX - 1
    assert R.balanced_digits(-2 * QBIG, 7)[0] == [4, 0, 0, 0, 0, 0, -128]
    places, marks = PAIRED_CASES[case]
    with gml.Problem(spins=spins, counts=counts) as p:
        nodes = np.arange(64, dtype=np.int64)
        th = rng.normal(scale=0.001, size=(64, n))
        for row, c in places:
            _edge(th, row, c)
        for form in ("RISE", "RPLE"):
            f, g = i8_pass(p, form, "i8w", nodes, th, compact=False)
            st = State(p)
            ti = internal(nodes, th, st.Qp, st.cconst)
            active = np.ones(64, dtype=bool)
            pred = R.predict_pass(ti, active, st.Qfp, st.cconst, 7, True, False)
            assert [pred["mark"][0], pred["mark"][1]] == marks, (case, pred["mark"])  # a 0 and a 1
            for row, _ in places:
                assert pred["scalars"][row]["sx"] == -57
            check_pass(st, 64, ti, 7, pairs=True, compact=False, wmax=_wmax(counts, K), form=form, wide=True, what=(case, form))
            for row, _ in places:
                f0, g0 = O.objgrad_pair(s, form, int(nodes[row]), th[row])
                assert f[row] == pytest.approx(f0, rel=FTOL, abs=FTOL), (case, form, row)
                np.testing.assert_allclose(g[row], g0, rtol=1e-10, atol=GTOL)
    _report_tau(f"paired planes {case}")


def test_edge_pair_in_an_inactive_row_marks_nothing():
    """(e) 64 rows with case (a) in row 50 mark the second tile; a pass over the first 40 rows then finds row 50 still in the workspace
    of Theta, in a slot it does not list: the tile runs on pairs"""
    n, K = 192, 256
    spins, counts = _problem(n, K, False, 39)
    rng = np.random.default_rng(40)
    with gml.Problem(spins=spins, counts=counts) as p:
        nodes = np.arange(64, dtype=np.int64)
        th = rng.normal(scale=0.001, size=(64, n))
        _edge(th, 50, "a")
        i8_pass(p, "RISE", "i8w", nodes, th, compact=False)
        st = State(p)
        ti = internal(nodes, th, st.Qp, st.cconst)
        pred = check_pass(st, 64, ti, 7, pairs=True, compact=False, wmax=1.0 / K, form="RISE", wide=True, what="64 rows")
        assert pred["mark"] == {0: 0, 1: 1}
        i8_pass(p, "RISE", "i8w", nodes[:40], th[:40], compact=False)
        st = State(p)
        assert np.array_equal(st.theta[50], ti[50]) and st.theta[50, A_COLS[0]] == BIG  # the entry is still there
        assert R.tile_marked(st.theta[32:64], [True] * 32, st.Qfp, st.cconst)  # (it would mark the tile if row 50 counted)
        pred = check_pass(st, 40, ti[:40], 7, pairs=True, compact=False, wmax=1.0 / K, form="RISE", wide=True, what="40 rows")
        assert pred["mark"] == {0: 0, 1: 0} and pred["paired"][1]
    _report_tau("inactive edge row")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. compaction lists
# ---------------------------------------------------------------------------------------------------------------------------
def _compaction_rows(rng, n, sizes):
    """32 rows per entry of sizes, non-zero on exactly that many columns between them (row 0 of a tile on all of them).  The columns of
    the first tile: 5 in each of the 8 (256-column block, wave) ranges of k_col_union."""
    th = np.zeros((32 * len(sizes), n))
    lists = []
    for t, size in enumerate(sizes):
        if t == 0:
            cols = np.concatenate([64 * w + rng.choice(62, size=size // 8, replace=False) for w in range(8)])
        else:
            cols = rng.choice(n - 2, size=size, replace=False)
        cols = np.sort(cols)
        lists.append(cols)
        for r in range(32):
            keep = rng.random(size) < 0.4
            th[32 * t + r, cols[keep]] = rng.normal(scale=0.01, size=int(keep.sum()))
        th[32 * t, cols] = 0.01
    return th, lists


def test_compaction_lists():
    """n = 512 (8 steps: capacity 2 steps = 128 columns), K = 256, 160 rows in five tiles with unions of 40, exactly 64, 100, exactly
    128 and 129 columns; then a tile of all-zero rows; then case (a) on two neighbours of a tile's list that are no neighbours on the
    column grid.  The rows belong to the nodes 510 and 511, so that the columns 0 .. 509 are free."""
    n, K = 512, 256
    spins, counts = _problem(n, K, False, 41)
    rng = np.random.default_rng(42)
    L = _hooks()
    with gml.Problem(spins=spins, counts=counts) as p:
        nodes = np.array([510 + (r & 1) for r in range(160)], dtype=np.int64)
        th, lists = _compaction_rows(rng, n, [40, 64, 100, 128, 129])
        kw = dict(pairs=True, compact=True, wmax=1.0 / K, form="RISE", wide=True)
        i8_pass(p, "RISE", "i8w", nodes, th)
        st = State(p)
        assert st.Qfp == 512 and R.compact_steps(st.Qfp) == 2
        ti = internal(nodes, th, st.Qp, st.cconst)
        pred = check_pass(st, 160, ti, 7, what="five unions", **kw)
        assert [pred["cnk"][t] for t in range(5)] == [1, 1, 2, 2, -1]
        assert {(c // 256, (c % 256) // 64) for c in lists[0]} == {(b, w) for b in range(2) for w in range(4)}
        assert (pred["cmap"][1] >= 0).all() and (pred["cmap"][3] >= 0).all() and (pred["cmap"][2][100:] == -1).all() and len(pred["cmap"][2]) == 128
        assert not any(pred["mark"].values()) and pred["paired"][0]  # compacted tiles on pairs: their images decode through the lists
        # a tile of all-zero rows: an empty list
        th2 = th.copy()
        th2[32:64] = 0.0
        i8_pass(p, "RISE", "i8w", nodes, th2)
        st = State(p)
        pred = check_pass(st, 160, internal(nodes, th2, st.Qp, st.cconst), 7, what="a zero tile", **kw)
        assert sorted({pred["cnk"][t] for t in range(5)}) == [-1, 0, 1, 2]
        # case (a) on the first and the fifth column of the first tile's list (positions 0 and 4 pair in a step; on the grid their
        # columns pair with others)
        th3 = th.copy()
        c0, c1 = int(lists[0][0]), int(lists[0][4])
        assert (R.pair_col(0, 0, 0), R.pair_col(0, 0, 1)) == (0, 4) and c1 - c0 != 4
        th3[2, [c0, c1]] = BIG
        i8_pass(p, "RISE", "i8w", nodes, th3)
        st = State(p)
        ti3 = internal(nodes, th3, st.Qp, st.cconst)
        pred = check_pass(st, 160, ti3, 7, what="neighbours of the list", **kw)
        assert pred["mark"][0] == 1 and not R.tile_marked(ti3[:32], [True] * 32, st.Qfp, st.cconst, None)
        assert [pred["mark"][t] for t in range(1, 5)] == [0, 0, 0, 0]
        # the same pass told not to compact; and the public path under GML_TUNE_NO_COMPACT
        i8_pass(p, "RISE", "i8w", nodes, th3, compact=False)
        st = State(p)
        pred = check_pass(st, 160, ti3, 7, what="not compacted", **dict(kw, compact=False))
        assert not any(pred["mark"].values())
        with tune(NO_COMPACT):
            p.objgrad("RISE", nodes, th, precision="i8w")
            assert not State(p).compact
        p.objgrad("RISE", nodes, th, precision="i8w")
        assert State(p).compact
        assert L.gml_test_tune(NO_COMPACT, 0.0) == 0.0
    _report_tau("compaction lists")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the public path takes the fast paths
# ---------------------------------------------------------------------------------------------------------------------------
def test_public_objgrad_takes_the_fast_paths():
    """Problem.objgrad at precision i8w on sparse rows with sum |theta| < 1 (uniform counts: the largest weight then stays within
    e^-2 of its bound and no row is re-run): paired, compacted, no tile marked, every tile on a list"""
    n, K = 192, 256
    spins, counts = _problem(n, K, False, 43)
    rng = np.random.default_rng(44)
    with gml.Problem(spins=spins, counts=counts) as p:
        nodes = np.arange(128, 192, dtype=np.int64)
        th = np.zeros((64, n))
        for t, size in enumerate((30, 64)):
            cols = rng.choice(128, size=size, replace=False)
            for r in range(32):
                keep = rng.random(size) < 0.3
                th[32 * t + r, cols[keep]] = rng.normal(scale=0.02, size=int(keep.sum()))
            th[32 * t, cols] = 0.005
        assert np.abs(th).sum(axis=1).max() < 1
        kw = dict(wmax=1.0 / K, form="RISE", wide=True)
        p.objgrad("RISE", nodes, th, precision="i8w")
        st = State(p)
        ti = internal(nodes, th, st.Qp, st.cconst)
        pred = check_pass(st, 64, ti, 7, pairs=True, compact=True, what="public", **kw)  # (tau at its bound: no row was re-run)
        assert pred["cnk"] == {0: 1, 1: 1} and pred["mark"] == {0: 0, 1: 0}
        assert (st.tdense[:2] == 0).all() and (st.cnk[:2] == 1).all()
        with tune(NO_PAIRS):
            p.objgrad("RISE", nodes, th, precision="i8w")
            check_pass(State(p), 64, ti, 7, pairs=False, compact=True, what="public, no pairs", **kw)
        with tune(NO_COMPACT):
            p.objgrad("RISE", nodes, th, precision="i8w")
            check_pass(State(p), 64, ti, 7, pairs=True, compact=False, what="public, no compaction", **kw)
        p.objgrad("RISE", nodes, th, precision="i8w")
        check_pass(State(p), 64, ti, 7, pairs=True, compact=True, what="public again", **kw)
    _report_tau("public path")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. sequences on one handle
# ---------------------------------------------------------------------------------------------------------------------------
def test_sequence_on_one_handle():
    n, K = 192, 256
    spins, counts = _problem(n, K, False, 45)
    rng = np.random.default_rng(46)
    with gml.Problem(spins=spins, counts=counts) as p:
        nodes = np.arange(64, dtype=np.int64)
        clean = rng.normal(scale=0.001, size=(64, n))
        edge = clean.copy()
        _edge(edge, 40, "a")
        kw = dict(compact=False, wmax=1.0 / K, form="RISE", wide=True)
        run = lambda th, **k: i8_pass(p, "RISE", "i8w", nodes[:len(th)], th, compact=False, **k)  # noqa: E731
        # a paired pass with a marked tile
        run(edge)
        st = State(p)
        ti_edge, ti_clean = internal(nodes, edge, st.Qp, st.cconst), internal(nodes, clean, st.Qp, st.cconst)
        pred = check_pass(st, 64, ti_edge, 7, pairs=True, what="1 marked", **kw)
        assert pred["mark"] == {0: 0, 1: 1}
        # the same rows without the entry: the mark is gone, the planes are on pairs
        run(clean)
        pred = check_pass(State(p), 64, ti_clean, 7, pairs=True, what="2 entry removed", **kw)
        assert pred["mark"] == {0: 0, 1: 0} and pred["paired"][1]
        # a coarse pass: plain planes (it reads the top four), the marks stay what they were
        run(edge, coarse=True)
        st = State(p)
        check_pass(st, 64, ti_edge, 7, pairs=False, what="3 coarse", **kw)
        assert (st.tdense[:2] == 0).all()
        # an objective pass and a Hessian-vector pass behind it: the objective pass pairs and marks; the product pass quantises its
        # directions into five plain planes of the same buffer and leaves the marks and the scalars of the objective pass alone
        vec = rng.normal(size=(64, n)) * (rng.random((64, n)) < 0.3)
        run(edge, vec=vec, hv=1, hv_lf=5)
        st = State(p)
        assert st.hv_lf == 5 and np.array_equal(st.theta[:64], internal(nodes, vec, st.Qp, st.cconst))
        st.theta[:64] = ti_edge  # (the workspace holds the directions now; the objective pass read these)
        pred = check_pass(st, 64, ti_edge, 7, pairs=True, what="4 products", images=False, **kw)
        assert pred["mark"] == {0: 0, 1: 1}
        tq5 = st.tq.reshape(-1)[:st.slots * 5 * st.Qfp].reshape(st.slots // 32, st.Qfp // 64, 5, 32, 64)
        tv = internal(nodes, vec, st.Qp, st.cconst)
        for r in (0, 31, 40, 63):
            assert np.array_equal(tq5[r // 32, :, :, r % 32, :], R.row_image(tv[r], st.Qfp, st.cconst, 5, False)), ("direction planes", r)
        # a paired pass again
        run(clean)
        pred = check_pass(State(p), 64, ti_clean, 7, pairs=True, what="5 paired again", **kw)
        assert pred["mark"] == {0: 0, 1: 0}
        # every tile forced dense
        run(edge)
        with tune(NO_PAIRS):
            run(clean)
            st = State(p)
            check_pass(st, 64, ti_clean, 7, pairs=False, what="6 no pairs", **kw)
            assert st.tdense[:2].tolist() == [0, 1]  # (what the pass before left: nothing reads or clears them now)
        # a pass over the first 32 rows only: the other tile's mark, image and scalars are untouched
        run(edge)
        before = State(p)
        assert before.tdense[:2].tolist() == [0, 1]
        other = rng.normal(scale=0.002, size=(32, n))
        run(other)
        st = State(p)
        check_pass(st, 32, internal(nodes[:32], other, st.Qp, st.cconst), 7, pairs=True, what="7 first tile only", **kw)
        assert st.tdense[:2].tolist() == [0, 1] and np.array_equal(st.tq[1], before.tq[1]) and not np.array_equal(st.tq[0], before.tq[0])
        for a in ("sigma", "tau", "qconst", "qconst2", "qpair"):
            assert np.array_equal(getattr(st, a)[32:64], getattr(before, a)[32:64]), a
        assert np.array_equal(st.theta[32:64], ti_edge[32:64])
    _report_tau("sequence")


def test_rescaled_rerun_leaves_the_marked_row_out():
    """The public objgrad on one tile: row 10 holds case (a) on the background of normal(0.001), the 31 others are normal(0.05).  The
    first pass marks the tile; its largest weights leave more than four bits of the 31 rows' planes unused (mmax < 2^27), so they
    are re-run with a tighter tau -- a pass that does not list row 10, pairs, and marks nothing.  f and G of the rows 9, 10, 11: the
    oracle, and the bits of the same call with every tile forced dense."""
    n, K = 192, 256
    spins, counts = _problem(n, K, True, 47)
    s = _hist(spins, counts)
    rng = np.random.default_rng(48)
    with gml.Problem(spins=spins, counts=counts) as p:
        nodes = np.arange(32, dtype=np.int64)
        th = rng.normal(scale=0.05, size=(32, n))
        th[10] = rng.normal(scale=0.001, size=n)
        _edge(th, 10, "a")
        res = []
        for dense in (1, 0):
            with tune(NO_PAIRS, float(dense)):
                res.append(p.objgrad("RISE", nodes, th, precision="i8w"))
        (fd, gd), (f, g) = res
        for x, y in ((f, fd), (g, gd)):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        for r in (9, 10, 11):
            f0, g0 = O.objgrad_pair(s, "RISE", r, th[r])
            assert f[r] == pytest.approx(f0, rel=FTOL, abs=FTOL)
            np.testing.assert_allclose(g[r], g0, rtol=1e-10, atol=GTOL)
        st = State(p)
        ti = internal(nodes, th, st.Qp, st.cconst)
        assert st.lf == 7 and st.paired and np.array_equal(st.theta[:32], ti)
        wmax = _wmax(counts, K)
        rerun = []
        for r in range(32):
            sc = R.row_scalars(ti[r], st.Qfp, st.cconst, 7)
            bound = float(R.tau(sc["sabs"], sc["sx"], wmax, "RISE", 6))
            assert st.tau[r] <= bound * (1 + 1e-14)
            if st.tau[r] < bound * (1 - 1e-6):
                rerun.append(r)
            assert st.sigma[r] == sc["sigma"] and st.qconst[r] == sc["qconst"] and st.qpair[r] == sc["qpair"]
        assert 10 not in rerun and {9, 11} <= set(rerun), rerun  # row 10 kept the tau of its bound: it ran once
        # the last pass listed the re-run rows only: it cleared the mark and wrote their planes on pairs; the others keep the plain
        # planes of the first pass, which row 10 had marked
        assert R.tile_marked(ti, [True] * 32, st.Qfp, st.cconst) and not R.tile_marked(ti, [r in rerun for r in range(32)], st.Qfp, st.cconst)
        assert st.tdense[0] == 0
        nk = st.Qfp // 64
        for r in range(32):
            want = R.row_image(ti[r], st.Qfp, st.cconst, 7, r in rerun)
            assert np.array_equal(st.row_image(r, nk), want), ("planes of row", r, "paired" if r in rerun else "plain")
