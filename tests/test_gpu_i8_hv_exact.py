"""The Hessian-vector (product) pass of the int8-limb GEMM kernels -- k_quant_theta with hv != 0, the HV branches of k_fwd_i8<LF, 3 or 4>,
k_bwd_i8<1, 2> and <1, 4> on Uq, k_finalize_i8 with hv -- cut at the limb planes Uq of the products and held on both sides to the host
model tests/_i8_hv_reference.py (itself held to brute force by tests/test_host_i8_hv_reference.py).  This is the inner loop of the
matrix-free Newton-CG (Solver::newton_cg_group).  Products run through the two runners that exist, gml_test_i8_pass (any form, hv, lf and
plan; as gml_test_i8_pass_vslot it takes a slot map: product row i reads the V planes and tau of slot vslot[i]) and gml_test_hv_sparse
(caller-given vslot, exp forms; its GEMM side runs hv = 2, lf = 2); Uq, the product pass's slot scalars and
the Tq image of the directions come back through gml_test_i8_uq, the V planes the products read through gml_test_i8_pass_state, the
accumulators, G and f through gml_test_i8_gacc.  All of them only copy.

A.  The direction: sigma, tau_hv, invtau and qconst of every product row are the model's, bit for bit (tau_hv from the tau the objective
    pass reported for the slot vmap[r], times vscale, times pn), and the Tq image is the model's byte for byte.  The model's invtau is
    numpy's 1 / pn: a difference would be a finding (none was seen: the assertion is on the bits).
B.  Uq, element by element, EXACTLY: hh_k from the device's own V planes of slot vmap[r] (all four planes of an i8x image, planes 2 .. 5 of
    an i8w image), x_k . p exact from the integers of the quantised direction, y = hh fl(x_k . p invtau) + d(node, k) evaluated exactly
    and rounded twice as the device rounds it (the fma to float64, then to an integer, ties to even).  RPLE's hh goes through a
    multiply, a divide, a subtract and a multiply in float64, reproduced one by one.  No element is allowed a unit: the comparison
    is np.array_equal on every participating sample of every product row.  Participating padding samples and samples of count zero have
    all four digits zero; the bytes of the samples outside the part equal what the previous product left there.  hv = 2: |u| <= 32639
    and the planes 2, 3 are zero on the part (the claim behind the factor 1.01).
C.  Behind Uq, given the device's own planes: csum = sum u over the part, asum = 0, mmax = 0; every Gacc entry is the model's sum_k u_l b
    over the part, int32 for int32 -- all four planes for hv = 1, the planes 0 and 1 for hv = 2 with the planes 2 and 3 exactly zero; G is
    the model's float64 bit for bit over all Qp columns (tau (csum - 2 sum 256^l Gacc_l) below Qf, tau csum at the constant column,
    zeros elsewhere); the workspace's f keeps the objective pass's bits.
D.  End to end the products also meet the product bound of tests/test_gpu_i8_pass_variants.py against its 80-bit reference (Ref) on
    the same inputs, so an exact match with a wrong model cannot pass; and gml_test_i8_instances shows that every product instance
    reachable below 32768 statistics columns ran here.

Shapes (the smallest that reach the code; all used by tests/test_gpu_i8_pass_exact.py or tests/test_gpu_hv_sparse_direct.py already):
  splitk   pairwise n = 40, K = 2049: Kp = 3072, Qfp = 64 (one column step), 40 rows (two node tiles, the second partial), full plan
           (2048, 2048): two split-K chunks, the last partial; sub-sampled plans (2048, 1024), (2048, 256)
  narrow   pairwise n = 97, K = 9000: Kp = 9216, Qfp = 128, rows _rows(97, 45, 1); once with counts (3 % zero) and once with uniform
           counts (the UNIW instances and the padding guard of FORM 4); plans full, (2048, 256), (4096, 512) and (4096, 2048), whose third
           chunk [8192, 9216) is shorter than kpart
  order3   n = 20, K = 4099: Kp = 5120, Qf = 210, Qfp = 256 (46 padding columns), rows _rows(20, 45, 3); directions with entries on the
           last statistics columns, next to the padding
Directions of one pass, by row: dense normal; the node's field alone (rows 1, 33); two entries (row 2); largest entry a power of two
(row 4); all zeros (rows 5, 34: the pn = 1 fallback).
The matrix is a cover, not a full product: test_product_exact runs every (shape, form, source image, hv, lf) with the full plan and ONE
sub-sampled plan each, rotated through the shape's plans by the case's index; every plan of a shape runs at (2, 2) in
test_every_plan_at_the_default.  The slot map that is no identity runs RPLE and RISE at (2, 2), (1, 5) and (1, 3) on every pairwise shape and
both source images (test_slot_map), and the exp forms once more through gml_test_hv_sparse."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _i8_hv_reference as H
import _i8_pack_reference as R
import _i8_pass_reference as M
import gml_amd as gml
from test_gpu_hv_sparse_direct import hv_two_ways
from test_gpu_i8_pack_state import State
from test_gpu_i8_pass_exact import Prob, _same_bits
from test_gpu_i8_pass_variants import Ref, _counts, _rows, _thetas, bwd_bit, fwd_bit, i8_pass, instances, need_ld, quant_defect

_lib = importlib.import_module("gml_amd._lib")
HVLF = [(2, 2), (1, 2), (1, 3), (1, 4), (1, 5), (2, 5)]  # (2, 2): the solver's default
PLANS = {"splitk": [(2048, 1024), (2048, 256)], "narrow-counts": [(2048, 256), (4096, 512), (4096, 2048)],
         "narrow-uniform": [(2048, 256), (4096, 512), (4096, 2048)], "order3": [(2048, 256), (4096, 512)]}
VPL0 = {4: 0, 6: 2}
VSCALE = {4: 1.0, 6: 65536.0}


# ---------------------------------------------------------------------------------------------------------------------------
# problems, on the host
# ---------------------------------------------------------------------------------------------------------------------------
class HvProb(Prob):
    def __init__(self, name):
        if name == "order3":
            Prob.__init__(self, name)
            return
        self.name = name
        if name == "splitk":
            self.n, self.K, self.order, seed = 40, 2049, 2, 17
            self.counts, self.nodes = _counts(self.K, 18), _rows(40, 40, 5)
        else:
            self.n, self.K, self.order, seed = 97, 9000, 2, 7
            self.counts, self.nodes = (None if name.endswith("uniform") else _counts(self.K, 8)), _rows(97, 45, 1)
        rng = np.random.default_rng(seed)
        n = self.n
        self.spins = np.where(rng.random((self.K, n)) < 0.55, 1, -1).astype(np.int8)
        self.Kp = (self.K + 1023) // 1024 * 1024
        self.keys = R.stat_keys(n, 2)
        self.Qf = len(self.keys)
        c = np.ones(self.K) if self.counts is None else self.counts
        self.w = np.zeros(self.Kp)
        self.w[:self.K] = c / c.sum()
        self.wmax = float(self.w.max())
        self.colidx = {tuple(int(i) for i in k if i >= 0): c for c, k in enumerate(self.keys)}
        self.pkeys, self.P = None, n
        self._bits = {}
        self.sb = np.zeros((n, self.Kp), dtype=np.uint8)
        self.sb[:, :self.K] = (self.spins.T < 0)

    def field(self, r):
        """the parameter of row r that is the node's own field"""
        u = int(self.nodes[r])
        return u if self.order == 2 else [len(k) for k in self.pkeys[u]].index(1)

    def last_columns(self, r):
        """parameters of row r on the last statistics columns (next to the padding columns of the last step)"""
        u = int(self.nodes[r])
        if self.order == 2:
            return [self.n - 1 if u != self.n - 1 else self.n - 2]
        cols = [self.column(u, k) for k in self.pkeys[u]]
        return [int(i) for i in np.argsort(cols)[-3:]]

    def directions(self, seed):
        R_, P = len(self.nodes), self.P
        rng = np.random.default_rng(seed)
        v = rng.normal(size=(R_, P))
        for r in (1, 33):
            v[r] = 0.0
            v[r, self.field(r)] = rng.normal()
        v[2] = 0.0
        v[2, [self.field(2), self.last_columns(2)[0]]] = rng.normal(size=2)
        v[4] = np.clip(0.2 * v[4], -0.49, 0.49)
        v[4, self.last_columns(4)[-1]] = -0.5  # frexp gives 0.5 x 2^0: the largest entry is a power of two
        v[[5, 34]] = 0.0
        return v


_probs = {}


def prob(name):
    if name not in _probs:
        _probs[name] = HvProb(name)
    return _probs[name]


# ---------------------------------------------------------------------------------------------------------------------------
# hooks
# ---------------------------------------------------------------------------------------------------------------------------
def _hooks():
    L = _lib.lib()
    v = C.c_void_p
    L.gml_test_i8_uq.argtypes = [v, v, v]
    L.gml_test_i8_pass_state.argtypes = [v, v, v, v, v, v]
    L.gml_test_i8_gacc.argtypes = [v, v, v, v, v]
    return L


class UqState:
    """gml_test_i8_uq, and -- through the hooks of the objective pass -- the V planes, sc[0].tau, the accumulators, G and f"""

    def __init__(self, p):
        L = _hooks()
        d = np.zeros(8, dtype=np.int64)
        _lib.check(L.gml_test_i8_uq(p._h, _lib._ptr(d), None))
        self.slots, lb, self.Kp, self.K, self.lf, self.Qfp, tqb, self.has_uq = (int(x) for x in d)
        assert lb == H.LB and self.has_uq == 1
        ns = self.slots
        self.uq = np.zeros(ns * lb * self.Kp, dtype=np.int8)
        self.sigma, self.tau, self.invtau = np.zeros(ns), np.zeros(ns), np.zeros(ns)
        self.qconst, self.csum, self.asum = (np.zeros(ns, dtype=np.int64) for _ in range(3))
        self.mmax = np.zeros(ns, dtype=np.uint32)
        tq = np.zeros(tqb, dtype=np.int8)
        arrs = [self.uq, self.sigma, self.tau, self.invtau, self.qconst, self.csum, self.asum, self.mmax, tq]
        ptrs = (C.c_void_p * 9)(*[a.ctypes.data if a.size else None for a in arrs])
        _lib.check(L.gml_test_i8_uq(p._h, _lib._ptr(d), ptrs))
        self.planes = M.unpack_vq(self.uq, ns, self.Kp, lb)
        self.tq = tq.reshape(ns // 32, self.Qfp // 64, self.lf, 32, 64) if self.lf else None
        # the V planes of the last objective pass
        slots, planes, kp = C.c_int64(0), C.c_int(0), C.c_int64(0)
        _lib.check(L.gml_test_i8_pass_state(p._h, C.byref(slots), C.byref(planes), C.byref(kp), None, None))
        self.lbt = int(planes.value)
        vq = np.zeros(ns * self.lbt * self.Kp, dtype=np.int8)
        sums = np.zeros((5, ns), dtype=np.int64)  # (the hook copies both or neither; the objective pass's sums are not this file's subject)
        _lib.check(L.gml_test_i8_pass_state(p._h, C.byref(slots), C.byref(planes), C.byref(kp), _lib._ptr(vq), _lib._ptr(sums)))
        self.vplanes = M.unpack_vq(vq, ns, self.Kp, self.lbt)
        # accumulators (a product pass lays them out in four planes per slot whatever the workspace's images hold), G, f
        g8 = np.zeros(8, dtype=np.int64)
        _lib.check(L.gml_test_i8_gacc(p._h, _lib._ptr(g8), None, None, None))
        gplanes, stride, qfp, gslots, glbt, self.ws_rows, self.Qp, _ = (int(x) for x in g8)
        assert gplanes == 1 and qfp == self.Qfp and gslots == ns and glbt == self.lbt
        g = np.zeros(gplanes * stride, dtype=np.int32)
        self.G, self.F = np.zeros((self.ws_rows, self.Qp)), np.zeros(self.ws_rows)
        _lib.check(L.gml_test_i8_gacc(p._h, _lib._ptr(g8), _lib._ptr(g), _lib._ptr(self.G), _lib._ptr(self.F)))
        self.gacc = M.gacc_rows(g[:ns * lb * self.Qfp], ns, lb, self.Qfp)


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


_seen = set()
_ran = set()
_worst = {}
_refs = {}
_near = [0, 0]  # elements the model evaluated in rational arithmetic, of all


def theta_of(pb):
    return _thetas(len(pb.nodes), pb.P, seed=pb.P)["dense"]


def reference(p, pb, form, vkey, vec):
    """Ref's sums over every plan of the problem, once per (problem, form, direction set)"""
    key = (pb.name, form, vkey)
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
        keep = [(pb.Kp, pb.Kp)] + PLANS[pb.name]
        _refs[key] = (keep, ref.run(pb.nodes, [dict(form=form, theta=theta_of(pb), vec=vec, keep=keep)])[0])
    return _refs[key]


# ---------------------------------------------------------------------------------------------------------------------------
# the checks of one product pass
# ---------------------------------------------------------------------------------------------------------------------------
def check_product(tag, pb, us, form, hv, lf, plan, rows_int, nodes, vmap, tau_v, prev_planes, G_dev, G_before=None):
    """us: UqState after the pass; rows_int [R][Qp]: the directions in the internal layout; nodes, vmap [R]: the node and the source
    slot of every product row; tau_v [slots]: sc[0].tau; prev_planes: Uq as the previous product left it (None: not compared);
    G_dev [R][Qp]: the products as the pass wrote them.  Returns the model's u [R][Kp] on the part."""
    R_ = len(nodes)
    Rp = (R_ + 31) // 32 * 32
    Qfp, Kp = us.Qfp, us.Kp
    cconst, Qp, Qf = Qfp, us.Qp, pb.Qf
    lbt = us.lbt
    bits, x = pb.bits(Qfp)
    kchunk, kpart = plan
    part = H.participating(Kp, kchunk, kpart)
    assert us.lf == lf and part.sum() == 256 * len(H.remap_tiles(Kp, kchunk, kpart))
    uval = M.value_of(us.planes[:R_])
    real = (np.arange(Kp) < pb.K) & (pb.w > 0)
    for r in range(R_):
        u, vs = int(nodes[r]), int(vmap[r])
        # A: the direction
        d = H.direction(rows_int[r], Qfp, cconst, lf, hv, tau_v[vs], VSCALE[lbt])
        got = (us.sigma[r], us.tau[r], us.invtau[r])
        assert _same_bits(np.array(got), np.array([d["sigma"], d["tau"], d["invtau"]])), (tag, "sigma, tau, invtau of row", r, got, d["tau"], d["invtau"])
        assert int(us.qconst[r]) == d["qconst"], (tag, "qconst", r)
        assert np.array_equal(us.tq[r // 32, :, :, r % 32, :], d["image"]), (tag, "Tq image of row", r)
        # B: the elements
        hh = H.hh_planes(us.vplanes[vs], VPL0[lbt])
        Ea, _, _ = H.xdotp(rows_int[r], Qfp, cconst, lf, bits, x)
        um, nnear = H.product_row(form, hh, float(tau_v[vs]) * VSCALE[lbt], pb.w, Ea, us.invtau[r], u)
        _near[0] += nnear
        _near[1] += Kp
        bad = np.flatnonzero(part & (uval[r] != um))
        assert not len(bad), (tag, "products differ from the model: row", r, "samples", bad[:4].tolist(), "device", uval[r][bad[:4]].tolist(),
                              "model", um[bad[:4]].tolist(), len(bad))
        assert not us.planes[r][:, part & ~real].any(), (tag, "a padding or zero-count sample has a digit", r)
        if hv == 2:
            assert np.abs(uval[r][part]).max() <= H.U2MAX and not us.planes[r][2:, part].any(), (tag, "a two-limb product leaves two digits", r)
    if prev_planes is not None:
        assert np.array_equal(us.planes[:R_][:, :, ~part], prev_planes[:R_][:, :, ~part]), (tag, "bytes outside the part were written")
    # C: behind Uq
    csum, g = H.behind_uq(us.planes[:Rp], part, bits, hv)
    assert np.array_equal(us.csum[:R_], csum[:R_]), (tag, "csum")
    assert not us.asum[:R_].any() and not us.mmax[:R_].any(), (tag, "asum, mmax")
    bad = np.argwhere(us.gacc[:Rp] != g)
    assert not len(bad), (tag, "Gacc [slot, plane, column]", bad[:4].tolist(), len(bad))
    if hv == 2:
        assert not us.gacc[:Rp, 2:].any(), (tag, "accumulator planes 2, 3 of a two-limb pass")
    active = np.arange(Rp) < R_
    G = H.finalize(us.tau, csum, g, active, Qf, Qp, cconst)
    assert _same_bits(G_dev[:R_], G[:R_]), (tag, "G", np.argwhere(G_dev[:R_] != G[:R_])[:4].tolist())
    if G_before is not None and G_before.size:  # (empty: the first pass of a handle sized the workspace, there is nothing to compare)
        assert G_before.shape == us.G.shape
        assert _same_bits(us.G[R_:], G_before[R_:]), (tag, "rows of unused slots were written")


def check_bound(tag, pb, o, keep, out, form, hv, lf, plan, vec, vscale, vslot=None):
    """the product bound of test_gpu_i8_pass_variants.py against Ref; vslot: the slot whose tau_V each product row reads"""
    e = keep.index(plan if plan[0] else (pb.Kp, pb.Kp))
    hv_ref = o["hv"][e].astype(np.float64)
    err = np.abs(out["hv"] - hv_ref).max(axis=1)
    K = pb.K
    kc, kp = plan if plan[0] else (pb.Kp, pb.Kp)
    kpart = (K // kc) * kp + min(K % kc, kp)
    tau_h, tau_v = out["s1"][:, 1], (out["s0"][:, 1] if vslot is None else out["s0"][vslot, 1]) * vscale
    ch = 2.0 if form == "RPLE" else 1.0
    bound = (1e-13 * np.abs(o["f"].astype(np.float64)) + 3.3 * np.sqrt(kpart) * tau_h + 3.3 * np.sqrt(kpart) * ch * tau_v * np.abs(vec).sum(axis=1)
             + quant_defect(vec, lf) * o["hsum"][e].astype(np.float64))
    ratio = float((err / bound).max())
    assert ratio <= 1.0, (tag, "the product bound of test_gpu_i8_pass_variants.py against the 80-bit reference", ratio)
    _worst[tag] = ratio
    return ratio


def read_G(p):
    L = _hooks()
    d = np.zeros(8, dtype=np.int64)
    _lib.check(L.gml_test_i8_gacc(p._h, _lib._ptr(d), None, None, None))
    G = np.zeros((int(d[5]), int(d[6])))
    if G.size:
        _lib.check(L.gml_test_i8_gacc(p._h, _lib._ptr(d), None, _lib._ptr(G), None))
    return G


def run_product(handles, name, form, prec, hv, lf, plan, vkey, prev=None, bound=True):
    """one objective pass (form, prec) and one product pass (hv, lf, plan) of the direction set vkey through gml_test_i8_pass, held to
    A .. D; prev: the UqState of the product before it on the same slots"""
    pb, p = prob(name), handle(handles, name)
    th, vec = theta_of(pb), pb.directions(vkey)
    R_ = len(pb.nodes)
    tag = (name, form, prec, f"hv{hv}/lf{lf}", plan, vkey)
    G0 = read_G(p)
    out = i8_pass(p, form, prec, pb.nodes, th, vec=vec, hv=hv, hv_lf=lf, kchunk=plan[0], kpart=plan[1])
    us, st = UqState(p), State(p)
    assert (st.Kp, st.K, st.Qf, st.cconst, st.hv_lf) == (pb.Kp, pb.K, pb.Qf, st.Qfp, lf) and us.lbt == M.LBT[prec]
    eff = out["plan"] if not plan[0] else plan
    assert plan[0] == 0 or out["plan"] == plan
    assert eff[0] == eff[1] or plan[0], (tag, "a full pass")
    rows_int = pb.internal(vec, st.Qp, st.cconst)
    assert np.array_equal(st.theta[:R_], rows_int), (tag, "the directions the pass read")
    check_product(tag, pb, us, form, hv, lf, eff, st.theta[:R_], pb.nodes, np.arange(R_), st.tau, None if prev is None else prev.planes,
                  us.G, G0)
    assert np.array_equal(out["s1"][:, 1], us.tau[:R_]) and not out["s1"][:, 2].any(), (tag, "slot results of the product pass")
    assert _same_bits(us.F[:R_], out["f"]), (tag, "the workspace's f after the product pass")
    if bound:
        keep, o = reference(p, pb, form, vkey, vec)
        check_bound(tag, pb, o, keep, out, form, hv, lf, plan, vec, VSCALE[us.lbt])
    _seen.update(instances())
    return us, out


# ---------------------------------------------------------------------------------------------------------------------------
# the matrix
# ---------------------------------------------------------------------------------------------------------------------------
PAIRWISE = ["splitk", "narrow-counts", "narrow-uniform"]


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("hv,lf", HVLF)
@pytest.mark.parametrize("prec", ["i8x", "i8w"])
@pytest.mark.parametrize("form", ["RISE", "RPLE"])
@pytest.mark.parametrize("name", PAIRWISE)
def test_product_exact(handles, name, form, prec, hv, lf):
    """a full product of the direction set 1, then a sub-sampled one of the set 2 on the same slots: its part is the model's, the
    bytes outside it are the first product's"""
    _ran.add((name, form, prec, hv, lf))
    first, _ = run_product(handles, name, form, prec, hv, lf, (0, 0), 1)
    plans = PLANS[name]
    plan = plans[(HVLF.index((hv, lf)) + (prec == "i8w") + 2 * (form == "RPLE")) % len(plans)]
    run_product(handles, name, form, prec, hv, lf, plan, 2, prev=first)


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("name", PAIRWISE)
def test_product_exact_logrise(handles, name):
    """logRISE runs the instances of RISE (FORM 3): once per shape, at the solver's default"""
    first, _ = run_product(handles, name, "logRISE", "i8x", 2, 2, (0, 0), 1)
    run_product(handles, name, "logRISE", "i8x", 2, 2, PLANS[name][0], 2, prev=first)


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("name", PAIRWISE)
def test_every_plan_at_the_default(handles, name):
    """every sub-sampled plan of the shape at hv = 2, lf = 2, each after a full product of another direction set; the narrow shapes
    include (4096, 2048), whose last chunk is shorter than kpart"""
    for form, prec in (("RISE", "i8x"), ("RPLE", "i8w")):
        for plan in PLANS[name]:
            first, _ = run_product(handles, name, form, prec, 2, 2, (0, 0), 1, bound=False)
            run_product(handles, name, form, prec, 2, 2, plan, 2, prev=first)


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["i8x", "i8w"])
def test_order3(handles, prec):
    """mixed one- and two-spin statistics, 46 padding columns, directions with entries on the last statistics columns"""
    for form, hv, lf in (("RISE", 2, 2), ("RISE", 1, 5), ("RPLE", 1, 3)):
        first, _ = run_product(handles, "order3", form, prec, hv, lf, (0, 0), 1)
        run_product(handles, "order3", form, prec, hv, lf, PLANS["order3"][hv - 1], 2, prev=first)


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("name", PAIRWISE)
def test_pass_order(handles, name):
    """hv = 1 followed by hv = 2 on the same slots, and the reverse: each pass is the model's whatever the other left in Uq, Gacc and the
    product scalars (a two-limb pass leaves the planes 2, 3 of an earlier four-limb pass's part zeroed, not stale)"""
    for a, b in (((1, 5), (2, 2)), ((2, 5), (1, 2))):
        first, _ = run_product(handles, name, "RISE", "i8x", a[0], a[1], (0, 0), 1, bound=False)
        second, _ = run_product(handles, name, "RISE", "i8x", b[0], b[1], (0, 0), 2, prev=first, bound=False)
        run_product(handles, name, "RISE", "i8x", a[0], a[1], PLANS[name][0], 1, prev=second, bound=False)


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("name", PAIRWISE)
def test_pack_state_after_a_product(handles, name):
    """after a product pass gml_test_i8_pack_state reports dims[18] = its LF; a following objective pass resets it and reproduces its own
    earlier bits: the Tq image, tau, f and G"""
    pb, p = prob(name), handle(handles, name)
    th = theta_of(pb)
    R_ = len(pb.nodes)  # (tau of the unused slots is whatever the allocation held, NaN included: not compared)
    for prec in ("i8x", "i8w"):
        a = i8_pass(p, "RISE", prec, pb.nodes, th)
        sa = State(p)
        assert sa.hv_lf == 0
        run_product(handles, name, "RISE", prec, 2, 2, (0, 0), 1, bound=False)
        assert State(p).hv_lf == 2
        b = i8_pass(p, "RISE", prec, pb.nodes, th)
        sb = State(p)
        assert sb.hv_lf == 0 and sb.lf == sa.lf and np.array_equal(sb.tq, sa.tq) and np.array_equal(sb.tau[:R_], sa.tau[:R_])
        assert _same_bits(a["f"], b["f"]) and _same_bits(a["g"], b["g"])


def i8_pass_vslot(p, form, prec, nodes, theta, vslot, vec, hv, hv_lf, plan, tauovr=None):
    """gml_test_i8_pass_vslot: the objective pass over (nodes, theta), then product row i = (slot i, node nodes[vslot[i]], direction vec[i] in
    that node's parameter order) on the weights of slot vslot[i]"""
    L = _lib.lib()
    v, i64 = C.c_void_p, C.c_int64
    L.gml_test_i8_pass_vslot.argtypes = [v, C.c_int, C.c_int, i64, v, v, v, v, i64, v, v, v, v, v, v, v]
    nodes = np.ascontiguousarray(nodes, dtype=np.int64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    vec = np.ascontiguousarray(vec, dtype=np.float64)
    vslot = np.ascontiguousarray(vslot, dtype=np.int32)
    R_, P = theta.shape
    kn = np.array([0, 0, 1, 1, 0, hv, hv_lf, 1, plan[0], plan[1], 0], dtype=np.int64)
    f, g, h = np.zeros(R_), np.zeros((R_, P)), np.zeros((R_, P))
    slots, pl = np.zeros((2, R_, 3)), np.zeros(2, dtype=np.int64)
    tv = None if tauovr is None else np.ascontiguousarray(tauovr, dtype=np.float64)
    _lib.check(L.gml_test_i8_pass_vslot(p._h, _lib.FORMULATION_IDS[form], _lib.PRECISIONS[prec], R_, _lib._ptr(nodes), _lib._ptr(theta),
                                        None if tv is None else _lib._ptr(tv),
                                        _lib._ptr(vec), P, _lib._ptr(kn), _lib._ptr(f), _lib._ptr(g), _lib._ptr(h), _lib._ptr(slots), _lib._ptr(pl),
                                        _lib._ptr(vslot)))
    return dict(f=f, g=g, hv=h, s0=slots[0], s1=slots[1], plan=tuple(int(x) for x in pl))


def slot_map(R_):
    """every product row reads another slot: slots used twice and slots never used, rows of both node tiles drawing from both tiles"""
    vslot = np.random.default_rng(67).integers(0, R_, size=R_).astype(np.int32)
    vslot[:6] = [R_ - 1, 3, 3, 0, 34, 2]
    vslot[32:36] = [3, R_ - 2, 1, 33]
    assert not (vslot == np.arange(R_)).all() and (vslot[:32] >= 32).any() and (vslot[32:] < 32).any()
    return vslot


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["i8x", "i8w"])
@pytest.mark.parametrize("name", PAIRWISE)
def test_slot_map(handles, name, prec):
    """vmap != identity through the GEMM pass for FORM 4 as well: RPLE's hh = 2 a (1 - a tvh / (2 w)) reads tau_V of the slot vmap[r], which
    the identity map cannot tell from the row's own -- the rows' tau differ (checked), so the wrong slot's tau_V changes tau_hv, invtau's
    partner and every RPLE element.  Solver::newton_cg_group runs its products this way (vmap = the slot of the row).
    An RPLE pass gives every slot the same tau, 2 w_max (1 + 1e-12) / vdiv, so its objective pass runs with a tau imposed per row (tauovr,
    the operator's rescaled re-run): 0.90 .. 0.99 of that, which the planes hold as long as (w_k / w_max) sig_k, sig = 1 / (1 + e^2E), stays
    below the row's factor on every sample -- asserted on the host from the rows' energies before the pass runs."""
    pb, p = prob(name), handle(handles, name)
    th = theta_of(pb)
    R_, P = th.shape
    vslot = slot_map(R_)
    nodes = pb.nodes[vslot]
    sub = HvProb.__new__(HvProb)
    sub.__dict__.update(pb.__dict__)
    sub.nodes = nodes
    vec = sub.directions(3)
    for form, hv, lf, plan in (("RPLE", 2, 2, (0, 0)), ("RPLE", 1, 5, PLANS[name][-1]), ("RISE", 1, 3, (0, 0))):
        tag = (name, form, prec, f"hv{hv}/lf{lf}", plan, "slot map")
        ovr = None
        if form == "RPLE":
            fac = 0.90 + 0.09 * np.arange(R_) / R_
            ovr = 2.0 * pb.wmax / R.VDIV[M.LBT[prec]] * fac
            Qfp = (pb.Qf + 63) // 64 * 64
            ti = pb.internal(th, Qfp + 64, Qfp)
            E = (ti[:, :Qfp] @ pb.bits(Qfp)[1] + ti[:, [Qfp]]) * (1.0 - 2.0 * pb.sb[pb.nodes])
            top = ((pb.w / pb.wmax) / (1.0 + np.exp(2.0 * E))).max(axis=1)
            assert (top < 0.98 * fac).all(), (tag, "an imposed tau would leave the planes", float((top / fac).max()))
        out = i8_pass_vslot(p, form, prec, pb.nodes, th, vslot, vec, hv, lf, plan, ovr)
        us, st = UqState(p), State(p)
        assert us.lbt == M.LBT[prec] and st.hv_lf == lf
        tau_v = st.tau
        assert (ovr is None or np.array_equal(tau_v[:R_], ovr)) and np.array_equal(tau_v[:R_], out["s0"][:, 1]) and (tau_v[vslot] != tau_v[:R_]).sum() > R_ // 2, (tag, "the slots' tau differ")
        rows_int = sub.internal(vec, st.Qp, st.cconst)
        assert np.array_equal(st.theta[:R_], rows_int), (tag, "the directions the pass read")
        eff = plan if plan[0] else out["plan"]
        check_product(tag, pb, us, form, hv, lf, eff, rows_int, nodes, vslot, tau_v, None, us.G)
        assert np.array_equal(out["s1"][:, 1], us.tau[:R_]) and _same_bits(us.F[:R_], out["f"]), (tag, "slot results, f")
        key = (name, form, "slot map")
        if key not in _refs:
            _refs[key] = Ref(pb.spins, pb.counts).run(nodes, [dict(form=form, theta=th[vslot], vec=vec, keep=[(pb.Kp, pb.Kp), PLANS[name][-1]])])[0]
        check_bound(tag, pb, _refs[key], [(pb.Kp, pb.Kp), PLANS[name][-1]], out, form, hv, lf, plan, vec, VSCALE[us.lbt], vslot)
    _seen.update(instances())


@need_ld
@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["i8x", "i8w"])
@pytest.mark.parametrize("name", PAIRWISE)
def test_one_slot_serves_two_directions(handles, name, prec):
    """vmap != identity, through gml_test_hv_sparse (its GEMM side: hv = 2, lf = 2): 34 product rows from both node tiles read the V planes
    and tau of other slots, some slots twice with different directions"""
    pb, p = prob(name), handle(handles, name)
    th = theta_of(pb)
    R_, P = th.shape
    rng = np.random.default_rng(61)
    nloc = 34
    vslot = rng.integers(0, R_, size=nloc).astype(np.int32)
    vslot[:4] = [R_ - 1, 3, 3, 0]
    vslot[32:] = [3, R_ - 2]
    vec = rng.normal(size=(nloc, P))
    vec[2] = 0.0
    vec[2, int(pb.nodes[3])] = 0.3  # the node's field alone
    vec[7] = 0.0
    lists = [np.arange(P) for _ in range(nloc)]
    plan = PLANS[name][0]
    for form in ("RISE", "logRISE"):
        hs, hg, cm = hv_two_ways(p, form, prec, pb.nodes, th, vslot, vec, lists, 128, P, plan)
        us, st = UqState(p), State(p)
        nodes = pb.nodes[vslot]
        rows_int = np.zeros((nloc, st.Qp))
        for i in range(nloc):
            rows_int[i, cm[i]] = vec[i]
        sub = HvProb.__new__(HvProb)
        sub.__dict__.update(pb.__dict__)
        sub.nodes = nodes
        assert np.array_equal(rows_int, sub.internal(vec, st.Qp, st.cconst))
        check_product((name, form, prec, "vslot"), pb, us, form, 2, 2, plan, rows_int, nodes, vslot, st.tau, None, hg)
        for i in range(nloc):  # (the entry-by-entry form writes the listed entries only)
            assert _same_bits(hs[i, cm[i]], hg[i, cm[i]]), (name, form, prec, "the entry-by-entry form", i)
    _seen.update(instances())


@need_ld
@pytest.mark.gpu
def test_every_product_instance_ran(handles):
    """the record of this file's tests (in order, in one process) holds every product instance reachable below 32768 statistics columns:
    forward LF 2 .. 5 x FORM 3 / 4 x UNIW, backward NL 2 and 4 at pl0 = 0, finalise with hv"""
    if len(_ran) < len(PAIRWISE) * 2 * 2 * len(HVLF):
        pytest.skip("needs the whole matrix of this file in the same session")
    want = {fwd_bit(LF, FORM, 0, 0, 0, UNIW) for LF in (2, 3, 4, 5) for FORM in (3, 4) for UNIW in (0, 1)}
    want |= {bwd_bit(2, 0), bwd_bit(4, 0), 305}
    assert not (want - _seen), sorted(want - _seen)
    print(f"elements evaluated in rational arithmetic: {_near[0]} of {_near[1]} ({_near[0] / max(_near[1], 1):.2e})")
    print(f"worst product-bound ratio against Ref: {max(_worst.values()):.6g} at {max(_worst, key=_worst.get)}")
