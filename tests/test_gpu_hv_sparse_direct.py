"""The entry-by-entry Hessian-vector products (csrc/gml_hv_sparse.hip: k_hvs_quant, k_hvs_fwd, k_hvs_mid, k_hvs_bwd, k_hvs_finalize)
against the GEMM product pass they claim to equal bit for bit, on lists aimed at the boundaries of the code rather than on whatever
working sets a solve happens to produce.

Through gml_test_hv_sparse: one objective pass (device_pass) over 40 rows -- two node tiles -- then one product of caller-given
directions two ways, i8_hv_sparse over caller-given lists and the GEMM pass with hv = 2, lf = 2 and the same (kchunk, kpart).  Per
product row the two outputs must be equal as float64 bit patterns on every listed entry, and the entry-by-entry form must leave
every other entry of its output untouched.  Directions are zero outside their lists (the GEMM pass multiplies whole rows).

Covered: RISE and logRISE at i8x and at i8w (k_hvs_mid reading the top four of six planes: lbt = 6, vpl0 = 2, vscale = 65536);
nw in {1, 2, 3, 4, 5, 255, 256, 257, n} (the four-entry unroll, EC = 256); lists with the node's field (the constant column)
first, last or absent; six rows of different nw under one wcap, equal to the largest nw and larger, from both node tiles, one slot
twice with two directions; a direction whose largest entry is a power of two (frexp), one of all zeros (the pn fallback); the plans
full, (2048, 1024), (2048, 256), (4096, 512) on Kp = 9216 (no multiple of 8192, the last chunk partial); an order-3 handle, whose
lists mix one- and two-spin statistics.  One case per form and precision also holds the GEMM side to the extended-precision
reference of tests/test_gpu_i8_pass_variants.py with that file's product bound, so the identity is not one between two wrong
answers."""
import ctypes as C
import importlib

import numpy as np
import pytest

import gml_amd as gml
from test_gpu_i8_pass_variants import LD, Ref, need_ld, quant_defect

_lib = importlib.import_module("gml_amd._lib")
pytestmark = pytest.mark.gpu
FILL = -7.25  # what the outputs hold before the products run
NROWS = 40
PLANS = [(0, 0), (2048, 1024), (2048, 256), (4096, 512)]
VSCALE = {"i8x": 1.0, "i8w": 65536.0}


def _hooks():
    L = _lib.lib()
    v, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    L.gml_test_hv_sparse.argtypes = [v, i32, i32, i64, v, v, i64, i64, v, v, v, v, v, i32, i64, i64, i64, C.c_double, v, v, v]
    L.gml_test_i8_pack_state.argtypes = [v, i64, v, v]
    return L


def _dims(p):
    d = np.zeros(20, dtype=np.int64)
    _lib.check(_hooks().gml_test_i8_pack_state(p._h, 0, _lib._ptr(d), None))
    return dict(slots=int(d[0]), Qp=int(d[6]), Qfp=int(d[7]), Qf=int(d[8]), cconst=int(d[9]), Kp=int(d[10]))


def _tau(p):
    ns = _dims(p)["slots"]
    tau = np.zeros(ns)
    d = np.zeros(20, dtype=np.int64)
    ptrs = (C.c_void_p * 13)(*[tau.ctypes.data if i == 5 else None for i in range(13)])
    _lib.check(_hooks().gml_test_i8_pack_state(p._h, 0, _lib._ptr(d), ptrs))
    return tau


def hv_two_ways(p, form, prec, nodes, theta, vslot, vec, lists, T, wcap, plan):
    """(hs, hg [nloc][Qp], colmap [nloc][P]) of gml_test_hv_sparse; lists: one array of parameter indices per product row"""
    L = _hooks()
    nodes = np.ascontiguousarray(nodes, dtype=np.int64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    vec = np.ascontiguousarray(vec, dtype=np.float64)
    vslot = np.ascontiguousarray(vslot, dtype=np.int32)
    nloc, P = vec.shape
    nw = np.array([len(x) for x in lists], dtype=np.int32)
    nt = (nw + T - 1) // T
    t0 = np.concatenate([[0], np.cumsum(nt)[:-1]]).astype(np.int64)
    FV = np.zeros(int(nt.sum()) * T, dtype=np.int32)
    for i, lst in enumerate(lists):
        FV[t0[i] * T:t0[i] * T + len(lst)] = lst
    Qp = _dims(p)["Qp"]
    hs, hg = np.zeros((nloc, Qp)), np.zeros((nloc, Qp))
    colmap = np.zeros((nloc, P), dtype=np.int32)
    _lib.check(L.gml_test_hv_sparse(p._h, _lib.FORMULATION_IDS[form], _lib.PRECISIONS[prec], len(nodes), _lib._ptr(nodes), _lib._ptr(theta),
                                    theta.shape[1], nloc, _lib._ptr(vslot), _lib._ptr(vec), _lib._ptr(FV), _lib._ptr(t0), _lib._ptr(nw), T, wcap,
                                    plan[0], plan[1], FILL, _lib._ptr(hs), _lib._ptr(hg), _lib._ptr(colmap)))
    return hs, hg, colmap


def check_equal(hs, hg, colmap, lists, label):
    some = False
    for i, lst in enumerate(lists):
        c = colmap[i][np.asarray(lst)]
        assert len(set(c.tolist())) == len(lst)
        a, b = hs[i, c], hg[i, c]
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), (label, "row", i, "nw", len(lst), int((a != b).sum()),
                                                                     float(np.abs(a - b).max()), float(np.abs(b).max()))
        assert not (a == FILL).any(), (label, "row", i, "a listed entry was not written")
        rest = np.ones(hs.shape[1], dtype=bool)
        rest[c] = False
        assert (hs[i, rest] == FILL).all(), (label, "row", i, "wrote outside its list")
        some |= bool((b != 0).any())
    return some


def _list(rng, P, u, nw, field):
    """nw distinct parameters of node u's row; field: None (absent), 'first' or 'last' position of its own field (parameter u)"""
    if nw == P:
        lst = rng.permutation(np.delete(np.arange(P), u))
        return np.concatenate([[u], lst]) if field == "first" else np.concatenate([lst, [u]])
    lst = np.sort(rng.choice(np.delete(np.arange(P), u), size=nw, replace=False))
    if field == "first":
        lst[0] = u
    elif field == "last":
        lst[-1] = u
    return lst


def _direction(rng, P, lst, kind="normal"):
    v = np.zeros(P)
    if kind == "zero":
        return v
    v[lst] = rng.normal(size=len(lst))
    if kind == "pow2":
        v[lst] = np.clip(0.2 * v[lst], -0.49, 0.49)
        v[lst[len(lst) // 2]] = -0.5  # the largest entry is a power of two: frexp gives 0.5 x 2^0
    return v


@pytest.fixture(scope="module")
def pair():
    n, K = 300, 9000
    rng = np.random.default_rng(41)
    spins = np.where(rng.random((K, n)) < 0.55, 1, -1).astype(np.int8)
    counts = np.floor(10 ** rng.uniform(0, 2, size=K))
    counts[rng.random(K) < 0.03] = 0.0
    with gml.Problem(spins=spins, counts=counts) as p:
        assert _dims(p)["Kp"] == 9216
        nodes = np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), size=NROWS - 2, replace=False)]).astype(np.int64)
        theta = rng.normal(scale=0.15, size=(NROWS, n)) * (rng.random((NROWS, n)) < 0.1)
        yield dict(p=p, n=n, K=K, nodes=nodes, theta=theta, ref=None)


def _sweep_rows(rng, n, nodes):
    """nine product rows, nw = 1 .. n, slots from both node tiles, the field first / last / absent in turn"""
    sizes = [1, 2, 3, 4, 5, 255, 256, 257, n]
    vslot = [0, 33, 2, 35, 4, 37, 6, 39, 1]
    field = ["first", None, "last", "first", None, "last", "first", None, "last"]
    lists = [_list(rng, n, int(nodes[s]), m, f) for m, s, f in zip(sizes, vslot, field)]
    vec = np.stack([_direction(rng, n, lst) for lst in lists])
    return vslot, lists, vec


def _mixed_rows(rng, n, nodes):
    """six rows of different nw: slot 34 twice with two directions, a power-of-two direction, a zero direction; both node tiles"""
    sizes = [7, 130, 61, 258, 33, 4]
    vslot = [34, 34, 3, 38, 36, 5]
    field = [None, "last", "first", None, "last", None]
    kinds = ["normal", "normal", "normal", "normal", "pow2", "zero"]
    lists = [_list(rng, n, int(nodes[s]), m, f) for m, s, f in zip(sizes, vslot, field)]
    vec = np.stack([_direction(rng, n, lst, k) for lst, k in zip(lists, kinds)])
    return vslot, lists, vec


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("prec", ["i8x", "i8w"])
@pytest.mark.parametrize("form", ["RISE", "logRISE"])
def test_pairwise_lists_equal_the_gemm_pass(pair, form, prec, plan):
    p, n, nodes, theta = pair["p"], pair["n"], pair["nodes"], pair["theta"]
    rng = np.random.default_rng(42)
    vslot, lists, vec = _sweep_rows(rng, n, nodes)
    hs, hg, cm = hv_two_ways(p, form, prec, nodes, theta, vslot, vec, lists, 128, n, plan)
    assert check_equal(hs, hg, cm, lists, (form, prec, plan, "sweep"))
    vslot, lists, vec = _mixed_rows(rng, n, nodes)
    for wcap in (258, 295):  # the largest nw, and above it
        hs, hg, cm = hv_two_ways(p, form, prec, nodes, theta, vslot, vec, lists, 64, wcap, plan)
        assert check_equal(hs, hg, cm, lists, (form, prec, plan, "mixed", wcap))
        assert not hg[5, cm[5][lists[5]]].any()  # the zero direction: zero products (and no division by a zero norm)
        a, b = cm[0][lists[0]], cm[1][lists[1]]
        assert hg[0, a].any() and hg[1, b].any()  # the slot used twice


@need_ld
@pytest.mark.parametrize("prec", ["i8x", "i8w"])
@pytest.mark.parametrize("form", ["RISE", "logRISE"])
def test_gemm_side_meets_the_reference(pair, form, prec):
    # sum_k h_k (x_k . p) x_k over the configurations k mod kchunk < kpart, in np.longdouble (raw: logRISE's Hess Z p), and the product
    # bound of tests/test_gpu_i8_pass_variants.py: 1e-13 |f| + 3.3 sqrt(Kpart) tau_hv + 3.3 sqrt(Kpart) c_h tau_V |p|_1 + d_p sum h, c_h = 1,
    # tau_V the unit of the four planes the products read (tau vscale), tau_hv = tau_V pn the unit of the rounded products with
    # pn = 65536 * 1.01 * sigma sum |q| of the direction's two-digit quantisation (k_hvs_quant's header)
    p, n, K, nodes, theta = pair["p"], pair["n"], pair["K"], pair["nodes"], pair["theta"]
    if pair["ref"] is None:
        pair["ref"] = Ref(p.spins(), p.counts())
    rng = np.random.default_rng(43)
    vslot, lists, vec = _mixed_rows(rng, n, nodes)
    plan = (2048, 1024)
    hs, hg, cm = hv_two_ways(p, form, prec, nodes, theta, vslot, vec, lists, 64, 258, plan)
    assert check_equal(hs, hg, cm, lists, (form, prec, "reference"))
    tau_v = _tau(p)[vslot] * VSCALE[prec]
    o = pair["ref"].run(nodes[vslot], [dict(form=form, theta=theta[vslot], vec=vec, keep=[plan])])[0]
    kpart = (K // plan[0]) * plan[1] + min(K % plan[0], plan[1])
    worst = 0.0
    for i, lst in enumerate(lists):
        pv = vec[i]
        mx = np.abs(pv).max()
        sg = 2.0 ** ((np.frexp(mx)[1] if mx > 0 else 0) - 14)
        emax = np.abs(np.rint(pv / sg)).sum() * sg
        tau_h = tau_v[i] * (emax if emax > 0 else 1.0) * 65536.0 * 1.01
        p1 = np.abs(pv).sum()
        bound = (1e-13 * abs(float(o["f"][i])) + 3.3 * np.sqrt(kpart) * tau_h + 3.3 * np.sqrt(kpart) * tau_v[i] * p1
                 + quant_defect(pv[None, :], 2)[0] * float(o["hsum"][0][i]))
        err = float(np.abs(hg[i, cm[i]].astype(LD) - o["hv"][0][i])[lst].max())
        worst = max(worst, err / bound)
        assert err <= bound, (form, prec, i, err / bound)
    print(f"{form} {prec}: GEMM products against the reference, measured / bound = {worst:.3g}")


@pytest.mark.parametrize("plan", [(0, 0), (2048, 256)])
@pytest.mark.parametrize("prec", ["i8x", "i8w"])
def test_order3_lists_equal_the_gemm_pass(prec, plan):
    # n = 20, order 3: 191 statistics columns per node -- 20 one-spin keys (k_hvs_quant moves a key's spin to the first slot) and 171 pairs
    n, K = 20, 3000
    rng = np.random.default_rng(44)
    spins = np.where(rng.random((K, n)) < 0.5, 1, -1).astype(np.int8)
    with gml.Problem(spins=spins, order=3) as p:
        P = p.P
        assert P == 191
        nodes = np.arange(NROWS, dtype=np.int64) % n
        theta = rng.normal(scale=0.1, size=(NROWS, P)) * (rng.random((NROWS, P)) < 0.2)
        sizes, vslot = [1, 5, 190, 191, 64, 3], [0, 32, 7, 39, 7, 20]
        lists = []
        for m in sizes:
            lists.append(rng.permutation(P)[:m] if m < P else rng.permutation(P))
        lists[0] = np.array([0])  # parameter 0 alone
        vec = np.stack([_direction(rng, P, lst) for lst in lists])
        for form in ("RISE", "logRISE"):
            hs, hg, cm = hv_two_ways(p, form, prec, nodes, theta, vslot, vec, lists, 128, 191 if plan[0] else 200, plan)
            assert check_equal(hs, hg, cm, lists, (form, prec, plan, "order 3"))
