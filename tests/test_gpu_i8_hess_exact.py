"""The second-order kernels of the int8-limb path (csrc/gml_i8_hess.hip: k_make_hw, k_build_mb, k_hess_bits_small, k_hess_bits_blk<4>,
k_hess_i8_fin) and the FP64 Hessian kernel (k_hess_f64), held to the host model tests/_i8_hess_reference.py.

One handle: pairwise, n = 544 (Qfp is padded; 512 distinct columns fit a list), K = 3000 with counts (Kp = 3072: a zero-weight
tail; some counts are zero), spins of synthetic.block_ising, 40 rows (rows 32..39: node tile 1).  One call mixes the sizes 0, 1, 31,
32, 33, 96, 128, 129, 160, 257, 416, 512 and others, i.e. skipped rows, the one-workgroup kernel and the blocked kernel together.
Among the rows: two of dense theta (sum |theta| = 60: their weights sit some 70 bits below the bound tau starts from, so device_pass
ends on rescaled re-runs of a subset of the rows; tau and mmax are the re-run's -- checked: every mmax fills its planes), one at theta = 0, one whose list holds a column twice, two whose lists hold the node's own field; every list whose size
is no multiple of 32 is padded by repeating its entries.

Through gml_test_hessian_run (device_pass, then i8_hessian, as a solver iteration) every case checks, with the device's own V
image, mmax, tau (gml_test_i8_pass_state, gml_test_i8_pack_state) and Hessian state (gml_test_i8_hess_state):
  1. Mb equals the model's (once per handle);
  2. Hq and hS of every flagged row equal the model's h2 -- exactly, RPLE's float64 expression included (on the device no sample
     of any RPLE case differed from the model, so that check is np.array_equal too);
  3. H64 on every lower 32 x 32 tile of every block equals T_ij formed from the device's Hq and the natural-order bits;
  4. every upper tile of H64 is zero;  5. hS of every skipped row is zero;
  6. the doubles returned equal ldexp(tau vscale, sh) (hS - 2 T_ii - 2 T_jj + 4 T_ij) bit for bit, and are zero on the upper tiles;
  7. against np.longdouble sums of the true weights (statistics in the reference's order, independent of the internal layout), per
     entry:  |H - H_true| <= Kh_nz (U + c_h tau vscale) + 1e-13 sum_k h_k,  U = 2^sh tau vscale.
     Derivation: a sample's weight enters as 2^sh tau' h2 (tau' = tau vscale) with h2 = floor((mag + dither) / 2^sh), 0 <= dither
     < 2^sh: off by less than U from mag tau'; mag tau' is the pass's V_k, off from the true weight by c_h tau' (i8x: dithered
     rounding to a multiple of tau, c_h = 1; i8w: the top four planes are V / 65536 tau to nearest, c_h = 1/2; RPLE: h = 2a(1 - a/2w)
     has |dh/da| <= 2, twice that).  |x_i x_j| = 1, and a configuration of count 0 has V = 0 and h2 = 0 exactly, so the Kh_nz
     configurations of non-zero count in the sub-sample add up.  1e-13 sum h covers the FP64 exp and the quantised theta, as in
     tests/test_gpu_i8_pass_variants.py.  Each case prints measured / bound; the bound is derived, not measured.
FP64: k_hess_f64 after the FP64 pass against the same sums, per entry (1e-12 + (Kh + 4) 2^-53) sum_k h_k: FTOL of the FP64 pass plus
the summation bound; skipped rows and upper tiles stay zero."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _i8_hess_reference as HR
import gml_amd as gml
from test_gpu_i8_pass_variants import LD, Ref, _xdot, need_ld

_lib = importlib.import_module("gml_amd._lib")
synthetic = importlib.import_module("gml_amd.synthetic")
pytestmark = [pytest.mark.gpu, need_ld]

N, K, NR, CAP = 544, 3000, 40, 512
HESS_WGS, HESS_BLK_WGS = 2, 10  # gml_solver.h: GML_TUNE_HESS_WGS, GML_TUNE_HESS_BLK_WGS
SIZES = [0, 1, 31, 32, 33, 96, 128, 129, 160, 257, 416, 512,
         33, 0, 96, 129, 1, 32, 160, 31, 128, 257, 0, 64, 100, 200, 5, 127, 130, 300, 2, 97,
         512, 0, 1, 129, 96, 0, 416, 33]
DENSE_ROWS, ZERO_ROW, DUP_ROW, FIELD_ROWS = (5, 38), 7, 8, (6, 10)
VSCALE = {"i8x": 1.0, "i8w": 65536.0}
_ratios = {}


# ---------------------------------------------------------------------------------------------------------------------------
# the hooks
# ---------------------------------------------------------------------------------------------------------------------------
def _hooks():
    L = _lib.lib()
    v, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    L.gml_test_hessian_run.argtypes = [v, i32, i32, i64, v, v, i64, v, i32, i64, i64, i32, i32, v, v, v, v, v, v, i64, v]
    L.gml_test_i8_hess_state.argtypes = [v, v, v]
    L.gml_test_i8_pass_state.argtypes = [v, C.POINTER(i64), C.POINTER(i32), C.POINTER(i64), v, v]
    L.gml_test_i8_pack_state.argtypes = [v, i64, v, v]
    L.gml_test_tune.restype = C.c_double
    L.gml_test_tune.argtypes = [i32, C.c_double]
    return L


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def hessian_run(p, form, prec, nodes, theta, cols, mtV, hoffV, htotal, Kh, kstride, tiles=None):
    L = _hooks()
    nodes = np.ascontiguousarray(nodes, dtype=np.int64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    cols, mtV = _i32(cols), _i32(mtV)
    hoffV = np.ascontiguousarray(hoffV, dtype=np.int64)
    H = np.full(htotal, np.nan)
    if tiles is None:
        T, nt, tp = 0, 0, [None] * 4
    else:
        T, nt = tiles["T"], len(tiles["wrow"])
        keep = [_i32(tiles[k]) for k in ("tcols", "vm", "wrow", "hflag")]
        tp = [_lib._ptr(a) for a in keep]
    _lib.check(L.gml_test_hessian_run(p._h, _lib.FORMULATION_IDS[form], _lib.PRECISIONS[prec], len(nodes), _lib._ptr(nodes), _lib._ptr(theta),
                                      theta.shape[1], _lib._ptr(cols), cols.shape[1], Kh, kstride, T, nt, tp[0], tp[1], tp[2], tp[3],
                                      _lib._ptr(mtV), _lib._ptr(hoffV), htotal, _lib._ptr(H)))
    return H


def pass_state(p):
    """(vq int8 [tiles][Kp / 64][planes][32][64], mmax [slots], tau [slots]) of the last objective pass"""
    L = _hooks()
    ns, npl, kp = C.c_int64(), C.c_int(), C.c_int64()
    _lib.check(L.gml_test_i8_pass_state(p._h, C.byref(ns), C.byref(npl), C.byref(kp), None, None))
    ns, npl, kp = ns.value, npl.value, kp.value
    vq = np.zeros(ns * npl * kp, dtype=np.int8)
    sums = np.zeros((5, ns), dtype=np.int64)
    a, b, c = C.c_int64(), C.c_int(), C.c_int64()
    _lib.check(L.gml_test_i8_pass_state(p._h, C.byref(a), C.byref(b), C.byref(c), _lib._ptr(vq), _lib._ptr(sums)))
    tau = np.zeros(ns)
    d = np.zeros(20, dtype=np.int64)
    ptrs = (C.c_void_p * 13)(*[tau.ctypes.data if i == 5 else None for i in range(13)])
    _lib.check(L.gml_test_i8_pack_state(p._h, 0, _lib._ptr(d), ptrs))
    return vq.reshape(ns // 32, kp // 64, npl, 32, 64), sums[4], tau


def pack_dims(p):
    d = np.zeros(20, dtype=np.int64)
    _lib.check(_hooks().gml_test_i8_pack_state(p._h, 0, _lib._ptr(d), None))
    return dict(Qp=int(d[6]), Qfp=int(d[7]), Qf=int(d[8]), cconst=int(d[9]), Kp=int(d[10]), K=int(d[11]))


def hess_state(p, want_mb=False):
    L = _hooks()
    d = np.zeros(8, dtype=np.int64)
    _lib.check(L.gml_test_i8_hess_state(p._h, _lib._ptr(d), None))
    pitch, hrows, hcap, Qp, Kp, mbb, _, hl = (int(x) for x in d)
    assert hl == HR.HL
    hq = np.zeros(hrows * hl * pitch, dtype=np.int8)
    h64 = np.zeros(hcap, dtype=np.int64)
    mb = np.zeros(mbb // 4 if want_mb else 0, dtype=np.uint32)
    ptrs = (C.c_void_p * 3)(hq.ctypes.data, h64.ctypes.data, mb.ctypes.data if mb.size else None)
    _lib.check(L.gml_test_i8_hess_state(p._h, _lib._ptr(d), ptrs))
    return hq.reshape(hrows // 32, hl, 32, pitch), h64, mb.reshape(Qp, Kp // 64, 2) if mb.size else None


class knobs:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        for k in (HESS_WGS, HESS_BLK_WGS):
            _hooks().gml_test_tune(k, float(self.value))

    def __exit__(self, *a):
        for k in (HESS_WGS, HESS_BLK_WGS):
            _hooks().gml_test_tune(k, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# the handle, the rows and their lists
# ---------------------------------------------------------------------------------------------------------------------------
class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    spins, _ = synthetic.block_ising(N, K, block=16, seed=5)
    rng = np.random.default_rng(6)
    counts = np.floor(10 ** rng.uniform(0, 2, size=K))
    counts[rng.random(K) < 0.03] = 0.0
    c = Ctx()
    with gml.Problem(spins=spins, counts=counts) as p:
        c.p = p
        c.S, c.c = p.spins(), p.counts()
        assert c.S.shape == (K, N)
        c.ref = Ref(c.S, c.c)
        c.w64 = c.c / c.c.sum()
        c.nodes = np.concatenate([[0, N - 1], rng.choice(np.arange(1, N - 1), size=NR - 2, replace=False)]).astype(np.int64)
        th = rng.normal(scale=0.1, size=(NR, N)) * (rng.random((NR, N)) < 0.1)
        for r in DENSE_ROWS:
            th[r] = rng.normal(size=N)
            th[r] *= 60.0 / np.abs(th[r]).sum()
        th[ZERO_ROW] = 0.0
        c.theta = th
        # the lists: distinct parameters, the padding up to whole tiles of 32 repeats them from the start
        c.cols = np.zeros((NR, CAP), dtype=np.int32)
        for r, m in enumerate(SIZES):
            if m == 0:
                continue
            u = int(c.nodes[r])
            lst = rng.choice(np.delete(np.arange(N), u), size=m, replace=False)
            if r in FIELD_ROWS:
                lst[m // 2] = u  # the node's own field
            if r == DUP_ROW:
                lst[5] = lst[2]  # the same column twice
            mp = (m + 31) // 32 * 32
            c.cols[r, :mp] = np.resize(lst, mp)
        c.dims = None
        c.htrue = {}
        c.mb_checked = False
        yield c


def _bits(c):
    """natural-order bits of the internal columns uint8 [Qp][Kp]: column j < n is spin j; the constant column and the padding are zero"""
    if c.dims is None:
        c.dims = pack_dims(c.p)
        d = c.dims
        assert d["Kp"] == 3072 and d["K"] == K and d["Qf"] == N and d["Qfp"] > N and d["cconst"] >= d["Qfp"]
        c.B = np.zeros((d["Qp"], d["Kp"]), dtype=np.uint8)
        c.B[:N, :K] = (c.S < 0).T
    return c.B


def _internal(u, params, cconst):
    """pairwise: parameter j of node u's row is column j, its field (j = u) the constant column"""
    params = np.asarray(params)
    return np.where(params == u, cconst, params)


def _true_h(c, form, r):
    """the curvature weights of row r at its theta, np.longdouble [K]"""
    key = (form, r)
    if key not in c.htrue:
        X = c.ref.stats(int(c.nodes[r]), 0, K)
        E = _xdot(X, c.theta[r].astype(LD)[:, None])[:, 0]
        if form == "RPLE":
            sig = 1 / (1 + np.exp(2 * E))
            c.htrue[key] = 4 * c.ref.w * sig * (1 - sig)
        else:
            c.htrue[key] = c.ref.w * np.exp(-E)
    return c.htrue[key]


def _hxx(Xw, h):
    """sum_k h_k x_ki x_kj in np.longdouble, exactly up to 2^-78 of max h per term: h cut into 26-bit pieces, +-1 GEMMs in float64"""
    mx = float(np.abs(h).max())
    s = LD(2.0) ** (np.frexp(mx)[1] if mx > 0 else 0)
    y = h / s
    out = np.zeros((Xw.shape[1], Xw.shape[1]), dtype=LD)
    for sh in (26, 52, 78):
        piece = np.round(y * LD(2.0) ** sh) / LD(2.0) ** sh
        out += ((Xw * piece.astype(np.float64)[:, None]).T @ Xw).astype(LD)
        y = y - piece
    return out * s


def _true_block(c, form, r, params, Kh, kstride):
    """(H_true [m][m] longdouble, sum h, Kh_nz) of row r's weights over the list `params` (reference order) and the sub-sample"""
    cfg = HR.compact_configs(Kh, kstride)
    idx = cfg[cfg < K]
    h = _true_h(c, form, r)[idx]
    X = c.ref.stats(int(c.nodes[r]), 0, K)[idx][:, params]
    return _hxx(np.ascontiguousarray(X), h), h.sum(), int((c.c[idx] > 0).sum())


def _layout(sizes, ntiles=0, T=0):
    mt = [(m + 31) // 32 for m in sizes] + [T // 32] * ntiles
    hoff = np.concatenate([[0], np.cumsum([(32 * m) ** 2 for m in mt])]).astype(np.int64)
    return np.array(mt, dtype=np.int32), hoff[:-1], int(max(hoff[-1], 1))


# ---------------------------------------------------------------------------------------------------------------------------
# one call and its checks
# ---------------------------------------------------------------------------------------------------------------------------
def run_and_check(c, form, prec, Kh, kstride, *, rows=NR, sizes=None, tiles=None, label=""):
    p = c.p
    sizes = list(SIZES[:rows] if sizes is None else sizes)
    nodes, theta, cols = c.nodes[:rows], c.theta[:rows], c.cols[:rows]
    nt = 0 if tiles is None else len(tiles["wrow"])
    T = 0 if tiles is None else tiles["T"]
    mtV, hoffV, htotal = _layout(sizes, nt, T)
    flag = np.array([m > 0 for m in sizes])
    if tiles is not None:
        flag |= np.asarray(tiles["hflag"]) != 0
        tiles = dict(tiles, hflag=flag.astype(np.int32))
    H = hessian_run(p, form, prec, nodes, theta, cols, mtV, hoffV, htotal, Kh, kstride, tiles)
    B = _bits(c)
    d = c.dims
    vq, mmax, tau = pass_state(p)
    hq, h64, mb = hess_state(p, want_mb=not c.mb_checked)
    vpl0, vscale = vq.shape[2] - 4, VSCALE[prec]
    assert vq.shape[2] == (6 if prec == "i8w" else 4)
    # 1. Mb
    if mb is not None:
        assert np.array_equal(mb, HR.mb_image(B[:d["Qfp"]], d["Kp"], d["Qfp"], d["Qp"])), "Mb"
        c.mb_checked = True
    Rp = (rows + 31) // 32 * 32
    assert hq.shape[3] == d["Kp"] and hq.shape[0] * 32 >= Rp and len(h64) >= htotal + Rp
    hS = h64[htotal:htotal + Rp]
    cfg = HR.compact_configs(Kh, kstride)
    # 2. Hq and hS;  5. skipped rows
    h2dev, shift = {}, {}
    ndiff = 0
    for r in range(rows):
        if not flag[r]:
            assert hS[r] == 0, (label, "hS of a skipped row", r)
            continue
        u = int(nodes[r])
        want, sh = HR.row_h2(vq, r, vpl0, u, B[u].astype(bool), int(mmax[r]), form, Kh, kstride, tau=tau[r], vscale=vscale, w=np.concatenate([c.w64, np.zeros(d["Kp"] - K)]))
        got = HR.hq_decode(hq, r, Kh)
        assert np.array_equal(got, want), (label, "Hq of row", r, int((got != want).sum()), int(np.abs(got - want).max()))
        assert np.array_equal(hq[r >> 5, :, r & 31, :Kh], HR.hq_encode(want)), (label, "digits of row", r)
        assert hS[r] == int(got.sum()), (label, "hS of row", r)
        if form != "RPLE":
            assert int(mmax[r]) >= (1 << 27 if prec == "i8w" else 1 << 23), (label, "the planes of row", r, "are not rescaled")
            if kstride == 1:  # (the row's largest weight is in the sum: the shift is the smallest that fits it)
                assert got.max() >= 16000, (label, "row", r, "does not use its 15 bits", int(got.max()))
        h2dev[r], shift[r] = got, sh
    assert not hS[rows:].any(), (label, "hS of the padding rows")
    # the blocks: rows, then tiles
    blocks = [(r, r, _internal(int(nodes[r]), cols[r, :32 * mtV[r]], d["cconst"]), cols[r, :32 * mtV[r]]) for r in range(rows) if mtV[r] > 0]
    for t in range(nt):
        wr = int(tiles["wrow"][t])
        blocks.append((rows + t, wr, _internal(int(nodes[wr]), tiles["tcols"][t], d["cconst"]), np.asarray(tiles["tcols"][t])))
    covered = np.zeros(htotal, dtype=bool)
    worst = 0.0
    for b, wr, F, params in blocks:
        m32 = len(F)
        low = HR.lower_tiles(m32)
        sl = slice(int(hoffV[b]), int(hoffV[b]) + m32 * m32)
        covered[sl] = True
        T64 = h64[sl].reshape(m32, m32)
        Td = H[sl].reshape(m32, m32)
        # 3. / 4. the integer block
        want = HR.t_block(h2dev[wr], B[F][:, cfg])
        assert np.array_equal(T64[low], want[low]), (label, "T of block", b, int((T64 != want)[low].sum()))
        assert not T64[~low].any(), (label, "upper tiles of H64, block", b)
        # 6. the finish
        fin = HR.finish(T64, int(hS[wr]), tau[wr], vscale, shift[wr])
        assert np.array_equal(Td[low], fin[low]), (label, "finish of block", b)
        assert not Td[~low].any(), (label, "upper tiles of H, block", b)
        # 7. against the true weights
        ref, sumh, knz = _true_block(c, form, wr, params, Kh, kstride)
        tv = tau[wr] * vscale
        ch = (1.0 if prec == "i8x" else 0.5) * (2.0 if form == "RPLE" else 1.0)
        bound = knz * (np.ldexp(tv, shift[wr]) + ch * tv) + 1e-13 * float(sumh)
        err = float(np.abs(Td.astype(LD) - ref)[low].max())
        worst = max(worst, err / bound)
        assert err <= bound, (label, "block", b, "measured / bound", err / bound)
    assert not H[~covered].any() and not h64[:htotal][~covered].any(), (label, "outside the blocks")
    # duplicated column: equal rows of the product
    if rows > DUP_ROW and sizes[DUP_ROW] > 5:
        Td = H[int(hoffV[DUP_ROW]):int(hoffV[DUP_ROW]) + (32 * mtV[DUP_ROW]) ** 2].reshape(32 * mtV[DUP_ROW], -1)
        assert np.array_equal(Td[5, :3], Td[2, :3]) and Td[5, 2] == Td[2, 2] == Td[5, 5]
    _ratios[label] = worst
    print(f"{label}: {len(blocks)} blocks, Kh = {Kh}, kstride = {kstride}: end-to-end measured / bound = {worst:.3g}")
    return H


CASES = [("RISE", "i8x", 1), ("RISE", "i8w", 1), ("logRISE", "i8w", 1), ("RPLE", "i8x", 1), ("RPLE", "i8w", 1),
         ("RISE", "i8x", 2), ("logRISE", "i8w", 3), ("RPLE", "i8x", 3), ("RISE", "i8w", 2), ("RPLE", "i8w", 2), ("RISE", "i8x", 3)]


@pytest.mark.parametrize("form,prec,kstride", CASES)
def test_blocks_are_the_models(ctx, form, prec, kstride):
    run_and_check(ctx, form, prec, 3072 // kstride, kstride, label=f"{form} {prec} kstride={kstride}")


@pytest.mark.parametrize("form,prec", [("RISE", "i8w"), ("RPLE", "i8x")])
@pytest.mark.parametrize("wgs", [1, 1 << 20])
def test_chunking_does_not_change_a_bit(ctx, form, prec, wgs):
    # wgs = 1: one chunk of all six 512-groups per block in both MFMA kernels -- the three-stage rings wrap; large: chunks of 1024
    base = run_and_check(ctx, form, prec, 3072, 1, label=f"{form} {prec} default split")
    with knobs(wgs):  # (restored on the way out, whatever happens inside)
        H = run_and_check(ctx, form, prec, 3072, 1, label=f"{form} {prec} split target {wgs}")
    assert np.array_equal(H, base)


def _tile_set(c, T):
    """9 tiles over 3 matrix-free rows (own size 0) in both node tiles; sizes in use: full, partial and 1"""
    rng = np.random.default_rng(T)
    cg = [13, 33, 37]
    vm = [T, T, 40, T, 1, T - 1, T, 17, T]
    wrow = [13, 13, 13, 33, 33, 33, 37, 37, 37]
    tcols = np.zeros((9, T), dtype=np.int32)
    for t in range(9):
        u = int(c.nodes[wrow[t]])
        lst = rng.choice(np.delete(np.arange(N), u), size=vm[t], replace=False)
        if t == 3:
            lst[0] = u
        tcols[t] = np.resize(lst, T)
    hflag = np.zeros(NR, dtype=np.int32)
    hflag[cg] = 1
    assert all(SIZES[r] == 0 for r in cg)
    return dict(T=T, tcols=tcols, vm=vm, wrow=wrow, hflag=hflag)


@pytest.mark.parametrize("form,prec,T,kstride", [("RISE", "i8x", 64, 1), ("logRISE", "i8w", 128, 1), ("RPLE", "i8w", 64, 3), ("RPLE", "i8x", 128, 2)])
def test_preconditioner_tiles_beside_row_blocks(ctx, form, prec, T, kstride):
    # the tiles are of the small size class: the one-workgroup kernel runs them with the rows' small blocks, the blocked kernel the
    # rows' large blocks alone
    run_and_check(ctx, form, prec, 3072 // kstride, kstride, tiles=_tile_set(ctx, T), label=f"{form} {prec} tiles T={T} kstride={kstride}")


def test_tiles_alone_and_rows_of_one_class(ctx):
    # only tiles (every row skipped but flagged or not), then only small rows, then only large rows: each launch on its own
    none = [0] * NR
    run_and_check(ctx, "RISE", "i8w", 3072, 1, sizes=none, tiles=_tile_set(ctx, 128), label="tiles alone")
    run_and_check(ctx, "RISE", "i8w", 3072, 1, sizes=[m if m <= 128 else 0 for m in SIZES], label="small rows alone")
    run_and_check(ctx, "RISE", "i8w", 1536, 2, sizes=[m if m > 128 else 0 for m in SIZES], label="large rows alone")


def test_second_call_reuses_the_buffers(ctx):
    # a full call, then fewer rows and smaller blocks on the same handle: Hq and H64 are not reallocated, their tails are stale
    run_and_check(ctx, "RISE", "i8x", 3072, 1, label="first call")
    before = hess_state(ctx.p)[1].size
    run_and_check(ctx, "RISE", "i8x", 1024, 3, rows=10, sizes=[33, 0, 31, 1, 129, 0, 64, 0, 32, 96], label="second call, 10 rows")
    assert hess_state(ctx.p)[1].size == before
    run_and_check(ctx, "logRISE", "i8x", 3072, 1, label="third call, all rows again")


@pytest.mark.parametrize("form", ["RISE", "RPLE"])
@pytest.mark.parametrize("kstride", [1, 3])
def test_fp64_blocks(ctx, form, kstride):
    c = ctx
    Kh = 3072 // kstride
    mtV, hoffV, htotal = _layout(SIZES)
    H = hessian_run(c.p, form, "f64", c.nodes, c.theta, c.cols, mtV, hoffV, htotal, Kh, kstride)
    covered = np.zeros(htotal, dtype=bool)
    worst = 0.0
    for r in range(NR):
        if mtV[r] == 0:
            continue
        m32 = 32 * int(mtV[r])
        low = HR.lower_tiles(m32)
        sl = slice(int(hoffV[r]), int(hoffV[r]) + m32 * m32)
        covered[sl] = True
        Td = H[sl].reshape(m32, m32)
        ref, sumh, _ = _true_block(c, form, r, c.cols[r, :m32], Kh, kstride)
        bound = (1e-12 + (Kh + 4) * 2.0 ** -53) * float(sumh)
        err = float(np.abs(Td.astype(LD) - ref)[low].max())
        worst = max(worst, err / bound)
        assert err <= bound, (form, kstride, r, err / bound)
        assert not Td[~low].any(), (form, kstride, "upper tiles of row", r)
    assert not H[~covered].any()
    print(f"f64 {form} kstride={kstride}: measured / bound = {worst:.3g}")
