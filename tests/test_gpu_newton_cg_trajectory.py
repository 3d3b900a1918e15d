"""The matrix-free direction phase of learn() (csrc/gml_newton_cg.cpp: the matrix-free half of direction_blocks, newton_cg,
newton_cg_group), iteration by iteration, against the host model of tests/_newton_cg_reference.py.  The solver records what this phase
did while the recorder of csrc/gml_testhooks.cpp is armed (gml_test_traj_cg_*; csrc/gml_solver.h: TRC_*); the rows need not converge,
what is held is each recorded iteration.

Decisions -- the group of every row, ksub, every plan and the step at which it was set, the fallback kpart = kchunk, the live list after
every step, the break at max_cg, the `again` list, the route, the control block of every product -- are recomputed from the record's
own numbers (CgState, kkt, nviol / nsupp, Z, FaceOut) and compared with ==.  wsub, sc and the tiles' s1 are held relative to nb 2^-52
(a sum of nb doubles in another order and the divisions), as tests/test_gpu_solver_trajectory.py holds hscale and s1.  A row's plane
slot must be the same in every control block of an iteration and no two rows may share one; whose planes a slot holds shows in the
products.

Tiles.  nW, t0, vm, wrow and FV (W in column order, padded with Qp - 1) equal the model's.  Every tile block before its inversion is
held per entry of its lower 32 x 32 tiles to the block of (row wrow[t], the tile's columns, the Kh / kstride sub-sample) with the
bound of tests/test_gpu_i8_hess_exact.py: Kh_nz (2^sh tau' + c_h tau') + 1e-13 sum h, sh from the row's recorded mmax, plus the rounding
of the float64 reference ((Kh + 8) 2^-53 sum h).  Every inverse is held to the inverse of s1 (the recorded block) - s2 g g^T by the
rule of test_tile_preconditioner_matches_numpy: 1e-9 of the largest entry; tiles numpy does not find positive definite are counted.

Products.  Every recorded raw product is held on W to sum_k h_k (x_k . p) x_k over k mod kchunk < kpart with the row's weights at its
iterate, by the product bound of tests/test_gpu_i8_pass_variants.py / tests/test_gpu_hv_sparse_direct.py: 1e-13 |f| + 3.3 sqrt(Kpart)
tau_hv + 3.3 sqrt(Kpart) c_h tau_V |p|_1 + d_p sum h, tau_V the recorded unit of the row's planes, plus the rounding of the float64
reference ((K + 2 P + 8) 2^-53 + (P + 2) 2^-53 |theta|_1) sum h |p|_1.  All products are checked; none is skipped.

PCG.  Every step is held from the device's previous state.  The replays of a row (float64 and long double, fed the record's inverted
tiles and products) take the recorded Rv, Pv and rz before a step; their pHp is held; they take the step length from the device's pHp;
then rs after the step, Rv, Pv and rz before the next step (the preconditioner and the direction kernel), D at the end of every round
(the sum of the steps) and the state after every face re-solve are held -- all to the long-double replay by the rule of
test_pcg_kernels_match_the_host_model: 16 x |float64 replay - long-double replay| + |W| 2^-53 scale (4 |W| 2^-53 for the scalars).
Why the cuts are this fine.  Replays that run on from their own state take their products from the device's direction, not from their
own, and leave the rule (hv_subsample-3, row 35, |W| = 12, step 0: rs off by 49 x 2^-53 with 48 allowed; polish, row 21, |W| = 41,
step 5: 577 x 2^-53 with 334 allowed).  Cut at the state alone, a first step that reduces the residual 38-fold turns one unit in the last
place of the device's pHp (a tree sum; numpy's sum of the 8 terms came out correctly rounded in both replays, so delta_k was 0) into
74 x 2^-53 of rs with 32 allowed (hv_subsample-1, row 30, |W| = 8); with the device's pHp in the step length the two replays differ by
the rounding of that division and of the update, as the device does.  nfixed, mass and total of the faces come from the device's own
D; both replays go on from the device's D after a face round.

An armed and an unarmed run of a case give the same out, kkt, iterations, passes and hv_evals.

Measured on an MI355X (HISTORY.md section 25; each test prints its own as "NEWTON-CG <case>: ..."), per case: products checked /
skipped, largest product error over its bound, largest tile-block error over its bound, largest PCG distance over delta_k and over
what the rule allows:
  one-tile           583 / 0   0.606   0.066   16   0.52        weightless         132 / 0   0.712   0.082   16   0.83
  two-tile-RISE      140 / 0   0.182   0.036    5   0.06        hv_subsample-1     124 / 0   0.771   0.050   16   0.32
  two-tile-logRISE   142 / 0   0.256   0.034    3   0.06        hv_subsample-3     124 / 0   0.661   0.056   16   0.22
  two-tile-RPLE      117 / 0   0.067   0.033    5   0.06        cap                570 / 0   0.606   0.066   16   0.52
  order-3             32 / 0   0.157   0.032    4   0.05        fp64-phase         124 / 0   0.606   0.050   12   0.84
  polish            6013 / 0   0.606   0.067   16   0.52
Every tile inverse lies within 4.1e-15 of the largest entry of numpy's; numpy found every tile positive definite.  None of the
thresholds is fitted to these figures.  The fp64-phase case found the FP64 phase's borrowed int8 pass running with the previous iterate's
scale (its tile block of row 0 was off by 1 963 x the bound, mmax 4 140 806 889 beyond the 31 bits of the planes): gml_solver.cpp now
adds an accepted FP64 step's |step|_1 to dref."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _i8_hess_reference as HR
import _newton_cg_reference as N
import gml_amd as gml
from oracle import oracle as O
from test_gpu_i8_pass_variants import need_ld, quant_defect

_lib = importlib.import_module("gml_amd._lib")
synthetic = importlib.import_module("gml_amd.synthetic")
pytestmark = [pytest.mark.gpu, need_ld]
P_ = _lib._ptr
U53 = 2.0 ** -53
VSCALE = {1: 1.0, 3: 65536.0}  # by GML_PREC_* of the planes
_tallies = {}


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def _data(which):
    if which == "n48":
        spins = synthetic.block_ising(48, 14000, block=16, seed=5)[0]
    elif which == "n160":
        spins = synthetic.block_ising(160, 26000, block=16, seed=6)[0]
    else:
        spins = synthetic.block_ising(20, 26000, block=10, seed=7)[0]
    counts = np.random.default_rng(len(spins)).integers(0, 4, size=len(spins)).astype(np.float64)
    return spins, counts


_cache = {}


def data(which, zero_blocks=()):
    key = (which, tuple(zero_blocks))
    if key not in _cache:
        spins, counts = _data(which)
        counts = counts.copy()
        for b in zero_blocks:
            counts[512 * b:512 * b + 512] = 0
        w = counts / counts.sum()
        Kp = (len(spins) + 1023) // 1024 * 1024
        wblk = np.zeros(Kp // 512)
        for b in range(len(wblk)):  # (in the order of the library's sum: configuration by configuration)
            s = 0.0
            for v in w[512 * b:512 * b + 512]:
                s += float(v)
            wblk[b] = s
        _cache[key] = dict(spins=spins, counts=counts, w=w, wblk=wblk, Kp=Kp, S=spins.astype(np.float64))
    return _cache[key]


def case(data="n48", form="RISE", c=0.05, nodes=(0, 40), order=2, prec="i8x", max_working=32, max_iter=3, tol=1e-7, hv_subsample=0, max_cg=0,
         cg_eta=0.0, ratio=0.3, polish=False, knobs=None, zero_blocks=(), hess_samples=1024):
    return dict(data=data, form=form, c=c, nodes=nodes, order=order, prec=prec, max_working=max_working, max_iter=max_iter, tol=tol,
                hv_subsample=hv_subsample, max_cg=max_cg, cg_eta=cg_eta, ratio=ratio, polish=polish, knobs=knobs or {}, zero_blocks=zero_blocks, hess_samples=hess_samples)


CASES = {
    "one-tile": case(max_iter=9),
    "two-tile-RISE": case("n160", max_working=128, max_iter=8, hess_samples=4096),
    "two-tile-logRISE": case("n160", "logRISE", max_working=128, max_iter=8, hess_samples=4096),
    "two-tile-RPLE": case("n160", "RPLE", max_working=128, max_iter=8, hess_samples=4096),
    "order-3": case("n20", order=3, nodes=(0, 20), max_working=64, max_iter=4, hess_samples=4096),
    "weightless": case(zero_blocks=(0, 8, 16, 24)),
    "hv_subsample-1": case(hv_subsample=1),
    "hv_subsample-3": case(hv_subsample=3),
    "cap": case(max_cg=3, max_iter=9),
    "fp64-phase": case(prec="f64"),
    "polish": case(tol=1e-11, max_iter=40, polish=True),
}


def _hooks():
    L = _lib.lib()
    L.gml_test_tune.restype = C.c_double
    L.gml_test_tune.argtypes = [C.c_int, C.c_double]
    L.gml_test_hv_sparse_ratio.restype = C.c_double
    L.gml_test_hv_sparse_ratio.argtypes = [C.c_double]
    L.gml_test_traj_cg_count.argtypes = [C.c_int, C.c_void_p]
    L.gml_test_traj_cg_event.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.gml_test_traj_cg_data.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.gml_test_traj_iter.argtypes = [C.c_int] + [C.c_void_p] * 5
    L.gml_test_i8_pack_state.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    return L


def run(cs, armed=True):
    """one learn() of the case: (out, kkt, stats, records, dims).  records: per recorded iteration dict(hdr, events); dims of the handle"""
    L = _hooks()
    d = data(cs["data"], cs["zero_blocks"])
    old = {k: L.gml_test_tune(k, float(v)) for k, v in cs["knobs"].items()}
    old_ratio = L.gml_test_hv_sparse_ratio(float(cs["ratio"]))
    L.gml_test_traj_arm(1 if armed else 0)
    recs = []
    try:
        with gml.Problem(spins=d["spins"], counts=d["counts"], order=cs["order"], node_range=cs["nodes"]) as p:
            out, kkt, st = p.learn(cs["form"], cs["c"], tol=cs["tol"], max_iter=cs["max_iter"], precision=cs["prec"], max_working=cs["max_working"], hess_samples=cs["hess_samples"],
                                   polish=cs["polish"], hv_subsample=cs["hv_subsample"], max_cg=cs["max_cg"], cg_eta=cs["cg_eta"], raise_on_fail=False)
            dm = np.zeros(20, dtype=np.int64)
            _lib.check(L.gml_test_i8_pack_state(p._h, 0, P_(dm), None))
            dims = dict(Qp=int(dm[6]), Qfp=int(dm[7]), cconst=int(dm[9]), Kp=int(dm[10]), K=int(dm[11]), P=p.P)
        if armed:
            tdims = np.zeros(8, dtype=np.int64)
            _lib.check(L.gml_test_traj_dims(P_(tdims)))
            n, R, Qp = int(tdims[0]), int(tdims[1]), int(tdims[2])
            assert Qp == dims["Qp"] and R == cs["nodes"][1] - cs["nodes"][0]
            for i in range(n):
                hdr = np.zeros(int(tdims[4]))
                _lib.check(L.gml_test_traj_iter(i, P_(hdr), None, None, None, None))
                ne = np.zeros(1, dtype=np.int64)
                _lib.check(L.gml_test_traj_cg_count(i, P_(ne)))
                evs = []
                for e in range(int(ne[0])):
                    ed = np.zeros(3, dtype=np.int64)
                    _lib.check(L.gml_test_traj_cg_event(i, e, P_(ed)))
                    iv, dv = np.zeros(max(1, int(ed[1])), dtype=np.int64), np.zeros(max(1, int(ed[2])))
                    _lib.check(L.gml_test_traj_cg_data(i, e, P_(iv), P_(dv)))
                    evs.append(N.parse_event(int(ed[0]), iv[:int(ed[1])], dv[:int(ed[2])], Qp))
                recs.append(dict(hdr=hdr, events=evs))
    finally:
        L.gml_test_traj_arm(0)
        L.gml_test_hv_sparse_ratio(old_ratio)
        for k, v in old.items():
            L.gml_test_tune(k, v)
    return out, kkt, st, recs, dims


# ---- the references of one row ---------------------------------------------------------------------------------------------------------
_keys = {}


def stats(cs, d, u):
    """x_k of node u in the order of the result's parameters, [K][P] float64"""
    S = d["S"]
    if cs["order"] == 2:
        X = S * S[:, [u]]
        X[:, u] = S[:, u]
        return X
    n = S.shape[1]
    if (n, u) not in _keys:
        _keys[(n, u)] = O.multi_keys(n, cs["order"], u)
    X = np.ones((len(S), len(_keys[(n, u)])))
    for j, key in enumerate(_keys[(n, u)]):
        for s in key:
            X[:, j] *= S[:, s]
    return X


def row_checker(cs, d, dims, b, tally):
    """product(i, row, items) of check_iteration for one iteration (its `blocks` event b); holds the row's tile blocks on the way"""
    form, K, Qp = cs["form"], dims["K"], dims["Qp"]
    vscale = VSCALE[1 if b["prec"] == 0 else b["prec"]]  # (the FP64 phase borrows i8x passes for the planes)
    ch = 2.0 if form == "RPLE" else 1.0
    s2 = 1.0 if form == "logRISE" else 0.0
    T_ = b["T"]

    def product(i, r, items):
        u = cs["nodes"][0] + r
        cols = b["cols"][i]
        if cs["order"] == 2:  # the stated layout: parameter j in column j, the node's field in the constant column
            assert list(cols) == [dims["cconst"] if j == u else j for j in range(dims["P"])]
        Xs = stats(cs, d, u)
        Pn = Xs.shape[1]
        theta = b["X"][i][cols]
        E = Xs @ theta
        h = N.curvature_weights(form, d["w"], E)
        if form == "RPLE":
            t = -2 * E
            f = float((d["w"] * (np.maximum(t, 0) + np.log1p(np.exp(-np.abs(t))))).sum())
        else:
            f = float(h.sum())
        th1 = float(np.abs(theta).sum())
        # -- the tile blocks of this row before their inversion, and their inverses
        where = np.full(Qp, -1)
        where[cols] = np.arange(Pn)
        cfg = HR.compact_configs(b["Kh"], b["kstride"])
        cfg = cfg[cfg < K]
        tv = float(b["tau"][i]) * vscale
        sh = HR.hw_shift(int(b["mmax"][i]), form)
        knz = int((d["counts"][cfg] > 0).sum())
        sumh = float(h[cfg].sum())
        chb = (1.0 if vscale == 1.0 else 0.5) * ch
        Xc, hc = Xs[cfg], h[cfg]
        for t in range(int(b["t0"][i]), int(b["t0"][i]) + -(-int(b["nW"][i]) // T_)):
            assert int(b["wrow"][t]) == r
            m = int(b["vm"][t])
            pc = where[b["FV"][t, :m]]
            assert (pc >= 0).all()
            Xt = Xc[:, pc]
            ref = (Xt * hc[:, None]).T @ Xt
            low = (np.arange(m)[:, None] // 32) >= (np.arange(m)[None, :] // 32)
            bound = knz * (np.ldexp(tv, sh) + chb * tv) + 1e-13 * sumh + (len(cfg) + 8) * U53 * sumh
            err = float(np.abs(b["Hpre"][t, :m, :m] - ref)[low].max())
            tally.block = max(tally.block, err / bound)
            tally.blocks_held += 1
            assert err <= bound, ("tile block", t, "of row", r, "measured / bound", err / bound, "tau", tv, "mmax", int(b["mmax"][i]), "shift", sh,
                                  b["Hpre"][t, :2, :2], ref[:2, :2])
            Hl = np.where(low, b["Hpre"][t, :m, :m], 0.0)
            Hs = np.where(low, Hl, Hl.T)
            g = b["G"][i][b["FV"][t, :m]]
            A = float(b["s1"][i]) * Hs - s2 * np.outer(g, g)
            try:
                np.linalg.cholesky(A)
            except np.linalg.LinAlgError:
                tally.fallback_tiles += 1
                continue
            want = np.linalg.inv(A)
            ierr = float(np.abs(b["Hinv"][t, :m, :m] - want).max() / np.abs(want).max())
            tally.inverse = max(tally.inverse, ierr / 1e-9)
            assert ierr <= 1e-9, ("inverse of tile", t, "of row", r, ierr)
        # -- the products
        V = np.stack([e["vec"][k][cols] for e, k, _, _ in items], axis=1)
        Tm = Xs @ V
        masks = {}
        for j, (e, k, kchunk, kpart) in enumerate(items):
            if (kchunk, kpart) not in masks:
                masks[(kchunk, kpart)] = ((np.arange(K) % kchunk) < kpart).astype(np.float64)
            Tm[:, j] *= h * masks[(kchunk, kpart)]
        Om = Xs.T @ Tm
        out = []
        for j, (e, k, kchunk, kpart) in enumerate(items):
            mk = masks[(kchunk, kpart)]
            kp = float(mk.sum())
            hsum = float((h * mk).sum())
            pv = V[:, j]
            p1 = float(np.abs(pv).sum())
            mx = float(np.abs(pv).max())
            sg = 2.0 ** ((np.frexp(mx)[1] if mx > 0 else 0) - 14)
            emax = float(np.abs(np.rint(pv / sg)).sum() * sg)
            tau_v = float(e["tau"][k]) * vscale
            tau_h = tau_v * (emax if emax > 0 else 1.0) * 65536.0 * 1.01
            bound = (1e-13 * abs(f) + 3.3 * np.sqrt(kp) * tau_h + 3.3 * np.sqrt(kp) * ch * tau_v * p1 + quant_defect(pv[None, :], 2)[0] * hsum
                     + ((K + 2 * Pn + 8) * U53 + (Pn + 2) * U53 * th1) * hsum * p1)
            ref = np.zeros(Qp)
            ref[cols] = Om[:, j]
            out.append((ref, bound))
        return out

    return product


def hold(name, cs):
    """the armed run of a case with every recorded iteration held; returns (tally, out, kkt, stats, records)"""
    out, kkt, st, recs, dims = run(cs, armed=True)
    d = data(cs["data"], cs["zero_blocks"])
    assert dims["Kp"] == d["Kp"] and dims["K"] == len(d["spins"])
    R = cs["nodes"][1] - cs["nodes"][0]
    par = dict(K=dims["K"], Kp=dims["Kp"], Qfp=dims["Qfp"], R=R, Rp=-(-R // 32) * 32, node0=cs["nodes"][0], form=cs["form"], order=cs["order"], tol=cs["tol"],
               hv_subsample=cs["hv_subsample"], max_cg=cs["max_cg"], cg_eta=cs["cg_eta"], ratio=cs["ratio"])
    tally = N.Tally()
    tally.iterations = 0
    tally.precs = set()
    for it, rec in enumerate(recs):
        if not rec["events"]:
            continue
        b = rec["events"][0]
        N.check_iteration(rec["events"], par, d["wblk"], tally, product=row_checker(cs, d, dims, b, tally))
        tally.iterations += 1
        tally.precs.add(int(rec["hdr"][8]))
    print(f"NEWTON-CG {name}: {tally.iterations} iterations with matrix-free rows of {len(recs)} (solver precisions {sorted(tally.precs)}), branches "
          f"{sorted(tally.seen)}; products checked {tally.checked}, skipped {tally.skipped}, largest error / bound {tally.product:.3g}; tile blocks held "
          f"{tally.blocks_held}, largest error / bound {tally.block:.3g}, inverses {tally.inverse:.3g} x 1e-9, tiles not positive definite "
          f"{tally.fallback_tiles}; largest PCG distance / delta_k {tally.pcg:.3g}, / what the rule allows {tally.pcg_allowed:.3g}")
    assert tally.iterations > 0, "no iteration took the matrix-free branch"
    _tallies[name] = tally
    return tally, out, kkt, st, recs


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.mark.parametrize("name", list(CASES))
def test_recorded_iterations_follow_the_model(name):
    """The cases (counts in {0 .. 3}, spins of synthetic.block_ising, c = 0.05, i8x, tol 1e-7, three iterations unless said):
      one-tile          pairwise n = 48, K = 14 000 (Kp = 14 336), nodes [0, 40), max_working = 32: |W| <= 47 < the tile, ksub = 8, kchunk = 4096,
                        kpart = 512, both relax factors apply
      two-tile-*        n = 160, K = 26 000, max_working = 128, nodes [0, 40): a full and a partial tile per row; RISE, logRISE (1 / Z in sc,
                        s2 = 1), RPLE (the GEMM route always)
      order-3           n = 20, order 3 (P = 191), K = 26 000, max_working = 64: the multi-body column map in FV
      weightless        one-tile without counts on the blocks 0, 8, 16, 24 the coarse plan samples: kpart = kchunk, sc without 1 / wsub
      hv_subsample-1/3  no coarse group and no relax; a forced ksub for the coarse group and no relax
      cap               max_cg = 3: the loop ends with rows still live
      fp64-phase        precision f64: the planes come from an extra int8 objective pass, s1cg still holds
      polish            i8x to tol 1e-11 with the polish on: the FP64 phase reopens matrix-free rows"""
    cs = CASES[name]
    tally, out, kkt, st, recs = hold(name, cs)
    out2, kkt2, st2, _, _ = run(cs, armed=False)
    assert same_bits(out, out2) and same_bits(kkt, kkt2), "an armed and an unarmed run differ"
    assert all(st[k] == st2[k] for k in ("iterations", "passes", "hv_evals")), (st, st2)
    if name == "one-tile":
        plans = [e for r in recs for e in r["events"] if e["tag"] == "plan"]
        assert any((e["ksub"], e["kchunk"], e["kpart"]) == (8, 4096, 512) for e in plans) and {"relax2", "relax4"} <= tally.seen
    if name.startswith("two-tile"):
        bl = [r["events"][0] for r in recs if r["events"]]
        assert any((b["nW"] > 128).sum() >= 16 for b in bl), "rows with a full and a partial tile"
        assert all(list(b["vm"][b["t0"][i]:b["t0"][i] + 2]) == [128, m - 128] for b in bl for i, m in enumerate(b["nW"]) if m > 128)
        ks = {e["ksub"] for r in recs for e in r["events"] if e["tag"] == "plan" and e["where"] == 0 and e["ksub"] > 1}
        assert name == "two-tile-RPLE" or (ks and all(2 <= k <= 8 for k in ks)), ks
        if name == "two-tile-logRISE":
            assert all(abs(z - 1) > 1e-3 for r in recs for e in r["events"] if e["tag"] == "group" for z in e["Z"])
        if name == "two-tile-RPLE":
            assert "entries" not in tally.seen and "gemm" in tally.seen
    if name == "weightless":
        assert "weightless" in tally.seen
    if name == "hv_subsample-1":
        assert "coarse" not in tally.seen and not {"relax2", "relax4"} & tally.seen
    if name == "hv_subsample-3":
        assert "coarse" in tally.seen and not {"relax2", "relax4"} & tally.seen
        assert all(e["ksub"] in (1, 3) for r in recs for e in r["events"] if e["tag"] == "plan")
    if name == "cap":
        assert "cap" in tally.seen
    if name == "fp64-phase":
        assert tally.precs == {0}
    if name == "polish":
        assert st["polished"] == 1 and {0, 1} <= tally.precs, (st["polished"], tally.precs)


def test_route_follows_the_ratio_and_does_not_change_a_bit():
    """gml_test_hv_sparse_ratio at -1 (never entry by entry), at 1e30 (always) and at 0.3: the recorded route of every product follows the
    rule (held by the comparison), and the three recorded trajectories are equal bit for bit"""
    res = {}
    for ratio in (-1.0, 0.3, 1e30):
        cs = dict(CASES["one-tile"], ratio=ratio)
        tally, out, kkt, st, recs = hold(f"routes {ratio:g}", cs)
        res[ratio] = (tally, out, kkt, st, recs)
    assert "entries" not in res[-1.0][0].seen and "gemm" not in res[1e30][0].seen and {"entries", "gemm"} <= res[0.3][0].seen
    base = res[0.3]
    for ratio in (-1.0, 1e30):
        t, out, kkt, st, recs = res[ratio]
        assert same_bits(out, base[1]) and same_bits(kkt, base[2]) and all(st[k] == base[3][k] for k in ("iterations", "passes", "hv_evals"))
        assert len(recs) == len(base[4])
        for ra, rb in zip(recs, base[4]):
            assert len(ra["events"]) == len(rb["events"])
            for ea, eb in zip(ra["events"], rb["events"]):
                assert ea["tag"] == eb["tag"]
                W = None
                for key in ea:
                    if key in ("sparse", "tag"):
                        continue
                    va, vb = ea[key], eb[key]
                    if key == "ctl":
                        assert all(np.array_equal(va[k], vb[k]) for k in va)
                    elif key == "Hp":  # (the entry-by-entry form writes the listed entries only)
                        bl = ra["events"][0]
                        for k, r in enumerate(ea["rows"]):
                            i = list(bl["cg_rows"]).index(int(r))
                            W = N.working_set(bl["X"][i], bl["PG"][i], bl["kind"][i])
                            assert same_bits(va[k][W], vb[k][W]), (ratio, ea["tag"], "Hp of row", int(r))
                    elif isinstance(va, np.ndarray) and va.dtype == np.float64:
                        assert same_bits(va, vb), (ratio, ea["tag"], key)
                    else:
                        assert np.array_equal(va, vb), (ratio, ea["tag"], key)


def test_every_branch_was_recorded():
    """over all cases, at least once each: a coarse group, a fine group, a plan change at step 2 and one at step 4, a face re-solve, the
    entries route, the GEMM route, a live list that shrank inside a node tile, the weightless fallback (and the cap, and the FP64 phase)"""
    assert len(_tallies) >= len(CASES), "run the whole file: the coverage is over all cases"
    seen = set().union(*(t.seen for t in _tallies.values()))
    print("NEWTON-CG branches over all cases:", sorted(seen))
    assert {"coarse", "fine", "relax2", "relax4", "resolve", "entries", "gemm", "shrank", "weightless", "cap"} <= seen, sorted(seen)
