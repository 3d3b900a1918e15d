"""learn()'s Newton iterations, step by step, against the host model of tests/_trajectory_reference.py: the solver records every outer
iteration while the recorder of csrc/gml_testhooks.cpp is armed (gml_test_traj_*; csrc/gml_solver.h: TrajRecorder), and every recorded
decision of the host logic of csrc/gml_solver.cpp -- the Hessian budget and its rescaling, the secant switch, the noise levels, the line
search, the stall and best-iterate bookkeeping, finish -- is compared with the model's.  Precision f64, Cholesky rows only; the int8
precisions are held to the schedule (set_kh at the recorded nactive and Z), their Hessians being dithered.

Discrete fields are equal.  hscale and s1 are held relative to nb 2^-52 (a sum of nb doubles in another order, and one division).
X, kkt, Fobj and Z per (row, iteration) are held to MARGIN times the gap between the model's long-double and float64 runs at the same
record (the largest over the row for X), plus a floor of 8 ulp of the row's scale (1 for kkt and Z, whose terms are weights that sum to
one; max(1, |Fobj|); max |x| of the row).  Records from a row's first fragile decision on are left out (_trajectory_reference.fragile_map;
tests/test_host_trajectory_reference.py asserts the cap on them without a GPU).

Measured on an MI355X (HISTORY.md section 23): the largest device-to-model distance of any held number beyond its floor, in units of the
model's long-double-to-float64 gap at the same record, per case (each test prints its own as "GAPS"):
  strided-RISE 0.97, strided-logRISE 1.14, strided-RPLE 1.19, every-RISE 10.3, adaptive-RISE 0.86, weightless-RISE 0.03, scale-logRISE 0.69,
  backtrack-RISE 0.65, faces-RISE 0.97, cap-RISE 0.97, shard-RISE 0.97; no record was left out in any case.
MARGIN = 1e3 is the smallest power of ten that clears the largest (10.3) with at least 10x to spare (1e2 would leave 9.7x); every
case re-asserts the 10x on its own measurement."""
import ctypes as C

import numpy as np
import pytest

import _trajectory_reference as T
from gml_amd import _lib
import gml_amd as gml

pytestmark = pytest.mark.gpu

MARGIN = 1e3
U52 = 2.0 ** -52
H = dict(it=0, nactive=1, Kh=2, kstride=3, hscale=4, secant=5, rounds=6, stall_cap=7, prec=8, line_search=9)
RW = dict(done=0, atfloor=1, kkt=2, best=3, Fobj=4, stall=5, m=6, nsupp=7, nviol=8, f=9, fn=10, Z=11, s1=12, ynoise=13, npairs=14, trials=15, alpha=16,
          nreg=17, full=18, accepted=19, gave_up=20)
P = _lib._ptr


def run(case, polish=True):
    """one learn() of the case with the recorder armed: (records, out, kkt, stats, from_best or None, last error)"""
    L = _lib.lib()
    L.gml_test_tune.restype = C.c_double
    L.gml_test_tune.argtypes = [C.c_int, C.c_double]
    L.gml_test_traj_iter.argtypes = [C.c_int] + [C.c_void_p] * 5
    old = {k: L.gml_test_tune(k, float(v)) for k, v in case.knobs.items()}
    L.gml_test_traj_arm(1)
    try:
        with gml.Problem(spins=case.spins, counts=case.counts, node_range=(case.node0, case.node1)) as p:
            out, kkt, st = p.learn(case.form, case.c, tol=case.tol, max_iter=case.max_iter, precision=case.prec, hess_samples=case.hess_samples,
                                   polish=polish, raise_on_fail=False)
        err = L.gml_last_error().decode()
        dims = np.zeros(8, dtype=np.int64)
        _lib.check(L.gml_test_traj_dims(P(dims)))
        n, R, Qp, cap, nh, nr, fin = (int(v) for v in dims[:7])
        assert (R, Qp, cap, nh, nr) == (case.R, case.Qp, T.CAP, 12, 24), dims
        recs = []
        for i in range(n):
            hdr, rows, F, X, hx = np.zeros(nh), np.zeros((R, nr)), np.zeros((R, cap), dtype=np.int32), np.zeros((R, Qp)), C.c_int(0)
            _lib.check(L.gml_test_traj_iter(i, P(hdr), P(rows), P(F), P(X), C.byref(hx)))
            recs.append(dict(hdr=hdr, rows=rows, F=F, X=X if hx.value else None))
        fb = None
        if fin:
            fb = np.zeros(R, dtype=np.uint8)
            _lib.check(L.gml_test_traj_finish(P(fb)))
    finally:
        L.gml_test_traj_arm(0)
        for k, v in old.items():
            L.gml_test_tune(k, v)
    return recs, out, kkt, st, fb, err


def close(dev, hi, lo, scale, worst, tag):
    """|dev - hi| within MARGIN x max |hi - lo| + 8 ulp of scale; notes the distance in units of the gap term"""
    dev, hi, lo = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (dev, hi, lo))
    if not np.isfinite(hi).all():  # (no best iterate yet)
        assert np.array_equal(dev, hi), tag
        return
    gap = float(np.abs(hi - lo).max())
    d = float(np.abs(dev - hi).max())
    floor = 8 * U52 * scale
    if d > floor:
        worst[0] = max(worst[0], (d - floor) / gap if gap > 0 else float("inf"))
    assert d <= MARGIN * gap + floor, (tag, d, gap, floor)


@pytest.mark.parametrize("name", T.F64_CASES)
def test_f64_trajectory_matches_the_model(name):
    """The cases (n = 24, K = 5 000 -- 10 blocks of 512 -- unless said; counts in {0 .. 3}; tol 1e-7):
      strided (RISE, logRISE, RPLE)  hess_samples = 1024: two blocks, kstride 5, hscale = 1 / (wblk[0] + wblk[5]), secant on, 0 -> 1 -> 2 pairs
      every        hess_samples = -1: Kh = Kp, hscale = 1, no secant, no pairs
      adaptive     n = 16, K = 9 000, knob 0 = 1024, one strongly coupled node: Kh follows R // nactive up to "take it all"
      weightless   no counts on exactly the sampled blocks 0 and 5: every block, hscale = 1
      scale        logRISE with Z down to 0.77: s1 = hscale / Z of the iterate, also after a rejected trial
      backtrack    full steps rejected: alpha 1 -> 1/2 on a forward-only trial (the gradient pass follows), and in the noise regime
      faces        knob 1 = 3: two face rounds inside the solve
      cap          max_iter = 3: not converged; out is the best iterate per row, kkt_out = min(best, kkt)
      shard        nodes [5, 13): R = 8 in the budget, rows by local index
    Measured distances (GAPS) are printed per case."""
    case, hi, lo, first, why = T.model(name)
    recs, out, kkt, st, fb, err = run(case)
    worst = [0.0]
    assert len(recs) == len(hi["iters"]), (len(recs), len(hi["iters"]))
    assert st["iterations"] == hi["iterations"] and st["not_converged"] == hi["not_converged"]
    for i, (dv, mh, ml) in enumerate(zip(recs, hi["iters"], lo["iters"])):
        h = dv["hdr"]
        assert (h[H["it"]], h[H["stall_cap"]], h[H["prec"]]) == (mh["it"], 10, 0), (i, h)
        live = first > i
        if live.all():  # (what depends on every row)
            assert (h[H["nactive"]], h[H["Kh"]], h[H["kstride"]], h[H["secant"]], h[H["rounds"]], h[H["line_search"]]) == \
                (mh["nactive"], mh["Kh"], mh["kstride"], mh["secant"], mh["rounds"], int(mh["line_search"])), (i, h, mh["Kh"], mh["kstride"])
            if mh["line_search"]:
                nb = mh["Kh"] // 512
                assert abs(h[H["hscale"]] - mh["hscale"]) <= nb * U52 * mh["hscale"], (i, h[H["hscale"]], mh["hscale"])
        for r in np.flatnonzero(live):
            q, a, b = dv["rows"][r], mh["rows"][r], ml["rows"][r]
            tag = (name, i, r)
            assert (q[RW["done"]], q[RW["atfloor"]], q[RW["stall"]]) == (a["done"], a["atfloor"], a["stall"]), tag
            close(q[RW["kkt"]], a["kkt"], b["kkt"], 1.0, worst, tag + ("kkt",))
            close(q[RW["best"]], a["best"], b["best"], 1.0, worst, tag + ("best",))
            close(q[RW["Fobj"]], a["Fobj"], b["Fobj"], max(1.0, abs(a["Fobj"])), worst, tag + ("Fobj",))
            close(q[RW["Z"]], a["Z"], b["Z"], 1.0, worst, tag + ("Z",))
            if a["selected"]:
                m = a["m"]
                assert (q[RW["m"]], q[RW["nsupp"]], q[RW["nviol"]]) == (m, a["nsupp"], a["nviol"]), tag
                assert list(dv["F"][r, :m]) == list(a["F"]), tag
            if not (mh["line_search"] and a.get("trials", 0) > 0):
                continue
            # the noise of f, from the recorded f and Z alone: bit for bit
            fv = q[RW["Z"]] if case.form == "logRISE" else q[RW["f"]]
            fn = 1e-13 * max(1.0, abs(fv)) / (fv if case.form == "logRISE" else 1.0)
            assert q[RW["fn"]] == fn and q[RW["ynoise"]] == 100.0 * fn, tag
            nb = mh["Kh"] // 512
            s1 = mh["hscale"] / (q[RW["Z"]] if case.form == "logRISE" else 1.0)  # (the device's own Z, held above)
            assert abs(q[RW["s1"]] - s1) <= nb * U52 * s1, tag + (q[RW["s1"]], s1)
            got = (q[RW["npairs"]], q[RW["trials"]], q[RW["alpha"]], q[RW["nreg"]], q[RW["full"]], q[RW["accepted"]], q[RW["gave_up"]])
            want = (a["npairs"], a["trials"], a["alpha"], a["nreg"], a["full"], a["accepted"], a["gave_up"])
            assert got == tuple(float(v) for v in want), tag + (got, want)
            close(dv["X"][r], a["X"], b["X"], max(float(np.abs(a["X"]).max()), 1e-300), worst, tag + ("X",))
    n = len(recs)
    fin = first >= n
    assert fb is not None and (fb[fin] == hi["from_best"][fin]).all()
    for r in np.flatnonzero(fin):
        close(out[r], hi["rows"][r], lo["rows"][r], max(float(np.abs(hi["rows"][r]).max()), 1e-300), worst, (name, "out", r))
        close(kkt[r], hi["kkt"][r], lo["kkt"][r], 1.0, worst, (name, "kkt_out", r))
    if hi["not_converged"]:
        assert "did not reach the KKT tolerance" in err
    print(f"GAPS {name}: iterations {hi['iterations']}, records left out {int((n - np.minimum(first, n)).sum())} of {n * case.R}, "
          f"largest device-to-model distance {worst[0]:.3g} x the model's long-double-to-float64 gap")
    assert worst[0] * 10 <= MARGIN


@pytest.mark.parametrize("prec,form", [("i8w", "RISE"), ("i8x", "logRISE")])
def test_int8_schedule_follows_set_kh(prec, form):
    """n = 8, K = 140 000 (274 blocks), hess_samples = 0: Kh_base = clamp(2^23 / 8, 32 768, 131 072) = 131 072 on the int8 paths (32 768 on
    the FP64 path).  The recorded Kh, kstride, hscale, secant and s1 of every iteration are the model's set_kh at the RECORDED nactive
    and Z; the trajectory itself is the int8 Hessians' own."""
    spins, counts = T.histogram(8, 140000, 7, J=0.3)
    case = T.Case(f"i8-{form}", spins, counts, form, {"RISE": 0.4, "logRISE": 0.8}[form], tol=1e-7, prec=prec)
    assert case.base == 131072 and T.kh_base("f64", 8, case.Kp) == 32768
    recs, out, kkt, st, fb, err = run(case, polish=False)
    seen = set()
    for dv in recs:
        h = dv["hdr"]
        if not h[H["line_search"]]:
            continue
        kh = T.set_kh(case.K, case.Kp, case.R, int(h[H["nactive"]]), case.base, 0, case.wblk)
        seen.add(kh["Kh"])
        assert (h[H["Kh"]], h[H["kstride"]], h[H["secant"]], h[H["prec"]]) == (kh["Kh"], kh["kstride"], int(kh["Kh"] < case.Kp), T.PREC[prec]), h
        assert abs(h[H["hscale"]] - kh["hscale"]) <= kh["nb"] * U52 * kh["hscale"], (h[H["hscale"]], kh["hscale"])
        for r in range(case.R):
            q = dv["rows"][r]
            if q[RW["done"]]:
                continue
            s1 = kh["hscale"] / (q[RW["Z"]] if form == "logRISE" else 1.0)
            assert abs(q[RW["s1"]] - s1) <= kh["nb"] * U52 * s1, (r, q[RW["s1"]], s1)
    assert 131072 in seen, seen
