"""Host model of learn()'s outer iterations on the FP64 path with Cholesky rows (the host logic of csrc/gml_solver.cpp: select's
bookkeeping, set_kh, the direction phase, the line search, finish), composed of the per-kernel models of tests/_solver_reference.py and a
plain pass over the pairwise statistics.  Numpy only; nothing of the code under test is imported.
tests/test_host_trajectory_reference.py holds it to the oracle's optimum; tests/test_gpu_solver_trajectory.py holds the device's recorded
iterations (csrc/gml_solver.h: TrajRecorder) to it.

The model runs a case twice: with the pass, the Hessian and the secant correction in np.longdouble, and with them in float64.  Every
decision the host logic takes is logged as a signed value whose sign is the outcome (`Dec`); the gap between the two runs' values of one
decision is the rounding that decision is exposed to, and a decision whose value is below FRAGILE times that gap is *fragile*: the
device, which rounds differently again, may take it the other way.  compare() leaves a fragile decision, and everything after it in
that row, out (a fragile `done` or `nreg`, which change what the other rows get -- the Hessian budget, the kind of pass -- from that
iteration on in every row)."""
import math

import numpy as np

import _solver_reference as M

LD = np.longdouble
FRAGILE = 100.0
MAX_ADD, CAP, VIOL_FRAC, FACE_SHARE = 64, 512, 0.5, 0.05
PREC = {"f64": 0, "i8x": 1, "i8w": 3}  # (include/gml.h: GML_PREC_*)


# ---- set_kh: the Hessian budget (include/gml.h: hess_samples) ---------------------------------------------------------
def kh_base(prec, R, Kp, knob0=0, hess_samples=0):
    """configurations per row and Newton Hessian before the adaptive factor: 32 768 on the FP64 path, clamp(2^23 / local rows, 32 768,
    131 072) on the int8 paths; knob 0 overrides that, hess_samples overrides both (< 0: every configuration)"""
    base = 32768
    if prec != "f64":
        base = min(131072, max(32768, (1 << 23) // max(R, 1)))
    if knob0 > 0:
        base = int(knob0)
    if hess_samples != 0:
        base = Kp if hess_samples < 0 else int(hess_samples)
    return base


def set_kh(K, Kp, R, nactive, base, hess_samples, wblk):
    """The sub-sample of one iteration: want = base x (R // nactive) configurations (adaptive: hess_samples == 0), in nb >= 2 blocks of
    512; once they cover K, every block; else every kstride-th block, kstride = blocks // nb, rescaled by the weight of those blocks; a
    sub-sample without weight falls back to every block.  Returns dict(nb, kstride, Kh, hscale, wsum, blocks)."""
    nblk = Kp // 512
    want = base
    if hess_samples == 0 and nactive > 0:
        want = base * max(1, R // nactive)
    nb = min(nblk, max(2, (want + 511) // 512))
    if nb * 512 >= K:
        nb = nblk
    kstride = nblk // nb
    wsum = 0.0
    for cb in range(nb):
        wsum += float(wblk[cb * kstride])
    if not wsum > 0:
        nb, kstride, wsum = nblk, 1, 1.0
    hscale = 1.0 if nb == nblk else 1.0 / wsum
    return dict(nb=nb, kstride=kstride, Kh=nb * 512, hscale=hscale, wsum=wsum, blocks=[cb * kstride for cb in range(nb)])


def face_rounds(K, Qp, knob1=0):
    """re-solves on the orthant faces inside the Cholesky solve: two where a backtracking pass costs more than a solve (K x columns >=
    2^28), else none; knob 1 = rounds + 1"""
    return int(knob1) - 1 if knob1 > 0 else (2 if K * Qp >= 268435456 else 0)


# ---- the problem ------------------------------------------------------------------------------------------------------------------
class Case:
    """A pairwise problem and the options of one learn(): spins [K][n] (+-1), counts [K], the node shard [node0, node1)."""

    def __init__(self, name, spins, counts, form, c, *, tol=1e-7, max_iter=100, hess_samples=0, knobs=None, nodes=None, prec="f64"):
        self.name, self.form, self.c, self.tol, self.max_iter, self.hess_samples, self.prec = name, form, c, tol, max_iter, hess_samples, prec
        self.knobs = dict(knobs or {})
        self.spins = np.ascontiguousarray(spins, dtype=np.int8)
        self.counts = np.asarray(counts, dtype=np.float64)
        self.K, self.n = self.spins.shape
        self.node0, self.node1 = nodes if nodes else (0, self.n)
        self.R = self.node1 - self.node0
        self.Kp = (self.K + 1023) // 1024 * 1024
        self.Qfp = (self.n + 63) // 64 * 64
        self.cconst, self.Qp = self.Qfp, self.Qfp + 64
        self.Msum = float(self.counts.sum())
        self.w = self.counts / self.Msum
        self.lam = c * math.sqrt(math.log(self.n * self.n / 0.05) / self.Msum)
        self.wblk = np.zeros(self.Kp // 512)
        for b in range(len(self.wblk)):  # (in the order of the library's sum: configuration by configuration)
            s = 0.0
            for v in self.w[512 * b:512 * b + 512]:
                s += float(v)
            self.wblk[b] = s
        self.base = kh_base(prec, self.R, self.Kp, self.knobs.get(0, 0), hess_samples)
        self.rounds = face_rounds(self.K, self.Qp, self.knobs.get(1, 0))

    def samples(self):
        """the histogram as the oracle takes it: [K][1 + n], the count first"""
        return np.concatenate([self.counts[:, None], self.spins.astype(np.float64)], axis=1)

    def kind(self, r):
        u = self.node0 + r
        k = np.zeros(self.Qp, dtype=np.uint8)
        k[:self.n] = 2
        k[u] = 0
        k[self.cconst] = 1
        return k

    def to_reference(self, r, x):
        """a row of the internal layout in the reference's: slot j = column j, the field in slot u"""
        u = self.node0 + r
        out = np.array(x[:self.n], dtype=np.float64)
        out[u] = x[self.cconst]
        return out


class Pass:
    """f, Z, the noise of f and the gradient of one row at x (internal layout), and the working-set Hessian over a list of blocks of
    512, in `dt`.  Y = s_u [x_c ..., 1]: E = Y theta."""

    def __init__(self, case, dt):
        self.c, self.dt = case, dt
        S = case.spins.astype(dt)
        self.Xe = np.concatenate([S, np.ones((case.K, 1), dtype=dt)], axis=1)  # [K][n + 1]: the spins, the constant column
        self.w = case.w.astype(dt)

    def cols(self, x):
        return np.concatenate([x[:self.c.n], x[self.c.cconst:self.c.cconst + 1]]).astype(self.dt)

    def weights(self, r, x):
        """E, e (the terms of f or Z) and v = -de/dE per configuration"""
        s = self.Xe[:, self.c.node0 + r]
        E = s * (self.Xe @ self.cols(x))
        if self.c.form == "RPLE":
            t = -2 * E
            l = np.log1p(np.exp(-np.abs(t)))
            e = self.w * np.where(t > 0, t + l, l)
            v = 2 * self.w / (1 + np.exp(2 * E))
        else:
            e = self.w * np.exp(-E)
            v = e
        return s, e, v

    def __call__(self, r, x, want_grad=True):
        c = self.c
        s, e, v = self.weights(r, x)
        fv = float(e.sum())
        noise = 1e-13 * max(1.0, abs(fv))
        g = None
        if want_grad:
            gc = -((v * s) @ self.Xe)
            if c.form == "logRISE":
                gc = gc / e.sum()
            g = np.zeros(c.Qp)
            g[:c.n] = gc[:c.n].astype(np.float64)
            g[c.cconst] = float(gc[c.n])  # (the node's own column is no parameter: its entry is never read)
        if c.form == "logRISE":
            return dict(f=math.log(fv), Z=fv, fn=noise / fv, g=g)
        return dict(f=fv, Z=1.0, fn=noise, g=g)

    def hessian(self, r, x, F, blocks):
        """sum over the configurations of the listed blocks of h_k x_kF x_kF^T (logRISE: of Z, not of log Z)"""
        c = self.c
        k = np.concatenate([np.arange(512 * b, min(512 * b + 512, c.K)) for b in blocks]).astype(np.int64)
        s, e, v = self.weights(r, x)
        if c.form == "RPLE":
            wk = self.w[k]
            pos = wk > 0
            h = np.where(pos, 2 * v[k] * (1 - v[k] / np.where(pos, 2 * wk, 1)), 0)
        else:
            h = v[k]
        ci = np.where(np.asarray(F) == c.cconst, c.n, F)
        XF = self.Xe[np.ix_(k, ci)]
        return (XF * h[:, None]).T @ XF


# ---- decisions --------------------------------------------------------------------------------------------------------------------
class Dec:
    """One logged decision of a (row, iteration): `name`, the values whose signs are the outcome, and whether it reaches every row."""
    GLOBAL = ("done", "stalled", "nreg")

    def __init__(self, name, values):
        self.name, self.v = name, np.atleast_1d(np.asarray(values, dtype=np.float64))


def _bool(log, name, value):
    """value >= 0 is the outcome; logged"""
    log.append(Dec(name, value))
    return bool(value >= 0)


# ---- one solve ---------------------------------------------------------------------------------------------------------------------
def solve(case, dt=LD):
    """The iterations of learn() on `case`.  Returns dict(iters: list of records, rows [R][n] (reference layout), kkt [R], from_best [R],
    not_converged, iterations).  A record: dict(it, nactive, Kh, kstride, hscale, secant, rounds, line_search, rows: list of per-row dicts,
    dec: per-row lists of Dec).  Per-row dict: done, atfloor, kkt, best, Fobj, stall, m, nsupp, nviol, F, Z, s1, ynoise, npairs, trials,
    alpha, nreg, full, accepted, gave_up, X (after the line search)."""
    c = case
    R, Qp, lam = c.R, c.Qp, c.lam
    ps = Pass(c, dt)
    kinds = [c.kind(r) for r in range(R)]
    x = np.zeros((R, Qp))
    xb = np.zeros((R, Qp))
    st = [ps(r, x[r]) for r in range(R)]  # f, Z, fn, g at the iterate
    best, Fbest, kkt = np.full(R, math.inf), np.full(R, math.inf), np.full(R, math.inf)
    Fobj = np.zeros(R)
    stall = np.zeros(R, dtype=int)
    done, atfloor = np.zeros(R, dtype=bool), np.zeros(R, dtype=bool)
    sec = [M.SecantState(CAP) for _ in range(R)]
    stall_cap = 10
    iters = []
    it = 0
    for it in range(c.max_iter):
        rec = dict(it=it, rows=[dict() for _ in range(R)], dec=[[] for _ in range(R)], line_search=False, secant=-1, rounds=-1, Kh=0, kstride=0,
                   hscale=0.0)
        sel = [None] * R
        nactive = 0
        for r in range(R):
            log = rec["dec"][r]
            if not done[r]:
                s = sel[r] = M.select_row(x[r], st[r]["g"], kinds[r], lam, MAX_ADD, CAP, CAP, VIOL_FRAC, best[r])
                # admission: which zero coordinates violate at all (|g| against lambda), and the cut among them where there is one
                z = (kinds[r] == 2) & (x[r] == 0)
                log.append(Dec("violator", np.abs(st[r]["g"][z]) - lam))
                if s["thr"]:
                    a = np.abs(s["pg"][z & (s["pg"] != 0)])
                    cut = np.sort(a)[::-1][s["max_add"] - 1:s["max_add"] + 1]
                    log.append(Dec("admission", cut[0] - cut[-1]))
                nz = (kinds[r] != 0) & (x[r] != 0)
                log.append(Dec("support sign", x[r][nz]))
                if s["nsupp"] > 1 and s["worstW"] > 0:
                    log.append(Dec("addv", s["worstW"] - s["worst"] * 0.999999))
                if s["better"]:
                    xb[r] = x[r]
                Fobj[r] = st[r]["f"] + s["l1"]
                kkt[r] = s["worst"] if math.isfinite(s["worst"]) and math.isfinite(st[r]["f"]) else math.inf
                fdown = not _bool(log, "fdown", Fobj[r] - (Fbest[r] - max(10.0 * st[r]["fn"], 1e-13 * abs(Fobj[r])))) if math.isfinite(Fbest[r]) else True
                if Fobj[r] < Fbest[r]:
                    Fbest[r] = Fobj[r]
                better = not _bool(log, "best", kkt[r] - best[r]) if math.isfinite(best[r]) else kkt[r] < best[r]
                if better:
                    best[r], stall[r] = kkt[r], 0
                elif fdown:
                    stall[r] = 0
                else:
                    stall[r] += 1
                if _bool(log, "done", c.tol - kkt[r]):
                    done[r] = True
                elif stall[r] >= stall_cap:
                    log.append(Dec("stalled", 1.0))
                    done[r] = atfloor[r] = True
                else:
                    nactive += 1
            q = rec["rows"][r]
            s = sel[r]
            q.update(done=bool(done[r]), atfloor=bool(atfloor[r]), kkt=kkt[r], best=best[r], Fobj=Fobj[r], stall=int(stall[r]), selected=s is not None,
                     Z=st[r]["Z"], f=st[r]["f"], fn=st[r]["fn"])
            if s is not None:
                q.update(m=s["m"], nsupp=s["nsupp"], nviol=s["nviol"], F=s["F"][:max(s["m"], 0)].copy())
        rec["nactive"] = nactive
        iters.append(rec)
        if nactive == 0:
            break
        kh = set_kh(c.K, c.Kp, R, nactive, c.base, c.hess_samples, c.wblk)
        secant = kh["Kh"] < c.Kp
        rec.update(Kh=kh["Kh"], kstride=kh["kstride"], hscale=kh["hscale"], secant=int(secant), rounds=c.rounds, line_search=True)
        s2 = 1.0 if c.form == "logRISE" else 0.0
        D = np.zeros((R, Qp))
        for r in np.flatnonzero(~done):
            s, q, log = sel[r], rec["rows"][r], rec["dec"][r]
            m = s["m"]
            assert 0 < m <= CAP, "the model covers Cholesky rows only"
            F, gF, pgF = s["F"][:m], s["gF"][:m], s["pgF"][:m]
            s1 = kh["hscale"] * (1.0 / st[r]["Z"] if c.form == "logRISE" else 1.0)
            yn = 100.0 * st[r]["fn"]
            H = ps.hessian(r, x[r], F, kh["blocks"])
            if secant:
                info = sec[r].step(F, x[r][F], gF, yn)
                if info is not None and info["ss"] > 0:
                    log.append(Dec("pair", [info["ys"] - 1e-4 * math.sqrt(info["ss"] * info["yy"]), info["ymax"] - yn]))
                _, B, _ = M.corrected_block(H, gF, s1, s2, sec[r].pairs(m), dtype=dt)
            else:
                B = s1 * H - s2 * np.outer(gF, gF).astype(dt)
            B = np.asarray(B, dtype=np.float64)
            d, flog = M.solve_faces(B, pgF, x[r][F], kinds[r][F], FACE_SHARE, c.rounds)
            for e in flog:  # the candidates' sign tests, and their share of the predicted decrease against FACE_SHARE
                log.append(Dec("face candidates", e["signs"]))
                log.append(Dec("face", [e["mass"] - FACE_SHARE * e["total"]] if e["n"] else [-1.0]))
            D[r, F] = d
            q.update(s1=s1, ynoise=yn, npairs=sec[r].npairs, nface=sum(e["again"] for e in flog), d=d.copy())
        # ---- the line search: every row that still needs a trial takes one per round; the round's pass is a full one on the first
        # round and whenever one of its rows is in the noise regime
        need = ~done
        alpha = np.ones(R)
        fwd = np.zeros(R, dtype=bool)
        for r in range(R):
            rec["rows"][r].update(trials=0, accepted=False, gave_up=False, full=False, alpha=1.0, nreg=False)
        for ls in range(30):
            rows = np.flatnonzero(need)
            if len(rows) == 0:
                break
            tr, nreg = {}, {}
            for r in rows:
                t = tr[r] = M.trial_row(x[r], D[r], sel[r]["pg"], kinds[r], lam, alpha[r])
                log = rec["dec"][r]
                mv = (kinds[r] == 2) & (D[r] != 0)
                log.append(Dec("clip", (x[r] + alpha[r] * D[r])[mv]))
                log.append(Dec("descent", -t["dd_first"]))
                nreg[r] = _bool(log, "nreg", 8.0 * st[r]["fn"] + 0.1 * t["dd"])
            full = ls == 0 or any(nreg.values())
            for r in rows:
                t, q, log = tr[r], rec["rows"][r], rec["dec"][r]
                pt = ps(r, t["xt"], want_grad=full)
                q.update(trials=q["trials"] + 1, alpha=float(alpha[r]), nreg=nreg[r])
                if nreg[r]:
                    bk = M.back_row(x[r], t["xt"], pt["g"], kinds[r], lam)[0]
                    ok = _bool(log, "accept", bk + 0.5 * abs(t["dd"]))
                else:
                    Fn = pt["f"] + t["l1t"]
                    ok = _bool(log, "accept", Fobj[r] + 1e-4 * t["dd"] + st[r]["fn"] + pt["fn"] - Fn)
                if ok:
                    x[r] = t["xt"]
                    if full:
                        st[r] = pt
                    else:
                        st[r] = dict(pt, g=st[r]["g"])
                        fwd[r] = True
                    need[r] = False
                    q.update(accepted=True, full=bool(full))
                else:
                    alpha[r] *= 0.5
                    if nreg[r] and alpha[r] < 1.0 / 64:
                        need[r] = False
                        stall[r] += 3
                        q["gave_up"] = True
        for r in np.flatnonzero(fwd):
            st[r] = ps(r, x[r])
        for r in range(R):
            rec["rows"][r]["X"] = x[r].copy()
        it += 1
    kk = np.minimum(best, kkt)
    from_best = best <= kkt
    rows = np.array([c.to_reference(r, xb[r] if from_best[r] else x[r]) for r in range(R)])
    return dict(iters=iters, rows=rows, kkt=kk, from_best=from_best, not_converged=int((~(kk <= c.tol)).sum()), iterations=it)


# ---- fragility ------------------------------------------------------------------------------------------------------------------------
def fragile_map(case, hi, lo):
    """first[r] = the first iteration from which row r is left out (len(iters) when never): the first decision of the long-double run
    `hi` whose value is below FRAGILE times its distance to the float64 run `lo`'s value (or which `lo` took differently, or did not
    take); a fragile decision that reaches every row (Dec.GLOBAL) ends them all after that iteration.  Returns (first [R], reasons)."""
    n = len(hi["iters"])
    first = np.full(case.R, n, dtype=int)
    why = {}
    for i, rec in enumerate(hi["iters"]):
        for r in range(case.R):
            if first[r] < i:
                continue
            other = lo["iters"][i]["dec"][r] if i < len(lo["iters"]) else None
            mine = rec["dec"][r]
            bad = None
            if other is None or [d.name for d in mine] != [d.name for d in other] or any(len(a.v) != len(b.v) for a, b in zip(mine, other)):
                bad = Dec("the float64 run took another path", 0.0)
            else:
                for a, b in zip(mine, other):
                    gap = np.abs(a.v - b.v)
                    if ((np.abs(a.v) < FRAGILE * gap) | ((a.v >= 0) != (b.v >= 0))).any():
                        bad = a
                        break
            if bad is not None:
                why[(r, i)] = bad.name
                if bad.name in Dec.GLOBAL or bad.name.startswith("the float64"):
                    first = np.minimum(first, i)
                else:
                    first[r] = min(first[r], i)
    return first, why


def check_cap(case, hi, first, branch_iters=()):
    """The cap on what may be left out: at most 10 % of the (row, iteration) records, none in iterations 0 to 3, none in the
    iterations `branch_iters` where the case's named branch first occurs.  Returns the share left out."""
    n = len(hi["iters"])
    total = n * case.R
    out = int((n - first).sum())
    assert out <= 0.1 * total, (case.name, out, total)
    assert (first > min(3, n - 1)).all(), (case.name, first)
    for i in branch_iters:
        assert (first > i).all(), (case.name, i, first)
    return out / total


# ---- the cases of tests/test_gpu_solver_trajectory.py ---------------------------------------------------------------------------
def histogram(n, K, seed, J=0.35, strong=None):
    """K random configurations with counts in {0 .. 3} that follow exp(sum J s_i s_{i+1} + ...) of a ring (zeros included: the weights
    of the blocks of 512 all differ); `strong` = (node, coupling): that node is tied to three others with this coupling"""
    rng = np.random.default_rng(seed)
    spins = np.where(rng.random((K, n)) < 0.5, 1, -1).astype(np.int8)
    S = spins.astype(np.float64)
    E = J * (S * np.roll(S, 1, axis=1)).sum(axis=1) + 0.2 * S[:, 0]
    if strong:
        u, Js = strong
        E = E + Js * S[:, u] * (S[:, (u + 2) % n] + S[:, (u + 5) % n] - S[:, (u + 7) % n])
    p = np.exp(E - E.max())
    counts = rng.binomial(3, np.clip(p / np.quantile(p, 0.9), 0.02, 1.0)).astype(np.float64)
    return spins, counts


def case(name):
    """the cases by name: '<what>-<formulation>'"""
    what, form = name.split("-")
    c = {"RISE": 0.4, "logRISE": 0.8, "RPLE": 0.2}[form]
    if what in ("strided", "every", "weightless", "faces", "cap", "shard"):
        spins, counts = histogram(24, 5000, 1)
        kw = dict(hess_samples=1024)
        if what == "every":
            kw = dict(hess_samples=-1)
        if what == "weightless":  # no count on exactly the sampled blocks 0 and 5
            counts[0:512] = 0
            counts[2560:3072] = 0
        if what == "faces":
            kw["knobs"] = {1: 3}
        if what == "cap":
            kw["max_iter"] = 3
        if what == "shard":
            kw["nodes"] = (5, 13)
        return Case(name, spins, counts, form, c, **kw)
    if what == "adaptive":  # one strongly coupled node among weak ones: the rows finish in different iterations
        spins, counts = histogram(16, 9000, 2, J=0.1, strong=(3, 0.6))
        return Case(name, spins, counts, form, c, hess_samples=0, knobs={0: 1024})
    if what == "scale":  # theta large enough that Z leaves 1 by tens of per cent
        spins, counts = histogram(24, 5000, 5, J=1.0, strong=(7, 1.2))
        return Case(name, spins, counts, form, 0.05, hess_samples=1024)
    if what == "backtrack":  # strong couplings, a weak penalty and a thin sub-sample: full steps overshoot
        spins, counts = histogram(24, 5000, 5, J=1.0, strong=(7, 1.2))
        return Case(name, spins, counts, form, 0.02, hess_samples=1024)
    raise KeyError(name)


F64_CASES = ["strided-RISE", "strided-logRISE", "strided-RPLE", "every-RISE", "adaptive-RISE", "weightless-RISE", "scale-logRISE", "backtrack-RISE",
             "faces-RISE", "cap-RISE", "shard-RISE"]
_cache = {}


def branch_iters(name, hi):
    """the iterations in which the branch a case is named for first occurs in the run `hi` (asserted to occur): none of their records
    may be left out of the comparison"""
    what, its = name.split("-")[0], hi["iters"]

    def first(pred, tag):
        for rec in its:
            if rec["line_search"] and any(pred(rec, q) for q in rec["rows"] if q.get("trials", 0) > 0):
                return rec["it"]
        raise AssertionError(f"{name}: the model never reaches '{tag}'")
    if what in ("strided", "shard"):
        assert its[0]["Kh"] == 1024 and its[0]["kstride"] == 5 and its[0]["secant"] == 1 and its[0]["hscale"] != 1.0
        return [0, first(lambda rec, q: q["npairs"] == 1, "one pair"), first(lambda rec, q: q["npairs"] == 2, "two pairs")]
    if what in ("every", "weightless"):
        assert all(rec["Kh"] == 5120 and rec["hscale"] == 1.0 and rec["secant"] == 0 and rec["kstride"] == 1 for rec in its if rec["line_search"])
        assert all(q["npairs"] == 0 for rec in its for q in rec["rows"] if q.get("trials", 0) > 0)
        return [0]
    if what == "adaptive":
        assert len({rec["nactive"] for rec in its}) >= 4  # the rows finish in different iterations
        return [0, first(lambda rec, q: 1024 < rec["Kh"] < 9216, "a larger budget"), first(lambda rec, q: rec["Kh"] == 9216 and rec["hscale"] == 1.0, "take it all")]
    if what == "scale":
        return [first(lambda rec, q: abs(q["Z"] - 1) > 0.1, "Z far from 1"), first(lambda rec, q: q["trials"] > 1 and abs(q["Z"] - 1) > 0.02, "a rejected trial")]
    if what == "backtrack":
        return [first(lambda rec, q: q["accepted"] and q["alpha"] < 1 and not q["full"], "a forward-only trial accepted below alpha = 1"),
                first(lambda rec, q: q["accepted"] and q["alpha"] < 1 and q["nreg"], "a noise-regime trial accepted below alpha = 1")]
    if what == "faces":
        assert its[0]["rounds"] == 2
        return [first(lambda rec, q: q["nface"] > 0, "a face re-solve")]
    if what == "cap":
        assert hi["iterations"] == 3 and hi["not_converged"] > 0
        return [0, 1, 2]
    raise KeyError(name)


def model(name):
    """(case, long-double run, float64 run, first iteration left out per row, reasons) of a case: computed once, shared, left unchanged"""
    if name not in _cache:
        cs = case(name)
        hi, lo = solve(cs, LD), solve(cs, np.float64)
        first, why = fragile_map(cs, hi, lo)
        _cache[name] = (cs, hi, lo, first, why)
    return _cache[name]
