"""Host model of the matrix-free direction phase of learn() (csrc/gml_newton_cg.cpp: the matrix-free half of direction_blocks, newton_cg,
newton_cg_group; its rules: csrc/gml_cg_rules.h), restated from the rules the solver documents, and the comparison of a recorded iteration (csrc/gml_solver.h: TRC_*)
with it.  Numpy only; nothing of the code under test is imported.

Three parts.
  * The rules: split_plan, plan_blocks / wsub, scales, ksub_rule, relax_schedule, is_coarse, eta_rule, stays_live, solves_again,
    route_is_sparse, tile_layout.
  * The pieces a record is cut at: reference_product (sum_k h_k (x_k . p) x_k over the participating configurations of a plan) and the
    replay of one row's PCG on the record's own inverted tiles and products (_solver_reference.Pcg with supplied products).
  * check_iteration: walks the events of one iteration in the order the rules prescribe.  Every decision is recomputed from the
    record's own numbers (CgState, kkt, nviol / nsupp, Z, FaceOut) and compared with ==; numbers are held by the tolerances the callers
    of this module document (tests/test_gpu_newton_cg_trajectory.py).  simulate() builds such a record from the model alone, for
    tests/test_host_newton_cg_reference.py and its mutations.

Slots.  The plane slot of a row is the slot book's business (csrc/gml_slots.h, tests/native/plane_slots.cpp); here the control blocks of
one iteration must agree with one another -- one slot per row, no slot twice -- and a slot that belongs to another row shows in the
products, which read that row's weights."""
import math

import numpy as np

import _solver_reference as M

LD = np.longdouble
U52, U53 = 2.0 ** -52, 2.0 ** -53
TAGS = ("blocks", "group", "plan", "step", "round_end", "faces", "resolve")
ETA_ADMIT, FACE_SHARE, FACE_ROUNDS, MAX_CG, CG_ETA, SPARSE_RATIO = 0.25, 0.05, 2, 16, 0.05, 0.3


# ---- the rules ----------------------------------------------------------------------------------------------------------------------
def split_plan(Kp, ngroups, Qfp, ksub):
    """Split-K plan of a product pass over `ngroups` node tiles of 32 rows: (kchunk, kpart, nsplit).  Chunks: a multiple of 8, as many
    as give each of 512 workgroup slots one workgroup over node tiles x column tiles of 256, at least 24, at most 256.  The chunk length
    is Kp over that count, rounded up to the granularity -- 512 ksub for a sub-sampled pass, else 256 -- and at least 2048 (rounded up
    likewise); histograms above 2^24 configurations keep chunks of at most 2^22.  The first kchunk / ksub of every chunk take part."""
    tiles = ngroups * -(-Qfp // 256)
    nsplit = -(-(-(-512 // tiles)) // 8) * 8
    nsplit = min(256, max(24, nsplit))
    ksub = max(1, ksub)
    gran = 512 * ksub if ksub > 1 else 256
    up = lambda v: -(-v // gran) * gran
    kchunk = up(-(-Kp // nsplit))
    if kchunk < 2048:
        kchunk = up(2048)
    if Kp > (1 << 24) and kchunk > (1 << 22):
        kchunk = (1 << 22) // gran * gran
    return kchunk, kchunk // ksub, -(-Kp // kchunk)


def plan_blocks(Kp, kchunk, kpart):
    """the blocks b of 512 configurations that take part: (512 b) mod kchunk < kpart, ascending"""
    return [b for b in range(Kp // 512) if (512 * b) % kchunk < kpart]


def wsub(wblk, Kp, kchunk, kpart):
    """weight of the participating blocks, summed in block order"""
    s = 0.0
    for b in plan_blocks(Kp, kchunk, kpart):
        s += float(wblk[b])
    return s


def scales(form, Z, Rp, kchunk, kpart, ws):
    """(kpart as the products get it, sc [Rp]): a sub-sample that shrinks and carries weight rescales by 1 / wsub, any other runs over
    whole chunks; logRISE divides by the row's Z (Hess log Z = Hess Z / Z - g g^T); Z [R], the padding rows have no Z"""
    zi = np.ones(Rp)
    if form == "logRISE":
        zi[:len(Z)] = 1.0 / np.asarray(Z, dtype=np.float64)
    if kpart < kchunk and ws > 0:
        return kpart, zi / ws
    return kchunk, zi


def ksub_rule(K, maxW, hv_subsample, coarse):
    """products of the coarse group run over ~1 / ksub of the configurations: as many as keep 32 per working-set entry, at most 8 --
    or what hv_subsample forces; the fine group takes them all"""
    if not coarse:
        return 1
    return hv_subsample if hv_subsample > 0 else min(8, max(1, K // (32 * maxW)))


def relax_schedule(K, maxW, hv_subsample, coarse):
    """[(step, ksub)] of round 0 of the fine group: over 1/2 from step 2, over 1/8 from step 4, each while 16 configurations per
    working-set entry remain; none when hv_subsample is set"""
    if coarse or hv_subsample != 0:
        return []
    out = []
    for step, f in ((2, 2), (4, 8)):
        ks = min(f, K // (16 * maxW))
        if ks > 1:
            out.append((step, ks))
    return out


def admitting(nviol, nsupp):
    return nviol * 16 > nsupp


def is_coarse(hv_subsample, nviol, nsupp, kkt, tol):
    return hv_subsample != 1 and admitting(nviol, nsupp) and kkt > max(1e3 * tol, 1e-5)


def eta_rule(nviol, nsupp, kkt, cg_eta=CG_ETA):
    return ETA_ADMIT if admitting(nviol, nsupp) else min(cg_eta, math.sqrt(max(kkt, 1e-300)))


def stays_live(cg, eta):
    """cg = (rs, rs0, pHp, rz) after the step"""
    return bool(cg[2] > 0 and cg[0] > eta * eta * cg[1])


def solves_again(nfixed, mass, total, share=FACE_SHARE):
    return bool(nfixed > 0 and mass > share * total)


def route_is_sparse(sparse_ok, sumW, ratio, Qfp, n):
    """entry by entry when the live rows' working sets sum to less than ratio x (statistics columns x node tiles of the GEMM pass)"""
    return bool(sparse_ok and float(sumW) < ratio * float(Qfp) * float(-(-n // 32)))


def sparse_allowed(form, order, has_i8=True, hv_lf=2, hv_lb=2, maxW=1):
    """the entry-by-entry form exists for the exp forms, two-limb products, statistics of at most two spins besides the node's own
    (interaction order <= 3) and working sets up to 65 536"""
    return bool(has_i8 and form != "RPLE" and hv_lf == 2 and hv_lb == 2 and order <= 3 and maxW <= 65536)


def tile_layout(nW, T):
    """(t0 per row, vm per tile, index of the row per tile) of the rows' tiles in list order"""
    t0, vm, own = [], [], []
    for i, m in enumerate(nW):
        t0.append(len(vm))
        for t in range(-(-m // T)):
            vm.append(min(T, m - t * T))
            own.append(i)
    return t0, vm, own


def working_set(x, pg, kind):
    return np.flatnonzero((kind != 0) & ((x != 0) | (pg != 0)))


# ---- the reference product ----------------------------------------------------------------------------------------------------------
def curvature_weights(form, w, E):
    """h_k of the formulation at the energies E: RISE / logRISE w e^-E (logRISE raw: of Z), RPLE 4 w sig (1 - sig), sig = 1 / (1 + e^2E)"""
    if form == "RPLE":
        sig = 1 / (1 + np.exp(2 * E))
        return 4 * w * sig * (1 - sig)
    return w * np.exp(-E)


def reference_product(Xs, h, vec, kchunk, kpart):
    """sum_k h_k (x_k . p) x_k over the configurations k mod kchunk < kpart (raw: no 1 / wsub, no 1 / Z).  Xs [K][P] float64 (+-1), h [K],
    vec [P].  Returns (product [P] float64, hsum of the participating h, the float64 rounding bound of this evaluation per entry:
    (K + 2 P + 8) 2^-53 sum_k h_k |p|_1 -- every term is at most h_k |p|_1)."""
    K, P = Xs.shape
    m = (np.arange(K) % kchunk) < kpart
    hm = np.where(m, np.asarray(h, dtype=np.float64), 0.0)
    t = Xs @ np.asarray(vec, dtype=np.float64)
    out = Xs.T @ (hm * t)
    hsum = float(hm.sum())
    return out, hsum, (K + 2 * P + 8) * U53 * hsum * float(np.abs(vec).sum())


# ---- parsing a recorded event (csrc/gml_solver.h: TRC_*) ---------------------------------------------------------------------------
def _ctl(iv, at, n, npad):
    c = np.asarray(iv[at:at + 3 * npad + npad // 32 + 4], dtype=np.int64)
    return dict(row=c[:npad], node=c[npad:2 * npad], slot=c[2 * npad:3 * npad], tile=c[3 * npad:3 * npad + npad // 32], tail=c[3 * npad + npad // 32:])


def parse_event(tag, iv, dv, Qp=None):
    """the dict of one event; Qp: the row length of the vectors (every event but `blocks`, which carries it)"""
    iv, dv = np.asarray(iv, dtype=np.int64), np.asarray(dv, dtype=np.float64)
    name = TAGS[tag]
    if name == "blocks":
        ncg, T, nt, Kh, kstride, Qp, prec, P = (int(v) for v in iv[:8])
        a = 8
        take = lambda k: iv[a:a + k]
        e = dict(tag=name, T=T, ntiles=nt, Kh=Kh, kstride=kstride, Qp=Qp, prec=prec, P=P)
        for key, k, shape in (("cg_rows", ncg, None), ("nW", ncg, None), ("t0", ncg, None), ("vm", nt, None), ("wrow", nt, None), ("FV", nt * T, (nt, T)),
                              ("kind", ncg * Qp, (ncg, Qp)), ("mmax", ncg, None), ("cols", ncg * P, (ncg, P))):
            v = take(k)
            e[key] = v.reshape(shape) if shape else v
            a += k
        assert a == len(iv)
        e["hscale"] = float(dv[0])
        b = 1
        for key, k, shape in (("s1", ncg, None), ("tau", ncg, None), ("X", ncg * Qp, (ncg, Qp)), ("PG", ncg * Qp, (ncg, Qp)), ("G", ncg * Qp, (ncg, Qp)),
                              ("Hpre", nt * T * T, (nt, T, T)), ("Hinv", nt * T * T, (nt, T, T))):
            v = dv[b:b + k]
            e[key] = v.reshape(shape) if shape else v
            b += k
        assert b == len(dv)
        return e
    if name == "group":
        n = int(iv[1])
        return dict(tag=name, coarse=int(iv[0]), maxW=int(iv[2]), rows=iv[3:3 + n], nviol=iv[3 + n:3 + 2 * n], nsupp=iv[3 + 2 * n:3 + 3 * n], kkt=dv[:n], Z=dv[n:2 * n])
    if name == "plan":
        return dict(tag=name, where=int(iv[0]), round=int(iv[1]), ci=int(iv[2]), ksub=int(iv[3]), kchunk=int(iv[4]), kpart=int(iv[5]), nsplit=int(iv[6]),
                    ngroups=int(iv[7]), Rp=int(iv[8]), wsub=float(dv[0]), sc=dv[1:])
    if name in ("step", "resolve"):
        h = 2 if name == "step" else 1
        sparse, n, npad = (int(v) for v in iv[h:h + 3])
        e = dict(tag=name, round=int(iv[0]), ci=int(iv[1]) if name == "step" else 0, sparse=sparse, rows=iv[h + 3:h + 3 + n], ctl=_ctl(iv, h + 3 + n, n, npad))
        nv = 3 if name == "step" else 2
        assert len(iv) == h + 3 + n + 3 * npad + npad // 32 + 4 and len(dv) == nv * n * Qp + 5 * n
        e.update(vec=dv[:n * Qp].reshape(n, Qp), tau=dv[n * Qp:n * Qp + n], Hp=dv[(nv - 1) * n * Qp + n:nv * n * Qp + n].reshape(n, Qp), cg=dv[nv * n * Qp + n:].reshape(n, 4))
        if name == "step":
            e["Rv"] = dv[n * Qp + n:2 * n * Qp + n].reshape(n, Qp)
        return e
    if name == "round_end":
        n = int(iv[1])
        return dict(tag=name, round=int(iv[0]), rows=iv[2:2 + n], D=dv.reshape(n, Qp))
    assert name == "faces"
    n, na = int(iv[1]), int(iv[2])
    return dict(tag=name, round=int(iv[0]), rows=iv[3:3 + n], nfixed=iv[3 + n:3 + 2 * n], again=iv[3 + 2 * n:3 + 2 * n + na], mass=dv[:n], total=dv[n:2 * n])


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
class Tally:
    """what a comparison measured: largest product error over its bound, largest PCG distance over delta_k, products checked / skipped,
    and which branches the records went through"""

    def __init__(self):
        self.product, self.pcg, self.pcg_allowed, self.checked, self.skipped = 0.0, 0.0, 0.0, 0, 0
        self.block, self.inverse, self.blocks_held, self.fallback_tiles = 0.0, 0.0, 0, 0
        self.seen = set()

    def note_pcg(self, dist, delta, allowed=None):
        """pcg: the largest distance in units of delta_k (where the two replays differ at all); pcg_allowed: in units of what the rule allows"""
        if delta > 0:
            self.pcg = max(self.pcg, dist / delta)
        if allowed is not None and dist > 0:
            self.pcg_allowed = max(self.pcg_allowed, dist / allowed if allowed > 0 else math.inf)


def _spread(got, m64, mld, nW, what, tally):
    """the rule of tests/test_gpu_solver_kernels.py: within 16 x |float64 model - longdouble model| + |W| 2^-53 scale"""
    ref = np.asarray(mld, dtype=np.float64)
    delta = float(np.abs(np.asarray(m64, dtype=np.float64) - ref).max())
    dist = float(np.abs(np.asarray(got) - ref).max())
    scale = float(np.abs(ref).max())
    tally.note_pcg(dist, delta, 16 * delta + nW * U53 * scale)
    assert dist <= 16 * delta + nW * U53 * scale, (what, dist, delta, scale)


def _scalars(got, c64, cld, nW, what, tally, names=("rs", "rs0", "pHp", "rz")):
    for k, name in enumerate(("rs", "rs0", "pHp", "rz")):
        if name not in names:
            continue
        a, b = float(getattr(c64, name)), float(getattr(cld, name))
        tally.note_pcg(abs(got[k] - b), abs(a - b), 16 * abs(a - b) + 4 * nW * U53 * abs(b))
        assert abs(got[k] - b) <= 16 * abs(a - b) + 4 * nW * U53 * abs(b), (what, name, got[k], b, a, "|W|", nW)


def check_blocks(b, par):
    """the tile bookkeeping of direction_blocks: W in column order with its padding, nW, t0, vm, wrow"""
    T, Qp = b["T"], b["Qp"]
    Ws = [working_set(b["X"][i], b["PG"][i], b["kind"][i]) for i in range(len(b["cg_rows"]))]
    assert list(b["nW"]) == [len(W) for W in Ws], ("nW", list(b["nW"]))
    t0, vm, own = tile_layout([len(W) for W in Ws], T)
    assert list(b["t0"]) == t0 and b["ntiles"] == len(vm), ("t0", list(b["t0"]), t0)
    assert list(b["vm"]) == vm, ("vm", list(b["vm"]), vm)
    assert list(b["wrow"]) == [int(b["cg_rows"][i]) for i in own], ("wrow", list(b["wrow"]))
    for i, W in enumerate(Ws):
        nt = -(-len(W) // T)
        fv = b["FV"][t0[i]:t0[i] + nt].reshape(-1)
        assert (fv[:len(W)] == W).all() and (fv[len(W):] == Qp - 1).all(), ("FV of row", int(b["cg_rows"][i]))
    return Ws


def check_iteration(events, par, wblk, tally, product=None, replay=True, product_filter=None):
    """One iteration's events against the rules.  par: K, Kp, Qfp, R, Rp, node0, form, order, tol, hv_subsample, max_cg, cg_eta, face_rounds,
    ratio.  product(i, row, items) -> one (reference [Qp], bound [Qp] or scalar) per item, the products of one row gathered over the
    iteration: items = [(event, k, kchunk, kpart)], the k-th row of a step / resolve event under that plan; i = the row's index among the
    matrix-free rows.  product_filter(ev, first_of_plan) says which products are required."""
    form, K, Kp, Qfp, R, Rp = par["form"], par["K"], par["Kp"], par["Qfp"], par["R"], par["Rp"]
    s2 = 1.0 if form == "logRISE" else 0.0
    maxcg, rounds_cap = par.get("max_cg") or MAX_CG, par.get("face_rounds", FACE_ROUNDS)
    cg_eta = par.get("cg_eta") or CG_ETA
    b = events[0]
    assert b["tag"] == "blocks"
    Ws = check_blocks(b, par)
    T, Qp = b["T"], b["Qp"]
    index = {int(r): i for i, r in enumerate(b["cg_rows"])}
    nW = {int(r): len(Ws[index[int(r)]]) for r in b["cg_rows"]}
    assert list(b["cg_rows"]) == sorted(index), "matrix-free rows in row order"
    pos = [1]
    pending = {}

    def nxt(tag):
        assert pos[0] < len(events), ("the record ends where the rules expect", tag)
        e = events[pos[0]]
        pos[0] += 1
        assert e["tag"] == tag, ("event", pos[0] - 1, e["tag"], "expected", tag)
        return e

    # the groups: by the inputs recorded with them (nviol, nsupp, kkt are per row: gather them from whichever group has the row)
    info = {}
    for e in events:
        if e["tag"] == "group":
            for k, r in enumerate(e["rows"]):
                info[int(r)] = (int(e["nviol"][k]), int(e["nsupp"][k]), float(e["kkt"][k]), float(e["Z"][k]))
    assert sorted(info) == sorted(index), "every matrix-free row is in exactly one group"
    coarse = [r for r in sorted(index) if is_coarse(par["hv_subsample"], info[r][0], info[r][1], info[r][2], par["tol"])]
    fine = [r for r in sorted(index) if r not in coarse]
    Zall = np.ones(R)
    for r, v in info.items():
        Zall[r] = v[3]
    slot_of = {}

    def check_plan(e, where, rnd, ci, ksub, nrows):
        assert (e["where"], e["round"], e["ci"], e["ksub"]) == (where, rnd, ci, ksub), ("plan", e["where"], e["round"], e["ci"], e["ksub"], "expected", where, rnd, ci, ksub)
        kchunk, kpart, nsplit = split_plan(Kp, -(-nrows // 32), Qfp, ksub)
        assert (e["kchunk"], e["nsplit"], e["ngroups"]) == (kchunk, nsplit, -(-nrows // 32)), ("plan", e, kchunk, nsplit)
        blocks = plan_blocks(Kp, kchunk, kpart)
        ws = wsub(wblk, Kp, kchunk, kpart)
        nb = max(1, len(blocks))
        if ksub > 1:
            assert abs(e["wsub"] - ws) <= nb * U52 * ws, ("wsub", e["wsub"], ws)
        kp2, sc = scales(form, [Zall[r] if r in info else 1.0 for r in range(R)], Rp, kchunk, kpart, ws)
        # (rows outside the group: the solver writes 1 / Z of every local row, whatever it last held)
        assert e["kpart"] == kp2, ("kpart", e["kpart"], kp2)
        for r in info:
            assert abs(e["sc"][r] - sc[r]) <= nb * U52 * sc[r], ("sc of row", r, e["sc"][r], sc[r])
        assert (np.abs(e["sc"][R:] - sc[R:]) <= nb * U52 * sc[R:]).all(), "sc of the padding rows"
        if kp2 == kchunk and ksub > 1:
            tally.seen.add("weightless")
        if where == 1:
            tally.seen.add(f"relax{ci}")
        return dict(kchunk=kchunk, kpart=kp2, ksub=ksub, fresh=True, sc=e["sc"])

    def check_ctl(e, rows, sparse_ok):
        n = len(rows)
        npad = -(-n // 32) * 32
        c = e["ctl"]
        assert list(e["rows"]) == rows, (e["tag"], e["round"], e["ci"], "rows", list(e["rows"]), rows)
        assert list(c["row"]) == rows + [0] * (npad - n) and list(c["node"]) == [par["node0"] + r for r in rows] + [-1] * (npad - n)
        assert list(c["tile"]) == list(range(npad // 32)) and (c["tail"] == -1).all() and (c["slot"][n:] == 0).all()
        for k, r in enumerate(rows):
            s = int(c["slot"][k])
            assert s >= 0 and slot_of.setdefault(r, s) == s, ("slot of row", r, s, slot_of[r])
        assert len(set(slot_of.values())) == len(slot_of), "two rows in one slot"
        want = route_is_sparse(sparse_ok, sum(nW[r] for r in rows), par["ratio"], Qfp, n)
        assert bool(e["sparse"]) == want, (e["tag"], e["round"], e["ci"], "route", e["sparse"], want)
        tally.seen.add("entries" if want else "gemm")

    def check_products(e, plan):
        first = plan["fresh"]
        plan["fresh"] = False
        if product is None:
            return
        if product_filter is not None and not product_filter(e, first):
            tally.skipped += len(e["rows"])
            return
        for k, r in enumerate(e["rows"]):
            pending.setdefault(int(r), []).append((e, k, plan["kchunk"], plan["kpart"]))

    for is_c, rows in ((1, coarse), (0, fine)):
        if not rows:
            continue
        g = nxt("group")
        assert (g["coarse"], list(g["rows"])) == (is_c, rows), ("group", g["coarse"], list(g["rows"]), "expected", is_c, rows)
        tally.seen.add("coarse" if is_c else "fine")
        maxW = max(1, max(nW[r] for r in rows))
        assert g["maxW"] == maxW
        # s1 of the tiles: hscale / Z (held to nb 2^-52 like the Cholesky rows')
        nbh = b["Kh"] // 512
        for r in rows:
            s1 = b["hscale"] / (info[r][3] if form == "logRISE" else 1.0)
            assert abs(b["s1"][index[r]] - s1) <= nbh * U52 * s1, ("s1 of row", r)
        sparse_ok = sparse_allowed(form, par["order"], maxW=maxW)
        plan = check_plan(nxt("plan"), 0, 0, 0, ksub_rule(K, maxW, par["hv_subsample"], is_c), len(rows))
        relax = relax_schedule(K, maxW, par["hv_subsample"], is_c)
        cgs = {}
        if replay:
            for r in rows:
                i = index[r]
                t0 = int(b["t0"][i])
                Mi = [b["Hinv"][t0 + t] for t in range(-(-nW[r] // T))]
                cgs[r] = [M.Pcg(None, plan["sc"][r], s2, b["X"][i], b["PG"][i], b["G"][i], b["kind"][i], T, dt, Minv=Mi) for dt in (np.float64, LD)]
        cur, rnd = list(rows), 0
        while True:
            live = list(cur)
            for ci in range(maxcg):
                if not live:
                    break
                if rnd == 0:
                    for step, ks in relax:
                        if ci == step:
                            plan = check_plan(nxt("plan"), 1, rnd, ci, ks, len(live))
                e = nxt("step")
                assert (e["round"], e["ci"]) == (rnd, ci), ("step", e["round"], e["ci"], "expected", rnd, ci)
                check_ctl(e, live, sparse_ok)
                check_products(e, plan)
                keep = []
                for k, r in enumerate(live):
                    nv, ns, kkt, _ = info[r]
                    if stays_live(e["cg"][k], eta_rule(nv, ns, kkt, cg_eta)):
                        keep.append(r)
                    if replay:
                        c64, cld = cgs[r]
                        what = ("row", r, "round", rnd, "step", ci)
                        # what the previous kernels left, against the replays' (which went on from the device's state before them) ...
                        _spread(e["vec"][k], c64.p, cld.p, nW[r], what + ("Pv",), tally)
                        _spread(e["Rv"][k], c64.r, cld.r, nW[r], what + ("Rv",), tally)
                        _scalars(e["cg"][k], c64, cld, nW[r], what, tally, ("rz",))
                        # ... and this step from the device's own state
                        for c in (c64, cld):
                            c.s1 = c.dt(plan["sc"][r])
                            c.p, c.r, c.rz = e["vec"][k].astype(c.dt), e["Rv"][k].astype(c.dt), c.dt(e["cg"][k][3])
                            c.update(e["Hp"][k], pHp=e["cg"][k][2])
                        a, bb = float(c64.pHp_own), float(cld.pHp_own)  # (the step length then comes from the device's pHp: see the caller's notes)
                        tally.note_pcg(abs(e["cg"][k][2] - bb), abs(a - bb), 16 * abs(a - bb) + 4 * nW[r] * U53 * abs(bb))
                        assert abs(e["cg"][k][2] - bb) <= 16 * abs(a - bb) + 4 * nW[r] * U53 * abs(bb), (what, "pHp", e["cg"][k][2], bb, a)
                        _scalars(e["cg"][k], c64, cld, nW[r], what, tally, ("rs", "rs0"))
                        if r in keep and ci + 1 < maxcg:
                            c64.advance()
                            cld.advance()
                if len(keep) < len(live) and keep and (len(live) - 1) // 32 == (len(keep) - 1) // 32:
                    tally.seen.add("shrank")
                live = keep
                if live and ci + 1 == maxcg:
                    tally.seen.add("cap")
                if not live or ci + 1 == maxcg:
                    break
            e = nxt("round_end")
            assert (e["round"], list(e["rows"])) == (rnd, cur), ("round end", e["round"], list(e["rows"]), cur)
            if replay:
                for k, r in enumerate(cur):
                    _spread(e["D"][k], cgs[r][0].d, cgs[r][1].d, nW[r], ("row", r, "round", rnd, "D"), tally)
            Dend = e["D"]
            if rnd >= rounds_cap:
                break
            f = nxt("faces")
            assert (f["round"], list(f["rows"])) == (rnd, cur)
            again = [r for k, r in enumerate(cur) if solves_again(int(f["nfixed"][k]), float(f["mass"][k]), float(f["total"][k]))]
            assert list(f["again"]) == again, ("again", list(f["again"]), again)
            if replay:  # FaceOut from the device's own D
                for k, r in enumerate(cur):
                    c64 = cgs[r][0]
                    i = index[r]
                    cand, fixed, mass, total, margin = M.face_candidates(b["X"][i], Dend[k], b["PG"][i], b["kind"][i], c64.Wm.copy())
                    assert int(f["nfixed"][k]) == int(cand.sum()), ("nfixed of row", r, int(f["nfixed"][k]), int(cand.sum()))
                    assert abs(f["mass"][k] - mass) <= nW[r] * U53 * mass and abs(f["total"][k] - total) <= nW[r] * U53 * total, ("FaceOut of row", r)
            if not again:
                break
            tally.seen.add("resolve")
            sub = {r: k for k, r in enumerate(cur)}
            cur = again
            if relax:
                plan = check_plan(nxt("plan"), 2, rnd + 1, 0, 1, len(cur))
            e = nxt("resolve")
            assert e["round"] == rnd + 1
            check_ctl(e, cur, sparse_ok)
            check_products(e, plan)
            if replay:
                for k, r in enumerate(cur):
                    c64, cld = cgs[r]

                    def hd(d, k=k, r=r):
                        assert np.array_equal(np.asarray(d, dtype=np.float64), e["vec"][k]), ("the re-solve's vector of row", r)
                        return e["Hp"][k]
                    for c in (c64, cld):
                        c.s1 = c.dt(plan["sc"][r])
                        c.d = np.asarray(Dend[sub[r]], dtype=c.dt).copy()  # (both replays go on from the device's step)
                        c.faces(hd)
                    got = e["cg"][k]
                    assert got[2] == 0, ("pHp after the residual, row", r)
                    for kk, name in ((0, "rs"), (1, "rs0"), (3, "rz")):
                        a, bb = float(getattr(c64, name)), float(getattr(cld, name))
                        tally.note_pcg(abs(got[kk] - bb), abs(a - bb), 16 * abs(a - bb) + 4 * nW[r] * U53 * abs(bb))
                        assert abs(got[kk] - bb) <= 16 * abs(a - bb) + 4 * nW[r] * U53 * abs(bb), ("row", r, "re-solve", name, got[kk], bb, a)
            rnd += 1
    assert pos[0] == len(events), ("events beyond what the rules prescribe", len(events) - pos[0])
    for r in sorted(pending):
        i = index[r]
        W = Ws[i]
        for (e, k, _, _), (ref, bound) in zip(pending[r], product(i, r, pending[r])):
            err = np.abs(e["Hp"][k][W] - ref[W])
            bd = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)[W]
            ratio = float((err / bd).max())
            tally.product = max(tally.product, ratio)
            tally.checked += 1
            assert ratio <= 1.0, ("product of row", r, e["tag"], e["round"], e["ci"], "measured / bound", ratio)


# ---- a record from the model alone --------------------------------------------------------------------------------------------------
class Synthetic:
    """A small problem in a layout of its own: Qp = n + 1 columns (n statistics and the unpenalised column n), R rows, K configurations of
    random +-1 statistics with weights, RISE or logRISE.  Rows sit at given iterates; every row is matrix-free."""

    def __init__(self, form="RISE", seed=0, R=3, n=11, K=6000, T=4, zero_blocks=()):
        rng = np.random.default_rng(seed)
        self.form, self.R, self.n, self.K, self.T = form, R, n, K, T
        self.Kp, self.Qp, self.Qfp = -(-K // 1024) * 1024, n + 1, 64
        lat = rng.normal(size=(K, 3)) @ rng.normal(size=(3, n)) + 1.5 * rng.normal(size=(K, n))  # (correlated: CG takes its steps)
        self.Xs = np.concatenate([np.where(lat > 0, 1.0, -1.0), rng.choice([-1.0, 1.0], size=(K, 1))], axis=1)  # (the last: the node's own spin)
        c = rng.integers(0, 4, size=K).astype(np.float64)
        for blk in zero_blocks:
            c[512 * blk:512 * blk + 512] = 0
        self.w = c / c.sum()
        self.wblk = np.zeros(self.Kp // 512)
        for blk in range(len(self.wblk)):
            s = 0.0
            for v in self.w[512 * blk:512 * blk + 512]:
                s += float(v)
            self.wblk[blk] = s
        self.x = rng.normal(scale=0.2, size=(R, self.Qp)) * (rng.random((R, self.Qp)) < 0.6)
        self.x[:, 1::3] *= 0.02  # (small entries: the Newton step takes some of them through zero)
        self.kind = np.full((R, self.Qp), 2, dtype=np.int64)
        self.kind[:, n] = 1
        self.lam = 0.1
        self.h, self.G, self.PG, self.Z = [], np.zeros((R, self.Qp)), np.zeros((R, self.Qp)), np.ones(R)
        for r in range(R):
            E = self.Xs @ self.x[r]
            h = curvature_weights(form, self.w, E)
            g = -(self.Xs.T @ h)
            if form == "logRISE":
                self.Z[r] = h.sum()
                g = g / self.Z[r]
            self.h.append(h)
            self.G[r] = g
            self.PG[r] = M.pseudo_grad(self.x[r], g, np.where(self.kind[r] == 2, self.lam, 0.0))
        self.par = dict(K=K, Kp=self.Kp, Qfp=self.Qfp, R=R, Rp=32, node0=0, form=form, order=2, tol=1e-7, hv_subsample=0, max_cg=0, cg_eta=0.0,
                        face_rounds=FACE_ROUNDS, ratio=SPARSE_RATIO)

    def dense(self, r, kchunk, kpart):
        m = (np.arange(self.K) % kchunk) < kpart
        return (self.Xs * np.where(m, self.h[r], 0.0)[:, None]).T @ self.Xs

    def product(self, i, r, items):
        out = []
        for ev, k, kchunk, kpart in items:
            ref, hsum, bound = reference_product(self.Xs, self.h[r], ev["vec"][k], kchunk, kpart)
            out.append((ref, 4 * bound + 1e-300))  # (two float64 evaluations of the same sum, each within the bound, and their orders)
        return out


def simulate(S, nviol, nsupp, kkt, mut=None):
    """The events of one iteration of the problem S, by the rules above; every row matrix-free.  mut: the name of one deliberate
    mistake (tests/test_host_newton_cg_reference.py)."""
    par, form, R, Qp, T = S.par, S.form, S.R, S.Qp, S.T
    s2 = 1.0 if form == "logRISE" else 0.0
    rows = list(range(R))
    Ws = [working_set(S.x[r], S.PG[r], S.kind[r]) for r in rows]
    nW = [len(W) for W in Ws]
    t0, vm, own = tile_layout(nW, T)
    FV = np.full((len(vm), T), Qp - 1, dtype=np.int64)
    for r in rows:
        FV.reshape(-1)[t0[r] * T:t0[r] * T + nW[r]] = Ws[r]
    wrow = list(own)
    if mut == "wrow":
        wrow[-1] -= 1
    zi = 1.0 / S.Z if form == "logRISE" else np.ones(R)
    Hpre, Hinv = np.zeros((len(vm), T, T)), np.zeros((len(vm), T, T))
    for t, r in enumerate(own):
        cols = FV[t, :vm[t]]
        A = S.dense(r, S.Kp, S.Kp)[np.ix_(cols, cols)]
        Hpre[t, :vm[t], :vm[t]] = A
        Hinv[t, :vm[t], :vm[t]] = np.linalg.inv(zi[r] * A - s2 * np.outer(S.G[r][cols], S.G[r][cols]))
    ev = [dict(tag="blocks", T=T, ntiles=len(vm), Kh=S.Kp, kstride=1, Qp=Qp, prec=1, P=Qp - 1, cg_rows=np.array(rows), nW=np.array(nW), t0=np.array(t0),
               vm=np.array(vm), wrow=np.array(wrow), FV=FV, kind=S.kind, mmax=np.zeros(R, dtype=np.int64), cols=None, hscale=1.0, s1=zi.copy(), tau=np.zeros(R),
               X=S.x, PG=S.PG, G=S.G, Hpre=Hpre, Hinv=Hinv)]
    maxcg = par.get("max_cg") or MAX_CG
    coarse = [r for r in rows if is_coarse(par["hv_subsample"], nviol[r], nsupp[r], kkt[r], par["tol"])]
    fine = [r for r in rows if r not in coarse]
    state = {}

    def plan_event(where, rnd, ci, ksub, nrows):
        kchunk, kpart, nsplit = split_plan(S.Kp, -(-nrows // 32), S.Qfp, ksub)
        ws = wsub(S.wblk, S.Kp, kchunk, kpart)
        if mut == "wsub_head":  # over the first kpart samples only
            ws = sum(float(S.wblk[blk]) for blk in range(kpart // 512))
        kp2, sc = scales(form, S.Z, par["Rp"], kchunk, kpart, ws)
        if mut == "no_wsub" and kp2 < kchunk:
            sc = sc * ws
        if mut == "no_z":
            sc = sc * np.concatenate([S.Z, np.ones(par["Rp"] - R)])
        ev.append(dict(tag="plan", where=where, round=rnd, ci=ci, ksub=ksub, kchunk=kchunk, kpart=kp2, nsplit=nsplit, ngroups=-(-nrows // 32), Rp=par["Rp"],
                       wsub=ws, sc=sc))
        state.update(kchunk=kchunk, kpart=kp2, sc=sc)

    def ctl_of(live):
        n, npad = len(live), -(-len(live) // 32) * 32
        return dict(row=np.array(live + [0] * (npad - n)), node=np.array(live + [-1] * (npad - n)), slot=np.array([r + 32 for r in live] + [0] * (npad - n)),
                    tile=np.arange(npad // 32), tail=np.full(4, -1))

    def products(live, vecs):
        out = np.zeros((len(live), Qp))
        for k, r in enumerate(live):
            src = (r + 1) % R if mut == "neighbour" else r
            out[k] = S.dense(src, state["kchunk"], state["kpart"]) @ vecs[k]
        return out

    for is_c, grp in ((1, coarse), (0, fine)):
        if not grp:
            continue
        maxW = max(1, max(nW[r] for r in grp))
        ev.append(dict(tag="group", coarse=is_c, maxW=maxW, rows=np.array(grp), nviol=np.array([nviol[r] for r in grp]), nsupp=np.array([nsupp[r] for r in grp]),
                       kkt=np.array([kkt[r] for r in grp]), Z=np.array([S.Z[r] for r in grp])))
        plan_event(0, 0, 0, ksub_rule(S.K, maxW, par["hv_subsample"], is_c), len(grp))
        relax = relax_schedule(S.K, maxW, par["hv_subsample"], is_c)
        if mut == "relax_early":
            relax = [(s - 1, k) for s, k in relax]
        sparse_ok = sparse_allowed(form, 2, maxW=maxW)
        cg = {r: M.Pcg(None, state["sc"][r], s2, S.x[r], S.PG[r], S.G[r], S.kind[r], T, np.float64, Minv=[Hinv[t0[r] + t] for t in range(-(-nW[r] // T))])
              for r in grp}
        cur, rnd = list(grp), 0
        while True:
            live = list(cur)
            for ci in range(maxcg):
                if not live:
                    break
                if rnd == 0:
                    for step, ks in relax:
                        if ci == step:
                            plan_event(1, rnd, ci, ks, len(live))
                vecs = np.stack([cg[r].p.copy() for r in live])
                Rvs = np.stack([cg[r].r.copy() for r in live])
                Hp = products(live, vecs)
                cgv = np.zeros((len(live), 4))
                keep = []
                for k, r in enumerate(live):
                    c = cg[r]
                    c.s1 = np.float64(state["sc"][r])
                    c.update(Hp[k])
                    if mut == "negative_php" and rnd == 0 and ci == 1 and k == 0:
                        c.pHp = -abs(c.pHp)
                    cgv[k] = (c.rs, c.rs0, c.pHp, c.rz)
                    src = grp[(grp.index(r) + 1) % len(grp)] if mut == "eta_row" else r
                    stay = stays_live(cgv[k], eta_rule(nviol[src], nsupp[src], kkt[src], par.get("cg_eta") or CG_ETA))
                    if mut == "negative_php" and cgv[k][2] <= 0:
                        stay = True
                    if stay:
                        keep.append(r)
                        if ci + 1 < maxcg:
                            c.advance()
                ev.append(dict(tag="step", round=rnd, ci=ci, sparse=int(route_is_sparse(sparse_ok, sum(nW[r] for r in live), par["ratio"], S.Qfp, len(live))),
                               rows=np.array(live), ctl=ctl_of(live), vec=vecs, tau=np.zeros(len(live)), Rv=Rvs, Hp=Hp, cg=cgv))
                live = keep
                if not live or ci + 1 == maxcg:
                    break
            D = np.stack([cg[r].d.copy() for r in cur])
            ev.append(dict(tag="round_end", round=rnd, rows=np.array(cur), D=D))
            if rnd >= par.get("face_rounds", FACE_ROUNDS):
                break
            fo = [M.face_candidates(S.x[r], cg[r].d, S.PG[r], S.kind[r], cg[r].Wm.copy()) for r in cur]
            again = [r for r, f in zip(cur, fo) if solves_again(int(f[0].sum()), f[2], f[3])]
            ev.append(dict(tag="faces", round=rnd, rows=np.array(cur), nfixed=np.array([int(f[0].sum()) for f in fo]), again=np.array(again, dtype=np.int64),
                           mass=np.array([f[2] for f in fo]), total=np.array([f[3] for f in fo])))
            if not again:
                break
            cur = again
            if relax:
                plan_event(2, rnd + 1, 0, 1, len(cur))
            vecs, Hp, cgv = np.zeros((len(cur), Qp)), np.zeros((len(cur), Qp)), np.zeros((len(cur), 4))
            for k, r in enumerate(cur):
                c = cg[r]
                c.s1 = np.float64(state["sc"][r])

                def hd(d, k=k, r=r):
                    vecs[k] = d
                    Hp[k] = products([r], d[None, :])[0]
                    return Hp[k]
                c.faces(hd)
                cgv[k] = (c.rs, c.rs0, c.pHp, c.rz)
                cgv[k][2] = 0.0
            ev.append(dict(tag="resolve", round=rnd + 1, ci=0, sparse=int(route_is_sparse(sparse_ok, sum(nW[r] for r in cur), par["ratio"], S.Qfp, len(cur))),
                           rows=np.array(cur), ctl=ctl_of(cur), vec=vecs, tau=np.zeros(len(cur)), Hp=Hp, cg=cgv))
            rnd += 1
    return ev
