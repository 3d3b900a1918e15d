"""The host rules of the matrix-free direction phase (csrc/gml_cg_rules.h: groups, ksub, the relaxed schedule, eta, stays_live, the face
rule, the route of a product, the tile layout, a plan's weight and scales, the control block of a product) are plain C++ functions:
tests/native/cg_rules.cpp evaluates them on the host and this module compares every result with == to the model the GPU tests use
(tests/_newton_cg_reference.py), on cases that sit on the rules' edges.  No GPU, no library.

What == means for the doubles.  eta is one sqrt and one min, correctly rounded on both sides.  sc is 1 / Z / wsub, two correctly rounded
divisions in the same order.  wsub is a sum of the same doubles in the same (ascending block) order -- for ksub > 1, where every chunk
is a multiple of 512; for ksub = 1 the products run over every configuration, wsub is never used, and the C++ sum over chunks whose
length is no multiple of 512 need not be the model's: there only kpart and sc are compared, as the issue of this test states."""
import math
import os
import subprocess

import numpy as np
import pytest

import _newton_cg_reference as N
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "cg_rules.cpp")
CSRC = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "csrc")


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cg_rules") / "cg_rules")
    # a host compiler and the one header: it must not need a device header to compile
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", out])

    def ask(lines):
        """one answer (a list of tokens) per command"""
        r = subprocess.run([out], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        ans = r.stdout.splitlines()
        assert len(ans) == len(lines), (len(ans), len(lines))
        return [a.split() for a in ans]
    return ask


def hx(v):
    return float(v).hex()


def up(v):
    return math.nextafter(v, math.inf)


def down(v):
    return math.nextafter(v, -math.inf)


def test_constants(rules):
    a = rules(["constants"])[0]
    assert (float.fromhex(a[0]), float.fromhex(a[1]), int(a[2])) == (N.ETA_ADMIT, N.FACE_SHARE, N.FACE_ROUNDS)
    assert [int(v) for v in a[3:]] == [32, 16, 2, 2, 4, 8]


def test_groups(rules):
    """nviol * 16 against nsupp on both sides of equality; kkt at max(1e3 tol, 1e-5) exactly and one ulp to either side"""
    cases = [(nviol, nsupp) for nsupp in (0, 16, 32, 47, 48, 49) for nviol in (0, 1, 2, 3, 4)] + [(3, 16 * 3 + d) for d in (-1, 0, 1)]
    got = rules([f"admitting {a} {b}" for a, b in cases])
    assert [int(g[0]) for g in got] == [int(N.admitting(a, b)) for a, b in cases]
    assert {N.admitting(a, b) for a, b in cases} == {True, False}
    cases = []
    for tol in (1e-7, 1e-9):
        thr = max(1e3 * tol, 1e-5)
        for kkt in (down(thr), thr, up(thr), 0.0, 1.0):
            for hv in (0, 1, 3):
                for nviol, nsupp in ((2, 31), (2, 32), (2, 33), (0, 0)):
                    cases.append((hv, nviol, nsupp, kkt, tol))
    got = rules([f"is_coarse {hv} {a} {b} {hx(k)} {hx(t)}" for hv, a, b, k, t in cases])
    want = [int(N.is_coarse(*c)) for c in cases]
    assert [int(g[0]) for g in got] == want and 0 < sum(want) < len(want)
    assert N.is_coarse(0, 2, 31, up(1e-5), 1e-9) and not N.is_coarse(0, 2, 31, 1e-5, 1e-9)  # (the edge is among the cases)


def test_ksub_and_relaxed_schedule(rules):
    """K / (32 maxW) in {0, 1, 7, 8, 9} and K / (16 maxW) in {1, 2, 7, 8}, on both ends of each quotient's range of K"""
    cases = []
    for maxW in (1, 47, 400):
        for q in (0, 1, 7, 8, 9):
            for K in {max(q * 32 * maxW, 1), (q + 1) * 32 * maxW - 1}:
                assert K // (32 * maxW) == q
                for hv in (0, 1, 3):
                    for coarse in (0, 1):
                        cases.append((K, maxW, hv, coarse))
    got = rules([f"ksub_rule {K} {w} {hv} {c}" for K, w, hv, c in cases])
    assert [int(g[0]) for g in got] == [N.ksub_rule(K, w, hv, bool(c)) for K, w, hv, c in cases]
    cases = []
    for maxW in (1, 47, 400):
        for q in (0, 1, 2, 7, 8):
            for K in {max(q * 16 * maxW, 1), (q + 1) * 16 * maxW - 1}:
                for hv in (0, 1, 3):
                    for coarse in (0, 1):
                        cases.append((K, maxW, hv, coarse))
    got = rules([f"relax_schedule {K} {w} {hv} {c}" for K, w, hv, c in cases])
    want = [N.relax_schedule(K, w, hv, bool(c)) for K, w, hv, c in cases]
    assert [[(int(g[i]), int(g[i + 1])) for i in range(1, len(g), 2)] for g in got] == want
    assert {tuple(w) for w in want} >= {(), ((2, 2), (4, 2)), ((2, 2), (4, 7)), ((2, 2), (4, 8))}


def test_eta_and_stays_live(rules):
    cases = [(nviol, nsupp, kkt, cg_eta) for nviol, nsupp in ((2, 31), (2, 32), (0, 5)) for kkt in (0.0, 1e-310, 1e-12, 0.0025, down(0.0025), up(0.0025), 1.0)
             for cg_eta in (0.05, 0.0005)]
    got = rules([f"eta_rule {a} {b} {hx(k)} {hx(e)}" for a, b, k, e in cases])
    assert [float.fromhex(g[0]) for g in got] == [N.eta_rule(*c) for c in cases]
    assert len({N.eta_rule(*c) for c in cases}) >= 6  # (the admitting constant, both caps, and the square roots)
    cases = []
    for eta, rs0 in ((0.25, 16.0), (0.05, 3.0), (1e-150, 1.0)):
        edge = eta * eta * rs0
        for rs in (down(edge), edge, up(edge)):
            for pHp in (0.0, -1e-300, 1e-300, 1.0):
                cases.append((rs, rs0, pHp, eta))
    got = rules([f"stays_live {hx(rs)} {hx(rs0)} {hx(q)} {hx(e)}" for rs, rs0, q, e in cases])
    want = [int(N.stays_live((rs, rs0, q, 0.0), e)) for rs, rs0, q, e in cases]
    assert [int(g[0]) for g in got] == want and 0 < sum(want) < len(want)
    assert not N.stays_live((1.0, 16.0, 1.0, 0.0), 0.25) and N.stays_live((up(1.0), 16.0, 1e-300, 0.0), 0.25)


def test_faces_and_route(rules):
    cases = []
    for total in (1.0, 3.0, 1e-300):
        edge = N.FACE_SHARE * total
        for mass in (down(edge), edge, up(edge)):
            for nfixed in (0, 1, 7):
                cases.append((nfixed, mass, total))
    got = rules([f"solves_again {n} {hx(m)} {hx(t)}" for n, m, t in cases])
    want = [int(N.solves_again(*c)) for c in cases]
    assert [int(g[0]) for g in got] == want and 0 < sum(want) < len(want)
    cases = []
    for n in (1, 32, 33):
        tiles = -(-n // 32)
        for ratio, Qfp, thr in ((0.25, 64, 16 * tiles), (0.3, 64, 20 * tiles - (tiles - 1)), (-1.0, 64, 0), (1e30, 64, 10 ** 9)):
            for sumW in (thr - 1, thr, thr + 1):
                for ok in (0, 1):
                    cases.append((ok, sumW, ratio, Qfp, n))
    got = rules([f"route_is_sparse {ok} {s} {hx(r)} {q} {n}" for ok, s, r, q, n in cases])
    want = [int(N.route_is_sparse(bool(ok), s, r, q, n)) for ok, s, r, q, n in cases]
    assert [int(g[0]) for g in got] == want and 0 < sum(want) < len(want)
    assert N.route_is_sparse(True, 15, 0.25, 64, 32) and not N.route_is_sparse(True, 16, 0.25, 64, 32) and N.route_is_sparse(True, 31, 0.25, 64, 33)
    cases = [(has, form, lf, lb, order, maxW) for has in (0, 1) for form in ("RISE", "logRISE", "RPLE") for lf, lb in ((2, 2), (3, 2), (2, 4))
             for order in (2, 3, 4) for maxW in (1, 65536, 65537)]
    got = rules([f"sparse_allowed {has} {int(form == 'RPLE')} {lf} {lb} {order - 1} {w}" for has, form, lf, lb, order, w in cases])  # ko = order - 1
    assert [int(g[0]) for g in got] == [int(N.sparse_allowed(form, order, bool(has), lf, lb, w)) for has, form, lf, lb, order, w in cases]


def test_tile_layout(rules):
    """rows in list order; the model numbers rows by their place in the list, the header by local row"""
    cases = [(128, 1, [0], [1]), (128, 1, [0], [128]), (128, 1, [0], [129]), (128, 3, [0, 1, 2], [148, 5, 256]), (4, 4, [0, 1, 2, 3], [5, 0, 8, 9]),
             (128, 6, [4, 1, 3], [7, 300, 7, 128, 1, 7]), (128, 3, [], [1, 2, 3])]
    got = rules([f"tile_layout {T} {R} {len(rows)} " + " ".join(str(v) for v in rows + nW) for T, R, rows, nW in cases])
    for (T, R, rows, nW), g in zip(cases, got):
        parts = " ".join(g).split("|")
        ntiles, t0, vm, wrow = int(parts[0]), [int(v) for v in parts[1].split()], [int(v) for v in parts[2].split()], [int(v) for v in parts[3].split()]
        mt0, mvm, own = N.tile_layout([nW[r] for r in rows], T)
        assert ntiles == len(mvm) and vm == mvm and wrow == [rows[i] for i in own], (T, rows, nW)
        assert len(t0) == R and [t0[r] for r in rows] == mt0 and all(t0[r] == 0 for r in range(R) if r not in rows)
    assert N.tile_layout([148, 5, 256], 128) == ([0, 2, 3], [128, 20, 5, 128, 128], [0, 0, 1, 2, 2])


def _plan_cases():
    """the grid tests/test_host_newton_cg_reference.py holds split_plan on (the large histograms thinned as there), and the GPU
    case `weightless`: Kp = 14 336, one node tile, 64 columns, ksub = 8 with no weight on the sampled blocks 0, 8, 16, 24"""
    for Kp in (2048, 5120, 14336, 26624, 140288, 1 << 20, (1 << 24) + 1024, (1 << 25) + 4096):
        wblk = np.random.default_rng(Kp % 9973).random(Kp // 512)
        grid = [(g, q, k) for g in (1, 2, 3, 16, 40) for q in (64, 192, 256, 320, 1024) for k in (1, 2, 3, 5, 8)]
        if Kp > 1 << 22:
            grid = [(g, q, k) for g, q, k in grid if g <= 2 and k not in (3, 5) and q in (64, 320, 1024)]
        yield Kp, wblk, grid
    wblk = np.random.default_rng(14336).random(28)
    wblk[[0, 8, 16, 24]] = 0.0
    yield 14336, wblk, [(1, 64, 8), (1, 64, 2), (1, 64, 1), (2, 64, 8)]


def test_plan_weight_and_scales(rules):
    R, Rp = 5, 32
    Z = np.random.default_rng(7).uniform(0.5, 2.0, size=R)
    lines, want = [f"Z {R} " + " ".join(hx(v) for v in Z)], [None]
    weightless = 0
    for Kp, wblk, grid in _plan_cases():
        lines.append(f"wblk {len(wblk)} " + " ".join(hx(v) for v in wblk))
        want.append(None)
        for ngroups, Qfp, ksub in grid:
            kchunk, kpart, nsplit = N.split_plan(Kp, ngroups, Qfp, ksub)
            ws = N.wsub(wblk, Kp, kchunk, kpart)
            weightless += ksub > 1 and ws == 0
            for form in ("RISE", "logRISE"):
                lines.append(f"plan_scales {kchunk} {kpart} {nsplit} {Kp} {int(form == 'logRISE')} {Rp}")
                want.append((ksub, ws) + N.scales(form, Z, Rp, kchunk, kpart, ws))
    got = rules(lines)
    assert weightless >= 1
    for line, g, w in zip(lines, got, want):
        if w is None:
            assert g == ["ok"], line
            continue
        ksub, ws, kp, sc = w
        assert int(g[1]) == kp and [float.fromhex(v) for v in g[2:]] == list(sc), line
        if ksub > 1:
            assert float.fromhex(g[0]) == ws, line


def test_product_control_block(rules):
    """row [np] | node [np] | slot [np] | node tile [np / 32] | 4 unused, the padding 0, -1, 0, then -1: what check_iteration's check_ctl
    holds of a recorded block"""
    cases = []
    for n in (1, 31, 32, 40):
        rng = np.random.default_rng(n)
        rows = sorted(rng.choice(64, size=n, replace=False).tolist())
        cases.append((n, 100, rows, rng.permutation(96)[:n].tolist()))
    got = rules([f"hv_ctl {n} {node0} " + " ".join(str(v) for v in rows + slots) for n, node0, rows, slots in cases])
    for (n, node0, rows, slots), g in zip(cases, got):
        npad = -(-n // 32) * 32
        assert (int(g[0]), int(g[1]), g[2]) == (npad, 3 * npad + npad // 32 + 4, "|")
        iv = [int(v) for v in g[3:]]
        assert len(iv) == int(g[1])
        c = N._ctl(iv, 0, n, npad)
        assert list(c["row"]) == rows + [0] * (npad - n) and list(c["node"]) == [node0 + r for r in rows] + [-1] * (npad - n)
        assert list(c["slot"]) == slots + [0] * (npad - n)
        assert list(c["tile"]) == list(range(npad // 32)) and list(c["tail"]) == [-1] * 4
