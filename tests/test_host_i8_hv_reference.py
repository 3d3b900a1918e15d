"""tests/_i8_hv_reference.py, the host model tests/test_gpu_i8_hv_exact.py holds the product pass of the int8-limb GEMM kernels to,
against brute force on tiny cases -- element by element, with code that shares nothing with the model's own:
  * a triple loop at n = 5, K = 70 (Kp = 128), pairwise and order 3, that reads the weights byte by byte out of a V image through the
    offset table tests/native/i8_pass_tables.cpp prints from csrc/gml_bits.h, quantises the direction with Python's round() on
    rationals, forms x_k . p in Python integers and y = hh fl(x_k . p invtau) + d in rational arithmetic with the two roundings applied
    by hand, and sums csum, Gacc and G entry by entry -- four- and six-plane source images, RISE and RPLE, hv = 1 and 2, a slot map
    that is no identity, a part of the samples with stale bytes outside it;
  * the HV branch's digit trick (v ^ 0x80808080) - 0x80808080 over its range, the two-limb recombination acc0 + (acc1 << 8) and the
    two-digit range of the products at the edges +-32639 and +-32640;
  * the remap of the compact sample tiles of a sub-sampled pass against an enumeration of the samples, for the plans of the device
    tests on Kp = 9216 and 3072, a last chunk shorter than kpart included;
  * the integer ranges behind the model's exactness claims on every shape the device tests use, in Python integers;
  * the share of the elements float64 arithmetic alone decides (the others are evaluated in rational arithmetic): >= 0.999.
Then the same comparison with a perturbed model -- the dither one sample off, pn without the factor 1.01, vpl0 = 1 on a six-plane
image, the part taken as the first kpart samples only, csum over all samples, the planes (1, 2) for hv = 2: each must be noticed.
No GPU, no library."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _i8_hv_reference as H
import _i8_pack_reference as R
import _i8_pass_reference as M
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "i8_pass_tables.cpp")
CSRC = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "csrc")
SLOTS, KP, K, N, QFP = 32, 128, 70, 5, 64
CCONST, QP = QFP, QFP + 64
NODES = [0, 4, 2, 2, 1, 3]
VMAP = [1, 0, 2, 2, 5, 3]
PLAN = (64, 32)  # (the model takes any chunking; the device's are multiples of 256)


@pytest.fixture(scope="module")
def offsets(tmp_path_factory):
    """{lbt: int array [slots][lbt][Kp] of byte offsets}, from the header the kernels compile"""
    exe = str(tmp_path_factory.mktemp("i8_hv_tables") / "i8_pass_tables")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], input=f"{SLOTS} {KP}", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {4: np.full((SLOTS, 4, KP), -1), 6: np.full((SLOTS, 6, KP), -1)}
    for line in r.stdout.splitlines():
        name, *rest = line.split()
        if name == "off":
            lbt, row, l, k, off = (int(x) for x in rest)
            out[lbt][row, l, k] = off
    assert all((o >= 0).all() for o in out.values())
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the tiny case
# ---------------------------------------------------------------------------------------------------------------------------
def tiny(order, lbt, seed, form="RISE"):
    rng = np.random.default_rng(seed)
    spins = np.where(rng.random((K, N)) < 0.5, 1, -1).astype(np.int8)
    keys = R.stat_keys(N, order)
    Qf = len(keys)
    counts = np.floor(10 ** rng.uniform(0, 2, size=K))
    counts[[3, 40]] = 0.0
    w = np.zeros(KP)
    w[:K] = counts / counts.sum()
    bits = R.stat_bits(spins, keys, QFP, KP)
    # V planes as an objective pass leaves them: zero on padding and on samples of count zero
    rple = form == "RPLE"
    top = M.VMAX[lbt] // (8 if rple else 1)
    val = rng.integers(-top, top + 1, size=(SLOTS, KP))
    if not rple:
        val[0, 7], val[1, 9] = M.VMAX[lbt], -M.VMAX[lbt]  # (the top four planes at their largest)
    val[:, w == 0] = 0
    vplanes = np.ascontiguousarray(M.digits_of(val, lbt).transpose(1, 0, 2))
    tau_v = 10.0 ** rng.uniform(-12, -9, size=SLOTS)
    if rple:  # an RPLE pass keeps |V| <= 2 w: a tvh / (2 w) in [0, 1], so that 2 a (1 - a tvh / (2 w)) stays inside 31 bits
        tau_v = rng.uniform(0.5, 1.0, size=SLOTS) * 2.0 * w[w > 0].min() / 2.0 ** 31 / (65536.0 if lbt == 6 else 1.0)
    rows = np.zeros((len(NODES), QP))
    rows[:, :Qf] = rng.normal(size=(len(NODES), Qf))
    rows[:, CCONST] = rng.normal(size=len(NODES))
    rows[1] = 0.0
    rows[1, CCONST] = 0.37  # the node's field alone: |x . p| = emax on every sample
    rows[3] = 0.0           # all zeros: pn = 1
    rows[4] = np.clip(0.2 * rows[4], -0.49, 0.49)
    rows[4, Qf - 1] = -0.5  # the largest entry a power of two
    prev = rng.integers(-128, 128, size=(SLOTS, 4, KP)).astype(np.int8)  # what an earlier product left in Uq
    return dict(order=order, lbt=lbt, spins=spins, keys=keys, Qf=Qf, w=w, bits=bits, vplanes=vplanes, tau_v=tau_v, rows=rows, prev=prev)


# ---------------------------------------------------------------------------------------------------------------------------
# brute force: loops, Python integers, rationals
# ---------------------------------------------------------------------------------------------------------------------------
def _fl(x):
    """a rational to the nearest double, ties to even"""
    return float(Fraction(x))


def _dither32(u, k):
    h = (u * 0x85EBCA6B + k * 0x9E3779B9) % (1 << 32)
    return h - (1 << 32) if h >= 1 << 31 else h


def brute(c, form, hv, lf, plan, off):
    lbt, Qf, bits = c["lbt"], c["Qf"], c["bits"]
    vimg = M.pack_vq(c["vplanes"])
    vpl0, vscale = lbt - 4, (65536.0 if lbt == 6 else 1.0)
    uq = c["prev"].copy()
    out = dict(sigma=[], tau=[], invtau=[], qconst=[], csum=[], u=[])
    inpart = [k for k in range(KP) if k % plan[0] < plan[1]]
    for r, (node, vs) in enumerate(zip(NODES, VMAP)):
        p = c["rows"][r]
        mx = max([abs(float(v)) for v in p[:QFP]] + [abs(float(p[CCONST]))])
        ex = 0
        while mx > 0 and 2.0 ** ex <= mx:
            ex += 1
        while mx > 0 and 2.0 ** (ex - 1) > mx:
            ex -= 1
        sx = ex - (8 * lf - 2)
        sg = Fraction(2) ** sx
        q = [round(Fraction(float(v)) / sg) for v in p[:QFP]]
        q0 = round(Fraction(float(p[CCONST])) / sg)
        sabs = abs(q0) + sum(abs(v) for v in q)
        emax = _fl(Fraction(sabs) * sg)
        pn = (emax if emax > 0 else 1.0) * ((65536.0 * 1.01) if hv == 2 else 1.0)
        tvh = c["tau_v"][vs] * vscale
        tau = tvh * pn
        it = 1.0 / pn
        us = []
        for k in range(KP):
            if k not in inpart:
                us.append(None)
                continue
            v = sum(int(vimg[off[lbt][vs, l, k]]) * 256 ** (l - vpl0) for l in range(vpl0, vpl0 + 4))
            a = abs(v)
            if form == "RPLE":
                wk = float(c["w"][k])
                if wk > 0:
                    t1 = _fl(Fraction(a) * Fraction(tvh))
                    t2 = _fl(Fraction(t1) / Fraction(2 * wk))
                    t3 = _fl(1 - Fraction(t2))
                    hh = _fl(Fraction(2 * a) * Fraction(t3))
                else:
                    hh = 0.0
            else:
                hh = float(a)
            eint = q0 + sum(qc * (1 - 2 * int(bits[col, k])) for col, qc in enumerate(q))
            assert abs(eint) < 2 ** 53
            Ea = float(eint) * float(sg)
            e = _fl(Fraction(Ea) * Fraction(it))
            y = Fraction(hh) * Fraction(e) + Fraction(_dither32(node, k), 1 << 32)
            u = round(Fraction(_fl(y)))  # the fma's rounding, then to an integer, ties to even
            us.append(u)
            word = u & 0xFFFFFFFF
            dj = ((word + 0x80808080) & 0xFFFFFFFF) ^ 0x80808080  # the kernel's digit split
            for l in range(4):
                b = (dj >> (8 * l)) & 0xFF
                uq[r, l, k] = b - 256 if b >= 128 else b
        out["u"].append(us)
        out["sigma"].append(float(sg))
        out["tau"].append(tau)
        out["invtau"].append(it)
        out["qconst"].append(q0 + sum(q))
        out["csum"].append(sum(u for u in us if u is not None))
    nl = 2 if hv == 2 else 4
    gacc = np.zeros((len(NODES), 4, QFP), dtype=np.int64)
    G = np.zeros((len(NODES), QP))
    for r in range(len(NODES)):
        for col in range(Qf + 2):
            for l in range(nl):
                gacc[r, l, col] = sum(int(uq[r, l, k]) * int(bits[col, k]) for k in inpart)
        for col in range(Qf):
            s = sum(256 ** l * int(gacc[r, l, col]) for l in range(4))
            G[r, col] = out["tau"][r] * _fl(out["csum"][r] - 2 * s)
        G[r, CCONST] = out["tau"][r] * _fl(out["csum"][r])
    out.update(uq=uq, gacc=gacc, G=G)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the model on the same case, with the perturbations of the tests below
# ---------------------------------------------------------------------------------------------------------------------------
def model(c, form, hv, lf, plan, dither_shift=0, pn_factor=H.PN2, vpl0=None, part=None, csum_all=False, planes=None):
    lbt, Qf, bits = c["lbt"], c["Qf"], c["bits"]
    vpl0 = lbt - 4 if vpl0 is None else vpl0
    vscale = 65536.0 if lbt == 6 else 1.0
    part = H.participating(KP, *plan) if part is None else part
    uq = c["prev"].copy()
    out = dict(sigma=[], tau=[], invtau=[], qconst=[], u=[])
    for r, (node, vs) in enumerate(zip(NODES, VMAP)):
        d = H.direction(c["rows"][r], QFP, CCONST, lf, hv, c["tau_v"][vs], vscale, pn_factor)
        hh = H.hh_planes(c["vplanes"][vs], vpl0)
        Ea, _, _ = H.xdotp(c["rows"][r], QFP, CCONST, lf, bits)
        u, _ = H.product_row(form, hh, c["tau_v"][vs] * vscale, c["w"], Ea, d["invtau"], node, dither_shift)
        uq[r][:, part] = M.digits_of(u, 4)[:, part]
        out["u"].append([int(v) if part[k] else None for k, v in enumerate(u)])
        for key in ("sigma", "tau", "invtau", "qconst"):
            out[key].append(d[key])
    csum, g = H.behind_uq(uq, np.ones(KP, dtype=bool) if csum_all else part, bits, hv, planes)
    if csum_all:
        g = H.behind_uq(uq, part, bits, hv, planes)[1]
    G = H.finalize(out["tau"] + [0.0] * (SLOTS - len(NODES)), csum, g, np.arange(SLOTS) < len(NODES), Qf, QP, CCONST)
    out.update(uq=uq, csum=[int(v) for v in csum[:len(NODES)]], gacc=g[:len(NODES)], G=G[:len(NODES)])
    return out


def mismatches(a, b):
    bad = 0
    for key in ("sigma", "tau", "invtau"):
        bad += int((np.array(a[key]).view(np.int64) != np.array(b[key]).view(np.int64)).sum())
    bad += sum(x != y for x, y in zip(a["qconst"], b["qconst"])) + sum(x != y for x, y in zip(a["csum"], b["csum"]))
    bad += sum(x != y for ra, rb in zip(a["u"], b["u"]) for x, y in zip(ra, rb))
    bad += int((a["uq"] != b["uq"]).sum()) + int((a["gacc"] != b["gacc"]).sum())
    bad += int((a["G"].view(np.int64) != b["G"].view(np.int64)).sum())
    return bad


CASES = [(2, 4, "RISE", 1, 5), (2, 4, "RPLE", 2, 2), (2, 6, "RISE", 2, 2), (2, 6, "RPLE", 1, 3), (3, 4, "RISE", 2, 5), (3, 6, "RPLE", 1, 4),
         (3, 4, "RISE", 1, 2)]


@pytest.mark.parametrize("order,lbt,form,hv,lf", CASES)
def test_model_against_brute_force(offsets, order, lbt, form, hv, lf):
    c = tiny(order, lbt, 100 * order + 10 * lbt + lf, form)
    for plan in ((KP, KP), PLAN):
        b = brute(c, form, hv, lf, plan, offsets)
        assert mismatches(model(c, form, hv, lf, plan), b) == 0
        # not vacuous: products on most samples, stale bytes outside the part, and -- hv = 2 -- inside two digits
        us = [u for row in b["u"] for u in row if u is not None]
        assert sum(u != 0 for u in us) > len(us) // 4 and all(u == 0 for u in b["u"][3] if u is not None)
        if hv == 2:
            assert max(abs(u) for u in us) <= H.U2MAX and not b["gacc"][:, 2:].any()
        if plan != (KP, KP):
            out = ~H.participating(KP, *plan)
            assert np.array_equal(b["uq"][:, :, out], c["prev"][:, :, out]) and c["prev"][:6, :, out].any()


# ---------------------------------------------------------------------------------------------------------------------------
# a perturbed model is noticed
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_dither_one_sample_off_is_noticed(offsets):
    c = tiny(2, 4, 1)
    b = brute(c, "RISE", 1, 5, (KP, KP), offsets)
    assert mismatches(model(c, "RISE", 1, 5, (KP, KP)), b) == 0
    assert mismatches(model(c, "RISE", 1, 5, (KP, KP), dither_shift=1), b) > 0


def test_pn_without_the_factor_is_noticed_and_leaves_two_digits(offsets):
    """row 1 is the node's field alone (|x . p| = emax on every sample) and reads slot 0, whose sample 7 holds the largest number four
    planes spell: with pn = 65536 emax the product there is 32639.498 + d, which rounds to 32640 -- outside two balanced digits --
    whenever d > 0.002; the factor 1.01 keeps it at 32316"""
    c = tiny(2, 4, 2)
    b = brute(c, "RISE", 2, 2, (KP, KP), offsets)
    good, bad = model(c, "RISE", 2, 2, (KP, KP)), model(c, "RISE", 2, 2, (KP, KP), pn_factor=65536.0)
    assert mismatches(good, b) == 0 and mismatches(bad, b) > 0
    assert abs(good["u"][1][7]) in (32316, 32317)
    # the dither of (node 4, sample 7) decides whether the unscaled product leaves the range; some sample of the slot does
    hh = float(M.VMAX[4])
    over = [k for k in range(K) if round(Fraction(hh) / 65536 + Fraction(_dither32(4, k), 1 << 32)) > H.U2MAX]
    assert len(over) > K // 3


def test_vpl0_off_by_one_on_a_six_plane_image_is_noticed(offsets):
    c = tiny(2, 6, 3)
    b = brute(c, "RISE", 1, 5, (KP, KP), offsets)
    assert mismatches(model(c, "RISE", 1, 5, (KP, KP)), b) == 0
    assert mismatches(model(c, "RISE", 1, 5, (KP, KP), vpl0=1), b) > 0


def test_a_part_of_the_first_chunk_only_is_noticed(offsets):
    c = tiny(2, 4, 4)
    b = brute(c, "RISE", 1, 5, PLAN, offsets)
    assert mismatches(model(c, "RISE", 1, 5, PLAN), b) == 0
    assert mismatches(model(c, "RISE", 1, 5, PLAN, part=np.arange(KP) < PLAN[1]), b) > 0


def test_csum_over_all_samples_is_noticed(offsets):
    c = tiny(2, 4, 5)
    b = brute(c, "RISE", 1, 5, PLAN, offsets)
    m = model(c, "RISE", 1, 5, PLAN, csum_all=True)
    assert mismatches(m, b) > 0 and np.array_equal(m["gacc"], b["gacc"]) and m["csum"] != b["csum"]


def test_the_planes_1_and_2_for_two_limbs_are_noticed(offsets):
    c = tiny(2, 4, 6)
    b = brute(c, "RISE", 2, 2, (KP, KP), offsets)
    assert mismatches(model(c, "RISE", 2, 2, (KP, KP)), b) == 0
    assert mismatches(model(c, "RISE", 2, 2, (KP, KP), planes=(1, 2)), b) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# digits, recombination, remap, ranges
# ---------------------------------------------------------------------------------------------------------------------------
def test_digit_trick_of_the_hv_branch_over_its_range():
    """(v ^ 0x80808080) - 0x80808080 on the word of four digit bytes is the signed number the digits spell, over the int32 values an
    objective pass writes (four balanced digits reach down to -0x80808080, below int32: the forward kernels split an int)"""
    rng = np.random.default_rng(7)
    lo = -(1 << 31)
    vals = np.concatenate([rng.integers(lo, M.VMAX[4] + 1, size=200000), [lo, lo + 1, M.VMAX[4], 0, -1, 1, 127, 128, -128, -129, 32639, 32640,
                                                                                   -32896, -32897, 0x7F7F7F, 0x7F7F80]])
    d = M.digits_of(vals, 4).astype(np.int64)
    word = sum((d[l] & 0xFF) << (8 * l) for l in range(4))
    got = ((word ^ 0x80808080) - 0x80808080 + (1 << 31)) % (1 << 32) - (1 << 31)  # (int) of the unsigned difference
    assert np.array_equal(got, vals)


def test_two_limb_recombination_and_range_at_the_edges():
    # the digits of a two-limb direction: acc0 + (acc1 << 8) in int32 is sum_c q_c b_c
    rng = np.random.default_rng(8)
    q = np.concatenate([rng.integers(-(1 << 14), (1 << 14) + 1, size=250), [32639, -32639, -32640, 1 << 14, -(1 << 14), 0]])
    d, rest = R.digits_np(q, 2)
    assert not rest.any()
    b = rng.integers(0, 2, size=(1000, len(q)))
    acc = (b @ d.astype(np.int64).T).astype(np.int32)
    assert np.array_equal((acc[:, 0] + (acc[:, 1] << 8)).astype(np.int64), b @ q)
    # two balanced digits spell -32896 .. 32639: 32640 needs a third one, -32640 does not
    for v, fits in ((32639, True), (32640, False), (-32639, True), (-32640, True), (-32896, True), (-32897, False)):
        assert (R.balanced_digits(v, 2)[1] == 0) == fits, v
        assert (not M.digits_of(np.array([v]), 4)[2:].any()) == fits, v
    assert H.U2MAX == 127 * 256 + 127


PLANS = [(2048, 1024), (2048, 256), (4096, 512), (4096, 2048)]


@pytest.mark.parametrize("Kp", [9216, 3072])
@pytest.mark.parametrize("plan", PLANS)
def test_remap_of_compact_tiles_against_an_enumeration(Kp, plan):
    kchunk, kpart = plan
    want = sorted({k // 256 for k in range(Kp) if k % kchunk < kpart})
    got = H.remap_tiles(Kp, kchunk, kpart)
    assert got == want and len(set(got)) == len(got)
    assert H.participating(Kp, kchunk, kpart).sum() == 256 * len(want)
    nsplit, pt = -(-Kp // kchunk), kpart // 256
    early = nsplit * pt - len(got)  # compact tiles that return early: the last chunk is shorter than kpart
    assert early == max(0, (nsplit - 1) * kchunk + kpart - Kp) // 256
    if (Kp, plan) == (9216, (4096, 2048)):
        assert early == 4  # the third chunk [8192, 9216) is shorter than kpart
    assert H.remap_tiles(Kp, 2048, 2048) == list(range(Kp // 256))


# (name, Kp, Qfp) of the device tests
SHAPES = [("splitk", 3072, 64), ("narrow", 9216, 128), ("order3", 5120, 256)]


def test_integer_ranges_of_every_device_shape():
    for name, Kp, Qfp in SHAPES:
        assert 128 * Kp < 2 ** 31, name                       # every |Gacc| partial: |digit| <= 128 over at most Kp samples
        for lf in (2, 3, 4, 5):
            sabs = (Qfp + 1) * 2 ** (8 * lf - 2)              # sum |q| at most: |q| <= 2^(8 LF - 2) per column, the constant column too
            assert sabs < 2 ** 53 and 3 * sabs < 2 ** 53, name  # fl(sum |q|) exact; |qconst - 2 A| <= 3 sum |q|
            assert 128 * Qfp * 257 < 2 ** 31, name              # acc0 + (acc1 << 8) in int32
        csum = Kp * 2 ** 31
        s = sum(256 ** l * 128 * Kp for l in range(4))
        assert csum + 2 * s < 2 ** 53, name                    # (double)(csum - 2 s) is exact


def test_share_of_elements_float64_alone_decides():
    """u_of evaluates in rational arithmetic the elements within NEAR = 2^-20 of a half-integer; the dither makes y equidistributed
    modulo 1, so their share is about 2^-19, far below the 0.001 a looser rule would be allowed to leave undecided.  And on those
    elements the rational path is the one that matters: forced onto every element it returns the same integers."""
    rng = np.random.default_rng(9)
    n = 1 << 17
    hh = rng.integers(0, M.VMAX[4], size=n).astype(np.float64)
    e = rng.uniform(-1, 1, size=n)
    d32 = M.dither(5, np.arange(n))
    u, near = H.u_of(hh, e, d32)
    assert 1.0 - near / n >= 0.999
    idx = rng.integers(0, n, size=3000)
    assert all(int(u[i]) == H._exact_u(hh[i], e[i], d32[i]) for i in idx)
    # a tie of the second rounding: y = 2.5 exactly rounds to 2, y = 3.5 to 4; a tie of the first: ulp-level
    z = np.zeros(2, dtype=np.int64)
    assert H.u_of(np.array([5.0, 7.0]), np.array([0.5, 0.5]), z)[0].tolist() == [2, 4]
    assert H.u_of(np.array([1.0, 1.0]), np.array([0.0, 0.0]), np.array([-(1 << 31), (1 << 31) - 1]))[0].tolist() == [0, 0]
