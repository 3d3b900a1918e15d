"""tests/_i8_pass_reference.py, the host model tests/test_gpu_i8_pass_exact.py holds the int8-limb pass to, against brute force on tiny
cases -- entry by entry, and with code that shares nothing with the model's own:
  * vq_pos and the offset of every (row, plane, sample) against tests/native/i8_pass_tables.cpp, which walks the bytes of an image in
    memory order with csrc/gml_bits.h's own vq_sample;
  * the digit split and its inverse over the whole range of both plane counts, with the device's own bit trick ((v + C) ^ C on the
    two's complement word, C = 0x80 in every byte) as the other statement;
  * the dither of a few (node, sample) pairs written out by hand, wrap-around of k * GOLD included;
  * the two finalise formulas against exact rational arithmetic and one rounding;
  * the backward sums against a triple loop (K = 70, n = 5), the slot sums against loops over the samples;
  * the forward numbers against decimal arithmetic (50 digits) element by element.
Then the same checks on a model whose dither index is shifted by one, which drops a digit, or whose layout map swaps two bytes: each
must fail.  No GPU, no library."""
import decimal
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _i8_pass_reference as M
from _i8_pack_reference import quantise
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "i8_pass_tables.cpp")
CSRC = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "csrc")
D = decimal.Decimal
HAVE_LD = np.finfo(np.longdouble).nmant >= 63
need_ld = pytest.mark.skipif(not HAVE_LD, reason="np.longdouble is not the 80-bit x87 format here")
SLOTS, KP = 64, 192


# ---------------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("i8_pass_tables") / "i8_pass_tables")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], input=f"{SLOTS} {KP}", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {"off": {4: [], 6: []}}
    for line in r.stdout.splitlines():
        name, *rest = line.split()
        nums = [int(x) for x in rest]
        if name == "off":
            out["off"][nums[0]].append(nums[1:])
        else:
            out[name] = nums
    return out


def layout_mismatches(t):
    bad = sum(t["vq_pos"][s] != M.vq_pos(s) for s in range(64))
    for lbt in (4, 6):
        rows = np.array(t["off"][lbt])
        assert len(rows) == SLOTS * lbt * KP and sorted(rows[:, 3].tolist()) == list(range(len(rows)))
        want = [M.vq_off(int(r), int(l), int(k), KP, lbt) for r, l, k, _ in rows]
        bad += int((np.array(want) != rows[:, 3]).sum())
        # the vectorised unpacking is the same map: a buffer that holds its own offsets (mod 251) comes out where vq_off says
        buf = (np.arange(len(rows)) % 251 - 125).astype(np.int8)
        pl = M.unpack_vq(buf, SLOTS, KP, lbt)
        bad += int((pl[rows[:, 0], rows[:, 1], rows[:, 2]] != buf[rows[:, 3]]).sum())
        bad += int((M.pack_vq(pl) != buf).sum())
    return bad


def test_layout_matches_the_header(tables):
    assert sorted(tables["vq_pos"]) == list(range(64))
    assert [tables["vq_sample"][tables["vq_pos"][s]] for s in range(64)] == list(range(64))
    assert layout_mismatches(tables) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# digits
# ---------------------------------------------------------------------------------------------------------------------------
def _device_digits(v, lbt):
    """(v + C) ^ C on the two's complement word of 8 lbt bits, C = 0x80 in every byte; byte l, read as signed, is digit l"""
    bits = 8 * lbt
    c = int("80" * lbt, 16)
    word = (((v + (1 << bits)) % (1 << bits)) + c) % (1 << bits) ^ c
    return [((word >> (8 * l)) & 255) - 256 * (((word >> (8 * l)) & 255) >= 128) for l in range(lbt)]


def _digit_values(lbt):
    rng = np.random.default_rng(lbt)
    v = [0, 1, -1, 127, -127, 128, -128, 129, -129, 255, 256, -256, 32639, 32640, -32896, M.VMAX[lbt], M.VMAX[lbt] - 1, M.VMIN[lbt], M.VMIN[lbt] + 1]
    v += [0x7F7F7F7F, -0x80808080] if lbt == 6 else []
    v += [int(x) for x in rng.integers(M.VMIN[lbt], M.VMAX[lbt] + 1, size=4000)]
    v += [int(x) for b in range(1, 8 * lbt - 1) for x in ((1 << b) - 1, 1 << b, -(1 << b), -(1 << b) - 1) if M.VMIN[lbt] <= x <= M.VMAX[lbt]]
    return v


def digit_mismatches():
    bad = 0
    for lbt in (4, 6):
        v = _digit_values(lbt)
        d = M.digits_of(np.array(v, dtype=np.int64), lbt)
        for i, x in enumerate(v):
            bad += [int(a) for a in d[:, i]] != _device_digits(x, lbt)
        back = M.value_of(np.ascontiguousarray(d.T)[None].transpose(0, 2, 1))  # [1 slot][lbt][samples]
        bad += int((back[0] != np.array(v, dtype=np.int64)).sum())
    return bad


def test_digit_split_and_inverse_over_the_whole_range():
    assert _device_digits(0x7F7F7F7F, 4) == [127] * 4 and _device_digits(-0x80808080, 4) == [-128] * 4
    assert _device_digits(128, 4) == [-128, 1, 0, 0] and _device_digits(-129, 4) == [127, -1, 0, 0]
    assert digit_mismatches() == 0
    for lbt in (4, 6):
        for x in (M.VMAX[lbt] + 1, M.VMIN[lbt] - 1):
            with pytest.raises(AssertionError):
                M.digits_of(np.array([x], dtype=np.int64), lbt)


def test_coarse_forms_of_the_planes():
    rng = np.random.default_rng(5)
    for lbt in (4, 6):
        unit, pl0 = M.COARSE_UNIT[lbt], M.COARSE_PL0[lbt]
        mag = rng.integers(-0x808080, 0x7F7F7F + 1, size=(32, 64))  # what three balanced digits spell
        d = np.ascontiguousarray(M.digits_of(mag * unit, lbt).transpose(1, 0, 2))  # [32][lbt][64]
        assert not d[:, :pl0].any() and d[:, pl0:].any()
        assert np.array_equal(M.value_of(d), mag * unit)
        stale = d.copy()
        stale[:, :pl0 - 1] = 77  # what an earlier full-width pass left in the planes a coarse pass does not write
        assert np.array_equal(M.value_of(M.live_planes(stale, True)), mag * unit)
        assert not np.array_equal(M.value_of(M.live_planes(stale, False)), mag * unit) or pl0 == 1
        s = M.slot_sums(stale, True, True, True)
        assert np.array_equal(s["csum"] + (s["csum2"] << 24), (mag * unit).sum(axis=1))
        if lbt == 6:
            assert not s["csum"].any()


# ---------------------------------------------------------------------------------------------------------------------------
# dither
# ---------------------------------------------------------------------------------------------------------------------------
HAND = [  # (u, k, low 32 bits of u * 0x85EBCA6B + k * 0x9E3779B9 as a signed integer)
    (0, 0, 0),
    (0, 1, 0x9E3779B9 - 2 ** 32),          # GOLD itself is above 2^31: negative
    (1, 0, 0x85EBCA6B - 2 ** 32),
    (0, 2, 0x3C6EF372),                    # 2 GOLD wraps once
    (1, 1, 0x24234424),                    # 0x85EBCA6B + 0x9E3779B9 = 0x1_24234424
    (96, 10006, None),
    (3, (2 ** 31) // 0x9E3779B9 + 1, None),
    (7, 2 ** 31 + 5, None),                # an index past 2^31
    (2 ** 20, 2 ** 24 + 123, None),
]


def dither_mismatches():
    bad = 0
    for u, k, want in HAND:
        low = (u * 0x85EBCA6B + k * 0x9E3779B9) % 2 ** 32
        byhand = low - 2 ** 32 if low >= 2 ** 31 else low
        assert want is None or want == byhand
        bad += int(M.dither(u, k)) != byhand
    got = M.dither(5, np.arange(300))
    bad += sum(int(got[k]) != ((5 * 0x85EBCA6B + k * 0x9E3779B9 + 2 ** 31) % 2 ** 32) - 2 ** 31 for k in range(300))
    return bad


def test_dither_by_hand():
    assert dither_mismatches() == 0
    d = M.dither(11, np.arange(100000)) / 2.0 ** 32
    assert -0.5 <= d.min() and d.max() < 0.5 and abs(d.mean()) < 0.01  # a Weyl sequence: equidistributed


# ---------------------------------------------------------------------------------------------------------------------------
# slot sums, backward, finalise
# ---------------------------------------------------------------------------------------------------------------------------
def _tiny(lbt, coarse, seed, K=70, n=5):
    """planes of 32 slots over Kp = 128 samples as a pass of that form leaves them, bits of n statistics in 64 columns"""
    rng = np.random.default_rng(seed)
    Kp = 128
    unit = M.COARSE_UNIT[lbt] if coarse else 1
    top = 0x7F7F7F if coarse else M.VMAX[lbt]
    val = rng.integers(-top, top + 1, size=(32, Kp)) * unit
    val[:, K:] = 0
    val[3, 7] = top * unit
    val[4, 9] = (-top if coarse else M.VMIN[lbt]) * unit  # (coarse magnitudes stay below vdiv / unit < 2^23 - 3, where k_fwd_i8w caps its mmax)
    planes = np.ascontiguousarray(M.digits_of(val, lbt).transpose(1, 0, 2))
    bits = np.zeros((64, Kp), dtype=np.uint8)
    bits[:n, :K] = rng.integers(0, 2, size=(n, K))
    return planes, val, bits, K, n


def sums_mismatches():
    bad = 0
    for lbt in (4, 6):
        for coarse in (False, True):
            planes, val, _, K, _ = _tiny(lbt, coarse, 10 * lbt + coarse)
            unit = M.COARSE_UNIT[lbt] if coarse else 1
            s = M.slot_sums(planes, coarse, True, True)
            for r in range(32):
                tot = sum(int(v) for v in val[r])
                ab = [abs(int(v)) // unit for v in val[r]]
                if lbt == 4:
                    bad += int(s["csum"][r]) != tot
                    bad += int(s["asum"][r]) != sum(ab) * unit
                    bad += int(s["mmax"][r]) != ((max(ab) + 1) << 8 if coarse else max(ab))
                else:
                    lo = sum(int(planes[r, l, k]) * 256 ** l for l in range(3) for k in range(128))
                    hi = sum(int(planes[r, l, k]) * 256 ** (l - 3) for l in range(3, 6) for k in range(128))
                    bad += (int(s["csum"][r]), int(s["csum2"][r])) != ((0 if coarse else lo), hi)
                    bad += int(s["csum"][r]) + (int(s["csum2"][r]) << 24) != tot
                    waves = [sum(ab[64 * w:64 * w + 64]) for w in range(2)]
                    bad += int(s["asum"][r]) != sum(w & 0xFFFFFFFF for w in waves)
                    bad += int(s["asum2"][r]) != sum(w >> 32 for w in waves)
                    bad += (int(s["asum2"][r]) << 32) + int(s["asum"][r]) != sum(ab)
                    a, b = s["mmax"][r]
                    # (mmax + 1) 2^16 tau bounds |V|, and exceeds it by little: the header's statement of what the number is for
                    bad += not (a <= b and (a + 1) * 65536 > max(ab) * unit)
                    bad += not (b * 65536 <= (max(ab) + 4) * unit * (1 + 2.0 ** -19) + 2 * 65536)
            z = M.slot_sums(planes, coarse, True, False)
            bad += bool(np.any(z["asum"])) + bool(np.any(z["asum2"]))
    return bad


def test_slot_sums_against_loops():
    assert sums_mismatches() == 0
    # the high word: ymax is the next double with a zero low word above the largest y
    assert M.mmax_wide_of_y(0.0, False) == 0 and M.mmax_wide_of_y(2.0 ** 48 * 1.5, False) == 1
    assert M.mmax_wide_of_y(2.0 ** 32 * 5, True) == (5 + 2) << 8 and M.mmax_wide_of_y(2.0 ** 32 * (2 ** 23 + 9), True) == (8388605 + 2) << 8
    # full width: |V| / tau < ymax 2^-32 + 1/2 and mmax = floor((ymax 2^-32 + 1/2) / 2^16) with ymax within 2^-20 above y
    m = M.mmax_wide_of_y(2.0 ** 32 * 1.4e14, False)
    assert 1.4e14 / 65536 - 1 <= m <= 1.4e14 * (1 + 2.0 ** -19) / 65536 + 1


def backward_mismatches():
    bad = 0
    for lbt in (4, 6):
        for coarse in (False, True):
            planes, _, bits, K, n = _tiny(lbt, coarse, 20 * lbt + coarse)
            g = M.backward(planes, bits, coarse)
            pl0 = M.COARSE_PL0[lbt] if coarse else 0
            for r in (0, 3, 4, 31):
                for l in range(lbt):
                    for c in range(n + 1):
                        want = sum(int(planes[r, l, k]) * int(bits[c, k]) for k in range(K)) if l >= pl0 else 0
                        bad += int(g[r, l, c]) != want
            bad += bool(g[:, :, n:].any())
            dev = np.ascontiguousarray(g.reshape(1, 32, lbt, 64).transpose(0, 2, 1, 3)).astype(np.int32)  # the device's order
            bad += not np.array_equal(M.gacc_rows(dev, 32, lbt, 64), g)
    return bad


def test_backward_against_a_triple_loop():
    assert backward_mismatches() == 0


def _round(fr):
    """a rational to the nearest double, ties to even"""
    return float(fr) if isinstance(fr, Fraction) else float(Fraction(fr))


def finalize_mismatches():
    bad = 0
    for lbt in (4, 6):
        for coarse in (False, True):
            planes, val, bits, K, n = _tiny(lbt, coarse, 30 * lbt + coarse)
            g = M.backward(planes, bits, coarse)
            rowcol = np.full(32, -1)
            rowcol[:6] = [0, 4, 2, 2, 1, 3]
            tau = np.random.default_rng(lbt).uniform(1e-14, 3e-9, size=32) * (1 + 2.0 ** -30)
            Qf, Qp, cconst = n, 128, 64
            for want_grad in (True, False):
                s = M.slot_sums(planes, coarse, True, not want_grad)
                G, f = M.finalize(lbt, coarse, tau, s, g, rowcol, Qf, Qp, cconst, want_grad, True)
                for r in range(32):
                    if rowcol[r] < 0:
                        bad += not (np.isnan(f[r]) and (G is None or np.isnan(G[r]).all()))
                        continue
                    t = Fraction(float(tau[r]))
                    x = 1 - 2 * bits[:, :].astype(np.int64)
                    if want_grad:
                        # sum_k V x exactly, rounded once to the double the kernel multiplies tau with, then the product rounded
                        for c in range(Qp):
                            if c < Qf:
                                inner = sum(int(val[r, k]) * int(x[c, k]) for k in range(128))
                            elif c == cconst:
                                inner = sum(int(v) for v in val[r])
                            else:
                                inner = None
                            want = 0.0 if inner is None else _round(t * Fraction(_round(Fraction(inner))))
                            bad += G[r, c] != want
                        u = int(rowcol[r])
                        inner = sum(int(val[r, k]) * int(x[u, k]) for k in range(128))
                        bad += f[r] != -_round(t * Fraction(_round(Fraction(inner))))
                    else:
                        unit = M.COARSE_UNIT[lbt] if coarse else 1
                        tot = sum(abs(int(v)) for v in val[r])
                        if lbt == 4:
                            want = _round(t * Fraction(_round(Fraction(tot))))
                        else:  # asum2 2^32 + asum = sum |V| / (unit tau) rounded once; tau * unit is exact
                            want = _round(t * unit * Fraction(_round(Fraction(tot // unit))))
                        bad += f[r] != want
    return bad


def test_finalise_against_rational_arithmetic():
    assert finalize_mismatches() == 0


def test_finalise_rounds_once():
    # a sum above 2^53: csum2 2^24 + csum is rounded once, not its halves separately (the i8w formula; 2^24 (2^30 + 1) + (2^23 + 1))
    cs2, cs = 2 ** 30 + 1, 2 ** 29 + 2 ** 23 + 1
    assert M._gcol(6, False, cs, cs2, [0] * 6) == float(cs2 * 2 ** 24 + cs)
    assert M._gcol(6, True, cs, cs2, [0] * 6) == float(cs2 * 2 ** 24)
    assert M._gcol(4, False, 10, 0, [1, 1, 0, 0]) == float(10 - 2 * 257)


# ---------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------
def _forward_case(form, lbt, coarse, lf, seed):
    rng = np.random.default_rng(seed)
    n, K, Kp, Qfp, cconst, Qp = 5, 70, 128, 64, 64, 128
    spins = rng.choice([-1, 1], size=(K, n))
    u = int(rng.integers(0, n))
    th = np.zeros(Qp)
    th[:n] = rng.normal(size=n) * 0.7
    th[u] = 0.0
    th[cconst] = rng.normal() * 0.3
    bits = np.zeros((Qfp, Kp), dtype=np.uint8)
    bits[:n, :K] = (spins.T < 0)
    counts = np.floor(10 ** rng.uniform(0, 3, size=K))
    counts[5] = 0.0
    w = np.zeros(Kp)
    w[:K] = counts / counts.sum()
    lfq = 7 if lbt == 6 else (4 if coarse else lf)
    sx, q, q0 = quantise(th, Qfp, cconst, lfq)
    sabs = abs(int(q0)) + sum(abs(int(x)) for x in q)
    vdiv = 2130000000.0 if lbt == 4 else 1.400e14
    tau = (2.0 * w.max() if form == "RPLE" else w.max() * np.exp(sabs * 2.0 ** sx)) * (1 + 1e-12) / vdiv
    return dict(form=form, lbt=lbt, coarse=coarse, lf=lf, th=th, Qfp=Qfp, cconst=cconst, u=u, sbit=bits[u].copy(), bits=bits, w=w, tau=float(tau),
                K=K, spins=spins, sx=sx, q=q, q0=q0)


def forward_mismatches(cases):
    bad = 0
    decimal.getcontext().prec = 50
    for c in cases:
        o = M.forward_row(c["form"], c["lbt"], c["coarse"], c["lf"], c["th"], c["Qfp"], c["cconst"], c["u"], c["sbit"], c["bits"], c["w"],
                          c["tau"], c["K"])
        unit = M.COARSE_UNIT[c["lbt"]] if c["coarse"] else 1
        q, q0, sx = [int(x) for x in c["q"]], int(c["q0"]), c["sx"]
        if c["coarse"] and c["lbt"] == 6:  # the top four planes: q with three balanced digits taken off
            def top(v):
                for _ in range(3):
                    v = (v - (((v + 128) & 255) - 128)) >> 8
                return v
            q, q0, sx = [top(x) for x in q], top(q0), sx + 24
        for k in range(c["K"]):
            s = int(c["spins"][k, c["u"]])
            eint = q0 + sum(q[j] * int(c["spins"][k, j]) for j in range(c["spins"].shape[1]))
            E = D(s * eint) * D(2) ** sx
            F = (-E).exp() if c["form"] != "RPLE" else 2 / (1 + (2 * E).exp())
            low = (c["u"] * 0x85EBCA6B + k * 0x9E3779B9) % 2 ** 32
            dith = D(low - 2 ** 32 if low >= 2 ** 31 else low) / D(2 ** 32)
            y = D(float(c["w"][k])) / (D(c["tau"]) * unit) * F + dith
            want = int(y.to_integral_value(rounding=decimal.ROUND_HALF_EVEN)) if c["w"][k] > 0 else 0
            margin = abs(y - y.to_integral_value(rounding=decimal.ROUND_FLOOR) - D("0.5"))
            bad += bool(o["real"][k]) != (c["w"][k] > 0)
            bad += abs(D(float(o["y"][k])) - y) > D("1e-4") + abs(y) * D(2) ** -50  # (float(): the comparison only, 53 bits of the model's y)
            bad += abs(D(float(o["margin"][k])) - margin) > D("1e-4") + abs(y) * D(2) ** -50
            if margin > abs(y) * D(2) ** -60 + D("1e-15"):
                bad += int(o["mag"][k]) != want
            bad += int(o["sign"][k]) != -s
            bad += abs(o["E"][k] - float(E)) > 1e-15 * (1 + abs(float(E)))
        bad += bool(np.any(o["mag"][c["K"]:])) + bool(np.any(o["real"][c["K"]:]))
    return bad


def _forward_cases():
    return [_forward_case(form, lbt, coarse, lf, seed)
            for seed, (form, lbt, coarse, lf) in enumerate([("RISE", 4, False, 5), ("RISE", 4, False, 3), ("RISE", 4, False, 4), ("RISE", 4, True, 0),
                                                            ("RPLE", 4, False, 5), ("RISE", 6, False, 0), ("RISE", 6, True, 0), ("RPLE", 6, False, 0)])]


@need_ld
def test_forward_against_decimal_arithmetic():
    assert forward_mismatches(_forward_cases()) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the checks above notice a perturbed model
# ---------------------------------------------------------------------------------------------------------------------------
@need_ld
def test_a_shifted_dither_index_is_noticed(monkeypatch):
    orig = M.dither
    monkeypatch.setattr(M, "dither", lambda u, k: orig(u, np.asarray(k) + 1))
    assert dither_mismatches() > 0
    assert forward_mismatches(_forward_cases()[:1]) > 0


def test_a_dropped_digit_is_noticed(monkeypatch):
    orig = M.digits_np

    def dropped(v, n):
        d, rest = orig(v, n)
        d[0] = 0
        return d, rest

    monkeypatch.setattr(M, "digits_np", dropped)
    assert digit_mismatches() > 0
    monkeypatch.undo()
    orig_v = M.value_of
    monkeypatch.setattr(M, "value_of", lambda planes: orig_v(np.concatenate([np.zeros_like(planes[:, :1]), planes[:, 1:]], axis=1)))
    assert digit_mismatches() > 0 and sums_mismatches() > 0
    monkeypatch.undo()
    orig_b = M.backward

    def short(planes, bits, coarse):  # one sample's lowest digit left out of the GEMM
        p = planes.copy()
        p[:, M.COARSE_PL0[p.shape[1]] if coarse else 0, 11] = 0
        return orig_b(p, bits, coarse)

    monkeypatch.setattr(M, "backward", short)
    assert backward_mismatches() > 0 and finalize_mismatches() > 0


def test_a_perturbed_layout_map_is_noticed(tables, monkeypatch):
    pos = M._POS.copy()
    pos[[8, 9]] = pos[[9, 8]]
    monkeypatch.setattr(M, "_POS", pos)
    assert layout_mismatches(tables) > 0
    monkeypatch.undo()
    orig = M.vq_pos
    monkeypatch.setattr(M, "vq_pos", lambda s: orig(s ^ 4))  # the two lane halves exchanged
    assert layout_mismatches(tables) > 0
