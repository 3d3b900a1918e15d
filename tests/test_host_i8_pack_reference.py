"""tests/_i8_pack_reference.py, the host model tests/test_gpu_i8_pack_state.py holds the device to, against the headers the kernels
compile: tests/native/i8_pack_tables.cpp prints the tables of xb_col, vq_sample, pair_slot, pair_col and xtb_from_natural (on
single-bit words), and pair_in_range and seven balanced digits on a fixed list of integers -- 0, +-1, +-127, +-128, PAIR_MAX and
PAIR_MIN with both neighbours, +-(2^55 - 4) and 300 seeded random values below 2^55.  The model must agree entry for entry.  Then
the model against itself: digits recombine, images decode, the documented worked examples.  No GPU, no library."""
import math
import os
import subprocess

import numpy as np
import pytest

import _i8_pack_reference as R
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "i8_pack_tables.cpp")
CSRC = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "csrc")


def _values():
    v = [0, 1, -1, 127, -127, 128, -128, R.PAIR_MAX, R.PAIR_MAX + 1, R.PAIR_MAX - 1, R.PAIR_MIN, R.PAIR_MIN + 1, R.PAIR_MIN - 1,
         2 ** 55 - 4, -(2 ** 55 - 4), 2 ** 54 - 2, -(2 ** 54 - 2), 2 ** 54, -(2 ** 54)]
    rng = np.random.default_rng(20)
    for _ in range(300):
        bits = int(rng.integers(1, 56))
        v.append(int(rng.integers(-(2 ** bits) + 1, 2 ** bits)))
    return v


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("i8_pack_tables") / "i8_pack_tables")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe])
    v = _values()
    r = subprocess.run([exe], input=" ".join(str(x) for x in [len(v)] + v), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = {"digits": [], "range": []}
    for line in r.stdout.splitlines():
        name, *rest = line.split()
        nums = [int(x) for x in rest]
        if name in out:
            out[name].append(nums)
        else:
            out[name] = nums
    return v, out


def test_index_maps_match_the_headers(tables):
    _, t = tables
    assert t["xb_col"] == [R.xb_col(j, h) for h in range(2) for j in range(32)]
    assert t["vq_sample"] == [R.vq_sample(p) for p in range(64)]
    assert t["pair_slot"] == [R.pair_slot(h, m) for h in range(2) for m in range(16)]
    assert t["pair_col"] == [R.pair_col(h, m, s) for h in range(2) for m in range(16) for s in range(2)]
    assert t["xtb_from_natural"] == [R.xtb_from_natural(1 << i) for i in range(32)]
    assert t["limits"] == [R.PAIR_UNIT, R.PAIR_MAX, R.PAIR_MIN]
    # each is a bijection, and the two statements of the backward dword in gml_bits.h agree: bit j of dword h holds the sample
    # vq_sample(xb_col(j, h)) of the step, i.e. natural bit vq_sample(...) - 32 h of word h
    for h in range(2):
        assert sorted(R.xb_col(j, h) for j in range(32)) == sorted(c for c in range(64) if (c >> 4) & 1 == h)
        for j in range(32):
            assert R.xtb_bit(R.vq_sample(R.xb_col(j, h)) - 32 * h) == j
    assert sorted(R.vq_sample(p) for p in range(64)) == list(range(64))
    assert sorted(s + d for h in range(2) for m in range(16) for s in [R.pair_slot(h, m)] for d in (0, 1)) == list(range(64))
    assert sorted(R.pair_col(h, m, s) for h in range(2) for m in range(16) for s in range(2)) == list(range(64))


def test_digits_and_range_match_the_headers(tables):
    v, t = tables
    assert len(t["digits"]) == len(v) and len(t["range"]) == 3 * len(v)
    for x, row in zip(v, t["digits"]):
        d, rest = R.balanced_digits(x, 7)
        assert row == [x] + d + [rest], x
        assert all(-128 <= e <= 127 for e in d) and sum(e * 256 ** l for l, e in enumerate(d)) + rest * 256 ** 7 == x
        assert (rest == 0) == (R.PAIR_MIN <= x <= R.PAIR_MAX), x  # seven digits spell exactly that range
        dn, rn = R.digits_np(np.array([x]), 7)
        assert dn[:, 0].tolist() == d and int(rn[0]) == rest
        assert int(R.undigits_np(dn)[0]) == x - rest * 256 ** 7
    seen = set()
    for a, b, ok in t["range"]:
        assert bool(ok) == R.pair_in_range(a, b), (a, b)
        seen.add(bool(ok))
    assert seen == {False, True}
    # only the difference outside: q = -q' at full scale; the range reaches one unit further down than up
    q = 2 ** 54 - 2
    assert not R.pair_in_range(q, -q) and not R.pair_in_range(q, q) and R.pair_in_range(-q, -q) and R.pair_in_range(-q, q)
    assert R.balanced_digits(-2 * q, 7) == ([4, 0, 0, 0, 0, 0, -128], 0)


def test_quantisation_examples():
    Qfp, cconst = 192, 192
    big = float(np.nextafter(0.125, 0.0))
    th = np.zeros(256)
    th[:129] = big
    sx, margin = R.sigma_exponent(th, Qfp, cconst, 7)
    assert sx == -56 and margin > 1e-3  # sum |theta| = 16.125 > 2^(-57 + 61): one exponent up, far from the next power of two
    th[:] = 0.0
    th[[3, 7]] = big
    sx, q, q0 = R.quantise(th, Qfp, cconst, 7)
    assert sx == -57 and int(q[3]) == 2 ** 54 - 2 and q0 == 0
    for lf in (3, 4, 5):
        assert R.sigma_exponent(th, Qfp, cconst, lf)[0] == -3 - (8 * lf - 2)
    assert R.sigma_exponent(np.zeros(256), Qfp, cconst, 7) == (-54, 1.0)
    s = R.row_scalars(th, Qfp, cconst, 7)
    assert s["qconst"] == 2 ** 55 - 4 and s["sabs"] == 2 ** 55 - 4 and s["qpair"] == 0
    assert s["qconst2"] == 2 * ((2 ** 54 - 2 + 2) >> 24)  # digits [-2, 0, 0, ...]: the rest after three is 2^30


def test_images_decode_and_marks():
    rng = np.random.default_rng(4)
    Qfp, cconst = 192, 192
    rows = rng.normal(scale=0.001, size=(32, 256)) * (rng.random((32, 256)) < 0.2)
    rows[:, 192:] = 0.0
    rows[:, cconst] = 0.01
    act = [True] * 32
    assert not R.tile_marked(rows, act, Qfp, cconst)
    nk, cm = R.column_union(rows, act, Qfp, 3)
    assert nk == 3 and (cm[:-1][cm[1:] >= 0] < cm[1:][cm[1:] >= 0]).all()
    for paired in (False, True):
        for lst in (None, cm):
            img = R.row_image(rows[5], Qfp, cconst, 7, paired, lst)
            _, q, _ = R.quantise(rows[5], Qfp, cconst, 7)
            assert np.array_equal(R.decode_image(img, paired), R._grid(q, Qfp, lst))
    big = float(np.nextafter(0.125, 0.0))
    c0, c1 = 128 + R.pair_col(1, 5, 0), 128 + R.pair_col(1, 5, 1)
    assert (c0, c1) == (153, 157)
    rows[9, [c0, c1]] = big
    assert R.tile_marked(rows, act, Qfp, cconst)
    act[9] = False
    assert not R.tile_marked(rows, act, Qfp, cconst)  # an inactive row marks nothing
    # a union above the capacity has no list; one of exactly the capacity has
    assert R.column_union(rows, [True] * 32, Qfp, 1) == (-1, None)
    one = np.zeros((32, 256))
    one[0, :64] = 1.0
    nk, cm = R.column_union(one, [True] * 32, Qfp, 1)
    assert nk == 1 and cm.tolist() == list(range(64))
    assert R.compact_steps(64) == 0 and R.compact_steps(128) == 1 and R.compact_steps(512) == 2 and R.compact_steps(64 * 200) == 32


def test_bit_images_of_a_small_problem():
    rng = np.random.default_rng(5)
    n, K, Kp = 12, 70, 1024
    spins = rng.choice(np.array([-1, 1], dtype=np.int8), size=(K, n))
    keys = R.stat_keys(n, 3)
    assert keys.shape == (12 + 66, 2) and keys[0].tolist() == [0, -1] and keys[12].tolist() == [0, 1] and keys[-1].tolist() == [10, 11]
    B = R.stat_bits(spins, keys, 128, Kp)
    assert B[12, :K].tolist() == ((spins[:, 0] * spins[:, 1]) < 0).astype(int).tolist() and not B[:, K:].any() and not B[78:].any()
    xb = R.xb_image(B, Kp, 128)
    xtb = R.xtb_image(B, Kp, 128)
    assert xb.size == Kp * 128 // 32 and xtb.size == 256 * Kp // 32
    for k, c in ((0, 0), (69, 77), (33, 12), (5, 64), (64, 70)):
        kt, j64 = c // 64, c % 64
        h = (j64 >> 4) & 1
        j = [R.xb_col(b, h) for b in range(32)].index(j64)
        assert (int(xb[(((k >> 7) * 2 + kt) * 128 + (k & 127)) * 2 + h]) >> j) & 1 == B[c, k]
        st, s64 = k // 64, k % 64
        pos = [R.vq_sample(p) for p in range(64)].index(s64)
        h = (pos >> 4) & 1
        j = [R.xb_col(b, h) for b in range(32)].index(pos)
        assert (int(xtb[(((c >> 7) * (Kp // 64) + st) * 128 + (c & 127)) * 2 + h]) >> j) & 1 == B[c, k]
    assert sum(bin(int(x)).count("1") for x in xb) == int(B.sum()) == sum(bin(int(x)).count("1") for x in xtb)
    cm = np.array([77, 3] + [-1] * 62, dtype=np.int32)
    xc = R.xc_image(B, Kp, 1, cm)
    assert sum(bin(int(x)).count("1") for x in xc) == int(B[77].sum() + B[3].sum())


def test_tau_is_formed_in_extended_precision():
    t = R.tau(2 ** 55, -57, 0.25, "RISE", 6)
    assert abs(float(t) / (0.25 * math.exp(0.25) * (1 + 1e-12) / 1.4e14) - 1) < 1e-15
    assert float(R.tau(123, -57, 0.25, "RPLE", 4)) == pytest.approx(0.5 * (1 + 1e-12) / 2.13e9, rel=1e-15)
