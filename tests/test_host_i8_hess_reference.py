"""tests/_i8_hess_reference.py, the host model tests/test_gpu_i8_hess_exact.py holds the device to, against the header the kernels
compile: tests/native/i8_hw.cpp prints hw_shift, hw_dither, hw_clip and hw_digits of csrc/gml_i8_hw.h on
  * every mm of the form 2^a - 1, 2^a, 2^a + 1 for a in 0..31, and 32638, 32639, 32640;
  * for each of them (its shift), the magnitudes 0, 1, mm, mm - 1 and a few thousand random ones, under random (node, sample) pairs
    (samples beyond 2^32 included: the kernel takes their low 32 bits).
The model must agree entry for entry.  Then the properties the kernels rely on: the shift is the smallest that fits, no exp-form
weight mag <= mm reaches the clip, the digits recombine and stay in their ranges, and the layouts of the model invert.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import _i8_hess_reference as H
import _i8_pack_reference as R
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "i8_hw.cpp")
CSRC = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "csrc")


def _mms():
    out = []
    for a in range(32):
        out += [2 ** a - 1, 2 ** a, 2 ** a + 1]
    return sorted(set(out + [32638, 32639, 32640, 2 ** 32 - 1]))


def _cuts():
    rng = np.random.default_rng(31)
    out = []
    for mm in _mms():
        mags = [0, 1, mm, max(mm - 1, 0)] + [int(x) for x in rng.integers(0, mm + 1, size=40)] + [int(x) for x in rng.integers(0, 2 ** 32, size=8)]
        for mag in mags:
            u = int(rng.integers(0, 2 ** 20))
            k = int(rng.integers(0, 2 ** 34)) if rng.random() < 0.2 else int(rng.integers(0, 2 ** 24))
            out.append((u, k, mm, mag))
    return out


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("i8_hw") / "i8_hw")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe])
    mms, cuts = _mms(), _cuts()
    text = " ".join(str(x) for x in [len(mms)] + mms + [len(cuts)] + [v for c in cuts for v in c])
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    shift, cut, limits = [], [], None
    for line in r.stdout.splitlines():
        name, *rest = line.split()
        nums = [int(x) for x in rest]
        if name == "shift":
            shift.append(nums)
        elif name == "cut":
            cut.append(nums)
        else:
            limits = nums
    return mms, cuts, shift, cut, limits


def test_shift_matches_the_header(native):
    mms, _, shift, _, limits = native
    assert limits == [H.HL, H.CLIP]
    assert [s[0] for s in shift] == mms
    seen = set()
    for mm, sh_exp, sh_rple in shift:
        assert sh_exp == H.hw_shift(mm, "RISE") == H.hw_shift(mm, "logRISE"), mm
        assert sh_rple == H.hw_shift(mm, "RPLE") == 16
        seen.add(sh_exp)
        if mm < 2 ** 32 - 1:  # the smallest shift under which the row's largest weight, dithered, fits two balanced digits
            assert (mm >> sh_exp) + 1 <= H.CLIP and (sh_exp == 0 or (mm >> (sh_exp - 1)) + 1 > H.CLIP), mm
    assert seen == set(range(18))  # every shift a 32-bit mm can ask for
    assert H.hw_shift(32638, "RISE") == 0 and H.hw_shift(32639, "RISE") == 1 and H.hw_shift(2 ** 31 + 1, "RISE") == 17
    assert H.hw_shift(2 ** 32 - 1, "RISE") == 0  # (mm + 1 wraps to 0 in 32 bits: the passes never record it, |V| / tau < 2^31)


def test_dither_clip_and_digits_match_the_header(native):
    _, cuts, _, cut, _ = native
    assert len(cut) == 2 * len(cuts) > 4000
    clipped = 0
    for i, (u, k, mm, mag) in enumerate(cuts):
        for f, form in enumerate(("RISE", "RPLE")):
            row = cut[2 * i + f]
            assert row[:5] == [u, k, mm, mag, 2 * f]
            sh = H.hw_shift(mm, form)
            dth = int(H.dither(u, np.array([k]), sh)[0])
            h2 = int(H.clip(np.array([mag]), dth, sh)[0])
            lo, hi = (int(x[0]) for x in H.split(np.array([h2])))
            assert row[5:] == [sh, dth, h2, lo, hi], (u, k, mm, mag, form)
            assert 0 <= dth < 2 ** sh and 0 <= h2 <= H.CLIP
            assert -128 <= lo <= 127 and 0 <= hi <= 127 and lo + 256 * hi == h2
            # the floor of the dithered weight: within one unit of 2^sh below, less than one above
            if h2 < H.CLIP:
                assert mag - 2 ** sh < h2 * 2 ** sh <= mag + 2 ** sh - 1
            clipped += h2 == H.CLIP and (mag + dth) >> sh > H.CLIP
            # an exp-form weight no larger than the row's recorded largest never reaches the clip
            if form == "RISE" and mag <= mm < 2 ** 32 - 1:
                assert (mag + dth) >> sh <= H.CLIP, (mm, mag)
    assert clipped > 0  # (the random magnitudes above mm do: the clip itself is compared too)


def test_no_exp_weight_up_to_mm_clips_whatever_the_dither():
    # the worst dither word, 2^sh - 1, on the largest weight: (mm + 2^sh - 1) >> sh <= (mm >> sh) + 1 <= 32639
    for mm in _mms()[:-1]:
        sh = H.hw_shift(mm, "RISE")
        for mag in {mm, max(mm - 1, 0)}:
            assert (mag + 2 ** sh - 1) >> sh <= H.CLIP
            assert int(H.clip(np.array([mag]), 2 ** sh - 1, sh)[0]) == (mag + 2 ** sh - 1) >> sh


def test_layouts_of_the_model_invert():
    rng = np.random.default_rng(32)
    # gml_bits.h: sample 32 i + 8 g + 4 h + j sits at byte 32 h + 16 i + 4 g + j
    assert np.array_equal(H.VQ_SAMPLE[H.VQ_POS], np.arange(64))
    assert H.VQ_POS.tolist() == [32 * ((s >> 2) & 1) + 16 * (s >> 5) + 4 * ((s >> 3) & 3) + (s & 3) for s in range(64)]
    cfg = H.compact_configs(1536, 3)
    assert cfg[0] == 0 and cfg[511] == 511 and cfg[512] == 1536 and cfg[1535] == 2 * 1536 + 511 and len(set(cfg.tolist())) == 1536
    assert np.array_equal(H.compact_configs(1024, 1), np.arange(1024))
    h2 = rng.integers(0, H.CLIP + 1, size=1024)
    planes = H.hq_encode(h2)
    hq = np.zeros((2, H.HL, 32, 2048), dtype=np.int8)
    hq[1, :, 7, :1024] = planes
    assert np.array_equal(H.hq_decode(hq, 39, 1024), h2)
    # byte p of a 64-sample piece holds the sample vq_sample(p)
    one = np.zeros(64, dtype=np.int64)
    one[R.vq_sample(5)] = 77
    assert H.hq_encode(one)[0, 5] == 77
    # T and the finish on a block small enough to do by hand: two entries, three samples
    bits = np.array([[1, 0, 1], [1, 1, 0]], dtype=np.uint8)
    T = H.t_block(np.array([3, 5, 7]), bits)
    assert T.tolist() == [[10, 3], [3, 8]]
    Hd = H.finish(T, 15, 0.5, 1.0, 2)
    x = 1.0 - 2.0 * bits
    assert np.array_equal(Hd, 2.0 * (x * np.array([3.0, 5.0, 7.0])) @ x.T)
    assert H.lower_tiles(64)[31, 0] and H.lower_tiles(64)[0, 31] and not H.lower_tiles(64)[0, 32] and H.lower_tiles(64)[32, 0]


def test_mb_is_the_row_major_twin_of_xtb():
    rng = np.random.default_rng(33)
    n, K, Kp = 70, 100, 1024
    spins = rng.choice(np.array([-1, 1], dtype=np.int8), size=(K, n))
    B = R.stat_bits(spins, R.stat_keys(n, 2), 128, Kp)
    mb = H.mb_image(B, Kp, 128, 192)
    assert mb.shape == (192, 16, 2) and not mb[128:].any()
    xtb = R.xtb_image(B, Kp, 128)
    for c, kt, h in ((0, 0, 0), (69, 1, 1), (127, 15, 0), (64, 3, 1)):
        assert mb[c, kt, h] == xtb[(((c >> 7) * 16 + kt) * 128 + (c & 127)) * 2 + h]
    # a bit of Mb: sample 64 kt + vq_sample(xb_col(j, h)) of column c
    for c, k in ((3, 0), (69, 99), (12, 64)):
        kt, pos = k // 64, int(H.VQ_POS[k % 64])
        h = (pos >> 4) & 1
        j = [R.xb_col(b, h) for b in range(32)].index(pos)
        assert (int(mb[c, kt, h]) >> j) & 1 == B[c, k]
