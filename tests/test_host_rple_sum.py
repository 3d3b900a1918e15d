"""The two-word integer form in which the FP64-grade int8 pass adds up RPLE's objective (gml_kernels_i8w.hip: a wave's part fp goes as
rint(fp 2^32) and the remainder in units of 2^-72), restated in Python integers: the sum does not depend on the order of the parts
and stays within 2^-73 per part of the exact sum."""
import math
from fractions import Fraction

import numpy as np


def two_words(fp):
    hi = int(np.rint(fp * 2.0 ** 32))
    rem = math.fma(-float(hi), 2.0 ** -32, fp) if hasattr(math, "fma") else float(Fraction(fp) - Fraction(hi, 2 ** 32))
    return hi, int(np.rint(rem * 2.0 ** 72))


def put_together(hi, lo):
    return float(lo) * 2.0 ** -72 + float(hi) * 2.0 ** -32


def test_split_is_exact_to_the_last_unit():
    rng = np.random.default_rng(0)
    for fp in np.concatenate([rng.uniform(0, 1e-3, 200), rng.uniform(0, 50, 50), [0.0, 2.0 ** -80, 1.0, 2.0 ** 29]]):
        hi, lo = two_words(float(fp))
        assert abs(lo) <= 2 ** 39 + 1  # the remainder is at most 2^-33
        assert abs(Fraction(hi, 2 ** 32) + Fraction(lo, 2 ** 72) - Fraction(float(fp))) <= Fraction(1, 2 ** 73)


def test_sum_is_order_independent_and_accurate():
    rng = np.random.default_rng(1)
    parts = rng.uniform(0, 2e-4, size=16000)  # 4 waves x 4000 sample tiles of a row
    words = [two_words(float(x)) for x in parts]
    his, los = sum(h for h, _ in words), sum(l for _, l in words)
    perm = rng.permutation(len(words))
    assert (sum(words[i][0] for i in perm), sum(words[i][1] for i in perm)) == (his, los)
    assert abs(los) < 2 ** 62 and abs(his) < 2 ** 62
    exact = sum(Fraction(float(x)) for x in parts)
    got = put_together(his, los)
    assert abs(Fraction(got) - exact) <= Fraction(len(parts), 2 ** 73) + Fraction(math.ulp(got))
    # the order-dependent FP64 sum it replaces wanders by more than that
    a, b = float(np.sum(parts)), float(np.sum(parts[perm]))
    assert abs(Fraction(got) - exact) <= max(abs(Fraction(a) - exact), abs(Fraction(b) - exact)) + Fraction(math.ulp(got))
