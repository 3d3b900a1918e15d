"""The model of a handle's resident state (tests/_ingest_reference.py) against the host side of ingest -- no GPU needed:
the sum of counts M in its one defined order against gml_pack_histogram, the condition that makes the GPU tests of route equality
meaningful (the chosen fractional counts DO tell the summation orders apart), the model's own summaries and refusals on cases small
enough to state by hand, and the sub-range form of the packer (tests/native/pack_ranges.cpp) under the host sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import gml_amd as gml
from gml_amd import _lib
from conftest import ROOT

import _ingest_reference as R

CSRC = os.path.join(ROOT, "graphicalmodellearning.jl_amd", "csrc")


def _hist(counts, dtype, order, seed=0):
    K = len(counts)
    h = np.empty((K, 2), dtype=dtype, order=order)
    h[:, 0] = counts
    h[:, 1] = np.random.default_rng(seed).choice(np.array([-1, 1]), size=K)
    return h


COUNT_KINDS = {
    "integer": (np.int64, lambda K: np.random.default_rng(K).integers(0, 50, size=K) + (np.arange(K) == 0)),
    "fractional": (np.float64, lambda K: R.fractional_counts(K, 1)),
    "uniform": (np.float64, lambda K: np.full(K, 0.3)),
    # sums beyond 2^53: integers, yet every addition rounds -- the order shows here too
    "huge": (np.int64, lambda K: np.random.default_rng(K).integers(2 ** 31, 2 ** 45, size=K)),
}


@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("kind", list(COUNT_KINDS))
@pytest.mark.parametrize("K", [1, 65536, 65537, 70001, 131073])
def test_model_M_and_counts_equal_gml_pack_histogram(K, kind, order):
    dtype, make = COUNT_KINDS[kind]
    counts = make(K)
    h = _hist(counts, dtype, order)
    bits, cnt, M = _lib.pack_histogram(h)
    want = counts.astype(np.float64)
    assert np.array_equal(cnt.view(np.uint64), want.view(np.uint64))
    assert np.float64(M).view(np.uint64) == np.float64(R.blocked_sum(want)).view(np.uint64)
    assert np.array_equal(bits, R.numpy_pack(h[:, 1:]))


@pytest.mark.parametrize("kind", list(R.ORDER_TELLING))
def test_the_fractional_cases_of_the_gpu_tests_tell_the_summation_orders_apart(kind):
    """on the model alone: were blocked and plain sums equal for these counts, the GPU tests of route equality would pass whatever
    order a route summed in"""
    c = R.order_telling_counts(kind)
    blocked, plain = R.blocked_sum(c), R.sum_left_to_right(c)
    assert blocked != plain
    assert abs(blocked - plain) < 1e-12 * plain  # (the two are roundings of one sum)
    # ... and the difference reaches the weights: some w_k = c_k / M differs in its last bits
    assert np.any(c / blocked != c / plain)


def test_one_block_and_one_block_plus_one_are_plain_sums():
    """why K = 65 536 and 65 537 are not among the order-telling cases"""
    for K in (65536, 65537):
        c = R.fractional_counts(K, 1)
        assert R.blocked_sum(c) == R.sum_left_to_right(c)


def test_model_summaries_on_a_case_stated_by_hand():
    spins = np.array([[1, -1], [-1, -1], [1, 1]])
    st = R.handle_state(np.array([1.0, 2.0, 5.0]), spins)
    assert st["M"] == 8.0 and st["counts_int"] and st["wuni"] == 0.0 and st["wmax"] == 0.625
    assert st["w"].shape == (1024,) and np.array_equal(st["w"][:4], [0.125, 0.25, 0.625, 0.0]) and not st["w"][3:].any()
    assert st["wblk"].shape == (2,) and st["wblk"][0] == 1.0 and st["wblk"][1] == 0.0
    assert st["Sb"].shape == (2, 32) and st["Sb"][0, 0] == 0b010 and st["Sb"][1, 0] == 0b011 and not st["Sb"][:, 1:].any()
    st = R.handle_state(None, spins)
    assert st["M"] == 3.0 and st["counts_int"] and st["wuni"] == 1.0 / 3.0 == st["wmax"]
    st = R.handle_state(np.full(3, 0.3), spins)
    assert not st["counts_int"] and st["wuni"] == 0.3 / (0.3 + 0.3 + 0.3) and st["wuni"] != 0.0
    # wblk: row 512 opens the second block
    st = R.handle_state(np.arange(1.0, 514.0), np.ones((513, 1), dtype=np.int64))
    assert st["wblk"][1] == st["w"][512] and st["wblk"][0] == R.sum_left_to_right(st["w"][:512])


def test_model_refusals_follow_the_precedence_of_gml_pack_histogram():
    """the host packer is the one route a CPU box can run: the model's code and text must be what it answers"""
    K, n = 45, 6  # K % 32 != 0: bad rows in the scalar tail
    rng = np.random.default_rng(2)
    base = np.concatenate([rng.integers(1, 9, size=(K, 1)), rng.choice(np.array([-1, 1]), size=(K, n))], axis=1).astype(np.float64)

    def answer(h):
        try:
            _lib.pack_histogram(h)
        except gml.GMLError as e:
            return e.code, str(e).split(": ", 1)[1]
        return None

    cases = []
    for order in ("C", "F"):
        h = np.array(base, order=order)
        cases.append(h.copy(order=order))  # accepted
        for k, j, v in ((0, 1, 0.0), (K - 1, n, 2.0), (40, 2, np.nan)):
            g = h.copy(order=order)
            g[k, j] = v
            cases.append(g)
        g = h.copy(order=order)
        g[40, 2] = 0.0
        g[33, 5] = -0.0  # the later column holds the earlier row
        cases.append(g)
        g = h.copy(order=order)
        g[10, 0] = -1.0
        g[5, 3] = 0.5  # a bad count at row 10 beats a bad spin at row 5
        cases.append(g)
        g = h.copy(order=order)
        g[:, 0] = 0.0
        g[5, 3] = 0.5  # all-zero counts beat a bad spin
        cases.append(g)
        g = h.copy(order=order)
        g[7, 0] = -0.0  # accepted
        cases.append(g)
    for h in cases:
        assert answer(h) == R.refusal(h)
    assert R.refusal(cases[0]) is None and R.refusal(cases[4]) == (1, "configuration 33 holds a spin that is not +-1")
    assert R.refusal(cases[5]) == (1, "count of configuration 10 is negative or not finite")
    assert R.refusal(cases[6]) == (1, "sum of counts is zero")
    assert R.refusal(base, K=0) == (1, "empty histogram (K=0, n=6)")
    assert R.refusal(base, dtype=9) == (1, "unknown dtype 9")
    assert R.refusal(base, ld=n) == (1, f"leading dimension {n} too small")
    assert R.refusal(np.asfortranarray(base), ld=K - 1) == (1, f"leading dimension {K - 1} too small")


def test_pack_ranges_under_the_host_sanitizers(tmp_path):
    """pack_spins over sub-ranges of spins -- what every stage of the ingest pipeline calls -- on exactly sized buffers, under
    AddressSanitizer and UndefinedBehaviorSanitizer.  A stand-alone host program: nothing is preloaded, no device is touched."""
    exe = str(tmp_path / "pack_ranges")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "native", "pack_ranges.cpp"),
                           os.path.join(CSRC, "gml_pack.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-4000:]
