"""The forward sweep of the i8w pass on signed column pairs (csrc/gml_i8_pairs.h): k_quant_theta<7> writes the digit planes of
(q + q', q - q') per column pair, k_fwd_i8w multiplies them with the 2:4 structured-sparse int8 MFMA -- one instruction per
64-column step where the dense sweep issues two -- and a tile in which a pair leaves the range of seven digits keeps plain planes
and the dense sweep.  Every sum is the same integer and the fold rounds once, so the two paths must produce THE SAME BITS: f
(RPLE's, an FP64 sum added with atomics, to 1e-13), G, the raw planes of V and the per-slot sums.  GML_TUNE_NO_PAIRS (knob 9 of
gml_test_tune) forces every tile dense, so one process runs both.  The paired results are also held to the oracle at the 1e-12 of
tests/test_gpu_parity.py.

Shapes: 64 / 128 / 192 columns (one step, the ring's fill, an odd step count) x K = 256 / 300 (padding samples) / 512 x uniform and
weighted counts (1 + k mod 3), each with 32 rows (one full tile) and 40 (a tile with inactive rows); RISE, logRISE (objective only)
and RPLE; a compacted pass and the same rows swept over all columns; an all-zero Theta; a tile in which one row holds the two
largest representable entries in paired columns (alpha = 2^55 - 4 overflows seven digits: that tile must run dense); 33 153
columns (the wide fold; RPLE keeps its two dense sweeps there)."""
import ctypes as C

import numpy as np
import pytest

import gml_amd as gml
from oracle import oracle as O

pytestmark = pytest.mark.gpu
NO_COMPACT, NO_PAIRS = 6, 9  # gml_solver.h: GML_TUNE_NO_COMPACT, GML_TUNE_NO_PAIRS
FTOL = GTOL = 1e-12


def _lib():
    L = gml._lib.lib()
    L.gml_test_i8_pass_state.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
    L.gml_test_tune.restype = C.c_double
    L.gml_test_tune.argtypes = [C.c_int, C.c_double]
    return L


def _state(p):
    """the raw V planes and the per-slot sums of the handle's last i8w pass"""
    L = _lib()
    ns, npl, kp = C.c_int64(), C.c_int(), C.c_int64()
    assert L.gml_test_i8_pass_state(p._h, C.byref(ns), C.byref(npl), C.byref(kp), None, None) == 0
    vq = np.zeros(ns.value * npl.value * kp.value, np.int8)
    sums = np.zeros((5, ns.value), np.int64)
    assert L.gml_test_i8_pass_state(p._h, C.byref(ns), C.byref(npl), C.byref(kp), vq.ctypes.data, sums.ctypes.data) == 0
    return vq, sums


def _both(p, form, nodes, th, want_grad=True):
    """one pass on column pairs and one with every tile forced dense: (f, g, vq, sums) of each"""
    L = _lib()
    out = []
    for dense in (0, 1):
        L.gml_test_tune(NO_PAIRS, dense)
        try:
            f, g = p.objgrad(form, nodes, th, precision="i8w", want_grad=want_grad)
        finally:
            L.gml_test_tune(NO_PAIRS, 0)
        out.append((f, g) + _state(p))
    return out


def _same_bits(a, b, form, what):
    for x, y, name in zip(a, b, ("f", "g", "vq", "sums")):
        if x is None and y is None:
            continue
        assert x.shape == y.shape and x.dtype == y.dtype, (what, name)
        if name == "f" and form == "RPLE":  # the kernel's FP64 sum, added with atomics in no fixed order
            assert np.abs(x / y - 1).max() <= 1e-13, (what, name)
            continue
        # bits, not values: -0.0 against 0.0 or two NaNs would not pass
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, name, int((x != y).sum()))


def _hist(n, K, weighted, seed):
    rng = np.random.default_rng(seed)
    spins = rng.choice(np.array([-1.0, 1.0]), size=(K, n))
    counts = 1.0 + (np.arange(K) % 3) if weighted else np.ones(K)
    return np.concatenate([counts[:, None], spins], axis=1)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [256, 300, 512])
@pytest.mark.parametrize("n", [64, 128, 192])
def test_pairs_match_dense_and_oracle(n, K, weighted):
    s = _hist(n, K, weighted, seed=n + K)
    rng = np.random.default_rng(11)
    with gml.Problem(s) as p:
        for rows in (32, 40):
            nodes = np.arange(rows, dtype=np.int64)
            th = rng.normal(scale=0.05, size=(rows, p.P))
            for form, want_grad in (("RISE", True), ("logRISE", False), ("RPLE", True)):
                pairs, dense = _both(p, form, nodes, th, want_grad)
                _same_bits(pairs, dense, form, (rows, form))
                assert np.count_nonzero(pairs[2]) > 0  # (the passes produced planes)
                for r in (0, rows - 1):  # against the oracle: the first row and the last (in the partly filled tile when rows = 40)
                    f0, g0 = O.objgrad_pair(s, form, int(nodes[r]), th[r])
                    assert pairs[0][r] == pytest.approx(f0, rel=FTOL, abs=FTOL)
                    if want_grad:
                        np.testing.assert_allclose(pairs[1][r], g0, rtol=1e-10, atol=GTOL)


def test_pairs_compacted_and_zero_theta():
    """Compaction pairs neighbours of the tile's compact column list (padded with zero columns); the same rows swept over all columns
    pair other columns; every row zero sweeps nothing."""
    n, K = 256, 512
    s = _hist(n, K, False, seed=5)
    rng = np.random.default_rng(12)
    L = _lib()
    with gml.Problem(s) as p:
        nodes = np.arange(64, dtype=np.int64)
        th = np.zeros((64, p.P))
        cols = rng.choice(np.arange(64, n), size=40, replace=False)  # 40 columns for the whole tile: one compact step, 24 padded
        for r in range(64):
            th[r, cols] = rng.normal(scale=0.2, size=len(cols))
        res = {}
        for nocompact in (0, 1):
            L.gml_test_tune(NO_COMPACT, nocompact)
            try:
                pairs, dense = _both(p, "RISE", nodes, th)
            finally:
                L.gml_test_tune(NO_COMPACT, 0)
            _same_bits(pairs, dense, "RISE", ("compact", nocompact))
            res[nocompact] = pairs
        _same_bits(res[0][:2], res[1][:2], "RISE", "compacted against all columns")
        f0, g0 = O.objgrad_pair(s, "RISE", 3, th[3])
        assert res[0][0][3] == pytest.approx(f0, rel=FTOL, abs=FTOL)
        np.testing.assert_allclose(res[0][1][3], g0, rtol=1e-10, atol=GTOL)
        for form in ("RISE", "RPLE"):
            pairs, dense = _both(p, form, nodes, np.zeros((64, p.P)))
            _same_bits(pairs, dense, form, ("zero", form))


def test_pair_outside_seven_digits_runs_its_tile_dense():
    """Row 10 holds 2^-3 (1 - 2^-53) twice, in columns 0 and 4 -- pair 0 of lane half 0 of the first step (gml_bits.h: xb_col(0, 0) = 0,
    xb_col(1, 0) = 4; a pairwise row's column i is spin i).  Both quantise to 2^54 - 2, their sum leaves the seven digits: the
    first tile keeps plain planes, the second runs on pairs, and nothing may change."""
    n, K = 128, 256
    s = _hist(n, K, True, seed=6)
    rng = np.random.default_rng(13)
    with gml.Problem(s) as p:
        nodes = np.arange(64, dtype=np.int64)
        th = rng.normal(scale=0.001, size=(64, p.P))
        big = np.nextafter(0.125, 0.0)
        assert big == 0.125 * (1 - 2.0 ** -53)
        th[10, 0] = th[10, 4] = big
        for form in ("RISE", "RPLE"):
            pairs, dense = _both(p, form, nodes, th)
            _same_bits(pairs, dense, form, ("outside", form))
            for r in (10, 11, 40):
                f0, g0 = O.objgrad_pair(s, form, r, th[r])
                assert pairs[0][r] == pytest.approx(f0, rel=FTOL, abs=FTOL)
                np.testing.assert_allclose(pairs[1][r], g0, rtol=1e-10, atol=GTOL)


def test_pairs_wide():
    """order 3, n = 258: 257 + 257 * 256 / 2 = 33153 statistics columns (> 32768: the wide fold in FP64; RPLE keeps two dense sweeps)"""
    n, K = 258, 1024
    rng = np.random.default_rng(7)
    spins = rng.choice(np.array([-1, 1], dtype=np.int8), size=(K, n))
    with gml.Problem(spins=spins, order=3) as p:
        nodes = np.arange(64, dtype=np.int64)
        th = rng.normal(scale=0.0005, size=(len(nodes), p.P))  # (sum |theta| about 13: inside the planes' range)
        for form in ("RISE", "RPLE"):
            pairs, dense = _both(p, form, nodes, th)
            _same_bits(pairs, dense, form, ("wide", form))
            assert np.count_nonzero(pairs[2]) > 0 and np.abs(pairs[1]).max() > 0
