"""The paired step of k_fwd_i8w with its LDS reads pinned ahead of its MFMAs (csrc/gml_kernels_i8w.hip: pstep): the step loop is
unrolled by the ring depth of 4, the ring is entered at a stage that depends on the step count, the steps that issue no stage are
peeled, and the fragments, the bit dwords and the DMA destinations are addressed with immediates per stage.  What can go wrong there
goes wrong at step counts the earlier tests (1 to 3 steps, and 5) do not reach, so this file walks them: against the same pass with
every tile forced dense (GML_TUNE_NO_PAIRS, knob 9 of gml_test_tune) f, G, the raw V planes and the per-slot sums must be THE SAME
BITS (RPLE's f, an FP64 sum added with atomics in no fixed order, to 1e-13), and two rows per case are held to the oracle at the
1e-12 of tests/test_gpu_i8w_pairs.py.

Shapes.  Columns n = 64 nk, nk = 1 .. 9 and 11: fewer steps than the ring's prologue of 3 (1, 2), none, one, two and three odd issuing
steps in front of the unrolled loop (nk = 3, 4, 5, 6), one full turn of the ring (7), a turn behind an odd step or two (8, 9), two
turns (11).  K = 256 / 300 / 768: one sample tile, padding samples, three tiles.  32 rows and 40
(a tile with inactive rows), uniform and weighted (1 + k mod 3) counts; RISE with the gradient, logRISE objective only, RPLE.  A
launch in which the middle tile of three must run dense between paired neighbours (its row 10 holds a pair outside seven digits); an
all-zero Theta; compacted passes whose tiles sweep different step counts.

On the compacted case: the library compacts a tile only while its column list fits a quarter of the columns (gml_i8_pass.hip), 2 steps
of the 9 at n = 576, so there lists of 1, 2 and 5 steps run as 1, 2 and all 9 steps; the same lists at n = 1280 (capacity 5) run as
1, 2 and 5 compact steps.  Both are held to the same rows swept over all columns."""
import ctypes as C

import numpy as np
import pytest

import gml_amd as gml
from oracle import oracle as O

pytestmark = pytest.mark.gpu
NO_COMPACT, NO_PAIRS = 6, 9  # gml_solver.h: GML_TUNE_NO_COMPACT, GML_TUNE_NO_PAIRS
FTOL = GTOL = 1e-12
FORMS = (("RISE", True), ("logRISE", False), ("RPLE", True))


def _lib():
    L = gml._lib.lib()
    L.gml_test_i8_pass_state.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
    L.gml_test_i8_pack_state.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
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


def _marks(p, ntiles):
    """what the handle's last objective pass left per node tile: (tdense -- 0 = swept on pairs, 1 = dense --, compact steps or -1)"""
    L = _lib()
    d = np.zeros(20, dtype=np.int64)
    assert L.gml_test_i8_pack_state(p._h, 0, d.ctypes.data, None) == 0
    nt = int(d[0]) // 32
    tdense, cnk = np.full(nt, -7, dtype=np.int32), np.full(nt, -7, dtype=np.int32)
    ptrs = (C.c_void_p * 13)()
    ptrs[1], ptrs[2] = tdense.ctypes.data, cnk.ctypes.data
    assert L.gml_test_i8_pack_state(p._h, 0, d.ctypes.data, ptrs) == 0
    return tdense[:ntiles].tolist(), cnk[:ntiles].tolist()


def _both(p, form, nodes, th, want_grad=True):
    """one pass on column pairs and one with every tile forced dense: (f, g, vq, sums) of each, and the marks of the paired pass"""
    L = _lib()
    out, marks = [], None
    for dense in (0, 1):
        L.gml_test_tune(NO_PAIRS, dense)
        try:
            f, g = p.objgrad(form, nodes, th, precision="i8w", want_grad=want_grad)
        finally:
            L.gml_test_tune(NO_PAIRS, 0)
        out.append((f, g) + _state(p))
        if not dense:
            marks = _marks(p, (len(nodes) + 31) // 32)
    return out[0], out[1], marks


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


def _oracle_rows(s, form, nodes, th, got, rows, want_grad=True):
    for r in rows:
        f0, g0 = O.objgrad_pair(s, form, int(nodes[r]), th[r])
        assert got[0][r] == pytest.approx(f0, rel=FTOL, abs=FTOL), (form, r)
        if want_grad:
            np.testing.assert_allclose(got[1][r], g0, rtol=1e-10, atol=GTOL)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [256, 300, 768])
@pytest.mark.parametrize("nk", [1, 2, 3, 4, 5, 6, 7, 8, 9, 11])
def test_every_step_count_matches_dense_and_oracle(nk, K, weighted):
    n = 64 * nk
    s = _hist(n, K, weighted, seed=1000 * nk + K)
    rng = np.random.default_rng(19)
    with gml.Problem(s) as p:
        for rows in (32, 40):
            nodes = np.arange(rows, dtype=np.int64)
            th = rng.normal(scale=0.05, size=(rows, p.P))
            for form, want_grad in FORMS:
                pairs, dense, (tdense, _) = _both(p, form, nodes, th, want_grad)
                assert tdense == [0] * len(tdense), (rows, form, tdense)  # (every tile took the paired sweep)
                _same_bits(pairs, dense, form, (nk, rows, form))
                assert np.count_nonzero(pairs[2]) > 0  # (the passes produced planes)
                _oracle_rows(s, form, nodes, th, pairs, (0, rows - 1), want_grad)  # (the last: in the partly filled tile when rows = 40)


def test_dense_tile_between_paired_tiles():
    """96 rows at n = 320 (5 steps).  Row 42 holds 2^-3 (1 - 2^-53) twice, in columns 0 and 4 -- pair 0 of lane half 0 of the first step,
    as in tests/test_gpu_i8w_pairs.py.  Both quantise to 2^54 - 2 and their sum leaves the seven digits: the middle tile keeps plain
    planes and the dense sweep, the tiles on either side of it run on pairs, in one launch, and nothing may change."""
    n, K = 320, 300
    s = _hist(n, K, True, seed=6)
    rng = np.random.default_rng(23)
    with gml.Problem(s) as p:
        nodes = np.arange(96, dtype=np.int64)
        th = rng.normal(scale=0.001, size=(96, p.P))
        big = np.nextafter(0.125, 0.0)
        assert big == 0.125 * (1 - 2.0 ** -53)
        th[42, 0] = th[42, 4] = big
        for form, want_grad in FORMS:
            pairs, dense, (tdense, _) = _both(p, form, nodes, th, want_grad)
            assert tdense == [0, 1, 0], (form, tdense)
            _same_bits(pairs, dense, form, ("mixed", form))
            _oracle_rows(s, form, nodes, th, pairs, (10, 42, 43, 95), want_grad)


@pytest.mark.parametrize("n,steps", [(576, [1, 2, -1]), (1280, [1, 2, 5])])
def test_compacted_tiles_sweep_different_step_counts(n, steps):
    """Three tiles whose rows are non-zero on 40, 100 and 300 columns: compact lists of 1, 2 and 5 steps (n = 576: the third exceeds
    the capacity of 2 steps and sweeps all 9).  Each against the dense sweep, and the compacted pass against all columns."""
    K = 512
    s = _hist(n, K, False, seed=n)
    rng = np.random.default_rng(29)
    L = _lib()
    with gml.Problem(s) as p:
        nodes = np.arange(96, dtype=np.int64)
        th = np.zeros((96, p.P))
        for t, ncols in enumerate((40, 100, 300)):
            cols = rng.choice(np.arange(96, n), size=ncols, replace=False)  # one list for the whole tile
            for r in range(32 * t, 32 * t + 32):
                th[r, cols] = rng.normal(scale=0.2 / np.sqrt(ncols / 40), size=ncols)
        res = {}
        for nocompact in (0, 1):
            L.gml_test_tune(NO_COMPACT, nocompact)
            try:
                pairs, dense, (tdense, cnk) = _both(p, "RISE", nodes, th)
            finally:
                L.gml_test_tune(NO_COMPACT, 0)
            assert tdense == [0, 0, 0]
            if not nocompact:
                assert cnk == steps, cnk
            _same_bits(pairs, dense, "RISE", ("compact", n, nocompact))
            res[nocompact] = pairs
        _same_bits(res[0][:2], res[1][:2], "RISE", "compacted against all columns")
        _oracle_rows(s, "RISE", nodes, th, res[0], (3, 40, 95))


def test_zero_theta_sweeps_nothing():
    n, K = 320, 300
    s = _hist(n, K, True, seed=8)
    with gml.Problem(s) as p:
        nodes = np.arange(40, dtype=np.int64)
        th = np.zeros((40, p.P))
        for form, want_grad in FORMS:
            pairs, dense, _ = _both(p, form, nodes, th, want_grad)
            _same_bits(pairs, dense, form, ("zero", form))
            _oracle_rows(s, form, nodes, th, pairs, (0, 39), want_grad)
