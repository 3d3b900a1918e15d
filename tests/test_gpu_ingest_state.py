"""Every route into a handle leaves ONE resident state, and it is the model's (tests/_ingest_reference.py): the sign bits Sb, the
weights w as they sit in HBM, M, and the host-side summaries wmax, wuni, counts_int and wblk that select the uniform-weight kernels,
the quantisation bounds, the exact-moments contract and the sub-sampled Hessian weights.  All comparisons are bit for bit (doubles as
uint64 views), so the routes equal one another because each equals the model.  The routes:
    create         gml_problem_create (host packer, bits uploaded)
    device         gml_problem_create_device_convert (raw upload, converted on the device)
    spins          gml_problem_create_spins
    packed_hist    gml_problem_create_packed of gml_pack_histogram's output
    packed_handle  gml_problem_create_packed of another handle's sign_bits() and counts()
Faulty inputs are answered with one code and one text on both matrix routes: refusal() of the model."""
import ctypes as C

import numpy as np
import pytest

from gml_amd import _lib

import _ingest_reference as R

pytestmark = pytest.mark.gpu

DTYPES = [np.int8, np.int32, np.int64, np.float64]
ROUTES = ["create", "device", "spins", "packed_hist", "packed_handle"]
TUNE_STAGE_SPINS = 11  # csrc/gml_solver.h: GML_TUNE_STAGE_SPINS


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def resident_state(p):
    """what the handle holds: Sb and w from HBM, the summaries from the host side (gml_test_weight_state: copies only)"""
    L = _lib.lib()
    L.gml_test_weight_state.argtypes = [C.c_void_p] * 4
    Kp = (p.K + 1023) // 1024 * 1024
    w, summary, wblk = np.full(Kp, np.nan), np.full(4, np.nan), np.full(Kp // 512, np.nan)
    _lib.check(L.gml_test_weight_state(p._h, _lib._ptr(w), _lib._ptr(summary), _lib._ptr(wblk)))
    assert p.M == summary[0]
    return {"Sb": p.sign_bits(), "w": w, "M": summary[0], "wmax": summary[1], "wuni": summary[2], "counts_int": bool(summary[3]),
            "wblk": wblk}


def assert_state(p, want, what=""):
    got = resident_state(p)
    assert got["Sb"].shape == want["Sb"].shape and np.array_equal(got["Sb"], want["Sb"]), f"{what}: Sb"
    for key in ("M", "wmax", "wuni"):
        assert u64(got[key]) == u64(want[key]), f"{what}: {key} = {got[key]!r}, model {want[key]!r}"
    assert got["counts_int"] == want["counts_int"], f"{what}: counts_int"
    for key in ("w", "wblk"):
        assert got[key].shape == want[key].shape, f"{what}: {key} shape"
        d = np.flatnonzero(u64(got[key]) != u64(want[key]))
        assert len(d) == 0, f"{what}: {key} differs in {len(d)} entries, first at {d[0]}: {got[key][d[0]]!r}, model {want[key][d[0]]!r}"


def matrix(counts, spins, dtype, order):
    h = np.empty((spins.shape[0], spins.shape[1] + 1), dtype=dtype, order=order)
    h[:, 0] = counts
    h[:, 1:] = spins
    assert np.array_equal(h[:, 0].astype(np.float64), counts)  # the dtype holds these counts
    return h


def open_route(route, counts, spins, dtype=np.float64, order="F"):
    """(handle, the counts this route was given): the last route reads its counts back from another handle"""
    if route in ("create", "device"):
        return _lib.Problem(matrix(counts, spins, dtype, order), ingest={"create": "host", "device": "device"}[route]), counts
    if route == "spins":
        return _lib.Problem(counts=counts, spins=spins.astype(np.int8)), counts
    if route == "packed_hist":
        bits, cnt, _ = _lib.pack_histogram(matrix(counts, spins, dtype, order))
        return _lib.Problem(packed=(bits, cnt, len(cnt))), counts
    with _lib.Problem(matrix(counts, spins, dtype, order)) as a:
        bits, cnt = a.sign_bits(), a.counts()
    return _lib.Problem(packed=(bits, cnt, len(cnt))), cnt


def random_spins(K, n, seed):
    return np.random.default_rng(seed).choice(np.array([-1, 1], dtype=np.int64), size=(K, n))


def small_counts(K, seed):
    c = np.random.default_rng(seed).integers(0, 50, size=K).astype(np.float64)
    c[0] = 7.0
    return c


# K around the word (32) and the padding unit (1024); n around the 32-column groups of the row-major packer and above 64
SMALL_SHAPES = [(1, 1), (1, 70), (31, 3), (32, 33), (33, 1), (33, 64), (1023, 70), (1024, 3), (1025, 33), (1025, 64)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("K,n", SMALL_SHAPES)
def test_matrix_routes_hold_the_models_state(K, n, order, dtype):
    spins, counts = random_spins(K, n, K + n), small_counts(K, K)
    want = R.handle_state(counts, spins)
    for route in ("create", "device"):
        p, _ = open_route(route, counts, spins, dtype, order)
        with p:
            assert_state(p, want, route)
            assert np.array_equal(p.spins(), spins)


@pytest.mark.parametrize("K,n", SMALL_SHAPES)
def test_split_input_and_packed_routes_hold_the_models_state(K, n):
    spins, counts = random_spins(K, n, K + n), small_counts(K, K)
    want = R.handle_state(counts, spins)
    for route in ("spins", "packed_hist", "packed_handle"):
        p, given = open_route(route, counts, spins)
        with p:
            assert np.array_equal(given, counts)
            assert_state(p, want, route)
    # no counts at all: every row counts once
    want = R.handle_state(None, spins)
    bits = R.numpy_pack(spins)
    with _lib.Problem(spins=spins.astype(np.int8)) as p, _lib.Problem(packed=(bits, None, K)) as q:
        assert_state(p, want, "spins, counts NULL")
        assert_state(q, want, "packed, counts NULL")
    # bits beyond K in the caller's words belong to padding configurations: they do not reach the handle
    dirty = bits.copy()
    if K % 32:
        dirty[:, K // 32] |= np.uint32((0xFFFFFFFF << (K % 32)) & 0xFFFFFFFF)
    dirty[:, (K + 31) // 32:] = 0xFFFFFFFF
    with _lib.Problem(packed=(dirty, None, K)) as q:
        assert_state(q, want, "packed, dirty tail")


KINDS = list(R.count_kinds(4))
FRACTIONAL_KINDS = ("uniform_0.3", "fractional")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", [65536, 65537, 70001])
def test_every_route_holds_the_models_weights(K, kind):
    """K beyond one block of the sum of counts: M, and with it every w_k, depends on the order a route sums in (fractional kinds at
    K = 70 001; tests/test_host_ingest_reference.py shows on the model alone that these counts tell the orders apart)"""
    n = 3
    counts = R.count_kinds(K)[kind]
    if K == 70001 and kind == "fractional":
        counts = R.order_telling_counts("random")
    if K == 70001 and kind == "uniform_0.3":
        counts = R.order_telling_counts("uniform")
    spins = random_spins(K, n, K)
    dtype = np.float64 if kind in FRACTIONAL_KINDS else np.int64
    want = R.handle_state(counts, spins)
    assert want["counts_int"] == (kind not in FRACTIONAL_KINDS)
    assert (want["wuni"] != 0.0) == bool(np.all(counts == counts[0]))
    if kind in ("ones", "threes", "uniform_0.3"):  # (M_2^50 is uniform too where K divides 2^50)
        assert want["wuni"] != 0.0
    if kind == "M_2^50":
        assert want["M"] == 2.0 ** 50
    for route in ROUTES:
        p, given = open_route(route, counts, spins, dtype, "F" if route != "device" else "C")
        with p:
            if route == "packed_handle" and kind in FRACTIONAL_KINDS:
                # gml_problem_get_counts rounds fractional counts to 1e-6: this route was GIVEN other counts -- the model of those
                assert_state(p, R.handle_state(given, spins), route)
            else:
                assert np.array_equal(given, counts)
                assert_state(p, want, route)


def padded(h, col_major):
    """(buffer of exactly the extent the interface allows, ld): ld = K + 5 column-major, n + 1 + 4 row-major; the padding holds NaN
    (float64) or 7 (integers) -- never a legal spin, never a legal count"""
    K, n1 = h.shape
    pad = np.nan if h.dtype == np.float64 else 7
    if col_major:
        ld = K + 5
        buf = np.full(ld * (n1 - 1) + K, pad, dtype=h.dtype)
        for j in range(n1):
            buf[j * ld:j * ld + K] = h[:, j]
    else:
        ld = n1 + 4
        full = np.full((K, ld), pad, dtype=h.dtype)
        full[:, :n1] = h
        buf = full.ravel()[:(K - 1) * ld + n1].copy()
    return buf, ld


def raw_create(route, buf, dt, K, n, ld, col_major):
    """the C call itself: ((code, text), None) of a refusal, or (None, Problem)"""
    L = _lib.lib()
    fn = {"create": L.gml_problem_create, "device": L.gml_problem_create_device_convert}[route]
    h = C.c_void_p()
    rc = fn(_lib._ptr(buf), int(dt), int(K), int(n), int(ld), int(col_major), 2, 0, max(int(n), 1), 0, C.byref(h))
    if rc != _lib.GML_OK:
        assert not h.value
        return (rc, L.gml_last_error().decode()), None
    return None, _lib.Problem._from_handle(h, 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("col_major", [0, 1])
@pytest.mark.parametrize("K,n", [(33, 3), (1025, 33), (70001, 3)])
def test_padded_leading_dimensions_give_the_tight_state(K, n, col_major, dtype):
    spins, counts = random_spins(K, n, K + n), small_counts(K, K)
    want = R.handle_state(counts, spins)
    buf, ld = padded(matrix(counts, spins, dtype, "C"), col_major)
    for route in ("create", "device"):
        refused, p = raw_create(route, buf, R.DTYPE_IDS[np.dtype(dtype)], K, n, ld, col_major)
        assert refused is None, f"{route}: the padding was taken for an entry: {refused}"
        with p:
            assert_state(p, want, route)


_STAGED = {}


def staged_case():
    if not _STAGED:
        K, n = 70001, 70
        spins = random_spins(K, n, 5)
        _STAGED.update(spins=spins, counts=small_counts(K, 6), want=None)
        _STAGED["want"] = R.handle_state(_STAGED["counts"], spins)
    return _STAGED


@pytest.mark.parametrize("dtype", [np.int8, np.float64])
@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("cap,chunks", [(5, 14), (32, 3), (33, 3)])
def test_staged_fill_in_many_chunks(cap, chunks, order, dtype):
    """fill_sign_bits with its stage capped at 5, 32 and 33 spins (14, 3 and 3 chunks of the 70 spins; fewer than 32 spins per chunk,
    whole 32-column groups, and a group cut by the chunk end).  This holds the offsets of the chunks in Sb and the per-range fill of
    the packer.  It does NOT hold the event waits that keep a stage from being refilled while its copy is in flight: at this size a
    missing wait would not show."""
    c = staged_case()
    assert -(-c["spins"].shape[1] // cap) == chunks
    h = matrix(c["counts"], c["spins"], dtype, order)
    L = _lib.lib()
    L.gml_test_tune.restype = C.c_double
    L.gml_test_tune.argtypes = [C.c_int, C.c_double]
    L.gml_test_fill_chunks.restype = C.c_longlong
    with _lib.Problem(h) as p:  # the knob is off by default: the 70 spins fit one stage
        assert L.gml_test_fill_chunks() == 1
    assert L.gml_test_tune(TUNE_STAGE_SPINS, float(cap)) == 0.0
    try:
        with _lib.Problem(h) as p:
            assert L.gml_test_fill_chunks() == chunks  # (the count fill_sign_bits itself kept of its stages)
            assert_state(p, c["want"], f"cap {cap}")
        bits, cnt, _ = _lib.pack_histogram(h)
        with _lib.Problem(packed=(bits, cnt, len(cnt))) as p:  # the packed route fills through the same stages
            assert L.gml_test_fill_chunks() == chunks
            assert_state(p, c["want"], f"packed, cap {cap}")
    finally:
        assert L.gml_test_tune(TUNE_STAGE_SPINS, 0.0) == float(cap)


_DOWNSTREAM = {}


def downstream_case():
    """the fractional case of the downstream tests: K = 70 001 counts that tell the summation orders apart, n = 3"""
    if not _DOWNSTREAM:
        counts = R.order_telling_counts("random")
        _DOWNSTREAM.update(counts=counts, spins=random_spins(len(counts), 3, 11), theta=np.random.default_rng(3).normal(scale=0.3, size=(3, 3)))
    return _DOWNSTREAM


# the routes that are GIVEN the case's counts.  packed_handle reads its counts back through gml_problem_get_counts, which rounds
# fractional counts to 1e-6: it is given another input, so it is held to the host route OF THAT INPUT ("create_readback": gml_problem_create
# of the counts packed_handle was given), not to the other four
SAME_INPUT_ROUTES = ["create", "device", "spins", "packed_hist"]


def objgrad_by_route(prec, repeat=1):
    """{route: [(f, g)] * repeat} of the four routes given the case's counts, and of packed_handle and create_readback"""
    c = downstream_case()
    n = c["spins"].shape[1]
    outs = {}

    def run(name, p):
        with p:
            assert p.P == n
            outs[name] = [p.objgrad("RISE", np.arange(n), c["theta"], precision=prec) for _ in range(repeat)]

    for route in SAME_INPUT_ROUTES:
        run(route, open_route(route, c["counts"], c["spins"], np.float64, "C")[0])
    p, given = open_route("packed_handle", c["counts"], c["spins"], np.float64, "C")
    assert not np.array_equal(given, c["counts"]) and np.abs(given - c["counts"]).max() <= 5e-7 + 2.0 ** -50 * c["counts"].max()
    run("packed_handle", p)
    run("create_readback", open_route("create", given, c["spins"], np.float64, "C")[0])
    return outs


def assert_same_bits(outs, names, ref):
    f0, g0 = outs[ref][0]
    assert np.all(np.isfinite(f0)) and np.all(np.isfinite(g0)) and np.abs(g0).max() > 0
    for name in names:
        for f, g in outs[name]:  # (every call on the handle)
            assert np.array_equal(u64(f), u64(f0)) and np.array_equal(u64(g), u64(g0)), (name, ref)


def test_objgrad_i8w_bits_do_not_depend_on_the_route():
    """equal resident state, integer sums in the pass: the same objective and gradient bits from every route"""
    outs = objgrad_by_route("i8w", repeat=2)
    assert_same_bits(outs, SAME_INPUT_ROUTES, "create")
    assert_same_bits(outs, ["packed_handle", "create_readback"], "create_readback")


def test_objgrad_f64_bits_do_not_depend_on_the_route():
    """The same at precision f64, and two calls on one handle.  This test found that the FP64 pass was not reproducible at all: it
    added the parts of f and G of its K / 128 waves with FP64 atomics, in whatever order the waves finished, so that at K = 70 001 a
    second call on ONE handle differed from the first by 3 to 10 ulp in f and 1 to 2 in G, and the routes from one another by as much
    (measured on MI355X with every route holding the model's state bit for bit).  The workgroups now store their parts and a second
    kernel adds them in a fixed order (csrc/gml_kernels_f64gemm.hip: k_fsum_reduce, k_bwd_f64_reduce)."""
    outs = objgrad_by_route("f64", repeat=2)
    f0, g0 = outs["create"][0]

    def ulps(a, b):
        return int(np.abs(u64(a).astype(np.int64) - u64(b).astype(np.int64)).max())

    for route, calls in outs.items():
        print(f"f64 objgrad, {route}: against create, f {ulps(calls[0][0], f0)} ulp, g {ulps(calls[0][1], g0)} ulp; second call on the "
              f"same handle against its first, f {ulps(calls[1][0], calls[0][0])} ulp, g {ulps(calls[1][1], calls[0][1])} ulp")
    assert_same_bits(outs, SAME_INPUT_ROUTES, "create")
    assert_same_bits(outs, ["packed_handle", "create_readback"], "create_readback")


@pytest.mark.parametrize("prec", ["f64", "i8w"])
def test_objgrad_bits_with_two_row_groups_and_four_chunks(prec):
    """n = 40 rows are two 32-row groups, and K = 8 000 gives the FP64 backward GEMM four split-K chunks and its forward sixteen
    workgroups per group: the group terms of the indices of the parts of f and G (csrc/gml_kernels_f64gemm.hip) are held to the same
    bits from two routes and from two calls on each handle, all three formulations."""
    K, n = 8000, 40
    spins, counts = random_spins(K, n, 21), R.fractional_counts(K, 2)
    theta = np.random.default_rng(4).normal(scale=0.05, size=(n, n))
    outs = {}
    for route, order in (("create", "F"), ("device", "C")):
        p, _ = open_route(route, counts, spins, np.float64, order)
        with p:
            outs[route] = [p.objgrad(form, np.arange(n), theta, precision=prec) for form in ("RISE", "logRISE", "RPLE") for _ in range(2)]
    for a, b in ((0, 1), (2, 3), (4, 5)):  # two calls on one handle
        for calls in outs.values():
            assert np.array_equal(u64(calls[a][0]), u64(calls[b][0])) and np.array_equal(u64(calls[a][1]), u64(calls[b][1]))
    for x, y in zip(outs["create"], outs["device"]):  # two routes
        assert np.array_equal(u64(x[0]), u64(y[0])) and np.array_equal(u64(x[1]), u64(y[1]))
    assert np.abs(outs["create"][0][1][33]).max() > 0  # (a row of the second group has a gradient)


def test_exact_moments_are_refused_or_equal_on_every_route():
    c = downstream_case()
    counts, spins = c["counts"], c["spins"]
    K, n = spins.shape
    L = _lib.lib()
    # fractional counts: GML_EUNSUPPORTED on every route (the fifth route's counts, rounded to 1e-6, are fractional too)
    for route in ROUTES:
        p, _ = open_route(route, counts, spins, np.float64, "C")
        with p:
            s1 = np.zeros(n, dtype=np.int64)
            rc = L.gml_problem_moments(p._h, _lib._ptr(s1), None)
            assert rc == _lib.GML_EUNSUPPORTED, route
            assert "fractional count" in L.gml_last_error().decode()
    # integer counts: the exact moments work on every route and are, sum for sum, those of the integers themselves
    counts = R.count_kinds(K)["small_int_with_zeros"]
    ci = counts.astype(np.int64)
    want1 = (ci[:, None] * spins).sum(axis=0)
    want2 = (spins * ci[:, None]).T @ spins
    for route in ROUTES:
        p, _ = open_route(route, counts, spins, np.int64, "F")
        with p:
            s1, s2 = p.moments(raw=True)
            assert np.array_equal(s1, want1) and np.array_equal(s2, want2), route


@pytest.mark.parametrize("K", [1, 33, 70001])
def test_get_counts(K):
    """exact for integer counts up to M = 2^50; fractional counts c come back within 5e-7 + 2^-50 c: the documented rounding to 1e-6
    plus the three roundings of w = c / M, w * M and the scaling by 1e6 (each relative 2^-53)"""
    spins = random_spins(K, 3, K)
    kinds = R.count_kinds(K)
    for kind, counts in kinds.items():
        for route in ("create", "device"):
            p, _ = open_route(route, counts, spins, np.float64 if kind in FRACTIONAL_KINDS else np.int64, "F")
            with p:
                got = p.counts()
            if kind in FRACTIONAL_KINDS:
                err = np.abs(got - counts)
                print(f"get_counts {kind} K={K} {route}: max error {err.max():.3e}")
                assert np.all(err <= 5e-7 + 2.0 ** -50 * counts), (kind, route)
            else:
                assert np.array_equal(u64(got), u64(counts)), (kind, route)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
BAD_SPINS = {
    np.int8: [0, 2, -2, 127, -127, -128],
    np.int32: [0, 2, -2, 257],
    np.int64: [0, 2, -2, 2 ** 32 + 1],
    np.float64: [0.0, 2.0, -2.0, 0.5, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), np.nextafter(-1.0, -2.0), np.nextafter(-1.0, 0.0),
                 -0.0, np.nan, np.inf, -np.inf],
}
RK, RN = 77, 6  # K % 32 != 0: rows 64 .. 76 are packed by the scalar tail


def good_matrix(dtype, order):
    rng = np.random.default_rng(4)
    return matrix(rng.integers(1, 9, size=RK).astype(np.float64), rng.choice(np.array([-1, 1]), size=(RK, RN)), dtype, order)


def assert_refused_alike(h, **override):
    """both matrix routes answer `h` with the model's code and full text; returns it"""
    want = R.refusal(h, **override)
    assert want is not None
    args = dict(K=h.shape[0], n=h.shape[1] - 1, dt=R.DTYPE_IDS[h.dtype], col_major=int(h.flags.f_contiguous and not h.flags.c_contiguous))
    args["ld"] = args["K"] if args["col_major"] else args["n"] + 1
    for key, v in override.items():
        args["dt" if key == "dtype" else key] = v
    for route in ("create", "device"):
        got, p = raw_create(route, h, args["dt"], args["K"], args["n"], args["ld"], args["col_major"])
        if p is not None:
            p.close()
        assert got == want, route
    return want


def assert_device_still_works(dtype, order):
    """a refused call leaves nothing behind: the next create on the same device works, on both routes"""
    h = good_matrix(dtype, order)
    want = R.handle_state(h[:, 0].astype(np.float64), h[:, 1:])
    for ingest in ("host", "device"):
        with _lib.Problem(h, ingest=ingest) as p:
            assert_state(p, want, ingest)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ["C", "F"])
def test_bad_spins_are_refused_alike(dtype, order):
    base = good_matrix(dtype, order)
    for v in BAD_SPINS[dtype]:
        h = base.copy(order=order)
        h[70, 4] = v
        assert assert_refused_alike(h) == (1, "configuration 70 holds a spin that is not +-1"), v
    # positions: the first row, row K - 1 (the scalar tail), the last column, and two bad entries where the later column holds the
    # earlier row
    for entries, first in (([(0, 1)], 0), ([(RK - 1, 3)], RK - 1), ([(40, RN)], 40), ([(RK - 1, RN)], RK - 1), ([(70, 2), (66, 5)], 66),
                           ([(50, 1), (3, RN)], 3)):
        h = base.copy(order=order)
        for k, j in entries:
            h[k, j] = 0
        assert assert_refused_alike(h) == (1, f"configuration {first} holds a spin that is not +-1")
    assert_device_still_works(dtype, order)


@pytest.mark.parametrize("order", ["C", "F"])
def test_bad_counts_are_refused_alike_and_before_bad_spins(order):
    base = good_matrix(np.float64, order)
    for v in (-1.0, np.nan, np.inf):
        h = base.copy(order=order)
        h[10, 0] = v
        assert assert_refused_alike(h) == (1, "count of configuration 10 is negative or not finite")
        h[5, 3] = 0.5  # a bad spin at an earlier row: the count is reported
        assert assert_refused_alike(h) == (1, "count of configuration 10 is negative or not finite")
    h = base.copy(order=order)
    h[:, 0] = 0.0
    assert assert_refused_alike(h) == (1, "sum of counts is zero")
    h[5, 3] = 0.5
    assert assert_refused_alike(h) == (1, "sum of counts is zero")
    for dtype in (np.int8, np.int32, np.int64):
        h = good_matrix(dtype, order)
        h[10, 0] = -1
        h[5, 3] = 0
        assert assert_refused_alike(h) == (1, "count of configuration 10 is negative or not finite")
    # -0.0 is a count of zero
    h = base.copy(order=order)
    h[10, 0] = -0.0
    assert R.refusal(h) is None
    want = R.handle_state(h[:, 0].copy(), h[:, 1:])
    for ingest in ("host", "device"):
        with _lib.Problem(h, ingest=ingest) as p:
            assert_state(p, want, ingest)


def test_argument_checks_are_refused_alike():
    for order in ("C", "F"):
        h = good_matrix(np.int64, order)
        assert assert_refused_alike(h, K=0) == (1, f"empty histogram (K=0, n={RN})")
        assert assert_refused_alike(h, n=0) == (1, f"empty histogram (K={RK}, n=0)")
        assert assert_refused_alike(h, dtype=4) == (1, "unknown dtype 4")
        assert assert_refused_alike(h, dtype=-1) == (1, "unknown dtype -1")
        small = (RK if order == "F" else RN + 1) - 1
        assert assert_refused_alike(h, ld=small) == (1, f"leading dimension {small} too small")
        assert_device_still_works(np.int64, order)
