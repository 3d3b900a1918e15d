"""Structured learn on the device (gml_learn_structured, gml_structure_from_rows, gml_structure_from_keys; include/gml.h): the two
structure kernels byte for byte against tests/_structure_reference.py, and restricted solves against the CPU oracle -- a row whose
parameters are restricted to a set A is the oracle's own solve on the sub-histogram of the columns [u] + A, with the regulariser
rescaled so that lambda is the full problem's.  Run with -m gpu on an MI355X.

Bounds: the oracle-gradient KKT residual on the allowed slots <= 5e-9 and the distances to the oracle's rows <= 1e-6 (relative
Frobenius, max-abs over max) are those of tests/test_gpu_parity.py at tol 1e-9; excluded slots are exactly 0.0."""
import ctypes as C
import functools

import numpy as np
import pytest

import _structure_reference as SR
import gml_amd as gml
from oracle import oracle as O

pytestmark = pytest.mark.gpu
synthetic = __import__("importlib").import_module("gml_amd.synthetic")
_lib = gml._lib
EXCLUDED, FREE, PENALISED = gml.EXCLUDED, gml.FREE, gml.PENALISED
FORMS = ["RISE", "logRISE", "RPLE"]
PRECS = ["f64", "i8w", "i8x"]
RULES = ["row", "mean", "all", "any"]
# order 3: P = 781, the triples cross the kernels' 32-wide tiles; wide6, wide8: keys of up to six and eight spins (P = 382, 255), named
# so that they sort behind the older shapes, whose seeds are their positions in the sorted list
SHAPES = {"pairwise": (40, 2), "order3": (40, 3), "order4": (9, 4), "wide6": (10, 6), "wide8": (9, 8)}
N, K, C_PEN = 40, 3000, 0.4


def hist_from_spins(spins):
    return np.concatenate([np.ones((spins.shape[0], 1)), spins.astype(np.float64)], axis=1)


# ---- shared data and references (computed once) -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_data():
    """block_ising(40, 3000, block=8): K is no multiple of 1024 and the rows cross one 32-node tile; per row a random allowed set of
    3 .. 9 other spins"""
    spins, _ = synthetic.block_ising(N, K, block=8, seed=5)
    rng = np.random.default_rng(17)
    allowed = []
    for u in range(N):
        others = np.array([j for j in range(N) if j != u])
        allowed.append(np.sort(rng.choice(others, size=int(rng.integers(3, 10)), replace=False)))
    return spins, allowed


def structure_of(allowed, kind, n=N, field=FREE):
    S = np.full((n, n), EXCLUDED, dtype=np.uint8)
    for u, a in enumerate(allowed):
        S[u, a] = kind
        S[u, u] = field
    return S


def oracle_sub_row(spins, form, u, allowed, c):
    """the oracle's solution of node u restricted to `allowed`: learn_pair on the sub-histogram of the columns [u] + allowed, row 0;
    c' = c sqrt(log(n^2 / 0.05) / log(n'^2 / 0.05)) makes lambda the full problem's"""
    n = spins.shape[1]
    cols = [u] + [int(j) for j in allowed]
    c_sub = c * np.sqrt(np.log(n * n / 0.05) / np.log(len(cols) ** 2 / 0.05))
    sub, _, _ = O.learn_pair(hist_from_spins(spins[:, cols]), form, c=c_sub, symmetrize=False, tol=1e-12)
    row = np.zeros(n)
    row[cols] = sub[0]
    return row


@functools.lru_cache(maxsize=None)
def oracle_rows(form, case):
    """(n x n oracle rows, structure, c) of case "free" (allowed slots FREE, c = 0) or "pen" (PENALISED, c = 0.4)"""
    spins, allowed = pair_data()
    c = 0.0 if case == "free" else C_PEN
    rows = np.stack([oracle_sub_row(spins, form, u, allowed[u], c) for u in range(N)])
    return rows, structure_of(allowed, FREE if case == "free" else PENALISED), c


def oracle_kkt(form, spins, rows, S, lam, nodes=None):
    """max |pseudo-gradient| over the slots that are not excluded, from the oracle's gradient"""
    nodes = np.arange(rows.shape[0]) if nodes is None else np.asarray(nodes)
    _, g = O.objgrad_nodes(form, None, spins, nodes, rows[nodes])
    worst = 0.0
    for a, u in enumerate(nodes):
        x, ga = rows[u], g[a]
        pen = np.where(x > 0, ga + lam, np.where(x < 0, ga - lam, np.sign(ga) * np.maximum(np.abs(ga) - lam, 0)))
        pg = np.where(S[u] == FREE, ga, np.where(S[u] == PENALISED, pen, 0.0))
        worst = max(worst, float(np.abs(pg).max()))
    return worst


def assert_matches_oracle(form, spins, out, ref, S, lam, rows=None, label=""):
    rows = np.arange(out.shape[0]) if rows is None else np.asarray(rows)
    kkt = oracle_kkt(form, spins, out, S, lam, rows)
    fro = np.linalg.norm(out[rows] - ref[rows]) / np.linalg.norm(ref[rows])
    mx = np.abs(out[rows] - ref[rows]).max() / np.abs(ref[rows]).max()
    print(f"{label}: oracle KKT on the allowed slots {kkt:.2e}, rel-Frobenius {fro:.2e}, max-abs / max {mx:.2e}")
    assert kkt <= 5e-9
    assert fro <= 1e-6 and mx <= 1e-6
    assert (out[S == EXCLUDED] == 0.0).all() and not np.signbit(out[S == EXCLUDED]).any()


# ---- 1. the structure kernels equal the reference byte for byte -------------------------------------------------------------------------
def c_from_rows(rows_ptr, ld, n, order, rule, thr, kinds, S_ptr, ld_s):
    kept = C.c_int64(-1)
    _lib.check(_lib.lib().gml_structure_from_rows(rows_ptr, ld, n, order, _lib.RULES[rule], float(thr), *kinds, 0, S_ptr, ld_s, C.byref(kept)))
    return kept.value


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_structure_from_rows_equals_the_reference_byte_for_byte(shape, rule):
    import torch
    n, order = SHAPES[shape]
    P = SR.params_per_node(n, order)
    ld, ld_s = P + 3, P + 5
    rng = np.random.default_rng(sorted(SHAPES).index(shape))
    rows = np.full((n, ld), 1e300)  # (the padding of the rows must not be read)
    rows[:, :P] = rng.normal(size=(n, P))
    rows[n // 2, P // 3] = np.nan  # compares false: dropped
    for thr, kinds in ((float(np.nanmedian(np.abs(rows[:, :P]))), (FREE, EXCLUDED, FREE)), (0.0, (PENALISED, FREE, EXCLUDED))):
        want, kept_want = SR.structure_from_rows(rows[:, :P], n, order, thr, rule, *kinds)
        S = np.full((n, ld_s), 0xAA, dtype=np.uint8)
        kept = c_from_rows(_lib._ptr(rows), ld, n, order, rule, thr, kinds, _lib._ptr(S), ld_s)
        assert np.array_equal(S[:, :P], want) and (S[:, P:] == 0xAA).all()
        assert kept == kept_want == int((want == kinds[0]).sum()) - (n if kinds[2] == kinds[0] else 0)
        rows_d = torch.from_numpy(rows).cuda()
        S_d = torch.full((n, ld_s), 0xAA, dtype=torch.uint8, device="cuda")
        kept_d = c_from_rows(C.c_void_p(rows_d.data_ptr()), ld, n, order, rule, thr, kinds, C.c_void_p(S_d.data_ptr()), ld_s)
        assert np.array_equal(S_d.cpu().numpy(), S) and kept_d == kept  # device pointers: the same bytes, the padding untouched
    # the Python wrapper (host arrays, no padding)
    got, kept = gml.structure_from_rows(rows[:, :P], n, order, thr, rule=rule, keep=kinds[0], drop=kinds[1], field=kinds[2])
    assert got.dtype == np.uint8 and np.array_equal(got, want) and kept == kept_want


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_structure_from_keys_equals_the_reference_byte_for_byte(shape):
    import torch
    n, order = SHAPES[shape]
    P = SR.params_per_node(n, order)
    ld_s = P + 5
    rng = np.random.default_rng(100 + order)
    keys0 = [tuple(int(v) for v in rng.choice(n, size=int(rng.integers(1, order + 1)), replace=False)) for _ in range(60)]
    keys0 += keys0[:10] + [(3,), (3,), (n - 1,)]  # duplicates, keys of one spin
    want = SR.structure_from_keys(keys0, n, order, PENALISED, EXCLUDED, FREE)
    assert (want == PENALISED).sum() > 60
    karr = np.full((len(keys0), order + 1), -1, dtype=np.int32)  # (a stride above the order; unused slots anywhere in a key)
    for t, k in enumerate(keys0):
        karr[t, 1:1 + len(k)] = k
    L = _lib.lib()
    S = np.full((n, ld_s), 0xAA, dtype=np.uint8)
    _lib.check(L.gml_structure_from_keys(_lib._ptr(karr), order + 1, len(karr), n, order, PENALISED, EXCLUDED, FREE, 0, _lib._ptr(S), ld_s))
    assert np.array_equal(S[:, :P], want) and (S[:, P:] == 0xAA).all()
    S_d = torch.full((n, ld_s), 0xAA, dtype=torch.uint8, device="cuda")
    _lib.check(L.gml_structure_from_keys(_lib._ptr(karr), order + 1, len(karr), n, order, PENALISED, EXCLUDED, FREE, 0, C.c_void_p(S_d.data_ptr()), ld_s))
    assert np.array_equal(S_d.cpu().numpy(), S)
    # the wrapper takes the 1-based containers of Problem.term_moments; other kinds
    got = gml.structure_from_keys({tuple(i + 1 for i in k): 0.0 for k in keys0}, n, order, listed=FREE, other=PENALISED, field=EXCLUDED)
    assert np.array_equal(got, SR.structure_from_keys(keys0, n, order, FREE, PENALISED, EXCLUDED))
    assert np.array_equal(gml.structure_from_keys([], n, order), SR.structure_from_keys([], n, order))  # no term: fields only


# ---- 2. a restricted solve equals the oracle's ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", ["free", "pen"])
def test_restricted_solve_equals_the_oracle(case, form, prec):
    spins, _ = pair_data()
    ref, S, c = oracle_rows(form, case)
    with gml.Problem(spins=spins) as p:
        out, kkt, st = p.learn(form, c, tol=1e-9, precision=prec, structure=S)
    assert st["not_converged"] == 0 and kkt.max() <= 1e-9
    assert_matches_oracle(form, spins, out, ref, S, st["lambda_"], label=f"{case} {form} {prec}")
    if case == "pen":
        # outside the allowed set the gradient exceeds lambda: the unstructured problem has another solution
        _, g = O.objgrad_nodes(form, None, spins, np.arange(N), out)
        assert (np.abs(g)[S == EXCLUDED] > st["lambda_"]).any()


# ---- 3. the default structure is today's solve ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["i8w", "f64"])
def test_default_structure_gives_the_bits_of_the_plain_solve(prec):
    spins, _ = pair_data()
    S = np.full((N, N), PENALISED, dtype=np.uint8)
    S[np.arange(N), np.arange(N)] = FREE
    with gml.Problem(spins=spins) as p:
        opts = dict(tol=1e-9, precision=prec, hess_samples=-1)
        plain, kkt0, st0 = p.learn("RISE", C_PEN, **opts)
        got, kkt1, st1 = p.learn("RISE", C_PEN, structure=S, **opts)
    assert np.array_equal(plain, got) and np.array_equal(kkt0, kkt1)
    assert (st0["iterations"], st0["passes"], st0["forward_passes"]) == (st1["iterations"], st1["passes"], st1["forward_passes"])


# ---- 4. a node shard takes its rows of the structure ----------------------------------------------------------------------------------------
def test_shard_with_its_structure_rows_matches_the_full_handle():
    spins, _ = pair_data()
    _, S, c = oracle_rows("RISE", "pen")
    with gml.Problem(spins=spins) as p:
        full, _, st = p.learn("RISE", c, tol=1e-9, structure=S)
    with gml.Problem(spins=spins, node_range=(8, 40)) as p:
        part, kkt, stp = p.learn("RISE", c, tol=1e-9, structure=S[8:40])
    assert st["not_converged"] == 0 and stp["not_converged"] == 0
    assert np.abs(part - full[8:40]).max() <= 2e-9  # the header's bound between shardings at tol 1e-9
    assert ((part == 0) == (full[8:40] == 0)).all()


# ---- 5. matrix-free rows honour the structure -----------------------------------------------------------------------------------------------
def test_matrix_free_rows_honour_the_structure():
    n = 48
    spins, _ = synthetic.block_ising(n, 4000, block=8, seed=6)
    rng = np.random.default_rng(3)
    allowed = [np.sort(rng.choice(np.array([j for j in range(n) if j != u]), size=40, replace=False)) for u in range(n)]
    S = structure_of(allowed, FREE, n=n)
    assert ((S == FREE).sum(1) == 41).all() and ((S == EXCLUDED).sum(1) == 7).all()
    with gml.Problem(spins=spins) as p:
        cg, kkt_cg, st_cg = p.learn("RISE", 0.0, tol=1e-9, max_working=32, max_iter=200, structure=S)   # 41 > 32: Newton-CG
        ch, kkt_ch, st_ch = p.learn("RISE", 0.0, tol=1e-9, max_working=512, max_iter=200, structure=S)  # Cholesky blocks
    assert st_cg["not_converged"] == 0 and st_ch["not_converged"] == 0
    assert st_cg["hv_evals"] > 0 and st_ch["hv_evals"] == 0  # the matrix-free path really ran, and only there
    print(f"Newton-CG against Cholesky: max-abs {np.abs(cg - ch).max():.2e}")
    assert np.abs(cg - ch).max() <= 1e-7
    for out in (cg, ch):
        assert oracle_kkt("RISE", spins, out, S, 0.0) <= 5e-9
        assert (out[S == EXCLUDED] == 0.0).all()


# ---- 6. a row without parameters --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_row_without_parameters_is_complete_at_once(prec):
    spins, _ = pair_data()
    ref, S, c = oracle_rows("RISE", "pen")
    S = S.copy()
    S[5] = EXCLUDED  # the field included
    with gml.Problem(spins=spins) as p:
        out, kkt, st = p.learn("RISE", c, tol=1e-9, precision=prec, structure=S)
    assert (out[5] == 0.0).all() and kkt[5] == 0.0 and st["not_converged"] == 0
    rest = np.array([u for u in range(N) if u != 5])
    assert kkt[rest].max() <= 1e-9
    assert_matches_oracle("RISE", spins, out, ref, S, st["lambda_"], rows=rest, label=f"empty row {prec}")
    with gml.Problem(spins=spins, node_range=(4, 7)) as p:  # ... and a handle all of whose rows are empty
        out, kkt, st = p.learn("RISE", c, tol=1e-9, precision=prec, structure=np.zeros((3, N), dtype=np.uint8), x0=np.ones((3, N)))
    assert (out == 0.0).all() and (kkt == 0.0).all() and st["not_converged"] == 0 and st["passes"] == 0


# ---- 7. multi-body -------------------------------------------------------------------------------------------------------------------------------
def test_multibody_structure_from_the_true_keys():
    n, order = 12, 3
    spins, terms = synthetic.block_multibody(n, 4000, block=12, seed=2)
    hist = hist_from_spins(spins)
    S = gml.structure_from_keys(terms, n, order, listed=FREE, other=EXCLUDED)
    assert S.shape == (n, 67) and np.array_equal(S, SR.structure_from_keys([tuple(i - 1 for i in k) for k in terms], n, order, FREE, EXCLUDED, FREE))
    assert (S[:, 0] == FREE).all() and 0 < (S == FREE).sum() < S.size
    x0 = np.random.default_rng(1).normal(scale=0.1, size=S.shape)
    assert (x0[S == EXCLUDED] != 0).all()  # must be ignored ...
    x0[np.nonzero(S == EXCLUDED)[0][0], np.nonzero(S == EXCLUDED)[1][0]] = np.nan  # ... whatever they hold
    with gml.Problem(spins=spins, order=order) as p:
        assert p.P == 67
        out, kkt, st = p.learn("RISE", 0.0, tol=1e-9, structure=S, x0=x0)
        cold, _, _ = p.learn("RISE", 0.0, tol=1e-9, structure=S)
    assert st["not_converged"] == 0 and kkt.max() <= 1e-9
    assert (out[S == EXCLUDED] == 0.0).all()
    worst = 0.0
    for u in range(n):
        _, g = O.objgrad_multi(hist, order, u, out[u])
        worst = max(worst, float(np.abs(g[S[u] == FREE]).max()))
    print(f"order 3: oracle gradient on the allowed slots {worst:.2e}, warm against cold start {np.abs(out - cold).max():.2e}")
    assert worst <= 5e-9
    assert np.abs(out - cold).max() <= 2e-9 * max(1.0, np.abs(cold).max()) * 100  # the same (unique) optimum from either start


# ---- 8. the front door: l1 solve, support, refit ---------------------------------------------------------------------------------------------
def gap_threshold(values, near=0.1, width=1e-3):
    """the midpoint, nearest `near`, of a gap at least `width` wide in the sorted magnitudes: a support cut there cannot flip on a 1e-9
    difference between two solvers"""
    v = np.sort(np.abs(np.asarray(values)).ravel())
    gaps = np.nonzero(np.diff(v) >= width)[0]
    mids = 0.5 * (v[gaps] + v[gaps + 1])
    return float(mids[np.argmin(np.abs(mids - near))])


@functools.lru_cache(maxsize=None)
def oracle_refit(symmetrize):
    """(tau, support mask, refit rows of the oracle) for RISE(0.4, symmetrize) on the pair data"""
    spins, _ = pair_data()
    l1, _, _ = O.learn_pair(hist_from_spins(spins), "RISE", c=C_PEN, symmetrize=symmetrize, tol=1e-12)
    off = ~np.eye(N, dtype=bool)
    tau = gap_threshold(l1[off])
    support = (np.abs(l1) >= tau) & off
    rows = np.stack([oracle_sub_row(spins, "RISE", u, np.nonzero(support[u])[0], 0.0) for u in range(N)])  # unpenalised: c = 0
    return tau, support, rows


@pytest.mark.parametrize("symmetrize", [True, False])
def test_front_door_refit_on_the_learned_support(symmetrize):
    spins, _ = pair_data()
    tau, support, rows = oracle_refit(symmetrize)
    assert 0 < support.sum() < N * (N - 1)
    assert not symmetrize or (support == support.T).all()
    want = 0.5 * (rows + rows.T) if symmetrize else rows
    method = gml.HIP(refit=tau)
    got = gml.learn(hist_from_spins(spins), gml.RISE(C_PEN, symmetrize), method)
    off = ~np.eye(N, dtype=bool)
    assert np.array_equal((got != 0) & off, support)  # the oracle's thresholded support ...
    assert (got[~support & off] == 0.0).all()          # ... and exactly 0 off it
    assert method.stats["support"] == int(support.sum())
    assert method.stats["refit"]["not_converged"] == 0 and method.stats["not_converged"] == 0
    fro = np.linalg.norm(got - want) / np.linalg.norm(want)
    mx = np.abs(got - want).max() / np.abs(want).max()
    print(f"refit, symmetrize {symmetrize}: tau {tau:.4f}, support {int(support.sum())}, rel-Frobenius {fro:.2e}, max-abs / max {mx:.2e}")
    assert fro <= 1e-6 and mx <= 1e-6
    # the shrinkage is gone: the refit is not the l1 solution restricted to the support
    l1 = gml.learn(hist_from_spins(spins), gml.RISE(C_PEN, symmetrize), gml.HIP())
    assert np.abs(got[support]).mean() > np.abs(l1[support]).mean()


def test_front_door_structure_and_node_range():
    spins, _ = pair_data()
    ref, S, c = oracle_rows("RISE", "pen")
    hist = hist_from_spins(spins)
    got = gml.learn(hist, gml.RISE(c, False), gml.HIP(structure=S))
    assert_matches_oracle("RISE", spins, got, ref, S, O.lam(c, N, K), label="front door")
    part = gml.learn(hist, gml.RISE(c, False), gml.HIP(structure=S, node_range=(8, 40)))  # the method slices its rows
    assert part.shape == (32, N) and np.abs(part - got[8:40]).max() <= 2e-9


# ---- 9. errors on the device path -------------------------------------------------------------------------------------------------------------
def test_device_structure_with_a_bad_value_is_refused_and_the_handle_lives_on():
    import torch
    spins, _ = pair_data()
    _, S, c = oracle_rows("RISE", "pen")
    L = _lib.lib()
    o = _lib.Opts()
    L.gml_default_opts(C.byref(o))
    out = np.zeros((N, N))
    with gml.Problem(spins=spins) as p:
        bad = S.copy()
        bad[33, 7] = 3
        S_d = torch.from_numpy(bad).cuda()
        rc = L.gml_learn_structured(p._h, 0, c, C.byref(o), C.c_void_p(S_d.data_ptr()), N, None, _lib._ptr(out), None, None)
        assert rc == _lib.GML_EINVAL and "row 33, slot 7" in L.gml_last_error().decode()
        with pytest.raises(gml.GMLError, match="row 33, slot 7"):  # a host array: refused before any device work
            p.learn("RISE", c, structure=bad)
        rc = L.gml_learn_structured(p._h, 0, c, C.byref(o), C.c_void_p(S_d.data_ptr()), N - 1, None, _lib._ptr(out), None, None)
        assert rc == _lib.GML_EINVAL and "leading dimension" in L.gml_last_error().decode()
        # the handle is still usable: a good device structure gives the bits of the host one
        S_d = torch.from_numpy(S).cuda()
        rc = L.gml_learn_structured(p._h, 0, c, C.byref(o), C.c_void_p(S_d.data_ptr()), N, None, _lib._ptr(out), None, None)
        assert rc == _lib.GML_OK
        host, _, _ = p.learn("RISE", c, structure=S)
    assert np.array_equal(out, host)
