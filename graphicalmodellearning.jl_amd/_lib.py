"""ctypes binding of libgml_hip.so (C ABI: include/gml.h).

The library is the only compute path: if it is missing, or no HIP device is present, every
call fails loudly -- there is no CPU fallback in the product.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GML_LIB_OVERRIDE") or os.path.join(_HERE, "libgml_hip.so")  # override: A/B builds

GML_OK, GML_EINVAL, GML_ENOTCONV, GML_EHIP, GML_ENOMEM, GML_EUNSUPPORTED = range(6)
GML_ABI_VERSION = 6  # include/gml.h: the revision of the C ABI the mirrors below (Opts, Stats, argument lists) were written against
FORMULATION_IDS = {"RISE": 0, "RISEA": 0, "multiRISE": 0, "logRISE": 1, "RPLE": 2}
DTYPES = {np.dtype(np.int8): 0, np.dtype(np.int32): 1, np.dtype(np.int64): 2, np.dtype(np.float64): 3}
EXCLUDED, FREE, PENALISED = 0, 1, 2  # GML_PARAM_*: the kind of a parameter slot in a structure (gml_learn_structured)
RULES = {"row": 0, "mean": 1, "all": 2, "any": 3}  # GML_RULE_*: how structure_from_rows decides a key from its members' entries
PRECISIONS = {"f64": 0, "i8x": 1, "auto": 2, "i8w": 3}  # auto: i8x, i8w for tight tolerances / small problems / operator calls; i8w: FP64-grade int8 limbs


class GMLError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libgml_hip error {code}: {msg}")
        self.code = code


class GMLConvergenceError(AssertionError):
    """Mirrors the reference's `@assert termination_status == LOCALLY_SOLVED`
    (GraphicalModelLearning.jl:127,180,251,289,327)."""


class Opts(C.Structure):
    _fields_ = [("tol", C.c_double), ("max_iter", C.c_int32), ("precision", C.c_int32),
                ("max_working", C.c_int32), ("max_add", C.c_int32), ("verbose", C.c_int32),
                ("hess_samples", C.c_int32), ("polish", C.c_int32), ("max_cg", C.c_int32),
                ("limbs_fwd", C.c_int32), ("hv_limbs_fwd", C.c_int32), ("hv_limbs_bwd", C.c_int32), ("debug_row", C.c_int32),
                ("hv_subsample", C.c_int32), ("coarse", C.c_int32), ("cg_viol_frac", C.c_double), ("cg_eta", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("passes", C.c_int32), ("forward_passes", C.c_int32),
                ("hessian_passes", C.c_int32), ("node_evals", C.c_int64), ("max_kkt", C.c_double),
                ("lambda_", C.c_double), ("t_pack", C.c_double), ("t_pass", C.c_double),
                ("t_hess", C.c_double), ("t_host", C.c_double), ("t_total", C.c_double),
                ("not_converged", C.c_int32), ("polished", C.c_int32), ("hv_evals", C.c_int64), ("t_assemble", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


_lib = None


def lib():
    """Load libgml_hip.so.  torch (if installed) is imported first so that both share one HIP
    runtime (same libamdhip64 SONAME)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GMLError(GML_EHIP, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                 "(make -C graphicalmodellearning.jl_amd/csrc)")
    try:
        import torch  # noqa: F401  (loads torch's libamdhip64.so first)
    except Exception:
        pass
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    i64, dbl, p, i32 = C.c_int64, C.c_double, C.c_void_p, C.c_int
    _check_abi(L)
    L.gml_last_error.restype = C.c_char_p
    L.gml_default_opts.argtypes = [C.POINTER(Opts)]
    L.gml_default_opts.restype = None
    L.gml_lambda.restype = dbl
    L.gml_lambda.argtypes = [dbl, i64, dbl]
    L.gml_problem_create.argtypes = [p, i32, i64, i64, i64, i32, i32, i64, i64, i32, C.POINTER(p)]
    L.gml_problem_create_device_convert.argtypes = L.gml_problem_create.argtypes
    L.gml_problem_ingest_times.argtypes = [p, p]
    L.gml_packed_words.restype = i64
    L.gml_packed_words.argtypes = [i64]
    L.gml_pack_histogram.argtypes = [p, i32, i64, i64, i64, i32, p, i64, p, C.POINTER(dbl)]
    L.gml_problem_create_packed.argtypes = [p, i64, p, i64, i64, i32, i64, i64, i32, C.POINTER(p)]
    L.gml_problem_get_sign_bits.argtypes = [p, p]
    L.gml_problem_create_spins.argtypes = [p, p, i64, i64, i32, i64, i64, i32, C.POINTER(p)]
    L.gml_problem_create_sampled.argtypes = [p, i64, i64, C.c_uint64, i32, i64, i64, i32, C.POINTER(p)]
    L.gml_problem_create_sampled_terms.argtypes = [p, i32, p, i64, i64, i64, C.c_uint64, i32, i64, i64, i32, C.POINTER(p)]
    L.gml_problem_create_mcmc_terms.argtypes = [p, i32, p, i64, i64, i64, C.c_uint64, i32, i32, i64, i64, i32, C.POINTER(p)]
    L.gml_problem_create_mcmc_chains.argtypes = [p, i64, i64, i64, i32, i32, C.c_uint64, i32, i32, i64, i64, i32, C.POINTER(p)]
    L.gml_problem_create_mcmc_terms_chains.argtypes = [p, i32, p, i64, i64, i64, i64, i32, i32, C.c_uint64, i32, i32, i64, i64, i32,
                                                       C.POINTER(p)]
    L.gml_problem_create_mcmc_terms_tempered.argtypes = [p, i32, p, i64, i64, i64, i64, i32, i32, p, i32, i32, C.c_uint64, i32, i32, i64,
                                                         i64, i32, p, C.POINTER(p)]
    L.gml_log_partition_ais.argtypes = [p, i32, p, i64, i64, i64, p, i64, i32, C.c_uint64, i32, p, p, p, p]
    L.gml_model_exact.argtypes = [p, i32, p, i64, i64, p, i32, i64, i32, C.POINTER(dbl), p, p, p]
    L.gml_problem_create_mcmc_terms_conditional.argtypes = [p, i32, p, i64, i64, p, p, i32, i64, i32, i32, C.c_uint64, i32, i64, i64,
                                                            C.POINTER(p)]
    L.gml_conditional_means.argtypes = [p, i32, p, i64, i64, p, p, i32, i64, i32, i32, C.c_uint64, p]
    L.gml_problem_create_mcmc_terms_masked.argtypes = [p, i32, p, i64, i64, p, p, i32, i64, i32, i32, C.c_uint64, i32, i64, i64, C.POINTER(p)]
    L.gml_conditional_means_masked.argtypes = [p, i32, p, i64, i64, p, p, i32, i64, i32, i32, C.c_uint64, p]
    L.gml_conditional_exact.argtypes = [p, i32, p, i64, i64, p, p, p, p, p]
    L.gml_conditional_exact_masked.argtypes = [p, i32, p, i64, i64, p, p, p, p, p]
    L.gml_model_best_states.argtypes = [p, i32, p, i64, i64, i64, i32, C.POINTER(i64), p, p]
    L.gml_model_elim_plan.argtypes = [p, i32, p, i64, i64, p, p, C.POINTER(C.c_int32), C.POINTER(dbl), C.POINTER(dbl)]
    L.gml_model_elim.argtypes = [p, i32, p, i64, i64, p, i32, C.POINTER(dbl), p, p]
    L.gml_problem_create_sampled_elim.argtypes = [p, i32, p, i64, i64, i64, C.c_uint64, p, i32, i32, i64, i64, i32, C.POINTER(p)]
    L.gml_conditional_mode.argtypes = [p, i32, p, i64, i64, p, p, p, p, p]
    L.gml_conditional_mode_masked.argtypes = [p, i32, p, i64, i64, p, p, p, p, p]
    L.gml_conditional_draw.argtypes = [p, i32, p, i64, i64, p, p, i32, C.c_uint64, p, p, p]
    L.gml_conditional_draw_masked.argtypes = [p, i32, p, i64, i64, p, p, i32, C.c_uint64, p, p, p]
    L.gml_problem_create_sampled_hist.argtypes =[p, i32, p, i64, i64, i64, C.c_uint64, i32, i32, i64, i64, i32, C.POINTER(p)]
    L.gml_problem_get_counts.argtypes = [p, p]
    L.gml_problem_get_spins.argtypes = [p, p]
    L.gml_problem_moments.argtypes = [p, p, p]
    L.gml_problem_term_moments.argtypes = [p, p, i32, i64, p]
    L.gml_problem_fold_sizes.argtypes = [p, i32, C.c_uint64, p]
    L.gml_problem_split.argtypes = [p, i32, i32, C.c_uint64, i32, C.POINTER(p)]
    L.gml_problem_destroy.argtypes = [p]
    L.gml_problem_destroy.restype = None
    L.gml_problem_info.argtypes = [p] + [p] * 6
    L.gml_multi_keys.argtypes = [p, i64, p]
    L.gml_objgrad_batch.argtypes = [p, i32, i32, i64, p, p, i64, p, p]
    L.gml_hessvec_batch.argtypes = [p, i32, i64, p, p, p, i64, p]
    L.gml_hessvec_batch_prec.argtypes = [p, i32, i32, i64, p, p, p, i64, p]
    L.gml_multi_create.argtypes = [p, i32, i64, i64, i64, i32, i32, p, i32, C.POINTER(p)]
    L.gml_multi_info.argtypes = [p] + [p] * 6
    L.gml_multi_learn.argtypes = [p, i32, dbl, C.POINTER(Opts), p, p, C.POINTER(Stats), p]
    L.gml_multi_part_stats.argtypes = [p, p]
    L.gml_multi_destroy.argtypes = [p]
    L.gml_multi_destroy.restype = None
    L.gml_learn.argtypes = [p, i32, dbl, C.POINTER(Opts), p, p, C.POINTER(Stats)]
    L.gml_learn_warm.argtypes = [p, i32, dbl, C.POINTER(Opts), p, p, p, C.POINTER(Stats)]
    L.gml_learn_structured.argtypes = [p, i32, dbl, C.POINTER(Opts), p, i64, p, p, p, C.POINTER(Stats)]
    L.gml_stderr.argtypes = [p, i32, p, i64, p, i64, p, p, p]
    L.gml_structure_from_rows.argtypes = [p, i64, i64, i32, i32, dbl, i32, i32, i32, i32, p, i64, C.POINTER(i64)]
    L.gml_structure_from_keys.argtypes = [p, i32, i64, i64, i32, i32, i32, i32, i32, p, i64]
    L.gml_terms_count.restype = i64
    L.gml_terms_count.argtypes = [i64, i32, i32]
    L.gml_terms_assemble.argtypes = [p, i64, i64, i32, i32, i32, p]
    L.gml_terms_keys.argtypes = [i64, i32, i32, i64, i64, p]
    L.gml_terms_rank.restype = i64
    L.gml_terms_rank.argtypes = [i64, i32, i32, p, i32]
    L.gml_learn_terms.argtypes = [p, i32, dbl, i32, C.POINTER(Opts), p, p, C.POINTER(Stats)]
    L.gml_learn_matrix.argtypes = [p, i32, dbl, i32, C.POINTER(Opts), p, p, C.POINTER(Stats)]
    L.gml_matrix_symmetrize.argtypes = [p, i64, i64, i32, p]
    L.gml_bench_pass.argtypes = [p, i32, i32, p, i32, i32, p]
    L.gml_bench_pass_resident.argtypes = [p, i32, i32, p, i32, i32, p, p, p, p]
    _lib = L
    return L


def _check_abi(L):
    """A library of another ABI revision would read / write Opts and Stats at the wrong offsets without any error: refuse it
    (include/gml.h, "ABI identity").  Libraries older than the check itself lack the symbols."""
    try:
        L.gml_sizeof_opts.restype = L.gml_sizeof_stats.restype = C.c_int64
        got = (int(L.gml_abi_version()), int(L.gml_sizeof_opts()), int(L.gml_sizeof_stats()))
    except AttributeError:
        raise GMLError(GML_EUNSUPPORTED, f"{LIB_PATH} predates gml_abi_version(): rebuild it (this binding is ABI {GML_ABI_VERSION})")
    want = (GML_ABI_VERSION, C.sizeof(Opts), C.sizeof(Stats))
    if got != want:
        raise GMLError(GML_EUNSUPPORTED, f"{LIB_PATH} has ABI version / sizeof(gml_opts) / sizeof(gml_stats) = {got}, this binding "
                                         f"was written against {want}: library and binding come from different revisions")


def check(rc, allow=()):
    if rc != GML_OK and rc not in allow:
        raise GMLError(rc, lib().gml_last_error().decode())
    return rc


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _hist_args(samples):
    """(array kept alive, dtype id, K, n, ld, col_major) of a K x (1+n) histogram in the layout it already has"""
    s = np.asarray(samples)
    if s.ndim != 2 or s.shape[1] < 2:
        raise GMLError(GML_EINVAL, "samples must be a K x (1+n) histogram matrix")
    if s.dtype not in DTYPES:
        s = s.astype(np.float64)
    col_major = bool(s.flags.f_contiguous and not s.flags.c_contiguous)
    if not (s.flags.c_contiguous or s.flags.f_contiguous):
        s = np.ascontiguousarray(s)
    K, n = s.shape[0], s.shape[1] - 1
    return s, DTYPES[s.dtype], K, n, (K if col_major else n + 1), int(col_major)


def trim_cache():
    """Return the device memory the library keeps for reuse to the driver (gml_trim_cache); bytes released."""
    L = lib()
    L.gml_trim_cache.restype = C.c_int64
    return int(L.gml_trim_cache())


def set_cache_limit(bytes_per_device):
    """Cap of that cache per device (gml_set_cache_limit): 0 = keep nothing, < 0 = the default (a quarter of the device)."""
    L = lib()
    L.gml_set_cache_limit.restype = None
    L.gml_set_cache_limit.argtypes = [C.c_int64]
    L.gml_set_cache_limit(int(bytes_per_device))


def pack_histogram(samples):
    """Host-only (gml_pack_histogram): histogram matrix -> (sign_bits [n][words] uint32, counts [K] float64, M)."""
    L = lib()
    s, dt, K, n, ld, cm = _hist_args(samples)
    wpr = L.gml_packed_words(K)
    bits = np.empty((n, wpr), dtype=np.uint32)
    counts = np.empty(K, dtype=np.float64)
    M = C.c_double()
    check(L.gml_pack_histogram(_ptr(s), dt, K, n, ld, cm, _ptr(bits), wpr, _ptr(counts), C.byref(M)))
    return bits, counts, M.value


def terms_count(n, order, symmetrize):
    """number of terms of a learned model of `n` spins (gml_terms_count): symmetrised C(n,1)+...+C(n,order), else n P"""
    T = int(lib().gml_terms_count(int(n), int(order), int(bool(symmetrize))))
    if T < 0:
        raise GMLError(GML_EUNSUPPORTED, lib().gml_last_error().decode())
    return T


def terms_assemble(rows, n, order, symmetrize, device=0, ld=None):
    """gml_terms_assemble: the n solved rows -> the model's weights in (length, key) order, on the device.  rows: an (n, P)
    float64 ndarray, or an int device pointer (then ld = its row pitch in doubles)."""
    out = np.empty(terms_count(n, order, symmetrize))
    if isinstance(rows, (int, np.integer)):
        ptr, ld = C.c_void_p(int(rows)), int(ld)
    else:
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[0] != n:
            raise GMLError(GML_EINVAL, f"terms_assemble needs the rows of all {n} nodes, got {rows.shape}")
        ptr, ld = _ptr(rows), rows.shape[1]
    check(lib().gml_terms_assemble(ptr, ld, int(n), int(order), int(bool(symmetrize)), int(device), _ptr(out)))
    return out


def matrix_symmetrize(rows, device=0):
    """gml_matrix_symmetrize: 0.5 (R + R') of the gathered n x n rows, on the device (:184-186); same bits as the host expression"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[0] != rows.shape[1]:
        raise GMLError(GML_EINVAL, f"matrix_symmetrize needs the rows of all nodes (a square matrix), got {rows.shape}")
    out = np.empty_like(rows)
    check(lib().gml_matrix_symmetrize(_ptr(rows), rows.shape[1], rows.shape[0], int(device), _ptr(out)))
    return out


def params_per_node(n, order):
    """P: parameters per node (n for order 2, sum_{s <= order} C(n-1, s-1) in general): the row length of learn() and of a structure"""
    n, order = int(n), int(order)
    return n if order == 2 else terms_count(n, order, False) // n


def structure_from_rows(rows, n, order, threshold, rule="mean", keep=FREE, drop=EXCLUDED, field=FREE, device=0):
    """gml_structure_from_rows: the structure of a refit from the n solved rows ((n, P) float64; order 2: also the symmetrised
    n x n matrix), on the device.  A non-field slot is `keep` where its entry -- rule "row" -- or its key's mean / every / some member
    entry -- "mean" / "all" / "any" -- reaches `threshold` in magnitude, else `drop`; fields are `field`.  Returns (uint8 [n, P],
    kept): the structure for Problem.learn(structure=...) and the number of kept non-field entries."""
    if rule not in RULES:
        raise GMLError(GML_EINVAL, f"structure_from_rows: unknown rule {rule!r} (use 'row', 'mean', 'all' or 'any')")
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    P = params_per_node(n, order)
    if rows.shape != (int(n), P):
        raise GMLError(GML_EINVAL, f"structure_from_rows needs the rows of all {n} nodes, {(int(n), P)}, got {rows.shape}")
    out = np.empty((int(n), P), dtype=np.uint8)
    kept = C.c_int64()
    check(lib().gml_structure_from_rows(_ptr(rows), P, int(n), int(order), RULES[rule], float(threshold), int(keep), int(drop), int(field),
                                        int(device), _ptr(out), P, C.byref(kept)))
    return out, int(kept.value)


def structure_from_keys(terms, n, order, listed=PENALISED, other=EXCLUDED, field=FREE, device=0):
    """gml_structure_from_keys: the structure that holds the listed terms -- the containers and the 1-based keys of
    Problem.term_moments (a dict or list of tuples, a FactorGraph, a TermArray).  Every slot is `other` and every field `field`,
    except that a listed key S sets the slot of (u, S without u) in the row of each of its members u to `listed` (a key of one spin:
    that spin's field).  Returns uint8 [n, P]."""
    P = params_per_node(n, order)
    out = np.empty((int(n), P), dtype=np.uint8)
    windows = list(moment_key_windows(terms)) or [np.zeros((0, 1), dtype=np.int32)]
    if len(windows) > 1:  # (an array-backed model comes in windows of one stride)
        windows = [np.concatenate(windows, axis=0)]
    keys = windows[0]
    check(lib().gml_structure_from_keys(_ptr(keys), keys.shape[1], len(keys), int(n), int(order), int(listed), int(other), int(field),
                                        int(device), _ptr(out), P))
    return out


def terms_keys(n, order, symmetrize, first=0, count=None):
    """keys of the terms [first, first + count) (gml_terms_keys; host only): int32 [count, order], 0-based spins, -1 = unused"""
    if count is None:
        count = terms_count(n, order, symmetrize) - first
    keys = np.empty((int(count), int(order)), dtype=np.int32)
    check(lib().gml_terms_keys(int(n), int(order), int(bool(symmetrize)), int(first), int(count), _ptr(keys)))
    return keys


def terms_rank(n, order, symmetrize, key0):
    """position of the 0-based key among the terms (gml_terms_rank), -1 if the model has no such key"""
    k = np.ascontiguousarray(key0, dtype=np.int32)
    return int(lib().gml_terms_rank(int(n), int(order), int(bool(symmetrize)), _ptr(k), len(k)))


def _node_range(node_range, n):
    """(node0, node1) of a handle: the given range, by default every node."""
    return node_range if node_range is not None else (0, int(n))


def moment_key_windows(terms, chunk=1 << 22):
    """The keys of `terms` as the C ABI takes them, window by window: int32 arrays [count, stride], 0-based spins, -1 = unused slot.
    terms: what Problem(terms=...) takes for keys -- a dict of 1-based tuples (its values are not looked at), any iterable of
    1-based tuples, a FactorGraph (its terms), or a TermArray, whose key table is generated window by window through keys_array
    and never held whole.  Host only."""
    terms = getattr(terms, "terms", terms)  # a FactorGraph
    if hasattr(terms, "keys_array"):
        for a in range(0, len(terms), chunk):
            yield np.ascontiguousarray(terms.keys_array(a, min(chunk, len(terms) - a)) - 1, dtype=np.int32)
        return
    klist = [tuple(int(i) for i in k) for k in terms]
    if not klist:
        return
    for k in klist:
        if any(i < 1 for i in k):
            raise GMLError(GML_EINVAL, f"term {k}: spins are numbered from 1")
    stride = max(1, max(len(k) for k in klist))
    keys = np.full((len(klist), stride), -1, dtype=np.int32)
    for t, k in enumerate(klist):
        keys[t, :len(k)] = np.asarray(k, dtype=np.int64) - 1
    yield keys


def term_arrays(terms, n=None):
    """(keys int32 [T, stride] 0-based with -1 = unused slot, weights float64 [T], stride, n) of a model given as {1-based key tuple:
    weight} or as an array-backed TermArray: the term list as the C ABI takes it.  n: the number of spins, by default the largest
    spin named.  Host only."""
    if hasattr(terms, "keys_array"):
        # an array-backed learned model (factor_graph.TermArray: millions of terms): its non-zero terms, without a Python loop
        nz = np.flatnonzero(terms.weights != 0.0)
        if n is None:
            n = terms.varible_count
        stride = terms.order
        wts = np.ascontiguousarray(terms.weights[nz])
        keys = np.empty((len(nz), stride), dtype=np.int32)
        chunk = 1 << 22
        for a in range(0, len(terms), chunk):  # (the key table is generated window by window: it is never held whole)
            lo, hi = np.searchsorted(nz, (a, min(len(terms), a + chunk)))
            if hi > lo:
                keys[lo:hi] = terms.keys_array(a, min(chunk, len(terms) - a))[nz[lo:hi] - a] - 1
        if len(nz) == 0:
            keys, wts = np.array([[0] + [-1] * (stride - 1)], dtype=np.int32), np.zeros(1)
    else:
        if n is None:
            n = max(max(k) for k in terms if len(k))
        stride = max(1, max(len(k) for k in terms))
        keys = np.full((len(terms), stride), -1, dtype=np.int32)
        wts = np.zeros(len(terms), dtype=np.float64)
        for t, (k, v) in enumerate(terms.items()):
            keys[t, :len(k)] = np.asarray(k, dtype=np.int64) - 1
            wts[t] = v
    return keys, wts, stride, n


def log_partition_ais(terms, n, chains, betas, sweeps_per_step=1, seed=0, device=0, return_states=False):
    """gml_log_partition_ais on a term list as term_arrays takes it: (result [3] = log Z, its standard error, the effective sample
    size; log_weights [chains]; energies [chains] and spins [chains, n] int8 with return_states, else None)."""
    keys, wts, stride, n = term_arrays(terms, n)
    betas = np.ascontiguousarray(betas, dtype=np.float64).ravel()
    chains = int(chains)
    if not 1 <= chains <= 2 ** 31:  # (the library's own check, made before the output arrays are)
        raise GMLError(GML_EINVAL, f"chains must lie in [1, 2^31] (given {chains})")
    logw, result = np.zeros(chains), np.zeros(3)
    energies = np.zeros(chains) if return_states else None
    spins = np.zeros((chains, int(n)), dtype=np.int8) if return_states else None
    check(lib().gml_log_partition_ais(_ptr(keys), stride, _ptr(wts), len(wts), int(n), chains, _ptr(betas), len(betas),
                                      int(sweeps_per_step), int(seed), int(device), _ptr(logw), _ptr(energies), _ptr(spins), _ptr(result)))
    return result, logw, energies, spins


def model_exact(terms, n, queries=None, pairs=True, device=0):
    """gml_model_exact on a term list as term_arrays takes it: (log_z, m [n], C [n, n] or None without pairs, q [len(queries)] or
    None without queries) -- exact log Z, means, pair correlations and the expectations of the query keys (what
    Problem.term_moments takes for keys), by enumeration on the device; components of at most 40 spins."""
    keys, wts, stride, n = term_arrays(terms, n)
    n = int(n)
    qkeys = None
    if queries is not None:
        windows = list(moment_key_windows(queries)) or [np.zeros((0, 1), dtype=np.int32)]
        width = max(w.shape[1] for w in windows)
        qkeys = np.full((sum(len(w) for w in windows), width), -1, dtype=np.int32)
        at = 0
        for w in windows:
            qkeys[at:at + len(w), :w.shape[1]] = w
            at += len(w)
    nq = 0 if qkeys is None else len(qkeys)
    log_z = C.c_double()
    m = np.zeros(max(n, 0))
    corr = np.zeros((max(n, 0), max(n, 0))) if pairs else None
    q = np.zeros(max(nq, 1)) if qkeys is not None else None
    check(lib().gml_model_exact(_ptr(keys), stride, _ptr(wts), len(wts), n, _ptr(qkeys) if nq else None, qkeys.shape[1] if nq else 1, nq,
                                int(device), C.byref(log_z), _ptr(m), _ptr(corr), _ptr(q) if nq else None))
    return float(log_z.value), m, corr, (q[:nq] if q is not None else None)


def model_best_states(terms, n, k, device=0):
    """gml_model_best_states on a term list as term_arrays takes it: (states int8 [found, n] of +-1, energies float64 [found]) -- the
    found = min(k, 2^n) most probable states, energy descending, equal energies in state order (spin i at bit i, a set bit is -1); by
    enumeration on the device, k <= 256, components of at most 40 spins."""
    keys, wts, stride, n = term_arrays(terms, n)
    n, k = int(n), int(k)
    rows = min(max(k, 0), 256)  # (the library refuses a k outside [1, 256] before it writes)
    states = np.zeros((rows, max(n, 0)), dtype=np.int8)
    energies = np.zeros(rows)
    found = C.c_int64()
    check(lib().gml_model_best_states(_ptr(keys), stride, _ptr(wts), len(wts), n, k, int(device), C.byref(found), _ptr(states),
                                      _ptr(energies)))
    return states[:found.value], energies[:found.value]


def _elim_order(order, n):
    """a caller's elimination order (1-based spins, as the keys of a model are) as the 0-based int32 array of the C ABI, or None"""
    if order is None:
        return None
    order = np.ascontiguousarray(np.asarray(order, dtype=np.int64).ravel() - 1, dtype=np.int32)
    if len(order) != n:
        raise GMLError(GML_EINVAL, f"order must name each of the {n} spins once (given {len(order)} entries)")
    return order


def model_elim_plan(terms, n, order=None):
    """gml_model_elim_plan on a term list as term_arrays takes it: (order int32 [n] of 1-based spins, width, work, stored) -- the
    elimination order (order=None: the greedy one; else a permutation of 1 .. n), the largest scope, sum_t 2^|scope_t| and
    sum_t 2^|F_t|.  Host only: no device is needed."""
    keys, wts, stride, n = term_arrays(terms, n)
    n = int(n)
    order = _elim_order(order, n)
    out = np.zeros(max(n, 0), dtype=np.int32)
    width, work, stored = C.c_int32(), C.c_double(), C.c_double()
    check(lib().gml_model_elim_plan(_ptr(keys), stride, _ptr(wts), len(wts), n, _ptr(order), _ptr(out), C.byref(width), C.byref(work),
                                    C.byref(stored)))
    return out + 1, int(width.value), float(work.value), float(stored.value)


def model_elim(terms, n, order=None, mean=True, texp=True, device=0):
    """gml_model_elim on a term list as term_arrays takes it: (log_z, m [n] or None, e [number of terms] or None) -- exact log Z, the
    means and the expectation of every term of the model (in the order term_arrays lists them: a dict's own order; the non-zero terms
    of an array-backed model), by variable elimination on the device; elimination orders of width at most 30."""
    keys, wts, stride, n = term_arrays(terms, n)
    n = int(n)
    order = _elim_order(order, n)
    log_z = C.c_double()
    m = np.zeros(max(n, 0)) if mean else None
    e = np.zeros(len(wts)) if texp else None
    check(lib().gml_model_elim(_ptr(keys), stride, _ptr(wts), len(wts), n, _ptr(order), int(device), C.byref(log_z), _ptr(m), _ptr(e)))
    return float(log_z.value), m, e


class Problem:
    """RAII wrapper of a gml_problem handle (packed spins + weights resident in HBM)."""

    def __init__(self, samples=None, *, counts=None, spins=None, packed=None, model=None, terms=None, n=None, num_samples=None,
                 seed=0, mcmc_sweeps=None, order=2, node_range=None, device=0, ingest="host", histogram=False, burn_in=None, thin=None,
                 samples_per_chain=None, mcmc_thin=None, mcmc_samples_per_chain=None, mcmc_betas=None, mcmc_swap_every=1, elim=False,
                 elim_order=None):
        """histogram=True (sampled handles, n <= 64): the handle holds the distinct configurations with their counts
        (gml_problem_create_sampled_hist: sorted and run-length encoded on the device), not one row per draw.
        burn_in / thin / samples_per_chain (with model=): num_samples // samples_per_chain Glauber chains of a pairwise model on the
        int8 matrix cores, each recorded samples_per_chain times (gml_problem_create_mcmc_chains; defaults 200, 10, 1).
        mcmc_thin / mcmc_samples_per_chain (with terms=; either one, even 1, selects it): num_samples // mcmc_samples_per_chain
        Glauber chains of the term list with exact integer fields, burnt in for mcmc_sweeps sweeps (required) and then recorded every
        mcmc_thin sweeps (gml_problem_create_mcmc_terms_chains; defaults thin 10, samples per chain 1).  mcmc_sweeps alone: one
        sample per chain (gml_problem_create_mcmc_terms).
        mcmc_betas (with terms=; needs mcmc_sweeps): replica exchange -- num_samples // mcmc_samples_per_chain ladders of
        len(mcmc_betas) rungs at these inverse temperatures (non-increasing, the first positive; 1, 2, 4 .. 64 of them), swaps
        between neighbouring rungs every mcmc_swap_every sweeps, rung 0 recorded as above (gml_problem_create_mcmc_terms_tempered).
        The handle's swap_counts is then the (2, R - 1) int64 array of swap attempts and accepts per pair (None otherwise).
        elim=True (with terms=): num_samples exact, independent draws by backward sampling on the tables of variable elimination
        (gml_problem_create_sampled_elim: sparse models of any size, elimination orders of width at most 30); elim_order: a
        permutation of the 1-based spins, or None for the library's greedy order, as in model_elim."""
        L = lib()
        h = C.c_void_p()
        if elim or elim_order is not None:
            if not elim or terms is None or model is not None or samples is not None or spins is not None or packed is not None:
                raise GMLError(GML_EINVAL, "elim / elim_order apply to a term list given as terms= (with elim=True)")
            if mcmc_sweeps or mcmc_thin is not None or mcmc_samples_per_chain is not None or mcmc_betas is not None:
                raise GMLError(GML_EINVAL, "elim=True draws exactly: the mcmc_ arguments do not apply")
            if num_samples is None:
                raise GMLError(GML_EINVAL, "elim=True needs num_samples")
        term_chains = mcmc_thin is not None or mcmc_samples_per_chain is not None or mcmc_betas is not None
        self.swap_counts = None
        if term_chains:
            tc_names = "mcmc_thin / mcmc_samples_per_chain" + (" / mcmc_betas" if mcmc_betas is not None else "")
            if terms is None or model is not None or samples is not None or spins is not None or packed is not None:
                raise GMLError(GML_EINVAL, f"{tc_names} apply to a term list given as terms=")
            if not mcmc_sweeps:
                raise GMLError(GML_EINVAL, f"{tc_names} need mcmc_sweeps (the burn-in)")
            tc_spc = 1 if mcmc_samples_per_chain is None else int(mcmc_samples_per_chain)
            if tc_spc < 1 or num_samples is None or int(num_samples) < 1 or int(num_samples) % tc_spc != 0:
                raise GMLError(GML_EINVAL, f"num_samples must be a positive multiple of mcmc_samples_per_chain ({tc_spc})")
        if burn_in is not None or thin is not None or samples_per_chain is not None:
            if model is None or terms is not None or samples is not None or spins is not None or packed is not None:
                raise GMLError(GML_EINVAL, "burn_in / thin / samples_per_chain apply to a pairwise model given as model=")
            spc = 1 if samples_per_chain is None else int(samples_per_chain)
            if spc < 1 or num_samples is None or int(num_samples) % spc != 0:
                raise GMLError(GML_EINVAL, f"num_samples must be a positive multiple of samples_per_chain ({spc})")
            m = np.ascontiguousarray(model, dtype=np.float64)
            if m.ndim != 2 or m.shape[0] != m.shape[1]:
                raise GMLError(GML_EINVAL, "the model matrix must be square")
            n = m.shape[0]
            n0, n1 = _node_range(node_range, n)
            check(L.gml_problem_create_mcmc_chains(_ptr(m), n, int(num_samples) // spc, spc, int(200 if burn_in is None else burn_in),
                                                   int(10 if thin is None else thin), int(seed), int(bool(histogram)), int(order), n0,
                                                   n1, int(device), C.byref(h)))
            model, histogram = None, False
        if histogram and (samples is not None or spins is not None or packed is not None):
            raise GMLError(GML_EINVAL, "histogram=True applies to handles sampled on the device (model= or terms=)")
        if histogram and model is not None and terms is None:
            # matrix -> terms exactly as gml_problem_create_sampled lists them (row by row, j <= i: the same seed then gives the
            # same draws), with its symmetry check (models.jl:105-134: the matrix of a FactorGraph is symmetric)
            m = np.asarray(model, dtype=np.float64)
            if m.ndim != 2 or m.shape[0] != m.shape[1] or not np.array_equal(m, m.T):
                raise GMLError(GML_EINVAL, "the model matrix is not symmetric")
            terms = {}
            for i in range(m.shape[0]):
                for j in range(i + 1):
                    if m[i, j] != 0.0:
                        terms[(j + 1, i + 1) if j < i else (i + 1,)] = m[i, j]
            n, model = m.shape[0], None
            if not terms:
                terms = {(1,): 0.0}
        if h.value:
            pass  # made above (Glauber chains on the matrix cores)
        elif packed is not None:
            # (sign_bits [n][words] uint32, counts [K] or None, K): the packed form (pack_histogram / sign_bits())
            bits, cnt, K = packed
            bits = np.ascontiguousarray(bits, dtype=np.uint32)
            if cnt is not None:
                cnt = np.ascontiguousarray(cnt, dtype=np.float64)
            n = bits.shape[0]
            n0, n1 = _node_range(node_range, n)
            check(L.gml_problem_create_packed(_ptr(bits), bits.shape[1], _ptr(cnt), int(K), n, int(order), n0, n1, int(device),
                                              C.byref(h)))
        elif terms is not None:
            # sample on the device from a model of any order given as {1-based key tuple: weight}: sampling.jl:60-88
            keys, wts, stride, n = term_arrays(terms, n)
            n0, n1 = _node_range(node_range, n)
            if elim:  # exact draws by backward sampling on the elimination's tables (sparse models of any size)
                check(L.gml_problem_create_sampled_elim(_ptr(keys), stride, _ptr(wts), len(wts), int(n), int(num_samples), int(seed),
                                                        _ptr(_elim_order(elim_order, int(n))), int(bool(histogram)), int(order), n0, n1,
                                                        int(device), C.byref(h)))
            elif mcmc_betas is not None:  # replica exchange on the same chains: ladders of len(betas) rungs, rung 0 recorded
                betas = np.ascontiguousarray(mcmc_betas, dtype=np.float64).ravel()
                swaps = np.zeros((2, max(len(betas) - 1, 0)), dtype=np.int64)
                check(L.gml_problem_create_mcmc_terms_tempered(_ptr(keys), stride, _ptr(wts), len(wts), int(n), int(num_samples) // tc_spc,
                                                               tc_spc, int(mcmc_sweeps), int(10 if mcmc_thin is None else mcmc_thin),
                                                               _ptr(betas), len(betas), int(mcmc_swap_every), int(seed),
                                                               int(bool(histogram)), int(order), n0, n1, int(device), _ptr(swaps),
                                                               C.byref(h)))
                self.swap_counts = swaps
            elif term_chains:  # thinned chains with exact integer fields (any order, any sparsity)
                check(L.gml_problem_create_mcmc_terms_chains(_ptr(keys), stride, _ptr(wts), len(wts), int(n), int(num_samples) // tc_spc,
                                                             tc_spc, int(mcmc_sweeps), int(10 if mcmc_thin is None else mcmc_thin),
                                                             int(seed), int(bool(histogram)), int(order), n0, n1, int(device),
                                                             C.byref(h)))
            elif histogram:
                check(L.gml_problem_create_sampled_hist(_ptr(keys), stride, _ptr(wts), len(wts), int(n), int(num_samples), int(seed),
                                                        int(mcmc_sweeps or 0), int(order), n0, n1, int(device), C.byref(h)))
            elif mcmc_sweeps:  # Glauber chains instead of exact enumeration (components above 22 spins)
                check(L.gml_problem_create_mcmc_terms(_ptr(keys), stride, _ptr(wts), len(wts), int(n), int(num_samples),
                                                      int(seed), int(mcmc_sweeps), int(order), n0, n1, int(device), C.byref(h)))
            else:
                check(L.gml_problem_create_sampled_terms(_ptr(keys), stride, _ptr(wts), len(wts), int(n), int(num_samples),
                                                         int(seed), int(order), n0, n1, int(device), C.byref(h)))
        elif model is not None:
            # sample on the device from a pairwise model (n x n, diagonal = fields): sampling.jl:34-57
            m = np.ascontiguousarray(model, dtype=np.float64)
            n = m.shape[0]
            n0, n1 = _node_range(node_range, n)
            check(L.gml_problem_create_sampled(_ptr(m), n, int(num_samples), int(seed), int(order), n0, n1, int(device),
                                               C.byref(h)))
        elif samples is not None:
            s, dt, K, n, ld, cm = _hist_args(samples)
            n0, n1 = _node_range(node_range, n)
            # ingest: "host" = packed on the host, bits uploaded (default); "device" = raw upload, converted on the device
            create = {"host": L.gml_problem_create, "device": L.gml_problem_create_device_convert}[ingest]
            check(create(_ptr(s), dt, K, n, ld, cm, int(order), n0, n1, int(device), C.byref(h)))
        else:
            spins = np.ascontiguousarray(spins, dtype=np.int8)
            K, n = spins.shape
            if counts is not None:
                counts = np.ascontiguousarray(counts, dtype=np.float64)
            n0, n1 = _node_range(node_range, n)
            check(L.gml_problem_create_spins(_ptr(counts), _ptr(spins), K, n, int(order), n0, n1, int(device),
                                             C.byref(h)))
        self._adopt(h, order)

    def _adopt(self, h, order):
        """take ownership of the handle h (a c_void_p) and read its sizes"""
        self._h = h
        nn, KK, PP, a, b = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        M = C.c_double()
        check(lib().gml_problem_info(h, C.byref(nn), C.byref(KK), C.byref(M), C.byref(PP), C.byref(a), C.byref(b)))
        self.n, self.K, self.M, self.P, self.node0, self.node1 = nn.value, KK.value, M.value, PP.value, a.value, b.value
        self.order = int(order)

    @classmethod
    def _from_handle(cls, h, order):
        """a Problem around a handle the library has already made (split): no creator runs"""
        self = cls.__new__(cls)
        self.swap_counts = None
        self._adopt(h, order)
        return self

    def fold_sizes(self, folds, seed=0):
        """the number of the handle's samples in each of `folds` folds (gml_problem_fold_sizes): int64 [folds], summing to M"""
        out = np.zeros(64, dtype=np.int64)  # (the library refuses folds outside [2, 64] before it writes)
        check(lib().gml_problem_fold_sizes(self._h, int(folds), int(seed), _ptr(out)))
        return out[:int(folds)].copy()

    def split(self, folds, fold, seed=0, complement=False):
        """A new Problem holding the samples of fold `fold` of `folds` (complement=True: all the others), split on the device
        (gml_problem_split; include/gml.h defines the fold of every sample from the seed).  Same device, order and node range;
        independent of this handle, and the same handle as Problem(packed=...) of the selected rows and their new counts."""
        h = C.c_void_p()
        check(lib().gml_problem_split(self._h, int(folds), int(fold), int(seed), int(bool(complement)), C.byref(h)))
        return Problem._from_handle(h, self.order)

    def close(self):
        if getattr(self, "_h", None):
            lib().gml_problem_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def spins(self):
        """the +-1 configurations held by the handle (K x n int8)"""
        out = np.zeros((self.K, self.n), dtype=np.int8)
        check(lib().gml_problem_get_spins(self._h, _ptr(out)))
        return out

    def counts(self):
        """the counts of the handle's K rows (column 1 of the histogram, sampling.jl:54)"""
        out = np.zeros(self.K)
        check(lib().gml_problem_get_counts(self._h, _ptr(out)))
        return out

    def moments(self, pairs=True, raw=False):
        """(m [n], C [n, n]): the sample magnetisations <s_i> and pair correlations <s_i s_j> of the handle (float64 = the exact integer
        sums of gml_problem_moments over M; raw=True: the int64 sums themselves).  pairs=False: C is None and only m is computed.
        Integer counts and M <= 2^50 (GMLError GML_EUNSUPPORTED otherwise); independent of the handle's order and node range."""
        s1 = np.zeros(self.n, dtype=np.int64)
        s2 = np.zeros((self.n, self.n), dtype=np.int64) if pairs else None
        check(lib().gml_problem_moments(self._h, _ptr(s1), _ptr(s2)))
        if raw:
            return s1, s2
        return s1 / self.M, (s2 / self.M if pairs else None)

    def term_moments(self, terms, raw=False):
        """<prod_{i in t} s_i> of every term t of `terms`, in the caller's order (gml_problem_term_moments; raw=True: the int64 sums).
        terms: a dict of 1-based tuples, a list of tuples, a FactorGraph or a TermArray (moment_key_windows).  A spin named twice
        cancels; the empty key gives 1 (raw: M)."""
        out = []
        for keys in moment_key_windows(terms):
            sums = np.zeros(len(keys), dtype=np.int64)
            check(lib().gml_problem_term_moments(self._h, _ptr(keys), keys.shape[1], len(keys), _ptr(sums)))
            out.append(sums)
        sums = np.concatenate(out) if out else np.zeros(0, dtype=np.int64)
        return sums if raw else sums / self.M

    def sign_bits(self):
        """the packed form of the handle's samples: [n][gml_packed_words(K)] uint32, bit set <=> spin -1"""
        out = np.zeros((self.n, lib().gml_packed_words(self.K)), dtype=np.uint32)
        check(lib().gml_problem_get_sign_bits(self._h, _ptr(out)))
        return out

    def ingest_times(self):
        t = np.zeros(6)
        check(lib().gml_problem_ingest_times(self._h, _ptr(t)))
        return {"pack_s": t[0], "upload_s": t[1], "images_s": t[2], "total_s": t[3], "alloc_s": t[4], "weights_s": t[5]}

    def multi_keys(self, u):
        keys = np.zeros((self.P, self.order), dtype=np.int32)
        check(lib().gml_multi_keys(self._h, int(u), _ptr(keys)))
        return [tuple(int(v) for v in row if v >= 0) for row in keys]

    def objgrad(self, formulation, nodes, theta, precision="auto", want_grad=True):
        nodes = np.ascontiguousarray(nodes, dtype=np.int64)
        theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(len(nodes), -1)
        f = np.zeros(len(nodes))
        g = np.zeros_like(theta) if want_grad else None
        check(lib().gml_objgrad_batch(self._h, FORMULATION_IDS[formulation], PRECISIONS[precision], len(nodes),
                                      _ptr(nodes), _ptr(theta), theta.shape[1], _ptr(f), _ptr(g)))
        return f, g

    def objgrad_device(self, formulation, nodes, theta_ptr, ld, f_ptr, g_ptr=None, precision="auto"):
        """gml_objgrad_batch on rows resident in HBM: theta_ptr / f_ptr / g_ptr are device addresses (ints: tensor.data_ptr()) of
        [len(nodes), ld], [len(nodes)] and [len(nodes), ld] float64 arrays on the handle's GPU; nothing is staged through the host.
        Ordered after the caller's work on the device's null stream; returns when f and g are written."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int64)
        check(lib().gml_objgrad_batch(self._h, FORMULATION_IDS[formulation], PRECISIONS[precision], len(nodes), _ptr(nodes),
                                      C.c_void_p(int(theta_ptr)), int(ld), C.c_void_p(int(f_ptr)),
                                      C.c_void_p(int(g_ptr)) if g_ptr else None))

    def hessvec_device(self, formulation, nodes, theta_ptr, vec_ptr, ld, hv_ptr, precision="i8x"):
        """gml_hessvec_batch_prec on rows resident in HBM (device addresses, as objgrad_device)"""
        nodes = np.ascontiguousarray(nodes, dtype=np.int64)
        check(lib().gml_hessvec_batch_prec(self._h, FORMULATION_IDS[formulation], PRECISIONS[precision], len(nodes), _ptr(nodes),
                                           C.c_void_p(int(theta_ptr)), C.c_void_p(int(vec_ptr)), int(ld), C.c_void_p(int(hv_ptr))))

    def hessvec(self, formulation, nodes, theta, vec, precision="i8x"):
        """Hess f_u(theta) @ vec for the listed nodes (gml_hessvec_batch_prec): "i8x" = int8-limb passes (~1e-8), "f64" = FP64 MFMA."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int64)
        theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(len(nodes), -1)
        vec = np.ascontiguousarray(vec, dtype=np.float64).reshape(len(nodes), -1)
        out = np.zeros_like(theta)
        check(lib().gml_hessvec_batch_prec(self._h, FORMULATION_IDS[formulation], PRECISIONS[precision], len(nodes), _ptr(nodes), _ptr(theta),
                                           _ptr(vec), theta.shape[1], _ptr(out)))
        return out

    def learn(self, formulation, c, *, tol=1e-9, max_iter=100, precision="auto", max_working=512, max_add=64,
              verbose=0, hess_samples=0, polish=True, max_cg=0, limbs_fwd=0, hv_limbs_fwd=0, hv_limbs_bwd=0, debug_row=0,
              hv_subsample=0, cg_viol_frac=0.0, cg_eta=0.0, coarse=True, out_ptr=None, raise_on_fail=True, terms=None, x0=None, matrix=None,
              structure=None):
        """gml_learn: (rows, kkt, stats).  terms = True / False (handles over all nodes): gml_learn_terms instead -- the solved
        rows stay on the device and the first result is the model's weight array in (length, key) order, symmetrised (True) or
        not (False): the input of a FactorGraph (TermArray).  x0: rows to start from ((node1-node0) x P, the layout of the result;
        gml_learn_warm) -- a regularisation path solves each c from the previous solution.  matrix = True / False (pairwise handles
        over all nodes): gml_learn_matrix -- the n x n result, symmetrised on the device (True) or as it is (False).
        structure: uint8 (node1-node0) x P, the kind of every parameter slot in the layout of the result -- EXCLUDED (fixed at 0), FREE
        (estimated, no penalty) or PENALISED (gml_learn_structured; structure_from_rows / structure_from_keys build one); combines
        with x0, not with terms or matrix."""
        L = lib()
        o = Opts()
        L.gml_default_opts(C.byref(o))
        o.tol, o.max_iter, o.precision = float(tol), int(max_iter), PRECISIONS[precision]
        o.max_working, o.max_add, o.verbose = int(max_working), int(max_add), int(verbose)
        o.hess_samples = int(hess_samples)
        o.polish = 0 if polish else -1
        o.max_cg = int(max_cg)
        o.limbs_fwd, o.hv_limbs_fwd, o.hv_limbs_bwd, o.debug_row = int(limbs_fwd), int(hv_limbs_fwd), int(hv_limbs_bwd), int(debug_row)
        o.cg_viol_frac, o.cg_eta, o.hv_subsample = float(cg_viol_frac), float(cg_eta), int(hv_subsample)
        # precision i8w: early iterations in the cheap 30 / 23-bit form of the pass (True), never (False), or until KKT 10^-coarse
        o.coarse = (0 if coarse else -1) if isinstance(coarse, bool) else int(coarse)
        R = self.node1 - self.node0
        out = None
        kkt = np.zeros(R)
        st = Stats()
        if matrix is not None and (terms is not None or x0 is not None or out_ptr is not None):
            raise GMLError(GML_EINVAL, "matrix (gml_learn_matrix) cannot be combined with terms, x0 or out_ptr")
        if terms is not None and x0 is not None:
            raise GMLError(GML_EINVAL, "x0 (gml_learn_warm) and terms (gml_learn_terms) cannot be combined: solve with x0, then terms_assemble")
        if structure is not None:
            if terms is not None or matrix is not None:
                raise GMLError(GML_EINVAL, "structure (gml_learn_structured) cannot be combined with terms or matrix: solve, then assemble the rows")
            structure = np.asarray(structure)
            if structure.dtype != np.uint8 or structure.shape != (R, self.P):
                raise GMLError(GML_EINVAL, f"structure is {structure.dtype} {structure.shape}, the handle's rows take uint8 {(R, self.P)}")
            structure = np.ascontiguousarray(structure)
        if matrix is not None:
            out = np.zeros((R, self.P))
            rc = L.gml_learn_matrix(self._h, FORMULATION_IDS[formulation], float(c), int(bool(matrix)), C.byref(o), _ptr(out), _ptr(kkt),
                                    C.byref(st))
        elif terms is not None:
            out = np.empty(terms_count(self.n, self.order, terms))
            rc = L.gml_learn_terms(self._h, FORMULATION_IDS[formulation], float(c), int(bool(terms)), C.byref(o), _ptr(out), _ptr(kkt),
                                   C.byref(st))
        else:
            if out_ptr is None:
                out = np.zeros((R, self.P))
                out_ptr = _ptr(out)
            if x0 is not None:
                x0 = np.ascontiguousarray(x0, dtype=np.float64)
                if x0.shape != (R, self.P):
                    raise GMLError(GML_EINVAL, f"x0 has shape {x0.shape}, the handle's rows are {(R, self.P)}")
            if structure is not None:
                rc = L.gml_learn_structured(self._h, FORMULATION_IDS[formulation], float(c), C.byref(o), _ptr(structure), self.P, _ptr(x0),
                                            out_ptr, _ptr(kkt), C.byref(st))
            elif x0 is not None:
                rc = L.gml_learn_warm(self._h, FORMULATION_IDS[formulation], float(c), C.byref(o), _ptr(x0), out_ptr, _ptr(kkt), C.byref(st))
            else:
                rc = L.gml_learn(self._h, FORMULATION_IDS[formulation], float(c), C.byref(o), out_ptr, _ptr(kkt), C.byref(st))
        if rc == GML_ENOTCONV:
            if raise_on_fail:
                err = GMLConvergenceError(L.gml_last_error().decode())
                err.stats, err.kkt = st.asdict(), kkt  # what the solver reached, for the caller's diagnostics
                raise err
        else:
            check(rc)
        return out, kkt, st.asdict()

    def stderr(self, formulation, rows, structure=None):
        """gml_stderr: (se, status) of the solved rows `rows` ((node1-node0) x P, the layout of learn's result) -- the M-estimator
        ("sandwich") standard error of every parameter of the support (FREE slots, PENALISED slots with rows != 0; structure as in
        learn, None = the field free, the rest penalised), 0.0 elsewhere; status per row: 0 ok, 1 singular support (se NaN there), 2 a
        support of more than 512 entries (NaN).  Conditional on the support; meant for refitted rows (include/gml.h)."""
        R = self.node1 - self.node0
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.shape != (R, self.P):
            raise GMLError(GML_EINVAL, f"rows have shape {rows.shape}, the handle's rows are {(R, self.P)}")
        if structure is not None:
            structure = np.asarray(structure)
            if structure.dtype != np.uint8 or structure.shape != (R, self.P):
                raise GMLError(GML_EINVAL, f"structure is {structure.dtype} {structure.shape}, the handle's rows take uint8 {(R, self.P)}")
            structure = np.ascontiguousarray(structure)
        se = np.zeros((R, self.P))
        status = np.zeros(R, dtype=np.int32)
        check(lib().gml_stderr(self._h, FORMULATION_IDS[formulation], _ptr(rows), self.P, _ptr(structure), self.P, _ptr(se), _ptr(status),
                               None))
        return se, status

    def multi_keys_array(self, u):
        """gml_multi_keys as it comes: int32 [P, order], 0-based, -1 = unused slot"""
        keys = np.zeros((self.P, self.order), dtype=np.int32)
        check(lib().gml_multi_keys(self._h, int(u), _ptr(keys)))
        return keys

    def bench_pass(self, formulation, theta=None, steps=5, warmup=1, precision="f64"):
        ms = np.zeros(3)
        th = None if theta is None else np.ascontiguousarray(theta, dtype=np.float64)
        check(lib().gml_bench_pass(self._h, FORMULATION_IDS[formulation], PRECISIONS[precision], _ptr(th), int(steps),
                                   int(warmup), _ptr(ms)))
        return {"fwd_ms": ms[0], "bwd_ms": ms[1], "pass_ms": ms[2]}

    def bench_pass_resident(self, formulation, theta, steps=5, warmup=1, precision="f64", want_output=False):
        """Theta uploaded once, then warmup + steps passes back to back with no host round trip
        (gml_bench_pass_resident).  Returns the kernel times and, if asked, (f, g) of the last pass."""
        ms = np.zeros(4)
        th = np.ascontiguousarray(theta, dtype=np.float64)
        nloc = self.node1 - self.node0
        f = np.zeros(nloc) if want_output else None
        g = np.zeros((nloc, self.P)) if want_output else None
        step = np.zeros(int(steps))
        check(lib().gml_bench_pass_resident(self._h, FORMULATION_IDS[formulation], PRECISIONS[precision], _ptr(th), int(steps),
                                            int(warmup), _ptr(ms), _ptr(f), _ptr(g), _ptr(step)))
        out = {"fwd_ms": ms[0], "bwd_ms": ms[1], "pass_ms": ms[2], "device_ms_per_pass": ms[3], "step_ms": step}
        return (out, f, g) if want_output else out


def conditional_chains(terms, n, evidence, hidden, replicas=1, samples_per_chain=1, burn_in=200, thin=10, seed=0, *, means=False,
                       order=2, node_range=None):
    """The conditional chains of a term list as term_arrays takes it (include/gml.h): evidence an open Problem, hidden the 0-BASED
    hidden spins.  means=False: gml_problem_create_mcmc_terms_conditional, a Problem of K replicas samples_per_chain rows (row
    (t, r, k) at (t replicas + r) K + k) on the evidence's device.  means=True: gml_conditional_means, float64 [H, K replicas], the
    hidden spins in ascending order."""
    keys, wts, stride, n = term_arrays(terms, n)
    mask = np.zeros(max(int(n), 0), dtype=np.uint8)
    hidden = np.asarray(hidden, dtype=np.int64).ravel()
    if len(hidden) and (hidden.min() < 0 or hidden.max() >= n):
        raise GMLError(GML_EINVAL, f"a hidden spin lies outside [0, {int(n)})")
    mask[hidden] = 1
    common = (_ptr(keys), stride, _ptr(wts), len(wts), int(n), evidence._h, _ptr(mask), int(replicas), int(samples_per_chain), int(burn_in),
              int(thin), int(seed))
    if means:
        out = np.zeros((int(mask.sum()), evidence.K * max(int(replicas), 0)))
        check(lib().gml_conditional_means(*common, _ptr(out)))
        return out
    h = C.c_void_p()
    n0, n1 = _node_range(node_range, n)
    check(lib().gml_problem_create_mcmc_terms_conditional(*common, int(order), n0, n1, C.byref(h)))
    return Problem._from_handle(h, order)


def conditional_chains_masked(terms, n, evidence, mask, replicas=1, samples_per_chain=1, burn_in=200, thin=10, seed=0, *, means=False,
                              order=2, node_range=None):
    """The conditional chains whose hidden set is a property of the row (include/gml.h): evidence and mask two open Problems of the same
    n, K and device; a -1 in row k of the mask hides that spin in row k of the evidence.  means=False:
    gml_problem_create_mcmc_terms_masked, a Problem of K replicas samples_per_chain rows (row (t, r, k) at (t replicas + r) K + k).
    means=True: gml_conditional_means_masked, float64 [n, K replicas] (observed entries hold the evidence value)."""
    keys, wts, stride, n = term_arrays(terms, n)
    common = (_ptr(keys), stride, _ptr(wts), len(wts), int(n), evidence._h, mask._h, int(replicas), int(samples_per_chain), int(burn_in),
              int(thin), int(seed))
    if means:
        out = np.zeros((max(int(n), 0), evidence.K * max(int(replicas), 0)))
        check(lib().gml_conditional_means_masked(*common, _ptr(out)))
        return out
    h = C.c_void_p()
    n0, n1 = _node_range(node_range, n)
    check(lib().gml_problem_create_mcmc_terms_masked(*common, int(order), n0, n1, C.byref(h)))
    return Problem._from_handle(h, order)


def conditional_exact(terms, n, evidence, hidden, *, means=True, log_w=True, log_p=True):
    """gml_conditional_exact on a term list as term_arrays takes it: evidence an open Problem, hidden the 0-BASED hidden spins, the same
    in every row (at most 24).  Returns (means float64 [H, K], the hidden spins ascending; log_w [K]; log_p [K]), None for what was
    not asked for: exact conditional means, log sum_{s_H} exp E and the conditional log-probability of the values the evidence holds on
    the hidden spins, by enumeration on the evidence's device."""
    keys, wts, stride, n = term_arrays(terms, n)
    mask = np.zeros(max(int(n), 0), dtype=np.uint8)
    hidden = np.asarray(hidden, dtype=np.int64).ravel()
    if len(hidden) and (hidden.min() < 0 or hidden.max() >= n):
        raise GMLError(GML_EINVAL, f"a hidden spin lies outside [0, {int(n)})")
    mask[hidden] = 1
    m = np.zeros((int(mask.sum()), evidence.K)) if means else None
    lw = np.zeros(evidence.K) if log_w else None
    lp = np.zeros(evidence.K) if log_p else None
    check(lib().gml_conditional_exact(_ptr(keys), stride, _ptr(wts), len(wts), int(n), evidence._h, _ptr(mask), _ptr(m), _ptr(lw), _ptr(lp)))
    return m, lw, lp


def conditional_exact_masked(terms, n, evidence, mask, *, means=True, log_w=True, log_p=True):
    """gml_conditional_exact_masked: evidence and mask two open Problems of the same n, K and device; a -1 in row k of the mask hides that
    spin in row k of the evidence (at most 24 per row).  Returns (means float64 [n, K], observed entries holding the evidence value;
    log_w [K]; log_p [K]), None for what was not asked for."""
    keys, wts, stride, n = term_arrays(terms, n)
    m = np.zeros((max(int(n), 0), evidence.K)) if means else None
    lw = np.zeros(evidence.K) if log_w else None
    lp = np.zeros(evidence.K) if log_p else None
    check(lib().gml_conditional_exact_masked(_ptr(keys), stride, _ptr(wts), len(wts), int(n), evidence._h, mask._h, _ptr(m), _ptr(lw),
                                             _ptr(lp)))
    return m, lw, lp


def conditional_mode(terms, n, evidence, hidden, *, energy=True, log_p=True):
    """gml_conditional_mode on a term list as term_arrays takes it: evidence an open Problem, hidden the 0-BASED hidden spins, the same
    in every row (at most 24).  Returns (states int8 [H, K], the hidden spins ascending; energy [K]; log_p [K]), None for what was not
    asked for: every row's most probable joint state of the hidden spins, its energy E_k and its conditional log-probability, by
    enumeration on the evidence's device.  Without log_p the device computes no exponential."""
    keys, wts, stride, n = term_arrays(terms, n)
    mask = np.zeros(max(int(n), 0), dtype=np.uint8)
    hidden = np.asarray(hidden, dtype=np.int64).ravel()
    if len(hidden) and (hidden.min() < 0 or hidden.max() >= n):
        raise GMLError(GML_EINVAL, f"a hidden spin lies outside [0, {int(n)})")
    mask[hidden] = 1
    st = np.zeros((int(mask.sum()), evidence.K), dtype=np.int8)
    en = np.zeros(evidence.K) if energy else None
    lp = np.zeros(evidence.K) if log_p else None
    check(lib().gml_conditional_mode(_ptr(keys), stride, _ptr(wts), len(wts), int(n), evidence._h, _ptr(mask), _ptr(st), _ptr(en), _ptr(lp)))
    return st, en, lp


def conditional_mode_masked(terms, n, evidence, mask, *, energy=True, log_p=True):
    """gml_conditional_mode_masked: evidence and mask two open Problems of the same n, K and device; a -1 in row k of the mask hides that
    spin in row k of the evidence (at most 24 per row).  Returns (states int8 [n, K], observed entries holding the evidence value;
    energy [K]; log_p [K]), None for what was not asked for."""
    keys, wts, stride, n = term_arrays(terms, n)
    st = np.zeros((max(int(n), 0), evidence.K), dtype=np.int8)
    en = np.zeros(evidence.K) if energy else None
    lp = np.zeros(evidence.K) if log_p else None
    check(lib().gml_conditional_mode_masked(_ptr(keys), stride, _ptr(wts), len(wts), int(n), evidence._h, mask._h, _ptr(st), _ptr(en),
                                            _ptr(lp)))
    return st, en, lp


def conditional_draw(terms, n, evidence, hidden, replicas=1, seed=0, *, energy=True, log_p=True):
    """gml_conditional_draw on a term list as term_arrays takes it: evidence an open Problem, hidden the 0-BASED hidden spins, the same
    in every row (at most 24).  Returns (states int8 [H, K replicas], the hidden spins ascending, chain r K + k replica r of row k;
    energy [K replicas], the unperturbed energy of every draw; log_p [K replicas]), None for what was not asked for: exact draws of
    every row's hidden spins given its visible ones, by enumeration on the evidence's device (Gumbel-max, no chain).  Without log_p the
    device computes no exponential of the sums; states and energy are the same bytes either way."""
    keys, wts, stride, n = term_arrays(terms, n)
    mask = np.zeros(max(int(n), 0), dtype=np.uint8)
    hidden = np.asarray(hidden, dtype=np.int64).ravel()
    if len(hidden) and (hidden.min() < 0 or hidden.max() >= n):
        raise GMLError(GML_EINVAL, f"a hidden spin lies outside [0, {int(n)})")
    mask[hidden] = 1
    chains = evidence.K * max(int(replicas), 0)
    st = np.zeros((int(mask.sum()), chains), dtype=np.int8)
    en = np.zeros(chains) if energy else None
    lp = np.zeros(chains) if log_p else None
    check(lib().gml_conditional_draw(_ptr(keys), stride, _ptr(wts), len(wts), int(n), evidence._h, _ptr(mask), int(replicas),
                                     int(seed), _ptr(st), _ptr(en), _ptr(lp)))
    return st, en, lp


def conditional_draw_masked(terms, n, evidence, mask, replicas=1, seed=0, *, energy=True, log_p=True):
    """gml_conditional_draw_masked: evidence and mask two open Problems of the same n, K and device; a -1 in row k of the mask hides that
    spin in row k of the evidence (at most 24 per row).  Returns (states int8 [n, K replicas], observed entries holding the evidence
    value; energy [K replicas]; log_p [K replicas]), None for what was not asked for."""
    keys, wts, stride, n = term_arrays(terms, n)
    chains = evidence.K * max(int(replicas), 0)
    st = np.zeros((max(int(n), 0), chains), dtype=np.int8)
    en = np.zeros(chains) if energy else None
    lp = np.zeros(chains) if log_p else None
    check(lib().gml_conditional_draw_masked(_ptr(keys), stride, _ptr(wts), len(wts), int(n), evidence._h, mask._h, int(replicas),
                                            int(seed), _ptr(st), _ptr(en), _ptr(lp)))
    return st, en, lp


def moments(samples_or_problem, terms=None, raw=False, device=0):
    """Sample moments of a K x (1+n) histogram matrix (a handle is built and closed) or of an open Problem: (m, C) as
    Problem.moments, or with terms= the per-term expectations of Problem.term_moments."""
    if isinstance(samples_or_problem, Problem):
        p = samples_or_problem
        return p.moments(raw=raw) if terms is None else p.term_moments(terms, raw=raw)
    with Problem(samples_or_problem, device=device) as p:
        return p.moments(raw=raw) if terms is None else p.term_moments(terms, raw=raw)


class MultiProblem:
    """One problem on several GPUs of this node from one process (gml_multi_*): GPU g owns the nodes [g n/G, (g+1) n/G),
    one host thread per device inside the library; what the Julia wrapper's HIP(devices = ...) binds."""

    def __init__(self, samples, devices, order=2):
        L = lib()
        s, dt, K, n, ld, cm = _hist_args(samples)
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        check(L.gml_multi_create(_ptr(s), dt, K, n, ld, cm, int(order), _ptr(dev), len(dev), C.byref(h)))
        self._h = h
        nn, KK, PP, nd = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        M = C.c_double()
        check(L.gml_multi_info(h, C.byref(nn), C.byref(KK), C.byref(M), C.byref(PP), C.byref(nd), None))
        self.n, self.K, self.M, self.P, self.ndev = nn.value, KK.value, M.value, PP.value, nd.value
        self.devices = [int(v) for v in dev]

    def part_stats(self):
        """statistics of every part (node shard) of the last learn(): list of dicts"""
        arr = (Stats * self.ndev)()
        check(lib().gml_multi_part_stats(self._h, arr))
        return [a.asdict() for a in arr]

    def diag(self):
        """how the RCCL communicators came about and which path the last gather took (gml_multi_diag)"""
        buf = C.create_string_buffer(256)
        check(lib().gml_multi_diag(self._h, buf, 256))
        return buf.value.decode()

    def gather_kind(self):
        buf = C.create_string_buffer(32)
        check(lib().gml_multi_info(self._h, None, None, None, None, None, buf))
        return buf.value.decode()

    def close(self):
        if getattr(self, "_h", None):
            lib().gml_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def learn(self, formulation, c, *, tol=1e-9, max_iter=100, precision="auto", max_working=512, max_add=64, verbose=0,
              hess_samples=0, polish=True, dev_out=None, raise_on_fail=True):
        """dev_out: optional list of device pointers (ints), one per part, each an n x P float64 buffer on that part's GPU;
        the gathered matrix is left in all of them (RCCL all-gather)."""
        L = lib()
        o = Opts()
        L.gml_default_opts(C.byref(o))
        o.tol, o.max_iter, o.precision = float(tol), int(max_iter), PRECISIONS[precision]
        o.max_working, o.max_add, o.verbose, o.hess_samples = int(max_working), int(max_add), int(verbose), int(hess_samples)
        o.polish = 0 if polish else -1
        out = np.zeros((self.n, self.P))
        kkt = np.zeros(self.n)
        st = Stats()
        dptr = None
        if dev_out is not None:
            dptr = (C.c_void_p * self.ndev)(*[C.c_void_p(int(v)) for v in dev_out])
        rc = L.gml_multi_learn(self._h, FORMULATION_IDS[formulation], float(c), C.byref(o), _ptr(out), _ptr(kkt), C.byref(st), dptr)
        if rc == GML_ENOTCONV:
            if raise_on_fail:
                err = GMLConvergenceError(L.gml_last_error().decode())
                err.stats, err.kkt = st.asdict(), kkt
                raise err
        else:
            check(rc)
        return out, kkt, st.asdict()
