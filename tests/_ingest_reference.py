"""One model of what a handle holds after ANY creation route (csrc/gml_ingest.cpp): the sign bits Sb, the sum of counts M, the
weights w = counts / M and the host-side summaries of them (wmax, wuni, counts_int, wblk), and of what a faulty input is answered
with.  Plain numpy and Python floats, no GPU, no library.  tests/test_host_ingest_reference.py holds the model to the host packer,
tests/test_gpu_ingest_state.py every route into a handle to the model."""
import numpy as np

GML_EINVAL = 1
DTYPE_IDS = {np.dtype(np.int8): 0, np.dtype(np.int32): 1, np.dtype(np.int64): 2, np.dtype(np.float64): 3}
SUM_BLOCK = 65536  # M is summed in blocks of this many counts (include/gml.h, next to gml_pack_histogram)


def numpy_pack(spins):
    """spins K x n in {-1,+1} -> [n][round_up(K,1024)/32] uint32: bit j of word w <-> configuration 32 w + j, set <=> -1"""
    K, n = spins.shape
    Kp = (K + 1023) // 1024 * 1024
    neg = np.zeros((n, Kp), dtype=np.uint8)
    neg[:, :K] = (spins.T < 0)
    return np.packbits(neg.reshape(n, Kp // 32, 32), axis=2, bitorder="little").view(np.uint32).reshape(n, Kp // 32)


def sum_left_to_right(values):
    s = 0.0
    for v in values.tolist():
        s += v
    return s


def blocked_sum(counts):
    """THE definition of M: blocks of 65 536 counts summed left to right, then the partial sums added left to right"""
    c = np.asarray(counts, dtype=np.float64)
    M = 0.0
    for b in range(0, len(c), SUM_BLOCK):
        M += sum_left_to_right(c[b:b + SUM_BLOCK])
    return M


def handle_state(counts, spins):
    """counts: float64 [K] or None (all ones); spins: K x n in {-1, +1}.  The resident state of the handle as a dict:
    Sb uint32 [n][Kp / 32], M, w float64 [Kp] (0.0 on the padding rows), wmax, wuni, counts_int, wblk float64 [Kp / 512]."""
    spins = np.asarray(spins)
    K = spins.shape[0]
    Kp = (K + 1023) // 1024 * 1024
    given = counts is not None
    c = np.asarray(counts, dtype=np.float64) if given else np.ones(K)
    assert c.shape == (K,)
    M = blocked_sum(c)
    w = np.zeros(Kp)
    w[:K] = c / M  # one IEEE division per row
    wblk = np.zeros(Kp // 512)
    for j in range(len(wblk)):
        wblk[j] = sum_left_to_right(w[512 * j:min(512 * j + 512, K)])
    return {
        "Sb": numpy_pack(spins),
        "M": M,
        "w": w,
        "wmax": float(w[:K].max()),
        "wuni": float(w[0]) if bool(np.all(w[:K] == w[0])) else 0.0,
        "counts_int": bool(np.all(c == np.rint(c))) if given else True,
        "wblk": wblk,
    }


def spin_ok(v):
    return bool(v == 1) or bool(v == -1)  # (-0.0, NaN, +-inf, nextafter(+-1) and 257 are all neither)


def refusal(matrix, *, K=None, n=None, dtype=None, ld=None, col_major=None):
    """(code, text) a K x (1+n) histogram `matrix` (column 0 = counts) is refused with by gml_problem_create,
    gml_problem_create_device_convert and gml_pack_histogram, or None if it is accepted.  K, n, dtype (the id), ld and col_major
    default to what the matrix is; a test of the argument checks overrides them.  ONE precedence: the argument checks, then the
    first bad count, then a zero sum of counts, then the first bad spin = the smallest configuration index over all columns."""
    m = np.asarray(matrix)
    K = m.shape[0] if K is None else K
    n = m.shape[1] - 1 if n is None else n
    dtype = DTYPE_IDS[m.dtype] if dtype is None else dtype
    col_major = bool(m.flags.f_contiguous and not m.flags.c_contiguous) if col_major is None else bool(col_major)
    ld = (K if col_major else n + 1) if ld is None else ld
    if K <= 0 or n <= 0:
        return GML_EINVAL, f"empty histogram (K={K}, n={n})"
    if dtype not in (0, 1, 2, 3):
        return GML_EINVAL, f"unknown dtype {dtype}"
    if ld < (K if col_major else n + 1):
        return GML_EINVAL, f"leading dimension {ld} too small"
    c = m[:K, 0].astype(np.float64)
    bad = np.flatnonzero(~(c >= 0) | ~np.isfinite(c))
    if len(bad):
        return GML_EINVAL, f"count of configuration {int(bad[0])} is negative or not finite"
    if not blocked_sum(c) > 0:
        return GML_EINVAL, "sum of counts is zero"
    s = m[:K, 1:n + 1]
    rows = np.flatnonzero(~((s == 1) | (s == -1)).all(axis=1))
    if len(rows):
        return GML_EINVAL, f"configuration {int(rows[0])} holds a spin that is not +-1"
    return None


# ---- the count kinds of the tests (all float64 [K], or None) ------------------------------------------------------------------
def fractional_counts(K, seed):
    return 3.0 * np.random.default_rng(seed).random(K)


# Fractional cases whose M tells the two summation orders apart: tests/test_host_ingest_reference.py asserts, on this model alone,
# that blocked_sum differs from the plain left-to-right sum for each of them (K = 65 536 and 65 537 cannot: one block, and one
# block plus one count, are left-to-right sums).  The GPU tests of route equality take their fractional inputs from here.
ORDER_TELLING = {"random": (70001, 1), "uniform": (70001, 0.3)}


def order_telling_counts(kind):
    K, v = ORDER_TELLING[kind]
    return fractional_counts(K, v) if kind == "random" else np.full(K, v)


def count_kinds(K, seed=0):
    """{name: counts} of the kinds a handle's weights are tested with at K rows"""
    rng = np.random.default_rng(1000 + seed)
    small = rng.integers(0, 5, size=K).astype(np.float64)
    small[0] = 2.0  # (never all zero)
    if K > 2:
        small[1] = 0.0
    single = np.zeros(K)
    single[K // 2] = 5.0
    big = rng.integers(2 ** 31 + 1, 2 ** 33, size=K).astype(np.float64)
    pow50 = np.full(K, float(2 ** 50 // K))  # integers summing to exactly 2^50: the edge of the exactness contract
    pow50[K - 1] += float(2 ** 50 - (2 ** 50 // K) * K)
    return {
        "small_int_with_zeros": small,
        "ones": np.ones(K),
        "threes": np.full(K, 3.0),
        "uniform_0.3": np.full(K, 0.3),
        "fractional": fractional_counts(K, 1),
        "single_nonzero": single,
        "int64_above_2^31": big,
        "M_2^50": pow50,
    }
