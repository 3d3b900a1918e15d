"""numpy restatement of gml_problem_fold_sizes / gml_problem_split (include/gml.h): the handle's M samples are its units, unit g of
configuration k (g = C_k .. C_k + c_k - 1, C the exclusive prefix sum of the counts) lies in fold
min(nfolds - 1, floor(nfolds u01(seed, kU01FoldStream, g))), and a part of the split is the rows with a positive new count, in source
order, with their sign bits re-packed."""
import numpy as np

from _mcmc_chains_reference import u01

FOLD_STREAM = 0x8000000000000000  # kU01FoldStream (gml_rng.h)


def unit_folds(M, nfolds, seed):
    """fold of every unit g = 0 .. M - 1 (int64 [M])"""
    u = u01(seed, FOLD_STREAM, np.arange(int(M), dtype=np.uint64))
    return np.minimum(nfolds - 1, np.floor(nfolds * u).astype(np.int64))


def fold_table(counts, nfolds, seed):
    """T [K, nfolds]: the number of units of configuration k in fold f"""
    c = np.asarray(counts)
    assert np.array_equal(c, np.rint(c)) and (c >= 0).all()
    c = c.astype(np.int64)
    labels = unit_folds(c.sum(), nfolds, seed)
    owner = np.repeat(np.arange(len(c)), c)
    T = np.zeros((len(c), nfolds), dtype=np.int64)
    np.add.at(T, (owner, labels), 1)
    return T


def fold_sizes(counts, nfolds, seed):
    return fold_table(counts, nfolds, seed).sum(axis=0)


def new_counts(counts, nfolds, fold, seed, complement):
    """c'_k of every source row (zeros included)"""
    T = fold_table(counts, nfolds, seed)
    return T.sum(axis=1) - T[:, fold] if complement else T[:, fold].copy()


def pack_bits(spins):
    """K x n +-1 -> sign words [n][round_up(K, 1024) / 32] uint32 (bit j of word w <-> row 32 w + j, set <=> -1)"""
    S = np.asarray(spins)
    K, n = S.shape
    Kp = (K + 1023) // 1024 * 1024
    b = np.zeros((n, Kp), dtype=np.uint32)
    b[:, :K] = (S.T < 0)
    return (b.reshape(n, Kp // 32, 32) << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint64).astype(np.uint32)


def unpack_bits(bits, K):
    """sign words -> K x n +-1 int8"""
    n = bits.shape[0]
    sp = ((bits[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(n, -1)[:, :K].T
    return (1 - 2 * sp.astype(np.int8)).astype(np.int8)


def split(spins, counts, nfolds, fold, seed, complement):
    """(rows kept [K'], counts' [K'] float64, bits' [n][words'] uint32, K') of one part; K' = 0: the part is empty"""
    cn = new_counts(counts, nfolds, fold, seed, complement)
    rows = np.flatnonzero(cn > 0)
    S = np.asarray(spins)[rows]
    bits = pack_bits(S) if len(rows) else np.zeros((np.asarray(spins).shape[1], 0), dtype=np.uint32)
    return rows, cn[rows].astype(np.float64), bits, len(rows)
