"""Dense numpy FP64 model of gml_stderr (include/gml.h): the M-estimator ("sandwich") covariance of one node's solve.

For node u with parameters x on the support S, statistics s_k = nodal_stat[k, S] (GraphicalModelLearning.jl:162; multi-body
:106-108), a_k = x . s_k, w_k = count_k / M:

                 phi'' weight (A)                          score psi_k
    RISE         e_k = exp(-a_k)                           -e_k s_k
    RPLE         4 sg_k (1 - sg_k), sg = 1/(1+exp(-2a))    -2 (1 - sg_k) s_k
    logRISE      A = (sum w e s s^T)/Z - gb gb^T,          -(e_k / Z)(s_k + gb)
                 Z = sum w e, gb = -(sum w e s)/Z

    A = sum_k w_k phi''_k s_k s_k^T,  B = sum_k w_k psi_k psi_k^T - m m^T,  m = sum_k w_k psi_k,
    C = A^-1 B A^-1 / M,  se_j = sqrt(C_jj).

Written from the formulas alone: it shares no code with the kernels, and nodal_stat is built as the reference's lines build it."""
import numpy as np


def nodal_stat(spins, u, keys=None):
    """[K, P]: pairwise (:162) column j = s_u (j == u) or s_u s_j; multi-body (:106-108) column j = prod of the spins of keys[j]
    (0-based tuples that start with u)"""
    spins = np.asarray(spins, dtype=np.float64)
    if keys is None:
        n = spins.shape[1]
        return np.stack([spins[:, u] if j == u else spins[:, u] * spins[:, j] for j in range(n)], axis=1)
    return np.stack([np.prod(spins[:, [i for i in key if i >= 0]], axis=1) for key in keys], axis=1)


def scores(form, w, s, x):
    """(per-sample A-weights phi'' (None for logRISE), per-sample scores psi [K, m]); s = the statistics on the support"""
    a = s @ x
    if form == "RISE":
        e = np.exp(-a)
        return e, -e[:, None] * s
    if form == "RPLE":
        sg = 1.0 / (1.0 + np.exp(-2.0 * a))
        return 4.0 * sg * (1.0 - sg), -2.0 * (1.0 - sg)[:, None] * s
    if form == "logRISE":
        e = np.exp(-a)
        Z = np.sum(w * e)
        gb = -(w * e) @ s / Z
        return None, -(e / Z)[:, None] * (s + gb[None, :])
    raise ValueError(form)


def sandwich(form, counts, spins, u, x, support, keys=None):
    """A, B, g, se, cond2(A) for node u; x: the full parameter row (reference layout), support: the slots of S in ascending order.
    g is the gradient on S (logRISE: grad log Z); se has the length of the support."""
    counts = np.asarray(counts, dtype=np.float64)
    M = counts.sum()
    w = counts / M
    support = np.asarray(support, dtype=np.int64)
    s = nodal_stat(spins, u, keys)[:, support]
    xs = np.asarray(x, dtype=np.float64)[support]
    h, psi = scores(form, w, s, xs)
    if form == "logRISE":
        e = np.exp(-(s @ xs))
        Z = np.sum(w * e)
        gb = -(w * e) @ s / Z
        A = (s.T * (w * e)) @ s / Z - np.outer(gb, gb)
        g = gb
    else:
        A = (s.T * (w * h)) @ s
        g = w @ psi
    m = w @ psi
    B = (psi.T * w) @ psi - np.outer(m, m)
    Ainv = np.linalg.inv(A)
    C = Ainv @ B @ Ainv / M
    return A, B, g, np.sqrt(np.diag(C)), float(np.linalg.cond(A))
