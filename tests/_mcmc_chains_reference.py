"""numpy restatement of gml_problem_create_mcmc_chains (include/gml.h): the samplers' u01 hash in wrapping uint64 arithmetic,
the per-row quantisation of the couplings, the exact integer fields and the heat-bath update, vectorised over chains.
Returns the +-1 states the handle holds, row t * chains + c."""
import numpy as np

_STEP = np.uint64(0x9E3779B97F4A7C15)
_STREAM = np.uint64(0xD1B54A32D192ED03)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def u01(seed, stream, k):
    """u01(seed, stream, k) of gml_rng.h for an array of counters k (uint64, wraps)"""
    with np.errstate(over="ignore"):
        k = np.asarray(k, dtype=np.uint64)
        z = np.uint64(seed) + _STEP * (k + np.uint64(1)) + _STREAM * (np.uint64(stream) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def quantise(A):
    """sigma_i = 2^(e - 38) with max_{j != i} |A_ij| < 2^e, q_ij = rint(A_ij / sigma_i), q_ii = 0 -> (q as int64, sigma)"""
    A = np.asarray(A, dtype=np.float64)
    off = A - np.diag(np.diag(A))
    mx = np.abs(off).max(axis=1) if A.shape[0] > 1 else np.zeros(1)
    _, ex = np.frexp(mx)
    ex = np.where(mx > 0, ex, 0)
    q = np.rint(np.ldexp(off, (38 - ex)[:, None])).astype(np.int64)
    np.fill_diagonal(q, 0)
    return q, np.ldexp(1.0, ex - 38)


def chains(A, nchains, samples_per_chain, burn_in, thin, seed):
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    q, sig = quantise(A)
    qf = q.astype(np.float64)  # |q| <= 2^38 and every partial sum < n 2^38 < 2^53: FP64 sums of these integers are exact
    diag = np.diag(A).copy()
    c = np.arange(nchains, dtype=np.uint64)
    S = np.empty((n, nchains), dtype=np.float64)
    for i in range(n):
        S[i] = np.where(u01(seed, 0xFFFFFFFF, c * np.uint64(n) + np.uint64(i)) < 0.5, 1.0, -1.0)
    out = np.empty((nchains * samples_per_chain, n), dtype=np.int8)
    for sw in range(burn_in + (samples_per_chain - 1) * thin):
        for i in range(n):
            h = diag[i] + sig[i] * (qf[i] @ S)
            pup = 1.0 / (1.0 + np.exp(-2.0 * h))
            S[i] = np.where(u01(seed, sw, c * np.uint64(n) + np.uint64(i)) < pup, 1.0, -1.0)
        done = sw + 1
        if done >= burn_in and (done - burn_in) % thin == 0:
            t = (done - burn_in) // thin
            out[t * nchains:(t + 1) * nchains] = S.T.astype(np.int8)
    return out
