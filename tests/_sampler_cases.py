"""The cases of tests/test_gpu_sampler_exact.py, and the bound its CDF comparison uses.  tests/test_host_sampler_reference.py asserts,
on the reference alone, that no random number of any case lies close enough to a decision edge for the device's rounding to flip it
(the margin rule); the GPU tests then demand equality draw for draw and exclude nothing.  numpy only."""
import functools
import importlib
import itertools

import numpy as np

import _high_order_cases as H
import _sampler_reference as R
from conftest import MODELS

SEEDS = (11, 2 ** 64 - 3)
U = 2.0 ** -53  # unit roundoff of FP64


def en_bound(nt, sumw):
    """|en_device - en| of k_block_energies: e = ((w_1 + w_2) + ...) + w_nt, signs included, is nt - 1 FP64 additions whose partial
    sums are at most sum|w| in magnitude, so each rounds by at most U sum|w|: (nt - 1) U sum|w| <= nt U sum|w|."""
    return nt * U * sumw


def cdf_bound(sb, nt, sumw):
    """B_cdf, the bound on |cdf_device - cdf| of k_block_cdf, in units of the normalised CDF (<= 1), with per = ceil(2^sb / 1024):

      (per + 1024 + 8) U   the sums and the normalisation.  p_j = exp(en_j - max) > 0, so a sequential sum carries every term
                           through with a relative error of at most U per addition it takes part in: at most per additions inside
                           its thread's chunk and 1023 in the serial scan of the 1024 partial sums.  cdf_i = A_i / T is a ratio of
                           two such sums that share the scan's prefix; a relative error of at most e on every term of A_i and T
                           moves the ratio by at most e (it moves it by 2 e x (1 - x) <= e / 2 when all terms err alike, x the
                           ratio itself).  The 8 U: exp at 1 ulp = 2 U relative (the documented accuracy of the device's FP64
                           exp), the running sum's last addition, 1 / T, the product with it, and their second-order terms.
      2 nt U sum|w|        the exponent.  en_j and the maximum each carry (nt - 1) U sum|w| (en_bound), and their difference, at
                           most 2 sum|w| in magnitude, rounds by 2 U sum|w|: exp turns an absolute error d of its argument into
                           a relative error d of p_j, which the ratio passes on as above."""
    per = ((1 << sb) + 1023) // 1024
    return (per + 1024 + 8) * U + 2 * nt * U * sumw


# ------------------------------------------------------------------------------------------
# a. one block through the hook: terms as (local 0-based spins, weight)
# ------------------------------------------------------------------------------------------
def _ring_fields(sb, seed):
    rng = np.random.default_rng(seed)
    return [((i, (i + 1) % sb), float(rng.normal(scale=0.4))) for i in range(sb)] + \
           [((i,), float(rng.normal(scale=0.3))) for i in range(sb)]


def _subsets13():
    rng = np.random.default_rng(13)
    return [(c, float(rng.normal(scale=0.05))) for k in (1, 2, 3, 4) for c in itertools.combinations(range(13), k)]


def _chain22():
    rng = np.random.default_rng(25)
    return [((i, i + 1), float(rng.normal(scale=0.3))) for i in range(21)] + [((i,), float(rng.normal(scale=0.2))) for i in range(22)]


def _steep10():
    # exp(-160) and below against 1: flat CDF runs, and 2^10 - 2^5 states whose probability underflows to nothing
    return [((2 * i,), 80.0 * (-1) ** i) for i in range(5)] + [((2 * i + 1,), 0.3) for i in range(5)]


def _wide12():
    """terms of 5 to 8 spins on 12: masks of five to eight bits (the keys that name a spin twice are reduced here, as the host half
    reduces them before the kernels see a mask)"""
    out = []
    for key, w in H.wide_terms(12, 12, scale=0.15).items():
        odd = sorted(i - 1 for i in set(key) if key.count(i) % 2)
        out.append((tuple(odd), w))
    return out


BLOCK_MODELS = {
    "isolated_sb1": (1, lambda: []),
    "field_sb1": (1, lambda: [((0,), 0.7)]),
    "ring_sb8": (8, lambda: _ring_fields(8, 8)),
    "ring_sb10": (10, lambda: _ring_fields(10, 10)),
    "ring_sb11": (11, lambda: _ring_fields(11, 11)),
    "subsets_sb13": (13, _subsets13),
    "chain_sb22": (22, _chain22),
    "steep_sb10": (10, _steep10),
    "wide_sb12": (12, _wide12),
}
# (N, seed, block) of the launches of every block model: each N, each seed and each stream at least once
BLOCK_RUNS = ((1, SEEDS[0], 0), (257, SEEDS[1], 3), (20000, SEEDS[0], 3), (20000, SEEDS[1], 0))


@functools.lru_cache(maxsize=None)
def block_model(name):
    """(sb, masks uint32 [nt], wts float64 [nt], members int32 [sb], n, en, cdf): members are every third spin of n = 3 sb + 1
    in a shuffled order; en and cdf the reference's, np.longdouble"""
    sb, make = BLOCK_MODELS[name]
    terms = make()
    masks = np.array([sum(1 << i for i in k) for k, _ in terms], dtype=np.uint32)
    wts = np.array([w for _, w in terms], dtype=np.float64)
    members = (3 * np.random.default_rng(sb).permutation(sb) + 1).astype(np.int32)
    en = R.block_energies(masks, wts, sb)
    return sb, masks, wts, members, 3 * sb + 1, en, R.block_cdf(en)


@functools.lru_cache(maxsize=None)
def block_draws(name, N, seed, block):
    """(S [N, n] int8 with 0 outside the members, margin) of one launch"""
    sb, _, _, members, n, _, cdf = block_model(name)
    st, margin = R.draw_states(cdf, N, seed, block)
    S = np.zeros((N, n), dtype=np.int8)
    for t in range(sb):
        S[:, members[t]] = np.where((st >> t) & 1, 1, -1)
    return S, margin


def seed_with_u(bits53, stream, k):
    """the seed at which u01(seed, stream, k) = bits53 / 2^53 exactly: the hash of gml_rng.h is a bijection of the counter word,
    undone here step by step (x ^= x >> s is undone by repeating it; the multipliers are odd)"""
    mask = (1 << 64) - 1
    z = bits53 << 11
    z ^= z >> 31
    z ^= z >> 62
    z = z * pow(0x94D049BB133111EB, -1, 1 << 64) & mask
    z ^= z >> 27
    z ^= z >> 54
    z = z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64) & mask
    z ^= z >> 30
    z ^= z >> 60
    return (z - 0x9E3779B97F4A7C15 * (k + 1) - 0xD1B54A32D192ED03 * (stream + 1)) & mask


# The tie: an isolated spin has the CDF (0.5, 1.0), which the device computes without any rounding (exp(0) = 1, 1 + 1, 1 / 2), so
# this edge cannot move and a u of exactly 0.5 may sit on it: "the first state whose cdf > u" is then the upper state, +1.
# Sample TIE_K of stream TIE_BLOCK draws u = 0.5 at TIE_SEED; every other sample of the run keeps the margin of its case.
TIE_BLOCK, TIE_K, TIE_N = 3, 100, 257
TIE_SEED = seed_with_u(1 << 52, TIE_BLOCK, TIE_K)


# ------------------------------------------------------------------------------------------
# b. the front door of the exact sampler: (terms, n, N)
# ------------------------------------------------------------------------------------------
def matrix_terms(m):
    """the term list of a symmetric matrix as gml_problem_create_sampled lists it: row by row, j <= i, zeros skipped"""
    terms = {}
    for i in range(m.shape[0]):
        for j in range(i + 1):
            if m[i, j] != 0.0:
                terms[(j + 1, i + 1) if j < i else (i + 1,)] = float(m[i, j])
    return terms


def _interleaved29():
    """components of 5, 9 and 12 spins dealt out over n = 29, the spins 5, 18 and 29 left alone (1-based)"""
    rng = np.random.default_rng(29)
    free = [v for v in range(1, 30) if v not in (5, 18, 29)]
    comps = ([], [], [])
    want = (5, 9, 12)
    c = 0
    for v in free:  # round robin over the components that still lack spins
        while len(comps[c % 3]) == want[c % 3]:
            c += 1
        comps[c % 3].append(v)
        c += 1
    terms = {}
    for sp in comps:
        for a in range(len(sp) - 2):
            terms[(sp[a + 2], sp[a], sp[a + 1])] = float(rng.normal(scale=0.4))  # order 3, keys not ascending
        for a in range(0, len(sp) - 3, 2):
            terms[(sp[a], sp[a + 1], sp[a + 2], sp[a + 3])] = float(rng.normal(scale=0.3))
        for v in sp:
            terms[(v,)] = float(rng.normal(scale=0.3))
    A, B, C = comps
    terms[(A[0], B[0])] = 0.0                 # would join the first two components
    terms[(18, 18, B[1], B[4])] = 0.35        # spin 18 cancels: the pair (B[1], B[4]), and 18 stays alone
    terms[(A[1], C[2], A[1], C[5])] = -0.25   # A[1] cancels: the pair (C[2], C[5]), and the components stay apart
    terms[(C[0], C[0])] = 0.5                 # all cancel: the empty term
    return terms, 29, 3001


def blocks64_matrix():
    """64 spins in four independent blocks of 16 (the model of test_block_structured_model_beyond_enumeration)"""
    return importlib.import_module("gml_amd.synthetic").block_ising(64, 10, block=16, seed=5)[1]


def _blocks64():
    return matrix_terms(blocks64_matrix()), 64, 5000


def _twins():
    """two blocks with the same terms: their draws come from different streams"""
    rng = np.random.default_rng(2)
    w = rng.normal(scale=0.4, size=6)
    terms = {}
    for off in (0, 4):
        for t, k in enumerate([(1, 2), (2, 3), (3, 4), (1, 2, 3), (1,), (4,)]):
            terms[tuple(v + off for v in k)] = float(w[t])
    return terms, 8, 2000


def _wide19():
    """a component of 12 spins held together by terms of 5 to 8 spins (cancellations included), one of 6 spins under a single
    6-spin term and its fields, and spin 19 alone; the spins of the two components interleaved"""
    big = [1, 2, 4, 5, 7, 8, 10, 11, 13, 14, 16, 17]
    small = [3, 6, 9, 12, 15, 18]
    terms = H.wide_terms(19, 19, spins=big, scale=0.15)
    terms[tuple(reversed(small))] = 0.4
    terms[(3,)] = -0.2
    terms[(19, 19)] = 0.3  # the empty term
    return terms, 19, 3001


EXACT_CASES = {
    "interleaved29": _interleaved29,
    "blocks64": _blocks64,
    "golden_c": lambda: (matrix_terms(MODELS["c"]), 4, 4000),
    "twins": _twins,
    "n1": lambda: ({(1,): 0.4}, 1, 2000),
    "rings33": lambda: ({k: w for off in (0, 11, 22) for k, w in
                         [((off + i + 1, off + (i + 1) % 11 + 1), 0.3 + 0.01 * i) for i in range(11)] + [((off + 1,), 0.2)]}, 33, 3000),
    "wide19": _wide19,
}


@functools.lru_cache(maxsize=None)
def exact_case(name, seed):
    """(terms, n, N, S, margin, the largest B_cdf of its blocks)"""
    terms, n, N = EXACT_CASES[name]()
    S, margin = R.exact_draws(terms, n, N, seed)
    bound = max(cdf_bound(len(sp), len(w), float(np.abs(w).sum())) for sp, _, w in R.blocks(terms, n))
    return terms, n, N, S, margin, bound


# ------------------------------------------------------------------------------------------
# c. k_glauber: (terms, n, N, sweeps)
# ------------------------------------------------------------------------------------------
def sparse3(n, seed, dyadic=False, skip=()):
    """order-3 terms and pairs among the spins not in `skip`, fields on every second spin, keys that name a spin twice; dyadic:
    weights that are multiples of 2^-8 below 1 in magnitude, whose field sums are exact in any order"""
    rng = np.random.default_rng(seed)
    live = np.array([i for i in range(1, n + 1) if i not in skip])
    wt = (lambda s: float(np.clip(np.rint(rng.normal(scale=s) * 256), -255, 255) / 256)) if dyadic else (lambda s: float(rng.normal(scale=s)))
    terms = {}
    for _ in range(n):
        terms[tuple(int(v) for v in rng.choice(live, 3, replace=False))] = wt(0.3)
    for _ in range(n):
        terms[tuple(int(v) for v in rng.choice(live, 2, replace=False))] = wt(0.3)
    for i in range(1, n + 1, 2):
        if i not in skip:
            terms[(i,)] = wt(0.2)
    for _ in range(n // 6):
        i, j, k = (int(v) for v in rng.choice(live, 3, replace=False))
        terms[(i, i, j, k)] = wt(0.3)  # the pair (j, k)
        terms[(i, j, i)] = wt(0.3)     # the field of j
    return terms


def ring(n, w=0.3, h=0.1):
    terms = {(i + 1, (i + 1) % n + 1): w * (1 if i % 3 else -1) for i in range(n)}
    terms.update({(i + 1,): h * ((i % 5) - 2) for i in range(n)})
    return terms


GLAUBER_CASES = {
    "n1": lambda: ({(1,): 0.3}, 1, 300, 3),
    "sparse33": lambda: (sparse3(33, 33, skip=(8, 22)), 33, 1000, 7),  # the spins 8 and 22 are in no term
    "sparse70": lambda: (sparse3(70, 70), 70, 257, 4),
    "one_chain12": lambda: (sparse3(12, 12), 12, 1, 1),
    "dyadic33": lambda: (sparse3(33, 34, dyadic=True, skip=(8,)), 33, 1000, 7),
    "ring64": lambda: (ring(64), 64, 5000, 6),
    "wide24": lambda: (H.wide_terms(24, 24, scale=0.2), 24, 1000, 5),  # terms of 5 to 8 spins, cancellations included
}


@functools.lru_cache(maxsize=None)
def glauber_case(name, seed):
    """(terms, n, N, sweeps, S, margin)"""
    terms, n, N, sweeps = GLAUBER_CASES[name]()
    S, margin = R.glauber(terms, n, N, sweeps, seed)
    return terms, n, N, sweeps, S, margin


# d. histogram handles: cases of b (sample-major draws) and of c (spin-major draws) with n = 1, 33 and 64
HIST_EXACT = ("n1", "rings33", "blocks64")
HIST_GLAUBER = ("n1", "sparse33", "ring64")
