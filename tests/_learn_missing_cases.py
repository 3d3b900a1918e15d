"""The case of the learn_missing tests (host and device): an n = 8 model -- a ring of +-0.6 couplings, one chord of 0.5, fields in
+-0.3 -- DRAWS exact draws, 30 % of the entries removed at random by a seeded numpy mask, the default RISE().  Four errors on the same
data, each the largest absolute difference over fields and symmetrised couplings from the truth: e_full (learn on the data before
masking), e_cc (learn on the rows without a hole), e_0 (the first EM iterate: coin-flip imputation), e_em (the last iterate).

BOUND on e_em.  The host loop (tests/test_host_learn_missing.py: the numpy restatement of the masked chains, the CPU oracle's solve)
at the five seeds 0 .. 4, the seed setting the draws, the mask and the imputations alike, the rows in the order the front door
runs them in (inference._mask_order):

    seed   e_full    e_cc     e_0      e_em
    0      0.0330    0.1248   0.4145   0.0554
    1      0.0314    0.1009   0.4167   0.0484
    2      0.0472    0.1026   0.4129   0.0343
    3      0.0336    0.0940   0.4173   0.0344
    4      0.0289    0.1281   0.4181   0.0461

The error of the iterates falls by about 0.67x per iteration to iteration 6 or so and then moves between 0.03 and 0.06.
BOUND = sqrt(worst e_em x smallest e_cc) = sqrt(0.0554 x 0.0940) = 0.0722: between what the method does and what the user had before
it; neither number comes from the device code."""
import numpy as np

N = 8
DRAWS = 20000
MISSING = 0.3
BOUND = 0.0722
SEEDS = (0, 1, 2, 3, 4)


def true_terms():
    """{1-based key: weight} and the same model as a symmetric matrix with the fields on its diagonal"""
    rng = np.random.default_rng(0)
    terms = {}
    for i in range(N):
        terms[(i + 1, (i + 1) % N + 1) if i + 1 < N else (1, N)] = 0.6 * (1.0 if rng.random() < 0.5 else -1.0)
    terms[(1, 5)] = 0.5
    for i in range(N):
        terms[(i + 1,)] = float(rng.uniform(-0.3, 0.3))
    truth = np.zeros((N, N))
    for k, w in terms.items():
        if len(k) == 1:
            truth[k[0] - 1, k[0] - 1] = w
        else:
            truth[k[0] - 1, k[1] - 1] = truth[k[1] - 1, k[0] - 1] = w
    return terms, truth


def with_holes(spins, seed):
    """(hist with holes, hist of the full data, hist of the rows without a hole): K x (1+n) matrices of count 1; 0 = missing"""
    spins = np.asarray(spins, dtype=np.int64)
    gone = np.random.default_rng(seed).random(spins.shape) < MISSING
    ones = np.ones((len(spins), 1), dtype=np.int64)
    full = np.concatenate([ones, spins], axis=1)
    holes = np.concatenate([ones, np.where(gone, 0, spins)], axis=1)
    return holes, full, full[~gone.any(axis=1)]


def error(model, truth):
    return float(np.abs(np.asarray(model) - truth).max())
