"""Host model of the pack layer of the int8-limb passes: the bit images of the samples, the quantisation of the rows of Theta into
balanced base-256 digit planes (plain and on signed column pairs), the tile marks and the compact column lists.  numpy and Python
integers only, written from the comments of csrc/gml_bits.h, csrc/gml_i8_pairs.h and csrc/gml_i8_pack.hip; it imports and calls
nothing compiled from them.  tests/test_host_i8_pack_reference.py pins its index maps and digit rules to those headers, entry for
entry; tests/test_gpu_i8_pack_state.py holds the device's arrays to its predictions, bit for bit.

Everything here is an exact integer or a bit except tau(), which is formed in np.longdouble."""
import itertools
import math

import numpy as np

LD = np.longdouble
PAIR_UNIT = 0x01010101010101  # (256^7 - 1) / 255: seven balanced digits spell exactly PAIR_MIN .. PAIR_MAX
PAIR_MAX, PAIR_MIN = 127 * PAIR_UNIT, -128 * PAIR_UNIT
VDIV = {4: 2130000000.0, 6: 1.400e14}  # largest |V| / tau of a 4-plane (i8x) and a 6-plane (i8w) V image


# ---------------------------------------------------------------------------------------------------------------------------
# index maps (gml_bits.h, gml_i8_pairs.h)
# ---------------------------------------------------------------------------------------------------------------------------
def xb_col(j, h):
    """column, within its 64-column step, of bit j of the forward dword of lane half h: bit e + 8 b <-> 32 (e >> 2) + 16 h + 4 (e & 3) + b"""
    e, b = j & 7, j >> 3
    return 32 * (e >> 2) + 16 * h + 4 * (e & 3) + b


def vq_sample(p):
    """sample, within its 64-sample step, at operand position p: the lane (node, half h) owns the samples 32 i + 8 g + 4 h + j and keeps
    them at byte 32 h + 16 i + 4 g + j"""
    h, i, g, j = p >> 5, (p >> 4) & 1, (p >> 2) & 3, p & 3
    return 32 * i + 8 * g + 4 * h + j


def pair_slot(h, m):
    """byte of alpha of pair m (0..15) of lane half h in a row's 64 bytes of a plane (beta: the next byte): byte m of the lane's sparse
    operand multiplies K slots 32 (m >> 3) + 16 h + 4 ((m & 7) >> 1) + {0..3}, the lower two for even m, the upper two for odd m"""
    return 32 * (m >> 3) + 16 * h + 4 * ((m & 7) >> 1) + 2 * (m & 1)


def pair_col(h, m, second):
    """the columns pair m of lane half h pairs: bits 2 m and 2 m + 1 of the dword"""
    return xb_col(2 * m + second, h)


def xtb_bit(i):
    """bit of the backward dword that holds natural bit i = 8 e + 4 t + b (e < 4, t < 2, b < 4) of the same 32 samples: 4 t + e + 8 b"""
    e, t, b = i >> 3, (i >> 2) & 1, i & 3
    return 4 * t + e + 8 * b


def xtb_from_natural(x):
    return sum(1 << xtb_bit(i) for i in range(32) if (x >> i) & 1)


# ---------------------------------------------------------------------------------------------------------------------------
# digits
# ---------------------------------------------------------------------------------------------------------------------------
def balanced_digits(v, n):
    """n balanced base-256 digits (-128..127, least significant first) of the Python integer v, and what is left"""
    v = int(v)
    out = []
    for _ in range(n):
        d = ((v + 128) & 255) - 128
        out.append(d)
        v = (v - d) >> 8
    return out, v


def pair_in_range(q, qp):
    a, b = int(q) + int(qp), int(q) - int(qp)
    return PAIR_MIN <= a <= PAIR_MAX and PAIR_MIN <= b <= PAIR_MAX


def digits_np(v, n):
    """balanced_digits on an int64 array (|v| < 2^62): int8 [n, ...] and the rest"""
    v = np.asarray(v, dtype=np.int64).copy()
    out = np.zeros((n,) + v.shape, dtype=np.int8)
    for l in range(n):
        d = ((v + 128) & 255) - 128
        out[l] = d.astype(np.int8)
        v = (v - d) >> 8
    return out, v


def undigits_np(planes):
    """the integers int8 planes [n, ...] spell"""
    v = np.zeros(planes.shape[1:], dtype=np.int64)
    for l in reversed(range(planes.shape[0])):
        v = v * 256 + planes[l].astype(np.int64)
    return v


# ---------------------------------------------------------------------------------------------------------------------------
# quantisation of one row (k_quant_theta)
# ---------------------------------------------------------------------------------------------------------------------------
def _frexp_e(x):
    return math.frexp(x)[1] if x > 0 else 0


def sigma_exponent(th, Qfp, cconst, LF):
    """sx with sigma = 2^sx: 2^(ex - (8 LF - 2)) with max |theta| < 2^ex; seven planes: raised so that sum |theta| * 1.0000001 < 2^(sx + 61).
    Returns (sx, margin): margin is the relative distance of that sum from the nearest power of two -- the device adds the |theta| in
    another order, so a caller makes sure the margin is far above a rounding error"""
    a = np.abs(np.concatenate([th[:Qfp], th[cconst:cconst + 1]]))
    mx = float(a.max()) if a.size else 0.0
    sx = _frexp_e(mx) - (8 * LF - 2)
    margin = 1.0
    if LF > 5:
        s1 = math.fsum(a.tolist()) * 1.0000001
        e1 = _frexp_e(s1)
        if s1 > 0:
            m = s1 / math.ldexp(1.0, e1)  # in [0.5, 1)
            margin = min(m - 0.5, 1.0 - m) * 2
        sx = max(sx, e1 - 61)
    return sx, margin


def quantise(th, Qfp, cconst, LF):
    """(sx, q int64 [Qfp], q0): q = rint(theta / sigma), the constant column's integer apart"""
    sx, _ = sigma_exponent(th, Qfp, cconst, LF)
    isg = math.ldexp(1.0, -sx)
    q = np.rint(th[:Qfp] * isg).astype(np.int64)
    q0 = int(np.rint(th[cconst] * isg))
    return sx, q, q0


def row_scalars(th, Qfp, cconst, LF):
    """sigma, qconst = qpair + sum q, qconst2 = the same sum over what three digits taken off leave, qpair = the constant column's
    integer, sabs = sum |q| (constant column included)"""
    sx, q, q0 = quantise(th, Qfp, cconst, LF)
    qs = [int(x) for x in q]
    out = dict(sx=sx, sigma=math.ldexp(1.0, sx), qpair=q0, qconst=q0 + sum(qs), sabs=abs(q0) + sum(abs(x) for x in qs))
    out["qconst2"] = sum(balanced_digits(x, 3)[1] for x in qs + [q0])
    return out


def tau(sabs, sx, wmax, form, planes_v):
    """B (1 + 1e-12) / vdiv in np.longdouble: B = 2 w_max (RPLE) or w_max exp(emax).  emax is the kernel's own bound on the energies,
    fl64(sum |q|) * sigma: the integer sum (up to 61 bits with seven planes) converted to a double, to nearest even as Python's
    float() does, times a power of two.  That conversion belongs to the definition of tau, not to its error: e^x carries a change of
    x over |x| times, so a model that exponentiated the unrounded sum would differ from any FP64 evaluation by up to
    2^-53 sum |theta| -- 25 ulp on a row of sum |theta| = 50 -- and say nothing about the exp and the two roundings a caller bounds."""
    emax = LD(float(int(sabs))) * LD(2.0) ** sx
    B = LD(2.0) * LD(wmax) if form == "RPLE" else LD(wmax) * np.exp(emax)
    return B * (LD(1.0) + LD(1e-12)) / LD(VDIV[planes_v])


# ---------------------------------------------------------------------------------------------------------------------------
# one tile: column union, marks, digit planes
# ---------------------------------------------------------------------------------------------------------------------------
def compact_steps(Qfp):
    """capacity of a tile's compact list in 64-column steps; 0: problems of one step never compact"""
    nk = Qfp // 64
    return min(32, max(1, nk // 4)) if nk >= 2 else 0


def column_union(rows, active, Qfp, csteps):
    """(cnk, list): the columns < Qfp on which an active row of the tile is non-zero, ascending, padded with -1 to whole steps;
    cnk = ceil(count / 64), or -1 (list None) above csteps * 64"""
    nz = np.zeros(Qfp, dtype=bool)
    for r, a in zip(rows, active):
        if a:
            nz |= r[:Qfp] != 0.0
    cols = np.flatnonzero(nz)
    if len(cols) > csteps * 64:
        return -1, None
    nk = (len(cols) + 63) // 64
    out = np.full(nk * 64, -1, dtype=np.int32)
    out[:len(cols)] = cols
    return nk, out


def _grid(q, Qfp, cm):
    """the integers at the positions the tile's image covers: all columns, or those of the compact list (-1: a zero column)"""
    if cm is None:
        return q[:Qfp]
    return np.where(cm >= 0, q[np.maximum(cm, 0)], 0)


_PAIRS = [(h, m) for h in range(2) for m in range(16)]


def pairs_of(qg):
    """(alpha, beta) int64 [steps, 2, 16] of the positions qg [steps * 64]"""
    g = qg.reshape(-1, 64)
    c0 = np.array([[pair_col(h, m, 0) for m in range(16)] for h in range(2)])
    c1 = np.array([[pair_col(h, m, 1) for m in range(16)] for h in range(2)])
    return g[:, c0] + g[:, c1], g[:, c0] - g[:, c1]


def tile_marked(rows, active, Qfp, cconst, cm=None):
    """does an active row hold a pair outside seven digits, among the pairs a pass over these positions visits?"""
    for r, a in zip(rows, active):
        if not a:
            continue
        _, q, _ = quantise(r, Qfp, cconst, 7)
        al, be = pairs_of(_grid(q, Qfp, cm))
        if (al > PAIR_MAX).any() or (al < PAIR_MIN).any() or (be > PAIR_MAX).any() or (be < PAIR_MIN).any():
            return True
    return False


def row_image(th, Qfp, cconst, LF, paired, cm=None):
    """int8 [steps][LF][64]: the row's bytes in the tile's image.  Plain: byte j of a step is position j.  Paired: alpha at byte
    pair_slot(h, m), beta in the next, of the positions pair_col(h, m, 0 / 1)."""
    _, q, _ = quantise(th, Qfp, cconst, LF)
    qg = _grid(q, Qfp, cm)
    steps = len(qg) // 64
    if not paired:
        d, _ = digits_np(qg.reshape(steps, 64), LF)
        return np.ascontiguousarray(d.transpose(1, 0, 2))
    al, be = pairs_of(qg)
    v = np.zeros((steps, 64), dtype=np.int64)
    for h, m in _PAIRS:
        v[:, pair_slot(h, m)] = al[:, h, m]
        v[:, pair_slot(h, m) + 1] = be[:, h, m]
    d, _ = digits_np(v, LF)
    return np.ascontiguousarray(d.transpose(1, 0, 2))


def decode_image(img_row, paired):
    """the integers a row's bytes int8 [steps][LF][64] spell: plain -> q [steps * 64] by position; paired -> (q, q') recovered from
    (alpha, beta) at the positions of the pair, None where alpha + beta is odd (no pair of integers spells it)"""
    v = undigits_np(np.ascontiguousarray(img_row.transpose(1, 0, 2)))
    if not paired:
        return v.reshape(-1)
    out = np.zeros_like(v)
    for h, m in _PAIRS:
        a, b = v[:, pair_slot(h, m)], v[:, pair_slot(h, m) + 1]
        if ((a + b) & 1).any():
            return None
        out[:, pair_col(h, m, 0)] = (a + b) // 2
        out[:, pair_col(h, m, 1)] = (a - b) // 2
    return out.reshape(-1)


def predict_pass(theta, active, Qfp, cconst, LF, pairs, compact):
    """What one objective pass leaves for the slots it lists.  theta [Rp][Qp] internal-layout rows, active [Rp] bool; pairs / compact:
    the pass pairs columns (seven planes only) / compacts.  Per tile t with an active row: cnk[t], cmap[t] (compact), mark[t] (pairs),
    and per active slot the scalars and the bytes image[slot] = int8 [steps][LF][64] of the steps the pass writes."""
    Rp = len(theta)
    csteps = compact_steps(Qfp) if compact else 0
    res = dict(cnk={}, cmap={}, mark={}, image={}, scalars={}, paired={}, csteps=csteps)
    for t in range(Rp // 32):
        sl = range(32 * t, 32 * t + 32)
        act = [bool(active[s]) for s in sl]
        if not any(act):
            continue
        rows = [theta[s] for s in sl]
        cm = None
        if csteps:
            nk, lst = column_union(rows, act, Qfp, csteps)
            res["cnk"][t] = nk
            res["cmap"][t] = lst
            cm = lst
        paired = False
        if pairs:
            res["mark"][t] = int(tile_marked(rows, act, Qfp, cconst, cm))
            paired = not res["mark"][t]
        res["paired"][t] = paired
        for s, a in zip(sl, act):
            if a:
                res["image"][s] = row_image(theta[s], Qfp, cconst, LF, paired, cm)
                res["scalars"][s] = row_scalars(theta[s], Qfp, cconst, LF)
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# bit images
# ---------------------------------------------------------------------------------------------------------------------------
def stat_keys(n, order):
    """the statistics columns: the non-empty subsets of the spins up to size max(order - 1, 1), by size, then lexicographic;
    int32 [Qf][ko], unused slots -1"""
    ko = max(order - 1, 1)
    keys = []
    for q in range(1, ko + 1):
        for c in itertools.combinations(range(n), q):
            keys.append(list(c) + [-1] * (ko - q))
    return np.array(keys, dtype=np.int32).reshape(-1, ko)


def stat_bits(spins, keys, rows, Kp):
    """uint8 [rows][Kp]: the bit of a statistic is the XOR of its spins' sign bits (set <=> -1); padding samples and the columns
    beyond the keys are zero bits"""
    K, n = spins.shape
    neg = (spins < 0).astype(np.uint8)
    B = np.zeros((rows, Kp), dtype=np.uint8)
    for c, key in enumerate(keys):
        for i in key:
            if i >= 0:
                B[c, :K] ^= neg[:, i]
    return B


def _forward_image(B, Kp, nk, col_of):
    """dwords [Kp / 128][nk][128 samples][2 h]: bit j of dword (k, kt, h) is column col_of(kt, xb_col(j, h)) (-1: zero)"""
    img = np.zeros((Kp // 128, nk, 128, 2), dtype=np.uint32)
    for kt in range(nk):
        for h in range(2):
            v = np.zeros(Kp, dtype=np.uint32)
            for j in range(32):
                c = col_of(kt, xb_col(j, h))
                if c >= 0:
                    v |= B[c].astype(np.uint32) << np.uint32(j)
            img[:, kt, :, h] = v.reshape(Kp // 128, 128)
    return img.reshape(-1)


def xb_image(B, Kp, Qfp):
    return _forward_image(B, Kp, Qfp // 64, lambda kt, j: 64 * kt + j)


def xc_image(B, Kp, cnk, cm):
    """the forward image of a compacted tile: Xb through the tile's list, with the tile's own step count"""
    return _forward_image(B, Kp, cnk, lambda kt, j: int(cm[64 * kt + j]))


def xtb_image(B, Kp, Qfp):
    """dwords [Qc / 128][Kp / 64][128 columns][2 h], Qc = Qfp rounded up to 256: bit j of dword (c, kt, h) is the sample
    64 kt + vq_sample(xb_col(j, h)) of column c"""
    Qc = (Qfp + 255) // 256 * 256
    nkk = Kp // 64
    img = np.zeros((Qc // 128, nkk, 128, 2), dtype=np.uint32)
    Bc = np.zeros((Qc, nkk, 64), dtype=np.uint32)
    Bc[:B.shape[0]] = B.reshape(B.shape[0], nkk, 64)
    for h in range(2):
        v = np.zeros((Qc, nkk), dtype=np.uint32)
        for j in range(32):
            v |= Bc[:, :, vq_sample(xb_col(j, h))] << np.uint32(j)
        img[:, :, :, h] = v.reshape(Qc // 128, 128, nkk).transpose(0, 2, 1)
    return img.reshape(-1)
