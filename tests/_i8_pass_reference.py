"""Host model of one objective pass of the int8-limb operator, cut at the limb planes Vq of V: what k_fwd_i8 / k_fwd_i8w write into Vq
and the slot sums, and what k_bwd_i8 and k_finalize_i8 / k_finalize_i8w make of Vq.  numpy, Python integers and np.longdouble only,
written from the comments of csrc/gml_i8.h, csrc/gml_i8_fwd.h, csrc/gml_i8_fwd.hip, csrc/gml_kernels_i8w.hip, csrc/gml_i8_bwd.hip,
csrc/gml_bits.h and csrc/gml_dev.h; it imports and calls nothing compiled from them.  tests/test_host_i8_pass_reference.py holds it to
brute force; tests/test_gpu_i8_pass_exact.py holds the device to it.

Names: a pass has `lbt` limb planes per V image (4: i8x, 6: i8w).  V[r][k] / tau_r = sum_l 256^l v_l[r][k] with balanced digits v_l in
[-128, 127].  A coarse pass rounds V to multiples of unit * tau, unit = 2^8 (i8x: plane 0 zero) or 2^24 (i8w: plane 2 zero, planes 0 and 1
not written at all); `pl0` is the first plane that carries a value then (1 resp. 3) and the backward GEMM multiplies the planes from pl0 on.

Everything from Vq on is integers and float64 operations reproduced one by one.  The forward half is exact up to the device's exp: it
returns, per element, the real number y the device rounds (np.longdouble) and its distance from the nearest rounding boundary."""
import struct

import numpy as np

from _i8_pack_reference import digits_np, quantise

LD = np.longdouble
DITHER_NODE, GOLD = 0x85EBCA6B, 0x9E3779B9  # gml_i8_fwd.h
LBT = {"i8x": 4, "i8w": 6}
LF_WIDE = 7
COARSE_UNIT = {4: 1 << 8, 6: 1 << 24}
COARSE_PL0 = {4: 1, 6: 3}
VMAX = {4: 0x7F7F7F7F, 6: 0x7F7F7F7F7F7F}  # the largest and (negated, minus one digit step) smallest numbers lbt balanced digits spell
VMIN = {4: -0x80808080, 6: -0x808080808080}


# ---------------------------------------------------------------------------------------------------------------------------
# a. layout (gml_bits.h: vq_pos; gml_dev.h: vq_off)
# ---------------------------------------------------------------------------------------------------------------------------
def vq_pos(s):
    """byte, within the 64 bytes of a row of a step's image, of sample s of the step: the lane (node, half h) owns the samples
    32 i + 8 g + 4 h + j and stores them at byte 32 h + 16 i + 4 g + j"""
    i, g, h, j = s >> 5, (s >> 3) & 3, (s >> 2) & 1, s & 3
    return 32 * h + 16 * i + 4 * g + j


def vq_off(r, l, k, Kp, lbt):
    """byte of limb l of V[r][k]: images [node tile r / 32][step k / 64] of [lbt planes][32 rows][64 bytes], contiguous"""
    return ((((r >> 5) * (Kp >> 6) + (k >> 6)) * lbt + l) * 32 + (r & 31)) * 64 + vq_pos(k & 63)


_POS = np.array([vq_pos(s) for s in range(64)])


def unpack_vq(vq, slots, Kp, lbt):
    """int8 [slots][lbt][Kp], samples in their natural order, from the bytes of the device image"""
    img = np.asarray(vq, dtype=np.int8).reshape(slots // 32, Kp // 64, lbt, 32, 64)[..., _POS]
    return np.ascontiguousarray(img.transpose(0, 3, 2, 1, 4)).reshape(slots, lbt, Kp)


def pack_vq(planes):
    """the inverse of unpack_vq: the bytes of the image of int8 [slots][lbt][Kp]"""
    slots, lbt, Kp = planes.shape
    img = np.zeros((slots // 32, Kp // 64, lbt, 32, 64), dtype=np.int8)
    img[..., _POS] = planes.reshape(slots // 32, 32, lbt, Kp // 64, 64).transpose(0, 3, 2, 1, 4)
    return img.reshape(-1)


def live_planes(planes, coarse):
    """the planes as a pass of that form defines them: a coarse pass leaves the planes below pl0 - 1 unwritten (i8w: 0 and 1; they
    keep an earlier pass's bytes), so they read zero here; plane pl0 - 1 is written, as zeros"""
    lbt = planes.shape[1]
    if not coarse:
        return planes
    out = planes.copy()
    out[:, :COARSE_PL0[lbt] - 1] = 0
    return out


def value_of(planes):
    """V / tau as int64 [slots][Kp]: sum_l 256^l v_l"""
    v = np.zeros((planes.shape[0], planes.shape[2]), dtype=np.int64)
    for l in reversed(range(planes.shape[1])):
        v = v * 256 + planes[:, l].astype(np.int64)
    return v


def digits_of(v, lbt):
    """the lbt balanced base-256 digits of the integers v (int8 [lbt, ...]); they must spell v: VMIN <= v <= VMAX"""
    d, rest = digits_np(v, lbt)
    assert not np.any(rest), "value outside the planes"
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# b. the slot sums of a pass, from its planes
# ---------------------------------------------------------------------------------------------------------------------------
def _hi_word(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0] >> 32


def _from_hi_word(hi):
    return struct.unpack("<d", struct.pack("<q", int(hi) << 32))[0]


def mmax_wide_of_y(y32, coarse):
    """k_fwd_i8w's mmax from the largest y32 = 2^32 (|V| / unit tau + dither) of a slot (a float64 >= 0; the device keeps only its high
    word): ymax = the double whose high word is one more, low word 0.  Full width: floor(ymax 2^-48 + 2^-17), capped at 2^32 - 1;
    coarse: (floor(min(ymax 2^-32, 8388605)) + 2) << 8.  Units of 2^16 tau."""
    ymax = _from_hi_word(max(_hi_word(max(float(y32), 0.0)), 0) + 1)
    if coarse:
        return (int(min(ymax * 2.0 ** -32, 8388605.0)) + 2) << 8
    return int(min(ymax * 2.0 ** -48 + 2.0 ** -17, 4294967295.0))


def slot_sums(planes, coarse, exp_form, want_f):
    """What the forward kernel leaves per slot besides the planes, as far as the planes determine it.  planes: int8 [slots][lbt][Kp]
    as read back.  Returns int64 arrays (Python ints for the mmax interval):
      csum, csum2   i8x: csum = sum_k V / tau.  i8w: csum = the planes 0..2 (a coarse pass adds nothing: 0), csum2 = the planes 3..5
      asum, asum2   objective-only passes of the exp forms (want_f): i8x: sum_k |V| / tau.  i8w: every wave (64 consecutive samples)
                    adds the low 32 bits of its sum of |V| / (unit tau) to asum and the rest to asum2.  Zero otherwise (RPLE i8w uses
                    them for f: not modelled, None)
      mmax          exp forms; i8x: max_k |V| / tau, coarse (max_k |V| / (2^8 tau) + 1) << 8.  i8w: the pair (lo, hi) of mmax_wide_of_y at
                    the ends of the interval 2^32 (M -+ 1/2), M = max_k |V| / (unit tau): the dither is not in the planes.  RPLE: 0"""
    slots, lbt, Kp = planes.shape
    pl = live_planes(planes, coarse).astype(np.int64)
    psum = pl.sum(axis=2)  # [slots][lbt]
    unit = COARSE_UNIT[lbt] if coarse else 1
    val = value_of(pl)
    mag = np.abs(val) // unit
    out = {}
    if lbt == 4:
        out["csum"] = psum[:, 0] + 256 * psum[:, 1] + 65536 * psum[:, 2] + 16777216 * psum[:, 3]
        out["csum2"] = np.zeros(slots, dtype=np.int64)
        out["asum"] = np.abs(val).sum(axis=1) if (want_f and exp_form) else np.zeros(slots, dtype=np.int64)
        out["asum2"] = np.zeros(slots, dtype=np.int64)
        mx = mag.max(axis=1)
        out["mmax"] = ((mx + 1) << 8 if coarse else mx) if exp_form else np.zeros(slots, dtype=np.int64)
    else:
        out["csum"] = np.zeros(slots, dtype=np.int64) if coarse else psum[:, 0] + 256 * psum[:, 1] + 65536 * psum[:, 2]
        out["csum2"] = psum[:, 3] + 256 * psum[:, 4] + 65536 * psum[:, 5]
        if not exp_form:
            out["asum"] = out["asum2"] = None
            out["mmax"] = [(0, 0)] * slots
        else:
            if want_f:
                pw = mag.reshape(slots, Kp // 64, 64).sum(axis=2)
                out["asum"], out["asum2"] = (pw & 0xFFFFFFFF).sum(axis=1), (pw >> 32).sum(axis=1)
            else:
                out["asum"] = out["asum2"] = np.zeros(slots, dtype=np.int64)
            out["mmax"] = [(mmax_wide_of_y(max(float(m) - 0.5, 0.0) * 4294967296.0, coarse), mmax_wide_of_y((float(m) + 0.5) * 4294967296.0, coarse))
                           for m in mag.max(axis=1)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# c. backward GEMM and finalisation
# ---------------------------------------------------------------------------------------------------------------------------
def backward(planes, bits, coarse):
    """Gacc_l[r][c] = sum_k v_l[r][k] b[k][c] as int64 [slots][lbt][Qfp]: bits uint8 [Qfp][Kp], the sign bit of statistic c in sample k
    (set <=> -1).  A coarse pass multiplies the planes from pl0 on; the accumulators of the others stay zero.  Every sum must fit
    the device's int32."""
    slots, lbt, Kp = planes.shape
    pl0 = COARSE_PL0[lbt] if coarse else 0
    g = np.zeros((slots, lbt, bits.shape[0]), dtype=np.int64)
    bt = np.ascontiguousarray(bits.T).astype(np.float64)  # (|sum| <= 128 Kp < 2^53: the float64 GEMM is exact)
    g[:, pl0:] = np.rint(planes[:, pl0:].astype(np.float64).reshape(-1, Kp) @ bt).astype(np.int64).reshape(slots, lbt - pl0, -1)
    assert np.abs(g).max(initial=0) < 2 ** 31, "an accumulator of the model leaves int32"
    return g


def gacc_rows(gacc, slots, lbt, Qfp):
    """the device's accumulator set int32 [slots / 32][lbt][32][Qfp] as [slots][lbt][Qfp]"""
    return np.ascontiguousarray(np.asarray(gacc).reshape(slots // 32, lbt, 32, Qfp).transpose(0, 2, 1, 3)).reshape(slots, lbt, Qfp)


def _recombine(g):
    """sum_l 256^l g_l over the planes given (axis 0), int64"""
    g = np.asarray(g, dtype=np.int64)
    s = np.zeros(g.shape[1:], dtype=np.int64)
    for a in g[::-1]:
        s = s * 256 + a
    return s


def _as_double(i):
    """(double) of int64 values: to nearest, ties to even -- the conversion the kernels' casts and numpy's perform alike"""
    return np.asarray(i, dtype=np.int64).astype(np.float64)


def _gcol(lbt, coarse, csum, csum2, g):
    """the number k_finalize_* multiplies tau with, for the accumulators g [lbt, ...] of some columns: float64.
    i8x: (double)(csum - 2 s).  i8w: fma((double)(csum2 - 2 s1), 2^24, (double)(csum - 2 s0)), the low half absent from a coarse pass:
    both casts are exact (below 2^53) and so is the product by 2^24, so the fma rounds the exact integer hi 2^24 + lo once."""
    g = np.asarray(g, dtype=np.int64)
    if lbt == 4:
        return _as_double(np.int64(csum) - 2 * _recombine(g))
    hi = np.int64(csum2) - 2 * _recombine(g[3:])
    lo = np.zeros_like(hi) if coarse else np.int64(csum) - 2 * _recombine(g[:3])
    assert np.all(np.abs(hi) < 2 ** 37) and np.all(np.abs(lo) < 2 ** 53)  # (hi 2^24 + lo stays inside int64)
    return _as_double(hi * 16777216 + lo)


def finalize(lbt, coarse, tau, sums, gacc, rowcol, Qf, Qp, cconst, want_grad, exp_form):
    """G float64 [slots][Qp] (None without the gradient; rows of unused slots NaN: the kernels leave them alone) and f [slots] (NaN
    for RPLE, whose f is a sum of device FP64 terms, and for unused slots).
      G[r][c] = tau_r * gcol(c) for c < Qf, tau_r * gcol(no accumulators) at c = cconst, 0 on the other columns
      f[r] = -tau_r * gcol(u), u = rowcol[r] (with the gradient); tau_r * (double)asum (i8x) or
             tau_r * [2^24] * fma((double)asum2, 2^32, (double)asum) (i8w, the factor for a coarse pass) without it"""
    slots = len(rowcol)
    G = np.full((slots, Qp), np.nan) if want_grad else None
    f = np.full(slots, np.nan)
    zero = np.zeros(lbt, dtype=np.int64)
    for r in range(slots):
        u = int(rowcol[r])
        if u < 0:
            continue
        t = float(tau[r])
        cs, cs2 = sums["csum"][r], sums["csum2"][r]
        if want_grad:
            G[r] = 0.0
            G[r, :Qf] = t * _gcol(lbt, coarse, cs, cs2, gacc[r, :, :Qf])
            G[r, cconst] = t * float(_gcol(lbt, coarse, cs, cs2, zero))
        if exp_form:
            if want_grad:
                f[r] = -t * float(_gcol(lbt, coarse, cs, cs2, gacc[r, :, u]))
            elif lbt == 4:
                f[r] = t * float(_as_double(sums["asum"][r]))
            else:  # both casts exact (below 2^53); the fma rounds asum2 2^32 + asum once
                a = int(sums["asum2"][r]) * 4294967296 + int(sums["asum"][r])
                assert abs(int(sums["asum2"][r])) < 2 ** 53 and abs(int(sums["asum"][r])) < 2 ** 53
                f[r] = t * (16777216.0 if coarse else 1.0) * float(a)
    return G, f


# ---------------------------------------------------------------------------------------------------------------------------
# d. forward: the number each element rounds
# ---------------------------------------------------------------------------------------------------------------------------
def dither(u, k):
    """2^32 times the dither of node u, global sample index k (an int32, as int64): the low 32 bits of u * DITHER_NODE + k * GOLD read
    as a signed integer.  The dither itself is that times 2^-32, in [-1/2, 1/2)."""
    h = (np.asarray(u, dtype=np.uint64) * np.uint64(DITHER_NODE) + np.asarray(k, dtype=np.uint64) * np.uint64(GOLD)) & np.uint64(0xFFFFFFFF)
    h = h.astype(np.int64)
    return np.where(h >= 2 ** 31, h - 2 ** 32, h)


def energy_integers(theta_row, Qfp, cconst, lf, coarse_wide, bits, x=None):
    """(sx, Eint int64 [Kp]): E_k / s_k = 2^sx * Eint_k, Eint_k = q_0 + sum_c q_c x_kc with x = 1 - 2 b, q = rint(theta / sigma) as
    k_quant_theta quantises at lf planes (x: 1 - 2 bits as float64, if the caller keeps it).  coarse_wide: the top four of seven planes -- what three balanced digits taken off each q
    leave, at 2^24 sigma."""
    sx, q, q0 = quantise(theta_row, Qfp, cconst, lf)
    if coarse_wide:
        q, q0, sx = digits_np(q, 3)[1], int(digits_np(np.array([q0]), 3)[1][0]), sx + 24
    if x is None:
        x = 1.0 - 2.0 * bits.astype(np.float64)  # [Qfp][Kp]
    # q = p0 + 2^24 p1 + 2^48 p2 in 24-bit pieces: each float64 product with the +-1 matrix is an exact integer sum below 2^53
    q1 = q >> 24
    pieces = (q & 0xFFFFFF, q1 & 0xFFFFFF, q1 >> 24)
    e = np.zeros(x.shape[1], dtype=np.int64)
    for j in (2, 1, 0):
        e = e * (1 << 24) + np.rint(pieces[j].astype(np.float64) @ x).astype(np.int64)
    return sx, int(q0) + e


def forward_row(form, lbt, coarse, lf, theta_row, Qfp, cconst, u, sbit, bits, w, tau, K, x=None):
    """One slot's elements.  sbit uint8 [Kp]: the sign bit of spin u (set <=> s = -1); w float64 [Kp]: the weights c_k / M, zero on
    padding; tau: the scale the pass reports.  Returns a dict of arrays over the Kp samples:
      E      float64, s_k 2^sx Eint_k (to the nearest double: only the error bound uses it)
      y      longdouble: (w_k / (unit tau)) F(E_k) + dither(u, k), F = exp(-E) (RISE, logRISE) or 2 / (1 + exp(2 E)) (RPLE)
      mag    int64 rint(y), ties to even; the element's value is V / tau = -s_k unit mag
      margin longdouble |y - the nearest half-integer|
      ymag   longdouble, the first term of y alone (what a relative error of F scales with)
      real   bool: k < K and w_k > 0; the others round the dither alone, to 0"""
    Kp = bits.shape[1]
    lf_q = LF_WIDE if lbt == 6 else (4 if coarse else lf)
    sx, eint = energy_integers(theta_row, Qfp, cconst, lf_q, coarse and lbt == 6, bits, x)
    s = 1 - 2 * sbit.astype(np.int64)
    e_ld = (s * eint).astype(LD) * LD(2.0) ** sx  # exact: |Eint| < 2^63
    unit = COARSE_UNIT[lbt] if coarse else 1
    wt = w.astype(LD) / (LD(tau) * LD(unit))
    if form == "RPLE":
        uu = np.exp(-np.abs(2 * e_ld))
        sig = np.where(e_ld >= 0, uu / (1 + uu), 1 / (1 + uu))
        ymag = 2 * wt * sig
    else:
        ymag = wt * np.exp(-e_ld)
    d = dither(u, np.arange(Kp)).astype(LD) * LD(2.0) ** -32
    y = ymag + d
    fl = np.floor(y)
    margin = np.abs(y - fl - LD(0.5))
    mag = np.rint(y).astype(np.int64)
    real = (np.arange(Kp) < K) & (w > 0)
    mag = np.where(real, mag, 0)
    return dict(E=e_ld.astype(np.float64), y=y, mag=mag, margin=margin, ymag=ymag, real=real, sign=-s, unit=unit)
