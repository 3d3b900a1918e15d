"""Host model of one Hessian-vector (product) pass of the int8-limb GEMM kernels, cut at the limb planes Uq of the products u_k: what
k_quant_theta (hv != 0) makes of a direction, what the HV branches of k_fwd_i8 write into Uq from the V planes of another slot, and what
k_bwd_i8 and k_finalize_i8 make of Uq.  numpy, Python integers and fractions only, written from the comments of csrc/gml_i8_pack.hip,
csrc/gml_i8_fwd.hip, csrc/gml_i8_fwd.h, csrc/gml_i8_pass.hip and csrc/gml_i8_bwd.hip; it imports and calls nothing compiled from them.
tests/test_host_i8_hv_reference.py holds it to brute force; tests/test_gpu_i8_hv_exact.py holds the device to it.

One product row r multiplies the curvature weights of the slot vmap[r] of the last objective pass with a direction p:
  q = rint(p / sigma), sigma = 2^(ex - (8 LF - 2)) with max |p| < 2^ex;  qconst = q_0 + sum_c q_c;  emax = fl(sum |q|) sigma
  pn = (emax > 0 ? emax : 1) * (hv == 2 ? fl(65536 * 1.01) : 1);  tau_hv = (tauV[vmap[r]] * vscale) * pn;  invtau = 1 / pn
  hh_k = |the number the four planes vpl0 .. vpl0 + 3 of V[vmap[r]][k] spell|   (vpl0 = 0, vscale = 1: four-plane images; vpl0 = 2,
         vscale = 65536: six-plane images);  RPLE: hh_k <- (2 hh_k) * (1 - (hh_k * tvh) / (2 w_k)), tvh = tauV vscale, 0 where w_k = 0
  Ea_k = sigma (qconst - 2 sum_c q_c b_kc)   (exact: a power of two times an integer below 2^53)
  u_k = rint(fl(hh_k * fl(Ea_k * invtau) + d(node, k)))   -- one fma, then the rounding to an integer, ties to even
for the samples k < Kp with k mod kchunk < kpart; the others keep the bytes an earlier product left.  Behind Uq everything is integers:
csum = sum u, Gacc_l = sum_k u_l b (planes 0, 1 only when hv = 2), G = tau_hv (csum - 2 sum_l 256^l Gacc_l)."""
from fractions import Fraction

import numpy as np

import _i8_pack_reference as R
import _i8_pass_reference as M

LB = 4
PN2 = 65536.0 * 1.01  # the compiler folds the product of the two literals: one rounding, as here
U2MAX = 32639          # the largest number two balanced digits spell
NEAR = 2.0 ** -20      # |y - half-integer| above this: float64 arithmetic decides the rounding (u_of)


# ---------------------------------------------------------------------------------------------------------------------------
# a. the direction (k_quant_theta, hv != 0)
# ---------------------------------------------------------------------------------------------------------------------------
def direction(row, Qfp, cconst, lf, hv, tau_v, vscale, pn_factor=PN2):
    """the scalars and the bytes of one direction (an internal-layout row): sx, sigma, qconst, sabs, emax, pn, tau, invtau, and
    image int8 [Qfp / 64][lf][64].  tau_v: tau of the slot the row's weights come from, as the objective pass reported it."""
    sc = R.row_scalars(row, Qfp, cconst, lf)
    assert sc["sabs"] < 2 ** 53  # (double) of the integer sum is exact
    emax = float(sc["sabs"]) * sc["sigma"]
    pn = (emax if emax > 0.0 else 1.0) * (pn_factor if hv == 2 else 1.0)
    sc.update(emax=emax, pn=pn, tau=(float(tau_v) * float(vscale)) * pn, invtau=1.0 / pn, image=R.row_image(row, Qfp, cconst, lf, False))
    return sc


# ---------------------------------------------------------------------------------------------------------------------------
# b. the curvature weights, from the V planes of the source slot
# ---------------------------------------------------------------------------------------------------------------------------
def hh_planes(vplanes, vpl0):
    """|the number the planes vpl0 .. vpl0 + 3 spell| as int64 [..., Kp]; vplanes int8 [..., lbt, Kp]"""
    v = np.zeros(vplanes.shape[:-2] + vplanes.shape[-1:], dtype=np.int64)
    for l in reversed(range(vpl0, vpl0 + LB)):
        v = v * 256 + vplanes[..., l, :].astype(np.int64)
    return np.abs(v)


def hh_rple(hh, tvh, w):
    """RPLE: 2 a (1 - a tvh / (2 w)) in float64 in the kernel's order -- (2 a) * (1 - (a * tvh) / (2 w)), four roundings at most (the
    doublings are exact) -- and 0 where w = 0 (samples of count zero, padding)"""
    a = hh.astype(np.float64)
    ws = np.where(w > 0.0, w, 1.0)
    return np.where(w > 0.0, (2.0 * a) * (1.0 - (a * float(tvh)) / (2.0 * ws)), 0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# c. x_k . p and the products
# ---------------------------------------------------------------------------------------------------------------------------
def xdotp(row, Qfp, cconst, lf, bits, x=None):
    """Ea float64 [Kp] = sigma (qconst - 2 A_k), exact: asserted to fit 53 bits"""
    sx, eint = M.energy_integers(row, Qfp, cconst, lf, False, bits, x)
    assert max(abs(int(eint.max(initial=0))), abs(int(eint.min(initial=0)))) < 2 ** 53
    return eint.astype(np.float64) * 2.0 ** sx, eint, sx


def _exact_u(hh, e, d32):
    """one element in rational arithmetic: y = hh e + d exactly, to the nearest double (ties to even: CPython's int / int), then to
    the nearest integer (ties to even)"""
    y = Fraction(float(hh)) * Fraction(float(e)) + Fraction(int(d32), 1 << 32)
    return int(np.rint(float(y)))


def u_of(hh, e, d32):
    """u = rint(fl(hh e + d32 2^-32)) as int64: hh, e float64, d32 the dither as an int.  Exact: the float64 evaluation fl(fl(hh e) + d)
    is within 2^-22 of y for |y| < 2^31 (two roundings of half an ulp of 2^-22) and the device's fl(y) within 2^-23, so wherever it
    lies further than NEAR = 2^-20 from a half-integer all three round to the same integer; the other elements (about 2^-19 of them)
    are evaluated in rational arithmetic with the two roundings applied one after the other.  Returns (u, number of those)."""
    hh = np.asarray(hh, dtype=np.float64)
    ya = hh * e + d32.astype(np.float64) * 2.0 ** -32
    assert np.abs(ya).max(initial=0.0) < 2.0 ** 31 - 1.0, "a product leaves 31 bits"
    u = np.rint(ya).astype(np.int64)
    near = np.flatnonzero(np.abs(ya - np.floor(ya) - 0.5) <= NEAR)
    for i in near:
        u[i] = _exact_u(hh[i], e[i], d32[i])
    return u, len(near)


def product_row(form, hh_int, tvh, w, Ea, invtau, node, dither_shift=0):
    """u int64 [Kp] of one product row over ALL samples (the caller masks the part): hh_int the weights of hh_planes, w the sample
    weights (zero on padding), Ea of xdotp, invtau the DEVICE's or the model's 1 / pn"""
    Kp = len(Ea)
    hh = hh_rple(hh_int, tvh, w) if form == "RPLE" else hh_int.astype(np.float64)
    e = Ea * float(invtau)  # one float64 multiply
    d32 = M.dither(node, np.arange(Kp) + dither_shift)
    return u_of(hh, e, d32)


# ---------------------------------------------------------------------------------------------------------------------------
# d. the part of a sub-sampled pass, and the kernel's remap of its compact sample tiles
# ---------------------------------------------------------------------------------------------------------------------------
def participating(Kp, kchunk, kpart):
    """bool [Kp]: k mod kchunk < kpart (kchunk = 0 or kpart = kchunk: every sample)"""
    k = np.arange(Kp)
    return np.ones(Kp, dtype=bool) if not kchunk else (k % kchunk) < kpart


def remap_tiles(Kp, kchunk, kpart):
    """the 256-sample tiles the forward kernel of a sub-sampled pass runs, as it finds them: compact tile st of ntk = nsplit part_tiles
    stands for (st / part_tiles) chunk_tiles + st % part_tiles, and returns early when that tile starts at or beyond Kp"""
    ct, pt = kchunk // 256, kpart // 256
    nsplit = -(-Kp // kchunk)
    if pt == ct:
        return list(range(Kp // 256))
    out = []
    for st in range(nsplit * pt):
        t = (st // pt) * ct + st % pt
        if t * 256 < Kp:
            out.append(t)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# e. behind Uq
# ---------------------------------------------------------------------------------------------------------------------------
def behind_uq(uplanes, part, bits, hv, planes=None):
    """(csum int64 [slots], gacc int64 [slots][4][Qfp]) from the planes int8 [slots][4][Kp] as read back, over the samples of `part`;
    hv = 2 multiplies the planes 0 and 1 only (`planes`: another pair, for the tests of the tests)"""
    pl = np.where(part[None, None, :], uplanes, 0).astype(np.int8)
    csum = M.value_of(pl).sum(axis=1)
    use = list(planes) if planes is not None else ([0, 1] if hv == 2 else [0, 1, 2, 3])
    g = np.zeros((pl.shape[0], LB, bits.shape[0]), dtype=np.int64)
    full = M.backward(pl, bits, False)
    g[:, use] = full[:, use]
    return csum, g


def finalize(tau, csum, gacc, active, Qf, Qp, cconst):
    """G float64 [slots][Qp]: tau (double)(csum - 2 sum_l 256^l Gacc_l) below Qf, tau (double)csum at cconst, 0 elsewhere; NaN rows for
    the slots that are not active"""
    slots = len(csum)
    G = np.full((slots, Qp), np.nan)
    zero = np.zeros(LB, dtype=np.int64)
    for r in range(slots):
        if not active[r]:
            continue
        t = float(tau[r])
        G[r] = 0.0
        G[r, :Qf] = t * M._gcol(LB, False, csum[r], 0, gacc[r, :, :Qf])
        G[r, cconst] = t * float(M._gcol(LB, False, csum[r], 0, zero))
    return G
