"""Host model of the working-set Hessians of the int8-limb path (csrc/gml_i8_hess.hip): the cut of a row's 31-bit curvature weights to
two balanced base-256 digits (csrc/gml_i8_hw.h), the compact index of the sub-sample, the byte layout of the weight planes Hq, the
row-major bit image Mb, the integer blocks T_ij and the FP64 finish.  numpy and Python integers only, written from the comments of
those two files, csrc/gml_bits.h and csrc/gml_dev.h (vq_off); it imports and calls nothing compiled from them.
tests/test_host_i8_hess_reference.py pins the digit rules to the header entry for entry; tests/test_gpu_i8_hess_exact.py holds the
device's arrays to the predictions, bit for bit.

    H_r[i][j] = sum_k h_rk x_ki x_kj = S - 2 T_ii - 2 T_jj + 4 T_ij,   T_ij = sum_k h_rk b_ki b_kj,  S = sum_k h_rk,  x = 1 - 2 b

over the Kh configurations of the compact index: block cb of 512 <-> the samples [512 cb kstride, +512)."""
import math

import numpy as np

from _i8_pack_reference import vq_sample, xtb_image

M32 = 0xFFFFFFFF
HL = 2
CLIP = 32639  # 127 + 256 * 127: the largest number two balanced digits with a non-negative high one spell
VQ_SAMPLE = np.array([vq_sample(p) for p in range(64)])
VQ_POS = np.argsort(VQ_SAMPLE)  # position of sample s within its 64


# ---------------------------------------------------------------------------------------------------------------------------
# the digit rules (gml_i8_hw.h)
# ---------------------------------------------------------------------------------------------------------------------------
def hw_shift(mm, form):
    """bits by which a row's weights are shifted down: RPLE 16; exp forms the smallest sh with (mm >> sh) + 1 <= 32639, mm the row's
    largest |V| in the unit of the planes -- in 32-bit unsigned arithmetic, as the kernel forms it"""
    if form == "RPLE":
        return 16
    sh = 0
    while (((int(mm) & M32) >> sh) + 1) & M32 > CLIP:
        sh += 1
    return sh


def dither(u, k, sh):
    """the dither word of (node u, sample k): a fixed function in [0, 2^sh); u scalar, k an int64 array"""
    k = np.asarray(k, dtype=np.int64).astype(np.uint64) & np.uint64(M32)  # (the kernel takes the low 32 bits of the sample index)
    a = (k * np.uint64(0x9E3779B1) & np.uint64(M32)).astype(np.int64)  # (uint64 products wrap; the low 32 bits are the 32-bit product)
    b = (int(u) * 0x85EBCA6B) & M32
    return ((a ^ b) >> 9) & ((1 << sh) - 1)


def clip(mag, dth, sh):
    """h2 = min((mag + dither) >> sh, 32639); mag an unsigned 32-bit number"""
    return np.minimum((np.asarray(mag, dtype=np.int64) + dth) >> sh, CLIP)


def split(h2):
    """the two balanced digits: h2 = lo + 256 hi, lo in -128..127"""
    h2 = np.asarray(h2, dtype=np.int64)
    lo = ((h2 + 128) & 255) - 128
    return lo, (h2 - lo) >> 8


# ---------------------------------------------------------------------------------------------------------------------------
# the sub-sample
# ---------------------------------------------------------------------------------------------------------------------------
def compact_configs(Kh, kstride):
    """configuration of every compact index j < Kh"""
    j = np.arange(Kh, dtype=np.int64)
    return (j >> 9) * kstride * 512 + (j & 511)


# ---------------------------------------------------------------------------------------------------------------------------
# the weights of one row from the V image its last pass left
# ---------------------------------------------------------------------------------------------------------------------------
def v_magnitudes(vq, slot, vpl0, cfg, spin_bits):
    """mag_k = -q_k s_k clamped at 0, q the integer the four planes from vpl0 on spell, s the node's spin (spin_bits: 1 where s = -1).
    vq: the image of gml_test_i8_pass_state as int8 [tiles][Kp / 64][planes][32][64] (bytes of a step in vq_pos order); configurations
    beyond the image (cfg >= Kp) read as zero."""
    Kp = vq.shape[1] * 64
    ok = cfg < Kp
    c = np.where(ok, cfg, 0)
    b = vq[slot >> 5, c >> 6, vpl0:vpl0 + 4, slot & 31, VQ_POS[c & 63]].astype(np.int64)  # [len][4]
    q = b[:, 0] + 256 * (b[:, 1] + 256 * (b[:, 2] + 256 * b[:, 3]))
    q = np.where(ok, q, 0)
    mag = np.where(spin_bits[c] & ok, q, -q)
    return np.maximum(mag, 0)


def rple_magnitudes(mag, tau, vscale, w):
    """RPLE: h = 2 a (1 - a / 2w) of a = |V| in the planes' unit, the kernel's float64 expression; > 2^32 - 256 saturates to 2^32 - 1"""
    tt = np.float64(tau) * np.float64(vscale)
    a = mag.astype(np.float64) * tt
    with np.errstate(divide="ignore", invalid="ignore"):
        hv = np.where(w > 0, np.rint(2.0 * a * (1.0 - a / (2.0 * w)) / tt), 0.0)
    out = np.where(hv > 0.0, np.where(hv < 4294967040.0, hv, float(M32)), 0.0)
    return out.astype(np.int64)


def row_h2(vq, slot, vpl0, node, spin_bits, mm, form, Kh, kstride, tau=None, vscale=None, w=None):
    """h2 [Kh] of one row over the compact index, in natural sample order, and its shift"""
    cfg = compact_configs(Kh, kstride)
    mag = v_magnitudes(vq, slot, vpl0, cfg, spin_bits)
    if form == "RPLE":
        Kp = vq.shape[1] * 64
        wk = np.zeros(Kh)
        ok = cfg < Kp
        wk[ok] = w[cfg[ok]]
        mag = rple_magnitudes(mag, tau, vscale, wk)
    sh = hw_shift(mm, form)
    return clip(mag, dither(node, cfg, sh), sh), sh


# ---------------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------------
def hq_decode(hq, row, Kh):
    """h2 [Kh] in natural sample order from the device's planes hq int8 [tiles][HL][32][pitch]: byte jc + p of a row (jc a multiple of
    64) holds the sample jc + vq_sample(p)"""
    j = np.arange(Kh)
    pos = (j & ~63) + VQ_POS[j & 63]
    d = hq[row >> 5, :, row & 31, :][:, pos].astype(np.int64)
    return d[0] + 256 * d[1]


def hq_encode(h2):
    """int8 [HL][Kh]: the bytes of a row's planes"""
    Kh = len(h2)
    j = np.arange(Kh)
    pos = (j & ~63) + VQ_POS[j & 63]
    lo, hi = split(h2)
    out = np.zeros((HL, Kh), dtype=np.int8)
    out[0, pos] = lo.astype(np.int8)
    out[1, pos] = hi.astype(np.int8)
    return out


def mb_image(B, Kp, Qfp, Qp):
    """Mb uint32 [Qp][Kp / 64][2]: the dwords of Xtb row-major; the rows from Qfp on (constant column, padding) hold zero bits"""
    Qc = (Qfp + 255) // 256 * 256
    nkk = Kp // 64
    x = xtb_image(B, Kp, Qfp).reshape(Qc // 128, nkk, 128, 2).transpose(0, 2, 1, 3).reshape(Qc, nkk, 2)
    out = np.zeros((Qp, nkk, 2), dtype=np.uint32)
    out[:Qfp] = x[:Qfp]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------------------------------------
def t_block(h2, bits):
    """T int64 [m][m] = sum_k h2_k b_ki b_kj; bits uint8 [m][Kh] in natural order.  (float64 GEMM of integers: every sum is below
    32639 Kh < 2^53, exact.)"""
    assert CLIP * len(h2) < 2 ** 53
    Bf = bits.astype(np.float64)
    return np.rint((Bf * h2.astype(np.float64)) @ Bf.T).astype(np.int64)


def finish(T, hS, tau, vscale, sh):
    """ldexp(tau vscale, sh) * (hS - 2 T_ii - 2 T_jj + 4 T_ij) as the kernel forms it: the integer exactly, one float64 product"""
    dg = np.diagonal(T)
    v = int(hS) - 2 * dg[:, None] - 2 * dg[None, :] + 4 * T
    assert np.abs(v).max(initial=0) < 2 ** 53
    return np.float64(math.ldexp(float(np.float64(tau) * np.float64(vscale)), sh)) * v.astype(np.float64)


def lower_tiles(m32):
    """bool [m32][m32]: the 32 x 32 tiles on and below the diagonal, which the kernels fill"""
    t = np.arange(m32) >> 5
    return t[None, :] <= t[:, None]
