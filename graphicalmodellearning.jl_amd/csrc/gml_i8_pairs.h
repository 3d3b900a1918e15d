// Signed column pairs of the forward sweep of precision i8w (k_fwd_i8w, k_quant_theta<7>).  Plain C++ (host and device;
// tests/native/i8_pairs.cpp drives it on the host).
//
// The statistics are +-1, so for two columns c, c' of a row with quantised integers q, q':  x q + x' q' = x (q + q') if x = x' and
// x (q - q') if not.  A paired Tq image stores the balanced base-256 digit planes of alpha = q + q' and beta = q - q' where a plain one
// stores those of q and q'; four consecutive K slots of the dense MFMA operand are then [alpha1, beta1, alpha2, beta2] of two pairs, and
// the sample operand picks one of the slots {0, 1} and one of {2, 3}, each with the value x = +-1: 2:4 structured sparsity, which
// v_smfmac_i32_32x32x64_i8 multiplies in one instruction per 64-column step where the dense sweep issues two.  The sums are the same
// integers: sum_c x_c q_c = sum_c q_c - 2 sum_c b_c q_c (b = [x = -1], what the dense sweep multiplies).
//
// Which columns pair, and where they sit (operand layout found on the device: scripts/ubench/smfmac_i8_rate.hip).  The bit image of a
// step is unchanged: lane half h of a sample reads dword h, whose bit j is column xb_col(j, h) of the step.  Pair m (0..15) of dword h
// is its bits 2 m (x) and 2 m + 1 (x'): the lane's pick index is then 0x88888888 | ((v ^ v >> 1) & 0x55555555) and the +-1 bytes come
// from the even bits.  Byte m of the lane's sparse operand multiplies K slots 32 (m >> 3) + 16 h + 4 ((m & 7) >> 1) + {0..3}, the pair
// owning the lower two of them for even m and the upper two for odd m: alpha sits at byte pair_slot(h, m) of the row's 64 and beta
// right after it.
#pragma once
#include "gml_bits.h"

namespace gml {

// seven balanced base-256 digits (-128..127 each) spell exactly the integers PAIR_MIN..PAIR_MAX: (256^7 - 1) / 255 = 0x01010101010101
constexpr long long PAIR_UNIT = 0x01010101010101ll, PAIR_MAX = 127 * PAIR_UNIT, PAIR_MIN = -128 * PAIR_UNIT;

// |q|, |q'| <= 2^54 (k_quant_theta): the sum and the difference cannot overflow 64 bits, but they can reach 2^55 > PAIR_MAX.  A tile with
// such a pair in any row keeps plain planes and the dense sweep.
GML_HD bool pair_in_range(long long q, long long qp) {
    const long long a = q + qp, b = q - qp;
    return a >= PAIR_MIN && a <= PAIR_MAX && b >= PAIR_MIN && b <= PAIR_MAX;
}

// digit l of v, and v with l digits taken off: the recurrence k_quant_theta writes its planes by
GML_HD long long balanced_digit(long long &v) {
    const long long d = ((v + 128) & 255) - 128;
    v = (v - d) >> 8;
    return d;
}

// pair m of lane half h within a 64-column step: byte of alpha in the row's 64 bytes of a plane (beta: the next byte) ...
GML_HD int pair_slot(int h, int m) { return 32 * (m >> 3) + 16 * h + 2 * (m & 7); }
// ... and the columns of the step it pairs (second = 0: the column whose x signs the pick; 1: its partner)
GML_HD int pair_col(int h, int m, int second) { return xb_col(2 * m + second, h); }

} // namespace gml
