// Hessian weights of the int8-limb path (k_make_hw, k_hess_i8_fin in gml_i8_hess.hip): the integer rules that cut a row's 31-bit
// weights to two balanced base-256 digits.  Plain C++ (host and device; tests/native/i8_hw.cpp drives it on the host).
//
// A weight enters as mag >= 0 in the unit of the row's V planes.  With sh = hw_shift(mm, form) the kernel stores
//   h2 = min((mag + hw_dither(node, sample, sh)) >> sh, 32639)
// as the digits (lo, hi) of hw_digits: h2 = lo + 256 hi, lo in -128..127, hi in 0..127 (32 639 = 127 + 256 * 127).
#pragma once
#include "gml_bits.h"

namespace gml {

constexpr int HL = 2; // digit planes of a Hessian weight

// bits by which a row's weights are shifted down so that its largest fits the 15 bits of two balanced digits.  exp forms: mm = the row's largest |V| in the unit
// of the planes, as its last pass recorded it.  RPLE: the passes do not record it, and need not: tau comes from the bound 2 w_max,
// which the weights of a well-classified configuration reach, and h = 4 w sig (1 - sig) <= w_max = half the planes' range (2^30).
GML_HD int hw_shift(unsigned mm, int form) {
    if (form == 2) return 16;
    int sh = 0;
    while ((mm >> sh) + 1u > 32639u) ++sh; // (the dither adds less than one unit after the shift; 32 639 = two balanced digits' largest)
    return sh;
}

// 15 bits below the row's largest, unbiased: a fixed function of (node, sample) in [0, 2^sh) is added before the shift
GML_HD unsigned hw_dither(int u, int64_t k, int sh) {
    const unsigned dmask = (1u << sh) - 1u;
    return ((((unsigned)(k) * 0x9E3779B1u) ^ ((unsigned)u * 0x85EBCA6Bu)) >> 9) & dmask;
}

// the shift and the clip (balanced digits: the high one must stay <= 127); mag as unsigned: RPLE weights reach 2 |V| < 2^32
GML_HD unsigned hw_clip(int mag, unsigned dth, int sh) {
    unsigned long long hq = ((unsigned long long)(unsigned)mag + dth) >> sh;
    return hq > 32639ull ? 32639u : (unsigned)hq;
}

// the two balanced digits of h2 <= 32 639
GML_HD void hw_digits(unsigned h2, int &lo, int &hi) {
    lo = (int)((h2 + 128u) & 255u) - 128;
    hi = ((int)h2 - lo) >> 8;
}

} // namespace gml
