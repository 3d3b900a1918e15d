// Device-side pieces shared by the enumeration kernels, k_exact_enumerate (gml_exact.hip), k_exact_best (gml_best.hip) and
// k_cond_exact (gml_cond_exact.hip): the padded LDS vector of one chunk, the radix-16 Walsh-Hadamard passes over it, and the order
// of the selecting forms.  Include from .hip files only.
#pragma once
#include <hip/hip_runtime.h>

namespace gml {

// the transform's vector in LDS: element i at i + (i >> 4), one pad double per 16.  With i = a + 16 b + 256 d (4 bits each) that is
// a + 17 b + 272 d, and the three radix-16 passes read, per ds_read_b64 and half wave:
//   pass A (a in registers, lanes = b, d): stride 34 dwords, 32 distinct even banks -- conflict-free;
//   pass B (b in registers, lanes = a, d): 16 consecutive doubles and 16 more 544 = 32 (mod 64) dwords on -- conflict-free;
//   pass C (d in registers, lanes = a, b): 16 consecutive doubles and 16 more 34 dwords on -- the last lane meets the first on one
//   bank pair (3 LDS cycles instead of 2).
// k_cond_exact keeps two more arrays in LDS.  coef [kCondCoefs] doubles, the row's coefficients in the order of their low masks: the
//   scatter of a chunk reads coef[run_off[s] + i] in thread s -- with one coefficient per low mask (always so for h <= 12) the lanes
//   read consecutive doubles, conflict-free; with runs of r coefficients the stride is 2 r dwords, conflict-free for odd r and
//   gcd(r, 32) ways otherwise (it is one read per coefficient and chunk, against 96 per lane in the passes).  The row's sign bits
//   (514 words) and the partial sums of the row coefficients lie in the transform's vector itself, which the row phase does not
//   use: the bits are read at the words the terms name (a gather: as many ways as lanes meet on a bank with different words,
//   broadcast where they name the same word), the partial sums as k_exact_enumerate reads its own.
__device__ __forceinline__ int exact_pad(int i) { return i + (i >> 4); }

// 16-point Walsh-Hadamard transform in registers: x[k | s] takes the difference (a set bit is a spin of -1)
__device__ __forceinline__ void wht16(double (&x)[16]) {
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k & s) continue;
            const double a = x[k], b = x[k | s];
            x[k] = a + b;
            x[k | s] = a - b;
        }
    }
}

// The order of the best states (k_exact_best, the mode forms of k_cond_exact): energy descending, equal energies state ascending.
// Whether (ea, sa) comes before (eb, sb).
template <class Idx> __device__ __forceinline__ bool best_before(double ea, Idx sa, double eb, Idx sb) {
    return ea > eb || (ea == eb && sa < sb);
}
// The first pair of a workgroup of 256 threads in that order; every thread gets it.  le, ls: 4 elements of LDS each, free again
// after the next barrier.
__device__ __forceinline__ void best_of_block(double &e, unsigned long long &s, double *le, unsigned long long *ls) {
    for (int o = 32; o > 0; o >>= 1) {
        const double oe = __shfl_xor(e, o);
        const unsigned long long os = __shfl_xor(s, o);
        if (best_before(oe, os, e, s)) {
            e = oe;
            s = os;
        }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        le[threadIdx.x >> 6] = e;
        ls[threadIdx.x >> 6] = s;
    }
    __syncthreads();
    e = le[0];
    s = ls[0];
    for (int wv = 1; wv < 4; ++wv)
        if (best_before(le[wv], ls[wv], e, s)) {
            e = le[wv];
            s = ls[wv];
        }
}

__device__ __forceinline__ void exact_load(const double *v, int base, int stride, double (&x)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = v[base + stride * k];
}
__device__ __forceinline__ void exact_store(double *v, int base, int stride, const double (&x)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) v[base + stride * k] = x[k];
}

} // namespace gml
