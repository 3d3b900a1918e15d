// The toolkit of the term-list chains (k_term_chains, k_tempered_chains, k_ais_chains, k_cond_chains, k_masked_chains), on top of the
// chain's definition in gml_chain.h.  First the exact integer field: the odd part of a spin's incidence records,
//   sum_e q_e prod_{j in others(e)} s_j = Q_i - 2 sum_{e: prod = -1} q_e,
// read from the record stream of TermChainSpin (gml_dev.h) through the scalar path and from the lane's bit-state column in LDS,
// bits[w][T] (word w of a chain: spins 32 w .. 32 w + 31, bit set <=> -1).  Then the steps on that column that the kernels share
// (bit write, energy step, means update): device side, like gml_chain.h.  Last, host side, the one launch of a kernel on a chain tile.
// Internal.  (The file keeps the name it had when it held the field alone: the field is still most of it.)
#pragma once
#include <hip/hip_runtime.h>
#include "gml_dev.h"
#include "gml_chain.h"

namespace gml {

// q_e if the product of the other spins of the record r is -1 (an odd number of set bits), else 0.  my: the lane's chain column.
template <int K>
__device__ __forceinline__ long long odd_q(const unsigned *r, const unsigned *my, int T) {
    const unsigned w0 = r[0];
    const long long q = (long long)(((unsigned long long)r[1] << 32) | w0) >> 24;
    unsigned j = w0 & 0xFFFFFFu;
    unsigned p = my[(j >> 5) * T] >> (j & 31);
#pragma unroll
    for (int m = 2; m <= K; ++m) {
        j = r[m];
        p ^= my[(j >> 5) * T] >> (j & 31);
    }
    const unsigned m = (unsigned)((int)(p << 31) >> 31); // 0 or ~0
    return q & (long long)(((unsigned long long)m << 32) | m);
}

// G records from word e on: one wait for their scalar loads, G independent LDS reads (per other spin) in flight
template <int K, int G>
__device__ __forceinline__ long long odd_step(const unsigned *__restrict__ rec, long long e, const unsigned *my, int T) {
    long long acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = odd_q<K>(rec + e + g * (K + 1), my, T);
#pragma unroll
    for (int w = 1; w < G; w <<= 1)
#pragma unroll
        for (int g = 0; g + w < G; g += 2 * w) acc[g] += acc[g + w];
    return acc[0];
}

// the odd part of the records with K other spins in the words [beg, end).  Every step waits for its scalar loads (one wave per SIMD
// at 65 536 chains: nothing else hides them), so a list is walked in the largest steps that fit -- up to 32 words of records
// (16 pairs, 8 triples, 4 records beyond) -- and a short one still takes one wait per 4 records, not one per record.
template <int K>
__device__ __forceinline__ long long odd_sum(const unsigned *__restrict__ rec, long long beg, long long end, const unsigned *my, int T) {
    constexpr int R = K + 1, G = K == 1 ? 16 : K == 2 ? 8 : 4;
    long long s = 0, e = beg;
    for (; e + G * R <= end; e += G * R) s += odd_step<K, G>(rec, e, my, T);
    if constexpr (G > 8) {
        if (e + 8 * R <= end) s += odd_step<K, 8>(rec, e, my, T), e += 8 * R;
    }
    if constexpr (G > 4) {
        if (e + 4 * R <= end) s += odd_step<K, 4>(rec, e, my, T), e += 4 * R;
    }
    for (; e < end; e += R) s += odd_q<K>(rec + e, my, T);
    return s;
}

// sum_e q_e prod_{j in others(e)} s_j of the spin record r as the exact int64 (k_cond_chains adds a per-chain constant before it converts)
__device__ __forceinline__ long long term_field_int(const TermChainSpin &r, const unsigned *__restrict__ rec, const unsigned *my, int T) {
    long long odd = odd_sum<1>(rec, r.off[0], r.off[1], my, T);
    odd += odd_sum<2>(rec, r.off[1], r.off[2], my, T);
    odd += odd_sum<3>(rec, r.off[2], r.off[3], my, T);
    odd += odd_sum<4>(rec, r.off[3], r.off[4], my, T);
    odd += odd_sum<5>(rec, r.off[4], r.off[5], my, T);
    odd += odd_sum<6>(rec, r.off[5], r.off[6], my, T);
    odd += odd_sum<7>(rec, r.off[6], r.off[7], my, T);
    return r.Q - 2 * odd;
}

// the same as a double: the int64 sum is exact and converts exactly
__device__ __forceinline__ double term_field(const TermChainSpin &r, const unsigned *__restrict__ rec, const unsigned *my, int T) {
    return (double)term_field_int(r, rec, my, T);
}

// ------------------------------------------------------------------------------------------
// The steps of a chain on that column that more than one kernel takes.
// ------------------------------------------------------------------------------------------
// write the state bit `neg` at bit `bit` of the word *wp; returns the bit that was there
__device__ __forceinline__ unsigned chain_set_bit(unsigned *wp, int bit, unsigned neg) {
    const unsigned word = *wp, old = (word >> bit) & 1u;
    *wp = (word & ~(1u << bit)) | (neg << bit);
    return old;
}
// the same for spin i of the lane's column
__device__ __forceinline__ unsigned chain_set_spin(unsigned *my, int T, int i, unsigned neg) {
    return chain_set_bit(my + (i >> 5) * T, i & 31, neg);
}

// the energy after spin i went from bit `old` to bit `neg` in the field h: E - (s_new - s_old) h with s = 1 - 2 bit, so
// s_new - s_old = 2 (old - neg); the product is exact (0 or +-2 h), one rounding per flip
__device__ __forceinline__ double chain_energy_step(double E, unsigned old, unsigned neg, double h) {
    return E - (double)(2 * ((int)old - (int)neg)) * h;
}

// the Rao-Blackwellised mean of a spin on a recorded sweep: *m += 2 pup - 1, times inv = 1 / samples_per_chain on the last sweep
// (always a recorded one).  A coalesced read-modify-write: m is the lane's entry of a [.][chains] array.
__device__ __forceinline__ void chain_mean_add(double *m, double pup, bool last, double inv) {
    const double v = *m + (2.0 * pup - 1.0);
    *m = last ? v * inv : v;
}

// Host side: launch `kernel` with one lane per chain on tiles of T lanes, `words` LDS words per lane (ceil(n / 32) state words, or
// twice that with the mask words beside them)
template <class... P, class... A>
void launch_on_chain_tile(void (*kernel)(P...), int T, int64_t words, int64_t lanes, hipStream_t st, A... args) {
    const int shmem = (int)words * T * 4;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, shmem);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((lanes + T - 1) / T)), dim3(T), shmem, st, args...);
}

} // namespace gml
