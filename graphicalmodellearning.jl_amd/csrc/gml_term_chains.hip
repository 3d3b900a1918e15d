// Long Glauber chains of any term list with exact integer fields (gml_problem_create_mcmc_terms_chains, include/gml.h).
//
// The chain of k_glauber / k_mcmc_chains (same start, scan order, update formula and u01 stream) on the incidence lists of
// create_mcmc_terms, with the couplings of spin i quantised as w_e = sigma_i q_e (sigma_i = 2^(E - 38), max_e |w_e| < 2^E):
//   h_i = a_i + sigma_i (double) sum_e q_e prod_{j in others(e)} s_j,   sum_e q_e prod s_j = Q_i - 2 sum_{e: prod = -1} q_e,
// with Q_i = sum_e q_e.  The sum is exact in int64, so the samples do not depend on the order of the incidences, the chain tile, the
// grid or the device; on the term list of a pairwise matrix h_i is the double k_mcmc_chains computes.
//
// One lane per chain; a workgroup owns T chains for the whole run and its waves share nothing (no barrier).  The state is held as
// bits in LDS, bits[w][T] (word w of a chain: spins 32 w .. 32 w + 31, bit set <=> -1): every lane of a wave reads the same word
// index of its own chain, one conflict-free ds_read_b32 per other spin.  The model is wave-uniform (the wave updates spin i of its 64
// chains at once and walks spin i's incidences), so the spin records and the incidence stream are read through the scalar path.
// The incidences of a spin are grouped by arity, so the inner loops do not branch on it.  Recorded sweeps write the states as
// +-1 bytes, spin-major [n][ld], row t * chains + c.
#include "../../include/gml.h"
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

__global__ __launch_bounds__(256) void k_term_chains(const TermChainSpin *__restrict__ spin, const unsigned *__restrict__ rec, int n,
                                                     int64_t chains, int burn_in, int thin, int spc, unsigned long long seed,
                                                     int8_t *__restrict__ out, int64_t ld) {
    extern __shared__ unsigned bits[]; // [nw][T]
    const int T = blockDim.x, tid = threadIdx.x, nw = (n + 31) >> 5;
    const int64_t c = (int64_t)blockIdx.x * T + tid; // the chain this lane updates (chains beyond `chains` run but are not stored)
    unsigned *my = bits + tid;
    for (int b = 0; b < nw; ++b) my[b * T] = chain_start_word(seed, c, n, b);
    const int sweeps = burn_in + (spc - 1) * thin;
    for (int sw = 0; sw < sweeps; ++sw) {
        const unsigned long long z0 = chain_z0(seed, c, n, sw);
        for (int i = 0; i < n; ++i) {
            const TermChainSpin &r = spin[i];
            long long odd = odd_sum<1>(rec, r.off[0], r.off[1], my, T);
            odd += odd_sum<2>(rec, r.off[1], r.off[2], my, T);
            odd += odd_sum<3>(rec, r.off[2], r.off[3], my, T);
            odd += odd_sum<4>(rec, r.off[3], r.off[4], my, T);
            odd += odd_sum<5>(rec, r.off[4], r.off[5], my, T);
            odd += odd_sum<6>(rec, r.off[5], r.off[6], my, T);
            odd += odd_sum<7>(rec, r.off[6], r.off[7], my, T);
            const double f = (double)(r.Q - 2 * odd);
            const unsigned neg = chain_heat_bath(z0, (unsigned long long)i, r.a + r.sig * f);
            unsigned *wp = my + (i >> 5) * T;
            *wp = (*wp & ~(1u << (i & 31))) | (neg << (i & 31));
        }
        chain_record(sw + 1, burn_in, thin, c, chains, n, nw, my, T, out, ld);
    }
}

// The tile: the largest of 256, 128, 64 chains whose state fits 64 KiB (two workgroups per CU at least; n <= 2048: 256, <= 4096:
// 128, <= 8192: 64), 64 chains in up to kMcmcChainsLds beyond; then halved (down to 64) while the grid would leave CUs idle.
int term_chains_tile(int64_t n, int64_t chains) {
    const int64_t nw = (n + 31) / 32;
    const int forced = g_term_chains_tile;
    if ((forced == 64 || forced == 128 || forced == 256) && nw * forced * 4 <= kMcmcChainsLds) return forced;
    int T = 256;
    while (T > 64 && nw * T * 4 > 64 * 1024) T >>= 1;
    if (nw * T * 4 > kMcmcChainsLds) return 0;
    while (T > 64 && (chains + T - 1) / T < 256) T >>= 1;
    return T;
}

void launch_term_chains(const TermChainSpin *dspin, const unsigned *drec, int64_t n, int64_t chains, int burn_in, int thin, int spc,
                        unsigned long long seed, int8_t *dout, int64_t ld, hipStream_t st) {
    const int T = term_chains_tile(n, chains);
    const int shmem = (int)((n + 31) / 32) * T * 4;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_term_chains), hipFuncAttributeMaxDynamicSharedMemorySize, shmem);
    hipLaunchKernelGGL(k_term_chains, dim3((unsigned)((chains + T - 1) / T)), dim3(T), shmem, st, dspin, drec, (int)n, chains, burn_in,
                       thin, spc, seed, dout, ld);
}

} // namespace gml
