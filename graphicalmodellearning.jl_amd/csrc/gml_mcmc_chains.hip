// Long Glauber chains for dense pairwise models on the int8 matrix cores (gml_problem_create_mcmc_chains, include/gml.h).
//
// The same Markov chain as k_glauber (gml_sampler.hip) on the term list {(i,j): A_ij, i < j; (i): A_ii}: sequential-scan
// heat-bath sweeps, P(s_i = +1 | rest) = 1 / (1 + exp(-2 h_i)), the same random numbers.  The local fields come from the
// int8-limb GEMM of gml_i8.h instead of an incidence list:
//   h_i = A_ii + sigma_i sum_{j != i} q_ij s_j,   q_ij = rint(A_ij / sigma_i) in 5 balanced base-256 digit planes,
// sigma_i = 2^(e - 38) with max_{j != i} |A_ij| < 2^e (the rule of the 5-plane Theta of k_quant_theta).  Every sum is an exact
// integer (< n 2^38 < 2^53: held in FP64 without rounding), so the samples depend only on the model, the seed and the run's
// shape -- not on the chain tile, the grid or the device.
//
// One workgroup of NW waves owns CT = 64 NW chains for the whole run; wave w owns the chains [64 w, 64 w + 64) of the tile and
// touches no other wave's state, so the kernel has no grid- and no data-carrying workgroup synchronisation.  The state is held
// as bits in LDS, bits[b][CT] (word b of a chain: spins 32 b .. 32 b + 31, bit set <=> -1).  Per block b of 32 spins:
//   1. GEMM: P_l[i][c] = sum_j d_l[i][j] [s_cj = -1] over all n spins, A = the block's digit planes (Dg, pre-tiled so that one
//      1 KB fragment is one coalesced 16 B load per lane), B = the chain bits expanded to 0/1 bytes; two 32-chain MFMA tiles
//      per wave, 5 planes.  sum_j q_ij s_j = sum_j q_ij - 2 sum_l 256^l P_l  (the form of k_fwd_i8; qsum = sum_j q_ij).
//      The spins of the block itself enter with their values before this sweep's update of the block.
//   2. v_permlane32_swap hands every lane the 32 fields of ONE chain (lane = chain of the wave).
//   3. Update: the lane updates its chain's 32 spins in order; the spins of the block already updated enter through the exact
//      correction  h_i += sum_{j in B, j < i} q_ij (s_j,new - s_j,old)  (the block's 32 x 32 q, read as uniform scalars).
// Recorded sweeps write the states as +-1 bytes, spin-major [n][ld], row t * chains + c.
#include "../../include/gml.h"
#include "gml_dev.h"
#include "gml_i8.h"
#include "gml_chain.h"

namespace gml {

// 16 bits -> 16 bytes 0/1 (bit t <-> byte t): one operand fragment of MFMA_I8
__device__ __forceinline__ v4i expand16(unsigned x) {
    v4i r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned v = (x >> (4 * e)) & 0xFu;
        r[e] = (int)((v & 1u) | ((v & 2u) << 7) | ((v & 4u) << 14) | ((v & 8u) << 21));
    }
    return r;
}

__device__ __forceinline__ void swap_halves(double &x0, double &x1) {
    const unsigned long long a = (unsigned long long)__double_as_longlong(x0), b = (unsigned long long)__double_as_longlong(x1);
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)a, (unsigned)b, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(a >> 32), (unsigned)(b >> 32), false, false);
    x0 = __longlong_as_double((long long)(((unsigned long long)hi[0] << 32) | lo[0]));
    x1 = __longlong_as_double((long long)(((unsigned long long)hi[1] << 32) | lo[1]));
}

// Dg: [nb][nb][5][64 lanes][16 B]: fragment (b, kt, l), lane (il, hh) byte t = digit l of q[32 b + il][32 kt + 16 hh + t]
// qblk: [nb][32][32] the blocks' own q (q_ii = 0) as doubles; diag, sig, qsum: [32 nb] (zero beyond n)
__global__ __launch_bounds__(256) void k_mcmc_chains(const int8_t *__restrict__ Dg, const double *__restrict__ qblk,
                                                     const double *__restrict__ diag, const double *__restrict__ sig,
                                                     const double *__restrict__ qsum, int n, int nb, int64_t chains, int burn_in,
                                                     int thin, int spc, unsigned long long seed, int8_t *__restrict__ out, int64_t ld) {
    extern __shared__ unsigned bits[]; // [nb][CT]
    const int CT = blockDim.x, tid = threadIdx.x, lane = tid & 63, lr = lane & 31, h = lane >> 5;
    const int wc = tid & ~63;                          // the wave's first chain in the tile
    const int64_t c = (int64_t)blockIdx.x * CT + tid; // the chain this lane updates (chains beyond `chains` run but are not stored)
    for (int b = 0; b < nb; ++b) bits[b * CT + tid] = chain_start_word(seed, c, n, b);
    const int sweeps = burn_in + (spc - 1) * thin;
    for (int sw = 0; sw < sweeps; ++sw) {
        const unsigned long long z0 = chain_z0(seed, c, n, sw);
        for (int b = 0; b < nb; ++b) {
            v16i acc[2][5];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int l = 0; l < 5; ++l)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[t][l][e] = 0;
            const int8_t *dp = Dg + (int64_t)b * nb * 5 * 1024 + lane * 16;
            v4i a[5];
#pragma unroll
            for (int l = 0; l < 5; ++l) a[l] = *reinterpret_cast<const v4i *>(dp + l * 1024);
            for (int kt = 0; kt < nb; ++kt) {
                v4i an[5];
                if (kt + 1 < nb) {
#pragma unroll
                    for (int l = 0; l < 5; ++l) an[l] = *reinterpret_cast<const v4i *>(dp + ((int64_t)(kt + 1) * 5 + l) * 1024);
                }
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const v4i bf = expand16(bits[kt * CT + wc + 32 * t + lr] >> (16 * h));
#pragma unroll
                    for (int l = 0; l < 5; ++l) acc[t][l] = MFMA_I8(a[l], bf, acc[t][l]);
                }
                if (kt + 1 < nb) {
#pragma unroll
                    for (int l = 0; l < 5; ++l) a[l] = an[l];
                }
            }
            // acc[t][l][e]: spin 32 b + 8 (e / 4) + 4 h + e % 4, chain wc + 32 t + lr
            double S[2][16];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    double p = (double)acc[t][4][e];
#pragma unroll
                    for (int l = 3; l >= 0; --l) p = fma(p, 256.0, (double)acc[t][l][e]);
                    S[t][e] = fma(-2.0, p, qsum[32 * b + 8 * (e >> 2) + 4 * h + (e & 3)]);
                }
            // afterwards lane (lr, h) holds chain wc + lane: spin 8 g + r (r < 4) in S[0][4 g + r], 8 g + 4 + r in S[1][4 g + r]
#pragma unroll
            for (int e = 0; e < 16; ++e) swap_halves(S[0][e], S[1][e]);
            unsigned word = bits[b * CT + tid];
            const double *qb = qblk + (int64_t)b * 1024;
            const unsigned long long zb = z0 + kU01Step * (unsigned long long)(32 * b);
            double dl[32]; // s_new - s_old of the block's spins updated so far
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int s = 32 * b + i;
                if (s >= n) continue; // (uniform: the padding of the last block)
                double f = (i & 4) ? S[1][4 * (i >> 3) + (i & 3)] : S[0][4 * (i >> 3) + (i & 3)];
#pragma unroll
                for (int j = 0; j < i; ++j) f = fma(qb[i * 32 + j], dl[j], f);
                const unsigned neg = chain_heat_bath(zb, (unsigned long long)i, diag[s] + sig[s] * f);
                const unsigned old = (word >> i) & 1u;
                dl[i] = 2.0 * (double)((int)old - (int)neg);
                word ^= (old ^ neg) << i;
            }
            bits[b * CT + tid] = word;
            __syncthreads(); // not for data (every wave owns its chains): keeps the waves on the same digit fragments (L1 reuse)
        }
        chain_record(sw + 1, burn_in, thin, c, chains, n, nb, bits + tid, CT, out, ld);
    }
}

int mcmc_chains_tile(int64_t n) {
    const int64_t nb = (n + 31) / 32;
    for (int nw = 4; nw >= 1; nw >>= 1)
        if (nb * 64 * nw * 4 <= kMcmcChainsLds) return 64 * nw;
    return 0;
}

void launch_mcmc_chains(const int8_t *dDg, const double *dqblk, const double *ddiag, const double *dsig, const double *dqsum, int64_t n,
                        int64_t chains, int burn_in, int thin, int spc, unsigned long long seed, int8_t *dout, int64_t ld, hipStream_t st) {
    const int CT = mcmc_chains_tile(n);
    const int nb = (int)((n + 31) / 32);
    const int shmem = nb * CT * 4;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mcmc_chains), hipFuncAttributeMaxDynamicSharedMemorySize, shmem);
    hipLaunchKernelGGL(k_mcmc_chains, dim3((unsigned)((chains + CT - 1) / CT)), dim3(CT), shmem, st, dDg, dqblk, ddiag, dsig, dqsum, (int)n,
                       nb, chains, burn_in, thin, spc, seed, dout, ld);
}

} // namespace gml
