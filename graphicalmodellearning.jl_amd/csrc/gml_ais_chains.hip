// Annealed importance sampling of any term list: log Z from chains walked from beta = 0 to beta = 1 (gml_log_partition_ais,
// include/gml.h).
//
// The chain of k_term_chains / k_tempered_chains (gml_term_chains.hip: same model records, exact int64 fields, bit state in LDS,
// scalar-path model), one lane per chain, with two running doubles per lane: the energy E of the lane's state and the log weight.
// The start state is an exact draw at beta = 0; its energy counts every term once, at the smallest spin it names: the start pass is
// term_field on a second set of spin records (spin0) that list, for spin i, only the incidences whose other spins are all above i
// (the host filters; same stream, same quantisation a_i, sigma_i).  Step t adds -(beta_t - beta_(t-1)) E to the log weight -- three
// separately rounded operations, no fused multiply-add -- and then sweeps at beta_t, tracking E -= (s_new - s_old) h_i as the
// tempered kernel does (the product is exact, one rounding per flip).  The schedule is wave-uniform: betas is indexed by the step
// counter only and comes through the scalar path.  Waves share nothing; no barrier.  Every output is written once, at the end.
#include "../../include/gml.h"
#include "gml_dev.h"
#include "gml_term_field.h"

namespace gml {

// logw - (b1 - b0) E: the difference, the product and the subtraction each rounded.  hipcc contracts a * b + c by default, and its
// __dmul_rn / __dsub_rn are the plain operators, which contract too once inlined: the pragma is what forbids the fused multiply-add.
__device__ __forceinline__ double step_weight(double logw, double b1, double b0, double E) {
#pragma clang fp contract(off)
    const double d = b1 - b0;
    const double p = d * E;
    return logw - p;
}

__global__ __launch_bounds__(256) void k_ais_chains(const TermChainSpin *__restrict__ spin, const TermChainSpin *__restrict__ spin0,
                                                    const unsigned *__restrict__ rec, int n, int64_t chains,
                                                    const double *__restrict__ betas, int nsteps, int sps, unsigned long long seed,
                                                    double *__restrict__ logw_out, double *__restrict__ E_out,
                                                    int8_t *__restrict__ states) {
    extern __shared__ unsigned bits[]; // [nw][T]
    const int T = blockDim.x, tid = threadIdx.x, nw = (n + 31) >> 5;
    const int64_t c = (int64_t)blockIdx.x * T + tid; // the chain this lane walks (chains beyond `chains` run but store nothing)
    unsigned *my = bits + tid;
    for (int b = 0; b < nw; ++b) my[b * T] = chain_start_word(seed, c, n, b);
    double E = 0.0;
    for (int i = 0; i < n; ++i) {
        const TermChainSpin &s = spin0[i];
        const double t = s.a + s.sig * term_field(s, rec, my, T); // sigma_i is a power of two: one rounding, fused or not
        const unsigned bit = (my[(i >> 5) * T] >> (i & 31)) & 1u;
        E -= (double)(1 - 2 * (int)bit) * t; // s = 1 - 2 bit
    }
    double logw = 0.0;
    int sw = 0;
    for (int t = 0; t < nsteps; ++t) {
        const double beta = betas[(int64_t)t + 1];
        logw = step_weight(logw, beta, betas[t], E);
        for (int k = 0; k < sps; ++k, ++sw) {
            const unsigned long long z0 = chain_z0(seed, c, n, sw);
            for (int i = 0; i < n; ++i) {
                const TermChainSpin &s = spin[i];
                const double h = s.a + s.sig * term_field(s, rec, my, T);
                const unsigned neg = chain_heat_bath(z0, (unsigned long long)i, beta * h);
                E = chain_energy_step(E, chain_set_spin(my, T, i, neg), neg, h);
            }
        }
    }
    if (c >= chains) return;
    logw_out[c] = logw;
    if (E_out) E_out[c] = E;
    if (states) chain_unpack(n, nw, my, T, states + c * n, 1); // row-major
}

void launch_ais_chains(const TermChainSpin *dspin, const TermChainSpin *dspin0, const unsigned *drec, int64_t n, int64_t chains,
                       const double *dbetas, int64_t nbetas, int sps, unsigned long long seed, double *dlogw, double *dE,
                       int8_t *dstates, hipStream_t st) {
    launch_on_chain_tile(k_ais_chains, term_chains_tile(n, chains), (n + 31) / 32, chains, st, dspin, dspin0, drec, (int)n, chains, dbetas,
                         (int)(nbetas - 1), sps, seed, dlogw, dE, dstates);
}

} // namespace gml
