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
#include "gml_term_field.h"

namespace gml {

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
            const double f = term_field(r, rec, my, T);
            const unsigned neg = chain_heat_bath(z0, (unsigned long long)i, r.a + r.sig * f);
            chain_set_spin(my, T, i, neg);
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
    launch_on_chain_tile(k_term_chains, term_chains_tile(n, chains), (n + 31) / 32, chains, st, dspin, drec, (int)n, chains, burn_in, thin,
                         spc, seed, dout, ld);
}

} // namespace gml
