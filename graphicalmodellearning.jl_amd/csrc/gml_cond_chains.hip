// Conditional Glauber chains: the term-list chain started from the rows of a resident handle, with the observed spins held fixed
// (gml_problem_create_mcmc_terms_conditional, gml_conditional_means, include/gml.h).
//
// The chain of k_term_chains (gml_term_chains.hip: same records, exact int64 fields, bit state bits[w][T] in LDS, one lane per chain,
// waves share nothing, no barrier, the model through the scalar path) with three differences.
//   start   chain c = r K + k takes its visible spins from row k of the evidence handle's sign bits Sb [n][wpr] (bit k & 31 of word
//           k >> 5 of the spin's row) and its hidden spins from chain_start_bit: every state word is composed bit by bit under the
//           hidden mask.  This runs once per chain, so the bits are not transposed.
//   sweep   only the hidden spins hid[0 .. H) are visited, in ascending order, with the counter word of their own index i -- with
//           every spin hidden the chain is k_term_chains's, bit for bit.
//   means   on a recorded sweep the lane adds 2 pup - 1 of every hidden spin to mean[a][c] (global, [H][chains], zeroed by the
//           caller): a coalesced read-modify-write once per recorded sweep and hidden spin; the last sweep, always a recorded one,
//           scales the sum by 1 / samples_per_chain.
// The constant part of the field.  An incidence of hidden spin i whose other spins are all visible contributes the same integer
// to S_i in every sweep of a chain.  With cspin != NULL the host has split the records of every hidden spin into two sets of the one
// stream: cspin[a] (const: all other spins visible) and hspin[a] (live: some other spin hidden), each with its own Q.  After the
// start pass the lane stores cst[a][c] = Q_const - 2 odd_const, term_field_int on the const records; a sweep then takes
// S_i = cst[a][c] + (Q_live - 2 odd_live).  Both parts are exact int64 and so is their sum: the double h_i, hence every bit of the
// result, is that of the walk over all records (cspin == NULL: hspin holds them all).  The constant costs one coalesced 8-byte global
// load per update in place of an LDS read per visible other spin.
#include "../../include/gml.h"
#include "gml_dev.h"
#include "gml_term_field.h"

namespace gml {

// SPLIT: cspin / cst are given; MEANS: means is given.  Both are wave-uniform facts of the launch: as template arguments they cost the
// update loop no branch.
template <bool SPLIT, bool MEANS>
__global__ __launch_bounds__(256) void k_cond_chains(const TermChainSpin *__restrict__ hspin, const TermChainSpin *__restrict__ cspin,
                                                     const int *__restrict__ hid, const uint8_t *__restrict__ hidden,
                                                     const unsigned *__restrict__ rec, const unsigned *__restrict__ Sb, int64_t wpr,
                                                     int64_t K, int n, int H, int64_t chains, int burn_in, int thin, int spc,
                                                     unsigned long long seed, int8_t *__restrict__ out, int64_t ld,
                                                     double *__restrict__ means, long long *cst) {
    extern __shared__ unsigned bits[]; // [nw][T]
    const int T = blockDim.x, tid = threadIdx.x, nw = (n + 31) >> 5;
    const int64_t c = (int64_t)blockIdx.x * T + tid; // the chain this lane updates (chains beyond `chains` run but store nothing)
    const bool mine = c < chains;
    unsigned *my = bits + tid;
    {
        const int64_t k = c % K; // the evidence row (a lane beyond `chains` reads a row that exists)
        const unsigned *col = Sb + (k >> 5);
        const int sh = (int)(k & 31);
        for (int b = 0; b < nw; ++b) {
            unsigned word = 0;
            for (int i = 0; i < 32 && 32 * b + i < n; ++i) {
                const int s = 32 * b + i;
                const unsigned bit = hidden[s] ? chain_start_bit(seed, c, n, s) : (col[(int64_t)s * wpr] >> sh) & 1u;
                word |= bit << i;
            }
            my[b * T] = word;
        }
    }
    if constexpr (SPLIT)
        for (int a = 0; a < H; ++a) {
            const long long v = term_field_int(cspin[a], rec, my, T);
            if (mine) cst[(int64_t)a * chains + c] = v;
        }
    const int sweeps = burn_in + (spc - 1) * thin;
    const double inv = 1.0 / (double)spc;
    for (int sw = 0; sw < sweeps; ++sw) {
        const unsigned long long z0 = chain_z0(seed, c, n, sw);
        const bool recorded = chain_recorded(sw + 1, burn_in, thin), last = sw == sweeps - 1;
        for (int a = 0; a < H; ++a) {
            const TermChainSpin &r = hspin[a];
            const int i = hid[a];
            long long S = term_field_int(r, rec, my, T);
            if constexpr (SPLIT) S += mine ? cst[(int64_t)a * chains + c] : 0;
            const double h = r.a + r.sig * (double)S;
            double pup = 0.0;
            chain_set_spin(my, T, i, chain_heat_bath_pup(z0, (unsigned long long)i, h, &pup));
            if constexpr (MEANS)
                if (recorded && mine) chain_mean_add(means + (int64_t)a * chains + c, pup, last, inv);
        }
        if (out) chain_record(sw + 1, burn_in, thin, c, chains, n, nw, my, T, out, ld);
    }
}

void launch_cond_chains(const TermChainSpin *dhspin, const TermChainSpin *dcspin, const int *dhid, const uint8_t *dhidden,
                        const unsigned *drec, const unsigned *dSb, int64_t wpr, int64_t K, int64_t n, int64_t H, int64_t chains,
                        int burn_in, int thin, int spc, unsigned long long seed, int8_t *dout, int64_t ld, double *dmeans, long long *dcst,
                        hipStream_t st) {
    auto launch = [&](auto kernel) {
        launch_on_chain_tile(kernel, term_chains_tile(n, chains), (n + 31) / 32, chains, st, dhspin, dcspin, dhid, dhidden, drec, dSb, wpr, K,
                             (int)n, (int)H, chains, burn_in, thin, spc, seed, dout, ld, dmeans, dcst);
    };
    const bool split = dcspin != nullptr, want_means = dmeans != nullptr;
    if (split && want_means) launch(&k_cond_chains<true, true>);
    else if (split) launch(&k_cond_chains<true, false>);
    else if (want_means) launch(&k_cond_chains<false, true>);
    else launch(&k_cond_chains<false, false>);
}

} // namespace gml
