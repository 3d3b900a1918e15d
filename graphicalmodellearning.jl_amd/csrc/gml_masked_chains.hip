// Conditional Glauber chains whose hidden set is a property of the row (gml_problem_create_mcmc_terms_masked,
// gml_conditional_means_masked, include/gml.h): the chain of k_cond_chains (gml_cond_chains.hip) with "hidden" read per evidence row
// from the sign bits of a second handle, the mask.
//
// One lane per chain, waves share nothing, no barrier, the model through the scalar path, exact int64 fields (gml_term_field.h).  The
// lane holds two bit columns in LDS: its state bits[w][T] and, beside it, its own mask words mbits[w][T] (bit set <=> the spin is
// hidden in this chain's row), both filled in the start pass from Sb of the two handles.
//   start   chain c = r K + k: word by word, a hidden spin from chain_start_bit, an observed one from row k of the evidence.  With
//           MEANS the lane also writes the whole column mean[.][c] here: 0.0 for a hidden entry, the evidence value for an observed one.
//   sweep   a wave must pay for the spins one of its lanes hides, not for n.  Per state word the wave ORs its 64 mask words into a
//           union, takes it through readfirstlane (so the walk below is scalar: s_ff1 / s_and on an SGPR, the spin record through the
//           scalar path) and visits only the set bits, ascending.  At such a spin every lane evaluates the field and the heat bath; a
//           lane writes its bit and adds to its mean only where its own mask bit is set.  The random stream is counter based on
//           (sw, c n + i), so a skipped update changes no bit of any other: the states and means are those of a walk over all n spins
//           predicated per lane, which is the rule.
//   means   as k_cond_chains: on a recorded sweep mean[i][c] += 2 pup - 1 (a coalesced read-modify-write), scaled by
//           1 / samples_per_chain in the last sweep, always a recorded one.
// There is no split of the field into a per-chain constant and a live part: which records are constant depends on the mask, and here
// every lane has its own.
#include "../../include/gml.h"
#include "gml_dev.h"
#include "gml_term_field.h"

namespace gml {

// OR over the 64 lanes of the wave, as a wave-uniform (scalar) value
__device__ __forceinline__ unsigned wave_or(unsigned v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v |= (unsigned)__shfl_xor((int)v, m, 64);
    return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}

template <bool MEANS>
__global__ __launch_bounds__(256) void k_masked_chains(const TermChainSpin *__restrict__ spin, const unsigned *__restrict__ rec,
                                                       const unsigned *__restrict__ Sb, int64_t wpr, const unsigned *__restrict__ Mb,
                                                       int64_t mwpr, int64_t K, int n, int64_t chains, int burn_in, int thin, int spc,
                                                       unsigned long long seed, int8_t *__restrict__ out, int64_t ld,
                                                       double *__restrict__ means) {
    extern __shared__ unsigned bits[]; // [nw][T] state, then [nw][T] mask
    const int T = blockDim.x, tid = threadIdx.x, nw = (n + 31) >> 5;
    const int64_t c = (int64_t)blockIdx.x * T + tid; // the chain this lane updates (chains beyond `chains` hide nothing, store nothing)
    const bool mine = c < chains;
    unsigned *my = bits + tid;
    unsigned *mym = bits + nw * T + tid;
    {
        const int64_t k = c % K; // the row of both handles (a lane beyond `chains` reads a row that exists)
        const unsigned *col = Sb + (k >> 5), *mcol = Mb + (k >> 5);
        const int sh = (int)(k & 31);
        for (int b = 0; b < nw; ++b) {
            unsigned word = 0, mword = 0;
            for (int i = 0; i < 32 && 32 * b + i < n; ++i) {
                const int s = 32 * b + i;
                const unsigned hid = mine ? (mcol[(int64_t)s * mwpr] >> sh) & 1u : 0u;
                const unsigned bit = hid ? chain_start_bit(seed, c, n, s) : (col[(int64_t)s * wpr] >> sh) & 1u;
                word |= bit << i;
                mword |= hid << i;
                if constexpr (MEANS)
                    if (mine) means[(int64_t)s * chains + c] = hid ? 0.0 : (bit ? -1.0 : 1.0);
            }
            my[b * T] = word;
            mym[b * T] = mword;
        }
    }
    const int sweeps = burn_in + (spc - 1) * thin;
    const double inv = 1.0 / (double)spc;
    for (int sw = 0; sw < sweeps; ++sw) {
        const unsigned long long z0 = chain_z0(seed, c, n, sw);
        const bool recorded = chain_recorded(sw + 1, burn_in, thin), last = sw == sweeps - 1;
        for (int b = 0; b < nw; ++b) {
            const unsigned mword = mym[b * T];
            unsigned *wp = my + b * T;
            for (unsigned u = wave_or(mword); u; u &= u - 1) { // the spins of this word that some lane of the wave hides
                const int bit = __builtin_ctz(u), i = 32 * b + bit;
                const TermChainSpin &r = spin[i];
                const long long S = term_field_int(r, rec, my, T);
                const double h = r.a + r.sig * (double)S;
                double pup = 0.0;
                const unsigned neg = chain_heat_bath_pup(z0, (unsigned long long)i, h, &pup);
                if ((mword >> bit) & 1u) {
                    chain_set_bit(wp, bit, neg); // (word pointer and bit index come from the walk)
                    if constexpr (MEANS)
                        if (recorded) chain_mean_add(means + (int64_t)i * chains + c, pup, last, inv);
                }
            }
        }
        if (out) chain_record(sw + 1, burn_in, thin, c, chains, n, nw, my, T, out, ld);
    }
}

// term_chains_tile's rule at twice the words: 64 chains of 2 ceil(n / 32) words fit kMcmcChainsLds up to n = 8192
int masked_chains_tile(int64_t n, int64_t chains) { return term_chains_tile(64 * ((n + 31) / 32), chains); }

void launch_masked_chains(const TermChainSpin *dspin, const unsigned *drec, const unsigned *dSb, int64_t wpr, const unsigned *dMb,
                          int64_t mwpr, int64_t K, int64_t n, int64_t chains, int burn_in, int thin, int spc, unsigned long long seed,
                          int8_t *dout, int64_t ld, double *dmeans, hipStream_t st) {
    auto launch = [&](auto kernel) {
        launch_on_chain_tile(kernel, masked_chains_tile(n, chains), 2 * ((n + 31) / 32), chains, st, dspin, drec, dSb, wpr, dMb, mwpr, K, (int)n,
                             chains, burn_in, thin, spc, seed, dout, ld, dmeans);
    };
    if (dmeans) launch(&k_masked_chains<true>);
    else launch(&k_masked_chains<false>);
}

} // namespace gml
