// Replica-exchange (parallel tempering) chains of any term list (gml_problem_create_mcmc_terms_tempered, include/gml.h).
//
// The chain of k_term_chains (gml_term_chains.hip: same model records, exact int64 fields, bit state in LDS, scalar-path model) run at
// R inverse temperatures per ladder.  One lane per rung: lane c = l R + r is rung r of ladder l, and R divides 64, so a ladder is R
// neighbouring lanes of one wave (the tile is a multiple of 64).  Rung r updates at beta_r with the stream of chain c and tracks its
// energy relative to the ladder's common start state, E -= (s_new - s_old) h_i: the product is exact (0 or +-2 h_i), one rounding per
// flip.  A swap round needs nothing outside the wave: the partner's E and beta come through a cross-lane read, both lanes of a pair
// decide from the same hash, and the pair exchanges its state words through its two LDS columns -- every lane reads its partner's
// word, then the accepting lanes write their own; the two are one ds_read and one ds_write of the same wave, which LDS executes in
// program order.  No workgroup barrier anywhere.  The random stream, beta and the swap counters belong to the rung (the lane); the
// state and its energy travel.  Rung 0 is recorded, after the swap.
#include "../../include/gml.h"
#include "gml_dev.h"
#include "gml_term_field.h"

namespace gml {

// v summed over the lanes of the wave that hold the same rung (lane mod R): the ladders of one wave
__device__ __forceinline__ unsigned long long sum_over_ladders(unsigned long long v, int R) {
    for (int off = R; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_tempered_chains(const TermChainSpin *__restrict__ spin, const unsigned *__restrict__ rec, int n,
                                                         int64_t ladders, int R, const double *__restrict__ betas, int swap_every,
                                                         int burn_in, int thin, int spc, unsigned long long seed,
                                                         int8_t *__restrict__ out, int64_t ld,
                                                         unsigned long long *__restrict__ swap_counts) {
    extern __shared__ unsigned bits[]; // [nw][T]
    const int T = blockDim.x, tid = threadIdx.x, nw = (n + 31) >> 5;
    const int64_t c = (int64_t)blockIdx.x * T + tid; // the rung this lane updates (ladders beyond `ladders` run but are not stored)
    const int r = (int)(c & (R - 1));
    const int64_t ladder = c / R;
    const double beta = betas[r];
    unsigned *my = bits + tid;
    for (int b = 0; b < nw; ++b) my[b * T] = chain_start_word(seed, c - r, n, b); // every rung starts from the state of chain l R
    double E = 0.0;                                                                // relative to that start
    unsigned attempts = 0, accepts = 0;                                            // of the pair (r, r + 1), held by lane r
    const int sweeps = burn_in + (spc - 1) * thin;
    for (int sw = 0; sw < sweeps; ++sw) {
        const unsigned long long z0 = chain_z0(seed, c, n, sw);
        for (int i = 0; i < n; ++i) {
            const TermChainSpin &s = spin[i];
            const double h = s.a + s.sig * term_field(s, rec, my, T);
            const unsigned neg = chain_heat_bath(z0, (unsigned long long)i, beta * h);
            E = chain_energy_step(E, chain_set_spin(my, T, i, neg), neg, h);
        }
        const int done = sw + 1;
        if (R > 1 && done % swap_every == 0) {
            // round m = done / swap_every pairs (r, r + 1) for r = m - 1 (mod 2).  All lanes take the cross-lane reads (a lane
            // without a partner reads itself); the hash is that of the pair's lower rung.
            const int parity = (done / swap_every - 1) & 1;
            const bool lower = (r & 1) == parity;
            const int pr = lower ? r + 1 : r - 1;
            const int d = pr >= 0 && pr < R ? pr - r : 0;
            const int src = (tid & 63) + d;
            const double Ep = __shfl(E, src, 64), bp = __shfl(beta, src, 64);
            const double dd = lower ? (beta - bp) * (E - Ep) : (bp - beta) * (Ep - E);
            const double u = u01(seed, 0x100000000ull + (unsigned long long)sw, (unsigned long long)(lower ? c : c - 1));
            const bool swap = d != 0 && u < exp(fmin(dd, 0.0));
            for (int b = 0; b < nw; ++b) {
                const unsigned theirs = my[b * T + d];
                if (swap) my[b * T] = theirs;
            }
            if (swap) E = Ep;
            if (lower && d != 0) attempts += 1u, accepts += swap ? 1u : 0u;
        }
        if (r == 0) chain_record(done, burn_in, thin, ladder, ladders, n, nw, my, T, out, ld);
    }
    if (R > 1) {
        // [2][R - 1] attempts, accepts: the ladders of a wave summed across lanes, one atomic per wave, pair and counter
        const bool counted = ladder < ladders;
        const unsigned long long att = sum_over_ladders(counted ? attempts : 0u, R), acc = sum_over_ladders(counted ? accepts : 0u, R);
        if ((tid & 63) < R - 1) {
            if (att) atomicAdd(swap_counts + r, att);
            if (acc) atomicAdd(swap_counts + (R - 1) + r, acc);
        }
    }
}

void launch_tempered_chains(const TermChainSpin *dspin, const unsigned *drec, int64_t n, int64_t ladders, int replicas,
                            const double *dbetas, int swap_every, int burn_in, int thin, int spc, unsigned long long seed, int8_t *dout,
                            int64_t ld, unsigned long long *dswap_counts, hipStream_t st) {
    const int64_t lanes = ladders * replicas;
    launch_on_chain_tile(k_tempered_chains, term_chains_tile(n, lanes), (n + 31) / 32, lanes, st, dspin, drec, (int)n, ladders, replicas,
                         dbetas, swap_every, burn_in, thin, spc, seed, dout, ld, dswap_counts);
}

} // namespace gml
