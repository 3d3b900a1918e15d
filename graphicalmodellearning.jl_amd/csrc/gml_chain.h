// The Glauber chain of the samplers (include/gml.h: gml_problem_create_mcmc_terms, _mcmc_chains, _mcmc_terms_chains): its start state,
// its random stream, its heat-bath update and its recorded sweeps, once.  k_glauber, k_mcmc_chains and the term-list kernels differ in
// how they compute the local field h_i and in how they hold the state; everything else that defines the chain is here, so "the same
// chain" is one text.  What only the term-list kernels share is gml_term_field.h.
// Internal, device side.  Chain c of n spins, spin s, sweep sw (0-based, burn-in included); a state bit set <=> the spin is -1.
#pragma once
#include "gml_rng.h"

namespace gml {

// start: spin s of chain c is +1 iff u01(seed, 0xFFFFFFFF, c n + s) < 0.5.  Returns the state bit (1 for -1).
__device__ __forceinline__ unsigned chain_start_bit(unsigned long long seed, int64_t c, int64_t n, int64_t s) {
    return u01(seed, 0xFFFFFFFFull, (unsigned long long)(c * n + s)) < 0.5 ? 0u : 1u;
}

// word b of the start state of the bit-state chains: the spins 32 b .. 32 b + 31 (those below n)
__device__ __forceinline__ unsigned chain_start_word(unsigned long long seed, int64_t c, int n, int b) {
    unsigned word = 0;
    for (int i = 0; i < 32 && 32 * b + i < n; ++i)
        if (chain_start_bit(seed, c, n, 32 * b + i)) word |= 1u << i;
    return word;
}

// the counter word of spin s in sweep sw is chain_z0(seed, c, n, sw) + kU01Step s: that of u01(seed, sw, c n + s), gml_rng.h
// (the stream's + 1 is taken in the caller's type of sw: k_glauber counts sweeps in 64 bits, the bit-state kernels in int, where
// sw + 1 <= 2^31 - 1, the sweep count of a run, cannot overflow)
template <class Sweep>
__device__ __forceinline__ unsigned long long chain_z0(unsigned long long seed, int64_t c, int64_t n, Sweep sw) {
    return seed + kU01Step * ((unsigned long long)(c * n) + 1ull) + kU01Stream * (unsigned long long)(sw + 1);
}

// heat bath of spin s: +1 iff u < pup = 1 / (1 + exp(-2 h)), u the hash of the spin's counter word z0 + kU01Step s and h its local field.
// Returns the state bit and hands back pup (the conditional chains average 2 pup - 1).
__device__ __forceinline__ unsigned chain_heat_bath_pup(unsigned long long z0, unsigned long long s, double field, double *pup_out) {
    const double pup = 1.0 / (1.0 + exp(-2.0 * field));
    *pup_out = pup;
    return u01_mix(z0 + kU01Step * s) < pup ? 0u : 1u;
}

// the same heat bath with pup dropped
__device__ __forceinline__ unsigned chain_heat_bath(unsigned long long z0, unsigned long long s, double field) {
    double pup;
    return chain_heat_bath_pup(z0, s, field, &pup);
}

// is sweep `done` (the number of completed sweeps) a recorded one
__device__ __forceinline__ bool chain_recorded(int done, int burn_in, int thin) {
    if (done < burn_in) return false;
    return (done - burn_in) % thin == 0;
}

// the n spins of a lane whose words are col[b * stride], as +-1 bytes o[s * ld]
__device__ __forceinline__ void chain_unpack(int n, int nw, const unsigned *col, int stride, int8_t *o, int64_t ld) {
    for (int b = 0; b < nw; ++b) {
        const unsigned word = col[b * stride];
        for (int i = 0; i < 32 && 32 * b + i < n; ++i) o[(int64_t)(32 * b + i) * ld] = (word >> i) & 1u ? (int8_t)-1 : (int8_t)1;
    }
}

// A recorded sweep of the bit-state chains: after `done` completed sweeps, chain c (a lane whose words are col[b * stride]) writes its
// state as +-1 bytes, spin-major [n][ld], row (done - burn_in) / thin * chains + c -- if this sweep is recorded and the chain exists.
__device__ __forceinline__ void chain_record(int done, int burn_in, int thin, int64_t c, int64_t chains, int n, int nw, const unsigned *col,
                                             int stride, int8_t *__restrict__ out, int64_t ld) {
    if (done < burn_in || (done - burn_in) % thin != 0 || c >= chains) return;
    chain_unpack(n, nw, col, stride, out + (int64_t)((done - burn_in) / thin) * chains + c, ld);
}

} // namespace gml
