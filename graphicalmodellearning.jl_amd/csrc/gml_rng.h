// The samplers' random numbers (gml_sampler.hip, gml_mcmc_chains.hip): a counter-based splitmix64 hash of (seed, stream, k)
// -> a double in [0, 1) with 53 random bits.  Internal, device side.  Its bits are part of what the samplers promise (the same
// seed gives the same draws on every device and tiling), so this is the one definition both kernels use.
#pragma once
#include <hip/hip_runtime.h>

namespace gml {

constexpr unsigned long long kU01Step = 0x9E3779B97F4A7C15ull;   // per counter k
constexpr unsigned long long kU01Stream = 0xD1B54A32D192ED03ull; // per stream (block / sweep)
// The stream of the fold labels (gml_split.hip: unit g of a handle lies in fold floor(nfolds u01(seed, kU01FoldStream, g))).  The
// samplers count their streams up from 0: a handle sampled with seed s and split with seed s shares no draw with its sampler.
constexpr unsigned long long kU01FoldStream = 0x8000000000000000ull;

// the hash of a counter word z = seed + kU01Step (k + 1) + kU01Stream (stream + 1)  (mod 2^64)
__device__ __forceinline__ double u01_mix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ double u01(unsigned long long seed, unsigned long long stream, unsigned long long k) {
    return u01_mix(seed + kU01Step * (k + 1) + kU01Stream * (stream + 1));
}

} // namespace gml
