// Device-side pieces shared by the solver's kernels (gml_solver.hip) and the batched Newton solve (gml_newton_solve.hip):
// the reductions over a workgroup of 256 threads and the orthant-face rule.  Include from .hip files only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gml {

// Sum / maximum over the 256 threads of a workgroup; every thread gets the result.  Order: xor-shuffles within a wave (32, 16, ... 1),
// then the four waves' values left to right.  red: 4 elements of LDS, free again after the next barrier.
__device__ __forceinline__ double block_sum(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ double block_max(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}
__device__ __forceinline__ int block_sum_i(int v, int *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// The orthant-face rule.  The line search projects a step onto the orthant of the iterate: a penalised entry (kind 2) at zero may
// only move against its pseudo-gradient, a non-zero one not past zero.  Whether the step d of an entry at x with pseudo-gradient pg
// leaves that face; *fixed: the step the projection leaves it with (to zero, or none).
__device__ __forceinline__ bool face_candidate(double x, double d, double pg, uint8_t kind, double *fixed) {
    *fixed = x == 0.0 ? 0.0 : -x;
    return kind == 2 && (x == 0.0 ? d * pg > 0.0 : (x + d) * x < 0.0);
}

} // namespace gml
