// Exact log Z and exact expectations of one connected component by streaming enumeration (gml_model_exact, include/gml.h;
// DESIGN 3.18).  No table of 2^sb energies: the component's spins are split into the low kExactChunkBits "chunk" bits and the high
// bits, and one workgroup takes a chunk -- all states of the low bits at one setting h of the high bits -- through LDS:
//   1. every term is (sign of its high part at h) x (a mask over the low bits): the signed weights are summed per low mask into a
//      coefficient vector (the host has sorted the terms by low mask and cut every mask's run into items of at most L terms, so
//      every sum has a fixed order; no atomics);
//   2. a Walsh-Hadamard transform of the coefficients gives the energies of all states of the chunk;
//   3. p = exp(E - m) with the running maximum m of the accumulation group;
//   4. a second Walsh-Hadamard transform of p gives S[mask] = sum_x p(x) chi_mask(x) for every low mask at once, so a query term
//      costs one signed pick S[low mask] x sign(high part at h) per chunk.  S[0] is the chunk's share of Z.
// A component of c < kExactChunkBits low bits runs the same transforms: the bits above c belong to no term, every sum over them is
// an exact doubling, and the host takes the factor 2^(kExactChunkBits - c) out of Z again.
// Group g of G takes the chunks [g cpg, (g + 1) cpg) in order, 1024 chunks into a first accumulator and those into a second, each
// with its own running maximum; k_exact_combine adds the groups in index order.  G and cpg are functions of (sb, c) alone, so the
// result is a function of the model alone.
#include "../../include/gml.h"
#include "gml_dev.h"
#include "gml_exact_wht.h"
#include "gml_wg.h"

namespace gml {

__global__ __launch_bounds__(256) void k_exact_enumerate(const ExactPlan P) {
    __shared__ double v[kExactVec], part[kExactParts], red[4];
    const int tid = threadIdx.x;
    // thread tid owns the queries tid + 256 j: their masks and both accumulators stay in registers
    constexpr int kOwn = kExactWindow / 256;
    int qlo[kOwn];
    unsigned long long qhi[kOwn];
    double acc0[kOwn], acc1[kOwn];
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
        const int q = tid + 256 * j;
        qlo[j] = q < P.nq ? exact_pad(P.q_lo[q]) : 0;
        qhi[j] = q < P.nq ? P.q_hi[q] : 0ull;
        acc0[j] = acc1[j] = 0.0;
    }
    double m0 = -INFINITY, m1 = -INFINITY; // the running maxima of the two accumulators (the same in every thread)
    const int baseA = 17 * tid, baseB = (tid & 15) + 272 * (tid >> 4), baseC = (tid & 15) + 17 * (tid >> 4);
    double x[16];
    for (long long k = 0; k < P.cpg; ++k) {
        const unsigned long long h = (unsigned long long)blockIdx.x * (unsigned long long)P.cpg + (unsigned long long)k;
        __syncthreads(); // (the picks of the chunk before have read v)
#pragma unroll
        for (int e = 0; e < 16; ++e) v[baseA + e] = 0.0;
        __syncthreads();
        // 1. the coefficient vector: items in term order; the only item of a low mask writes its slot, the others a partial sum
        for (int it = tid; it < P.ni; it += 256) {
            double s = 0.0;
            for (int t = P.item_off[it], t1 = P.item_off[it + 1]; t < t1; ++t) s += (__popcll(P.hi[t] & h) & 1) ? -P.w[t] : P.w[t];
            const int dst = P.item_dst[it];
            if (dst >= 0) v[dst] = s;
            else part[~dst] = s;
        }
        if (P.nm) {
            __syncthreads();
            for (int s = tid; s < P.nm; s += 256) { // (at most kExactParts partial sums in all)
                double sum = 0.0;
                for (int a = P.ms_off[s], a1 = P.ms_off[s + 1]; a < a1; ++a) sum += part[a];
                v[P.ms_dst[s]] = sum;
            }
        }
        __syncthreads();
        // 2. energies of the chunk's states: passes A, B, C; the last stays in registers
        exact_load(v, baseA, 1, x);
        wht16(x);
        exact_store(v, baseA, 1, x);
        __syncthreads();
        exact_load(v, baseB, 17, x);
        wht16(x);
        exact_store(v, baseB, 17, x);
        __syncthreads();
        exact_load(v, baseC, 272, x);
        wht16(x);
        // 3. p = exp(E - m0) at the group's running maximum; a chunk that raises it rescales what has been accumulated
        double mx = x[0];
#pragma unroll
        for (int e = 1; e < 16; ++e) mx = fmax(mx, x[e]);
        const double mn = fmax(m0, block_max(mx, red));
        const double scale = exp(m0 - mn); // (0 at the first chunk: m0 = -inf)
        m0 = mn;
#pragma unroll
        for (int e = 0; e < 16; ++e) x[e] = exp(x[e] - m0);
        // 4. S = WHT(p): passes C, B, A
        wht16(x);
        exact_store(v, baseC, 272, x);
        __syncthreads();
        exact_load(v, baseB, 17, x);
        wht16(x);
        exact_store(v, baseB, 17, x);
        __syncthreads();
        exact_load(v, baseA, 1, x);
        wht16(x);
        exact_store(v, baseA, 1, x);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kOwn; ++j) { // (a slot beyond nq picks S[0] and is never written out)
            const double val = v[qlo[j]];
            acc0[j] = acc0[j] * scale + ((__popcll(qhi[j] & h) & 1) ? -val : val);
        }
        if ((k & (kExactBlock - 1)) == kExactBlock - 1 || k == P.cpg - 1) { // at most kExactBlock chunks in acc0: on to acc1
            const double mn1 = fmax(m1, m0), s1 = exp(m1 - mn1), s0 = exp(m0 - mn1);
#pragma unroll
            for (int j = 0; j < kOwn; ++j) {
                acc1[j] = acc1[j] * s1 + acc0[j] * s0;
                acc0[j] = 0.0;
            }
            m1 = mn1;
            m0 = -INFINITY;
        }
    }
    if (tid == 0) P.gm[blockIdx.x] = m1;
#pragma unroll
    for (int j = 0; j < kOwn; ++j)
        if (tid + 256 * j < P.nq) P.gacc[(size_t)blockIdx.x * P.nq + tid + 256 * j] = acc1[j];
}

// res[q] = sum_g gacc[g][q] exp(gm[g] - M) in group order, M = max_g gm[g] -> res[nq]
__global__ __launch_bounds__(256) void k_exact_combine(const double *__restrict__ gm, const double *__restrict__ gacc, int G, int nq,
                                                       double *__restrict__ res) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    double M = gm[0];
    for (int g = 1; g < G; ++g) M = fmax(M, gm[g]);
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += gacc[(size_t)g * nq + q] * exp(gm[g] - M);
    res[q] = s;
    if (q == 0) res[nq] = M;
}

void launch_exact(const ExactPlan &P, int G, double *dres, hipStream_t st) {
    hipLaunchKernelGGL(k_exact_enumerate, dim3((unsigned)G), dim3(256), 0, st, P);
    hipLaunchKernelGGL(k_exact_combine, dim3((unsigned)((P.nq + 255) / 256)), dim3(256), 0, st, P.gm, P.gacc, G, P.nq, dres);
}

} // namespace gml
