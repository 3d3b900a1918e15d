// Exact log Z, means and term expectations of a sparse model by variable elimination (gml_model_elim, include/gml.h):
// the step kernels.  Every table holds logarithms (gml_elim.h: the slots of a table, the scope of a step).
//   k_elim_forward   one launch per step: introduce v_t, add phi_t, sum out up to kElimMaxRetire retiring spins.  The joint over
//                    the scope is never written: the thread of output entry j reads the 2^r inputs it sums, in index order.
//   k_elim_backward  one launch per step and window of kElimQuant quantities: recomputes phi_t, reads alpha_{t-1} and beta_t,
//                    writes beta_{t-1} and reduces the signed sums of p_t = exp(alpha_{t-1} + phi_t + beta_t - alpha_n).
//   k_elim_fold      adds the workgroups' sums, 1024 at a time in index order.
// Every sum has a fixed order and the grids are functions of the table sizes alone: the same arguments give the same bits.
// Streaming FP64 kernels: a forward step reads 2^kin and writes 2^kout doubles, a backward step reads 2^kin + 2^kout and writes 2^kin.
#include "gml_elim.h"

namespace gml {

// phi[c] += the signed weights of the step's terms at the scope states s[c]; the terms in list order, staged in LDS tile by tile
template <int C>
__device__ __forceinline__ void elim_phi(const unsigned *__restrict__ tmask, const double *__restrict__ tw, int nt, const unsigned (&s)[C],
                                         double (&phi)[C], unsigned *lm, double *lw) {
    for (int t0 = 0; t0 < nt; t0 += kElimTermTile) {
        const int cnt = min(kElimTermTile, nt - t0);
        __syncthreads(); // (the tile before has been read)
        if ((int)threadIdx.x < cnt) {
            lm[threadIdx.x] = tmask[t0 + threadIdx.x];
            lw[threadIdx.x] = tw[t0 + threadIdx.x];
        }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            const unsigned m = lm[t];
            const double w = lw[t];
#pragma unroll
            for (int c = 0; c < C; ++c) phi[c] += (__popc(s[c] & m) & 1) ? -w : w;
        }
    }
}

template <int R> __global__ __launch_bounds__(256) void k_elim_forward(const ElimForward S) {
    static_assert(kElimTermTile == 256, "one term per thread and tile");
    __shared__ unsigned lm[kElimTermTile];
    __shared__ double lw[kElimTermTile];
    constexpr int C = 1 << R;
    const unsigned count = 1u << S.kout;
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    const bool live = j < count;
    const unsigned base = elim_scope_of(live ? j : 0u, S.map);
    unsigned s[C];
    double x[C];
    elim_candidates<R>(base, S.rbit, s);
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = 0.0;
    elim_phi<C>(S.tmask, S.tw, S.nt, s, x, lm, lw);
    if (!live) return;
    const unsigned inmask = (1u << S.kin) - 1u;
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = S.in[s[c] & inmask] + x[c];
    double r = x[0];
    if (R > 0) {
        double m = x[0];
#pragma unroll
        for (int c = 1; c < C; ++c) m = fmax(m, x[c]);
        double sum = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) sum += exp(x[c] - m);
        r = m + log(sum);
    }
    S.out[j] = r;
}

__global__ __launch_bounds__(256) void k_elim_backward(const ElimBackward S) {
    __shared__ unsigned lm[kElimTermTile];
    __shared__ double lw[kElimTermTile];
    __shared__ double red[4][kElimQuant];
    constexpr int E = kElimChunk / 256; // entries per thread, two scope states each
    const unsigned count = 1u << S.kin, vbit = 1u << S.kin;
    const int tid = threadIdx.x;
    unsigned s[2 * E];
    double phi[2 * E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const unsigned i = blockIdx.x * (unsigned)kElimChunk + (unsigned)e * 256u + (unsigned)tid;
        s[2 * e] = i < count ? i : 0u;
        s[2 * e + 1] = s[2 * e] | vbit;
        phi[2 * e] = phi[2 * e + 1] = 0.0;
    }
    elim_phi<2 * E>(S.tmask, S.tw, S.nt, s, phi, lm, lw);
    const double log_z = *S.log_z;
    double acc[kElimQuant];
#pragma unroll
    for (int q = 0; q < kElimQuant; ++q) acc[q] = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const unsigned i = blockIdx.x * (unsigned)kElimChunk + (unsigned)e * 256u + (unsigned)tid;
        if (i >= count) continue;
        const double a = S.alpha[i];
        const double b0 = phi[2 * e] + S.beta[elim_index_of(s[2 * e], S.map)];
        const double b1 = phi[2 * e + 1] + S.beta[elim_index_of(s[2 * e + 1], S.map)];
        if (S.beta_out) {
            const double m = fmax(b0, b1);
            S.beta_out[i] = m + log(exp(b0 - m) + exp(b1 - m));
        }
        const double p0 = exp(a + b0 - log_z), p1 = exp(a + b1 - log_z);
#pragma unroll
        for (int q = 0; q < kElimQuant; ++q)
            if (q < S.nq) {
                const unsigned m = S.qmask[q];
                acc[q] += (__popc(s[2 * e] & m) & 1) ? -p0 : p0;
                acc[q] += (__popc(s[2 * e + 1] & m) & 1) ? -p1 : p1;
            }
    }
    // the workgroup's sums: xor-shuffles within a wave (32, 16, ... 1), then the four waves left to right
#pragma unroll
    for (int q = 0; q < kElimQuant; ++q)
        if (q < S.nq) {
            double v = acc[q];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if ((tid & 63) == 0) red[tid >> 6][q] = v;
        }
    __syncthreads();
    if (tid < S.nq) S.part[(size_t)blockIdx.x * S.nq + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

__global__ __launch_bounds__(256) void k_elim_fold(const double *__restrict__ in, long long count, int nq, double *__restrict__ out) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long groups = (count + kElimChunk - 1) / kElimChunk;
    if (id >= groups * nq) return;
    const long long g = id / nq;
    const int q = (int)(id % nq);
    const long long i1 = min(count, (g + 1) * kElimChunk);
    double sum = 0.0;
    for (long long i = g * kElimChunk; i < i1; ++i) sum += in[i * nq + q];
    out[id] = sum;
}

void launch_elim_forward(const ElimForward &S, int r, hipStream_t st) {
    const dim3 grid((unsigned)((((size_t)1 << S.kout) + 255) / 256)), block(256);
    switch (r) {
    case 0: hipLaunchKernelGGL(k_elim_forward<0>, grid, block, 0, st, S); break;
    case 1: hipLaunchKernelGGL(k_elim_forward<1>, grid, block, 0, st, S); break;
    case 2: hipLaunchKernelGGL(k_elim_forward<2>, grid, block, 0, st, S); break;
    default: hipLaunchKernelGGL(k_elim_forward<3>, grid, block, 0, st, S); break;
    }
}

void launch_elim_backward(const ElimBackward &S, hipStream_t st) {
    const size_t wgs = std::max<size_t>(1, ((size_t)1 << S.kin) / kElimChunk);
    hipLaunchKernelGGL(k_elim_backward, dim3((unsigned)wgs), dim3(256), 0, st, S);
}

void launch_elim_fold(const double *in, long long count, int nq, double *out, hipStream_t st) {
    const long long groups = (count + kElimChunk - 1) / kElimChunk;
    hipLaunchKernelGGL(k_elim_fold, dim3((unsigned)((groups * nq + 255) / 256)), dim3(256), 0, st, in, count, nq, out);
}

} // namespace gml
