// Ingest conversion kernels and the FP64 working-set Hessian.  gfx950 only.
//   k_convert_hist   a histogram [K][1 + n] of any supported type, row- or column-major -> counts and +-1 spins (first bad row noted)
//   k_check_pm1      whether spins given as int8 are all +-1
//   k_transpose_i8   spins [K][n] <-> [n][K]
//   k_hess_f64       H_r += sum_k h_rk x_k x_k^T on the lower 32 x 32 tiles of a row's working set: an "NT" product on
//                    v_mfma_f64_16x16x4_f64 with the +-1 operand converted from int8 in registers; operands go straight from global
//                    memory / L2 to VGPRs (one f64 MFMA takes 64 cycles per SIMD, which leaves ample time for the few loads per
//                    step), no LDS.  h_rk is the second derivative of the formulation's sample term (below).
// (The GEMM-shaped kernels of the pass -- energies + pointwise, gradient -- live in gml_kernels_f64gemm.hip; the solves that consume
// the Hessian blocks in gml_newton_solve.hip.)
#include "../../include/gml.h"
#include "gml_dev.h"

namespace gml {

typedef double v4d __attribute__((ext_vector_type(4)));

#define MFMA_F64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

// ------------------------------------------------------------------------------------------
// packing
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_transpose_i8(const int8_t *__restrict__ src, int64_t rows,
                                                      int64_t cols, int64_t ld_src,
                                                      int8_t *__restrict__ dst, int64_t ld_dst) {
    __shared__ int8_t tile[64][65];
    const int64_t r0 = (int64_t)blockIdx.y * 64, c0 = (int64_t)blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        int64_t r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < rows && c < cols) ? src[r * ld_src + c] : (int8_t)0;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        int64_t c = c0 + i, r = r0 + tx;
        if (c < cols && r < rows) dst[c * ld_dst + r] = tile[tx][i];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_convert_hist(const T *__restrict__ H, int64_t K, int64_t n, int64_t ld, int col_major,
                                                      double *__restrict__ counts, int8_t *__restrict__ spins,
                                                      long long *__restrict__ bad) {
    // one thread per element, the fastest-varying source index on threadIdx: both reads and writes coalesce
    const int64_t total = K * (n + 1), stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        int64_t k, j;
        if (col_major) {
            j = e / K;
            k = e - j * K;
        } else {
            k = e / (n + 1);
            j = e - k * (n + 1);
        }
        const double v = (double)H[col_major ? k + j * ld : k * ld + j];
        if (j == 0) {
            counts[k] = v;
        } else {
            int8_t sv = 0;
            if (v == 1.0) sv = 1;
            else if (v == -1.0) sv = -1;
            else atomicMin(reinterpret_cast<unsigned long long *>(bad), (unsigned long long)k);
            spins[col_major ? (j - 1) * K + k : k * n + (j - 1)] = sv;
        }
    }
}

void launch_convert_hist(const void *H, int dtype, int64_t K, int64_t n, int64_t ld, int col_major, double *counts, int8_t *spins,
                         long long *bad, hipStream_t st) {
    const dim3 grid(8192), block(256);
    switch (dtype) {
    case GML_I8: hipLaunchKernelGGL(k_convert_hist<int8_t>, grid, block, 0, st, (const int8_t *)H, K, n, ld, col_major, counts, spins, bad); break;
    case GML_I32: hipLaunchKernelGGL(k_convert_hist<int32_t>, grid, block, 0, st, (const int32_t *)H, K, n, ld, col_major, counts, spins, bad); break;
    case GML_I64: hipLaunchKernelGGL(k_convert_hist<long long>, grid, block, 0, st, (const long long *)H, K, n, ld, col_major, counts, spins, bad); break;
    default: hipLaunchKernelGGL(k_convert_hist<double>, grid, block, 0, st, (const double *)H, K, n, ld, col_major, counts, spins, bad);
    }
}

__global__ __launch_bounds__(256) void k_check_pm1(const int8_t *__restrict__ S, int64_t total, int64_t n,
                                                   long long *__restrict__ bad) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int8_t v = S[i];
        if (v != 1 && v != -1) {
            // first offender: bad starts at -1, so compare in the unsigned order (-1 = largest)
            atomicMin(reinterpret_cast<unsigned long long *>(bad), (unsigned long long)(i / n));
        }
    }
}

void launch_check_pm1(const int8_t *S, int64_t K, int64_t n, long long *bad, hipStream_t st) {
    hipLaunchKernelGGL(k_check_pm1, dim3(4096), dim3(256), 0, st, S, K * n, n, bad);
}

void launch_transpose_i8(const int8_t *src, int64_t rows, int64_t cols, int64_t ld_src, int8_t *dst,
                         int64_t ld_dst, hipStream_t st) {
    dim3 grid((unsigned)((cols + 63) / 64), (unsigned)((rows + 63) / 64));
    hipLaunchKernelGGL(k_transpose_i8, grid, dim3(256), 0, st, src, rows, cols, ld_src, dst, ld_dst);
}

// ------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void load8d(const double *p, double (&d)[8]) {
    const double4 *q = reinterpret_cast<const double4 *>(p);
    double4 a = q[0], b = q[1];
    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
    d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
}
__device__ __forceinline__ void load8b(const int8_t *p, double (&d)[8]) {
    // 8 consecutive int8 -> 8 doubles
    uint2 u = *reinterpret_cast<const uint2 *>(p);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        d[s] = (double)(int)(int8_t)((u.x >> (8 * s)) & 0xff);
        d[4 + s] = (double)(int)(int8_t)((u.y >> (8 * s)) & 0xff);
    }
}

// ------------------------------------------------------------------------------------------
// working-set Hessian: H_r[i][j] += sum_k h_rk * Xt[F_ri][k] * Xt[F_rj][k]  for the lower
// triangular 32x32 tiles of row r's working set.  h_rk is the second-derivative weight:
//   RISE / logRISE(Z): h = w_k exp(-E) = V*s ;   RPLE: h = 4 w sg (1-sg), sg = (V*s)/(2w).
// One wave per (row, tile pair, k-split); grid = (ceil(nsplit/4), maxpairs, R).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hess_f64(const double *__restrict__ V,
                                                  const int8_t *__restrict__ Xt,
                                                  const double *__restrict__ w,
                                                  const int *__restrict__ rowcol,
                                                  const int *__restrict__ F, const int *__restrict__ mt,
                                                  const long long *__restrict__ hoff, int cap, int64_t Kp,
                                                  int64_t Kh, int64_t kchunk, int64_t kstride, int nsplit, int form,
                                                  double *__restrict__ H) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int li = lane & 15, q = lane >> 4;
    const int r = blockIdx.z;
    const int m = mt[r];
    const int pair = blockIdx.y;
    if (pair >= m * (m + 1) / 2) return;
    const int ks = blockIdx.x * 4 + wave;
    if (ks >= nsplit) return;
    int ti = (int)((sqrtf(8.0f * pair + 1.0f) - 1.0f) * 0.5f);
    while ((ti + 1) * (ti + 2) / 2 <= pair) ++ti;
    while (ti * (ti + 1) / 2 > pair) --ti;
    const int tj = pair - ti * (ti + 1) / 2;
    const int64_t kb = (int64_t)ks * kchunk;
    // Kh configurations of a compact index whose block cb of 512 stands for the samples [512 cb kstride, +512)
    const int64_t ke = (kb + kchunk < Kh) ? kb + kchunk : Kh;
    const int rc = rowcol[r];
    if (rc < 0) return;

    const int *Fr = F + (int64_t)r * cap;
    const int8_t *arow[2], *brow[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) arow[mi] = Xt + (int64_t)Fr[ti * 32 + 16 * mi + li] * Kp + 8 * q;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) brow[ni] = Xt + (int64_t)Fr[tj * 32 + 16 * ni + li] * Kp + 8 * q;
    const double *vrow = V + (int64_t)r * Kp + 8 * q;
    const int8_t *srow = Xt + (int64_t)rc * Kp + 8 * q;
    const double *wrow = w + 8 * q;

    v4d acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = (v4d){0, 0, 0, 0};

    for (int64_t tc = kb; tc < ke; tc += 32) {
        const int64_t t0 = (tc >> 9) * kstride * 512 + (tc & 511);
        double h[8], sg[8], a[2][8], b[2][8];
        load8d(vrow + t0, h);
        load8b(srow + t0, sg);
#pragma unroll
        for (int s = 0; s < 8; ++s) h[s] *= -sg[s]; // |V| = w |phi'|
        if (form == 2) {
            double wk[8];
            load8d(wrow + t0, wk);
#pragma unroll
            for (int s = 0; s < 8; ++s) h[s] = wk[s] > 0 ? 2.0 * h[s] * (1.0 - h[s] / (2.0 * wk[s])) : 0.0;
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) load8b(arow[mi] + t0, a[mi]);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) load8b(brow[ni] + t0, b[ni]);
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    acc[mi][ni] = MFMA_F64(a[mi][s] * h[s], b[ni][s], acc[mi][ni]);
    }
    double *Hr = H + hoff[r]; // row r's block: (32 m) x (32 m), pitch 32 m
    const int hp = 32 * m;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = ti * 32 + 16 * mi + q + 4 * j;
                const int jj = tj * 32 + 16 * ni + li;
                unsafeAtomicAdd(&Hr[(int64_t)i * hp + jj], acc[mi][ni][j]);
            }
}

void launch_hess_f64(const DevProblem &P, const double *V,
                     const int *rowcol, const int *F, const int *mt, const long long *hoff, int R, int cap, int form,
                     int64_t Kh, int64_t kstride, double *H, hipStream_t st) {
    const int tiles = cap / 32;
    const int maxpairs = tiles * (tiles + 1) / 2;
    int64_t nsplit = (8192 + (int64_t)R * maxpairs - 1) / ((int64_t)R * maxpairs);
    const int64_t maxsplit = Kh / 512 > 0 ? Kh / 512 : 1;
    if (nsplit > maxsplit) nsplit = maxsplit;
    if (nsplit < 1) nsplit = 1;
    int64_t kchunk = (Kh + nsplit - 1) / nsplit;
    kchunk = (kchunk + 31) / 32 * 32;
    nsplit = (Kh + kchunk - 1) / kchunk;
    dim3 grid((unsigned)((nsplit + 3) / 4), (unsigned)maxpairs, (unsigned)R);
    hipLaunchKernelGGL(k_hess_f64, grid, dim3(256), 0, st, V, P.Xt, P.w, rowcol, F, mt, hoff, cap, P.Kp, Kh, kchunk,
                       kstride, (int)nsplit, form, H);
}

} // namespace gml
