// The two GEMM-shaped kernels of the FP64 device path (precision "f64": the reference's own arithmetic, instruction for
// instruction, on v_mfma_f64_16x16x4_f64):
//   energies  A[r][k] = sum_c Theta[r][c] x[k][c]   + the pointwise epilogue      (GraphicalModelLearning.jl:162, :170, :196)
//   gradient  G[r][c] = sum_k V[r][k] x[k][c]                                      (:205-207)
// Round-4 form.  The +-1 operand comes from the BIT images the int8 kernels use (Xb sample-major, Xtb feature-major: one dword per
// lane and 32-deep block, expanded to +-1.0 by two integer instructions per element) -- the two 1-GB byte images of rounds 1-3
// are gone from these kernels.  The waves of a workgroup share the FP64 operand and split the +-1 side: 4 waves = 32 rows x 512
// samples (forward) / 8 waves = 32 rows x 1024 columns (backward), wave tile 32 x 128 = 16 MFMA tiles, 128 accumulator registers.  With
// every column of a row group in ONE workgroup the backward kernel reads V from HBM once per pass (8.2 GB at the headline size;
// the round-1 kernel re-read it once per 256-column block: 61 GB fetched per launch), and a 32-deep block carries 128 MFMAs of
// 64 cycles each per wave against 16 + 8 loads: the kernels need no LDS staging, and a barrier only now and then.
#include "../../include/gml.h"
#include "gml_dev.h"
#include <algorithm>

namespace gml {

typedef double v4d __attribute__((ext_vector_type(4)));
#define MFMA_F64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

namespace {

__device__ __forceinline__ void ld8(const double *p, double (&d)[8]) {
    const double4 *q = reinterpret_cast<const double4 *>(p);
    const double4 a = q[0], b = q[1];
    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
    d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
}
// bit `sh` of w set (spin -1) -> -1.0, else +1.0
__device__ __forceinline__ double pm1(unsigned w, int sh) { return __hiloint2double((int)(((w >> sh) << 31) | 0x3FF00000u), 0); }

constexpr int NT = 8; // 16-wide MFMA tiles of the +-1 side per wave (wave tile 32 x 128)

} // namespace

// ------------------------------------------------------------------------------------------
// forward.  grid = (Kp / 512, listed row groups); workgroup = 4 waves x 128 samples of one 32-row group.
// Lane (li = lane & 15, q = lane >> 4) feeds MFMA step s of a 32-column block with the element at contraction index 8 q + s
// of both operands: Theta[row li][.. + 8 q + s] (8 consecutive doubles) and, from the lane's dword (sample li, step kt,
// half h = q >> 1) of the Xb image, the bit of column 64 kt + 32 g + 8 q + s: bit 4 g + 2 (q & 1) + (s >> 2) + 8 (s & 3)
// (gml_bits.h: xb_col).  The constant statistic (column cconst, x = 1) is added in the epilogue.
// ------------------------------------------------------------------------------------------
// Forward workgroups are 4 waves (32 rows x 512 samples), two per CU: the epilogue of one -- 64 exp per lane and the V stores, with
// no matrix work -- then runs beside the other's GEMM loop (8-wave workgroups, one per CU: 36.7 ms; 4-wave: 32.7 ms).
#ifndef F64_FWD_WAVES
#define F64_FWD_WAVES 4
#endif
// Kp is a multiple of 1024: with 128 F64_FWD_WAVES samples per workgroup dividing it, the grid covers Kp exactly, every wave of a
// workgroup has samples, and all of them reach the barrier before the workgroup's part of f is stored
static_assert(F64_FWD_WAVES == 1 || F64_FWD_WAVES == 2 || F64_FWD_WAVES == 4 || F64_FWD_WAVES == 8, "128 * F64_FWD_WAVES must divide 1024");
__global__ __launch_bounds__(64 * F64_FWD_WAVES, 8 / F64_FWD_WAVES) void k_fwd_f64(const double *__restrict__ Theta, const unsigned *__restrict__ Xb,
                                                    const unsigned *__restrict__ Sb, const int *__restrict__ rowcol,
                                                    const int *__restrict__ groups, const double *__restrict__ w, int64_t Qp,
                                                    int64_t cconst, int64_t Kp, int nk, int form, double *__restrict__ V,
                                                    double *__restrict__ fpartial) {
    __shared__ double fred[F64_FWD_WAVES][32]; // the waves' parts of f of the group's 32 rows
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int li = lane & 15, q = lane >> 4;
    const int grp = groups[blockIdx.y]; // 32-row group of this workgroup (-1: padding of the list)
    if (grp < 0) return;
    const int r0 = grp * 32;
    const int64_t k0 = (int64_t)blockIdx.x * (128 * F64_FWD_WAVES) + wave * 128; // this wave's 128 samples: one 128-sample piece of Xb
    v4d acc[2][NT];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = (v4d){0, 0, 0, 0};

    const double *arow[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) arow[mi] = Theta + (int64_t)(r0 + 16 * mi + li) * Qp + 8 * q;
    // dword (sample k0 + 16 ni + li, step kt, half q >> 1): piece (k0 >> 7), 256 dwords per step
    const unsigned *bp = Xb + ((k0 >> 7) * nk * 128 + li) * 2 + (q >> 1);
    const int qs = 2 * (q & 1);

    for (int kt = 0; kt < nk; ++kt) {
        unsigned bw[NT];
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) bw[ni] = bp[(int64_t)kt * 256 + ni * 32] >> qs;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            double a[2][8];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) ld8(arow[mi] + 64 * kt + 32 * g, a[mi]);
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                double bd[NT];
#pragma unroll
                for (int ni = 0; ni < NT; ++ni) bd[ni] = pm1(bw[ni], 4 * g + (s >> 2) + 8 * (s & 3));
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = MFMA_F64(a[mi][s], bd[ni], acc[mi][ni]);
            }
        }
    }

    // epilogue: lane holds C[r = r0 + 16 mi + q + 4 j][k = k0 + 16 ni + li]
    const int64_t wpr = Kp >> 5;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = r0 + 16 * mi + q + 4 * j;
            const int rc = rowcol[r];
            const double tc = rc >= 0 ? Theta[(int64_t)r * Qp + cconst] : 0.0;
            double fpart = 0.0;
#pragma unroll
            for (int ni = 0; ni < NT; ++ni) {
                const int64_t k = k0 + 16 * ni + li;
                if (rc >= 0) {
                    const double wk = w[k];
                    const double s = ((Sb[(int64_t)rc * wpr + (k >> 5)] >> (k & 31)) & 1u) ? -1.0 : 1.0; // the node's own spin
                    const double E = s * (acc[mi][ni][j] + tc);
                    double val;
                    if (form >= 4) {
                        // Hessian-vector forward (forms 4..6; Theta holds the direction p): U_k = h_k (acc + tc), acc + tc = sum_j p_j x_kj
                        // over the raw columns -- the backward GEMM contracts U with the same raw columns, which gives H p since s^2 = 1.
                        // The curvature weight h_k comes from the V the objective pass at theta left in this row: RISE / logRISE Z:
                        // V = -w e^-E s, h = w e^-E = -V s; RPLE: V = -2 w sigma(-2E) s, h = 4 w sigma(-2E) sigma(2E).
                        const double vold = V[(int64_t)r * Kp + k];
                        double h = -vold * s;
                        if (form == 6) {
                            const double sg = wk > 0.0 ? h / (2.0 * wk) : 0.0; // sigma(-2E)
                            h = 2.0 * h * (1.0 - sg);
                        }
                        val = h * (E * s); // (E s = acc + tc)
                        V[(int64_t)r * Kp + k] = val;
                        continue;
                    }
                    if (form == 2) { // RPLE (:317)
                        const double t = -2.0 * E;
                        const double sp = t > 0 ? t + log1p(exp(-t)) : log1p(exp(t));
                        const double sg = 1.0 / (1.0 + exp(2.0 * E));
                        fpart += wk * sp;
                        val = -2.0 * wk * sg * s; // d/dE of w log(1+exp(-2E)), times s
                    } else { // RISE (:196) / logRISE Z (:279)
                        // (w = 0 -- the padding samples, whose energy is the plain sum of the row -- contributes 0 whatever exp(-E) is:
                        // beyond E = -709.8 the product would be 0 * inf)
                        const double e = wk != 0.0 ? wk * exp(-E) : 0.0;
                        fpart += e;
                        val = -e * s; // partial_obj (:204) times the node's sign
                    }
                    V[(int64_t)r * Kp + k] = val; // (inactive rows keep their previous V)
                }
            }
            // reduce over the 16 lanes sharing this row (li = 0..15)
            fpart += __shfl_xor(fpart, 1);
            fpart += __shfl_xor(fpart, 2);
            fpart += __shfl_xor(fpart, 4);
            fpart += __shfl_xor(fpart, 8);
            if (li == 0) fred[wave][16 * mi + q + 4 * j] = fpart; // (0 for a padding row)
        }
    }
    if (form >= 4) return; // (a Hessian-vector forward has no objective)
    // the workgroup's part of f, its waves added in their own order, goes to its own place: k_fsum_reduce adds the workgroups' parts in
    // a fixed order too, so f is the same bits on every call (FP64 atomics on fsum added them in the order the waves happened to finish)
    __syncthreads();
    if (threadIdx.x < 32) {
        double s = fred[0][threadIdx.x];
#pragma unroll
        for (int v = 1; v < F64_FWD_WAVES; ++v) s += fred[v][threadIdx.x];
        fpartial[((int64_t)blockIdx.y * 32 + threadIdx.x) * gridDim.x + blockIdx.x] = s;
    }
}

// fsum[r] += the nx workgroup parts of row r, one wave per row: lane l adds the parts l, l + 64, ... in ascending order, the lanes meet in
// a fixed butterfly
__global__ __launch_bounds__(256) void k_fsum_reduce(const double *__restrict__ fpartial, const int *__restrict__ rowcol,
                                                     const int *__restrict__ groups, int nx, double *__restrict__ fsum) {
    const int grp = groups[blockIdx.y];
    if (grp < 0) return;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int r = grp * 32 + t;
    if (rowcol[r] < 0) return;
    const double *src = fpartial + ((int64_t)blockIdx.y * 32 + t) * nx;
    double s = 0.0;
    for (int x = lane; x < nx; x += 64) s += src[x];
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) fsum[r] += s;
}

void launch_fwd_f64(const DevProblem &P, const double *Theta, const int *rowcol, const int *groups, int ngroups4, int form, double *V,
                    double *fsum, double *ws, hipStream_t st) {
    dim3 grid((unsigned)((P.Kp + 128 * F64_FWD_WAVES - 1) / (128 * F64_FWD_WAVES)), (unsigned)ngroups4);
    hipLaunchKernelGGL(k_fwd_f64, grid, dim3(64 * F64_FWD_WAVES), 0, st, Theta, P.Xb, P.Sb, rowcol, groups, P.w, P.Qp, P.cconst, P.Kp, (int)(P.Qfp / 64), form,
                       V, ws);
    if (form < 4) hipLaunchKernelGGL(k_fsum_reduce, dim3(8, (unsigned)ngroups4), dim3(256), 0, st, ws, rowcol, groups, (int)grid.x, fsum);
}

// ------------------------------------------------------------------------------------------
// backward.  grid = (ceil(Qfp / 1024), row groups, split-K chunks); workgroup = 8 waves x 128 columns of one 32-row group over
// one chunk of the samples; every chunk stores its partial sums in a place of its own (Gpart [chunk][listed row][Qp]) and
// k_bwd_f64_reduce adds them in ascending chunk order: G is the same bits on every call (FP64 atomics added the chunks in the order
// they happened to finish).  A single chunk adds to G directly.  Lane (li, q) feeds step s of a 32-sample block with
// V[row li][k + 8 q + s] and, from the lane's dword (column li, block) of the Xtb image, the bit of sample k + 8 q + s:
// bit q + 4 (s >> 2) + 8 (s & 3) (gml_bits.h: xtb_from_natural).  The constant statistic (x = 1 on every real sample; V is 0 on
// the padding ones) is the plain row sum of V: wave 0 of the first column block adds it up on the side.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 1) void k_bwd_f64(const double *__restrict__ V, const unsigned *__restrict__ Xtb,
                                                    const int *__restrict__ groups, int64_t Qp, int64_t Qf, int64_t Qc /* columns of the image */,
                                                    int64_t cconst, int64_t Kp, int64_t kchunk, double *__restrict__ G,
                                                    double *__restrict__ Gpart) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int li = lane & 15, q = lane >> 4;
    const int r0 = groups[blockIdx.y] * 32;
    const int64_t c0 = (int64_t)blockIdx.x * 1024 + wave * 128;
    if (c0 >= Qf) return;
    const int64_t kb = (int64_t)blockIdx.z * kchunk;
    const int64_t ke = (kb + kchunk < Kp) ? kb + kchunk : Kp;
    const int64_t nkk = Kp >> 6;
    const bool sums = blockIdx.x == 0 && wave == 0;

    v4d acc[2][NT];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = (v4d){0, 0, 0, 0};
    double rs[2] = {0.0, 0.0};

    const double *arow[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) arow[mi] = V + (int64_t)(r0 + 16 * mi + li) * Kp + 8 * q;
    // dword (column c, 64-sample step kt, half h) of the image: pieces [Qc / 128][Kp / 64][128 columns][2]
    const unsigned *bp[NT];
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
        int64_t c = c0 + 16 * ni + li;
        if (c >= Qc) c = Qc - 1; // (beyond the image: any column, the result is not stored)
        bp[ni] = Xtb + ((c >> 7) * nkk * 128 + (c & 127)) * 2;
    }

    for (int64_t k = kb; k < ke; k += 32) {
        // the 8 waves read the same V: kept within 32 blocks of each other (one barrier per 4096 MFMAs of a wave), the seven
        // followers hit in L2 (-1.7 % on the kernel; every 8 blocks: +0.5 %)
        if ((((k - kb) >> 5) & 31) == 31) __builtin_amdgcn_s_barrier();
        const int64_t boff = (k >> 6) * 256 + ((k >> 5) & 1);
        unsigned bw[NT];
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) bw[ni] = bp[ni][boff] >> q;
        double a[2][8];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) ld8(arow[mi] + k, a[mi]);
        if (sums) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int s = 0; s < 8; ++s) rs[mi] += a[mi][s];
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            double bd[NT];
#pragma unroll
            for (int ni = 0; ni < NT; ++ni) bd[ni] = pm1(bw[ni], 4 * (s >> 2) + 8 * (s & 3));
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = MFMA_F64(a[mi][s], bd[ni], acc[mi][ni]);
        }
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
            const int64_t c = c0 + 16 * ni + li;
            if (c < Qf) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int rr = 16 * mi + q + 4 * j;
                    if (gridDim.z == 1) G[(int64_t)(r0 + rr) * Qp + c] += acc[mi][ni][j]; // (this lane alone owns the entry)
                    else Gpart[(((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * 32 + rr) * Qp + c] = acc[mi][ni][j];
                }
            }
        }
    if (sums) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            double v = rs[mi];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (q == 0) {
                const int rr = 16 * mi + li;
                if (gridDim.z == 1) G[(int64_t)(r0 + rr) * Qp + cconst] += v;
                else Gpart[(((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * 32 + rr) * Qp + cconst] = v;
            }
        }
    }
}

// G[r][c] += the nsplit chunk parts of the entry in ascending chunk order; grid = (listed rows, ceil(Qp / 256))
__global__ __launch_bounds__(256) void k_bwd_f64_reduce(const double *__restrict__ Gpart, const int *__restrict__ groups, int64_t Qp, int64_t Qf,
                                                        int64_t cconst, int nsplit, double *__restrict__ G) {
    const int64_t c = (int64_t)blockIdx.y * 256 + threadIdx.x;
    if (c >= Qp || (c >= Qf && c != cconst)) return;
    const int64_t rr = blockIdx.x, nrows = gridDim.x;
    double *dst = G + ((int64_t)groups[rr >> 5] * 32 + (rr & 31)) * Qp + c;
    double s = *dst;
    for (int z = 0; z < nsplit; ++z) s += Gpart[((int64_t)z * nrows + rr) * Qp + c];
    *dst = s;
}

// split of the samples over the workgroups of a backward launch with `ngroups` row groups
static void bwd_f64_split(const DevProblem &P, int ngroups, unsigned *gx_out, int64_t *nsplit_out, int64_t *kchunk_out) {
    const unsigned gx = (unsigned)((P.Qf + 1023) / 1024 > 0 ? (P.Qf + 1023) / 1024 : 1), gy = (unsigned)(ngroups > 0 ? ngroups : 1);
    // one 8-wave workgroup per CU at a time: about two rounds of workgroups over the 256 CUs, in whole 1024-sample chunks
    int64_t nsplit = (512 + (int64_t)gx * gy - 1) / ((int64_t)gx * gy);
    const int64_t maxsplit = P.Kp / 2048 > 0 ? P.Kp / 2048 : 1;
    if (nsplit > maxsplit) nsplit = maxsplit;
    if (nsplit < 1) nsplit = 1;
    int64_t kchunk = (P.Kp + nsplit - 1) / nsplit;
    kchunk = (kchunk + 63) / 64 * 64;
    nsplit = (P.Kp + kchunk - 1) / kchunk;
    *gx_out = gx;
    *nsplit_out = nsplit;
    *kchunk_out = kchunk;
}

// bytes of the workspace `ws` of launch_fwd_f64 / launch_bwd_f64 for launches of up to `rows` rows (a multiple of 32): the larger of the
// forward's parts of f ([row][Kp / 512], the group list padded to 4) and the backward's chunk parts of G for any number of listed groups
size_t f64_reduce_ws_bytes(const DevProblem &P, int64_t rows) {
    const int64_t ng_max = rows / 32 > 0 ? rows / 32 : 1;
    size_t bytes = sizeof(double) * (size_t)((ng_max + 3) / 4 * 4 * 32) * (size_t)(P.Kp / (128 * F64_FWD_WAVES));
    for (int64_t ng = 1; ng <= ng_max; ++ng) {
        unsigned gx;
        int64_t nsplit, kchunk;
        bwd_f64_split(P, (int)ng, &gx, &nsplit, &kchunk);
        if (nsplit > 1) bytes = std::max(bytes, sizeof(double) * (size_t)nsplit * (size_t)ng * 32 * (size_t)P.Qp);
    }
    return bytes;
}

void launch_bwd_f64(const DevProblem &P, const double *V, const int *groups, int ngroups, double *G, double *ws, hipStream_t st) {
    unsigned gx;
    int64_t nsplit, kchunk;
    bwd_f64_split(P, ngroups, &gx, &nsplit, &kchunk);
    dim3 grid(gx, (unsigned)ngroups, (unsigned)nsplit);
    const int64_t Qc = (P.Qfp + 255) / 256 * 256;
    hipLaunchKernelGGL(k_bwd_f64, grid, dim3(512), 0, st, V, P.Xtb, groups, P.Qp, P.Qf, Qc, P.cconst, P.Kp, kchunk, G, ws);
    if (nsplit > 1)
        hipLaunchKernelGGL(k_bwd_f64_reduce, dim3((unsigned)ngroups * 32, (unsigned)((P.Qp + 255) / 256)), dim3(256), 0, st, ws, groups, P.Qp, P.Qf,
                           P.cconst, (int)nsplit, G);
}

} // namespace gml
