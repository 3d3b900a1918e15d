// Standard errors of learned parameters: the M-estimator ("sandwich") covariance of a node-wise solve, on the device
// (gml_stderr, include/gml.h).  gfx950 only.
//
// For local row r = node u with solution x on its support S (the FREE slots, and the PENALISED slots with x != 0):
//     C = A^-1 B A^-1 / M,   se_j = sqrt(C_jj)
//     A = sum_k w_k phi''(a_k) s_k s_k^T,   B = sum_k w_k psi_k psi_k^T - m m^T,   m = sum_k w_k psi_k,   a_k = x . s_k
// with s_k the reference's statistic vector of configuration k (`nodal_stat[k, :]`, GraphicalModelLearning.jl:162, :106-108) and
// w_k = count_k / M.  Every sum runs over ALL K configurations.  Both matrices are Grams of the same +-1 statistics under two
// per-sample weights (hA_k, hB_k), extended by the unit statistic "1" (the product of spin u with itself), whose row carries the
// sums the corrections need:
//     RISE     hA = w e,             hB = w e^2,          e = exp(-a)         g = -A[1][S],   B -= g g^T
//     RPLE     hA = 4 w sg (1 - sg), hB = 4 w (1 - sg)^2, sg = 1/(1+exp(-2a)) g = -(A[1][S] + B[1][S]) / 2 (hA + hB = 4 w (1 - sg)),   B -= g g^T
//     logRISE  as RISE;  Z = A[1][1],  gb = -A[1][S] / Z,  A = A_SS / Z - gb gb^T,
//              B = (B_SS + gb B[1][S]^T + B[1][S] gb^T + B[1][1] gb gb^T) / Z^2      (the score -(e/Z)(s + gb) expanded; m = 0)
// Three kernels:
//   k_sandwich_list    row -> the compact list of its support (slots, columns, x), its size, the first offending (row, slot)
//   k_sandwich_gram    one sweep over the samples: sign bits of the listed statistics -> LDS, a_k and the two weights in FP64,
//                      both Grams on v_mfma_f64_16x16x4_f64 from ONE set of operand fragments; K-split partial sums are stored,
//                      not added: k_sandwich_reduce adds them in ascending split order (fixed order: the same bits whatever
//                      else runs, whichever rows share the call)
//   k_sandwich_finish  corrections above, Cholesky A = L L^T, T = L^-1, A^-1 = T^T T, se_j^2 = (A^-1 B A^-1)_jj / M, scatter
#include "../../include/gml.h"
#include "gml_internal.h"
#include "gml_solver.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace gml {

typedef double v4d_s __attribute__((ext_vector_type(4)));
#define MFMA_F64_S(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

constexpr int kSeCap = 512;           // largest support (the solver's max_working ceiling)
constexpr int kSeList = kSeCap + 32;  // pitch of the per-row lists: the support, the unit statistic, padding to a 32-tile
constexpr int kSeSub = 512;           // samples per LDS stage of the Gram sweep
constexpr int kSeWords = kSeSub / 32; // sign words per statistic and stage
constexpr int kSePitch = kSeWords + 1; // LDS pitch of a statistic's words (odd: the 16 rows of a fragment hit 16 banks)
constexpr int kSeLdsMax = 128;        // supports of up to this many entries are factored with the matrix in LDS

// ------------------------------------------------------------------------------------------
// k_sandwich_list: one workgroup per row.  Walks the row's parameter slots in the reference's order (the slot -> column map of
// k_ref_to_internal / k_apply_structure), keeps the slots of the support in ascending slot order, and prepares the row of se:
// 0.0 outside the support, NaN on it (what a singular or oversized support leaves there; k_sandwich_finish overwrites it).
// *bad = the smallest (group row) * P + slot with x != 0 at an excluded slot (initialised to ~0).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sandwich_list(const double *__restrict__ X, const uint8_t *__restrict__ kind, int64_t Qp, int64_t P,
                                                       const int *__restrict__ node, int64_t cconst, const int32_t *__restrict__ cols,
                                                       int *__restrict__ Fc, int *__restrict__ Fj, double *__restrict__ Fx,
                                                       int *__restrict__ msz, unsigned long long *__restrict__ bad, double *__restrict__ se,
                                                       int64_t ld_se) {
    const int64_t r = blockIdx.x;
    const int u = node[r];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ int wcnt[4];
    int base = 0; // entries kept so far (uniform)
    for (int64_t j0 = 0; j0 < P; j0 += 256) {
        const int64_t j = j0 + tid;
        bool in = false;
        int64_t c = 0;
        double xv = 0.0;
        if (j < P) {
            c = cols ? cols[r * P + j] : (j == u ? cconst : j);
            const uint8_t kd = kind[r * Qp + c];
            xv = X[r * Qp + c];
            in = kd == GML_PARAM_FREE || (kd == GML_PARAM_PENALISED && xv != 0.0);
            if (kd == GML_PARAM_EXCLUDED && xv != 0.0) atomicMin(bad, (unsigned long long)(r * P + j));
            se[r * ld_se + j] = in ? NAN : 0.0;
        }
        const unsigned long long bal = __ballot(in);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int pos = base + before;
        for (int w = 0; w < wave; ++w) pos += wcnt[w];
        if (in && pos < kSeCap) {
            Fc[r * kSeList + pos] = (int)c;
            Fj[r * kSeList + pos] = (int)j;
            Fx[r * kSeList + pos] = xv;
        }
        base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    }
    if (tid == 0) msz[r] = base;
}

// ------------------------------------------------------------------------------------------
// k_sandwich_gram: grid (K-splits, groups of 4 tile pairs, active rows), 4 waves.  Active row a = group row arow[a] with m = msz
// entries, m1 = m + 1 statistics (the unit statistic last), mt = ceil(m1 / 32) tiles.  Per stage of 512 samples:
//   (0) the sign words of the m1 statistics -> LDS: statistic i = column Fc[i] of the internal layout = the XOR of the sign rows
//       of its key's spins (Sb is the feature-major bit image of the single-spin columns; DevProblem::keys names the spins of
//       the others), XOR the sign row of spin u; the unit statistic is the zero word;
//   (1) every thread forms a_k = sum_i x_i s_ki of two samples in FP64 (ascending i) from those words, then the two weights;
//       a configuration with w_k = 0 (zero count, padding) gets the weights 0 whatever exp gave;
//   (2) every wave accumulates its 32 x 32 tile pair of BOTH Grams: the fragments' sign bytes are read once, +-hA, +-hB are
//       the A operands, +-1 the B operand of both.
// A row with a single tile (m1 <= 32: the l1-sparse rows) gives its one tile pair to all four waves, each taking every fourth
// word of the stage; the four accumulators meet in LDS and are added as (w0 + w1) + (w2 + w3).  With m1 <= 16 only the first of
// the tile's four 16 x 16 products is issued (the other three multiply zeros: the same bits).
// The partial sums of split s go to part + poff[a] + s * 2 * blk (A, then B; blk = (32 mt)^2, pitch 32 mt; lower tile pairs only).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sandwich_gram(const unsigned *__restrict__ Sb, const int32_t *__restrict__ keys, int ko, int64_t Qf,
                                                       const double *__restrict__ w, int64_t Kp, const int *__restrict__ node,
                                                       const int *__restrict__ arow, const int *__restrict__ Fc,
                                                       const double *__restrict__ Fx, const int *__restrict__ msz,
                                                       const int *__restrict__ nsplit, const long long *__restrict__ poff, int form,
                                                       double *__restrict__ part) {
    const int a = blockIdx.z, r = arow[a];
    const int m = msz[r], m1 = m + 1, mt = (m1 + 31) >> 5, npairs = mt * (mt + 1) / 2;
    const int ns = nsplit[a], split = blockIdx.x;
    if (split >= ns || (int)blockIdx.y * 4 >= npairs) return; // (uniform over the workgroup)
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 15, q = lane >> 4;
    const int u = node[r];
    const int64_t wpr = Kp >> 5;
    const int64_t nsub = Kp / kSeSub, per = (nsub + ns - 1) / ns;
    const int64_t sub0 = (int64_t)split * per, sub1 = sub0 + per < nsub ? sub0 + per : nsub;

    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double *hA = reinterpret_cast<double *>(lds_raw);   // [512]
    double *hB = hA + kSeSub;                           // [512]
    double *xs = hB + kSeSub;                           // [32 mt]
    unsigned *bits = reinterpret_cast<unsigned *>(xs + 32 * mt); // [32 mt][kSePitch]
    for (int i = tid; i < 32 * mt; i += 256) xs[i] = i < m ? Fx[(int64_t)r * kSeList + i] : 0.0;

    const bool sliced = npairs == 1; // one tile pair: the four waves share it, wave v takes the words v, v + 4, ...
    const bool half = m1 <= 16;      // ... and only its first 16 x 16 product holds statistics (supports of up to 15 entries: the
                                     // l1 optima of the headline configuration): a quarter of the MFMAs
    const int pair = sliced ? 0 : blockIdx.y * 4 + wave;
    const bool live = pair < npairs;
    int ti = 0, tj = 0;
    if (live) {
        ti = (int)((sqrtf(8.0f * pair + 1.0f) - 1.0f) * 0.5f);
        while ((ti + 1) * (ti + 2) / 2 <= pair) ++ti;
        while (ti * (ti + 1) / 2 > pair) --ti;
        tj = pair - ti * (ti + 1) / 2;
    }
    int ia[2], ib[2]; // this lane's statistics of the A and B fragments
    bool va[2], vb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        ia[h] = ti * 32 + 16 * h + li;
        ib[h] = tj * 32 + 16 * h + li;
        va[h] = ia[h] < m1;
        vb[h] = ib[h] < m1;
    }
    v4d_s accA[2][2], accB[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) accA[mi][ni] = accB[mi][ni] = (v4d_s){0, 0, 0, 0};

    for (int64_t sub = sub0; sub < sub1; ++sub) {
        const int64_t w0 = sub * kSeWords; // first sign word of the stage
        __syncthreads();                   // (the previous stage's readers are done)
        // (0) sign words: entry (i, t) = statistic i, word t
        for (int e = tid; e < m1 * kSeWords; e += 256) {
            const int i = e / kSeWords, t = e - i * kSeWords;
            unsigned v = 0u;
            if (i < m) {
                const int64_t c = Fc[(int64_t)r * kSeList + i];
                v = Sb[(int64_t)u * wpr + w0 + t];
                if (c < Qf) {
                    for (int s = 0; s < ko; ++s) {
                        const int sp = keys[c * ko + s];
                        if (sp >= 0) v ^= Sb[(int64_t)sp * wpr + w0 + t];
                    }
                }
            }
            bits[i * kSePitch + t] = v;
        }
        __syncthreads();
        // (1) energies and weights of the samples 2 tid, 2 tid + 1 of the stage
        {
            const int t = tid >> 4, b0 = (tid & 15) * 2;
            double a0 = 0.0, a1 = 0.0;
            for (int i = 0; i < m; ++i) {
                const unsigned v = bits[i * kSePitch + t] >> b0;
                const double x = xs[i];
                a0 += (v & 1u) ? -x : x;
                a1 += (v & 2u) ? -x : x;
            }
            const int64_t k = sub * kSeSub + 2 * tid;
            const double wk0 = w[k], wk1 = w[k + 1];
            double A0, B0, A1, B1;
            if (form == GML_RPLE) {
                const double s0 = 1.0 / (1.0 + exp(-2.0 * a0)), q0 = 1.0 / (1.0 + exp(2.0 * a0));
                const double s1 = 1.0 / (1.0 + exp(-2.0 * a1)), q1 = 1.0 / (1.0 + exp(2.0 * a1));
                A0 = 4.0 * wk0 * s0 * q0;
                B0 = 4.0 * wk0 * q0 * q0;
                A1 = 4.0 * wk1 * s1 * q1;
                B1 = 4.0 * wk1 * q1 * q1;
            } else {
                const double e0 = exp(-a0), e1 = exp(-a1);
                A0 = wk0 * e0;
                B0 = A0 * e0;
                A1 = wk1 * e1;
                B1 = A1 * e1;
            }
            hA[2 * tid] = wk0 > 0.0 ? A0 : 0.0;
            hB[2 * tid] = wk0 > 0.0 ? B0 : 0.0;
            hA[2 * tid + 1] = wk1 > 0.0 ? A1 : 0.0;
            hB[2 * tid + 1] = wk1 > 0.0 ? B1 : 0.0;
        }
        __syncthreads();
        // (2) the tile pair: lane (li, q) feeds statistic li of each 16-row half, the samples 8 q .. 8 q + 7 of every word
        if (live) {
            for (int t = sliced ? wave : 0; t < kSeWords; t += sliced ? 4 : 1) {
                unsigned ba[2], bb[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    ba[h] = va[h] ? (bits[ia[h] * kSePitch + t] >> (8 * q)) & 0xffu : 0u;
                    bb[h] = vb[h] ? (bits[ib[h] * kSePitch + t] >> (8 * q)) & 0xffu : 0u;
                }
                const double *pa = hA + 32 * t + 8 * q, *pb = hB + 32 * t + 8 * q;
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const double wa = pa[s], wb = pb[s];
                    double fa[2], fb[2], fo[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const bool neg = (ba[h] >> s) & 1u;
                        fa[h] = va[h] ? (neg ? -wa : wa) : 0.0;
                        fb[h] = va[h] ? (neg ? -wb : wb) : 0.0;
                        fo[h] = vb[h] ? (((bb[h] >> s) & 1u) ? -1.0 : 1.0) : 0.0;
                    }
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                        for (int ni = 0; ni < 2; ++ni) {
                            if ((mi | ni) && half) continue; // (uniform; the other three products of such a tile are zeros)
                            accA[mi][ni] = MFMA_F64_S(fa[mi], fo[ni], accA[mi][ni]);
                            accB[mi][ni] = MFMA_F64_S(fb[mi], fo[ni], accB[mi][ni]);
                        }
                }
            }
        }
    }
    const int hp = 32 * mt;
    const int64_t blk = (int64_t)hp * hp;
    double *PA = part + poff[a] + (int64_t)split * 2 * blk, *PB = PA + blk;
    if (sliced) {
        // the four waves' sums of the one tile pair: wave v leaves its 2 x 1024 values in LDS, then entry e = (w0 + w1) + (w2 + w3)
        __syncthreads();
        double *red = reinterpret_cast<double *>(lds_raw); // [4][2][1024] (64 KB: the launch sizes the LDS for it)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = 16 * mi + q + 4 * j, jj = 16 * ni + li;
                    red[(wave * 2 + 0) * 1024 + i * 32 + jj] = accA[mi][ni][j];
                    red[(wave * 2 + 1) * 1024 + i * 32 + jj] = accB[mi][ni][j];
                }
        __syncthreads();
        for (int e = tid; e < 2048; e += 256) {
            const int g = e >> 10, o = e & 1023;
            const double v = (red[(0 * 2 + g) * 1024 + o] + red[(1 * 2 + g) * 1024 + o]) + (red[(2 * 2 + g) * 1024 + o] + red[(3 * 2 + g) * 1024 + o]);
            (g ? PB : PA)[o] = v; // (hp = 32: entry (i, jj) at i * 32 + jj)
        }
    } else if (live) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = ti * 32 + 16 * mi + q + 4 * j, jj = tj * 32 + 16 * ni + li;
                    PA[(int64_t)i * hp + jj] = accA[mi][ni][j];
                    PB[(int64_t)i * hp + jj] = accB[mi][ni][j];
                }
    }
}

// The second stage of the K-split: G[a] = part[a][0] + part[a][1] + ... in ascending split order, entry by entry (A and B
// planes at once: entry e < 2 blk of a split's record; the lower tile pairs only -- the upper tiles of the records and of GA / GB
// are never written and hold whatever the allocator left).  GA / GB: the two planes of the reduced Grams, block a at hoff[a].
__global__ __launch_bounds__(256) void k_sandwich_reduce(const double *__restrict__ part, const long long *__restrict__ poff,
                                                         const long long *__restrict__ hoff, const int *__restrict__ arow,
                                                         const int *__restrict__ msz, const int *__restrict__ nsplit, double *__restrict__ GA,
                                                         double *__restrict__ GB) {
    const int a = blockIdx.y;
    const int mt = (msz[arow[a]] + 1 + 31) >> 5;
    const int64_t blk = (int64_t)(32 * mt) * (32 * mt);
    const int ns = nsplit[a];
    const double *p = part + poff[a];
    const int hp = 32 * mt;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < 2 * blk; e += (int64_t)gridDim.x * 256) {
        const int64_t o = e < blk ? e : e - blk;
        if ((int)(o % hp) >> 5 > (int)(o / hp) >> 5) continue; // an upper tile: no split wrote it, nothing reads it
        double s = p[e];
        for (int k = 1; k < ns; ++k) s += p[(int64_t)k * 2 * blk + e];
        if (e < blk) GA[hoff[a] + e] = s;
        else GB[hoff[a] + e - blk] = s;
    }
}

// ------------------------------------------------------------------------------------------
// k_sandwich_finish: one workgroup per active row.  GA / GB: the reduced Grams (lower tile pairs valid, pitch hp = 32 mt; the unit
// statistic is row m).  WA / WB: two more planes of the same shape.
//   (1) corrections (top of the file): WA <- A, WB <- B as full symmetric m x m matrices, gout <- g;  stop != 0 ends here (the
//       test hook reads the three);
//   (2) Cholesky A = L L^T, right-looking in panels of 32 columns, on the matrix in LDS (m <= 128) or in place in WA; a pivot
//       that is not above 1e-13 x the largest diagonal entry of A ends the row with status 1;
//   (3) T = L^-1, one thread per column, into the strict upper triangle as U[j][i] = T[i][j] (rows of U contiguous), 1 / L_jj apart;
//   (4) A^-1 = T^T T -> GA (full symmetric; the raw Gram is no longer needed);
//   (5) se_j^2 = sum_l (sum_k A^-1[j][k] B[k][l]) A^-1[j][l] / M, one wave per j, scattered to the row's slots.
// ------------------------------------------------------------------------------------------
template <bool INLDS>
__global__ __launch_bounds__(256) void k_sandwich_finish(double *__restrict__ GA, double *__restrict__ GB, double *__restrict__ WA,
                                                         double *__restrict__ WB, const long long *__restrict__ hoff,
                                                         const int *__restrict__ arow, const int *__restrict__ msz,
                                                         const int *__restrict__ Fj, int form, double M, int stop,
                                                         double *__restrict__ gout, int *__restrict__ status, double *__restrict__ se,
                                                         int64_t ld_se) {
    const int a = blockIdx.x, r = arow[a];
    const int m = msz[r];
    if ((m <= kSeLdsMax) != INLDS) return;
    const int hp = 32 * ((m + 1 + 31) >> 5);
    double *RA = GA + hoff[a], *RB = GB + hoff[a], *A = WA + hoff[a], *B = WB + hoff[a];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double *g = sm, *bu = sm + kSeCap, *dinv = bu + kSeCap, *W = dinv + kSeCap; // g, B[1][S], 1 / L_jj [512 each] | W [m][m | 1] (INLDS)
    __shared__ double red[4];
    __shared__ int sing;
    // (1) corrections
    const double Zr = RA[(int64_t)m * hp + m], Buu = RB[(int64_t)m * hp + m];
    const double Z = form == GML_LOGRISE ? Zr : 1.0;
    for (int i = tid; i < m; i += 256) {
        const double au = RA[(int64_t)m * hp + i], bv = RB[(int64_t)m * hp + i];
        g[i] = form == GML_RPLE ? -0.5 * (au + bv) : -au / Z;
        bu[i] = bv;
        gout[(int64_t)r * kSeList + i] = g[i];
    }
    if (tid == 0) sing = 0;
    __syncthreads();
    for (int e = tid; e < m * m; e += 256) {
        const int i = e / m, j = e - i * m;
        if (j > i) continue;
        const double ra = RA[(int64_t)i * hp + j], rb = RB[(int64_t)i * hp + j];
        double av, bvv;
        if (form == GML_LOGRISE) {
            av = ra / Z - g[i] * g[j];
            bvv = (rb + g[i] * bu[j] + bu[i] * g[j] + Buu * g[i] * g[j]) / (Z * Z);
        } else {
            av = ra;
            bvv = rb - g[i] * g[j];
        }
        A[(int64_t)i * hp + j] = A[(int64_t)j * hp + i] = av;
        B[(int64_t)i * hp + j] = B[(int64_t)j * hp + i] = bvv;
    }
    __syncthreads();
    if (stop) return;
    // (2) Cholesky on L (lower triangle), pitch lw
    double *L = INLDS ? W : A;
    const int lw = INLDS ? (m | 1) : hp;
    double dmax = 0.0;
    for (int i = tid; i < m; i += 256) dmax = fmax(dmax, A[(int64_t)i * hp + i]);
    for (int o = 32; o > 0; o >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, o));
    if (lane == 0) red[wave] = dmax;
    __syncthreads();
    dmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    if (INLDS) {
        for (int e = tid; e < m * m; e += 256) {
            const int i = e / m, j = e - i * m;
            W[i * lw + j] = A[(int64_t)i * hp + j];
        }
        __syncthreads();
    }
    for (int c0 = 0; c0 < m; c0 += 32) {
        const int pw = m - c0 < 32 ? m - c0 : 32, r0 = c0 + pw;
        // the panel, column by column: pivot, scale, update of the panel's later columns
        for (int c = c0; c < r0; ++c) {
            const double piv = L[(int64_t)c * lw + c];
            if (!(piv > 1e-13 * dmax) || !isfinite(piv)) { // (uniform: every thread reads the same value)
                if (tid == 0) sing = 1;
                break;
            }
            const double dg = sqrt(piv);
            __syncthreads(); // (everyone has read the pivot)
            for (int i = c + tid; i < m; i += 256) L[(int64_t)i * lw + c] = i == c ? dg : L[(int64_t)i * lw + c] / dg;
            __syncthreads();
            const int ncol = r0 - c - 1; // later columns of the panel
            for (int e = tid; e < ncol * (m - c - 1); e += 256) {
                const int jc = e % ncol, j = c + 1 + jc, i = c + 1 + e / ncol;
                if (i >= j) L[(int64_t)i * lw + j] = fma(-L[(int64_t)i * lw + c], L[(int64_t)j * lw + c], L[(int64_t)i * lw + j]);
            }
            __syncthreads();
        }
        __syncthreads();
        if (sing) break;
        // trailing update by the panel: rows / columns r0 .. m - 1, lower triangle
        const int nt = m - r0;
        for (int e = tid; e < nt * nt; e += 256) {
            const int i = r0 + e / nt, j = r0 + e % nt;
            if (j > i) continue;
            double v = 0.0;
            for (int c = c0; c < r0; ++c) v = fma(L[(int64_t)i * lw + c], L[(int64_t)j * lw + c], v);
            L[(int64_t)i * lw + j] -= v;
        }
        __syncthreads();
    }
    __syncthreads();
    if (sing) { // singular support: the NaN k_sandwich_list left on its slots stay
        if (tid == 0) status[r] = GML_SE_SINGULAR;
        return;
    }
    // (3) T = L^-1: U[j][i] = T[i][j] for i > j
    for (int j = tid; j < m; j += 256) dinv[j] = 1.0 / L[(int64_t)j * lw + j];
    __syncthreads();
    for (int j = tid; j < m; j += 256) {
        const double dj = dinv[j];
        for (int i = j + 1; i < m; ++i) {
            double s = L[(int64_t)i * lw + j] * dj;
            for (int k = j + 1; k < i; ++k) s = fma(L[(int64_t)i * lw + k], L[(int64_t)j * lw + k], s);
            L[(int64_t)j * lw + i] = -s * dinv[i];
        }
    }
    __syncthreads();
    // (4) A^-1[i][j] = sum_{k >= i} T[k][i] T[k][j], j <= i  -> RA, full symmetric
    for (int e = tid; e < m * m; e += 256) {
        const int i = e / m, j = e - i * m;
        if (j > i) continue;
        double s = dinv[i] * (i == j ? dinv[i] : L[(int64_t)j * lw + i]);
        for (int k = i + 1; k < m; ++k) s = fma(L[(int64_t)i * lw + k], L[(int64_t)j * lw + k], s);
        RA[(int64_t)i * hp + j] = RA[(int64_t)j * hp + i] = s;
    }
    __syncthreads();
    // (5) the diagonal of A^-1 B A^-1
    for (int j = wave; j < m; j += 4) {
        const double *aj = RA + (int64_t)j * hp;
        double s = 0.0;
        for (int l = lane; l < m; l += 64) {
            double y = 0.0;
            for (int k = 0; k < m; ++k) y = fma(aj[k], B[(int64_t)k * hp + l], y);
            s = fma(y, aj[l], s);
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) se[(int64_t)r * ld_se + Fj[(int64_t)r * kSeList + j]] = sqrt(fmax(s, 0.0) / M);
    }
}

} // namespace gml

using namespace gml;

namespace {
struct DevBufs { // device blocks of a call, released on every path
    std::vector<void *> v;
    template <typename T> hipError_t get(T **out, size_t count) {
        void *q = nullptr;
        const hipError_t e = dev_malloc_bytes(&q, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) v.push_back(q);
        *out = static_cast<T *>(q);
        return e;
    }
    void release() {
        for (void *q : v) (void)dev_free(q);
        v.clear();
    }
    ~DevBufs() { release(); }
};
} // namespace

// Argument errors of gml_stderr, decided without any device work (include/gml.h).
static int sandwich_check_args(const gml_problem *p, int formulation, const double *x, int64_t ld, const uint8_t *structure, int64_t ld_s,
                               const double *se) {
    if (!p || !x || !se) return fail(GML_EINVAL, "NULL argument");
    if (formulation < 0 || formulation > 2) return fail(GML_EINVAL, "unknown formulation %d", formulation);
    if (ld < p->P) return fail(GML_EINVAL, "leading dimension %lld < %lld parameters per node", (long long)ld, (long long)p->P);
    if (structure && ld_s < p->P)
        return fail(GML_EINVAL, "structure: leading dimension %lld < %lld parameters per node", (long long)ld_s, (long long)p->P);
    const int64_t R = p->node1 - p->node0;
    if (structure && !gml_is_device_ptr(structure))
        for (int64_t r = 0; r < R; ++r)
            for (int64_t j = 0; j < p->P; ++j)
                if (structure[r * ld_s + j] > GML_PARAM_PENALISED)
                    return fail(GML_EINVAL, "structure: row %lld, slot %lld holds %d, not one of GML_PARAM_EXCLUDED, _FREE, _PENALISED",
                                (long long)r, (long long)j, (int)structure[r * ld_s + j]);
    if (!gml_is_device_ptr(x))
        for (int64_t r = 0; r < R; ++r)
            for (int64_t j = 0; j < p->P; ++j)
                if (!std::isfinite(x[r * ld + j]))
                    return fail(GML_EINVAL, "x: row %lld, slot %lld is not finite", (long long)r, (long long)j);
    return GML_OK;
}

// gml_stderr and the test hook behind one body.  hook != NULL: the finish kernel stops after the corrections, and the lists and
// the A, B, g blocks of the rows hook->rows are copied out (pitch hook->cap >= every listed support).
int gml_sandwich_run(gml_problem *p, int formulation, const double *x, int64_t ld, const uint8_t *structure, int64_t ld_s, double *se,
                     int32_t *status, double *times, const GmlSandwichHook *hook) {
    const int rc0 = sandwich_check_args(p, formulation, x, ld, structure, ld_s, se);
    if (rc0) return rc0;
    if (formulation != GML_RISE && p->order != 2)
        return fail(GML_EUNSUPPORTED, "multi-body statistics are defined for RISE only (multiRISE, :83-152)");
    HIPCHK(hipSetDevice(p->device));
    hipStream_t st = p->st;
    const DevProblem &d = p->d;
    const int64_t R = p->node1 - p->node0, P = p->P, Qp = d.Qp;
    const bool x_dev = gml_is_device_ptr(x), se_dev = gml_is_device_ptr(se), s_dev = structure && gml_is_device_ptr(structure);
    double tph[3] = {0, 0, 0};
    std::vector<int32_t> hstatus((size_t)R, GML_SE_OK);

    // rows in groups whose dense per-row arrays (X, kind: 9 bytes per column) stay within 1 GB
    const int64_t gmax = std::max<int64_t>(1, std::min<int64_t>(4096, ((int64_t)1 << 30) / (9 * Qp)));
    for (int64_t g0 = 0; g0 < R; g0 += gmax) {
        const int64_t Rg = std::min(gmax, R - g0);
        DevBufs bufs;
        double t0 = gml_now_s();
        // ---- lists ----------------------------------------------------------------------
        int *dNode = nullptr, *dFc = nullptr, *dFj = nullptr, *dMsz = nullptr, *dFlag = nullptr, *dCnt = nullptr;
        double *dX = nullptr, *dFx = nullptr, *dSe = nullptr, *dGout = nullptr;
        uint8_t *dKind = nullptr;
        int32_t *dCols = nullptr;
        unsigned long long *dBad = nullptr;
        HIPCHK(bufs.get(&dNode, (size_t)Rg));
        HIPCHK(bufs.get(&dX, (size_t)Rg * Qp));
        HIPCHK(bufs.get(&dKind, (size_t)Rg * Qp));
        HIPCHK(bufs.get(&dFc, (size_t)Rg * kSeList));
        HIPCHK(bufs.get(&dFj, (size_t)Rg * kSeList));
        HIPCHK(bufs.get(&dFx, (size_t)Rg * kSeList));
        HIPCHK(bufs.get(&dGout, (size_t)Rg * kSeList));
        HIPCHK(bufs.get(&dMsz, (size_t)Rg));
        HIPCHK(bufs.get(&dFlag, 4));
        HIPCHK(bufs.get(&dCnt, (size_t)Rg));
        HIPCHK(bufs.get(&dBad, 2));
        std::vector<int> hnode((size_t)Rg);
        for (int64_t r = 0; r < Rg; ++r) hnode[r] = (int)(p->node0 + g0 + r);
        HIPCHK(hipMemcpyAsync(dNode, hnode.data(), sizeof(int) * Rg, hipMemcpyHostToDevice, st));
        std::vector<int32_t> hcols;
        if (p->order != 2) { // multi-body key order (:94-104): the column of every parameter slot
            hcols.resize((size_t)Rg * P);
            gml_parallel_for(Rg, [&](int64_t r) {
                NodeLayout L;
                gml_build_layout(p, p->node0 + g0 + r, L);
                std::memcpy(hcols.data() + (size_t)r * P, L.cols.data(), sizeof(int32_t) * P);
            });
            HIPCHK(bufs.get(&dCols, (size_t)Rg * P));
            HIPCHK(hipMemcpyAsync(dCols, hcols.data(), sizeof(int32_t) * Rg * P, hipMemcpyHostToDevice, st));
        }
        const double *xsrc = x + g0 * ld;
        int64_t ldx = ld;
        if (!x_dev) {
            double *tmp = nullptr;
            HIPCHK(bufs.get(&tmp, (size_t)Rg * P));
            HIPCHK(hipMemcpy2DAsync(tmp, sizeof(double) * P, xsrc, sizeof(double) * ld, sizeof(double) * P, (size_t)Rg, hipMemcpyHostToDevice, st));
            xsrc = tmp;
            ldx = P;
        }
        double *sedst = se + g0 * ld;
        int64_t ldse = ld;
        if (!se_dev) {
            HIPCHK(bufs.get(&dSe, (size_t)Rg * P));
            sedst = dSe;
            ldse = P;
        }
        HIPCHK(hipMemsetAsync(dX, 0, sizeof(double) * Rg * Qp, st));
        HIPCHK(hipMemsetAsync(dFlag, 0, sizeof(int) * 4, st));
        HIPCHK(hipMemsetAsync(dBad, 0xFF, sizeof(unsigned long long) * 2, st));
        HIPCHK(hipMemsetAsync(dCnt, 0, sizeof(int) * Rg, st));
        launch_kind(d, p->order, dNode, (int)Rg, dKind, st);
        if (structure) {
            const uint8_t *ssrc = structure + g0 * ld_s;
            int64_t lds = ld_s;
            if (!s_dev) {
                uint8_t *tmp = nullptr;
                HIPCHK(bufs.get(&tmp, (size_t)Rg * P));
                HIPCHK(hipMemcpy2DAsync(tmp, (size_t)P, ssrc, (size_t)ld_s, (size_t)P, (size_t)Rg, hipMemcpyHostToDevice, st));
                ssrc = tmp;
                lds = P;
            }
            launch_apply_structure(ssrc, lds, Rg, P, Qp, dNode, d.cconst, dCols, dKind, dCnt, dBad, st);
        }
        launch_ref_to_internal(xsrc, ldx, Rg, P, Qp, dNode, d.cconst, dCols, dX, dFlag, st);
        hipLaunchKernelGGL(k_sandwich_list, dim3((unsigned)Rg), dim3(256), 0, st, dX, dKind, Qp, P, dNode, d.cconst, dCols, dFc, dFj, dFx, dMsz,
                           dBad + 1, sedst, ldse);
        HIPCHK(hipGetLastError());
        std::vector<int> hmsz((size_t)Rg);
        int hflag[4] = {0, 0, 0, 0};
        unsigned long long hbad[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(hmsz.data(), dMsz, sizeof(int) * Rg, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hflag, dFlag, sizeof hflag, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hbad, dBad, sizeof hbad, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (hbad[0] != ~0ull)
            return fail(GML_EINVAL, "structure: row %lld, slot %lld holds a value outside {0, 1, 2}", (long long)(g0 + hbad[0] / (unsigned long long)P),
                        (long long)(hbad[0] % (unsigned long long)P));
        if (hflag[0]) return fail(GML_EINVAL, "x contains a non-finite value");
        if (hbad[1] != ~0ull)
            return fail(GML_EINVAL, "x is non-zero at an excluded parameter: row %lld, slot %lld", (long long)(g0 + hbad[1] / (unsigned long long)P),
                        (long long)(hbad[1] % (unsigned long long)P));
        tph[0] += gml_now_s() - t0;

        // ---- Grams and finish, in batches of active rows whose workspaces fit ------------------------
        std::vector<int> act;
        for (int64_t r = 0; r < Rg; ++r) {
            if (hmsz[r] > kSeCap) hstatus[g0 + r] = GML_SE_TOO_LARGE;
            else if (hmsz[r] > 0) act.push_back((int)r);
        }
        size_t fb = 0, tb = 0;
        HIPCHK(dev_mem_info(&fb, &tb));
        const int64_t budget = std::max<int64_t>((int64_t)64 << 20, std::min<int64_t>((int64_t)2 << 30, (int64_t)(fb / 2))) / 8; // doubles
        const int64_t nsub = d.Kp / kSeSub;
        int *dStatus = nullptr;
        HIPCHK(bufs.get(&dStatus, (size_t)Rg));
        HIPCHK(hipMemsetAsync(dStatus, 0, sizeof(int) * Rg, st));
        size_t b0 = 0;
        while (b0 < act.size()) {
            t0 = gml_now_s();
            // The K-split of a row depends on the row alone (its tile count and K): 128 workgroups per row where K allows it.  So
            // the order of every sum, hence every bit of the result, is the same whichever rows share the call, the group or the batch.
            std::vector<int> arow, nsp;
            std::vector<long long> hoff, poff;
            int64_t htot = 0, ptot = 0;
            int maxpg = 0, maxns = 0, maxmt = 0;
            bool any_lds = false, any_glb = false;
            size_t b1 = b0;
            for (; b1 < act.size(); ++b1) {
                const int m = hmsz[act[b1]], mt = (m + 1 + 31) / 32, pg = (mt * (mt + 1) / 2 + 3) / 4;
                const int64_t blk = (int64_t)(32 * mt) * (32 * mt);
                const int ns = (int)std::max<int64_t>(1, std::min<int64_t>(nsub, (128 + pg - 1) / pg));
                if (b1 > b0 && 4 * (htot + blk) + ptot + 2 * blk * ns > budget) break;
                arow.push_back(act[b1]);
                nsp.push_back(ns);
                hoff.push_back(htot);
                poff.push_back(ptot);
                htot += blk;
                ptot += 2 * blk * ns;
                maxpg = std::max(maxpg, pg);
                maxns = std::max(maxns, ns);
                maxmt = std::max(maxmt, mt);
                (m <= kSeLdsMax ? any_lds : any_glb) = true;
            }
            const int na = (int)arow.size();
            DevBufs wb;
            int *dArow = nullptr, *dNs = nullptr;
            long long *dHoff = nullptr, *dPoff = nullptr;
            double *dPlanes = nullptr, *dPart = nullptr;
            HIPCHK(wb.get(&dArow, (size_t)na));
            HIPCHK(wb.get(&dNs, (size_t)na));
            HIPCHK(wb.get(&dHoff, (size_t)na));
            HIPCHK(wb.get(&dPoff, (size_t)na));
            HIPCHK(wb.get(&dPlanes, (size_t)(4 * htot)));
            HIPCHK(wb.get(&dPart, (size_t)ptot));
            HIPCHK(hipMemcpyAsync(dArow, arow.data(), sizeof(int) * na, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(dNs, nsp.data(), sizeof(int) * na, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(dHoff, hoff.data(), sizeof(long long) * na, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(dPoff, poff.data(), sizeof(long long) * na, hipMemcpyHostToDevice, st));
            double *GA = dPlanes, *GB = dPlanes + htot, *WA = dPlanes + 2 * htot, *WB = dPlanes + 3 * htot;
            // LDS of the sweep: two weight arrays, x, the sign words; at least the 64 KB the single-tile rows' final sum takes
            size_t lds = sizeof(double) * (2 * kSeSub + 32 * maxmt) + sizeof(unsigned) * (size_t)(32 * maxmt) * kSePitch;
            lds = std::max<size_t>(lds, sizeof(double) * 8 * 1024);
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sandwich_gram), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_sandwich_gram, dim3((unsigned)maxns, (unsigned)maxpg, (unsigned)na), dim3(256), lds, st, d.Sb, d.keys, d.ko, d.Qf,
                               d.w, d.Kp, dNode, dArow, dFc, dFx, dMsz, dNs, dPoff, formulation, dPart);
            hipLaunchKernelGGL(k_sandwich_reduce, dim3((unsigned)std::min<int64_t>(64, (2 * (int64_t)(32 * maxmt) * (32 * maxmt) + 255) / 256),
                                                       (unsigned)na),
                               dim3(256), 0, st, dPart, dPoff, dHoff, dArow, dMsz, dNs, GA, GB);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
            tph[1] += gml_now_s() - t0;
            t0 = gml_now_s();
            const int stop = hook ? 1 : 0;
            if (any_lds) {
                const size_t l2 = sizeof(double) * (3 * kSeCap + (size_t)kSeLdsMax * (kSeLdsMax | 1));
                HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sandwich_finish<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)l2));
                hipLaunchKernelGGL(k_sandwich_finish<true>, dim3((unsigned)na), dim3(256), l2, st, GA, GB, WA, WB, dHoff, dArow, dMsz, dFj, formulation,
                                   p->M, stop, dGout, dStatus, sedst, ldse);
            }
            if (any_glb)
                hipLaunchKernelGGL(k_sandwich_finish<false>, dim3((unsigned)na), dim3(256), sizeof(double) * 3 * kSeCap, st, GA, GB, WA, WB, dHoff, dArow,
                                   dMsz, dFj, formulation, p->M, stop, dGout, dStatus, sedst, ldse);
            HIPCHK(hipGetLastError());
            if (hook) {
                for (int64_t h = 0; h < hook->nrows; ++h) {
                    const int64_t lr = hook->rows[h] - g0;
                    const auto it = std::find(arow.begin(), arow.end(), (int)lr);
                    if (lr < 0 || lr >= Rg || it == arow.end()) continue;
                    const size_t ai = (size_t)(it - arow.begin());
                    const int m = hmsz[lr], hp = 32 * ((m + 1 + 31) / 32), cap = hook->cap;
                    if (m > cap) return fail(GML_EINVAL, "hook: row %lld has %d entries, cap is %d", (long long)hook->rows[h], m, cap);
                    HIPCHK(hipMemcpy2DAsync(hook->A + h * cap * cap, sizeof(double) * cap, WA + hoff[ai], sizeof(double) * hp, sizeof(double) * m, (size_t)m,
                                            hipMemcpyDeviceToHost, st));
                    HIPCHK(hipMemcpy2DAsync(hook->B + h * cap * cap, sizeof(double) * cap, WB + hoff[ai], sizeof(double) * hp, sizeof(double) * m, (size_t)m,
                                            hipMemcpyDeviceToHost, st));
                    HIPCHK(hipMemcpyAsync(hook->g + h * cap, dGout + lr * kSeList, sizeof(double) * m, hipMemcpyDeviceToHost, st));
                    HIPCHK(hipMemcpyAsync(hook->lists + h * cap, dFj + lr * kSeList, sizeof(int) * m, hipMemcpyDeviceToHost, st));
                }
            }
            HIPCHK(hipStreamSynchronize(st));
            tph[2] += gml_now_s() - t0;
            b0 = b1;
        }
        if (hook)
            for (int64_t h = 0; h < hook->nrows; ++h) {
                const int64_t lr = hook->rows[h] - g0;
                if (lr >= 0 && lr < Rg) hook->msz[h] = hmsz[lr];
            }
        t0 = gml_now_s();
        std::vector<int> hst((size_t)Rg);
        HIPCHK(hipMemcpyAsync(hst.data(), dStatus, sizeof(int) * Rg, hipMemcpyDeviceToHost, st));
        if (!se_dev)
            HIPCHK(hipMemcpy2DAsync(se + g0 * ld, sizeof(double) * ld, dSe, sizeof(double) * P, sizeof(double) * P, (size_t)Rg, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int64_t r = 0; r < Rg; ++r)
            if (hst[r]) hstatus[g0 + r] = hst[r];
        tph[2] += gml_now_s() - t0;
    }
    if (status) std::copy(hstatus.begin(), hstatus.end(), status);
    if (times) std::copy(tph, tph + 3, times);
    return GML_OK;
}

extern "C" int gml_stderr(gml_problem *p, int formulation, const double *x, int64_t ld, const uint8_t *structure, int64_t ld_s, double *se,
                          int32_t *status, double *times) {
    return gml_sandwich_run(p, formulation, x, ld, structure, ld_s, se, status, times, nullptr);
}
