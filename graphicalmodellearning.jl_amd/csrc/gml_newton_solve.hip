// Dense FP64 solves of the direction phase of learn(), for every precision of the passes.  gfx950 only.
//
// launch_newton_solve -- the batched Newton solve on the ragged Hessian blocks (contract: gml_dev.h).  For every row r
//   A d = -pg,   A = s1[r] * H_r  -  s2 * gF gF^T        (s2 = 1 for logRISE: Hess log Z = Hess Z / Z - g g^T)
// by Cholesky with a ridge restart (0 -> 1e-12 max|A_ii| -> x 100, ten attempts; all fail: d = 0).  H_r is row r's block at
// H + hoff[r], pitch 32 mt[r], lower 32 x 32 tiles valid, msz[r] entries; gF / pgF / dout are [R][cap]; Sdiag[r] = A[m-1][m-1] (the
// constant column, the Hessian's diagonal scale).  Entries may be fixed at a given step (fix / dfix, tests): they are decoupled (unit
// diagonal) and the others solve A_ff d_f = -pg_f - A_fx dfix_x.  With NewtonFaces the kernels find the entries whose step leaves
// the orthant face of the iterate themselves and solve again without them (face_round below), up to `rounds` times.
// One workgroup of 256 threads per row, two kernels, split at kCholLds = 128 entries:
//   k_newton_chol_lds  blocks of up to kCholLds entries (the working sets of the pairwise configurations): the whole matrix in LDS,
//                      read once from the global block, which is never written; trailing update on FP64 MFMA tiles; the BFGS
//                      correction by the row's secant pairs (SecantPairs) applied to the matrix in LDS;
//   k_newton_chol      larger blocks (up to 512): the matrix stays in global memory, the factor goes to the strict upper triangle of
//                      the block; trailing update in 4 x 4 register tiles.  (Their secant correction is k_secant's, gml_solver.hip.)
// Both are launched over all R rows and return at once on the rows of the other.  They share the pieces every blocked Cholesky
// here needs: the 32 x 32 diagonal block factored by one wave in registers (chol_diag_block), the right-hand side with fixed
// entries (rhs_with_fixed), the ridge schedule (next_ridge) and the face round.  They differ on purpose in the back substitution
// (division by L_kk there, multiplication by its reciprocal here; shuffle reductions there, partial sums in LDS here) and in the
// matrix the right-hand side is formed from (the global block there, the corrected matrix in LDS here).
//
// launch_tile_inverse -- the preconditioner tiles of the matrix-free rows, inverted in LDS (k_tile_inverse).
#include "../../include/gml.h"
#include "gml_dev.h"
#include "gml_wg.h"
#include <algorithm>

namespace gml {

typedef double v4d __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------
// Inverse of a preconditioner tile (see gml_solver.hip, Newton-CG): A = sc * H_t - s2 g g^T on the tile's first m entries,
// Cholesky A = L L^T in LDS (left-looking, one thread per row), L^-1 into the upper triangle (thread j owns column j of
// L^-1, kept as row j above the diagonal), A^-1 = L^-T L^-1 written over the tile as a full symmetric matrix.
// ------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(256) void k_tile_inverse(double *__restrict__ H, const long long *__restrict__ hoff, const int *__restrict__ vm,
                                                      const int *__restrict__ wrow, const double *__restrict__ s1, double s2,
                                                      const double *__restrict__ gV) {
    constexpr int LP = T + 1;
    const int64_t v = blockIdx.x;
    const int m = vm[v], tid = threadIdx.x;
    if (m == 0) return;
    double *A = H + hoff[v];
    const double sc = s1[wrow[v]];
    extern __shared__ double sm[]; // L [T][T + 1] | gg [T] | dinv [T] | adiag [T]
    double *L = sm, *gg = sm + T * LP, *dinv = gg + T, *adiag = dinv + T;
    __shared__ double red[4], pivot;
    __shared__ int bad;
    if (tid < T) gg[tid] = (s2 != 0.0 && tid < m) ? gV[v * T + tid] : 0.0;
    __syncthreads();
    double dmax = 0.0;
    if (tid < m) {
        adiag[tid] = sc * A[(int64_t)tid * T + tid] - s2 * gg[tid] * gg[tid];
        dmax = fabs(adiag[tid]);
    }
    for (int o = 32; o > 0; o >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, o));
    if ((tid & 63) == 0) red[tid >> 6] = dmax;
    __syncthreads();
    dmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    double ridge = 0.0;
    bool ok = false;
    for (int attempt = 0; attempt < 6 && !ok; ++attempt) {
        for (int idx = tid; idx < m * T; idx += 256) {
            const int i = idx / T, j = idx % T;
            if (j <= i) L[i * LP + j] = sc * A[(int64_t)i * T + j] - s2 * gg[i] * gg[j] + (i == j ? ridge : 0.0);
        }
        if (tid == 0) bad = 0;
        __syncthreads();
        for (int c = 0; c < m; ++c) {
            double x = 0.0;
            if (tid >= c && tid < m) {
                double x0 = L[tid * LP + c], x1 = 0.0, x2 = 0.0, x3 = 0.0;
                int k = 0;
                for (; k + 3 < c; k += 4) {
                    x0 = fma(-L[tid * LP + k], L[c * LP + k], x0);
                    x1 = fma(-L[tid * LP + k + 1], L[c * LP + k + 1], x1);
                    x2 = fma(-L[tid * LP + k + 2], L[c * LP + k + 2], x2);
                    x3 = fma(-L[tid * LP + k + 3], L[c * LP + k + 3], x3);
                }
                for (; k < c; ++k) x0 = fma(-L[tid * LP + k], L[c * LP + k], x0);
                x = (x0 + x1) + (x2 + x3);
                if (tid == c) pivot = x;
            }
            __syncthreads();
            const double piv = pivot;
            if (!(piv > 1e-12 * dmax) || !isfinite(piv)) { // (uniform: every thread reads the same pivot)
                if (tid == 0) bad = 1;
                break;
            }
            const double dgc = sqrt(piv);
            if (tid == c) {
                L[c * LP + c] = dgc;
                dinv[c] = 1.0 / dgc;
            } else if (tid > c && tid < m) {
                L[tid * LP + c] = x / dgc;
            }
            __syncthreads();
        }
        __syncthreads();
        ok = !bad;
        __syncthreads();
        if (!ok) ridge = ridge == 0.0 ? 1e-10 * fmax(dmax, 1e-300) : ridge * 100.0;
    }
    if (!ok) { // not positive definite (duplicate statistics): the diagonal
        for (int idx = tid; idx < m * T; idx += 256) {
            const int i = idx / T, j = idx % T;
            if (j < m) A[(int64_t)i * T + j] = i == j ? 1.0 / fmax(adiag[i], 1e-300) : 0.0;
        }
        return;
    }
    // column j of L^-1 by forward substitution, stored as row j right of the diagonal: U[j][i] = (L^-1)[i][j], i > j
    if (tid < m) {
        const int j = tid;
        const double dj = dinv[j];
        for (int i = j + 1; i < m; ++i) {
            double s0 = L[i * LP + j] * dj, s1 = 0.0;
            int k = j + 1;
            for (; k + 1 < i; k += 2) {
                s0 = fma(L[i * LP + k], L[j * LP + k], s0);
                s1 = fma(L[i * LP + k + 1], L[j * LP + k + 1], s1);
            }
            if (k < i) s0 = fma(L[i * LP + k], L[j * LP + k], s0);
            L[j * LP + i] = -(s0 + s1) * dinv[i];
        }
    }
    __syncthreads();
    // A^-1[i][j] = sum_{k >= i} (L^-1)[k][i] (L^-1)[k][j],  j <= i
    for (int idx = tid; idx < m * m; idx += 256) {
        const int i = idx / m, j = idx % m;
        if (j > i) continue;
        double a0 = dinv[i] * (i == j ? dinv[i] : L[j * LP + i]), a1 = 0.0;
        int k = i + 1;
        for (; k + 1 < m; k += 2) {
            a0 = fma(L[i * LP + k], L[j * LP + k], a0);
            a1 = fma(L[i * LP + k + 1], L[j * LP + k + 1], a1);
        }
        if (k < m) a0 = fma(L[i * LP + k], L[j * LP + k], a0);
        const double a = a0 + a1;
        A[(int64_t)i * T + j] = a;
        A[(int64_t)j * T + i] = a;
    }
}

void launch_tile_inverse(int T, double *H, const long long *hoff, const int *vm, const int *wrow, const double *s1, double s2, const double *gV,
                         int64_t ntiles, hipStream_t st) {
    if (ntiles <= 0) return;
    const size_t lds = sizeof(double) * ((size_t)T * (T + 1) + 3 * T);
    if (T == 64) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_tile_inverse<64>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_tile_inverse<64>, dim3((unsigned)ntiles), dim3(256), lds, st, H, hoff, vm, wrow, s1, s2, gV);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_tile_inverse<128>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_tile_inverse<128>, dim3((unsigned)ntiles), dim3(256), lds, st, H, hoff, vm, wrow, s1, s2, gV);
    }
}

// ------------------------------------------------------------------------------------------
// The pieces the two Cholesky kernels share
// ------------------------------------------------------------------------------------------
constexpr int PW = 32; // panel width: columns factored together, one lane of a half-wave per row of the diagonal block

// value of lane l (wave-uniform index) of a double: two v_readlane_b32, the result in scalar registers.  (__shfl goes through
// ds_bpermute: an LDS round trip per value -- the 496 of a 32 x 32 diagonal block were most of the batched Cholesky kernels' time.)
__device__ __forceinline__ double readlane_f64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// sum over the 256 threads of a workgroup through 8 x 32 doubles of LDS (no shuffles); every thread gets the result
__device__ __forceinline__ double wg_sum(double v, double *buf /* [256] */) {
    __syncthreads();
    buf[threadIdx.x] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x < 64) {
        s = buf[threadIdx.x] + buf[threadIdx.x + 64] + buf[threadIdx.x + 128] + buf[threadIdx.x + 192];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    }
    __syncthreads();
    if (threadIdx.x == 0) buf[0] = s;
    __syncthreads();
    return buf[0];
}

// the ridge of the next attempt after a failed factorisation
__device__ __forceinline__ double next_ridge(double ridge, double dmax) { return ridge == 0.0 ? 1e-12 * fmax(dmax, 1e-300) : ridge * 100.0; }

// Entry i of the right-hand side: -pg_i for a free entry -- less, when some entries are fixed (anyfixed), the fixed steps' share
// A[i][j] dfx[j] -- and the fixed step itself for a fixed one.  a_sym(i, j): the matrix without masks, any order of i and j.
template <typename Mat>
__device__ __forceinline__ double rhs_with_fixed(int i, int m, bool anyfixed, const double *pg, const double *fx, const double *dfx, Mat a_sym) {
    double v = -pg[i];
    if (anyfixed) {
        if (fx[i] != 0.0) {
            v = dfx[i];
        } else {
            for (int j = 0; j < m; ++j)
                if (fx[j] != 0.0 && dfx[j] != 0.0) v -= a_sym(i, j) * dfx[j];
        }
    }
    return v;
}

// The 32 x 32 diagonal block of a panel, by one wave.  Lane `lane` holds row t = lane & 31 of the block in v (lower part and
// diagonal; rows from pw on: zeros).  Right-looking: column c is scaled, then every lane updates the rest of its row with L[k][c]
// read from lane k -- independent FMAs: the dependent chain is the 32 pivots, not the 496 inner products an LDS-resident
// left-looking sweep serialises.  Straight-line code: a pivot that fails (not above 1e-300 dmax, or not finite) or lies beyond the
// block is replaced by 1 and remembered, so that no control flow separates the columns and the scheduler can start a pivot's chain
// under the previous column's updates; the rows from pw on being zero, the live entries see the same operations either way.
// On success v holds row t of L, store(v, L_tt, 1 / L_tt) puts them where the kernel keeps them, and yp[0 .. pw) -- the panel's
// part of the right-hand side -- is forward-substituted (lanes = rows of the block).  Returns whether a live pivot failed;
// then nothing is stored and the attempt is to be discarded.
template <typename Store>
__device__ __forceinline__ bool chol_diag_block(double (&v)[PW], int lane, int pw, double dmax, double *yp, Store store) {
    const int t = lane & 31;
    bool fail = false;
#pragma unroll
    for (int c = 0; c < PW; ++c) {
        double piv = readlane_f64(v[c], c);
        const bool live = c < pw, good = piv > 1e-300 * dmax && isfinite(piv);
        fail |= live && !good;
        piv = live && good ? piv : 1.0;
        // 1 / sqrt(piv): the hardware estimate + two Newton steps (a square root and a division in FP64 are ~40 instructions
        // each, and the 32 pivots are the kernels' one sequential chain)
        double inv = __builtin_amdgcn_rsq(piv);
        inv = inv * fma(-0.5 * piv * inv, inv, 1.5);
        inv = inv * fma(-0.5 * piv * inv, inv, 1.5);
        const double dgc = piv * inv;
        v[c] = t == c ? dgc : v[c] * inv;
        const double ltc = t > c ? v[c] : 0.0;
#pragma unroll
        for (int k = c + 1; k < PW; ++k) v[k] = fma(-ltc, readlane_f64(v[c], k), v[k]);
    }
    if (fail) return true;
    double dgt = 1.0;
#pragma unroll
    for (int k = 0; k < PW; ++k)
        if (k == t) dgt = v[k];
    const double invd = 1.0 / dgt;
    store(v, dgt, invd);
    double yc = t < pw ? yp[t] : 0.0;
#pragma unroll
    for (int k = 0; k < PW; ++k) {
        if (k < pw) {
            const double yk = readlane_f64(yc, k) * readlane_f64(invd, k);
            if (t == k) yc = yk;
            else if (t > k) yc = fma(-v[k], yk, yc);
        }
    }
    if (lane < pw) yp[t] = yc;
    return false;
}

// Orthant faces.  The line search projects the step onto the orthant of the iterate (face_candidate, gml_wg.h).  Entries whose
// step leaves that face are fixed where the projection would put them and, when they carry more than `share` of the predicted
// decrease, the others are solved again -- with correlated statistics the unconstrained solution is full of moves that cancel each
// other, and clipping one of a pair leaves the other uncompensated (the matrix-free rows do the same: k_pcg_faces).
// One round on the solution y of a row's m entries (columns Fr of the iterate Xr with kinds kr): returns whether to solve again, with
// the candidates marked in fx (1) and their steps in dfx; otherwise fx is as it was.  (While it runs a candidate is 2.0 in fx.)
__device__ __forceinline__ bool face_round(int m, double *fx, double *dfx, const double *y, const double *pg, const int *Fr, const double *Xr,
                                           const uint8_t *kr, double share, double *red, int *redi) {
    const int tid = threadIdx.x;
    int nf = 0;
    double mass = 0, total = 0;
    for (int a = tid; a < m; a += 256) {
        if (fx[a] != 0.0) continue;
        const int c = Fr[a];
        const double dc = y[a], pv = pg[a];
        total += fabs(pv * dc);
        double fixed;
        if (face_candidate(Xr[c], dc, pv, kr[c], &fixed)) {
            mass += fabs(pv * (dc - fixed));
            fx[a] = 2.0;
            dfx[a] = fixed;
            ++nf;
        }
    }
    nf = block_sum_i(nf, redi);
    mass = block_sum(mass, red);
    total = block_sum(total, red);
    const bool again = nf > 0 && mass > share * total;
    for (int a = tid; a < m; a += 256)
        if (fx[a] == 2.0) fx[a] = again ? 1.0 : 0.0;
    __syncthreads();
    return again;
}

// ------------------------------------------------------------------------------------------
// k_newton_chol: blocked right-looking Cholesky on the global block.
//
// A = s1 H - s2 g g^T is read from the lower triangle of the block and never written, so a ridge restart starts from it again; the
// factor goes to the strict upper triangle as U[k][i] = L[i][k] (row k = column k of L, contiguous in i), its diagonal to LDS.
// Per panel of 32 columns:
//   (1) the 32 x 32 diagonal block -> LDS, factored by one wave, which also forward-solves the panel of the right-hand side;
//   (2) every row below the panel solves its 32 entries against that block (one thread per row, the entries in registers,
//       the block read from LDS as broadcasts) and leaves them in LDS (Lp) and in U;
//   (3) the trailing matrix is updated from Lp alone, in 4 x 4 register tiles spread over the 256 threads -- first panel:
//       read from the lower triangle, written to the upper; later panels: updated in place in the upper -- and so is the
//       rest of the right-hand side: the forward substitution costs no pass of its own.
// The back substitution walks the panels in reverse: 32 dot products of rows of U with the solved tail (coalesced, one wave
// per 8 rows), the diagonal block back into LDS, one wave for the 32 x 32 triangular solve.
// Why: the first two versions had a left-looking panel Cholesky (every panel re-read all previous ones through L2, two barriers per
// 32 x 32 block, the diagonal block factored by 496 dependent LDS inner products) and a one-wave LDS path for small blocks (m
// dependent column steps): 0.32 ms at 100 entries, 0.44 ms at 190, 0.68 ms at 250 for 128 rows (scripts/gpu_newton_ubench.py); this
// one: 0.13 / 0.28 / 0.45 ms, 0.03 ms at 30 entries.  What is left is latency: three dependent global round trips and one
// wave's 32 pivots per panel.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_newton_chol(double *__restrict__ H, const long long *__restrict__ hoff, const int *__restrict__ mt,
                                                     const int *__restrict__ msz, const double *__restrict__ s1, double s2,
                                                     const double *__restrict__ gF, const double *__restrict__ pgF, int cap,
                                                     double *__restrict__ dout, double *__restrict__ Sdiag, int mcap /* >= every msz */,
                                                     // orthant faces: the working sets' columns, the iterates and their column kinds,
                                                     // the share of the predicted decrease that triggers a re-solve, the number of
                                                     // re-solves; F = NULL: none
                                                     const int *__restrict__ F, const double *__restrict__ X, const uint8_t *__restrict__ kind,
                                                     int64_t Qp, double share, int rounds,
                                                     // entries fixed from the start (tests): fix != 0 keeps the step dfix
                                                     const uint8_t *__restrict__ fix, const double *__restrict__ dfix,
                                                     int mlo /* blocks of up to mlo entries are another kernel's */) {
    constexpr int LP = PW + 1;
    const int r = blockIdx.x;
    const int m = msz[r];
    if (m == 0 || m <= mlo) return;
    const int hp = 32 * mt[r];
    double *A = H + hoff[r];
    const double sc = s1[r];
    const double *g = gF + (int64_t)r * cap, *pg = pgF + (int64_t)r * cap;
    extern __shared__ double sm[]; // dgw | dg | y | gg | fx | dfx [mcap each] | Ld [32][33] | tmp [32] | Lp [mcap - 32 (>= 32)][33]
    double *dgw = sm, *dg = sm + mcap, *y = sm + 2 * mcap, *gg = sm + 3 * mcap, *fx = sm + 4 * mcap, *dfx = sm + 5 * mcap, *Ld = sm + 6 * mcap,
           *tmp = Ld + PW * LP, *Lp = tmp + PW;
    __shared__ int bad;
    __shared__ double red[4];
    __shared__ int redi[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool masked = fix != nullptr || F != nullptr; // some entries may be fixed
    for (int i = tid; i < m; i += 256) {
        gg[i] = s2 != 0.0 ? g[i] : 0.0;
        fx[i] = fix && fix[(int64_t)r * cap + i] ? 1.0 : 0.0;
        dfx[i] = fix ? dfix[(int64_t)r * cap + i] : 0.0;
    }
    __syncthreads();
    auto a_orig = [&](int i, int j) { return sc * A[(int64_t)i * hp + j] - s2 * gg[i] * gg[j]; }; // i >= j: the matrix itself
    auto a_low = [&](int i, int j) { // ... with the fixed entries decoupled (unit diagonal)
        if (masked && (fx[i] != 0.0 || fx[j] != 0.0)) return i == j ? 1.0 : 0.0;
        return a_orig(i, j);
    };
    double dmax = 0;
    for (int i = tid; i < m; i += 256) dmax = fmax(dmax, fabs(a_low(i, i)));
    dmax = block_max(dmax, red);
    if (tid == 0) Sdiag[r] = a_orig(m - 1, m - 1);
    for (int face = 0;; ++face) { // (re-solves on an orthant face, see the end of the loop)
    double ridge = 0.0;
    bool ok = false;
    for (int attempt = 0; attempt < 10 && !ok; ++attempt) {
        for (int i = tid; i < m; i += 256) {
            dgw[i] = a_low(i, i) + (fx[i] != 0.0 ? 0.0 : ridge);
            y[i] = rhs_with_fixed(i, m, masked, pg, fx, dfx, [&](int a, int b) { return a >= b ? a_orig(a, b) : a_orig(b, a); });
        }
        if (tid == 0) bad = 0;
        __syncthreads();
        for (int c0 = 0; c0 < m; c0 += PW) {
            const int pw = m - c0 < PW ? m - c0 : PW;
            const bool first = c0 == 0;
            // (1) diagonal block -> Ld (lower part; the working diagonal from dgw)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = tid + 256 * q, c = e >> 5, k = e & 31;
                double v = 0.0;
                if (c < pw && k < c) v = first ? a_low(c0 + c, c0 + k) : A[(int64_t)(c0 + k) * hp + c0 + c];
                else if (c < pw && k == c) v = dgw[c0 + c];
                Ld[c * LP + k] = v;
            }
            __syncthreads();
            if (wave == 0) {
                const int t = lane & 31;
                double v[PW];
#pragma unroll
                for (int k = 0; k < PW; ++k) v[k] = Ld[t * LP + k];
                const bool fail = chol_diag_block(v, lane, pw, dmax, y + c0, [&](const double (&l)[PW], double dgt, double invd) {
                    if (lane < pw) {
#pragma unroll
                        for (int k = 0; k < PW; ++k) Ld[t * LP + k] = k <= t ? l[k] : 0.0;
                        dg[c0 + t] = dgt;
                    }
                    tmp[t] = invd; // 1 / L_tt of this block, for the panel solve
                });
                if (fail && lane == 0) bad = 1;
            }
            __syncthreads();
            if (!bad) { // the factored block's strict lower part -> U (the back substitution reads it from there)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = tid + 256 * q, c = e >> 5, k = e & 31;
                    if (c < pw && k < c) A[(int64_t)(c0 + k) * hp + c0 + c] = Ld[c * LP + k];
                }
            }
            if (bad) break;
            const int r0 = c0 + pw, nt = m - r0; // trailing rows
            if (nt <= 0) break;
            // (2) panel solve: row i = r0 + a, a = tid, tid + 256
            for (int a = tid; a < nt; a += 256) {
                const int i = r0 + a;
                double x[PW];
#pragma unroll
                for (int c = 0; c < PW; ++c) x[c] = c < pw ? (first ? a_low(i, c0 + c) : A[(int64_t)(c0 + c) * hp + i]) : 0.0;
#pragma unroll
                for (int c = 0; c < PW; ++c) {
                    if (c < pw) {
                        double v = x[c];
#pragma unroll
                        for (int k = 0; k < c; ++k) v = fma(-x[k], Ld[c * LP + k], v);
                        x[c] = v * tmp[c];
                    }
                }
#pragma unroll
                for (int c = 0; c < PW; ++c) {
                    Lp[a * LP + c] = x[c];
                    if (c < pw) A[(int64_t)(c0 + c) * hp + i] = x[c];
                }
            }
            __syncthreads();
            // (3) trailing update in 4 x 4 tiles (ib >= jb), and the rest of the right-hand side
            const int nb = (nt + 3) >> 2, ntile = nb * (nb + 1) / 2;
            for (int tile = tid; tile < ntile; tile += 256) {
                int ib = (int)((sqrt(8.0 * (double)tile + 1.0) - 1.0) * 0.5);
                while ((ib + 1) * (ib + 2) / 2 <= tile) ++ib;
                while (ib * (ib + 1) / 2 > tile) --ib;
                const int jb = tile - ib * (ib + 1) / 2;
                double acc[4][4], old[4][4]; // (the entries to be updated are requested first: their latency hides under the products)
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        acc[a][b] = 0.0;
                        const int ia = 4 * ib + a, jbb = 4 * jb + b;
                        old[a][b] = (ia < nt && jbb < ia) ? (first ? a_low(r0 + ia, r0 + jbb) : A[(int64_t)(r0 + jbb) * hp + r0 + ia]) : 0.0;
                    }
                const double *li = Lp + (4 * ib) * LP, *lj = Lp + (4 * jb) * LP;
                for (int c = 0; c < pw; ++c) {
                    double va[4], vb[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        va[a] = li[a * LP + c];
                        vb[a] = lj[a * LP + c];
                    }
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) acc[a][b] = fma(va[a], vb[b], acc[a][b]);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int ia = 4 * ib + a, jbb = 4 * jb + b;
                        if (ia >= nt || jbb > ia) continue;
                        const int i = r0 + ia, j = r0 + jbb;
                        if (i == j) dgw[i] -= acc[a][b];
                        else A[(int64_t)j * hp + i] = old[a][b] - acc[a][b];
                    }
            }
            for (int a = tid; a < nt; a += 256) {
                double v = 0.0;
                for (int c = 0; c < pw; ++c) v = fma(Lp[a * LP + c], y[c0 + c], v);
                y[r0 + a] -= v;
            }
            __syncthreads();
        }
        __syncthreads();
        ok = !bad;
        __syncthreads();
        if (!ok) ridge = next_ridge(ridge, dmax);
    }
    if (!ok) {
        for (int i = tid; i < m; i += 256) dout[(int64_t)r * cap + i] = 0.0;
        return;
    }
    // back substitution L^T d = y, panels in reverse
    for (int c0 = (m - 1) / PW * PW; c0 >= 0; c0 -= PW) {
        const int pw = m - c0 < PW ? m - c0 : PW, r0 = c0 + pw;
        // tmp[c] = sum_{i >= r0} L[i][c0 + c] d_i = sum_i U[c0 + c][i] y[i]
        double ldv[4]; // (requested before the dot products: one round trip for both)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q, c = e >> 5, k = e & 31;
            ldv[q] = (c < pw && k < c) ? A[(int64_t)(c0 + k) * hp + c0 + c] : 0.0;
        }
        for (int c = wave; c < pw; c += 4) {
            double v = 0.0;
            for (int i = r0 + lane; i < m; i += 64) v = fma(A[(int64_t)(c0 + c) * hp + i], y[i], v);
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) tmp[c] = v;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q;
            Ld[(e >> 5) * LP + (e & 31)] = ldv[q];
        }
        __syncthreads();
        if (wave == 0) {
            const int c = lane & 31;
            double yc = c < pw ? y[c0 + c] - tmp[c] : 0.0;
            for (int k = pw - 1; k >= 0; --k) { // d_k = y_k / L_kk; y_c -= L[c0 + k][c0 + c] d_k for c < k
                const double dk = readlane_f64(yc, k) / dg[c0 + k];
                if (c == k) yc = dk;
                else if (c < k) yc = fma(-Ld[k * LP + c], dk, yc);
            }
            if (lane < pw) y[c0 + c] = yc;
        }
        __syncthreads();
    }
    if (!F || face >= rounds) break;
    if (!face_round(m, fx, dfx, y, pg, F + (int64_t)r * cap, X + (int64_t)r * Qp, kind + (int64_t)r * Qp, share, red, redi)) break;
    } // face
    for (int i = tid; i < m; i += 256) dout[(int64_t)r * cap + i] = y[i];
}

// ------------------------------------------------------------------------------------------
// k_newton_chol_lds: the same solve for blocks of up to kCholLds entries with the whole matrix in LDS.
//
// k_newton_chol keeps the block in global memory and pays three dependent L2 round trips per panel: 0.13 ms for 128 rows of 100
// entries, one launch per Newton iteration of a solve whose other kernels had shrunk to less (profiles/r5_shard128_kernel_stats.csv).
// Here A = s1 H - s2 g g^T (lower triangle, masked) is loaded once into W [mcap][mcap + 1] and factored in place: the diagonal block
// by one wave in registers (as there), the panel below it one thread per row, the trailing matrix by v_mfma_f64_16x16x4_f64 tiles
// straight from W (lane (li, q) feeds A[row li][k q] and B[k q][col li], i.e. the same access for both operands of L21 L21^T), the
// back substitution from W.  A ridge restart or an orthant-face re-solve reloads W from the global block, which is never written.
// Same arithmetic order inside a panel as there; results agree to rounding.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_newton_chol_lds(const double *__restrict__ H, const long long *__restrict__ hoff, const int *__restrict__ mt,
                                                         const int *__restrict__ msz, const double *__restrict__ s1, double s2,
                                                         const double *__restrict__ gF, const double *__restrict__ pgF, int cap,
                                                         double *__restrict__ dout, double *__restrict__ Sdiag, int mcap /* multiple of 32, <= 128, >= every msz handled here */,
                                                         const int *__restrict__ F, const double *__restrict__ X, const uint8_t *__restrict__ kind,
                                                         int64_t Qp, double share, int rounds, const uint8_t *__restrict__ fix,
                                                         const double *__restrict__ dfix,
                                                         // BFGS correction of the (sub-sampled) block by the row's last secant pairs,
                                                         // applied to the matrix in LDS (npairs = NULL: none)
                                                         const double *__restrict__ secS, const double *__restrict__ secY,
                                                         const int *__restrict__ npairs, int64_t pair_stride) {
    const int r = blockIdx.x;
    const int m = msz[r];
    if (m == 0 || m > mcap) return;
    const int hp = 32 * mt[r], LDW = mcap + 1, mp = (m + 15) & ~15;
    const double *A = H + hoff[r];
    const double sc = s1[r];
    const double *g = gF + (int64_t)r * cap, *pg = pgF + (int64_t)r * cap;
    extern __shared__ double sm[]; // W [mcap][mcap + 1] | idg | y | gg | fx | dfx [mcap each]
    double *W = sm, *idg = W + mcap * LDW, *y = idg + mcap, *gg = y + mcap, *fx = gg + mcap, *dfx = fx + mcap;
    __shared__ double part8[8 * 32];
    __shared__ int bad;
    __shared__ double red[4];
    __shared__ int redi[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool masked = fix != nullptr || F != nullptr; // some entries may be fixed
    // one global round trip: the lower triangle of s1 H straight into W, eight independent loads per thread and turn (one element
    // per turn, each waiting for its own load, took 28 of the 99 us of a 100-entry solve); the rank-one term, the masks and the ridge
    // are applied in LDS
    for (int i = tid; i < m; i += 256) gg[i] = s2 != 0.0 ? g[i] : 0.0;
    auto load_raw = [&]() { // W <- sc * H on the lower triangle of the first mp rows (rows m .. mp - 1, the MFMA tile padding: zero)
        const int total = mp * mp;
        for (int base = 0; base < total; base += 256 * 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int idx = base + tid + 256 * u, i = idx / mp, j = idx - i * mp;
                v[u] = (idx < total && j <= i && i < m) ? A[(int64_t)i * hp + j] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int idx = base + tid + 256 * u, i = idx / mp, j = idx - i * mp;
                if (idx < total && j <= i) W[i * LDW + j] = sc * v[u];
            }
        }
    };
    // B <- B + y y^T / (y.s) - (B s)(B s)^T / (s.B s) for the row's pairs, oldest first, on B = s1 H - s2 g g^T (the pairs come from
    // exact gradients, so they describe the true Hessian along the last steps: gml_solver.hip, k_secant, which keeps them and
    // applies them itself to the larger blocks).  W holds s1 H; the rank-one term rides along in B s only.
    const int np = npairs ? npairs[r] : 0;
    auto secant = [&]() {
        double *vs = fx, *vy = dfx; // (free here: the masks are set up after the correction) -- s and y of the pair; y doubles as B s below
        for (int l = 0; l < np; ++l) {
            __syncthreads();
            for (int i = tid; i < m; i += 256) {
                vs[i] = secS[l * pair_stride + (int64_t)r * cap + i];
                vy[i] = secY[l * pair_stride + (int64_t)r * cap + i];
            }
            __syncthreads();
            double gs = 0.0;
            if (s2 != 0.0) {
                for (int i = tid; i < m; i += 256) gs += gg[i] * vs[i];
                gs = wg_sum(gs, part8);
            }
            double bs = 0.0, sAs = 0.0, ysl = 0.0;
            if (tid < m) {
                const int i = tid;
                for (int j = 0; j <= i; ++j) bs = fma(W[i * LDW + j], vs[j], bs);
                for (int j = i + 1; j < m; ++j) bs = fma(W[j * LDW + i], vs[j], bs);
                bs -= s2 * gg[i] * gs;
                sAs = vs[i] * bs;
                ysl = vs[i] * vy[i];
            }
            sAs = wg_sum(sAs, part8);
            ysl = wg_sum(ysl, part8);
            if (!(sAs > 0.0 && ysl > 0.0)) continue; // (uniform)
            if (tid < m) y[tid] = bs; // (y: the right-hand side's place, not set yet)
            __syncthreads();
            const double ia = 1.0 / sAs, iy = 1.0 / ysl;
            for (int idx = tid; idx < m * m; idx += 256) {
                const int i = idx / m, j = idx - i * m;
                if (j <= i) W[i * LDW + j] += vy[i] * vy[j] * iy - y[i] * y[j] * ia;
            }
        }
        __syncthreads();
    };
    load_raw();
    __syncthreads();
    if (np > 0) secant();
    for (int i = tid; i < m; i += 256) { // (the masks, after the correction borrowed their place)
        fx[i] = fix && fix[(int64_t)r * cap + i] ? 1.0 : 0.0;
        dfx[i] = fix ? dfix[(int64_t)r * cap + i] : 0.0;
    }
    __syncthreads();
    double dmax = 0;
    for (int i = tid; i < m; i += 256) dmax = fmax(dmax, masked && fx[i] != 0.0 ? 1.0 : fabs(W[i * LDW + i] - s2 * gg[i] * gg[i]));
    dmax = block_max(dmax, red);
    if (tid == 0) Sdiag[r] = W[(m - 1) * LDW + m - 1] - s2 * gg[m - 1] * gg[m - 1];
    bool fresh = true;              // W holds the raw block
    bool anyfixed = fix != nullptr; // some entries are decoupled (test hook, or a face re-solve below)
    for (int face = 0;; ++face) { // (re-solves on an orthant face, see the end of the loop)
    double ridge = 0.0;
    bool ok = false;
    for (int attempt = 0; attempt < 10 && !ok; ++attempt) {
        if (!fresh) {
            __syncthreads();
            load_raw();
            __syncthreads();
            if (np > 0) { // (the correction borrows the masks' place: saved around it)
                double f0 = 0.0, d0 = 0.0;
                if (tid < m) {
                    f0 = fx[tid];
                    d0 = dfx[tid];
                }
                secant();
                if (tid < m) {
                    fx[tid] = f0;
                    dfx[tid] = d0;
                }
                __syncthreads();
            }
        }
        fresh = false;
        // the right-hand side first, from the matrix as it stands in W -- s1 H with the secant correction, the SAME matrix that is
        // factored below -- before the masks decouple the fixed entries: a free row's share of the fixed steps is A_corr[i][j] dfx[j]
        // (the global block lacks the correction: both sides of a face re-solve must see one matrix)
        for (int i = tid; i < m; i += 256)
            y[i] = rhs_with_fixed(i, m, anyfixed, pg, fx, dfx,
                                  [&](int a, int b) { return (a >= b ? W[a * LDW + b] : W[b * LDW + a]) - s2 * gg[a] * gg[b]; });
        __syncthreads();
        // the (masked) matrix: rank-one term, fixed entries decoupled (unit diagonal), ridge on the free diagonal
        if (s2 != 0.0 || anyfixed || ridge != 0.0) {
            for (int idx = tid; idx < m * m; idx += 256) {
                const int i = idx / m, j = idx - i * m;
                if (j > i) continue;
                double v = W[i * LDW + j] - s2 * gg[i] * gg[j];
                if (anyfixed && (fx[i] != 0.0 || fx[j] != 0.0)) v = i == j ? 1.0 : 0.0;
                else if (i == j) v += ridge;
                W[i * LDW + j] = v;
            }
        }
        if (tid == 0) bad = 0;
        __syncthreads();
        for (int c0 = 0; c0 < m; c0 += PW) {
            const int pw = m - c0 < PW ? m - c0 : PW;
            if (wave == 0) { // (1) diagonal block, in place
                const int t = lane & 31;
                double v[PW];
#pragma unroll
                for (int k = 0; k < PW; ++k) v[k] = (t < pw && k <= t) ? W[(c0 + t) * LDW + c0 + k] : 0.0;
                const bool fail = chol_diag_block(v, lane, pw, dmax, y + c0, [&](const double (&l)[PW], double, double invd) {
                    if (lane < pw) {
#pragma unroll
                        for (int k = 0; k < PW; ++k)
                            if (k <= t) W[(c0 + t) * LDW + c0 + k] = l[k];
                        idg[c0 + t] = invd; // 1 / L_tt
                    }
                });
                if (fail && lane == 0) bad = 1;
            }
            __syncthreads();
            if (bad) break;
            const int r0 = c0 + pw, nt = m - r0; // trailing rows
            if (nt <= 0) break;
            // (2) panel solve: row i = r0 + a, one thread per row (pw = 32 here: only the last panel is narrower, and it has no rows below)
            for (int a = tid; a < nt; a += 256) {
                double *wr = W + (r0 + a) * LDW + c0;
                double x[PW];
#pragma unroll
                for (int c = 0; c < PW; ++c) x[c] = wr[c];
#pragma unroll
                for (int c = 0; c < PW; ++c) {
                    double v = x[c];
                    const double *lc = W + (c0 + c) * LDW + c0;
#pragma unroll
                    for (int k = 0; k < c; ++k) v = fma(-x[k], lc[k], v);
                    x[c] = v * idg[c0 + c];
                }
#pragma unroll
                for (int c = 0; c < PW; ++c) wr[c] = x[c];
            }
            __syncthreads();
            // (3) trailing update W22 -= L21 L21^T in 16 x 16 MFMA tiles (I >= J) over the waves, and the rest of the right-hand side
            {
                const int li = lane & 15, q = lane >> 4;
                const int T = (nt + 15) >> 4, ntile = T * (T + 1) / 2;
                for (int tile = wave; tile < ntile; tile += 4) {
                    int I = 0, rem = tile;
                    while (rem > I) {
                        rem -= I + 1;
                        ++I;
                    }
                    const int J = rem;
                    const double *pa = W + (r0 + 16 * I + li) * LDW + c0 + q, *pb = W + (r0 + 16 * J + li) * LDW + c0 + q;
                    v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int kk = 0; kk < PW / 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[4 * kk], pb[4 * kk], acc, 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int row = r0 + 16 * I + q + 4 * j, col = r0 + 16 * J + li;
                        if (row < mp && col <= row) W[row * LDW + col] -= acc[j];
                    }
                }
                for (int a = tid; a < nt; a += 256) {
                    const double *wr = W + (r0 + a) * LDW + c0;
                    double v = 0.0;
#pragma unroll
                    for (int c = 0; c < PW; ++c) v = fma(wr[c], y[c0 + c], v);
                    y[r0 + a] -= v;
                }
            }
            __syncthreads();
        }
        __syncthreads();
        ok = !bad;
        __syncthreads();
        if (!ok) ridge = next_ridge(ridge, dmax);
    }
    if (!ok) {
        for (int i = tid; i < m; i += 256) dout[(int64_t)r * cap + i] = 0.0;
        return;
    }
    // back substitution L^T d = y, panels in reverse
    for (int c0 = (m - 1) / PW * PW; c0 >= 0; c0 -= PW) {
        const int pw = m - c0 < PW ? m - c0 : PW, r0 = c0 + pw;
        // tmp[c] = sum_{i >= r0} L[i][c0 + c] d_i: lanes over the columns, the rows split over the eight half-waves, partial sums
        // through LDS (no shuffles: a xor-reduction is six ds_bpermute round trips per column)
        {
            const int c = lane & 31, part = tid >> 5;
            double v = 0.0;
            if (c < pw)
                for (int i = r0 + part; i < m; i += 8) v = fma(W[i * LDW + c0 + c], y[i], v);
            part8[part * 32 + c] = v;
        }
        __syncthreads();
        if (wave == 0) {
            const int c = lane & 31;
            double yc = 0.0;
            if (c < pw) {
                double ts = 0.0;
#pragma unroll
                for (int q = 0; q < 8; ++q) ts += part8[q * 32 + c];
                yc = y[c0 + c] - ts;
            }
            double lc[PW], iv = c < pw ? idg[c0 + c] : 0.0; // column c of the block, below the diagonal: L[c0 + k][c0 + c], k > c
#pragma unroll
            for (int k = 0; k < PW; ++k) lc[k] = (k < pw && c < k) ? W[(c0 + k) * LDW + c0 + c] : 0.0;
#pragma unroll
            for (int k = PW - 1; k >= 0; --k) { // d_k = y_k / L_kk; y_c -= L[c0 + k][c0 + c] d_k for c < k
                if (k < pw) {
                    const double dk = readlane_f64(yc, k) * readlane_f64(iv, k);
                    if (c == k) yc = dk;
                    else yc = fma(-lc[k], dk, yc);
                }
            }
            if (lane < pw) y[c0 + c] = yc;
        }
        __syncthreads();
    }
    if (!F || face >= rounds) break;
    if (!face_round(m, fx, dfx, y, pg, F + (int64_t)r * cap, X + (int64_t)r * Qp, kind + (int64_t)r * Qp, share, red, redi)) break;
    anyfixed = true;
    } // face
    for (int i = tid; i < m; i += 256) dout[(int64_t)r * cap + i] = y[i];
}

void launch_newton_solve(double *H, const long long *hoff, const int *mt, const int *msz, const double *s1, double s2,
                         const double *gF, const double *pgF, int R, int cap, double *dout, double *Sdiag, hipStream_t st, int maxm,
                         const NewtonFaces *faces, const uint8_t *fix, const double *dfix, const SecantPairs *pairs) {
    // maxm: largest block of this call, as far as the host knows it (0 = unknown): sizes the LDS of a workgroup
    int mcap = maxm <= 0 || maxm > cap ? cap : maxm;
    mcap = (mcap + 31) / 32 * 32;
    const NewtonFaces nf = faces ? *faces : NewtonFaces{};
    // blocks of up to 128 entries: the matrix in LDS (k_newton_chol_lds); larger ones: the blocked kernel on the global block
    const int msmall = mcap < kCholLds ? mcap : kCholLds;
    const SecantPairs sp = pairs ? *pairs : SecantPairs{};
    {
        const size_t lds = sizeof(double) * ((size_t)msmall * (msmall + 1) + 5 * (size_t)msmall + 32);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_newton_chol_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_newton_chol_lds, dim3((unsigned)R), dim3(256), lds, st, H, hoff, mt, msz, s1, s2, gF, pgF, cap, dout, Sdiag, msmall, nf.F,
                           nf.X, nf.kind, nf.Qp, nf.share, nf.rounds, fix, dfix, sp.S, sp.Y, sp.npairs, sp.stride);
    }
    if (mcap > kCholLds) {
        const size_t lds = sizeof(double) * ((size_t)6 * mcap + 32 * 33 + 32 + (size_t)std::max(mcap - 32, 32) * 33);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_newton_chol), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_newton_chol, dim3((unsigned)R), dim3(256), lds, st, H, hoff, mt, msz, s1, s2, gF, pgF, cap, dout, Sdiag, mcap, nf.F, nf.X,
                           nf.kind, nf.Qp, nf.share, nf.rounds, fix, dfix, kCholLds);
    }
}

} // namespace gml
