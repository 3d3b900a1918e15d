// What the two int8 forward kernels share (k_fwd_i8 in gml_i8_fwd.hip, k_fwd_i8w in gml_kernels_i8w.hip): both run a workgroup of
// 4 waves along the samples -- 256 samples x one 32-node tile, WM = 2 MFMA sample tiles per wave -- over an LDS-DMA ring whose
// 64-column steps are 2 KB of sample bits followed by the digit-plane rows of Theta, and both end in a pointwise epilogue that
// writes balanced base-256 digits of V.  The DMA issue and the waits, the layered exp epilogues and the folds of the plane sums
// differ on purpose and stay with the kernels.  Device side; included by those two files only.
#pragma once
#include "gml_i8.h"
#include "gml_i8_map.h"
#include <type_traits>

namespace gml {

constexpr int WM = 2; // 32-sample MFMA tiles per wave

// rounding to an integer by adding 1.5 * 2^52 (the integer is then the low word(s) of the sum); 1.5 * 2^84 rounds to multiples of
// 2^32, for values carried with a scale of 2^32
constexpr double MAGIC = 6755399441055744.0, MAGIC32 = 6755399441055744.0 * 4294967296.0;

// Dither of the V rounding.  Round-to-nearest is coherent whenever a sparse theta row leaves only a few distinct energies
// (thousands of samples share each rounding error), which made the realised error of f and grad approach the K * tau / 2 worst
// case instead of ~ sqrt(K) * tau.  The dither is a golden-ratio (Weyl) sequence in the global sample index, offset per node:
// a fixed function of (node, sample), independent of tiling, node sharding and compaction, so results stay bit-identical across
// GPU counts.  dither_seed(): the hash of the lane's first sample (kw: first sample of the wave, h: the lane's half);
// dither_hash(): that of its element idx = 32 i + 8 g + j, which sits idx samples further -- as an int, 2^32 times a dither in
// [-1/2, 1/2).
constexpr unsigned DITHER_NODE = 0x85EBCA6Bu, GOLD = 0x9E3779B9u;
__device__ __forceinline__ unsigned dither_seed(int rc, int64_t kw, int h) { return (unsigned)rc * DITHER_NODE + (unsigned)(kw + 4 * h) * GOLD; }
__device__ __forceinline__ unsigned dither_hash(unsigned dh0, int idx) { return dh0 + (unsigned)idx * GOLD; }
__device__ __forceinline__ double dither_unit(unsigned dh0, int idx) { return (double)(int)dither_hash(dh0, idx) * 2.3283064365386963e-10; } // 2^-32

// The tables behind the ring: 2^(j/64), j < 64 -- for the exp forms (FORM 0) with j << 14 taken off the high word: the exponent
// of 2^(n >> 6), n = 64 q + j, then goes on as n << 14 (= (q << 20) + (j << 14)) in one shift-add -- and for RPLE (FORM 2) the
// log table c_j = 1 + (j + 1/2)/64 -> 1/c_j, log c_j.  Ends with the barrier that makes them visible to every wave (the ring
// uses raw s_barrier without an LDS wait).
template <int FORM>
__device__ __forceinline__ void fill_tables(double *etab, int tid) {
    if (tid < 64) {
        const double v = exp2((double)tid / 64.0);
        etab[tid] = FORM == 0 ? __hiloint2double(__double2hiint(v) - (tid << 14), __double2loint(v)) : v;
    }
    if (FORM == 2 && tid < 64) {
        const double cj = 1.0 + ((double)tid + 0.5) / 64.0;
        etab[64 + tid] = 1.0 / cj;
        etab[128 + tid] = log(cj);
    }
    __syncthreads();
}

// The node tile of a block and the columns it sweeps: all of them, or the tile's compact list (gml_i8_pack.hip: k_col_union; the
// image then has the tile's own step count in its strides).
struct FwdTile {
    int mytile, nk; // node tile; 64-column steps of its sweep
    const int8_t *xbase; // the bit image it reads
};
__device__ __forceinline__ FwdTile fwd_tile(const int *__restrict__ groups, int gi, int nk_all, const unsigned *__restrict__ Xb,
                                            const int *__restrict__ cnk, const int8_t *__restrict__ Xc, int64_t xc_tile) {
    FwdTile t{groups[gi], nk_all, reinterpret_cast<const int8_t *>(Xb)};
    if (cnk) {
        const int ck = cnk[t.mytile];
        if (ck >= 0) {
            t.nk = ck;
            t.xbase = Xc + (int64_t)t.mytile * xc_tile;
        }
    }
    return t;
}

// The bit words of a wave's two sample tiles from a step's image: lane (lr, h) needs dword h of its sample's 8 bytes of bits.
// B64: one ds_read_b64 per lane reads both dwords: the 32 lanes of a half-wave cover 256 contiguous bytes, one bank each
// (ds_read_b32 banks modulo 32 dwords: lanes lr and lr + 16 collide).
template <bool B64>
__device__ __forceinline__ void read_bits(const int8_t *cur, int wave, int lr, int h, unsigned (&vb)[WM]) {
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const int row = wave * 64 + i * 32 + lr;
        if (B64) {
            const uint2 v = *reinterpret_cast<const uint2 *>(cur + (row >> 7) * 1024 + (row & 127) * 8);
            vb[i] = h ? v.y : v.x;
        } else {
            vb[i] = *reinterpret_cast<const unsigned *>(cur + (row >> 7) * 1024 + (((row & 127) * 2 + h) << 2));
        }
    }
}
// ... expanded to the 0/1 bytes of the A fragments of half-step t (32 columns): the A operand never touches LDS as bytes
__device__ __forceinline__ void expand_bits(const unsigned (&vb)[WM], int t, v4i (&fa)[WM]) {
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) fa[i][e] = (int)((vb[i] >> (4 * t + e)) & 0x01010101u);
}

// Signed column pairs (gml_i8_pairs.h): the sparse A operand of v_smfmac_i32_32x32x64_i8 for a step, from the lane's bit dword.  Bits
// 2 m and 2 m + 1 are the two columns of pair m; byte m of the fragment is x of the first (+1 / -1 for bit 0 / 1) and its 2-bit slot
// index picks alpha (the bits agree) or beta (they differ) in the pair's half of a group of four slots: slots {0, 1} for even m,
// {2, 3} for odd m.  `sel`: the byte selector of v_perm (a VOP3 instruction takes no literal on gfx9: a loop hands it in as a scalar
// register it keeps, so that the constant costs no vector register).
__device__ __forceinline__ void pair_picks(const unsigned (&vb)[WM], v4i (&fa)[WM], int (&ix)[WM], unsigned sel = 0x0000ff01u) {
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        ix[i] = (int)(0x88888888u | ((vb[i] ^ (vb[i] >> 1)) & 0x55555555u));
#pragma unroll
        for (int e = 0; e < 4; ++e) { // bits 8 e + {0, 2, 4, 6} -> bytes 0..3 as byte selectors 0 / 1 -> bytes 0x01 / 0xff
            const unsigned m = __umul24((vb[i] >> (8 * e)) & 0x55u, 0x41041u) & 0x01010101u;
            fa[i][e] = (int)__builtin_amdgcn_perm(0u, sel, m);
        }
    }
}

// nk = 0: every row of Theta is zero (the caller says so): all sums are 0, nothing is loaded
template <int NPL>
__device__ __forceinline__ void clear_acc(v16i (&acc)[WM][NPL]) {
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int l = 0; l < NPL; ++l)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][l][e] = 0;
}

// One ring stage of GEMM work on NPL digit planes: two consecutive 64-column steps (one barrier per two steps: the waves of a
// workgroup re-align half as often, and the LDS reads of a stage's second step issue under the MFMAs of its first), the second
// only if `both` (an odd number of steps: the last stage is half full).  FIRST: the stage's first MFMAs take the constant 0 as
// their C operand (no clearing moves).  The caller has waited for the stage and issued the next DMA.
template <bool FIRST, int NPL>
__device__ __forceinline__ void gemm_stage2(const int8_t *stage, int step_bytes, bool both, int wave, int lr, int h, v16i (&acc)[WM][NPL]) {
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
        if (sub > 0 && !both) break;
        const int8_t *cur = stage + sub * step_bytes;
        unsigned vb[WM];
        read_bits<false>(cur, wave, lr, h, vb);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            v4i fa[WM], fb[NPL];
#pragma unroll
            for (int l = 0; l < NPL; ++l) fb[l] = *reinterpret_cast<const v4i *>(cur + 2048 + lds_off(l * 32 + lr, 2 * t + h));
            expand_bits(vb, t, fa);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int l = 0; l < NPL; ++l) {
                    if (FIRST && sub == 0 && t == 0) acc[i][l] = MFMA_I8(fa[i], fb[l], ((v16i){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}));
                    else acc[i][l] = MFMA_I8(fa[i], fb[l], acc[i][l]);
                }
        }
    }
}

// ---- epilogue: lane <-> node row (lr), register e <-> sample (e&3) + 8*(e>>2) + 4*h within the 32-sample tile ----

// the node's sign bits for the 32 samples of the wave's MFMA tile i, shifted so that bit 8g + j is this lane's sample 8g + 4h + j of
// the tile.  (One word per call: filling an array through a reference costs k_fwd_i8w, at 256 registers, three spilled ones.)
__device__ __forceinline__ unsigned sign_word(const unsigned *__restrict__ Sb, int rc, bool active, int64_t Kp, int64_t kw, int h, int i) {
    return active ? (Sb[(int64_t)rc * (Kp >> 5) + (kw >> 5) + i] >> (4 * h)) : 0u;
}
// Samples at or beyond Kreal are padding (they carry no weight).  lane_real(): the lane's element idx = 32 i + 8 g + j sits idx
// samples after its first one, kw + 4 h, and is real iff idx < lane_real(); wave_real(): real samples among the wave's 64.
__device__ __forceinline__ int lane_real(int64_t Kreal, int64_t kw, int h) {
    const int64_t left = Kreal - (kw + 4 * h);
    return left > 64 ? 64 : (left < 0 ? 0 : (int)left);
}
__device__ __forceinline__ int wave_real(int64_t Kreal, int64_t kw) { return (int)((Kreal - kw) < 64 ? (Kreal - kw) : 64); }

// One element of RPLE (:317): f = w log(1 + exp(-2E)), V = -2 w s / (1 + exp(2E)), E = s Ea (neg: s = -1).  Returns
// y = |V| / tau + dither, not yet rounded, and adds the objective term to fp.
__device__ __forceinline__ double rple_point(double Ea, bool neg, double wk0, double it, double dith, const double *__restrict__ etab, double &fp) {
    const double E2 = neg ? -2.0 * Ea : 2.0 * Ea;
    const double u = exp_tab(-fabs(E2), etab); // in (0, 1]
    const double opu = 1.0 + u;
    double rcp = __builtin_amdgcn_rcp(opu); // 1 / (1 + u), two Newton steps
    rcp = fma(fma(-opu, rcp, 1.0), rcp, rcp);
    rcp = fma(fma(-opu, rcp, 1.0), rcp, rcp);
    const double sig = E2 >= 0.0 ? u * rcp : rcp; // 1 / (1 + exp(2E))
    const double y = fma(2.0 * wk0 * it, sig, dith);
    // log(1 + u), 1 + u in (1, 2]: table of log c_j on 64 intervals + log1p of the residual
    int jt = (int)(u * 64.0);
    jt = jt > 63 ? 63 : jt;
    const double r1 = fma(opu, etab[64 + jt], -1.0); // |r1| <= 1/128
    double lp = fma(r1, 1.0 / 7.0, -1.0 / 6.0);
    lp = fma(lp, r1, 0.2);
    lp = fma(lp, r1, -0.25);
    lp = fma(lp, r1, 1.0 / 3.0);
    lp = fma(lp, r1, -0.5);
    lp = fma(lp, r1, 1.0);
    const double l1p = fma(lp, r1, etab[128 + jt]);
    fp += wk0 * ((E2 < 0.0 ? -E2 : 0.0) + l1p);
    return y;
}

// Byte transpose, 4 samples x planes: d[j] holds 4 balanced base-256 digits of sample j, one per byte; the result holds byte b
// of the four, sample j in byte j -- one dword of plane b of the Vq image, in which a lane's 16 samples of a tile are 16
// contiguous bytes per plane (no LDS transpose, 16-byte stores).  The same permutation takes 4 planes' dwords back to samples.
__device__ __forceinline__ unsigned bytes_of4(const unsigned (&d)[4], int b) {
    const unsigned sel = ((4u + b) << 8) | (unsigned)b;
    const unsigned t01 = __builtin_amdgcn_perm(d[1], d[0], sel);
    const unsigned t23 = __builtin_amdgcn_perm(d[3], d[2], sel);
    return __builtin_amdgcn_perm(t23, t01, 0x05040100u);
}
// NPL planes of 4 samples into dword `slot` of pl[0..NPL): the digits 0..3 from dl, 4.. from dh; csl[lb] += the sum of the 4
// digits (sum_k V then comes from dot4 over the packed planes).
template <int NPL>
__device__ __forceinline__ void planes_of4(const unsigned (&dl)[4], const unsigned (&dh)[4], v4i *pl, int slot, int *csl) {
#pragma unroll
    for (int lb = 0; lb < NPL; ++lb) {
        const unsigned pk = lb < 4 ? bytes_of4(dl, lb) : bytes_of4(dh, lb - 4);
        pl[lb][slot] = (int)pk;
        csl[lb] = __builtin_amdgcn_sdot4((int)pk, 0x01010101, csl[lb], false);
    }
}

// tail: a node row's samples are split over the two halves of a wave (h); lane lr of the lower half then holds the wave's value
template <class T>
__device__ __forceinline__ T half_sum(T v) { return v + static_cast<T>(__shfl_xor(v, 32)); }
template <class T>
__device__ __forceinline__ T half_max(T v) {
    const T o = static_cast<T>(__shfl_xor(v, 32));
    return o > v ? o : v;
}

// Launch dispatch: calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...) for the run-time values b0, b1, ...
template <class F>
void dispatch_bools(F &&f) { f(); }
template <class F, class... Rest>
void dispatch_bools(F &&f, bool b, Rest... rest) {
    if (b) dispatch_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else dispatch_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

} // namespace gml
