// FP64-grade fixed-point pass of the learn() hot path on the int8 matrix cores (gfx950, v_mfma_i32_32x32x32_i8): precision
// "i8w".  Same idea as the i8x pass (gml_i8.h) -- the statistics are +-1 (GraphicalModelLearning.jl:162, :107), so the two
// contractions of the objective/gradient pass (:196, :205-207) are exact integer GEMMs once the real operand is written in
// balanced base-256 digits -- carried to the width of the reference's Float64 arithmetic:
//   Theta[r][c] = sigma_r * q,  q an integer of 54 bits in 7 digit planes (sigma_r a power of two: the entries within a factor
//                 two of the row's largest are represented exactly, the others to 2^-55 of it -- the rounding a Float64
//                 accumulation of E = sum_c theta_c x_c commits on every term);
//   V[r][k]     = tau_r * v,    v an integer of 47 bits in 6 digit planes, rounded with a dither (f and the gradient then carry
//                 ~0.4 sqrt(K) 2^-47 of the largest weight: 1e-15 relative at K = 1e6, the order of Float64 summation error);
//   exp         in FP64 (Cody-Waite reduction, 2^(j/64) table, degree-5 polynomial: 1e-16 relative).
// Results are deterministic and independent of tiling, split-K order and GPU count, like those of the i8x pass.
//
// Register budget.  The full-width forward kernel multiplies all 7 planes in ONE sweep over the columns: 7 planes x 2 sample
// tiles x 16 accumulators = 224 registers, the 4 of one plane's Theta fragment (read plane by plane, fed to both sample tiles),
// the 8 of the bit fragments, a handful of offsets: at most 256 at two workgroups per CU.  A ring stage is one 64-column step
// (2 KB of bits + 14 KB of digit planes, 4 DMA instructions per wave), 4 stages deep; the sample bits are read and expanded once
// per step.  After the sweep the 7 accumulators of each element are folded into its energy, element by element.  Where the tile's
// image holds signed column pairs (gml_i8_pairs.h: the planes of q + q', q - q'; full-width objective passes) the step runs on the 2:4
// sparse MFMA, v_smfmac_i32_32x32x64_i8: one instruction per plane and sample tile covers the 64 columns, 14 per step instead of 28,
// the fragment 8 registers instead of 4.  Two such fragments rotate, read with pinned ds_read ahead of the MFMAs that use them, the
// step loop unrolled by the ring depth so that every LDS address is a loop-invariant register and an immediate (255 - 256
// registers, no spill: profiles/r19_fwd_pairs_resources.txt; -DI8W_PLAIN_PAIR_FRAGS builds the step with plain loads).  The coarse
// form sweeps only the top four planes (its own ring, two steps per stage).  -DI8W_TWO_SWEEPS builds the earlier form for A/B
// runs: sweep A multiplies the planes 3..6 (128 accumulators), folds them into 32 FP64 partial energies per lane (64
// registers), sweep B multiplies the planes 0..2 (96 accumulators), the sample bits loaded twice.  V is kept as two halves of 3
// planes, V / tau = lo + 2^24 hi: the backward GEMM runs as two launches of the 3-plane form of k_bwd_i8 and every integer sum
// (per half) stays far inside 64 bits.
//
// Build flags: -DI8W_TWO_SWEEPS (above; tests/test_gpu_i8w_single_sweep.py), -DI8W_PLAIN_PAIR_FRAGS (above) and -DABL_TIMING (s_memrealtime stamps per phase,
// read back through the V planes: scripts/gpu_fwd_timing.py).  Variants that were measured and no longer have a flag -- they live
// in git history: the two-sweep kernel without its V stores, without its exp arithmetic, without both, and with sweep B cut to one
// stage (forward 7.36 ms -> 6.48 / 6.83 / 6.11 / 5.63 ms: profiles/r4_ab_i8w_forward_ablation.txt); the epilogue's sign words and
// 1 / tau fetched ahead of the sweeps (not adopted: registers are what the sweeps are short of); V stored in whole 128-byte
// lines through LDS (0.8 % slower: profiles/r5_ab_i8w_line_stores.txt).
#include "gml_i8_fwd.h"
#include <string>

namespace gml {

namespace {

constexpr int LFA = 4, LFB = 3;          // digit planes of Theta per sweep
constexpr int BRT = 32 * LFW;            // rows of a Tq image
constexpr int PA = 2 + 2 * LFA, PB = 2 + 2 * LFB; // 1-KB pieces of a 64-column step: bits + digit-plane rows
constexpr int STEPW = PA * 1024, DSW = 2, STAGEW = DSW * STEPW, NSW = 3, RINGW = NSW * STAGEW;
constexpr int NLA = DSW * PA / 4, NLB = DSW * PB / 4; // DMA instructions per wave and stage: 5, 4
static_assert(NLA == NLB + 1, "issue() drops the last load in sweep B");
// the single sweep over all 7 planes: one 64-column step per stage, 16 pieces (2 of bits + 14 of digit-plane rows), 4 per wave
constexpr int P1 = 2 + 2 * LFW, STEP1 = P1 * 1024, NS1 = 4, RING1 = NS1 * STEP1, NL1 = P1 / 4;
static_assert(P1 % 4 == 0 && NL1 == 4, "one stage: 4 DMA instructions per wave");
#ifdef I8W_TWO_SWEEPS
constexpr bool ONE_SWEEP = false;
#else
constexpr bool ONE_SWEEP = true;
#endif
// the paired step of the single sweep: LDS reads pinned ahead of the MFMAs, or (-DI8W_PLAIN_PAIR_FRAGS: A/B runs, tests) plain loads
#ifdef I8W_PLAIN_PAIR_FRAGS
constexpr bool PAIR_FRAGS_AHEAD = false;
#else
constexpr bool PAIR_FRAGS_AHEAD = true;
#endif
// the forms that take the single sweep: the full-width ones, but RPLE beyond 32768 columns (its epilogue keeps 2 more registers
// through the fold, which spills them: it keeps the two sweeps)
constexpr bool one_sweep(int form, bool wide, bool coarse) { return ONE_SWEEP && !coarse && !(form == 2 && wide); }
// bytes of the LDS ring of a form (the exp / log tables follow it)
constexpr int ring_bytes(int form, bool wide, bool coarse) { return one_sweep(form, wide, coarse) ? RING1 : RINGW; }

__device__ __forceinline__ double flip_if(double v, int mneg /* 0 or -1 */) {
    return __hiloint2double(__double2hiint(v) + (mneg << 31), __double2loint(v));
}

// 6 balanced base-256 digits of the 48-bit two's complement integer held in the mantissa of yr = v + 1.5 * 2^52 (or the scaled
// form): (v + C) ^ C; dl = digits 0..3, the low half of dh = digits 4, 5
__device__ __forceinline__ void digits6(double yr, unsigned &dl, unsigned &dh) {
    unsigned long long v = ((unsigned long long)(unsigned)__double2hiint(yr) << 32) | (unsigned)__double2loint(yr);
    v += 0x0000808080808080ull;
    v ^= 0x0000808080808080ull;
    dl = (unsigned)v;
    dh = (unsigned)(v >> 32);
}

} // namespace

// ------------------------------------------------------------------------------------------
// forward: energies by two sweeps of C[k][m] = sum_c b[k][c] * Tq[m][c] (b = [x = -1] from the bit image), then the pointwise
// epilogue   E = s sigma (C0 - 2 sum_l 256^l C_l),  V = -w exp(-E) s  (RISE / logRISE),  -2 w s / (1 + exp(2E))  (RPLE),
// V -> 6 balanced digits -> the planes of the wave's Vq image.  Workgroup = 4 waves along the samples: 256 samples x one
// 32-node tile (block mapping: gml_i8_map.h; what the kernel shares with k_fwd_i8: gml_i8_fwd.h).
// ------------------------------------------------------------------------------------------
template <int FORM /* 0: exp forms (RISE, logRISE), 2: RPLE */, bool WANTF, bool WIDE /* more than 32768 statistics columns */, bool UNIW,
          bool COARSE /* sweep A only: Theta from its top four planes (30 bits), V in three planes (dithered 23 bits: planes 3..5, plane 2
                         zero) -- the cheap form of the pass for iterates far from the optimum (exp forms) */>
__global__ __launch_bounds__(256, 2) void k_fwd_i8w(
    const unsigned *__restrict__ Xb, const unsigned *__restrict__ Sb, const int8_t *__restrict__ Tq, const int *__restrict__ rowcol,
    const int *__restrict__ groups, int ngroups, const double *__restrict__ w, const double *__restrict__ sigma,
    const long long *__restrict__ qconst, const long long *__restrict__ qconst2, const long long *__restrict__ qpair, const double *__restrict__ invtau, int64_t Kp, int ntiles_k,
    int nk_all /* 64-column steps of a sweep over all columns (0: every row of Theta is zero) */,
    double wuni, int64_t Kreal, int8_t *__restrict__ Vq, long long *__restrict__ csum, long long *__restrict__ csum2,
    long long *__restrict__ asum, long long *__restrict__ asum2, double *__restrict__ fsum, unsigned *__restrict__ mmax,
    // column compaction (gml_i8_pack.hip: k_col_union): steps of each tile's compact image (-1: all columns), the images, bytes per tile,
    // and the steps between two tiles' Tq images (= Qfp / 64 whatever is swept)
    const int *__restrict__ cnk, const int8_t *__restrict__ Xc, int64_t xc_tile, int nk_tq,
    // signed column pairs (gml_i8_pairs.h): per node tile, 0 = the tile's Tq image holds the planes of (q + q', q - q') and the sweep runs on
    // the 2:4 sparse MFMA, else plain planes and the dense sweep (NULL: every tile plain).  Single-sweep forms only.
    const int *__restrict__ tdense) {
    extern __shared__ __attribute__((aligned(16))) int8_t lds[]; // ring, then the exp (and log) tables
    double *etab = reinterpret_cast<double *>(lds + ring_bytes(FORM, WIDE, COARSE));

    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63, lr = lane & 31, h = lane >> 5; // (the single sweep takes them afresh after its GEMM)
    fill_tables<FORM>(etab, tid);

    const FwdBlock blk = fwd_block(blockIdx.x, ntiles_k, ngroups);
    if (!blk.live) return;
    const int st = blk.st;
    const int64_t k0 = (int64_t)st * 256;
    if (k0 >= Kp) return;
    const FwdTile tile = fwd_tile(groups, blk.gi, nk_all, Xb, cnk, Xc, xc_tile);
    const int mytile = tile.mytile, nk = tile.nk;
    const int8_t *const xbase = tile.xbase;

    const int voffX = lane * 16;
    const int voffT = (lane >> 2) * 64 + (((lane & 3) ^ ((lane >> 4) & 3)) << 4);
    const int8_t *const gX = xbase + (int64_t)(2 * st) * nk * 1024;
    const int8_t *const gT = Tq + (int64_t)mytile * nk_tq * BRT * 64;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) int8_t *)lds;
    int r = mytile * 32 + lr;
    int rc = rowcol[r];
    bool active = rc >= 0;

#ifdef ABL_TIMING
    unsigned long long tst[6];
    tst[0] = __builtin_amdgcn_s_memrealtime();
#endif
    double us[WM][16]; // E / s of the lane's 32 elements (the two-sweep form keeps the partial sums of sweep A here first)
    if constexpr (one_sweep(FORM, WIDE, COARSE)) {
        // DMA plan: a ring stage is ONE 64-column step; its 16 1-KB pieces are dealt to the four waves, 4 each: piece pc = wave + 4 j,
        // pc < 2 the two 128-sample pieces of bits (so j = 0 only), else 16 of the 224 digit-plane rows (planes 0..6).  Source
        // swizzle and per-lane offsets as in the two-sweep form below.
        const int8_t *base1[NL1];
        int adv1[NL1];
#pragma unroll
        for (int j = 0; j < NL1; ++j) {
            const int pc = wave + 4 * j;
            base1[j] = pc < 2 ? gX + (int64_t)pc * nk * 1024 : gT + (pc - 2) * 16 * 64;
            adv1[j] = pc < 2 ? 1024 : BRT * 64;
        }
        const int voff0 = wave < 2 ? voffX : voffT;
        const bool pairs = tdense && tdense[mytile] == 0; // (uniform over the workgroup)
        // the stage of step 0: the unrolled paired sweep enters the ring where its last NS1 - 1 steps come to lie in the stages 0, 1, 2
        const int rot = pairs && PAIR_FRAGS_AHEAD && nk >= NS1 - 1 ? (NS1 - 1 - nk) & (NS1 - 1) : 0;
        auto issue1 = [&](int ks) {
            const unsigned stage_base = lds0 + ((ks + rot) % NS1) * STEP1;
#pragma unroll
            for (int j = 0; j < NL1; ++j) dma16(base1[j] + (int64_t)ks * adv1[j], j == 0 ? voff0 : voffT, stage_base + (wave + 4 * j) * 1024);
        };
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < NS1 - 1; ++s)
            if (s < nk) issue1(s);
        v16i acc[WM][LFW];
        // one step: 7 planes x 2 sample tiles x 2 half-steps = 28 MFMAs; plane-outer, tile-inner, so that one plane's fragment of
        // Theta (4 registers) is live at a time
        auto step = [&](int ks, auto first) {
            constexpr bool FIRST = decltype(first)::value;
            // the next two stages may stay in flight: their loads are the last ones this wave issued
            if (ks + 2 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NL1) : "memory");
            else if (ks + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NL1) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            if (ks + NS1 - 1 < nk) issue1(ks + NS1 - 1); // (into the stage every wave finished reading before the barrier)
            const int8_t *cur = lds + ((ks + rot) % NS1) * STEP1;
            unsigned vb[WM];
            read_bits<true>(cur, wave, lr, h, vb);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                v4i fa[WM];
                expand_bits(vb, t, fa);
#pragma unroll
                for (int l = 0; l < LFW; ++l) {
                    const v4i fb = *reinterpret_cast<const v4i *>(cur + 2048 + lds_off(l * 32 + lr, 2 * t + h));
#pragma unroll
                    for (int i = 0; i < WM; ++i) {
                        if (FIRST && t == 0) acc[i][l] = MFMA_I8(fa[i], fb, ((v16i){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}));
                        else acc[i][l] = MFMA_I8(fa[i], fb, acc[i][l]);
                    }
                }
            }
        };
        // the same step on signed column pairs: the picks (+-1 bytes and their slot indices) come from the same bit dwords, one
        // plane's fragment is the lane's 32 K-contiguous bytes of the row (two reads), one sparse MFMA per plane and sample tile
        // covers the whole 64-column step: 14 where the dense step issues 28.  The sparse MFMA accumulates in place: no FIRST form.
        // (This is the step written with plain loads, which -DI8W_PLAIN_PAIR_FRAGS builds: a read, a wait, two MFMAs, seven times.)
        auto step_pairs = [&](int ks) {
            if (ks + 2 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NL1) : "memory");
            else if (ks + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NL1) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            if (ks + NS1 - 1 < nk) issue1(ks + NS1 - 1);
            const int8_t *cur = lds + ((ks + rot) % NS1) * STEP1;
            unsigned vb[WM];
            read_bits<true>(cur, wave, lr, h, vb);
            v4i fa[WM];
            int ix[WM];
            pair_picks(vb, fa, ix);
#pragma unroll
            for (int l = 0; l < LFW; ++l) {
                const v4i f0 = *reinterpret_cast<const v4i *>(cur + 2048 + lds_off(l * 32 + lr, 2 * h));
                const v4i f1 = *reinterpret_cast<const v4i *>(cur + 2048 + lds_off(l * 32 + lr, 2 * h + 1));
                const v8i fb = {f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3]};
#pragma unroll
                for (int i = 0; i < WM; ++i) acc[i][l] = SMFMAC_I8(fa[i], fb, acc[i][l], ix[i]);
            }
        };
        if (nk > 0 && pairs && PAIR_FRAGS_AHEAD) {
            clear_acc(acc);
            // The paired step with its LDS reads kept ahead of its MFMAs (the idiom of k_bwd_i8: gml_i8.h, FRAG_READ).  Two fragments of
            // Theta rotate: the bit dwords and the fragments of the planes 0 and 1 are read straight behind the barrier, the picks run
            // under that round trip, and the read of plane l + 2 goes out right behind the two MFMAs of plane l; every use waits, with a
            // counted lgkmcnt, for its own fragment only (LDS reads return in order: at most the next plane's two reads are behind it).
            // A step's reads stay inside its own stage -- the next one is only known to have landed behind its own wait and barrier.
            // The step loop is unrolled by the ring depth, so the stage is an immediate offset of the reads (at most 3 STEP1 + 2048 +
            // 6 * 2048 + 16 bits) and the lane's addresses are three loop-invariant registers: the two halves of a row's 32 bytes
            // (slots 2 h and 2 h + 1 of lds_off(), which differ in bit 4), a plane + 2048 bytes, and the bits.  The four DMA
            // instructions of a step go out between the plane groups, off the front of the chain, in the same order and number, so
            // the counted vmcnt waits hold as before; their target stage was read in the previous step, which every wave has left
            // once this step's barrier has passed.
            const unsigned a0 = lds0 + (unsigned)lds_off(lr, 2 * h), a1 = lds0 + (unsigned)lds_off(lr, 2 * h + 1);
            const unsigned ab = lds0 + (unsigned)((wave >> 1) * 1024 + ((wave & 1) * 64 + lr) * 8); // (read_bits<true>: rows wave * 64 + lr, + 32)
            const unsigned ldsw = lds0 + wave * 1024;
            unsigned sel = 0x0000ff01u;
            asm("" : "+s"(sel));
            const unsigned long long hmask = __ballot(h != 0);
            // the sources of the next stage to issue
            const int npro = nk < NS1 - 1 ? nk : NS1 - 1;
            const int8_t *nxt[NL1];
#pragma unroll
            for (int j = 0; j < NL1; ++j) nxt[j] = base1[j] + (int64_t)npro * adv1[j];
            auto pstep = [&](auto stage, auto issues, int ahead /* stages behind this one still to come (!ISSUES) */) {
                constexpr int S = decltype(stage)::value, OFF = S * STEP1, DST = ((S + NS1 - 1) % NS1) * STEP1;
                constexpr bool ISSUES = decltype(issues)::value; // the step issues a stage, two more are in flight
                if constexpr (ISSUES) {
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NL1) : "memory");
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                } else {
                    ring_wait_ahead<NL1>(ahead);
                }
                v2u b0, b1;
                v4i fA0, fA1, fB0, fB1, fa[WM];
                int ix[WM];
                FRAG_READ64(b0, ab, OFF);
                FRAG_READ64(b1, ab, OFF + 256);
                FRAG_READ(fA0, a0, OFF + 2048);
                FRAG_READ(fA1, a1, OFF + 2048);
                FRAG_READ(fB0, a0, OFF + 2 * 2048);
                FRAG_READ(fB1, a1, OFF + 2 * 2048);
                __builtin_amdgcn_sched_barrier(0);
                FRAG_WAIT2(b0, b1, 4);
                // (lane (lr, h) takes dword h: selected by a mask the loop keeps in scalar registers, so that no lane coordinate stays live)
                unsigned vb[WM];
                asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(vb[0]) : "v"(b0.x), "v"(b0.y), "s"(hmask));
                asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(vb[1]) : "v"(b1.x), "v"(b1.y), "s"(hmask));
                pair_picks(vb, fa, ix, sel);
                __builtin_amdgcn_sched_barrier(0);
#define PAIR_DMA(j)                                                                                                         \
    if constexpr (ISSUES) {                                                                                                 \
        dma16(nxt[j], (j) == 0 ? voff0 : voffT, ldsw + DST + 4 * (j) * 1024);                                               \
        nxt[j] += adv1[j];                                                                                                  \
    }
#define PAIR_USE(l, f0, f1)                                                                                                 \
    {                                                                                                                       \
        FRAG_WAIT2(f0, f1, (l) + 1 < LFW ? 2 : 0);                                                                          \
        const v8i fb = {f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3]};                                            \
        _Pragma("unroll") for (int i = 0; i < WM; ++i) acc[i][l] = SMFMAC_I8(fa[i], fb, acc[i][l], ix[i]);                  \
        __builtin_amdgcn_sched_barrier(0);                                                                                  \
        if constexpr ((l) + 2 < LFW) {                                                                                      \
            FRAG_READ(f0, a0, OFF + ((l) + 3) * 2048);                                                                      \
            FRAG_READ(f1, a1, OFF + ((l) + 3) * 2048);                                                                      \
        }                                                                                                                   \
    }
                PAIR_USE(0, fA0, fA1)
                PAIR_USE(1, fB0, fB1)
                PAIR_DMA(0)
                PAIR_USE(2, fA0, fA1)
                PAIR_USE(3, fB0, fB1)
                PAIR_DMA(1)
                PAIR_USE(4, fA0, fA1)
                PAIR_DMA(2)
                PAIR_USE(5, fB0, fB1)
                PAIR_USE(6, fA0, fA1)
                PAIR_DMA(3)
#undef PAIR_USE
#undef PAIR_DMA
            };
            // The steps that issue a stage (all but the last NS1 - 1), a turn of the ring per trip of the loop, the odd ones in front;
            // then the last NS1 - 1 (fewer when nk is), which issue nothing and wait for less each time.  The ring is entered at stage
            // `rot`, so that these last steps always sit in the stages 0, 1, 2: ten bodies, each one basic block -- no fragment is in
            // flight across a branch.
            using std::integral_constant;
            using std::true_type;
            using std::false_type;
            const int nis = nk - npro, odd = nis % NS1; // (npro < NS1 - 1: nis = 0)
            if (odd >= 3) pstep(integral_constant<int, 1>{}, true_type{}, 0);
            if (odd >= 2) pstep(integral_constant<int, 2>{}, true_type{}, 0);
            if (odd >= 1) pstep(integral_constant<int, 3>{}, true_type{}, 0);
            for (int turn = nis / NS1; turn > 0; --turn) {
                pstep(integral_constant<int, 0>{}, true_type{}, 0);
                pstep(integral_constant<int, 1>{}, true_type{}, 0);
                pstep(integral_constant<int, 2>{}, true_type{}, 0);
                pstep(integral_constant<int, 3>{}, true_type{}, 0);
            }
            static_assert(NS1 == 4, "the last NS1 - 1 steps are written out");
            pstep(integral_constant<int, 0>{}, false_type{}, npro - 1);
            if (npro > 1) pstep(integral_constant<int, 1>{}, false_type{}, npro - 2);
            if (npro > 2) pstep(integral_constant<int, 2>{}, false_type{}, 0);
        } else if (nk > 0 && pairs) {
            clear_acc(acc);
            for (int ks = 0; ks < nk; ++ks) step_pairs(ks);
        } else if (nk > 0) { // Qfp >= 64
            step(0, std::true_type{});
            for (int ks = 1; ks < nk; ++ks) step(ks, std::false_type{});
        } else {
            clear_acc(acc);
        }
#ifdef ABL_TIMING
        tst[1] = tst[2] = __builtin_amdgcn_s_memrealtime();
#endif
        // the lane's coordinates, taken afresh from the lane id: kept alive through the sweep, they are the registers it lacks
        lane = __lane_id();
        lr = lane & 31;
        h = lane >> 5;
        r = mytile * 32 + lr;
        rc = rowcol[r];
        active = rc >= 0;
        // what the fold needs is fetched behind the sweep: registers are what the sweep is short of, and the co-resident
        // workgroup covers the wait.  C0 = sum_c q_c + q_const = c_lo + 2^24 c_hi, 0 <= c_lo < 2^24 (see the two-sweep form).
        const double sg = active ? sigma[r] : 0.0;
        const long long qc = active ? (pairs ? qpair[r] : qconst[r]) : 0;
        const double c_lo = (double)(unsigned)(qc & 0xffffffll), c_hi = (double)(qc >> 24);
        // (the paired sweep has summed x q = (1 - 2 b) q itself: its plane sums count once, with their sign, where the dense ones count
        // -2 times, and its constant is the constant column's integer alone, not C0 = that + sum_c q_c.  Either way the two products below
        // are exact -- an integer below 2^53 times a power of two -- and the last fma rounds sigma * (C0 - 2 sum b q) = sigma * (q_0 +
        // sum x q) once: the same double)
        const double ksum = pairs ? 1.0 : -2.0; // (wave-uniform)
        const double sgT = sg * 16777216.0, us0 = c_hi * sgT, m2sT = ksum * sgT;
        // E / s = sigma (c_lo - 2 a_lo) + sigma 2^24 (c_hi - 2 a_hi), a_lo = sum_{l<3} 256^l C_l, a_hi = sum_{l>=3} 256^(l-3) C_l:
        // the two-sweep form's operations in its order, so the energies are the same bits.  Element by element, pinned, so that
        // the 7 accumulators of an element die as its energy appears.
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                double ahi, alo;
                if (WIDE) {
                    ahi = (double)acc[i][6][e];
#pragma unroll
                    for (int l = 5; l >= 3; --l) ahi = fma(ahi, 256.0, (double)acc[i][l][e]);
                    alo = fma((double)acc[i][2][e], 256.0, (double)acc[i][1][e]);
                    alo = fma(alo, 256.0, (double)acc[i][0][e]);
                } else { // |acc_l| <= 128 Qfp <= 2^22: pairs in int32
                    const int p0 = acc[i][3][e] + (acc[i][4][e] << 8), p1 = acc[i][5][e] + (acc[i][6][e] << 8);
                    ahi = fma((double)p1, 65536.0, (double)p0);
                    alo = fma((double)acc[i][2][e], 65536.0, (double)(acc[i][0][e] + (acc[i][1][e] << 8)));
                }
                us[i][e] = fma(fma(alo, ksum, c_lo), sg, fma(ahi, m2sT, us0));
                asm volatile("" : "+v"(us[i][e]));
            }
        __builtin_amdgcn_sched_barrier(0);
    } else {
        // DMA plan: a ring stage holds DSW = 2 consecutive 64-column steps of ONE sweep; its 2 PA (2 PB) 1-KB pieces are dealt to the
        // four waves, 5 (4) each.  Piece pc of a step: pc < 2 the two 128-sample pieces of bits, else 16 rows of the sweep's digit
        // planes.  Addresses = a wave-uniform part (piece, step) + one of two per-lane offsets: the XOR swizzle of lds_off() is
        // applied to the SOURCE (the LDS side of the DMA is linear) and depends on the lane only (16-row pieces: (row >> 2) & 3 =
        // (lane >> 4) & 3).
        const int nst = (nk + DSW - 1) / DSW; // ring stages per sweep; global stage gs < nst: sweep A, else sweep B
        // per DMA instruction of this wave (wave-uniform, scalar registers): source of step 0, bytes per step, step within the
        // stage, destination within the stage
        const int8_t *baseA[NLA], *baseB[NLB];
        int advA[NLA], advB[NLB], subA[NLA], subB[NLB], dstA[NLA], dstB[NLB];
        bool bitsA[NLA], bitsB[NLB];
        auto plan = [&](int sp, int pps, int row0, const int8_t *&base, int &adv, int &sub, int &dst, bool &bits) {
            sub = sp / pps;
            const int pc = sp - sub * pps;
            dst = sub * STEPW + pc * 1024;
            bits = pc < 2;
            base = bits ? gX + (int64_t)pc * nk * 1024 : gT + (row0 + (pc - 2) * 16) * 64;
            adv = bits ? 1024 : BRT * 64;
        };
#pragma unroll
        for (int j = 0; j < NLA; ++j) plan(wave + 4 * j, PA, 32 * LFB, baseA[j], advA[j], subA[j], dstA[j], bitsA[j]); // planes 3..6
#pragma unroll
        for (int j = 0; j < NLB; ++j) plan(wave + 4 * j, PB, 0, baseB[j], advB[j], subB[j], dstB[j], bitsB[j]);        // planes 0..2
        auto issue = [&](int gs) {
            const unsigned stage_base = lds0 + (gs % NSW) * STAGEW;
            if (gs < nst) {
#pragma unroll
                for (int j = 0; j < NLA; ++j) {
                    int kt = DSW * gs + subA[j];
                    kt = kt < nk ? kt : nk - 1; // (a step beyond the last one: the last one again, so that every stage counts the same loads)
                    dma16(baseA[j] + (int64_t)(kt * advA[j]), bitsA[j] ? voffX : voffT, stage_base + dstA[j]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < NLB; ++j) {
                    int kt = DSW * (gs - nst) + subB[j];
                    kt = kt < nk ? kt : nk - 1;
                    dma16(baseB[j] + (int64_t)(kt * advB[j]), bitsB[j] ? voffX : voffT, stage_base + dstB[j]);
                }
            }
        };

        // what the fold between the sweeps needs is fetched now, so that the latency hides under the GEMM; the inputs of the pointwise
        // arithmetic (sign bits, 1 / tau) are fetched behind sweep B -- registers are what this kernel is short of, and the
        // co-resident workgroup covers the wait
        const double sg = active ? sigma[r] : 0.0;
        // C0 = sum_c q_c + q_const: the energy of the all-(+1) configuration / sigma.  C0 = c_lo + 2^24 c_hi with 0 <= c_lo < 2^24: both
        // halves, and everything combined with them below, are exact in FP64.  The coarse form has its own constant: the sum of the
        // numbers the top four planes spell (q / 2^24 rounded to nearest, entry by entry).
        const long long qc = active ? (COARSE ? qconst2[r] : qconst[r]) : 0;
        const double c_lo = COARSE ? 0.0 : (double)(unsigned)(qc & 0xffffffll), c_hi = COARSE ? (double)qc : (double)(qc >> 24);
        const double sgT = sg * 16777216.0, us0 = c_hi * sgT, m2sT = -2.0 * sgT;

        __builtin_amdgcn_s_setprio(1);
        const int ntot = COARSE ? nst : 2 * nst; // (the ring of a coarse pass ends with sweep A)
#pragma unroll
        for (int s = 0; s < NSW - 1; ++s)
            if (s < ntot) issue(s);
        // one ring stage of GEMM work on NPL digit planes
        auto gemm_stage = [&](int gs, int ks, auto first, auto &acc) {
            constexpr bool FIRST = decltype(first)::value;
            // the next stage may stay in flight: its loads are the last ones this wave issued
            if (gs + 1 < ntot) {
                if (gs + 1 < nst) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLA) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLB) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            if (gs + NSW - 1 < ntot) issue(gs + NSW - 1);
            gemm_stage2<FIRST>(lds + (gs % NSW) * STAGEW, STEPW, DSW * ks + 1 < nk, wave, lr, h, acc);
        };

        // ---- sweep A: digit planes 3..6, folded into us = sigma 2^24 (c_hi - 2 a_hi), a_hi = sum_{l>=3} 256^(l-3) C_l (exact: an integer
        // below 2^53 times a power of two)
        {
            v16i acc[WM][LFA];
            if (nk > 0) { // Qfp >= 64
                gemm_stage(0, 0, std::true_type{}, acc);
                for (int ks = 1; ks < nst; ++ks) gemm_stage(ks, ks, std::false_type{}, acc);
            } else {
                clear_acc(acc);
            }
#ifdef ABL_TIMING
            tst[1] = __builtin_amdgcn_s_memrealtime();
#endif
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    double ahi;
                    if (WIDE) {
                        ahi = (double)acc[i][3][e];
#pragma unroll
                        for (int l = 2; l >= 0; --l) ahi = fma(ahi, 256.0, (double)acc[i][l][e]);
                    } else { // |acc_l| <= 128 Qfp <= 2^22: pairs in int32
                        const int p0 = acc[i][0][e] + (acc[i][1][e] << 8), p1 = acc[i][2][e] + (acc[i][3][e] << 8);
                        ahi = fma((double)p1, 65536.0, (double)p0);
                    }
                    us[i][e] = fma(ahi, m2sT, us0);
                    // (pinned here: left alone, the compiler sinks the whole fold behind sweep B and keeps the 128 accumulators of
                    // sweep A alive under the 96 of sweep B)
                    asm volatile("" : "+v"(us[i][e]));
                }
        }
#ifdef ABL_TIMING
        tst[2] = __builtin_amdgcn_s_memrealtime();
#endif
        if constexpr (!COARSE) {
            // ---- sweep B: digit planes 0..2; E / s = sigma (c_lo - 2 a_lo) + us with ONE rounding (c_lo - 2 a_lo is an exact integer).
            // Done for all 32 elements of the lane at once: the 96 accumulators and the 64 registers of `us` become 64 registers of
            // energies before the pointwise arithmetic starts.
            v16i acc[WM][LFB];
            if (nk > 0) {
                gemm_stage(nst, 0, std::true_type{}, acc);
                for (int ks = 1; ks < nst; ++ks) gemm_stage(nst + ks, ks, std::false_type{}, acc);
            } else {
                clear_acc(acc);
            }
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    double alo;
                    if (WIDE) {
                        alo = fma((double)acc[i][2][e], 256.0, (double)acc[i][1][e]);
                        alo = fma(alo, 256.0, (double)acc[i][0][e]);
                    } else {
                        alo = fma((double)acc[i][2][e], 65536.0, (double)(acc[i][0][e] + (acc[i][1][e] << 8)));
                    }
                    us[i][e] = fma(fma(alo, -2.0, c_lo), sg, us[i][e]);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __builtin_amdgcn_s_setprio(0);
#ifdef ABL_TIMING
    tst[3] = __builtin_amdgcn_s_memrealtime();
#endif

    const int64_t kw = k0 + wave * 64; // first sample of this wave
    unsigned sgn[WM];
#pragma unroll
    for (int i = 0; i < WM; ++i) sgn[i] = sign_word(Sb, rc, active, Kp, kw, h, i);
    const double it = active ? invtau[r] : 0.0;
    const int nreal = lane_real(Kreal, kw, h);

    // ---- epilogue ----------------------------------------------------------------------------
    // lane <-> node row (lr), register e <-> sample (e&3) + 8*(e>>2) + 4*h within the 32-sample tile; the Vq image stores a
    // step's samples in the order vq_pos() (gml_bits.h): this lane's 16 samples of tile i are 16 contiguous bytes per plane.
    int8_t *vimg = Vq + vq_off(mytile * 32 + lr, 0, kw, Kp, LBW) + h * 32;
    // 2^32 w / tau; a coarse pass rounds V to multiples of 2^24 tau (the same dither, one step up)
    const double wscale = COARSE ? 256.0 : 4294967296.0; // 2^32 / 2^24
    const double wk32 = wscale * (wuni * it);
    const unsigned dh0 = dither_seed(rc, kw, h);
    const int wleft = wave_real(Kreal, kw); // wave-uniform
    int csl[LBW] = {0, 0, 0, 0, 0, 0};
    unsigned long long as64 = 0;
    int ymax_hi = 0; // high word of the largest 2^32 (|V| / tau + dither): non-negative doubles order like their bit patterns
    double fp = 0.0;

    // digits of 4 consecutive samples -> one dword per plane, and the plane sums
    auto pack4 = [&](const unsigned (&dl)[4], const unsigned (&dhh)[4], v4i (&pl)[LBW], int slot) {
        if (COARSE) { // the three digits of the 23-bit value go to the planes 3..5; plane 2 reads zero (the consumers of the top four)
            planes_of4<3>(dl, dl, pl + 3, slot, csl + 3);
            pl[2][slot] = 0;
        } else {
            planes_of4<LBW>(dl, dhh, pl, slot, csl);
        }
    };

    if constexpr (FORM == 0) {
        // Exp forms: the arithmetic is laid out in layers of 8 independent instructions (two 4-sample groups), fenced by
        // sched_barriers -- a wave in its epilogue then issues back to back instead of waiting out the latency of each dependent
        // FP64 instruction (the element-at-a-time form left the scheduler, at 200+ live registers, emitting each element's chain
        // serially).
#define SB __builtin_amdgcn_sched_barrier(0)
#pragma unroll
        for (int i = 0; i < WM; ++i) {
            const unsigned nsg = ~sgn[i]; // bit 8g + j set <=> s = +1
            v4i pl[LBW];
#pragma unroll
            for (int hg = 0; hg < 2; ++hg) {
                double Ea[8], tm[8], x[8], tj0[8], yy[8], pp[8], wk[8];
                int mneg[8], nn[8];
                // A: the energies, the sign bits, the weights
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int pos = 8 * (2 * hg + (q >> 2)) + (q & 3);
                    Ea[q] = us[i][8 * hg + q];
                    asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(mneg[q]) : "v"(nsg), "n"(pos)); // -1 iff s = +1
                    if (!UNIW) wk[q] = w[kw + i * 32 + 8 * (2 * hg + (q >> 2)) + 4 * h + (q & 3)];
                }
                SB;
                // B: x = -s E, n = rint(64 x / ln2), r = x - n ln2 / 64 (two-part constant)
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    x[q] = flip_if(Ea[q], mneg[q]);
                    tm[q] = fma(x[q], 92.33248261689366, MAGIC);
                }
                SB;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    nn[q] = __double2loint(tm[q]);
                    tm[q] = tm[q] - MAGIC;
                    tj0[q] = etab[nn[q] & 63];
                }
                SB;
#pragma unroll
                for (int q = 0; q < 8; ++q) x[q] = fma(tm[q], -0.01083042469326756, x[q]);
                SB;
#pragma unroll
                for (int q = 0; q < 8; ++q) x[q] = fma(tm[q], -2.9815858269852933e-12, x[q]);
                SB;
                // C: expm1(r) in FP64, |r| <= ln2/128: degree 5 leaves 4e-17
#pragma unroll
                for (int q = 0; q < 8; ++q) pp[q] = fma(x[q], 8.3333333333333332e-03, 4.1666666666666664e-02);
                SB;
#pragma unroll
                for (int q = 0; q < 8; ++q) pp[q] = fma(pp[q], x[q], 1.6666666666666666e-01);
                SB;
#pragma unroll
                for (int q = 0; q < 8; ++q) pp[q] = fma(pp[q], x[q], 0.5);
                SB;
#pragma unroll
                for (int q = 0; q < 8; ++q) pp[q] = fma(pp[q], x[q], 1.0);
                SB;
#pragma unroll
                for (int q = 0; q < 8; ++q) pp[q] = pp[q] * x[q];
                SB;
                // D: 2^32 (w / tau exp(-E) + dither)
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int idx = i * 32 + 8 * (2 * hg + (q >> 2)) + (q & 3);
                    tj0[q] = __hiloint2double((int)((unsigned)__double2hiint(tj0[q]) + ((unsigned)nn[q] << 14)), __double2loint(tj0[q]));
                    yy[q] = (double)(int)dither_hash(dh0, idx);
                }
                SB;
#pragma unroll
                for (int q = 0; q < 8; ++q) x[q] = fma(tj0[q], pp[q], tj0[q]); // exp(-E)
                SB;
#pragma unroll
                for (int q = 0; q < 8; ++q) yy[q] = fma(UNIW ? wk32 : wscale * (wk[q] * it), x[q], yy[q]);
                if (UNIW && wleft < 64) { // the last sample tile: padding samples carry no weight
                    asm volatile("; padding samples" ::: "memory");
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (i * 32 + 8 * (2 * hg + (q >> 2)) + (q & 3) >= nreal) yy[q] = 0.0;
                }
                SB;
                // E: sign, rounding to the 48-bit integer, 6 balanced digits, 4 samples x 6 planes byte transpose
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    ymax_hi = max(ymax_hi, __double2hiint(yy[q]));
                    if (WANTF) {
                        const double ya = yy[q] + MAGIC32; // |V| / tau >= 0 rounded: its integer sits in the low 48 bits
                        as64 += (((unsigned long long)((unsigned)__double2hiint(ya) & 0xffffu)) << 32) | (unsigned)__double2loint(ya);
                    }
                    x[q] = flip_if(yy[q], mneg[q]) + MAGIC32;
                }
                SB;
#undef SB
#pragma unroll
                for (int gg = 0; gg < 2; ++gg) {
                    unsigned dl[4], dhh[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) digits6(x[4 * gg + j], dl[j], dhh[j]);
                    pack4(dl, dhh, pl, 2 * hg + gg);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (active) {
                // (every lane stores its 16 bytes per plane and tile straight from registers: an instruction covers 32 rows x 16 B, a
                // quarter of each 64-byte row, and the write-combining of L2 puts the lines together -- WRITE_SIZE reads 8.8 GB per
                // launch for 6.1 GB of planes.  A variant that staged the wave's image through LDS and stored whole 128-byte lines
                // removed that inflation and was 0.8 % SLOWER: profiles/r5_ab_i8w_line_stores.txt -- the partial writes cost no time,
                // the LDS round trip does.  It lives in git history.)
#pragma unroll
                for (int lb = COARSE ? 2 : 0; lb < LBW; ++lb) *reinterpret_cast<v4i *>(vimg + lb * 32 * 64 + i * 16) = pl[lb];
            }
        }
    } else { // RPLE
#pragma unroll
        for (int i = 0; i < WM; ++i) {
            v4i pl[LBW];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int64_t kk = kw + i * 32 + 8 * g + 4 * h;
                unsigned dl[4], dhh[4];
                asm volatile("" : "+v"(fp)); // gate each 4-sample group on the previous one (register pressure)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double dith = dither_unit(dh0, i * 32 + 8 * g + j); // [-1/2, 1/2)
                    const bool neg = ((sgn[i] >> (8 * g + j)) & 1u) != 0; // s_u^k = -1
                    const double wk0 = UNIW ? (i * 32 + 8 * g + j < nreal ? wuni : 0.0) : w[kk + j];
                    const double y = rple_point(us[i][4 * g + j], neg, wk0, it, dith, etab, fp);
                    digits6((neg ? y : -y) + MAGIC, dl[j], dhh[j]);
                }
                pack4(dl, dhh, pl, g);
            }
            if (active) {
#pragma unroll
                for (int lb = 0; lb < LBW; ++lb) *reinterpret_cast<v4i *>(vimg + lb * 32 * 64 + i * 16) = pl[lb];
            }
        }
    }
#ifdef ABL_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    tst[4] = __builtin_amdgcn_s_memrealtime();
    if (lane == 0 && wave == 0 && active) { // 100 MHz ticks: start, end of sweep A, of the fold, of sweep B, of the epilogue (stores landed)
        unsigned long long *o = reinterpret_cast<unsigned long long *>(Vq + vq_off(mytile * 32, 0, k0, Kp, LBW));
        for (int q = 0; q < 5; ++q) o[q] = tst[q];
        o[5] = (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) /* HW_ID */;
    }
#endif
    // per-slot sums: sum_k V (two halves), sum_k |V| (objective-only passes), max_k |V| >> 16
    long long cs_lo = (long long)csl[0] + 256ll * csl[1] + 65536ll * csl[2];
    long long cs_hi = (long long)csl[3] + 256ll * csl[4] + 65536ll * csl[5];
    cs_lo = half_sum(cs_lo);
    cs_hi = half_sum(cs_hi);
    if (active && h == 0) {
        if (!COARSE) atomicAdd(reinterpret_cast<unsigned long long *>(&csum[r]), (unsigned long long)cs_lo);
        atomicAdd(reinterpret_cast<unsigned long long *>(&csum2[r]), (unsigned long long)cs_hi);
    }
    if (FORM == 0) {
        if (WANTF) {
            as64 = half_sum(as64);
            if (active && h == 0) {
                atomicAdd(reinterpret_cast<unsigned long long *>(&asum[r]), as64 & 0xffffffffull);
                atomicAdd(reinterpret_cast<unsigned long long *>(&asum2[r]), as64 >> 32);
            }
        }
        ymax_hi = half_max(ymax_hi);
        // the high word + 1 bounds 2^32 max(|V| / tau + dither) from above (to 2^-20 relative); in units of 2^16 tau
        const double ymax = __hiloint2double(ymax_hi + 1, 0);
        // (coarse: ymax bounds 2^32 (|V| / (2^24 tau) + dither), the dither down to -1/2 of that unit: |V| / (2^24 tau) < floor(ymax 2^-32)
        // + 3/2, reported in units of 2^16 tau as the next multiple of 2^24 tau above it.  Full width: |V| / tau < ymax 2^-32 + 1/2, so
        // mmax = floor((ymax 2^-32 + 1/2) / 2^16) -- the sum is exact in FP64 -- and (mmax + 1) 2^16 tau > |V| for every sample)
        const unsigned mxu = COARSE ? (((unsigned)fmin(ymax * 2.3283064365386963e-10 /* 2^-32 */, 8388605.0) + 2u) << 8)
                                    : (unsigned)fmin(fma(ymax, 3.5527136788005009e-15 /* 2^-48 */, 7.62939453125e-06 /* 2^-17 */), 4294967295.0);
        if (active && h == 0) atomicMax(&mmax[r], mxu);
    } else {
        // RPLE: f as an exact integer sum, so that its bits do not depend on the order in which the waves' parts arrive.  The part fp
        // goes in two words -- rint(fp 2^32) into asum2, the remainder (at most 2^-33) in units of 2^-72 into asum; this form uses
        // neither otherwise -- which holds up to 2^23 parts of a row; k_finalize_i8w puts the two together.  A part that is not
        // finite or not below 2^30 keeps the FP64 atomic, so that f still says what happened.
        fp = half_sum(fp);
        if (active && h == 0) {
            if (fabs(fp) < 0x1p30) {
                const long long hi = __double2ll_rn(fp * 0x1p32);
                const long long lo = __double2ll_rn(fma(-(double)hi, 0x1p-32, fp) * 0x1p72);
                atomicAdd(reinterpret_cast<unsigned long long *>(&asum2[r]), (unsigned long long)hi);
                atomicAdd(reinterpret_cast<unsigned long long *>(&asum[r]), (unsigned long long)lo);
            } else {
                unsafeAtomicAdd(&fsum[r], fp);
            }
        }
    }
}

// G[row][c] = tau_r (C_lo - 2 S_lo + 2^24 (C_hi - 2 S_hi)),  S_half = sum_l 256^l Gacc_l over the half's three planes (x = 1 - 2b),
// C_half = sum_k of the half's digits; G[row][cconst] = tau_r (C_lo + 2^24 C_hi).  f: RISE / logRISE from the gradient's own
// column (with the gradient) or from sum |V| (objective-only passes); RPLE from the forward kernel's two-word integer sum.
__global__ __launch_bounds__(256) void k_finalize_i8w(const int32_t *__restrict__ Gacc, const double *__restrict__ tau,
                                                      const long long *__restrict__ csum, const long long *__restrict__ csum2,
                                                      const long long *__restrict__ asum, const long long *__restrict__ asum2,
                                                      const int *__restrict__ srow, const int *__restrict__ rowcol, int slot0, int64_t Qp,
                                                      int64_t Qfp, int64_t Qf, int64_t cconst, int form, int want_grad,
                                                      double *__restrict__ G, double *__restrict__ f, int nplanes, int64_t plane_stride,
                                                      const unsigned *__restrict__ mmax, SlotResult *__restrict__ res,
                                                      int coarse /* only the high half carries the values: multiples of 2^24 tau */) {
    const int r = slot0 + blockIdx.y;
    if (rowcol[r] < 0) return;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const double t = tau[r];
    const int tile = r >> 5, rl = r & 31;
    auto gcol = [&](int64_t col) -> double {
        long long s[2] = {0, 0};
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (coarse && half == 0) continue;
#pragma unroll
            for (int l = 2; l >= 0; --l) {
                long long a = 0;
                for (int pl = 0; pl < nplanes; ++pl) a += (long long)Gacc[pl * plane_stride + ((int64_t)(tile * LBW + 3 * half + l) * 32 + rl) * Qfp + col];
                s[half] = s[half] * 256 + a;
            }
        }
        return fma((double)(csum2[r] - 2 * s[1]), 16777216.0, coarse ? 0.0 : (double)(csum[r] - 2 * s[0]));
    };
    if (c == 0) {
        double fv = f ? f[r] : 0.0;
        if (form != 2) {
            if (want_grad) fv = -t * gcol(rowcol[r]); // f = sum_k w exp(-E) = -sum_k V_k s_k = -G[r][u]
            else fv = t * (coarse ? 16777216.0 : 1.0) * fma((double)asum2[r], 4294967296.0, (double)asum[r]);
            f[r] = fv;
        } else if (f) { // RPLE: the forward kernel's exact two-word sum (f[r] itself holds only parts that did not fit: normally 0)
            fv += fma((double)asum[r], 0x1p-72, (double)asum2[r] * 0x1p-32);
            f[r] = fv;
        }
        if (res) res[r] = SlotResult{fv, t, mmax[r], 0u};
    }
    if (!want_grad || c >= Qp) return;
    double v = 0.0;
    if (c < Qf) v = t * gcol(c);
    else if (c == cconst) v = t * fma((double)csum2[r], 16777216.0, coarse ? 0.0 : (double)csum[r]);
    G[(int64_t)srow[r] * Qp + c] = v;
}

void launch_finalize_i8w(const int32_t *Gacc, const SlotScalars &sc, const int *srow, const int *rowcol, int slot0, int ns, int64_t Qp,
                         int64_t Qfp, int64_t Qf, int64_t cconst, int form, int want_grad, double *G, double *f, int nplanes,
                         int64_t plane_stride, SlotResult *res, bool coarse, hipStream_t st) {
    i8_note_instance(306 + (coarse ? 1 : 0));
    hipLaunchKernelGGL(k_finalize_i8w, dim3((unsigned)((Qp + 255) / 256), (unsigned)ns), dim3(256), 0, st, Gacc, sc.tau, sc.csum, sc.csum2,
                       sc.asum, sc.asum2, srow, rowcol, slot0, Qp, Qfp, Qf, cconst, form, want_grad, G, f, nplanes, plane_stride, sc.mmax, res,
                       coarse ? 1 : 0);
}

template <int FORM, bool WANTF, bool WIDE, bool UNIW, bool COARSE>
static void launch_one(const FwdWArgs &a) {
    constexpr int shmem = ring_bytes(FORM, WIDE, COARSE) + 512 + 1024; // ring + exp, log tables
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_fwd_i8w<FORM, WANTF, WIDE, UNIW, COARSE>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, shmem); // per device: set on every launch
    i8_note_instance(256 + (FORM == 2) * 16 + WANTF * 8 + WIDE * 4 + UNIW * 2 + COARSE);
    const DevProblem &d = *a.d;
    const int ntk = (int)(d.Kp / 256);
    hipLaunchKernelGGL((k_fwd_i8w<FORM, WANTF, WIDE, UNIW, COARSE>), dim3(fwd_grid(ntk, a.ngroups)), dim3(256), shmem, a.st, d.Xb, d.Sb, a.Tq, a.rowcol, a.groups,
                       a.ngroups, d.w, a.sc->sigma, a.sc->qconst, a.sc->qconst2, a.sc->qpair, a.sc->invtau, d.Kp, ntk, a.zero_theta ? 0 : (int)(d.Qfp / 64), d.wuni, d.K, a.Vq,
                       a.sc->csum, a.sc->csum2, a.sc->asum, a.sc->asum2, a.F, a.sc->mmax, a.cc ? a.cc->cnk : nullptr, a.cc ? a.cc->Xc : nullptr,
                       a.cc ? a.cc->xc_tile : 0, (int)(d.Qfp / 64), one_sweep(FORM, WIDE, COARSE) ? a.tdense : nullptr);
}

// COARSE only for the exp forms (for RPLE a.coarse selects nothing)
template <int FORM, bool WANTF>
static void launch_fwd_w2(const FwdWArgs &a) {
    dispatch_bools([&](auto wide, auto uniw, auto coarse) {
        launch_one<FORM, WANTF, decltype(wide)::value, decltype(uniw)::value, decltype(coarse)::value && FORM == 0>(a);
    }, a.d->Qfp > 32768, a.d->wuni > 0.0, a.coarse);
}

bool fwd_i8w_one_sweep(int form, int64_t Qfp, bool coarse) { return one_sweep(form == GML_RPLE ? 2 : 0, Qfp > 32768, coarse && form != GML_RPLE); }

void launch_fwd_i8w(const FwdWArgs &a) {
    if (a.form == 2) launch_fwd_w2<2, true>(a);
    else if (a.want_f) launch_fwd_w2<0, true>(a);
    else launch_fwd_w2<0, false>(a);
}

} // namespace gml
