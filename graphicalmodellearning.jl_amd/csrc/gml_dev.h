// Internal device-side interface of libgml_hip (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "gml_bits.h"

namespace gml {

// Device memory of the library (gml_alloc.cpp): freed blocks of >= 1 MB are kept per device and size for the next handle of
// the same shape (a hipMalloc of a multi-GB block after a hipFree sporadically takes a second).
hipError_t dev_malloc_bytes(void **out, size_t bytes);
hipError_t dev_free(void *p);        // synchronises the block's device before the block can be handed out again (as hipFree does)
hipError_t dev_free_synced(void *p); // the caller has synchronised the device (or every stream that touched the block) itself
hipError_t dev_mem_info(size_t *free_bytes, size_t *total_bytes); // free = the driver's + the cache's
size_t dev_trim_cache();
template <typename T> inline hipError_t dev_malloc(T **out, size_t bytes) { return dev_malloc_bytes(reinterpret_cast<void **>(out), bytes); }

// Device-resident problem data (all padded, padding is zero).  The samples are stored as ONE BIT per entry:
//   Sb  [n][Kp/32]     sign bits of the spins, spin-major, natural order (bit j of word w <-> sample 32w + j; set <=> -1)
//   Xb                 forward operand of the int8 path: the design matrix sample-major, in the piece layout of
//                      k_build_xb (gml_i8_pack.hip)
//   Xtb                backward operand: the same matrix feature-major, piece layout of k_build_xtb
//   keys [Qf][ko]      spins of every statistic column (-1 = unused slot): column c = prod of its spins = XOR of sign bits
//   w   [Kp]     f64   c_k / M   (samples[k,1]/num_samples, GraphicalModelLearning.jl:170)
//   Xt [Qp][Kp] int8   feature-major byte image, built on first use by the FP64 path only (rows gathered by its Hessian kernel)
// Columns 0..n-1 are the single spins, then pairs (i<j) in lexicographic order, ... (multi-body, :94-108); column
// `cconst` is the empty key (constant 1: the node's field).  Column Qp-1 is always a zero (padding) column.
struct DevProblem {
    int64_t K, Kp, n;
    int64_t Qf, Qfp;  // statistic columns [0,Qf), zero padded to Qfp (multiple of 64)
    int64_t cconst;   // column of the constant statistic (= Qfp)
    int64_t Qp;       // row pitch of the parameter arrays / number of rows of Xt (= Qfp + 64)
    unsigned *Sb;
    unsigned *Xb, *Xtb;
    int32_t *keys;
    int ko;
    int8_t *Xt;
    double *w;
    double wmax;      // max_k w_k
    double wuni;      // the common weight when all K samples weigh the same (counts all equal), else 0
};

// ---- packing -----------------------------------------------------------------------------
void launch_transpose_i8(const int8_t *src, int64_t rows, int64_t cols, int64_t ld_src,
                         int8_t *dst, int64_t ld_dst, hipStream_t st);
// Sb from +-1 bytes: sample-major S [K][n] (ld ignored) or spin-major S [n][ld]
void launch_spin_bits(const int8_t *S, bool spin_major, int64_t K, int64_t n, int64_t ld, int64_t Kp, unsigned *Sb, hipStream_t st);
void launch_pack_bits(const DevProblem &d, hipStream_t st);      // Sb, keys -> Xb, Xtb
void launch_unpack_spins(const DevProblem &d, int64_t k0, int64_t kk, int8_t *out /* [kk][n] */, hipStream_t st);
void launch_expand_xt(const DevProblem &d, int8_t *Xt, hipStream_t st); // Sb, keys -> rows [0, Qf) of the byte image
// *bad = smallest configuration index holding an entry that is not +-1 (unchanged if there is none; init -1)
// Histogram matrix (K x (1+n), element type `dtype` of gml.h, leading dimension ld) -> counts [K] and +-1 int8 spins:
// column-major input gives spin-major output [n][K], row-major input sample-major [K][n].  *bad as in launch_check_pm1.
void launch_convert_hist(const void *H, int dtype, int64_t K, int64_t n, int64_t ld, int col_major, double *counts, int8_t *spins,
                         long long *bad, hipStream_t st);
void launch_check_pm1(const int8_t *S, int64_t K, int64_t n, long long *bad, hipStream_t st);
int64_t xtb_bytes(const DevProblem &d);
// device-pointer operator calls (gml_oplayout.hip): the caller's rows in the reference's parameter order <-> the internal columns
void launch_ref_to_internal(const double *theta, int64_t ld, int64_t R, int64_t P, int64_t Qp, const int *rowcol, int64_t cconst,
                            const int32_t *cols, double *X, int *bad, hipStream_t st);
void launch_internal_to_ref(const double *G, const double *F, int64_t R, int64_t Qp, int64_t P, int64_t ld, const int *rowcol, const uint8_t *sel,
                            int64_t cconst, const int32_t *cols, int logz, double *f, double *g, hipStream_t st);
void launch_hv_to_ref(const double *Hv, const double *Gz, const double *F, int64_t R, int64_t Qp, int64_t P, int64_t ld, const int *rowcol,
                      int64_t cconst, const int32_t *cols, int logz, const double *vec, double *hv, hipStream_t st);

// Byte offset of limb l of V[r][k] in the int8 limb image Vq of the fixed-point pass: images [node tile r/32][k/64]
// of [lbt limbs x 32 rows][64 B], contiguous (lbt = 4: 8 KB each, the i8x pass; 6: 12 KB, the i8w pass); within a row the
// 64 samples of the step are stored in the order vq_pos() (gml_bits.h), which the feature-major bit image shares, so the
// backward GEMM contracts position against position.
__host__ __device__ inline int64_t vq_off(int64_t r, int l, int64_t k, int64_t Kp, int lbt = 4) {
    return ((((r >> 5) * (Kp >> 6) + (k >> 6)) * lbt + l) * 32 + (r & 31)) * 64 + vq_pos((int)(k & 63));
}

// ---- int8-limb path --------------------------------------------------------------------------
// One pass of the fixed-point operator (gml_i8_pass.hip).  The rows to evaluate are listed in consecutive SLOTS
// (32 slots = one MFMA node tile; slot0, slot1 multiples of 32), so the tiles that run are full whatever subset of the
// caller's rows is active; all per-slot arrays (and the limb planes of V the Hessians are built from) live in the
// workspace, indexed by slot.
struct SlotResult { // per-slot scalars of a pass, packed for one download
    double f, tau;      // f per slot (RISE f, logRISE Z, RPLE f); scale of the V planes
    unsigned mmax, pad; // largest |V| / tau seen (dynamic-range check)
};
struct I8Pass {
    const double *theta;  // device, [rows][Qp]: the parameter rows (internal column layout, masked slots zero)
    const int *srow;      // device [slots]: slot -> row of theta / G (unused slots: anything)
    const int *rowcol;    // device [slots]: slot -> node u (whose sign row is the node's spin), -1 = unused slot
    const int *groups;    // device: the slot tiles to run (slot / 32), padded with -1 to a multiple of 4
    int ngroups;          // tiles listed (without the padding)
    int slot0, slot1;     // slot range the listed tiles lie in: its accumulators are zeroed, its rows quantised and finalised
    int form;             // GML_RISE / GML_LOGRISE (Z) / GML_RPLE
    bool want_grad;       // false: objective only (no backward GEMM)
    double *F;            // device [slots]: f per slot (RISE f, logRISE Z, RPLE f)
    double *G;            // device, [rows][Qp]: gradient rows (row srow[slot]); may be NULL when !want_grad
    const double *tauovr; // device [slots] or NULL: per-slot scale of V imposed by the caller (0 = from the bound)
    bool zero_theta;      // the caller guarantees that every listed row of theta is zero (a solve's first pass at x = 0): all energies are 0
                          // and the forward kernel skips its sweeps over the columns -- the same bits, without the GEMM
    const double *tauovr_lnrow; // device [rows of theta] or NULL: tauovr[slot] is multiplied by exp(tauovr_lnrow[srow[slot]]) (a trial
                          //    point's distance from the iterate the scale was measured at, left on the device by the kernel that formed it)
    int hv;               // 1: Hessian-vector product -- theta rows are directions p, G receives sum_k h_k (x_k.p) x_k with the
                          //    curvature weights h_k of the objective pass that last ran in slot vmap[slot]
                          //    2: the same with the products h_k (x_k.p) carried in 2 backward limbs (15 bits) instead of 4
    const int *vmap;      // hv: device [slots]
    int ksub;             // hv: the products run over ~1/ksub of the configurations (i8_split_plan); 0, 1 = all of them
    int64_t kchunk, kpart; // hv: a split plan fixed by the caller (one operator for all the steps of a CG solve); 0 = plan here
    int64_t *plan_out;    // host [2] or NULL: receives the kchunk, kpart the pass ran with
    SlotResult *res;      // device [slots] or NULL: {f, tau, mmax} of every slot of the pass, written by its last kernel
    int lf;               // forward limb planes (3, 4, 5; 0 = the default, 5; 2 for Hessian-vector directions): 8 lf - 2 significant bits of theta
    bool wide;            // the FP64-grade pass (precision i8w): theta in 7 limb planes (54 bits), V in 6 (47 bits), FP64 exp;
                          // the workspace then holds 6-plane V images, of which Hessians and Hessian-vector passes read the top 4
    bool compact;         // objective passes: the forward GEMM of a node tile sweeps only the columns on which one of the tile's rows is
                          // non-zero (l1-sparse iterates: a few dozen of thousands of columns) -- the compact column list and the bit
                          // image of those columns are built on the device in front of the pass; the integer sums, hence every result
                          // bit, are those of the sweep over all columns.  Tiles whose union exceeds a quarter of the columns run dense
    bool coarse;          // the cheap form of an objective pass (exp forms) for iterates far from the optimum.  wide: the top four
                          // planes of theta (30 bits), V in three planes (dithered 23 bits): one forward sweep and one backward launch
                          // instead of two; SlotResult.tau stays the unit of the 47-bit planes, the values are multiples of 2^24 tau.
                          // i8x: theta in 4 limb planes (30 bits), V in the planes 1..3 (23 bits, multiples of 2^8 tau), a 3-plane
                          // backward launch
};
void i8_split_plan(const DevProblem &d, int ngroups, int ksub, int64_t *kchunk, int64_t *kpart, int *nsplit);
int i8_pass(void **ws, const DevProblem &d, int64_t slot_capacity, const I8Pass &a, hipStream_t st, hipEvent_t *ev /* [3] or NULL */,
            std::string *err);
// Unit of SlotResult.mmax in multiples of SlotResult.tau, and the largest |V| / tau the planes hold, for a pass of the given width:
// (mmax + 1) * i8_mmax_unit * tau bounds max_k |V_k|; a caller-imposed scale is bound / i8_vdiv.
inline double i8_mmax_unit(bool wide) { return wide ? 65536.0 : 1.0; }
inline double i8_vdiv(bool wide) { return wide ? 1.400e14 : 2130000000.0; }
// unit of the values of a coarse pass, in multiples of SlotResult.tau (the noise of f and grad scales with it)
inline double i8_coarse_unit(bool wide) { return wide ? 16777216.0 : 256.0; }
void i8_free(void *ws);
void i8_compact_table(void *ws, const int **cnk, int *csteps);
// per-slot results of the last pass of the given kind (device pointers)
void i8_slot_results(void *ws, int hv, const double **tau, const unsigned **mmax);
// the limb planes of V of the workspace (device pointer, bytes): the kernel-timing experiments read per-workgroup timestamps from it
void i8_vq_buffer(void *ws, const int8_t **vq, int64_t *bytes, const DevProblem &d);
// Hessian-vector products of a few matrix-free rows over their working sets only, bit-identical to an i8_pass with hv = 2 and two
// forward limbs (gml_hv_sparse.hip).  rows / node / vslot [nrows]: local row, its spin, the slot of its V planes; nw, t0 (indexed by
// local row): size and first tile of the row's list of working-set columns in FV (tiles of T entries); wcap >= every listed nw,
// <= 65536; buf: i8_hv_sparse_bytes(d, nrows, wcap) bytes of device scratch.  Exp forms (RISE, logRISE), statistics of <= 2 spins.
size_t i8_hv_sparse_bytes(const DevProblem &d, int nrows, int64_t wcap);
int i8_hv_sparse(void *ws, const DevProblem &d, int nrows, const int *rows, const int *node, const int *vslot, const long long *t0, const int *nw,
                 const int *FV, int T, int64_t wcap, const double *P, double *Hout, int64_t kchunk, int64_t kpart, void *buf, hipStream_t st,
                 std::string *err);
// Extra blocks of a Hessian call: the preconditioner tiles of the matrix-free rows.  Block R + t (t < n) is the T x T Hessian of
// the T columns F[t T ..] under the weights of row wrow[t]; the caller's mt / hoff arrays cover R + n blocks (mt = T / 32 for a
// tile).  hflag [R]: rows whose weights are needed (those with a working set, and those with tiles).
struct HessTiles {
    int64_t n = 0;
    int T = 0;
    const int *F = nullptr, *wrow = nullptr, *hflag = nullptr;
};
int i8_hessian(void *ws, const DevProblem &d, const int *dRowcol, const int *dVslot, const int *dF, const int *dMt, const int *hMt,
               const long long *dHoff, int64_t htotal, int R, int cap, int form, int64_t Kh, int64_t kstride, double *dH,
               hipStream_t st, std::string *err, const HessTiles *tiles = nullptr);

// ---- FP64 path -----------------------------------------------------------------------------
// Theta [Rp][Qp] (internal column layout, masked slots zero), rowcol[r] = u (row of Xt
// holding node u's sign) or -1 for padding rows.  Rp multiple of 32.
// V [Rp][Kp]: V[r][k] = d f_r / d E_rk * s_rk = -w_k exp(-E) s (RISE: `partial_obj` of :204 times s)
// fsum [Rp]: sum_k w_k phi(E_rk)  (must be zeroed by the caller)
// ws: f64_reduce_ws_bytes(P, rows) bytes for launches of up to `rows` rows -- where the workgroups leave their parts of f and G, which a
// second kernel adds in a fixed order: the same bits on every call
// groups: ids of the 32-row groups to evaluate (padded with -1 to a multiple of 4).
void launch_fwd_f64(const DevProblem &P, const double *Theta, const int *rowcol, const int *groups,
                    int ngroups4, int form, double *V, double *fsum, double *ws, hipStream_t st);
size_t f64_reduce_ws_bytes(const DevProblem &P, int64_t rows);
// G [Rp][Qp] += sum_k V[r][k] * Xt[c][k] = the gradient (:205-207); must be zeroed by the caller
void launch_bwd_f64(const DevProblem &P, const double *V, const int *groups, int ngroups, double *G, double *ws,
                    hipStream_t st);
// H [Rp][cap][cap] += sum_k h_rk Xt[F_ri][k] Xt[F_rj][k], lower-triangular 32x32 tiles only.
// F [Rp][cap] column ids (padding = Qp-1), mt[r] = number of 32-tiles used by row r.
void launch_hess_f64(const DevProblem &P, const double *V,
                     const int *rowcol, const int *F, const int *mt, const long long *hoff, int R, int cap, int form,
                     int64_t Kh, int64_t kstride, double *H, hipStream_t st);
// H is ragged: row r's block starts at hoff[r] and is (32 mt[r]) x (32 mt[r]) with that pitch.
// Kh (multiple of 512, <= Kp), kstride: the Hessian is accumulated over Kh configurations, every kstride-th block
// of 512 (sub-sampled Newton: the gradient stays exact, so only the convergence rate is affected).

// Exact sampling of one block (connected component) of a model given as terms (bit masks over the block's
// spins + weights): energies of its 2^sb states, CDF, N draws written into S [N][n] (sample-major, +-1) at
// the block's spin columns.
void launch_block_sampler(const unsigned *dmasks, const double *dwts, int nt, int sb, const int *dmembers, int64_t N, int64_t n,
                          unsigned long long seed, int block, double *den, double *dcdf, int8_t *dS, hipStream_t st);

// Histogramming on the device (gml_dedupe.hip): distinct configurations of N samples held as +-1 bytes (n <= 64, N < 2^31) as
// ascending 64-bit keys (bit i set <=> spin i is -1) with their multiplicities; both arrays are device memory owned by the caller.
int dedupe_samples(const int8_t *dS, bool spin_major, int64_t ld, int64_t N, int64_t n, hipStream_t st, unsigned long long **dkeys_out,
                   int **dcounts_out, int64_t *K_out, std::string *err);
void launch_bits_from_keys(const unsigned long long *dkeys, int64_t K, int64_t n, int64_t Kp, unsigned *Sb, hipStream_t st);

// Row compaction of the sign bits (gml_split.hip): Sb_out [n][Kp_out / 32] row k' = row src[k'] of Sb [n][Kp_src / 32] for k' < Kout; Sb_out
// zeroed by the caller (rows >= Kout stay 0), Kp_out a multiple of 1024.
void launch_gather_bits(const unsigned *Sb, int64_t Kp_src, const int *src, int64_t Kout, int64_t n, int64_t Kp_out, unsigned *Sb_out,
                        hipStream_t st);

// Exact sample moments from the sign bits (gml_moments.hip): XOR of sign rows + population counts, integer sums throughout.
// planes [nplanes][Kp / 32]: bit b of every count c_k = rint(w_k M), packed like a sign row (launch_count_planes); nplanes = 0:
// all counts equal (the common count is applied by the caller / the finishing kernel).
void launch_count_planes(const DevProblem &d, double M, int nplanes, unsigned *planes, hipStream_t st);
// S2 [n][n] (zeroed by the caller) -> sum2 = M - 2 c N, N_ij = sum_k c_k [s_ki != s_kj] (c = 1 with planes)
void launch_moments_pairs(const DevProblem &d, const unsigned *planes, int nplanes, long long M, long long c, long long *S2, hipStream_t st);
// Nt [nterms] (zeroed by the caller) += sum_k c_k [prod of the key's spins at k is -1] (nplanes = 0: every c_k taken as 1).
// keys [nterms][L]: distinct spins of every key, -1 = unused slot
void launch_moments_terms(const DevProblem &d, const int32_t *keys, int L, int64_t nterms, const unsigned *planes, int nplanes,
                          unsigned long long *Nt, hipStream_t st);

// Glauber dynamics (N independent chains, `sweeps` sweeps) on incidence lists; St [n][Np] spin-major.
void launch_glauber(const int *dioff, const double *diw, const int *dooff, const int *doth, int64_t n, int64_t N, int64_t Np,
                    int sweeps, unsigned long long seed, int8_t *dSt, hipStream_t st);

// Glauber chains of a dense pairwise model on the int8 matrix cores (gml_mcmc_chains.hip): the quantised model (digit planes Dg,
// the blocks' own q, diagonal, scales, row sums of q), burn_in + (spc - 1) thin sweeps, the recorded states into out [n][ld].
// A workgroup's chain tile is mcmc_chains_tile(n) chains (0: n too large), its state kMcmcChainsLds bytes at most.
constexpr int64_t kMcmcChainsLds = 128 * 1024;
constexpr int64_t kMcmcChainsMaxN = 16384;
int mcmc_chains_tile(int64_t n);
void launch_mcmc_chains(const int8_t *dDg, const double *dqblk, const double *ddiag, const double *dsig, const double *dqsum, int64_t n,
                        int64_t chains, int burn_in, int thin, int spc, unsigned long long seed, int8_t *dout, int64_t ld, hipStream_t st);

// Glauber chains of any term list with exact integer fields (gml_term_chains.hip).  Spin i's record: its field sum a, scale sig,
// Q = sum_e q_e and the word offsets of its incidences grouped by arity: those with k other spins (k = 1 .. 7) are the records
// [off[k-1], off[k]) of the stream, k + 1 words each: the int64 q_e 2^24 + j_1 (low word first), then j_2 .. j_k.
struct TermChainSpin {
    double a, sig;
    long long Q;
    long long off[8];
};
constexpr int kTermChainsMaxOthers = 7;
// the chain tile of a workgroup for n spins and `chains` chains (0: n too large); g_term_chains_tile (gml_testhooks.cpp), when
// set to 64, 128 or 256 and the state fits, forces it
extern int g_term_chains_tile;
int term_chains_tile(int64_t n, int64_t chains);
void launch_term_chains(const TermChainSpin *dspin, const unsigned *drec, int64_t n, int64_t chains, int burn_in, int thin, int spc,
                        unsigned long long seed, int8_t *dout, int64_t ld, hipStream_t st);
// Replica-exchange chains of the same records (gml_tempered_chains.hip): `ladders` ladders of `replicas` rungs (a power of two up
// to 64) at dbetas[replicas], one lane per rung on the tile term_chains_tile(n, ladders replicas); rung 0 recorded into out [n][ld];
// dswap_counts [2][replicas - 1] (attempts, accepts; zeroed by the caller) is added to.
void launch_tempered_chains(const TermChainSpin *dspin, const unsigned *drec, int64_t n, int64_t ladders, int replicas,
                            const double *dbetas, int swap_every, int burn_in, int thin, int spc, unsigned long long seed, int8_t *dout,
                            int64_t ld, unsigned long long *dswap_counts, hipStream_t st);
// Annealed importance sampling on the same records (gml_ais_chains.hip): one lane per chain on the tile term_chains_tile(n, chains),
// walked along dbetas[0 .. nbetas) with `sps` sweeps per step.  dspin0: the spin records of the start energy -- a_i, sigma_i of
// dspin, Q and record offsets over the incidences whose other spins are all above i -- into the same stream drec.  dlogw / dE
// [chains]; dstates [chains][n] row-major +-1 bytes, or NULL.
void launch_ais_chains(const TermChainSpin *dspin, const TermChainSpin *dspin0, const unsigned *drec, int64_t n, int64_t chains,
                       const double *dbetas, int64_t nbetas, int sps, unsigned long long seed, double *dlogw, double *dE,
                       int8_t *dstates, hipStream_t st);
// Conditional chains on the same records (gml_cond_chains.hip): `chains` = K replicas chains, chain r K + k started from row k of the
// sign bits dSb [n][wpr] on the visible spins and from chain_start_bit on the hidden ones (dhidden [n], non-zero = hidden; dhid [H]
// their indices, ascending), swept over the hidden spins only.  dhspin [H]: the spin records of the hidden spins -- over all their
// incidences (dcspin, dcst NULL), or over those with a hidden other spin, dcspin [H] then holding the rest and dcst [H][chains]
// receiving their per-chain integer.  dout [n][ld] or NULL; dmeans [H][chains] (zeroed by the caller) or NULL.
// g_cond_split (gml_testhooks.cpp): whether the host splits the records -- 0 never, 1 by its rule, 2 wherever it can.
extern int g_cond_split;
void launch_cond_chains(const TermChainSpin *dhspin, const TermChainSpin *dcspin, const int *dhid, const uint8_t *dhidden,
                        const unsigned *drec, const unsigned *dSb, int64_t wpr, int64_t K, int64_t n, int64_t H, int64_t chains,
                        int burn_in, int thin, int spc, unsigned long long seed, int8_t *dout, int64_t ld, double *dmeans, long long *dcst,
                        hipStream_t st);
// Conditional chains whose hidden set is a property of the row (gml_masked_chains.hip): chain r K + k hides the spins whose bit is set
// in row k of the sign bits dMb [n][mwpr] of a second handle and takes the others from row k of dSb [n][wpr].  dspin [n]: the spin
// records of k_term_chains over all incidences.  dout [n][ld] or NULL; dmeans [n][chains] (every entry written) or NULL.  The tile is
// masked_chains_tile(n, chains): term_chains_tile's rule (and its test hook) at twice the state words, 0 beyond n = 8192.
int masked_chains_tile(int64_t n, int64_t chains);
void launch_masked_chains(const TermChainSpin *dspin, const unsigned *drec, const unsigned *dSb, int64_t wpr, const unsigned *dMb,
                          int64_t mwpr, int64_t K, int64_t n, int64_t chains, int burn_in, int thin, int spc, unsigned long long seed,
                          int8_t *dout, int64_t ld, double *dmeans, hipStream_t st);

// Exact log Z and expectations of one connected component by streaming enumeration (gml_exact.hip).  The component's terms sorted by
// their mask over the low chunk bits (w, hi = the mask over the high bits); the runs of equal low mask cut into items
// [item_off[it], item_off[it + 1]) of at most 1024 terms: item_dst >= 0 is the padded slot (i + (i >> 4)) of the low mask whose only
// item it is, item_dst < 0 the partial sum ~item_dst; the masks of several items add the partial sums [ms_off[s], ms_off[s + 1]) into
// the padded slot ms_dst[s].  Queries (q_lo, q_hi), nq <= kExactWindow of them, query 0 the empty one (Z).  Group g of the grid takes
// the chunks [g cpg, (g + 1) cpg); gm [G] and gacc [G][nq] receive its running maximum and sums, dres [nq + 1] the combined sums and,
// last, their common maximum.
constexpr int kExactChunkBits = 12;                      // low bits of a chunk: 4096 states per workgroup pass
constexpr int kExactVec = 4096 + 256;                    // the padded vector
constexpr int kExactParts = 512;                         // partial sums of one chunk's coefficient vector
constexpr int kExactWindow = 1024;                       // queries accumulated in one enumeration, Z among them
constexpr int kExactBlock = 1024;                        // chunks added serially into one accumulator
constexpr int kExactGroups = 1024;                       // accumulation groups at most
constexpr int kExactMaxSpins = 40;                       // spins of a component
// g_exact_chunk_bits (gml_testhooks.cpp): 1 .. kExactChunkBits low bits instead of min(sb, kExactChunkBits); 0 = that default
extern int g_exact_chunk_bits;
struct ExactPlan {
    const double *w;
    const unsigned long long *hi;
    const int *item_off, *item_dst, *ms_off, *ms_dst;
    int ni, nm;
    const int *q_lo;
    const unsigned long long *q_hi;
    int nq;
    long long cpg;
    double *gm, *gacc;
};
void launch_exact(const ExactPlan &P, int G, double *dres, hipStream_t st);
// The k <= kBestMax best states of the component (gml_best.hip): the plan's terms, items and partial sums as above (its queries and
// sums play no part), c low bits.  Group g writes its best min(k, states of the group) pairs (energy, state: bit i set <-> spin i of
// the component is -1) to dge / dgs [G][k], best first, the rest -inf / ~0.
constexpr int kBestMax = 256;                            // states asked for: the group's list, 4 KB of LDS (= the workgroup's threads)
void launch_exact_best(const ExactPlan &P, int G, int c, int k, double *dge, unsigned long long *dgs, hipStream_t st);

// Exact conditional inference, one workgroup per row (gml_cond_exact.hip).  A plan is one hidden set: h hidden spins hid [h] (ascending;
// local bit j <-> hid[j]), c chunk bits.  The model's terms sorted by their hidden part (stable): w [T], vis [T][S] the visible spins of
// every term (kCondNoSpin = unused slot).  Row phase: items [item_off[it], item_off[it + 1]) of at most 1024 terms; item_dst >= 0 is the
// coefficient the item alone makes, item_dst < 0 the partial sum ~item_dst; the hidden parts of several items add the partial sums
// [ms_off[s], ms_off[s + 1]) into coefficient ms_dst[s].  Chunk phase: the nc coefficients lie in the order of their low (chunk)
// masks, chi [nc] their high parts; low mask s of ns takes the coefficients [run_off[s], run_off[s + 1]) into the padded slot
// run_dst[s].  A job is (plan, row); the results of row k go to log_w[k], log_p[k] and means[j ldm + k], j < h (any of them NULL).
constexpr int kCondMaxHidden = 24;                       // hidden spins of a row
constexpr int kCondMaxHigh = 12;                         // of them above the chunk: 4096 chunks per row
constexpr int kCondCoefs = 1024;                         // distinct hidden parts of a row's terms (the LDS array of the coefficients)
constexpr int kCondParts = 1024;                         // partial sums of one row's coefficients (they lie in the transform's vector)
constexpr int kCondMaxTermSpins = 8;                     // distinct spins of a term
constexpr int64_t kCondMaxN = 16384;                     // spins: the row's sign bits lie in 512 words of LDS
constexpr unsigned short kCondNoSpin = 16384;            // an unused slot of vis: bit kCondMaxN of the row's bits is always 0
// where the calling thread's last call of either entry point spent its time (gml_testhooks.cpp: gml_test_cond_exact_times): seconds on
// the host before the downloads without the slabs (checks, the mask's bits, planning), seconds in the slabs (upload, launch, drain),
// seconds in all.  Per thread: concurrent calls from several host threads do not share it.
extern thread_local double g_cond_exact_times[3];
struct CondExactPlan {
    const double *w;
    const unsigned short *vis;
    const int *item_off, *item_dst, *ms_off, *ms_dst;
    const unsigned short *chi;
    const int *run_off, *run_dst;
    int hid[kCondMaxHidden];
    int S, ni, nm, nc, ns, h, c;
};
struct CondExactJob {
    long long row;
    int plan, rep; // (rep: the first replica of a draw job, 0 elsewhere)
};
void launch_cond_exact(const CondExactPlan *dplans, const CondExactJob *djobs, int64_t njobs, const unsigned *dSb, int64_t wpr, int64_t n,
                       double *dmeans, int64_t ldm, double *dlog_w, double *dlog_p, hipStream_t st);
// The same jobs for the most probable hidden state of every row (the mode forms of the kernel): dstates[j lds + k] = +-1, the value of
// hid[j] in the state of largest E_k (equal energies: the lower local state), denergy[k] (or NULL) that energy, dlog_p[k] (or NULL)
// that energy - log_w[k].  With dlog_p NULL the kernel computes no exp and no second transform.
void launch_cond_mode(const CondExactPlan *dplans, const CondExactJob *djobs, int64_t njobs, const unsigned *dSb, int64_t wpr, int64_t n,
                      int8_t *dstates, int64_t lds, double *denergy, double *dlog_p, hipStream_t st);
// The same jobs for exact draws (the draw forms of the kernel): job (plan, row k, rep) draws the replicas rep .. min(rep +
// kCondDrawBatch, replicas) - 1 of row k.  Chain ch = r K + k: dstates[j K replicas + ch] = +-1, denergy[ch] (or NULL) the unperturbed
// energy of the drawn state, dlog_p[ch] (or NULL) that energy - log_w[k].  With dlog_p NULL: no exp, no second transform.
constexpr int kCondDrawBatch = 8;                        // replicas of a row drawn in one pass over its states
void launch_cond_draw(const CondExactPlan *dplans, const CondExactJob *djobs, int64_t njobs, const unsigned *dSb, int64_t wpr, int64_t n,
                      int64_t K, int replicas, uint64_t seed, int8_t *dstates, double *denergy, double *dlog_p, hipStream_t st);

// Batched Newton solve on the ragged Hessian blocks: A = s1[r]*H_r - s2*gF gF^T, A d = -pgF, in place
// (Cholesky, ridge restart).  gF/pgF/dout are R x cap; Sdiag[r] = A[m-1][m-1].
// faces: the orthant-face re-solves inside the kernel (working-set columns F [R][cap], iterates X [R][Qp] and their column kinds,
// the share of the predicted decrease that triggers a re-solve, the number of re-solves); fix / dfix [R][cap]: entries fixed
// from the start (tests).
struct NewtonFaces {
    const int *F = nullptr;
    const double *X = nullptr;
    const uint8_t *kind = nullptr;
    int64_t Qp = 0;
    double share = 0.05;
    int rounds = 0;
};
// the rows' last secant pairs (k_secant keeps them): pair l of row r at S / Y + l * stride + r * cap, npairs[r] of them.  Blocks of up
// to 128 entries take the BFGS correction inside the solve kernel, on the matrix it holds in LDS
struct SecantPairs {
    const double *S = nullptr, *Y = nullptr;
    const int *npairs = nullptr;
    int64_t stride = 0;
};
constexpr int kCholLds = 128; // blocks of up to this many entries are solved with the matrix in LDS
void launch_newton_solve(double *H, const long long *hoff, const int *mt, const int *msz, const double *s1, double s2,
                         const double *gF, const double *pgF, int R, int cap, double *dout, double *Sdiag, hipStream_t st, int maxm = 0,
                         const NewtonFaces *faces = nullptr, const uint8_t *fix = nullptr, const double *dfix = nullptr,
                         const SecantPairs *pairs = nullptr);
// Preconditioner tiles (T = 64 or 128): tile t holds the lower triangle of its T x T Hessian block at H + hoff[t] (pitch T);
// A = s1[wrow[t]] * H_t - s2 * g g^T on its first vm[t] entries is replaced, in place, by its inverse (full symmetric matrix);
// a block that is not positive definite even with a ridge becomes its inverse diagonal.
void launch_tile_inverse(int T, double *H, const long long *hoff, const int *vm, const int *wrow, const double *s1, double s2, const double *gV,
                         int64_t ntiles, hipStream_t st);

} // namespace gml
