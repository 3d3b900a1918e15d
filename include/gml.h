/*
 * gml.h -- C ABI of the MI355X-native learn() hot path of GraphicalModelLearning.jl.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / C++ types.  Every
 * entry point names the reference interface it replaces (paths relative to
 * /root/reference/src/GraphicalModelLearning.jl).  The reference-side binding (Julia
 * `ccall`) is shown in INTEGRATION.md and graphicalmodellearning.jl_amd/julia/.
 *
 * All functions return 0 on success or a GML_E* code; gml_last_error() returns a
 * thread-local message for the last failure.  The library never falls back to a CPU
 * implementation: without a usable HIP device every compute entry point fails with
 * GML_EHIP.
 */
#ifndef GML_H
#define GML_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------- */
#define GML_OK 0
#define GML_EINVAL 1     /* bad argument: shape, dtype, non +-1 spin, negative count, ...   */
#define GML_ENOTCONV 2   /* a node did not reach the KKT tolerance (reference: the
                            `@assert termination_status == LOCALLY_SOLVED` at :127,180,251,289,327) */
#define GML_EHIP 3       /* HIP runtime error / no device                                   */
#define GML_ENOMEM 4     /* the problem does not fit the device                             */
#define GML_EUNSUPPORTED 5

/* ---- formulations: the GMLFormulation subtypes (:20-56) ----------------------------- */
#define GML_RISE 0       /* RISE    (:30-35), objective :169-172; RISEA (:37-42, :191-260) is the same math */
#define GML_LOGRISE 1    /* logRISE (:44-49), objective :278-281                            */
#define GML_RPLE 2       /* RPLE    (:51-56), objective :316-319                            */

/* ---- element types of the sample histogram ------------------------------------------ */
#define GML_I8 0
#define GML_I32 1
#define GML_I64 2        /* what `sample()` returns (sampling.jl:52-54)                     */
#define GML_F64 3        /* what `readdlm` returns (test/runtests.jl:71)                    */

/* ---- arithmetic of the device objective/gradient pass ------------------------------- */
#define GML_PREC_F64 0   /* FP64 MFMA (v_mfma_f64_16x16x4_f64)                             */
#define GML_PREC_I8X 1   /* fixed point on v_mfma_i32_*_i8: Theta in 38-bit and V in 31-bit int8 limbs (V rounded
                            with a dither), integer GEMMs without further rounding: f, grad to ~1e-9 relative      */
#define GML_PREC_I8W 3   /* FP64-grade fixed point on the same int8 matrix cores: Theta in 54-bit (7 limb planes; entries within a
                            factor two of a row's largest are exact), V in dithered 47-bit int8 limbs (6 planes), exp in FP64,
                            integer GEMMs without further rounding: f, grad agree with a Float64 evaluation (:191-208) to the
                            1e-12 the GML_PREC_F64 path is held to, at ~6x its speed.  gml_learn builds its Hessians and
                            Hessian-vector products from the top 31 bits of the same V planes                              */
#define GML_PREC_AUTO 2  /* gml_objgrad_batch (the pair an external solver registers in place of the reference's Float64 obj / grad):
                            GML_PREC_I8W.  gml_learn: GML_PREC_I8X, except for solves with tol < 2e-10 and for small problems
                            (samples x parameters x spins <= 2^28: a property of the problem, not of the call or of the node
                            shard -- the reference's own fixtures, the README example; every kernel is launch-bound there), which
                            take GML_PREC_I8W (as few iterations as Float64; the 31-bit weights would stall at their noise floor).  Never GML_EUNSUPPORTED for a
                            valid histogram: beyond 2^24 configurations the int8 path keeps one set of i32
                            gradient accumulators per 2^23 configurations and adds them in int64             */

typedef struct gml_problem gml_problem; /* opaque: packed spins + weights resident in HBM  */

typedef struct gml_opts {
    double tol;          /* KKT tolerance: max |pseudo-gradient| per node (default 1e-9)    */
    int32_t max_iter;    /* outer (Newton) iterations (default 100)                         */
    int32_t precision;   /* GML_PREC_* (default GML_PREC_AUTO)                               */
    int32_t max_working; /* cap on a node's Newton block (default = max = 512, multiple of 32); a
                            denser optimum is solved by cycling blocks (block Gauss-Seidel)    */
    int32_t max_add;     /* new (violating) coordinates admitted per node per iteration (default 64; twice that while a node has
                            more than 16 max_working violators: a dense optimum) */
    int32_t verbose;     /* 0 silent, 1 per-iteration line on stderr                        */
    int32_t hess_samples; /* Newton Hessians use hess_samples configurations, rounded up to nb blocks of 512 (at least 2): every
                            kstride-th block of 512 of the histogram, kstride = blocks / nb rounded down (so the first nb blocks
                            once nb exceeds half of them), rescaled by the weight of those blocks; all of them once nb x 512
                            reaches the number of configurations (< 0 = all; 0 = adaptive: Kh_base x (local nodes / nodes still active), Kh_base = 32768 on
                            the FP64 path, so the last few nodes get all of them); the gradient always uses all     */
    int32_t polish;      /* precision i8x only: 0 = rows that stall above tol at the noise floor of the int8-limb
                            arithmetic continue on the FP64 path when its workspaces fit (default); -1 = never */
    int32_t max_cg;      /* conjugate-gradient iterations per Newton step of the matrix-free rows (working sets above
                            max_working); each costs one Hessian-vector pass (default 16) */
    /* tuning of the fixed-point arithmetic and of the matrix-free Newton-CG; 0 = the default named */
    int32_t limbs_fwd;   /* int8 limb planes of Theta in the objective passes: 3, 4 or 5 (default 5: 38 significant bits)  */
    int32_t hv_limbs_fwd; /* ... of the CG direction in the Hessian-vector passes: 2..5 (default 2: 14 bits, ample for an
                            inexact Newton step that stops at a 5 % residual)                                              */
    int32_t hv_limbs_bwd; /* limb planes of the products h_k (x_k . p) in those passes: 2 or 4 (default 2)                  */
    int32_t debug_row;   /* local row traced on stderr when verbose >= 2 (default 0)                                       */
    int32_t hv_subsample; /* the Hessian-vector products of the matrix-free rows run over 1/hv_subsample of the configurations,
                            spread over the whole histogram (the gradient always uses all of them, so only the convergence
                            rate is affected).  0 = automatic: rows still admitting their support: as many as keep >= 32
                            configurations per working-set entry, at most 8; rows with their support final: every configuration
                            for the first two steps of a solve, 1/2 from step 2, 1/8 from step 4 on (inexact Krylov: the later a
                            step, the less accurate its product needs to be).  1 = every configuration, always.  n > 1: the
                            admitting rows over 1/n, the others over every configuration                                     */
    int32_t coarse;      /* int8-limb precisions, exp forms: 0 = while every active node is farther than max(1e-7, 100 tol) (KKT) from its
                            optimum the passes run in a cheap form -- theta in 30 bits (i8w: its top four limb planes, one forward sweep
                            instead of two; i8x: four limb planes instead of five), the weights in three limb planes (dithered 23 bits),
                            one 3-plane backward launch -- and at full width for the rest of the solve, starting with a re-evaluation of
                            the rows that ended the phase: a coarse gradient certifies nothing (default); -1 = every pass at full width;
                            e > 0: the coarse phase ends at 10^-e                                                                  */
    double cg_viol_frac; /* matrix-free rows admit, per iteration, the violators within this fraction of the largest
                            violation (default 0.5: full Newton steps throughout on dense optima)           */
    double cg_eta;       /* CG stops at a residual reduced by min(cg_eta, sqrt(kkt)) (default 0.05); rows that are still building
                            their support (violators > 1/16 of the support) stop at 0.25                                   */
} gml_opts;

typedef struct gml_stats {
    int32_t iterations;      /* outer iterations                                            */
    int32_t passes;          /* full objective+gradient passes (all local nodes)            */
    int32_t forward_passes;  /* objective-only passes (line-search trials)                  */
    int32_t hessian_passes;
    int64_t node_evals;      /* sum over the objective(/gradient) passes of the number of nodes evaluated (their time: t_pass) */
    double max_kkt;          /* worst final KKT residual over local nodes                   */
    double lambda;           /* the regulariser actually used (:157)                        */
    double t_pack, t_pass, t_hess, t_host, t_total; /* seconds; t_pack = building the handle (gml_problem_ingest_times
                                t[3]: host packing + uploads + operand images), not part of t_total */
    int32_t not_converged;   /* number of local nodes above tol                             */
    int32_t polished;        /* 1 if rows were finished on the FP64 path (precision i8x, see gml_opts.polish) */
    int64_t hv_evals;        /* node evaluations of the Hessian-vector passes of the matrix-free rows (their time: t_hess) */
    double t_assemble;       /* gml_learn_terms: the device-side assembly of the term array + its copy to the caller (part of t_total) */
} gml_stats;

/*
 * ABI identity.  gml_opts and gml_stats are plain structs mirrored field by field in the bindings (the Julia file, the ctypes
 * twin): a binding built against another revision of this header would read and write the wrong bytes without any error.  Every
 * binding therefore checks, when it loads the library, that gml_abi_version() is the GML_ABI_VERSION it was written against and that
 * gml_sizeof_opts() / gml_sizeof_stats() equal the sizes of its own mirrors -- and refuses to run otherwise.  GML_ABI_VERSION is
 * bumped by every change of a struct layout, of an argument list or of the meaning of a constant.
 */
#define GML_ABI_VERSION 6
int gml_abi_version(void);
int64_t gml_sizeof_opts(void);
int64_t gml_sizeof_stats(void);

const char *gml_last_error(void);
void gml_default_opts(gml_opts *o);

/*
 * gml_problem_create -- replaces what every `learn` method does first: `data_info(samples)`
 * (:76-81) and the per-node `nodal_stat` comprehension (:162, :218, :271, :309; multi-body
 * :94-108), which it never materialises.
 *
 *   samples   K x (1+n) histogram, column 0 = counts, columns 1..n = spins in {-1,+1}
 *             (the `Array{T,2}` produced by sampling.jl:52-54).  ld = leading dimension;
 *             col_major != 0 for a Julia matrix (element (k,j) at samples[k + j*ld]),
 *             0 for a C/numpy matrix (samples[k*ld + j]).
 *   order     interaction order of the statistics: 2 = pairwise (RISE/logRISE/RPLE),
 *             p >= 2 = multiRISE(..., p) (:22-28).  order 1 = fields only.
 *   node0,node1  this handle solves nodes [node0, node1) (0-based); node-wise sharding for
 *             one-process-per-GPU runs (the `for current_spin = 1:num_spins` loop, :161).
 *             What a node range changes and what it does not: objective, gradient and Hessian-vector values of a row are the
 *             same bits whatever range the handle covers (int8-limb precisions).  The SOLVE's trajectory is not: the Newton
 *             Hessians are built from a sub-sample whose size depends on how many rows share the GPU (2^23 / rows, 32 768 ..
 *             131 072 configurations; gml_opts.hess_samples pins it), and the coarse phase ends for all rows of a handle at
 *             once -- so a row's iteration count and the last bits of its solution depend on the sharding (and on the GPU count),
 *             while every sharding ends within tol of the same optimum (tests: 2e-9 between shardings at tol 1e-9).
 *   device    HIP device ordinal.
 * The caller keeps ownership of `samples`; it is not referenced after return.
 */
int gml_problem_create(const void *samples, int dtype, int64_t K, int64_t n, int64_t ld,
                       int col_major, int order, int64_t node0, int64_t node1, int device,
                       gml_problem **out);

/*
 * Ingest.  gml_problem_create reads the caller's matrix exactly ONCE, on the host: a streaming packer (worker threads,
 * AVX2) turns 32 consecutive 8-byte elements of a spin column into one sign word, validates the +-1 alphabet and the
 * counts in the same sweep, and K n / 8 bytes of sign bits + 8 K bytes of weights cross PCIe instead of the
 * 8 K (n+1) of the Matrix{Int64} (`copy` of the Adjoint at :73; C3: 0.13 GB instead of 8.2 GB).  Packing overlaps the
 * copies (two pinned stages).  gml_problem_ingest_times reports the split:
 *   t[0] host packing (counts + sign words), t[1] allocations / uploads not hidden behind it, t[2] MFMA operand images
 *   (device), t[3] whole create call, t[4] of t[1]: stream + device allocations, t[5] of t[1]: weights; seconds.
 */
int gml_problem_ingest_times(const gml_problem *p, double t[6]);

/* The other route: the raw matrix is uploaded as it is and converted / validated on the device (64x the PCIe bytes;
 * for hosts with few cores).  Same arguments and the same resulting handle, bit for bit. */
int gml_problem_create_device_convert(const void *samples, int dtype, int64_t K, int64_t n, int64_t ld,
                                      int col_major, int order, int64_t node0, int64_t node1, int device,
                                      gml_problem **out);

/*
 * Packed form of a histogram, for callers that build several handles from one matrix (other processes, other GPUs) or
 * keep the samples packed: sign_bits [n][words_per_spin] dwords, spin-major, bit j of word w <-> configuration 32 w + j,
 * set <=> the spin is -1 (bits beyond K ignored); counts [K] doubles (NULL = all ones).
 *   gml_packed_words(K)         words_per_spin of the device image (K rounded up to 1024, / 32)
 *   gml_pack_histogram          host only (no device needed): matrix -> sign_bits, counts, *M = sum of counts (:76-81)
 *   gml_problem_create_packed   handle from the packed form
 *   gml_problem_get_sign_bits   the packed form of a handle's samples ([n][gml_packed_words(K)] dwords, host pointer),
 *                               e.g. of a handle sampled on the device
 * M has ONE definition on every route that takes counts (gml_problem_create, _create_device_convert, _create_spins, _create_packed,
 * gml_pack_histogram, gml_multi_create): the counts are summed left to right in blocks of 65 536 configurations, and the partial
 * sums are then added left to right.  Integer counts sum exactly in any order; for fractional counts this order is what makes
 * gml_problem_create_packed of gml_pack_histogram's output the handle of gml_problem_create, weight for weight (w_k = counts_k / M).
 * Refusals follow one precedence on all of these routes: the argument checks, the first count that is negative or not finite, a
 * zero sum of counts, then the first configuration (smallest index over all spins) that holds an entry other than +-1.
 */
int64_t gml_packed_words(int64_t K);
int gml_pack_histogram(const void *samples, int dtype, int64_t K, int64_t n, int64_t ld, int col_major,
                       uint32_t *sign_bits, int64_t words_per_spin, double *counts, double *M);
int gml_problem_create_packed(const uint32_t *sign_bits, int64_t words_per_spin, const double *counts, int64_t K, int64_t n,
                              int order, int64_t node0, int64_t node1, int device, gml_problem **out);
int gml_problem_get_sign_bits(gml_problem *p, uint32_t *sign_bits);

/* Same, from split inputs: counts (K doubles, NULL = all ones) and spins (K x n int8,
 * row-major).  Used by the synthetic benchmark so that no 8-byte histogram is built. */
int gml_problem_create_spins(const double *counts, const int8_t *spins, int64_t K, int64_t n,
                             int order, int64_t node0, int64_t node1, int device,
                             gml_problem **out);

/*
 * gml_problem_create_sampled -- the step BEFORE the path: replaces `sample(gm, N)` for pairwise models
 * (src/sampling.jl:34-57, 94-106) and feeds the result straight into a handle, all on the device.
 * `model` is the n x n symmetric matrix of FactorGraph(matrix) (models.jl:105-134): off-diagonal =
 * couplings, diagonal = fields.  Sampling is exact (enumeration + CDF inversion, the reference's own
 * method) per connected component of the coupling graph, so every component must have <= 22 spins
 * (GML_EUNSUPPORTED otherwise).  The handle holds N rows with count 1 each (M = N).
 */
int gml_problem_create_sampled(const double *model, int64_t n, int64_t N, uint64_t seed, int order,
                               int64_t node0, int64_t node1, int device, gml_problem **out);

/* Same for a model of any interaction order given as a term list (the reference's general sampler,
 * src/sampling.jl:60-88, dispatch :94-106): term t couples the spins keys[t*key_stride .. +key_stride)
 * (0-based, -1 = unused slot) with weight weights[t]; P(s) ~ exp(sum_t w_t prod_{i in t} s_i).  Exact per
 * connected component of the term hypergraph (<= 22 spins each).  A spin named twice in a key cancels (s^2 = 1) and is not part of
 * the term: it joins no component through it.  Zero-weight terms join nothing either.  Component b, counted in the order of the
 * components' smallest spins, draws sample k at u01(seed, b, k). */
int gml_problem_create_sampled_terms(const int32_t *keys, int key_stride, const double *weights, int64_t nterms,
                                     int64_t n, int64_t N, uint64_t seed, int order, int64_t node0,
                                     int64_t node1, int device, gml_problem **out);

/* Beyond the reference (whose only sampler is exact enumeration): N independent Glauber (heat-bath) chains of
 * `sweeps` sequential sweeps from a random start, for models whose components exceed 22 spins (lattices, ...).
 * Same term-list arguments as above; the final states of the chains become the handle's samples.
 * Both term-list entry points (and gml_problem_create_sampled_hist) check every argument and limit, the 22-spin component limit
 * included, before they look for the device: a bad term list is GML_EINVAL / GML_EUNSUPPORTED with or without a GPU. */
int gml_problem_create_mcmc_terms(const int32_t *keys, int key_stride, const double *weights, int64_t nterms,
                                  int64_t n, int64_t N, uint64_t seed, int sweeps, int order, int64_t node0,
                                  int64_t node1, int device, gml_problem **out);

/*
 * gml_problem_create_mcmc_chains -- long Glauber chains of a dense PAIRWISE model on the int8 matrix cores, several recorded
 * samples per chain.  `model` is the n x n symmetric matrix of FactorGraph(matrix) (diagonal = fields), as in
 * gml_problem_create_sampled.  The chain is the one of gml_problem_create_mcmc_terms on the term list {(i,j): A_ij, i < j; (i): A_ii}:
 *   start:    spin i of chain c is +1 iff u01(seed, 0xFFFFFFFF, c n + i) < 0.5;
 *   sweep sw (0-based, burn-in included) updates the spins 0 .. n-1 in order (spins before i carry their new values):
 *             u = u01(seed, sw, c n + i),  s_i = +1 iff u < 1.0 / (1.0 + exp(-2.0 h_i)),
 * with u01 the samplers' counter-based splitmix64 hash (53 bits).  The fields use a fixed quantisation of the couplings, row by
 * row: A_ij = sigma_i q_ij with sigma_i = 2^(e - 38), max_{j != i} |A_ij| < 2^e (e = 0 for a row without couplings), q_ij =
 * rint(A_ij / sigma_i) (to nearest, ties to even) held in 5 balanced int8 digit planes, q_ii = 0, and
 *   h_i = A_ii + sigma_i * (double) sum_{j != i} q_ij s_j,
 * where the integer sum is exact (|sum| < n 2^38) and converts to FP64 exactly.  The samples therefore depend only on the model,
 * seed, burn_in, thin, samples_per_chain and the chain index -- not on the kernel's chain tile, the grid or the device.  With
 * samples_per_chain = 1, row c is what gml_problem_create_mcmc_terms gives for chain c at sweeps = burn_in, up to the quantisation
 * (a decision whose u lies within ~1e-10 of its probability can differ).
 * Recorded: chain c's state after burn_in + t thin completed sweeps (t = 0 .. samples_per_chain-1) is row t chains + c, count 1,
 * M = chains samples_per_chain.  histogram != 0 (n <= 64): the handle holds the distinct configurations with their counts, as in
 * gml_problem_create_sampled_hist.
 * Cost: n^2 per chain-sweep (5 int8 planes on the matrix cores) WHATEVER the model's density; a sparse model stays cheaper on
 * gml_problem_create_mcmc_terms, whose cost grows with the degree of a spin.
 * GML_EINVAL (checked before any HIP call): NULL pointers, a non-symmetric or non-finite model, chains, samples_per_chain, burn_in
 * or thin below 1, a bad order or node range.  GML_EUNSUPPORTED: n > 16384 (the kernel's limit), histogram with n > 64.
 */
int gml_problem_create_mcmc_chains(const double *model, int64_t n, int64_t chains, int64_t samples_per_chain, int burn_in, int thin,
                                   uint64_t seed, int histogram, int order, int64_t node0, int64_t node1, int device,
                                   gml_problem **out);

/*
 * gml_problem_create_mcmc_terms_chains -- long Glauber chains of ANY term list (any order up to 8, any sparsity), several recorded
 * samples per chain, with exact integer fields.  The term list is that of gml_problem_create_mcmc_terms (keys: 0-based spins, -1 =
 * unused slot).  Every term contributes one incidence to each of its spins; a spin named twice in a key cancels (s^2 = 1);
 * zero-weight terms are skipped.  For spin i:
 *   a_i       the FP64 sum, left to right in term order, of the weights of its incidences with NO other spin (0 if none);
 *   sigma_i   2^(E - 38), where max |w_e| < 2^E over its incidences e WITH other spins (frexp; E = 0 if there are none);
 *   q_e       rint(w_e / sigma_i) (nearbyint: to nearest, ties to even) -- the rule gml_problem_create_mcmc_chains applies to a row;
 *   h_i       a_i + sigma_i * (double) sum_e q_e prod_{j in others(e)} s_j, the integer sum exact in int64 (|q| <= 2^38, fewer than
 *             2^24 incidences per spin) and converted to double once.
 * Start state, scan order, update and random stream are those of gml_problem_create_mcmc_chains:
 *   start:    spin i of chain c is +1 iff u01(seed, 0xFFFFFFFF, c n + i) < 0.5;
 *   sweep sw (0-based, burn-in included) updates the spins 0 .. n-1 in order (spins before i carry their new values):
 *             pup = 1.0 / (1.0 + exp(-2.0 * h_i)),  s_i = +1 iff u01(seed, sw, c n + i) < pup.
 * Recorded: chain c's state after burn_in + t thin completed sweeps (t = 0 .. samples_per_chain-1) is row t chains + c, count 1,
 * M = chains samples_per_chain.  The samples depend only on (model, seed, burn_in, thin, samples_per_chain, chain index): not on the
 * order of the terms with other spins, how incidences are grouped, the kernel's chain tile, the grid or the device.  On the term list
 * of a pairwise matrix ({(i,j): A_ij, i < j; (i): A_ii}) h_i is the double gml_problem_create_mcmc_chains computes, and the samples
 * are bit-identical to it.  histogram != 0 (n <= 64, M < 2^31): the handle holds the distinct configurations with their counts.
 * Cost: one LDS read per other spin of every incidence, per chain-sweep -- it follows the model's sparsity.
 * GML_EINVAL (checked before any HIP call): NULL pointers, key_stride < 1, a spin outside [0, n), a non-finite weight; chains,
 * samples_per_chain, burn_in or thin below 1; burn_in + (samples_per_chain - 1) thin > 2^31 - 1 or chains samples_per_chain
 * > 2^40; a bad order or node range.  GML_EUNSUPPORTED (before any HIP call, the limit named): n > 16384, a term with more than 8
 * distinct spins after cancellation, 2^24 or more incidences with other spins on one spin, histogram with n > 64.
 */
int gml_problem_create_mcmc_terms_chains(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                         int64_t chains, int64_t samples_per_chain, int burn_in, int thin, uint64_t seed, int histogram,
                                         int order, int64_t node0, int64_t node1, int device, gml_problem **out);

/*
 * gml_problem_create_mcmc_terms_tempered -- replica-exchange (parallel tempering) chains of ANY term list: the sampler for models with
 * more than one deep well (a ferromagnet below its transition, a glass at low temperature, a sharply learned model), where a
 * single-temperature chain stays in the well it fell into.  Term list, incidences, a_i, sigma_i, q_e and the exact int64 field h_i
 * are those of gml_problem_create_mcmc_terms_chains; E(s) = - sum_t w_t prod_{i in t} s_i.
 * Ladder l (of `ladders`) holds R = replicas states at the inverse temperatures betas[0] >= betas[1] >= ... >= betas[R-1] >= 0,
 * betas[0] > 0; rung r of ladder l has the chain index c = l R + r and targets P ~ exp(-beta_r E).  Only rung 0 is recorded.
 *   start:    every rung of ladder l starts from the start state of chain l R (spin i is +1 iff u01(seed, 0xFFFFFFFF, l R n + i) <
 *             0.5) with the tracked energy E_r = 0: energies are relative to the ladder's common start, which is all a swap needs.
 *   sweep sw (0-based, burn-in included): rung r updates the spins 0 .. n-1 in order,
 *             pup = 1.0 / (1.0 + exp(-2.0 * (beta_r * h_i))),  s_i = +1 iff u01(seed, sw, c n + i) < pup,
 *             E_r <- E_r - (s_new - s_old) * h_i in FP64 (the factor is 0 or +-2: the product is exact, one rounding per flip).
 *             The random stream belongs to the rung, not to the state that travels.
 *   swap:     after done = sw + 1 completed sweeps with done % swap_every == 0, round m = done / swap_every: for every r with
 *             r = m - 1 (mod 2) and r + 1 < R,  d = (beta_r - beta_{r+1}) * (E_r - E_{r+1});  the two rungs exchange their states
 *             and tracked energies iff u01(seed, 2^32 + sw, l R + r) < exp(fmin(d, 0.0)).  (Stream 2^32 + sw is no sweep's stream --
 *             a run has at most 2^31 - 1 sweeps -- and not the start's.)
 * Recorded, after the swap: rung 0 of ladder l after burn_in + t thin completed sweeps (t = 0 .. samples_per_chain-1) is row
 * t ladders + l, count 1, M = ladders samples_per_chain.  histogram as in gml_problem_create_mcmc_terms_chains.
 * swap_counts (host, [2][R-1], may be NULL): attempts[r] and accepts[r] of the pair (r, r+1), summed over all ladders and all rounds,
 * burn-in included; exact integers.
 * The samples and the counts depend only on (model, seed, betas, swap_every, burn_in, thin, samples_per_chain, ladder index): not on
 * the order of the terms with other spins, the kernel's tile, the grid or the device.  With replicas = 1 and betas[0] == 1.0 the
 * samples are those of gml_problem_create_mcmc_terms_chains, bit for bit.
 * GML_EINVAL (checked before any HIP call): everything gml_problem_create_mcmc_terms_chains rejects (ladders in the place of chains);
 * betas NULL; replicas not one of 1, 2, 4, 8, 16, 32, 64; a non-finite, negative or increasing beta; betas[0] <= 0; swap_every < 1;
 * ladders replicas > 2^40.  GML_EUNSUPPORTED: as gml_problem_create_mcmc_terms_chains.
 */
int gml_problem_create_mcmc_terms_tempered(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                           int64_t ladders, int64_t samples_per_chain, int burn_in, int thin, const double *betas,
                                           int replicas, int swap_every, uint64_t seed, int histogram, int order, int64_t node0,
                                           int64_t node1, int device, int64_t *swap_counts, gml_problem **out);

/*
 * gml_log_partition_ais -- log Z of ANY term list by annealed importance sampling (AIS): the missing half of the log-likelihood
 *   (1/M) sum_k c_k log P(s_k) = sum_t w_t <prod_{i in t} s_i>_data - log Z,
 * whose first half gml_problem_term_moments gives exactly.  Enumeration stops at about 22 spins; this is the term-list chain walked
 * from beta = 0 to the last beta with a running weight.  No handle is made; all pointers are host pointers.
 * Model.  The term list, incidences, a_i, sigma_i, q_e and the exact int64 field h_i are those of
 * gml_problem_create_mcmc_terms_chains.  E(s) = - sum_t w_t prod_{i in t} s_i.
 * Arguments and start.  betas[0 .. nbetas) must have nbetas >= 2 and betas[0] == 0.0.  Every value must be finite and >= 0.  The
 * sequence need not be monotone.  The estimate is of log Z(betas[nbetas-1]), normally 1.0.  Chain c starts like every chain here:
 * spin i is +1 iff u01(seed, 0xFFFFFFFF, c n + i) < 0.5.  That is an exact draw at beta = 0.
 * Start energy.  Every term is counted once, at the smallest spin it names, with that spin's quantisation.
 *   S_i = sum q_e prod_{j in others(e)} s_j over the incidences e of spin i whose other spins are all > i.  The sum is exact in
 *         int64 and converted to double once.
 *   t_i = a_i + sigma_i * (double)S_i.  sigma_i is a power of two, so this is one rounding.
 *   E = 0.0, then for i = 0 .. n-1 in order: E = E - s_i * t_i.  The product is exact.
 * Steps.  logw = 0.0, sw = 0.  For t = 1 .. nbetas-1:
 *   logw = logw - (betas[t] - betas[t-1]) * E.  The difference is rounded, the product is rounded, then the subtraction is rounded.
 *         No fused multiply-add is allowed on this line.  Every other FP64 product in the contract is exact, so contraction cannot
 *         change it.
 *   Then sweeps_per_step sweeps.  Each sweep updates spins 0 .. n-1 in order:
 *         pup = 1.0 / (1.0 + exp(-2.0 * (betas[t] * h_i))),  s_i = +1 iff u01(seed, sw, c n + i) < pup,
 *         E = E - (s_new - s_old) * h_i;
 *         sw += 1 after each sweep.
 * Outputs.  log_weights[c] = logw.  energies[c] = E at the end.  spins holds the final states.  All three depend only on (model,
 * seed, betas, sweeps_per_step, chain index).  They do not depend on the order of terms with other spins, the tile, the grid or the
 * device.
 * result.  Computed on the host in FP64, in chain order:
 *   m = max logw, x_c = exp(logw_c - m), s1 = sum x_c, s2 = sum x_c^2.
 *   result[0] = n * log(2.0) + m + log(s1 / chains).
 *   result[1] is the delta-method standard error sqrt((s2/chains - (s1/chains)^2) / (chains - 1)) / (s1/chains).  It is 0 when
 *             chains = 1 (and a difference that rounds below 0 counts as 0).
 *   result[2] = s1^2 / s2, the effective sample size.
 * What the numbers mean.  AIS is unbiased for Z.  It is therefore biased LOW for log Z in expectation (Jensen), and a likelihood
 * built on it is an optimistic one.  The standard error is that of the weights the chains produced: it does not see a well that no
 * chain found.  An effective sample size near 1 says the schedule is too short.
 * GML_EINVAL, before any HIP call: NULL keys, weights, betas or log_weights; key_stride < 1, nterms < 0, a spin outside [0, n), a
 * non-finite weight, n < 1; chains < 1 or > 2^31; nbetas < 2; betas[0] != 0; a negative or non-finite beta; sweeps_per_step < 1;
 * (nbetas - 1) * sweeps_per_step > 2^31 - 1.  GML_EUNSUPPORTED (before any HIP call, the limit named): n > 16384, a term with more than
 * 8 distinct spins after cancellation, 2^24 or more incidences with other spins on one spin.  The device is looked for last.
 * Cost: that of (nbetas - 1) * sweeps_per_step sweeps of gml_problem_create_mcmc_terms_chains over `chains` chains, plus one pass
 * over the terms for the start energy.  Device memory (the model's records twice, 16 bytes and n bytes per chain) is released
 * before the call returns.
 */
int gml_log_partition_ais(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, int64_t chains,
                          const double *betas, int64_t nbetas, int sweeps_per_step, uint64_t seed, int device,
                          double *log_weights /* [chains], host */, double *energies /* [chains] or NULL */,
                          int8_t *spins /* [chains][n] row-major, +-1, or NULL */, double *result /* [3] or NULL */);

/*
 * gml_model_exact -- exact log Z and exact model-side expectations of ANY term list whose connected components have at most 40
 * spins, by streaming enumeration on the device (no table of 2^n energies).  The yardstick for the estimate above, for the chain
 * samplers and for learned models.  No handle is made; all pointers are host pointers.
 * Model.  The term list as for gml_problem_create_sampled_terms: 0-based spins, -1 = unused slot, a spin named twice cancels, a term
 * of weight zero joins nothing.  P(s) = exp(sum_t w_t prod_{i in t} s_i) / Z.  A term that reduces to the empty key adds its weight to
 * log Z; a spin in no term (of non-zero weight) contributes ln 2 and has mean 0.
 * Components.  The work is done per connected component of the term hypergraph; log Z is the sum over the components.
 * Outputs.  *log_z.  mean [n] (or NULL): <s_i>.  corr [n][n] row-major (or NULL): <s_i s_j>, 1.0 on the diagonal, the product of
 * the two means for spins of different components.  qexp [nq] (or NULL when nq = 0): <prod_{i in q} s_i> of every query key in
 * qkeys [nq][qkey_stride] (the conventions of the term keys), the product over the components of the expectations of the key's
 * restrictions; an empty or fully cancelled query gives 1.0.
 * Arithmetic.  FP64 throughout.  Every sum has a fixed order that depends on the model alone -- the terms of one low mask in the
 * caller's order, the chunks of an accumulation group in index order, the groups in index order; no accumulator takes more than 1024
 * summands serially -- so two calls with the same arguments return the same bits, on any grid.  The weights enter through running
 * maxima: couplings of +-150 neither overflow nor underflow.  A-priori error of log Z and of every expectation: about
 * (12 + log2 T) 2^-53 sum_t |w_t| from the energies plus 1e-13 from the sums.
 * GML_EINVAL, before any HIP call: log_z NULL; NULL keys or weights with nterms > 0; key_stride < 1; nterms < 0; n < 1; a spin outside
 * [0, n) in a term or a query; a non-finite weight; nq < 0; nq > 0 with NULL qkeys or qexp or qkey_stride < 1.  GML_EUNSUPPORTED,
 * before any HIP call: a component of more than 40 spins, or of more than 2^20 terms of non-zero weight.  The device is looked for
 * last.
 * Cost.  One enumeration of 2^sb states per component of sb spins and per window of 1023 expectations (the means and, with corr, the
 * pairs of the component, then the restrictions of the queries): measured times in DESIGN 3.18.  Device memory (the component's
 * terms, 8 MB of group sums) is released before the call returns.
 */
int gml_model_exact(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, const int32_t *qkeys,
                    int qkey_stride, int64_t nq, int device, double *log_z, double *mean /* [n] or NULL */,
                    double *corr /* [n][n] or NULL */, double *qexp /* [nq] or NULL */);

/*
 * gml_problem_create_mcmc_terms_conditional, gml_conditional_means -- conditional inference: Glauber chains of ANY term list that
 * start from the rows of a resident handle and hold the observed spins fixed.  "Given these spins, what are the others?"
 * Inputs: a term list (keys, key_stride, weights, nterms, n) as for gml_problem_create_mcmc_terms_chains; a resident handle `evidence`
 * with the same n and K rows; a mask hidden [n] of uint8 (non-zero = hidden) with at least one hidden spin; replicas >= 1,
 * samples_per_chain, burn_in, thin, seed.  Let the hidden spins in ascending order be i_0 < ... < i_{H-1}.
 * Chains.  There are chains = K * replicas.  Chain c = r * K + k is replica r of evidence row k.  The counts of the evidence handle
 *   play no part: every row gets `replicas` chains.
 * Start.  A visible spin s has the value of row k of the evidence handle.  A hidden spin s starts as in every chain here:
 *   chain_start_bit(seed, c, n, s), i.e. +1 iff u01(seed, 0xFFFFFFFF, c n + s) < 0.5.
 * Sweep sw.  It is 0-based and burn-in is included.  For a = 0 .. H-1 in order, with i = i_a:  h = a_i + sigma_i * (double)S_i.
 *   a_i, sigma_i, q_e are those of gml_problem_create_mcmc_terms_chains (unchanged).  S_i is the exact int64 sum over ALL incidences of
 *   spin i at the current state.  pup = 1 / (1 + exp(-2 h)).  The new spin is +1 iff u01(seed, sw, c n + i) < pup.  Visible spins
 *   are never visited.  The stream is that of gml_problem_create_mcmc_terms_chains, unchanged.
 * Recording.  Recorded sweeps are those of gml_problem_create_mcmc_terms_chains: after done = sw + 1 completed sweeps with
 *   done >= burn_in and (done - burn_in) % thin == 0, t = (done - burn_in) / thin.  The state is written at row t * chains + c.
 * Conditional means (Rao-Blackwellised).  mean[a][c] = (1 / samples_per_chain) * sum over the recorded sweeps of (2 pup - 1), where
 *   pup is the value the heat bath used for spin i_a in that sweep.  The sum is accumulated in FP64 in sweep order and multiplied by
 *   the FP64 quotient 1.0 / samples_per_chain once.  Output layout is [H][chains], hidden-major.
 * Consequence.  With every spin hidden and replicas = 1 the states are those of gml_problem_create_mcmc_terms_chains with chains = K
 *   and the same seed, bit for bit.
 * The results depend only on (model, evidence rows, hidden, replicas, samples_per_chain, burn_in, thin, seed): not on the order of
 * the terms with other spins, the kernel's chain tile, the grid or the device, and not on whether the kernel sums the incidences
 * whose other spins are all visible once per chain or in every sweep (both sums are exact integers).
 * gml_problem_create_mcmc_terms_conditional: the new handle lives on the evidence handle's device and has chains * samples_per_chain
 *   rows with count 1.  There is no histogram flag: row (t, r, k) of the result belongs to row k of the evidence, and deduplication
 *   would break that.
 * gml_conditional_means: means [H][K * replicas] (host).  It makes no handle and no state buffer; its device memory is released
 *   before it returns.
 * GML_EINVAL, before any device work: NULL evidence, hidden, out or means; no hidden spin; n different from the evidence handle's;
 *   replicas < 1; everything gml_problem_create_mcmc_terms_chains rejects, with chains = K * replicas.  GML_EUNSUPPORTED: the limits of
 *   gml_problem_create_mcmc_terms_chains (n > 16384, more than 8 distinct spins in a term, 2^24 incidences on a spin).
 * Cost per chain-sweep: the incidences of the hidden spins -- where the all-visible ones are summed once per chain (the library does
 *   so when they are many enough to pay), only those that name another hidden spin, plus one 8-byte load per hidden spin.
 */
int gml_problem_create_mcmc_terms_conditional(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                              gml_problem *evidence, const uint8_t *hidden /* [n], host */, int replicas,
                                              int64_t samples_per_chain, int burn_in, int thin, uint64_t seed, int order, int64_t node0,
                                              int64_t node1, gml_problem **out);
int gml_conditional_means(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, gml_problem *evidence,
                          const uint8_t *hidden /* [n], host */, int replicas, int64_t samples_per_chain, int burn_in, int thin,
                          uint64_t seed, double *means /* [H][K * replicas], host */);

/*
 * gml_problem_create_mcmc_terms_masked, gml_conditional_means_masked -- the conditional chains for data with holes: the hidden set is a
 * property of the ROW.  "This sample lacks these spins, that sample lacks others: what are they?"
 * Inputs.  A term list, as for gml_problem_create_mcmc_terms_conditional.  A resident handle `evidence` (n, K rows).  A resident handle
 *   `mask` on the same device with the same n and K: in its sign bits a set bit (spin -1) means "hidden in this row" and +1 means
 *   "observed".  replicas >= 1, samples_per_chain, burn_in, thin, seed.  The mask is a handle because that reuses the ingest and the
 *   layout of the sign bits, because it stays resident, and because gml_problem_split with one seed cuts evidence and mask into matching
 *   folds.  The counts of both handles play no part.  Where row k of the mask hides spin s, the value row k of the evidence holds for
 *   s plays no part either.
 * Everything else is the rule of gml_problem_create_mcmc_terms_conditional with "hidden" read per row.
 * Chain index.  Chain c = r K + k is replica r of row k.
 * Start.  Observed spins come from evidence row k.  Hidden spins come from chain_start_bit(seed, c, n, s).
 * Sweep.  Sweep sw visits i = 0 .. n - 1 in ascending order.  Chain c updates spin i iff it is hidden in row k.
 * Update.  h = a_i + sigma_i (double) S_i over all incidences of spin i, with the unfiltered records of
 *   gml_problem_create_mcmc_terms_chains.  pup = 1 / (1 + exp(-2 h)).  The new spin is +1 iff u01(seed, sw, c n + i) < pup.
 * Recorded sweeps.  As gml_problem_create_mcmc_terms_chains: row t * chains + c.
 * Means.  Layout is [n][K * replicas], FP64.  For a hidden entry: the Rao-Blackwellised mean of 2 pup - 1 over the recorded sweeps,
 *   summed in sweep order, times 1.0 / samples_per_chain.  For an observed entry: the evidence value, +-1.0.
 * Rows without holes.  A row with no hidden spin is legal.  Its chains return the row.
 * Consequence.  When every row of `mask` equals one vector, states and means (its rows i_0 < ... < i_{H-1}) are those of
 *   gml_problem_create_mcmc_terms_conditional / gml_conditional_means with that vector as `hidden`, bit for bit.
 * The random stream is counter based on (sw, c n + i): the library evaluates an update only where some chain of a group of 64
 *   consecutive chains hides the spin, and what it skips changes no bit.  Cost per chain-sweep: the incidences of the spins hidden
 *   by one of the 64 chains c .. c + 63 (c a multiple of 64) -- rows with similar masks are cheapest next to each other.
 * GML_EINVAL, before any device work, in the order of gml_problem_create_mcmc_terms_conditional: NULL evidence, mask, out or means; n
 *   different from the evidence handle's; a mask handle whose n, K or device differs from the evidence handle's; replicas < 1;
 *   everything gml_problem_create_mcmc_terms_chains rejects, with chains = K * replicas.  GML_EUNSUPPORTED: the limits of
 *   gml_problem_create_mcmc_terms_chains, and n > 8192 (a chain holds its state and its mask on chip: twice the words).
 * gml_conditional_means_masked makes no handle and no state buffer; every device buffer of both is released on every path.
 */
int gml_problem_create_mcmc_terms_masked(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                         gml_problem *evidence, gml_problem *mask, int replicas, int64_t samples_per_chain, int burn_in,
                                         int thin, uint64_t seed, int order, int64_t node0, int64_t node1, gml_problem **out);
int gml_conditional_means_masked(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                 gml_problem *evidence, gml_problem *mask, int replicas, int64_t samples_per_chain, int burn_in, int thin,
                                 uint64_t seed, double *means /* [n][K * replicas], host */);

/*
 * gml_conditional_exact, gml_conditional_exact_masked -- exact conditional inference: every row's hidden spins are enumerated on the
 * device, no chain.  The yardstick for the conditional chains above, and the only way to the joint conditional probability of held-out
 * values and to the marginal likelihood of a partly observed row.  Any n <= 16384, at most 24 hidden spins per row.
 * Model.  The term list with the conventions of gml_model_exact: 0-based spins, -1 = unused slot, a spin named twice cancels, a term of
 *   weight zero joins nothing.  The weights are FP64 and NOT quantised (the chains quantise every spin's couplings to 2^-38 of its
 *   largest).
 * Definitions.  Row k of the evidence handle has a hidden set H_k of h_k spins and observed values x_O.  For a reduced term t,
 *   hid(t) = t & H_k and sigma_{t,k} = prod_{j in t \ H_k} x_{k,j}.  E_k(s_H) = sum_t w_t sigma_{t,k} prod_{i in hid(t)} s_i, over ALL
 *   terms: those with an empty hidden part and the empty key are the row's constant.
 * Outputs, per row (host; any may be NULL, not all three).
 *   log_w [K]: log sum_{s_H} exp(E_k(s_H)).  log P(x_O) = log_w[k] - log Z.  A row without a hidden spin gives E(row).
 *   means: E[s_i | x_O] of the hidden spins.
 *   log_p [K]: E_k(the values the evidence row holds on H_k) - log_w[k] = log P(x_H = held values | x_O).  Meaningful where the held
 *     values are the truth (a predictive check); it plays no part otherwise.
 * gml_conditional_exact: one hidden set for every row, hidden [n] of uint8 (non-zero = hidden), at least one; means is [H][K],
 *   hidden-major, the hidden spins ascending -- the layout of gml_conditional_means with replicas = 1.
 * gml_conditional_exact_masked: the hidden set of row k is the set bits of row k of the handle `mask` (as for
 *   gml_conditional_means_masked); means is [n][K], an observed entry holding its evidence value +-1.0.  A row without holes is
 *   legal.  The counts of the handles play no part in either.
 * Determinism.  The result of a row is a pure function of the model, that row and that row's hidden set: the same bits on every call,
 *   wherever the row sits, whatever the other rows are, on any grid.  Every sum has a fixed order -- the terms of one hidden part in
 *   the caller's order, the coefficients of one chunk mask in ascending order of their hidden parts, the chunks in index order -- and no
 *   accumulator takes more than 1024 summands serially.  A mask handle whose rows all equal one vector gives, bit for bit, what
 *   gml_conditional_exact gives with that vector.
 * Arithmetic.  That of gml_model_exact: FP64, running maxima (couplings of +-150 neither overflow nor underflow), the a-priori error
 *   of every output about (12 + log2 T) 2^-53 sum_t |w_t| plus 1e-13.
 * GML_EINVAL, before any device work, in this order: all three outputs NULL; NULL evidence; NULL hidden / mask; NULL keys or weights,
 *   key_stride < 1, nterms < 0; n different from the evidence handle's; a mask handle whose n, K or device differs from the evidence
 *   handle's; no hidden spin (gml_conditional_exact only); a non-finite weight or a spin outside [0, n).
 * GML_EUNSUPPORTED, the limit named in gml_last_error, in this order: n > 16384; more than 24 hidden spins (the masked form names the
 *   first such row; it reads the hidden sets from the device, so this one check of it follows the download of the mask's bits and
 *   precedes every enumeration); a term of more than 8 distinct spins (of non-zero weight; in the masked form this one precedes the
 *   download); more than 1024 distinct hidden parts hid(t) under one hidden set; more than 1024 partial sums under one hidden
 *   set (the hidden parts of more than 1024 terms are summed in items of 1024: any model of up to 2^19 terms fits, and up to 2^20 where
 *   they gather in one hidden part, as the visible-only terms of a dense model do).  For gml_conditional_exact all of these precede any device work.
 * Cost.  Per row one pass over the T terms (the row's coefficients) and 2^h states in chunks of 4096; per distinct hidden set one
 *   pass over the terms and a sort of them on the host.  Measured times in DESIGN 3.19.  No handle is made; every device buffer is
 *   released on every path.
 */
int gml_conditional_exact(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, gml_problem *evidence,
                          const uint8_t *hidden /* [n], host */, double *means /* [H][K] or NULL */, double *log_w /* [K] or NULL */,
                          double *log_p /* [K] or NULL */);
int gml_conditional_exact_masked(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                 gml_problem *evidence, gml_problem *mask, double *means /* [n][K] or NULL */,
                                 double *log_w /* [K] or NULL */, double *log_p /* [K] or NULL */);

/*
 * gml_model_best_states -- the k most probable states of ANY term list whose connected components have at most 40 spins, certified
 * by streaming enumeration on the device: the states the model "means".  The pipeline of gml_model_exact up to the energies of every
 * state, which are then selected instead of summed (no exponential, no second transform).  No handle is made; all pointers are host
 * pointers.
 * Model.  The conventions of gml_model_exact: 0-based spins, -1 = unused slot, a spin named twice cancels, a term of weight zero joins
 *   nothing, FP64 weights as given.  E(s) = sum_t w_t prod_{i in t} s_i; a term that reduces to the empty key is a constant of every
 *   energy.
 * Outputs.  *found = min(k, 2^n).  states [found][n] row-major, +-1, and energies [found]: the found states of largest E, energy
 *   descending; equal energies in state order -- the state read as a binary number with spin i at bit i, a set bit = spin -1, the
 *   smaller number first (for n > 64: compared from the highest spin down).  The rows beyond found are not written.
 * Limits.  1 <= k <= 256.  The cap is a design choice: a workgroup keeps its running list of k (energy, state) pairs in 4 KB of LDS
 *   beside the transform's vector, and the groups' lists come down to the host (1024 k pairs at most, 4 MB).
 * Selection on the device, order on the host.  Per component the device selects by the energies its butterflies produce -- a pure
 *   function of (model, chunk width) at every state -- and gives equal ones to the lower state.  For every selected state the host
 *   then recomputes the energy as the plain FP64 sum of the component's reduced terms in the caller's order (no accumulator takes more
 *   than 1024 summands serially: halves above that) and sorts by (that energy descending, state ascending).  energies are therefore
 *   plain sums, not butterfly outputs.  Consequence: among states whose true energies agree within the a-priori bound of
 *   gml_model_exact, (12 + log2 T) 2^-53 sum_t |w_t|, which of them make the cut at position k follows the device's rounding: it is
 *   deterministic and a pure function of the model, and otherwise unspecified.  The pair s, -s of a model with only even terms
 *   recomputes to bit-equal energies and comes out in state order when both are inside the cut.
 * Components.  A sum of independent parts: every component gives its own list of min(k, 2^sb) states (a spin in no term: two states of
 *   energy 0, +1 first, no device work), and the lists are merged on the host in pairs, in the order of the components' smallest spins,
 *   starting from the constant: the k best sums e_A + e_B of two sorted lists (a heap over the pairs, carried past k through every sum
 *   that ties with the k-th), ordered by (sum descending, joint state ascending).  The merge is a function of the model alone.
 * Two calls with the same arguments return the same bytes.
 * GML_EINVAL, before any HIP call, in this order: NULL keys or weights with nterms > 0, key_stride < 1; n < 1 or nterms < 0; a spin
 *   outside [0, n) or a non-finite weight; k < 1; NULL found, states or energies.  GML_EUNSUPPORTED, before any HIP call, the limit
 *   named in gml_last_error, in this order: k > 256; a component of more than 40 spins, or of more than 2^20 terms of non-zero weight.
 *   The device is looked for last.
 * Cost.  One enumeration of 2^sb states per component; k = 1 keeps one best per thread and costs about three quarters of "log Z
 *   alone"; k > 1 adds a sort only in the chunks that beat the list's k-th energy.  Measured times in DESIGN 3.20.  Device memory is
 *   released before the call returns.
 */
int gml_model_best_states(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, int64_t k, int device,
                          int64_t *found, int8_t *states /* [k][n] row-major, +-1 */, double *energies /* [k] */);

/*
 * gml_model_elim_plan, gml_model_elim -- exact log Z, means and term expectations of a SPARSE term list of any number of spins, by
 * variable elimination on the device.  The cost follows the width of an elimination order, not the number of spins: a 16 x 16
 * lattice (256 spins in one component, refused by gml_model_exact) has width 17.  No handle is made; all pointers are host pointers.
 * Model.  The conventions of gml_model_exact: 0-based spins, -1 = unused slot, a spin named twice cancels, a term of weight zero joins
 *   nothing.  Spins that share a term of non-zero weight are neighbours.
 * Order.  order [n]: a permutation of 0 .. n - 1, or NULL for the greedy one.  The connected components are taken in the order of
 *   their smallest spin, each one's spins in the order the permutation names them.  Greedy: a component starts at its lowest spin;
 *   then, among the unprocessed spins with a processed neighbour, the one whose step leaves the smallest frontier, the lowest index
 *   among equals.  order_out [n] (or NULL): the order used, component by component.
 * Plan.  A term is applied at the step of its last spin.  The frontier F_t: the processed spins with an unprocessed neighbour.  The
 *   scope of step t: F_{t-1} and v_t.  *width = the largest scope; *work = sum_t 2^|scope_t|; *stored = sum_t 2^|F_t| (t = 1 .. n;
 *   both sums in step order in FP64).  A spin in no term is a step of scope 1.  gml_model_elim_plan makes no HIP call and refuses
 *   nothing but bad arguments: it is how a caller learns the width beforehand.
 * Recursion, per component, every table in the log domain (couplings of +-150 neither overflow nor underflow), FP64:
 *   alpha_t = logsumexp over the spins retiring at t of (alpha_{t-1} + phi_t), phi_t = the signed weights of the terms applied at t in
 *   the caller's order; log Z = alpha_n + the weights of the empty keys + ln 2 per spin in no term, the components in order.  With
 *   mean or texp a backward pass: p_t = exp(alpha_{t-1} + phi_t + beta_t - alpha_n), <s_u> = sum p_t s_u for u retiring at t,
 *   <prod_{i in k} s_i> = sum p_t prod s_i for term k applied at t, beta_{t-1} = logsumexp over v_t of (phi_t + beta_t).
 * Outputs.  *log_z.  mean [n] (or NULL); a spin in no term has mean 0.  texp [nterms] (or NULL): the expectation of every term's
 *   reduced key, in the caller's order; an empty or cancelled key gives 1.0.  The recursion sees a key's spins in one scope only where
 *   the term has a non-zero weight (it is what makes them neighbours): a term of weight zero gives NaN, unless its reduced key has
 *   at most one spin (1.0, or that spin's mean).  A key of non-zero weight lies within one component by construction, so no product
 *   over components arises; use gml_model_exact for the expectation of a key the model does not hold.
 * Determinism.  Every sum has a fixed order and every grid is a function of the table sizes: per thread in index order, per workgroup
 *   a tree, the workgroups 1024 at a time in index order; two calls with the same arguments return the same bits.
 * Error.  With L = sum_t |w_t| + n ln 2 and T terms: about 2^-53 (T + 4 n) L for log Z, four times that plus 1e-13 for the
 *   expectations.
 * GML_EINVAL, before any HIP call, in this order: log_z NULL; NULL keys or weights with nterms > 0, key_stride < 1; n < 1 or
 *   nterms < 0; a spin outside [0, n) or a non-finite weight; order not a permutation of 0 .. n - 1.  GML_EUNSUPPORTED, before any
 *   HIP call: a width above GML_ELIM_MAX_WIDTH; with mean or texp, stored above 2^32 entries (32 GiB of forward tables; log_z alone
 *   keeps two tables).  The device is looked for last.  GML_ENOMEM: the device cannot hold the tables.
 * Cost.  Planning: per step the neighbour lists of the current candidates (up to frontier x degree of them) -- quadratic in n on
 *   hub-like graphs whose frontier grows with n.  All components run on one stream with one synchronisation per call.  One launch per
 *   step forward (more where over 3 spins retire at once), one or two per step backward; a forward step reads
 *   2^|F_{t-1}| and writes 2^|F_t| doubles.  Measured times in DESIGN 3.22.  Device memory is released before the call returns.
 */
#define GML_ELIM_MAX_WIDTH 30
int gml_model_elim_plan(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                        const int32_t *order /* [n] permutation, or NULL: greedy */, int32_t *order_out /* [n] or NULL */,
                        int32_t *width, double *work /* sum_t 2^|scope_t| */, double *stored /* sum_t 2^|F_t| */);
int gml_model_elim(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                   const int32_t *order /* or NULL */, int device, double *log_z, double *mean /* [n] or NULL */,
                   double *texp /* [nterms] or NULL */);

/*
 * gml_problem_create_sampled_elim -- N exact, independent draws of a SPARSE term list of any number of spins into a resident handle,
 * by backward sampling on the tables of gml_model_elim: no chain, no burn-in.  Where gml_problem_create_sampled_terms refuses a
 * component of more than 22 spins, this one asks for an elimination order of width at most GML_ELIM_MAX_WIDTH.
 * Model, order, plan.  Exactly those of gml_model_elim: the conventions of the keys, the components in the order of their smallest
 *   spin, the caller's permutation or the greedy order, a term applied at the step of its last spin.
 * Tables.  A table over a frontier of k spins has 2^k entries; bit b of an index set <=> the spin in slot b is -1.  The scope of a
 *   step: the slots of its input table plus, at bit k, the spin the step introduces.  A step whose retiring spins number R is run as
 *   max(1, ceil(R / 3)) launches: the first introduces the spin and adds phi (the signed weights of the step's terms in the caller's
 *   order, summed from 0.0 in FP64), each sums out the at most 3 retiring spins of lowest scope position that are left.  Slot rule of
 *   a launch's output table: the surviving bits below the new size keep their place; the others fill the freed bits in ascending
 *   order.  scope_of(j): the scope state whose surviving bits are those of output index j, the retiring bits 0.
 *   out[j] = logsumexp over the retiring bits of (in[s & inmask] + phi(s)), inmask = 2^kin - 1: the forward pass of gml_model_elim
 *   with moments, which keeps every step's table; here the tables between the launches of one step are kept too.
 * Launch numbers.  The forward launches of the whole call are numbered 0, 1, 2, ...: the components in their order, the launches of
 *   a component in forward order.  A component of a single spin with a field is a launch like any other.
 * The draw.  Sample k walks the launches from the last to the first and carries one table index j: the entry of the launch's output
 *   table that the spins drawn so far select.  The last launch of a component writes one entry: j = 0.  At launch l with r retiring
 *   bits rbit[0] < ... < rbit[r-1]:
 *     candidates  c = 0 .. 2^r - 1 in ascending order, bit i of c <-> rbit[i]; s_c = scope_of(j) | the bits of c;
 *                 x_c = in[s_c & inmask] + phi(s_c), the expression, the term order and the bits of the forward pass
 *     weights     m = max_c x_c; p_c = exp(x_c - m); total = p_0 + ... + p_{2^r - 1}, summed in that order
 *     number      u = u01(seed, l, k) of gml_rng.h (stream = the launch number, counter = the sample)
 *     pick        the smallest c with p_0 + ... + p_c > u * total (the running sum of the total); the last c if rounding leaves none
 *     result      retiring spin i is -1 iff bit i of the picked c is set; the index for launch l - 1 is s_c & inmask
 *   A launch with r = 0 draws nothing, consumes no number and maps the index: j <- scope_of(j) & inmask.
 *   A spin i in no term (of non-zero weight) is +1 iff u01(seed, 2^62 + i, k) < 0.5.
 * Exactness.  The product of the picked p_c / total along a walk telescopes to exp(E(s) - log Z): the draws are exact and
 *   independent up to FP64 rounding of the tables (the error of gml_model_elim) and the 53 bits of u per launch.  The limit: a
 *   candidate whose p_c is below about 2^-53 of its launch's total is never drawn.
 * Determinism.  Row k is a pure function of (model, order, seed, k): not of N, the grid, `histogram` or the device.  The same
 *   arguments give the same bytes.
 * Handle.  porder, node0, node1, histogram: those of gml_problem_create_mcmc_terms_chains.  N rows of count 1, M = N; with
 *   histogram != 0 the distinct configurations with their counts (n <= 64, N < 2^31).
 * GML_EINVAL, before any HIP call, in this order: out NULL; NULL keys or weights with nterms > 0, key_stride < 1; n < 1 or
 *   nterms < 0; a spin outside [0, n) or a non-finite weight; porder outside [1, 8] or a bad node range; N outside [1, 2^40]; order not a
 *   permutation of 0 .. n - 1.  GML_EUNSUPPORTED, before any HIP call, the limit named in gml_last_error, in this order: a width above
 *   GML_ELIM_MAX_WIDTH; more than 2^32 kept table entries (`stored` of gml_model_elim_plan plus the tables between the launches of
 *   one step); n > 16384; histogram with n > 64 or N >= 2^31.  The device is looked for last.  GML_ENOMEM: the device cannot hold
 *   the tables and the n x N output bytes.
 * Cost.  The forward pass once per call, whatever N is; then per sample one read of every launch record and term of the model and
 *   2^r table entries per launch.  All on one stream with one synchronisation before the handle is built.  Measured times in
 *   DESIGN 3.23.  Everything but the handle is released before the call returns.
 */
int gml_problem_create_sampled_elim(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, int64_t N,
                                    uint64_t seed, const int32_t *order /* [n] or NULL: greedy */, int histogram, int porder,
                                    int64_t node0, int64_t node1, int device, gml_problem **out);

/*
 * gml_conditional_mode, gml_conditional_mode_masked -- the most probable JOINT completion of every row's hidden spins: s_H* = argmax
 * over the 2^h hidden states of E_k(s_H), by the enumeration of gml_conditional_exact[_masked] with the energies selected instead of
 * summed.  Not the signs of the conditional means, which decide spin by spin.
 * Model, evidence, hidden / mask, E_k, limits: exactly those of gml_conditional_exact and gml_conditional_exact_masked.
 * Outputs, per row (host).
 *   states: the values (+-1) of the hidden spins in s_H*.  Equal energies (as the device's butterflies produce them) go to the lower
 *     local state -- bit j <-> the j-th hidden spin of the row, ascending, a set bit = spin -1 -- so a hidden spin in no term is +1.
 *     gml_conditional_mode: [H][K], hidden-major, the hidden spins ascending.  gml_conditional_mode_masked: [n][K], an observed entry
 *     holding its evidence value; a row without holes is legal and comes back as it is.
 *   energy [K] (or NULL): E_k(s_H*), the row's constant included.
 *   log_p [K] (or NULL): E_k(s_H*) - log_w[k] = log P(x_H = s_H* | x_O), with log_w[k] the same bits gml_conditional_exact[_masked]
 *     returns for that row.  With log_p NULL the device computes no exponential and no second transform; states and energy are the
 *     same bits either way.
 * Determinism.  The promise of gml_conditional_exact: a row's result is a pure function of the model, that row and that row's hidden
 *   set; a mask handle whose rows all equal one vector gives, bit for bit, what gml_conditional_mode gives with that vector.
 * GML_EINVAL and GML_EUNSUPPORTED: the cases of gml_conditional_exact[_masked] in their order, with "states is NULL" in the place of
 *   "all three outputs NULL".
 * Cost.  That of gml_conditional_exact[_masked]; without log_p the chunk phase takes about 0.6 of it.  Measured times in DESIGN 3.20.
 */
int gml_conditional_mode(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, gml_problem *evidence,
                         const uint8_t *hidden /* [n], host */, int8_t *states /* [H][K], hidden-major, hidden spins ascending */,
                         double *energy /* [K] or NULL */, double *log_p /* [K] or NULL */);
int gml_conditional_mode_masked(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                gml_problem *evidence, gml_problem *mask,
                                int8_t *states /* [n][K]; an observed entry holds its evidence value */,
                                double *energy /* [K] or NULL */, double *log_p /* [K] or NULL */);

/*
 * gml_conditional_draw, gml_conditional_draw_masked -- exact draws of every row's hidden spins from P(x_H | x_O), no chain and no
 * burn-in: the enumeration of gml_conditional_mode[_masked] on energies perturbed by Gumbel noise (Gumbel-max: the state of largest
 * E(s) + G(s), G i.i.d. standard Gumbel, is a draw from softmax(E)).  The yardstick for the draws of the conditional chains, and the
 * completion step of learning from data with holes.
 * Model, evidence, hidden / mask, E_k, limits: exactly those of gml_conditional_exact and gml_conditional_exact_masked.
 * Chains.  chains = K * replicas.  Chain c = r K + k is replica r of evidence row k, the numbering of gml_conditional_means.
 * States.  Row k hides h_k <= 24 spins.  Local state s in [0, 2^h_k): bit j <-> the j-th hidden spin of the row, ascending; a set bit =
 *   spin -1.
 * Energy.  E_k(s) is that of gml_conditional_exact, over all terms, with the FP64 weights as given.
 * Perturbation.  u = u01(seed, c, s) of gml_rng.h (stream = c, counter = s); g = -log(-log u) in FP64, u = 0 gives -inf;
 *   key(c, s) = E_k(s) + g.
 * Draw.  The draw of chain c is the state of largest key; equal keys go to the lower state (the order of the mode).
 * A hidden spin in no term is a coin flip here (both of its values have the same energy and their own g), where the mode makes it +1.
 * A row without a hidden spin (masked form) comes back as it is, with energy E(row) and log_p 0.
 * Exactness.  Exact up to the 53 bits of u: g <= -log(-log(1 - 2^-53)) = 36.74, so a state whose probability is below about 2^-53 of
 *   the mode's can never be drawn; every other state is drawn with its probability up to that resolution.
 * Outputs, per chain (host).
 *   states: the values (+-1) of the hidden spins in the draw.  gml_conditional_draw: [H][K * replicas], hidden-major, the hidden spins
 *     ascending.  gml_conditional_draw_masked: [n][K * replicas], an observed entry holding its evidence value.
 *   energy [K * replicas] (or NULL): the UNPERTURBED E_k of the drawn state, the row's constant included.
 *   log_p [K * replicas] (or NULL): energy - log_w[k] = log P(x_H = the draw | x_O), with log_w[k] the same bits
 *     gml_conditional_exact[_masked] returns for that row.  With log_p NULL the device computes no exponential of the sums and no
 *     second transform; states and energy are the same bytes either way.
 * Determinism.  A chain's result is a pure function of (model, row k's bits, its hidden set, seed, c): not of the grid, the other rows,
 *   the slab, how the replicas of a row were batched, or which outputs were asked for; the same bytes on every call.  A mask handle
 *   whose rows all equal one vector gives, byte for byte, what gml_conditional_draw gives with that vector.
 * GML_EINVAL and GML_EUNSUPPORTED: the cases of gml_conditional_mode[_masked] in their order, with replicas < 1 after "states is NULL".
 * Cost.  That of gml_conditional_mode[_masked] per row and distinct hidden set (planning is per hidden set, not per replica), plus one
 *   hash and two FP64 logarithms per state and replica; eight replicas of a row share one pass over its states.  Measured times in
 *   DESIGN 3.21.
 */
int gml_conditional_draw(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, gml_problem *evidence,
                         const uint8_t *hidden /* [n], host */, int replicas, uint64_t seed,
                         int8_t *states /* [H][K * replicas], hidden-major, hidden spins ascending */,
                         double *energy /* [K * replicas] or NULL */, double *log_p /* [K * replicas] or NULL */);
int gml_conditional_draw_masked(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                gml_problem *evidence, gml_problem *mask, int replicas, uint64_t seed,
                                int8_t *states /* [n][K * replicas]; an observed entry holds its evidence value */,
                                double *energy /* [K * replicas] or NULL */, double *log_p /* [K * replicas] or NULL */);

/*
 * gml_problem_create_sampled_hist -- sample AND histogram on the device: what `sample(gm, N)` returns is the countmap of the
 * draws (sampling.jl:52-54: one row per distinct configuration, column 1 = its count).  Same term-list arguments as above
 * (mcmc_sweeps = 0: exact sampling, > 0: Glauber chains); n <= 64, N < 2^31.  The N draws become 64-bit keys, are radix-sorted
 * and run-length encoded on the device, and the handle holds the K' <= min(N, 2^n) DISTINCT configurations (ascending key
 * order: bit i of the key <=> spin i is -1) with their multiplicities as counts, M = N.  A 9-spin model sampled 1e8 times
 * gives a 512-row handle, and learn() on it costs 512 rows, not 1e8.
 */
int gml_problem_create_sampled_hist(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                    int64_t N, uint64_t seed, int mcmc_sweeps, int order, int64_t node0, int64_t node1,
                                    int device, gml_problem **out);

/* The counts of a handle's K rows (host pointer, K doubles): column 1 of the histogram (sampling.jl:54).  A handle created from
 * integer counts returns them exactly (M <= 2^50); fractional counts come back rounded to 1e-6. */
int gml_problem_get_counts(gml_problem *p, double *counts);

/*
 * gml_problem_moments, gml_problem_term_moments -- the exact sample moments of a handle, computed on the device from its sign bits
 * (a product of spins is the XOR of their sign rows, a sum over configurations a population count; gml_moments.hip).  Host
 * pointers.  With c_k the count of row k and s_ki = +-1:
 *   sum1[i]    = sum_k c_k s_ki                         [n]
 *   sum2[i][j] = sum_k c_k s_ki s_kj                    [n][n] row-major, the full symmetric matrix, diagonal = M; NULL: not computed
 *   sums[t]    = sum_k c_k prod_{i in key t} s_ki       [nterms]
 * keys as everywhere in this header: spins of term t = keys[t*key_stride .. +key_stride), 0-based, -1 = unused slot, any
 * key_stride >= 1 (no limit on the order); a spin named twice in a key cancels (s^2 = 1); the empty key gives M.  The moments are
 * these sums divided by M (gml_problem_info).  They do not depend on the handle's order or node range (every handle holds all n
 * spins), and padding rows contribute nothing.
 * Exactness: for a handle whose counts are all integers and whose M <= 2^50, every output is the exact integer above -- all sums
 * are integer additions, so the result does not depend on the kernels' tiles, their split over K, the grid or the device.  Every
 * sampled handle (exact, Glauber, both chain kinds, histogram or not) and every histogram with integer counts (the reference's
 * Matrix{Int64}) is such a handle; whether the counts were integers is decided from the caller's values when the handle is
 * created, on every creation route.  (The device keeps w_k = c_k / M; M <= 2^50 is what makes rint(w_k M) = c_k: two roundings of
 * relative 2^-53 each stay below 1/2.)  gml_problem_get_counts returns the counts of such a handle exactly.
 * Cost: sum2 is a binary GEMM on the vector ALU, n^2 / 2 pairs x K bits as xor + popcount; handles whose counts are not all equal
 * (histograms) run it once per bit of the largest count -- the cost grows with log2(max c_k), acceptable because a histogram
 * handle has few rows.  sum1 and the term sums stream (key length) x K / 8 bytes per term.  Device memory beyond the outputs
 * (8 n^2 bytes for sum2): the count planes (K / 8 bytes per bit of the largest count) and the reduced keys; all of it is released
 * before the call returns.
 * GML_EINVAL (checked before any device work): NULL p / sum1 / keys / sums, key_stride < 1, nterms < 0, a spin outside [0, n)
 * (the text names the term).  nterms = 0 is a no-op.  GML_EUNSUPPORTED: a handle created with a fractional count, or M > 2^50 (the
 * text says which); there is no floating-point fallback.  Handles of gml_multi are not covered.
 */
int gml_problem_moments(gml_problem *p, int64_t *sum1 /* [n] */, int64_t *sum2 /* [n][n] row-major, or NULL */);
int gml_problem_term_moments(gml_problem *p, const int32_t *keys, int key_stride, int64_t nterms, int64_t *sums /* [nterms] */);

/*
 * gml_problem_fold_sizes, gml_problem_split -- a resident handle split into folds on the device (cross-validation; gml_split.hip).
 *
 * The definition.  The handle's M samples are its UNITS: configuration k (the handle's row order) with the integer count c_k owns
 * the units g = C_k .. C_k + c_k - 1, C_k = c_0 + .. + c_(k-1).  Unit g belongs to fold
 *     min(nfolds - 1, (int)floor(nfolds * u01(seed, kU01FoldStream, g)))
 * with u01 the samplers' counter hash (gml_rng.h: splitmix64 of seed + kU01Step (g + 1) + kU01Stream (stream + 1), top 53 bits) and
 * kU01FoldStream = 0x8000000000000000: the samplers count their streams up from 0, so a handle sampled with seed s and split with
 * seed s shares no draw with its sampler.  The labels depend on (seed, nfolds, g) alone -- not on a launch shape, the device or the
 * order of a reduction (integer tallies throughout).
 *
 * gml_problem_fold_sizes: sizes[f] = the number of units in fold f (host pointer, nfolds values; they sum to M).
 * gml_problem_split: *out = a NEW handle, independent of p (p may be destroyed first), on p's device, with p's order and node range.
 * It holds exactly the configurations with a positive new count c'_k, in source order, where c'_k = the units of k whose fold ==
 * `fold` (complement = 0: the held-out part) or != `fold` (complement != 0: the training part); M' = sum c'_k.  The handle is
 * indistinguishable from gml_problem_create_packed(bits', counts', K'): the same sign words (bits of the rows >= K' zero), weights,
 * summaries and bit images, hence bit-identical results from every call.  The held-out and the training part of one (nfolds, fold,
 * seed) partition the source's counts.
 * GML_EINVAL (checked before any device work): NULL p / sizes / out, nfolds outside [2, 64], fold outside [0, nfolds); and, from the
 * split itself, an empty part (M' = 0; the text names the fold).  GML_EUNSUPPORTED: a handle created with a fractional count, M >=
 * 2^40 (the work is per unit), K >= 2^31 - 1.  Handles of gml_multi are not covered.
 * Cost: one hash per unit (a wave per configuration, its lanes striding over the units), two scans over K, and the compaction of
 * the sign bits, which reads n K / 8 and writes n K' / 8 bytes; then the bit images of the new handle, as for every creator.
 */
int gml_problem_fold_sizes(gml_problem *p, int nfolds, uint64_t seed, int64_t *sizes /* [nfolds] */);
int gml_problem_split(gml_problem *p, int nfolds, int fold, uint64_t seed, int complement, gml_problem **out);

/* The +-1 configurations held by a handle, K x n row-major (host pointer). */
int gml_problem_get_spins(gml_problem *p, int8_t *spins);

void gml_problem_destroy(gml_problem *p);

/* Device blocks of >= 1 MB that handles and solves release are kept by the library, per device and size, for the next handle of the
 * same shape (up to a quarter of the device's memory; an allocation that fails empties the cache and tries again): on MI355X /
 * ROCm 7 a hipMalloc of a multi-GB block after a hipFree sporadically takes 0.4-1.3 s, several times the headline solve.
 * gml_trim_cache() returns all of it to the driver; the return value is the number of bytes released. */
int64_t gml_trim_cache(void);
/* Cap of that cache in bytes per device: 0 = keep nothing (every release goes back to the driver: for processes that share a GPU
 * with other allocators -- a framework's caching allocator, other ranks), < 0 = the default, a quarter of the device's memory.
 * When a release does not fit, the blocks released longest ago are returned to the driver first. */
void gml_set_cache_limit(int64_t bytes_per_device);

/* sizes: n, K (rows given), M = sum(counts) (:79), P = parameters per node
 * (n for order 2; sum_{p<=order} C(n-1,p-1) in general), local node range */
int gml_problem_info(const gml_problem *p, int64_t *n, int64_t *K, double *M, int64_t *P,
                     int64_t *node0, int64_t *node1);

/* lambda = c*sqrt(log(n^2/0.05)/M)  (:157; identical at :86, :213, :266, :304) */
double gml_lambda(double c, int64_t n, double M);

/* Multi-body keys of node u in the reference's construction order (:94-104 with
 * models.jl:228-246): P rows of `order` int32 (0-based spin ids, -1 = unused slot). */
int gml_multi_keys(const gml_problem *p, int64_t u, int32_t *keys);

/*
 * gml_objgrad_batch -- the operator boundary.  Replaces the pair the reference registers
 * with JuMP, `obj(x...)` / `grad(g, x...)` = risea_obj / grad_risea_obj (:191-208, :221-233),
 * for many nodes at once, and the @NLobjective smooth parts of logRISE (:278-281) and
 * RPLE (:316-319).
 *
 *   nodes[r]        node id (0-based, any node, repeats allowed), r < nrows
 *   theta[r*ld + j] parameter j of row r in the REFERENCE's layout: pairwise -> j = spin
 *                   index, slot j == nodes[r] is the field (the u-th column of nodal_stat
 *                   is s_u, :162); multi-body -> j indexes gml_multi_keys(nodes[r]).
 *   f[r]            smooth objective (no l1 term)
 *   g[r*ld + j]     its gradient, same layout as theta
 * One "node evaluation" = one row.
 *
 * Sparse rows are cheaper: the forward GEMM of a 32-row node tile sweeps only the statistics columns on which one of its rows is
 * non-zero (the compact column list and the bit image of those columns are built on the device in front of the pass; lists longer than
 * a quarter of the columns sweep everything).  The sums are the same integers, so f and g are the same bits as a sweep over all columns; a
 * pass at rows with ~15 non-zeros of 1024 costs 7.7 ms instead of 10.7 (headline size, precision i8w).
 *
 * theta, f and g are host pointers, or -- all three -- DEVICE pointers on the handle's GPU (detected): rows that live in HBM (a
 * device-side optimiser, torch / CuPy / Julia GPU arrays) are scattered into the internal layout, evaluated and gathered back by
 * kernels, with no staging copy and nothing crossing PCIe but the control block and two small per-row arrays (headline pass
 * n = 1024, K = 1e6: 10.4 ms instead of 13.4 through host pointers; the same bits either way).  `nodes` is a host array in both
 * forms.  Ordering: the kernels run on the handle's own stream, a blocking stream -- ordered after everything the caller enqueued on
 * the device's null stream (torch's default stream) before the call; work on other streams must have completed.  The call returns
 * when f and g are written.
 */
int gml_objgrad_batch(gml_problem *p, int formulation, int precision, int64_t nrows,
                      const int64_t *nodes, const double *theta, int64_t ld, double *f,
                      double *g);

/*
 * gml_hessvec_batch -- beyond the reference (whose registered operator is first-order, :221-233, so Ipopt falls back
 * to a limited-memory Hessian there): the curvature operator  hv[r] = Hess f_{nodes[r]}(theta[r]) * vec[r]  for
 * second-order / Newton-CG external solvers, same layouts as gml_objgrad_batch.  Two GEMM passes on the int8 matrix
 * cores with the curvature weights of an objective pass at theta (precision i8x; ~1e-8 relative).  This is the
 * operator gml_learn's matrix-free Newton-CG uses for working sets above max_working.
 * theta, vec and hv: host pointers, or all three device pointers (as gml_objgrad_batch).
 */
int gml_hessvec_batch(gml_problem *p, int formulation, int64_t nrows, const int64_t *nodes, const double *theta,
                      const double *vec, int64_t ld, double *hv);
/* The same with the arithmetic named: GML_PREC_I8X (what gml_hessvec_batch runs; GML_PREC_AUTO means this), or GML_PREC_F64 --
 * both passes on the FP64 matrix cores (an objective pass at theta, then U_k = h_k (x_k . vec) formed in place of its weights and
 * contracted by the same backward GEMM): the curvature operator at the accuracy of the reference's Float64 arithmetic (1e-12
 * against a dense numpy Hessian, tests/test_gpu_operator_export.py), for external second-order solvers that want their Hessian
 * as good as their gradient; ~10x the time of the int8 form.  GML_PREC_I8W: GML_EUNSUPPORTED (the Hessian-vector forms read
 * 31-bit curvature weights whatever the objective pass wrote). */
int gml_hessvec_batch_prec(gml_problem *p, int formulation, int precision, int64_t nrows, const int64_t *nodes, const double *theta,
                           const double *vec, int64_t ld, double *hv);

/*
 * gml_learn -- replaces learn(samples, formulation, method) for the handle's node range
 * (:154-189 RISE, :263-298 logRISE, :301-336 RPLE, :210-260 RISEA, :83-133 multiRISE up to
 * the per-node solve).  For every local node it minimises
 *     f_u(x) + lambda * sum_{j penalised} |x_j|
 * (the problem the reference hands to Ipopt through the z >= |x| epigraph, :166-181).
 *
 *   out   (node1-node0) x P, row-major: row r = solution of node node0+r in the reference's
 *         layout (pairwise: reconstruction[u, 1:n] of :181, diagonal slot = field).
 *         May be a host pointer or a device pointer (detected).
 *   kkt   optional (node1-node0) host array: final max|pseudo-gradient| per node.
 * Symmetrisation (:184-186, :135-149) needs all rows: handles over all nodes take gml_learn_matrix / gml_learn_terms (solve and
 * result assembly in one call, on the device), node shards gather their rows and call gml_matrix_symmetrize / gml_terms_assemble.
 * Returns GML_ENOTCONV if some node stayed above opts->tol (out is still filled).
 * Ordering, for gml_learn and every gml_learn_* below: the solve runs on the handle's own stream, a blocking stream -- ordered after
 * everything the caller enqueued on the device's null stream before the call (a device x0 / structure / out written or filled there);
 * work on other streams must have completed.  The call returns when out (terms) and kkt are written and that stream is idle.
 */
int gml_learn(gml_problem *p, int formulation, double regularizer_c, const gml_opts *opts,
              double *out, double *kkt, gml_stats *stats);

/*
 * gml_learn_warm -- gml_learn from a starting point instead of x = 0: x0 = (node1-node0) x P rows in the layout of `out` (host or
 * device pointer; NULL = zeros = gml_learn).  The optimum does not depend on it (the problems are convex); the number of iterations
 * does.  For regularisation paths -- the same samples solved at a sequence of c, each from the previous solution (the reference
 * re-solves from scratch: JuMP start values are never set, :166-167) -- and for re-solves after more samples arrived.
 * out may be x0 itself.
 */
int gml_learn_warm(gml_problem *p, int formulation, double regularizer_c, const gml_opts *opts, const double *x0, double *out,
                   double *kkt, gml_stats *stats);

/*
 * gml_learn_structured -- gml_learn_warm with the STRUCTURE of every row stated by the caller (beyond the reference, whose only
 * structure is "the field free, every other parameter penalised", :118, :171): which parameters exist, and which of those carry the
 * l1 penalty.  For refits on a learned support (threshold the l1 solution, re-estimate the kept couplings without the shrinkage), for
 * known graphs (a lattice, a chip's couplers, no external fields) and for partly known models (known couplings free, the rest
 * l1-screened).
 *   structure[r*ld_s + j]   kind of parameter slot j of local row r (node node0 + r), in the layout of `out` (pairwise: slot j = spin
 *                           j, slot u = the field; multi-body: the order of gml_multi_keys, slot 0 = the field); ld_s >= P.  Host
 *                           pointer, or device pointer on the handle's GPU (detected, as x0 and out are).  NULL = gml_learn_warm.
 * Any kind is allowed in any slot, the field included (every field GML_PARAM_EXCLUDED: a zero-field model).  x0, out, kkt and stats
 * as in gml_learn_warm; entries of x0 at excluded slots are ignored (taken as 0), out is exactly 0.0 at every excluded slot, kkt[r] is
 * the max |pseudo-gradient| over the slots that are not excluded.  A row without any parameter is complete before the first
 * iteration: x = 0, kkt = 0, converged.  Sparse structures are cheap: the passes sweep only the non-zero columns of a node tile.
 * GML_EINVAL: ld_s < P, or a value outside {0, 1, 2} (the text names row and slot; a host array is checked before any device work, a
 * device array by a kernel in front of the solve).
 */
#define GML_PARAM_EXCLUDED 0   /* fixed at 0: not a parameter of this row               */
#define GML_PARAM_FREE 1       /* estimated, not penalised (as the field is today)      */
#define GML_PARAM_PENALISED 2  /* estimated, lambda |x| (as every coupling is today)    */
int gml_learn_structured(gml_problem *p, int formulation, double regularizer_c, const gml_opts *opts, const uint8_t *structure,
                         int64_t ld_s, const double *x0, double *out, double *kkt, gml_stats *stats);

/*
 * gml_stderr -- standard errors of solved rows (beyond the reference, which returns point estimates only): the M-estimator
 * ("sandwich") covariance of every local node's solve, computed on the device from the handle's sign bits and weights.  For local row
 * r = node u with solution x on its support S, s_k the reference's statistic vector of configuration k (`nodal_stat[k, :]`, :162;
 * multi-body :106-108), a_k = x . s_k, w_k = count_k / M, every sum over ALL K configurations (no sub-sample):
 *     Cov(x_S) ~ A^-1 B A^-1 / M,   se_j = sqrt of its diagonal
 *     A = sum_k w_k phi''(a_k) s_k s_k^T (the Hessian on S),   B = sum_k w_k psi_k psi_k^T - m m^T,   m = sum_k w_k psi_k
 *     RISE     phi'' = e_k = exp(-a_k);                 psi_k = -e_k s_k
 *     RPLE     phi'' = 4 sg_k (1 - sg_k), sg_k = 1 / (1 + exp(-2 a_k));   psi_k = -2 (1 - sg_k) s_k
 *     logRISE  A = (sum w e s s^T) / Z - gb gb^T, Z = sum w e, gb = grad log Z = -(sum w e s) / Z;   psi_k = -(e_k / Z)(s_k + gb), m = 0
 *   x          (node1-node0) x P rows in the layout of gml_learn's `out`, leading dimension ld >= P
 *   structure  as in gml_learn_structured (ld_s >= P); NULL = the reference's: the field free, the rest penalised.  The support of a
 *              row is every GML_PARAM_FREE slot (also at x = 0) plus every GML_PARAM_PENALISED slot with x != 0
 *   se         (node1-node0) x P, leading dimension ld: se_j at the slots of the support, 0.0 at every other slot
 *   status     host, [node1-node0], may be NULL: GML_SE_OK; GML_SE_SINGULAR -- a pivot of the Cholesky of A is not above 1e-13 x the
 *              largest diagonal entry of A (duplicated or constant statistics in the support): the se of that row's support is NaN;
 *              GML_SE_TOO_LARGE -- a support of more than 512 entries (gml_opts.max_working's ceiling): NaN likewise.  Other rows are
 *              not affected.  A row with an empty support: se = 0, GML_SE_OK
 *   times      host, [3], may be NULL: seconds spent on the support lists, the Gram sweep, the factorisations
 * x, se and structure: host pointers or device pointers on the handle's GPU, each detected on its own.
 * Ordering: the kernels run on the handle's own stream, a blocking stream -- ordered after what the caller enqueued on the device's null
 * stream before the call; the call returns when se and status are written and that stream is idle.
 * What the numbers mean, and what they do not:
 *   - with penalised active coordinates this is the covariance CONDITIONAL on the selected support and signs, not a post-selection
 *     valid interval; the intended use is after a refit (gml_learn_structured on the kept support), where every parameter is FREE;
 *   - the M samples are taken as independent draws: thinned-chain output with residual autocorrelation makes the se optimistic;
 *   - covariances between the rows of different nodes are not computed, so there is no exact se of a symmetrised coupling
 *     (x_uv + x_vu) / 2; (se_uv + se_vu) / 2 bounds it from above whatever the correlation;
 *   - the reference has nothing comparable: tests/_sandwich_reference.py (dense numpy) is the yardstick.
 * The result does not depend on the handle's node range, on host or device pointers, or on what else the call computes: the
 * partial sums of a row are combined in a fixed order that depends on the row's support size and K only.
 * GML_EINVAL, before any device work: NULL p / x / se, ld < P, ld_s < P, an unknown formulation, a structure byte outside {0, 1, 2}
 * or a non-finite x in a host array (device arrays are checked by the kernels that read them).  GML_EINVAL after the lists are built: a
 * non-zero x at a GML_PARAM_EXCLUDED slot (the text names row and slot).  GML_EUNSUPPORTED: logRISE / RPLE on a multi-body handle.
 */
#define GML_SE_OK 0
#define GML_SE_SINGULAR 1
#define GML_SE_TOO_LARGE 2
int gml_stderr(gml_problem *p, int formulation, const double *x, int64_t ld, const uint8_t *structure, int64_t ld_s,
               double *se, int32_t *status, double *times);

/*
 * Structures for gml_learn_structured, built on the device in the (node, slot) layout of the rows (closed-form for multi-body models:
 * no key table).  `structure` is n x P bytes with leading dimension ld_s >= P, host or device pointer; bytes [P, ld_s) of a row are
 * not written.  `device`: where the kernels run when no argument is a device pointer.
 * Ordering (gml_structure_from_rows, gml_structure_from_keys): the kernels run on the device's NULL stream -- ordered after what the
 * caller enqueued there before the call; the call returns when structure (and kept) are written and the null stream is idle.
 *
 *   gml_structure_from_rows   from solved rows: rows = the n x P solved rows of all nodes (leading dimension ld, host or device
 *                             pointer; for order 2 also the symmetrised n x n matrix).  A non-field slot (u, S') -- the key S = {u} + S'
 *                             -- gets kind_keep or kind_drop by `rule`:
 *                               GML_RULE_ROW    keep iff |rows[u][slot]| >= threshold
 *                               GML_RULE_MEAN   keep iff |mean over v in S of row v's entry for (v, S \ {v})| >= threshold; the mean is
 *                                               formed as gml_terms_assemble forms it (added in ascending v, then / |S|), so the decision
 *                                               is bit-consistent with thresholding the assembled model
 *                               GML_RULE_ALL    keep iff every member's entry is >= threshold in magnitude ("AND")
 *                               GML_RULE_ANY    keep iff some member's entry is ("OR")
 *                             (MEAN, ALL, ANY decide per key: all |S| slots of a key get the same kind.)  A NaN compares false: dropped.
 *                             Field slots get kind_field and are never thresholded.  kept (host, may be NULL): the exact number of
 *                             non-field (u, slot) entries that got kind_keep.
 *                             GML_EINVAL (before any HIP call): NULL rows / structure, order < 1, an unknown rule or kind, threshold
 *                             negative or not finite, ld < P or ld_s < P.
 *   gml_structure_from_keys   from a list of terms: keys as everywhere in this header (host, term t = keys[t*key_stride ..
 *                             +key_stride), 0-based, -1 = unused slot).  Every slot starts as kind_other, the fields as kind_field;
 *                             a key S with 2 <= |S| <= order sets, for every member u, row u's slot of (u, S \ {u}) to kind_listed; a
 *                             key of one spin sets that spin's field to kind_listed.  Duplicate keys are harmless, nterms = 0 is allowed.
 *                             GML_EINVAL (before any HIP call): NULL structure (or keys with nterms > 0), key_stride < 1, an unknown
 *                             kind, ld_s < P, a spin outside [0, n), a spin named twice in one key (a structure key is a set), a key
 *                             of more than `order` spins or of none; the text names the term.
 */
#define GML_RULE_ROW 0
#define GML_RULE_MEAN 1
#define GML_RULE_ALL 2
#define GML_RULE_ANY 3
int gml_structure_from_rows(const double *rows, int64_t ld, int64_t n, int order, int rule, double threshold, int kind_keep,
                            int kind_drop, int kind_field, int device, uint8_t *structure, int64_t ld_s, int64_t *kept);
int gml_structure_from_keys(const int32_t *keys, int key_stride, int64_t nterms, int64_t n, int order, int kind_listed, int kind_other,
                            int kind_field, int device, uint8_t *structure, int64_t ld_s);

/*
 * Result assembly of multiRISE on the device -- replaces the tail of learn(samples, ::multiRISE, ...): the per-node
 * `reconstruction[inter] = ...` (:129-132), the symmetrisation (group by sorted key, `mean`: :135-149) and the Dict that
 * FactorGraph(order, n, :spin, reconstruction) (:151, models.jl:8-17) is built from.  The terms of the learned model are returned
 * as ONE array of weights in the order the reference itself lists a model's terms in (models.jl:61,72: `sort(..., by = x ->
 * (length(x), x))`), so no key table exists anywhere; a key <-> its position is closed-form (combinatorial number system):
 *   symmetrize != 0   every ascending key S with |S| <= order: by size, lexicographic within a size; C(n,1) + ... + C(n,order)
 *                     weights, each the mean over u in S of row u's entry for (u, S \ {u}), added in ascending u
 *   symmetrize == 0   every key (u, S'), S' an ascending subset of the other spins: by size, then u, then S'; n P weights
 *
 *   gml_terms_count     number of terms (-1: unsupported order / overflow)
 *   gml_terms_assemble  rows: the n x P solved rows (row u in the layout of gml_learn's `out`, leading dimension ld), host OR device
 *                       pointer; out: gml_terms_count doubles, host OR device pointer.  One kernel launch on `device` (on the
 *                       device that holds rows / out when one of them is a device pointer); host rows are staged through it.
 *                       Ordering: it runs on the device's NULL stream -- ordered after what the caller enqueued there before the
 *                       call; the call returns when out is written and the null stream is idle
 *   gml_terms_keys      host only: the keys of the terms [first, first + count), `order` int32 per term, 0-based spins, -1 = unused
 *   gml_terms_rank      host only: position of a key of `len` spins (0-based), -1 if the model has no such key
 *   gml_learn_terms     gml_learn over ALL nodes of the handle + the assembly, the rows never leaving the device: `terms` (host or
 *                       device pointer) receives the term array; kkt, stats as gml_learn (stats->t_assemble = the assembly).
 *                       GML_EINVAL for a handle over a node sub-range (gather the rows, then gml_terms_assemble).
 *                       C5 (n = 512, order 3): 67.0 M row entries -> 22.5 M terms (179 MB) in one launch.
 */
int64_t gml_terms_count(int64_t n, int order, int symmetrize);
int gml_terms_assemble(const double *rows, int64_t ld, int64_t n, int order, int symmetrize, int device, double *out);
int gml_terms_keys(int64_t n, int order, int symmetrize, int64_t first, int64_t count, int32_t *keys);
int64_t gml_terms_rank(int64_t n, int order, int symmetrize, const int32_t *key, int len);
int gml_learn_terms(gml_problem *p, int formulation, double regularizer_c, int symmetrize, const gml_opts *opts, double *terms,
                    double *kkt, gml_stats *stats);

/*
 * The pairwise counterpart: `reconstruction = 0.5 * (reconstruction + transpose(reconstruction))` (:184-186) on the device.
 * On the host that one line walks the transposed operand with a stride of n doubles: 16 ms at n = 1024 (a sixth of the headline
 * solve), 0.22 s at n = 4096 (as much as a whole config-4 solve on eight GPUs).  (a + b) * 0.5 in FP64: the same bits.
 *   gml_learn_matrix        gml_learn over ALL nodes of a pairwise handle + the symmetrisation (symmetrize != 0), the rows never
 *                           leaving the device: out = the n x n matrix the reference's learn returns (host or device pointer);
 *                           stats->t_assemble = the symmetrisation + the copy.  symmetrize == 0: plain gml_learn.
 *   gml_matrix_symmetrize   the same for rows gathered from node shards: rows n x n (leading dimension ld), out n x n, host or
 *                           device pointers, in place allowed.  Ordering: it runs on the device's NULL stream -- ordered after what
 *                           the caller enqueued there before the call; the call returns when out is written and that stream is idle
 */
int gml_learn_matrix(gml_problem *p, int formulation, double regularizer_c, int symmetrize, const gml_opts *opts, double *out,
                     double *kkt, gml_stats *stats);
int gml_matrix_symmetrize(const double *rows, int64_t ld, int64_t n, int device, double *out);

/*
 * gml_multi_* -- the node loop of `learn` (:161: `for current_spin = 1:num_spins`, rows stored at :181) over several
 * GPUs of one node from a single caller (the reference's host language has no process group: Julia's
 * `learn(samples, RISE(), HIP(devices = 0:7))` binds these).  GPU g owns the nodes [g n / G, (g+1) n / G): one handle and
 * one host thread per device, the sample bits replicated, no communication while solving.
 *
 *   gml_multi_create   as gml_problem_create, for the devices listed (a device may be listed more than once): the matrix
 *                      is packed ONCE on the host and each chunk of sign bits is copied to every device while the next
 *                      one is being packed (C4: 0.5 GB per GPU instead of 32.8 GB per GPU)
 *   gml_multi_learn    out: n x P row-major host matrix (may be NULL), rows written by the part that owns them; kkt: n.
 *                      dev_out: NULL, or one device pointer per part (n x P doubles on that part's GPU): the full
 *                      matrix is left on EVERY GPU by one RCCL all-gather over xGMI (librccl is loaded at run time;
 *                      peer copies when it is absent, the device list repeats a GPU, or n is not a multiple of G).
 *                      stats: totals over the parts, times of the slowest part.
 *                      With dev_out every part writes its rows device to device into its own block of dev_out[g]
 *                      (nothing returns to the host on the way) and the all-gather runs in place.
 *   gml_multi_info     gather_kind (>= 32 bytes or NULL): how the last dev_out gather was done
 *                      ("rccl-allgather", "peer-copy", "host" when none was asked for)
 *   gml_multi_part_stats  parts: ndev gml_stats, the statistics of every part of the last gml_multi_learn (iterations,
 *                      node evaluations, t_total ...): exposes stragglers among the node shards
 */
typedef struct gml_multi gml_multi;
int gml_multi_create(const void *samples, int dtype, int64_t K, int64_t n, int64_t ld, int col_major, int order,
                     const int *devices, int ndev, gml_multi **out);
int gml_multi_info(const gml_multi *m, int64_t *n, int64_t *K, double *M, int64_t *P, int *ndev, char *gather_kind);
int gml_multi_learn(gml_multi *m, int formulation, double regularizer_c, const gml_opts *opts, double *out, double *kkt,
                    gml_stats *stats, double **dev_out);
int gml_multi_part_stats(const gml_multi *m, gml_stats *parts);
/* diagnostics of the collective path, as text (nbuf >= 160 holds it): whether librccl was loaded, whether ncclCommInitAll succeeded
 * (with ncclGetErrorString's text when not) and which path the last dev_out gather took */
int gml_multi_diag(const gml_multi *m, char *buf, int nbuf);
void gml_multi_destroy(gml_multi *m);

/* Timing hook for the benchmark: runs `steps` full objective+gradient passes over the local
 * nodes at the given theta ((node1-node0) x P, reference layout, host) on the handle's
 * stream and returns the average device time of the dominant kernels measured with HIP
 * events.  kernel_ms[0] = forward (energies + pointwise), [1] = backward (gradient),
 * [2] = whole pass. */
int gml_bench_pass(gml_problem *p, int formulation, int precision, const double *theta,
                   int steps, int warmup, double kernel_ms[3]);

/* The same with Theta resident in HBM: uploaded once, then warmup + steps passes back to back without host round
 * trips (how a device-side optimiser would drive the operator); f ((node1-node0)) and g ((node1-node0) x P) of the
 * last pass are returned if not NULL.  kernel_ms[3] = device time per pass; step_ms (steps doubles, or NULL) = the
 * device time of every timed pass. */
int gml_bench_pass_resident(gml_problem *p, int formulation, int precision, const double *theta, int steps,
                            int warmup, double kernel_ms[4], double *f_out, double *g_out, double *step_ms);

#ifdef __cplusplus
}
#endif
#endif /* GML_H */
