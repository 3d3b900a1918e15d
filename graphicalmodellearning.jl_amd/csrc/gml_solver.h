// Interface between the host solver (gml_solver.cpp, gml_newton_cg.cpp) and its device kernels (gml_solver.hip).
#pragma once
#include "gml_dev.h"

#include <atomic>
#include <vector>

namespace gml {

struct SelectOut {
    double l1;     // lambda * sum |x_c| over the penalised columns
    double worst;  // KKT residual: max |pseudo-gradient|
    double worstW; // the same over the current support
    int m;         // working-set size (Cholesky row), or -|W| for a matrix-free (Newton-CG) row
    int nsupp, nviol;
    int pad;
};
// (test hook, gml_testhooks.cpp) the Hessian-vector products of few live rows go entry by entry when the sum of their working-set
// sizes is below this multiple of (statistics columns x node tiles of the GEMM pass); < 0: never
extern double g_hv_sparse_ratio;
extern std::atomic<long long> g_hv_sparse_calls; // products taken entry by entry so far (all solves of the process)
// experiment knobs (gml_test_tune; 0 = the built-in rule): what scripts/gpu_tune_*.py sweep, not an interface.  Tests and the benchmark
// address the knobs by number, so an index never moves: 3 belonged to an experiment that was removed and stays reserved (unused)
enum { GML_TUNE_KH_BASE = 0, GML_TUNE_FACE_ROUNDS = 1 /* value - 1 = rounds */, GML_TUNE_HESS_WGS = 2, GML_TUNE_NO_ZERO_SHORTCUT = 4 /* 1: the first pass runs its GEMM like any other */, GML_TUNE_NO_ZEROCOPY = 5 /* 1: results and row lists through device arrays and copies, as on handles too large for the pinned arena */, GML_TUNE_NO_COMPACT = 6 /* 1: the forward GEMMs of objective passes sweep all columns, always (A/B of the column compaction) */, GML_TUNE_BENCH_COMPACT = 7 /* 1: the timing hooks gml_bench_pass* compact too (they sweep all columns by default: the bench headline prices the dense contraction) */, GML_TUNE_SOLVER_COMPACT = 8 /* 1: gml_learn's own passes try the compaction whatever the column count.  By default they do from 4 096 statistics columns on (multi-body problems, thousands of spins: config 5 at c = 1.2 3.5 -> 2.2 s): measured (profiles/r6_compact_ab.txt) -- with the 1 024 columns of the headline problem a node's optimum keeps ~100 noise-level coefficients, a tile's 32 rows cover every column after the third pass: no gain, 1 - 5 % overhead */, GML_TUNE_NO_PAIRS = 9 /* 1: the forward sweep of precision i8w runs dense on plain digit planes in every tile, as it does where a column pair leaves the range of seven digits (gml_i8_pairs.h): the same result bits, so a test can hold the two paths against each other */, GML_TUNE_HESS_BLK_WGS = 10 /* workgroups the k-split of the blocked Hessian kernel aims at (0: 4096), as GML_TUNE_HESS_WGS for the one-workgroup kernel: tests reach long chunks at small shapes */, GML_TUNE_STAGE_SPINS = 11 /* > 0: fill_sign_bits (gml_ingest.cpp) stages at most this many spins per chunk of its pinned pipeline instead of what the stage holds, and nothing else changes: tests reach many chunks, and chunks of fewer than 32 spins, at small shapes */, GML_NTUNE = 16 };
extern double g_tune[GML_NTUNE];
extern std::atomic<long long> g_fill_chunks; // (test hook) stages the last fill_sign_bits of the process went through (gml_ingest.cpp)

// (test hook, gml_testhooks.cpp: gml_test_traj_*) the record of a solve's outer iterations: what the host logic of gml_solver.cpp decided,
// step by step, for tests/test_gpu_solver_trajectory.py.  Off by default; while it is armed a solve appends one TrajIter per outer iteration
// (and waits for the stream and downloads to do so -- unarmed, the solver queues nothing more than it would without the recorder).  One
// solve at a time: the record belongs to the last gml_learn of the process that began while it was armed.
enum { // the header of an iteration
    TRH_IT = 0, TRH_NACTIVE, TRH_KH, TRH_KSTRIDE, TRH_HSCALE, TRH_SECANT /* -1: no Cholesky row this iteration */, TRH_FACE_ROUNDS /* in force; -1 likewise */,
    TRH_STALL_CAP, TRH_PREC, TRH_LINE_SEARCH /* 1: the iteration went on to directions and a line search */, TRH_N = 12 };
enum { // per local row (doubles; the integers among them are exact)
    // after select
    TRR_DONE = 0, TRR_ATFLOOR, TRR_KKT, TRR_BEST, TRR_FOBJ, TRR_STALL, TRR_M /* sel.m */, TRR_NSUPP, TRR_NVIOL, TRR_F, TRR_FN, TRR_Z,
    // before the solve (rows that are not done)
    TRR_S1, TRR_YNOISE, TRR_NPAIRS /* after k_secant; -1: the row was in no Cholesky solve */,
    // after the line search
    TRR_TRIALS, TRR_ALPHA /* of the accepting trial; of the last one for a row that was not accepted */, TRR_NREG /* of that trial */,
    TRR_FULL /* the accepting trial was a full pass (0: forward only, its gradient pass followed) */, TRR_ACCEPTED, TRR_GAVE_UP,
    TRR_N = 24 };
// What the matrix-free half of an iteration did (gml_newton_cg.cpp: direction_blocks, newton_cg_group), in order, for tests/test_gpu_newton_cg_trajectory.py:
// a list of events, each a tag, integers and doubles.  n = rows of the event, np = n rounded up to 32, ctl = the control block of the
// product as uploaded (row [np] | node0 + row [np] | plane slot [np] | node tile [np / 32] | 4 unused), rows of vectors are whole rows of Qp.
enum {
    // iv: ncg, T, ntiles, Kh, kstride, Qp, prec, P | cg_rows [ncg] | nW [ncg] | t0 [ncg] | vm [ntiles] | wrow [ntiles] (t0, vm, wrow: the device's
    //     copies) | FV [ntiles T] as k_cg_tiles wrote it | kind [ncg Qp] | mmax [ncg] of the rows' V planes | the column of every parameter
    //     of the result's layout [ncg P]
    // dv: hscale | s1 [ncg] | tau [ncg], the unit of the rows' V planes | X [ncg Qp] | PG [ncg Qp] | G [ncg Qp] | the tile blocks of dH before launch_tile_inverse [ntiles T T] | after
    TRC_BLOCKS = 0,
    // iv: coarse (1) or fine (0), n, maxW | rows [n] | nviol [n] | nsupp [n];  dv: kkt [n] | Z [n]
    TRC_GROUP,
    // iv: where (0 before step 0, 1 at step ci of round 0, 2 before a face re-solve), round, ci, ksub, kchunk, kpart (as the products get
    //     it), nsplit, node tiles the plan was made for, Rp;  dv: wsub | sc [Rp] as uploaded
    TRC_PLAN,
    // iv: round, ci, route (1 entry by entry, 0 GEMM), n, np | live [n] | ctl;  dv: Pv [n Qp] | tau [n], the unit of the rows' V planes | Rv [n Qp] before the step | the raw product Hp [n Qp] | CgState [n 4]
    // after the step
    TRC_STEP,
    // iv: round, n | rows of the round [n];  dv: D [n Qp] after the last step of the round
    TRC_ROUND_END,
    // iv: round, n, nagain | rows of the round [n] | nfixed [n] | again [nagain];  dv: mass [n] | total [n]
    TRC_FACES,
    // iv: round (the one that begins), route, n, np | rows [n] | ctl;  dv: D [n Qp] the product's vector | tau [n] | the raw product Hp [n Qp] |
    // CgState [n 4] after the residual and the first direction
    TRC_RESOLVE
};
struct TrajCgEvent {
    int tag;
    std::vector<int64_t> iv;
    std::vector<double> dv;
};
struct TrajIter {
    double hdr[TRH_N];
    std::vector<TrajCgEvent> cg; // matrix-free rows only (empty: the iteration had none)
    std::vector<double> rows; // [R][TRR_N]
    std::vector<int> F;       // [R][capP]: the working sets as k_select left them (F[0..m) of the Cholesky rows)
    std::vector<double> X;    // [R][Qp]: the iterates after the line search (empty: no line search)
};
struct TrajRecorder {
    bool armed = false;
    int64_t R = 0, Qp = 0;
    int capP = 0;
    std::vector<TrajIter> its;
    std::vector<uint8_t> from_best; // after finish, per row: 1 the result is the best iterate Xb, 0 the last iterate X
};
extern TrajRecorder g_traj;

// the rows' lists of working-set columns (k_cg_tiles): row r's |W| = nw[r] columns, in column order, at FV + t0[r] * T
struct WList {
    const int *FV;
    const long long *t0;
    const int *nw;
    int T;
};

// One Hessian-vector product of the matrix-free rows as the solver calls it (gml_newton_cg.cpp; the test hook gml_test_hv_sparse of
// gml_operator.cpp makes the same call): out = (sum_k h_k x_k x_k^T) vec for the n product rows of the control block ctl (device, laid
// out by cg::HvCtl of gml_cg_rules.h), over the configurations of the plan.  sparse: entry by entry over the rows' lists wl (wcap >= every
// listed size, scratch of i8_hv_sparse_bytes); else the GEMM pass over the slots [0, np) of the workspace *ws.
namespace cg {
struct HvCtl;
}
struct HvPlan {
    int64_t kchunk, kpart;
    int lf, lb; // limbs of the direction in the forward GEMM, of the products in the backward one (GEMM route)
};
int hv_product_call(void **ws, const DevProblem &d, int64_t slot_capacity, int formulation, bool sparse, const cg::HvCtl &L, const int *ctl,
                    const WList &wl, int64_t wcap, void *scratch, const HvPlan &plan, const double *vec, double *out, hipStream_t st,
                    std::string *err);

struct CgState {
    double rs, rs0, pHp, rz;
};
struct FaceOut {
    int nfixed, pad; // coordinates of W whose step left the orthant face (fixed at zero, removed from W)
    double mass;     // their share sum |pg_c (d_c - fixed_c)| of ...
    double total;    // ... sum |pg_c d_c| over W
};
struct TrialOut {
    double dd;    // pg . (xt - x)
    double stepn; // |xt - x|_1
    double l1t;   // lambda * sum |xt_c|
    double back;  // F'(xt; x - xt) (k_back)
};

void launch_kind(const DevProblem &d, int order, const int *dnode, int R, uint8_t *kind, hipStream_t st);
void launch_apply_structure(const uint8_t *S, int64_t ld_s, int64_t R, int64_t P, int64_t Qp, const int *dnode, int64_t cconst, const int32_t *cols,
                            uint8_t *kind, int *nparam, unsigned long long *bad, hipStream_t st);
void launch_mask_x0(const uint8_t *kind, int64_t R, int64_t Qp, double *X, int *bad, hipStream_t st);
void launch_scale_rows(const int *drows, int nrows, const double *dscale, int64_t Qp, double *G, hipStream_t st);
void launch_copy_rows(const int *drows, int nrows, int64_t Qp, const double *s0, double *d0, const double *s1, double *d1, hipStream_t st);
void launch_scale_slots_inv(const int *srow, const int *rowcol, int slot0, int ns, const SlotResult *res, int64_t Qp, double *G, hipStream_t st);
void launch_scale_rows_inv(const int *drows, int nrows, const double *fs, int64_t Qp, double *G, hipStream_t st);
void launch_rows_to_reference(const double *X, int64_t R, int64_t Qp, int64_t P, int64_t node0, int64_t cconst, const int32_t *cols, double *out,
                              hipStream_t st);
void launch_select(const int *drows, int nrows, const double *X, const double *G, const uint8_t *kind, int64_t Qp, double lambda,
                   int max_add, int capW, int capP, double viol_frac, double *PG, int *F, double *gF, double *pgF, SelectOut *out, double *best,
                   double *Xbest, hipStream_t st);
void launch_scatter_dir(const int *drows, int nrows, const int *F, const double *dsol, const int *msz, int capP, int64_t Qp, double *D,
                        hipStream_t st);
void launch_secant(const int *drows, int nrows, const int *F, const int *msz, int cap, const double *X, int64_t Qp, const double *gF, double *H,
                   const long long *hoff, const int *mt, const double *s1, double s2, const double *ynoise, int *Fprev, int *mprev, double *xprev,
                   double *gprev, double *S, double *Y, int *npairs, int64_t pair_stride, int apply_above, hipStream_t st);
void launch_trial(const int *drows, int nrows, const double *X, const double *D, const double *PG, const uint8_t *kind, int64_t Qp,
                  double lambda, const double *alpha, double *Xt, TrialOut *out, double *stepn, hipStream_t st);
void launch_back(const int *drows, int nrows, const double *X, const double *Xt, const double *Gt, const uint8_t *kind, int64_t Qp,
                 double lambda, TrialOut *out, hipStream_t st);
void launch_cg_tiles(const int *drows, int nrows, const double *X, const double *PG, const double *G, const uint8_t *kind, int64_t Qp, int T,
                     const long long *t0, int *FV, double *gV, hipStream_t st);
void launch_tile_apply(int T, const double *Minv, const int *FV, const int *vm, const int *wrow, const int *live, int64_t ntiles, int64_t Qp,
                       const double *Rv, double *Zv, hipStream_t st);
void launch_pcg_init(const int *drows, int nrows, const double *X, const double *PG, const uint8_t *kind, int64_t Qp, double *D, double *Rv,
                     double *Zv, double *Pv, uint8_t *Wm, CgState *cg, hipStream_t st);
void launch_pcg_dir(const int *drows, int nrows, int64_t Qp, const uint8_t *Wm, const double *Rv, const double *Zv, double *Pv, int first,
                    CgState *cg, const WList &wl, hipStream_t st);
void launch_pcg_step(const int *drows, int nrows, const double *G, const uint8_t *Wm, int64_t Qp, const double *s1, double s2, double *Hp,
                     double *D, double *Rv, const double *Pv, CgState *cg, const WList &wl, hipStream_t st);
void launch_pcg_faces(const int *drows, int nrows, const double *X, const double *PG, const uint8_t *kind, int64_t Qp, double *D, uint8_t *Wm,
                      FaceOut *out, hipStream_t st);
void launch_pcg_resid(const int *drows, int nrows, const double *PG, const double *G, int64_t Qp, const double *s1, double s2, const double *Hd,
                      const double *D, const uint8_t *Wm, double *Rv, CgState *cg, hipStream_t st);

} // namespace gml
