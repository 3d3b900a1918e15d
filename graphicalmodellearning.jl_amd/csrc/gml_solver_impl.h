// The Solver of gml_learn and its helpers, private to its two source files: gml_solver.cpp (passes, selection, Cholesky rows, line
// search, the outer iteration) and gml_newton_cg.cpp (the matrix-free direction phase).  Nothing else includes this header.
#pragma once
#include "gml_cg_rules.h"
#include "gml_internal.h"
#include "gml_slots.h"
#include "gml_solver.h"

#include <algorithm>
#include <cstring>
#include <functional>

#define RCCHK(expr)             \
    do {                        \
        const int rc__ = (expr); \
        if (rc__) return rc__;  \
    } while (0)

namespace gml {

// device allocations of one gml_learn call, released together
struct Arena {
    std::vector<void *> ptrs;
    ~Arena() {
        // also reached by the early returns of a failed solve, with kernels possibly still queued on the blocks: wait once,
        // then the blocks may go back to the library's cache (which hands them out without waiting)
        if (!ptrs.empty()) (void)hipDeviceSynchronize();
        for (void *q : ptrs)
            if (q) (void)dev_free_synced(q);
    }
    // give one block back before the arena dies (regrown buffers)
    void release(void *q) {
        for (auto &x : ptrs)
            if (x == q && q) {
                (void)dev_free(q);
                x = nullptr;
            }
    }
    template <typename T> hipError_t get(T **out, size_t count) {
        *out = nullptr;
        hipError_t e = dev_malloc(reinterpret_cast<void **>(out), sizeof(T) * std::max<size_t>(count, 1));
        if (e == hipSuccess) ptrs.push_back(*out);
        return e;
    }
};

// Small host <-> device transfers of the solver (control blocks up, per-row scalars down) go through one pinned arena:
// a copy from or to pageable memory is staged by the runtime and costs the host 20-30 us each.  h2d copies the bytes into
// the arena and queues an asynchronous copy from there -- the caller's buffer is free as soon as h2d returns; d2h queues
// the copy into the arena and hands the bytes to the caller's buffer at the next sync(), which is the only place the
// stream is waited for.  A transfer too large for the arena goes the plain way and is waited for at once.
struct Stage {
    char *base = nullptr;
    size_t cap = 0, off = 0, floor = 0; // [0, floor): arrays that live as long as the solve (persist); the rest is recycled at every sync()
    bool mapped = false;                // the device reads and writes the arena under its host address (checked by the solver's init)
    hipStream_t st = nullptr;
    struct Pend {
        void *host;
        const void *pin;
        size_t n;
    };
    std::vector<Pend> pend;
    void *take(size_t n) {
        const size_t a = (off + 63) & ~(size_t)63;
        if (a + n > cap) return nullptr;
        off = a + n;
        return base + a;
    }
    // Zero-copy: the arena is pinned, mapped host memory, so a kernel can read its control data from it and write its per-row results
    // into it directly.  On small node shards an iteration is a chain of short launches, and every hipMemcpyAsync in it was a 4-us blit
    // kernel plus 5 us of host time (profiles/r5_shard128_trace_before.txt: 15 per iteration).
    // persist: an array the kernels write and the host reads after sync(), for the whole solve (before the first take only)
    template <typename T> T *persist(size_t count) {
        const size_t a = (floor + 63) & ~(size_t)63;
        // only while nothing has been taken from the recycled part: [floor, off) may hold bytes of a copy still in flight
        if (!mapped || off != floor || !pend.empty() || a + sizeof(T) * count > cap / 2) return nullptr;
        floor = a + sizeof(T) * count;
        if (off < floor) off = floor;
        return reinterpret_cast<T *>(base + a);
    }
    // put: control data for kernels queued before the next sync(); NULL when it does not fit (the caller copies to a device buffer)
    template <typename T> const T *put(const T *host, size_t count) {
        void *q = mapped && sizeof(T) * count <= cap / 4 ? take(sizeof(T) * std::max<size_t>(count, 1)) : nullptr;
        if (q && count) std::memcpy(q, host, sizeof(T) * count);
        return reinterpret_cast<const T *>(q);
    }
    hipError_t h2d(void *dev, const void *host, size_t n) {
        if (n == 0) return hipSuccess;
        void *q = n <= cap / 4 ? take(n) : nullptr;
        if (!q) {
            hipError_t e = hipMemcpyAsync(dev, host, n, hipMemcpyHostToDevice, st);
            return e != hipSuccess ? e : hipStreamSynchronize(st); // the caller's buffer may die after return
        }
        std::memcpy(q, host, n);
        return hipMemcpyAsync(dev, q, n, hipMemcpyHostToDevice, st);
    }
    hipError_t d2h(void *host, const void *dev, size_t n) {
        if (n == 0) return hipSuccess;
        void *q = n <= cap / 4 ? take(n) : nullptr;
        if (!q) return hipMemcpyAsync(host, dev, n, hipMemcpyDeviceToHost, st);
        pend.push_back({host, q, n});
        return hipMemcpyAsync(q, dev, n, hipMemcpyDeviceToHost, st);
    }
    hipError_t sync() {
        const hipError_t e = hipStreamSynchronize(st);
        for (const Pend &x : pend) std::memcpy(x.host, x.pin, x.n);
        pend.clear();
        off = floor;
        return e;
    }
};

// Device time of the direction phase (Hessians, Cholesky, CG): measured with events, so that the host need not wait for
// the stream there just to read a clock.
struct PhaseTimer {
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    hipStream_t st = nullptr;
    ~PhaseTimer() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    void mark() {
        if (used == ev.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return;
            ev.push_back(e);
        }
        (void)hipEventRecord(ev[used++], st);
    }
    double seconds() { // sum over the (begin, end) pairs; call after the stream has been waited for
        double s = 0;
        for (size_t i = 0; i + 1 < used; i += 2) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) s += ms * 1e-3;
        }
        return s;
    }
};

template <typename T> const T *rebase(const T *p, int64_t lo) { // p' with p'[lo + i] == p[i] (indexed by absolute slot on the device only)
    return reinterpret_cast<const T *>(reinterpret_cast<uintptr_t>(p) - sizeof(T) * (size_t)lo);
}

// State of the matrix-free direction phase (gml_newton_cg.cpp).  Solver::init sets the options and allocates dLive; the rest is set and
// read in that file alone.
struct MatrixFree {
    static constexpr int kTile = 128; // entries of a working set per preconditioner tile
    // options: set by init, read by cg_round and hv_product
    double cg_eta = 0.05, hv_sparse_ratio = g_hv_sparse_ratio; // (sparse when sum |W| of the live rows < ratio * columns * node tiles of the GEMM pass)
    int maxcg = 16, hv_lf = 2, hv_lb = 2;
    // the tiles of this iteration: set by direction_blocks (upload_tile_ctl grows the buffers, k_cg_tiles fills dFV and dgV), read by the tile
    // inverses and by every step of the group solves.  dVm, dWrow and dT0m (NULL until a row has gone matrix-free) point into dTctl
    char *dTctl = nullptr;
    size_t dTctl_bytes = 0;
    int64_t tile_cap = 0, ntiles = 0, tile_base = 0; // capacity of dFV / dgV in tiles; tiles of this iteration; offset of the first one's block in dH
    int *dFV = nullptr, *dVm = nullptr, *dWrow = nullptr;
    double *dgV = nullptr;
    const long long *dT0m = nullptr; // first tile of each local row's list of working-set columns
    // the CG solves' vectors, mask of the system's coordinates, |W| by row and control block of a product: allocated by begin_group on
    // first use (dLive, the flag by row: by init), written by the kernels of every step; the scratch of the entry-by-entry products: hv_product
    double *Rv = nullptr, *Pv = nullptr, *Hp = nullptr, *Zv = nullptr;
    uint8_t *Wm = nullptr;
    FaceOut *dFaces = nullptr;
    int *dNw = nullptr, *dLive = nullptr, *dHv = nullptr;
    void *dHvsBuf = nullptr;
    size_t hvs_bytes = 0;
    // the group being solved: set by begin_group (kchunk, kpart: by every set_plan), read by cg_round, face_round and hv_product
    int64_t maxW = 1, kchunk = 0, kpart = 0;
    bool sparse_ok = false;
    std::vector<std::pair<int, int>> relax;
    std::vector<int> liveflag;
    std::vector<CgState> cgs; // as the last step left them (cg_round)
    std::vector<FaceOut> faces;
    WList wl() const { return WList{dFV, dT0m, dNw, kTile}; }
};
struct HessCall; // what a Hessian call takes from the two control blocks of direction_blocks (gml_newton_cg.cpp)

struct Solver {
    // ---- problem, options ----------------------------------------------------------------------------------------------
    gml_problem *p;
    const DevProblem &d;
    const int formulation;
    gml_opts o;
    gml_stats stats{};
    hipStream_t st;
    const double *x0 = nullptr; // warm start (gml_learn_warm): the rows to start from, reference layout [R][P], host or device; NULL = zeros
    // the caller's structure (gml_learn_structured): kind of every parameter slot of every local row, reference layout [R][ld_s] bytes, host or
    // device; NULL = the reference's (field free, the rest penalised: k_kind alone)
    const uint8_t *structure = nullptr;
    int64_t ld_s = 0;
    std::vector<int> nparam; // with a structure: parameters (slots not excluded) per row; a row without any is complete before the first pass
    int32_t *dColsRef = nullptr; // multi-body: column of every parameter slot of every local row (:94-104), built once (warm start, finish)
    int compact_skip = 0, compact_backoff = 0; // passes that do not try the column compaction after one that came out dense (run_pass)
    bool underflow = false; // the solve ended because a row's weights left the fixed-point range at an iterate (gml_learn: auto -> FP64)
    bool at_zero = false; // the pass being queued evaluates X = 0 (the first pass of a solve; also its rescaled re-runs)
    double tune[GML_NTUNE] = {}; // the experiment knobs as they stood when the solve began (gml_test_tune may be called meanwhile)
    Stage stg;
    Arena A;
    PhaseTimer dir_time;
    double t_dir_host = 0; // host time between the two marks of the direction phases (launches, and the waits of the CG steps)
    const int64_t R, Rp, Qp, P;
    const size_t nd;
    int capW = 0, capP = 0;
    double lambda = 0;
    int64_t Scap = 0;  // slots of the int8-limb workspace
    PlaneSlots slots;  // ... and which row owns which V planes in them (gml_slots.h)
    double viol_frac = 0.5;
    int64_t dbg_row = 0, worst_row = 0;
    const double t_begin = gml_now_s();
    // precision i8w: the passes run in their coarse form (30-bit theta, 23-bit weights) until the first active row comes within
    // coarse_thr of its optimum, then at full width for the rest of the solve
    bool coarse_on = false;
    double coarse_thr = 1e-7;
    int prec = GML_PREC_I8X; // arithmetic of the passes: switches to FP64 for the rows the int8 path leaves above tol ("polish")
    bool can_polish = false;
    int stall_cap = 10;

    // ---- device state ----------------------------------------------------------------------------------------------------
    double *X = nullptr, *G = nullptr, *Xt = nullptr, *Gt = nullptr, *Xb = nullptr, *D = nullptr, *PG = nullptr, *Gs = nullptr;
    uint8_t *kind = nullptr;
    int *dNode = nullptr, *dRows = nullptr, *dRows2 = nullptr, *dRowsP = nullptr, *dFidx = nullptr;
    char *dPass = nullptr;  // control block of a pass: srow | rowcol | groups | tau overrides (one upload)
    char *dHctl = nullptr;  // control block of the direction phase (one upload)
    SlotResult *dRes = nullptr;
    CgState *dCg = nullptr;
    double *dBest = nullptr, *dAlpha = nullptr, *dFs = nullptr, *dgF = nullptr, *dpgF = nullptr, *dsol = nullptr,
           *dSdiag = nullptr, *dH = nullptr;
    SelectOut *dSel = nullptr;
    TrialOut *dTrial = nullptr;
    int64_t dH_elems = 0;
    // pointers into dHctl (set by direction_blocks)
    int *dMt = nullptr, *dPlane = nullptr;
    long long *dHoff = nullptr;
    double *dS1 = nullptr, *dS1cg = nullptr;
    // secant pairs of the Cholesky rows (k_secant): previous working set, x and g on it, the last two (s, y)
    int *dFprev = nullptr, *dMprev = nullptr, *dNpairs = nullptr;
    double *dXprev = nullptr, *dGprev = nullptr, *dSec = nullptr, *dYnoise = nullptr;
    MatrixFree mf; // everything only the matrix-free direction phase uses (gml_newton_cg.cpp)

    // ---- host state (scalars per row) ------------------------------------------------------------------------------------
    std::vector<double> f, ft, Fobj, kkt, best, Z, Zt, alpha, dd, fn, fnt, l1t, Fbest;
    std::vector<uint8_t> done, atfloor, nreg, accepted_fwd, need, iscg;
    std::vector<int> stall, msz, nW;
    // per-row results of k_select / k_trial + k_back / the passes' last kernels: written by the kernels straight into pinned host
    // memory (Stage::persist) and read here after the stream has been waited for; device arrays + one download each when the
    // pinned arena is too small for them (tens of thousands of local rows)
    SelectOut *sel = nullptr, *kSel = nullptr;
    TrialOut *trial = nullptr, *kTrial = nullptr;
    SlotResult *res = nullptr, *kRes = nullptr;
    std::vector<SelectOut> sel_v;
    std::vector<TrialOut> trial_v;
    std::vector<SlotResult> res_v;
    bool zc = false;
    double *dStepn = nullptr; // |trial - x|_1 by row, left on the device by k_trial: scales the weights' unit of the trial pass (k_quant_theta)
    // Scale of the fixed-point V (int8 path): instead of the worst-case bound w_max exp(sum|theta|) every pass after a row's
    // first uses vref = max_k |V_rk| measured by its previous pass, times exp(||theta - theta_ref||_1), which bounds the new
    // weights rigorously (|E_k' - E_k| <= ||theta' - theta||_1).  Near the optimum the steps are tiny, so V keeps all 31 bits
    // relative to its actual maximum and the noise floor of f and grad drops by the bits the bound would have wasted.
    std::vector<double> vref, dref, stepn;
    // where a pass leaves its results, by row: f (or log Z), Z (logRISE), the noise of f -- at the iterates, at the trial points
    struct PassOut {
        std::vector<double> &f, &Z, &noise;
    };
    const PassOut at_x{f, Z, fn}, at_xt{ft, Zt, fnt};
    // sub-sampled Newton: Hessians over Kh configurations -- every kstride-th block of 512 (set_kh)
    int64_t Kh_base = 0, nblk512 = 0, Kh = 0, kstride = 1;
    double hscale = 1.0;
    // the record of the outer iterations (gml_solver.h: TrajRecorder), NULL unless a test armed it before the solve began
    TrajRecorder *rec = nullptr;
    double *rec_row(int64_t r) { return rec->its.back().rows.data() + (size_t)r * TRR_N; }
    int rec_select(int it, int64_t nactive);
    int rec_download(void *host, const void *dev, size_t bytes) { // (armed only: waits for the stream)
        HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return GML_OK;
    }
    // the matrix-free events of the iteration (TRC_*), armed only: gml_newton_cg.cpp, at its end.  rec_cg(tag) opens an event; the methods
    // that "add to the open event" append to the last one of the iteration
    TrajCgEvent &rec_cg(int tag) {
        rec->its.back().cg.push_back(TrajCgEvent{tag, {}, {}});
        return rec->its.back().cg.back();
    }
    TrajCgEvent &rec_open() { return rec->its.back().cg.back(); }
    using Rows = std::vector<int>;
    int rec_rows_of(const double *dev, const Rows &rows), rec_cgstate(const Rows &rows), rec_tau(const Rows &rows, std::vector<double> &tau, std::vector<unsigned> *mmax);
    int rec_blocks(const Rows &cg_rows, const cg::RowCtl &h), rec_blocks_inverses(), rec_round_end(int round, const Rows &cur);
    int rec_product_head(bool sparse, const cg::HvCtl &L, const Rows &rows, const Rows &ctl, const double *vec);
    void rec_row_scales(const cg::RowCtl &h), rec_group(const Rows &rows, bool coarse), rec_step_state(const Rows &live);
    void rec_plan(int where, int round, int ci, int ksub, int64_t kchunk, int nsplit, int64_t ngroups, const cg::PlanScales &ps);
    void rec_faces(int round, const Rows &cur, const Rows &again);

    Solver(gml_problem *p_, int form, const gml_opts &o_, double lam)
        : p(p_), d(p_->d), formulation(form), o(o_), st(p_->st), R(p_->node1 - p_->node0), Rp(gml_round_up(R, 32)), Qp(p_->d.Qp), P(p_->P),
          nd((size_t)Rp * p_->d.Qp), lambda(lam) {}

    void trace(const char *name) {
        if (o.verbose >= 3) {
            (void)stg.sync();
            fprintf(stderr, "[gml]     stage %s at %.4f s (last error: %s)\n", name, gml_now_s() - t_begin, hipGetErrorString(hipGetLastError()));
            fflush(stderr);
        }
    }
    void reopen(int r) { // a finished row is solved on (other arithmetic): its best-iterate record and its stall count start over
        done[r] = atfloor[r] = 0;
        stall[r] = 0;
        best[r] = Fbest[r] = INFINITY;
    }
    int upload_rows(const std::vector<int> &rows, int *dst) {
        if (!rows.empty()) HIPCHK(stg.h2d(dst, rows.data(), sizeof(int) * rows.size()));
        return GML_OK;
    }
    // a row list (or any small control array) for kernels queued before the next wait: read from the pinned arena where it fits,
    // else uploaded to `fallback`
    template <typename T> int ctl(const std::vector<T> &v, T *fallback, const T **out) {
        const T *q = v.empty() ? nullptr : stg.put(v.data(), v.size());
        *out = q ? q : fallback;
        if (!q && !v.empty()) HIPCHK(stg.h2d(fallback, v.data(), sizeof(T) * v.size()));
        return GML_OK;
    }
    int fetch(void *host, const void *dev, size_t bytes) { // results the kernels left in device arrays (not zero-copy)
        if (!zc) HIPCHK(stg.d2h(host, dev, bytes));
        return GML_OK;
    }

    int init();
    void set_kh(int64_t nactive);
    // One objective(/gradient) pass over the listed rows.  src: X or Xt; dst: G or Gt (want_grad); out: where the results per row
    // go.  pp: the arithmetic of this pass (< 0: the solver's current precision; the FP64 phase borrows int8 passes for the V planes
    // its matrix-free rows need).  after: queued on the stream right behind the pass and before the host waits for it (the
    // acceptance scalars of a trial ride along with the pass results).  step_on_device: a trial whose |trial - x|_1 is still on
    // the device (dStepn) and comes down with the results.
    int run_pass(const std::vector<int> &rows, const double *src, double *dst, bool want_grad, bool at_trial, const PassOut &out, int pp = -1,
                 const std::function<int()> *after = nullptr, bool step_on_device = false);
    struct PassArgs { // what every round of one run_pass call shares
        const double *src;
        double *dst;
        bool want_grad, at_trial;
        int pp;
        const std::function<int()> *after;
    };
    using PassRaw = std::vector<SlotResult>; // per listed row, as the kernels left it: f (or Z); on the int8 path also tau and mmax
    int pass_i8(const PassArgs &q, const std::vector<int> &rows, const std::vector<double> *ovr_in, bool step_on_device, PassRaw &raw);
    int pass_f64(const PassArgs &q, const std::vector<int> &rows, PassRaw &raw);
    void compaction_backoff(const std::vector<int> &ctab);
    void judge_rows(const PassArgs &q, const std::vector<int> &rows, const PassRaw &raw, const PassOut &out, std::vector<int> &again,
                    std::vector<double> &ovr2);
    int select(int it, int64_t *nactive);
    int start_polish(bool *started);
    int refresh_stale();
    int newton_blocks(const std::vector<int> &chol_rows);
    int line_search();
    double s2() const { return formulation == GML_LOGRISE ? 1.0 : 0.0; } // Hess log Z = Hess Z / Z - s2 g g^T
    // ---- the Hessian blocks of both kinds of row and the matrix-free direction phase (gml_newton_cg.cpp), each in the order of its steps ----
    int direction_blocks(const Rows &cg_rows);
    int borrow_i8_planes(const Rows &cg_rows), grow_hessian(int64_t htotal), check_planes(const cg::RowCtl &h);
    void fill_row_ctl(const cg::RowCtl &h);
    int upload_row_ctl(const std::vector<char> &blk), upload_tile_ctl(const std::vector<char> &blk, const Rows &cg_rows, HessCall *hc);
    int launch_hessians(const HessCall &hc, int64_t htotal);
    int newton_cg(const Rows &cg_rows), newton_cg_group(const Rows &rows, bool coarse), begin_group(const Rows &rows, bool coarse);
    int set_live(const Rows &rows), set_plan(int ksub, size_t nrows, int where, int round, int ci);
    int hv_product(const Rows &rows, const double *vec, double *out);
    void precondition_and_direct(const Rows &rows, int first);
    int cg_round(int round, const Rows &cur), face_round(int round, const Rows &cur, Rows *again);
    int finish(double *out, double *kkt_out, int iterations);
    int ref_cols();
    int apply_structure();
    int load_x0();
    int iterate(double *out, double *kkt_out);
};

} // namespace gml
