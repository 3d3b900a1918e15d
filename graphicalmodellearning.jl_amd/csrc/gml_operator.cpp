// libgml_hip, host side: the operator boundary -- gml_objgrad_batch / gml_hessvec_batch (GraphicalModelLearning.jl:191-208,
// :221-233) and the timing hooks of the benchmark: orchestration of the device passes for host-pointer callers.
#include "gml_cg_rules.h"
#include "gml_internal.h"
#include "gml_solver.h"
#include "gml_pack.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

using namespace gml;

// operator calls compact the forward GEMM (sparse rows are what an l1 solver evaluates); the timing hooks sweep all columns unless asked
static bool op_compact() { return g_tune[GML_TUNE_NO_COMPACT] == 0; }
static bool bench_compact() { return g_tune[GML_TUNE_NO_COMPACT] == 0 && g_tune[GML_TUNE_BENCH_COMPACT] > 0; }

// ------------------------------------------------------------------------------------------
// workspace of the operator calls and the timing hooks
// ------------------------------------------------------------------------------------------
int gml_ensure_ws(gml_problem *p, int64_t rows) {
    const int64_t Rp = gml_round_up(rows, 32);
    if (Rp <= p->ws_rows) return GML_OK;
    void *ptrs[] = {p->dTheta, p->dV, p->dG, p->dF, p->dSrow};
    for (void *q : ptrs)
        if (q) (void)dev_free(q);
    void *hptrs[] = {p->hTh, p->hG, p->hF, p->hCtl};
    for (void *q : hptrs)
        if (q) (void)hipHostFree(q);
    p->hTh = p->hG = p->hF = nullptr;
    p->hCtl = nullptr;
    p->dTheta = p->dV = p->dG = p->dF = nullptr;
    p->dSrow = p->dRowcol = p->dGroups = nullptr;
    p->ws_rows = 0;
    size_t freeb = 0, totalb = 0;
    HIPCHK(dev_mem_info(&freeb, &totalb));
    const double need = 2.0 * Rp * p->d.Qp * 8.0;
    if (need > 0.9 * (double)freeb)
        return fail(GML_ENOMEM, "workspace of %.1f GB for %lld rows does not fit in %.1f GB free HBM", need / 1e9,
                    (long long)Rp, freeb / 1e9);
    HIPCHK(dev_malloc(&p->dTheta, sizeof(double) * Rp * p->d.Qp));
    HIPCHK(dev_malloc(&p->dG, sizeof(double) * Rp * p->d.Qp));
    HIPCHK(dev_malloc(&p->dF, sizeof(double) * Rp));
    // control block: srow [Rp] | rowcol [Rp] | active tiles, padded with -1 [Rp/32 + 4]; one pinned twin, one upload per pass
    const int64_t nctl = 2 * Rp + Rp / 32 + 4;
    HIPCHK(dev_malloc(&p->dSrow, sizeof(int) * nctl));
    p->dRowcol = p->dSrow + Rp;
    p->dGroups = p->dRowcol + Rp;
    HIPCHK(hipHostMalloc(&p->hCtl, sizeof(int) * nctl));
    HIPCHK(hipHostMalloc(&p->hTh, sizeof(double) * Rp * p->d.Qp));
    HIPCHK(hipHostMalloc(&p->hG, sizeof(double) * Rp * p->d.Qp));
    HIPCHK(hipHostMalloc(&p->hF, sizeof(double) * Rp));
    HIPCHK(hipMemsetAsync(p->dTheta, 0, sizeof(double) * Rp * p->d.Qp, p->st));
    p->ws_rows = Rp;
    return GML_OK;
}

// What only the FP64 path needs: the two byte images of the design matrix and V [vrows][Kp].
int gml_ensure_f64(gml_problem *p, int64_t vrows) {
    DevProblem &d = p->d;
    size_t freeb = 0, totalb = 0;
    if (!d.Xt) { // feature-major byte image: the rows the FP64 Hessian kernel gathers (the GEMM kernels read the bit images)
        HIPCHK(dev_mem_info(&freeb, &totalb));
        if ((double)d.Kp * d.Qp > 0.9 * (double)freeb)
            return fail(GML_EUNSUPPORTED, "the FP64 path needs a %.1f GB byte image of the design matrix: use precision i8x or i8w",
                        (double)d.Kp * d.Qp / 1e9);
        HIPCHK(dev_malloc(&d.Xt, (size_t)d.Kp * d.Qp));
        HIPCHK(hipMemsetAsync(d.Xt, 0, (size_t)d.Kp * d.Qp, p->st));
        launch_expand_xt(d, d.Xt, p->st);
        HIPCHK(hipMemsetAsync(d.Xt + d.cconst * d.Kp, 1, (size_t)p->K, p->st)); // the constant statistic
    }
    vrows = gml_round_up(vrows, 32);
    if (!p->dV || p->dVrows < vrows) {
        if (p->dV) (void)dev_free(p->dV);
        p->dV = nullptr;
        p->dVrows = 0;
        HIPCHK(dev_mem_info(&freeb, &totalb));
        if ((double)vrows * d.Kp * 8.0 > 0.9 * (double)freeb)
            return fail(GML_ENOMEM, "FP64 workspace of %.1f GB does not fit: use precision i8x", (double)vrows * d.Kp * 8.0 / 1e9);
        HIPCHK(dev_malloc(&p->dV, sizeof(double) * vrows * d.Kp));
        HIPCHK(hipMemsetAsync(p->dV, 0, sizeof(double) * vrows * d.Kp, p->st));
        p->dVrows = vrows;
    }
    if (p->dRedRows != p->dVrows) { // the parts of f and G before their fixed-order reduction: sized with V, once per size of V
        const size_t red = f64_reduce_ws_bytes(d, p->dVrows);
        if (p->dRedBytes < red) {
            if (p->dRed) (void)dev_free(p->dRed);
            p->dRed = nullptr;
            p->dRedBytes = 0;
            p->dRedRows = 0;
            HIPCHK(dev_mem_info(&freeb, &totalb));
            if ((double)red > 0.9 * (double)freeb)
                return fail(GML_ENOMEM, "FP64 reduction workspace of %.2f GB does not fit: use precision i8x", (double)red / 1e9);
            HIPCHK(dev_malloc(&p->dRed, red));
            p->dRedBytes = red;
        }
        p->dRedRows = p->dVrows;
    }
    return GML_OK;
}

// control block of a pass over the rows flagged in act (slot = row): srow | rowcol | active tiles padded with -1 to a multiple of 4,
// through its pinned twin in one upload; returns the tiles and their padded count
static int upload_ctl(gml_problem *p, int64_t R, const int64_t *nodes, const std::vector<uint8_t> &act, std::vector<int> &groups, int *npad_out) {
    const int64_t Rp = gml_round_up(R, 32), W = p->ws_rows;
    groups.clear();
    for (int64_t r = 0; r < Rp; ++r) {
        p->hCtl[r] = (int)r;
        p->hCtl[W + r] = (r < R && act[r]) ? (int)nodes[r] : -1; // the node whose sign bits the row uses
    }
    for (int64_t gidx = 0; gidx < Rp / 32; ++gidx) {
        bool any = false;
        for (int64_t r = gidx * 32; r < std::min(R, (gidx + 1) * 32); ++r) any |= (act[r] != 0);
        if (any) groups.push_back((int)gidx);
    }
    int npad = 0;
    for (size_t g = 0; g < groups.size() || (npad % 4); ++g, ++npad) p->hCtl[2 * W + g] = g < groups.size() ? groups[g] : -1;
    *npad_out = npad;
    HIPCHK(hipMemcpyAsync(p->dSrow, p->hCtl, sizeof(int) * (2 * W + npad), hipMemcpyHostToDevice, p->st));
    return GML_OK;
}

// One pass over the tiles of the uploaded control block (slots 0 .. Rp): theta rows in dTheta, f into dF and the gradient into dG
// (want_grad) -- or, hv, the Hessian-vector pass of the directions in dTheta, which leaves H p (RISE, RPLE) / Hess Z p (logRISE) in
// dG from the curvature weights the objective pass left in the same slots.  tauovr: device [Rp] or NULL, the per-slot scale of a
// rescaled re-run.  ev: [3] or NULL, recorded before the forward, between the two halves and after the backward.
// kn: the forms of an int8-limb pass the public entry points leave at their defaults, set by the test hook gml_test_i8_pass (NULL:
// the defaults)
struct PassKnobs {
    bool coarse = false, zero_theta = false;
    int lf = 0, hv = 1, ksub = 0; // hv: 1 or 2 (a Hessian-vector pass only)
    int64_t kchunk = 0, kpart = 0;
    gml::SlotResult *res = nullptr;
    int64_t *plan_out = nullptr;
    const int *vmap = nullptr; // a Hessian-vector pass: the slot whose V planes and tau each slot reads (device; NULL: its own)
};
static int launch_pass(gml_problem *p, int64_t Rp, int ngroups, int npad, int form, int precision, bool want_grad, bool hv,
                       const double *tauovr, bool compact, hipEvent_t *ev, const PassKnobs *kn = nullptr) {
    hipStream_t st = p->st;
    if (gml_is_i8(precision)) {
        gml::I8Pass a{};
        a.theta = p->dTheta;
        a.srow = p->dSrow;
        a.rowcol = p->dRowcol;
        a.groups = p->dGroups;
        a.ngroups = ngroups;
        a.slot0 = 0;
        a.slot1 = (int)Rp;
        a.form = form;
        a.want_grad = want_grad;
        a.F = hv ? nullptr : p->dF;
        a.G = p->dG;
        a.tauovr = tauovr;
        a.wide = precision == GML_PREC_I8W;
        a.compact = compact;
        a.hv = hv ? 1 : 0;
        a.vmap = hv ? p->dSrow : nullptr; // (slot = row: the weights of the objective pass that ran in the same slot)
        if (kn) {
            a.coarse = kn->coarse;
            a.zero_theta = kn->zero_theta;
            a.lf = kn->lf;
            if (hv) a.hv = kn->hv;
            a.ksub = kn->ksub;
            a.kchunk = kn->kchunk;
            a.kpart = kn->kpart;
            a.res = kn->res;
            a.plan_out = kn->plan_out;
            if (hv && kn->vmap) a.vmap = kn->vmap;
        }
        std::string err;
        const int rc = gml::i8_pass(&p->i8ws, p->d, p->ws_rows, a, st, ev, &err);
        return rc ? fail(rc, "%s", err.c_str()) : GML_OK;
    }
    const int rc = gml_ensure_f64(p, p->ws_rows);
    if (rc) return rc;
    if (!hv) HIPCHK(hipMemsetAsync(p->dF, 0, sizeof(double) * Rp, st));
    if (want_grad) HIPCHK(hipMemsetAsync(p->dG, 0, sizeof(double) * Rp * p->d.Qp, st));
    if (ev) HIPCHK(hipEventRecord(ev[0], st));
    launch_fwd_f64(p->d, p->dTheta, p->dRowcol, p->dGroups, npad, hv ? form + 4 : form, p->dV, p->dF, p->dRed, st); // (hv: V <- h (x . p), in place)
    if (ev) HIPCHK(hipEventRecord(ev[1], st));
    if (want_grad) launch_bwd_f64(p->d, p->dV, p->dGroups, ngroups, p->dG, p->dRed, st);
    if (ev) HIPCHK(hipEventRecord(ev[2], st));
    HIPCHK(hipGetLastError());
    return GML_OK;
}

// Dynamic range of the fixed-point V: tau_r was derived from the bound w_max exp(sum_j |theta_rj|).  When the largest |V_rk| actually
// seen is more than 8 bits (i8w: 4 bits) below that bound (dense theta), the row is re-run with tau_r taken from it: (mmax + 1) tau
// bounds every |V_rk| rigorously, so the re-run cannot overflow.  (The FP64-grade pass is stricter: it is re-run as soon as four of
// its 47 bits would go unused, so that its error stays at 2^-43 of the largest weight whatever the bound was.)
struct Rescale {
    std::vector<uint8_t> again; // [R] rows to re-run
    std::vector<double> ovr;    // [Rp] their tau (0 elsewhere)
    int64_t n = 0;
    double *dOvr = nullptr; // ovr on the device, kept across the re-runs of one call and freed with it, early returns included
    Rescale() = default;
    Rescale(const Rescale &) = delete;
    Rescale &operator=(const Rescale &) = delete;
    ~Rescale() {
        if (dOvr) (void)dev_free(dOvr);
    }
    int upload(gml_problem *p, int64_t Rp) {
        if (!dOvr) HIPCHK(dev_malloc(&dOvr, sizeof(double) * Rp));
        HIPCHK(hipMemcpyAsync(dOvr, ovr.data(), sizeof(double) * Rp, hipMemcpyHostToDevice, p->st));
        return GML_OK;
    }
};

// Downloads tau / mmax of the pass just launched (int8-limb exp forms), synchronises the stream, and lists the active rows to re-run.
static int rescale_rows(gml_problem *p, int64_t R, const std::vector<uint8_t> &act, int form, int precision, Rescale &rs) {
    const int64_t Rp = gml_round_up(R, 32);
    const bool wide = precision == GML_PREC_I8W;
    std::vector<double> tau;
    std::vector<unsigned> mmax;
    if (gml_is_i8(precision) && form != GML_RPLE) {
        const double *dtau = nullptr;
        const unsigned *dmm = nullptr;
        gml::i8_slot_results(p->i8ws, 0, &dtau, &dmm);
        tau.resize((size_t)Rp);
        mmax.resize((size_t)Rp);
        HIPCHK(hipMemcpyAsync(tau.data(), dtau, sizeof(double) * Rp, hipMemcpyDeviceToHost, p->st));
        HIPCHK(hipMemcpyAsync(mmax.data(), dmm, sizeof(unsigned) * Rp, hipMemcpyDeviceToHost, p->st));
    }
    HIPCHK(hipStreamSynchronize(p->st));
    rs.again.assign((size_t)R, 0);
    rs.ovr.assign((size_t)Rp, 0.0);
    rs.n = 0;
    if (mmax.empty()) return GML_OK;
    const unsigned mm_min = wide ? (1u << 27) : (1u << 23);
    for (int64_t r = 0; r < R; ++r)
        if (act[r] && mmax[r] < mm_min) {
            rs.again[r] = 1;
            rs.ovr[r] = ((double)mmax[r] + 1.0) * gml::i8_mmax_unit(wide) * tau[r] * (1.0 + 1e-12) / gml::i8_vdiv(wide);
            ++rs.n;
        }
    return GML_OK;
}

// The pass after one that left rows to re-run: the same precision rescaled, up to six times.  Six rescalings that did not bring a
// row's largest weight into the planes mean energies spread over hundreds of units (|theta|_1 in the hundreds -- a far trial point
// of an external solver).  The reference's Float64 operator (GraphicalModelLearning.jl:191-197) returns a number there, so `auto`
// -- its stand-in, f64_fallback -- evaluates these rows on the FP64 path, as a fresh pass (depth 0); a caller who named an
// int8-limb precision gets the error.
static int rescale_next(int *depth, int *precision, bool *f64_fallback) {
    if (*depth < 6) {
        ++*depth;
        return GML_OK;
    }
    if (!*f64_fallback)
        return fail(GML_EUNSUPPORTED, "precision %s: the weights exp(-E) of a row underflow its fixed-point range; use precision f64 (or auto)",
                    *precision == GML_PREC_I8W ? "i8w" : "i8x");
    *depth = 0;
    *precision = GML_PREC_F64;
    *f64_fallback = false;
    return GML_OK;
}

// Rows of the reference order -> the internal column layout on the host: dst [R][Qp] from src [R][ld], and dst2 from src2 when
// given (the caller zeroes the columns no parameter lands on); lay receives the nodes' layouts.  Returns the first row holding a
// non-finite value, -1 if none.
static int64_t to_internal(const gml_problem *p, int64_t R, const int64_t *nodes, std::vector<NodeLayout> &lay, const double *src, int64_t ld,
                           double *dst, const double *src2 = nullptr, double *dst2 = nullptr) {
    const int64_t P = p->P, Qp = p->d.Qp;
    lay.assign((size_t)R, NodeLayout{});
    std::vector<uint8_t> bad((size_t)R, 0);
    gml_parallel_for(R, [&](int64_t r) {
        gml_build_layout(p, nodes[r], lay[r]);
        for (int64_t j = 0; j < P; ++j) {
            const int64_t c = r * Qp + lay[r].cols[j];
            dst[c] = src[r * ld + j];
            if (!std::isfinite(dst[c])) bad[r] = 1;
            if (src2) {
                dst2[c] = src2[r * ld + j];
                if (!std::isfinite(dst2[c])) bad[r] = 1;
            }
        }
    });
    for (int64_t r = 0; r < R; ++r)
        if (bad[r]) return r;
    return -1;
}

// The internal layout -> rows of the reference order, with the finish of logRISE, whose pass leaves Z and its derivatives: f = log Z
// and g = grad Z / Z.  For a Hessian-vector product (Gz = grad Z, vec = the directions) g receives Hess log Z v = Hess Z v / Z - g (g . v)
// with g = grad Z / Z (:279).  f, g may be NULL.
static void to_reference(const std::vector<NodeLayout> &lay, int64_t P, int64_t Qp, int form, const double *Z, const double *src, double *f,
                         double *g, int64_t ld, const double *Gz = nullptr, const double *vec = nullptr) {
    const bool logz = form == GML_LOGRISE;
    gml_parallel_for((int64_t)lay.size(), [&](int64_t r) {
        const int32_t *cols = lay[r].cols.data();
        const double z = Z[r];
        if (f) f[r] = logz ? std::log(z) : z;
        if (!g) return;
        double gv = 0.0;
        if (logz && Gz)
            for (int64_t j = 0; j < P; ++j) gv += Gz[(size_t)r * Qp + cols[j]] / z * vec[r * ld + j];
        for (int64_t j = 0; j < P; ++j) {
            double v = src[(size_t)r * Qp + cols[j]];
            if (logz) v = Gz ? v / z - Gz[(size_t)r * Qp + cols[j]] / z * gv : v / z;
            g[r * ld + j] = v;
        }
    });
}

// One device pass over the R rows of theta (R x Qp host, internal layout), with the rescaled re-runs of the rows the fixed point does
// not hold: writes f[r], and g (R x Qp) when want_grad.  ms [2] or NULL: device time of the first pass's forward and backward halves.
static int device_pass(gml_problem *p, int64_t R, const int64_t *nodes, const double *theta, int form, int precision, bool want_grad,
                       bool compact, bool f64_fallback, double *f, double *g, float *ms = nullptr) {
    const int64_t Qp = p->d.Qp, Rp = gml_round_up(R, 32);
    int rc = gml_ensure_ws(p, R);
    if (rc) return rc;
    hipStream_t st = p->st;
    std::vector<uint8_t> act((size_t)R, 1);
    std::vector<int> groups;
    Rescale rs;
    for (int depth = 0;;) {
        int npad = 0;
        rc = upload_ctl(p, R, nodes, act, groups, &npad);
        if (rc) return rc;
        if (groups.empty()) return GML_OK;
        // one contiguous upload covering the active groups, through the pinned staging buffer
        const int64_t ra = (int64_t)groups.front() * 32, rb = std::min(R, (int64_t)groups.back() * 32 + 32);
        gml_parallel_for((rb - ra + 31) / 32, [&](int64_t b) {
            const int64_t r0 = ra + b * 32, r1 = std::min(rb, r0 + 32);
            std::memcpy(p->hTh + r0 * Qp, theta + r0 * Qp, sizeof(double) * (r1 - r0) * Qp);
        });
        HIPCHK(hipMemcpyAsync(p->dTheta + ra * Qp, p->hTh + ra * Qp, sizeof(double) * (rb - ra) * Qp, hipMemcpyHostToDevice, st));
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        if (ms)
            for (auto &e : ev) HIPCHK(hipEventCreate(&e));
        if (depth > 0 && (rc = rs.upload(p, Rp))) return rc;
        rc = launch_pass(p, Rp, (int)groups.size(), npad, form, precision, want_grad, false, depth > 0 ? rs.dOvr : nullptr, compact,
                         ms ? ev : nullptr);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(p->hF, p->dF, sizeof(double) * Rp, hipMemcpyDeviceToHost, st));
        if (want_grad)
            HIPCHK(hipMemcpyAsync(p->hG + ra * Qp, p->dG + ra * Qp, sizeof(double) * (rb - ra) * Qp, hipMemcpyDeviceToHost, st));
        rc = rescale_rows(p, R, act, form, precision, rs);
        if (rc) return rc;
        if (ms) {
            HIPCHK(hipEventElapsedTime(&ms[0], ev[0], ev[1]));
            HIPCHK(hipEventElapsedTime(&ms[1], ev[1], ev[2]));
            for (auto &e : ev) (void)hipEventDestroy(e);
            ms = nullptr; // (the re-runs are not timed)
        }
        for (int64_t r = 0; r < R; ++r)
            if (act[r]) f[r] = p->hF[r];
        if (want_grad)
            gml_parallel_for((int64_t)groups.size(), [&](int64_t a) {
                for (int i = 0; i < 32; ++i) {
                    const int64_t r = (int64_t)groups[a] * 32 + i;
                    if (r < R && act[r]) std::memcpy(g + r * Qp, p->hG + r * Qp, sizeof(double) * Qp);
                }
            });
        if (rs.n == 0) return GML_OK;
        if ((rc = rescale_next(&depth, &precision, &f64_fallback))) return rc;
        act = rs.again;
    }
}

// ------------------------------------------------------------------------------------------
// The same pass for callers whose rows live in HBM (device pointers for theta / f / g): the reference-order rows are
// scattered into the internal layout by a kernel, the pass runs, a kernel gathers the results back -- no staging, no PCIe.
// The only host round trip is the one the dynamic-range check needs (two small per-row arrays).
// ------------------------------------------------------------------------------------------
// slot -> column table of a multi-body node list on the device (NULL for pairwise: closed form in the kernels)
static int dev_cols(gml_problem *p, int64_t nrows, const int64_t *nodes, const int32_t **out) {
    *out = nullptr;
    if (p->order == 2) return GML_OK;
    if (p->opCols && (int64_t)p->opNodes.size() == nrows && std::equal(nodes, nodes + nrows, p->opNodes.begin())) {
        *out = p->opCols;
        return GML_OK;
    }
    if (p->opCols) (void)dev_free(p->opCols);
    p->opCols = nullptr;
    p->opNodes.clear();
    const int64_t P = p->P;
    std::vector<int32_t> cols((size_t)nrows * P);
    gml_parallel_for(nrows, [&](int64_t r) {
        NodeLayout L;
        gml_build_layout(p, nodes[r], L);
        std::memcpy(cols.data() + (size_t)r * P, L.cols.data(), sizeof(int32_t) * P);
    });
    HIPCHK(dev_malloc(&p->opCols, sizeof(int32_t) * (size_t)nrows * P));
    HIPCHK(hipMemcpyAsync(p->opCols, cols.data(), sizeof(int32_t) * (size_t)nrows * P, hipMemcpyHostToDevice, p->st));
    HIPCHK(hipStreamSynchronize(p->st)); // cols is a local
    p->opNodes.assign(nodes, nodes + nrows);
    *out = p->opCols;
    return GML_OK;
}

static int dev_scratch(gml_problem *p, int64_t Rp) {
    if (!p->opFlag) HIPCHK(dev_malloc(&p->opFlag, sizeof(int) * 4));
    if (p->opSelCap < Rp) {
        if (p->opSel) (void)dev_free(p->opSel);
        p->opSel = nullptr;
        p->opSelCap = 0;
        HIPCHK(dev_malloc(&p->opSel, (size_t)Rp));
        p->opSelCap = Rp;
    }
    return GML_OK;
}

// dtheta [R][ld] in, df [R] / dg [R][ldg] out (either may be NULL); raw: f and g as the pass leaves them (logRISE: Z and grad Z, no
// log / division)
static int pass_dev(gml_problem *p, int64_t R, const int64_t *nodes, const double *dtheta, int64_t ld, int form, int precision, bool want_grad,
                    bool f64_fallback, double *df, double *dg, int64_t ldg, const int32_t *dcols, bool raw = false) {
    const int64_t Qp = p->d.Qp, P = p->P, Rp = gml_round_up(R, 32);
    int rc = gml_ensure_ws(p, R);
    if (rc) return rc;
    rc = dev_scratch(p, Rp);
    if (rc) return rc;
    hipStream_t st = p->st;
    std::vector<uint8_t> act((size_t)R, 1), sel((size_t)Rp, 0);
    std::vector<int> groups;
    Rescale rs;
    for (int depth = 0;;) {
        int npad = 0;
        rc = upload_ctl(p, R, nodes, act, groups, &npad);
        if (rc) return rc;
        if (groups.empty()) return GML_OK;
        if (depth == 0) { // (a re-run finds the rows where the first pass put them)
            HIPCHK(hipMemsetAsync(p->opFlag, 0, sizeof(int) * 4, st));
            HIPCHK(hipMemsetAsync(p->dTheta, 0, sizeof(double) * Rp * Qp, st));
            launch_ref_to_internal(dtheta, ld, R, P, Qp, p->dRowcol, p->d.cconst, dcols, p->dTheta, p->opFlag, st);
        }
        if (depth > 0 && (rc = rs.upload(p, Rp))) return rc;
        rc = launch_pass(p, Rp, (int)groups.size(), npad, form, precision, want_grad, false, depth > 0 ? rs.dOvr : nullptr, op_compact(),
                         nullptr);
        if (rc) return rc;
        int bad[4] = {0, 0, 0, 0};
        if (depth == 0) HIPCHK(hipMemcpyAsync(bad, p->opFlag, sizeof bad, hipMemcpyDeviceToHost, st));
        rc = rescale_rows(p, R, act, form, precision, rs);
        if (rc) return rc;
        if (bad[0]) return fail(GML_EINVAL, "theta contains a non-finite value");
        // the rows this pass settled go back to the caller's arrays (a re-run of the others overwrites the workspace rows of its tiles)
        for (int64_t r = 0; r < R; ++r) sel[r] = act[r] && !rs.again[r];
        HIPCHK(hipMemcpyAsync(p->opSel, sel.data(), (size_t)Rp, hipMemcpyHostToDevice, st));
        launch_internal_to_ref(p->dG, p->dF, R, Qp, P, ldg, p->dRowcol, p->opSel, p->d.cconst, dcols, (form == GML_LOGRISE && !raw) ? 1 : 0, df,
                               want_grad ? dg : nullptr, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st)); // (sel is reused; and the call returns with its outputs written)
        if (rs.n == 0) return GML_OK;
        if ((rc = rescale_next(&depth, &precision, &f64_fallback))) return rc;
        act = rs.again;
    }
}

// The argument checks of gml_objgrad_batch and gml_hessvec_batch_prec.  theta and the two arrays `names` lists (b == NULL: as theta)
// are all host or all device pointers; *dev: device (rows resident in HBM).
static int check_rows(gml_problem *p, int formulation, int64_t nrows, const int64_t *nodes, int64_t ld, const double *theta, const double *a,
                      const double *b, const char *names, bool *dev) {
    if (formulation < 0 || formulation > 2) return fail(GML_EINVAL, "unknown formulation %d", formulation);
    if (nrows <= 0) return fail(GML_EINVAL, "nrows must be positive");
    if (ld < p->P) return fail(GML_EINVAL, "ld %lld smaller than the %lld parameters per node", (long long)ld, (long long)p->P);
    for (int64_t r = 0; r < nrows; ++r)
        if (nodes[r] < 0 || nodes[r] >= p->n) return fail(GML_EINVAL, "node id %lld out of range", (long long)nodes[r]);
    HIPCHK(hipSetDevice(p->device));
    const bool td = gml_is_device_ptr(theta), ad = gml_is_device_ptr(a), bd = b ? gml_is_device_ptr(b) : td;
    if (td != ad || td != bd) return fail(GML_EINVAL, "%s must be all host or all device pointers", names);
    *dev = td;
    return GML_OK;
}

// ------------------------------------------------------------------------------------------
// gml_objgrad_batch: the operator (:191-208, :221-233)
// ------------------------------------------------------------------------------------------
extern "C" int gml_objgrad_batch(gml_problem *p, int formulation, int precision, int64_t nrows,
                                 const int64_t *nodes, const double *theta, int64_t ld, double *f, double *g) {
    if (!p || !nodes || !theta || !f) return fail(GML_EINVAL, "NULL argument");
    const bool asked_auto = precision == GML_PREC_AUTO;
    {
        const int asked = precision;
        precision = gml_resolve_precision(p, asked);
        if (precision < 0) return fail(GML_EINVAL, "unknown precision %d", asked);
    }
    bool dev = false;
    int rc = check_rows(p, formulation, nrows, nodes, ld, theta, f, g, "theta, f and g", &dev);
    if (rc) return rc;
    if (dev) {
        const int32_t *dcols = nullptr;
        rc = dev_cols(p, nrows, nodes, &dcols);
        if (rc) return rc;
        return pass_dev(p, nrows, nodes, theta, ld, formulation, precision, g != nullptr, asked_auto, f, g, ld, dcols);
    }
    const int64_t Qp = p->d.Qp;
    std::vector<NodeLayout> lay;
    std::vector<double> Th((size_t)nrows * Qp, 0.0), Gi(g ? (size_t)nrows * Qp : 0), fv((size_t)nrows);
    const int64_t bad = to_internal(p, nrows, nodes, lay, theta, ld, Th.data());
    if (bad >= 0) return fail(GML_EINVAL, "theta of row %lld contains a non-finite value", (long long)bad);
    rc = device_pass(p, nrows, nodes, Th.data(), formulation, precision, g != nullptr, op_compact(), asked_auto, fv.data(), Gi.data());
    if (rc) return rc;
    to_reference(lay, p->P, Qp, formulation, fv.data(), Gi.data(), f, g, ld);
    return GML_OK;
}

// gml_hessvec_batch for rows resident in HBM: the objective pass at theta leaves the curvature weights in the slots, the directions are
// scattered into the internal layout, the Hessian-vector pass runs, a kernel writes hv (logRISE: with the rank-one correction)
static int hessvec_dev(gml_problem *p, int form, int precision, int64_t nrows, const int64_t *nodes, const double *dtheta, const double *dvec,
                       int64_t ld, double *dhv) {
    const int64_t Qp = p->d.Qp, P = p->P, Rp = gml_round_up(nrows, 32);
    const int32_t *dcols = nullptr;
    int rc = dev_cols(p, nrows, nodes, &dcols);
    if (rc) return rc;
    double *G2 = nullptr, *F2 = nullptr;
    if (form == GML_LOGRISE) { // Z and grad Z of every row, in the reference order, kept across the second pass
        if (p->opG2rows < nrows) {
            if (p->opG2) (void)dev_free(p->opG2);
            p->opG2 = nullptr;
            p->opG2rows = 0;
            HIPCHK(dev_malloc(&p->opG2, sizeof(double) * ((size_t)nrows * P + (size_t)Rp)));
            p->opG2rows = nrows;
        }
        G2 = p->opG2;
        F2 = p->opG2 + (size_t)p->opG2rows * P;
    }
    rc = pass_dev(p, nrows, nodes, dtheta, ld, form, precision, true, false, F2, G2, P, dcols, true);
    if (rc) return rc;
    hipStream_t st = p->st;
    std::vector<uint8_t> act((size_t)nrows, 1);
    std::vector<int> groups;
    int npad = 0;
    rc = upload_ctl(p, nrows, nodes, act, groups, &npad);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(p->opFlag, 0, sizeof(int) * 4, st));
    HIPCHK(hipMemsetAsync(p->dTheta, 0, sizeof(double) * Rp * Qp, st));
    launch_ref_to_internal(dvec, ld, nrows, P, Qp, p->dRowcol, p->d.cconst, dcols, p->dTheta, p->opFlag, st);
    rc = launch_pass(p, Rp, (int)groups.size(), npad, form, precision, true, true, nullptr, false, nullptr);
    if (rc) return rc;
    launch_hv_to_ref(p->dG, G2, F2, nrows, Qp, P, ld, p->dRowcol, p->d.cconst, dcols, form == GML_LOGRISE ? 1 : 0, dvec, dhv, st);
    HIPCHK(hipGetLastError());
    int bad[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(bad, p->opFlag, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad[0]) return fail(GML_EINVAL, "vec contains a non-finite value");
    return GML_OK;
}

// ------------------------------------------------------------------------------------------
// gml_hessvec_batch: curvature operator, H_u(theta) v for many nodes at once
// ------------------------------------------------------------------------------------------
extern "C" int gml_hessvec_batch(gml_problem *p, int formulation, int64_t nrows, const int64_t *nodes, const double *theta,
                                 const double *vec, int64_t ld, double *hv) {
    return gml_hessvec_batch_prec(p, formulation, GML_PREC_I8X, nrows, nodes, theta, vec, ld, hv);
}

static int hv_precision(int precision) {
    if (precision == GML_PREC_AUTO) return GML_PREC_I8X; // (an inexact Newton step needs no more; name f64 for the Float64-grade operator)
    if (precision == GML_PREC_I8X || precision == GML_PREC_F64) return precision;
    return -1;
}

extern "C" int gml_hessvec_batch_prec(gml_problem *p, int formulation, int precision, int64_t nrows, const int64_t *nodes, const double *theta,
                                      const double *vec, int64_t ld, double *hv) {
    if (!p || !nodes || !theta || !vec || !hv) return fail(GML_EINVAL, "NULL argument");
    {
        const int asked = precision;
        precision = hv_precision(asked);
        if (precision < 0)
            return fail(asked == GML_PREC_I8W ? GML_EUNSUPPORTED : GML_EINVAL,
                        "Hessian-vector products run at precision i8x (31-bit curvature weights, ~1e-8) or f64 (FP64 MFMA, 1e-12); got %d", asked);
    }
    bool dev = false;
    int rc = check_rows(p, formulation, nrows, nodes, ld, theta, vec, hv, "theta, vec and hv", &dev);
    if (rc) return rc;
    if (dev) return hessvec_dev(p, formulation, precision, nrows, nodes, theta, vec, ld, hv);
    const int64_t Qp = p->d.Qp, Rp = gml_round_up(nrows, 32);
    // 1. objective + gradient pass at theta: leaves the curvature weights (limb planes of V) in the slots 0..nrows-1
    std::vector<NodeLayout> lay;
    std::vector<double> Th((size_t)nrows * Qp, 0.0), Vc((size_t)nrows * Qp, 0.0), Gi((size_t)nrows * Qp), fv((size_t)nrows);
    const int64_t bad = to_internal(p, nrows, nodes, lay, theta, ld, Th.data(), vec, Vc.data());
    if (bad >= 0) return fail(GML_EINVAL, "row %lld contains a non-finite value", (long long)bad);
    rc = device_pass(p, nrows, nodes, Th.data(), formulation, precision, true, op_compact(), false, fv.data(), Gi.data());
    if (rc) return rc;
    // 2. Hessian-vector pass: the rows of the direction through the same slots (vmap = identity)
    hipStream_t st = p->st;
    std::memcpy(p->hTh, Vc.data(), sizeof(double) * nrows * Qp);
    HIPCHK(hipMemcpyAsync(p->dTheta, p->hTh, sizeof(double) * nrows * Qp, hipMemcpyHostToDevice, st));
    // control block of ALL rows: device_pass may have ended on a rescaled re-run of a subset (dense theta rows), which
    // leaves rowcol = -1 for the others and a shortened tile list
    std::vector<uint8_t> act((size_t)nrows, 1);
    std::vector<int> groups;
    int npad = 0;
    rc = upload_ctl(p, nrows, nodes, act, groups, &npad);
    if (rc) return rc;
    rc = launch_pass(p, Rp, (int)groups.size(), npad, formulation, precision, true, true, nullptr, false, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(p->hG, p->dG, sizeof(double) * nrows * Qp, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    to_reference(lay, p->P, Qp, formulation, fv.data(), p->hG, nullptr, hv, ld, Gi.data(), vec);
    return GML_OK;
}

// Test hook (not part of include/gml.h): the working-set Hessian blocks the solver builds its Newton steps from (gml_i8_hess.hip), for
// a few rows at theta -- an int8-limb objective pass leaves the curvature weights in the rows' slots, then i8_hessian runs over the
// configurations of every kstride-th block of 512 (Kh of them).  cols [nrows][m]: the working set of each row as parameter indices
// in the reference's order.  H [nrows][mp][mp] (mp = m rounded up to 32): the lower 32 x 32 tiles of sum_k h_k stat_i stat_j over
// the sub-sample, in the unit of f, not rescaled by the sub-sample's weight.
extern "C" int gml_test_hessian_blocks(gml_problem *p, int formulation, int precision, int64_t nrows, const int64_t *nodes, const double *theta,
                                       int64_t ld, const int32_t *cols, int m, int64_t Kh, int64_t kstride, double *H) {
    if (!p || !nodes || !theta || !cols || !H || nrows <= 0 || m <= 0 || m > 512) return fail(GML_EINVAL, "bad argument");
    if (!gml_is_i8(precision)) return fail(GML_EINVAL, "an int8-limb precision (the planes of V are what the kernel reads)");
    HIPCHK(hipSetDevice(p->device));
    const int64_t Qp = p->d.Qp, P = p->P;
    const int mt = (m + 31) / 32, mp = mt * 32;
    std::vector<NodeLayout> lay;
    std::vector<double> Th((size_t)nrows * Qp, 0.0), Gi((size_t)nrows * Qp), fv((size_t)nrows);
    to_internal(p, nrows, nodes, lay, theta, ld, Th.data());
    std::vector<int> F((size_t)nrows * mp, 0);
    for (int64_t r = 0; r < nrows; ++r)
        for (int a = 0; a < mp; ++a) {
            const int32_t j = cols[r * m + (a < m ? a : 0)]; // (the padding repeats the first entry, as the solver's lists do not care)
            if (j < 0 || j >= P) return fail(GML_EINVAL, "working-set entry out of range");
            F[(size_t)r * mp + a] = lay[r].cols[j];
        }
    int rc = device_pass(p, nrows, nodes, Th.data(), formulation, precision, true, op_compact(), false, fv.data(), Gi.data());
    if (rc) return rc;
    hipStream_t st = p->st;
    std::vector<int> ctl((size_t)(3 * nrows), 0); // rowcol | vslot | mt
    std::vector<long long> hoff((size_t)nrows + 1, 0);
    std::vector<int> hmt((size_t)nrows, mt);
    for (int64_t r = 0; r < nrows; ++r) {
        ctl[r] = (int)nodes[r];
        ctl[nrows + r] = (int)r;
        ctl[2 * nrows + r] = mt;
        hoff[r + 1] = hoff[r] + (long long)mp * mp;
    }
    int *dCtl = nullptr, *dF = nullptr;
    long long *dHoff = nullptr;
    double *dH = nullptr;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(st);
        for (void *q : {(void *)dCtl, (void *)dF, (void *)dHoff, (void *)dH})
            if (q) (void)dev_free_synced(q);
    };
    const size_t htotal = (size_t)nrows * mp * mp;
    hipError_t e = dev_malloc(&dCtl, sizeof(int) * ctl.size());
    if (e == hipSuccess) e = dev_malloc(&dF, sizeof(int) * F.size());
    if (e == hipSuccess) e = dev_malloc(&dHoff, sizeof(long long) * hoff.size());
    if (e == hipSuccess) e = dev_malloc(&dH, sizeof(double) * htotal);
    if (e == hipSuccess) e = hipMemcpyAsync(dCtl, ctl.data(), sizeof(int) * ctl.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dF, F.data(), sizeof(int) * F.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dHoff, hoff.data(), sizeof(long long) * hoff.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(dH, 0, sizeof(double) * htotal, st);
    if (e != hipSuccess) {
        cleanup();
        return fail(GML_EHIP, "gml_test_hessian_blocks: %s", hipGetErrorString(e));
    }
    std::string err;
    rc = gml::i8_hessian(p->i8ws, p->d, dCtl, dCtl + nrows, dF, dCtl + 2 * nrows, hmt.data(), dHoff, (int64_t)htotal, (int)nrows, mp, formulation, Kh, kstride,
                         dH, st, &err, nullptr);
    if (rc == GML_OK) {
        e = hipMemcpyAsync(H, dH, sizeof(double) * htotal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = GML_EHIP;
    }
    cleanup();
    if (rc) return fail(rc, "%s", err.empty() ? "gml_test_hessian_blocks failed" : err.c_str());
    return GML_OK;
}

// Test hook (not part of include/gml.h): the Hessian call of one solver iteration on caller-given blocks -- the flow of
// gml_test_hessian_blocks (device_pass at theta, rescaled re-runs included, then i8_hessian) with what direction_blocks (gml_newton_cg.cpp) can
// hand the call and that hook cannot: a ragged size per row (mtV[r] tiles of 32, 0 = the row is skipped), blocks at caller-given
// offsets, and optionally the preconditioner tiles of matrix-free rows.
//   cols [nrows][cap]: every row's list, parameter indices in the reference's order; all cap entries are translated and uploaded (the
//                      kernels read the first 32 mtV[r] of them), so the padding is the caller's
//   ntiles > 0: T in {64, 128}; tcols [ntiles][T] the tiles' lists, parameters of row wrow[t] in the reference's order; vm [ntiles]
//               (entries in use: uploaded with the control block as direction_blocks lays it out -- hoffV | mtV | vm | wrow | hflag -- the Hessian
//               kernels do not read it), wrow [ntiles], hflag [nrows] (rows whose weights are needed)
//   mtV, hoffV [nrows + ntiles]: tiles of 32 and offset of every block in H (tiles: mtV = T / 32); htotal: elements of H
// precision f64: the FP64 pass, then launch_hess_f64 on its V (the Newton matrices of the FP64 phase); no tiles.
// H [htotal] is cleared first: what no kernel writes stays zero.  tests/test_gpu_i8_hess_exact.py.
extern "C" int gml_test_hessian_run(gml_problem *p, int formulation, int precision, int64_t nrows, const int64_t *nodes, const double *theta,
                                    int64_t ld, const int32_t *cols, int cap, int64_t Kh, int64_t kstride, int T, int ntiles,
                                    const int32_t *tcols, const int32_t *vm, const int32_t *wrow, const int32_t *hflag, const int32_t *mtV,
                                    const int64_t *hoffV, int64_t htotal, double *H) {
    if (!p || !nodes || !theta || !cols || !mtV || !hoffV || !H || nrows <= 0 || nrows > 65535 || htotal <= 0) return fail(GML_EINVAL, "bad argument");
    if (formulation < 0 || formulation > 2) return fail(GML_EINVAL, "unknown formulation %d", formulation);
    const bool f64 = precision == GML_PREC_F64;
    if (!f64 && !gml_is_i8(precision)) return fail(GML_EINVAL, "precision f64, i8x or i8w");
    if (cap <= 0 || cap % 32 || cap > 512) return fail(GML_EINVAL, "cap: a multiple of 32 up to 512");
    if (ntiles < 0 || (ntiles > 0 && (f64 || (T != 64 && T != 128) || !tcols || !vm || !wrow || !hflag))) return fail(GML_EINVAL, "bad tile set");
    const int64_t Qp = p->d.Qp, P = p->P, Kp = p->d.Kp, NV = nrows + ntiles;
    // the sub-sample stays inside the histogram: block cb of the compact index is the samples [512 cb kstride, +512)
    if (Kh <= 0 || Kh % 512 || kstride < 1 || ((Kh / 512 - 1) * kstride + 1) * 512 > Kp) return fail(GML_EINVAL, "bad sub-sample");
    for (int64_t b = 0; b < NV; ++b) {
        const int64_t m = b < nrows ? mtV[b] : T / 32;
        if (mtV[b] != m || m < 0 || m * 32 > (b < nrows ? cap : T) || hoffV[b] < 0 || hoffV[b] + m * 32 * m * 32 > htotal)
            return fail(GML_EINVAL, "block %lld outside H or its list", (long long)b);
    }
    for (int64_t r = 0; r < nrows; ++r)
        if (nodes[r] < 0 || nodes[r] >= p->n) return fail(GML_EINVAL, "node id out of range");
    HIPCHK(hipSetDevice(p->device));
    std::vector<NodeLayout> lay;
    std::vector<double> Th((size_t)nrows * Qp, 0.0), Gi((size_t)nrows * Qp), fv((size_t)nrows);
    if (to_internal(p, nrows, nodes, lay, theta, ld, Th.data()) >= 0) return fail(GML_EINVAL, "a row contains a non-finite value");
    std::vector<int> F((size_t)nrows * cap + (size_t)ntiles * T, 0);
    for (int64_t r = 0; r < nrows; ++r)
        for (int a = 0; a < cap; ++a) {
            const int32_t j = cols[r * cap + a];
            if (j < 0 || j >= P) return fail(GML_EINVAL, "working-set entry out of range");
            F[(size_t)r * cap + a] = lay[r].cols[j];
        }
    for (int64_t t = 0; t < ntiles; ++t) {
        if (wrow[t] < 0 || wrow[t] >= nrows || vm[t] < 1 || vm[t] > T) return fail(GML_EINVAL, "bad tile %lld", (long long)t);
        for (int a = 0; a < T; ++a) {
            const int32_t j = tcols[t * T + a];
            if (j < 0 || j >= P) return fail(GML_EINVAL, "tile entry out of range");
            F[(size_t)nrows * cap + (size_t)t * T + a] = lay[wrow[t]].cols[j];
        }
    }
    int rc = device_pass(p, nrows, nodes, Th.data(), formulation, precision, true, op_compact(), false, fv.data(), Gi.data());
    if (rc) return rc;
    hipStream_t st = p->st;
    // rowcol [R] | vslot [R] (slot = row) | mtV [NV] | vm [ntiles] | wrow [ntiles] | hflag [R]
    std::vector<int> ctl((size_t)(3 * nrows + NV + 2 * ntiles), 0);
    for (int64_t r = 0; r < nrows; ++r) {
        ctl[r] = (int)nodes[r];
        ctl[nrows + r] = (int)r;
        if (ntiles > 0) ctl[2 * nrows + NV + 2 * ntiles + r] = hflag[r];
    }
    for (int64_t b = 0; b < NV; ++b) ctl[2 * nrows + b] = mtV[b];
    for (int64_t t = 0; t < ntiles; ++t) {
        ctl[2 * nrows + NV + t] = vm[t];
        ctl[2 * nrows + NV + ntiles + t] = wrow[t];
    }
    std::vector<long long> hoff(hoffV, hoffV + NV);
    std::vector<int> hmt(mtV, mtV + NV);
    int *dCtl = nullptr, *dF = nullptr;
    long long *dHoff = nullptr;
    double *dH = nullptr;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(st);
        for (void *q : {(void *)dCtl, (void *)dF, (void *)dHoff, (void *)dH})
            if (q) (void)dev_free_synced(q);
    };
    hipError_t e = dev_malloc(&dCtl, sizeof(int) * ctl.size());
    if (e == hipSuccess) e = dev_malloc(&dF, sizeof(int) * F.size());
    if (e == hipSuccess) e = dev_malloc(&dHoff, sizeof(long long) * hoff.size());
    if (e == hipSuccess) e = dev_malloc(&dH, sizeof(double) * (size_t)htotal);
    if (e == hipSuccess) e = hipMemcpyAsync(dCtl, ctl.data(), sizeof(int) * ctl.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dF, F.data(), sizeof(int) * F.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dHoff, hoff.data(), sizeof(long long) * hoff.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(dH, 0, sizeof(double) * (size_t)htotal, st);
    if (e != hipSuccess) {
        cleanup();
        return fail(GML_EHIP, "gml_test_hessian_run: %s", hipGetErrorString(e));
    }
    const int *dMtV = dCtl + 2 * nrows;
    std::string err;
    if (f64) {
        launch_hess_f64(p->d, p->dV, dCtl, dF, dMtV, dHoff, (int)nrows, cap, formulation, Kh, kstride, dH, st);
        if (hipGetLastError() != hipSuccess) rc = GML_EHIP;
    } else {
        gml::HessTiles tl;
        if (ntiles > 0) {
            tl.n = ntiles;
            tl.T = T;
            tl.F = dF + (size_t)nrows * cap;
            tl.wrow = dMtV + NV + ntiles;
            tl.hflag = dMtV + NV + 2 * ntiles;
        }
        rc = gml::i8_hessian(p->i8ws, p->d, dCtl, dCtl + nrows, dF, dMtV, hmt.data(), dHoff, htotal, (int)nrows, cap, formulation, Kh, kstride, dH, st, &err,
                             ntiles > 0 ? &tl : nullptr);
    }
    if (rc == GML_OK) {
        e = hipMemcpyAsync(H, dH, sizeof(double) * (size_t)htotal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = GML_EHIP;
    }
    cleanup();
    if (rc) return fail(rc, "%s", err.empty() ? "gml_test_hessian_run failed" : err.c_str());
    return GML_OK;
}

// Test hook (not part of include/gml.h): one Hessian-vector product two ways.  device_pass runs the objective pass (RISE or logRISE, i8x
// or i8w; rescaled re-runs included) over the rows (nodes, theta), which leaves their curvature weights in the slots 0 .. nrows.  Then,
// for the nloc product rows -- row i multiplies the weights of slot vslot[i] with the direction vec[i] -- through the solver's own
// product call (hv_product_call, gml_newton_cg.cpp: its control block, its arguments), once per route:
//   hs: i8_hv_sparse over the caller's lists: row i's nw[i] entries at FV[t0[i] T ..] (parameters of node nodes[vslot[i]] in the
//       reference's order), wcap >= every nw, the plan (kchunk, kpart);
//   hg: the GEMM pass with hv = 2, lf = 2 and the same (kchunk, kpart), slot i <- (row i, node, vmap = vslot[i]).
// kchunk = 0: the plan i8_split_plan makes for all configurations.  The entry-by-entry form runs FIRST: the GEMM pass rewrites Tq, Uq
// and the product scalars (sc[1]), none of which the entry-by-entry form reads, and neither touches the V planes or sc[0]; run first, it is
// also seen to need nothing the GEMM pass leaves behind.
// hs, hg [nloc][Qp] in the internal column order, both filled with `fill` beforehand (the entry-by-entry form writes the listed entries
// only); colmap [nloc][P]: the internal column of every parameter.  tests/test_gpu_hv_sparse_direct.py.
extern "C" int gml_test_hv_sparse(gml_problem *p, int formulation, int precision, int64_t nrows, const int64_t *nodes, const double *theta,
                                  int64_t ld, int64_t nloc, const int32_t *vslot, const double *vec, const int32_t *FV, const int64_t *t0,
                                  const int32_t *nw, int T, int64_t wcap, int64_t kchunk, int64_t kpart, double fill, double *hs, double *hg,
                                  int32_t *colmap) {
    if (!p || !nodes || !theta || !vslot || !vec || !FV || !t0 || !nw || !hs || !hg || !colmap || nrows <= 0 || nloc <= 0 || nloc > 65535 || T <= 0)
        return fail(GML_EINVAL, "bad argument");
    if (formulation != GML_RISE && formulation != GML_LOGRISE) return fail(GML_EINVAL, "an exp form");
    if (!gml_is_i8(precision)) return fail(GML_EINVAL, "an int8-limb precision");
    const int64_t Qp = p->d.Qp, P = p->P, np = gml_round_up(nloc, 32);
    if (wcap < 1 || wcap > 65536 || kchunk < 0 || kchunk % 256 || kpart < 0 || kpart % 256 || (kchunk > 0 && (kpart == 0 || kpart > kchunk)))
        return fail(GML_EINVAL, "bad wcap or plan");
    for (int64_t r = 0; r < nrows; ++r)
        if (nodes[r] < 0 || nodes[r] >= p->n) return fail(GML_EINVAL, "node id out of range");
    int64_t fvlen = 0;
    std::vector<int64_t> lnodes((size_t)nloc);
    for (int64_t i = 0; i < nloc; ++i) {
        if (vslot[i] < 0 || vslot[i] >= nrows || nw[i] < 1 || nw[i] > wcap || t0[i] < 0) return fail(GML_EINVAL, "bad product row %lld", (long long)i);
        fvlen = std::max<int64_t>(fvlen, t0[i] * T + nw[i]);
        lnodes[i] = nodes[vslot[i]];
    }
    HIPCHK(hipSetDevice(p->device));
    int rc = gml_ensure_ws(p, std::max(nrows, nloc));
    if (rc) return rc;
    std::vector<NodeLayout> lay, llay;
    std::vector<double> Th((size_t)nrows * Qp, 0.0), Gi((size_t)nrows * Qp), fv((size_t)nrows), Pv((size_t)nloc * Qp, 0.0);
    if (to_internal(p, nrows, nodes, lay, theta, ld, Th.data()) >= 0) return fail(GML_EINVAL, "a row contains a non-finite value");
    if (to_internal(p, nloc, lnodes.data(), llay, vec, ld, Pv.data()) >= 0) return fail(GML_EINVAL, "a direction contains a non-finite value");
    std::vector<int> Fi((size_t)fvlen, 0);
    for (int64_t i = 0; i < nloc; ++i) {
        std::memcpy(colmap + i * P, llay[i].cols.data(), sizeof(int32_t) * P);
        for (int a = 0; a < nw[i]; ++a) {
            const int32_t j = FV[t0[i] * T + a];
            if (j < 0 || j >= P) return fail(GML_EINVAL, "list entry out of range");
            Fi[(size_t)(t0[i] * T + a)] = llay[i].cols[j];
        }
    }
    rc = device_pass(p, nrows, nodes, Th.data(), formulation, precision, true, op_compact(), false, fv.data(), Gi.data());
    if (rc) return rc;
    hipStream_t st = p->st;
    if (kchunk == 0) {
        int nsplit = 0;
        gml::i8_split_plan(p->d, (int)(np / 32), 1, &kchunk, &kpart, &nsplit);
    }
    // the solver's control block of a product (product row i = row i of vec), then the lists' sizes: nw [nloc]
    const gml::cg::HvCtl L(nloc);
    std::vector<int> ctl = L.pack([&](int64_t a) { return std::array<int, 3>{(int)a, (int)lnodes[a], vslot[a]}; });
    ctl.insert(ctl.end(), nw, nw + nloc);
    std::vector<long long> t0l(t0, t0 + nloc);
    std::vector<double> init((size_t)nloc * Qp, fill);
    const size_t bufb = gml::i8_hv_sparse_bytes(p->d, (int)nloc, wcap);
    int *dCtl = nullptr, *dFV = nullptr;
    long long *dT0 = nullptr;
    double *dP = nullptr, *dHs = nullptr, *dHg = nullptr;
    char *dBuf = nullptr;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(st);
        for (void *q : {(void *)dCtl, (void *)dFV, (void *)dT0, (void *)dP, (void *)dHs, (void *)dHg, (void *)dBuf})
            if (q) (void)dev_free_synced(q);
    };
    const size_t rowb = sizeof(double) * (size_t)np * Qp; // (the GEMM pass writes the rows of whole slot tiles)
    hipError_t e = dev_malloc(&dCtl, sizeof(int) * ctl.size());
    if (e == hipSuccess) e = dev_malloc(&dFV, sizeof(int) * Fi.size());
    if (e == hipSuccess) e = dev_malloc(&dT0, sizeof(long long) * t0l.size());
    if (e == hipSuccess) e = dev_malloc(&dP, rowb);
    if (e == hipSuccess) e = dev_malloc(&dHs, rowb);
    if (e == hipSuccess) e = dev_malloc(&dHg, rowb);
    if (e == hipSuccess) e = dev_malloc(&dBuf, bufb);
    if (e == hipSuccess) e = hipMemcpyAsync(dCtl, ctl.data(), sizeof(int) * ctl.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dFV, Fi.data(), sizeof(int) * Fi.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dT0, t0l.data(), sizeof(long long) * t0l.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(dP, 0, rowb, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dP, Pv.data(), sizeof(double) * (size_t)nloc * Qp, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(dHs, 0, rowb, st);
    if (e == hipSuccess) e = hipMemsetAsync(dHg, 0, rowb, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dHs, init.data(), sizeof(double) * (size_t)nloc * Qp, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dHg, init.data(), sizeof(double) * (size_t)nloc * Qp, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) {
        cleanup();
        return fail(GML_EHIP, "gml_test_hv_sparse: %s", hipGetErrorString(e));
    }
    std::string err;
    const gml::WList wl{dFV, dT0, dCtl + L.size(), T};
    const gml::HvPlan plan{kchunk, kpart, 2, 2};
    rc = gml::hv_product_call(&p->i8ws, p->d, p->ws_rows, formulation, true, L, dCtl, wl, wcap, dBuf, plan, dP, dHs, st, &err);
    if (rc == GML_OK) rc = gml::hv_product_call(&p->i8ws, p->d, p->ws_rows, formulation, false, L, dCtl, wl, wcap, dBuf, plan, dP, dHg, st, &err);
    if (rc == GML_OK) {
        e = hipMemcpyAsync(hs, dHs, sizeof(double) * (size_t)nloc * Qp, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(hg, dHg, sizeof(double) * (size_t)nloc * Qp, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = GML_EHIP;
    }
    cleanup();
    if (rc) return fail(rc, "%s", err.empty() ? "gml_test_hv_sparse failed" : err.c_str());
    return GML_OK;
}

// Test hook (not part of include/gml.h): ONE objective pass over caller-given rows in a form the public entry points do not choose, and
// optionally one Hessian-vector pass after it, with no rescaled re-runs.  Host pointers; rows in the reference's parameter order.
//   kn [11]: coarse, lf (0 / 3 / 4 / 5), want_grad, compact, zero_theta, then the product pass: hv (0 = none, 1, 2), its lf (2 .. 5),
//            ksub, kchunk, kpart (0: planned in the pass)
//   tauovr [nrows] or NULL: the per-row scale of V imposed on the objective pass (the operator's rescaled re-run), 0 = from the bound
//   vec [nrows][ld]: the directions (read when hv)
//   vslot [nrows] or NULL (gml_test_i8_pass: NULL): product row i, in slot i, multiplies the weights of slot vslot[i] -- its node is
//            nodes[vslot[i]], in whose parameter order vec[i] and hv[i] are -- so that one slot's V can serve several directions
// Out: f [nrows] and g [nrows][ld] (may be NULL) of the objective pass, hv [nrows][ld] of the products, all as the passes leave them
// (logRISE: Z, grad Z and Hess Z v, without the log finish); slots [2][nrows][3] = {f, tau, mmax} of every row in each pass (each pass's
// SlotResult); plan [2] = the kchunk, kpart of the product pass.
extern "C" int gml_test_i8_pass_vslot(gml_problem *p, int formulation, int precision, int64_t nrows, const int64_t *nodes, const double *theta,
                                      const double *tauovr, const double *vec, int64_t ld, const int64_t *kn, double *f, double *g, double *hv,
                                      double *slots, int64_t *plan, const int32_t *vslot) {
    if (!p || !nodes || !theta || !kn || !f || !slots) return fail(GML_EINVAL, "NULL argument");
    if (precision != GML_PREC_F64 && !gml_is_i8(precision)) return fail(GML_EINVAL, "unknown precision %d", precision);
    const int hvk = (int)kn[5];
    if (hvk && (!vec || !hv)) return fail(GML_EINVAL, "a product pass needs vec and hv");
    if (vslot && (!hvk || !gml_is_i8(precision))) return fail(GML_EINVAL, "a slot map belongs to a product pass of an int8-limb precision");
    bool dev = false;
    int rc = check_rows(p, formulation, nrows, nodes, ld, theta, f, nullptr, "theta and f", &dev);
    if (rc) return rc;
    if (dev) return fail(GML_EINVAL, "gml_test_i8_pass takes host pointers");
    const int64_t Qp = p->d.Qp, Rp = gml_round_up(nrows, 32);
    if ((rc = gml_ensure_ws(p, nrows))) return rc;
    hipStream_t st = p->st;
    std::vector<NodeLayout> lay, llay;
    std::vector<double> Th((size_t)nrows * Qp, 0.0), Vc((size_t)nrows * Qp, 0.0), Gi((size_t)nrows * Qp, 0.0), Hi((size_t)nrows * Qp, 0.0),
        fv((size_t)Rp, 0.0);
    std::vector<int64_t> lnodes; // slot map: the node of every product row
    std::vector<int> vm;
    if (vslot) {
        lnodes.resize((size_t)nrows);
        vm.assign((size_t)Rp, 0);
        for (int64_t i = 0; i < nrows; ++i) {
            if (vslot[i] < 0 || vslot[i] >= nrows) return fail(GML_EINVAL, "slot map entry %lld out of range", (long long)i);
            lnodes[i] = nodes[vslot[i]];
            vm[i] = vslot[i];
        }
    }
    const bool own = hvk && !vslot; // the directions in the layout of the rows' own nodes
    if (to_internal(p, nrows, nodes, lay, theta, ld, Th.data(), own ? vec : nullptr, own ? Vc.data() : nullptr) >= 0)
        return fail(GML_EINVAL, "a row contains a non-finite value");
    if (vslot && to_internal(p, nrows, lnodes.data(), llay, vec, ld, Vc.data()) >= 0) return fail(GML_EINVAL, "a direction contains a non-finite value");
    std::vector<uint8_t> act((size_t)nrows, 1);
    std::vector<int> groups;
    int npad = 0;
    if ((rc = upload_ctl(p, nrows, nodes, act, groups, &npad))) return rc;
    Rescale rs;
    if (tauovr) {
        rs.ovr.assign((size_t)Rp, 0.0);
        std::copy(tauovr, tauovr + nrows, rs.ovr.begin());
        if ((rc = rs.upload(p, Rp))) return rc;
    }
    gml::SlotResult *dRes = nullptr;
    int *dVmap = nullptr;
    HIPCHK(dev_malloc(&dRes, sizeof(gml::SlotResult) * 2 * Rp));
    hipError_t e0 = hipMemsetAsync(dRes, 0, sizeof(gml::SlotResult) * 2 * Rp, st);
    if (e0 == hipSuccess && vslot) e0 = dev_malloc(&dVmap, sizeof(int) * Rp);
    if (e0 == hipSuccess && vslot) e0 = hipMemcpyAsync(dVmap, vm.data(), sizeof(int) * Rp, hipMemcpyHostToDevice, st);
    if (e0 != hipSuccess) {
        (void)hipStreamSynchronize(st);
        (void)dev_free(dRes);
        if (dVmap) (void)dev_free(dVmap);
        return fail(GML_EHIP, "gml_test_i8_pass: %s", hipGetErrorString(e0));
    }
    std::vector<gml::SlotResult> res((size_t)2 * Rp);
    auto run = [&]() -> int {
        PassKnobs k;
        k.coarse = kn[0] != 0;
        k.lf = (int)kn[1];
        k.zero_theta = kn[4] != 0;
        k.res = dRes;
        const bool want_grad = kn[2] != 0;
        std::memcpy(p->hTh, Th.data(), sizeof(double) * nrows * Qp);
        HIPCHK(hipMemcpyAsync(p->dTheta, p->hTh, sizeof(double) * nrows * Qp, hipMemcpyHostToDevice, st));
        int rc2 = launch_pass(p, Rp, (int)groups.size(), npad, formulation, precision, want_grad, false, tauovr ? rs.dOvr : nullptr,
                              kn[3] != 0, nullptr, &k);
        if (rc2) return rc2;
        HIPCHK(hipMemcpyAsync(p->hF, p->dF, sizeof(double) * Rp, hipMemcpyDeviceToHost, st));
        if (want_grad) HIPCHK(hipMemcpyAsync(p->hG, p->dG, sizeof(double) * nrows * Qp, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        std::memcpy(fv.data(), p->hF, sizeof(double) * Rp);
        if (want_grad) std::memcpy(Gi.data(), p->hG, sizeof(double) * nrows * Qp);
        if (!hvk) return GML_OK;
        PassKnobs k2;
        k2.hv = hvk;
        k2.lf = (int)kn[6];
        k2.ksub = (int)kn[7];
        k2.kchunk = kn[8];
        k2.kpart = kn[9];
        k2.res = dRes + Rp;
        k2.plan_out = plan;
        k2.vmap = dVmap;
        if (vslot) { // (the stream is idle: the control block's pinned twin is free) slot i <- (row i, node of slot vslot[i])
            int rc3 = upload_ctl(p, nrows, lnodes.data(), act, groups, &npad);
            if (rc3) return rc3;
        }
        std::memcpy(p->hTh, Vc.data(), sizeof(double) * nrows * Qp);
        HIPCHK(hipMemcpyAsync(p->dTheta, p->hTh, sizeof(double) * nrows * Qp, hipMemcpyHostToDevice, st));
        rc2 = launch_pass(p, Rp, (int)groups.size(), npad, formulation, precision, true, true, nullptr, false, nullptr, &k2);
        if (rc2) return rc2;
        HIPCHK(hipMemcpyAsync(p->hG, p->dG, sizeof(double) * nrows * Qp, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        std::memcpy(Hi.data(), p->hG, sizeof(double) * nrows * Qp);
        return GML_OK;
    };
    rc = run();
    if (rc == GML_OK) {
        hipError_t e = hipMemcpyAsync(res.data(), dRes, sizeof(gml::SlotResult) * 2 * Rp, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = fail(GML_EHIP, "gml_test_i8_pass: %s", hipGetErrorString(e));
    }
    (void)hipStreamSynchronize(st);
    (void)dev_free(dRes);
    if (dVmap) (void)dev_free(dVmap);
    if (rc) return rc;
    // (raw sums: the layout gather of RISE, which leaves logRISE's Z and grad Z as they are)
    to_reference(lay, p->P, Qp, GML_RISE, fv.data(), Gi.data(), f, kn[2] ? g : nullptr, ld);
    if (hvk) to_reference(vslot ? llay : lay, p->P, Qp, GML_RISE, fv.data(), Hi.data(), nullptr, hv, ld);
    for (int pass = 0; pass < 2; ++pass)
        for (int64_t r = 0; r < nrows; ++r) {
            const gml::SlotResult &s = res[(size_t)pass * Rp + r];
            double *o = slots + ((size_t)pass * nrows + r) * 3;
            o[0] = s.f;
            o[1] = s.tau;
            o[2] = (double)s.mmax;
        }
    return GML_OK;
}

extern "C" int gml_test_i8_pass(gml_problem *p, int formulation, int precision, int64_t nrows, const int64_t *nodes, const double *theta,
                                const double *tauovr, const double *vec, int64_t ld, const int64_t *kn, double *f, double *g, double *hv,
                                double *slots, int64_t *plan) {
    return gml_test_i8_pass_vslot(p, formulation, precision, nrows, nodes, theta, tauovr, vec, ld, kn, f, g, hv, slots, plan, nullptr);
}

// Timing hook with the parameters RESIDENT in HBM: Theta is uploaded once, then `warmup + steps` passes run back
// to back on the handle's stream with no host round trip (a device-side optimiser would call the operator this
// way); f and the gradient of the last pass are downloaded once at the end.  kernel_ms[3] = device time per pass.
extern "C" int gml_bench_pass_resident(gml_problem *p, int formulation, int precision, const double *theta, int steps,
                                       int warmup, double kernel_ms[4], double *f_out, double *g_out, double *step_ms) {
    if (!p || !kernel_ms || !theta || steps < 1 || warmup < 0) return fail(GML_EINVAL, "bad argument");
    if (formulation < 0 || formulation > 2) return fail(GML_EINVAL, "unknown formulation %d", formulation);
    HIPCHK(hipSetDevice(p->device));
    const int64_t R = p->node1 - p->node0, Qp = p->d.Qp, P = p->P, Rp = gml_round_up(R, 32);
    int rc = gml_ensure_ws(p, R);
    if (rc) return rc;
    hipStream_t st = p->st;
    std::vector<int64_t> nodes((size_t)R);
    std::iota(nodes.begin(), nodes.end(), p->node0);
    std::vector<NodeLayout> lay;
    std::memset(p->hTh, 0, sizeof(double) * Rp * Qp);
    to_internal(p, R, nodes.data(), lay, theta, P, p->hTh);
    HIPCHK(hipMemcpyAsync(p->dTheta, p->hTh, sizeof(double) * Rp * Qp, hipMemcpyHostToDevice, st));
    std::vector<uint8_t> act((size_t)R, 1);
    std::vector<int> groups;
    int npad = 0;
    rc = upload_ctl(p, R, nodes.data(), act, groups, &npad);
    if (rc) return rc;
    {
        const int asked = precision;
        precision = gml_resolve_precision(p, asked);
        if (precision < 0) return fail(GML_EINVAL, "unknown precision %d", asked);
    }
    std::vector<hipEvent_t> ev((size_t)3 * steps, nullptr);
    for (auto &e : ev) HIPCHK(hipEventCreate(&e));
    for (int s = 0; s < warmup + steps; ++s) {
        rc = launch_pass(p, Rp, (int)groups.size(), npad, formulation, precision, true, false, nullptr, bench_compact(),
                         s >= warmup ? ev.data() + (size_t)3 * (s - warmup) : nullptr);
        if (rc) return rc;
    }
    hipEvent_t e_end = nullptr;
    HIPCHK(hipEventCreate(&e_end));
    HIPCHK(hipEventRecord(e_end, st));
    HIPCHK(hipMemcpyAsync(p->hF, p->dF, sizeof(double) * Rp, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(p->hG, p->dG, sizeof(double) * Rp * Qp, hipMemcpyDeviceToHost, st));
    std::vector<unsigned> mm;
    if (gml_is_i8(precision) && formulation != GML_RPLE) {
        mm.resize((size_t)Rp);
        const double *tau_ = nullptr;
        const unsigned *mm_ = nullptr;
        gml::i8_slot_results(p->i8ws, 0, &tau_, &mm_);
        HIPCHK(hipMemcpyAsync(mm.data(), mm_, sizeof(unsigned) * Rp, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (size_t r = 0; r < mm.size() && (int64_t)r < R; ++r)
        if (mm[r] < (1u << 23))
            return fail(GML_EUNSUPPORTED, "row %zu uses fewer than 23 bits of the fixed-point range at this theta: time it through "
                                         "gml_bench_pass (which rescales)", r);
    double sum[2] = {0, 0};
    float ms = 0;
    for (int s = 0; s < steps; ++s) {
        HIPCHK(hipEventElapsedTime(&ms, ev[(size_t)3 * s], ev[(size_t)3 * s + 1]));
        sum[0] += ms;
        HIPCHK(hipEventElapsedTime(&ms, ev[(size_t)3 * s + 1], ev[(size_t)3 * s + 2]));
        sum[1] += ms;
    }
    if (step_ms) // device time of every pass: from its forward launch to the next pass's (the last one: to the end)
        for (int s = 0; s < steps; ++s) {
            HIPCHK(hipEventElapsedTime(&ms, ev[(size_t)3 * s], s + 1 < steps ? ev[(size_t)3 * (s + 1)] : e_end));
            step_ms[s] = ms;
        }
    HIPCHK(hipEventElapsedTime(&ms, ev[0], e_end));
    kernel_ms[0] = sum[0] / steps;
    kernel_ms[1] = sum[1] / steps;
    kernel_ms[2] = kernel_ms[0] + kernel_ms[1];
    kernel_ms[3] = ms / steps; // from the first timed forward launch to the end of the last pass (quantisation of pass 1 excluded)
    for (auto &e : ev) (void)hipEventDestroy(e);
    (void)hipEventDestroy(e_end);

    if (f_out || g_out) to_reference(lay, P, Qp, formulation, p->hF, p->hG, f_out, g_out, P);
    return GML_OK;
}

extern "C" int gml_bench_pass(gml_problem *p, int formulation, int precision, const double *theta, int steps,
                              int warmup, double kernel_ms[3]) {
    if (!p || !kernel_ms) return fail(GML_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(p->device));
    const int64_t R = p->node1 - p->node0, Qp = p->d.Qp;
    std::vector<int64_t> nodes((size_t)R);
    std::iota(nodes.begin(), nodes.end(), p->node0);
    std::vector<double> Th((size_t)R * Qp, 0.0), Gi((size_t)R * Qp), fv((size_t)R);
    if (theta) {
        std::vector<NodeLayout> lay;
        to_internal(p, R, nodes.data(), lay, theta, p->P, Th.data());
    }
    double sum[2] = {0, 0};
    for (int s = 0; s < warmup + steps; ++s) {
        float ms[2] = {0, 0};
        int rc = device_pass(p, R, nodes.data(), Th.data(), formulation, precision, true, bench_compact(), false, fv.data(), Gi.data(), ms);
        if (rc) return rc;
        if (s >= warmup) {
            sum[0] += ms[0];
            sum[1] += ms[1];
        }
    }
    kernel_ms[0] = sum[0] / steps;
    kernel_ms[1] = sum[1] / steps;
    kernel_ms[2] = kernel_ms[0] + kernel_ms[1];
    return GML_OK;
}
