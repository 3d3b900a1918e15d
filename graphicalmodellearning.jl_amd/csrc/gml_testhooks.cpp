// libgml_hip: test and experiment hooks (not part of include/gml.h).
#include "gml_internal.h"
#include "gml_i8.h"
#include "gml_i8_hw.h"
#include "gml_solver.h"
#include "gml_pack.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <thread>

using namespace gml;

namespace gml {
double g_hv_sparse_ratio = 0.3; // (config 5 at the default regulariser: 25.6 s never, 23.6 s at 0.3 and at 0.6)
std::atomic<long long> g_hv_sparse_calls{0}; // (every part of a gml_multi_learn counts from its own host thread)
int g_term_chains_tile = 0;                   // 0: the rule of term_chains_tile (gml_term_chains.hip)
double g_tune[GML_NTUNE] = {};               // experiment knobs of the solver, 0 = the built-in rule (gml_solver.h)
// the kernel instances the int8-limb launchers have run (gml_i8.h: kI8InstBits)
static std::atomic<uint64_t> g_i8_inst[(kI8InstBits + 63) / 64];
void i8_note_instance(int bit) { g_i8_inst[bit >> 6].fetch_or(1ull << (bit & 63), std::memory_order_relaxed); }
}
// The record of launched int8-limb kernel instances (bit numbering: gml_i8.h): copies the first n words to out (if not NULL) and
// clears the record when reset is set.  Host memory only.  Returns the number of words of the record.
extern "C" int gml_test_i8_instances(uint64_t *out, int n, int reset) {
    constexpr int nw = (kI8InstBits + 63) / 64;
    for (int i = 0; i < nw; ++i) {
        const uint64_t v = reset ? g_i8_inst[i].exchange(0, std::memory_order_relaxed) : g_i8_inst[i].load(std::memory_order_relaxed);
        if (out && i < n) out[i] = v;
    }
    return nw;
}
// the solver's switch between the GEMM form and the entry-by-entry form of a Hessian-vector pass (gml_solver.h); returns the old value
extern "C" long long gml_test_hv_sparse_calls(void) { return g_hv_sparse_calls.load(); }
// experiment knob `id` of the solver (gml_solver.h: GML_TUNE_*); returns the old value.  Not part of include/gml.h; set between solves only
extern "C" double gml_test_tune(int id, double value) {
    if (id < 0 || id >= GML_NTUNE) return NAN;
    const double old = g_tune[id];
    g_tune[id] = value;
    return old;
}
// forces the chain tile of the term-list chain kernel (64, 128 or 256 chains; 0 = its rule); returns the old value, -1 for another T.
// A forced tile whose state does not fit the kernel's LDS budget is not used.  Set between calls only
extern "C" int gml_test_term_chains_tile(int T) {
    if (T != 0 && T != 64 && T != 128 && T != 256) return -1;
    const int old = g_term_chains_tile;
    g_term_chains_tile = T;
    return old;
}
extern "C" double gml_test_hv_sparse_ratio(double ratio) {
    const double old = g_hv_sparse_ratio;
    g_hv_sparse_ratio = ratio;
    return old;
}


extern "C" int gml_test_tile_precond(int T, int ntiles, const int *m, const double *tiles /* ntiles x T x T */, double s1, double s2,
                                     const double *g /* ntiles x T */, const double *r /* ntiles x T */, double *z_out /* ntiles x T */,
                                     int device) {
    if ((T != 64 && T != 128) || ntiles <= 0) return fail(GML_EINVAL, "bad tile size");
    HIPCHK(hipSetDevice(device));
    const size_t nt = (size_t)ntiles, ne = nt * T;
    std::vector<long long> hoff(nt);
    std::vector<int> wrow(nt, 0), fv(ne), live(1, 1);
    for (size_t t = 0; t < nt; ++t) hoff[t] = (long long)t * T * T;
    for (size_t e = 0; e < ne; ++e) fv[e] = (int)e; // tile t owns the columns [t T, (t + 1) T) of the one row
    double *dH = nullptr, *dS1 = nullptr, *dG = nullptr, *dR = nullptr, *dZ = nullptr;
    long long *dHoff = nullptr;
    int *dM = nullptr, *dWrow = nullptr, *dFv = nullptr, *dLive = nullptr;
    auto freeall = [&]() {
        void *ptrs[] = {dH, dS1, dG, dR, dZ, dHoff, dM, dWrow, dFv, dLive};
        for (void *q : ptrs)
            if (q) (void)dev_free(q);
    };
#define TCHK2(expr)                                                                              \
    do {                                                                                        \
        if ((expr) != hipSuccess) {                                                             \
            freeall();                                                                          \
            return fail(GML_EHIP, "%s failed: %s", #expr, hipGetErrorString(hipGetLastError())); \
        }                                                                                       \
    } while (0)
    TCHK2(dev_malloc(&dH, sizeof(double) * ne * T));
    TCHK2(dev_malloc(&dS1, sizeof(double)));
    TCHK2(dev_malloc(&dG, sizeof(double) * ne));
    TCHK2(dev_malloc(&dR, sizeof(double) * ne));
    TCHK2(dev_malloc(&dZ, sizeof(double) * ne));
    TCHK2(dev_malloc(&dHoff, sizeof(long long) * nt));
    TCHK2(dev_malloc(&dM, sizeof(int) * nt));
    TCHK2(dev_malloc(&dWrow, sizeof(int) * nt));
    TCHK2(dev_malloc(&dFv, sizeof(int) * ne));
    TCHK2(dev_malloc(&dLive, sizeof(int)));
    TCHK2(hipMemcpy(dH, tiles, sizeof(double) * ne * T, hipMemcpyHostToDevice));
    TCHK2(hipMemcpy(dS1, &s1, sizeof(double), hipMemcpyHostToDevice));
    TCHK2(hipMemcpy(dG, g, sizeof(double) * ne, hipMemcpyHostToDevice));
    TCHK2(hipMemcpy(dR, r, sizeof(double) * ne, hipMemcpyHostToDevice));
    TCHK2(hipMemset(dZ, 0, sizeof(double) * ne));
    TCHK2(hipMemcpy(dHoff, hoff.data(), sizeof(long long) * nt, hipMemcpyHostToDevice));
    TCHK2(hipMemcpy(dM, m, sizeof(int) * nt, hipMemcpyHostToDevice));
    TCHK2(hipMemcpy(dWrow, wrow.data(), sizeof(int) * nt, hipMemcpyHostToDevice));
    TCHK2(hipMemcpy(dFv, fv.data(), sizeof(int) * ne, hipMemcpyHostToDevice));
    TCHK2(hipMemcpy(dLive, live.data(), sizeof(int), hipMemcpyHostToDevice));
    launch_tile_inverse(T, dH, dHoff, dM, dWrow, dS1, s2, dG, ntiles, nullptr);
    launch_tile_apply(T, dH, dFv, dM, dWrow, dLive, ntiles, (int64_t)ne, dR, dZ, nullptr);
    TCHK2(hipGetLastError());
    TCHK2(hipDeviceSynchronize());
    TCHK2(hipMemcpy(z_out, dZ, sizeof(double) * ne, hipMemcpyDeviceToHost));
#undef TCHK2
    freeall();
    return GML_OK;
}

// Test hook (not part of include/gml.h): the batched Newton solve on caller-given blocks -- A_r d_r = -pg_r for R symmetric positive
// definite m_r x m_r blocks (row-major, m_r <= cap <= 512), exactly as gml_learn's direction phase calls it.  tests/test_gpu_newton_solve.py.
static int test_newton_solve(int R, const int *m, int cap, const double *blocks, const double *pg, double s2, const double *g, double *d_out,
                             int device, const unsigned char *fix /* R x cap or NULL */, const double *dfix /* R x cap */) {
    HIPCHK(hipSetDevice(device));
    std::vector<long long> hoff((size_t)R + 1, 0);
    std::vector<int> mt((size_t)R);
    int maxm = 0;
    for (int r = 0; r < R; ++r) {
        if (m[r] < 0 || m[r] > cap || cap > 512) return fail(GML_EINVAL, "bad block size");
        mt[r] = (m[r] + 31) / 32;
        hoff[r + 1] = hoff[r] + (long long)mt[r] * 32 * mt[r] * 32;
        maxm = std::max(maxm, m[r]);
    }
    std::vector<double> H((size_t)std::max<long long>(hoff[R], 1), 0.0), s1((size_t)R, 1.0), gz((size_t)R * cap, 0.0);
    for (int r = 0; r < R; ++r) {
        const int hp = 32 * mt[r];
        for (int i = 0; i < m[r]; ++i)
            for (int j = 0; j < m[r]; ++j) H[(size_t)hoff[r] + (size_t)i * hp + j] = blocks[((size_t)r * cap + i) * cap + j];
        for (int i = m[r]; i < hp; ++i) H[(size_t)hoff[r] + (size_t)i * hp + i] = 1.0; // padding: identity
    }
    double *dH = nullptr, *dS1 = nullptr, *dG = nullptr, *dPg = nullptr, *dOut = nullptr, *dSd = nullptr, *dDfix = nullptr;
    long long *dHoff = nullptr;
    int *dMt = nullptr, *dM = nullptr, *dRedo = nullptr;
    uint8_t *dFix = nullptr;
    auto freeall = [&]() {
        void *ptrs[] = {dH, dS1, dG, dPg, dOut, dSd, dHoff, dMt, dM, dDfix, dRedo, dFix};
        for (void *q : ptrs)
            if (q) (void)dev_free(q);
    };
#define TCHK(expr)                                                           \
    do {                                                                     \
        if ((expr) != hipSuccess) {                                          \
            freeall();                                                       \
            return fail(GML_EHIP, "%s failed: %s", #expr, hipGetErrorString(hipGetLastError())); \
        }                                                                    \
    } while (0)
    TCHK(dev_malloc(&dH, sizeof(double) * H.size()));
    TCHK(dev_malloc(&dS1, sizeof(double) * R));
    TCHK(dev_malloc(&dG, sizeof(double) * R * cap));
    TCHK(dev_malloc(&dPg, sizeof(double) * R * cap));
    TCHK(dev_malloc(&dOut, sizeof(double) * R * cap));
    TCHK(dev_malloc(&dSd, sizeof(double) * R));
    TCHK(dev_malloc(&dHoff, sizeof(long long) * (R + 1)));
    TCHK(dev_malloc(&dMt, sizeof(int) * R));
    TCHK(dev_malloc(&dM, sizeof(int) * R));
    TCHK(hipMemcpy(dH, H.data(), sizeof(double) * H.size(), hipMemcpyHostToDevice));
    TCHK(hipMemcpy(dS1, s1.data(), sizeof(double) * R, hipMemcpyHostToDevice));
    TCHK(hipMemcpy(dG, g ? g : gz.data(), sizeof(double) * R * cap, hipMemcpyHostToDevice));
    TCHK(hipMemcpy(dPg, pg, sizeof(double) * R * cap, hipMemcpyHostToDevice));
    TCHK(hipMemcpy(dHoff, hoff.data(), sizeof(long long) * (R + 1), hipMemcpyHostToDevice));
    TCHK(hipMemcpy(dMt, mt.data(), sizeof(int) * R, hipMemcpyHostToDevice));
    TCHK(hipMemcpy(dM, m, sizeof(int) * R, hipMemcpyHostToDevice));
    TCHK(hipMemset(dOut, 0, sizeof(double) * R * cap));
    if (fix) { // some entries fixed from the start
        TCHK(dev_malloc(&dFix, (size_t)R * cap));
        TCHK(dev_malloc(&dDfix, sizeof(double) * R * cap));
        TCHK(hipMemcpy(dFix, fix, (size_t)R * cap, hipMemcpyHostToDevice));
        TCHK(hipMemcpy(dDfix, dfix, sizeof(double) * R * cap, hipMemcpyHostToDevice));
    }
    launch_newton_solve(dH, dHoff, dMt, dM, dS1, s2, dG, dPg, R, cap, dOut, dSd, nullptr, maxm, nullptr, dFix, dDfix);
    TCHK(hipGetLastError());
    TCHK(hipDeviceSynchronize());
    TCHK(hipMemcpy(d_out, dOut, sizeof(double) * R * cap, hipMemcpyDeviceToHost));
#undef TCHK
    freeall();
    return GML_OK;
}

extern "C" int gml_test_newton_solve(int R, const int *m, int cap, const double *blocks /* R x cap x cap, block r uses its leading m_r x m_r */,
                                     const double *pg /* R x cap */, double s2, const double *g /* R x cap or NULL */, double *d_out /* R x cap */,
                                     int device) {
    return test_newton_solve(R, m, cap, blocks, pg, s2, g, d_out, device, nullptr, nullptr);
}
// ... and the re-solve with some entries fixed (fix != 0: d = dfix there; the others solve A_ff d_f = -pg_f - A_fx dfix_x)
extern "C" int gml_test_newton_solve_fixed(int R, const int *m, int cap, const double *blocks, const double *pg, double s2, const double *g,
                                           const unsigned char *fix, const double *dfix, double *d_out, int device) {
    return test_newton_solve(R, m, cap, blocks, pg, s2, g, d_out, device, fix, dfix);
}

// Experiment hook (not part of include/gml.h): bytes [off, off + bytes) of the V limb planes of the handle's int8 workspace.  The
// timing builds of the forward kernels (scripts/build_variant.sh ... -DABL_TIMING) leave per-workgroup timestamps there.
extern "C" int gml_debug_read_vq(gml_problem *p, int64_t off, int64_t bytes, void *out) {
    if (!p || !out) return fail(GML_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(p->device));
    const int8_t *vq = nullptr;
    int64_t total = 0;
    gml::i8_vq_buffer(p->i8ws, &vq, &total, p->d);
    if (!vq || off < 0 || off + bytes > total) return fail(GML_EINVAL, "range outside the %lld bytes of V planes", (long long)total);
    HIPCHK(hipStreamSynchronize(p->st));
    HIPCHK(hipMemcpy(out, vq + off, (size_t)bytes, hipMemcpyDeviceToHost));
    return GML_OK;
}


// Test hook (not part of include/gml.h): what the last objective/gradient pass of an int8-limb precision left on the device -- the
// Vq image (slots x planes x Kp bytes, in the layout of gml_i8.h) and the per-slot sums csum, csum2, asum, asum2 (sums[5][slots]:
// the fifth row is mmax, widened).  Null outputs: only the sizes.  tests/test_gpu_i8w_single_sweep.py.
extern "C" int gml_test_i8_pass_state(gml_problem *p, int64_t *slots, int *planes, int64_t *kp, int8_t *vq, long long *sums) {
    if (!p || !slots || !planes || !kp) return fail(GML_EINVAL, "bad argument");
    const gml::I8Ws *w = static_cast<const gml::I8Ws *>(p->i8ws);
    *slots = w ? w->slots : 0;
    *planes = w ? w->LBT : 0;
    *kp = p->d.Kp;
    if (!w || !vq || !sums) return GML_OK;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->st));
    const size_t ns = (size_t)w->slots;
    HIPCHK(hipMemcpy(vq, w->Vq, ns * w->LBT * p->d.Kp, hipMemcpyDeviceToHost));
    const gml::SlotScalars &sc = w->sc[0];
    const long long *src[4] = {sc.csum, sc.csum2, sc.asum, sc.asum2};
    for (int j = 0; j < 4; ++j) HIPCHK(hipMemcpy(sums + j * ns, src[j], sizeof(long long) * ns, hipMemcpyDeviceToHost));
    std::vector<unsigned> mm(ns);
    HIPCHK(hipMemcpy(mm.data(), sc.mmax, sizeof(unsigned) * ns, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ns; ++i) sums[4 * ns + i] = mm[i];
    return GML_OK;
}

// Test hook (not part of include/gml.h): the operands the last objective pass of an int8-limb precision was given -- what the pack layer
// (gml_i8_pack.hip) and i8_pass left on the device.  Read only: synchronises the handle's stream and copies; launches nothing.
//   dims [20]: 0 slots, 1 planes the Tq buffer is sized for, 2 LF of the last objective pass (0: none yet), 3 it paired columns (i8_pass
//              handed tdense on), 4 it compacted (handed a column table on), 5 csteps (0: never tried, -1: no memory), 6 Qp, 7 Qfp, 8 Qf,
//              9 cconst, 10 Kp, 11 K, 12 bytes of the Tq image of that LF, 13 bytes of Xb, 14 bytes of Xtb, 15 bytes of one tile's Xc,
//              16 rows of the Theta workspace, 17 the workspace has marks (7 planes), 18 LF of a Hessian-vector pass that has rewritten
//              Tq since (0: Tq is the objective pass's), 19 0
//   out [13] or NULL (only the sizes); a NULL entry is skipped:
//              0 Tq int8 [dims 12] = [tile][Qfp / 64][LF][32][64];  1 tdense int [slots / 32] (zeros without marks);  2 cnk int [slots / 32];
//              3 cmap int [slots / 32][csteps * 64] (2, 3: untouched while csteps <= 0);  4 sigma, 5 tau double [slots];  6 qconst, 7 qconst2,
//              8 qpair int64 [slots] of sc[0];  9 Theta double [dims 16][Qp], the internal-layout rows the pass read;  10 Xb;  11 Xtb;
//              12 Xc of tile `xc_tile`
extern "C" int gml_test_i8_pack_state(gml_problem *p, int64_t xc_tile, int64_t *dims, void **out) {
    if (!p || !dims) return fail(GML_EINVAL, "bad argument");
    const gml::I8Ws *w = static_cast<const gml::I8Ws *>(p->i8ws);
    const DevProblem &d = p->d;
    const int64_t ns = w ? w->slots : 0, nt = ns / 32;
    const int64_t v[20] = {ns, w ? w->LF : 0, w ? w->last_lf : 0, w && w->last_paired, w && w->last_compact, w ? w->csteps : 0, d.Qp, d.Qfp, d.Qf, d.cconst,
                           d.Kp, d.K, w ? ns * w->last_lf * d.Qfp : 0, d.Kp * (d.Qfp / 8), xtb_bytes(d), w ? w->xc_tile : 0, p->ws_rows,
                           w && w->tdense, w ? w->tq_hv_lf : 0, 0};
    std::copy(v, v + 20, dims);
    if (!out) return GML_OK;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->st));
    auto get = [&](int i, const void *src, size_t bytes) -> hipError_t {
        return out[i] && src && bytes ? hipMemcpy(out[i], src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
    };
    HIPCHK(get(10, d.Xb, (size_t)v[13]));
    HIPCHK(get(11, d.Xtb, (size_t)v[14]));
    if (p->dTheta) HIPCHK(get(9, p->dTheta, sizeof(double) * (size_t)p->ws_rows * d.Qp));
    if (!w) return GML_OK;
    HIPCHK(get(0, w->Tq, (size_t)v[12]));
    if (out[1]) {
        if (w->tdense) HIPCHK(get(1, w->tdense, sizeof(int) * nt));
        else std::memset(out[1], 0, sizeof(int) * nt);
    }
    if (w->csteps > 0) {
        HIPCHK(get(2, w->cnk, sizeof(int) * nt));
        HIPCHK(get(3, w->cmap, sizeof(int) * nt * w->csteps * 64));
        if (out[12]) {
            if (xc_tile < 0 || xc_tile >= nt) return fail(GML_EINVAL, "tile %lld outside the %lld tiles of the workspace", (long long)xc_tile, (long long)nt);
            HIPCHK(get(12, w->Xc + xc_tile * w->xc_tile, (size_t)w->xc_tile));
        }
    }
    const gml::SlotScalars &sc = w->sc[0];
    HIPCHK(get(4, sc.sigma, sizeof(double) * ns));
    HIPCHK(get(5, sc.tau, sizeof(double) * ns));
    HIPCHK(get(6, sc.qconst, sizeof(long long) * ns));
    HIPCHK(get(7, sc.qconst2, sizeof(long long) * ns));
    HIPCHK(get(8, sc.qpair, sizeof(long long) * ns));
    return GML_OK;
}

// Test hook (not part of include/gml.h): what the last working-set Hessian call (i8_hessian, gml_i8_hess.hip) left in the handle's int8
// workspace.  Read only: synchronises the handle's stream and copies; launches nothing.
//   dims [8]: 0 pitch of the weight planes (= Kp; 0: no Hessian call yet), 1 rows the planes are sized for (a multiple of 32), 2 elements
//             H64 is sized for, 3 Qp, 4 Kp, 5 bytes of Mb (0: not built), 6 Qfp, 7 digit planes of a weight (HL)
//   out [3] or NULL (only the sizes); a NULL entry is skipped:
//             0 Hq int8 [dims 1 / 32][HL][32][dims 0], the digits of the weights over the compact index, vq_pos order within each 64;
//             1 H64 int64 [dims 2]: the integer blocks T_ij of the last call at its offsets, then (from its htotal on) the rows' sums hS --
//               beyond them whatever larger earlier calls left;  2 Mb uint32 [Qp][Kp / 64][2]
extern "C" int gml_test_i8_hess_state(gml_problem *p, int64_t *dims, void **out) {
    if (!p || !dims) return fail(GML_EINVAL, "bad argument");
    const gml::I8Ws *w = static_cast<const gml::I8Ws *>(p->i8ws);
    const DevProblem &d = p->d;
    const int64_t v[8] = {w ? w->hKh : 0, w ? w->hrows : 0, w ? w->hcap_elems : 0, d.Qp, d.Kp, w && w->Mb ? d.Qp * (d.Kp / 8) : 0, d.Qfp, gml::HL};
    std::copy(v, v + 8, dims);
    if (!out || !w) return GML_OK;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->st));
    auto get = [&](int i, const void *src, size_t bytes) -> hipError_t {
        return out[i] && src && bytes ? hipMemcpy(out[i], src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
    };
    HIPCHK(get(0, w->Hq, (size_t)v[1] * gml::HL * v[0]));
    HIPCHK(get(1, w->H64, sizeof(long long) * (size_t)v[2]));
    HIPCHK(get(2, w->Mb, (size_t)v[5]));
    return GML_OK;
}
