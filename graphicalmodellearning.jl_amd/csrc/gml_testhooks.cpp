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
int g_cond_split = 1;                         // the conditional chains' constant part: 0 never, 1 by the host's rule, 2 always
thread_local double g_cond_exact_times[3] = {0, 0, 0}; // the time split of this thread's last gml_conditional_exact[_masked] call
int g_exact_chunk_bits = 0;                   // the exact enumeration's chunk bits: 0 = min(component size, kExactChunkBits)
std::atomic<long long> g_fill_chunks{0};      // chunks the last fill_sign_bits staged (gml_test_fill_chunks)
double g_tune[GML_NTUNE] = {};            // experiment knobs of the solver, 0 = the built-in rule (gml_solver.h)
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
namespace gml {
TrajRecorder g_traj; // the record of a solve's outer iterations (gml_solver.h), off by default
}
// Test hooks (not part of include/gml.h): the record of the outer iterations of the last solve that began while the recorder was armed
// (gml_solver.h: TrajRecorder, TRH_*, TRR_*).  tests/test_gpu_solver_trajectory.py.  Arm between solves only; one solve at a time.
// gml_test_traj_arm: arms (on != 0) or disarms the recorder and drops the record; returns the old state.
extern "C" int gml_test_traj_arm(int on) {
    const int old = g_traj.armed;
    g_traj = TrajRecorder{};
    g_traj.armed = on != 0;
    return old;
}
// dims [8]: 0 iterations recorded, 1 R (local rows), 2 Qp, 3 capP, 4 TRH_N, 5 TRR_N, 6 finish was reached (from_best is there), 7 0
extern "C" int gml_test_traj_dims(int64_t *dims) {
    if (!dims) return fail(GML_EINVAL, "NULL argument");
    const int64_t v[8] = {(int64_t)g_traj.its.size(), g_traj.R, g_traj.Qp, g_traj.capP, TRH_N, TRR_N, g_traj.from_best.empty() ? 0 : 1, 0};
    std::memcpy(dims, v, sizeof v);
    return GML_OK;
}
// record i: hdr [TRH_N], rows [R][TRR_N], F [R][capP], X [R][Qp] (a NULL output is skipped).  Returns in *has_x whether the iteration had a
// line search (X is written only then).
extern "C" int gml_test_traj_iter(int i, double *hdr, double *rows, int *F, double *X, int *has_x) {
    if (i < 0 || (size_t)i >= g_traj.its.size()) return fail(GML_EINVAL, "no iteration %d in the record of %zu", i, g_traj.its.size());
    const TrajIter &t = g_traj.its[(size_t)i];
    if (hdr) std::memcpy(hdr, t.hdr, sizeof t.hdr);
    if (rows) std::memcpy(rows, t.rows.data(), sizeof(double) * t.rows.size());
    if (F) std::memcpy(F, t.F.data(), sizeof(int) * t.F.size());
    if (X && !t.X.empty()) std::memcpy(X, t.X.data(), sizeof(double) * t.X.size());
    if (has_x) *has_x = !t.X.empty();
    return GML_OK;
}
// the matrix-free events of record i (gml_solver.h: TRC_*).  gml_test_traj_cg_count: *n = how many; gml_test_traj_cg_event: dims [3] = tag,
// integers, doubles of event e; gml_test_traj_cg_data: copies them (a NULL output is skipped)
static const TrajCgEvent *traj_cg_event(int i, int e) {
    if (i < 0 || (size_t)i >= g_traj.its.size() || e < 0 || (size_t)e >= g_traj.its[(size_t)i].cg.size()) {
        fail(GML_EINVAL, "no event %d in iteration %d of the record", e, i);
        return nullptr;
    }
    return &g_traj.its[(size_t)i].cg[(size_t)e];
}
extern "C" int gml_test_traj_cg_count(int i, int64_t *n) {
    if (!n || i < 0 || (size_t)i >= g_traj.its.size()) return fail(GML_EINVAL, "no iteration %d in the record of %zu", i, g_traj.its.size());
    *n = (int64_t)g_traj.its[(size_t)i].cg.size();
    return GML_OK;
}
extern "C" int gml_test_traj_cg_event(int i, int e, int64_t *dims) {
    const TrajCgEvent *ev = traj_cg_event(i, e);
    if (!ev || !dims) return GML_EINVAL;
    dims[0] = ev->tag;
    dims[1] = (int64_t)ev->iv.size();
    dims[2] = (int64_t)ev->dv.size();
    return GML_OK;
}
extern "C" int gml_test_traj_cg_data(int i, int e, int64_t *iv, double *dv) {
    const TrajCgEvent *ev = traj_cg_event(i, e);
    if (!ev) return GML_EINVAL;
    if (iv && !ev->iv.empty()) std::memcpy(iv, ev->iv.data(), sizeof(int64_t) * ev->iv.size());
    if (dv && !ev->dv.empty()) std::memcpy(dv, ev->dv.data(), sizeof(double) * ev->dv.size());
    return GML_OK;
}
// from_best [R]: 1 where finish took the row from the best iterate, 0 where from the last
extern "C" int gml_test_traj_finish(unsigned char *from_best) {
    if (!from_best || g_traj.from_best.empty()) return fail(GML_EINVAL, "the recorded solve did not reach its finish");
    std::memcpy(from_best, g_traj.from_best.data(), g_traj.from_best.size());
    return GML_OK;
}
// forces the chain tile of the term-list chain kernel (64, 128 or 256 chains; 0 = its rule); returns the old value, -1 for another T.
// A forced tile whose state does not fit the kernel's LDS budget is not used.  Set between calls only
extern "C" int gml_test_term_chains_tile(int T) {
    if (T != 0 && T != 64 && T != 128 && T != 256) return -1;
    const int old = g_term_chains_tile;
    g_term_chains_tile = T;
    return old;
}
// the constant part of the conditional chains' fields (gml_cond_chains.hip): 1 (default) the incidences of a hidden spin whose other
// spins are all observed are summed once per chain where the host's rule expects that to pay (gml_chains_host.cpp), 2 wherever there is
// such an incidence, 0 never -- every sweep walks them; the same bits in all three.  Returns the old value, -1 for another value
extern "C" int gml_test_cond_split(int on) {
    if (on < 0 || on > 2) return -1;
    const int old = g_cond_split;
    g_cond_split = on;
    return old;
}
// the low "chunk" bits of the exact enumeration (gml_exact.hip): c = 1 .. 12 instead of min(component size, 12), 0 restores that
// default; small values take tiny models through the multi-chunk and multi-group paths.  Returns the old value, -1 for another value
// out [3] = the host, slab and total seconds of the calling thread's last call of gml_conditional_exact / gml_conditional_exact_masked
// (gml_cond_exact.cpp; scripts/cond_exact_times.py reports the host's share from it)
extern "C" int gml_test_cond_exact_times(double *out) {
    if (!out) return -1;
    for (int i = 0; i < 3; ++i) out[i] = g_cond_exact_times[i];
    return 0;
}

extern "C" int gml_test_exact_chunk_bits(int c) {
    if (c < 0 || c > kExactChunkBits) return -1;
    const int old = g_exact_chunk_bits;
    g_exact_chunk_bits = c;
    return old;
}
extern "C" double gml_test_hv_sparse_ratio(double ratio) {
    const double old = g_hv_sparse_ratio;
    g_hv_sparse_ratio = ratio;
    return old;
}

// gml_stderr up to the factorisation: the support lists (reference slots, ascending) and sizes of the local rows `rows`, and the A, B
// and g blocks as the Cholesky of k_sandwich_finish receives them (gml_sandwich.hip; host arrays, pitch cap).  se / status as gml_stderr
// leaves them before the finish (0.0 off the support, NaN on it).
extern "C" int gml_test_sandwich_grams(gml_problem *p, int formulation, const double *x, int64_t ld, const uint8_t *structure, int64_t ld_s,
                                       int64_t nrows, const int64_t *rows, int cap, int32_t *lists, int32_t *msz, double *A, double *B, double *g) {
    if (!p || !rows || !lists || !msz || !A || !B || !g || nrows < 1 || cap < 1) return fail(GML_EINVAL, "NULL argument");
    std::vector<double> se((size_t)(p->node1 - p->node0) * (size_t)std::max<int64_t>(ld, 1));
    const GmlSandwichHook hook{nrows, rows, cap, lists, msz, A, B, g};
    return gml_sandwich_run(p, formulation, x, ld, structure, ld_s, se.data(), nullptr, nullptr, &hook);
}
// 1 if everything queued on the handle's stream has completed, 0 while work is pending there (or the query fails).  Queues nothing and
// waits for nothing.  tests/test_gpu_device_pointers.py: a call that "returns when its outputs are written" leaves the stream idle.
extern "C" int gml_test_stream_idle(gml_problem *p) {
    if (!p || hipSetDevice(p->device) != hipSuccess) return 0;
    if (hipStreamQuery(p->st) == hipSuccess) return 1;
    (void)hipGetLastError(); // (hipErrorNotReady is no failure of the caller's next HIP call)
    return 0;
}
// Test hook (not part of include/gml.h): the number of stages the last fill_sign_bits of the process uploaded its sign bits in (the
// host-packer and packed creation routes; a refused fill counts the chunks before the bad one)
extern "C" long long gml_test_fill_chunks(void) { return g_fill_chunks.load(); }
// Test hook (not part of include/gml.h): the weights of a handle as every creation route leaves them -- w [Kp] from HBM (copied on the
// handle's stream), summary [4] = M, wmax, wuni, counts_int (1.0 / 0.0) and wblk [Kp / 512] from the host side.  A NULL output is
// skipped.  Read only: copies; launches nothing.  tests/test_gpu_ingest_state.py.
extern "C" int gml_test_weight_state(gml_problem *p, double *w, double *summary, double *wblk) {
    if (!p) return fail(GML_EINVAL, "NULL argument");
    if (w) {
        if (!p->d.w) return fail(GML_EINVAL, "the handle holds no weights");
        HIPCHK(hipSetDevice(p->device));
        HIPCHK(hipMemcpyAsync(w, p->d.w, sizeof(double) * (size_t)p->d.Kp, hipMemcpyDeviceToHost, p->st));
        HIPCHK(hipStreamSynchronize(p->st));
    }
    if (summary) {
        const double v[4] = {p->M, p->d.wmax, p->d.wuni, p->counts_int ? 1.0 : 0.0};
        std::memcpy(summary, v, sizeof v);
    }
    if (wblk) {
        if ((int64_t)p->wblk.size() != p->d.Kp / 512) return fail(GML_EINVAL, "wblk holds %zu blocks, not Kp / 512", p->wblk.size());
        std::memcpy(wblk, p->wblk.data(), sizeof(double) * p->wblk.size());
    }
    return GML_OK;
}
// A handle that holds sizes only -- no device, no samples -- for the tests of argument checks that run before any device work
// (tests/test_host_sandwich.py).  Release it with gml_problem_destroy.
extern "C" int gml_test_problem_stub(int64_t n, int64_t P, int order, int64_t node0, int64_t node1, gml_problem **out) {
    if (!out || n < 1 || P < 1 || node0 < 0 || node1 > n || node0 > node1) return fail(GML_EINVAL, "bad stub");
    gml_problem *q = gml_new_problem(0, n, 1.0, order, node0, node1, 0);
    q->P = P;
    *out = q;
    return GML_OK;
}

namespace {
// device arrays of one hook call: freed when the call returns, whichever way
struct DevArrays {
    std::vector<void *> ptrs;
    ~DevArrays() {
        for (void *q : ptrs) (void)dev_free(q);
    }
    // n elements on the device, copied from h (NULL: zeroed)
    template <typename T> hipError_t up(T **d, const T *h, size_t n) {
        const size_t bytes = sizeof(T) * std::max<size_t>(n, 1);
        const hipError_t e = dev_malloc(d, bytes);
        if (e != hipSuccess) return e;
        ptrs.push_back(*d);
        return h && n ? hipMemcpy(*d, h, sizeof(T) * n, hipMemcpyHostToDevice) : hipMemset(*d, 0, bytes);
    }
    template <typename T> static hipError_t down(T *h, const T *d, size_t n) {
        return h && n ? hipMemcpy(h, d, sizeof(T) * n, hipMemcpyDeviceToHost) : hipSuccess;
    }
};
// blocks [R][cap][cap], block r being its leading m_r x m_r (0 <= m_r <= cap), into the ragged layout the solver keeps its Hessian
// blocks in: block r at H + hoff[r] with pitch 32 mt[r], mt[r] = ceil(m_r / 32) tiles; the padding is the identity.  hoff gets R + 1
// entries.  Returns the largest m_r.
int pack_ragged_blocks(int R, const int *m, int cap, const double *blocks, std::vector<int> &mt, std::vector<long long> &hoff,
                       std::vector<double> &H) {
    mt.assign((size_t)R, 0);
    hoff.assign((size_t)R + 1, 0);
    int maxm = 0;
    for (int r = 0; r < R; ++r) {
        mt[r] = (m[r] + 31) / 32;
        hoff[r + 1] = hoff[r] + (long long)mt[r] * 32 * mt[r] * 32;
        maxm = std::max(maxm, m[r]);
    }
    H.assign((size_t)std::max<long long>(hoff[R], 1), 0.0);
    for (int r = 0; r < R; ++r) {
        const int hp = 32 * mt[r];
        for (int i = 0; i < m[r]; ++i)
            for (int j = 0; j < m[r]; ++j) H[(size_t)hoff[r] + (size_t)i * hp + j] = blocks[((size_t)r * cap + i) * cap + j];
        for (int i = m[r]; i < hp; ++i) H[(size_t)hoff[r] + (size_t)i * hp + i] = 1.0; // padding: identity
    }
    return maxm;
}
} // namespace

extern "C" int gml_test_tile_precond(int T, int ntiles, const int *m, const double *tiles /* ntiles x T x T */, double s1, double s2,
                                     const double *g /* ntiles x T */, const double *r /* ntiles x T */, double *z_out /* ntiles x T */,
                                     int device) {
    if ((T != 64 && T != 128) || ntiles <= 0) return fail(GML_EINVAL, "bad tile size");
    HIPCHK(hipSetDevice(device));
    const size_t nt = (size_t)ntiles, ne = nt * T;
    std::vector<long long> hoff(nt);
    std::vector<int> wrow(nt, 0), fv(ne);
    const int live = 1;
    for (size_t t = 0; t < nt; ++t) hoff[t] = (long long)t * T * T;
    for (size_t e = 0; e < ne; ++e) fv[e] = (int)e; // tile t owns the columns [t T, (t + 1) T) of the one row
    DevArrays A;
    double *dH = nullptr, *dS1 = nullptr, *dG = nullptr, *dR = nullptr, *dZ = nullptr;
    long long *dHoff = nullptr;
    int *dM = nullptr, *dWrow = nullptr, *dFv = nullptr, *dLive = nullptr;
    HIPCHK(A.up(&dH, tiles, ne * T));
    HIPCHK(A.up(&dS1, &s1, 1));
    HIPCHK(A.up(&dG, g, ne));
    HIPCHK(A.up(&dR, r, ne));
    HIPCHK(A.up(&dZ, static_cast<const double *>(nullptr), ne));
    HIPCHK(A.up(&dHoff, hoff.data(), nt));
    HIPCHK(A.up(&dM, m, nt));
    HIPCHK(A.up(&dWrow, wrow.data(), nt));
    HIPCHK(A.up(&dFv, fv.data(), ne));
    HIPCHK(A.up(&dLive, &live, 1));
    launch_tile_inverse(T, dH, dHoff, dM, dWrow, dS1, s2, dG, ntiles, nullptr);
    launch_tile_apply(T, dH, dFv, dM, dWrow, dLive, ntiles, (int64_t)ne, dR, dZ, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(A.down(z_out, dZ, ne));
    return GML_OK;
}

// Test hook (not part of include/gml.h): the batched Newton solve on caller-given blocks -- A_r d_r = -pg_r for R symmetric positive
// definite m_r x m_r blocks (row-major, m_r <= cap <= 512), exactly as gml_learn's direction phase calls it.  tests/test_gpu_newton_solve.py.
static int test_newton_solve(int R, const int *m, int cap, const double *blocks, const double *pg, double s2, const double *g, double *d_out,
                             int device, const unsigned char *fix /* R x cap or NULL */, const double *dfix /* R x cap */) {
    HIPCHK(hipSetDevice(device));
    for (int r = 0; r < R; ++r)
        if (m[r] < 0 || m[r] > cap || cap > 512) return fail(GML_EINVAL, "bad block size");
    std::vector<long long> hoff;
    std::vector<int> mt;
    std::vector<double> H;
    const int maxm = pack_ragged_blocks(R, m, cap, blocks, mt, hoff, H);
    const size_t nc = (size_t)R * cap;
    const std::vector<double> s1((size_t)R, 1.0);
    DevArrays A;
    double *dH = nullptr, *dS1 = nullptr, *dG = nullptr, *dPg = nullptr, *dOut = nullptr, *dSd = nullptr, *dDfix = nullptr;
    long long *dHoff = nullptr;
    int *dMt = nullptr, *dM = nullptr;
    uint8_t *dFix = nullptr;
    HIPCHK(A.up(&dH, H.data(), H.size()));
    HIPCHK(A.up(&dS1, s1.data(), (size_t)R));
    HIPCHK(A.up(&dG, g, nc)); // (NULL: zeros)
    HIPCHK(A.up(&dPg, pg, nc));
    HIPCHK(A.up(&dOut, static_cast<const double *>(nullptr), nc));
    HIPCHK(A.up(&dSd, static_cast<const double *>(nullptr), (size_t)R));
    HIPCHK(A.up(&dHoff, hoff.data(), (size_t)R + 1));
    HIPCHK(A.up(&dMt, mt.data(), (size_t)R));
    HIPCHK(A.up(&dM, m, (size_t)R));
    if (fix) { // some entries fixed from the start
        HIPCHK(A.up(&dFix, fix, nc));
        HIPCHK(A.up(&dDfix, dfix, nc));
    }
    launch_newton_solve(dH, dHoff, dMt, dM, dS1, s2, dG, dPg, R, cap, dOut, dSd, nullptr, maxm, nullptr, dFix, dDfix);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(A.down(d_out, dOut, nc));
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

// Test hook (not part of include/gml.h): what the backward GEMM and the finalisation of the last int8-limb pass left on the device -- the
// i32 accumulator planes Gacc, and the operator workspace's rows of G and f in the internal column layout, before any gather into the
// caller's order.  Read only: synchronises the handle's stream and copies; launches nothing.
//   dims [8]: 0 gplanes (sets of accumulators, one per 2^24 configurations), 1 plane_stride (elements between two sets = slots * LBT * Qfp),
//             2 Qfp, 3 slots, 4 LBT (accumulator planes per slot: 4 i8x, 6 i8w), 5 rows of the operator workspace, 6 Qp, 7 0
//   gacc int32 [dims 0][dims 3 / 32][dims 4][32][dims 2] or NULL;  G double [dims 5][dims 6] or NULL;  F double [dims 5] or NULL
extern "C" int gml_test_i8_gacc(gml_problem *p, int64_t *dims, int32_t *gacc, double *G, double *F) {
    if (!p || !dims) return fail(GML_EINVAL, "bad argument");
    const gml::I8Ws *w = static_cast<const gml::I8Ws *>(p->i8ws);
    const DevProblem &d = p->d;
    const int64_t stride = w ? w->slots * w->LBT * d.Qfp : 0;
    const int64_t v[8] = {w ? w->gplanes : 0, stride, d.Qfp, w ? w->slots : 0, w ? w->LBT : 0, p->ws_rows, d.Qp, 0};
    std::copy(v, v + 8, dims);
    if (!gacc && !G && !F) return GML_OK;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->st));
    if (gacc && w && w->Gacc && stride) HIPCHK(hipMemcpy(gacc, w->Gacc, sizeof(int32_t) * (size_t)w->gplanes * (size_t)stride, hipMemcpyDeviceToHost));
    if (G && p->dG && p->ws_rows) HIPCHK(hipMemcpy(G, p->dG, sizeof(double) * (size_t)p->ws_rows * d.Qp, hipMemcpyDeviceToHost));
    if (F && p->dF && p->ws_rows) HIPCHK(hipMemcpy(F, p->dF, sizeof(double) * (size_t)p->ws_rows, hipMemcpyDeviceToHost));
    return GML_OK;
}

// Test hook (not part of include/gml.h): what the last Hessian-vector (product) pass of the int8-limb GEMM kernels left on the device --
// the limb planes Uq of the products u_k, the pass's own slot scalars (sc[1]) and the Tq image of the directions it quantised.  Read
// only: synchronises the handle's stream and copies; launches nothing.  The V planes the pass read, its accumulators and G come back
// through gml_test_i8_pass_state and gml_test_i8_gacc.
//   dims [8]: 0 slots, 1 planes of Uq (LB = 4), 2 Kp, 3 K, 4 LF of the product pass that last wrote Tq (0: an objective pass has
//             rewritten it since, or none ran), 5 Qfp, 6 bytes of the Tq image at that LF, 7 Uq exists
//   out [9] or NULL (only the sizes); a NULL entry is skipped:
//             0 Uq int8 [slots][4][Kp] in the layout of gml_i8.h (vq_off with 4 planes);  1 sigma, 2 tau, 3 invtau double [slots];
//             4 qconst, 5 csum, 6 asum int64 [slots];  7 mmax uint32 [slots];  8 Tq int8 [dims 6] = [tile][Qfp / 64][LF][32][64]
extern "C" int gml_test_i8_uq(gml_problem *p, int64_t *dims, void **out) {
    if (!p || !dims) return fail(GML_EINVAL, "bad argument");
    const gml::I8Ws *w = static_cast<const gml::I8Ws *>(p->i8ws);
    const DevProblem &d = p->d;
    const int64_t ns = w ? w->slots : 0;
    const int64_t v[8] = {ns, gml::LB, d.Kp, d.K, w ? w->tq_hv_lf : 0, d.Qfp, w ? ns * w->tq_hv_lf * d.Qfp : 0, w && w->Uq};
    std::copy(v, v + 8, dims);
    if (!out || !w) return GML_OK;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->st));
    auto get = [&](int i, const void *src, size_t bytes) -> hipError_t {
        return out[i] && src && bytes ? hipMemcpy(out[i], src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
    };
    HIPCHK(get(0, w->Uq, (size_t)ns * gml::LB * d.Kp));
    const gml::SlotScalars &sc = w->sc[1];
    HIPCHK(get(1, sc.sigma, sizeof(double) * ns));
    HIPCHK(get(2, sc.tau, sizeof(double) * ns));
    HIPCHK(get(3, sc.invtau, sizeof(double) * ns));
    HIPCHK(get(4, sc.qconst, sizeof(long long) * ns));
    HIPCHK(get(5, sc.csum, sizeof(long long) * ns));
    HIPCHK(get(6, sc.asum, sizeof(long long) * ns));
    HIPCHK(get(7, sc.mmax, sizeof(unsigned) * ns));
    HIPCHK(get(8, w->Tq, (size_t)v[6])); // (the buffer is sized for the workspace's LF >= every product LF)
    return GML_OK;
}

// Test hook (not part of include/gml.h): V of the FP64 pass (k_fwd_f64 writes it, k_bwd_f64 and k_hess_f64 read it) as the last pass
// left it.  Read only: synchronises the handle's stream and copies; launches nothing.
//   dims [3]: 0 rows V is sized for (0: no FP64 pass yet), 1 Kp, 2 K
//   V double [dims 0][dims 1] or NULL (only the sizes)
extern "C" int gml_test_f64_v(gml_problem *p, int64_t *dims, double *V) {
    if (!p || !dims) return fail(GML_EINVAL, "bad argument");
    const int64_t rows = p->dV ? p->dVrows : 0;
    dims[0] = rows;
    dims[1] = p->d.Kp;
    dims[2] = p->d.K;
    if (!V || !rows) return GML_OK;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->st));
    HIPCHK(hipMemcpy(V, p->dV, sizeof(double) * (size_t)rows * (size_t)p->d.Kp, hipMemcpyDeviceToHost));
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

// ------------------------------------------------------------------------------------------
// Test hooks of the solver's device kernels (gml_solver.hip) and of the direction phase around the batched solve: host arrays in, the
// launchers as gml_solver.cpp calls them, the results back out.  Nothing stays on the device between calls: the state the kernels
// carry from one iteration to the next goes in and out as arguments.  tests/test_gpu_solver_kernels.py, tests/test_gpu_newton_solve.py.
// ------------------------------------------------------------------------------------------
namespace {
bool rows_in_range(const int *rows, int nrows, int R) {
    for (int a = 0; a < nrows; ++a)
        if (rows[a] < 0 || rows[a] >= R) return false;
    return true;
}
} // namespace

// k_select on the listed rows (any subset of the R rows, in any order).  PG, Xbest [R][Qp], F, gF, pgF [R][capP], out [R] (SelectOut), best
// [R] are read from the caller and written back: what the kernel leaves alone keeps the caller's values.
extern "C" int gml_test_solver_select(int R, int64_t Qp, int nrows, const int *rows, const double *X, const double *G, const unsigned char *kind,
                                      double lambda, int max_add, int capW, int capP, double viol_frac, double *PG, int *F, double *gF, double *pgF,
                                      void *out, double *best, double *Xbest, int device) {
    if (R <= 0 || Qp <= 0 || nrows < 0 || capP <= 0 || capW > capP || !rows_in_range(rows, nrows, R)) return fail(GML_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(device));
    DevArrays A;
    const size_t nd = (size_t)R * Qp, nc = (size_t)R * capP;
    int *dRows = nullptr, *dF = nullptr;
    double *dX = nullptr, *dG = nullptr, *dPG = nullptr, *dgF = nullptr, *dpgF = nullptr, *dBest = nullptr, *dXbest = nullptr;
    uint8_t *dKind = nullptr;
    SelectOut *dOut = nullptr;
    HIPCHK(A.up(&dRows, rows, (size_t)nrows));
    HIPCHK(A.up(&dX, X, nd));
    HIPCHK(A.up(&dG, G, nd));
    HIPCHK(A.up(&dKind, kind, nd));
    HIPCHK(A.up(&dPG, PG, nd));
    HIPCHK(A.up(&dF, F, nc));
    HIPCHK(A.up(&dgF, gF, nc));
    HIPCHK(A.up(&dpgF, pgF, nc));
    HIPCHK(A.up(&dOut, static_cast<const SelectOut *>(out), (size_t)R));
    HIPCHK(A.up(&dBest, best, (size_t)R));
    HIPCHK(A.up(&dXbest, Xbest, nd));
    launch_select(dRows, nrows, dX, dG, dKind, Qp, lambda, max_add, capW, capP, viol_frac, dPG, dF, dgF, dpgF, dOut, dBest, dXbest, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(A.down(PG, dPG, nd));
    HIPCHK(A.down(F, dF, nc));
    HIPCHK(A.down(gF, dgF, nc));
    HIPCHK(A.down(pgF, dpgF, nc));
    HIPCHK(A.down(static_cast<SelectOut *>(out), dOut, (size_t)R));
    HIPCHK(A.down(best, dBest, (size_t)R));
    HIPCHK(A.down(Xbest, dXbest, nd));
    return GML_OK;
}

// k_trial on the listed rows, then (Gt != NULL) k_back with that gradient at the trial points.  Xt [R][Qp], out [R] (TrialOut) and stepn
// [R] (or NULL: the kernel gets NULL) are read from the caller and written back.
extern "C" int gml_test_solver_trial(int R, int64_t Qp, int nrows, const int *rows, const double *X, const double *D, const double *PG,
                                     const unsigned char *kind, double lambda, const double *alpha, double *Xt, void *out, double *stepn,
                                     const double *Gt, int device) {
    if (R <= 0 || Qp <= 0 || nrows < 0 || !rows_in_range(rows, nrows, R)) return fail(GML_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(device));
    DevArrays A;
    const size_t nd = (size_t)R * Qp;
    int *dRows = nullptr;
    double *dX = nullptr, *dD = nullptr, *dPG = nullptr, *dAl = nullptr, *dXt = nullptr, *dStepn = nullptr, *dGt = nullptr;
    uint8_t *dKind = nullptr;
    TrialOut *dOut = nullptr;
    HIPCHK(A.up(&dRows, rows, (size_t)nrows));
    HIPCHK(A.up(&dX, X, nd));
    HIPCHK(A.up(&dD, D, nd));
    HIPCHK(A.up(&dPG, PG, nd));
    HIPCHK(A.up(&dKind, kind, nd));
    HIPCHK(A.up(&dAl, alpha, (size_t)R));
    HIPCHK(A.up(&dXt, Xt, nd));
    HIPCHK(A.up(&dOut, static_cast<const TrialOut *>(out), (size_t)R));
    if (stepn) HIPCHK(A.up(&dStepn, stepn, (size_t)R));
    if (Gt) HIPCHK(A.up(&dGt, Gt, nd));
    launch_trial(dRows, nrows, dX, dD, dPG, dKind, Qp, lambda, dAl, dXt, dOut, dStepn, nullptr);
    if (Gt) launch_back(dRows, nrows, dX, dXt, dGt, dKind, Qp, lambda, dOut, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(A.down(Xt, dXt, nd));
    HIPCHK(A.down(static_cast<TrialOut *>(out), dOut, (size_t)R));
    if (stepn) HIPCHK(A.down(stepn, dStepn, (size_t)R));
    return GML_OK;
}

// The direction phase of the Cholesky rows as Solver::newton_blocks runs it: (secant != 0) launch_secant on the listed rows with the
// caller's apply_above, launch_newton_solve over all R rows -- per-row s1, the rank-one term s2, (pairs != 0) the rows' secant pairs for
// the blocks it corrects itself, (faces != 0) the orthant faces from F / X / kind with `share` and `rounds`, (fix != NULL) entries fixed
// from the start -- and launch_scatter_dir on the listed rows.  blocks [R][cap][cap]: row r's leading m_r x m_r, packed to pitch 32 mt
// (pack_ragged_blocks); on return the lower triangle the solve read (k_secant's correction included), mirrored.  The secant state
// (Fprev, xprev, gprev [R][cap], mprev, npairs [R], S, Y [2][R][cap]), dsol [R][cap], Sdiag [R] and D [R][Qp] are read from the caller and
// written back.  A row that is not listed takes m = 0.
extern "C" int gml_test_newton_direction(int R, int cap, int64_t Qp, int nrows, const int *rows, const int *m, const int *F, double *blocks,
                                         const double *gF, const double *pgF, const double *s1, double s2, const double *X,
                                         const unsigned char *kind, int secant, int apply_above, int pairs, const double *ynoise, int *Fprev,
                                         int *mprev, double *xprev, double *gprev, double *S, double *Y, int *npairs, int faces, double share,
                                         int rounds, const unsigned char *fix, const double *dfix, double *dsol, double *Sdiag, double *D,
                                         int device) {
    if (R <= 0 || cap <= 0 || cap > 512 || Qp <= 0 || nrows < 0 || !rows_in_range(rows, nrows, R)) return fail(GML_EINVAL, "bad argument");
    std::vector<int> listed((size_t)R, 0);
    for (int a = 0; a < nrows; ++a) listed[rows[a]] = 1;
    for (int r = 0; r < R; ++r) {
        if (m[r] < 0 || m[r] > cap || (m[r] > 0 && !listed[r])) return fail(GML_EINVAL, "bad block size");
        for (int a = 0; a < m[r]; ++a)
            if (F[(size_t)r * cap + a] < 0 || F[(size_t)r * cap + a] >= Qp) return fail(GML_EINVAL, "working-set column out of range");
    }
    std::vector<long long> hoff;
    std::vector<int> mt;
    std::vector<double> H;
    const int maxm = std::max(1, pack_ragged_blocks(R, m, cap, blocks, mt, hoff, H));
    HIPCHK(hipSetDevice(device));
    DevArrays A;
    const size_t nd = (size_t)R * Qp, nc = (size_t)R * cap;
    int *dRows = nullptr, *dM = nullptr, *dMt = nullptr, *dF = nullptr, *dFprev = nullptr, *dMprev = nullptr, *dNp = nullptr;
    long long *dHoff = nullptr;
    double *dH = nullptr, *dgF = nullptr, *dpgF = nullptr, *dS1 = nullptr, *dX = nullptr, *dYn = nullptr, *dXprev = nullptr, *dGprev = nullptr,
           *dS = nullptr, *dY = nullptr, *dDfix = nullptr, *dSol = nullptr, *dSd = nullptr, *dD = nullptr;
    uint8_t *dKind = nullptr, *dFix = nullptr;
    HIPCHK(A.up(&dRows, rows, (size_t)nrows));
    HIPCHK(A.up(&dM, m, (size_t)R));
    HIPCHK(A.up(&dMt, mt.data(), (size_t)R));
    HIPCHK(A.up(&dHoff, hoff.data(), (size_t)R + 1));
    HIPCHK(A.up(&dF, F, nc));
    HIPCHK(A.up(&dH, H.data(), H.size()));
    HIPCHK(A.up(&dgF, gF, nc));
    HIPCHK(A.up(&dpgF, pgF, nc));
    HIPCHK(A.up(&dS1, s1, (size_t)R));
    HIPCHK(A.up(&dX, X, nd));
    HIPCHK(A.up(&dKind, kind, nd));
    HIPCHK(A.up(&dYn, ynoise, (size_t)R));
    HIPCHK(A.up(&dFprev, Fprev, nc));
    HIPCHK(A.up(&dMprev, mprev, (size_t)R));
    HIPCHK(A.up(&dXprev, xprev, nc));
    HIPCHK(A.up(&dGprev, gprev, nc));
    HIPCHK(A.up(&dS, S, 2 * nc));
    HIPCHK(A.up(&dY, Y, 2 * nc));
    HIPCHK(A.up(&dNp, npairs, (size_t)R));
    HIPCHK(A.up(&dSol, dsol, nc));
    HIPCHK(A.up(&dSd, Sdiag, (size_t)R));
    HIPCHK(A.up(&dD, D, nd));
    if (fix) {
        HIPCHK(A.up(&dFix, fix, nc));
        HIPCHK(A.up(&dDfix, dfix, nc));
    }
    if (secant)
        launch_secant(dRows, nrows, dF, dM, cap, dX, Qp, dgF, dH, dHoff, dMt, dS1, s2, dYn, dFprev, dMprev, dXprev, dGprev, dS, dY, dNp, (int64_t)nc,
                      apply_above, nullptr);
    NewtonFaces nf;
    nf.F = dF;
    nf.X = dX;
    nf.kind = dKind;
    nf.Qp = Qp;
    nf.share = share;
    nf.rounds = rounds;
    const SecantPairs sp{dS, dY, dNp, (int64_t)nc};
    launch_newton_solve(dH, dHoff, dMt, dM, dS1, s2, dgF, dpgF, R, cap, dSol, dSd, nullptr, maxm, faces ? &nf : nullptr, dFix, dDfix,
                        pairs ? &sp : nullptr);
    launch_scatter_dir(dRows, nrows, dF, dSol, dM, cap, Qp, dD, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(A.down(H.data(), dH, H.size()));
    for (int r = 0; r < R; ++r) {
        const int hp = 32 * mt[r];
        for (int i = 0; i < m[r]; ++i)
            for (int j = 0; j <= i; ++j)
                blocks[((size_t)r * cap + i) * cap + j] = blocks[((size_t)r * cap + j) * cap + i] = H[(size_t)hoff[r] + (size_t)i * hp + j];
    }
    HIPCHK(A.down(Fprev, dFprev, nc));
    HIPCHK(A.down(mprev, dMprev, (size_t)R));
    HIPCHK(A.down(xprev, dXprev, nc));
    HIPCHK(A.down(gprev, dGprev, nc));
    HIPCHK(A.down(S, dS, 2 * nc));
    HIPCHK(A.down(Y, dY, 2 * nc));
    HIPCHK(A.down(npairs, dNp, (size_t)R));
    HIPCHK(A.down(dsol, dSol, nc));
    HIPCHK(A.down(Sdiag, dSd, (size_t)R));
    HIPCHK(A.down(D, dD, nd));
    return GML_OK;
}

// The matrix-free Newton-CG of the listed rows in the order of Solver::newton_cg_group, with the device operator's raw product
// (sum_k h_k x_k x_k^T) v replaced by Hd[r] v, formed here on the host between the launches (Hd [R][Qp][Qp], symmetric):
// k_cg_tiles, the tiles' blocks gathered from Hd at FV, the tile inverses, k_pcg_init / tile_apply / k_pcg_dir(first), nsteps x {product,
// k_pcg_step, tile_apply, k_pcg_dir}; then, with faces != 0, k_pcg_faces, the product of D, k_pcg_resid, tile_apply, k_pcg_dir(first) and
// nsteps2 more steps.  The per-step kernels run on the listed rows with live[r] != 0; k_cg_tiles, k_pcg_init and k_pcg_faces on all
// listed rows.  FV, gV [ntiles T] (ntiles = sum over the listed rows, in list order, of ceil(|W| / T); the caller sizes them for
// R ceil(Qp / T) tiles), D, Rv, Zv, Pv [R][Qp], Wm [R][Qp], cg [R] (CgState), fout [R] (FaceOut) are read from the caller and written back.
extern "C" int gml_test_pcg(int R, int64_t Qp, int T, int nrows, const int *rows, const double *Hd, const double *s1, double s2, const double *X,
                            const double *PG, const double *G, const unsigned char *kind, const int *live, int nsteps, int faces, int nsteps2,
                            int *FV, double *gV, double *D, double *Rv, double *Zv, double *Pv, unsigned char *Wm, void *cg, void *fout,
                            int device) {
    if ((T != 64 && T != 128) || R <= 0 || Qp <= 0 || nrows <= 0 || !rows_in_range(rows, nrows, R)) return fail(GML_EINVAL, "bad argument");
    const size_t nd = (size_t)R * Qp, tcap = (size_t)R * ((Qp + T - 1) / T);
    std::vector<int> nW((size_t)R, 0), vm, wrow, liverows;
    std::vector<long long> t0((size_t)R, 0), hoff;
    for (int a = 0; a < nrows; ++a) {
        const int r = rows[a];
        int w = 0;
        for (int64_t c = 0; c < Qp; ++c) w += kind[r * Qp + c] && (X[r * Qp + c] != 0.0 || PG[r * Qp + c] != 0.0);
        nW[r] = w;
        t0[r] = (long long)vm.size();
        for (int b = 0; b < w; b += T) {
            vm.push_back(std::min(T, w - b));
            wrow.push_back(r);
            hoff.push_back((long long)hoff.size() * T * T);
        }
        if (live[r]) liverows.push_back(r);
    }
    const size_t ntiles = vm.size();
    if (ntiles == 0 || ntiles > tcap) return fail(GML_EINVAL, "no working set");
    HIPCHK(hipSetDevice(device));
    DevArrays A;
    int *dRows = nullptr, *dLiveRows = nullptr, *dLive = nullptr, *dFV = nullptr, *dVm = nullptr, *dWrow = nullptr, *dNw = nullptr;
    long long *dT0 = nullptr, *dHoff = nullptr;
    double *dS1 = nullptr, *dX = nullptr, *dPG = nullptr, *dG = nullptr, *dgV = nullptr, *dHt = nullptr, *dD = nullptr, *dRv = nullptr, *dZv = nullptr,
           *dPv = nullptr, *dHp = nullptr;
    uint8_t *dKind = nullptr, *dWm = nullptr;
    CgState *dCg = nullptr;
    FaceOut *dFo = nullptr;
    HIPCHK(A.up(&dRows, rows, (size_t)nrows));
    HIPCHK(A.up(&dLiveRows, liverows.data(), liverows.size()));
    HIPCHK(A.up(&dLive, live, (size_t)R));
    HIPCHK(A.up(&dFV, FV, tcap * T));
    HIPCHK(A.up(&dgV, gV, tcap * T));
    HIPCHK(A.up(&dVm, vm.data(), ntiles));
    HIPCHK(A.up(&dWrow, wrow.data(), ntiles));
    HIPCHK(A.up(&dNw, nW.data(), (size_t)R));
    HIPCHK(A.up(&dT0, t0.data(), (size_t)R));
    HIPCHK(A.up(&dHoff, hoff.data(), ntiles));
    HIPCHK(A.up(&dS1, s1, (size_t)R));
    HIPCHK(A.up(&dX, X, nd));
    HIPCHK(A.up(&dPG, PG, nd));
    HIPCHK(A.up(&dG, G, nd));
    HIPCHK(A.up(&dKind, kind, nd));
    HIPCHK(A.up(&dD, D, nd));
    HIPCHK(A.up(&dRv, Rv, nd));
    HIPCHK(A.up(&dZv, Zv, nd));
    HIPCHK(A.up(&dPv, Pv, nd));
    HIPCHK(A.up(&dWm, Wm, nd));
    HIPCHK(A.up(&dHp, static_cast<const double *>(nullptr), nd));
    HIPCHK(A.up(&dCg, static_cast<const CgState *>(cg), (size_t)R));
    HIPCHK(A.up(&dFo, static_cast<const FaceOut *>(fout), (size_t)R));
    launch_cg_tiles(dRows, nrows, dX, dPG, dG, dKind, Qp, T, dT0, dFV, dgV, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    std::vector<int> fv(ntiles * T);
    HIPCHK(A.down(fv.data(), dFV, fv.size()));
    std::vector<double> Ht(ntiles * T * T, 0.0);
    for (size_t t = 0; t < ntiles; ++t) {
        const double *Hr = Hd + (size_t)wrow[t] * Qp * Qp;
        for (int i = 0; i < vm[t]; ++i)
            for (int j = 0; j < vm[t]; ++j) {
                const int ci = fv[t * T + i], cj = fv[t * T + j];
                if (ci < 0 || ci >= Qp || cj < 0 || cj >= Qp) return fail(GML_EHIP, "k_cg_tiles listed a column out of range");
                Ht[(t * T + i) * T + j] = Hr[(size_t)ci * Qp + cj];
            }
    }
    HIPCHK(A.up(&dHt, Ht.data(), Ht.size()));
    const WList wl{dFV, dT0, dNw, T};
    const int nl = (int)liverows.size();
    std::vector<double> hv(nd), hp(nd, 0.0);
    // Hp[r] = Hd[r] v[r] for the given rows (long double accumulation: the operator's integer sums carry no rounding either)
    auto product = [&](const std::vector<int> &rs, const double *dV) -> int {
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(A.down(hv.data(), dV, nd));
        for (int r : rs) {
            const double *Hr = Hd + (size_t)r * Qp * Qp, *v = hv.data() + (size_t)r * Qp;
            for (int64_t i = 0; i < Qp; ++i) {
                long double s = 0.0L;
                for (int64_t j = 0; j < Qp; ++j)
                    if (v[j] != 0.0) s += (long double)Hr[i * Qp + j] * v[j];
                hp[(size_t)r * Qp + i] = (double)s;
            }
        }
        HIPCHK(hipMemcpy(dHp, hp.data(), sizeof(double) * nd, hipMemcpyHostToDevice));
        return GML_OK;
    };
    auto steps = [&](int n) -> int {
        for (int k = 0; k < n && nl > 0; ++k) {
            const int rc = product(liverows, dPv);
            if (rc) return rc;
            launch_pcg_step(dLiveRows, nl, dG, dWm, Qp, dS1, s2, dHp, dD, dRv, dPv, dCg, wl, nullptr);
            launch_tile_apply(T, dHt, dFV, dVm, dWrow, dLive, (int64_t)ntiles, Qp, dRv, dZv, nullptr);
            launch_pcg_dir(dLiveRows, nl, Qp, dWm, dRv, dZv, dPv, 0, dCg, wl, nullptr);
        }
        return GML_OK;
    };
    launch_tile_inverse(T, dHt, dHoff, dVm, dWrow, dS1, s2, dgV, (int64_t)ntiles, nullptr);
    launch_pcg_init(dRows, nrows, dX, dPG, dKind, Qp, dD, dRv, dZv, dPv, dWm, dCg, nullptr);
    launch_tile_apply(T, dHt, dFV, dVm, dWrow, dLive, (int64_t)ntiles, Qp, dRv, dZv, nullptr);
    launch_pcg_dir(dLiveRows, nl, Qp, dWm, dRv, dZv, dPv, 1, dCg, wl, nullptr);
    int rc = steps(nsteps);
    if (rc) return rc;
    if (faces) {
        launch_pcg_faces(dRows, nrows, dX, dPG, dKind, Qp, dD, dWm, dFo, nullptr);
        rc = product(liverows, dD);
        if (rc) return rc;
        launch_pcg_resid(dLiveRows, nl, dPG, dG, Qp, dS1, s2, dHp, dD, dWm, dRv, dCg, nullptr);
        launch_tile_apply(T, dHt, dFV, dVm, dWrow, dLive, (int64_t)ntiles, Qp, dRv, dZv, nullptr);
        launch_pcg_dir(dLiveRows, nl, Qp, dWm, dRv, dZv, dPv, 1, dCg, wl, nullptr);
        rc = steps(nsteps2);
        if (rc) return rc;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(A.down(FV, dFV, tcap * T));
    HIPCHK(A.down(gV, dgV, tcap * T));
    HIPCHK(A.down(D, dD, nd));
    HIPCHK(A.down(Rv, dRv, nd));
    HIPCHK(A.down(Zv, dZv, nd));
    HIPCHK(A.down(Pv, dPv, nd));
    HIPCHK(A.down(Wm, dWm, nd));
    HIPCHK(A.down(static_cast<CgState *>(cg), dCg, (size_t)R));
    HIPCHK(A.down(static_cast<FaceOut *>(fout), dFo, (size_t)R));
    return GML_OK;
}

// The three kernels of the exact block sampler (gml_sampler.hip) on one caller-given block: masks, wts [nt] (the block's terms as bit
// masks over its sb <= 22 spins), members [sb] (the global ids, each in [0, n)), N samples of n spins, the random stream `block`, on device 0.
// One launch_block_sampler on a stream of its own; back come en, cdf [2^sb] as the kernels left them and S [N][n], zeroed first, so that
// the spins outside `members` read 0.  tests/test_gpu_sampler_exact.py.
extern "C" int gml_test_block_sampler(const unsigned *masks, const double *wts, int nt, int sb, const int *members, int64_t N, int64_t n,
                                      uint64_t seed, int block, double *en_out, double *cdf_out, int8_t *S_out) {
    if (nt < 0 || sb < 1 || sb > 22 || N < 1 || n < sb || !members || !en_out || !cdf_out || !S_out || (nt > 0 && (!masks || !wts)))
        return fail(GML_EINVAL, "bad argument");
    for (int t = 0; t < sb; ++t)
        if (members[t] < 0 || members[t] >= n) return fail(GML_EINVAL, "member %d outside [0,%lld)", members[t], (long long)n);
    for (int t = 0; t < nt; ++t)
        if ((masks[t] >> sb) != 0) return fail(GML_EINVAL, "mask %d names a spin outside the block", t);
    HIPCHK(hipSetDevice(0));
    struct Stream {
        hipStream_t st = nullptr;
        ~Stream() {
            if (st) (void)hipStreamDestroy(st);
        }
    } s;
    HIPCHK(hipStreamCreate(&s.st));
    DevArrays A; // (freed before the stream goes: declared after it)
    const size_t ns = (size_t)1 << sb;
    unsigned *dMasks = nullptr;
    double *dWts = nullptr, *dEn = nullptr, *dCdf = nullptr;
    int *dMem = nullptr;
    int8_t *dS = nullptr;
    HIPCHK(A.up(&dMasks, masks, (size_t)nt));
    HIPCHK(A.up(&dWts, wts, (size_t)nt));
    HIPCHK(A.up(&dMem, members, (size_t)sb));
    HIPCHK(A.up(&dEn, static_cast<const double *>(nullptr), ns));
    HIPCHK(A.up(&dCdf, static_cast<const double *>(nullptr), ns));
    HIPCHK(A.up(&dS, static_cast<const int8_t *>(nullptr), (size_t)N * (size_t)n));
    HIPCHK(hipDeviceSynchronize()); // the uploads and the zeroing went through the null stream
    launch_block_sampler(dMasks, dWts, nt, sb, dMem, N, n, (unsigned long long)seed, block, dEn, dCdf, dS, s.st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s.st));
    HIPCHK(A.down(en_out, dEn, ns));
    HIPCHK(A.down(cdf_out, dCdf, ns));
    HIPCHK(A.down(S_out, dS, (size_t)N * (size_t)n));
    return GML_OK;
}
