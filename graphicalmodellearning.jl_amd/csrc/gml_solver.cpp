// gml_learn: the batched l1 solver of libgml_hip, device-resident.
//
// Every local node u solves   min_x f_u(x) + lambda * sum_{j penalised} |x_j|   -- the problem the reference builds
// for Ipopt with the z >= |x| epigraph (GraphicalModelLearning.jl:166-177, one model per node in the loop :161) -- and
// all nodes advance in lock-step (Solver::iterate):
//   1. select        pseudo-gradient / KKT residual and working set per node (k_select); converged nodes drop out;
//                    rows the int8-limb arithmetic cannot bring below tol continue on the FP64 path (polish);
//   2. directions    Hessian blocks by one device kernel over a sub-sample of the configurations + batched Cholesky
//                    (newton_blocks: working sets up to max_working entries), or matrix-free conjugate gradients with
//                    Hessian-vector products from the same GEMM kernels (newton_cg: larger working sets, dense optima) --
//                    direction_blocks and newton_cg live in gml_newton_cg.cpp, their rules in gml_cg_rules.h;
//   3. line_search   projected (orthant-wise) backtracking: the first trial is a full pass (it usually succeeds), further
//                    trials are objective-only passes over the rows that need them.
// One device pass (run_pass) gives f and the full gradient of every listed row (int8-limb or FP64 MFMA kernels).
// The iterates X, gradients G, trial points, directions and pseudo-gradients are [rows][Qp] arrays that stay in HBM;
// per iteration only per-row scalars (a few dozen bytes per node) and the small control blocks of the passes cross PCIe.
// A pass evaluates exactly the active rows, packed into consecutive slots of the int8-limb workspace (full MFMA tiles
// whatever subset is still active).
//
// Host <-> device traffic of an iteration is batched: one upload per pass (its control block), one per direction phase, one
// download per pass (SlotResult), and the host waits for the stream only where it must decide something: after select,
// after the trial points, and after each pass (whose acceptance scalars ride along).  On small node shards these round
// trips, not the kernels, are what an iteration costs.
#include "gml_solver_impl.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace gml;

int Solver::init() {
    if (!(o.tol > 0)) o.tol = 1e-9;
    if (o.max_iter <= 0) o.max_iter = 100;
    if (o.max_working < 32) o.max_working = 512;
    if (o.max_working > 512) o.max_working = 512;
    o.max_working = (int)gml_round_up(o.max_working, 32);
    if (o.max_add <= 0) o.max_add = 64;
    capW = capP = o.max_working;
    // Matrix-free rows admit, per iteration, only the violators within this fraction of the largest violation (measured on
    // the order-3 config at the reference's default regulariser: with every violator at once -- 0 -- or a quarter of the
    // largest -- 0.25 -- the projected Newton steps are damped to nothing by the line search; 0.5 takes full steps throughout;
    // 0.7 converges too, in 1.6x the iterations)
    viol_frac = o.cg_viol_frac > 0 ? o.cg_viol_frac : 0.5;
    mf.cg_eta = o.cg_eta > 0 ? o.cg_eta : 0.05;
    // at most 16 CG steps per Newton step: the number of Newton iterations is set by the admission of the violators, not by
    // the accuracy of the directions (order-3 probe: 32 iterations with a cap of 40, 16 or 15 -- 545 / 349 / 333
    // Hessian-vector passes; 40 iterations, 279 passes with a cap of 8)
    mf.maxcg = o.max_cg > 0 ? o.max_cg : 16;
    // limbs of the CG direction p in the Hessian-vector passes: 2 (14 bits of max|p|) are enough for an inexact Newton
    // step that stops at a residual of 5 % -- the iteration counts of the 64-node probe of config 5 are 59 / 59 / 56
    // with 4 / 3 / 2 limbs, and the forward GEMM of an H.v pass costs in proportion
    mf.hv_lf = o.hv_limbs_fwd ? std::min(5, std::max(2, (int)o.hv_limbs_fwd)) : 2;
    // ... and the products u_k = h_k (x_k . p) go to the backward GEMM in 2 limbs (15 bits of the largest) instead of 4:
    // half the MFMAs and half the V reads of that GEMM; config 5 at the default regulariser 116 -> 93 s with 10 % more
    // iterations
    mf.hv_lb = o.hv_limbs_bwd == 4 ? 4 : 2;
    dbg_row = o.debug_row > 0 ? o.debug_row : 0;
    if (o.limbs_fwd != 0 && o.limbs_fwd != 3 && o.limbs_fwd != 4 && o.limbs_fwd != 5) return fail(GML_EINVAL, "limbs_fwd must be 3, 4 or 5");

    if (!p->stage) {
        p->stage_bytes = (size_t)8 << 20;
        // (portable + mapped: one process may drive several devices -- gml_multi -- and the kernels of this handle's device read and
        // write the arena directly)
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&p->stage), p->stage_bytes, hipHostMallocPortable | hipHostMallocMapped));
    }
    {
        void *dp = nullptr; // zero-copy only where the device sees the arena under the same address (unified addressing); else copies
        stg.mapped = hipHostGetDevicePointer(&dp, p->stage, 0) == hipSuccess && dp == static_cast<void *>(p->stage);
        if (!stg.mapped) (void)hipGetLastError();
        for (int i = 0; i < GML_NTUNE; ++i) tune[i] = g_tune[i];
        if (tune[GML_TUNE_NO_ZEROCOPY] > 0) stg.mapped = false; // (tests: the copy path that very large handles take)
    }
    stg.base = p->stage;
    stg.cap = p->stage_bytes;
    stg.st = st;
    stg.off = stg.floor = 0;
    dir_time.st = st;
    stats.lambda = lambda;
    prec = o.precision;
    // (launch-bound problems gain nothing from cheaper passes and pay for the re-evaluation at the switch: config 2 takes 16 + 3
    // passes instead of 13 + 2)
    // (decided on the whole problem -- n, not the local rows -- so that a node shard runs the form its problem would run on one GPU;
    // WHEN the phase ends still depends on the rows of this handle: it ends for all of them with the first that gets close, a per-row
    // switch having been measured slower, DESIGN.md 4.2 -- trajectories differ between shardings, optima do not)
    coarse_on = gml_is_i8(o.precision) && o.coarse >= 0 && formulation != GML_RPLE && (double)p->K * (double)Qp * (double)p->n >= 17179869184.0;
    if (o.coarse > 0) coarse_thr = std::pow(10.0, -(double)o.coarse); // (tuning: the KKT residual at which the coarse phase ends)

    // slots of the int8-limb workspace: every active row of a pass in its own slot, the passes of one iteration in
    // disjoint ranges (their V planes feed the next Hessians).  Objective-only passes (line-search trials whose V planes
    // nobody reads) run in a scratch range above the main one.
    const int64_t Smain = gml_is_i8(o.precision) ? Rp + gml_round_up(std::max<int64_t>(R / 2, 96), 32) + 64 : Rp + 64;
    Scap = Smain + Rp;
    if (!slots.reset(R, Smain, Scap)) return fail(GML_EHIP, "internal: %lld rows do not fit the slot ranges %lld + %lld", (long long)R, (long long)Smain, (long long)(Scap - Smain));
    {
        size_t freeb = 0, totalb = 0;
        HIPCHK(dev_mem_info(&freeb, &totalb));
        const double need_b = 7.0 * 8.0 * (double)nd + (double)nd;
        if (need_b > 0.9 * (double)freeb)
            return fail(GML_ENOMEM, "solver state of %.1f GB for %lld rows does not fit in %.1f GB free HBM", need_b / 1e9, (long long)R,
                        freeb / 1e9);
    }
    HIPCHK(A.get(&X, nd));
    HIPCHK(A.get(&G, nd));
    HIPCHK(A.get(&Xt, nd));
    HIPCHK(A.get(&Gt, nd));
    HIPCHK(A.get(&Xb, nd));
    HIPCHK(A.get(&D, nd));
    HIPCHK(A.get(&PG, nd));
    HIPCHK(A.get(&kind, nd));
    HIPCHK(A.get(&dNode, (size_t)Rp));
    HIPCHK(A.get(&dRows, (size_t)Rp));
    HIPCHK(A.get(&dRows2, (size_t)Rp));
    HIPCHK(A.get(&dRowsP, (size_t)Rp));
    HIPCHK(A.get(&dPass, (size_t)(sizeof(int) * (2 * Scap + Scap / 32 + 16) + sizeof(double) * Scap + 64)));
    HIPCHK(A.get(&dHctl, (size_t)(sizeof(int) * 5 * Rp + sizeof(long long) * (Rp + 1) + sizeof(double) * 3 * Rp + 256)));
    HIPCHK(A.get(&mf.dLive, (size_t)Rp));
    HIPCHK(A.get(&dFprev, (size_t)Rp * capP));
    HIPCHK(A.get(&dMprev, (size_t)Rp));
    HIPCHK(A.get(&dNpairs, (size_t)Rp));
    HIPCHK(A.get(&dXprev, (size_t)Rp * capP));
    HIPCHK(A.get(&dGprev, (size_t)Rp * capP));
    HIPCHK(A.get(&dSec, (size_t)4 * Rp * capP)); // S[0], S[1], Y[0], Y[1]
    HIPCHK(hipMemsetAsync(dMprev, 0, sizeof(int) * Rp, st));
    HIPCHK(hipMemsetAsync(dNpairs, 0, sizeof(int) * Rp, st));
    HIPCHK(A.get(&dRes, (size_t)Scap));
    HIPCHK(A.get(&dFidx, (size_t)Rp * capP));
    HIPCHK(A.get(&dCg, (size_t)Rp));
    HIPCHK(A.get(&dBest, (size_t)Rp));
    HIPCHK(A.get(&dAlpha, (size_t)Rp));
    HIPCHK(A.get(&dFs, (size_t)Scap));
    HIPCHK(A.get(&dgF, (size_t)Rp * capP));
    HIPCHK(A.get(&dpgF, (size_t)Rp * capP));
    HIPCHK(A.get(&dsol, (size_t)Rp * capP));
    HIPCHK(A.get(&dSdiag, (size_t)Rp));
    HIPCHK(A.get(&dSel, (size_t)Rp));
    HIPCHK(A.get(&dTrial, (size_t)Rp));
    HIPCHK(A.get(&dStepn, (size_t)Rp));
    HIPCHK(hipMemsetAsync(dStepn, 0, sizeof(double) * Rp, st));
    sel = stg.persist<SelectOut>((size_t)Rp);
    trial = stg.persist<TrialOut>((size_t)Rp);
    res = stg.persist<SlotResult>((size_t)Scap);
    zc = sel && trial && res;
    if (zc) {
        kSel = sel;
        kTrial = trial;
        kRes = res;
        std::memset(sel, 0, sizeof(SelectOut) * Rp);
        std::memset(trial, 0, sizeof(TrialOut) * Rp);
        std::memset(res, 0, sizeof(SlotResult) * Scap);
    } else {
        stg.off = stg.floor = 0;
        sel_v.resize((size_t)Rp);
        trial_v.resize((size_t)Rp);
        res_v.resize((size_t)Scap);
        sel = sel_v.data();
        trial = trial_v.data();
        res = res_v.data();
        kSel = dSel;
        kTrial = dTrial;
        kRes = dRes;
    }
    HIPCHK(hipMemsetAsync(X, 0, sizeof(double) * nd, st));
    HIPCHK(hipMemsetAsync(Xb, 0, sizeof(double) * nd, st));
    HIPCHK(hipMemsetAsync(G, 0, sizeof(double) * nd, st));
    HIPCHK(hipMemsetAsync(D, 0, sizeof(double) * nd, st));
    {
        std::vector<int> node((size_t)Rp, -1);
        for (int64_t r = 0; r < R; ++r) node[r] = (int)(p->node0 + r);
        std::vector<double> inf((size_t)Rp, INFINITY);
        HIPCHK(stg.h2d(dNode, node.data(), sizeof(int) * Rp));
        HIPCHK(stg.h2d(dBest, inf.data(), sizeof(double) * Rp));
    }
    launch_kind(d, p->order, dNode, (int)Rp, kind, st);
    if (structure) RCCHK(apply_structure());

    for (auto *v : {&f, &ft, &Fobj, &dd, &fn, &fnt, &l1t, &vref, &dref, &stepn}) v->assign((size_t)R, 0.0);
    for (auto *v : {&Z, &Zt, &alpha}) v->assign((size_t)R, 1.0);
    for (auto *v : {&kkt, &best, &Fbest}) v->assign((size_t)R, INFINITY);
    for (auto *v : {&done, &atfloor, &nreg, &accepted_fwd, &need, &iscg}) v->assign((size_t)R, 0);
    for (auto *v : {&stall, &msz, &nW}) v->assign((size_t)R, 0);

    if (gml_is_i8(o.precision) && o.polish >= 0) {
        size_t freeb = 0, totalb = 0;
        if (dev_mem_info(&freeb, &totalb) == hipSuccess) {
            const double need_b = (d.Xt ? 0.0 : (double)d.Kp * (double)Qp) + (p->dV && p->dVrows >= Rp ? 0.0 : 8.0 * (double)Rp * (double)d.Kp) +
                                  8.0 * (double)nd + (o.precision == GML_PREC_I8W ? 6.0 : 4.0) * (double)Scap * d.Kp /* the i8 workspace still to come */;
            can_polish = need_b < 0.8 * (double)freeb;
        }
    }
    stall_cap = can_polish ? 4 : 10;

    // sub-sampled Newton: the budget (rows x configurations) is kept roughly constant: as nodes converge, the remaining
    // ones get more configurations, up to all of them -- an inexact Hessian only costs iterations, and it costs the most on
    // the few ill-conditioned nodes that are still active at the end.
    // The base: 32 768 configurations per row, more on small node shards -- below ~2^23 row-configurations a Hessian launch costs its
    // latency, not its work, so a shard of 128 rows takes 65 536 per row for the price of 32 768 and saves two of fourteen iterations
    // (profiles/r5_hess_budget_sweep.txt; 1 024 rows: 32 768 -> 109 ms, 49 152 -> 113 ms, 24 576 -> 112 ms).  Like the rule above this
    // makes a row's Newton trajectory -- not its optimum -- depend on how many rows share its GPU.
    // (int8 kernels only: the FP64 path's Hessian kernel is bound by its FP64 work at any size -- n = 200, K = 1e5 on that path took
    // 17 % longer with the larger budget, profiles/r5_robust_sweep.txt)
    Kh_base = 32768;
    if (gml_is_i8(o.precision)) Kh_base = std::min<int64_t>(131072, std::max<int64_t>(32768, ((int64_t)1 << 23) / std::max<int64_t>(R, 1)));
    if (tune[GML_TUNE_KH_BASE] > 0) Kh_base = (int64_t)tune[GML_TUNE_KH_BASE];
    if (o.hess_samples != 0) Kh_base = o.hess_samples < 0 ? d.Kp : (int64_t)o.hess_samples;
    nblk512 = d.Kp / 512;
    set_kh(R);
    if (g_traj.armed) { // (the record of an earlier solve goes)
        rec = &g_traj;
        rec->R = R;
        rec->Qp = Qp;
        rec->capP = capP;
        rec->its.clear();
        rec->from_best.clear();
    }
    return GML_OK;
}

// a new record: the header as far as it is known, and what select left per row (with the working sets, downloaded)
int Solver::rec_select(int it, int64_t nactive) {
    rec->its.emplace_back();
    TrajIter &t = rec->its.back();
    for (double &h : t.hdr) h = 0.0;
    t.hdr[TRH_IT] = it;
    t.hdr[TRH_NACTIVE] = (double)nactive;
    t.hdr[TRH_SECANT] = t.hdr[TRH_FACE_ROUNDS] = -1.0;
    t.hdr[TRH_STALL_CAP] = stall_cap;
    t.hdr[TRH_PREC] = prec;
    t.rows.assign((size_t)R * TRR_N, 0.0);
    t.F.assign((size_t)R * capP, -1);
    RCCHK(rec_download(t.F.data(), dFidx, sizeof(int) * (size_t)R * capP));
    for (int64_t r = 0; r < R; ++r) {
        double *q = rec_row(r);
        q[TRR_DONE] = done[r];
        q[TRR_ATFLOOR] = atfloor[r];
        q[TRR_KKT] = kkt[r];
        q[TRR_BEST] = best[r];
        q[TRR_FOBJ] = Fobj[r];
        q[TRR_STALL] = stall[r];
        q[TRR_M] = sel[r].m;
        q[TRR_NSUPP] = sel[r].nsupp;
        q[TRR_NVIOL] = sel[r].nviol;
        q[TRR_F] = f[r];
        q[TRR_FN] = fn[r];
        q[TRR_Z] = Z[r];
        q[TRR_NPAIRS] = -1.0;
    }
    return GML_OK;
}

void Solver::set_kh(int64_t nactive) {
    // (a budget scaled to the working-set size -- 64 configurations per entry, 8192 at least -- was measured and dropped: the
    // headline problem then needs 20-22 iterations instead of 14)
    int64_t want = Kh_base;
    if (o.hess_samples == 0 && nactive > 0) want = Kh_base * std::max<int64_t>(1, R / nactive);
    int64_t nb = std::min(nblk512, std::max<int64_t>(2, (want + 511) / 512));
    if (nb * 512 >= p->K) nb = nblk512; // (nearly) everything: take it all
    kstride = nblk512 / nb;
    Kh = nb * 512;
    double wsum = 0;
    for (int64_t cb = 0; cb < nb; ++cb) wsum += p->wblk[(size_t)(cb * kstride)];
    if (!(wsum > 0)) { // a sub-sample without weight (degenerate histogram): use every configuration
        nb = nblk512;
        kstride = 1;
        Kh = d.Kp;
        wsum = 1.0;
    }
    hscale = nb == nblk512 ? 1.0 : 1.0 / wsum; // rescaled by the weight of the sub-sample
}

int Solver::run_pass(const std::vector<int> &rows, const double *src, double *dst, bool want_grad, bool at_trial, const PassOut &out, int pp,
                     const std::function<int()> *after, bool step_on_device) {
    if (rows.empty()) return GML_OK;
    const double t0 = gml_now_s();
    const PassArgs q{src, dst, want_grad, at_trial, pp < 0 ? prec : pp, after};
    // Round 0 evaluates the listed rows.  Rows whose weights turn out to use less of the fixed-point range than their scale allowed
    // (judge_rows) run again with a tighter one, up to six times: in the slots they hold, with the host's stepn (round 0 brought it
    // down), and with `after` repeated -- what it queued for these rows was computed from the first run's gradient.
    std::vector<int> cur = rows, again;
    std::vector<double> ovr, ovr2;
    int rc = GML_OK;
    for (int round = 0; rc == GML_OK && !cur.empty(); ++round) {
        trace(want_grad ? "pass" : "fwd pass");
        PassRaw raw;
        rc = gml_is_i8(q.pp) ? pass_i8(q, cur, round ? &ovr : nullptr, step_on_device && round == 0, raw) : pass_f64(q, cur, raw);
        if (rc) break;
        if (step_on_device && round == 0) // (the trial's scalars came down with the pass)
            for (int r : cur) stepn[r] = trial[r].stepn;
        judge_rows(q, cur, raw, out, again, ovr2);
        stats.node_evals += (int64_t)cur.size();
        if (want_grad) ++stats.passes;
        else ++stats.forward_passes;
        if (!again.empty() && round >= 6) {
            // the weights exp(-E) of these rows underflow the fixed-point range even after six rescalings (|theta|_1 in the
            // hundreds): a trial point that far out is simply rejected; at the iterate itself it is an error
            if (!at_trial) {
                underflow = true;
                rc = fail(GML_EUNSUPPORTED, "precision %s: the weights exp(-E) of a row underflow its fixed-point range at an iterate; use precision f64 "
                                            "(or auto, which does so by itself)", q.pp == GML_PREC_I8W ? "i8w" : "i8x");
                break;
            }
            for (int r : again) {
                out.f[r] = INFINITY;
                out.noise[r] = 0.0;
            }
            break;
        }
        cur.swap(again);
        ovr.swap(ovr2);
    }
    stats.t_pass += gml_now_s() - t0;
    return rc;
}

// One round on the int8-limb kernels: the rows' slots, the control block (one upload), the pass, and one wait for its results.
// ovr_in: by row, the scales of a re-run (run_pass), which keeps the slots its rows hold.
int Solver::pass_i8(const PassArgs &q, const std::vector<int> &rows, const std::vector<double> *ovr_in, bool step_on_device, PassRaw &raw) {
    const int64_t n = (int64_t)rows.size();
    const bool track = formulation != GML_RPLE, wide = q.pp == GML_PREC_I8W;
    // objective-only trial: scratch slots, the rows keep the V planes of their iterates; else a fresh range of the main slots
    const PlaneSlots::Range g = ovr_in ? slots.held(rows) : !q.want_grad && q.at_trial ? slots.scratch(rows) : slots.claim(rows, q.at_trial);
    const int64_t lo = g.lo, hi = g.hi, ns = hi - lo;
    // control block of the pass, one upload: srow [ns] | rowcol [ns] | tiles, padded with -1 to a multiple of 4 | tau [ns]
    std::vector<uint8_t> tile((size_t)(ns / 32), 0);
    for (int64_t a = 0; a < n; ++a) tile[(g.slot[a] - lo) / 32] = 1;
    int ng = 0;
    for (int64_t t = 0; t < ns / 32; ++t) ng += tile[t];
    const int ng4 = (int)gml_round_up(ng, 4);
    const size_t ints = (size_t)(2 * ns + ng4), ioff = (ints * sizeof(int) + 7) & ~(size_t)7;
    std::vector<char> blk(ioff + sizeof(double) * ns, 0);
    int *srow = reinterpret_cast<int *>(blk.data()), *rowcol = srow + ns, *groups = rowcol + ns;
    double *ovr = reinterpret_cast<double *>(blk.data() + ioff);
    for (int64_t s = 0; s < ns; ++s) rowcol[s] = -1;
    for (int64_t a = 0; a < n; ++a) {
        const int64_t s = g.slot[a] - lo;
        const int r = rows[a];
        srow[s] = r;
        rowcol[s] = (int)(p->node0 + r);
        if (ovr_in) ovr[s] = (*ovr_in)[r];
        else if (track && vref[r] > 0.0) // (step_on_device: times exp(|trial - x|_1), which k_trial left in dStepn)
            ovr[s] = vref[r] * std::exp(dref[r] + (q.at_trial && !step_on_device ? stepn[r] : 0.0)) * (1.0 + 1e-6) / i8_vdiv(wide);
    }
    {
        int k = 0;
        for (int64_t t = 0; t < ns / 32; ++t)
            if (tile[t]) groups[k++] = (int)(lo / 32 + t);
        for (; k < ng4; ++k) groups[k] = -1;
    }
    HIPCHK(stg.h2d(dPass, blk.data(), blk.size()));
    const int *dsrow = reinterpret_cast<const int *>(dPass);
    I8Pass a{};
    a.theta = q.src;
    a.srow = rebase(dsrow, lo); // indexed by slot on the device
    a.rowcol = rebase(dsrow + ns, lo);
    a.groups = dsrow + 2 * ns;
    a.ngroups = ng;
    a.slot0 = (int)lo;
    a.slot1 = (int)hi;
    a.form = formulation;
    a.want_grad = q.want_grad;
    a.F = dFs;
    a.G = q.dst;
    a.tauovr = rebase(reinterpret_cast<const double *>(dPass + ioff), lo);
    a.tauovr_lnrow = !ovr_in && track && step_on_device ? dStepn : nullptr;
    a.res = kRes;
    a.lf = o.limbs_fwd;
    a.wide = wide;
    a.coarse = coarse_on;
    a.zero_theta = at_zero && tune[GML_TUNE_NO_ZERO_SHORTCUT] == 0; // the first pass of a solve: X = 0 for every row
    // Column compaction of the forward GEMM.  It pays where the rows are sparse RELATIVE TO THE COLUMN COUNT: multi-body
    // statistics, thousands of spins (config 5 at c = 1.2: 25 non-zeros of 130 817 per node, learn() 3.5 -> 2.2 s).  With the
    // 1 024 columns of the headline problem a tile's 32 rows cover every column after the third pass and the two extra launches
    // cost a 128-node shard 5 %: problems below 4 096 columns do not try.  A pass whose tiles came out (mostly) dense makes the
    // next 2, 4, ... 16 passes skip the attempt.
    const bool may_compact = tune[GML_TUNE_NO_COMPACT] == 0 && (tune[GML_TUNE_SOLVER_COMPACT] > 0 || d.Qfp >= 4096);
    if (may_compact && compact_skip > 0) --compact_skip;
    else a.compact = may_compact;
    std::string err;
    const int rc = i8_pass(&p->i8ws, d, Scap, a, st, nullptr, &err);
    if (rc) return fail(rc, "%s", err.c_str());
    if (formulation == GML_LOGRISE && q.want_grad) // grad log Z = grad Z / Z (:279), Z from the pass results on the device
        launch_scale_slots_inv(a.srow, a.rowcol, (int)lo, (int)ns, kRes, Qp, q.dst, st);
    RCCHK(fetch(res + lo, dRes + lo, sizeof(SlotResult) * ns));
    if (q.after) RCCHK((*q.after)());
    HIPCHK(hipGetLastError());
    std::vector<int> ctab;
    if (a.compact) { // what the compaction made of this pass comes down with its results
        const int *dcnk = nullptr;
        int cs = 0;
        i8_compact_table(p->i8ws, &dcnk, &cs);
        if (dcnk) {
            ctab.assign((size_t)ns / 32, 0);
            HIPCHK(stg.d2h(ctab.data(), dcnk + lo / 32, sizeof(int) * ctab.size()));
        }
    }
    HIPCHK(stg.sync());
    if (!ctab.empty()) compaction_backoff(ctab);
    raw.resize((size_t)n);
    for (int64_t a2 = 0; a2 < n; ++a2) raw[a2] = res[(size_t)g.slot[a2]];
    return GML_OK;
}

// ctab: per tile of the pass just waited for, the column steps its compacted forward GEMM swept (< 0: all of them)
void Solver::compaction_backoff(const std::vector<int> &ctab) {
    const int nk_all = (int)(d.Qfp / 64);
    long long swept = 0;
    for (int v : ctab) swept += v < 0 ? nk_all : v;
    if ((double)swept > 0.6 * (double)nk_all * (double)ctab.size()) {
        compact_backoff = std::min(16, std::max(2, 2 * compact_backoff));
        compact_skip = compact_backoff;
    } else {
        compact_backoff = 0;
    }
    if (o.verbose >= 2)
        fprintf(stderr, "[gml]   compaction: %lld of %lld column steps swept over %zu tiles%s\n", swept, (long long)nk_all * (long long)ctab.size(),
                ctab.size(), compact_skip ? " (the next passes do not try)" : "");
}

// One round on the FP64 path: slot = row; a tile's backward GEMM writes every row of the tile, so the gradient goes to a
// scratch array first and only the listed rows are copied out
int Solver::pass_f64(const PassArgs &q, const std::vector<int> &rows, PassRaw &raw) {
    const int64_t n = (int64_t)rows.size();
    RCCHK(gml_ensure_f64(p, Rp));
    if (!Gs) HIPCHK(A.get(&Gs, nd));
    std::vector<int> ctl((size_t)(Rp + Rp / 32 + 8), -1);
    std::vector<uint8_t> tile((size_t)(Rp / 32), 0);
    for (int r : rows) {
        ctl[r] = (int)(p->node0 + r);
        tile[r >> 5] = 1;
    }
    int ng = 0;
    for (int64_t t = 0; t < Rp / 32; ++t)
        if (tile[t]) ctl[Rp + ng++] = (int)t;
    const int ng4 = (int)gml_round_up(ng, 4);
    int *dctl = reinterpret_cast<int *>(dPass);
    HIPCHK(stg.h2d(dctl, ctl.data(), sizeof(int) * (Rp + ng4)));
    HIPCHK(hipMemsetAsync(dFs, 0, sizeof(double) * Rp, st));
    launch_fwd_f64(d, q.src, dctl, dctl + Rp, ng4, formulation, p->dV, dFs, p->dRed, st);
    if (q.want_grad) {
        HIPCHK(hipMemsetAsync(Gs, 0, sizeof(double) * nd, st));
        launch_bwd_f64(d, p->dV, dctl + Rp, ng, Gs, p->dRed, st);
        RCCHK(upload_rows(rows, dRowsP));
        launch_copy_rows(dRowsP, (int)n, Qp, Gs, q.dst, nullptr, nullptr, st);
        if (formulation == GML_LOGRISE) launch_scale_rows_inv(dRowsP, (int)n, dFs, Qp, q.dst, st);
    }
    std::vector<double> fh((size_t)Rp);
    HIPCHK(stg.d2h(fh.data(), dFs, sizeof(double) * Rp));
    for (int r : rows) slots.set_row_indexed(r); // (V [row][Kp] of the FP64 path is indexed by row)
    if (q.after) RCCHK((*q.after)());
    HIPCHK(hipGetLastError());
    HIPCHK(stg.sync());
    raw.assign((size_t)n, SlotResult{});
    for (int64_t a = 0; a < n; ++a) raw[a].f = fh[rows[a]];
    return GML_OK;
}

// What the round's results are worth: f and its noise by row into `out`, and on the int8 path the scale the rows' next passes
// start from (vref, dref).  again / ovr2: the rows that must run once more, and (by row) the tighter scale they run with.
void Solver::judge_rows(const PassArgs &q, const std::vector<int> &rows, const PassRaw &raw, const PassOut &out, std::vector<int> &again,
                        std::vector<double> &ovr2) {
    const bool track = gml_is_i8(q.pp) && formulation != GML_RPLE, wide = q.pp == GML_PREC_I8W;
    again.clear();
    ovr2.clear();
    for (size_t a = 0; a < rows.size(); ++a) {
        const int r = rows[a];
        const double fv = raw[a].f;
        // f64: summation rounding.  int8 limbs: every V_rk is rounded to a multiple of tau_r with a dither that is
        // equidistributed over the samples, so the errors (each within one unit, standard deviation 0.41 tau) add like a
        // random walk: 8 sigma of sqrt(K) terms (the worst case K * tau is never approached).
        double noise = 1e-13 * std::max(1.0, std::fabs(fv));
        if (track) {
            noise += 3.3 * std::sqrt((double)p->K) * raw[a].tau * (coarse_on ? i8_coarse_unit(wide) : 1.0); // (coarse: multiples of 2^24 / 2^8 tau)
            // i8x exp forms: the FP32 expm1 of the forward epilogue (vq_exp) is off by up to 1e-9 of every |V_k| before the rounding
            // (three FP32 roundings of about 2^-24 |r| each, |r| <= ln2/128: 3 * 2^-24 * ln2/128 / (1 - ln2/128) = 9.74e-10; 7.7e-10
            // measured) -- one error for all the samples that share an energy, so it adds up with f, not like a random walk
            if (!wide && formulation != GML_RPLE) noise += 1e-9 * std::fabs(fv);
            const double vmax = ((double)raw[a].mmax + 1.0) * i8_mmax_unit(wide) * raw[a].tau; // rigorous bound on max_k |V_rk|
            vref[r] = vmax;
            dref[r] = q.at_trial ? stepn[r] : 0.0; // distance from the current iterate to the point just evaluated
            // Dynamic range: tau_r was derived from a bound; when the largest |V_rk| actually seen is more than 8 bits
            // below it (dense theta), the row is re-run with tau_r taken from that maximum
            if (raw[a].mmax < (1u << 23)) {
                if (ovr2.empty()) ovr2.assign((size_t)R, 0.0);
                again.push_back(r);
                ovr2[r] = vmax * (1.0 + 1e-12) / i8_vdiv(wide);
            }
        }
        if (formulation == GML_LOGRISE) { // f = log Z, g = grad Z / Z   (:279)
            out.Z[r] = fv;
            out.f[r] = std::log(fv);
            out.noise[r] = noise / fv;
        } else {
            out.f[r] = fv;
            out.noise[r] = noise;
        }
    }
}

// KKT residuals and working sets (device); decides which rows are done.
int Solver::select(int it, int64_t *nactive_out) {
    std::vector<int> act;
    for (int64_t r = 0; r < R; ++r)
        if (!done[r]) act.push_back((int)r);
    const int *rows_k = nullptr;
    RCCHK(ctl(act, dRows, &rows_k));
    trace("select");
    launch_select(rows_k, (int)act.size(), X, G, kind, Qp, lambda, o.max_add, capW, capP, viol_frac, PG, dFidx, dgF, dpgF, kSel, dBest, Xb, st);
    RCCHK(fetch(sel, dSel, sizeof(SelectOut) * Rp));
    HIPCHK(hipGetLastError());
    HIPCHK(stg.sync());
    int64_t nactive = 0, ncg = 0;
    double worst_all = 0;
    int maxm = 0;
    for (int r : act) {
        const SelectOut &s = sel[r];
        Fobj[r] = f[r] + s.l1;
        kkt[r] = std::isfinite(s.worst) && std::isfinite(f[r]) ? s.worst : INFINITY;
        // progress = a smaller KKT residual (the device made the same comparison and saved the iterate) or a smaller
        // objective beyond its noise: with thousands of coordinates entering at once (dense optima) the residual is
        // not monotone along a converging sequence, the objective is
        const bool fdown = Fobj[r] < Fbest[r] - std::max(10.0 * fn[r], 1e-13 * std::fabs(Fobj[r]));
        if (Fobj[r] < Fbest[r]) Fbest[r] = Fobj[r];
        if (kkt[r] < best[r]) {
            best[r] = kkt[r];
            stall[r] = 0;
        } else if (fdown) {
            stall[r] = 0;
        } else {
            ++stall[r];
        }
        if (kkt[r] <= o.tol) {
            done[r] = 1;
            continue;
        }
        if (stall[r] >= stall_cap) { // no progress: at the noise floor of the pass arithmetic (or a failed line search)
            done[r] = 1;
            atfloor[r] = 1;
            continue;
        }
        ++nactive;
        iscg[r] = s.m < 0;
        msz[r] = s.m < 0 ? 0 : s.m; // working set of the Cholesky step
        nW[r] = s.m < 0 ? -s.m : 0; // ... of a matrix-free row (listed in tiles for its preconditioner)
        if (iscg[r]) ++ncg;
        maxm = std::max(maxm, msz[r]);
    }
    worst_row = 0;
    for (int64_t r = 0; r < R; ++r) {
        if (done[r]) msz[r] = 0;
        const double k = std::min(kkt[r], best[r]);
        if (k > worst_all) worst_row = r;
        worst_all = std::max(worst_all, k);
    }
    if (o.verbose)
        fprintf(stderr, "[gml] it %3d active %6lld (cg %lld)  max-kkt %.3e  max|W| %d  passes %d fwd %d  hv %lld  t %.2f s%s\n", it, (long long)nactive,
                (long long)ncg, worst_all, maxm, stats.passes, stats.forward_passes, (long long)stats.hv_evals, gml_now_s() - t_begin,
                prec == GML_PREC_F64 && o.precision != prec ? "  [fp64 polish]" : "");
    if (o.verbose >= 2)
        for (int64_t r : {dbg_row, worst_row})
            if (r < R && (r == dbg_row || worst_row != dbg_row))
                fprintf(stderr, "[gml]   row %lld: kkt %.3e best %.3e F %.15e m %d nsupp %d nviol %d stall %d\n", (long long)r, kkt[r], best[r], Fobj[r],
                        sel[r].m, sel[r].nsupp, sel[r].nviol, stall[r]);
    *nactive_out = nactive;
    return GML_OK;
}

// Polish: rows that the int8-limb arithmetic could not bring below tol (its gradient carries ~sqrt(K) 2^-31 of noise relative
// to the largest weight, which an ill-conditioned, weakly regularised problem amplifies) continue on the FP64 path from their
// best iterate, when that path fits in memory.
int Solver::start_polish(bool *started) {
    *started = false;
    std::vector<int> fl;
    for (int64_t r = 0; r < R; ++r)
        if (atfloor[r] && !(std::min(best[r], kkt[r]) <= o.tol)) fl.push_back((int)r);
    if (!(gml_is_i8(prec) && can_polish && !fl.empty())) return GML_OK;
    if (gml_ensure_f64(p, Rp) != GML_OK) return GML_OK; // does not fit after all: the rows stay as they are (reported not converged)
    prec = GML_PREC_F64;
    stall_cap = 10;
    RCCHK(upload_rows(fl, dRows));
    launch_copy_rows(dRows, (int)fl.size(), Qp, Xb, X, nullptr, nullptr, st); // back to the best iterate
    std::vector<double> inf((size_t)Rp, INFINITY);
    HIPCHK(stg.h2d(dBest, inf.data(), sizeof(double) * Rp));
    for (int r : fl) reopen(r);
    if (o.verbose) fprintf(stderr, "[gml] polish: %zu rows continue on the FP64 path\n", fl.size());
    RCCHK(run_pass(fl, X, G, true, false, at_x));
    set_kh((int64_t)fl.size());
    stats.polished = 1;
    *started = true;
    return GML_OK;
}

// rows whose V planes were overwritten (a wrapped slot range) need a fresh pass before the curvature; such a pass can
// itself overwrite planes that are still needed, hence the loop: its last round re-evaluates every active row from
// slot 0 (they always fit)
int Solver::refresh_stale() {
    for (int round = 0; round < 3; ++round) {
        std::vector<int> stale;
        for (int64_t r = 0; r < R; ++r)
            if (!done[r] && slots.needs_refresh((int)r)) stale.push_back((int)r);
        if (stale.empty()) break;
        if (round == 2) {
            stale.clear();
            for (int64_t r = 0; r < R; ++r)
                if (!done[r]) stale.push_back((int)r);
            slots.start_over();
        }
        RCCHK(run_pass(stale, X, G, true, false, at_x));
    }
    return GML_OK;
}


// batched Cholesky on the device; the directions are scattered into D
int Solver::newton_blocks(const std::vector<int> &chol_rows) {
    if (chol_rows.empty()) return GML_OK;
    trace("cholesky");
    int maxm = 1;
    for (int r : chol_rows) maxm = std::max(maxm, msz[r]);
    const int *rows_k = nullptr;
    RCCHK(ctl(chol_rows, dRows, &rows_k));
    // (a block over every configuration is the Hessian itself: nothing to correct -- and a secant over a finite step would spoil it)
    const bool secant = Kh < d.Kp;
    if (secant)
        launch_secant(rows_k, (int)chol_rows.size(), dFidx, dMt + 2 * R, capP, X, Qp, dgF, dH, dHoff, dMt, dS1, s2(), dYnoise, dFprev, dMprev, dXprev, dGprev,
                      dSec, dSec + 2 * Rp * capP, dNpairs, Rp * (int64_t)capP, kCholLds, st);
    if (secant && o.verbose >= 2) {
        std::vector<int> npv((size_t)Rp);
        HIPCHK(hipMemcpyAsync(npv.data(), dNpairs, sizeof(int) * Rp, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        int c[3] = {0, 0, 0};
        for (int r : chol_rows) ++c[std::min(2, npv[r])];
        fprintf(stderr, "[gml]   secant pairs in use: none %d rows, one %d, two %d\n", c[0], c[1], c[2]);
    }
    // (the kernel also re-solves on the orthant face where the projection of the line search would clip the step: as for the
    // matrix-free rows, newton_cg_group, but inside the one launch)
    NewtonFaces nf;
    nf.F = dFidx;
    nf.X = X;
    nf.kind = kind;
    nf.Qp = Qp;
    nf.share = cg::kFaceShare;
    // (a re-solve costs as much as the solve; what it saves is backtracking passes, whose cost grows with configurations x
    // statistics: config 2 -- 1e5 x 256 -- is 0.4 ms faster without, the headline problem 4 % faster with)
    nf.rounds = (double)p->K * (double)Qp >= 268435456.0 ? cg::kFaceRounds : 0;
    if (tune[GML_TUNE_FACE_ROUNDS] > 0) nf.rounds = (int)tune[GML_TUNE_FACE_ROUNDS] - 1;
    if (rec) { // the pairs as k_secant left them (without a secant: as they were)
        std::vector<int> npv((size_t)Rp);
        RCCHK(rec_download(npv.data(), dNpairs, sizeof(int) * Rp));
        for (int r : chol_rows) rec_row(r)[TRR_NPAIRS] = npv[r];
        rec->its.back().hdr[TRH_SECANT] = secant;
        rec->its.back().hdr[TRH_FACE_ROUNDS] = nf.rounds;
    }
    // (blocks of up to kCholLds entries take the secant correction inside the solve, on the matrix in LDS; k_secant above kept the
    // pairs and corrected the larger blocks itself)
    SecantPairs sp;
    if (secant) sp = SecantPairs{dSec, dSec + 2 * Rp * capP, dNpairs, Rp * (int64_t)capP};
    launch_newton_solve(dH, dHoff, dMt, dMt + 2 * R, dS1, s2(), dgF, dpgF, (int)R, capP, dsol, dSdiag, st, maxm, &nf, nullptr, nullptr, secant ? &sp : nullptr);
    launch_scatter_dir(rows_k, (int)chol_rows.size(), dFidx, dsol, dMt + 2 * R, capP, Qp, D, st);
    HIPCHK(hipGetLastError());
    return GML_OK;
}


// Projected backtracking line search.  Two acceptance regimes per row:
//  * the predicted decrease is well above the uncertainty of f  -> Armijo on F;
//  * otherwise ("noise regime": near the optimum, or a noisy int8-limb f) function values cannot certify the step; the trial
//    is then a full pass and is accepted iff the directional derivative of F at the trial point back towards x is >= 0 (up
//    to an overshoot allowance): F is convex, so such a trial cannot have increased F.
// The passes of this iteration use fresh slot ranges: the V planes of the previous ones are no longer needed.
int Solver::line_search() {
    slots.start_over();
    for (int64_t r = 0; r < R; ++r) {
        need[r] = !done[r];
        alpha[r] = 1.0;
        accepted_fwd[r] = 0;
    }
    for (int ls = 0; ls < 30; ++ls) {
        std::vector<int> rows;
        for (int64_t r = 0; r < R; ++r)
            if (need[r]) rows.push_back((int)r);
        if (rows.empty()) break;
        const int *rows_k = nullptr;
        const double *alpha_k = nullptr;
        RCCHK(ctl(rows, dRows, &rows_k));
        RCCHK(ctl(alpha, dAlpha, &alpha_k));
        trace("trial");
        launch_trial(rows_k, (int)rows.size(), X, D, PG, kind, Qp, lambda, alpha_k, Xt, kTrial, dStepn, st);
        // The first trial of an iteration is a full pass whatever the trial's scalars say, and the one thing the pass needs of them --
        // |trial - x|_1, which scales the unit of its weights -- is applied on the device (k_quant_theta): the host does not wait here,
        // the scalars come down with the results of the pass.  Later trials choose their kind of pass from the scalars.
        const bool early = ls > 0;
        auto read_trial = [&]() {
            for (int r : rows) {
                dd[r] = trial[r].dd;
                stepn[r] = trial[r].stepn; // ||trial - x||_1: bounds the change of every energy
                l1t[r] = trial[r].l1t;
                nreg[r] = !(-0.1 * dd[r] > 8.0 * fn[r]); // the step's expected decrease (~|dd|/2) vs the uncertainty of f
            }
        };
        bool anynoise = false;
        if (early) {
            RCCHK(fetch(trial, dTrial, sizeof(TrialOut) * Rp));
            HIPCHK(hipGetLastError());
            HIPCHK(stg.sync());
            read_trial();
            for (int r : rows) anynoise |= nreg[r] != 0;
        }
        const bool full = (ls == 0) || anynoise;
        // a full pass is followed on the stream by the directional derivatives back towards x: both come down in one wait
        const std::function<int()> back = [&]() -> int {
            const int *rk = nullptr; // (listed again: a re-run of some rows repeats this after a wait, which recycles the arena)
            RCCHK(ctl(rows, dRows, &rk));
            launch_back(rk, (int)rows.size(), X, Xt, Gt, kind, Qp, lambda, kTrial, st);
            RCCHK(fetch(trial, dTrial, sizeof(TrialOut) * Rp));
            return GML_OK;
        };
        RCCHK(run_pass(rows, Xt, Gt, full, true, at_xt, -1, full ? &back : nullptr, !early));
        if (!early) read_trial();
        std::vector<int> acc;
        for (int r : rows) {
            bool ok;
            if (rec) {
                rec_row(r)[TRR_TRIALS] += 1.0;
                rec_row(r)[TRR_ALPHA] = alpha[r];
                rec_row(r)[TRR_NREG] = nreg[r];
            }
            if (nreg[r]) {
                const double bk = trial[r].back;
                ok = std::isfinite(ft[r]) && std::isfinite(bk) && bk >= -0.5 * std::fabs(dd[r]);
            } else {
                const double Fn = ft[r] + l1t[r];
                ok = std::isfinite(Fn) && Fn <= Fobj[r] + 1e-4 * dd[r] + fn[r] + fnt[r];
            }
            if (o.verbose >= 2 && r == dbg_row)
                fprintf(stderr, "[gml]   row %d: ls %d alpha %.3g nreg %d ft %.12e Fobj %.12e dd %.3e fnt %.3e back %.3e ok %d\n", r, ls, alpha[r],
                        (int)nreg[r], ft[r], Fobj[r], dd[r], fnt[r], trial[r].back, (int)ok);
            if (ok) {
                // int8 passes: the iterate moves onto the point the scale was measured at.  FP64 phase: its trial passes measure no scale,
                // so the iterate moves away from where the last int8 pass of the row measured one -- the objective pass that direction_blocks
                // borrows for the matrix-free rows must allow for that distance, or its weights leave the fixed-point range
                dref[r] = gml_is_i8(prec) ? 0.0 : dref[r] + stepn[r];
                f[r] = ft[r];
                fn[r] = fnt[r];
                Z[r] = Zt[r];
                acc.push_back(r);
                if (!full) accepted_fwd[r] = 1; // (its V planes still belong to the old iterate)
                need[r] = 0;
                if (rec) {
                    rec_row(r)[TRR_ACCEPTED] = 1.0;
                    rec_row(r)[TRR_FULL] = full;
                }
            } else {
                if (!gml_is_i8(prec)) slots.mark_stale(r); // the FP64 path's V is indexed by row: every trial overwrites it
                else if (full) slots.reject_trial(r);      // the planes just written belong to the rejected point
                alpha[r] *= 0.5;
                if (nreg[r] && alpha[r] < 1.0 / 64) {
                    need[r] = 0;   // cannot improve along this direction: the stall counter ends the row,
                    stall[r] += 3; // after at most three such line searches (each costs ~7 passes)
                    if (rec) rec_row(r)[TRR_GAVE_UP] = 1.0;
                }
            }
        }
        if (o.verbose >= 2) {
            int nn = 0;
            for (int r : rows) nn += nreg[r] != 0;
            fprintf(stderr, "[gml]   ls %2d: %zu rows (%d in the noise regime), %zu accepted, %s pass\n", ls, rows.size(), nn, acc.size(), full ? "full" : "forward");
        }
        const int *acc_k = nullptr;
        RCCHK(ctl(acc, dRows2, &acc_k));
        launch_copy_rows(acc_k, (int)acc.size(), Qp, Xt, X, full ? Gt : nullptr, G, st);
        HIPCHK(hipGetLastError());
    }
    // rows accepted on an objective-only trial still need their gradient (and V)
    std::vector<int> rows;
    for (int64_t r = 0; r < R; ++r)
        if (accepted_fwd[r]) rows.push_back((int)r);
    if (!rows.empty()) RCCHK(run_pass(rows, X, G, true, false, at_x));
    // rows whose line search failed entirely stay where they are; the stall counter ends them
    if (rec) {
        TrajIter &t = rec->its.back();
        t.hdr[TRH_LINE_SEARCH] = 1.0;
        t.X.assign((size_t)R * Qp, 0.0);
        RCCHK(rec_download(t.X.data(), X, sizeof(double) * (size_t)R * Qp));
    }
    return GML_OK;
}

// results in the reference layout
int Solver::finish(double *out, double *kkt_out, int iterations) {
    int notconv = 0;
    double maxk = 0;
    std::vector<int> frombest, fromx;
    for (int64_t r = 0; r < R; ++r) {
        const double k = std::min(best[r], kkt[r]);
        if (!(k <= o.tol)) ++notconv;
        maxk = std::max(maxk, k);
        if (kkt_out) kkt_out[r] = k;
        (best[r] <= kkt[r] ? frombest : fromx).push_back((int)r);
    }
    if (rec) {
        rec->from_best.assign((size_t)R, 0);
        for (int r : frombest) rec->from_best[r] = 1;
    }
    // best iterate per row -> Xt (free now)
    RCCHK(upload_rows(frombest, dRows));
    launch_copy_rows(dRows, (int)frombest.size(), Qp, Xb, Xt, nullptr, nullptr, st);
    RCCHK(upload_rows(fromx, dRows2));
    launch_copy_rows(dRows2, (int)fromx.size(), Qp, X, Xt, nullptr, nullptr, st);
    // reference layout on the device (the direction array D is free now), then ONE copy: to the caller's host matrix, or --
    // `out` a device pointer (gml_multi_learn's dev_out blocks, device-side callers) -- device to device
    double *dres = D; // [R][P], P <= Qp
    RCCHK(ref_cols());
    launch_rows_to_reference(Xt, R, Qp, P, p->node0, d.cconst, dColsRef, dres, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dres, sizeof(double) * R * P, gml_is_device_ptr(out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    HIPCHK(stg.sync());
    stats.iterations = iterations;
    stats.max_kkt = maxk;
    stats.not_converged = notconv;
    stats.t_hess = dir_time.seconds();
    // (the host does not wait at the end of the direction phase: what of it was still running when the first trial pass was queued
    // shows up in that pass's host-side wait)
    stats.t_pass = std::max(0.0, stats.t_pass - std::max(0.0, stats.t_hess - t_dir_host));
    if (notconv)
        return fail(GML_ENOTCONV, "%d of %lld nodes did not reach the KKT tolerance %.1e (worst %.3e)", notconv, (long long)R, o.tol, maxk);
    return GML_OK;
}

// multi-body key order (:94-104): the column of every parameter slot of every local row, from the host, once per solve
int Solver::ref_cols() {
    if (p->order == 2 || dColsRef) return GML_OK;
    std::vector<int32_t> cols((size_t)R * P);
    gml_parallel_for(R, [&](int64_t r) {
        NodeLayout L;
        gml_build_layout(p, p->node0 + r, L);
        std::memcpy(cols.data() + (size_t)r * P, L.cols.data(), sizeof(int32_t) * P);
    });
    HIPCHK(A.get(&dColsRef, (size_t)R * P));
    HIPCHK(hipMemcpyAsync(dColsRef, cols.data(), sizeof(int32_t) * R * P, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st)); // cols is a local
    return GML_OK;
}

// the caller's structure over the kinds k_kind wrote (host or device pointer; a host array was checked by gml_learn_structured)
int Solver::apply_structure() {
    RCCHK(ref_cols());
    const uint8_t *src = structure;
    int64_t lds = ld_s;
    if (!gml_is_device_ptr(structure)) {
        uint8_t *tmp = nullptr;
        HIPCHK(A.get(&tmp, (size_t)R * P));
        HIPCHK(hipMemcpy2DAsync(tmp, (size_t)P, structure, (size_t)ld_s, (size_t)P, (size_t)R, hipMemcpyHostToDevice, st));
        src = tmp;
        lds = P;
    }
    int *dcnt = nullptr;
    unsigned long long *dbad = nullptr;
    HIPCHK(A.get(&dcnt, (size_t)R));
    HIPCHK(A.get(&dbad, 1));
    HIPCHK(hipMemsetAsync(dcnt, 0, sizeof(int) * R, st));
    HIPCHK(hipMemsetAsync(dbad, 0xFF, sizeof(unsigned long long), st));
    launch_apply_structure(src, lds, R, P, Qp, dNode, d.cconst, dColsRef, kind, dcnt, dbad, st);
    HIPCHK(hipGetLastError());
    nparam.assign((size_t)R, 0);
    unsigned long long bad = 0;
    HIPCHK(hipMemcpyAsync(nparam.data(), dcnt, sizeof(int) * R, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&bad, dbad, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad != ~0ull)
        return fail(GML_EINVAL, "structure: row %lld, slot %lld holds a value outside {0, 1, 2}", (long long)(bad / (unsigned long long)P),
                    (long long)(bad % (unsigned long long)P));
    return GML_OK;
}

// warm start: X <- the caller's rows (reference layout, host or device pointer)
int Solver::load_x0() {
    RCCHK(ref_cols());
    const double *src = x0;
    if (!gml_is_device_ptr(x0)) {
        double *tmp = nullptr;
        HIPCHK(A.get(&tmp, (size_t)R * P));
        HIPCHK(hipMemcpyAsync(tmp, x0, sizeof(double) * R * P, hipMemcpyHostToDevice, st));
        src = tmp;
    }
    int *dbad = nullptr;
    HIPCHK(A.get(&dbad, 4));
    HIPCHK(hipMemsetAsync(dbad, 0, sizeof(int) * 4, st));
    launch_ref_to_internal(src, P, R, P, Qp, dNode, d.cconst, dColsRef, X, dbad, st);
    if (structure) launch_mask_x0(kind, R, Qp, X, dbad + 1, st); // entries at excluded slots are ignored, whatever they hold
    HIPCHK(hipGetLastError());
    int bad[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(bad, dbad, sizeof bad, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad[structure ? 1 : 0]) return fail(GML_EINVAL, "the starting point contains a non-finite value");
    return GML_OK;
}

int Solver::iterate(double *out, double *kkt_out) {
    // first pass at X = 0: every energy is 0, the forward kernel skips its sweeps over the columns (the same bits without the GEMM:
    // 3.4 -> 1 ms of the headline solve's first pass); a warm start (gml_learn_warm) begins at the caller's rows instead
    std::vector<int> rows_all;
    for (int64_t r = 0; r < R; ++r) {
        if (structure && nparam[r] == 0) { // no parameter: x = 0 is the solution; the row never reaches a pass or the selection
            done[r] = 1;
            kkt[r] = best[r] = 0.0;
            continue;
        }
        rows_all.push_back((int)r);
    }
    if (x0) RCCHK(load_x0());
    at_zero = x0 == nullptr;
    const int rc0 = run_pass(rows_all, X, G, true, false, at_x);
    at_zero = false;
    RCCHK(rc0);
    int it = 0;
    for (it = 0; it < o.max_iter; ++it) {
        int64_t nactive = 0;
        const std::vector<uint8_t> done_before = coarse_on ? done : std::vector<uint8_t>();
        RCCHK(select(it, &nactive));
        if (coarse_on) {
            // A gradient of the coarse form (30-bit theta, 23-bit weights) must not certify anything: as soon as a row comes within
            // coarse_thr of its optimum -- or is declared converged -- by such a gradient, the coarse phase ends for good, those rows
            // are evaluated again at full width where they stand, their best-iterate records start over, and the selection is redone.
            const double thr = std::max(coarse_thr, 100.0 * o.tol);
            std::vector<int> low;
            bool dense = false; // a row has gone matrix-free: a dense optimum, whose many more iterations gain nothing from cheaper early
                                // passes (config 5 at the default regulariser: 52 iterations instead of 39 for the same wall-clock)
            for (int64_t r = 0; r < R; ++r) dense |= !done[r] && iscg[r];
            // (also the rows this selection ended at their stall count, above the threshold: declared done on coarse gradients)
            for (int64_t r = 0; r < R; ++r)
                if (!done_before[r] && (done[r] || !(kkt[r] > thr) || dense)) low.push_back((int)r);
            if (!low.empty()) {
                coarse_on = false;
                if (o.verbose)
                    fprintf(stderr, "[gml] it %3d: %s: the passes switch from the coarse form to full width (%zu rows re-evaluated)\n", it,
                            dense ? "rows have gone matrix-free (dense optimum)" : "rows have come within the coarse threshold of their optimum", low.size());
                const double inf = INFINITY;
                for (int r : low) {
                    reopen(r);
                    HIPCHK(stg.h2d(dBest + r, &inf, sizeof(double)));
                }
                RCCHK(run_pass(low, X, G, true, false, at_x));
                RCCHK(select(it, &nactive));
            }
        }
        if (rec) RCCHK(rec_select(it, nactive));
        if (nactive == 0) {
            bool polishing = false;
            RCCHK(start_polish(&polishing));
            if (!polishing) break;
            continue;
        }
        set_kh(nactive);
        if (rec) {
            double *h = rec->its.back().hdr;
            h[TRH_KH] = (double)Kh;
            h[TRH_KSTRIDE] = (double)kstride;
            h[TRH_HSCALE] = hscale;
        }
        trace("refresh");
        RCCHK(refresh_stale());
        trace("refreshed");
        std::vector<int> chol_rows, cg_rows;
        for (int64_t r = 0; r < R; ++r)
            if (!done[r]) (iscg[r] ? cg_rows : chol_rows).push_back((int)r);
        dir_time.mark();
        const double t_dir0 = gml_now_s();
        RCCHK(direction_blocks(cg_rows));
        RCCHK(newton_blocks(chol_rows));
        RCCHK(newton_cg(cg_rows));
        trace("directions done");
        dir_time.mark();
        t_dir_host += gml_now_s() - t_dir0;
        RCCHK(line_search());
    }
    return finish(out, kkt_out, it);
}

namespace {

// one solve of gml_learn_structured at precision prec, under `structure` (NULL: the reference's), from x0 (NULL: zeros) to out / kkt_out;
// *st: its stats, the wall-clock columns filled
int solve_once(gml_problem *p, int formulation, gml_opts o, int prec, double lambda, const uint8_t *structure, int64_t ld_s, const double *x0,
               double t_start, double *out, double *kkt_out, gml_stats *st, bool *underflow = nullptr) {
    o.precision = prec;
    Solver s(p, formulation, o, lambda);
    s.x0 = x0;
    s.structure = structure;
    s.ld_s = ld_s;
    int rc = s.init();
    if (rc == GML_OK) rc = s.iterate(out, kkt_out);
    s.stats.t_total = gml_now_s() - t_start;
    s.stats.t_pack = p->t_ingest[3];
    // everything that is neither a pass nor the direction phase: selection, trial points, bookkeeping
    s.stats.t_host = std::max(0.0, s.stats.t_total - s.stats.t_pass - s.stats.t_hess);
    *st = s.stats;
    if (underflow) *underflow = s.underflow;
    return rc;
}

} // namespace

extern "C" int gml_learn(gml_problem *p, int formulation, double regularizer_c, const gml_opts *opts_in, double *out,
                         double *kkt_out, gml_stats *stats_out) {
    return gml_learn_warm(p, formulation, regularizer_c, opts_in, nullptr, out, kkt_out, stats_out);
}

extern "C" int gml_learn_warm(gml_problem *p, int formulation, double regularizer_c, const gml_opts *opts_in, const double *x0, double *out,
                              double *kkt_out, gml_stats *stats_out) {
    return gml_learn_structured(p, formulation, regularizer_c, opts_in, nullptr, 0, x0, out, kkt_out, stats_out);
}

extern "C" int gml_learn_structured(gml_problem *p, int formulation, double regularizer_c, const gml_opts *opts_in, const uint8_t *structure,
                                    int64_t ld_s, const double *x0, double *out, double *kkt_out, gml_stats *stats_out) {
    if (!p || !out) return fail(GML_EINVAL, "NULL argument");
    if (formulation < 0 || formulation > 2) return fail(GML_EINVAL, "unknown formulation %d", formulation);
    if (formulation != GML_RISE && p->order != 2)
        return fail(GML_EUNSUPPORTED, "multi-body statistics are defined for RISE only (multiRISE, :83-152)");
    if (!(regularizer_c >= 0)) return fail(GML_EINVAL, "regularizer must be >= 0");
    gml_opts o;
    if (opts_in) o = *opts_in;
    else gml_default_opts(&o);
    // (auto: gml_internal.h -- the 38/31-bit limbs, the FP64-grade ones for tight tolerances and for small problems)
    const int asked = o.precision;
    const bool asked_auto = asked == GML_PREC_AUTO;
    o.precision = gml_resolve_precision(p, asked, o.tol > 0 ? o.tol : 1e-9);
    if (o.precision < 0) return fail(GML_EINVAL, "unknown precision %d", asked);
    if (structure) {
        if (ld_s < p->P) return fail(GML_EINVAL, "structure: leading dimension %lld < %lld parameters per node", (long long)ld_s, (long long)p->P);
        if (!gml_is_device_ptr(structure)) // (a device array is checked by the kernel that reads it: Solver::apply_structure)
            for (int64_t r = 0; r < p->node1 - p->node0; ++r)
                for (int64_t j = 0; j < p->P; ++j)
                    if (structure[r * ld_s + j] > GML_PARAM_PENALISED)
                        return fail(GML_EINVAL, "structure: row %lld, slot %lld holds %d, not one of GML_PARAM_EXCLUDED, _FREE, _PENALISED",
                                    (long long)r, (long long)j, (int)structure[r * ld_s + j]);
    }
    HIPCHK(hipSetDevice(p->device));
    const double t_start = gml_now_s();
    const double lambda = gml_lambda(regularizer_c, p->n, p->M);
    bool underflow = false;
    gml_stats st{};
    int rc = solve_once(p, formulation, o, o.precision, lambda, structure, ld_s, x0, t_start, out, kkt_out, &st, &underflow);
    if (stats_out && (rc == GML_OK || rc == GML_ENOTCONV)) *stats_out = st;
    if (rc == GML_EUNSUPPORTED && underflow && asked_auto) {
        // `auto` is the reference's Float64 solve (:164-181) by other means: a histogram whose optimum lies where exp(-E) spreads over
        // hundreds of units (c = 0 on near-separable data, |theta|_1 in the hundreds) cannot be held by the int8 limbs at an iterate;
        // the reference returns a result there, so `auto` runs the solve again on the FP64-MFMA path.  A caller who named an
        // int8-limb precision keeps the error.
        const std::string first = gml_last_error();
        rc = solve_once(p, formulation, o, GML_PREC_F64, lambda, structure, ld_s, x0, t_start, out, kkt_out, &st);
        if (rc != GML_OK && rc != GML_ENOTCONV)
            return fail(rc, "%s; the FP64 path, which precision auto falls back to, then failed: %s", first.c_str(), std::string(gml_last_error()).c_str());
        st.polished = 1; // (finished on the FP64 path)
        if (stats_out) *stats_out = st;
    } else if (rc == GML_ENOTCONV && asked_auto && gml_is_i8(o.precision) && (double)p->K * (double)p->P * (double)p->n <= 268435456.0) {
        // The other way an int8-limb solve can differ from the Float64 solve `auto` stands for: no row leaves the fixed-point range,
        // but the iterates wander along a nearly flat direction on the noise of the limbs and never certify (RPLE at c = 0 on
        // near-separable data: profiles/r6_robust_sweep.txt; the FP64 path converges there in 22 iterations).  On SMALL problems --
        // every kernel launch-bound, the FP64 solve a few milliseconds -- `auto` therefore tries the FP64 path before it reports
        // "not converged", and keeps whichever solve ended with fewer unconverged rows (then the smaller residual).  Host `out` only.
        if (!gml_is_device_ptr(out)) {
            const std::string first = gml_last_error();
            const size_t R = (size_t)(p->node1 - p->node0);
            std::vector<double> out1(out, out + R * (size_t)p->P), kkt1;
            if (kkt_out) kkt1.assign(kkt_out, kkt_out + R);
            const gml_stats st1 = st; // (the first solve's, as *stats_out holds them)
            const int rc2 = solve_once(p, formulation, o, GML_PREC_F64, lambda, structure, ld_s, x0, t_start, out, kkt_out, &st);
            const bool usable = rc2 == GML_OK || rc2 == GML_ENOTCONV;
            const bool better = usable && (!stats_out || st.not_converged < st1.not_converged ||
                                           (st.not_converged == st1.not_converged && st.max_kkt < st1.max_kkt));
            if (better) {
                rc = rc2;
                st.polished = 1;
                if (stats_out) *stats_out = st;
            } else { // the first solve stands
                std::copy(out1.begin(), out1.end(), out);
                if (kkt_out) std::copy(kkt1.begin(), kkt1.end(), kkt_out);
                if (stats_out) {
                    *stats_out = st1;
                    stats_out->t_total = gml_now_s() - t_start;
                }
                (void)fail(GML_ENOTCONV, "%s", first.c_str());
            }
        }
    }
    return rc;
}
