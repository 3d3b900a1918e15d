// The matrix-free direction phase of gml_learn (Solver: gml_solver_impl.h), and the Hessian blocks both kinds of row start from.
// direction_blocks builds, in one Hessian call, the working-set blocks of the Cholesky rows and the preconditioner tiles of the
// matrix-free rows; newton_cg then solves H_WW d = -pg_W of every matrix-free row by preconditioned conjugate gradients.  The rules of
// the phase are the plain functions of gml_cg_rules.h; this file uploads, launches, waits and records (the recorder: at the end).
#include "gml_solver_impl.h"

#include <cmath>
#include <cstdio>

namespace gml {

using cg::RowCtl;
using cg::TileCtl;
// what the Hessian kernels take from the two blocks: the rows' alone, or rows and tiles
struct HessCall {
    const int *dMt, *hMt; // tiles of 32 per block: device, host
    const long long *dHoff;
    HessTiles tl;
};

// ---- the Hessian blocks -----------------------------------------------------------------------------------------------------------------
// Hessian blocks (int8 kernel over the limb planes of the rows' last passes, or the FP64 MFMA kernel over V): the working
// set of a Cholesky row; for a matrix-free row the tiles of its block-diagonal preconditioner (gml_solver.hip), inverted here.
// One upload carries the control block of the rows, one that of the tiles.
int Solver::direction_blocks(const std::vector<int> &cg_rows) {
    constexpr int T = MatrixFree::kTile;
    RCCHK(borrow_i8_planes(cg_rows));
    std::vector<char> rblk(RowCtl::bytes(R, Rp), 0);
    const RowCtl hrow(rblk.data(), R, Rp);
    fill_row_ctl(hrow);
    if (rec) rec_row_scales(hrow);
    // the tiles: kTile consecutive entries of W each, behind the rows' blocks
    const cg::TileLayout lay = cg::tile_layout(R, cg_rows, nW.data(), T);
    mf.ntiles = lay.ntiles();
    mf.tile_base = hrow.hoff[R];
    const int64_t htotal = std::max<long long>(mf.tile_base + mf.ntiles * (long long)T * T, 1);
    std::vector<char> tblk(TileCtl::bytes(R, mf.ntiles));
    const TileCtl htile(tblk.data(), R, mf.ntiles);
    if (mf.ntiles > 0) htile.fill(R, gml_is_i8(prec), hrow, lay, cg_rows, mf.tile_base, T);
    RCCHK(grow_hessian(htotal));
    RCCHK(check_planes(hrow));
    RCCHK(upload_row_ctl(rblk));
    HessCall hc{dMt, mf.ntiles > 0 ? htile.mt : hrow.mt, dHoff, HessTiles()};
    if (mf.ntiles > 0) RCCHK(upload_tile_ctl(tblk, cg_rows, &hc));
    RCCHK(launch_hessians(hc, htotal));
    if (rec && mf.ntiles > 0) RCCHK(rec_blocks(cg_rows, hrow));
    if (mf.ntiles > 0) trace("tile inverses");
    if (mf.ntiles > 0) launch_tile_inverse(T, dH, hc.dHoff + R, mf.dVm, mf.dWrow, dS1, s2(), mf.dgV, mf.ntiles, st);
    if (rec && mf.ntiles > 0) RCCHK(rec_blocks_inverses());
    HIPCHK(hipGetLastError());
    ++stats.hessian_passes;
    return GML_OK;
}

// FP64 phase: the curvature weights of the matrix-free rows' Hessian-vector products and preconditioner tiles come from
// an int8-limb objective pass at the same iterate (those run on the int8 cores either way; only the curvature is approximate)
int Solver::borrow_i8_planes(const std::vector<int> &cg_rows) {
    if (cg_rows.empty() || gml_is_i8(prec)) return GML_OK;
    std::vector<double> tf((size_t)R), tz((size_t)R, 1.0), tn((size_t)R);
    return run_pass(cg_rows, X, nullptr, false, false, PassOut{tf, tz, tn}, gml_is_i8(o.precision) ? o.precision : GML_PREC_I8X);
}

void Solver::fill_row_ctl(const RowCtl &h) {
    h.hoff[0] = 0;
    for (int64_t r = 0; r < Rp; ++r) h.s1[r] = h.s1cg[r] = 1.0;
    for (int64_t r = 0; r < R; ++r) h.ynoise[r] = 100.0 * fn[r]; // a gradient difference below this is noise of the pass arithmetic, not curvature
    for (int64_t r = 0; r < R; ++r) {
        const int m = done[r] || iscg[r] ? 0 : msz[r];
        h.mt[r] = (m + 31) / 32;
        h.node[r] = (int)(p->node0 + r);
        h.msz[r] = m; // the Cholesky step solves these
        h.plane[r] = slots.slot((int)r);
        h.hoff[r + 1] = h.hoff[r] + (long long)h.mt[r] * 32 * h.mt[r] * 32;
        const double zi = formulation == GML_LOGRISE ? 1.0 / Z[r] : 1.0; // Hess log Z = Hess Z / Z - g g^T
        h.s1[r] = hscale * zi; // sub-sampled blocks
        h.s1cg[r] = zi;        // the Hessian-vector products use every configuration
    }
}

int Solver::grow_hessian(int64_t htotal) {
    if (htotal <= dH_elems) return GML_OK;
    // regrown: the superseded block goes back now (a long solve of rows that keep admitting violators would otherwise hold
    // every earlier size until gml_learn returns), and the new size is checked against what the device has left
    A.release(dH);
    dH = nullptr;
    dH_elems = htotal + htotal / 4;
    size_t freeb = 0, totalb = 0;
    HIPCHK(dev_mem_info(&freeb, &totalb));
    if (8.0 * (double)dH_elems > 0.95 * (double)freeb) {
        if (8.0 * (double)htotal > 0.95 * (double)freeb)
            return fail(GML_ENOMEM, "Hessian blocks of %.1f GB do not fit in %.1f GB free HBM (lower max_working)", 8.0 * htotal / 1e9, freeb / 1e9);
        dH_elems = htotal;
    }
    HIPCHK(A.get(&dH, (size_t)dH_elems));
    return GML_OK;
}

int Solver::check_planes(const RowCtl &h) {
    for (int64_t r = 0; r < R; ++r) {
        const bool needs_planes = (gml_is_i8(prec) && h.mt[r] > 0) || (mf.ntiles > 0 && iscg[r] && !done[r]);
        if (needs_planes && !slots.valid((int)r))
            return fail(GML_EHIP, "internal: row %lld enters the Hessian without valid V planes (slot %d, owner %d, stale %d)", (long long)r,
                        slots.slot((int)r), slots.slot_owner((int)r), (int)slots.stale((int)r));
    }
    return GML_OK;
}

int Solver::upload_row_ctl(const std::vector<char> &blk) {
    HIPCHK(stg.h2d(dHctl, blk.data(), blk.size()));
    const RowCtl dv(dHctl, R, Rp); // (newton_blocks reads node and msz behind dMt)
    dMt = dv.mt;
    dPlane = dv.plane;
    dHoff = dv.hoff;
    dS1 = dv.s1;
    dYnoise = dv.ynoise;
    dS1cg = dv.s1cg;
    return GML_OK;
}

// ... and the rows' lists of working-set columns with the gradient on them (k_cg_tiles)
int Solver::upload_tile_ctl(const std::vector<char> &blk, const std::vector<int> &cg_rows, HessCall *hc) {
    constexpr int T = MatrixFree::kTile;
    if (blk.size() > mf.dTctl_bytes) {
        A.release(mf.dTctl);
        mf.dTctl_bytes = blk.size() + blk.size() / 4;
        HIPCHK(A.get(&mf.dTctl, mf.dTctl_bytes));
    }
    if (mf.ntiles > mf.tile_cap) {
        A.release(mf.dFV);
        A.release(mf.dgV);
        mf.tile_cap = mf.ntiles + mf.ntiles / 4;
        HIPCHK(A.get(&mf.dFV, (size_t)mf.tile_cap * T));
        HIPCHK(A.get(&mf.dgV, (size_t)mf.tile_cap * T));
    }
    HIPCHK(stg.h2d(mf.dTctl, blk.data(), blk.size()));
    const TileCtl dv(mf.dTctl, R, mf.ntiles);
    mf.dT0m = dv.t0;
    mf.dVm = dv.vm;
    mf.dWrow = dv.wrow;
    RCCHK(upload_rows(cg_rows, dRows2));
    launch_cg_tiles(dRows2, (int)cg_rows.size(), X, PG, G, kind, Qp, T, dv.t0, mf.dFV, mf.dgV, st);
    *hc = HessCall{dv.mt, hc->hMt, dv.hoff, HessTiles{mf.ntiles, T, mf.dFV, dv.wrow, dv.hflag}};
    return GML_OK;
}

int Solver::launch_hessians(const HessCall &hc, int64_t htotal) {
    // (the int8 kernel's finalisation writes every lower tile of the rows' blocks and the solve reads nothing else of them; the FP64
    // kernel accumulates in place, and the tiles' inverses read whole tiles)
    if (!gml_is_i8(prec) || mf.ntiles > 0) HIPCHK(hipMemsetAsync(dH, 0, sizeof(double) * htotal, st));
    trace("hessian");
    if (gml_is_i8(prec) || mf.ntiles > 0) {
        std::string err;
        const int hrc = i8_hessian(p->i8ws, d, dMt + R, dPlane, dFidx, hc.dMt, hc.hMt, hc.dHoff, htotal, (int)R, capP, formulation, Kh, kstride, dH, st, &err,
                                   mf.ntiles > 0 ? &hc.tl : nullptr);
        if (hrc) return fail(hrc, "%s", err.empty() ? "int8 Hessian: working set above 512 entries" : err.c_str());
    }
    if (!gml_is_i8(prec)) launch_hess_f64(d, p->dV, dMt + R, dFidx, dMt, dHoff, (int)R, capP, formulation, Kh, kstride, dH, st);
    return GML_OK;
}

// ---- Newton-CG ----------------------------------------------------------------------------------------------------------------------------
int Solver::newton_cg(const std::vector<int> &cg_rows) {
    if (cg_rows.empty()) return GML_OK;
    // two groups (cg::is_coarse): sub-sampled curvature for the rows still admitting violators, every configuration for the others
    std::vector<int> coarse, fine;
    for (int r : cg_rows) (cg::is_coarse(o.hv_subsample, sel[r].nviol, sel[r].nsupp, kkt[r], o.tol) ? coarse : fine).push_back(r);
    if (o.verbose >= 2) fprintf(stderr, "[gml]   cg groups: %zu rows admitting (sub-sampled curvature), %zu rows with every configuration\n", coarse.size(), fine.size());
    RCCHK(newton_cg_group(coarse, true));
    return newton_cg_group(fine, false);
}

// One group: rounds of CG steps.  Round 0 solves every row of the group; each further round solves again, on the orthant face their
// step ran into, the rows the face rule names.
int Solver::newton_cg_group(const std::vector<int> &rows, bool coarse) {
    if (rows.empty()) return GML_OK;
    trace("pcg");
    RCCHK(begin_group(rows, coarse));
    std::vector<int> cur = rows; // rows of this round
    for (int round = 0;; ++round) {
        RCCHK(cg_round(round, cur));
        if (round >= cg::kFaceRounds) break;
        std::vector<int> again;
        RCCHK(face_round(round, cur, &again));
        if (again.empty()) break;
        cur.swap(again);
    }
    return GML_OK;
}

// the first residual, preconditioned, and the first direction of every row; the plan of the group's products
int Solver::begin_group(const std::vector<int> &rows, bool coarse) {
    if (!mf.Rv) {
        HIPCHK(A.get(&mf.Rv, nd));
        HIPCHK(A.get(&mf.Pv, nd));
        HIPCHK(A.get(&mf.Hp, nd));
        HIPCHK(A.get(&mf.Zv, nd));
        HIPCHK(A.get(&mf.Wm, nd));
        HIPCHK(A.get(&mf.dFaces, (size_t)Rp));
        HIPCHK(A.get(&mf.dHv, (size_t)(3 * Rp + Rp / 32 + 8)));
    }
    mf.liveflag.assign((size_t)Rp, 0);
    mf.cgs.resize((size_t)Rp);
    mf.faces.resize((size_t)Rp);
    mf.maxW = 1;
    for (int r : rows) mf.maxW = std::max<int64_t>(mf.maxW, -(int64_t)sel[r].m);
    mf.relax = cg::relax_schedule(p->K, mf.maxW, o.hv_subsample, coarse);
    mf.sparse_ok = cg::sparse_allowed(p->i8ws != nullptr, formulation == GML_RPLE, mf.hv_lf, mf.hv_lb, d.ko, mf.maxW) && mf.dT0m != nullptr;
    RCCHK(set_live(rows));
    if (rec) rec_group(rows, coarse);
    // the rows' lists of W (k_cg_tiles, direction_blocks): the per-step vector kernels walk them instead of the 131 k columns
    if (!mf.dNw) HIPCHK(A.get(&mf.dNw, (size_t)Rp));
    HIPCHK(stg.h2d(mf.dNw, nW.data(), sizeof(int) * R));
    launch_pcg_init(dRows2, (int)rows.size(), X, PG, kind, Qp, D, mf.Rv, mf.Zv, mf.Pv, mf.Wm, dCg, st);
    precondition_and_direct(rows, 1);
    // (the gradient is always exact, so the optimum does not move; one split plan serves every step of this CG solve: one operator)
    return set_plan(cg::ksub_rule(p->K, mf.maxW, o.hv_subsample, coarse), rows.size(), 0, 0, 0);
}

// the rows of the kernels that follow: their list, and a flag by row
int Solver::set_live(const std::vector<int> &rows) {
    RCCHK(upload_rows(rows, dRows2));
    std::fill(mf.liveflag.begin(), mf.liveflag.end(), 0);
    for (int r : rows) mf.liveflag[r] = 1;
    HIPCHK(stg.h2d(mf.dLive, mf.liveflag.data(), sizeof(int) * Rp));
    return GML_OK;
}

// the split plan and the scales of the products over 1/ksub of the configurations, spread over the whole histogram and rescaled by
// the weight of the part
int Solver::set_plan(int ksub, size_t nrows, int where, int round, int ci) {
    const int64_t ngroups = gml_round_up((int64_t)nrows, 32) / 32;
    int64_t kchunk = 0, kpart = 0;
    int nsplit = 0;
    i8_split_plan(d, (int)ngroups, ksub, &kchunk, &kpart, &nsplit);
    const cg::PlanScales ps = cg::plan_scales(kchunk, kpart, nsplit, p->wblk.data(), d.Kp, Z.data(), R, formulation == GML_LOGRISE, Rp);
    mf.kchunk = kchunk;
    mf.kpart = ps.kpart;
    if (ps.kpart < kchunk && o.verbose >= 2)
        fprintf(stderr, "[gml]   cg: Hessian-vector products over 1/%d of the configurations (weight %.4f)\n", ksub, ps.wsub);
    HIPCHK(stg.h2d(dS1cg, ps.sc.data(), sizeof(double) * Rp)); // (the sub-sample's weight replaces the full sum)
    if (rec) rec_plan(where, round, ci, ksub, kchunk, nsplit, ngroups, ps);
    return GML_OK;
}

// out = (sum_k h_k x_k x_k^T) vec for the listed rows: a product over slots [0, n) of the u-plane workspace
int Solver::hv_product(const std::vector<int> &rows, const double *vec, double *out) {
    const cg::HvCtl L((int64_t)rows.size());
    int64_t sumW = 0;
    for (int r : rows) sumW += nW[r];
    const bool sparse = cg::route_is_sparse(mf.sparse_ok, sumW, mf.hv_sparse_ratio, d.Qfp, L.n) && i8_hv_sparse_bytes(d, (int)L.n, mf.maxW) <= ((size_t)2 << 30);
    const std::vector<int> ctl = L.pack([&](int64_t a) { return std::array<int, 3>{rows[a], (int)(p->node0 + rows[a]), slots.slot(rows[a])}; });
    HIPCHK(stg.h2d(mf.dHv, ctl.data(), sizeof(int) * ctl.size()));
    if (rec) RCCHK(rec_product_head(sparse, L, rows, ctl, vec));
    const size_t need = sparse ? i8_hv_sparse_bytes(d, (int)L.n, mf.maxW) : 0;
    if (need > mf.hvs_bytes) { // scratch of the entry-by-entry products
        const double tr = gml_now_s();
        A.release(mf.dHvsBuf);
        mf.dHvsBuf = nullptr;
        mf.hvs_bytes = std::max(need + need / 2, (size_t)16 << 20);
        char *b = nullptr;
        HIPCHK(A.get(&b, mf.hvs_bytes));
        mf.dHvsBuf = b;
        if (o.verbose) fprintf(stderr, "[gml]   scratch of the entry-by-entry products: %.0f MB (%.1f ms)\n", mf.hvs_bytes / 1048576.0, 1e3 * (gml_now_s() - tr));
    }
    std::string err;
    const int rc = hv_product_call(&p->i8ws, d, Scap, formulation, sparse, L, mf.dHv, mf.wl(), mf.maxW, mf.dHvsBuf, HvPlan{mf.kchunk, mf.kpart, mf.hv_lf, mf.hv_lb},
                                   vec, out, st, &err);
    if (rc) return fail(rc, "%s", err.c_str());
    if (sparse) ++g_hv_sparse_calls;
    ++stats.hessian_passes;
    stats.hv_evals += L.n;
    return GML_OK;
}

int hv_product_call(void **ws, const DevProblem &d, int64_t slot_capacity, int formulation, bool sparse, const cg::HvCtl &L, const int *ctl,
                    const WList &wl, int64_t wcap, void *scratch, const HvPlan &plan, const double *vec, double *out, hipStream_t st,
                    std::string *err) {
    if (sparse)
        return i8_hv_sparse(*ws, d, (int)L.n, ctl + L.row(), ctl + L.node(), ctl + L.slot(), wl.t0, wl.nw, wl.FV, wl.T, wcap, vec, out, plan.kchunk,
                            plan.kpart, scratch, st, err);
    I8Pass a{}; // (slots [0, np); no F)
    a.theta = vec;
    a.srow = ctl + L.row();
    a.rowcol = ctl + L.node();
    a.vmap = ctl + L.slot();
    a.groups = ctl + L.tile();
    a.ngroups = (int)L.ntiles();
    a.slot1 = (int)L.np;
    a.form = formulation;
    a.want_grad = true;
    a.G = out;
    a.hv = plan.lb == 2 ? 2 : 1;
    a.lf = plan.lf;
    a.kchunk = plan.kchunk;
    a.kpart = plan.kpart;
    return i8_pass(ws, d, slot_capacity, a, st, nullptr, err);
}

// Zv = M^-1 Rv on the tiles of the live rows, then the direction Pv from it (first: of a solve, else conjugated to the last one);
// dRows2 and dLive hold `rows` (set_live)
void Solver::precondition_and_direct(const std::vector<int> &rows, int first) {
    launch_tile_apply(MatrixFree::kTile, dH + mf.tile_base, mf.dFV, mf.dVm, mf.dWrow, mf.dLive, mf.ntiles, Qp, mf.Rv, mf.Zv, st);
    launch_pcg_dir(dRows2, (int)rows.size(), Qp, mf.Wm, mf.Rv, mf.Zv, mf.Pv, first, dCg, mf.wl(), st);
}

// the CG steps of one round over the rows `cur`, each until its row has converged (cg::stays_live) or max_cg steps are done
int Solver::cg_round(int round, const std::vector<int> &cur) {
    std::vector<int> live = cur;
    for (int ci = 0; ci < mf.maxcg && !live.empty(); ++ci) {
        if (round == 0)
            for (const auto &sk : mf.relax)
                if (ci == sk.first) RCCHK(set_plan(sk.second, live.size(), 1, round, ci));
        if (rec) rec_cg(TRC_STEP).iv = {round, ci};
        RCCHK(hv_product(live, mf.Pv, mf.Hp));
        if (rec) RCCHK(rec_rows_of(mf.Rv, live));
        if (rec) RCCHK(rec_rows_of(mf.Hp, live));
        RCCHK(upload_rows(live, dRows2));
        launch_pcg_step(dRows2, (int)live.size(), G, mf.Wm, Qp, dS1cg, s2(), mf.Hp, D, mf.Rv, mf.Pv, dCg, mf.wl(), st);
        HIPCHK(stg.d2h(mf.cgs.data(), dCg, sizeof(CgState) * Rp));
        HIPCHK(hipGetLastError());
        HIPCHK(stg.sync());
        if (rec) rec_step_state(live);
        std::vector<int> nxt;
        for (int r : live)
            if (cg::stays_live(mf.cgs[r].rs, mf.cgs[r].rs0, mf.cgs[r].pHp, cg::eta_rule(sel[r].nviol, sel[r].nsupp, kkt[r], mf.cg_eta))) nxt.push_back(r);
        live.swap(nxt);
        if (o.verbose >= 2) {
            fprintf(stderr, "[gml]   cg %2d: %zu rows live", ci, live.size());
            for (int64_t r : {dbg_row, worst_row})
                if (r < R && std::find(cur.begin(), cur.end(), (int)r) != cur.end())
                    fprintf(stderr, "  row %lld |r|/|r0| %.3e", (long long)r, std::sqrt(mf.cgs[r].rs / std::max(mf.cgs[r].rs0, 1e-300)));
            fprintf(stderr, "\n");
        }
        if (live.empty() || ci + 1 == mf.maxcg) break; // (at the cap the next direction would not be used)
        RCCHK(set_live(live));
        precondition_and_direct(live, 0);
    }
    if (rec) RCCHK(rec_round_end(round, cur));
    return GML_OK;
}

// orthant faces (gml_solver.hip, k_pcg_faces): the coordinates the projected step of a row would push through zero are fixed there
// and leave its system; *again: the rows that solve once more without them (cg::solves_again), from the exact residual of their clipped step
int Solver::face_round(int round, const std::vector<int> &cur, std::vector<int> *again) {
    RCCHK(upload_rows(cur, dRows2));
    launch_pcg_faces(dRows2, (int)cur.size(), X, PG, kind, Qp, D, mf.Wm, mf.dFaces, st);
    HIPCHK(stg.d2h(mf.faces.data(), mf.dFaces, sizeof(FaceOut) * Rp));
    HIPCHK(hipGetLastError());
    HIPCHK(stg.sync());
    int64_t nfixed = 0;
    for (int r : cur) {
        nfixed += mf.faces[r].nfixed;
        if (cg::solves_again(mf.faces[r].nfixed, mf.faces[r].mass, mf.faces[r].total)) again->push_back(r);
    }
    if (o.verbose >= 2)
        fprintf(stderr, "[gml]   cg faces (round %d): %lld coordinates fixed at zero in %zu rows; %zu rows solve again\n", round, (long long)nfixed,
                cur.size(), again->size());
    if (rec) rec_faces(round, cur, *again);
    const std::vector<int> &rows = *again;
    if (rows.empty()) return GML_OK; // else their re-solve starts
    if (!mf.relax.empty()) RCCHK(set_plan(1, rows.size(), 2, round + 1, 0));
    if (rec) rec_cg(TRC_RESOLVE).iv = {round + 1};
    RCCHK(hv_product(rows, D, mf.Hp));
    if (rec) RCCHK(rec_rows_of(mf.Hp, rows));
    RCCHK(set_live(rows));
    launch_pcg_resid(dRows2, (int)rows.size(), PG, G, Qp, dS1cg, s2(), mf.Hp, D, mf.Wm, mf.Rv, dCg, st);
    precondition_and_direct(rows, 1);
    if (rec) RCCHK(rec_cgstate(rows));
    return GML_OK;
}

// ---- the recorder (gml_solver.h: TRC_*; armed by tests only -- every method waits for the stream and downloads) ---------------------------
// whole rows of a [Rp][Qp] device array, to the open event
int Solver::rec_rows_of(const double *dev, const std::vector<int> &rows) {
    TrajCgEvent &ev = rec_open();
    std::vector<double> all(nd);
    RCCHK(rec_download(all.data(), dev, sizeof(double) * nd));
    for (int r : rows) ev.dv.insert(ev.dv.end(), all.begin() + (size_t)r * Qp, all.begin() + (size_t)(r + 1) * Qp);
    return GML_OK;
}

int Solver::rec_cgstate(const std::vector<int> &rows) {
    TrajCgEvent &ev = rec_open();
    std::vector<CgState> c((size_t)Rp);
    RCCHK(rec_download(c.data(), dCg, sizeof(CgState) * Rp));
    for (int r : rows) ev.dv.insert(ev.dv.end(), {c[r].rs, c[r].rs0, c[r].pHp, c[r].rz});
    return GML_OK;
}

// the unit (and, where asked, the largest magnitude) of the listed rows' V planes: a later objective pass overwrites them
int Solver::rec_tau(const std::vector<int> &rows, std::vector<double> &tau, std::vector<unsigned> *mmax) {
    const double *dtau = nullptr;
    const unsigned *dmm = nullptr;
    i8_slot_results(p->i8ws, 0, &dtau, &dmm);
    int smax = 0;
    for (int r : rows) smax = std::max(smax, slots.slot(r));
    std::vector<double> t((size_t)smax + 1, 0.0);
    std::vector<unsigned> mm((size_t)smax + 1, 0u);
    if (dtau) RCCHK(rec_download(t.data(), dtau, sizeof(double) * t.size()));
    if (mmax && dmm) RCCHK(rec_download(mm.data(), dmm, sizeof(unsigned) * mm.size()));
    for (int r : rows) {
        const int s = slots.slot(r);
        tau.push_back(s >= 0 ? t[(size_t)s] : 0.0);
        if (mmax) mmax->push_back(s >= 0 ? mm[(size_t)s] : 0u);
    }
    return GML_OK;
}

void Solver::rec_row_scales(const RowCtl &h) {
    for (int64_t r = 0; r < R; ++r) {
        rec_row(r)[TRR_S1] = h.s1[r];
        rec_row(r)[TRR_YNOISE] = h.ynoise[r];
    }
}

// TRC_BLOCKS: what the tiles were built from, and the blocks before their inversion
int Solver::rec_blocks(const std::vector<int> &cg_rows, const RowCtl &h) {
    constexpr int T = MatrixFree::kTile;
    const int64_t ntiles = mf.ntiles;
    TrajCgEvent &ev = rec_cg(TRC_BLOCKS);
    ev.iv = {(int64_t)cg_rows.size(), T, ntiles, Kh, kstride, Qp, prec, P};
    for (int r : cg_rows) ev.iv.push_back(r);
    for (int r : cg_rows) ev.iv.push_back(nW[r]);
    std::vector<long long> t0d((size_t)R);
    RCCHK(rec_download(t0d.data(), mf.dT0m, sizeof(long long) * R));
    for (int r : cg_rows) ev.iv.push_back(t0d[r]);
    std::vector<int> tv((size_t)(2 * ntiles)), fv((size_t)ntiles * T);
    RCCHK(rec_download(tv.data(), mf.dVm, sizeof(int) * 2 * ntiles)); // (vm | wrow)
    RCCHK(rec_download(fv.data(), mf.dFV, sizeof(int) * ntiles * T));
    ev.iv.insert(ev.iv.end(), tv.begin(), tv.end());
    ev.iv.insert(ev.iv.end(), fv.begin(), fv.end());
    std::vector<uint8_t> kd((size_t)R * Qp);
    RCCHK(rec_download(kd.data(), kind, kd.size()));
    for (int r : cg_rows) ev.iv.insert(ev.iv.end(), kd.begin() + (size_t)r * Qp, kd.begin() + (size_t)(r + 1) * Qp);
    std::vector<double> tau;
    std::vector<unsigned> mm;
    RCCHK(rec_tau(cg_rows, tau, &mm));
    ev.iv.insert(ev.iv.end(), mm.begin(), mm.end());
    for (int r : cg_rows) { // the column of every parameter of the result's layout
        if (p->order == 2) {
            for (int64_t j = 0; j < P; ++j) ev.iv.push_back(j == p->node0 + r ? d.cconst : j);
        } else {
            NodeLayout L;
            gml_build_layout(p, p->node0 + r, L);
            ev.iv.insert(ev.iv.end(), L.cols.begin(), L.cols.begin() + P);
        }
    }
    ev.dv.push_back(hscale);
    for (int r : cg_rows) ev.dv.push_back(h.s1[r]);
    ev.dv.insert(ev.dv.end(), tau.begin(), tau.end());
    RCCHK(rec_rows_of(X, cg_rows));
    RCCHK(rec_rows_of(PG, cg_rows));
    RCCHK(rec_rows_of(G, cg_rows));
    const size_t nb = (size_t)ntiles * T * T, at = ev.dv.size();
    ev.dv.resize(at + 2 * nb);
    return rec_download(ev.dv.data() + at, dH + mf.tile_base, sizeof(double) * nb);
}

// ... and the inverses the preconditioner applies
int Solver::rec_blocks_inverses() {
    TrajCgEvent &ev = rec_open();
    const size_t nb = (size_t)mf.ntiles * MatrixFree::kTile * MatrixFree::kTile;
    return rec_download(ev.dv.data() + ev.dv.size() - nb, dH + mf.tile_base, sizeof(double) * nb);
}

void Solver::rec_group(const std::vector<int> &rows, bool coarse) {
    TrajCgEvent &ev = rec_cg(TRC_GROUP);
    ev.iv = {coarse ? 1 : 0, (int64_t)rows.size(), mf.maxW};
    for (int r : rows) ev.iv.push_back(r);
    for (int r : rows) ev.iv.push_back(sel[r].nviol);
    for (int r : rows) ev.iv.push_back(sel[r].nsupp);
    for (int r : rows) ev.dv.push_back(kkt[r]);
    for (int r : rows) ev.dv.push_back(Z[r]);
}

void Solver::rec_plan(int where, int round, int ci, int ksub, int64_t kchunk, int nsplit, int64_t ngroups, const cg::PlanScales &ps) {
    TrajCgEvent &ev = rec_cg(TRC_PLAN);
    ev.iv = {where, round, ci, ksub, kchunk, ps.kpart, nsplit, ngroups, Rp};
    ev.dv.push_back(ps.wsub);
    ev.dv.insert(ev.dv.end(), ps.sc.begin(), ps.sc.end());
}

// the head of the open TRC_STEP / TRC_RESOLVE event: the route, the rows, the control block as uploaded, the product's vector
int Solver::rec_product_head(bool sparse, const cg::HvCtl &L, const std::vector<int> &rows, const std::vector<int> &ctl, const double *vec) {
    TrajCgEvent &ev = rec_open();
    ev.iv.insert(ev.iv.end(), {sparse ? 1 : 0, L.n, L.np});
    ev.iv.insert(ev.iv.end(), rows.begin(), rows.end());
    ev.iv.insert(ev.iv.end(), ctl.begin(), ctl.end());
    RCCHK(rec_rows_of(vec, rows));
    return rec_tau(rows, ev.dv, nullptr);
}

void Solver::rec_step_state(const std::vector<int> &live) {
    TrajCgEvent &ev = rec_open();
    for (int r : live) ev.dv.insert(ev.dv.end(), {mf.cgs[r].rs, mf.cgs[r].rs0, mf.cgs[r].pHp, mf.cgs[r].rz});
}

int Solver::rec_round_end(int round, const std::vector<int> &cur) {
    TrajCgEvent &ev = rec_cg(TRC_ROUND_END);
    ev.iv = {round, (int64_t)cur.size()};
    ev.iv.insert(ev.iv.end(), cur.begin(), cur.end());
    return rec_rows_of(D, cur);
}

void Solver::rec_faces(int round, const std::vector<int> &cur, const std::vector<int> &again) {
    TrajCgEvent &ev = rec_cg(TRC_FACES);
    ev.iv = {round, (int64_t)cur.size(), (int64_t)again.size()};
    ev.iv.insert(ev.iv.end(), cur.begin(), cur.end());
    for (int r : cur) ev.iv.push_back(mf.faces[r].nfixed);
    ev.iv.insert(ev.iv.end(), again.begin(), again.end());
    for (int r : cur) ev.dv.push_back(mf.faces[r].mass);
    for (int r : cur) ev.dv.push_back(mf.faces[r].total);
}

} // namespace gml
