// The host rules of the matrix-free direction phase (gml_newton_cg.cpp): which group a row solves in, over how many configurations
// its Hessian-vector products run, when a row leaves a CG solve, which rows solve again on an orthant face, which route a product
// takes, how the working sets are cut into preconditioner tiles, and how the control block of a product is laid out.  Every rule is
// a function of plain numbers -- no device, no solver state -- under the name the Python model of the phase gives it
// (tests/_newton_cg_reference.py), so that the two read side by side.  The solver calls these functions and holds no copy of them.
//
// Modelled on gml_slots.h: plain C++17 with no device header; tests/native/cg_rules.cpp drives it on the host alone.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace gml {
namespace cg {

// ---- constants -------------------------------------------------------------------------------------------------------------------------
constexpr double kEtaAdmit = 0.25;  // residual reduction asked of a row that is still admitting violators
constexpr double kFaceShare = 0.05; // a row solves again when the clipped coordinates carry more than this share of its predicted decrease
constexpr int kFaceRounds = 2;      // re-solves of a CG system without the coordinates its step would push through zero
constexpr int kCoarsePerEntry = 32; // configurations per working-set entry the sub-sampled products of the coarse group keep
constexpr int kRelaxPerEntry = 16;  // ... and the relaxed products of the fine group
constexpr std::pair<int, int> kRelaxSteps[2] = {{2, 2}, {4, 8}}; // (from this CG step on, over 1 / this many configurations)

// ---- groups ----------------------------------------------------------------------------------------------------------------------------
// still building its support: violators at the scale of the support itself (k_select admits them by halves of the largest
// violation; once they are few next to the support, all at once)
inline bool admitting(int64_t nviol, int64_t nsupp) { return nviol * 16 > nsupp; }

// Two groups.  Rows that are still ADMITTING violators (coordinates at zero whose pseudo-gradient is not: the support is
// not final, the iteration count of a dense optimum is set by how many of them are let in per iteration, not by the
// accuracy of the step) and are not yet within max(1e3 tol, 1e-5) of their optimum take Hessian-vector products over a
// sub-sample of the configurations (the coarse group, ksub_rule).  Rows whose support is final take every configuration (the fine
// group): with the approximate curvature a row converges only linearly (the residual halves per iteration at 60 configurations per
// working-set entry -- the weights exp(-E) are far from uniform), and the last digits come from a few exact Newton steps (measured on
// config 5 at the default regulariser: sub-sampled throughout, a handful of the 512 rows creep at 5e-6 for a hundred iterations).
inline bool is_coarse(int hv_subsample, int64_t nviol, int64_t nsupp, double kkt, double tol) {
    return hv_subsample != 1 && admitting(nviol, nsupp) && kkt > std::max(1e3 * tol, 1e-5);
}

// ---- configurations of the products --------------------------------------------------------------------------------------------------
// Sub-sampled curvature: the products of the coarse group run over ~1/ksub of the configurations -- as many as keep 32 of them per
// working-set entry (the sample covariance of |W| statistics from 32 |W| configurations has its eigenvalues within (1 +- 0.18)^2 of
// the true ones: a Newton step that is only solved to a 5 % residual loses nothing to that), at most 8 -- or what hv_subsample forces.
inline int ksub_rule(int64_t K, int64_t maxW, int hv_subsample, bool coarse) {
    if (!coarse) return 1;
    return hv_subsample > 0 ? hv_subsample : (int)std::min<int64_t>(8, std::max<int64_t>(1, K / (kCoarsePerEntry * maxW)));
}

// Relaxed products (inexact Krylov: Simoncini & Szyld 2003, van den Eshof & Sleijpen 2004).  The error a product may carry
// without moving the attainable residual grows like 1 / |r_j|: the first steps of an exact-curvature solve need every
// configuration, the later ones -- whose search directions only correct a residual that is already a fraction of the
// right-hand side -- do not.  From step 2 on the products run over 1/2, from step 4 on over 1/8 of the configurations
// (as long as 16 configurations per working-set entry remain).  Config 5 at the default regulariser: the same 43-44 Newton
// iterations and 59-67 k products, 36.4 -> 26.2 s; the step where the cut starts matters (over 1/4 from step 2: 28.1 s and
// 70 k products; from step 1: 31.3 s, 56 iterations).  hv_subsample = 1 keeps every product exact.
// (step, ksub) of round 0 of the fine group.
inline std::vector<std::pair<int, int>> relax_schedule(int64_t K, int64_t maxW, int hv_subsample, bool coarse) {
    std::vector<std::pair<int, int>> relax;
    if (coarse || hv_subsample != 0) return relax;
    for (const std::pair<int, int> &sk : kRelaxSteps) {
        const int ks = (int)std::min<int64_t>(sk.second, K / (kRelaxPerEntry * maxW));
        if (ks > 1) relax.push_back({sk.first, ks});
    }
    return relax;
}

// What the products of one plan are scaled with.  (kchunk, kpart, nsplit) as i8_split_plan made them; wblk: the weight of every block
// of 512 configurations; Z [R] the rows' partition sums (read for logRISE only: Hess log Z = Hess Z / Z - g g^T).  wsub: the weight
// of the participating blocks, summed chunk by chunk, block by block.  A sub-sample that shrinks and carries weight rescales by
// 1 / wsub; any other runs over whole chunks (kpart = kchunk).  sc [Rp]: the padding rows have no Z.
struct PlanScales {
    double wsub;
    int64_t kpart; // as the products get it
    std::vector<double> sc;
};
inline PlanScales plan_scales(int64_t kchunk, int64_t kpart, int nsplit, const double *wblk, int64_t Kp, const double *Z, int64_t R, bool logrise,
                              int64_t Rp) {
    PlanScales s{0.0, kpart, std::vector<double>((size_t)Rp)};
    for (int c = 0; c < nsplit; ++c)
        for (int64_t b = c * kchunk / 512; b < std::min((c * kchunk + kpart) / 512, Kp / 512); ++b) s.wsub += wblk[(size_t)b];
    const bool shrinks = kpart < kchunk && s.wsub > 0;
    if (!shrinks) s.kpart = kchunk;
    for (int64_t r = 0; r < Rp; ++r) {
        const double zi = r < R && logrise ? 1.0 / Z[r] : 1.0;
        s.sc[r] = shrinks ? zi / s.wsub : zi;
    }
    return s;
}

// ---- one CG solve ----------------------------------------------------------------------------------------------------------------------
// Inexact Newton: the residual is reduced by eta = min(cg_eta, sqrt(kkt)); a row that is still admitting violators needs a step that
// is good at the scale of its largest violation, not more.
inline double eta_rule(int64_t nviol, int64_t nsupp, double kkt, double cg_eta) {
    return admitting(nviol, nsupp) ? kEtaAdmit : std::min(cg_eta, std::sqrt(std::max(kkt, 1e-300)));
}
// after a step: the row goes on while its curvature along the direction is positive and its residual is above eta of the first
inline bool stays_live(double rs, double rs0, double pHp, double eta) { return pHp > 0 && rs > eta * eta * rs0; }

// orthant faces: the rows whose projected step would lose a noticeable part of its predicted decrease to the clipping solve again
// without the clipped coordinates
inline bool solves_again(int64_t nfixed, double mass, double total, double share = kFaceShare) { return nfixed > 0 && mass > share * total; }

// ---- route of a product ----------------------------------------------------------------------------------------------------------------
// The GEMM pass costs the same for a tile of 32 rows whatever the number of live ones in it; few rows go entry by entry instead (same
// integers, gml_hv_sparse.hip: their iterates do not depend on the path).  The entry-by-entry form exists for the exp forms, two-limb
// products, statistics of at most two spins besides the node's own (ko <= 2) and working sets up to 65 536.
inline bool sparse_allowed(bool has_i8, bool rple, int hv_lf, int hv_lb, int ko, int64_t maxW) {
    return has_i8 && !rple && hv_lf == 2 && hv_lb == 2 && ko <= 2 && maxW <= 65536;
}
// ... and is taken when the working sets of the n live rows sum to less than ratio x (statistics columns x node tiles of the GEMM pass)
inline bool route_is_sparse(bool sparse_ok, int64_t sumW, double ratio, int64_t Qfp, int64_t n) {
    return sparse_ok && (double)sumW < ratio * (double)Qfp * (double)((n + 31) / 32);
}

// ---- preconditioner tiles --------------------------------------------------------------------------------------------------------------
// The tiles of the listed rows, in list order: T consecutive entries of a row's working set each.  t0 [R]: the first tile of every row
// (0 for a row without any); vm, wrow [ntiles]: entries in use and row of every tile.
struct TileLayout {
    std::vector<long long> t0;
    std::vector<int> vm, wrow;
    int64_t ntiles() const { return (int64_t)vm.size(); }
};
inline TileLayout tile_layout(int64_t R, const std::vector<int> &rows, const int *nW, int T) {
    TileLayout L;
    L.t0.assign((size_t)R, 0);
    for (int r : rows) {
        L.t0[r] = L.ntiles();
        for (int64_t t = 0; t < (nW[r] + T - 1) / T; ++t) {
            L.vm.push_back((int)std::min<int64_t>(T, nW[r] - t * T));
            L.wrow.push_back(r);
        }
    }
    return L;
}

// ---- control blocks of the Hessian call ----------------------------------------------------------------------------------------------
// Each block is laid out once, by a struct of pointers built over the host copy and again over the device buffer.
// The rows': mt [R] | node [R] | msz of the Cholesky rows [R] | (unused) [R] | plane slot [R] | hoff [R+1] | s1 [Rp] | ynoise [Rp] | s1cg [Rp]
struct RowCtl {
    int *mt, *node, *msz, *plane;
    long long *hoff;
    double *s1, *ynoise, *s1cg;
    static size_t ibytes(int64_t R) { return (sizeof(int) * 5 * R + 7) & ~(size_t)7; }
    static size_t bytes(int64_t R, int64_t Rp) { return ibytes(R) + sizeof(long long) * (R + 1) + sizeof(double) * 3 * Rp; }
    RowCtl(char *base, int64_t R, int64_t Rp)
        : mt(reinterpret_cast<int *>(base)), node(mt + R), msz(mt + 2 * R), plane(mt + 4 * R), hoff(reinterpret_cast<long long *>(base + ibytes(R))),
          s1(reinterpret_cast<double *>(hoff + R + 1)), ynoise(s1 + Rp), s1cg(s1 + 2 * Rp) {}
};
// The tiles' (NV = R + ntiles blocks, the tiles' behind the rows'): hoffV [NV] | t0 [R] | mtV [NV] | vm [ntiles] | wrow [ntiles] | hflag [R]
struct TileCtl {
    long long *hoff, *t0;
    int *mt, *vm, *wrow, *hflag;
    static size_t bytes(int64_t R, int64_t ntiles) { return sizeof(long long) * (2 * R + ntiles) + sizeof(int) * (2 * R + 3 * ntiles); }
    TileCtl(char *base, int64_t R, int64_t ntiles)
        : hoff(reinterpret_cast<long long *>(base)), t0(hoff + R + ntiles), mt(reinterpret_cast<int *>(t0 + R)), vm(mt + R + ntiles), wrow(vm + ntiles),
          hflag(wrow + ntiles) {}
    // rows_i8: the rows' blocks come from this call too (FP64 phase: from launch_hess_f64, the call then skips them); a tile is T / 32
    // tiles of 32 wide, the t-th at tile_base + t T T; hflag: the rows whose weights the call needs
    void fill(int64_t R, bool rows_i8, const RowCtl &rows, const TileLayout &lay, const std::vector<int> &cg_rows, long long tile_base, int T) const {
        for (int64_t r = 0; r < R; ++r) {
            mt[r] = rows_i8 ? rows.mt[r] : 0;
            hoff[r] = rows.hoff[r];
            hflag[r] = mt[r] > 0;
        }
        for (int r : cg_rows) hflag[r] = 1;
        for (int64_t t = 0; t < lay.ntiles(); ++t) {
            mt[R + t] = T / 32;
            hoff[R + t] = tile_base + t * (long long)T * T;
        }
        std::memcpy(t0, lay.t0.data(), sizeof(long long) * R);
        std::memcpy(vm, lay.vm.data(), sizeof(int) * lay.ntiles());
        std::memcpy(wrow, lay.wrow.data(), sizeof(int) * lay.ntiles());
    }
};

// ---- control block of a product ------------------------------------------------------------------------------------------------------
// n product rows in the slots [0, np), np = n rounded up to 32:  row [np] | node [np] | plane slot [np] | node tile [np / 32] | 4 unused.
// The padding slots hold row 0, node -1 (unused slot), plane slot 0; the unused tail holds -1 (it pads the tile list to a multiple of 4).
// One object gives the offsets to the host packing and to the device pointers.
struct HvCtl {
    int64_t n, np;
    explicit HvCtl(int64_t n_) : n(n_), np((n_ + 31) / 32 * 32) {}
    int64_t row() const { return 0; }
    int64_t node() const { return np; }
    int64_t slot() const { return 2 * np; }
    int64_t tile() const { return 3 * np; }
    int64_t ntiles() const { return np / 32; }
    size_t size() const { return (size_t)(3 * np + np / 32 + 4); }
    // entry(a) = {row, node, plane slot} of the a-th product row, a < n
    template <typename Entry> std::vector<int> pack(Entry entry) const {
        std::vector<int> ctl(size(), -1);
        for (int64_t a = 0; a < np; ++a) {
            const std::array<int, 3> e = a < n ? entry(a) : std::array<int, 3>{0, -1, 0};
            ctl[(size_t)(row() + a)] = e[0];
            ctl[(size_t)(node() + a)] = e[1];
            ctl[(size_t)(slot() + a)] = e[2];
        }
        for (int64_t g = 0; g < ntiles(); ++g) ctl[(size_t)(tile() + g)] = (int)g;
        return ctl;
    }
};

} // namespace cg
} // namespace gml
