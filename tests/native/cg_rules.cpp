// Drives the host rules of the matrix-free direction phase (csrc/gml_cg_rules.h) on the host alone: one command per line of stdin,
// one line of results per command.  Doubles come in as C hex floats (or decimals) and go out as hex floats, so that
// tests/test_host_cg_rules.py can compare them with == to its model (tests/_newton_cg_reference.py).
//   constants
//   admitting nviol nsupp                         is_coarse hv_subsample nviol nsupp kkt tol
//   ksub_rule K maxW hv_subsample coarse          relax_schedule K maxW hv_subsample coarse
//   eta_rule nviol nsupp kkt cg_eta               stays_live rs rs0 pHp eta
//   solves_again nfixed mass total                route_is_sparse sparse_ok sumW ratio Qfp n
//   sparse_allowed has_i8 rple hv_lf hv_lb ko maxW
//   tile_layout T R nrows rows [nrows] nW [R]     -> ntiles | t0 [R] | vm | wrow
//   wblk n values [n]   /   Z n values [n]        (kept for the plan_scales commands that follow; print "ok")
//   plan_scales kchunk kpart nsplit Kp logrise Rp -> wsub kpart sc [Rp]
//   hv_ctl n node0 rows [n] slots [n]             -> np size | the block
#include "gml_cg_rules.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace gml::cg;

static double rd(std::istringstream &in) { // (operator>> does not read hex floats)
    std::string s;
    in >> s;
    return std::strtod(s.c_str(), nullptr);
}
static long long ri(std::istringstream &in) {
    long long v = 0;
    in >> v;
    return v;
}

int main() {
    std::vector<double> wblk, Z;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "constants") {
            printf("%a %a %d %d %d", kEtaAdmit, kFaceShare, kFaceRounds, kCoarsePerEntry, kRelaxPerEntry);
            for (const auto &sk : kRelaxSteps) printf(" %d %d", sk.first, sk.second);
        } else if (cmd == "admitting") {
            const long long nviol = ri(in), nsupp = ri(in);
            printf("%d", (int)admitting(nviol, nsupp));
        } else if (cmd == "is_coarse") {
            const int hv = (int)ri(in);
            const long long nviol = ri(in), nsupp = ri(in);
            const double kkt = rd(in), tol = rd(in);
            printf("%d", (int)is_coarse(hv, nviol, nsupp, kkt, tol));
        } else if (cmd == "ksub_rule" || cmd == "relax_schedule") {
            const long long K = ri(in), maxW = ri(in);
            const int hv = (int)ri(in);
            const bool coarse = ri(in) != 0;
            if (cmd == "ksub_rule") {
                printf("%d", ksub_rule(K, maxW, hv, coarse));
            } else {
                printf("relax");
                for (const auto &sk : relax_schedule(K, maxW, hv, coarse)) printf(" %d %d", sk.first, sk.second);
            }
        } else if (cmd == "eta_rule") {
            const long long nviol = ri(in), nsupp = ri(in);
            const double kkt = rd(in), cg_eta = rd(in);
            printf("%a", eta_rule(nviol, nsupp, kkt, cg_eta));
        } else if (cmd == "stays_live") {
            const double rs = rd(in), rs0 = rd(in), pHp = rd(in), eta = rd(in);
            printf("%d", (int)stays_live(rs, rs0, pHp, eta));
        } else if (cmd == "solves_again") {
            const long long nfixed = ri(in);
            const double mass = rd(in), total = rd(in);
            printf("%d", (int)solves_again(nfixed, mass, total));
        } else if (cmd == "route_is_sparse") {
            const bool ok = ri(in) != 0;
            const long long sumW = ri(in);
            const double ratio = rd(in);
            const long long Qfp = ri(in), n = ri(in);
            printf("%d", (int)route_is_sparse(ok, sumW, ratio, Qfp, n));
        } else if (cmd == "sparse_allowed") {
            const bool has_i8 = ri(in) != 0, rple = ri(in) != 0;
            const int lf = (int)ri(in), lb = (int)ri(in), ko = (int)ri(in);
            printf("%d", (int)sparse_allowed(has_i8, rple, lf, lb, ko, ri(in)));
        } else if (cmd == "tile_layout") {
            const int T = (int)ri(in);
            const long long R = ri(in), nrows = ri(in);
            std::vector<int> rows((size_t)nrows), nW((size_t)R);
            for (int &r : rows) r = (int)ri(in);
            for (int &w : nW) w = (int)ri(in);
            const TileLayout L = tile_layout(R, rows, nW.data(), T);
            printf("%lld |", (long long)L.ntiles());
            for (long long t : L.t0) printf(" %lld", t);
            printf(" |");
            for (int v : L.vm) printf(" %d", v);
            printf(" |");
            for (int v : L.wrow) printf(" %d", v);
        } else if (cmd == "wblk" || cmd == "Z") {
            std::vector<double> &v = cmd == "Z" ? Z : wblk;
            v.resize((size_t)ri(in));
            for (double &x : v) x = rd(in);
            printf("ok");
        } else if (cmd == "plan_scales") {
            const long long kchunk = ri(in), kpart = ri(in);
            const int nsplit = (int)ri(in);
            const long long Kp = ri(in);
            const bool logrise = ri(in) != 0;
            const long long Rp = ri(in);
            if ((long long)wblk.size() != Kp / 512 || (long long)Z.size() > Rp) {
                printf("bad plan_scales");
            } else {
                const PlanScales s = plan_scales(kchunk, kpart, nsplit, wblk.data(), Kp, Z.data(), (int64_t)Z.size(), logrise, Rp);
                printf("%a %lld", s.wsub, (long long)s.kpart);
                for (double v : s.sc) printf(" %a", v);
            }
        } else if (cmd == "hv_ctl") {
            const long long n = ri(in), node0 = ri(in);
            std::vector<int> rows((size_t)n), slots((size_t)n);
            for (int &r : rows) r = (int)ri(in);
            for (int &s : slots) s = (int)ri(in);
            const HvCtl L(n);
            const std::vector<int> ctl = L.pack([&](int64_t a) { return std::array<int, 3>{rows[(size_t)a], (int)(node0 + rows[(size_t)a]), slots[(size_t)a]}; });
            if (L.row() != 0 || L.node() != L.np || L.slot() != 2 * L.np || L.tile() != 3 * L.np || ctl.size() != L.size()) {
                printf("bad hv_ctl");
            } else {
                printf("%lld %zu |", (long long)L.np, L.size());
                for (int v : ctl) printf(" %d", v);
            }
        } else {
            printf("unknown command %s", cmd.c_str());
        }
        printf("\n");
    }
    return 0;
}
