// libgml_hip, host side: exact log Z, means and term expectations by variable elimination (gml_model_elim_plan, gml_model_elim;
// gml_elim.hip) and exact draws by backward sampling on the same tables (gml_problem_create_sampled_elim;
// gml_elim_draw.hip).  The planner -- adjacency of the reduced keys, the greedy order, the frontier sizes -- is plain C++
// and makes no HIP call; the driver turns every connected component's steps into launches (slots, scope masks, maps) and runs the
// forward pass and then, for the moments, the backward pass or, for the draws, every sample's walk over the kept tables.
#include "gml_elim.h"
#include "gml_sampled.h"

#include <cstddef>
#include <limits>
#include <set>

using namespace gml;

namespace {

// The order and what it costs.  seq: the spins component by component (the components in the order of their smallest spin), comp_end[c]:
// one past the last step of component c.  last[u]: the step at which u retires (the step of its last neighbour, or its own).
struct ElimOrder {
    std::vector<std::vector<int>> adj;
    std::vector<int> seq, pos, last, comp_end;
    int width = 0;
    double work = 0.0, stored = 0.0;
};

// spins that share a term of non-zero weight (after cancellation) are neighbours
void build_adjacency(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, std::vector<std::vector<int>> &adj) {
    adj.assign((size_t)n, {});
    std::vector<int> sp;
    for (int64_t t = 0; t < nterms; ++t) {
        if (weights[t] == 0.0) continue;
        reduce_key(keys + t * key_stride, key_stride, sp);
        for (size_t a = 0; a < sp.size(); ++a)
            for (size_t b = 0; b < sp.size(); ++b)
                if (a != b) adj[(size_t)sp[a]].push_back(sp[b]);
    }
    for (auto &l : adj) {
        std::sort(l.begin(), l.end());
        l.erase(std::unique(l.begin(), l.end()), l.end());
    }
}

// The greedy order.  A component starts at its lowest spin; then, of the unprocessed spins next to the frontier, the one whose step
// leaves the smallest frontier, the lowest index among equals.  left[u] = the unprocessed neighbours of u: the step of c retires the
// frontier spins whose only unprocessed neighbour is c, and c itself if it has none.  Cost per step: the neighbour lists of
// every current candidate (up to frontier x degree of them): no scan of all spins, but O(n^2) visits in all where the frontier grows
// with n (hubs).
void greedy_order(const std::vector<std::vector<int>> &adj, std::vector<int> &seq) {
    const size_t n = adj.size();
    std::vector<int> left(n);
    for (size_t i = 0; i < n; ++i) left[i] = (int)adj[i].size();
    std::vector<char> done(n, 0);
    std::set<int> cand;
    size_t lowest = 0;
    int F = 0;
    seq.clear();
    while (seq.size() < n) {
        int v = -1;
        if (cand.empty()) {
            while (done[lowest]) ++lowest;
            v = (int)lowest;
        } else {
            int best = std::numeric_limits<int>::max();
            for (int c : cand) {
                int gone = left[(size_t)c] == 0 ? 1 : 0;
                for (int u : adj[(size_t)c])
                    if (done[(size_t)u] && left[(size_t)u] == 1) ++gone;
                if (F + 1 - gone < best) {
                    best = F + 1 - gone;
                    v = c;
                }
            }
        }
        seq.push_back(v);
        done[(size_t)v] = 1;
        cand.erase(v);
        F += left[(size_t)v] == 0 ? 0 : 1;
        for (int u : adj[(size_t)v]) {
            --left[(size_t)u];
            if (!done[(size_t)u]) cand.insert(u);
            else if (left[(size_t)u] == 0) --F;
        }
    }
}

// a caller's permutation: the components in the order of their smallest spin, each one's spins in the order the permutation names them
void caller_order(const std::vector<std::vector<int>> &adj, const int32_t *order, std::vector<int> &seq) {
    const size_t n = adj.size();
    std::vector<int> comp(n, -1), stack;
    int ncomp = 0;
    for (size_t i = 0; i < n; ++i) {
        if (comp[i] >= 0) continue;
        comp[i] = ncomp;
        stack.assign(1, (int)i);
        while (!stack.empty()) {
            const int u = stack.back();
            stack.pop_back();
            for (int w : adj[(size_t)u])
                if (comp[(size_t)w] < 0) {
                    comp[(size_t)w] = ncomp;
                    stack.push_back(w);
                }
        }
        ++ncomp;
    }
    std::vector<size_t> at((size_t)ncomp + 1, 0);
    for (size_t i = 0; i < n; ++i) ++at[(size_t)comp[i] + 1];
    for (int c = 0; c < ncomp; ++c) at[(size_t)c + 1] += at[(size_t)c];
    seq.assign(n, 0);
    for (size_t i = 0; i < n; ++i) seq[at[(size_t)comp[(size_t)order[i]]]++] = order[i];
}

int plan_order(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, const int32_t *order, ElimOrder &P) {
    if (order) {
        std::vector<char> seen((size_t)n, 0);
        for (int64_t i = 0; i < n; ++i) {
            if (order[i] < 0 || order[i] >= n || seen[(size_t)order[i]])
                return fail(GML_EINVAL, "order is not a permutation of 0 .. n - 1 (entry %lld is %d)", (long long)i, order[i]);
            seen[(size_t)order[i]] = 1;
        }
    }
    build_adjacency(keys, key_stride, weights, nterms, n, P.adj);
    if (order) caller_order(P.adj, order, P.seq);
    else greedy_order(P.adj, P.seq);
    P.pos.assign((size_t)n, 0);
    for (int64_t t = 0; t < n; ++t) P.pos[(size_t)P.seq[(size_t)t]] = (int)t;
    P.last.assign((size_t)n, 0);
    std::vector<int> retiring((size_t)n, 0);
    for (int64_t u = 0; u < n; ++u) {
        int l = P.pos[(size_t)u];
        for (int w : P.adj[(size_t)u]) l = std::max(l, P.pos[(size_t)w]);
        P.last[(size_t)u] = l;
        ++retiring[(size_t)l];
    }
    int F = 0;
    for (int64_t t = 0; t < n; ++t) {
        P.width = std::max(P.width, F + 1);
        P.work += std::ldexp(1.0, F + 1);
        F += 1 - retiring[(size_t)t];
        P.stored += std::ldexp(1.0, F);
        if (F == 0) P.comp_end.push_back((int)t + 1);
    }
    return GML_OK;
}

int check_model_args(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n) {
    if (int rc = check_term_pointers(keys, key_stride, weights, nterms)) return rc;
    if (n <= 0 || nterms < 0) return fail(GML_EINVAL, "n must be positive and nterms non-negative");
    if (n > std::numeric_limits<int32_t>::max()) return fail(GML_EINVAL, "n exceeds 2^31 - 1");
    return check_term_values(keys, key_stride, weights, nterms, n);
}

// ------------------------------------------------------------------------------------------
// One component as the kernels take it
// ------------------------------------------------------------------------------------------
struct Launch { // a forward launch; out_step: the step (1-based within the component) whose table it writes, -1: a table between
                // the launches of one step (scratch, unless the draws keep it); out_off: that table's place in the component's store
    int kin, kout, r, nt, t_off, mv_off, nmove, out_step;
    unsigned rbit[kElimMaxRetire], same;
    int spin[kElimMaxRetire]; // the spins at the retiring bits
    size_t out_off;
};
struct Step {
    int kin, kout, nt, t_off, mv_off, nmove, q_off, nq;
    unsigned same;
};
struct Component {
    std::vector<Step> steps;
    std::vector<Launch> launches;
    std::vector<unsigned> tmask, qmask;
    std::vector<double> tw;
    std::vector<unsigned short> mv;
    std::vector<int64_t> q_term; // per quantity: the caller's term (>= 0) or ~spin (a mean)
    std::vector<size_t> table_off; // table_off[t]: alpha_t in the forward store (t = 0 .. steps)
    size_t kept = 0;               // entries of the store with the tables between launches behind the alpha_t (the draws)
    int max_bits = 0, max_scratch_bits = 0;
    double log_z = 0.0;
    std::vector<double> res;
};

// Sum `ret` (positions, ascending) out of the table whose bit p holds cur[p]: the survivors below the new size keep their bit, the
// others fill the freed bits in ascending order.  Appends the moves (index bit | scope bit << 8); returns the mask of kept bits.
unsigned retire_bits(std::vector<int> &cur, const std::vector<int> &ret, std::vector<unsigned short> &mv, int &nmove) {
    const int k = (int)cur.size(), k2 = k - (int)ret.size();
    std::vector<char> goes((size_t)k, 0);
    for (int p : ret) goes[(size_t)p] = 1;
    std::vector<int> next((size_t)k2, -1);
    unsigned same = 0;
    int hi = k2;
    nmove = 0;
    for (int p = 0; p < k2; ++p) {
        if (!goes[(size_t)p]) {
            next[(size_t)p] = cur[(size_t)p];
            same |= 1u << p;
            continue;
        }
        while (goes[(size_t)hi]) ++hi;
        next[(size_t)p] = cur[(size_t)hi];
        mv.push_back((unsigned short)(p | hi << 8));
        ++nmove;
        ++hi;
    }
    cur.swap(next);
    return same;
}

// steps [t0, t1) of the order are one component
void plan_component(const ElimOrder &P, int t0, int t1, const std::vector<std::vector<int64_t>> &step_terms, const int32_t *keys,
                    int key_stride, const double *weights, Component &C) {
    std::vector<int> cur, sp, ret, scope_pos((size_t)P.adj.size(), -1);
    C.table_off.assign(1, 0);
    size_t stored = 1;
    for (int t = t0; t < t1; ++t) {
        const int v = P.seq[(size_t)t];
        Step S{};
        S.kin = (int)cur.size();
        cur.push_back(v);
        const std::vector<int> scope0 = cur; // the spin at every bit of the scope
        for (int p = 0; p <= S.kin; ++p) scope_pos[(size_t)cur[(size_t)p]] = p;
        // the step's terms and quantities as masks over the scope
        S.t_off = (int)C.tmask.size();
        S.q_off = (int)C.qmask.size();
        for (int64_t term : step_terms[(size_t)t]) {
            reduce_key(keys + term * key_stride, key_stride, sp);
            unsigned m = 0;
            for (int u : sp) m |= 1u << scope_pos[(size_t)u];
            C.tmask.push_back(m);
            C.tw.push_back(weights[term]);
            C.qmask.push_back(m);
            C.q_term.push_back(term);
        }
        S.nt = (int)C.tmask.size() - S.t_off;
        ret.clear();
        for (int p = 0; p <= S.kin; ++p)
            if (P.last[(size_t)cur[(size_t)p]] == t) {
                ret.push_back(p);
                C.qmask.push_back(1u << p);
                C.q_term.push_back(~(int64_t)cur[(size_t)p]);
            }
        S.nq = (int)C.qmask.size() - S.q_off;
        // the launches: the first introduces v and adds phi; each sums out at most kElimMaxRetire of the retiring spins
        size_t done = 0;
        do {
            Launch L{};
            L.kin = done == 0 ? S.kin : (int)cur.size();
            L.nt = done == 0 ? S.nt : 0;
            L.t_off = S.t_off;
            L.r = (int)std::min<size_t>(kElimMaxRetire, ret.size() - done);
            std::vector<int> now;
            for (int i = 0; i < L.r; ++i) {
                // (the positions of the spins still to retire, in the table as the launches before have left it)
                const int spin = scope0[(size_t)ret[done + (size_t)i]];
                const int p = (int)(std::find(cur.begin(), cur.end(), spin) - cur.begin());
                now.push_back(p);
            }
            std::sort(now.begin(), now.end());
            for (int i = 0; i < L.r; ++i) {
                L.rbit[i] = 1u << now[(size_t)i];
                L.spin[i] = cur[(size_t)now[(size_t)i]];
            }
            L.mv_off = (int)C.mv.size();
            L.same = retire_bits(cur, now, C.mv, L.nmove);
            L.kout = (int)cur.size();
            done += (size_t)L.r;
            L.out_step = done == ret.size() ? t - t0 + 1 : -1;
            L.out_off = stored; // (alpha_t; a table between launches gets its place below)
            if (L.out_step < 0) C.max_scratch_bits = std::max(C.max_scratch_bits, L.kout);
            C.launches.push_back(L);
        } while (done < ret.size());
        S.kout = (int)cur.size();
        // scope state -> index of the step's final table, for the backward pass
        S.mv_off = (int)C.mv.size();
        for (int b = 0; b < S.kout; ++b) {
            const int p = scope_pos[(size_t)cur[(size_t)b]];
            if (p == b) S.same |= 1u << b;
            else {
                C.mv.push_back((unsigned short)(b | p << 8));
                ++S.nmove;
            }
        }
        C.max_bits = std::max(C.max_bits, std::max(S.kin, S.kout));
        C.steps.push_back(S);
        stored += (size_t)1 << S.kout;
        C.table_off.push_back(stored - ((size_t)1 << S.kout));
    }
    for (Launch &L : C.launches)
        if (L.out_step < 0) {
            L.out_off = stored;
            stored += (size_t)1 << L.kout;
        }
    C.kept = stored;
}

// The whole model: the terms by the step of their last spin, in the caller's order (an empty key is a constant of log Z: its weight goes
// to `constants`); the components that need the device, in order; the spins in no term.
void plan_components(const ElimOrder &P, const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                     std::vector<Component> &comps, std::vector<int> &free_spins, std::vector<double> &constants) {
    std::vector<std::vector<int64_t>> step_terms((size_t)n);
    std::vector<int> sp;
    for (int64_t t = 0; t < nterms; ++t) {
        if (weights[t] == 0.0) continue;
        reduce_key(keys + t * key_stride, key_stride, sp);
        if (sp.empty()) {
            constants.push_back(weights[t]);
            continue;
        }
        int at = 0;
        for (int u : sp) at = std::max(at, P.pos[(size_t)u]);
        step_terms[(size_t)at].push_back(t);
    }
    for (size_t c = 0, t0 = 0; c < P.comp_end.size(); t0 = (size_t)P.comp_end[c++]) {
        if ((size_t)P.comp_end[c] == t0 + 1 && step_terms[t0].empty()) {
            free_spins.push_back(P.seq[t0]);
            continue;
        }
        comps.emplace_back();
        plan_component(P, (int)t0, P.comp_end[c], step_terms, keys, key_stride, weights, comps.back());
    }
}

// the entries of the tables between the launches of one step, over the whole order (what the draws keep beyond `stored`): a step of
// scope k that retires R > 3 spins leaves tables of k - 3, k - 6, ... bits before its last launch
double entries_between_launches(const ElimOrder &P) {
    std::vector<int> retiring(P.seq.size(), 0);
    for (int l : P.last) ++retiring[(size_t)l];
    double extra = 0.0;
    int F = 0;
    for (size_t t = 0; t < P.seq.size(); ++t) {
        for (int done = kElimMaxRetire; done < retiring[t]; done += kElimMaxRetire) extra += std::ldexp(1.0, F + 1 - done);
        F += 1 - retiring[t];
    }
    return extra;
}

ElimMap map_of(const unsigned short *dmv, int off, int nmove, unsigned same) { return ElimMap{same, nmove, dmv + off}; }

// What the launches of a call read, uploaded once: the terms and moves of all components in one array each; t0, q0, mv0: where
// component c starts in them (q0: in the quantities, which only the moments upload).  The host arrays live here until the caller has
// synchronised.
struct Uploaded {
    const unsigned *tmask = nullptr;
    const double *tw = nullptr;
    const unsigned short *mv = nullptr;
    std::vector<size_t> t0, q0, mv0;
    std::vector<unsigned> h_tmask, qmask;
    std::vector<double> h_tw;
    std::vector<unsigned short> h_mv;
    std::vector<ElimDrawLaunch> h_launches; // (the draws: the launch records, and the moves again as 32-bit words)
    std::vector<unsigned> h_mv32;
};

void upload_components(SamplerStaging &s, const std::vector<Component> &comps, Uploaded &U) {
    std::vector<unsigned> &tmask = U.h_tmask;
    std::vector<double> &tw = U.h_tw;
    std::vector<unsigned short> &mv = U.h_mv;
    mv.assign(1, 0); // (no empty upload)
    for (const Component &C : comps) {
        U.t0.push_back(tmask.size());
        U.q0.push_back(U.qmask.size());
        U.mv0.push_back(mv.size());
        tmask.insert(tmask.end(), C.tmask.begin(), C.tmask.end());
        tw.insert(tw.end(), C.tw.begin(), C.tw.end());
        U.qmask.insert(U.qmask.end(), C.qmask.begin(), C.qmask.end());
        mv.insert(mv.end(), C.mv.begin(), C.mv.end());
    }
    U.tmask = s.upload(tmask);
    U.tw = s.upload(tw);
    U.mv = s.upload(mv);
}

// The forward pass of component c on the stream: alpha_0 = 0 at alpha0, then its launches in order, each writing where place(L) says.
// Returns the place of alpha_n.
template <class Place> const double *run_forward(SamplerStaging &s, const Uploaded &U, const Component &C, size_t c, double *alpha0, Place &&place) {
    const unsigned *dtm = U.tmask + U.t0[c];
    const double *dtw = U.tw + U.t0[c];
    const unsigned short *dmv = U.mv + U.mv0[c];
    s.ok(hipMemsetAsync(alpha0, 0, sizeof(double), s.st), "hipMemsetAsync");
    const double *in = alpha0;
    for (const Launch &L : C.launches) {
        double *out = place(L);
        ElimForward A{};
        A.in = in;
        A.out = out;
        A.tmask = dtm + L.t_off;
        A.tw = dtw + L.t_off;
        A.nt = L.nt;
        A.map = map_of(dmv, L.mv_off, L.nmove, L.same);
        for (int i = 0; i < kElimMaxRetire; ++i) A.rbit[i] = L.rbit[i];
        A.kin = L.kin;
        A.kout = L.kout;
        launch_elim_forward(A, L.r, s.st);
        in = out;
    }
    return in;
}

// log Z and the moments.  All components of a call on one stream: their terms, quantities and moves uploaded together, the tables sized
// for the largest component and used by one after the other (the stream orders them), every component's alpha_n kept on the device for
// its backward pass, and one synchronisation at the end.
int run_components(std::vector<Component> &comps, bool moments, int device) {
    if (comps.empty()) return GML_OK;
    SamplerStaging s;
    if (int rc = s.open(device)) return rc;
    Uploaded U;
    upload_components(s, comps, U);
    const std::vector<size_t> &q0s = U.q0;
    int max_bits = 0, max_scratch_bits = 0;
    size_t max_store = 0;
    for (const Component &C : comps) {
        max_bits = std::max(max_bits, C.max_bits);
        max_scratch_bits = std::max(max_scratch_bits, C.max_scratch_bits);
        max_store = std::max(max_store, C.table_off.back() + 1);
    }
    const unsigned *dqm_all = s.upload(U.qmask);
    // forward tables: with the moments every alpha_t is kept; without, two tables take turns; the tables between the launches of one
    // step take turns in either case
    const size_t big = (size_t)1 << max_bits, scratch = (size_t)1 << max_scratch_bits, nq_all = U.qmask.size();
    const size_t wgs_max = std::max<size_t>(1, big / kElimChunk);
    double *store = nullptr, *ping[2] = {nullptr, nullptr}, *tmp[2], *beta[2] = {nullptr, nullptr}, *part[2] = {nullptr, nullptr};
    double *dres = nullptr;
    if (moments) {
        store = s.alloc<double>(max_store);
        beta[0] = s.alloc<double>(big);
        beta[1] = s.alloc<double>(big);
        part[0] = s.alloc<double>(wgs_max * kElimQuant);
        part[1] = s.alloc<double>((wgs_max / kElimChunk + 1) * kElimQuant);
        dres = s.alloc<double>(nq_all);
    } else {
        ping[0] = s.alloc<double>(big);
        ping[1] = s.alloc<double>(big);
    }
    tmp[0] = s.alloc<double>(scratch);
    tmp[1] = s.alloc<double>(scratch);
    double *dlogz = s.alloc<double>(comps.size());
    if (s.rc) return s.rc;
    for (size_t c = 0; c < comps.size() && s.rc == GML_OK; ++c) {
        const Component &C = comps[c];
        const unsigned *dtm = U.tmask + U.t0[c], *dqm = dqm_all + q0s[c];
        const double *dtw = U.tw + U.t0[c];
        const unsigned short *dmv = U.mv + U.mv0[c];
        const size_t nsteps = C.steps.size();
        int turn = 0, tturn = 0;
        const double *in = run_forward(s, U, C, c, moments ? store : ping[0], [&](const Launch &L) {
            if (L.out_step < 0) return tmp[tturn ^= 1];
            return moments ? store + L.out_off : ping[turn ^= 1];
        });
        s.ok(hipMemcpyAsync(dlogz + c, in, sizeof(double), hipMemcpyDeviceToDevice, s.st), "hipMemcpyAsync"); // alpha_n
        if (!moments) continue;
        // backward: beta_n = 0; step t reads beta_t and writes beta_{t-1}, whether or not it has quantities to sum; the quantities
        // of a step in windows of kElimQuant
        s.ok(hipMemsetAsync(beta[0], 0, sizeof(double), s.st), "hipMemsetAsync");
        int bt = 0;
        for (size_t t = nsteps; t-- > 0;) {
            const Step &S = C.steps[t];
            for (int q0 = 0; q0 == 0 || q0 < S.nq; q0 += kElimQuant) {
                ElimBackward B{};
                B.alpha = store + C.table_off[t];
                B.beta = beta[bt];
                B.beta_out = q0 == 0 ? beta[bt ^ 1] : nullptr;
                B.tmask = dtm + S.t_off;
                B.tw = dtw + S.t_off;
                B.nt = S.nt;
                B.map = map_of(dmv, S.mv_off, S.nmove, S.same);
                B.qmask = dqm + S.q_off + q0;
                B.nq = std::min(kElimQuant, S.nq - q0);
                B.kin = S.kin;
                B.log_z = dlogz + c;
                double *result = dres + q0s[c] + (size_t)(S.q_off + q0);
                long long count = (long long)std::max<size_t>(1, ((size_t)1 << S.kin) / kElimChunk);
                B.part = count == 1 ? result : part[0];
                launch_elim_backward(B, s.st);
                // the workgroups' sums, 1024 to one until one is left (a step without quantities has none)
                for (int side = 0; count > 1 && B.nq > 0; side ^= 1) {
                    const long long groups = (count + kElimChunk - 1) / kElimChunk;
                    launch_elim_fold(part[side], count, B.nq, groups == 1 ? result : part[side ^ 1], s.st);
                    count = groups;
                }
            }
            bt ^= 1;
        }
    }
    s.ok(hipGetLastError(), "the elimination's launches");
    std::vector<double> logz(comps.size()), res(std::max<size_t>(nq_all, 1));
    s.ok(hipMemcpyAsync(logz.data(), dlogz, sizeof(double) * logz.size(), hipMemcpyDeviceToHost, s.st), "hipMemcpyAsync");
    if (moments) s.ok(hipMemcpyAsync(res.data(), dres, sizeof(double) * nq_all, hipMemcpyDeviceToHost, s.st), "hipMemcpyAsync");
    if (s.sync()) return s.rc;
    for (size_t c = 0; c < comps.size(); ++c) {
        comps[c].log_z = logz[c];
        if (moments) comps[c].res.assign(res.begin() + (std::ptrdiff_t)q0s[c], res.begin() + (std::ptrdiff_t)(q0s[c] + comps[c].qmask.size()));
    }
    return GML_OK;
}

// The draws, into the output bytes of a begun staging (spin-major, leading dimension ld).  Every table of every component is kept --
// the store holds the components one behind the other -- so one kernel can walk all launches backward for every sample; then the
// spins in no term.  All on the staging's stream: no host round trip between the components, the synchronisation is finish()'s (U and
// free_spins hold the host side of the uploads until then).
void draw_components(SamplerStaging &s, const std::vector<Component> &comps, Uploaded &U, const std::vector<int> &free_spins, uint64_t seed,
                     int64_t N, int64_t ld) {
    if (!comps.empty()) {
        upload_components(s, comps, U);
        std::vector<size_t> base;
        size_t total = 0;
        for (const Component &C : comps) {
            base.push_back(total);
            total += C.kept;
        }
        double *store = s.alloc<double>(total);
        std::vector<ElimDrawLaunch> &recs = U.h_launches;
        for (size_t c = 0; c < comps.size() && s.rc == GML_OK; ++c) {
            const Component &C = comps[c];
            double *mine = store + base[c];
            run_forward(s, U, C, c, mine, [&](const Launch &L) { return mine + L.out_off; });
            size_t in_off = base[c]; // alpha_0
            for (const Launch &L : C.launches) {
                ElimDrawLaunch D{};
                D.in_off = (long long)in_off;
                D.t_off = (long long)(U.t0[c] + (size_t)L.t_off);
                D.same = L.same;
                for (int i = 0; i < kElimMaxRetire; ++i) {
                    D.rbit[i] = L.rbit[i];
                    D.spin[i] = L.spin[i];
                }
                D.kin = L.kin;
                D.r = L.r;
                D.nt = L.nt;
                D.mv_off = (int)(U.mv0[c] + (size_t)L.mv_off);
                D.nmove = L.nmove;
                recs.push_back(D);
                in_off = base[c] + L.out_off;
            }
        }
        ElimDraw D{};
        D.launches = s.upload(recs);
        D.nlaunch = (int)recs.size();
        D.store = store;
        D.tmask = U.tmask;
        D.tw = U.tw;
        U.h_mv32.assign(U.h_mv.begin(), U.h_mv.end());
        D.mv = s.upload(U.h_mv32);
        D.seed = seed;
        D.N = N;
        D.ld = ld;
        D.out = s.out;
        if (s.rc == GML_OK) launch_elim_draw(D, s.st);
    }
    const int *dfree = free_spins.empty() ? nullptr : s.upload(free_spins);
    if (s.rc == GML_OK) launch_elim_draw_free(dfree, (int)free_spins.size(), seed, N, ld, s.out, s.st);
}

double pairwise_sum(const double *v, size_t count) { // at most 1024 summands serially into one accumulator
    if (count <= 1024) {
        double s = 0.0;
        for (size_t i = 0; i < count; ++i) s += v[i];
        return s;
    }
    return pairwise_sum(v, count / 2) + pairwise_sum(v + count / 2, count - count / 2);
}

} // namespace

extern "C" int gml_model_elim_plan(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                   const int32_t *order, int32_t *order_out, int32_t *width, double *work, double *stored) {
    if (int rc = check_model_args(keys, key_stride, weights, nterms, n)) return rc;
    ElimOrder P;
    if (int rc = plan_order(keys, key_stride, weights, nterms, n, order, P)) return rc;
    if (order_out) std::copy(P.seq.begin(), P.seq.end(), order_out);
    if (width) *width = P.width;
    if (work) *work = P.work;
    if (stored) *stored = P.stored;
    return GML_OK;
}

extern "C" int gml_model_elim(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, const int32_t *order,
                              int device, double *log_z, double *mean, double *texp) {
    if (!log_z) return fail(GML_EINVAL, "log_z is NULL");
    if (int rc = check_model_args(keys, key_stride, weights, nterms, n)) return rc;
    ElimOrder P;
    if (int rc = plan_order(keys, key_stride, weights, nterms, n, order, P)) return rc;
    const bool moments = mean || texp;
    if (P.width > GML_ELIM_MAX_WIDTH)
        return fail(GML_EUNSUPPORTED, "the elimination order has width %d: variable elimination is limited to %d", P.width, GML_ELIM_MAX_WIDTH);
    if (moments && P.stored > std::ldexp(1.0, 32))
        return fail(GML_EUNSUPPORTED, "the moments need %.3g forward table entries: at most 2^32 (32 GiB) are stored", P.stored);
    // a spin in no term needs no device: ln 2, mean 0
    std::vector<Component> comps;
    std::vector<int> free_spins, sp;
    std::vector<double> parts;
    plan_components(P, keys, key_stride, weights, nterms, n, comps, free_spins, parts);
    const int64_t nfree = (int64_t)free_spins.size();
    if (int rc = gml_check_device(device)) return rc;
    std::vector<double> m((size_t)n, 0.0);
    if (texp)
        for (int64_t t = 0; t < nterms; ++t) texp[t] = std::numeric_limits<double>::quiet_NaN();
    if (int rc = run_components(comps, moments, device)) return rc;
    for (Component &C : comps) {
        parts.push_back(C.log_z);
        if (!moments) continue;
        for (size_t q = 0; q < C.q_term.size(); ++q) {
            if (C.q_term[q] < 0) m[(size_t)~C.q_term[q]] = C.res[q];
            else if (texp) texp[C.q_term[q]] = C.res[q];
        }
    }
    parts.push_back((double)nfree * std::log(2.0));
    *log_z = pairwise_sum(parts.data(), parts.size());
    if (mean) std::copy(m.begin(), m.end(), mean);
    if (texp)
        for (int64_t t = 0; t < nterms; ++t) { // what the recursion does not see: empty keys, and zero weights of at most one spin
            reduce_key(keys + t * key_stride, key_stride, sp);
            if (sp.empty()) texp[t] = 1.0;
            else if (weights[t] == 0.0 && sp.size() == 1) texp[t] = m[(size_t)sp[0]];
        }
    return GML_OK;
}

extern "C" int gml_problem_create_sampled_elim(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, int64_t N,
                                               uint64_t seed, const int32_t *order, int histogram, int porder, int64_t node0, int64_t node1,
                                               int device, gml_problem **out) {
    if (int rc = check_out(out)) return rc;
    if (int rc = check_model_args(keys, key_stride, weights, nterms, n)) return rc;
    if (int rc = gml_check_handle_args(n, porder, node0, node1)) return rc;
    if (N < 1 || N > (int64_t)1 << 40) return fail(GML_EINVAL, "N must lie in [1, 2^40] (given %lld)", (long long)N);
    ElimOrder P;
    if (int rc = plan_order(keys, key_stride, weights, nterms, n, order, P)) return rc;
    if (P.width > GML_ELIM_MAX_WIDTH)
        return fail(GML_EUNSUPPORTED, "the elimination order has width %d: variable elimination is limited to %d", P.width, GML_ELIM_MAX_WIDTH);
    const double kept = P.stored + entries_between_launches(P);
    if (kept > std::ldexp(1.0, 32))
        return fail(GML_EUNSUPPORTED, "the draws need %.3g kept table entries: at most 2^32 (32 GiB) are stored", kept);
    if (n > 16384) return fail(GML_EUNSUPPORTED, "the draws by elimination support n <= 16384 spins (n = %lld)", (long long)n);
    if (histogram)
        if (int rc = check_hist_limits(n, N)) return rc;
    std::vector<Component> comps;
    std::vector<int> free_spins;
    std::vector<double> constants; // (the empty keys: no part of a draw)
    plan_components(P, keys, key_stride, weights, nterms, n, comps, free_spins, constants);
    if (int rc = gml_check_device(device)) return rc;
    const int64_t ld = gml_round_up(N, 256);
    Uploaded U;
    SamplerStaging s;
    if (int rc = s.begin(device, N, n, porder, node0, node1, (size_t)n * (size_t)ld, true)) return rc;
    draw_components(s, comps, U, free_spins, seed, N, ld);
    return s.finish(true, ld, histogram != 0, out);
}
