// libgml_hip, host side: exact conditional inference (gml_conditional_exact, gml_conditional_exact_masked; gml_cond_exact.hip,
// DESIGN 3.19).  The argument checks in the order of the conditional chains (gml_chains_host.cpp), the model's terms reduced once,
// one plan per distinct hidden set (the terms sorted by hidden part, items, partial sums, the coefficients in the order of their
// chunk masks), plans and jobs uploaded in slabs, one launch and one synchronisation per slab.  The per-row form reads the hidden
// sets from the mask handle's sign bits, groups the rows by identical set and plans a set exactly as the uniform form plans its one:
// a mask whose rows are all equal therefore gives the uniform form's bits.  gml_conditional_mode and gml_conditional_mode_masked (every
// row's most probable hidden state) are the same two paths with other outputs (CondOutputs) and the kernel's mode forms;
// gml_conditional_draw and gml_conditional_draw_masked (exact draws of every row's hidden spins) are the mode calls with
// `replicas` chains per row and the kernel's draw forms: a plan per distinct hidden set as before, a job per kCondDrawBatch replicas.
#include "gml_sampled.h"

#include <map>
#include <numeric>

using namespace gml;

namespace {

constexpr size_t kCondSlabBytes = (size_t)64 << 20; // plans uploaded together
constexpr size_t kCondSlabPlans = 4096;

// the model's terms of non-zero weight after cancellation, in the caller's order: term t names sp[off[t] .. off[t + 1])
struct ReducedTerms {
    std::vector<size_t> off{0};
    std::vector<int> sp;
    std::vector<double> w;
    size_t size() const { return w.size(); }
};
int reduce_terms(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, ReducedTerms &R) {
    std::vector<int> sp;
    for (int64_t t = 0; t < nterms; ++t) {
        if (weights[t] == 0.0) continue;
        reduce_key(keys + t * key_stride, key_stride, sp);
        if (sp.size() > (size_t)kCondMaxTermSpins)
            return fail(GML_EUNSUPPORTED, "term %lld names %zu distinct spins: exact conditional inference supports at most %d", (long long)t,
                        sp.size(), kCondMaxTermSpins);
        R.sp.insert(R.sp.end(), sp.begin(), sp.end());
        R.off.push_back(R.sp.size());
        R.w.push_back(weights[t]);
    }
    return GML_OK;
}

// One hidden set as the kernel takes it (gml_dev.h: CondExactPlan).
struct CondPattern {
    std::vector<int> hid;
    int c = 0, S = 1;
    std::vector<double> w;
    std::vector<unsigned short> vis, chi;
    std::vector<int> item_off, item_dst, ms_off, ms_dst, run_off, run_dst;
};
// loc [n]: -1 everywhere, on entry and on return.  Cost: one pass over the terms' spins, one stable sort of the T terms.
int plan_pattern(const ReducedTerms &R, const std::vector<int> &hid, std::vector<int> &loc, CondPattern &pc) {
    const size_t T = R.size();
    const int h = (int)hid.size();
    pc.hid = hid;
    for (int j = 0; j < h; ++j) loc[(size_t)hid[(size_t)j]] = j;
    std::vector<unsigned> mask(T);
    size_t maxvis = 0;
    for (size_t t = 0; t < T; ++t) {
        unsigned m = 0;
        size_t nv = 0;
        for (size_t a = R.off[t]; a < R.off[t + 1]; ++a) {
            const int l = loc[(size_t)R.sp[a]];
            if (l >= 0) m |= 1u << l;
            else ++nv;
        }
        mask[t] = m;
        maxvis = std::max(maxvis, nv);
    }
    pc.S = maxvis <= 1 ? 1 : maxvis <= 2 ? 2 : maxvis <= 4 ? 4 : 8;
    std::vector<int> idx(T);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return mask[(size_t)a] < mask[(size_t)b]; });
    pc.w.resize(T);
    pc.vis.assign(T * (size_t)pc.S, kCondNoSpin);
    for (size_t t = 0; t < T; ++t) {
        const size_t src = (size_t)idx[t];
        pc.w[t] = R.w[src];
        size_t at = t * (size_t)pc.S;
        for (size_t a = R.off[src]; a < R.off[src + 1]; ++a)
            if (loc[(size_t)R.sp[a]] < 0) pc.vis[at++] = (unsigned short)R.sp[a];
    }
    for (int j = 0; j < h; ++j) loc[(size_t)hid[(size_t)j]] = -1;
    // the distinct hidden parts, ascending: part d is the terms [pstart[d], pstart[d + 1]) of the sorted list
    std::vector<unsigned> pm;
    std::vector<size_t> pstart;
    for (size_t t = 0; t < T; ++t)
        if (t == 0 || mask[(size_t)idx[t]] != mask[(size_t)idx[t - 1]]) {
            pm.push_back(mask[(size_t)idx[t]]);
            pstart.push_back(t);
        }
    pstart.push_back(T);
    const size_t D = pm.size();
    if (D > (size_t)kCondCoefs)
        return fail(GML_EUNSUPPORTED, "the terms have %zu distinct hidden parts under one hidden set: exact conditional inference supports at "
                                      "most %d", D, kCondCoefs);
    pc.c = std::min(h, g_exact_chunk_bits > 0 ? g_exact_chunk_bits : kExactChunkBits);
    pc.c = std::max(pc.c, h - kCondMaxHigh); // (a hooked c: at most 4096 chunks per row)
    const unsigned low = (1u << pc.c) - 1u;
    // the coefficients in the order of their low masks (stable: ascending high part within one)
    std::vector<int> ord(D), pos(D);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return (pm[(size_t)a] & low) < (pm[(size_t)b] & low); });
    pc.chi.resize(D);
    pc.run_off.clear();
    pc.run_dst.clear();
    for (size_t i = 0; i < D; ++i) {
        const unsigned m = pm[(size_t)ord[i]];
        pos[(size_t)ord[i]] = (int)i;
        pc.chi[i] = (unsigned short)(m >> pc.c);
        if (i == 0 || (m & low) != (pm[(size_t)ord[i - 1]] & low)) {
            pc.run_off.push_back((int)i);
            pc.run_dst.push_back((int)((m & low) + ((m & low) >> 4)));
        }
    }
    pc.run_off.push_back((int)D);
    // items of at most L terms; L doubles until the partial sums of the parts with several items fit kCondParts
    for (int L = 16;; L *= 2) {
        pc.item_off.assign(1, 0);
        pc.item_dst.clear();
        pc.ms_off.assign(1, 0);
        pc.ms_dst.clear();
        int parts = 0;
        for (size_t d = 0; d < D; ++d) {
            const size_t a = pstart[d], b = pstart[d + 1];
            const int nseg = (int)((b - a + (size_t)L - 1) / (size_t)L);
            for (int s = 0; s < nseg; ++s) {
                pc.item_off.push_back((int)std::min(b, a + (size_t)(s + 1) * (size_t)L));
                pc.item_dst.push_back(nseg == 1 ? pos[d] : ~(parts + s));
            }
            if (nseg > 1) {
                parts += nseg;
                pc.ms_off.push_back(parts);
                pc.ms_dst.push_back(pos[d]);
            }
        }
        if (parts <= kCondParts) break;
        if (L >= 1024)
            return fail(GML_EUNSUPPORTED, "too many terms share their hidden parts under one hidden set: exact conditional inference sums at "
                                          "most %d items of 1024 terms into the coefficients of a row", kCondParts);
    }
    return GML_OK;
}

// Plans and jobs that go to the device together: the plans' arrays in one pool per element type
struct Slab {
    struct Where {
        size_t w, vis, chi, item_off, item_dst, ms_off, ms_dst, run_off, run_dst;
        CondExactPlan p;
    };
    std::vector<double> w;
    std::vector<unsigned short> u16;
    std::vector<int> i32;
    std::vector<Where> plans;
    std::vector<CondExactJob> jobs;

    template <class T> static size_t put(std::vector<T> &pool, const std::vector<T> &v) {
        const size_t at = pool.size();
        pool.insert(pool.end(), v.begin(), v.end());
        if (v.empty()) pool.push_back(T{}); // (no empty upload, and every plan's pointers are valid)
        return at;
    }
    size_t bytes() const { return sizeof(double) * w.size() + sizeof(unsigned short) * u16.size() + sizeof(int) * i32.size(); }
    int add(const CondPattern &pc) {
        Where wh{};
        wh.w = put(w, pc.w);
        u16.resize((u16.size() + 7) / 8 * 8);
        wh.vis = put(u16, pc.vis);
        wh.chi = put(u16, pc.chi);
        wh.item_off = put(i32, pc.item_off);
        wh.item_dst = put(i32, pc.item_dst);
        wh.ms_off = put(i32, pc.ms_off);
        wh.ms_dst = put(i32, pc.ms_dst);
        wh.run_off = put(i32, pc.run_off);
        wh.run_dst = put(i32, pc.run_dst);
        CondExactPlan &p = wh.p;
        for (size_t j = 0; j < pc.hid.size(); ++j) p.hid[j] = pc.hid[j];
        p.S = pc.S;
        p.ni = (int)pc.item_dst.size();
        p.nm = (int)pc.ms_dst.size();
        p.nc = (int)pc.chi.size();
        p.ns = (int)pc.run_dst.size();
        p.h = (int)pc.hid.size();
        p.c = pc.c;
        plans.push_back(wh);
        return (int)plans.size() - 1;
    }
    void clear() {
        w.clear();
        u16.clear();
        i32.clear();
        plans.clear();
        jobs.clear();
    }
};

// what a call asks for (host pointers, any but the first of a family NULL): the sums of gml_conditional_exact[_masked] -- means, log_w,
// log_p -- or, with mode set, the most probable hidden state of every row of gml_conditional_mode[_masked] -- states, energy, log_p --
// or, with draw set as well, `replicas` exact draws per row with the same three outputs per chain (gml_conditional_draw[_masked])
struct CondOutputs {
    bool mode = false, draw = false;
    int replicas = 1;
    uint64_t seed = 0;
    double *means = nullptr, *log_w = nullptr;
    int8_t *states = nullptr;
    double *energy = nullptr;
    double *log_p = nullptr;
    bool per_spin() const { return mode ? states != nullptr : means != nullptr; }
};

// the device side of one call: the stream, the outputs [hmax][C], [C], [C] (those asked for; C = K chains, K replicas for the draws)
// and the slabs
struct CondExactRun {
    SamplerStaging s;
    const unsigned *dSb = nullptr;
    int64_t wpr = 0, n = 0, K = 0, C = 0;
    int replicas = 1; // (of the draws; a job takes kCondDrawBatch of a row's)
    uint64_t seed = 0;
    bool draw = false;
    double *dmeans = nullptr, *dlw = nullptr, *dlp = nullptr, *den = nullptr;
    int8_t *dstates = nullptr;
    bool mode = false;

    int open(gml_problem *evidence, gml_problem *mask) {
        if (s.open(evidence->device)) return s.rc;
        s.ok(hipStreamSynchronize(evidence->st), "hipStreamSynchronize");
        if (mask) s.ok(hipStreamSynchronize(mask->st), "hipStreamSynchronize");
        dSb = evidence->d.Sb;
        wpr = evidence->d.Kp / 32;
        n = evidence->n;
        K = evidence->K;
        return s.rc;
    }
    int outputs(size_t hmax, const CondOutputs &o) {
        mode = o.mode;
        draw = o.draw;
        replicas = o.replicas;
        seed = o.seed;
        C = K * replicas;
        if (o.means) dmeans = s.alloc<double>(std::max<size_t>(hmax, 1) * (size_t)C);
        if (o.states) dstates = s.alloc<int8_t>(std::max<size_t>(hmax, 1) * (size_t)C);
        if (o.log_w) dlw = s.alloc<double>((size_t)C);
        if (o.energy) den = s.alloc<double>((size_t)C);
        if (o.log_p) dlp = s.alloc<double>((size_t)C);
        return s.rc;
    }
    // the jobs of row k under a plan: one, or one per kCondDrawBatch replicas
    void add_jobs(Slab &sl, int64_t k, int plan) const {
        for (int r = 0; r < replicas; r += kCondDrawBatch) sl.jobs.push_back(CondExactJob{(long long)k, plan, r});
    }
    // upload, launch, drain, free: one synchronisation per slab
    int flush(Slab &sl) {
        if (sl.jobs.empty()) return s.rc;
        const double t0 = gml_now_s();
        const size_t mark = s.tmp.size();
        const double *dw = s.upload(sl.w);
        const unsigned short *du = s.upload(sl.u16);
        const int *di = s.upload(sl.i32);
        if (s.rc) return s.rc;
        std::vector<CondExactPlan> plans;
        for (const Slab::Where &wh : sl.plans) {
            CondExactPlan p = wh.p;
            p.w = dw + wh.w;
            p.vis = du + wh.vis;
            p.chi = du + wh.chi;
            p.item_off = di + wh.item_off;
            p.item_dst = di + wh.item_dst;
            p.ms_off = di + wh.ms_off;
            p.ms_dst = di + wh.ms_dst;
            p.run_off = di + wh.run_off;
            p.run_dst = di + wh.run_dst;
            plans.push_back(p);
        }
        const CondExactPlan *dplans = s.upload(plans);
        const CondExactJob *djobs = s.upload(sl.jobs);
        if (s.rc) return s.rc;
        if (draw) launch_cond_draw(dplans, djobs, (int64_t)sl.jobs.size(), dSb, wpr, n, K, replicas, seed, dstates, den, dlp, s.st);
        else if (mode) launch_cond_mode(dplans, djobs, (int64_t)sl.jobs.size(), dSb, wpr, n, dstates, K, den, dlp, s.st);
        else launch_cond_exact(dplans, djobs, (int64_t)sl.jobs.size(), dSb, wpr, n, dmeans, K, dlw, dlp, s.st);
        if (s.sync()) return s.rc;
        for (size_t i = mark; i < s.tmp.size(); ++i) (void)dev_free(s.tmp[i]);
        s.tmp.resize(mark);
        sl.clear();
        g_cond_exact_times[1] += gml_now_s() - t0;
        return s.rc;
    }
    template <class T> void download(T *dst, const T *src, size_t count) {
        if (dst && count) s.ok(hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyDeviceToHost, s.st), "hipMemcpyAsync");
    }
};

// what both entry points check alike before the model's values, in the order of check_conditional_args (gml_chains_host.cpp)
int check_cond_exact_args(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, const gml_problem *evidence,
                          const void *second, const char *second_name, const gml_problem *rowmask, const CondOutputs &o) {
    if (o.mode && !o.states) return fail(GML_EINVAL, "states is NULL");
    if (o.replicas < 1) return fail(GML_EINVAL, "replicas = %d: at least 1", o.replicas);
    if (!o.mode && !o.means && !o.log_w && !o.log_p) return fail(GML_EINVAL, "means, log_w and log_p are all NULL");
    if (!evidence) return fail(GML_EINVAL, "evidence is NULL");
    if (!second) return fail(GML_EINVAL, "%s is NULL", second_name);
    if (int rc = check_term_pointers(keys, key_stride, weights, nterms, true)) return rc;
    if (n != evidence->n) return fail(GML_EINVAL, "n = %lld differs from the evidence handle's %lld spins", (long long)n, (long long)evidence->n);
    if (rowmask && (rowmask->n != evidence->n || rowmask->K != evidence->K || rowmask->device != evidence->device))
        return fail(GML_EINVAL, "the mask handle (n = %lld, %lld rows, device %d) differs from the evidence handle (n = %lld, %lld rows, device %d)",
                    (long long)rowmask->n, (long long)rowmask->K, rowmask->device, (long long)evidence->n, (long long)evidence->K, evidence->device);
    return GML_OK;
}
int check_cond_exact_n(int64_t n) {
    if (n > kCondMaxN)
        return fail(GML_EUNSUPPORTED, "exact conditional inference supports n <= %lld spins (n = %lld)", (long long)kCondMaxN, (long long)n);
    return GML_OK;
}

// the times of one call into g_cond_exact_times (gml_dev.h; per thread): host = all - slabs - the final download
struct CondExactClock {
    double t0 = gml_now_s();
    CondExactClock() { g_cond_exact_times[0] = g_cond_exact_times[1] = g_cond_exact_times[2] = 0.0; }
    void before_download() { g_cond_exact_times[0] = gml_now_s() - t0 - g_cond_exact_times[1]; }
    ~CondExactClock() { g_cond_exact_times[2] = gml_now_s() - t0; }
};

// one hidden set for every row: gml_conditional_exact and gml_conditional_mode
int cond_uniform(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, gml_problem *evidence,
                 const uint8_t *hidden, const CondOutputs &o) {
    CondExactClock clock;
    if (int rc = check_cond_exact_args(keys, key_stride, weights, nterms, n, evidence, hidden, "hidden", nullptr, o)) return rc;
    std::vector<int> hid;
    for (int64_t i = 0; i < n; ++i)
        if (hidden[i]) hid.push_back((int)i);
    if (hid.empty()) return fail(GML_EINVAL, "no spin is hidden");
    if (int rc = check_term_values(keys, key_stride, weights, nterms, n)) return rc;
    if (int rc = check_cond_exact_n(n)) return rc;
    if (hid.size() > (size_t)kCondMaxHidden)
        return fail(GML_EUNSUPPORTED, "%zu spins are hidden: exact conditional inference enumerates at most %d hidden spins per row", hid.size(),
                    kCondMaxHidden);
    ReducedTerms R;
    if (int rc = reduce_terms(keys, key_stride, weights, nterms, R)) return rc;
    std::vector<int> loc((size_t)n, -1);
    CondPattern pc;
    if (int rc = plan_pattern(R, hid, loc, pc)) return rc;
    if (int rc = gml_check_device(evidence->device)) return rc;
    if (evidence->K == 0) return GML_OK; // (no row: nothing to enumerate)
    CondExactRun run;
    if (run.open(evidence, nullptr) || run.outputs(hid.size(), o)) return run.s.rc;
    Slab sl;
    const int plan = sl.add(pc);
    sl.jobs.reserve((size_t)run.K * (size_t)((o.replicas + kCondDrawBatch - 1) / kCondDrawBatch));
    for (int64_t k = 0; k < run.K; ++k) run.add_jobs(sl, k, plan);
    if (run.flush(sl)) return run.s.rc;
    clock.before_download();
    run.download(o.means, run.dmeans, hid.size() * (size_t)run.C);
    run.download(o.states, run.dstates, hid.size() * (size_t)run.C);
    run.download(o.log_w, run.dlw, (size_t)run.C);
    run.download(o.energy, run.den, (size_t)run.C);
    run.download(o.log_p, run.dlp, (size_t)run.C);
    return run.s.sync();
}

// a hidden set per row, read from the mask handle: gml_conditional_exact_masked and gml_conditional_mode_masked
int cond_masked(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, gml_problem *evidence,
                gml_problem *mask, const CondOutputs &o) {
    CondExactClock clock;
    if (int rc = check_cond_exact_args(keys, key_stride, weights, nterms, n, evidence, mask, "mask", mask, o)) return rc;
    const bool per_spin = o.per_spin();
    if (int rc = check_term_values(keys, key_stride, weights, nterms, n)) return rc;
    if (int rc = check_cond_exact_n(n)) return rc;
    ReducedTerms R;
    if (int rc = reduce_terms(keys, key_stride, weights, nterms, R)) return rc;
    if (int rc = gml_check_device(evidence->device)) return rc;
    if (evidence->K == 0) return GML_OK; // (no row: nothing to enumerate)
    CondExactRun run;
    if (run.open(evidence, mask)) return run.s.rc;
    const int64_t K = run.K;
    // the hidden sets: the mask's sign bits come down ([n][Kp / 32], bit k % 32 of word k / 32 <-> row k), and the evidence's with
    // them when the means (the states) are wanted (an observed entry holds its evidence value)
    const size_t mwpr = (size_t)(mask->d.Kp / 32), ewpr = (size_t)run.wpr;
    std::vector<unsigned> mb((size_t)n * mwpr), eb(per_spin ? (size_t)n * ewpr : 0);
    run.s.ok(hipMemcpyAsync(mb.data(), mask->d.Sb, sizeof(unsigned) * mb.size(), hipMemcpyDeviceToHost, run.s.st), "hipMemcpyAsync");
    if (per_spin) run.s.ok(hipMemcpyAsync(eb.data(), evidence->d.Sb, sizeof(unsigned) * eb.size(), hipMemcpyDeviceToHost, run.s.st), "hipMemcpyAsync");
    if (run.s.sync()) return run.s.rc;
    const size_t kwords = (size_t)((K + 31) / 32);
    auto for_holes = [&](const std::function<void(int64_t, int)> &fn) { // (row, spin) of every hole, the spins of a row ascending
        for (int64_t i = 0; i < n; ++i)
            for (size_t wd = 0; wd < kwords; ++wd)
                for (unsigned word = mb[(size_t)i * mwpr + wd]; word; word &= word - 1) {
                    const int64_t k = (int64_t)wd * 32 + __builtin_ctz(word);
                    if (k < K) fn(k, (int)i);
                }
    };
    std::vector<size_t> off((size_t)K + 1, 0);
    for_holes([&](int64_t k, int) { ++off[(size_t)k + 1]; });
    size_t hmax = 0;
    for (int64_t k = 0; k < K; ++k) {
        if (off[(size_t)k + 1] > (size_t)kCondMaxHidden)
            return fail(GML_EUNSUPPORTED, "row %lld hides %zu spins: exact conditional inference enumerates at most %d hidden spins per row",
                        (long long)k, off[(size_t)k + 1], kCondMaxHidden);
        hmax = std::max(hmax, off[(size_t)k + 1]);
        off[(size_t)k + 1] += off[(size_t)k];
    }
    std::vector<int> holes(off[(size_t)K]);
    {
        std::vector<size_t> at(off.begin(), off.end() - 1);
        for_holes([&](int64_t k, int i) { holes[at[(size_t)k]++] = i; });
    }
    // the rows grouped by identical hidden set, the sets in the order of their first rows
    std::map<std::vector<int>, size_t> seen;
    std::vector<std::pair<std::vector<int>, std::vector<int64_t>>> patterns;
    for (int64_t k = 0; k < K; ++k) {
        std::vector<int> hid(holes.begin() + (ptrdiff_t)off[(size_t)k], holes.begin() + (ptrdiff_t)off[(size_t)k + 1]);
        auto it = seen.find(hid);
        if (it == seen.end()) {
            it = seen.emplace(hid, patterns.size()).first;
            patterns.emplace_back(std::move(hid), std::vector<int64_t>());
        }
        patterns[it->second].second.push_back(k);
    }
    if (run.outputs(hmax, o)) return run.s.rc;
    std::vector<int> loc((size_t)n, -1);
    Slab sl;
    for (auto &pat : patterns) {
        CondPattern pc;
        if (int rc = plan_pattern(R, pat.first, loc, pc)) return rc;
        const int plan = sl.add(pc);
        for (int64_t k : pat.second) run.add_jobs(sl, k, plan);
        if (sl.bytes() >= kCondSlabBytes || sl.plans.size() >= kCondSlabPlans)
            if (run.flush(sl)) return run.s.rc;
    }
    if (run.flush(sl)) return run.s.rc;
    clock.before_download();
    const int64_t C = run.C;
    std::vector<double> hm(o.means ? std::max<size_t>(hmax, 1) * (size_t)C : 0);
    std::vector<int8_t> hs(o.states ? std::max<size_t>(hmax, 1) * (size_t)C : 0);
    run.download(o.means ? hm.data() : nullptr, run.dmeans, hm.size());
    run.download(o.states ? hs.data() : nullptr, run.dstates, hs.size());
    run.download(o.log_w, run.dlw, (size_t)C);
    run.download(o.energy, run.den, (size_t)C);
    run.download(o.log_p, run.dlp, (size_t)C);
    if (run.s.sync()) return run.s.rc;
    // [n][C], chain r K + k: the evidence values of row k, then its holes from the hidden-major results
    auto scatter = [&](auto *dst, const auto &src) {
        for (int64_t i = 0; i < n; ++i)
            for (int64_t r = 0; r < C; r += K)
                for (int64_t k = 0; k < K; ++k) dst[i * C + r + k] = ((eb[(size_t)i * ewpr + (size_t)(k >> 5)] >> (k & 31)) & 1u) ? -1 : 1;
        for (int64_t r = 0; r < C; r += K)
            for (int64_t k = 0; k < K; ++k)
                for (size_t a = off[(size_t)k]; a < off[(size_t)k + 1]; ++a)
                    dst[(int64_t)holes[a] * C + r + k] = src[(a - off[(size_t)k]) * (size_t)C + (size_t)(r + k)];
    };
    if (o.means) scatter(o.means, hm);
    if (o.states) scatter(o.states, hs);
    return GML_OK;
}

} // namespace

extern "C" int gml_conditional_exact(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                     gml_problem *evidence, const uint8_t *hidden, double *means, double *log_w, double *log_p) {
    CondOutputs o;
    o.means = means;
    o.log_w = log_w;
    o.log_p = log_p;
    return cond_uniform(keys, key_stride, weights, nterms, n, evidence, hidden, o);
}
extern "C" int gml_conditional_exact_masked(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                            gml_problem *evidence, gml_problem *mask, double *means, double *log_w, double *log_p) {
    CondOutputs o;
    o.means = means;
    o.log_w = log_w;
    o.log_p = log_p;
    return cond_masked(keys, key_stride, weights, nterms, n, evidence, mask, o);
}

// the most probable hidden state of every row (include/gml.h; the mode forms of k_cond_exact)
extern "C" int gml_conditional_mode(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                    gml_problem *evidence, const uint8_t *hidden, int8_t *states, double *energy, double *log_p) {
    CondOutputs o;
    o.mode = true;
    o.states = states;
    o.energy = energy;
    o.log_p = log_p;
    return cond_uniform(keys, key_stride, weights, nterms, n, evidence, hidden, o);
}
extern "C" int gml_conditional_mode_masked(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                           gml_problem *evidence, gml_problem *mask, int8_t *states, double *energy, double *log_p) {
    CondOutputs o;
    o.mode = true;
    o.states = states;
    o.energy = energy;
    o.log_p = log_p;
    return cond_masked(keys, key_stride, weights, nterms, n, evidence, mask, o);
}

// exact draws of every row's hidden spins (include/gml.h; the draw forms of k_cond_exact)
extern "C" int gml_conditional_draw(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                    gml_problem *evidence, const uint8_t *hidden, int replicas, uint64_t seed, int8_t *states,
                                    double *energy, double *log_p) {
    CondOutputs o;
    o.mode = o.draw = true;
    o.replicas = replicas;
    o.seed = seed;
    o.states = states;
    o.energy = energy;
    o.log_p = log_p;
    return cond_uniform(keys, key_stride, weights, nterms, n, evidence, hidden, o);
}
extern "C" int gml_conditional_draw_masked(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                           gml_problem *evidence, gml_problem *mask, int replicas, uint64_t seed, int8_t *states,
                                           double *energy, double *log_p) {
    CondOutputs o;
    o.mode = o.draw = true;
    o.replicas = replicas;
    o.seed = seed;
    o.states = states;
    o.energy = energy;
    o.log_p = log_p;
    return cond_masked(keys, key_stride, weights, nterms, n, evidence, mask, o);
}
