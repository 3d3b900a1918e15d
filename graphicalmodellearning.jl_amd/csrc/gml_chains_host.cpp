// libgml_hip, host side: the term-list chain family -- thinned chains, replica exchange, annealed importance sampling, conditional
// chains under a fixed mask and under a mask per row.  Every entry point makes its own argument checks, takes the model through
// TermChainModel (value check, limits, incidences, spin records, upload) and launches its kernel; what they share with the other
// samplers is gml_sampled.h.
#include "gml_sampled.h"

#include <algorithm>
#include <cmath>
#include <functional>

using namespace gml;

// The spin records of a term list.  The couplings of every spin are quantised: sigma_i = 2^(E - 38) with max_e |w_e| < 2^E over its
// incidences with other spins, q_e = rint(w_e / sigma_i), and the incidences grouped by arity into the record stream of TermChainSpin
// (gml_dev.h): per spin a_i, sigma_i, Q_i and the records (q_e 2^24 + j_1 as two words, then j_2 .. j_k).  The records are appended
// to rec.  keep (spin, its other spins), when given: a_i and sigma_i as always, but Q_i and the records cover only the incidences with
// other spins that it accepts (the start energy of gml_log_partition_ais, the record sets of the conditional chains).
using KeepIncidence = std::function<bool(int64_t, const std::vector<int> &)>;
static void build_spin_records(const Incidences &inc, std::vector<TermChainSpin> &spin, std::vector<unsigned> &rec,
                               const KeepIncidence &keep = nullptr) {
    const int64_t n = (int64_t)inc.size();
    spin.assign((size_t)n, TermChainSpin{});
    for (int64_t i = 0; i < n; ++i) {
        TermChainSpin &r = spin[(size_t)i];
        double a = 0.0, mx = 0.0;
        for (auto &e : inc[(size_t)i]) {
            if (e.second.empty()) a += e.first;
            else mx = std::max(mx, std::fabs(e.first));
        }
        int ex = 0;
        if (mx > 0) (void)std::frexp(mx, &ex);
        r.a = a;
        r.sig = std::ldexp(1.0, ex - 38);
        long long Q = 0;
        r.off[0] = (long long)rec.size();
        for (int k = 1; k <= kTermChainsMaxOthers; ++k) {
            for (auto &e : inc[(size_t)i]) {
                if (e.second.size() != (size_t)k) continue;
                if (keep && !keep(i, e.second)) continue;
                const long long q = (long long)std::nearbyint(std::ldexp(e.first, 38 - ex));
                Q += q;
                const unsigned long long P = ((unsigned long long)q << 24) | (unsigned long long)e.second[0];
                rec.push_back((unsigned)P);
                rec.push_back((unsigned)(P >> 32));
                for (int m = 1; m < k; ++m) rec.push_back((unsigned)e.second[(size_t)m]);
            }
            r.off[k] = (long long)rec.size();
        }
        r.Q = Q;
    }
    if (rec.empty()) rec.push_back(0u);
}

// the term-chain kernels' limits: distinct spins per term, incidences with other spins per spin
static int check_term_chain_limits(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n) {
    std::vector<int64_t> cnt((size_t)n, 0);
    std::vector<int> sp;
    for (int64_t t = 0; t < nterms; ++t) {
        if (weights[t] == 0.0) continue;
        reduce_key(keys + t * key_stride, key_stride, sp);
        if (sp.size() > (size_t)kTermChainsMaxOthers + 1)
            return fail(GML_EUNSUPPORTED, "term %lld names %zu distinct spins: the term-list chain kernel supports at most %d",
                        (long long)t, sp.size(), kTermChainsMaxOthers + 1);
        if (sp.size() > 1)
            for (int v : sp)
                if (++cnt[(size_t)v] >= ((int64_t)1 << 24))
                    return fail(GML_EUNSUPPORTED, "spin %d has 2^24 or more incidences with other spins: the term-list chain kernel "
                                                  "supports fewer than 2^24", v);
    }
    return GML_OK;
}

// Everything a term-list chain kernel needs from (keys, stride, weights, nterms, n) for a run of `lanes` lanes: two checks, then one
// record stream with up to two sets of spin records into it, then upload.
struct TermChainModel {
    Incidences inc;
    std::vector<unsigned> rec;
    std::vector<TermChainSpin> spin, spin2; // spin2: a second set into the same stream (AIS: the start energy; conditional: the
                                            // constant part of the field), empty when there is none
    const TermChainSpin *dspin = nullptr, *dspin2 = nullptr;
    const unsigned *drec = nullptr;

    // The refusals every entry point makes after its own arguments come in two steps, because three entry points have always reported
    // a limit of their own between them (the histogram, the masked tile).  First the term values, then n against the kernels' limit
    // and the chain tile.
    static int check_values_and_n(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, int64_t lanes) {
        if (int rc = check_term_values(keys, key_stride, weights, nterms, n)) return rc;
        if (n > kMcmcChainsMaxN || term_chains_tile(n, lanes) == 0)
            return fail(GML_EUNSUPPORTED, "the term-list chain kernel supports n <= %lld spins (n = %lld)", (long long)kMcmcChainsMaxN,
                        (long long)n);
        return GML_OK;
    }
    // Second the incidence limits; then the incidences.
    int check_incidences_and_build(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n) {
        if (int rc = check_term_chain_limits(keys, key_stride, weights, nterms, n)) return rc;
        inc = build_incidences(keys, key_stride, weights, nterms, n);
        return GML_OK;
    }
    // one more set of spin records (over the incidences keep accepts), its records appended to the stream
    std::vector<TermChainSpin> records(const KeepIncidence &keep = nullptr) {
        std::vector<TermChainSpin> s;
        build_spin_records(inc, s, rec, keep);
        return s;
    }
    void upload(SamplerStaging &s) {
        dspin = s.upload(spin);
        dspin2 = spin2.empty() ? nullptr : s.upload(spin2);
        drec = s.upload(rec);
    }
};

// gml_problem_create_mcmc_terms_chains: thinned Glauber chains of any term list with exact integer fields (gml_term_chains.hip).
extern "C" int gml_problem_create_mcmc_terms_chains(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                                    int64_t chains, int64_t samples_per_chain, int burn_in, int thin, uint64_t seed,
                                                    int histogram, int order, int64_t node0, int64_t node1, int device, gml_problem **out) {
    if (int rc = check_out(out)) return rc;
    if (int rc = check_term_pointers(keys, key_stride, weights, nterms, true)) return rc;
    if (int rc = check_chain_args(n, chains, samples_per_chain, burn_in, thin, order, node0, node1)) return rc;
    const int64_t M = chains * samples_per_chain, ld = gml_round_up(M, 256);
    if (int rc = TermChainModel::check_values_and_n(keys, key_stride, weights, nterms, n, chains)) return rc;
    if (histogram)
        if (int rc = check_hist_limits(n, M)) return rc;
    TermChainModel m;
    if (int rc = m.check_incidences_and_build(keys, key_stride, weights, nterms, n)) return rc;
    m.spin = m.records();
    if (int rc = gml_check_device(device)) return rc;
    SamplerStaging s;
    if (int rc = s.begin(device, M, n, order, node0, node1, (size_t)n * ld, true)) return rc;
    m.upload(s);
    if (s.rc) return s.rc;
    launch_term_chains(m.dspin, m.drec, n, chains, burn_in, thin, (int)samples_per_chain, (unsigned long long)seed, s.out, ld, s.st);
    return s.finish(true, ld, histogram != 0, out); // the recorded states, spin-major
}

// the ladder of gml_problem_create_mcmc_terms_tempered: a power of two of rungs up to 64, finite betas that do not increase, the first positive
static int check_ladder(const double *betas, int replicas, int swap_every, int64_t ladders) {
    if (!betas) return fail(GML_EINVAL, "betas is NULL");
    if (replicas < 1 || replicas > 64 || (replicas & (replicas - 1)) != 0)
        return fail(GML_EINVAL, "replicas must be one of 1, 2, 4, 8, 16, 32, 64 (given %d)", replicas);
    for (int r = 0; r < replicas; ++r) {
        if (!std::isfinite(betas[r]) || betas[r] < 0.0) return fail(GML_EINVAL, "betas[%d] is negative or not finite", r);
        if (r > 0 && betas[r] > betas[r - 1]) return fail(GML_EINVAL, "betas must not increase (betas[%d] > betas[%d])", r, r - 1);
    }
    if (!(betas[0] > 0.0)) return fail(GML_EINVAL, "betas[0] must be positive");
    if (swap_every < 1) return fail(GML_EINVAL, "swap_every must be at least 1");
    if (ladders > ((int64_t)1 << 40) / replicas) return fail(GML_EINVAL, "ladders * replicas is too large");
    return GML_OK;
}

// gml_problem_create_mcmc_terms_tempered: replica-exchange chains of any term list, rung 0 recorded (gml_tempered_chains.hip).
extern "C" int gml_problem_create_mcmc_terms_tempered(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                                      int64_t ladders, int64_t samples_per_chain, int burn_in, int thin,
                                                      const double *betas, int replicas, int swap_every, uint64_t seed, int histogram,
                                                      int order, int64_t node0, int64_t node1, int device, int64_t *swap_counts,
                                                      gml_problem **out) {
    if (int rc = check_out(out)) return rc;
    if (int rc = check_term_pointers(keys, key_stride, weights, nterms, true)) return rc;
    if (int rc = check_chain_args(n, ladders, samples_per_chain, burn_in, thin, order, node0, node1)) return rc;
    if (int rc = check_ladder(betas, replicas, swap_every, ladders)) return rc;
    const int64_t M = ladders * samples_per_chain, ld = gml_round_up(M, 256);
    if (int rc = TermChainModel::check_values_and_n(keys, key_stride, weights, nterms, n, ladders * replicas)) return rc;
    if (histogram)
        if (int rc = check_hist_limits(n, M)) return rc;
    TermChainModel m;
    if (int rc = m.check_incidences_and_build(keys, key_stride, weights, nterms, n)) return rc;
    m.spin = m.records();
    if (int rc = gml_check_device(device)) return rc;
    const size_t ncounts = 2 * (size_t)(replicas - 1);
    std::vector<unsigned long long> counts(std::max<size_t>(ncounts, 1), 0ull);
    const std::vector<double> ladder(betas, betas + replicas);
    SamplerStaging s;
    if (int rc = s.begin(device, M, n, order, node0, node1, (size_t)n * ld, true)) return rc;
    m.upload(s);
    const double *dbetas = s.upload(ladder);
    unsigned long long *dcounts = s.upload(counts); // zeros
    if (s.rc) return s.rc;
    launch_tempered_chains(m.dspin, m.drec, n, ladders, replicas, dbetas, swap_every, burn_in, thin, (int)samples_per_chain,
                           (unsigned long long)seed, s.out, ld, dcounts, s.st);
    s.ok(hipMemcpyAsync(counts.data(), dcounts, sizeof(unsigned long long) * counts.size(), hipMemcpyDeviceToHost, s.st), "hipMemcpyAsync");
    if (int rc = s.finish(true, ld, histogram != 0, out)) return rc; // the recorded states of rung 0, spin-major
    if (swap_counts)
        for (size_t k = 0; k < ncounts; ++k) swap_counts[k] = (int64_t)counts[k];
    return GML_OK;
}

// the schedule of gml_log_partition_ais: at least two finite betas >= 0, the first 0; a sweep count that fits the chains' counter
static int check_schedule(const double *betas, int64_t nbetas, int sweeps_per_step) {
    if (!betas) return fail(GML_EINVAL, "betas is NULL");
    if (nbetas < 2) return fail(GML_EINVAL, "nbetas must be at least 2 (given %lld)", (long long)nbetas);
    if (sweeps_per_step < 1) return fail(GML_EINVAL, "sweeps_per_step must be at least 1");
    if (nbetas - 1 > (int64_t)INT32_MAX / sweeps_per_step) return fail(GML_EINVAL, "(nbetas - 1) * sweeps_per_step exceeds 2^31 - 1 sweeps");
    for (int64_t t = 0; t < nbetas; ++t)
        if (!std::isfinite(betas[t]) || betas[t] < 0.0) return fail(GML_EINVAL, "betas[%lld] is negative or not finite", (long long)t);
    if (betas[0] != 0.0) return fail(GML_EINVAL, "betas[0] must be 0 (the chains start from an exact draw at beta = 0)");
    return GML_OK;
}

// gml_log_partition_ais: annealed importance sampling of any term list (gml_ais_chains.hip); the estimate itself on the host.
extern "C" int gml_log_partition_ais(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, int64_t chains,
                                     const double *betas, int64_t nbetas, int sweeps_per_step, uint64_t seed, int device,
                                     double *log_weights, double *energies, int8_t *spins, double *result) {
    if (!log_weights) return fail(GML_EINVAL, "log_weights is NULL");
    if (int rc = check_term_pointers(keys, key_stride, weights, nterms, true)) return rc;
    if (n <= 0) return fail(GML_EINVAL, "n must be positive");
    if (chains < 1 || chains > (int64_t)1 << 31) return fail(GML_EINVAL, "chains must lie in [1, 2^31] (given %lld)", (long long)chains);
    if (int rc = check_schedule(betas, nbetas, sweeps_per_step)) return rc;
    if (int rc = TermChainModel::check_values_and_n(keys, key_stride, weights, nterms, n, chains)) return rc;
    TermChainModel m;
    if (int rc = m.check_incidences_and_build(keys, key_stride, weights, nterms, n)) return rc;
    // two sets of spin records: the fields, and every term once for the start energy -- at its smallest spin, so the incidences whose
    // other spins are all above i
    m.spin = m.records();
    m.spin2 = m.records([](int64_t i, const std::vector<int> &others) { return *std::min_element(others.begin(), others.end()) >= i; });
    if (int rc = gml_check_device(device)) return rc;
    const std::vector<double> schedule(betas, betas + nbetas);
    SamplerStaging s;
    if (int rc = s.open(device)) return rc;
    m.upload(s);
    const double *dbetas = s.upload(schedule);
    double *dlogw = s.alloc<double>((size_t)chains), *dE = energies ? s.alloc<double>((size_t)chains) : nullptr;
    int8_t *dstates = spins ? s.alloc<int8_t>((size_t)chains * (size_t)n) : nullptr;
    if (s.rc) return s.rc;
    launch_ais_chains(m.dspin, m.dspin2, m.drec, n, chains, dbetas, nbetas, sweeps_per_step, (unsigned long long)seed, dlogw, dE, dstates, s.st);
    s.ok(hipGetLastError(), "the sampler's launch");
    s.ok(hipMemcpyAsync(log_weights, dlogw, sizeof(double) * (size_t)chains, hipMemcpyDeviceToHost, s.st), "hipMemcpyAsync");
    if (energies) s.ok(hipMemcpyAsync(energies, dE, sizeof(double) * (size_t)chains, hipMemcpyDeviceToHost, s.st), "hipMemcpyAsync");
    if (spins) s.ok(hipMemcpyAsync(spins, dstates, (size_t)chains * (size_t)n, hipMemcpyDeviceToHost, s.st), "hipMemcpyAsync");
    if (s.sync()) return s.rc;
    if (result) {
        // log of the mean weight around the largest one, its delta-method standard error, the effective sample size; chain order
        double mx = log_weights[0];
        for (int64_t c = 1; c < chains; ++c) mx = std::max(mx, log_weights[c]);
        double s1 = 0.0, s2 = 0.0;
        for (int64_t c = 0; c < chains; ++c) {
            const double x = std::exp(log_weights[c] - mx);
            s1 += x;
            s2 += x * x;
        }
        const double mean = s1 / (double)chains;
        result[0] = (double)n * std::log(2.0) + mx + std::log(mean);
        result[1] = chains > 1 ? std::sqrt(std::max(s2 / (double)chains - mean * mean, 0.0) / (double)(chains - 1)) / mean : 0.0;
        result[2] = s1 * s1 / s2;
    }
    return GML_OK;
}

// ------------------------------------------------------------------------------------------
// The conditional chains: gml_problem_create_mcmc_terms_conditional and gml_conditional_means under one mask `hidden` [n]
// (gml_cond_chains.hip), the _masked pair under the rows of a mask handle (gml_masked_chains.hip).  In both bodies out != NULL makes
// the handle of the recorded states and means != NULL (host) receives the Rao-Blackwellised conditional means.
// ------------------------------------------------------------------------------------------
// What all four entry points check alike, in their order: the evidence, `second` (hidden or the mask handle, named in the text), the
// term pointers, n, the mask handle's shape (rowmask != NULL), replicas, the chain arguments.  *chains = K replicas.
static int check_conditional_args(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                  const gml_problem *evidence, const void *second, const char *second_name, const gml_problem *rowmask,
                                  int replicas, int64_t samples_per_chain, int burn_in, int thin, int order, int64_t node0, int64_t node1,
                                  int64_t *chains) {
    if (!evidence) return fail(GML_EINVAL, "evidence is NULL");
    if (!second) return fail(GML_EINVAL, "%s is NULL", second_name);
    if (int rc = check_term_pointers(keys, key_stride, weights, nterms, true)) return rc;
    if (n != evidence->n) return fail(GML_EINVAL, "n = %lld differs from the evidence handle's %lld spins", (long long)n, (long long)evidence->n);
    if (rowmask && (rowmask->n != evidence->n || rowmask->K != evidence->K || rowmask->device != evidence->device))
        return fail(GML_EINVAL, "the mask handle (n = %lld, %lld rows, device %d) differs from the evidence handle (n = %lld, %lld rows, device %d)",
                    (long long)rowmask->n, (long long)rowmask->K, rowmask->device, (long long)evidence->n, (long long)evidence->K, evidence->device);
    if (replicas < 1) return fail(GML_EINVAL, "replicas must be at least 1 (given %d)", replicas);
    if (evidence->K > ((int64_t)1 << 40) / replicas) return fail(GML_EINVAL, "the evidence handle's rows times replicas is too large");
    *chains = evidence->K * replicas;
    return check_chain_args(n, *chains, samples_per_chain, burn_in, thin, order, node0, node1);
}

// The device side of both bodies opens and ends alike.  Open: the handle under construction (out) or only a stream, ordered after
// whatever the caller last ran on the handles read.  End: the means come down, then sync without a handle or finish with one -- the
// recorded states spin-major, row (t, r, k) belonging to evidence row k, so no histogram.
static int conditional_begin(SamplerStaging &s, gml_problem *evidence, gml_problem *rowmask, int64_t M, int64_t n, int64_t ld, int order,
                             int64_t node0, int64_t node1, gml_problem **out) {
    if (out ? s.begin(evidence->device, M, n, order, node0, node1, (size_t)n * ld, true) : s.open(evidence->device)) return s.rc;
    s.ok(hipStreamSynchronize(evidence->st), "hipStreamSynchronize");
    if (rowmask) s.ok(hipStreamSynchronize(rowmask->st), "hipStreamSynchronize");
    return s.rc;
}
static int conditional_end(SamplerStaging &s, double *means, const double *dmeans, size_t nmeans, int64_t ld, gml_problem **out) {
    s.ok(hipGetLastError(), "the sampler's launch");
    if (means) s.ok(hipMemcpyAsync(means, dmeans, sizeof(double) * nmeans, hipMemcpyDeviceToHost, s.st), "hipMemcpyAsync");
    if (!out) return s.sync();
    return s.finish(true, ld, false, out);
}

// one mask for every row: means is [H][K replicas]
static int conditional_chains(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, gml_problem *evidence,
                              const uint8_t *hidden, int replicas, int64_t samples_per_chain, int burn_in, int thin, uint64_t seed, int order,
                              int64_t node0, int64_t node1, gml_problem **out, double *means) {
    int64_t chains = 0;
    if (int rc = check_conditional_args(keys, key_stride, weights, nterms, n, evidence, hidden, "hidden", nullptr, replicas, samples_per_chain,
                                        burn_in, thin, order, node0, node1, &chains))
        return rc;
    std::vector<int> hid;
    for (int64_t i = 0; i < n; ++i)
        if (hidden[i]) hid.push_back((int)i);
    if (hid.empty()) return fail(GML_EINVAL, "no spin is hidden");
    if (int rc = TermChainModel::check_values_and_n(keys, key_stride, weights, nterms, n, chains)) return rc;
    TermChainModel m;
    if (int rc = m.check_incidences_and_build(keys, key_stride, weights, nterms, n)) return rc;
    // one stream of records for the hidden spins: all their incidences, or (the constant part of the field) those whose other spins are
    // all visible and those with a hidden other spin as two sets.  The constant costs an update one 8-byte global load and saves it
    // the LDS reads of the const records: the split is taken when these average kCondSplitReads per hidden spin (measured: a
    // lattice with 3.5 loses 12 %, a sparse order-3 model with 21 gains 23 %, a dense model with 900 runs five times as fast;
    // g_cond_split = 2 takes it whenever there is a const record, 0 never).  The bits are the same either way.
    constexpr int64_t kCondSplitReads = 8;
    const int64_t H = (int64_t)hid.size();
    auto some_hidden = [&](const std::vector<int> &others) {
        return std::any_of(others.begin(), others.end(), [&](int j) { return hidden[j] != 0; });
    };
    auto of_hidden = [&](const std::vector<TermChainSpin> &all) { // the records of the hidden spins, ascending
        std::vector<TermChainSpin> sel;
        for (int i : hid) sel.push_back(all[(size_t)i]);
        return sel;
    };
    if (g_cond_split) {
        m.spin2 = of_hidden(m.records([&](int64_t i, const std::vector<int> &others) { return hidden[i] && !some_hidden(others); }));
        int64_t reads = 0; // other spins named by the const records
        for (const TermChainSpin &r : m.spin2)
            for (int k = 1; k <= kTermChainsMaxOthers; ++k) reads += (r.off[k] - r.off[k - 1]) / (k + 1) * k;
        if (reads == 0 || (g_cond_split != 2 && reads < kCondSplitReads * H)) m.spin2.clear(), m.rec.clear();
    }
    const bool split = !m.spin2.empty();
    m.spin = of_hidden(m.records([&](int64_t i, const std::vector<int> &others) { return hidden[i] && (!split || some_hidden(others)); }));
    const std::vector<uint8_t> mask(hidden, hidden + n);
    if (int rc = gml_check_device(evidence->device)) return rc;
    const int64_t M = chains * samples_per_chain, ld = gml_round_up(M, 256);
    SamplerStaging s;
    if (conditional_begin(s, evidence, nullptr, M, n, ld, order, node0, node1, out)) return s.rc;
    m.upload(s);
    const int *dhid = s.upload(hid);
    const uint8_t *dmask = s.upload(mask);
    long long *dcst = split ? s.alloc<long long>((size_t)H * (size_t)chains) : nullptr;
    const size_t nmeans = (size_t)H * (size_t)chains;
    double *dmeans = means ? s.alloc<double>(nmeans) : nullptr;
    if (dmeans) s.ok(hipMemsetAsync(dmeans, 0, sizeof(double) * nmeans, s.st), "hipMemsetAsync");
    if (s.rc) return s.rc;
    launch_cond_chains(m.dspin, m.dspin2, dhid, dmask, m.drec, evidence->d.Sb, evidence->d.Kp / 32, evidence->K, n, H, chains, burn_in, thin,
                       (int)samples_per_chain, (unsigned long long)seed, s.out, ld, dmeans, dcst, s.st);
    return conditional_end(s, means, dmeans, nmeans, ld, out);
}

// a mask per row, the sign bits of the handle `mask`: the spin records of k_term_chains over all incidences; means is [n][K replicas]
static int masked_chains(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, gml_problem *evidence,
                         gml_problem *mask, int replicas, int64_t samples_per_chain, int burn_in, int thin, uint64_t seed, int order,
                         int64_t node0, int64_t node1, gml_problem **out, double *means) {
    int64_t chains = 0;
    if (int rc = check_conditional_args(keys, key_stride, weights, nterms, n, evidence, mask, "mask", mask, replicas, samples_per_chain, burn_in,
                                        thin, order, node0, node1, &chains))
        return rc;
    if (int rc = TermChainModel::check_values_and_n(keys, key_stride, weights, nterms, n, chains)) return rc;
    if (masked_chains_tile(n, chains) == 0) // (state and mask words of 64 chains: twice the LDS of the other chain kernels)
        return fail(GML_EUNSUPPORTED, "the per-row masked chain kernel supports n <= %lld spins (n = %lld)",
                    (long long)(kMcmcChainsLds / (64 * 4 * 2) * 32), (long long)n);
    TermChainModel m;
    if (int rc = m.check_incidences_and_build(keys, key_stride, weights, nterms, n)) return rc;
    m.spin = m.records();
    if (int rc = gml_check_device(evidence->device)) return rc;
    const int64_t M = chains * samples_per_chain, ld = gml_round_up(M, 256);
    SamplerStaging s;
    if (conditional_begin(s, evidence, mask, M, n, ld, order, node0, node1, out)) return s.rc;
    m.upload(s);
    const size_t nmeans = (size_t)n * (size_t)chains;
    double *dmeans = means ? s.alloc<double>(nmeans) : nullptr; // (the kernel writes every entry)
    if (s.rc) return s.rc;
    launch_masked_chains(m.dspin, m.drec, evidence->d.Sb, evidence->d.Kp / 32, mask->d.Sb, mask->d.Kp / 32, evidence->K, n, chains, burn_in, thin,
                         (int)samples_per_chain, (unsigned long long)seed, s.out, ld, dmeans, s.st);
    return conditional_end(s, means, dmeans, nmeans, ld, out);
}

extern "C" int gml_problem_create_mcmc_terms_conditional(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                                         gml_problem *evidence, const uint8_t *hidden, int replicas,
                                                         int64_t samples_per_chain, int burn_in, int thin, uint64_t seed, int order,
                                                         int64_t node0, int64_t node1, gml_problem **out) {
    if (int rc = check_out(out)) return rc;
    return conditional_chains(keys, key_stride, weights, nterms, n, evidence, hidden, replicas, samples_per_chain, burn_in, thin, seed, order,
                              node0, node1, out, nullptr);
}

extern "C" int gml_conditional_means(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                     gml_problem *evidence, const uint8_t *hidden, int replicas, int64_t samples_per_chain, int burn_in,
                                     int thin, uint64_t seed, double *means) {
    if (!means) return fail(GML_EINVAL, "means is NULL");
    return conditional_chains(keys, key_stride, weights, nterms, n, evidence, hidden, replicas, samples_per_chain, burn_in, thin, seed, 2, 0, n,
                              nullptr, means);
}

extern "C" int gml_problem_create_mcmc_terms_masked(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                                    gml_problem *evidence, gml_problem *mask, int replicas, int64_t samples_per_chain,
                                                    int burn_in, int thin, uint64_t seed, int order, int64_t node0, int64_t node1,
                                                    gml_problem **out) {
    if (int rc = check_out(out)) return rc;
    return masked_chains(keys, key_stride, weights, nterms, n, evidence, mask, replicas, samples_per_chain, burn_in, thin, seed, order, node0,
                         node1, out, nullptr);
}

extern "C" int gml_conditional_means_masked(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                            gml_problem *evidence, gml_problem *mask, int replicas, int64_t samples_per_chain, int burn_in,
                                            int thin, uint64_t seed, double *means) {
    if (!means) return fail(GML_EINVAL, "means is NULL");
    return masked_chains(keys, key_stride, weights, nterms, n, evidence, mask, replicas, samples_per_chain, burn_in, thin, seed, 2, 0, n, nullptr,
                         means);
}
