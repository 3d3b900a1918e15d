// libgml_hip, host side: handles whose samples are drawn on the device -- the step before the path (src/sampling.jl:34-106):
// exact block sampling, Glauber chains of a term list (k_glauber) and of a dense pairwise model (the int8 chains), histogramming of
// the draws; the moments of a handle and exact enumeration of a model.  The term-list chain family is gml_chains_host.cpp.
#include "gml_sampled.h"
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

static int64_t round_up(int64_t a, int64_t b) { return gml_round_up(a, b); }

// ------------------------------------------------------------------------------------------
// Argument checks of the creators (those that gml_chains_host.cpp shares are declared, and described, in gml_sampled.h).
// ------------------------------------------------------------------------------------------
int gml::check_out(gml_problem **out) {
    if (!out) return fail(GML_EINVAL, "out is NULL");
    *out = nullptr;
    return GML_OK;
}

int gml::check_term_pointers(const int32_t *keys, int stride, const double *weights, int64_t nterms, bool strict) {
    const bool null = !keys || !weights;
    if (stride < 1 || (null && (strict || nterms > 0)) || (strict && nterms < 0)) return fail(GML_EINVAL, "NULL or malformed term list");
    return GML_OK;
}

int gml::check_term_values(const int32_t *keys, int stride, const double *weights, int64_t nterms, int64_t n) {
    for (int64_t t = 0; t < nterms; ++t) {
        if (!std::isfinite(weights[t])) return fail(GML_EINVAL, "weight of term %lld is not finite", (long long)t);
        for (int a = 0; a < stride; ++a) {
            const int32_t v = keys[t * stride + a];
            if (v < -1 || v >= n) return fail(GML_EINVAL, "term %lld names spin %d outside [0,%lld)", (long long)t, v, (long long)n);
        }
    }
    return GML_OK;
}

int gml::reduce_key(const int32_t *key, int stride, std::vector<int> &sp) {
    sp.clear();
    int named = -1;
    for (int a = 0; a < stride; ++a) {
        const int v = key[a];
        if (v < 0) continue;
        named = v;
        auto itv = std::find(sp.begin(), sp.end(), v);
        if (itv != sp.end()) sp.erase(itv);
        else sp.push_back(v);
    }
    return named;
}

int gml::check_chain_args(int64_t n, int64_t chains, int64_t samples_per_chain, int burn_in, int thin, int order, int64_t node0,
                          int64_t node1) {
    if (n <= 0) return fail(GML_EINVAL, "n must be positive");
    if (chains < 1 || samples_per_chain < 1 || burn_in < 1 || thin < 1)
        return fail(GML_EINVAL, "chains, samples_per_chain, burn_in and thin must be at least 1");
    if (int rc = gml_check_handle_args(n, order, node0, node1)) return rc;
    if (samples_per_chain > (int64_t)1 << 40 || chains > ((int64_t)1 << 40) / samples_per_chain)
        return fail(GML_EINVAL, "chains * samples_per_chain is too large");
    if ((int64_t)burn_in + (samples_per_chain - 1) * (int64_t)thin > INT32_MAX)
        return fail(GML_EINVAL, "burn_in + (samples_per_chain - 1) * thin exceeds 2^31 - 1 sweeps");
    return GML_OK;
}

static int check_hist_spins(int64_t n) {
    if (n > 64) return fail(GML_EUNSUPPORTED, "histogramming on the device needs n <= 64 spins (n = %lld)", (long long)n);
    return GML_OK;
}
int gml::check_hist_limits(int64_t n, int64_t M) {
    if (int rc = check_hist_spins(n)) return rc;
    if (M >= ((int64_t)1 << 31)) return fail(GML_EUNSUPPORTED, "histogramming on the device needs fewer than 2^31 samples");
    return GML_OK;
}

static int check_symmetric_finite(const double *model, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j <= i; ++j) {
            const double v = model[i * n + j];
            if (!std::isfinite(v)) return fail(GML_EINVAL, "the model matrix is not finite at (%lld,%lld)", (long long)i, (long long)j);
            if (v != model[j * n + i])
                return fail(GML_EINVAL, "the model matrix is not symmetric at (%lld,%lld)", (long long)i, (long long)j);
        }
    return GML_OK;
}

// Connected components of the term hypergraph (the exact sampler, gml_model_exact): blocks[b] = the spins of component b in
// ascending order, the components in the order of their smallest spin; id[i] = the component of spin i.
struct TermComponents {
    std::vector<std::vector<int>> blocks;
    std::vector<int64_t> id;
};
static TermComponents term_components(const int32_t *keys, int stride, const double *weights, int64_t nterms, int64_t n) {
    std::vector<int64_t> parent((size_t)n);
    for (int64_t i = 0; i < n; ++i) parent[i] = i;
    std::function<int64_t(int64_t)> find = [&](int64_t a) {
        while (parent[a] != a) a = parent[a] = parent[parent[a]];
        return a;
    };
    // (a term joins the spins that remain after cancellation: a spin named twice is not part of it)
    std::vector<int> sp;
    for (int64_t t = 0; t < nterms; ++t) {
        if (weights[t] == 0.0) continue;
        reduce_key(keys + t * stride, stride, sp);
        for (size_t a = 1; a < sp.size(); ++a) parent[find(sp[a])] = find(sp[0]);
    }
    TermComponents tc;
    std::vector<int64_t> of_root((size_t)n, -1);
    tc.id.assign((size_t)n, -1);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = find(i);
        if (of_root[r] < 0) {
            of_root[r] = (int64_t)tc.blocks.size();
            tc.blocks.emplace_back();
        }
        tc.id[(size_t)i] = of_root[r];
        tc.blocks[(size_t)of_root[r]].push_back((int)i);
    }
    return tc;
}

// ------------------------------------------------------------------------------------------
// gml_problem_create_sampled: sample on the device, then build the handle from the device-resident
// samples (the step before the path; src/sampling.jl:34-57, 94-106)
// ------------------------------------------------------------------------------------------
static int create_sampled_terms(const int32_t *keys, int stride, const double *weights, int64_t nterms, int64_t n,
                                int64_t N, uint64_t seed, int order, int64_t node0, int64_t node1, int device,
                                gml_problem **out, bool dedupe = false) {
    if (int rc = check_out(out)) return rc;
    if (int rc = check_term_pointers(keys, stride, weights, nterms)) return rc;
    if (n <= 0 || N <= 0) return fail(GML_EINVAL, "n and N must be positive");
    if (int rc = gml_check_handle_args(n, order, node0, node1)) return rc;
    if (int rc = check_term_values(keys, stride, weights, nterms, n)) return rc;
    const TermComponents tc = term_components(keys, stride, weights, nterms, n);
    const std::vector<std::vector<int>> &blocks = tc.blocks;
    std::vector<int> sp;
    size_t maxsb = 0;
    for (auto &b : blocks) maxsb = std::max(maxsb, b.size());
    if (maxsb > 22)
        return fail(GML_EUNSUPPORTED, "a connected component of the model has %zu spins: exact enumeration is limited to 22 "
                                     "(an MCMC sampler is not implemented)", maxsb);
    // per block: its terms as bit masks over the block's spins (a repeated spin cancels: s^2 = 1)
    std::vector<int> local((size_t)n, 0);
    for (auto &b : blocks)
        for (size_t i = 0; i < b.size(); ++i) local[(size_t)b[i]] = (int)i;
    std::vector<std::vector<unsigned>> bmask(blocks.size());
    std::vector<std::vector<double>> bwt(blocks.size());
    size_t maxnt = 1;
    for (int64_t t = 0; t < nterms; ++t) {
        if (weights[t] == 0.0) continue;
        reduce_key(keys + t * stride, stride, sp);
        if (sp.empty()) continue; // the empty term, or one whose spins all cancel: a constant energy
        unsigned mask = 0;
        for (int v : sp) mask |= 1u << local[(size_t)v];
        const size_t b = (size_t)tc.id[(size_t)sp[0]];
        bmask[b].push_back(mask);
        bwt[b].push_back(weights[t]);
        maxnt = std::max(maxnt, bmask[b].size());
    }
    if (int rc = gml_check_device(device)) return rc;
    SamplerStaging s;
    if (int rc = s.begin(device, N, n, order, node0, node1, (size_t)N * n, false)) return rc;
    double *dwt = s.alloc<double>(maxnt);
    unsigned *dmask = s.alloc<unsigned>(maxnt);
    double *den = s.alloc<double>((size_t)1 << maxsb), *dcdf = s.alloc<double>((size_t)1 << maxsb);
    int *dmem = s.alloc<int>(maxsb);
    for (size_t b = 0; b < blocks.size(); ++b) {
        s.copy(dmask, bmask[b]);
        s.copy(dwt, bwt[b]);
        s.copy(dmem, blocks[b]);
        if (s.rc) break;
        launch_block_sampler(dmask, dwt, (int)bmask[b].size(), (int)blocks[b].size(), dmem, N, n, (unsigned long long)seed, (int)b, den,
                             dcdf, s.out, s.st);
        if (s.sync()) break; // (the staging buffers are reused by the next block)
    }
    return s.finish(false, 0, dedupe, out);
}

Incidences gml::build_incidences(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n) {
    Incidences inc((size_t)n);
    std::vector<int> sp;
    for (int64_t t = 0; t < nterms; ++t) {
        if (weights[t] == 0.0) continue;
        reduce_key(keys + t * key_stride, key_stride, sp);
        for (size_t a = 0; a < sp.size(); ++a) {
            std::vector<int> others;
            for (size_t b = 0; b < sp.size(); ++b)
                if (b != a) others.push_back(sp[b]);
            inc[(size_t)sp[a]].emplace_back(weights[t], std::move(others));
        }
    }
    return inc;
}

static int create_mcmc_terms(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, int64_t N, uint64_t seed,
                             int sweeps, int order, int64_t node0, int64_t node1, int device, gml_problem **out, bool dedupe) {
    if (int rc = check_out(out)) return rc;
    if (int rc = check_term_pointers(keys, key_stride, weights, nterms)) return rc;
    if (n <= 0 || N <= 0 || sweeps < 1) return fail(GML_EINVAL, "n, N and sweeps must be positive");
    if (int rc = gml_check_handle_args(n, order, node0, node1)) return rc;
    if (int rc = check_term_values(keys, key_stride, weights, nterms, n)) return rc;
    if (int rc = gml_check_device(device)) return rc;
    const Incidences inc = build_incidences(keys, key_stride, weights, nterms, n);
    std::vector<int> ioff((size_t)n + 1, 0), ooff(1, 0), oth;
    std::vector<double> iw;
    for (int64_t i = 0; i < n; ++i) {
        for (auto &e : inc[(size_t)i]) {
            iw.push_back(e.first);
            for (int j : e.second) oth.push_back(j);
            ooff.push_back((int)oth.size());
        }
        ioff[(size_t)i + 1] = (int)iw.size();
    }
    if (iw.empty()) iw.push_back(0.0);
    if (oth.empty()) oth.push_back(0);
    const int64_t Np = round_up(N, 256);
    SamplerStaging s;
    if (int rc = s.begin(device, N, n, order, node0, node1, (size_t)n * Np, true)) return rc;
    const int *dioff = s.upload(ioff), *dooff = s.upload(ooff), *doth = s.upload(oth);
    const double *diw = s.upload(iw);
    if (s.rc) return s.rc;
    launch_glauber(dioff, diw, dooff, doth, n, N, Np, sweeps, (unsigned long long)seed, s.out, s.st);
    return s.finish(true, Np, dedupe, out); // the chains' final states, spin-major
}

// The model of gml_problem_create_mcmc_chains, quantised row by row: sigma_i = 2^(e - 38) with max_{j != i} |A_ij| < 2^e, q_ij =
// rint(A_ij / sigma_i), q_ii = 0, held in 5 balanced base-256 digit planes (include/gml.h).  The digit planes are pre-tiled as the
// kernel reads them: fragment (b, kt, l) = [64 lanes][16 B], lane (il, hh) byte t = digit l of q[32 b + il][32 kt + 16 hh + t].
struct QuantisedRows {
    std::vector<int8_t> dg;
    std::vector<double> qblk, diag, sig, qsum;
};
static QuantisedRows quantise_rows(const double *model, int64_t n) {
    const int64_t nb = (n + 31) / 32, np = 32 * nb;
    const std::vector<double> zero((size_t)np, 0.0);
    QuantisedRows r{std::vector<int8_t>((size_t)(5 * np * np), 0), std::vector<double>((size_t)(nb * 1024), 0.0), zero, zero, zero};
    auto &[dg, qblk, diag, sig, qsum] = r;
    for (int64_t i = 0; i < n; ++i) {
        const double *row = model + i * n;
        double mx = 0.0;
        for (int64_t j = 0; j < n; ++j)
            if (j != i) mx = std::max(mx, std::fabs(row[j]));
        int ex = 0;
        if (mx > 0) (void)std::frexp(mx, &ex);
        diag[(size_t)i] = row[i];
        sig[(size_t)i] = std::ldexp(1.0, ex - 38);
        const int64_t b = i >> 5, il = i & 31;
        long long qs = 0;
        for (int64_t j = 0; j < n; ++j) {
            if (j == i) continue;
            long long q = (long long)std::nearbyint(std::ldexp(row[j], 38 - ex));
            qs += q;
            if ((j >> 5) == b) qblk[(size_t)(b * 1024 + il * 32 + (j & 31))] = (double)q;
            const int64_t kt = j >> 5, lane = ((j >> 4) & 1) * 32 + il, t = j & 15;
            int8_t *d = dg.data() + ((b * nb + kt) * 5 * 64 + lane) * 16 + t;
            for (int l = 0; l < 5; ++l) {
                const long long dgt = ((q + 128) & 255) - 128;
                q = (q - dgt) >> 8;
                d[l * 1024] = (int8_t)dgt;
            }
        }
        qsum[(size_t)i] = (double)qs;
    }
    return r;
}

// gml_problem_create_mcmc_chains: Glauber chains of a dense pairwise model on the int8 matrix cores (gml_mcmc_chains.hip).
extern "C" int gml_problem_create_mcmc_chains(const double *model, int64_t n, int64_t chains, int64_t samples_per_chain, int burn_in,
                                              int thin, uint64_t seed, int histogram, int order, int64_t node0, int64_t node1, int device,
                                              gml_problem **out) {
    if (int rc = check_out(out)) return rc;
    if (!model) return fail(GML_EINVAL, "model is NULL");
    if (int rc = check_chain_args(n, chains, samples_per_chain, burn_in, thin, order, node0, node1)) return rc;
    if (int rc = check_symmetric_finite(model, n)) return rc;
    const int64_t M = chains * samples_per_chain;
    if (n > kMcmcChainsMaxN || mcmc_chains_tile(n) == 0)
        return fail(GML_EUNSUPPORTED, "the int8 chain kernel supports n <= %lld spins (n = %lld)", (long long)kMcmcChainsMaxN, (long long)n);
    if (histogram)
        if (int rc = check_hist_limits(n, M)) return rc;
    if (int rc = gml_check_device(device)) return rc;
    const QuantisedRows q = quantise_rows(model, n);
    const int64_t ld = round_up(M, 256);
    SamplerStaging s;
    if (int rc = s.begin(device, M, n, order, node0, node1, (size_t)n * ld, true)) return rc;
    const int8_t *dDg = s.upload(q.dg);
    const double *dq = s.upload(q.qblk), *dd = s.upload(q.diag), *ds = s.upload(q.sig), *dsum = s.upload(q.qsum);
    if (s.rc) return s.rc;
    launch_mcmc_chains(dDg, dq, dd, ds, dsum, n, chains, burn_in, thin, (int)samples_per_chain, (unsigned long long)seed, s.out, ld, s.st);
    return s.finish(true, ld, histogram != 0, out); // the recorded states, spin-major
}

extern "C" int gml_problem_create_mcmc_terms(const int32_t *keys, int key_stride, const double *weights, int64_t nterms,
                                             int64_t n, int64_t N, uint64_t seed, int sweeps, int order, int64_t node0,
                                             int64_t node1, int device, gml_problem **out) {
    return create_mcmc_terms(keys, key_stride, weights, nterms, n, N, seed, sweeps, order, node0, node1, device, out, false);
}

extern "C" int gml_problem_create_sampled_hist(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                               int64_t N, uint64_t seed, int mcmc_sweeps, int order, int64_t node0, int64_t node1,
                                               int device, gml_problem **out) {
    if (int rc = check_hist_spins(n)) return rc; // (N < 2^31 is left to gml_create_from_device_bytes)
    if (mcmc_sweeps > 0) return create_mcmc_terms(keys, key_stride, weights, nterms, n, N, seed, mcmc_sweeps, order, node0, node1, device, out, true);
    return create_sampled_terms(keys, key_stride, weights, nterms, n, N, seed, order, node0, node1, device, out, true);
}

extern "C" int gml_problem_get_counts(gml_problem *p, double *counts) {
    if (!p || !counts) return fail(GML_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpyAsync(counts, p->d.w, sizeof(double) * p->K, hipMemcpyDeviceToHost, p->st));
    HIPCHK(hipStreamSynchronize(p->st));
    // w_k = counts_k / M (:170): integer counts come back exactly (M <= 2^50: two roundings of 2^-53 each stay below 1/2)
    const double unit = p->counts_int ? 1.0 : 1e6;
    for (int64_t k = 0; k < p->K; ++k) counts[k] = std::nearbyint(counts[k] * p->M * unit) / unit;
    return GML_OK;
}

// ------------------------------------------------------------------------------------------
// gml_problem_moments, gml_problem_term_moments: exact integer sums over the handle's configurations (gml_moments.hip)
// ------------------------------------------------------------------------------------------
// Device blocks of one moments call: freed on every path.
struct MomentsBlocks {
    std::vector<void *> blocks;
    ~MomentsBlocks() {
        for (void *q : blocks) (void)dev_free(q);
    }
    template <class T> hipError_t alloc(T **out, size_t count) {
        const hipError_t e = dev_malloc(out, sizeof(T) * std::max<size_t>(count, 1));
        if (e == hipSuccess) blocks.push_back(*out);
        return e;
    }
};

// The exactness contract (gml.h): integer counts and M <= 2^50, so that c_k = rint(w_k M) on the device.
static int check_moments_handle(const gml_problem *p) {
    if (!p->counts_int)
        return fail(GML_EUNSUPPORTED, "the handle was created with a fractional count: exact moments need integer counts");
    if (!(p->M <= 1125899906842624.0))
        return fail(GML_EUNSUPPORTED, "the sum of the counts M = %.17g exceeds 2^50: exact moments need M <= 2^50", p->M);
    return GML_OK;
}

// The count planes of a handle whose counts differ (none, *nplanes = 0, when they are all equal: *c is the common count).
static int moments_planes(gml_problem *p, MomentsBlocks &mb, unsigned **planes, int *nplanes, long long *c) {
    *planes = nullptr;
    *nplanes = 0;
    *c = 1;
    if (p->d.wuni != 0.0) {
        *c = (long long)std::nearbyint(p->d.wuni * p->M);
        return GML_OK;
    }
    const unsigned long long cmax = (unsigned long long)std::nearbyint(p->d.wmax * p->M);
    int nb = 1;
    while (nb < 64 && (cmax >> nb) != 0) ++nb;
    HIPCHK(mb.alloc(planes, (size_t)nb * (size_t)(p->d.Kp / 32)));
    launch_count_planes(p->d, p->M, nb, *planes, p->st);
    *nplanes = nb;
    return GML_OK;
}

// sums[t] = M - 2 c Nt[t] of the reduced keys (host vectors), through the term kernel
static int term_sums(gml_problem *p, MomentsBlocks &mb, const std::vector<int32_t> &rkeys, int L, int64_t nterms, const unsigned *planes,
                     int nplanes, long long c, int64_t *sums) {
    int32_t *dkeys = nullptr;
    unsigned long long *dNt = nullptr;
    HIPCHK(mb.alloc(&dkeys, rkeys.size()));
    HIPCHK(mb.alloc(&dNt, (size_t)nterms));
    HIPCHK(hipMemcpyAsync(dkeys, rkeys.data(), sizeof(int32_t) * rkeys.size(), hipMemcpyHostToDevice, p->st));
    HIPCHK(hipMemsetAsync(dNt, 0, sizeof(unsigned long long) * nterms, p->st));
    launch_moments_terms(p->d, dkeys, L, nterms, planes, nplanes, dNt, p->st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sums, dNt, sizeof(int64_t) * nterms, hipMemcpyDeviceToHost, p->st));
    HIPCHK(hipStreamSynchronize(p->st));
    const int64_t M = (int64_t)p->M;
    for (int64_t t = 0; t < nterms; ++t) sums[t] = M - 2 * c * sums[t];
    return GML_OK;
}

extern "C" int gml_problem_moments(gml_problem *p, int64_t *sum1, int64_t *sum2) {
    if (!p || !sum1) return fail(GML_EINVAL, "NULL argument");
    if (int rc = check_moments_handle(p)) return rc;
    HIPCHK(hipSetDevice(p->device));
    MomentsBlocks mb;
    unsigned *planes = nullptr;
    int nplanes = 0;
    long long c = 1;
    if (int rc = moments_planes(p, mb, &planes, &nplanes, &c)) return rc;
    std::vector<int32_t> keys((size_t)p->n);
    for (int64_t i = 0; i < p->n; ++i) keys[(size_t)i] = (int32_t)i;
    if (int rc = term_sums(p, mb, keys, 1, p->n, planes, nplanes, c, sum1)) return rc;
    if (!sum2) return GML_OK;
    long long *dS2 = nullptr;
    const size_t bytes = sizeof(long long) * (size_t)p->n * (size_t)p->n;
    HIPCHK(mb.alloc(&dS2, (size_t)p->n * (size_t)p->n));
    HIPCHK(hipMemsetAsync(dS2, 0, bytes, p->st));
    launch_moments_pairs(p->d, planes, nplanes, (long long)p->M, c, dS2, p->st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sum2, dS2, bytes, hipMemcpyDeviceToHost, p->st));
    HIPCHK(hipStreamSynchronize(p->st));
    return GML_OK;
}

extern "C" int gml_problem_term_moments(gml_problem *p, const int32_t *keys, int key_stride, int64_t nterms, int64_t *sums) {
    if (!p || !keys || !sums) return fail(GML_EINVAL, "NULL argument");
    if (key_stride < 1 || nterms < 0) return fail(GML_EINVAL, "key_stride must be at least 1 and nterms non-negative");
    for (int64_t t = 0; t < nterms; ++t)
        for (int a = 0; a < key_stride; ++a) {
            const int32_t v = keys[t * key_stride + a];
            if (v < -1 || v >= p->n) return fail(GML_EINVAL, "term %lld names spin %d outside [0,%lld)", (long long)t, v, (long long)p->n);
        }
    if (nterms == 0) return GML_OK;
    if (int rc = check_moments_handle(p)) return rc;
    // the distinct spins of every key (a spin named twice cancels), padded to the longest
    std::vector<int> sp;
    std::vector<int32_t> tmp((size_t)nterms * key_stride, -1);
    int L = 1;
    for (int64_t t = 0; t < nterms; ++t) {
        reduce_key(keys + t * key_stride, key_stride, sp);
        std::copy(sp.begin(), sp.end(), tmp.begin() + t * key_stride);
        L = std::max(L, (int)sp.size());
    }
    if (L < key_stride) {
        for (int64_t t = 1; t < nterms; ++t) std::copy(tmp.begin() + t * key_stride, tmp.begin() + t * key_stride + L, tmp.begin() + t * L);
        tmp.resize((size_t)nterms * L);
    }
    HIPCHK(hipSetDevice(p->device));
    MomentsBlocks mb;
    unsigned *planes = nullptr;
    int nplanes = 0;
    long long c = 1;
    if (int rc = moments_planes(p, mb, &planes, &nplanes, &c)) return rc;
    return term_sums(p, mb, tmp, L, nterms, planes, nplanes, c, sums);
}

extern "C" int gml_problem_create_sampled_terms(const int32_t *keys, int key_stride, const double *weights, int64_t nterms,
                                                int64_t n, int64_t N, uint64_t seed, int order, int64_t node0,
                                                int64_t node1, int device, gml_problem **out) {
    return create_sampled_terms(keys, key_stride, weights, nterms, n, N, seed, order, node0, node1, device, out);
}

extern "C" int gml_problem_create_sampled(const double *model, int64_t n, int64_t N, uint64_t seed, int order,
                                          int64_t node0, int64_t node1, int device, gml_problem **out) {
    if (!model || !out) return fail(GML_EINVAL, "NULL argument");
    *out = nullptr;
    if (n <= 0) return fail(GML_EINVAL, "n and N must be positive");
    if (int rc = check_symmetric_finite(model, n)) return rc;
    // the matrix as terms: 1/2 s^T A s = sum_{i<j} A_ij s_i s_j (sampling.jl:40), prior = diagonal (:41)
    std::vector<int32_t> keys;
    std::vector<double> wts;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j <= i; ++j) {
            const double v = model[i * n + j];
            if (v == 0.0) continue;
            keys.push_back((int32_t)j);
            keys.push_back(j < i ? (int32_t)i : -1);
            wts.push_back(v);
        }
    return create_sampled_terms(keys.data(), 2, wts.data(), (int64_t)wts.size(), n, N, seed, order, node0, node1, device, out);
}

// the +-1 configurations held by the handle, K x n row-major (for tests and for callers that want the
// samples back, e.g. to build the reference's histogram)
extern "C" int gml_problem_get_spins(gml_problem *p, int8_t *spins) {
    if (!p || !spins) return fail(GML_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(p->device));
    // sign bits -> +-1 bytes, sample-major, on the device (in slabs of <= 2^22 samples), one copy per slab
    const int64_t slab = std::min<int64_t>(p->K, (int64_t)1 << 22);
    int8_t *dT = nullptr;
    HIPCHK(dev_malloc(&dT, (size_t)slab * p->n));
    int rc = GML_OK;
    for (int64_t k0 = 0; k0 < p->K && rc == GML_OK; k0 += slab) {
        const int64_t kk = std::min(slab, p->K - k0);
        launch_unpack_spins(p->d, k0, kk, dT, p->st);
        if (hipMemcpyAsync(spins + k0 * p->n, dT, (size_t)kk * p->n, hipMemcpyDeviceToHost, p->st) != hipSuccess ||
            hipStreamSynchronize(p->st) != hipSuccess)
            rc = fail(GML_EHIP, "download of the spins failed: %s", hipGetErrorString(hipGetLastError()));
    }
    (void)dev_free(dT);
    return rc;
}

// ------------------------------------------------------------------------------------------
// gml_model_exact: exact log Z and exact expectations, component by component (gml_exact.hip)
// ------------------------------------------------------------------------------------------
// sum of v with at most 1024 terms added serially into one accumulator: halves above that
static double pairwise_sum(const double *v, size_t count) {
    if (count <= 1024) {
        double s = 0.0;
        for (size_t i = 0; i < count; ++i) s += v[i];
        return s;
    }
    const size_t half = count / 2;
    return pairwise_sum(v, half) + pairwise_sum(v + half, count - half);
}

// One component as the kernel takes it (gml_dev.h: ExactPlan): c low bits, the terms sorted by low mask (stable: the order of the
// caller's list within a mask), items, partial sums.  mask: the terms over the component's own spins.
struct ExactComponent {
    int sb = 0, c = 0;
    std::vector<double> w;
    std::vector<unsigned long long> hi;
    std::vector<int> item_off, item_dst, ms_off, ms_dst;
    std::vector<unsigned long long> queries; // masks over the component's spins whose expectations are wanted
    std::vector<double> expect;              // their expectations
    double log_z = 0.0;
};
static int plan_exact_component(const std::vector<unsigned long long> &mask, const std::vector<double> &wt, ExactComponent &pc) {
    const size_t T = mask.size();
    if (T > ((size_t)1 << 20))
        return fail(GML_EUNSUPPORTED, "a connected component of the model has %zu terms: exact enumeration takes at most 2^20", T);
    pc.c = std::min(pc.sb, g_exact_chunk_bits > 0 ? g_exact_chunk_bits : kExactChunkBits);
    pc.c = std::max(pc.c, pc.sb - 30); // (a hooked c: at most 2^20 chunks per group, kExactBlock blocks of kExactBlock chunks)
    const unsigned long long low = ((unsigned long long)1 << pc.c) - 1;
    std::vector<int> idx(T);
    for (size_t t = 0; t < T; ++t) idx[t] = (int)t;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return (mask[(size_t)a] & low) < (mask[(size_t)b] & low); });
    std::vector<int> lo(T);
    pc.w.resize(T);
    pc.hi.resize(T);
    for (size_t t = 0; t < T; ++t) {
        lo[t] = (int)(mask[(size_t)idx[t]] & low);
        pc.hi[t] = mask[(size_t)idx[t]] >> pc.c;
        pc.w[t] = wt[(size_t)idx[t]];
    }
    // items of at most L terms; L doubles until the partial sums of the masks with several items fit the kernel's kExactParts
    for (int L = 16;; L *= 2) {
        pc.item_off.assign(1, 0);
        pc.item_dst.clear();
        pc.ms_off.assign(1, 0);
        pc.ms_dst.clear();
        int parts = 0;
        for (size_t a = 0; a < T;) {
            size_t b = a;
            while (b < T && lo[b] == lo[a]) ++b;
            const int slot = lo[a] + (lo[a] >> 4), nseg = (int)((b - a + (size_t)L - 1) / (size_t)L);
            for (int s = 0; s < nseg; ++s) {
                pc.item_off.push_back((int)std::min(b, a + (size_t)(s + 1) * (size_t)L));
                pc.item_dst.push_back(nseg == 1 ? slot : ~(parts + s));
            }
            if (nseg > 1) {
                parts += nseg;
                pc.ms_off.push_back(parts);
                pc.ms_dst.push_back(slot);
            }
            a = b;
        }
        if (parts <= kExactParts) break;
        if (L >= 1024) return fail(GML_EUNSUPPORTED, "a connected component of the model has too many terms for exact enumeration");
    }
    return GML_OK;
}

// the planned component's terms, items and partial sums on the device, and its chunks dealt to G groups of cpg
static ExactPlan upload_exact_terms(SamplerStaging &s, ExactComponent &pc, int &G) {
    ExactPlan P{};
    P.ni = (int)pc.item_dst.size();
    P.nm = (int)pc.ms_dst.size();
    if (pc.ms_dst.empty()) pc.ms_dst.push_back(0); // (no empty upload; the vectors outlive the stream's copies)
    P.w = s.upload(pc.w);
    P.hi = s.upload(pc.hi);
    P.item_off = s.upload(pc.item_off);
    P.item_dst = s.upload(pc.item_dst);
    P.ms_off = s.upload(pc.ms_off);
    P.ms_dst = s.upload(pc.ms_dst);
    const long long nchunks = (long long)1 << (pc.sb - pc.c);
    G = (int)std::min<long long>(nchunks, kExactGroups);
    P.cpg = nchunks / G;
    return P;
}

// the enumerations of one planned component: its queries in windows of kExactWindow - 1 beside the empty query (Z)
static int run_exact_component(ExactComponent &pc, int device) {
    SamplerStaging s;
    if (int rc = s.open(device)) return rc;
    int G = 0;
    ExactPlan P = upload_exact_terms(s, pc, G);
    P.gm = s.alloc<double>((size_t)G);
    P.gacc = s.alloc<double>((size_t)G * kExactWindow);
    int *dqlo = s.alloc<int>(kExactWindow);
    unsigned long long *dqhi = s.alloc<unsigned long long>(kExactWindow);
    double *dres = s.alloc<double>(kExactWindow + 1);
    if (s.rc) return s.rc;
    P.q_lo = dqlo;
    P.q_hi = dqhi;
    const unsigned long long low = ((unsigned long long)1 << pc.c) - 1;
    const size_t nq = pc.queries.size(), step = kExactWindow - 1;
    pc.expect.assign(nq, 0.0);
    std::vector<double> res((size_t)kExactWindow + 1);
    for (size_t q0 = 0; q0 == 0 || q0 < nq; q0 += step) {
        const size_t cnt = std::min(step, nq - q0);
        std::vector<int> qlo(1, 0);
        std::vector<unsigned long long> qhi(1, 0);
        for (size_t q = q0; q < q0 + cnt; ++q) {
            qlo.push_back((int)(pc.queries[q] & low));
            qhi.push_back(pc.queries[q] >> pc.c);
        }
        P.nq = (int)cnt + 1;
        s.copy(dqlo, qlo);
        s.copy(dqhi, qhi);
        if (s.rc) return s.rc;
        launch_exact(P, G, dres, s.st);
        s.ok(hipGetLastError(), "the enumeration's launch");
        s.ok(hipMemcpyAsync(res.data(), dres, sizeof(double) * (size_t)(P.nq + 1), hipMemcpyDeviceToHost, s.st), "hipMemcpyAsync");
        if (s.sync()) return s.rc;
        // Z = 2^(c - 12) res[0] exp(M): the bits above c are in no term and doubled every sum (an exact scaling)
        const double Zs = res[0], M = res[(size_t)P.nq];
        pc.log_z = M + std::log(std::ldexp(Zs, pc.c - kExactChunkBits));
        for (size_t q = 0; q < cnt; ++q) pc.expect[q0 + q] = res[q + 1] / Zs;
    }
    return GML_OK;
}

// The model by connected components: local[i] = the place of spin i in its component, mask / wt [b] = the component's terms over its own
// spins in the caller's order, consts = the weights of the terms that reduce to the empty key.  Refuses a component above 40 spins.
struct ComponentTerms {
    TermComponents tc;
    std::vector<int> local;
    std::vector<std::vector<unsigned long long>> mask;
    std::vector<std::vector<double>> wt;
    std::vector<double> consts;
};
static int component_terms(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, ComponentTerms &ct) {
    ct.tc = term_components(keys, key_stride, weights, nterms, n);
    const size_t nb = ct.tc.blocks.size();
    for (auto &b : ct.tc.blocks)
        if (b.size() > (size_t)kExactMaxSpins)
            return fail(GML_EUNSUPPORTED, "a connected component of the model has %zu spins: exact enumeration is limited to %d", b.size(),
                        kExactMaxSpins);
    ct.local.assign((size_t)n, 0);
    for (auto &b : ct.tc.blocks)
        for (size_t i = 0; i < b.size(); ++i) ct.local[(size_t)b[i]] = (int)i;
    ct.mask.resize(nb);
    ct.wt.resize(nb);
    std::vector<int> sp;
    for (int64_t t = 0; t < nterms; ++t) {
        if (weights[t] == 0.0) continue;
        reduce_key(keys + t * key_stride, key_stride, sp);
        if (sp.empty()) {
            ct.consts.push_back(weights[t]);
            continue;
        }
        unsigned long long mask = 0;
        for (int v : sp) mask |= (unsigned long long)1 << ct.local[(size_t)v];
        const size_t b = (size_t)ct.tc.id[(size_t)sp[0]];
        ct.mask[b].push_back(mask);
        ct.wt[b].push_back(weights[t]);
    }
    return GML_OK;
}

extern "C" int gml_model_exact(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, const int32_t *qkeys,
                               int qkey_stride, int64_t nq, int device, double *log_z, double *mean, double *corr, double *qexp) {
    if (!log_z) return fail(GML_EINVAL, "log_z is NULL");
    if (int rc = check_term_pointers(keys, key_stride, weights, nterms)) return rc;
    if (n <= 0 || nterms < 0) return fail(GML_EINVAL, "n must be positive and nterms non-negative");
    if (nq < 0 || (nq > 0 && (!qkeys || !qexp || qkey_stride < 1))) return fail(GML_EINVAL, "NULL or malformed query list");
    if (int rc = check_term_values(keys, key_stride, weights, nterms, n)) return rc;
    for (int64_t q = 0; q < nq; ++q)
        for (int a = 0; a < qkey_stride; ++a) {
            const int32_t v = qkeys[q * qkey_stride + a];
            if (v < -1 || v >= n) return fail(GML_EINVAL, "query %lld names spin %d outside [0,%lld)", (long long)q, v, (long long)n);
        }
    // per component: its terms as masks over its own spins; the empty key is a constant of log Z
    ComponentTerms ct;
    if (int rc = component_terms(keys, key_stride, weights, nterms, n, ct)) return rc;
    const TermComponents &tc = ct.tc;
    const size_t nb = tc.blocks.size();
    const std::vector<int> &local = ct.local;
    const std::vector<std::vector<unsigned long long>> &bmask = ct.mask;
    const std::vector<std::vector<double>> &bwt = ct.wt;
    std::vector<double> parts = ct.consts; // the summands of log Z
    std::vector<int> sp;
    // a spin in no term needs no enumeration: ln 2, mean 0; the others are planned before the device is looked for
    const bool moments = mean || corr;
    std::vector<ExactComponent> comp(nb);
    int64_t nfree = 0;
    for (size_t b = 0; b < nb; ++b) {
        ExactComponent &pc = comp[b];
        if (bmask[b].empty()) {
            ++nfree;
            continue;
        }
        pc.sb = (int)tc.blocks[b].size();
        if (int rc = plan_exact_component(bmask[b], bwt[b], pc)) return rc;
        if (moments)
            for (int i = 0; i < pc.sb; ++i) pc.queries.push_back((unsigned long long)1 << i);
        if (corr)
            for (int i = 0; i < pc.sb; ++i)
                for (int j = i + 1; j < pc.sb; ++j) pc.queries.push_back(((unsigned long long)1 << i) | ((unsigned long long)1 << j));
    }
    // a query is the product over the components of the expectations of its restrictions: (component, index of the restriction)
    std::vector<int64_t> uq_off((size_t)nq + 1, 0);
    std::vector<std::pair<int64_t, int64_t>> uq;
    std::vector<uint8_t> uq_zero((size_t)nq, 0);
    std::vector<std::pair<int64_t, unsigned long long>> restr;
    for (int64_t q = 0; q < nq; ++q) {
        reduce_key(qkeys + q * qkey_stride, qkey_stride, sp);
        restr.clear();
        for (int v : sp) {
            const int64_t b = tc.id[(size_t)v];
            if (bmask[(size_t)b].empty()) uq_zero[(size_t)q] = 1; // a free spin: expectation 0
            auto it = std::find_if(restr.begin(), restr.end(), [&](auto &r) { return r.first == b; });
            if (it == restr.end()) it = restr.insert(restr.end(), {b, 0ull});
            it->second |= (unsigned long long)1 << local[(size_t)v];
        }
        std::sort(restr.begin(), restr.end());
        if (!uq_zero[(size_t)q])
            for (auto &r : restr) {
                uq.emplace_back(r.first, (int64_t)comp[(size_t)r.first].queries.size());
                comp[(size_t)r.first].queries.push_back(r.second);
            }
        uq_off[(size_t)q + 1] = (int64_t)uq.size();
    }
    if (int rc = gml_check_device(device)) return rc;
    for (size_t b = 0; b < nb; ++b) {
        if (bmask[b].empty()) continue;
        if (int rc = run_exact_component(comp[b], device)) return rc;
        parts.push_back(comp[b].log_z);
    }
    parts.push_back((double)nfree * std::log(2.0));
    *log_z = pairwise_sum(parts.data(), parts.size());
    if (moments) {
        std::vector<double> m((size_t)n, 0.0);
        for (size_t b = 0; b < nb; ++b)
            if (!bmask[b].empty())
                for (size_t i = 0; i < tc.blocks[b].size(); ++i) m[(size_t)tc.blocks[b][i]] = comp[b].expect[i];
        if (mean) std::copy(m.begin(), m.end(), mean);
        if (corr) {
            for (int64_t i = 0; i < n; ++i)
                for (int64_t j = 0; j < n; ++j) corr[i * n + j] = i == j ? 1.0 : m[(size_t)i] * m[(size_t)j];
            for (size_t b = 0; b < nb; ++b) {
                if (bmask[b].empty()) continue;
                const std::vector<int> &mem = tc.blocks[b];
                size_t at = mem.size(); // (the pairs follow the means, i < j in order)
                for (size_t i = 0; i < mem.size(); ++i)
                    for (size_t j = i + 1; j < mem.size(); ++j, ++at)
                        corr[(int64_t)mem[i] * n + mem[j]] = corr[(int64_t)mem[j] * n + mem[i]] = comp[b].expect[at];
            }
        }
    }
    for (int64_t q = 0; q < nq; ++q) {
        double e = uq_zero[(size_t)q] ? 0.0 : 1.0;
        for (int64_t a = uq_off[(size_t)q]; a < uq_off[(size_t)q + 1] && !uq_zero[(size_t)q]; ++a)
            e *= comp[(size_t)uq[(size_t)a].first].expect[(size_t)uq[(size_t)a].second];
        qexp[q] = e;
    }
    return GML_OK;
}

// ------------------------------------------------------------------------------------------
// gml_model_best_states: the k most probable states, component by component (gml_best.hip), merged on the host
// ------------------------------------------------------------------------------------------
namespace {

// best states over some of the spins, best first (energy descending, equal energies state ascending): entry r has energy e[r] and the
// n sign bits bits[r W .. (r + 1) W), bit i of word i / 64 set <-> spin i is -1 (a spin outside the list's spins: 0)
struct BestList {
    size_t W = 1;
    std::vector<double> e;
    std::vector<uint64_t> bits;
    size_t size() const { return e.size(); }
    const uint64_t *at(size_t r) const { return bits.data() + r * W; }
};

// The k best sums of two lists over disjoint spins.  A heap walks the pairs (i, j) in the order of e_A[i] + e_B[j] (rounded sums are
// monotone in either index, so the frontier rule holds), past k until the sum falls below the k-th: every pair that ties with the
// cut is seen.  The pairs are then sorted by (sum descending, joint state ascending -- compared from the highest spin down) and cut.
BestList merge_best(const BestList &A, const BestList &B, size_t k) {
    struct Pair {
        double e;
        uint32_t i, j;
    };
    const size_t W = A.W, na = A.size(), nb = B.size();
    auto state_less = [&](const Pair &p, const Pair &q) {
        for (size_t w = W; w-- > 0;) {
            const uint64_t x = A.at(p.i)[w] | B.at(p.j)[w], y = A.at(q.i)[w] | B.at(q.j)[w];
            if (x != y) return x < y;
        }
        return false;
    };
    auto lower_sum = [](const Pair &p, const Pair &q) { return p.e < q.e; };
    std::vector<Pair> heap, got;
    std::vector<uint8_t> seen(na * nb, 0);
    auto push = [&](size_t i, size_t j) {
        if (i >= na || j >= nb || seen[i * nb + j]) return;
        seen[i * nb + j] = 1;
        heap.push_back(Pair{A.e[i] + B.e[j], (uint32_t)i, (uint32_t)j});
        std::push_heap(heap.begin(), heap.end(), lower_sum);
    };
    push(0, 0);
    while (!heap.empty() && (got.size() < k || heap.front().e == got.back().e)) {
        std::pop_heap(heap.begin(), heap.end(), lower_sum);
        const Pair p = heap.back();
        heap.pop_back();
        got.push_back(p);
        push(p.i + 1, p.j);
        push(p.i, p.j + 1);
    }
    std::sort(got.begin(), got.end(), [&](const Pair &p, const Pair &q) { return p.e != q.e ? p.e > q.e : state_less(p, q); });
    if (got.size() > k) got.resize(k);
    BestList out;
    out.W = W;
    out.bits.resize(got.size() * W);
    for (size_t r = 0; r < got.size(); ++r) {
        out.e.push_back(got[r].e);
        for (size_t w = 0; w < W; ++w) out.bits[r * W + w] = A.at(got[r].i)[w] | B.at(got[r].j)[w];
    }
    return out;
}

// The min(k, 2^sb) best states of one planned component: the device selects by the energies of its butterflies (equal ones: the lower
// state), the host cuts the groups' lists to one, recomputes every selected energy as the plain sum of the component's terms in the
// caller's order (pairwise_sum) and sorts by (that energy descending, state ascending).
int run_best_component(ExactComponent &pc, const std::vector<unsigned long long> &mask, const std::vector<double> &wt, int k, int device,
                       std::vector<std::pair<double, unsigned long long>> &best) {
    SamplerStaging s;
    if (int rc = s.open(device)) return rc;
    int G = 0;
    const ExactPlan P = upload_exact_terms(s, pc, G);
    const size_t cand = (size_t)G * (size_t)k;
    double *dge = s.alloc<double>(cand);
    unsigned long long *dgs = s.alloc<unsigned long long>(cand);
    if (s.rc) return s.rc;
    launch_exact_best(P, G, pc.c, k, dge, dgs, s.st);
    s.ok(hipGetLastError(), "the selection's launch");
    std::vector<double> ge(cand);
    std::vector<unsigned long long> gs(cand);
    s.ok(hipMemcpyAsync(ge.data(), dge, sizeof(double) * cand, hipMemcpyDeviceToHost, s.st), "hipMemcpyAsync");
    s.ok(hipMemcpyAsync(gs.data(), dgs, sizeof(unsigned long long) * cand, hipMemcpyDeviceToHost, s.st), "hipMemcpyAsync");
    if (s.sync()) return s.rc;
    std::vector<size_t> idx;
    for (size_t a = 0; a < cand; ++a)
        if (gs[a] != ~0ull) idx.push_back(a);
    const unsigned long long states = (unsigned long long)1 << pc.sb;
    const size_t want = (size_t)std::min<unsigned long long>((unsigned long long)k, states);
    if (idx.size() < want) return fail(GML_EHIP, "the selection returned %zu of %zu states", idx.size(), want);
    std::partial_sort(idx.begin(), idx.begin() + (ptrdiff_t)want, idx.end(),
                      [&](size_t a, size_t b) { return ge[a] != ge[b] ? ge[a] > ge[b] : gs[a] < gs[b]; });
    idx.resize(want);
    best.clear();
    std::vector<double> summand(mask.size());
    for (size_t a : idx) {
        for (size_t t = 0; t < mask.size(); ++t) summand[t] = (__builtin_popcountll(mask[t] & gs[a]) & 1) ? -wt[t] : wt[t];
        best.emplace_back(pairwise_sum(summand.data(), summand.size()), gs[a]);
    }
    std::sort(best.begin(), best.end(), [](auto &p, auto &q) { return p.first != q.first ? p.first > q.first : p.second < q.second; });
    return GML_OK;
}

} // namespace

extern "C" int gml_model_best_states(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, int64_t k,
                                     int device, int64_t *found, int8_t *states, double *energies) {
    if (int rc = check_term_pointers(keys, key_stride, weights, nterms)) return rc;
    if (n <= 0 || nterms < 0) return fail(GML_EINVAL, "n must be positive and nterms non-negative");
    if (int rc = check_term_values(keys, key_stride, weights, nterms, n)) return rc;
    if (k < 1) return fail(GML_EINVAL, "k must be at least 1");
    if (!found || !states || !energies) return fail(GML_EINVAL, "found, states or energies is NULL");
    if (k > kBestMax) return fail(GML_EUNSUPPORTED, "k = %lld: at most %d best states are kept", (long long)k, kBestMax);
    ComponentTerms ct;
    if (int rc = component_terms(keys, key_stride, weights, nterms, n, ct)) return rc;
    const size_t nb = ct.tc.blocks.size();
    std::vector<ExactComponent> comp(nb);
    for (size_t b = 0; b < nb; ++b) {
        if (ct.mask[b].empty()) continue; // (a spin in no term: two states of energy 0, no device work)
        comp[b].sb = (int)ct.tc.blocks[b].size();
        if (int rc = plan_exact_component(ct.mask[b], ct.wt[b], comp[b])) return rc;
    }
    if (int rc = gml_check_device(device)) return rc;
    const size_t W = (size_t)((n + 63) / 64);
    BestList all; // the constant of every energy, over no spin
    all.W = W;
    all.e.push_back(pairwise_sum(ct.consts.data(), ct.consts.size()));
    all.bits.assign(W, 0);
    std::vector<std::pair<double, unsigned long long>> best;
    for (size_t b = 0; b < nb; ++b) {
        const std::vector<int> &mem = ct.tc.blocks[b];
        if (ct.mask[b].empty()) best = {{0.0, 0ull}, {0.0, 1ull}};
        else if (int rc = run_best_component(comp[b], ct.mask[b], ct.wt[b], (int)k, device, best)) return rc;
        BestList part;
        part.W = W;
        part.bits.assign(best.size() * W, 0);
        for (size_t r = 0; r < best.size(); ++r) {
            part.e.push_back(best[r].first);
            for (size_t i = 0; i < mem.size(); ++i)
                if ((best[r].second >> i) & 1ull) part.bits[r * W + (size_t)mem[i] / 64] |= (uint64_t)1 << (mem[i] % 64);
        }
        all = merge_best(all, part, (size_t)k);
    }
    *found = (int64_t)all.size();
    for (size_t r = 0; r < all.size(); ++r) {
        energies[r] = all.e[r];
        for (int64_t i = 0; i < n; ++i) states[(int64_t)r * n + i] = ((all.at(r)[(size_t)i / 64] >> (i % 64)) & 1u) ? -1 : 1;
    }
    return GML_OK;
}
