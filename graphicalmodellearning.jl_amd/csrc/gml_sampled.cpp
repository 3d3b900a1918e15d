// libgml_hip, host side: handles whose samples are drawn on the device -- the step before the path (src/sampling.jl:34-106):
// exact block sampling, Glauber chains, histogramming of the draws.
#include "gml_internal.h"
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
// gml_problem_create_sampled: sample on the device, then build the handle from the device-resident
// samples (the step before the path; src/sampling.jl:34-57, 94-106)
// ------------------------------------------------------------------------------------------
// Terms of one model: spins of term t = keys[t*stride .. +stride) (0-based, -1 = unused slot).
static int create_sampled_terms(const int32_t *keys, int stride, const double *weights, int64_t nterms, int64_t n,
                                int64_t N, uint64_t seed, int order, int64_t node0, int64_t node1, int device,
                                gml_problem **out, bool dedupe = false) {
    if (!out) return fail(GML_EINVAL, "out is NULL");
    *out = nullptr;
    if ((nterms > 0 && (!keys || !weights)) || stride < 1) return fail(GML_EINVAL, "NULL or malformed term list");
    if (n <= 0 || N <= 0) return fail(GML_EINVAL, "n and N must be positive");
    if (order < 1 || order > 8) return fail(GML_EINVAL, "interaction order %d out of range [1,8]", order);
    if (node0 < 0 || node1 > n || node0 >= node1)
        return fail(GML_EINVAL, "bad node range [%lld,%lld) for n=%lld", (long long)node0, (long long)node1, (long long)n);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(GML_EHIP, "no HIP device available (libgml_hip has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(GML_EINVAL, "device %d out of range (%d devices)", device, ndev);
    for (int64_t t = 0; t < nterms; ++t) {
        if (!std::isfinite(weights[t])) return fail(GML_EINVAL, "weight of term %lld is not finite", (long long)t);
        for (int a = 0; a < stride; ++a) {
            const int32_t v = keys[t * stride + a];
            if (v < -1 || v >= n) return fail(GML_EINVAL, "term %lld names spin %d outside [0,%lld)", (long long)t, v, (long long)n);
        }
    }
    // connected components of the term hypergraph
    std::vector<int64_t> parent((size_t)n);
    for (int64_t i = 0; i < n; ++i) parent[i] = i;
    std::function<int64_t(int64_t)> find = [&](int64_t a) {
        while (parent[a] != a) a = parent[a] = parent[parent[a]];
        return a;
    };
    for (int64_t t = 0; t < nterms; ++t) {
        if (weights[t] == 0.0) continue;
        int64_t first = -1;
        for (int a = 0; a < stride; ++a) {
            const int32_t v = keys[t * stride + a];
            if (v < 0) continue;
            if (first < 0) first = v;
            else parent[find(v)] = find(first);
        }
    }
    std::vector<std::vector<int>> blocks;
    std::vector<int64_t> id((size_t)n, -1);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = find(i);
        if (id[r] < 0) {
            id[r] = (int64_t)blocks.size();
            blocks.emplace_back();
        }
        blocks[(size_t)id[r]].push_back((int)i);
    }
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
        unsigned mask = 0;
        int64_t any = -1;
        for (int a = 0; a < stride; ++a) {
            const int32_t v = keys[t * stride + a];
            if (v < 0) continue;
            mask ^= 1u << local[(size_t)v];
            any = v;
        }
        if (any < 0) continue; // the empty term: a constant energy
        const size_t b = (size_t)id[find(any)];
        bmask[b].push_back(mask);
        bwt[b].push_back(weights[t]);
        maxnt = std::max(maxnt, bmask[b].size());
    }
    HIPCHK(hipSetDevice(device));
    gml_problem *p = new gml_problem();
    p->device = device;
    p->n = n;
    p->K = N;
    p->M = (double)N;
    p->order = order;
    p->node0 = node0;
    p->node1 = node1;
    hipStream_t st = nullptr;
    int8_t *dS = nullptr;
    double *dwt = nullptr, *den = nullptr, *dcdf = nullptr;
    unsigned *dmask = nullptr;
    int *dmem = nullptr;
    auto cleanup = [&](int rc) {
        if (dwt) (void)dev_free(dwt);
        if (dmask) (void)dev_free(dmask);
        if (den) (void)dev_free(den);
        if (dcdf) (void)dev_free(dcdf);
        if (dmem) (void)dev_free(dmem);
        if (st) (void)hipStreamDestroy(st);
        return rc;
    };
#define SCHK(expr)                                                                                              \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) {                                                                                 \
            if (dS) (void)dev_free(dS);                                                                          \
            delete p;                                                                                           \
            return cleanup(fail(e_ == hipErrorOutOfMemory ? GML_ENOMEM : GML_EHIP, "%s failed: %s", #expr,      \
                                hipGetErrorString(e_)));                                                        \
        }                                                                                                       \
    } while (0)
    SCHK(hipStreamCreate(&st));
    SCHK(dev_malloc(&dS, (size_t)N * n));
    SCHK(dev_malloc(&dwt, sizeof(double) * maxnt));
    SCHK(dev_malloc(&dmask, sizeof(unsigned) * maxnt));
    SCHK(dev_malloc(&den, sizeof(double) * ((size_t)1 << maxsb)));
    SCHK(dev_malloc(&dcdf, sizeof(double) * ((size_t)1 << maxsb)));
    SCHK(dev_malloc(&dmem, sizeof(int) * maxsb));
    for (size_t b = 0; b < blocks.size(); ++b) {
        const auto &mem = blocks[b];
        const int sb = (int)mem.size(), nt = (int)bmask[b].size();
        if (nt > 0) {
            SCHK(hipMemcpyAsync(dmask, bmask[b].data(), sizeof(unsigned) * nt, hipMemcpyHostToDevice, st));
            SCHK(hipMemcpyAsync(dwt, bwt[b].data(), sizeof(double) * nt, hipMemcpyHostToDevice, st));
        }
        SCHK(hipMemcpyAsync(dmem, mem.data(), sizeof(int) * sb, hipMemcpyHostToDevice, st));
        launch_block_sampler(dmask, dwt, nt, sb, dmem, N, n, (unsigned long long)seed, (int)b, den, dcdf, dS, st);
        SCHK(hipGetLastError());
        SCHK(hipStreamSynchronize(st)); // the staging buffers are reused by the next block
    }
#undef SCHK
    cleanup(0);
    return gml_create_from_device_bytes(p, dS, false, 0, nullptr, out, dedupe);
}

// Incidence lists of a term list (create_mcmc_terms, gml_problem_create_mcmc_terms_chains): for every spin the terms it belongs
// to, in term order (weight + the other spins; a spin named twice cancels, zero-weight terms are skipped).
using Incidences = std::vector<std::vector<std::pair<double, std::vector<int>>>>;
static int build_incidences(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, Incidences &inc) {
    inc.assign((size_t)n, {});
    for (int64_t t = 0; t < nterms; ++t) {
        if (!std::isfinite(weights[t])) return fail(GML_EINVAL, "weight of term %lld is not finite", (long long)t);
        std::vector<int> sp;
        for (int a = 0; a < key_stride; ++a) {
            const int32_t v = keys[t * key_stride + a];
            if (v < -1 || v >= n) return fail(GML_EINVAL, "term %lld names spin %d outside [0,%lld)", (long long)t, v, (long long)n);
            if (v < 0) continue;
            auto itv = std::find(sp.begin(), sp.end(), (int)v);
            if (itv != sp.end()) sp.erase(itv); // s^2 = 1
            else sp.push_back((int)v);
        }
        if (weights[t] == 0.0) continue;
        for (size_t a = 0; a < sp.size(); ++a) {
            std::vector<int> others;
            for (size_t b = 0; b < sp.size(); ++b)
                if (b != a) others.push_back(sp[b]);
            inc[(size_t)sp[a]].emplace_back(weights[t], std::move(others));
        }
    }
    return GML_OK;
}

static int create_mcmc_terms(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n, int64_t N, uint64_t seed,
                             int sweeps, int order, int64_t node0, int64_t node1, int device, gml_problem **out, bool dedupe) {
    if (!out) return fail(GML_EINVAL, "out is NULL");
    *out = nullptr;
    if ((nterms > 0 && (!keys || !weights)) || key_stride < 1) return fail(GML_EINVAL, "NULL or malformed term list");
    if (n <= 0 || N <= 0 || sweeps < 1) return fail(GML_EINVAL, "n, N and sweeps must be positive");
    if (order < 1 || order > 8) return fail(GML_EINVAL, "interaction order %d out of range [1,8]", order);
    if (node0 < 0 || node1 > n || node0 >= node1)
        return fail(GML_EINVAL, "bad node range [%lld,%lld) for n=%lld", (long long)node0, (long long)node1, (long long)n);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(GML_EHIP, "no HIP device available (libgml_hip has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(GML_EINVAL, "device %d out of range (%d devices)", device, ndev);
    Incidences inc;
    if (int rc = build_incidences(keys, key_stride, weights, nterms, n, inc)) return rc;
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
    HIPCHK(hipSetDevice(device));
    gml_problem *p = new gml_problem();
    p->device = device;
    p->n = n;
    p->K = N;
    p->M = (double)N;
    p->order = order;
    p->node0 = node0;
    p->node1 = node1;
    hipStream_t st = nullptr;
    const int64_t Np = round_up(N, 256);
    int8_t *dSt = nullptr;
    int *dioff = nullptr, *dooff = nullptr, *doth = nullptr;
    double *diw = nullptr;
    auto cleanup = [&](int rc) {
        void *ptrs[] = {dioff, dooff, doth, diw};
        for (void *q : ptrs)
            if (q) (void)dev_free(q);
        if (st) (void)hipStreamDestroy(st);
        return rc;
    };
#define SCHK(expr)                                                                                              \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) {                                                                                 \
            if (dSt) (void)dev_free(dSt);                                                                        \
            delete p;                                                                                           \
            return cleanup(fail(e_ == hipErrorOutOfMemory ? GML_ENOMEM : GML_EHIP, "%s failed: %s", #expr,      \
                                hipGetErrorString(e_)));                                                        \
        }                                                                                                       \
    } while (0)
    SCHK(hipStreamCreate(&st));
    SCHK(dev_malloc(&dSt, (size_t)n * Np));
    SCHK(dev_malloc(&dioff, sizeof(int) * ioff.size()));
    SCHK(dev_malloc(&dooff, sizeof(int) * ooff.size()));
    SCHK(dev_malloc(&doth, sizeof(int) * oth.size()));
    SCHK(dev_malloc(&diw, sizeof(double) * iw.size()));
    SCHK(hipMemcpyAsync(dioff, ioff.data(), sizeof(int) * ioff.size(), hipMemcpyHostToDevice, st));
    SCHK(hipMemcpyAsync(dooff, ooff.data(), sizeof(int) * ooff.size(), hipMemcpyHostToDevice, st));
    SCHK(hipMemcpyAsync(doth, oth.data(), sizeof(int) * oth.size(), hipMemcpyHostToDevice, st));
    SCHK(hipMemcpyAsync(diw, iw.data(), sizeof(double) * iw.size(), hipMemcpyHostToDevice, st));
    SCHK(hipMemsetAsync(dSt, 0, (size_t)n * Np, st));
    launch_glauber(dioff, diw, dooff, doth, n, N, Np, sweeps, (unsigned long long)seed, dSt, st);
    SCHK(hipGetLastError());
    SCHK(hipStreamSynchronize(st));
#undef SCHK
    cleanup(0);
    return gml_create_from_device_bytes(p, dSt, true, Np, nullptr, out, dedupe); // the chains' final states, spin-major
}

// gml_problem_create_mcmc_chains: Glauber chains of a dense pairwise model on the int8 matrix cores (gml_mcmc_chains.hip).  The
// model is quantised here, row by row: sigma_i = 2^(e - 38) with max_{j != i} |A_ij| < 2^e, q_ij = rint(A_ij / sigma_i), q_ii = 0,
// held in 5 balanced base-256 digit planes (include/gml.h).
extern "C" int gml_problem_create_mcmc_chains(const double *model, int64_t n, int64_t chains, int64_t samples_per_chain, int burn_in,
                                              int thin, uint64_t seed, int histogram, int order, int64_t node0, int64_t node1, int device,
                                              gml_problem **out) {
    if (!out) return fail(GML_EINVAL, "out is NULL");
    *out = nullptr;
    if (!model) return fail(GML_EINVAL, "model is NULL");
    if (n <= 0) return fail(GML_EINVAL, "n must be positive");
    if (chains < 1 || samples_per_chain < 1 || burn_in < 1 || thin < 1)
        return fail(GML_EINVAL, "chains, samples_per_chain, burn_in and thin must be at least 1");
    if (order < 1 || order > 8) return fail(GML_EINVAL, "interaction order %d out of range [1,8]", order);
    if (node0 < 0 || node1 > n || node0 >= node1)
        return fail(GML_EINVAL, "bad node range [%lld,%lld) for n=%lld", (long long)node0, (long long)node1, (long long)n);
    if (samples_per_chain > (int64_t)1 << 40 || chains > ((int64_t)1 << 40) / samples_per_chain)
        return fail(GML_EINVAL, "chains * samples_per_chain is too large");
    if ((int64_t)burn_in + (samples_per_chain - 1) * (int64_t)thin > INT32_MAX)
        return fail(GML_EINVAL, "burn_in + (samples_per_chain - 1) * thin exceeds 2^31 - 1 sweeps");
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j <= i; ++j) {
            const double v = model[i * n + j];
            if (!std::isfinite(v)) return fail(GML_EINVAL, "the model matrix is not finite at (%lld,%lld)", (long long)i, (long long)j);
            if (v != model[j * n + i])
                return fail(GML_EINVAL, "the model matrix is not symmetric at (%lld,%lld)", (long long)i, (long long)j);
        }
    const int64_t M = chains * samples_per_chain;
    if (n > kMcmcChainsMaxN || mcmc_chains_tile(n) == 0)
        return fail(GML_EUNSUPPORTED, "the int8 chain kernel supports n <= %lld spins (n = %lld)", (long long)kMcmcChainsMaxN, (long long)n);
    if (histogram && n > 64) return fail(GML_EUNSUPPORTED, "histogramming on the device needs n <= 64 spins (n = %lld)", (long long)n);
    if (histogram && M >= ((int64_t)1 << 31)) return fail(GML_EUNSUPPORTED, "histogramming on the device needs fewer than 2^31 samples");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(GML_EHIP, "no HIP device available (libgml_hip has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(GML_EINVAL, "device %d out of range (%d devices)", device, ndev);
    // quantisation; the digit planes pre-tiled as the kernel reads them: fragment (b, kt, l) = [64 lanes][16 B], lane (il, hh) byte t
    // = digit l of q[32 b + il][32 kt + 16 hh + t]
    const int64_t nb = (n + 31) / 32, np = 32 * nb;
    std::vector<int8_t> dg((size_t)(5 * np * np), 0);
    std::vector<double> qblk((size_t)(nb * 1024), 0.0), diag((size_t)np, 0.0), sig((size_t)np, 0.0), qsum((size_t)np, 0.0);
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
    HIPCHK(hipSetDevice(device));
    gml_problem *p = new gml_problem();
    p->device = device;
    p->n = n;
    p->K = M;
    p->M = (double)M;
    p->order = order;
    p->node0 = node0;
    p->node1 = node1;
    hipStream_t st = nullptr;
    const int64_t ld = round_up(M, 256);
    int8_t *dOut = nullptr, *dDg = nullptr;
    double *dq = nullptr, *dd = nullptr, *ds = nullptr, *dsum = nullptr;
    auto cleanup = [&](int rc) {
        void *ptrs[] = {dDg, dq, dd, ds, dsum};
        for (void *q : ptrs)
            if (q) (void)dev_free(q);
        if (st) (void)hipStreamDestroy(st);
        return rc;
    };
#define SCHK(expr)                                                                                              \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) {                                                                                 \
            if (dOut) (void)dev_free(dOut);                                                                      \
            delete p;                                                                                           \
            return cleanup(fail(e_ == hipErrorOutOfMemory ? GML_ENOMEM : GML_EHIP, "%s failed: %s", #expr,      \
                                hipGetErrorString(e_)));                                                        \
        }                                                                                                       \
    } while (0)
    SCHK(hipStreamCreate(&st));
    SCHK(dev_malloc(&dOut, (size_t)n * ld));
    SCHK(dev_malloc(&dDg, dg.size()));
    SCHK(dev_malloc(&dq, sizeof(double) * qblk.size()));
    SCHK(dev_malloc(&dd, sizeof(double) * np));
    SCHK(dev_malloc(&ds, sizeof(double) * np));
    SCHK(dev_malloc(&dsum, sizeof(double) * np));
    SCHK(hipMemcpyAsync(dDg, dg.data(), dg.size(), hipMemcpyHostToDevice, st));
    SCHK(hipMemcpyAsync(dq, qblk.data(), sizeof(double) * qblk.size(), hipMemcpyHostToDevice, st));
    SCHK(hipMemcpyAsync(dd, diag.data(), sizeof(double) * np, hipMemcpyHostToDevice, st));
    SCHK(hipMemcpyAsync(ds, sig.data(), sizeof(double) * np, hipMemcpyHostToDevice, st));
    SCHK(hipMemcpyAsync(dsum, qsum.data(), sizeof(double) * np, hipMemcpyHostToDevice, st));
    SCHK(hipMemsetAsync(dOut, 0, (size_t)n * ld, st));
    launch_mcmc_chains(dDg, dq, dd, ds, dsum, n, chains, burn_in, thin, (int)samples_per_chain, (unsigned long long)seed, dOut, ld, st);
    SCHK(hipGetLastError());
    SCHK(hipStreamSynchronize(st));
#undef SCHK
    cleanup(0);
    return gml_create_from_device_bytes(p, dOut, true, ld, nullptr, out, histogram != 0); // the recorded states, spin-major
}

// gml_problem_create_mcmc_terms_chains: thinned Glauber chains of any term list with exact integer fields (gml_term_chains.hip).
// The couplings of every spin are quantised here: sigma_i = 2^(E - 38) with max_e |w_e| < 2^E over its incidences with other spins,
// q_e = rint(w_e / sigma_i), and the incidences grouped by arity into the record stream of TermChainSpin (gml_dev.h).
extern "C" int gml_problem_create_mcmc_terms_chains(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                                    int64_t chains, int64_t samples_per_chain, int burn_in, int thin, uint64_t seed,
                                                    int histogram, int order, int64_t node0, int64_t node1, int device, gml_problem **out) {
    if (!out) return fail(GML_EINVAL, "out is NULL");
    *out = nullptr;
    if (!keys || !weights || key_stride < 1 || nterms < 0) return fail(GML_EINVAL, "NULL or malformed term list");
    if (n <= 0) return fail(GML_EINVAL, "n must be positive");
    if (chains < 1 || samples_per_chain < 1 || burn_in < 1 || thin < 1)
        return fail(GML_EINVAL, "chains, samples_per_chain, burn_in and thin must be at least 1");
    if (order < 1 || order > 8) return fail(GML_EINVAL, "interaction order %d out of range [1,8]", order);
    if (node0 < 0 || node1 > n || node0 >= node1)
        return fail(GML_EINVAL, "bad node range [%lld,%lld) for n=%lld", (long long)node0, (long long)node1, (long long)n);
    if (samples_per_chain > (int64_t)1 << 40 || chains > ((int64_t)1 << 40) / samples_per_chain)
        return fail(GML_EINVAL, "chains * samples_per_chain is too large");
    if ((int64_t)burn_in + (samples_per_chain - 1) * (int64_t)thin > INT32_MAX)
        return fail(GML_EINVAL, "burn_in + (samples_per_chain - 1) * thin exceeds 2^31 - 1 sweeps");
    for (int64_t t = 0; t < nterms; ++t) {
        if (!std::isfinite(weights[t])) return fail(GML_EINVAL, "weight of term %lld is not finite", (long long)t);
        for (int a = 0; a < key_stride; ++a) {
            const int32_t v = keys[t * key_stride + a];
            if (v < -1 || v >= n) return fail(GML_EINVAL, "term %lld names spin %d outside [0,%lld)", (long long)t, v, (long long)n);
        }
    }
    const int64_t M = chains * samples_per_chain;
    if (n > kMcmcChainsMaxN || term_chains_tile(n, chains) == 0)
        return fail(GML_EUNSUPPORTED, "the term-list chain kernel supports n <= %lld spins (n = %lld)", (long long)kMcmcChainsMaxN,
                    (long long)n);
    if (histogram && n > 64) return fail(GML_EUNSUPPORTED, "histogramming on the device needs n <= 64 spins (n = %lld)", (long long)n);
    if (histogram && M >= ((int64_t)1 << 31)) return fail(GML_EUNSUPPORTED, "histogramming on the device needs fewer than 2^31 samples");
    {   // the kernel's limits: distinct spins per term, incidences with other spins per spin
        std::vector<int64_t> cnt((size_t)n, 0);
        std::vector<int> sp;
        for (int64_t t = 0; t < nterms; ++t) {
            if (weights[t] == 0.0) continue;
            sp.clear();
            for (int a = 0; a < key_stride; ++a) {
                const int32_t v = keys[t * key_stride + a];
                if (v < 0) continue;
                auto itv = std::find(sp.begin(), sp.end(), (int)v);
                if (itv != sp.end()) sp.erase(itv);
                else sp.push_back((int)v);
            }
            if (sp.size() > (size_t)kTermChainsMaxOthers + 1)
                return fail(GML_EUNSUPPORTED, "term %lld names %zu distinct spins: the term-list chain kernel supports at most %d",
                            (long long)t, sp.size(), kTermChainsMaxOthers + 1);
            if (sp.size() > 1)
                for (int v : sp)
                    if (++cnt[(size_t)v] >= ((int64_t)1 << 24))
                        return fail(GML_EUNSUPPORTED, "spin %d has 2^24 or more incidences with other spins: the term-list chain kernel "
                                                      "supports fewer than 2^24", v);
        }
    }
    Incidences inc;
    if (int rc = build_incidences(keys, key_stride, weights, nterms, n, inc)) return rc;
    // per spin: a_i, sigma_i, Q_i and the records grouped by arity (q_e 2^24 + j_1 as two words, then j_2 .. j_k)
    std::vector<TermChainSpin> spin((size_t)n);
    std::vector<unsigned> rec;
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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(GML_EHIP, "no HIP device available (libgml_hip has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(GML_EINVAL, "device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));
    gml_problem *p = new gml_problem();
    p->device = device;
    p->n = n;
    p->K = M;
    p->M = (double)M;
    p->order = order;
    p->node0 = node0;
    p->node1 = node1;
    hipStream_t st = nullptr;
    const int64_t ld = round_up(M, 256);
    int8_t *dOut = nullptr;
    TermChainSpin *dspin = nullptr;
    unsigned *drec = nullptr;
    auto cleanup = [&](int rc) {
        if (dspin) (void)dev_free(dspin);
        if (drec) (void)dev_free(drec);
        if (st) (void)hipStreamDestroy(st);
        return rc;
    };
#define SCHK(expr)                                                                                              \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) {                                                                                 \
            if (dOut) (void)dev_free(dOut);                                                                      \
            delete p;                                                                                           \
            return cleanup(fail(e_ == hipErrorOutOfMemory ? GML_ENOMEM : GML_EHIP, "%s failed: %s", #expr,      \
                                hipGetErrorString(e_)));                                                        \
        }                                                                                                       \
    } while (0)
    SCHK(hipStreamCreate(&st));
    SCHK(dev_malloc(&dOut, (size_t)n * ld));
    SCHK(dev_malloc(&dspin, sizeof(TermChainSpin) * spin.size()));
    SCHK(dev_malloc(&drec, sizeof(unsigned) * rec.size()));
    SCHK(hipMemcpyAsync(dspin, spin.data(), sizeof(TermChainSpin) * spin.size(), hipMemcpyHostToDevice, st));
    SCHK(hipMemcpyAsync(drec, rec.data(), sizeof(unsigned) * rec.size(), hipMemcpyHostToDevice, st));
    SCHK(hipMemsetAsync(dOut, 0, (size_t)n * ld, st));
    launch_term_chains(dspin, drec, n, chains, burn_in, thin, (int)samples_per_chain, (unsigned long long)seed, dOut, ld, st);
    SCHK(hipGetLastError());
    SCHK(hipStreamSynchronize(st));
#undef SCHK
    cleanup(0);
    return gml_create_from_device_bytes(p, dOut, true, ld, nullptr, out, histogram != 0); // the recorded states, spin-major
}

extern "C" int gml_problem_create_mcmc_terms(const int32_t *keys, int key_stride, const double *weights, int64_t nterms,
                                             int64_t n, int64_t N, uint64_t seed, int sweeps, int order, int64_t node0,
                                             int64_t node1, int device, gml_problem **out) {
    return create_mcmc_terms(keys, key_stride, weights, nterms, n, N, seed, sweeps, order, node0, node1, device, out, false);
}

extern "C" int gml_problem_create_sampled_hist(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n,
                                               int64_t N, uint64_t seed, int mcmc_sweeps, int order, int64_t node0, int64_t node1,
                                               int device, gml_problem **out) {
    if (n > 64) return fail(GML_EUNSUPPORTED, "histogramming on the device needs n <= 64 spins (n = %lld)", (long long)n);
    if (mcmc_sweeps > 0) return create_mcmc_terms(keys, key_stride, weights, nterms, n, N, seed, mcmc_sweeps, order, node0, node1, device, out, true);
    return create_sampled_terms(keys, key_stride, weights, nterms, n, N, seed, order, node0, node1, device, out, true);
}

extern "C" int gml_problem_get_counts(gml_problem *p, double *counts) {
    if (!p || !counts) return fail(GML_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipMemcpyAsync(counts, p->d.w, sizeof(double) * p->K, hipMemcpyDeviceToHost, p->st));
    HIPCHK(hipStreamSynchronize(p->st));
    for (int64_t k = 0; k < p->K; ++k) counts[k] = std::nearbyint(counts[k] * p->M * 1e6) / 1e6; // w_k = counts_k / M (:170)
    return GML_OK;
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
    // the matrix as terms: 1/2 s^T A s = sum_{i<j} A_ij s_i s_j (sampling.jl:40), prior = diagonal (:41)
    std::vector<int32_t> keys;
    std::vector<double> wts;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j <= i; ++j) {
            const double v = model[i * n + j];
            if (j < i && v != model[j * n + i])
                return fail(GML_EINVAL, "the model matrix is not symmetric at (%lld,%lld)", (long long)i, (long long)j);
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

