// What the creators of sampled handles share on the host: gml_sampled.cpp (exact block sampler, k_glauber, the int8 chains, moments,
// gml_model_exact), gml_chains_host.cpp (the term-list chain family) and gml_cond_exact.cpp (exact conditional inference).  Internal;
// not part of the C ABI.
#pragma once
#include "gml_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

namespace gml {

// ------------------------------------------------------------------------------------------
// Argument checks shared by the creators.  All of them come before the device lookup (gml_check_device), so a bad argument
// is GML_EINVAL / GML_EUNSUPPORTED on every machine, with or without a GPU.
// ------------------------------------------------------------------------------------------
int check_out(gml_problem **out);
// Terms of one model: spins of term t = keys[t*stride .. +stride) (0-based, -1 = unused slot).  strict (the term chains): NULL
// pointers and a negative count are refused for an empty list too.
int check_term_pointers(const int32_t *keys, int stride, const double *weights, int64_t nterms, bool strict = false);
int check_term_values(const int32_t *keys, int stride, const double *weights, int64_t nterms, int64_t n);
// the shape of a run of thinned chains; the handle arguments sit where both chain creators have always checked them
int check_chain_args(int64_t n, int64_t chains, int64_t samples_per_chain, int burn_in, int thin, int order, int64_t node0, int64_t node1);
int check_hist_limits(int64_t n, int64_t M);

// The distinct spins of one key after cancellation (a spin named twice cancels: s^2 = 1), in the order that fixes the record stream
// of the term chains and the FP64 summation order of k_glauber.  Returns a spin the key names (cancelled or not), -1 for the empty key.
int reduce_key(const int32_t *key, int stride, std::vector<int> &sp);

// Incidence lists of a term list (create_mcmc_terms, the term-list chains): for every spin the terms it belongs to, in term order
// (weight + the other spins; a spin named twice cancels, zero-weight terms are skipped).
using Incidences = std::vector<std::vector<std::pair<double, std::vector<int>>>>;
Incidences build_incidences(const int32_t *keys, int key_stride, const double *weights, int64_t nterms, int64_t n);

// ------------------------------------------------------------------------------------------
// What a creator holds on the device while its sampler runs: the stream, the handle under construction, the sampler's output bytes
// and every temporary buffer.  begin, upload / alloc, the launches, finish; the destructor frees whatever finish has not handed on,
// on every path.  The first failed call is kept in rc (codes and texts as HIPCHK) and makes the later ones no-ops.
// ------------------------------------------------------------------------------------------
struct SamplerStaging {
    hipStream_t st = nullptr;
    gml_problem *p = nullptr;
    int8_t *out = nullptr; // the draws as +-1 bytes
    std::vector<void *> tmp;
    int rc = GML_OK;

    SamplerStaging() = default;
    SamplerStaging(const SamplerStaging &) = delete;
    SamplerStaging &operator=(const SamplerStaging &) = delete;
    ~SamplerStaging() {
        release();
        if (out) (void)dev_free(out);
        delete p;
    }
    bool ok(hipError_t e, const char *call) {
        if (rc == GML_OK && e != hipSuccess)
            rc = fail(e == hipErrorOutOfMemory ? GML_ENOMEM : GML_EHIP, "%s failed: %s", call, hipGetErrorString(e));
        return rc == GML_OK;
    }
    // no handle (gml_log_partition_ais): the device and a stream for upload / alloc / sync; the destructor releases as always
    int open(int device) {
        if (ok(hipSetDevice(device), "hipSetDevice")) ok(hipStreamCreate(&st), "hipStreamCreate");
        return rc;
    }
    // the handle's K rows of n spins; out_bytes of output, cleared if the sampler does not write all of them
    int begin(int device, int64_t K, int64_t n, int order, int64_t node0, int64_t node1, size_t out_bytes, bool clear) {
        if (!ok(hipSetDevice(device), "hipSetDevice")) return rc;
        p = gml_new_problem(K, n, (double)K, order, node0, node1, device);
        if (ok(hipStreamCreate(&st), "hipStreamCreate") && ok(dev_malloc(&out, out_bytes), "dev_malloc") && clear)
            ok(hipMemsetAsync(out, 0, out_bytes, st), "hipMemsetAsync");
        return rc;
    }
    template <class T> T *alloc(size_t count) {
        T *d = nullptr;
        if (rc != GML_OK || !ok(dev_malloc(&d, sizeof(T) * count), "dev_malloc")) return nullptr;
        tmp.push_back(d);
        return d;
    }
    template <class T> void copy(T *dst, const std::vector<T> &v) {
        if (rc == GML_OK && !v.empty()) ok(hipMemcpyAsync(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
    }
    template <class T> T *upload(const std::vector<T> &v) {
        T *d = alloc<T>(v.size());
        copy(d, v);
        return rc == GML_OK ? d : nullptr;
    }
    // after the launches: their errors, and the stream drained (the host vectors behind the uploads may go)
    int sync() {
        if (ok(hipGetLastError(), "the sampler's launch")) ok(hipStreamSynchronize(st), "hipStreamSynchronize");
        return rc;
    }
    void release() {
        for (void *q : tmp) (void)dev_free(q);
        tmp.clear();
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
    }
    // the handle from the output bytes (sample-major [K][n] or, spin_major, [n][ld]); gml_create_from_device_bytes owns both from here
    int finish(bool spin_major, int64_t ld, bool dedupe, gml_problem **result) {
        if (sync()) return rc;
        release();
        gml_problem *q = p;
        int8_t *bytes = out;
        p = nullptr;
        out = nullptr;
        return gml_create_from_device_bytes(q, bytes, spin_major, ld, nullptr, result, dedupe);
    }
};

} // namespace gml
