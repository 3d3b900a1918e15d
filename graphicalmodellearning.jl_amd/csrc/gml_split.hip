// Splitting a resident handle into folds (gml_problem_fold_sizes, gml_problem_split; include/gml.h).
//
// The handle's M samples are its units: row k with count c_k = rint(w_k M) owns the units C_k .. C_k + c_k - 1 (C = exclusive
// prefix sum of the counts), and unit g lies in fold min(nfolds - 1, floor(nfolds u01(seed, kU01FoldStream, g))).  A part of the
// split (one fold, or everything but one fold) is the rows with a positive new count c'_k, in source order: a stream compaction
// of the bit-packed samples Sb [n][Kp / 32].
//   k_counts         c_k from the weights                               (hipCUB exclusive sum -> C_k)
//   k_fold_counts    one wave per row, lanes stride over its units      -> c'_k, or the nfolds totals
//   k_keep_flags     [c'_k > 0]                                         (hipCUB exclusive sum -> position k' of every kept row)
//   k_write_src      src[k'] = k, counts'[k'] = c'_k
//   k_gather_bits    Sb'[i][k'] = Sb[i][src[k']]: a wave owns 64 output rows and ballots one spin's 64 bits at a time
// Everything is integer arithmetic on a hash of the unit's index: no result depends on the grid, the block size or the order of a
// reduction.
#include "../../include/gml.h"
#include "gml_internal.h"
#include "gml_rng.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

namespace gml {

__device__ __forceinline__ int fold_of_unit(unsigned long long seed, unsigned long long g, int nfolds) {
    const int f = (int)((double)nfolds * u01(seed, kU01FoldStream, g));
    return f < nfolds - 1 ? f : nfolds - 1;
}

// c_k = rint(w_k M) (exact for integer counts and M <= 2^50: gml.h, the moments' contract); c [K + 1], c[K] = 0 so that the
// exclusive sum over K + 1 items leaves M in C[K]
__global__ __launch_bounds__(256) void k_counts(const double *__restrict__ w, double M, int64_t K, unsigned long long *__restrict__ c) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > K) return;
    c[k] = k < K ? (unsigned long long)rint(w[k] * M) : 0ull;
}

// One wave per row k at a time: lane l looks at the units C_k + l, C_k + l + 64, ...
//   SIZES = false: cnew[k] = number of the row's units in fold `fold` (complement: outside it) -- the ballot's population count is
//                  already the wave's sum, every lane holds it
//   SIZES = true : totals[f] += the row's units in fold f, through a per-wave LDS histogram (integer atomics: any order, same sum)
template <bool SIZES>
__global__ __launch_bounds__(256) void k_fold_counts(const unsigned long long *__restrict__ c, const unsigned long long *__restrict__ C,
                                                     int64_t K, int nfolds, unsigned long long seed, int fold, int complement,
                                                     unsigned long long *__restrict__ cnew, unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long hist[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (SIZES) hist[wv][lane] = 0ull;
    __syncthreads();
    // (the rows of a wave: a grid-stride loop, so that the sizes cost one global atomic per fold and WORKGROUP, not per row)
    for (int64_t k = (int64_t)blockIdx.x * 4 + wv; k < K; k += (int64_t)gridDim.x * 4) {
        const unsigned long long ck = c[k], g0 = C[k];
        unsigned long long held = 0ull;
        for (unsigned long long t = 0; t < ck; t += 64) { // (wave-uniform trip count)
            const bool in = t + lane < ck;
            const int f = in ? fold_of_unit(seed, g0 + t + lane, nfolds) : -1;
            if (SIZES) {
                if (in) atomicAdd(&hist[wv][f], 1ull);
            } else {
                held += (unsigned long long)__popcll(__ballot(f == fold));
            }
        }
        if (!SIZES && lane == 0) cnew[k] = complement ? ck - held : held;
    }
    if (SIZES) {
        __syncthreads();
        if (wv == 0 && lane < nfolds) {
            const unsigned long long s = hist[0][lane] + hist[1][lane] + hist[2][lane] + hist[3][lane];
            if (s) atomicAdd(&totals[lane], s);
        }
    }
}

// keep [K + 1]: 1 where the row survives; keep[K] = 0 so that the exclusive sum over K + 1 items leaves K' in pos[K]
__global__ __launch_bounds__(256) void k_keep_flags(const unsigned long long *__restrict__ cnew, int64_t K, int *__restrict__ keep) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > K) return;
    keep[k] = (k < K && cnew[k] != 0ull) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_write_src(const unsigned long long *__restrict__ cnew, const int *__restrict__ pos, int64_t K,
                                                   int *__restrict__ src, unsigned long long *__restrict__ cout) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K || cnew[k] == 0ull) return;
    src[pos[k]] = (int)k;
    cout[pos[k]] = cnew[k];
}

// The compaction of the sign bits.  A workgroup of 16 waves covers the 1024 consecutive output rows [1024 b, 1024 b + 1024) (Kp' is a
// multiple of 1024: no partial workgroup), wave v the 64 rows from 1024 b + 64 v; lane l keeps the source row of output row
// 1024 b + 64 v + l.  For a spin i every lane reads the source word that holds its row's bit (neighbouring lanes read the same or
// the next few words) and the wave's ballot is the 64 output bits = output words 32 b + 2 v, 32 b + 2 v + 1 of row i.  Lane s keeps
// the ballot of spin s of the current chunk of 64 spins; the 16 waves then put their 64 x 8 bytes into LDS and the workgroup writes,
// for every spin of the chunk, the 128 contiguous bytes of its 32 words: one whole line per (workgroup, spin), where a store per
// (wave, spin) would leave each line to 16 waves.  LDS rows are padded to 34 words: the 64-bit writes of one wave (lane = spin) and
// the 32-bit reads (32 consecutive lanes = one spin's words) are both conflict free.
// The spins [s0, s1) of a workgroup: blockIdx.x = b * nsplit + part (rows outermost in x; no grid.y).
constexpr int kGatherChunk = 64;
constexpr int kGatherPitch = 34; // words per LDS row (32 + 2)
__global__ __launch_bounds__(1024) void k_gather_bits(const unsigned *__restrict__ Sb, int64_t wpr_src, const int *__restrict__ src,
                                                      int64_t Kout, int64_t n, int64_t wpr_out, int nsplit, int64_t spins_per_part,
                                                      unsigned *__restrict__ Sb_out) {
    __shared__ __attribute__((aligned(8))) unsigned stage[kGatherChunk * kGatherPitch];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t b = (int64_t)blockIdx.x / nsplit;
    const int part = (int)((int64_t)blockIdx.x % nsplit);
    const int64_t row = b * 1024 + tid;
    const bool valid = row < Kout;
    const int sk = valid ? src[row] : 0; // (padding rows read row 0 and drop the bit)
    const unsigned *base = Sb + (sk >> 5);
    const int sh = sk & 31;
    const int64_t s0 = (int64_t)part * spins_per_part;
    const int64_t s1 = s0 + spins_per_part < n ? s0 + spins_per_part : n;
    for (int64_t i0 = s0; i0 < s1; i0 += kGatherChunk) {
        unsigned long long mine = 0ull;
        // eight loads in flight per lane, none behind a branch: spins past s1 re-read spin s1 - 1 and padding rows row 0, and
        // their bits are dropped by the mask
        for (int s8 = 0; s8 < kGatherChunk; s8 += 8) {
            unsigned wds[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int64_t i = i0 + s8 + j;
                wds[j] = base[(i < s1 ? i : s1 - 1) * wpr_src];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool on = valid && i0 + s8 + j < s1 && ((wds[j] >> sh) & 1u) != 0u;
                const unsigned long long m = __ballot(on);
                if (lane == s8 + j) mine = m;
            }
        }
        // lane s of wave v: words 2 v, 2 v + 1 of LDS row s
        *reinterpret_cast<unsigned long long *>(&stage[lane * kGatherPitch + 2 * wv]) = mine;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int idx = r * 1024 + tid, s = idx >> 5, wd = idx & 31;
            const int64_t i = i0 + s;
            if (i < s1) Sb_out[i * wpr_out + b * 32 + wd] = stage[s * kGatherPitch + wd];
        }
        __syncthreads();
    }
}

void launch_gather_bits(const unsigned *Sb, int64_t Kp_src, const int *src, int64_t Kout, int64_t n, int64_t Kp_out, unsigned *Sb_out,
                        hipStream_t st) {
    const int64_t nblk = Kp_out / 1024, chunks = (n + kGatherChunk - 1) / kGatherChunk;
    // enough workgroups to fill the device when the part has few rows: the spins are cut into `nsplit` runs of whole chunks
    int64_t nsplit = nblk >= 1024 ? 1 : (1024 + nblk - 1) / nblk;
    if (nsplit > chunks) nsplit = chunks;
    const int64_t per = (chunks + nsplit - 1) / nsplit * kGatherChunk;
    nsplit = (n + per - 1) / per;
    hipLaunchKernelGGL(k_gather_bits, dim3((unsigned)(nblk * nsplit)), dim3(1024), 0, st, Sb, Kp_src / 32, src, Kout, n, Kp_out / 32,
                       (int)nsplit, per, Sb_out);
}

namespace {
// device blocks of one call: freed on every path
struct SplitBlocks {
    std::vector<void *> blocks;
    ~SplitBlocks() {
        for (void *q : blocks)
            if (q) (void)dev_free(q);
    }
    template <class T> hipError_t alloc(T **out, size_t count) {
        const hipError_t e = dev_malloc(out, sizeof(T) * (count ? count : 1));
        if (e == hipSuccess) blocks.push_back(*out);
        return e;
    }
    void release(void *q) { // the block passes to somebody else
        for (void *&b : blocks)
            if (b == q) b = nullptr;
    }
};

unsigned fold_counts_grid(int64_t K) { return (unsigned)std::min<int64_t>((K + 3) / 4, 8192); } // 4 rows per workgroup and step

template <class T> int exclusive_sum(SplitBlocks &sb, const T *in, T *out, int64_t items, hipStream_t st) {
    size_t tb = 0;
    char *tmp = nullptr;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)items, st));
    HIPCHK(sb.alloc(&tmp, tb));
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, in, out, (int)items, st));
    return GML_OK;
}

// (the argument errors of both entry points come first, then what the handle cannot do; all of it before any device work)
int check_fold_args(int nfolds, int fold) {
    if (nfolds < 2 || nfolds > 64) return fail(GML_EINVAL, "nfolds = %d outside [2, 64]", nfolds);
    if (fold < 0 || fold >= nfolds) return fail(GML_EINVAL, "fold = %d outside [0, %d)", fold, nfolds);
    return GML_OK;
}
int check_split_handle(const gml_problem *p) {
    if (!p->counts_int) return fail(GML_EUNSUPPORTED, "the handle was created with a fractional count: folds are drawn per sample and need integer counts");
    if (!(p->M < 1099511627776.0)) return fail(GML_EUNSUPPORTED, "the sum of the counts M = %.17g reaches 2^40: the split works per sample", p->M);
    if (p->K >= ((int64_t)1 << 31) - 1) return fail(GML_EUNSUPPORTED, "splitting a handle needs fewer than 2^31 - 1 rows");
    return GML_OK;
}

// c [K + 1] and C [K + 1] of the handle, on its stream
int unit_ranges(gml_problem *p, SplitBlocks &sb, unsigned long long **c, unsigned long long **C) {
    const int64_t K = p->K;
    HIPCHK(sb.alloc(c, (size_t)K + 1));
    HIPCHK(sb.alloc(C, (size_t)K + 1));
    hipLaunchKernelGGL(k_counts, dim3((unsigned)((K + 256) / 256)), dim3(256), 0, p->st, p->d.w, p->M, K, *c);
    HIPCHK(hipGetLastError());
    return exclusive_sum(sb, *c, *C, K + 1, p->st);
}
} // namespace

} // namespace gml

using namespace gml;

extern "C" int gml_problem_fold_sizes(gml_problem *p, int nfolds, uint64_t seed, int64_t *sizes) {
    if (!p || !sizes) return fail(GML_EINVAL, "NULL argument");
    if (int rc = check_fold_args(nfolds, 0)) return rc;
    if (int rc = check_split_handle(p)) return rc;
    HIPCHK(hipSetDevice(p->device));
    SplitBlocks sb;
    unsigned long long *c = nullptr, *C = nullptr, *tot = nullptr;
    if (int rc = unit_ranges(p, sb, &c, &C)) return rc;
    HIPCHK(sb.alloc(&tot, 64));
    HIPCHK(hipMemsetAsync(tot, 0, sizeof(unsigned long long) * 64, p->st));
    hipLaunchKernelGGL(k_fold_counts<true>, dim3(fold_counts_grid(p->K)), dim3(256), 0, p->st, c, C, p->K, nfolds, (unsigned long long)seed, 0,
                       0, (unsigned long long *)nullptr, tot);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sizes, tot, sizeof(int64_t) * nfolds, hipMemcpyDeviceToHost, p->st));
    HIPCHK(hipStreamSynchronize(p->st));
    return GML_OK;
}

extern "C" int gml_problem_split(gml_problem *p, int nfolds, int fold, uint64_t seed, int complement, gml_problem **out) {
    if (!p || !out) return fail(GML_EINVAL, "NULL argument");
    *out = nullptr;
    if (int rc = check_fold_args(nfolds, fold)) return rc;
    if (int rc = check_split_handle(p)) return rc;
    const double t_begin = gml_now_s();
    HIPCHK(hipSetDevice(p->device));
    const int64_t K = p->K;
    SplitBlocks sb;
    unsigned long long *c = nullptr, *C = nullptr, *cnew = nullptr, *cout = nullptr;
    int *keep = nullptr, *pos = nullptr, *src = nullptr;
    if (int rc = unit_ranges(p, sb, &c, &C)) return rc;
    HIPCHK(sb.alloc(&cnew, (size_t)K));
    HIPCHK(sb.alloc(&keep, (size_t)K + 1));
    HIPCHK(sb.alloc(&pos, (size_t)K + 1));
    hipLaunchKernelGGL(k_fold_counts<false>, dim3(fold_counts_grid(K)), dim3(256), 0, p->st, c, C, K, nfolds, (unsigned long long)seed, fold,
                       complement ? 1 : 0, cnew, (unsigned long long *)nullptr);
    hipLaunchKernelGGL(k_keep_flags, dim3((unsigned)((K + 256) / 256)), dim3(256), 0, p->st, cnew, K, keep);
    HIPCHK(hipGetLastError());
    if (int rc = exclusive_sum(sb, keep, pos, K + 1, p->st)) return rc;
    int Kn = 0;
    HIPCHK(hipMemcpyAsync(&Kn, pos + K, sizeof(int), hipMemcpyDeviceToHost, p->st));
    HIPCHK(hipStreamSynchronize(p->st));
    if (Kn <= 0)
        return fail(GML_EINVAL, "%sfold %d of %d (seed %llu) holds none of the handle's %.0f samples", complement ? "the complement of " : "", fold, nfolds,
                    (unsigned long long)seed, p->M);
    HIPCHK(sb.alloc(&src, (size_t)Kn));
    HIPCHK(sb.alloc(&cout, (size_t)Kn));
    hipLaunchKernelGGL(k_write_src, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, p->st, cnew, pos, K, src, cout);
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> hc((size_t)Kn);
    HIPCHK(hipMemcpyAsync(hc.data(), cout, sizeof(unsigned long long) * Kn, hipMemcpyDeviceToHost, p->st));
    // the new sign bits, at the new handle's own pitch; zeroed first: rows >= K' and the padding words stay 0
    const int64_t Kpn = gml_round_up(Kn, 1024);
    unsigned *Sbn = nullptr;
    HIPCHK(sb.alloc(&Sbn, (size_t)p->n * (size_t)(Kpn / 32)));
    HIPCHK(hipMemsetAsync(Sbn, 0, (size_t)p->n * (size_t)(Kpn / 8), p->st));
    HIPCHK(hipStreamSynchronize(p->st)); // (so that the time below is the compaction's alone)
    const double t_gather = gml_now_s();
    launch_gather_bits(p->d.Sb, p->d.Kp, src, Kn, p->n, Kpn, Sbn, p->st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->st)); // the new handle has a stream of its own
    std::vector<double> counts((size_t)Kn);
    double Mn = 0;
    for (int64_t k = 0; k < Kn; ++k) Mn += (counts[(size_t)k] = (double)hc[(size_t)k]);
    gml_problem *q = gml_new_problem(Kn, p->n, Mn, p->order, p->node0, p->node1, p->device);
    const double t_tail = gml_now_s();
    sb.release(Sbn); // owned by gml_create_from_device_bits from here on
    if (int rc = gml_create_from_device_bits(q, Sbn, counts.data(), out)) return rc;
    // gml_problem_ingest_times of a part: [0] fold counts, scans and the index list, [1] the compaction kernel, [2] the bit images
    (*out)->t_ingest[0] = t_gather - t_begin;
    (*out)->t_ingest[1] = t_tail - t_gather;
    (*out)->t_ingest[3] = gml_now_s() - t_begin;
    return GML_OK;
}
