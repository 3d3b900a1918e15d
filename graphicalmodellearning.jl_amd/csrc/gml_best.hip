// The k most probable states of one connected component by streaming enumeration (gml_model_best_states, include/gml.h).
// Steps 1 and 2 of k_exact_enumerate (gml_exact.hip), unchanged: the chunk's coefficient vector, then passes A, B, C of the
// Walsh-Hadamard transform, after which thread tid holds the energies of the states tid + 256 e of the chunk in x[e].  No exp and no
// second transform: the energies are selected, not summed.
//   k = 1: every thread keeps its best (energy, state) in registers -- strict > while the states ascend, so the lower state keeps a
//     tie -- and the group ends with one arg-max over the workgroup.  No list, no work per chunk beyond the 16 compares.
//   k > 1: the group keeps its k best pairs in LDS, sorted (energy descending, state ascending), and tau = the energy of the k-th
//     (-inf while the list is short).  The chunks of a group ascend, so every state of a chunk is above every state in the list, and a
//     state enters iff its energy is > tau.  A chunk whose maximum is not > tau costs one block_max.  One that is compacts its
//     qualifying states by a prefix sum into the transform's vector (free at that point), sorts them (a bitonic network over the next
//     power of two >= their number, <= 4096), and merges the best k of them with the list (one bitonic merge of 512).  The sort's key
//     (energy, state) is a total order, so the list after a chunk is a function of the list before and the chunk's energies only.
// With c < kExactChunkBits low bits the bits from c up are in no term: only the states below 2^c are candidates.
// Group g writes its list to ge / gs [g][k] (short lists padded with -inf / ~0); the host cuts the G k candidates to k.
#include "../../include/gml.h"
#include "gml_dev.h"
#include "gml_exact_wht.h"
#include "gml_wg.h"

namespace gml {

namespace {
constexpr unsigned long long kNoState = ~0ull;

// the bitonic compare-exchange of slots i < l: the earlier of the two to slot i if first, else to slot l
template <class Idx>
__device__ __forceinline__ void best_exchange(double *e, Idx *s, int i, int l, bool first) {
    const double a = e[i], b = e[l];
    const Idx sa = s[i], sb = s[l];
    if (best_before(b, sb, a, sa) == first) {
        e[i] = b;
        e[l] = a;
        s[i] = sb;
        s[l] = sa;
    }
}
} // namespace

template <bool kOne>
__global__ __launch_bounds__(256) void k_exact_best(const ExactPlan P, const int c, const int kk, double *__restrict__ ge,
                                                    unsigned long long *__restrict__ gs) {
    __shared__ double v[kExactVec], part[kExactParts], red[4];
    __shared__ double le[kBestMax];             // the group's list (k = 1: the threads' bests at the end)
    __shared__ unsigned long long ls[kBestMax];
    __shared__ unsigned short ci[1 << kExactChunkBits]; // the chunk states of the compacted energies
    __shared__ int wsum[4];
    const int tid = threadIdx.x;
    const int baseA = 17 * tid, baseB = (tid & 15) + 272 * (tid >> 4), baseC = (tid & 15) + 17 * (tid >> 4);
    const int nlow = 1 << c;
    double x[16];
    double be = -INFINITY; // k = 1: this thread's best
    unsigned long long bs = kNoState;
    int len = 0;            // k > 1: entries in the list and the energy to beat (the same in every thread)
    double tau = -INFINITY;
    for (long long k = 0; k < P.cpg; ++k) {
        const unsigned long long h = (unsigned long long)blockIdx.x * (unsigned long long)P.cpg + (unsigned long long)k;
        __syncthreads(); // (the chunk before has read v)
#pragma unroll
        for (int e = 0; e < 16; ++e) v[baseA + e] = 0.0;
        __syncthreads();
        // 1. the coefficient vector: items in term order; the only item of a low mask writes its slot, the others a partial sum
        for (int it = tid; it < P.ni; it += 256) {
            double s = 0.0;
            for (int t = P.item_off[it], t1 = P.item_off[it + 1]; t < t1; ++t) s += (__popcll(P.hi[t] & h) & 1) ? -P.w[t] : P.w[t];
            const int dst = P.item_dst[it];
            if (dst >= 0) v[dst] = s;
            else part[~dst] = s;
        }
        if (P.nm) {
            __syncthreads();
            for (int s = tid; s < P.nm; s += 256) { // (at most kExactParts partial sums in all)
                double sum = 0.0;
                for (int a = P.ms_off[s], a1 = P.ms_off[s + 1]; a < a1; ++a) sum += part[a];
                v[P.ms_dst[s]] = sum;
            }
        }
        __syncthreads();
        // 2. energies of the chunk's states: passes A, B, C; the last stays in registers (x[e]: state tid + 256 e)
        exact_load(v, baseA, 1, x);
        wht16(x);
        exact_store(v, baseA, 1, x);
        __syncthreads();
        exact_load(v, baseB, 17, x);
        wht16(x);
        exact_store(v, baseB, 17, x);
        __syncthreads();
        exact_load(v, baseC, 272, x);
        wht16(x);
        if constexpr (kOne) {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (tid + 256 * e < nlow && x[e] > be) {
                    be = x[e];
                    bs = (h << c) | (unsigned long long)(tid + 256 * e);
                }
        } else {
            double mx = -INFINITY;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (tid + 256 * e < nlow) mx = fmax(mx, x[e]);
            if (!(block_max(mx, red) > tau)) continue; // (the same in every thread; every thread is past its reads of v)
            // 3. the qualifying states, compacted in state order: v[0 .. q) and ci[0 .. q)
            int cnt = 0;
#pragma unroll
            for (int e = 0; e < 16; ++e) cnt += tid + 256 * e < nlow && x[e] > tau;
            int incl = cnt;
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o);
                if ((tid & 63) >= o) incl += up;
            }
            if ((tid & 63) == 63) wsum[tid >> 6] = incl;
            __syncthreads();
            int at = incl - cnt, q = 0;
            for (int wv = 0; wv < 4; ++wv) {
                if (wv < (tid >> 6)) at += wsum[wv];
                q += wsum[wv];
            }
            int pn = 1;
            while (pn < q) pn <<= 1;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (tid + 256 * e < nlow && x[e] > tau) {
                    v[at] = x[e];
                    ci[at] = (unsigned short)(tid + 256 * e);
                    ++at;
                }
            for (int i = q + tid; i < pn; i += 256) {
                v[i] = -INFINITY;
                ci[i] = 0xFFFFu;
            }
            __syncthreads();
            // 4. sorted, best first: a bitonic network over pn <= 4096 slots
            for (int k2 = 2; k2 <= pn; k2 <<= 1)
                for (int j = k2 >> 1; j > 0; j >>= 1) {
                    for (int t = tid; t < (pn >> 1); t += 256) {
                        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                        best_exchange(v, ci, i, i | j, (i & k2) == 0);
                    }
                    __syncthreads();
                }
            // 5. the best min(q, k) of them and the list, one against the other: candidates descending in slots 0 .. 255, the list
            // ascending in 256 .. 511, the unused slots between them last in the order -- a bitonic sequence, merged in 9 steps
            const int qk = q < kk ? q : kk;
            const double cand_e = tid < qk ? v[tid] : -INFINITY, list_e = tid < len ? le[tid] : -INFINITY;
            const unsigned long long cand_s = tid < qk ? (h << c) | (unsigned long long)ci[tid] : kNoState;
            const unsigned long long list_s = tid < len ? ls[tid] : kNoState;
            __syncthreads();
            double *me = v;
            unsigned long long *ms = reinterpret_cast<unsigned long long *>(v + 2 * kBestMax);
            me[tid] = cand_e;
            ms[tid] = cand_s;
            me[2 * kBestMax - 1 - tid] = list_e;
            ms[2 * kBestMax - 1 - tid] = list_s;
            __syncthreads();
            for (int j = kBestMax; j > 0; j >>= 1) {
                const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1));
                best_exchange(me, ms, i, i | j, true);
                __syncthreads();
            }
            le[tid] = me[tid];
            ls[tid] = ms[tid];
            len = len + qk < kk ? len + qk : kk;
            __syncthreads();
            tau = len == kk ? le[kk - 1] : -INFINITY;
        }
    }
    if constexpr (kOne) {
        best_of_block(be, bs, le, ls);
        if (tid == 0) {
            ge[blockIdx.x] = be;
            gs[blockIdx.x] = bs;
        }
    } else if (tid < kk) {
        ge[(size_t)blockIdx.x * kk + tid] = tid < len ? le[tid] : -INFINITY;
        gs[(size_t)blockIdx.x * kk + tid] = tid < len ? ls[tid] : kNoState;
    }
}

void launch_exact_best(const ExactPlan &P, int G, int c, int k, double *dge, unsigned long long *dgs, hipStream_t st) {
    if (k == 1) hipLaunchKernelGGL(k_exact_best<true>, dim3((unsigned)G), dim3(256), 0, st, P, c, k, dge, dgs);
    else hipLaunchKernelGGL(k_exact_best<false>, dim3((unsigned)G), dim3(256), 0, st, P, c, k, dge, dgs);
}

} // namespace gml
