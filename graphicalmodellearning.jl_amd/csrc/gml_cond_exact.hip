// Exact conditional inference by enumeration of every row's hidden spins (gml_conditional_exact, gml_conditional_exact_masked,
// include/gml.h).  One workgroup of 256 threads takes a job (plan, row) -- a plan is one hidden set of h <= 24 spins --
// from the row's sign bits to log sum_{s_H} exp E_k(s_H), the conditional means of the hidden spins and the energy of the state the
// row itself holds on them:
//   row phase, once per row.  The row's n sign bits are gathered into LDS.  Every term is (sign of its visible spins in this row) x
//     (its hidden part, a mask over the h local bits): the signed weights are summed per hidden part into the row's coefficients
//     (the host has sorted the terms by hidden part and cut every part's run into items of at most L terms, so every sum has a fixed
//     order; no atomics).  The coefficient of the empty part is the row's constant.  This is the only step that costs T.
//   chunk phase, 2^(h - c) times.  The c low local bits form a chunk; at the setting hv of the high bits every coefficient is (sign of
//     its high part at hv) x (a mask over the low bits).  From there on it is the pipeline of k_exact_enumerate (gml_exact.hip), the
//     same arithmetic in the same order: coefficients -> Walsh-Hadamard transform -> energies -> exp(E - m) under the running maximum ->
//     Walsh-Hadamard transform -> S[mask] for every low mask at once.  The picks are S[0] and the h singletons; a singleton of a high
//     bit is S[0] with the sign of that bit in hv.  1024 chunks go into a first accumulator and those into a second; a row has at most
//     4096 chunks, so its workgroup finishes it and nothing is combined across workgroups.
// A row of c < kExactChunkBits chunk bits runs the same transforms: the bits above c belong to no coefficient, every sum over them is
// an exact doubling, and the factor 2^(kExactChunkBits - c) is taken out of the sum again before its logarithm.
// The result of a row is a function of the model, the row's bits and the plan alone: not of the job's place, the grid or the other rows.
// The same kernel, compiled in two more forms, selects the row's most probable hidden state instead of (or beside) summing
// (gml_conditional_mode, gml_conditional_mode_masked), and in two more it draws from them: the mode of the energies
// perturbed by Gumbel noise (gml_conditional_draw, gml_conditional_draw_masked): see kMode below.
#include "../../include/gml.h"
#include "gml_dev.h"
#include "gml_exact_wht.h"
#include "gml_rng.h"
#include "gml_wg.h"

#include <algorithm>

namespace gml {

// whether an odd number of the term's S visible spins is -1 in the row (bits: the row's sign bits; an unused slot names a zero bit)
template <int S> __device__ __forceinline__ unsigned term_parity(const unsigned short *__restrict__ vs, const unsigned *bits) {
    unsigned par = 0;
#pragma unroll
    for (int a = 0; a < S; ++a) {
        const unsigned sp = vs[a];
        par ^= bits[sp >> 5] >> (sp & 31);
    }
    return par & 1u;
}
template <int S>
__device__ __forceinline__ double item_sum(const double *__restrict__ w, const unsigned short *__restrict__ vis, int t0, int t1,
                                           const unsigned *bits) {
    double s = 0.0;
    for (int t = t0; t < t1; ++t) s += term_parity<S>(vis + (size_t)t * S, bits) ? -w[t] : w[t];
    return s;
}

// kMode (compile time): kCondSums = the sums above; kCondModeSums = those and the row's most probable hidden state (its energy stands in
// log_p for the held one's); kCondModeOnly = that state and its energy alone -- steps 3 and 4 of the chunk are not compiled.  In the
// mode forms every thread keeps its best (energy, local state) over its 16 registers and all chunks -- strict > while the states
// ascend, so the lower state keeps a tie -- and the row ends with one arg-max over the workgroup; thread j writes hidden spin j.
// The mode forms write through the same parameters: means [h][ldm] is then the +-1 bytes of the state (Spin = int8_t), log_w [K] its
// energy, log_p [K] that energy - log sum exp.
// The draw forms, kCondDrawSums and kCondDrawOnly, are the mode forms on perturbed energies (Gumbel-max): chain ch = r K + k, replica
// r of row k, takes the state of largest key(ch, s) = E_k(s) - log(-log u01(seed, ch, s)), equal keys to the lower state.  A job names
// the replicas [rep, rep + kCondDrawBatch) of its row below `replicas`; the row phase and the transform run once for all of them, and
// every thread keeps (best key, its state, its energy) per replica.  The keys are formed in a rolled loop over the thread's 16 states,
// which it reads back from its own slots of v (the two logarithms are compiled once per replica of the batch, not 16 times).  Every
// state is hashed: passing over those whose E + 36.75 (above every perturbation) cannot beat the thread's best key was measured and
// bought nothing where the energies of a row lie closer together than that.
// The outputs go to chain ch where the other forms write row k: means [h][ldm] with ldm = K replicas.
enum { kCondSums = 0, kCondModeSums = 1, kCondModeOnly = 2, kCondDrawSums = 3, kCondDrawOnly = 4 };

template <int kMode, class Spin>
__global__ __launch_bounds__(256) void k_cond_exact(const CondExactPlan *__restrict__ plans, const CondExactJob *__restrict__ jobs,
                                                    long long njobs, const unsigned *__restrict__ Sb, long long wpr, int n,
                                                    Spin *__restrict__ means, long long ldm, double *__restrict__ log_w,
                                                    double *__restrict__ log_p, long long K, int replicas, unsigned long long seed) {
    constexpr bool kDraw = kMode == kCondDrawSums || kMode == kCondDrawOnly;
    constexpr bool kSelect = kMode == kCondModeSums || kMode == kCondModeOnly;
    constexpr bool kNoSums = kMode == kCondModeOnly || kMode == kCondDrawOnly;
    constexpr int RB = kDraw ? kCondDrawBatch : 1;
    // v: the transform's vector; the row phase, which does not transform, keeps the row's sign bits (514 words) and its partial sums
    // (kCondParts doubles from element 264 on) in it
    __shared__ double v[kExactVec], coef[kCondCoefs], red[4], res[kCondMaxHidden + 1];
    __shared__ double held_e;
    __shared__ unsigned held_bits;
    __shared__ unsigned long long red_s[4];
    __shared__ double drawn_e[kCondDrawBatch]; // (the draw forms: the energies of the batch's draws, for log_p)
    unsigned *bits = reinterpret_cast<unsigned *>(v);
    double *part = v + 264;
    const int tid = threadIdx.x;
    const int baseA = 17 * tid, baseB = (tid & 15) + 272 * (tid >> 4), baseC = (tid & 15) + 17 * (tid >> 4);
    double x[16];
    for (long long job = blockIdx.x; job < njobs; job += gridDim.x) {
        const CondExactPlan &P = plans[jobs[job].plan];
        const long long k = jobs[job].row;
        const int h = P.h, c = P.c, S = P.S, ni = P.ni, nm = P.nm, ns = P.ns;
        const int nrep = kDraw ? min(RB, replicas - jobs[job].rep) : 0;
        const long long ch0 = kDraw ? (long long)jobs[job].rep * K + k : 0; // (the job's first chain; replica r of the batch: ch0 + r K)
        __syncthreads(); // (the row before has read v, res, held_e and drawn_e)
        // the row's sign bits: bit i of the row = bit (k & 31) of word k / 32 of spin i's sign row.  32 neighbouring rows share every
        // word (and 1024 a cache line): consecutive workgroups take consecutive jobs, so all but the first find the words in L2.
        {
            const unsigned *col = Sb + (k >> 5);
            const int sh = (int)(k & 31);
            const int nround = (n + 63) & ~63;
            for (int i = tid; i < nround; i += 256) { // (i is a multiple of 64 in lane 0 and the bound one too: whole waves)
                const bool b = i < n && ((col[(long long)i * wpr] >> sh) & 1u);
                const unsigned long long m = __ballot(b);
                if ((tid & 63) == 0) {
                    bits[i >> 5] = (unsigned)m;
                    bits[(i >> 5) + 1] = (unsigned)(m >> 32);
                }
            }
            if (tid == 0) bits[kCondNoSpin >> 5] = 0u;
        }
        __syncthreads();
        // the state the row itself holds on the hidden spins: local bit j <-> hid[j], a set bit is a spin of -1
        if (tid < 64) {
            bool b = false;
            if (tid < h) {
                const int sp = P.hid[tid];
                b = (bits[sp >> 5] >> (sp & 31)) & 1u;
            }
            const unsigned long long m = __ballot(b);
            if (tid == 0) held_bits = (unsigned)m;
        }
        // the row coefficients: items in term order; the only item of a hidden part writes its coefficient, the others a partial sum
        {
            const double *w = P.w;
            const unsigned short *vis = P.vis;
            const int *item_off = P.item_off, *item_dst = P.item_dst;
            for (int it = tid; it < ni; it += 256) {
                const int t0 = item_off[it], t1 = item_off[it + 1];
                double s;
                switch (S) {
                case 1: s = item_sum<1>(w, vis, t0, t1, bits); break;
                case 2: s = item_sum<2>(w, vis, t0, t1, bits); break;
                case 4: s = item_sum<4>(w, vis, t0, t1, bits); break;
                default: s = item_sum<8>(w, vis, t0, t1, bits); break;
                }
                const int dst = item_dst[it];
                if (dst >= 0) coef[dst] = s;
                else part[~dst] = s;
            }
            if (nm) {
                __syncthreads();
                const int *ms_off = P.ms_off, *ms_dst = P.ms_dst;
                for (int s = tid; s < nm; s += 256) { // (at most kCondParts partial sums in all)
                    double sum = 0.0;
                    for (int a = ms_off[s], a1 = ms_off[s + 1]; a < a1; ++a) sum += part[a];
                    coef[ms_dst[s]] = sum;
                }
            }
        }
        __syncthreads();
        const unsigned held = held_bits, held_lo = held & ((1u << c) - 1u), held_hi = held >> c;
        // thread 0 picks S[0], thread j + 1 the singleton of local bit j: a slot of the vector for a chunk bit, S[0] with the sign of
        // the bit in hv for a high one (the threads beyond h pick S[0] and are never written out)
        const int j = tid - 1;
        const bool mine = tid >= 1 && tid <= h;
        const int qlo = mine && j < c ? exact_pad(1 << j) : 0;
        const unsigned qhi = mine && j >= c ? 1u << (j - c) : 0u;
        const unsigned short *chi = P.chi;
        const int *run_off = P.run_off, *run_dst = P.run_dst;
        const int nchunks = 1 << (h - c);
        double acc0 = 0.0, acc1 = 0.0, m0 = -INFINITY, m1 = -INFINITY; // (the maxima are the same in every thread)
        double be = -INFINITY; // (the mode forms: this thread's best)
        unsigned long long bs = ~0ull;
        double dk[RB], de[RB]; // (the draw forms: per replica of the batch this thread's best key, its energy and its state)
        unsigned ds[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) dk[r] = de[r] = -INFINITY, ds[r] = ~0u;
        for (int hv = 0; hv < nchunks; ++hv) {
            __syncthreads(); // (the picks of the chunk before, or the row phase, have read v)
#pragma unroll
            for (int e = 0; e < 16; ++e) v[baseA + e] = 0.0;
            __syncthreads();
            // 1. the coefficient vector of the chunk: every low mask sums its coefficients, signed by their high parts, in order
            for (int s = tid; s < ns; s += 256) {
                double sum = 0.0;
                for (int a = run_off[s], a1 = run_off[s + 1]; a < a1; ++a) sum += (__popc((unsigned)chi[a] & (unsigned)hv) & 1) ? -coef[a] : coef[a];
                v[run_dst[s]] = sum;
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
            if ((unsigned)hv == held_hi && (unsigned)tid == (held_lo & 255u)) {
                double he = x[0];
#pragma unroll
                for (int e = 1; e < 16; ++e)
                    if ((unsigned)e == (held_lo >> 8)) he = x[e];
                held_e = he;
            }
            if constexpr (kSelect) {
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (tid + 256 * e < (1 << c) && x[e] > be) {
                        be = x[e];
                        bs = ((unsigned long long)hv << c) | (unsigned long long)(tid + 256 * e);
                    }
            }
            if constexpr (kDraw) {
                exact_store(v, baseC, 272, x); // (the slots this thread alone has read)
#pragma unroll 1
                for (int e = 0; e < 16 && tid + 256 * e < (1 << c); ++e) {
                    const double en = v[baseC + 272 * e];
                    const unsigned s = ((unsigned)hv << c) | (unsigned)(tid + 256 * e);
#pragma unroll
                    for (int r = 0; r < RB; ++r) {
                        if (r >= nrep) continue;
                        const double key = en - log(-log(u01(seed, (unsigned long long)(ch0 + r * K), s)));
                        if (best_before(key, s, dk[r], ds[r])) { // (the states ascend: an equal key wins only over no state at all)
                            dk[r] = key;
                            de[r] = en;
                            ds[r] = s;
                        }
                    }
                }
            }
            if constexpr (kNoSums) continue;
            // 3. p = exp(E - m0) at the running maximum; a chunk that raises it rescales what has been accumulated
            double mx = x[0];
#pragma unroll
            for (int e = 1; e < 16; ++e) mx = fmax(mx, x[e]);
            const double mn = fmax(m0, block_max(mx, red));
            const double scale = exp(m0 - mn); // (0 at the first chunk: m0 = -inf)
            m0 = mn;
#pragma unroll
            for (int e = 0; e < 16; ++e) x[e] = exp(x[e] - m0);
            // 4. S = WHT(p): passes C, B, A
            wht16(x);
            exact_store(v, baseC, 272, x);
            __syncthreads();
            exact_load(v, baseB, 17, x);
            wht16(x);
            exact_store(v, baseB, 17, x);
            __syncthreads();
            exact_load(v, baseA, 1, x);
            wht16(x);
            exact_store(v, baseA, 1, x);
            __syncthreads();
            const double val = v[qlo];
            acc0 = acc0 * scale + ((__popc(qhi & (unsigned)hv) & 1) ? -val : val);
            if ((hv & (kExactBlock - 1)) == kExactBlock - 1 || hv == nchunks - 1) { // at most kExactBlock chunks in acc0: on to acc1
                const double mn1 = fmax(m1, m0), s1 = exp(m1 - mn1), s0 = exp(m0 - mn1);
                acc1 = acc1 * s1 + acc0 * s0;
                acc0 = 0.0;
                m1 = mn1;
                m0 = -INFINITY;
            }
        }
        if constexpr (kSelect) {
            best_of_block(be, bs, red, red_s);
            if (tid < h) means[(long long)tid * ldm + k] = (bs >> tid) & 1ull ? -1 : 1;
            if (tid == 0 && log_w) log_w[k] = be;
        }
        if constexpr (kDraw) {
            for (int r = 0; r < nrep; ++r) { // (static indices under the unrolled loop; nrep is the same in every thread)
                double bk = -INFINITY, mye = 0.0;
                unsigned long long st = ~0ull;
                unsigned mys = ~0u;
#pragma unroll
                for (int q = 0; q < RB; ++q)
                    if (q == r) bk = dk[q], mye = de[q], mys = ds[q], st = ds[q];
                best_of_block(bk, st, red, red_s);
                const long long ch = ch0 + r * K;
                if (mys == (unsigned)st) { // (one thread: the states of two threads differ, and state 0 is always taken)
                    if (log_w) log_w[ch] = mye;
                    drawn_e[r] = mye;
                }
                if (tid < h) means[(long long)tid * ldm + ch] = (st >> tid) & 1ull ? -1 : 1;
            }
        }
        if constexpr (!kNoSums) {
            if (tid <= h) res[tid] = acc1;
            __syncthreads();
            if (tid == 0) {
                const double lw = m1 + log(ldexp(res[0], c - kExactChunkBits));
                if constexpr (kMode == kCondSums) {
                    if (log_w) log_w[k] = lw;
                    if (log_p) log_p[k] = held_e - lw;
                } else if constexpr (kSelect) {
                    log_p[k] = be - lw;
                } else {
                    for (int r = 0; r < nrep; ++r) log_p[ch0 + r * K] = drawn_e[r] - lw;
                }
            }
            if constexpr (kMode == kCondSums)
                if (mine && means) means[(long long)j * ldm + k] = res[tid] / res[0];
        }
    }
}

void launch_cond_exact(const CondExactPlan *dplans, const CondExactJob *djobs, int64_t njobs, const unsigned *dSb, int64_t wpr, int64_t n,
                       double *dmeans, int64_t ldm, double *dlog_w, double *dlog_p, hipStream_t st) {
    if (njobs <= 0) return;
    const unsigned grid = (unsigned)std::min<int64_t>(njobs, (int64_t)1 << 20);
    hipLaunchKernelGGL((k_cond_exact<kCondSums, double>), dim3(grid), dim3(256), 0, st, dplans, djobs, (long long)njobs, dSb,
                       (long long)wpr, (int)n, dmeans, (long long)ldm, dlog_w, dlog_p, 0ll, 0, 0ull);
}

void launch_cond_mode(const CondExactPlan *dplans, const CondExactJob *djobs, int64_t njobs, const unsigned *dSb, int64_t wpr, int64_t n,
                      int8_t *dstates, int64_t lds, double *denergy, double *dlog_p, hipStream_t st) {
    if (njobs <= 0) return;
    const unsigned grid = (unsigned)std::min<int64_t>(njobs, (int64_t)1 << 20);
    if (dlog_p)
        hipLaunchKernelGGL((k_cond_exact<kCondModeSums, int8_t>), dim3(grid), dim3(256), 0, st, dplans, djobs, (long long)njobs, dSb,
                           (long long)wpr, (int)n, dstates, (long long)lds, denergy, dlog_p, 0ll, 0, 0ull);
    else
        hipLaunchKernelGGL((k_cond_exact<kCondModeOnly, int8_t>), dim3(grid), dim3(256), 0, st, dplans, djobs, (long long)njobs, dSb,
                           (long long)wpr, (int)n, dstates, (long long)lds, denergy, dlog_p, 0ll, 0, 0ull);
}

void launch_cond_draw(const CondExactPlan *dplans, const CondExactJob *djobs, int64_t njobs, const unsigned *dSb, int64_t wpr, int64_t n,
                      int64_t K, int replicas, uint64_t seed, int8_t *dstates, double *denergy, double *dlog_p, hipStream_t st) {
    if (njobs <= 0) return;
    const unsigned grid = (unsigned)std::min<int64_t>(njobs, (int64_t)1 << 20);
    const long long lds = (long long)K * replicas;
    if (dlog_p)
        hipLaunchKernelGGL((k_cond_exact<kCondDrawSums, int8_t>), dim3(grid), dim3(256), 0, st, dplans, djobs, (long long)njobs, dSb,
                           (long long)wpr, (int)n, dstates, lds, denergy, dlog_p, (long long)K, replicas, (unsigned long long)seed);
    else
        hipLaunchKernelGGL((k_cond_exact<kCondDrawOnly, int8_t>), dim3(grid), dim3(256), 0, st, dplans, djobs, (long long)njobs, dSb,
                           (long long)wpr, (int)n, dstates, lds, denergy, dlog_p, (long long)K, replicas, (unsigned long long)seed);
}

} // namespace gml
