// Exact draws of a sparse model by backward sampling on the tables of variable elimination (gml_problem_create_sampled_elim,
// include/gml.h).
//   k_elim_draw       one thread per sample, the whole walk in one kernel: the launches of every component from the last to the first,
//                     the table index in a register.  At a launch with r retiring bits the thread recomputes the 2^r values the
//                     forward launch summed for its output entry -- the same expression, term order and bits -- and picks one by a
//                     counter-based uniform number; the retiring spins go out as +-1 bytes, spin-major.
//   k_elim_draw_free  the spins in no term: a coin per spin and sample.
// Every lane of a wave reads the same launch record, moves and terms at the same time: those addresses depend on the launch number
// alone, so the compiler reads them with scalar loads (hence the moves as 32-bit words: there is no 16-bit scalar load) and the
// control flow is uniform, the switch on r included.  Per lane: 2^r gathers from the table, r byte stores (64 consecutive bytes per
// wave).  No LDS, no barrier, no atomics; a sample's bytes are a function of (model, order, seed, k).
#include "gml_elim.h"
#include "gml_rng.h"

#include <algorithm>

namespace gml {

// One launch of the walk for one sample: returns the index into the launch's input table (= the output table of the launch before).
template <int R>
__device__ __forceinline__ unsigned elim_draw_launch(const ElimDrawLaunch &L, const double *__restrict__ store, const unsigned *__restrict__ tmask,
                                                     const double *__restrict__ tw, const unsigned *__restrict__ mv, double u,
                                                     unsigned j, int8_t *__restrict__ out, long long ld, long long k, bool live) {
    constexpr int C = 1 << R;
    const unsigned base = elim_scope_of(j, L.same, L.nmove, mv + L.mv_off);
    const unsigned inmask = (1u << L.kin) - 1u;
    if (R == 0) return base & inmask;
    unsigned s[C];
    double x[C];
    elim_candidates<R>(base, L.rbit, s);
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = 0.0;
    const unsigned *__restrict__ tm = tmask + L.t_off;
    const double *__restrict__ w = tw + L.t_off;
    for (int t = 0; t < L.nt; ++t) { // phi, as elim_phi sums it
        const unsigned m = tm[t];
        const double wt = w[t];
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] += (__popc(s[c] & m) & 1) ? -wt : wt;
    }
    const double *__restrict__ in = store + L.in_off;
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = in[s[c] & inmask] + x[c];
    double m = x[0];
#pragma unroll
    for (int c = 1; c < C; ++c) m = fmax(m, x[c]);
    double run[C], total = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) run[c] = total += exp(x[c] - m);
    // the smallest c whose running sum exceeds u total; the last if rounding leaves none
    const double target = u * total;
    unsigned pick = C - 1;
#pragma unroll
    for (int c = C - 2; c >= 0; --c)
        if (run[c] > target) pick = (unsigned)c;
    unsigned next = base;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const bool minus = pick >> i & 1u;
        if (minus) next |= L.rbit[i];
        if (live) out[(long long)L.spin[i] * ld + k] = minus ? (int8_t)-1 : (int8_t)1;
    }
    return next & inmask;
}

__global__ __launch_bounds__(256) void k_elim_draw(const ElimDrawLaunch *__restrict__ launches, int nlaunch, const double *__restrict__ store,
                                                   const unsigned *__restrict__ tmask, const double *__restrict__ tw,
                                                   const unsigned *__restrict__ mv, unsigned long long seed, long long N, long long ld,
                                                   int8_t *__restrict__ out) {
    // samples in slabs of 256 per workgroup, the grid striding over them; a lane past N walks like any other (every index it meets
    // is a valid one) and stores nothing
    for (long long k0 = (long long)blockIdx.x * 256; k0 < N; k0 += (long long)gridDim.x * 256) {
        const long long k = k0 + threadIdx.x;
        const bool live = k < N;
        unsigned j = 0;
        for (int l = nlaunch - 1; l >= 0; --l) {
            const ElimDrawLaunch &L = launches[l];
            const double u = L.r > 0 ? u01(seed, (unsigned long long)l, (unsigned long long)k) : 0.0;
            switch (L.r) {
            case 0: j = elim_draw_launch<0>(L, store, tmask, tw, mv, u, j, out, ld, k, live); break;
            case 1: j = elim_draw_launch<1>(L, store, tmask, tw, mv, u, j, out, ld, k, live); break;
            case 2: j = elim_draw_launch<2>(L, store, tmask, tw, mv, u, j, out, ld, k, live); break;
            default: j = elim_draw_launch<3>(L, store, tmask, tw, mv, u, j, out, ld, k, live); break;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_elim_draw_free(const int *__restrict__ spins, int nfree, unsigned long long seed, long long N,
                                                        long long ld, int8_t *__restrict__ out) {
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < N; k += (long long)gridDim.x * 256)
        for (int f = 0; f < nfree; ++f) {
            const int i = spins[f];
            out[(long long)i * ld + k] = u01(seed, kElimFreeStream + (unsigned long long)i, (unsigned long long)k) < 0.5 ? (int8_t)1 : (int8_t)-1;
        }
}

// a grid that fills the device a few times over; the slabs beyond it are taken by the stride
static unsigned draw_grid(long long N) { return (unsigned)std::min<long long>((N + 255) / 256, 4096); }

void launch_elim_draw(const ElimDraw &D, hipStream_t st) {
    if (D.nlaunch == 0) return;
    hipLaunchKernelGGL(k_elim_draw, dim3(draw_grid(D.N)), dim3(256), 0, st, D.launches, D.nlaunch, D.store, D.tmask, D.tw, D.mv, D.seed, D.N,
                       D.ld, D.out);
}

void launch_elim_draw_free(const int *spins, int nfree, unsigned long long seed, long long N, long long ld, int8_t *out, hipStream_t st) {
    if (nfree == 0) return;
    hipLaunchKernelGGL(k_elim_draw_free, dim3(draw_grid(N)), dim3(256), 0, st, spins, nfree, seed, N, ld, out);
}

} // namespace gml
