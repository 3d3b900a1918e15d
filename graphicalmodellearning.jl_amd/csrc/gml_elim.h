// Variable elimination on the device (gml_model_elim, gml_problem_create_sampled_elim, include/gml.h): what
// gml_elim.cpp (planner, driver), gml_elim.hip (the step kernels) and gml_elim_draw.hip (the backward walk of the draws) share.
// Internal; not part of the C ABI.
//
// A table is indexed by the bits of the frontier's slots: bit b set <=> the spin in slot b is -1.  A frontier of k spins fills the
// slots 0 .. k - 1 (no holes), so a table has exactly 2^k entries.  The scope of a step is the table's slots plus, at bit k, the
// spin the step introduces.  ElimMap says where the bits of a table index sit in a scope state: the bits of `same` stay in place,
// move i takes bit (mv[i] & 255) of the index to bit (mv[i] >> 8) of the scope.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gml {

constexpr int kElimMaxWidth = 30;  // = GML_ELIM_MAX_WIDTH: spins of a scope
constexpr int kElimMaxRetire = 3;  // spins summed out by one forward launch (2^3 reads per output entry)
constexpr int kElimTermTile = 256; // terms of a step staged in LDS at a time
constexpr int kElimQuant = 16;     // signed sums of p_t one backward launch reduces
constexpr int kElimChunk = 1024;   // table entries per workgroup of the backward kernel, and the fan-in of k_elim_fold

struct ElimMap {
    unsigned same;
    int nmove;
    const unsigned short *mv;
};

// One forward launch: out[j] = logsumexp over the r retiring bits of (in[scope state & (2^kin - 1)] + phi(scope state)).
// nt = 0 and no introduced spin: a retire-only launch.
struct ElimForward {
    const double *in;
    double *out;
    const unsigned *tmask; // the step's terms as masks over the scope
    const double *tw;
    int nt;
    ElimMap map;       // output index -> scope state
    unsigned rbit[kElimMaxRetire]; // the retiring scope bits as masks, ascending
    int kin, kout;
};

// One backward launch of step t: beta_out[i] = logsumexp over the introduced spin of (phi + beta), and the signed sums
// part[workgroup][q] = sum over the workgroup's scope states of p_t x sign(popcount(state & qmask[q])).
struct ElimBackward {
    const double *alpha; // alpha_{t-1} [2^kin]
    const double *beta;  // beta_t, indexed through map
    double *beta_out;    // beta_{t-1} [2^kin], or NULL (a further window of quantities of the same step)
    const unsigned *tmask;
    const double *tw;
    int nt;
    ElimMap map; // scope state -> index of beta_t (the moves read the other way: scope bit mv >> 8 to index bit mv & 255)
    const unsigned *qmask;
    int nq; // <= kElimQuant
    double *part;
    int kin;
    const double *log_z; // alpha_n of the component, on the device
};

// index of a launch's output table -> scope state (the retiring bits 0), and a scope state -> index of the table its map describes.
// (Move: unsigned short as ElimMap holds them, or the same values as 32-bit words, which a wave can read with scalar loads.)
template <class Move> __device__ __forceinline__ unsigned elim_scope_of(unsigned j, unsigned same, int nmove, const Move *__restrict__ moves) {
    unsigned s = j & same;
    for (int i = 0; i < nmove; ++i) {
        const unsigned mv = moves[i];
        s |= ((j >> (mv & 255u)) & 1u) << (mv >> 8);
    }
    return s;
}
__device__ __forceinline__ unsigned elim_scope_of(unsigned j, const ElimMap &m) { return elim_scope_of(j, m.same, m.nmove, m.mv); }
__device__ __forceinline__ unsigned elim_index_of(unsigned s, const ElimMap &m) {
    unsigned j = s & m.same;
    for (int i = 0; i < m.nmove; ++i) {
        const unsigned mv = m.mv[i];
        j |= ((s >> (mv >> 8)) & 1u) << (mv & 255u);
    }
    return j;
}
// the 2^R scope states a launch sums over (forward) or picks among (the draw): bit i of c <-> rbit[i]
template <int R> __device__ __forceinline__ void elim_candidates(unsigned base, const unsigned (&rbit)[kElimMaxRetire], unsigned (&s)[1 << R]) {
#pragma unroll
    for (int c = 0; c < (1 << R); ++c) {
        unsigned v = base;
#pragma unroll
        for (int i = 0; i < R; ++i)
            if (c >> i & 1) v |= rbit[i];
        s[c] = v;
    }
}

// One forward launch as the backward walk of the draws reads it (gml_problem_create_sampled_elim): the records of all components of a
// call sit in one array in launch order, their terms and moves in the call's joint arrays, their tables in one store.  (The output
// table has no place here: the walk carries its index and never reads it.)
struct ElimDrawLaunch {
    long long in_off;              // the input table in the store
    long long t_off;               // the step's terms (nt of them; 0 on all but the first launch of a step)
    unsigned same;                 // with mv_off, nmove: output index -> scope state
    unsigned rbit[kElimMaxRetire]; // the retiring scope bits as masks, ascending
    int spin[kElimMaxRetire];      // the spins they hold
    int kin, r, nt, mv_off, nmove;
};
struct ElimDraw {
    const ElimDrawLaunch *launches;
    int nlaunch;
    const double *store;
    const unsigned *tmask;
    const double *tw;
    const unsigned *mv; // the moves of all launches, one 32-bit word each
    unsigned long long seed;
    long long N, ld; // samples; out[spin * ld + k]
    int8_t *out;     // +-1 bytes, spin-major
};
constexpr unsigned long long kElimFreeStream = 1ull << 62; // a spin i in no term: +1 iff u01(seed, kElimFreeStream + i, k) < 0.5

void launch_elim_forward(const ElimForward &S, int r, hipStream_t st);
void launch_elim_backward(const ElimBackward &S, hipStream_t st);
// out[g][q] = sum of in[i][q] over i in [1024 g, min(count, 1024 (g + 1))) in index order
void launch_elim_fold(const double *in, long long count, int nq, double *out, hipStream_t st);
// every sample's walk over all launches, last to first (gml_elim_draw.hip)
void launch_elim_draw(const ElimDraw &D, hipStream_t st);
// out[spins[f] * ld + k] for the nfree spins in no term
void launch_elim_draw_free(const int *spins, int nfree, unsigned long long seed, long long N, long long ld, int8_t *out, hipStream_t st);

} // namespace gml
