// Variable elimination on the device (gml_model_elim, include/gml.h): what gml_elim.cpp (planner, driver) and
// gml_elim.hip (the step kernels) share.  Internal; not part of the C ABI.
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

void launch_elim_forward(const ElimForward &S, int r, hipStream_t st);
void launch_elim_backward(const ElimBackward &S, hipStream_t st);
// out[g][q] = sum of in[i][q] over i in [1024 g, min(count, 1024 (g + 1))) in index order
void launch_elim_fold(const double *in, long long count, int nq, double *out, hipStream_t st);

} // namespace gml
