// Block mapping of the int8 forward kernels (k_fwd_i8, k_fwd_i8w): which (sample tile, node tile) a workgroup runs, and the
// grid that covers them.  Plain C++ (host and device; tests/native/i8_fwd_map.cpp drives it on the host).
#pragma once
#include "gml_bits.h"

namespace gml {

struct FwdBlock {
    int st, gi; // sample tile (256 samples), index into the pass's list of node tiles
    bool live;  // false: the block pads the sample tiles to a multiple of 8 and has nothing to do
};

// XCD-aware L2 blocking.  Blocks b and b + 8 share an XCD (round-robin dispatch); XCD x owns the sample tiles st = 8 i + x.
// Within an XCD: groups of TG node tiles (outer), sample tiles (middle), the TG node tiles (inner): Tq of the group stays
// resident in the XCD's L2 over the sweep and each bit piece is fetched once per node-tile group.  The last group holds
// ngroups % TG tiles; the grid has no idle workgroups beyond the sample tiles that pad ntiles_k to a multiple of 8 (a
// node-sharded rank runs few node tiles: half of its launch would otherwise be workgroups that start only to exit).
GML_HD FwdBlock fwd_block(int b, int ntiles_k, int ngroups) {
    constexpr int TG = 8;
    const int xcd = b & 7, bi = b >> 3;
    const int ntk8 = (ntiles_k + 7) >> 3;
    const int nfull = ngroups / TG, per_full = ntk8 * TG;
    int st, gi;
    if (bi < nfull * per_full) {
        const int rem = bi % per_full;
        st = (rem / TG) * 8 + xcd;
        gi = (bi / per_full) * TG + rem % TG;
    } else {
        const int lastn = ngroups - nfull * TG, rem = bi - nfull * per_full;
        st = (rem / lastn) * 8 + xcd;
        gi = nfull * TG + rem % lastn;
    }
    return FwdBlock{st, gi, st < ntiles_k};
}

// one workgroup per (sample tile, node tile), the sample tiles padded to a multiple of 8
GML_HD int fwd_grid(int ntiles_k, int ngroups) { return ((ntiles_k + 7) / 8) * 8 * ngroups; }

} // namespace gml
