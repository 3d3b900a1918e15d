// The block mapping of the int8 forward kernels (csrc/gml_i8_map.h), run on the host over a whole grid.
// usage: i8_fwd_map ntiles_k ngroups   (prints "ok" and exits 0, or the failed comparison and exits 1)
#include "gml_i8_map.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int ntk = 0, ng = 0;

#define CHECK(cond)                                                                                        \
    do {                                                                                                   \
        if (!(cond)) {                                                                                     \
            std::printf("FAILED line %d (ntiles_k = %d, ngroups = %d, b = %d): %s\n", __LINE__, ntk, ng, b, #cond); \
            std::exit(1);                                                                                  \
        }                                                                                                  \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    ntk = std::atoi(argv[1]);
    ng = std::atoi(argv[2]);
    const int grid = gml::fwd_grid(ntk, ng);
    int b = -1;
    CHECK(grid == (ntk + 7) / 8 * 8 * ng);
    std::vector<int> seen((size_t)ntk * ng, 0);
    // per XCD (blocks b, b + 8, ... share one): the group of 8 node tiles its latest block ran, and which groups it has left behind
    std::vector<int> cur(8, -1);
    std::vector<std::vector<char>> left(8, std::vector<char>((size_t)(ng + 7) / 8, 0));
    int live = 0;
    for (b = 0; b < grid; ++b) {
        const gml::FwdBlock k = gml::fwd_block(b, ntk, ng);
        CHECK(k.st >= 0 && k.st % 8 == b % 8); // XCD x owns the sample tiles 8 i + x
        CHECK(k.gi >= 0 && k.gi < ng);
        CHECK(k.live == (k.st < ntk));
        if (k.live) {
            ++live;
            CHECK(seen[(size_t)k.st * ng + k.gi]++ == 0); // no pair twice
        }
        // a node-tile group's blocks are contiguous in the XCD's sequence: a group once left does not come back
        const int x = b % 8, grp = k.gi / 8;
        if (grp != cur[x]) {
            CHECK(!left[x][grp]);
            if (cur[x] >= 0) left[x][cur[x]] = 1;
            cur[x] = grp;
        }
    }
    b = -1;
    CHECK(live == ntk * ng); // with "no pair twice": every pair exactly once, every other block not live
    std::printf("ok\n");
    return 0;
}
