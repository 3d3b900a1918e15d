// Prints, from the headers the kernels compile (csrc/gml_bits.h, csrc/gml_i8_pairs.h), the index maps of the pack layer and their digit
// and range rules on the integers read from stdin: tests/test_host_i8_pack_reference.py compares tests/_i8_pack_reference.py with
// every entry.  Input: a count n, then n integers.  Plain g++, no device.
#include "gml_i8_pairs.h"

#include <cstdio>
#include <vector>

using namespace gml;

int main() {
    std::printf("xb_col");
    for (int h = 0; h < 2; ++h)
        for (int j = 0; j < 32; ++j) std::printf(" %d", xb_col(j, h));
    std::printf("\nvq_sample");
    for (int p = 0; p < 64; ++p) std::printf(" %d", vq_sample(p));
    std::printf("\npair_slot");
    for (int h = 0; h < 2; ++h)
        for (int m = 0; m < 16; ++m) std::printf(" %d", pair_slot(h, m));
    std::printf("\npair_col");
    for (int h = 0; h < 2; ++h)
        for (int m = 0; m < 16; ++m)
            for (int s = 0; s < 2; ++s) std::printf(" %d", pair_col(h, m, s));
    std::printf("\nxtb_from_natural");
    for (int i = 0; i < 32; ++i) std::printf(" %u", xtb_from_natural(1u << i));
    std::printf("\nlimits %lld %lld %lld\n", PAIR_UNIT, PAIR_MAX, PAIR_MIN);
    int n = 0;
    if (std::scanf("%d", &n) != 1 || n < 0) return 2;
    std::vector<long long> v((size_t)n);
    for (auto &x : v)
        if (std::scanf("%lld", &x) != 1) return 2;
    for (long long x : v) {
        std::printf("digits %lld", x);
        long long r = x;
        for (int l = 0; l < 7; ++l) std::printf(" %lld", balanced_digit(r));
        std::printf(" %lld\n", r);
    }
    // the range rule on every value against its successor in the list (cyclic) and against its own negative
    for (int i = 0; i < n; ++i) {
        const long long a = v[(size_t)i], b = v[(size_t)((i + 1) % n)];
        std::printf("range %lld %lld %d\n", a, b, (int)pair_in_range(a, b));
        std::printf("range %lld %lld %d\n", a, -a, (int)pair_in_range(a, -a));
        std::printf("range %lld %lld %d\n", a, 0ll, (int)pair_in_range(a, 0));
    }
    return 0;
}
