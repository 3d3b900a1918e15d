// Prints what csrc/gml_i8_hw.h computes, for tests/test_host_i8_hess_reference.py (plain C++, no GPU).
// stdin: n, then n values mm; m, then m quadruples (node, sample, mm, mag) with mag an unsigned 32-bit number.
// stdout: "shift mm sh_exp sh_rple" per mm; "cut node sample mm mag form sh dither h2 lo hi" per quadruple and form (0 exp, 2 RPLE).
#include "gml_i8_hw.h"

#include <cstdio>

int main() {
    long long n = 0, m = 0;
    if (scanf("%lld", &n) != 1) return 1;
    for (long long i = 0; i < n; ++i) {
        unsigned long long mm;
        if (scanf("%llu", &mm) != 1) return 1;
        printf("shift %llu %d %d\n", mm, gml::hw_shift((unsigned)mm, 0), gml::hw_shift((unsigned)mm, 2));
    }
    if (scanf("%lld", &m) != 1) return 1;
    for (long long i = 0; i < m; ++i) {
        long long u, k;
        unsigned long long mm, mag;
        if (scanf("%lld %lld %llu %llu", &u, &k, &mm, &mag) != 4) return 1;
        for (int form = 0; form <= 2; form += 2) {
            const int sh = gml::hw_shift((unsigned)mm, form);
            const unsigned dth = gml::hw_dither((int)u, (int64_t)k, sh);
            const unsigned h2 = gml::hw_clip((int)(unsigned)mag, dth, sh);
            int lo, hi;
            gml::hw_digits(h2, lo, hi);
            printf("cut %lld %lld %llu %llu %d %d %u %u %d %d\n", u, k, mm, mag, form, sh, dth, h2, lo, hi);
        }
    }
    printf("limits %d %d\n", gml::HL, 32639);
    return 0;
}
