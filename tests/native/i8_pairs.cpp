// The signed column pairs of the i8w forward sweep (csrc/gml_i8_pairs.h), run on the host.
// usage: i8_pairs seed   (prints "ok" and exits 0, or the failed comparison and exits 1)
#include "gml_i8_pairs.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static unsigned long long seed = 0;
static uint64_t rs;
static uint64_t rnd() {
    rs ^= rs << 13;
    rs ^= rs >> 7;
    rs ^= rs << 17;
    return rs;
}

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::printf("FAILED line %d (seed %llu): %s\n", __LINE__, seed, #cond);  \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

typedef __int128 i128;
static const long long QMAX = 1ll << 54; // |q| <= 2^54 (k_quant_theta<7>)

// a quantised entry: uniform in its range, or at / next to an extreme, or small
static long long some_q() {
    const unsigned kind = (unsigned)(rnd() % 8);
    long long q;
    if (kind == 0) q = QMAX - (long long)(rnd() % 3);
    else if (kind == 1) q = -QMAX + (long long)(rnd() % 3);
    else if (kind == 2) q = (long long)(rnd() % 513) - 256;
    else if (kind == 3) q = gml::PAIR_MAX - QMAX + (long long)(rnd() % 5) - 2; // the partner of 2^54 at the edge of the range
    else q = (long long)(rnd() % (2ull * QMAX + 1)) - QMAX;
    return q;
}

// what v_smfmac_i32_32x32x64_i8 adds for one sample (both lane halves) and one plane row of 64 bytes, operands as pair_picks() of
// gml_i8_fwd.h builds them: byte m = +1 / -1 by bit 2 m, 2-bit index m of 0x88888888 | ((v ^ v >> 1) & 0x55555555), multiplying K
// slot 32 (m >> 3) + 16 h + 4 ((m & 7) >> 1) + index (layout measured on the device: scripts/ubench/smfmac_i8_rate.hip)
template <class T>
static i128 sparse_step(const uint32_t (&vb)[2], const T (&row)[64]) {
    i128 s = 0;
    for (int h = 0; h < 2; ++h) {
        const uint32_t idx = 0x88888888u | ((vb[h] ^ (vb[h] >> 1)) & 0x55555555u);
        for (int m = 0; m < 16; ++m) {
            const int x = ((vb[h] >> (2 * m)) & 1u) ? -1 : 1;
            const int t = (int)((idx >> (2 * m)) & 3u);
            CHECK((t >> 1) == (m & 1)); // even bytes pick the lower half of their group of four, odd bytes the upper
            s += (i128)x * (i128)row[32 * (m >> 3) + 16 * h + 4 * ((m & 7) >> 1) + t];
        }
    }
    return s;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    seed = std::strtoull(argv[1], nullptr, 10);
    rs = seed * 0x9E3779B97F4A7C15ull + 0x1234567ull;

    // ---- the column <-> slot map of a step is a bijection both ways
    {
        int slot_seen[64] = {0}, col_seen[64] = {0};
        for (int h = 0; h < 2; ++h)
            for (int m = 0; m < 16; ++m) {
                const int p = gml::pair_slot(h, m);
                CHECK(p >= 0 && p + 1 < 64 && (p & 1) == 0);
                ++slot_seen[p];
                ++slot_seen[p + 1];
                for (int s = 0; s < 2; ++s) {
                    const int c = gml::pair_col(h, m, s);
                    CHECK(c >= 0 && c < 64);
                    ++col_seen[c];
                }
                // the pair sits where the sparse operand of byte m looks: its half of the group of four of lane half h
                CHECK(p == 32 * (m >> 3) + 16 * h + 4 * ((m & 7) >> 1) + 2 * (m & 1));
            }
        for (int i = 0; i < 64; ++i) CHECK(slot_seen[i] == 1 && col_seen[i] == 1);
    }

    // ---- digits and range of alpha, beta
    CHECK(gml::PAIR_UNIT * 255 + 1 == (1ll << 56));
    for (int it = 0; it < 20000; ++it) {
        long long q = some_q(), qp = some_q();
        if (it == 0) { q = QMAX; qp = QMAX; }
        if (it == 1) { q = QMAX; qp = -QMAX; }
        if (it == 2) { q = gml::PAIR_MAX - QMAX; qp = QMAX; }     // alpha = PAIR_MAX: the last pair inside
        if (it == 3) { q = gml::PAIR_MAX - QMAX + 1; qp = QMAX; } // the first outside
        if (it == 4) { q = gml::PAIR_MIN + QMAX; qp = -QMAX; }
        if (it == 5) { q = gml::PAIR_MIN + QMAX - 1; qp = -QMAX; }
        const i128 ab[2] = {(i128)q + qp, (i128)q - qp};
        bool inside = true;
        for (int s = 0; s < 2; ++s) {
            // 128-bit check: seven balanced digits spell v iff stripping seven of them leaves nothing
            i128 v = ab[s], sum = 0, pw = 1;
            for (int l = 0; l < 7; ++l) {
                const i128 d = ((v + 128) & 255) - 128;
                v = (v - d) >> 8;
                sum += d * pw;
                pw *= 256;
            }
            const bool fits = v == 0;
            CHECK(fits == (ab[s] >= (i128)gml::PAIR_MIN && ab[s] <= (i128)gml::PAIR_MAX));
            CHECK(!fits || sum == ab[s]);
            inside &= fits;
        }
        CHECK(gml::pair_in_range(q, qp) == inside);
        if (inside) { // the header's own digits recombine exactly
            for (int s = 0; s < 2; ++s) {
                long long v = (long long)ab[s];
                i128 sum = 0, pw = 1;
                for (int l = 0; l < 7; ++l) {
                    const long long d = gml::balanced_digit(v);
                    CHECK(d >= -128 && d <= 127);
                    sum += (i128)d * pw;
                    pw *= 256;
                }
                CHECK(v == 0 && sum == ab[s]);
            }
        }
    }

    // ---- a 64-column step: the picks of the sparse operand times the paired row = sum_c x_c q_c, whole values and plane by plane
    for (int it = 0; it < 2000; ++it) {
        long long qcol[64];
        for (int c = 0; c < 64; ++c) {
            do qcol[c] = some_q();
            while (qcol[c] > QMAX / 2 || qcol[c] < -QMAX / 2); // (every pair inside the range)
        }
        uint32_t vb[2] = {(uint32_t)rnd(), (uint32_t)rnd()};
        static const uint32_t fixed[4] = {0u, 0x55555555u, 0xAAAAAAAAu, 0xFFFFFFFFu}; // the four sign cases (x, x'), everywhere
        if (it < 4) vb[0] = vb[1] = fixed[it];
        long long row[64];
        signed char planes[7][64];
        for (int h = 0; h < 2; ++h)
            for (int m = 0; m < 16; ++m) {
                const long long q = qcol[gml::pair_col(h, m, 0)], qp = qcol[gml::pair_col(h, m, 1)];
                CHECK(gml::pair_in_range(q, qp));
                const int p = gml::pair_slot(h, m);
                row[p] = q + qp;
                row[p + 1] = q - qp;
                for (int s = 0; s < 2; ++s) {
                    long long v = row[p + s];
                    for (int l = 0; l < 7; ++l) planes[l][p + s] = (signed char)gml::balanced_digit(v);
                }
            }
        i128 want = 0;
        int cases[4] = {0, 0, 0, 0};
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < 32; ++j) { // bit j of dword h is column xb_col(j, h) of the step (gml_bits.h)
                const int x = ((vb[h] >> j) & 1u) ? -1 : 1;
                want += (i128)x * qcol[gml::xb_col(j, h)];
                if (!(j & 1)) ++cases[((vb[h] >> j) & 3u)];
            }
        CHECK(sparse_step(vb, row) == want);
        i128 got = 0, pw = 1;
        for (int l = 0; l < 7; ++l) {
            got += sparse_step(vb, planes[l]) * pw;
            pw *= 256;
        }
        CHECK(got == want);
        if (it < 4) CHECK(cases[it] == 32);
    }
    std::printf("ok\n");
    return 0;
}
