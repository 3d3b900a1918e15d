// Stand-alone check of the host packer's sub-range form (csrc/gml_pack.cpp: pack_spins(h, i0, i1, ...)), the call fill_sign_bits
// makes once per stage of the pinned pipeline.  Built with a host compiler and -fsanitize=address,undefined by
// tests/test_host_ingest_reference.py; needs no device and no library.
//   * the four element types, both layouts, tight and padded leading dimensions (the padding holds NaN / 7: never a legal spin);
//   * K in {1, 31, 32, 33, 511, 512, 513, 1024, 1025, 4097}, n = 70 spins, walked in chunks of 1, 5, 31, 32, 33 and 64 spins;
//   * source and destination are allocated at exactly the extent the interface allows, so that a read or write beyond it faults;
//   * every output word (the zero words beyond K included) is compared with a scalar loop;
//   * with bad entries planted, every sub-range must report the smallest bad configuration among ITS spins, or -1.
// Prints "ok" and returns 0, or says what differed and returns 1.
#include "gml_pack.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

using namespace gml;

namespace {

const ParallelFor serial = [](int64_t cnt, const std::function<void(int64_t)> &fn) {
    for (int64_t t = 0; t < cnt; ++t) fn(t);
};

template <typename T> int dtype_of();
template <> int dtype_of<int8_t>() { return GML_I8; }
template <> int dtype_of<int32_t>() { return GML_I32; }
template <> int dtype_of<int64_t>() { return GML_I64; }
template <> int dtype_of<double>() { return GML_F64; }

template <typename T> T padding_value() {
    if constexpr (std::is_same<T, double>::value) return std::numeric_limits<double>::quiet_NaN();
    else return (T)7;
}

// values that are not +-1, some of them close to it in the bits the vector forms look at
template <typename T> std::vector<T> bad_values();
template <> std::vector<int8_t> bad_values() { return {0, 2, -2, 3, 127, -127, -128}; }
template <> std::vector<int32_t> bad_values() { return {0, 2, -2, 3, 257, -257, 65537}; }
template <> std::vector<int64_t> bad_values() { return {0, 2, -2, 3, 257, ((int64_t)1 << 32) + 1, -(((int64_t)1 << 32) + 1)}; }
template <> std::vector<double> bad_values() {
    return {0.0, -0.0, 0.5, 2.0, std::nextafter(1.0, 2.0), std::nextafter(-1.0, -2.0), std::nextafter(1.0, 0.0),
            std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
}

template <typename T> bool is_pm1(T v) { return v == (T)1 || v == (T)-1; }

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() { // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// A K x (1 + n) histogram in a buffer of exactly the elements the interface lets the packer read: column-major the last column
// ends after its K entries, row-major the last row after its 1 + n.
template <typename T> struct Hist {
    int64_t K, n, ld, extent;
    bool col_major;
    T *buf;
    Hist(int64_t K_, int64_t n_, bool cm, int64_t pad) : K(K_), n(n_), col_major(cm) {
        ld = (cm ? K : n + 1) + pad;
        extent = cm ? ld * n + K : (K - 1) * ld + (n + 1);
        buf = static_cast<T *>(std::malloc(sizeof(T) * (size_t)extent));
        for (int64_t e = 0; e < extent; ++e) buf[e] = padding_value<T>();
        for (int64_t k = 0; k < K; ++k) {
            at(k, 0) = (T)1;
            for (int64_t j = 1; j <= n; ++j) at(k, j) = (next_u64() & 1) ? (T)-1 : (T)1;
        }
    }
    ~Hist() { std::free(buf); }
    Hist(const Hist &) = delete;
    T &at(int64_t k, int64_t j) { return col_major ? buf[k + j * ld] : buf[k * ld + j]; }
    HistView view() const { return hist_view(buf, dtype_of<T>(), K, n, ld, col_major); }
};

int failures = 0;
void complain(const char *what, int dtype, bool cm, int64_t pad, int64_t K, int64_t step, int64_t i0, long long got, long long want) {
    if (++failures <= 20)
        std::printf("%s: dtype %d %s pad %lld K %lld step %lld i0 %lld: got %lld, want %lld\n", what, dtype, cm ? "col-major" : "row-major",
                    (long long)pad, (long long)K, (long long)step, (long long)i0, got, want);
}

template <typename T> void run_case(int64_t K, int64_t n, bool cm, int64_t pad) {
    const int64_t wpr = (K + 1023) / 1024 * 32;
    const int64_t steps[] = {1, 5, 31, 32, 33, 64};
    Hist<T> h(K, n, cm, pad);
    // the scalar statement of the packed form
    std::vector<uint32_t> want((size_t)(n * wpr), 0u);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t k = 0; k < K; ++k)
            if (h.at(k, 1 + i) == (T)-1) want[(size_t)(i * wpr + k / 32)] |= 1u << (k % 32);
    for (int64_t step : steps)
        for (int64_t i0 = 0; i0 < n; i0 += step) {
            const int64_t i1 = std::min(n, i0 + step);
            const size_t words = (size_t)((i1 - i0) * wpr);
            uint32_t *out = static_cast<uint32_t *>(std::malloc(sizeof(uint32_t) * words)); // exactly the rows of this range
            for (size_t e = 0; e < words; ++e) out[e] = 0xDEADBEEFu;                           // (every word must be written)
            const int64_t bad = pack_spins(h.view(), i0, i1, wpr, out, serial);
            if (bad != -1) complain("clean input refused", dtype_of<T>(), cm, pad, K, step, i0, bad, -1);
            for (size_t e = 0; e < words; ++e)
                if (out[e] != want[(size_t)(i0 * wpr) + e]) {
                    complain("sign word", dtype_of<T>(), cm, pad, K, step, i0, (long long)out[e], (long long)want[(size_t)(i0 * wpr) + e]);
                    break;
                }
            std::free(out);
        }
    // bad entries: the first and the last row, the last column, a later column that holds an earlier row than a sooner one
    const std::vector<T> bv = bad_values<T>();
    const int64_t plant[][2] = {{K - 1, 3}, {K / 2, 36}, {K / 3, 37}, {K - 1, 38}, {0, 66}, {K - 1, n - 1}, {(2 * K) / 3, 20}, {K / 4, 21}};
    size_t q = (size_t)(K % 7);
    for (const auto &pl : plant) h.at(pl[0], 1 + pl[1]) = bv[q++ % bv.size()];
    std::vector<uint32_t> out((size_t)(64 * wpr));
    for (int64_t step : steps)
        for (int64_t i0 = 0; i0 < n; i0 += step) {
            const int64_t i1 = std::min(n, i0 + step);
            int64_t first = -1;
            for (int64_t k = 0; k < K && first < 0; ++k)
                for (int64_t i = i0; i < i1; ++i)
                    if (!is_pm1(h.at(k, 1 + i))) {
                        first = k;
                        break;
                    }
            const int64_t bad = pack_spins(h.view(), i0, i1, wpr, out.data(), serial);
            if (bad != first) complain("first offender", dtype_of<T>(), cm, pad, K, step, i0, bad, first);
        }
}

template <typename T> void run_type() {
    const int64_t Ks[] = {1, 31, 32, 33, 511, 512, 513, 1024, 1025, 4097};
    for (int64_t K : Ks)
        for (int cm = 0; cm < 2; ++cm) {
            run_case<T>(K, 70, cm != 0, 0);
            run_case<T>(K, 70, cm != 0, cm ? 5 : 4); // ld = K + 5 column-major, n + 1 + 4 row-major
        }
}

} // namespace

int main() {
    run_type<int8_t>();
    run_type<int32_t>();
    run_type<int64_t>();
    run_type<double>();
    if (failures) {
        std::printf("%d differences\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
