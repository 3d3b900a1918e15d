// Prints, from the header the kernels compile (csrc/gml_bits.h), the sample order of a step of the Vq limb images and -- by walking the
// bytes of an image in memory order, as csrc/gml_dev.h lays it out: images [node tile][step] of [lbt planes][32 rows][64 bytes], the
// byte p of a row holding the step's sample vq_sample(p) -- the offset of every (row, plane, sample):
// tests/test_host_i8_pass_reference.py compares tests/_i8_pass_reference.py with every entry.  Input: slots, Kp.  Plain g++, no device.
#include "gml_bits.h"

#include <cstdio>

using namespace gml;

int main() {
    long long slots = 0, Kp = 0;
    if (std::scanf("%lld %lld", &slots, &Kp) != 2 || slots <= 0 || slots % 32 || Kp <= 0 || Kp % 64) return 2;
    std::printf("vq_pos");
    for (int s = 0; s < 64; ++s) std::printf(" %d", vq_pos(s));
    std::printf("\nvq_sample");
    for (int p = 0; p < 64; ++p) std::printf(" %d", vq_sample(p));
    std::printf("\n");
    for (int lbt = 4; lbt <= 6; lbt += 2) {
        long long off = 0;
        for (long long tile = 0; tile < slots / 32; ++tile)
            for (long long step = 0; step < Kp / 64; ++step)
                for (int l = 0; l < lbt; ++l)
                    for (int rl = 0; rl < 32; ++rl)
                        for (int p = 0; p < 64; ++p, ++off)
                            std::printf("off %d %lld %d %lld %lld\n", lbt, tile * 32 + rl, l, step * 64 + vq_sample(p), off);
    }
    return 0;
}
