// Microbenchmark: issue rate of v_xor_b32 and v_bcnt_u32_b32 (the two instructions of the pair-moments kernel, gml_moments.hip)
// per SIMD.  256 CUs x W waves per SIMD, each wave runs `iters` x 64 independent instructions of one kind (or xor + bcnt pairs).
// Prints wave-instructions per second and, at the in-kernel clock (s_memtime over s_memrealtime), cycles per instruction per SIMD.
//   hipcc -O3 --offload-arch=gfx950 scripts/ubench/popcount_rate.hip -o scripts/ubench/popcount_rate
#include <hip/hip_runtime.h>
#include <cstdio>

template <int MODE> // 0: xor only, 1: bcnt only (accumulating), 2: xor + bcnt, each bcnt right behind its xor, 3: 16 xor, then 16 bcnt
__global__ __launch_bounds__(256) void k(int iters, unsigned *out, unsigned long long *clk) {
    unsigned a[16], acc[16];
    for (int i = 0; i < 16; ++i) a[i] = threadIdx.x * 2654435761u + i, acc[i] = i;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    unsigned b = blockIdx.x + 1;
    for (int it = 0; it < iters; ++it) {
        if (MODE == 3) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                unsigned t[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) asm volatile("v_xor_b32 %0, %1, %2" : "=v"(t[i]) : "v"(a[(i + u) & 15]), "v"(b));
#pragma unroll
                for (int i = 0; i < 16; ++i) asm volatile("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc[i]) : "v"(t[i]));
            }
        } else
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                // (inline assembly: the compiler would hoist the loop-invariant parts of the plain C++ forms)
                unsigned t;
                if (MODE == 0) asm volatile("v_xor_b32 %0, %1, %0" : "+v"(acc[i]) : "v"(a[(i + u) & 15]));
                if (MODE == 1) asm volatile("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc[i]) : "v"(a[(i + u) & 15]));
                if (MODE == 2) {
                    asm volatile("v_xor_b32 %0, %1, %2" : "=v"(t) : "v"(a[(i + u) & 15]), "v"(b));
                    asm volatile("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc[i]) : "v"(t));
                }
            }
        b = b * 3 + acc[0];
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    unsigned s = 0;
    for (int i = 0; i < 16; ++i) s += acc[i];
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if (blockIdx.x == 0 && threadIdx.x == 0) clk[0] = t1 - t0, clk[1] = r1 - r0;
}

template <int MODE> void run(const char *name, int wps, int per_iter) {
    const int iters = 20000, blocks = 256 * wps;
    unsigned *out;
    unsigned long long *clk, h[2];
    hipMalloc(&out, sizeof(unsigned) * blocks * 256);
    hipMalloc(&clk, 16);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(256), 0, 0, 100, out, clk);
    hipEventRecord(e0);
    hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(256), 0, 0, iters, out, clk);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    hipMemcpy(h, clk, 16, hipMemcpyDeviceToHost);
    const double ghz = (double)h[0] / (double)h[1] * 0.1, insts = (double)iters * per_iter * wps; // per SIMD
    printf("%-10s %d waves/SIMD: %.3f ms, clock %.2f GHz, %.2f cycles per wave-instruction per SIMD\n", name, wps, ms, ghz,
           ms * 1e-3 * ghz * 1e9 / insts);
    hipFree(out);
    hipFree(clk);
}

int main() {
    for (int wps : {1, 2, 4}) {
        run<0>("xor", wps, 64);
        run<1>("bcnt", wps, 64);
        run<2>("xor+bcnt", wps, 128);
        run<3>("16x + 16b", wps, 128);
    }
    return 0;
}
