// Would signed column pairs on the 2:4 structured-sparse int8 MFMA carry the forward sweep of precision i8w faster than the dense
// one?  
//
// For two columns c, c' of a row with quantised integers q, q' and +-1 statistics x, x':  x q + x' q' = x (q + q') when x = x' and
// x (q - q') when not.  With the digit planes of (alpha, beta) = (q + q', q - q') in the Theta image, four consecutive K slots of the
// dense operand are [alpha1, beta1, alpha2, beta2] of two pairs and the sample operand picks one of slots {0, 1} and one of {2, 3},
// each with value +-1: 2:4 sparsity.  v_smfmac_i32_32x32x64_i8 takes the picks as its sparse A operand (16 bytes in 4 VGPRs plus one
// index VGPR per lane) and the digits as its dense B operand (32 bytes in 8 VGPRs): one instruction per 64-column step where the
// dense loop issues two v_mfma_i32_32x32x32_i8.
//
// This program (1) FINDS the operand layout by experiment: one launch of 4 096 single-entry probes (A lane x A byte x index value),
// each read back against two codings of the B registers; (2) checks 1 024-column sums of +-1 picks times random digits against
// integer arithmetic on every output; (3) measures what both instructions SUSTAIN on the forward kernel's accumulator set (2 sample
// tiles x 7 planes = 14 independent 32 x 32 accumulators, 2 waves per SIMD, every CU busy, operands from registers, A from random
// bits, B random digits) in 64-column steps per second, the two loops launched alternately.
// Build: hipcc -O3 --offload-arch=gfx950 smfmac_i8_rate.hip -o smfmac_i8_rate
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v16i __attribute__((ext_vector_type(16)));

#define SMFMAC(a, b, c, idx) __builtin_amdgcn_smfmac_i32_32x32x64_i8((a), (b), (c), (idx), 0, 0)
#define MFMA(a, b, c) __builtin_amdgcn_mfma_i32_32x32x32_i8((a), (b), (c), 0, 0, 0)

#define CHECK(x)                                                                              \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));        \
            return 2;                                                                         \
        }                                                                                     \
    } while (0)

// C/D layout of every 32 x 32 MFMA on gfx950: lane (lr = l & 31, h = l >> 5), register e: column lr, row (e & 3) + 8 (e >> 2) + 4 h.
static inline int cd_row(int lane, int e) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }

// ---- (1) layout probes.  Block p = (L * 16 + j) * 4 + t: the A operand is zero but for byte j of lane L, which is 1 and carries
// index value t; its partner in the group of four carries t ^ 2 (a different slot).  B byte jb of lane Lb is Lb (coding 0) or jb
// (coding 1).  Each probe writes its 32 x 32 result for both codings.
__global__ void k_probe(int *__restrict__ out) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int L = p >> 6, j = (p >> 2) & 15, t = p & 3;
    v4i a = {0, 0, 0, 0};
    int idx = 0;
    if (lane == L) {
        a[j >> 2] = 1 << (8 * (j & 3));
        idx = (t << (2 * j)) | ((t ^ 2) << (2 * (j ^ 1)));
    }
    for (int coding = 0; coding < 2; ++coding) {
        v8i b;
        for (int e = 0; e < 8; ++e) b[e] = coding == 0 ? lane * 0x01010101 : 0x03020100 + e * 0x04040404;
        v16i c;
        for (int e = 0; e < 16; ++e) c[e] = 0;
        c = SMFMAC(a, b, c, idx);
        for (int e = 0; e < 16; ++e) out[((size_t)(p * 2 + coding) * 64 + lane) * 16 + e] = c[e];
    }
}

// ---- (2) exactness: one wave per block, 16 instructions = 1 024 columns, operands from memory
__global__ void k_exact(const v4i *__restrict__ a, const int *__restrict__ idx, const v8i *__restrict__ b, int *__restrict__ out) {
    const int w = blockIdx.x, lane = threadIdx.x;
    v16i c;
    for (int e = 0; e < 16; ++e) c[e] = 0;
    for (int it = 0; it < 16; ++it) {
        const size_t o = ((size_t)w * 16 + it) * 64 + lane;
        c = SMFMAC(a[o], b[o], c, idx[o]);
    }
    for (int e = 0; e < 16; ++e) out[((size_t)w * 64 + lane) * 16 + e] = c[e];
}

// ---- (3) sustained rate.  One loop iteration is one 64-column step of a forward-kernel wave: 2 sample tiles x 7 planes.
// KIND 0: 28 dense MFMAs (A = 0/1 bytes of both K halves); KIND 1: 14 sparse ones (A = +-1 picks, index from the same bits).
// The 224 accumulator registers leave room for two or three B fragments, which the planes share in turn: the real loop re-reads B from
// LDS, so only the instruction mix and the operand data matter here.
template <int KIND>
__global__ __launch_bounds__(256, 2) void k_rate(const int *__restrict__ bits, const int *__restrict__ dig, int *__restrict__ out, int iters) {
    const int tid = blockIdx.x * 256 + threadIdx.x;
    v16i acc[2][7];
    for (int i = 0; i < 2; ++i)
        for (int l = 0; l < 7; ++l)
            for (int e = 0; e < 16; ++e) acc[i][l][e] = 0;
    if (KIND == 0) {
        v4i a[2][2], b[3];
        for (int i = 0; i < 2; ++i)
            for (int k = 0; k < 2; ++k)
                for (int e = 0; e < 4; ++e) a[i][k][e] = bits[(tid * 16 + i * 8 + k * 4 + e) & 0xfffff] & 0x01010101;
        for (int i = 0; i < 3; ++i)
            for (int e = 0; e < 4; ++e) b[i][e] = dig[(tid * 16 + i * 4 + e) & 0xfffff];
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int l = 0; l < 7; ++l)
#pragma unroll
                for (int k = 0; k < 2; ++k)
#pragma unroll
                    for (int i = 0; i < 2; ++i) acc[i][l] = MFMA(a[i][k], b[(2 * l + k) % 3], acc[i][l]);
        }
    } else {
        v4i a[2];
        v8i b[2];
        int idx[2];
        for (int i = 0; i < 2; ++i) {
            const int vb = bits[(tid * 16 + i * 8) & 0xfffff];
            idx[i] = (int)(0x88888888u | (((unsigned)vb ^ ((unsigned)vb >> 1)) & 0x55555555u));
            for (int e = 0; e < 4; ++e) { // +-1 bytes: 0x01 or 0xff
                const unsigned m = (unsigned)bits[(tid * 16 + i * 8 + 1 + e) & 0xfffff] & 0x01010101u;
                a[i][e] = (int)(0x01010101u | (m * 0xfeu));
            }
            for (int e = 0; e < 8; ++e) b[i][e] = dig[(tid * 16 + i * 8 + e) & 0xfffff];
        }
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int l = 0; l < 7; ++l)
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[i][l] = SMFMAC(a[i], b[l & 1], acc[i][l], idx[i]);
        }
    }
    int sum = 0;
    for (int i = 0; i < 2; ++i)
        for (int l = 0; l < 7; ++l)
            for (int e = 0; e < 16; ++e) sum += acc[i][l][e];
    out[tid] = sum;
}

// ---- (4) the same step fed as the forward kernel feeds it: a 4-stage LDS ring of 64-column steps (2 KB of sample bits + 7 planes x
// 32 rows x 64 bytes of digits, the kernel's XOR swizzle), one raw barrier per step, the bit dwords read once per step and expanded
// in registers, the fragments read plane by plane and fed to both sample tiles.  No DMA: the ring is filled once.  Dense: 14
// ds_read_b128 and 28 MFMAs per step; paired: the same 14 reads, two per instruction, and 14 sparse MFMAs.  Pairing as the Theta image
// would have it: bits 2 m and 2 m + 1 of a lane's dword are one pair, the +-1 bytes come from the even bits; a lane's 32 bytes of a
// plane row are K-contiguous, so by the layout of (1) the pair m of lane half h sits at bytes 32 (m >> 3) + 16 h + 2 (m & 7) + {0, 1}
// of the row -- an order of the columns inside the image, which costs the loop nothing.
__device__ __forceinline__ int lds_off(int row, int slot) { return row * 64 + ((slot ^ ((row >> 2) & 3)) << 4); }

template <bool SPARSE>
__global__ __launch_bounds__(256, 2) void k_ring(const int *__restrict__ bits, const int *__restrict__ dig, int *__restrict__ out, int iters) {
    __shared__ __attribute__((aligned(16))) int8_t lds[4 * 16384];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, h = lane >> 5;
    for (int i = tid; i < 16384; i += 256)
        reinterpret_cast<int *>(lds)[i] = (i & 4095) < 512 ? bits[(blockIdx.x * 2048 + i) & 0xfffff] : dig[(blockIdx.x * 16384 + i) & 0xfffff];
    __syncthreads();
    v16i acc[2][7];
    for (int i = 0; i < 2; ++i)
        for (int l = 0; l < 7; ++l)
            for (int e = 0; e < 16; ++e) acc[i][l][e] = 0;
    for (int it = 0; it < iters; ++it) {
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const int8_t *cur = lds + (it & 3) * 16384;
        unsigned vb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = wave * 64 + i * 32 + lr;
            const uint2 v = *reinterpret_cast<const uint2 *>(cur + (row >> 7) * 1024 + (row & 127) * 8);
            vb[i] = h ? v.y : v.x;
        }
        if (!SPARSE) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                v4i fa[2];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e) fa[i][e] = (int)((vb[i] >> (4 * t + e)) & 0x01010101u);
#pragma unroll
                for (int l = 0; l < 7; ++l) {
                    const v4i fb = *reinterpret_cast<const v4i *>(cur + 2048 + lds_off(l * 32 + lr, 2 * t + h));
#pragma unroll
                    for (int i = 0; i < 2; ++i) acc[i][l] = MFMA(fa[i], fb, acc[i][l]);
                }
            }
        } else {
            v4i fa[2];
            int idx[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                idx[i] = (int)(0x88888888u | ((vb[i] ^ (vb[i] >> 1)) & 0x55555555u));
#pragma unroll
                for (int e = 0; e < 4; ++e) { // bits 8 e + {0, 2, 4, 6} -> bytes 0..3 as selectors 0 / 1 -> bytes +1 / -1
                    const unsigned m = __umul24((vb[i] >> (8 * e)) & 0x55u, 0x41041u) & 0x01010101u;
                    fa[i][e] = (int)__builtin_amdgcn_perm(0u, 0x0000ff01u, m);
                }
            }
#pragma unroll
            for (int l = 0; l < 7; ++l) {
                const v4i f0 = *reinterpret_cast<const v4i *>(cur + 2048 + lds_off(l * 32 + lr, 2 * h));
                const v4i f1 = *reinterpret_cast<const v4i *>(cur + 2048 + lds_off(l * 32 + lr, 2 * h + 1));
                const v8i fb = {f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3]};
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[i][l] = SMFMAC(fa[i], fb, acc[i][l], idx[i]);
            }
        }
    }
    int sum = 0;
    for (int i = 0; i < 2; ++i)
        for (int l = 0; l < 7; ++l)
            for (int e = 0; e < 16; ++e) sum += acc[i][l][e];
    out[blockIdx.x * 256 + tid] = sum;
}

static const int GRID = 256 * 2 * 8; // 2 workgroups per CU resident, 8 rounds

template <int KIND> // 0, 1: k_rate dense, sparse; 2, 3: k_ring dense, sparse
static double run_ms(const int *bits, const int *dig, int *out, int iters) {
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, 0);
    for (int r = 0; r < 3; ++r) {
        if constexpr (KIND < 2) hipLaunchKernelGGL(k_rate<KIND>, dim3(GRID), dim3(256), 0, 0, bits, dig, out, iters);
        else hipLaunchKernelGGL(k_ring<KIND == 3>, dim3(GRID), dim3(256), 0, 0, bits, dig, out, iters);
    }
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ms / 3;
}

int main() {
    uint32_t s = 2463534242u;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; };

    // ---- (1) layout
    // The rule the observations are held against (the first run of this program printed what it saw; the rule was written from that:
    // the obvious guess, K = 32 h + 2 j + t, holds for half of the probes only).  B is K-major like the dense operand: byte jb of
    // lane (c, hb) is K slot 32 hb + jb of column c.  A byte j of lane (lr, h) is row lr; with index value t it multiplies K slot
    // 32 (j >> 3) + 16 h + 4 ((j & 7) >> 1) + t: the 64 slots are two blocks of 32, the lane's A registers 0, 1 belong to the first and
    // 2, 3 to the second, and inside a block lane half h owns 16 consecutive slots, as in v_mfma_i32_32x32x32_i8.  Index bits 2 j,
    // 2 j + 1 belong to byte j: nibble g of the index VGPR holds the picks of bytes 2 g and 2 g + 1, which share a group of four slots.
    bool layout_ok = false;
    {
        const int NP = 64 * 16 * 4;
        int *dout;
        CHECK(hipMalloc(&dout, (size_t)NP * 2 * 1024 * 4));
        hipLaunchKernelGGL(k_probe, dim3(NP), dim3(64), 0, 0, dout);
        CHECK(hipDeviceSynchronize());
        std::vector<int> ho((size_t)NP * 2 * 1024);
        CHECK(hipMemcpy(ho.data(), dout, ho.size() * 4, hipMemcpyDeviceToHost));
        int one_row = 0, match_all = 0, match_used = 0, n_used = 0;
        int seen_lb[64][16][4], seen_jb[64][16][4], seen_row[64][16][4];
        for (int p = 0; p < NP; ++p) {
            const int L = p >> 6, j = (p >> 2) & 15, t = p & 3;
            // the result as [row][col] for both codings
            static int D[2][32][32];
            for (int cod = 0; cod < 2; ++cod)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 16; ++e) D[cod][cd_row(lane, e)][lane & 31] = ho[((size_t)(p * 2 + cod) * 64 + lane) * 16 + e];
            // which rows are non-zero (coding 1 has a zero at byte 0, so use coding 0 for lanes > 0 and both together)
            int row = -1, rows = 0;
            for (int r = 0; r < 32; ++r) {
                bool nz = false;
                for (int c = 0; c < 32; ++c) nz |= D[0][r][c] != 0 || D[1][r][c] != 0;
                if (nz) { row = r; ++rows; }
            }
            bool ok = rows == 1;
            one_row += ok;
            int lb0 = -1, jb0 = -1;
            if (ok) {
                // B lane of column c must be c + 32 h' for one h', B byte the same for all c
                lb0 = D[0][row][0];
                jb0 = D[1][row][0];
                for (int c = 0; c < 32; ++c) ok &= D[0][row][c] == lb0 + c && D[1][row][c] == jb0;
            }
            seen_row[L][j][t] = row;
            seen_lb[L][j][t] = lb0;
            seen_jb[L][j][t] = jb0;
            const bool hyp = ok && row == (L & 31) && lb0 == 32 * (j >> 3) && jb0 == 16 * (L >> 5) + 4 * ((j & 7) >> 1) + t;
            match_all += hyp;
            const bool used = (j & 1) == (t >> 1); // even bytes pick slots 0, 1; odd bytes pick slots 2, 3
            n_used += used;
            match_used += hyp && used;
        }
        printf("layout: %d probes (A lane x A byte x index value), exactly one non-zero row in %d\n", NP, one_row);
        printf("layout: rule 'A byte j of lane (lr, h), index t -> row lr, times B byte 16 h + 4 ((j & 7) >> 1) + t of lane (col, j >> 3)': holds in %d of %d probes; "
               "in %d of %d of those the paired sweep uses (even byte picks slot 0 or 1, odd byte slot 2 or 3)\n",
               match_all, NP, match_used, n_used);
        for (int L : {0, 37})
            for (int j : {0, 1, 6, 15}) {
                printf("layout: observed  lane %2d byte %2d:", L, j);
                for (int t = 0; t < 4; ++t) printf("  t=%d -> row %2d, B lane col+%2d byte %2d", t, seen_row[L][j][t], seen_lb[L][j][t], seen_jb[L][j][t]);
                printf("\n");
            }
        layout_ok = match_used == n_used;
        (void)hipFree(dout);
    }

    // ---- (2) exactness, with the layout of (1): W waves x 1 024 columns
    {
        const int W = 8;
        const size_t n = (size_t)W * 16 * 64;
        std::vector<int> ha(n * 4), hi(n), hb(n * 8);
        for (size_t o = 0; o < n; ++o) {
            const uint32_t vb = rnd(); // 32 sample bits = 32 columns = 16 pairs: bit 2 m is x, bit 2 m + 1 is x' (1 = -1)
            hi[o] = (int)(0x88888888u | ((vb ^ (vb >> 1)) & 0x55555555u));
            for (int e = 0; e < 4; ++e) {
                uint32_t w = 0;
                for (int q = 0; q < 4; ++q) w |= (((vb >> (2 * (4 * e + q))) & 1) ? 0xffu : 0x01u) << (8 * q);
                ha[o * 4 + e] = (int)w;
            }
            for (int e = 0; e < 8; ++e) hb[o * 8 + e] = (int)rnd();
        }
        int *da, *di, *db, *dout;
        CHECK(hipMalloc(&da, n * 16));
        CHECK(hipMalloc(&di, n * 4));
        CHECK(hipMalloc(&db, n * 32));
        CHECK(hipMalloc(&dout, (size_t)W * 1024 * 4));
        CHECK(hipMemcpy(da, ha.data(), n * 16, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(di, hi.data(), n * 4, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(db, hb.data(), n * 32, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_exact, dim3(W), dim3(64), 0, 0, (const v4i *)da, di, (const v8i *)db, dout);
        CHECK(hipDeviceSynchronize());
        std::vector<int> ho((size_t)W * 1024);
        CHECK(hipMemcpy(ho.data(), dout, ho.size() * 4, hipMemcpyDeviceToHost));
        int good = 0;
        long long amax = 0;
        for (int w = 0; w < W; ++w)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 16; ++e) {
                    const int row = cd_row(lane, e), col = lane & 31;
                    long long want = 0;
                    for (int it = 0; it < 16; ++it)
                        for (int h = 0; h < 2; ++h) {
                            const size_t oa = ((size_t)w * 16 + it) * 64 + row + 32 * h;
                            const signed char *ab = (const signed char *)&ha[oa * 4];
                            for (int j = 0; j < 16; ++j) {
                                const size_t ob = ((size_t)w * 16 + it) * 64 + col + 32 * (j >> 3);
                                const signed char *bb = (const signed char *)&hb[ob * 8];
                                want += (long long)ab[j] * bb[16 * h + 4 * ((j & 7) >> 1) + (((unsigned)hi[oa] >> (2 * j)) & 3)];
                            }
                        }
                    good += want == ho[((size_t)w * 64 + lane) * 16 + e];
                    amax = std::max(amax, want < 0 ? -want : want);
                }
        printf("exactness: %d waves x 1 024-column sums of +-1 picks x random int8 digits against integer arithmetic: %d of %d outputs equal (max |sum| %lld)%s\n",
               W, good, W * 1024, amax, good == W * 1024 ? "  (exact)" : "  ** MISMATCH **");
        layout_ok &= good == W * 1024;
    }

    // ---- (3) sustained rates, dense and sparse launched alternately
    {
        std::vector<int> hbits(1 << 20), hdig(1 << 20);
        for (auto &v : hbits) v = (int)rnd();
        for (auto &v : hdig) v = (int)rnd();
        int *dbits, *ddig, *dout;
        CHECK(hipMalloc(&dbits, 4 << 20));
        CHECK(hipMalloc(&ddig, 4 << 20));
        CHECK(hipMalloc(&dout, (size_t)GRID * 256 * 4));
        CHECK(hipMemcpy(dbits, hbits.data(), 4 << 20, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(ddig, hdig.data(), 4 << 20, hipMemcpyHostToDevice));
        const int iters = 2000;
        run_ms<0>(dbits, ddig, dout, iters / 8); // warm-up
        run_ms<1>(dbits, ddig, dout, iters / 8);
        CHECK(hipDeviceSynchronize());
        const double steps = (double)GRID * 4.0 * iters; // 64-column steps of one wave (2 sample tiles x 7 planes) per launch
        std::vector<double> rd, rs;
        for (int rep = 0; rep < 5; ++rep) {
            const double md = run_ms<0>(dbits, ddig, dout, iters), ms = run_ms<1>(dbits, ddig, dout, iters);
            rd.push_back(md);
            rs.push_back(ms);
            // algorithmic int8 ops of a step: 2 tiles x 7 planes x 32 x 32 x 64 MACs
            const double ops = 2.0 * steps * 14.0 * 32 * 32 * 64;
            printf("round %d: dense 28 x 32x32x32: %.3f ms, %.1f G steps/s (%.2f POP/s)   sparse 14 x 32x32x64: %.3f ms, %.1f G steps/s (%.2f POP/s of the dense "
                   "work)   sparse / dense rate %.3f\n",
                   rep, md, steps / md / 1e6, ops / (md * 1e-3) / 1e15, ms, steps / ms / 1e6, ops / (ms * 1e-3) / 1e15, md / ms);
        }
        CHECK(hipDeviceSynchronize());
        std::sort(rd.begin(), rd.end());
        std::sort(rs.begin(), rs.end());
        printf("bare loops, median of 5: dense %.3f ms (%.3f..%.3f), sparse %.3f ms (%.3f..%.3f): one sparse instruction per 64-column step runs at %.3f x the "
               "rate of two dense ones\n",
               rd[2], rd[0], rd[4], rs[2], rs[0], rs[4], rd[2] / rs[2]);
        // ---- (4) the same from an LDS ring, with the bit expansion and a barrier per step
        run_ms<2>(dbits, ddig, dout, iters / 8);
        run_ms<3>(dbits, ddig, dout, iters / 8);
        rd.clear();
        rs.clear();
        for (int rep = 0; rep < 5; ++rep) {
            const double md = run_ms<2>(dbits, ddig, dout, iters), ms = run_ms<3>(dbits, ddig, dout, iters);
            rd.push_back(md);
            rs.push_back(ms);
            printf("ring round %d: dense step %.3f ms, %.1f G steps/s   paired step %.3f ms, %.1f G steps/s   paired / dense rate %.3f\n", rep, md,
                   steps / md / 1e6, ms, steps / ms / 1e6, md / ms);
        }
        CHECK(hipDeviceSynchronize());
        std::sort(rd.begin(), rd.end());
        std::sort(rs.begin(), rs.end());
        printf("LDS-fed steps, median of 5: dense %.3f ms (%.3f..%.3f), paired %.3f ms (%.3f..%.3f): ratio %.3f\n", rd[2], rd[0], rd[4], rs[2], rs[0],
               rs[4], rd[2] / rs[2]);
    }
    return layout_ok ? 0 : 1;
}
