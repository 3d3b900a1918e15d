// Exact sample moments of a handle from its sign bits (gml_problem_moments, gml_problem_term_moments).
//
// Sb holds one bit per entry (set <=> -1), spin-major, so a product of spins is the XOR of their sign rows and a sum over the
// configurations is a population count.  With integer counts c_k:
//   sum_k c_k prod_{i in key} s_ki = M - 2 N,   N = sum_k c_k [XOR of the key's sign bits at k],
// and N is accumulated in integers: no rounding anywhere, so the results do not depend on tiles, K split, grid or device.
//   * counts all equal (DevProblem::wuni != 0: every handle with one row per draw): N = c popcount(XOR);
//   * otherwise by bit planes of the counts: N = sum_b 2^b popcount(XOR & C_b), C_b = bit b of every c_k packed like a sign row
//     (k_count_planes).  The pair kernel runs once per plane on rows masked while they are staged; the term kernel loops over
//     the planes per word.
// Padding configurations (K .. Kp) have zero sign bits and zero plane bits: they add nothing.
#include "../../include/gml.h"
#include "gml_dev.h"

#include <algorithm>

namespace gml {

// ---- the counts as bit planes: planes [nplanes][wpr], bit j of word w of plane b = bit b of c_(32 w + j), c_k = rint(w_k M)
__global__ __launch_bounds__(256) void k_count_planes(const double *__restrict__ w, double M, int64_t K, int64_t wpr,
                                                      unsigned *__restrict__ planes) {
    const int64_t wd = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (wd >= wpr) return;
    unsigned v = 0;
    for (int j = 0; j < 32; ++j) {
        const int64_t k = wd * 32 + j;
        if (k < K) v |= (unsigned)(((unsigned long long)rint(w[k] * M) >> b) & 1ull) << j;
    }
    planes[(int64_t)b * wpr + wd] = v;
}

// ---- pair counts: a binary GEMM on the vector ALU --------------------------------------------------------------------------
// N[i][j] += (sum over the workgroup's K range of popcount((Sb_i ^ Sb_j) & plane)) << shift for a tile of 64 x 64 pairs,
// upper triangle of tiles only (blockIdx.y <= blockIdx.x).  256 threads; thread (ty, tx) owns the R x R = 4 x 4 pairs
// (ty + 16 a, tx + 16 b), so one 16-byte LDS read of a row feeds R columns: per staged uint4 step 2 R LDS reads for 4 R^2 xor
// + 4 R^2 v_bcnt.  K runs in chunks of 32 words (1024 configurations; the row pitch Kp / 32 is a multiple of 32): the next
// chunk is fetched into registers while the current one is counted.  LDS rows have a pitch of 36 words, so the 16 distinct rows
// a ds_read_b128 lane group touches fall on distinct banks (36 r mod 64 is a different multiple of 4 for r = 0 .. 15).
// (R = 8, a 128 x 128 tile with half the LDS reads and HBM bytes per pair, was measured and is slower at every shape: 226
// registers leave two waves per SIMD -- profiles/r10_moments_tile_sweep.txt.)
constexpr int kPairR = 4, kPairTile = 16 * kPairR;
constexpr int kPairChunkWords = 32;
constexpr int64_t kPairMaxChunksPerSplit = (int64_t)1 << 21; // see acc below

// acc + popcount(x) as the one instruction it is.  (Written as `acc += __popc(x)` the compiler re-associates the four counts of a
// pair into v_bcnt + v_add3 chains: a quarter more vector instructions, each waiting for the one before it.)
__device__ inline unsigned bcnt_add(unsigned x, unsigned acc) {
    unsigned r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

__global__ __launch_bounds__(256) void k_moments_pairs(const unsigned *__restrict__ Sb, int64_t wpr, int64_t n,
                                                       const unsigned *__restrict__ plane /* [wpr] or NULL */, int shift,
                                                       int64_t chunks_per_split, int64_t nchunks, unsigned long long *__restrict__ N) {
    constexpr int R = kPairR, T = kPairTile;
    constexpr int LD = R / 2; // uint4 per thread and operand of one chunk: T rows x 8 uint4 / 256 threads
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    __shared__ uint4 sA[T][9], sB[T][9];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t c0 = (int64_t)blockIdx.z * chunks_per_split, c1 = min(nchunks, c0 + chunks_per_split);
    if (c0 >= c1) return;
    // loader: uint4 q = tid + 256 h of the tile's T x 8: row q >> 3, uint4 q & 7 (8 lanes read 128 contiguous bytes of a row).
    // Rows beyond n are clamped to row n - 1: their pairs are never written
    const int lv = tid & 7, lrow = tid >> 3;
    const int64_t ia = (int64_t)bi * T + lrow, ib = (int64_t)bj * T + lrow;
    const uint4 *g4 = reinterpret_cast<const uint4 *>(Sb) + lv;
    const int64_t wpr4 = wpr / 4;
    const uint4 *gm = plane ? reinterpret_cast<const uint4 *>(plane) + lv : nullptr;
    // 32-bit partial counts: a chunk adds at most 32 words x 32 bits = 1024 to a pair, a workgroup runs at most
    // kPairMaxChunksPerSplit = 2^21 chunks (launch_moments_pairs), so acc <= 2^31 < 2^32; widened to 64 bits in the epilogue
    unsigned acc[R][R];
    for (int a = 0; a < R; ++a)
        for (int b = 0; b < R; ++b) acc[a][b] = 0;
    uint4 pa[LD], pb[LD];
    auto fetch = [&](int64_t c) {
        uint4 m = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (gm) m = gm[c * 8];
        for (int h = 0; h < LD; ++h) {
            pa[h] = g4[min(n - 1, ia + 32 * h) * wpr4 + c * 8];
            pb[h] = g4[min(n - 1, ib + 32 * h) * wpr4 + c * 8];
            pa[h].x &= m.x, pa[h].y &= m.y, pa[h].z &= m.z, pa[h].w &= m.w;
            pb[h].x &= m.x, pb[h].y &= m.y, pb[h].z &= m.z, pb[h].w &= m.w;
        }
    };
    fetch(c0);
    for (int64_t c = c0; c < c1; ++c) {
        for (int h = 0; h < LD; ++h) {
            sA[lrow + 32 * h][lv] = pa[h];
            sB[lrow + 32 * h][lv] = pb[h];
        }
        __syncthreads();
        if (c + 1 < c1) fetch(c + 1);
#pragma unroll 1
        for (int v = 0; v < 8; ++v) {
            uint4 B[R];
            for (int b = 0; b < R; ++b) B[b] = sB[tx + 16 * b][v];
            uint4 An = sA[ty][v];
            for (int a = 0; a < R; ++a) {
                const uint4 A = An;
                if (a + 1 < R) An = sA[ty + 16 * (a + 1)][v]; // (in flight while row a is counted)
                const unsigned Aw[4] = {A.x, A.y, A.z, A.w};
                // word by word, the R xors first and then the R counts, each adding into another accumulator: no instruction
                // waits for the one just before it
                for (int c = 0; c < 4; ++c) {
                    unsigned t[R];
                    for (int b = 0; b < R; ++b) t[b] = Aw[c] ^ (c == 0 ? B[b].x : c == 1 ? B[b].y : c == 2 ? B[b].z : B[b].w);
                    for (int b = 0; b < R; ++b) acc[a][b] = bcnt_add(t[b], acc[a][b]);
                }
            }
        }
        __syncthreads();
    }
    for (int a = 0; a < R; ++a) {
        const int64_t i = (int64_t)bi * T + ty + 16 * a;
        for (int b = 0; b < R; ++b) {
            const int64_t j = (int64_t)bj * T + tx + 16 * b;
            if (i < n && j < n && acc[a][b]) atomicAdd(&N[i * n + j], (unsigned long long)acc[a][b] << shift);
        }
    }
}

// N (upper triangle of T x T tiles) -> sum2 = M - 2 c N, in place, mirrored into the lower triangle through LDS so that both
// writes run along rows.  Same grid (x = column tile, y = row tile) and tile edge T as the pair kernel.
__global__ __launch_bounds__(256) void k_moments_pairs_finish(long long *__restrict__ S2, int64_t n, int T, long long M, long long c) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    __shared__ long long tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int si = 0; si < T; si += 32)
        for (int sj = 0; sj < T; sj += 32) {
            const int64_t i0 = (int64_t)bi * T + si, j0 = (int64_t)bj * T + sj;
            for (int r = ty; r < 32; r += 8) {
                const int64_t i = i0 + r, j = j0 + tx;
                long long v = 0;
                if (i < n && j < n) {
                    v = M - 2 * c * S2[i * n + j];
                    S2[i * n + j] = v;
                }
                tile[r][tx] = v;
            }
            __syncthreads();
            if (bi < bj)
                for (int r = ty; r < 32; r += 8) {
                    const int64_t j = j0 + r, i = i0 + tx;
                    if (i < n && j < n) S2[j * n + i] = tile[tx][r];
                }
            __syncthreads();
        }
}

void launch_moments_pairs(const DevProblem &d, const unsigned *planes, int nplanes, long long M, long long c, long long *S2, hipStream_t st) {
    const int64_t wpr = d.Kp / 32, nchunks = wpr / kPairChunkWords;
    const int T = kPairTile;
    const int64_t nt = (d.n + T - 1) / T, tiles = nt * (nt + 1) / 2;
    // K split: about 1024 workgroups (4 per CU) when K allows, never more than kPairMaxChunksPerSplit chunks per workgroup.
    // Integer sums: the split changes the time, never the result (measured: hardly the time either, once the device is full)
    const int64_t nsplit = std::min<int64_t>(std::min<int64_t>(nchunks, 65535),
                                             std::max<int64_t>((1024 + tiles - 1) / tiles, (nchunks + kPairMaxChunksPerSplit - 1) / kPairMaxChunksPerSplit));
    const int64_t cps = (nchunks + nsplit - 1) / nsplit;
    const dim3 grid((unsigned)nt, (unsigned)nt, (unsigned)((nchunks + cps - 1) / cps));
    auto *N = reinterpret_cast<unsigned long long *>(S2);
    for (int b = 0; b < std::max(1, nplanes); ++b) {
        const unsigned *pl = nplanes ? planes + (int64_t)b * wpr : nullptr;
        hipLaunchKernelGGL(k_moments_pairs, grid, dim3(256), 0, st, d.Sb, wpr, d.n, pl, b, cps, nchunks, N);
    }
    hipLaunchKernelGGL(k_moments_pairs_finish, dim3((unsigned)nt, (unsigned)nt), dim3(256), 0, st, S2, d.n, T, M, c);
}

// ---- term counts: one wave per term and K range -------------------------------------------------------------------------------
// Nt[t] += sum over the words [w0, w1) of popcount(XOR of the key's rows) (nplanes = 0) or sum_b 2^b popcount(XOR & C_b).
// keys [nterms][L]: the distinct spins of every key, -1 = unused slot.  A lane reads 16 bytes per row and step; 64-bit sums.
__global__ __launch_bounds__(256) void k_moments_terms(const unsigned *__restrict__ Sb, int64_t wpr, const int32_t *__restrict__ keys, int L,
                                                       int64_t nterms, const unsigned *__restrict__ planes, int nplanes,
                                                       int64_t words_per_split, unsigned long long *__restrict__ Nt) {
    const int lane = threadIdx.x & 63;
    const int64_t t = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (int64_t)blockIdx.x * 4;
    if (t >= nterms) return;
    const int64_t q0 = (int64_t)blockIdx.y * words_per_split / 4, q1 = min(wpr, ((int64_t)blockIdx.y + 1) * words_per_split) / 4;
    const int32_t *key = keys + t * L;
    unsigned long long acc = 0;
    for (int64_t q = q0 + lane; q < q1; q += 64) {
        uint4 x = make_uint4(0, 0, 0, 0);
        for (int a = 0; a < L; ++a) {
            const int s = key[a];
            if (s < 0) continue;
            const uint4 r = reinterpret_cast<const uint4 *>(Sb + (int64_t)s * wpr)[q];
            x.x ^= r.x, x.y ^= r.y, x.z ^= r.z, x.w ^= r.w;
        }
        if (nplanes == 0) acc += __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w);
        else
            for (int b = 0; b < nplanes; ++b) {
                const uint4 m = reinterpret_cast<const uint4 *>(planes + (int64_t)b * wpr)[q];
                acc += (unsigned long long)(__popc(x.x & m.x) + __popc(x.y & m.y) + __popc(x.z & m.z) + __popc(x.w & m.w)) << b;
            }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0 && acc) atomicAdd(&Nt[t], acc);
}

void launch_moments_terms(const DevProblem &d, const int32_t *keys, int L, int64_t nterms, const unsigned *planes, int nplanes,
                          unsigned long long *Nt, hipStream_t st) {
    const int64_t wpr = d.Kp / 32;
    // K split (in steps of 256 words = one uint4 per lane) so that few terms over many configurations still fill the device
    const int64_t steps = (wpr + 255) / 256;
    const int64_t nsplit = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(steps, 65535), 4096 / std::max<int64_t>(1, nterms)));
    const int64_t wps = (steps + nsplit - 1) / nsplit * 256;
    const unsigned gy = (unsigned)((wpr + wps - 1) / wps);
    const int64_t batch = (int64_t)1 << 30; // terms per launch (grid.x)
    for (int64_t t0 = 0; t0 < nterms; t0 += batch) {
        const int64_t nt = std::min(batch, nterms - t0);
        hipLaunchKernelGGL(k_moments_terms, dim3((unsigned)((nt + 3) / 4), gy), dim3(256), 0, st, d.Sb, wpr, keys + t0 * L, L, nt, planes,
                           nplanes, wps, Nt + t0);
    }
}

void launch_count_planes(const DevProblem &d, double M, int nplanes, unsigned *planes, hipStream_t st) {
    const int64_t wpr = d.Kp / 32;
    hipLaunchKernelGGL(k_count_planes, dim3((unsigned)((wpr + 255) / 256), (unsigned)nplanes), dim3(256), 0, st, d.w, M, d.K, wpr, planes);
}

} // namespace gml
