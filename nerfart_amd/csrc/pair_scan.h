// pair_scan.h - the exclusive scan of pairs of counts over a linear array that csrc/marching_cubes.hip (vertices per point, triangles per cell)
// and csrc/mesh_components.hip (vertex survives, face survives) both compact with: per 512-item block (wave64 shuffles + LDS) with block sums,
// the same scan on the block sums until one block is left - whose sums are the two totals - and an add-back on the way down.  Every kernel runs
// to completion on its own: no workgroup ever waits for another.  No atomics: the offsets are a pure function of the items.
//   first level    the user's own kernel: pair_scan_block(item, off, n, pair_scan_sums(L, 0, totals)) with item(i) -> the pair of item i;
//   the rest       pair_scan_finish(off, n, L, totals, stream).
#pragma once
#include "host_util.h"

namespace nerfart {

constexpr int PAIR_SCAN_BLOCK = 512;     // items per scan block: 256 threads x 2 (tests/test_gpu_marching_cubes.py states it)
constexpr int PAIR_SCAN_MAX_LEVELS = 4;  // n < 2^31 items / 512^3 < 16: at most three block-sum levels live in the workspace

// the block-sum levels, carved after the user's own buffers (each rounded up to 256 bytes): per level k its [m_k][2] sums,
// m_0 = ceil(n / 512), m_{k+1} = ceil(m_k / 512), while m_k > 1
struct PairScanLevels {
    unsigned* lvl[PAIR_SCAN_MAX_LEVELS];
    unsigned lvl_m[PAIR_SCAN_MAX_LEVELS];
    int n_lvl;
};
inline void pair_scan_carve(Carver& c, size_t n, PairScanLevels& L) {
    L.n_lvl = 0;
    for (size_t m = (n + PAIR_SCAN_BLOCK - 1) / PAIR_SCAN_BLOCK; m > 1 && L.n_lvl < PAIR_SCAN_MAX_LEVELS; m = (m + PAIR_SCAN_BLOCK - 1) / PAIR_SCAN_BLOCK) {
        L.lvl[L.n_lvl] = c.take<unsigned>(2 * m);
        L.lvl_m[L.n_lvl++] = (unsigned)m;
    }
}
// where the block sums of level k - 1 go (k = 0: of the items): the next level, or - from the last, one-block level - the caller's totals [2]
inline uint2* pair_scan_sums(const PairScanLevels& L, int k, unsigned* totals) { return (uint2*)(k < L.n_lvl ? L.lvl[k] : totals); }
inline dim3 pair_scan_blocks(unsigned m) { return dim3((m + PAIR_SCAN_BLOCK - 1) / PAIR_SCAN_BLOCK); }

// One 512-item block of the exclusive scan of pairs, for a 256-thread block: arr[i] = (sum of x before i, sum of y before i) within the block,
// sums[block] = the block's totals.  item(i) -> uint2, asked only for i < m.
template <class Item>
__device__ __forceinline__ void pair_scan_block(Item item, uint2* arr, unsigned m, uint2* __restrict__ sums) {
    __shared__ unsigned wave_tot[4][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t i0 = (size_t)blockIdx.x * PAIR_SCAN_BLOCK + 2 * threadIdx.x;
    unsigned v[2] = {0, 0}, t[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (i0 + k < m) { const uint2 a = item(i0 + k); v[k] = a.x; t[k] = a.y; }
    }
    const unsigned sv = v[0] + v[1], st = t[0] + t[1];
    unsigned iv = sv, it = st;                       // inclusive over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned a = __shfl_up(iv, d, 64), b = __shfl_up(it, d, 64);
        if (lane >= d) { iv += a; it += b; }
    }
    if (lane == 63) { wave_tot[w][0] = iv; wave_tot[w][1] = it; }
    __syncthreads();
    unsigned ev = iv - sv, et = it - st;             // exclusive at this thread's first item
    for (int j = 0; j < w; ++j) { ev += wave_tot[j][0]; et += wave_tot[j][1]; }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (i0 + k < m) arr[i0 + k] = make_uint2(ev, et);
        ev += v[k]; et += t[k];
    }
    if (threadIdx.x == 255) sums[blockIdx.x] = make_uint2(ev, et);
}

// the block sums, scanned in place (arr is read as the items and written as the offsets: no __restrict__ on it)
static __global__ void __launch_bounds__(256) k_pair_scan(uint2* arr, unsigned m, uint2* __restrict__ sums) {
    pair_scan_block([&](size_t i) { return arr[i]; }, arr, m, sums);
}

// arr[i] += sums[i / 512] (sums already scanned: the offset of the block)
static __global__ void __launch_bounds__(256) k_pair_scan_add_back(uint2* __restrict__ arr, unsigned m, const uint2* __restrict__ sums) {
    const uint2 s = sums[blockIdx.x];
    const size_t i0 = (size_t)blockIdx.x * PAIR_SCAN_BLOCK + 2 * threadIdx.x;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (i0 + k < m) { uint2 a = arr[i0 + k]; a.x += s.x; a.y += s.y; arr[i0 + k] = a; }
    }
}

// After the first level (off [n] scanned per block, its sums in pair_scan_sums(L, 0, totals)): up - each level's block sums are the next level's
// items, the last level is one block, whose sums are the totals; down - level k is complete once level k + 1 has been added to it.
inline int pair_scan_finish(unsigned* off, unsigned n, const PairScanLevels& L, unsigned* totals, hipStream_t st) {
    for (int k = 0; k < L.n_lvl; ++k) {
        hipLaunchKernelGGL(k_pair_scan, pair_scan_blocks(L.lvl_m[k]), dim3(256), 0, st, (uint2*)L.lvl[k], L.lvl_m[k], pair_scan_sums(L, k + 1, totals));
        NERFART_HIP(hipGetLastError());
    }
    for (int k = L.n_lvl - 1; k >= 0; --k) {
        uint2* below = (uint2*)(k ? L.lvl[k - 1] : off);
        const unsigned m = k ? L.lvl_m[k - 1] : n;
        hipLaunchKernelGGL(k_pair_scan_add_back, pair_scan_blocks(m), dim3(256), 0, st, below, m, (const uint2*)L.lvl[k]);
        NERFART_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace nerfart
