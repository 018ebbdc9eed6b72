// Exclusive scan of n counts into 64-bit offsets, in index order: tile sums, one block that scans the tiles, one pass that
// applies them; exclusive() launches the three.  Deterministic (no atomics).  Included by radius_graph.hip (counts per point),
// knn_graph.hip (flags per key) and periodic_graph.hip (counts per grid atom and per work item); the kernels are templates or
// static, one copy per file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace scan64 {

constexpr int kPer = 16;
constexpr int kTile = 256 * kPer;

inline uint32_t tiles(int64_t n) { return (uint32_t)((n + kTile - 1) / kTile); }

__device__ inline unsigned long long block_scan(unsigned long long v, unsigned long long *total)
{
    __shared__ unsigned long long wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned long long off = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) off += wsum[w];
        all += wsum[w];
    }
    __syncthreads();
    *total = all;
    return off + inc - v;
}

template <typename C>
__global__ __launch_bounds__(256) void tile_sum_kernel(int64_t n, const C *__restrict__ count, unsigned long long *__restrict__ tile_sum)
{
    const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPer;
    unsigned long long s = 0;
    for (int k = 0; k < kPer; ++k)
        if (base + k < n) s += count[base + k];
    unsigned long long total;
    (void)block_scan(s, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one block: tile_sum becomes the tiles' exclusive offsets, tile_sum[tiles] the grand total
static __global__ __launch_bounds__(256) void scan_tiles_kernel(uint32_t tiles, unsigned long long *__restrict__ tile_sum)
{
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < tiles; base += 256) {
        const uint32_t t = base + threadIdx.x;
        const unsigned long long v = t < tiles ? tile_sum[t] : 0ull;
        unsigned long long total;
        const unsigned long long ex = block_scan(v, &total);
        if (t < tiles) tile_sum[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tile_sum[tiles] = carry;
}

template <typename C>
__global__ __launch_bounds__(256) void apply_kernel(int64_t n, const C *__restrict__ count, const unsigned long long *__restrict__ tile_off,
                                                    unsigned long long *__restrict__ offset)
{
    const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPer;
    C c[kPer];
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        c[k] = base + k < n ? count[base + k] : (C)0;
        s += c[k];
    }
    unsigned long long total;
    unsigned long long run = tile_off[blockIdx.x] + block_scan(s, &total);
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        if (base + k < n) offset[base + k] = run;
        run += c[k];
    }
}

// The three passes on stream st: offset[i] = count[0] + ... + count[i - 1], i < n.  tile_sum holds tiles(n) + 1 words; the grand
// total is left in the last of them, and that device address is returned.
template <typename C>
inline const unsigned long long *exclusive(int64_t n, const C *count, unsigned long long *tile_sum, unsigned long long *offset, hipStream_t st)
{
    const uint32_t t = tiles(n);
    hipLaunchKernelGGL(tile_sum_kernel<C>, dim3(t), dim3(256), 0, st, n, count, tile_sum);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(256), 0, st, t, tile_sum);
    hipLaunchKernelGGL(apply_kernel<C>, dim3(t), dim3(256), 0, st, n, count, (const unsigned long long *)tile_sum, offset);
    return tile_sum + t;
}

} // namespace scan64
