// What the geometry entries share around their kernels, beside the carver of pieces.h and the staging of amp::Scratch (common.h):
// the word that kernels leave their smallest refused element in, and the longest row of a row pointer.  Unnamed namespace: one copy
// per file that includes this.
#pragma once
#include <algorithm>

#include "cell_start.h"
#include "common.h"
#include "pieces.h"

namespace {

// Armed to ~0; kernels atomicMin the index of what they refuse into *dev; the host reads the smallest back.
struct BadWord {
    unsigned long long *dev = nullptr;
    int arm(amp::Scratch &tmp, hipStream_t st)
    {
        static const unsigned long long none = ~0ull;
        if (tmp.get(&dev, 1)) return 1;
        AMP_HIP(hipMemcpyAsync(dev, &none, sizeof(none), hipMemcpyHostToDevice, st));
        return 0;
    }
    // *bad = the word (~0: nothing was refused); waits for the stream
    int fetch(unsigned long long *bad, hipStream_t st)
    {
        AMP_HIP(hipMemcpyAsync(bad, dev, sizeof(*bad), hipMemcpyDeviceToHost, st));
        AMP_HIP(hipStreamSynchronize(st));
        return 0;
    }
    // 0, or 2 with "<who>: <name>(<element>) = <value> outside [lo,hi]"
    int read(const char *who, const char *name, const int32_t *ids_dev, int32_t lo, int32_t hi, hipStream_t st)
    {
        unsigned long long bad = ~0ull;
        if (int rc = fetch(&bad, st)) return rc;
        if (bad == ~0ull) return 0;
        int32_t id = 0;
        AMP_HIP(hipMemcpy(&id, ids_dev + bad, sizeof(id), hipMemcpyDeviceToHost));
        amp::set_error("%s: %s(%llu) = %d outside [%d,%d]", who, name, bad + 1, id, lo, hi);
        return 2;
    }
};

constexpr int kLongestBlocks = 512;          // block partials of longest_row

// the largest row of rowptr [m + 1]: one partial per block, folded on the host
__global__ __launch_bounds__(256) void longest_row_kernel(int32_t m, const int32_t *__restrict__ rowptr, int32_t *__restrict__ partial)
{
    __shared__ int32_t part[4];
    int32_t best = 0;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < m; r += (int64_t)gridDim.x * 256) best = max(best, rowptr[r + 1] - rowptr[r]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) best = max(best, __shfl_xor(best, d, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = max(max(part[0], part[1]), max(part[2], part[3]));
}

// *longest = the largest rowptr[r + 1] - rowptr[r] over r < m, 0 where m == 0; partial: kLongestBlocks device words.  Waits for the stream.
inline int longest_row(int32_t m, const int32_t *rowptr, int32_t *partial, int32_t *longest, hipStream_t st)
{
    int32_t part[kLongestBlocks];
    const int n_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(kLongestBlocks, blocks(m)));
    hipLaunchKernelGGL(longest_row_kernel, dim3(n_blocks), dim3(256), 0, st, m, rowptr, partial);
    AMP_LAUNCH_CHECK();
    AMP_HIP(hipMemcpyAsync(part, partial, sizeof(int32_t) * n_blocks, hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    *longest = *std::max_element(part, part + n_blocks);
    return 0;
}

} // namespace
