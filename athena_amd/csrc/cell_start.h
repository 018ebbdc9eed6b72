// What every builder that sorts its points by cell needs after the sort, whatever its cells are (cell_grid.h for the point-cloud
// builders, periodic_graph.hip for its fractional grid): the cell starts, and the two launch helpers around them.  The kernel is
// in an unnamed namespace: one copy per file that includes this.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// cell_start[c] = first slot whose sorted key is >= c  (c = 0 .. n_cells)
__global__ __launch_bounds__(256) void rg_cell_start_kernel(uint32_t n_cells, const uint32_t *__restrict__ sorted_key, int32_t n,
                                                            int32_t *__restrict__ cell_start)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > (int64_t)n_cells) return;
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)sorted_key[mid] < c) lo = mid + 1; else hi = mid;
    }
    cell_start[c] = lo;
}

inline unsigned blocks(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }
inline int bits_for(unsigned long long max_value)
{
    int b = 1;
    while (b < 64 && (max_value >> b)) ++b;
    return b;
}

} // namespace
