// What the two-set builders share beyond the cell grid (bipartite_graph.hip: queries against sources by radius;
// knn_bipartite.hip: by k nearest neighbours): the check of their two offset arrays, and rowptr and edge_offsets from the scan of
// the queries' counts.  Unnamed namespace: one copy per file that includes this.
#pragma once
#include "cell_grid.h"
#include "common.h"

namespace {

// batch_offsets_check of cell_grid.h with the array named: two offset arrays enter here
inline int named_offsets_check(const char *who, const char *name, const char *unit, int32_t B, const int32_t *offsets, int32_t n)
{
    AMP_REQUIRE(offsets != nullptr, "%s: null %s", who, name);
    AMP_REQUIRE(offsets[0] == 0, "%s: %s(1) = %d, not 0", who, name, offsets[0]);
    for (int32_t b = 0; b < B; ++b)
        AMP_REQUIRE(offsets[b + 1] >= offsets[b], "%s: cloud %d: %s descend from %d to %d", who, b + 1, name, offsets[b], offsets[b + 1]);
    AMP_REQUIRE(offsets[B] == n, "%s: %s end at %d, the batch has %d %s", who, name, offsets[B], n, unit);
    return 0;
}

// rowptr [nq + 1] (int32, may be null) and edge_offsets [B + 1] from the scan; total < 2^31 is the caller's to check
__global__ __launch_bounds__(256) void bip_rowptr_kernel(int32_t nq, int32_t B, const int32_t *__restrict__ q_offsets,
                                                         const unsigned long long *__restrict__ offset,
                                                         const unsigned long long *__restrict__ total, int32_t *__restrict__ rowptr,
                                                         long long *__restrict__ edge_offsets)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (rowptr && t <= nq) rowptr[t] = (int32_t)(t < nq ? offset[t] : *total);
    if (edge_offsets && t <= B) {
        const int32_t v = q_offsets[t];
        edge_offsets[t] = (long long)(v < nq ? offset[v] : *total);
    }
}

} // namespace
