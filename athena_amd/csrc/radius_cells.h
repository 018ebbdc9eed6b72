// What the radius builders share beyond the cell grid (radius_graph.hip: points of one set; bipartite_graph.hip: queries against
// sources): the predicate, term by term, and how wide the cells of a cloud's grid are.  The margin argument that ties the two
// together is in the header of radius_graph.hip.  Unnamed namespace: one copy per file that includes this.
#pragma once
#include <math.h>

#include <algorithm>

#include "cell_grid.h"

namespace {

constexpr double kCellMargin = 1.0 / 1024.0;

// ---- the predicate, term by term in fp32 (-ffp-contract=off: no fused multiply-add) --------------------------------------------
template <int DIM> __device__ inline bool joined(const float *__restrict__ a, const float *__restrict__ b, float r2)
{
    const float d0 = a[0] - b[0];
    float s = d0 * d0;
    if (DIM > 1) {
        const float d1 = a[1] - b[1];
        s = s + d1 * d1;
    }
    if (DIM > 2) {
        const float d2 = a[2] - b[2];
        s = s + d2 * d2;
    }
    return s <= r2;
}

// at most kMaxCellsAxis cells per axis and 2 n in all, every cell at least radius * (1 + kCellMargin) wide; an axis whose extent
// is below that is one cell
inline Grid make_grid(const Box &box, int dim, int32_t n, float radius)
{
    Grid g;
    double extent[3] = {0, 0, 0};
    const double h = (double)radius * (1.0 + kCellMargin);
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = a < dim ? box.lo[a] : 0.f;
        g.nc[a] = 1;
        if (a < dim) {
            extent[a] = (double)box.hi[a] - (double)box.lo[a];
            const double cells = floor(extent[a] / h);
            g.nc[a] = cells < 1.0 ? 1 : cells > (double)kMaxCellsAxis ? kMaxCellsAxis : (int32_t)cells;
        }
    }
    const int64_t cap = std::min<int64_t>(2 * (int64_t)n, (int64_t)1 << 30);
    while ((int64_t)g.nc[0] * g.nc[1] * g.nc[2] > cap) {
        int a = 0;
        for (int k = 1; k < 3; ++k)
            if (g.nc[k] > g.nc[a]) a = k;
        g.nc[a] = (g.nc[a] + 1) / 2;
    }
    for (int a = 0; a < 3; ++a) g.inv_w[a] = g.nc[a] > 1 ? (float)((double)g.nc[a] / extent[a]) : 0.f;
    return g;
}

} // namespace
