// What the k-nearest-neighbour builders share beyond the cell grid (knn_graph.hip: the points of one set; knn_bipartite.hip:
// queries against sources): the squared distance term by term, the 64-bit key and the sort and merge of keys across the lanes of
// a wave, the constants of the stop rule, how wide the cells of a cloud's grid are, and the fold of the search statistics.  The
// proof that ties kMargin, kShrink and w_low together is in the header of knn_graph.hip; knn_bipartite.hip re-derives it for a
// query that may lie anywhere.  Unnamed namespace: one copy per file that includes this.
#pragma once
#include <float.h>
#include <math.h>

#include <algorithm>

#include "cell_grid.h"
#include "common.h"

namespace amp {
extern int64_t g_knn_stats[4];               // athena_mp_knn_stats: of the last k-nearest-neighbour call (knn_graph.hip)
}

namespace {

constexpr double kGridPoints = 2.0;          // points per cell the grid aims for -- not measured yet
constexpr float kMargin = 1.0f / 1024.0f;    // 2^-10: the header's bound on what the computed cell coordinates can hide
constexpr float kShrink = 1.0f - 0x1p-20f;   // covers the roundings of s and of the bound itself (header)
constexpr unsigned long long kNoKey = ~0ull;
constexpr int kQueryWaves = 4;               // query points per 256-thread block

struct WLow {
    float w[3];                              // 1 / inv_w rounded down, per axis (unused where nc = 1)
};

// the squared distance of the definition, term by term in fp32 (-ffp-contract=off: no fused multiply-add)
template <int DIM> __device__ inline float sq_dist(const float *p, const float *q)
{
    const float d0 = p[0] - q[0];
    float s = d0 * d0;
    if (DIM > 1) {
        const float d1 = p[1] - q[1];
        s = s + d1 * d1;
    }
    if (DIM > 2) {
        const float d2 = p[2] - q[2];
        s = s + d2 * d2;
    }
    return s;
}

__device__ inline unsigned long long key_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ inline unsigned long long key_max(unsigned long long a, unsigned long long b) { return a < b ? b : a; }

// the 64 keys of a wave, one per lane, ascending by lane
__device__ inline unsigned long long wave_sort(unsigned long long c, int lane)
{
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
        const bool up = (lane & size) == 0;                  // the last round (size 64) ascends in every lane
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const unsigned long long o = __shfl_xor(c, stride, 64);
            const bool low = (lane & stride) == 0;
            c = low == up ? key_min(c, o) : key_max(c, o);
        }
    }
    return c;
}

// list and step both ascending by lane: the 64 smallest keys of the two, ascending by lane
__device__ inline unsigned long long wave_merge(unsigned long long list, unsigned long long step, int lane)
{
    unsigned long long c = key_min(list, __shfl(step, 63 - lane, 64));     // bitonic, and it holds the 64 smallest
#pragma unroll
    for (int stride = 32; stride > 0; stride >>= 1) {
        const unsigned long long o = __shfl_xor(c, stride, 64);
        c = (lane & stride) == 0 ? key_min(c, o) : key_max(c, o);
    }
    return c;
}

// stat [3][n] -> out[block] = {sum, sum, max}: block partials, folded on the host in block order
constexpr int kStatBlocks = 256;
__global__ __launch_bounds__(256) void knn_stat_kernel(int32_t n, const uint32_t *__restrict__ stat, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long part[3][256];
    unsigned long long c = 0, v = 0, r = 0;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < n; s += (int64_t)gridDim.x * 256) {
        c += stat[s];
        v += stat[(int64_t)n + s];
        const unsigned long long x = stat[2 * (int64_t)n + s];
        r = x > r ? x : r;
    }
    part[0][threadIdx.x] = c;
    part[1][threadIdx.x] = v;
    part[2][threadIdx.x] = r;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            part[0][threadIdx.x] += part[0][threadIdx.x + s];
            part[1][threadIdx.x] += part[1][threadIdx.x + s];
            part[2][threadIdx.x] = key_max(part[2][threadIdx.x], part[2][threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) out[3 * blockIdx.x + threadIdx.x] = part[threadIdx.x][0];
}

// g_knn_stats = {queries, candidates examined, cells visited, the largest shell} from the block partials of knn_stat_kernel
inline void knn_stats_fold(int64_t queries, int stat_blocks, const unsigned long long *stat_part)
{
    int64_t *g = amp::g_knn_stats;
    g[0] = queries;
    g[1] = g[2] = g[3] = 0;
    for (int s = 0; s < stat_blocks; ++s) {
        g[1] += (int64_t)stat_part[3 * s];
        g[2] += (int64_t)stat_part[3 * s + 1];
        g[3] = std::max(g[3], (int64_t)stat_part[3 * s + 2]);
    }
}

inline float round_down(double v)
{
    float f = (float)v;
    if ((double)f > v) f = nextafterf(f, 0.f);
    return f;
}

// About kGridPoints points per cell, at most kMaxCellsAxis cells per axis and 2 m in all.  An axis of zero extent is one cell; so
// is one whose inv_w would not be a normal fp32 number with the relative accuracy the header's proof uses.
inline Grid make_knn_grid(const Box &box, int dim, int32_t m, WLow *wl)
{
    Grid g;
    double extent[3] = {0, 0, 0}, volume = 1.0;
    int active = 0;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = a < dim ? box.lo[a] : 0.f;
        g.nc[a] = 1;
        g.inv_w[a] = 0.f;
        wl->w[a] = 0.f;
        if (a < dim) extent[a] = (double)box.hi[a] - (double)box.lo[a];
        if (extent[a] > 0.0 && extent[a] < 1e37) {
            volume *= extent[a];
            ++active;
        } else {
            extent[a] = 0.0;
        }
    }
    if (active == 0) return g;
    const double want = std::max(1.0, (double)m / kGridPoints);
    const double w = pow(volume / want, 1.0 / active);
    for (int a = 0; a < 3; ++a) {
        if (extent[a] == 0.0) continue;
        const double cells = floor(extent[a] / w);
        g.nc[a] = !(cells >= 1.0) ? 1 : cells > (double)kMaxCellsAxis ? kMaxCellsAxis : (int32_t)cells;
    }
    const int64_t cap = std::min<int64_t>(2 * (int64_t)m, (int64_t)1 << 30);
    while ((int64_t)g.nc[0] * g.nc[1] * g.nc[2] > cap) {
        int a = 0;
        for (int c = 1; c < 3; ++c)
            if (g.nc[c] > g.nc[a]) a = c;
        g.nc[a] = (g.nc[a] + 1) / 2;
    }
    for (int a = 0; a < 3; ++a) {
        if (g.nc[a] <= 1) continue;
        const float inv_w = (float)((double)g.nc[a] / extent[a]);
        if (!(inv_w >= 1e-30f && inv_w <= 1e30f)) {
            g.nc[a] = 1;
            continue;
        }
        g.inv_w[a] = inv_w;
        wl->w[a] = round_down((1.0 / (double)inv_w) * (1.0 - 0x1p-30));
    }
    return g;
}

} // namespace
