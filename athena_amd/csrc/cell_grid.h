// The uniform cell grid of the point-cloud builders (radius_graph.hip, knn_graph.hip): bounding boxes with the first non-finite
// point, cell keys in disjoint ranges per cloud, positions in cell order, cell starts.  What a cell is -- floor(fl(fl(p - lo) *
// inv_w)) clamped to the axis -- is defined here once; how wide the cells are is each builder's own choice (make_grid there).
// The kernels are in an unnamed namespace: one copy per file that includes this.
#pragma once
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int kMaxCellsAxis = 2048;

struct Box {
    float lo[3], hi[3];
    unsigned long long first_bad;   // smallest index of a point with a non-finite coordinate, ~0 if none
};

struct Grid {
    float lo[3], inv_w[3];
    int32_t nc[3];
};

// ---- bounding box + validity: block partials, then one block folds them in block order -------------------------------------
__device__ inline void box_fold(Box &a, const Box &b)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.lo[k] = fminf(a.lo[k], b.lo[k]);
        a.hi[k] = fmaxf(a.hi[k], b.hi[k]);
    }
    a.first_bad = b.first_bad < a.first_bad ? b.first_bad : a.first_bad;
}

__device__ inline Box box_block_reduce(Box b)
{
    __shared__ Box part[256];
    part[threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) box_fold(part[threadIdx.x], part[threadIdx.x + s]);
        __syncthreads();
    }
    return part[0];
}

__device__ inline Box box_empty()
{
    Box b;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = INFINITY;
        b.hi[k] = -INFINITY;
    }
    b.first_bad = ~0ull;
    return b;
}

__global__ __launch_bounds__(256) void rg_box_kernel(int32_t n, int dim, const float *__restrict__ pts, Box *__restrict__ partial)
{
    Box b = box_empty();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        bool ok = true;
        for (int k = 0; k < dim; ++k) {
            const float v = pts[i * dim + k];
            ok = ok && isfinite(v);
            b.lo[k] = fminf(b.lo[k], v);
            b.hi[k] = fmaxf(b.hi[k], v);
        }
        if (!ok && (unsigned long long)i < b.first_bad) b.first_bad = (unsigned long long)i;
    }
    b = box_block_reduce(b);
    if (threadIdx.x == 0) partial[blockIdx.x] = b;
}

__global__ __launch_bounds__(256) void rg_box_final_kernel(int n_partial, const Box *__restrict__ partial, Box *__restrict__ out)
{
    Box b = box_empty();
    for (int i = threadIdx.x; i < n_partial; i += 256) box_fold(b, partial[i]);
    b = box_block_reduce(b);
    if (threadIdx.x == 0) *out = b;
}

// ---- grid ------------------------------------------------------------------------------------------------------------------
// the cell coordinate before the floor: two roundings, each within 2^-24 relative
__device__ inline float cell_q(float p, float lo, float inv_w) { return (p - lo) * inv_w; }

__device__ inline int32_t cell_coord(float p, float lo, float inv_w, int32_t nc)
{
    const float q = cell_q(p, lo, inv_w);
    const int32_t c = (int32_t)q;             // q >= 0 and finite: truncation is floor
    return c < nc - 1 ? c : nc - 1;
}

__global__ __launch_bounds__(256) void rg_cell_key_kernel(int32_t n, int dim, const float *__restrict__ pts, Grid g,
                                                          uint32_t *__restrict__ key)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t c = 0;
    for (int k = dim - 1; k >= 0; --k) c = c * (uint32_t)g.nc[k] + (uint32_t)cell_coord(pts[i * dim + k], g.lo[k], g.inv_w[k], g.nc[k]);
    key[i] = c;
}

// positions in cell order: a cell's points are one contiguous read
__global__ __launch_bounds__(256) void rg_gather_points_kernel(int32_t n, int dim, const float *__restrict__ pts,
                                                               const int32_t *__restrict__ perm, float *__restrict__ sorted)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int64_t i = perm[k];
    for (int a = 0; a < dim; ++a) sorted[k * dim + a] = pts[i * dim + a];
}

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

inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
inline int bits_for(unsigned long long max_value)
{
    int b = 1;
    while (b < 64 && (max_value >> b)) ++b;
    return b;
}

constexpr int kItemPoints = 4096;
constexpr int kItemWaves = 4;        // work items per 256-thread block

__device__ inline Box box_wave_reduce(Box b)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        Box o;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o.lo[k] = __shfl_xor(b.lo[k], d, 64);
            o.hi[k] = __shfl_xor(b.hi[k], d, 64);
        }
        o.first_bad = __shfl_xor(b.first_bad, d, 64);
        box_fold(b, o);
    }
    return b;
}

// one wave per work item (cloud, p0, p1): the box and the first non-finite point of points p0 .. p1-1 -> partial[item]
__global__ __launch_bounds__(64 * kItemWaves) void rgb_box_item_kernel(int32_t n_items, const int32_t *__restrict__ items, int dim,
                                                                       const float *__restrict__ pts, Box *__restrict__ partial)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * kItemWaves + (threadIdx.x >> 6);
    if (w >= n_items) return;
    const int32_t p0 = items[3 * w + 1], p1 = items[3 * w + 2];
    Box b = box_empty();
    for (int64_t i = (int64_t)p0 + lane; i < p1; i += 64) {
        bool ok = true;
        for (int k = 0; k < dim; ++k) {
            const float v = pts[i * dim + k];
            ok = ok && isfinite(v);
            b.lo[k] = fminf(b.lo[k], v);
            b.hi[k] = fmaxf(b.hi[k], v);
        }
        if (!ok && (unsigned long long)i < b.first_bad) b.first_bad = (unsigned long long)i;
    }
    b = box_wave_reduce(b);
    if (lane == 0) partial[w] = b;
}

// one thread per cloud: its items' partials in item order (an empty cloud has no item: the empty box).  first_bad stays per
// cloud; the host, which reads every box anyway, takes the smallest
__global__ __launch_bounds__(256) void rgb_box_cloud_kernel(int32_t B, const int32_t *__restrict__ item_first,
                                                            const Box *__restrict__ partial, Box *__restrict__ out)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    Box x = box_empty();
    for (int32_t w = item_first[b]; w < item_first[b + 1]; ++w) box_fold(x, partial[w]);
    out[b] = x;
}

// one wave per work item, so the cloud is known without a search: key = cell_base[cloud] + the cell in the cloud's own grid
__global__ __launch_bounds__(64 * kItemWaves) void rgb_cell_key_kernel(int32_t n_items, const int32_t *__restrict__ items, int dim,
                                                                       const float *__restrict__ pts, const Grid *__restrict__ grids,
                                                                       const uint32_t *__restrict__ cell_base, uint32_t *__restrict__ key)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * kItemWaves + (threadIdx.x >> 6);
    if (w >= n_items) return;
    const int32_t b = items[3 * w], p0 = items[3 * w + 1], p1 = items[3 * w + 2];
    const Grid g = grids[b];
    const uint32_t base = cell_base[b];
    for (int64_t i = (int64_t)p0 + lane; i < p1; i += 64) {
        uint32_t c = 0;
        for (int k = dim - 1; k >= 0; --k)
            c = c * (uint32_t)g.nc[k] + (uint32_t)cell_coord(pts[i * dim + k], g.lo[k], g.inv_w[k], g.nc[k]);
        key[i] = base + c;
    }
}

// the cloud of point i, 0 <= i < offsets[B]: the last b with offsets[b] <= i (empty clouds repeat a value and own no point)
__device__ inline int32_t cloud_of(int32_t B, const int32_t *__restrict__ offsets, int32_t i)
{
    int32_t lo = 0, hi = B;                       // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// the checks every batched entry makes on its offsets before anything touches the device: 0, or 2 with the message set
inline int batch_offsets_check(const char *who, int32_t B, const int32_t *offsets)
{
    AMP_REQUIRE(B >= 0, "%s: n_clouds = %d is negative", who, B);
    AMP_REQUIRE(offsets != nullptr, "%s: null offsets", who);
    AMP_REQUIRE(offsets[0] == 0, "%s: offsets(1) = %d, not 0", who, offsets[0]);
    for (int32_t b = 0; b < B; ++b)
        AMP_REQUIRE(offsets[b + 1] >= offsets[b], "%s: cloud %d: offsets descend from %d to %d", who, b + 1, offsets[b], offsets[b + 1]);
    return 0;
}

// The clouds cut into work items (cloud, points p0 .. p1-1) of at most kItemPoints points, in order of (cloud, first point), and
// what the kernels above need of them on the device.
struct BatchItems {
    std::vector<int32_t> items, item_first;      // item_first[b] = the first item of cloud b or of a later one
    int32_t W = 0, m_max = 0;                    // items (W <= n: only non-empty clouds have one), points of the largest cloud
    unsigned item_blocks = 0;
    int32_t *d_items = nullptr, *d_item_first = nullptr, *d_off = nullptr;
};

// items, their upload, and the bounding box of every cloud brought home; a non-finite coordinate is refused here, naming the
// cloud, component and point of the first one.  n > 0.  Synchronises the stream.
inline int batch_boxes(const char *who, int32_t B, const int32_t *offsets, int32_t dim, const float *points_dev, hipStream_t st,
                       amp::Scratch &tmp, BatchItems &it, std::vector<Box> &box)
{
    it.item_first.resize((size_t)B + 1);
    for (int32_t b = 0; b < B; ++b) {
        it.item_first[b] = (int32_t)(it.items.size() / 3);
        it.m_max = std::max(it.m_max, offsets[b + 1] - offsets[b]);
        for (int64_t p0 = offsets[b]; p0 < offsets[b + 1]; p0 += kItemPoints)
            it.items.insert(it.items.end(), {b, (int32_t)p0, (int32_t)std::min<int64_t>(p0 + kItemPoints, offsets[b + 1])});
    }
    const int32_t W = it.W = (int32_t)(it.items.size() / 3);
    it.item_first[B] = W;

    Box *d_partial = nullptr, *d_box = nullptr;
    if (tmp.get(&it.d_items, it.items.size()) || tmp.get(&it.d_item_first, (size_t)B + 1) || tmp.get(&it.d_off, (size_t)B + 1) ||
        tmp.get(&d_partial, W) || tmp.get(&d_box, B))
        return 1;
    AMP_HIP(hipMemcpyAsync(it.d_items, it.items.data(), sizeof(int32_t) * it.items.size(), hipMemcpyHostToDevice, st));
    AMP_HIP(hipMemcpyAsync(it.d_item_first, it.item_first.data(), sizeof(int32_t) * ((size_t)B + 1), hipMemcpyHostToDevice, st));
    AMP_HIP(hipMemcpyAsync(it.d_off, offsets, sizeof(int32_t) * ((size_t)B + 1), hipMemcpyHostToDevice, st));
    it.item_blocks = (unsigned)(((int64_t)W + kItemWaves - 1) / kItemWaves);
    hipLaunchKernelGGL(rgb_box_item_kernel, dim3(it.item_blocks), dim3(64 * kItemWaves), 0, st, W, (const int32_t *)it.d_items, (int)dim,
                       points_dev, d_partial);
    hipLaunchKernelGGL(rgb_box_cloud_kernel, dim3(blocks(B)), dim3(256), 0, st, B, (const int32_t *)it.d_item_first,
                       (const Box *)d_partial, d_box);
    AMP_LAUNCH_CHECK();
    box.resize((size_t)B);
    AMP_HIP(hipMemcpyAsync(box.data(), d_box, sizeof(Box) * (size_t)B, hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    unsigned long long first_bad = ~0ull;
    int32_t bad_cloud = 0;
    for (int32_t b = 0; b < B; ++b)
        if (box[b].first_bad < first_bad) {
            first_bad = box[b].first_bad;
            bad_cloud = b;
        }
    if (first_bad != ~0ull) {
        float p[3] = {0.f, 0.f, 0.f};
        AMP_HIP(hipMemcpy(p, points_dev + first_bad * (unsigned long long)dim, sizeof(float) * dim, hipMemcpyDeviceToHost));
        int a = 0;
        while (a < dim - 1 && isfinite(p[a])) ++a;
        amp::set_error("%s: cloud %d: points(%d,%llu) = %g is not finite", who, bad_cloud + 1, a + 1, first_bad + 1, (double)p[a]);
        return 2;
    }
    return 0;
}

} // namespace
