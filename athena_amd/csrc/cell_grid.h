// The uniform cell grid of the point-cloud builders (radius_graph.hip, knn_graph.hip), for a batch of clouds; one cloud is a batch
// of one.  build_cell_grid is the whole set-up, once: the clouds cut into work items, a bounding box per cloud with the first
// non-finite point, a grid per cloud, cell keys in disjoint ranges per cloud, one stable sort of (cell, point), positions in cell
// order, cell starts.  What a cell is -- floor(fl(fl(p - lo) * inv_w)) clamped to the axis -- is defined here once; how wide the
// cells are is each builder's own choice, the callable it hands to build_cell_grid.  The kernels are in an unnamed namespace: one
// copy per file that includes this.
#pragma once
#include <math.h>

#include <algorithm>
#include <vector>

#include "cell_start.h"
#include "common.h"
#include "radix_sort.h"

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

// ---- bounding box + validity: a partial per work item, folded per cloud in item order (one cloud alone: per block) -----------
__device__ inline void box_fold(Box &a, const Box &b)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.lo[k] = fminf(a.lo[k], b.lo[k]);
        a.hi[k] = fmaxf(a.hi[k], b.hi[k]);
    }
    a.first_bad = b.first_bad < a.first_bad ? b.first_bad : a.first_bad;
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

// One cloud alone (B = 1) keeps block partials folded by one block: a cloud of millions of points is a few hundred work items,
// too few waves to hide the loads of the item kernel below and a long serial fold for the one thread of the cloud kernel -- the
// box pass of the 2 M-point build takes 102 us this way and 262 us through the items (profiles/radius_graph_build.txt).  The
// fold is order-free, so the box is the same.
constexpr int kBoxBlocks = 512;

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

// positions in cell order: a cell's points are one contiguous read
__global__ __launch_bounds__(256) void rg_gather_points_kernel(int32_t n, int dim, const float *__restrict__ pts,
                                                               const int32_t *__restrict__ perm, float *__restrict__ sorted)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int64_t i = perm[k];
    for (int a = 0; a < dim; ++a) sorted[k * dim + a] = pts[i * dim + a];
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
// cloud (an entry that takes one cloud has none to name: name_cloud = false), component and point of the first one; `what` is what
// the entry calls the array.  n > 0.  Synchronises the stream.
inline int batch_boxes(const char *who, bool name_cloud, int32_t B, const int32_t *offsets, int32_t dim, const float *points_dev,
                       hipStream_t st, amp::Scratch &tmp, BatchItems &it, std::vector<Box> &box, const char *what = "points")
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
    const int box_blocks = B == 1 ? (int)std::min<int64_t>(kBoxBlocks, blocks(offsets[1])) : 0;   // one cloud alone: see kBoxBlocks
    if (tmp.get(&it.d_items, it.items.size()) || tmp.get(&it.d_item_first, (size_t)B + 1) || tmp.get(&it.d_off, (size_t)B + 1) ||
        tmp.get(&d_partial, std::max(W, box_blocks)) || tmp.get(&d_box, B))
        return 1;
    AMP_HIP(hipMemcpyAsync(it.d_items, it.items.data(), sizeof(int32_t) * it.items.size(), hipMemcpyHostToDevice, st));
    AMP_HIP(hipMemcpyAsync(it.d_item_first, it.item_first.data(), sizeof(int32_t) * ((size_t)B + 1), hipMemcpyHostToDevice, st));
    AMP_HIP(hipMemcpyAsync(it.d_off, offsets, sizeof(int32_t) * ((size_t)B + 1), hipMemcpyHostToDevice, st));
    it.item_blocks = (unsigned)(((int64_t)W + kItemWaves - 1) / kItemWaves);
    if (B == 1) {
        hipLaunchKernelGGL(rg_box_kernel, dim3(box_blocks), dim3(256), 0, st, offsets[1], (int)dim, points_dev, d_partial);
        hipLaunchKernelGGL(rg_box_final_kernel, dim3(1), dim3(256), 0, st, box_blocks, (const Box *)d_partial, d_box);
    } else {
        hipLaunchKernelGGL(rgb_box_item_kernel, dim3(it.item_blocks), dim3(64 * kItemWaves), 0, st, W, (const int32_t *)it.d_items,
                           (int)dim, points_dev, d_partial);
        hipLaunchKernelGGL(rgb_box_cloud_kernel, dim3(blocks(B)), dim3(256), 0, st, B, (const int32_t *)it.d_item_first,
                           (const Box *)d_partial, d_box);
    }
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
        if (name_cloud)
            amp::set_error("%s: cloud %d: %s(%d,%llu) = %g is not finite", who, bad_cloud + 1, what, a + 1, first_bad + 1, (double)p[a]);
        else
            amp::set_error("%s: %s(%d,%llu) = %g is not finite", who, what, a + 1, first_bad + 1, (double)p[a]);
        return 2;
    }
    return 0;
}

// What a search reads of the grid, on the device.  A cloud's cells are the keys [cell_base[b], cell_base[b+1]): disjoint ranges.
// Slot s of the cell order holds point perm[s], its cell key key_s[s] and its position sorted[s, :]; cell c is the slots
// cell_start[c] .. cell_start[c + 1] - 1.
struct CellGrid {
    BatchItems it;
    Grid *d_grids = nullptr;            // [B]
    uint32_t *d_cell_base = nullptr;    // [B + 1]
    uint32_t *d_key_s = nullptr;        // [n]
    int32_t *d_perm = nullptr;          // [n]
    int32_t *d_cell_start = nullptr;    // [n_cells + 1]
    float *d_sorted = nullptr;          // [n, dim]
    uint32_t n_cells = 0;
};

// The whole set-up, n > 0: boxes (batch_boxes, which refuses non-finite points), grids[b] = make(box of cloud b, its points m > 0,
// b) per non-empty cloud, cell_base = the exclusive sum of the clouds' cell counts (an empty cloud adds 0), the keys, the sort, the
// gather, the cell starts.  Everything lives in tmp.  Synchronises the stream once, for the boxes.
template <typename Make>
int build_cell_grid(const char *who, bool name_cloud, int32_t B, int32_t n, const int32_t *offsets, int32_t dim, const float *points_dev,
                    hipStream_t st, amp::Scratch &tmp, Make make, CellGrid &cg, const char *what = "points")
{
    std::vector<Box> box;
    if (int rc = batch_boxes(who, name_cloud, B, offsets, dim, points_dev, st, tmp, cg.it, box, what)) return rc;
    std::vector<Grid> grids((size_t)B);
    std::vector<uint32_t> cell_base((size_t)B + 1);
    int64_t total_cells = 0;
    for (int32_t b = 0; b < B; ++b) {
        cell_base[b] = (uint32_t)total_cells;
        const int32_t m = offsets[b + 1] - offsets[b];
        grids[b] = Grid{};
        if (m == 0) continue;
        grids[b] = make(box[b], m, b);
        total_cells += (int64_t)grids[b].nc[0] * grids[b].nc[1] * grids[b].nc[2];
        AMP_REQUIRE(total_cells < (int64_t)INT32_MAX, "%s: more than 2^31 grid cells over %d points", who, n);
    }
    cell_base[B] = (uint32_t)total_cells;
    const uint32_t n_cells = cg.n_cells = (uint32_t)total_cells;

    uint32_t *d_key = nullptr, *d_key_t = nullptr;
    int32_t *d_perm_t = nullptr;
    void *d_temp = nullptr;
    if (tmp.get(&cg.d_grids, B) || tmp.get(&cg.d_cell_base, (size_t)B + 1) || tmp.get(&d_key, n) || tmp.get(&cg.d_key_s, n) ||
        tmp.get(&d_key_t, n) || tmp.get(&cg.d_perm, n) || tmp.get(&d_perm_t, n) || tmp.get(&cg.d_cell_start, (size_t)n_cells + 1) ||
        tmp.get(&cg.d_sorted, (size_t)n * dim) || tmp.get((char **)&d_temp, amp::radix::scratch_bytes(n)))
        return 1;
    AMP_HIP(hipMemcpyAsync(cg.d_grids, grids.data(), sizeof(Grid) * (size_t)B, hipMemcpyHostToDevice, st));
    AMP_HIP(hipMemcpyAsync(cg.d_cell_base, cell_base.data(), sizeof(uint32_t) * ((size_t)B + 1), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(rgb_cell_key_kernel, dim3(cg.it.item_blocks), dim3(64 * kItemWaves), 0, st, cg.it.W, (const int32_t *)cg.it.d_items,
                       (int)dim, points_dev, (const Grid *)cg.d_grids, (const uint32_t *)cg.d_cell_base, d_key);
    AMP_LAUNCH_CHECK();
    if (int rc = amp::radix::sort_pairs<uint32_t>((const uint32_t *)d_key, nullptr, n, bits_for(n_cells - 1), cg.d_key_s, cg.d_perm, d_key_t,
                                             d_perm_t, d_temp, st))
        return rc;
    hipLaunchKernelGGL(rg_gather_points_kernel, dim3(blocks(n)), dim3(256), 0, st, n, (int)dim, points_dev, (const int32_t *)cg.d_perm,
                       cg.d_sorted);
    hipLaunchKernelGGL(rg_cell_start_kernel, dim3(blocks((int64_t)n_cells + 1)), dim3(256), 0, st, n_cells, (const uint32_t *)cg.d_key_s, n,
                       cg.d_cell_start);
    AMP_LAUNCH_CHECK();
    return 0;
}

} // namespace
