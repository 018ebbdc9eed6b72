// Points -> voxel-grid clusters on the device, a batch of clouds per call: every cloud is cut into cubic cells of edge `size`,
// every non-empty cell is one coarse point (the centroid of its members) and the membership is the pooling graph -- grid
// subsampling / voxel pooling, the O(n) coarsening beside farthest-point sampling (fps.hip), whose m dependent steps run on one
// compute unit.  Nothing here depends on a previous step: every pass is one launch over all points or all clusters.
//
// The definition (include/athena_mp.h; every implementation gives the same arrays, tests compare with np.array_equal):
//   * inv = fl(1 / size); per non-empty cloud and axis k, lo_k = the smallest k-th coordinate + 0 (-0 becomes +0), or origin_k;
//     the cell of point j is c_k = floor(fl(fl(p_jk - lo_k) * inv)) -- cell_coord of cell_grid.h, whose clamp never acts because
//     nc_k = floor(fl(fl(hi_k - lo_k) * inv)) + 1 and rounding is monotone.
//   * a cluster is a non-empty cell of a cloud; clusters are numbered in ascending order of (cloud, c_{dim-1}, .., c_0), members
//     in ascending point index.
//   * centroid_k = fl(lo_k + fl(S_k / fl(count))), S_k the SEQUENTIAL fp32 sum of fl(p_jk - lo_k) over the members in index
//     order; weights = fl(1 / fl(count)); nearest = the member with the smallest (s(p_j, centroid) bits, index).
//
// How.  THE KEY is one unsigned long long, (cloud << cbits) | cell with cell = (c_2 * nc_1 + c_1) * nc_0 + c_0 and
// cbits = bits_for(the largest cell count of a cloud - 1): there is no array over the cells, so their number is bounded by the key
// width alone (a LIDAR sweep at 5 cm voxels has 1e10 cells).  gc_key_kernel: one wave per work item of cell_grid.h, so the cloud
// is known without a search.  THE SORT is radix::sort_pairs on exactly cbits + bits_for(n_clouds - 1) bits; it is stable, so the
// members of a cluster stay in index order, and the positions are gathered into key order: a cluster is one contiguous read.
// THE HEADS: flag[s] = key_s[s] != key_s[s - 1]; scan64::exclusive over the flags numbers the clusters and counts them; the count
// and the clusters in front of each cloud (the scan at the cloud's first slot: a cloud's slots are its own points' range) come
// home in one copy, the only synchronisation after the boxes.  gc_fill_kernel then writes cluster[perm[s]], both rows of pairs,
// and rowptr at the heads.
// THE CLUSTER REDUCE (gc_reduce_kernel) is the arithmetic: a group of G = 4 lanes per cluster over rowptr in the scheme of
// row_groups.h.  Each lane loads one member; the members pass through the group in order by __shfl; lane sub < dim owns component
// sub and adds fl(p - lo) to its sum in member order.  Round one gives S, count, centroid, cell and weights; round two, over the
// same members, keeps the smallest (s bits, index) key per lane and folds the four.  A hub cluster simply takes more rounds.  No
// LDS, no atomics, no scratch.  Hub clusters are NOT balanced over waves: the summation order is the definition, and a cluster
// of thousands of members is one group's loop while the other groups of its wave wait.
// THE REVERSE (gc_grad_kernel): one lane per (point, component), dpoints[j, k] = fl(dcentroid[c, k] / fl(count_c)).
#include <math.h>
#include <string.h>

#include <algorithm>

#include "call_scratch.h"
#include "cell_grid.h"
#include "common.h"
#include "knn_cells.h"
#include "row_groups.h"
#include "scan64.h"
#include "two_sets.h"

namespace amp {
int64_t g_grid_clusters_stats[4] = {0, 0, 0, 0};       // athena_mp_grid_clusters_stats: of the last call
}

namespace {

constexpr int kGcG = 4;                      // lanes per cluster
constexpr float kGcMaxCellsAxis = 2097152.f; // 2^21

// one wave per work item (cloud, p0, p1): key = (cloud << cbits) | the cell in the cloud's own grid, c_0 fastest
__global__ __launch_bounds__(64 * kItemWaves) void gc_key_kernel(int32_t n_items, const int32_t *__restrict__ items, int dim,
                                                                 const float *__restrict__ pts, const Grid *__restrict__ grids, int cbits,
                                                                 unsigned long long *__restrict__ key)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * kItemWaves + (threadIdx.x >> 6);
    if (w >= n_items) return;
    const int32_t b = items[3 * w], p0 = items[3 * w + 1], p1 = items[3 * w + 2];
    const Grid g = grids[b];
    const unsigned long long high = (unsigned long long)(uint32_t)b << cbits;
    for (int64_t i = (int64_t)p0 + lane; i < p1; i += 64) {
        unsigned long long c = 0;
        for (int k = dim - 1; k >= 0; --k)
            c = c * (unsigned long long)g.nc[k] + (unsigned long long)cell_coord(pts[i * dim + k], g.lo[k], g.inv_w[k], g.nc[k]);
        key[i] = high | c;
    }
}

__global__ __launch_bounds__(256) void gc_flag_kernel(int32_t n, const unsigned long long *__restrict__ key_s, uint32_t *__restrict__ flag)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    flag[s] = (s == 0 || key_s[s] != key_s[s - 1]) ? 1u : 0u;
}

// slot s of the key order holds point perm[s] of cluster before[s] + flag[s] (1-based); each output may be null
__global__ __launch_bounds__(256) void gc_fill_kernel(int32_t n, int32_t m, const uint32_t *__restrict__ flag,
                                                      const unsigned long long *__restrict__ before, const int32_t *__restrict__ perm,
                                                      int32_t *__restrict__ cluster, int32_t *__restrict__ pairs, int32_t *__restrict__ rowptr)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s > n) return;
    if (s == n) {
        rowptr[m] = n;
        return;
    }
    const uint32_t head = flag[s];
    const int32_t id = (int32_t)before[s] + (int32_t)head;        // 1-based
    const int32_t j = perm[s];
    if (cluster) cluster[j] = id;
    if (pairs) {
        pairs[2 * s] = id;
        pairs[2 * s + 1] = j + 1;
    }
    if (head) rowptr[id - 1] = (int32_t)s;
}

// G = 4 lanes per cluster (header).  sorted / perm / key_s are in key order: cluster r is the slots rowptr[r] .. rowptr[r + 1] - 1.
template <int DIM>
__global__ __launch_bounds__(256) void gc_reduce_kernel(int32_t m, const int32_t *__restrict__ rowptr, const float *__restrict__ sorted,
                                                        const int32_t *__restrict__ perm, const unsigned long long *__restrict__ key_s,
                                                        int cbits, const Grid *__restrict__ grids, float *__restrict__ weights,
                                                        float *__restrict__ centroid, int32_t *__restrict__ nearest,
                                                        int32_t *__restrict__ cell)
{
    const amp::RowGroup<kGcG> rg(m, rowptr);
    const int own = rg.sub < DIM ? rg.sub : DIM - 1;              // the component this lane sums; lanes beyond dim store nothing
    const bool live = rg.len > 0;
    float lo = 0.f, inv_w = 0.f;
    int32_t nc = 1;
    if (live) {
        const Grid *g = grids + (key_s[rg.beg] >> cbits);
        lo = g->lo[own], inv_w = g->inv_w[own], nc = g->nc[own];
    }
    // round one: S in member order
    float S = 0.f, first_p = 0.f;
    for (int32_t k0 = 0; k0 < rg.rounds; k0 += kGcG) {
        const bool in = k0 + rg.sub < rg.len;
        const int64_t slot = in ? (int64_t)rg.beg + k0 + rg.sub : 0;
        float p[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < DIM; ++a) p[a] = sorted[slot * DIM + a];
#pragma unroll
        for (int j = 0; j < kGcG; ++j) {
            float x = __shfl(p[0], rg.first + j, 64);
            if (DIM > 1) {
                const float x1 = __shfl(p[1], rg.first + j, 64);
                x = own == 1 ? x1 : x;
            }
            if (DIM > 2) {
                const float x2 = __shfl(p[2], rg.first + j, 64);
                x = own == 2 ? x2 : x;
            }
            if (k0 + j < rg.len) S = S + (x - lo);
            if (k0 + j == 0) first_p = x;
        }
    }
    const float count = (float)rg.len;
    const float mine = lo + S / count;                            // of component `own`; unused where the row is empty
    const float w = 1.0f / count;
    if (live && rg.sub < DIM) {
        if (centroid) centroid[rg.row * DIM + rg.sub] = mine;
        if (cell) cell[rg.row * DIM + rg.sub] = cell_coord(first_p, lo, inv_w, nc);
    }
    if (!weights && !nearest) return;
    // round two: the smallest (s bits, index) over the same members; the weights go out with the lane that holds the member
    float c[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < DIM; ++a) c[a] = __shfl(mine, rg.first + a, 64);
    unsigned long long best = ~0ull;
    for (int32_t k0 = 0; k0 < rg.rounds; k0 += kGcG) {
        const bool in = k0 + rg.sub < rg.len;
        const int64_t slot = in ? (int64_t)rg.beg + k0 + rg.sub : 0;
        float p[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < DIM; ++a) p[a] = sorted[slot * DIM + a];
        const int32_t j = perm[slot];
        const unsigned long long key = ((unsigned long long)__float_as_uint(sq_dist<DIM>(p, c)) << 32) | (unsigned long long)(uint32_t)j;
        if (in) {
            best = key_min(best, key);
            if (weights) weights[slot] = w;
        }
    }
#pragma unroll
    for (int d = 1; d < kGcG; d <<= 1) best = key_min(best, __shfl_xor(best, d, 64));
    if (live && rg.sub == 0 && nearest) nearest[rg.row] = (int32_t)(uint32_t)best + 1;
}

template <typename... A> void launch_gc_reduce(int dim, int32_t m, hipStream_t st, A... a)
{
    const dim3 grid = amp::group_grid(m, kGcG), block(256);
    if (dim == 1) hipLaunchKernelGGL(gc_reduce_kernel<1>, grid, block, 0, st, m, a...);
    else if (dim == 2) hipLaunchKernelGGL(gc_reduce_kernel<2>, grid, block, 0, st, m, a...);
    else hipLaunchKernelGGL(gc_reduce_kernel<3>, grid, block, 0, st, m, a...);
}

// one lane per (point, component); a cluster id outside 1..m is not followed: the smallest such point lands in *bad
__global__ __launch_bounds__(256) void gc_grad_kernel(int64_t total, int dim, int32_t m, const int32_t *__restrict__ cluster,
                                                      const int32_t *__restrict__ rowptr, const float *__restrict__ dcentroid,
                                                      float *__restrict__ dpoints, unsigned long long *__restrict__ bad)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int64_t j = t / dim;
    const int k = (int)(t - j * dim);
    const int32_t c = cluster[j] - 1;
    if (c < 0 || c >= m) {
        atomicMin(bad, (unsigned long long)j);
        return;
    }
    const float count = (float)(rowptr[c + 1] - rowptr[c]);
    dpoints[t] = dcentroid[(int64_t)c * dim + k] / count;
}

// what every entry checks before anything touches the device: 0, or 2 with the message set; *inv = fl(1 / size)
int gc_arguments_check(const char *who, int32_t B, int32_t n, const int32_t *offsets, int32_t dim, float size, const float *origin, float *inv)
{
    AMP_REQUIRE(dim >= 1 && dim <= 3, "%s: dim = %d outside [1,3]", who, dim);
    AMP_REQUIRE(isfinite(size) && size > 0.f, "%s: size = %g is not finite and positive", who, (double)size);
    *inv = 1.0f / size;
    AMP_REQUIRE(isfinite(*inv), "%s: 1 / size = %g is not finite (size = %g)", who, (double)*inv, (double)size);
    AMP_REQUIRE(B >= 0, "%s: n_clouds = %d is negative", who, B);
    AMP_REQUIRE(n >= 0, "%s: n = %d is negative", who, n);
    if (int rc = named_offsets_check(who, "offsets", "points", B, offsets, n)) return rc;
    if (origin)
        for (int k = 0; k < dim; ++k) AMP_REQUIRE(isfinite(origin[k]), "%s: origin(%d) = %g is not finite", who, k + 1, (double)origin[k]);
    return 0;
}

} // namespace

namespace amp {

// Every output may be null alone.  Everything on the library's stream; synchronised on return.
int grid_clusters_core(const char *who, int32_t B, int32_t n, const int32_t *offsets, int32_t dim, const float *points_dev, float size,
                       const float *origin, int64_t capacity, int32_t *cluster_dev, int32_t *pairs_dev, int32_t *rowptr_dev,
                       float *weights_dev, float *centroid_dev, int32_t *nearest_dev, int32_t *cell_dev, int32_t *cluster_offsets_out,
                       float *origin_out, int64_t *n_clusters_out)
{
    std::fill(g_grid_clusters_stats, g_grid_clusters_stats + 4, (int64_t)0);
    AMP_REQUIRE(n_clusters_out != nullptr, "%s: null n_clusters_out", who);
    *n_clusters_out = 0;
    float inv = 0.f;
    if (int rc = gc_arguments_check(who, B, n, offsets, dim, size, origin, &inv)) return rc;
    AMP_REQUIRE(n == 0 || points_dev != nullptr, "%s: null points", who);
    if (cluster_offsets_out) std::fill(cluster_offsets_out, cluster_offsets_out + B + 1, 0);
    if (origin_out) std::fill(origin_out, origin_out + (size_t)B * dim, 0.f);
    const bool any_out = cluster_dev || pairs_dev || rowptr_dev || weights_dev || centroid_dev || nearest_dev || cell_dev;
    hipStream_t st = stream();
    if (n == 0 || B == 0) {
        AMP_REQUIRE(!any_out || capacity >= 0, "%s: the buffers hold %lld clusters, the batch has %lld", who, (long long)capacity, 0ll);
        if (rowptr_dev) {
            AMP_HIP(hipMemsetAsync(rowptr_dev, 0, sizeof(int32_t), st));
            AMP_HIP(hipStreamSynchronize(st));
        }
        return 0;
    }

    Scratch tmp;
    BatchItems it;
    std::vector<Box> box;
    if (int rc = batch_boxes(who, true, B, offsets, dim, points_dev, st, tmp, it, box)) return rc;

    // the grids: lo, the cell counts, the key layout
    std::vector<Grid> grids((size_t)B);
    unsigned long long cells_max = 1;
    for (int32_t b = 0; b < B; ++b) {
        Grid &g = grids[b];
        for (int k = 0; k < 3; ++k) g.lo[k] = 0.f, g.inv_w[k] = 0.f, g.nc[k] = 1;
        if (offsets[b + 1] == offsets[b]) continue;
        unsigned long long cells = 1;
        for (int k = 0; k < dim; ++k) {
            const float lo = origin ? origin[k] : box[b].lo[k] + 0.f, hi = box[b].hi[k];
            if (origin && origin[k] > box[b].lo[k]) {                 // name the first point of the cloud below the origin on this axis
                const int32_t nb = offsets[b + 1] - offsets[b];
                std::vector<float> p((size_t)nb * dim);
                AMP_HIP(hipMemcpy(p.data(), points_dev + (size_t)offsets[b] * dim, sizeof(float) * p.size(), hipMemcpyDeviceToHost));
                int32_t j = 0;
                while (j < nb - 1 && !(p[(size_t)j * dim + k] < origin[k])) ++j;
                set_error("%s: cloud %d: origin(%d) = %g is above points(%d,%d) = %g", who, b + 1, k + 1, (double)origin[k], k + 1,
                          offsets[b] + j + 1, (double)p[(size_t)j * dim + k]);
                return 2;
            }
            const float ext = hi - lo;
            AMP_REQUIRE(isfinite(ext), "%s: cloud %d: axis %d: the extent %g - %g is not finite", who, b + 1, k + 1, (double)hi, (double)lo);
            const float q = ext * inv;
            AMP_REQUIRE(q < kGcMaxCellsAxis, "%s: cloud %d: axis %d: %g cells of size %g, more than 2^21", who, b + 1, k + 1, floor((double)q) + 1.0,
                        (double)size);
            g.lo[k] = lo, g.inv_w[k] = inv, g.nc[k] = (int32_t)q + 1;
            cells *= (unsigned long long)g.nc[k];
            if (origin_out) origin_out[(size_t)b * dim + k] = lo;
        }
        cells_max = std::max(cells_max, cells);
    }
    const int cbits = bits_for(cells_max - 1), bbits = bits_for((unsigned long long)(B - 1));
    AMP_REQUIRE(cbits + bbits <= 62, "%s: the keys need %d + %d bits for %d clouds and %llu cells, more than 62", who, bbits, cbits, B, cells_max);
    const int bits = cbits + bbits;

    // one allocation cut into pieces (pieces.h): a hipMalloc and a hipFree per array would be most of a call's time
    const size_t N = (size_t)n;
    Grid *d_grids = nullptr;
    unsigned long long *d_key = nullptr, *d_key_s = nullptr, *d_key_t = nullptr, *d_before = nullptr, *d_tile = nullptr;
    long long *d_coff = nullptr;
    int32_t *d_perm = nullptr, *d_perm_t = nullptr, *d_rowptr = nullptr, *d_longest = nullptr;
    uint32_t *d_flag = nullptr;
    float *d_sorted = nullptr;
    char *d_temp = nullptr;
    Pieces pc;
    pc.add(&d_grids, (size_t)B), pc.add(&d_key, N), pc.add(&d_key_s, N), pc.add(&d_key_t, N), pc.add(&d_before, N);
    pc.add(&d_tile, (size_t)scan64::tiles(n) + 1), pc.add(&d_coff, (size_t)B + 1), pc.add(&d_perm, N), pc.add(&d_perm_t, N), pc.add(&d_flag, N);
    pc.add(&d_sorted, N * dim), pc.add(&d_rowptr, N + 1), pc.add(&d_longest, (size_t)kLongestBlocks), pc.add(&d_temp, radix::scratch_bytes(n));
    if (tmp.carve(pc)) return 1;
    AMP_HIP(hipMemcpyAsync(d_grids, grids.data(), sizeof(Grid) * (size_t)B, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(gc_key_kernel, dim3(it.item_blocks), dim3(64 * kItemWaves), 0, st, it.W, (const int32_t *)it.d_items, (int)dim, points_dev,
                       (const Grid *)d_grids, cbits, d_key);
    AMP_LAUNCH_CHECK();
    if (int rc = radix::sort_pairs<unsigned long long>((const unsigned long long *)d_key, nullptr, n, bits, d_key_s, d_perm, d_key_t, d_perm_t,
                                                       d_temp, st))
        return rc;
    hipLaunchKernelGGL(gc_flag_kernel, dim3(blocks(n)), dim3(256), 0, st, n, (const unsigned long long *)d_key_s, d_flag);
    const unsigned long long *d_total = scan64::exclusive<uint32_t>(n, (const uint32_t *)d_flag, d_tile, d_before, st);
    // a cloud's slots are its own points' range: the clusters in front of cloud b = the heads in front of slot offsets[b]
    hipLaunchKernelGGL(bip_rowptr_kernel, dim3(blocks((int64_t)B + 1)), dim3(256), 0, st, n, B, (const int32_t *)it.d_off,
                       (const unsigned long long *)d_before, d_total, (int32_t *)nullptr, d_coff);
    AMP_LAUNCH_CHECK();
    std::vector<long long> coff((size_t)B + 1);
    AMP_HIP(hipMemcpyAsync(coff.data(), d_coff, sizeof(long long) * ((size_t)B + 1), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    const int64_t m64 = coff[B];
    *n_clusters_out = m64;
    if (cluster_offsets_out)
        for (int32_t b = 0; b <= B; ++b) cluster_offsets_out[b] = (int32_t)coff[b];
    g_grid_clusters_stats[0] = m64;
    g_grid_clusters_stats[1] = bits;
    g_grid_clusters_stats[2] = bits <= 8 ? 1 : (bits + 7) / 8;
    if (!any_out) return 0;                                           // size query
    AMP_REQUIRE(capacity >= m64, "%s: the buffers hold %lld clusters, the batch has %lld", who, (long long)capacity, (long long)m64);
    const int32_t m = (int32_t)m64;

    if (rowptr_dev) d_rowptr = rowptr_dev;
    hipLaunchKernelGGL(gc_fill_kernel, dim3(blocks((int64_t)n + 1)), dim3(256), 0, st, n, m, (const uint32_t *)d_flag,
                       (const unsigned long long *)d_before, (const int32_t *)d_perm, cluster_dev, pairs_dev, d_rowptr);
    if (weights_dev || centroid_dev || nearest_dev || cell_dev) {
        hipLaunchKernelGGL(rg_gather_points_kernel, dim3(blocks(n)), dim3(256), 0, st, n, (int)dim, points_dev, (const int32_t *)d_perm, d_sorted);
        launch_gc_reduce(dim, m, st, (const int32_t *)d_rowptr, (const float *)d_sorted, (const int32_t *)d_perm,
                         (const unsigned long long *)d_key_s, cbits, (const Grid *)d_grids, weights_dev, centroid_dev, nearest_dev, cell_dev);
    }
    int32_t longest = 0;
    if (int rc = longest_row(m, (const int32_t *)d_rowptr, d_longest, &longest, st)) return rc;   // the wait; scratch dies with this scope
    g_grid_clusters_stats[3] = longest;
    return 0;
}

int grid_clusters_grad_core(const char *who, int32_t n, int32_t dim, int32_t m, const int32_t *cluster_dev, const int32_t *rowptr_dev,
                            const float *dcentroid_dev, float *dpoints_dev)
{
    AMP_REQUIRE(dim >= 1 && dim <= 3, "%s: dim = %d outside [1,3]", who, dim);
    AMP_REQUIRE(n >= 0 && m >= 0, "%s: n = %d, n_clusters = %d: negative", who, n, m);
    if (n == 0) return 0;
    AMP_REQUIRE(cluster_dev && rowptr_dev && dcentroid_dev && dpoints_dev, "%s: null array", who);
    hipStream_t st = stream();
    Scratch tmp;
    BadWord bad;
    if (int rc = bad.arm(tmp, st)) return rc;
    const int64_t total = (int64_t)n * dim;
    hipLaunchKernelGGL(gc_grad_kernel, dim3(blocks(total)), dim3(256), 0, st, total, (int)dim, m, cluster_dev, rowptr_dev, dcentroid_dev,
                       dpoints_dev, bad.dev);
    AMP_LAUNCH_CHECK();
    return bad.read(who, "cluster", cluster_dev, 1, m, st);
}

} // namespace amp

extern "C" int athena_mp_grid_clusters(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim, const float *points_dev,
                                       float size, const float *origin_host, int64_t capacity, int32_t *cluster_dev, int32_t *pairs_dev,
                                       int32_t *rowptr_dev, float *weights_dev, float *centroid_dev, int32_t *nearest_dev, int32_t *cell_dev,
                                       int32_t *cluster_offsets_host, float *origin_out_host, int64_t *n_clusters_out)
{
    return amp::grid_clusters_core("grid_clusters", n_clouds, n, offsets_host, dim, points_dev, size, origin_host, capacity, cluster_dev,
                                   pairs_dev, rowptr_dev, weights_dev, centroid_dev, nearest_dev, cell_dev, cluster_offsets_host,
                                   origin_out_host, n_clusters_out);
}

extern "C" int athena_mp_grid_clusters_grad(int32_t n, int32_t dim, int32_t n_clusters, const int32_t *cluster_dev, const int32_t *rowptr_dev,
                                            const float *dcentroid_dev, float *dpoints_dev)
{
    return amp::grid_clusters_grad_core("grid_clusters_grad", n, dim, n_clusters, cluster_dev, rowptr_dev, dcentroid_dev, dpoints_dev);
}

// Fortran arrays in, Fortran arrays out: one pass into buffers of n clusters (m <= n), narrowed on the way home
extern "C" int athena_mp_grid_clusters_host(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim, const float *points_host,
                                            float size, const float *origin_host, int64_t capacity, int32_t *cluster_out,
                                            int32_t *adj_ia_out, int32_t *adj_ja_out, float *weights_out, float *centroid_out,
                                            int32_t *nearest_out, int32_t *cell_out, int32_t *cluster_offsets_out, float *origin_out,
                                            int64_t *n_clusters_out)
{
    const char *who = "grid_clusters_host";
    AMP_REQUIRE(n_clusters_out != nullptr, "%s: null n_clusters_out", who);
    *n_clusters_out = 0;
    float inv = 0.f;
    // before the points are uploaded: dim and the counts size the copies
    if (int rc = gc_arguments_check(who, n_clouds, n, offsets_host, dim, size, origin_host, &inv)) return rc;
    AMP_REQUIRE(n == 0 || points_host != nullptr, "%s: null points", who);
    hipStream_t st = amp::stream();
    amp::Scratch tmp;
    const size_t N = (size_t)n;
    float *d_p = nullptr, *d_w = nullptr, *d_c = nullptr;
    int32_t *d_cluster = nullptr, *d_pairs = nullptr, *d_rowptr = nullptr, *d_near = nullptr, *d_cell = nullptr;
    if (tmp.upload(&d_p, points_host, N * dim, st)) return 1;
    const bool fill = adj_ja_out != nullptr;
    if (fill) {
        AMP_REQUIRE(adj_ia_out != nullptr, "%s: null output array", who);
        if (tmp.get(&d_pairs, 2 * N) || tmp.get(&d_rowptr, N + 1) || (cluster_out && tmp.get(&d_cluster, N)) ||
            (weights_out && tmp.get(&d_w, N)) || (centroid_out && tmp.get(&d_c, N * dim)) || (nearest_out && tmp.get(&d_near, N)) ||
            (cell_out && tmp.get(&d_cell, N * dim)))
            return 1;
    }
    int64_t m = 0;
    if (int rc = amp::grid_clusters_core(who, n_clouds, n, offsets_host, dim, d_p, size, origin_host, n, d_cluster, d_pairs, d_rowptr, d_w, d_c,
                                         d_near, d_cell, cluster_offsets_out, origin_out, &m))
        return rc;
    *n_clusters_out = m;
    if (!fill) return 0;                                              // size query
    AMP_REQUIRE(capacity >= m, "%s: the buffers hold %lld clusters, the batch has %lld", who, (long long)capacity, (long long)m);
    const size_t M = (size_t)m;
    std::vector<int32_t> pairs(2 * N);
    if (tmp.download(adj_ia_out, d_rowptr, M + 1, st) || tmp.download(pairs.data(), d_pairs, 2 * N, st) ||
        tmp.download(cluster_out, d_cluster, N, st) || tmp.download(weights_out, d_w, N, st) || tmp.download(centroid_out, d_c, M * dim, st) ||
        tmp.download(nearest_out, d_near, M, st) || tmp.download(cell_out, d_cell, M * dim, st))
        return 1;
    AMP_HIP(hipStreamSynchronize(st));
    for (size_t r = 0; r <= M; ++r) adj_ia_out[r] += 1;              // 1-based
    for (size_t e = 0; e < N; ++e) {                                  // (column, edge id): pair e is entry e
        adj_ja_out[2 * e] = pairs[2 * e + 1];
        adj_ja_out[2 * e + 1] = (int32_t)e + 1;
    }
    return 0;
}

extern "C" int athena_mp_grid_clusters_grad_host(int32_t n, int32_t dim, int32_t n_clusters, const int32_t *cluster, const int32_t *rowptr,
                                                 const float *dcentroid, float *dpoints)
{
    const char *who = "grid_clusters_grad_host";
    AMP_REQUIRE(dim >= 1 && dim <= 3, "%s: dim = %d outside [1,3]", who, dim);
    AMP_REQUIRE(n >= 0 && n_clusters >= 0, "%s: n = %d, n_clusters = %d: negative", who, n, n_clusters);
    if (n == 0) return 0;
    AMP_REQUIRE(cluster && rowptr && dcentroid && dpoints, "%s: null array", who);
    hipStream_t st = amp::stream();
    amp::Scratch tmp;
    const size_t N = (size_t)n, M = (size_t)n_clusters;
    int32_t *d_cluster = nullptr, *d_rowptr = nullptr;
    float *d_dc = nullptr, *d_dp = nullptr;
    if (tmp.upload(&d_cluster, cluster, N, st) || tmp.upload(&d_rowptr, rowptr, M + 1, st) || tmp.upload(&d_dc, dcentroid, M * dim, st) ||
        tmp.get(&d_dp, N * dim))
        return 1;
    if (int rc = amp::grid_clusters_grad_core(who, n, dim, n_clusters, d_cluster, d_rowptr, d_dc, d_dp)) return rc;
    if (tmp.download(dpoints, d_dp, N * dim, st)) return 1;
    AMP_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" int athena_mp_grid_clusters_stats(int64_t out[4])
{
    AMP_REQUIRE(out != nullptr, "grid_clusters_stats: null output");
    std::copy(amp::g_grid_clusters_stats, amp::g_grid_clusters_stats + 4, out);
    return 0;
}
