// Points -> radius graph on the device, one cloud or a batch of clouds as one block-diagonal pair list: the step in front of
// athena_mp_csr_from_edges / athena_mp_graph_create_from_edges for graph_nop_layer_type's inputs (a radius graph of a point cloud
// and its edge geometry, athena_graph_nop_layer.f90:743-758).  graphstruc has no such call.
//
// The definition (every implementation gives the same arrays; tests compare with np.array_equal):
//   * delta = p_i - p_j component by component in fp32, s = ((d0*d0) + d1*d1) + d2*d2 with every multiply and add rounded to
//     fp32 on its own (the library is built with -ffp-contract=off); i < j of ONE cloud are joined iff s <= fl(radius * radius).
//     No self pairs; two points at the same place are joined.
//   * pairs are numbered in lexicographic order of the global (i, j), i < j; coords[e, :] = p_i - p_j (smaller index minus
//     larger); edge_offsets[b] = pairs whose i is below offsets[b] (include/athena_mp.h).
// So a batch gives the pair lists of its slices points[offsets[b] : offsets[b+1]], in cloud order, offsets[b] added to both indices.
//
// How, in ONE pipeline (radius_pairs_batched_core; the single-cloud entries run it with offsets = {0, n}).  The grid set-up is
// build_cell_grid of cell_grid.h, shared with knn_graph.hip: the host cuts the clouds into work items (cloud, points p0 .. p1-1)
// of at most kItemPoints points, one 64-lane wave each; a bounding box per item (min and max are order-free; a wave folds with
// __shfl_xor and writes its own slot), folded per cloud in item order; the boxes come home and make_grid runs per cloud -- cells
// at least radius * (1 + 2^-10) wide on every axis, at most kMaxCellsAxis cells per axis, at most 2 m_b per cloud and so at most
// 2 n in all; a cloud's cells are the keys [cell_base[b], cell_base[b+1]): disjoint ranges, so after the key pass no kernel sees
// a candidate pair of two clouds; a stable radix sort of (cell, point id) (radix_sort.h), the positions copied into cell order,
// the cell starts.  Then a COUNT pass in which every point counts its partners with a larger id in the 3^dim cells around it -- a
// thread looks up its cloud (the last b with offsets[b] <= i: empty clouds repeat a value and own no point) and loads that
// cloud's grid; an exclusive scan of the counts IN POINT-ID ORDER (64-bit offsets, scan64.h), so the rows of the pair list already
// sit in lexicographic order of i; a FILL pass that writes keys into those rows; one radix sort of the keys, which puts the
// partners of every row in ascending order; one pass that decodes the keys into the 1-based pair list and the coordinate
// differences.  Both ends of a pair are in one cloud, so the key is i * M + (j - offsets[b]) with M the largest cloud: the order
// is that of (i, j), in fewer bits than i * n + j (one cloud: M = n, the key is i * n + j).  No atomics on data: counts, offsets
// and the final order are functions of the input alone; every access to points and coords is 4 bytes wide.
//
// Why the margin: the cell of a coordinate is floor(fl(fl(p - lo) * inv_w)) clamped to the axis -- monotone in p, each of the two
// roundings within 2^-24 relative, so a computed cell coordinate q is within 3 * 2^-24 * q <= 3 * 2^-24 * kMaxCellsAxis of the
// exact one.  A pair the predicate keeps has |p_i - p_j| <= radius * (1 + 2^-22) on every axis, i.e. at most
// (1 + 2^-22) / (1 + 2^-10) < 1 - 2^-10 + 2^-19 cells apart exactly, and 6 * 2^-24 * 2048 + 2^-19 < 2^-10: the computed
// coordinates differ by less than one, the cells by at most one.
#include <math.h>

#include <algorithm>

#include "cell_grid.h"
#include "common.h"
#include "radius_cells.h"
#include "radix_sort.h"
#include "scan64.h"

namespace {

// One thread per slot of the cell order: the point i = perm[slot] against every point j > i of the 3^DIM cells around its own,
// with the grid of the slot's cloud and the walk inside that cloud's cells.  FILL = false: count[i] = number of partners.
// FILL = true: key[offset[i] + t] = i * M + (j - offsets[cloud]) for the t-th partner found.
template <int DIM, bool FILL>
__global__ __launch_bounds__(256) void rgb_neighbour_kernel(int32_t n, int32_t B, const int32_t *__restrict__ offsets,
                                                            const Grid *__restrict__ grids, const uint32_t *__restrict__ cell_base,
                                                            unsigned long long M, float r2, const float *__restrict__ sorted,
                                                            const int32_t *__restrict__ perm, const uint32_t *__restrict__ sorted_key,
                                                            const int32_t *__restrict__ cell_start, uint32_t *__restrict__ count,
                                                            const unsigned long long *__restrict__ offset,
                                                            unsigned long long *__restrict__ key)
{
    const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (slot >= n) return;
    const int32_t i = perm[slot];
    const int32_t b = cloud_of(B, offsets, i);
    const Grid g = grids[b];
    const uint32_t cb = cell_base[b];
    const int32_t first_point = offsets[b];
    float p[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < DIM; ++a) p[a] = sorted[slot * DIM + a];
    uint32_t c = sorted_key[slot] - cb;
    int32_t cc[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        cc[a] = (int32_t)(c % (uint32_t)g.nc[a]);
        c /= (uint32_t)g.nc[a];
    }
    uint32_t found = 0;
    unsigned long long at = 0;
    if (FILL) at = offset[i];
    const int z0 = DIM > 2 ? max(cc[2] - 1, 0) : 0, z1 = DIM > 2 ? min(cc[2] + 1, g.nc[2] - 1) : 0;
    const int y0 = DIM > 1 ? max(cc[1] - 1, 0) : 0, y1 = DIM > 1 ? min(cc[1] + 1, g.nc[1] - 1) : 0;
    const int x0 = max(cc[0] - 1, 0), x1 = min(cc[0] + 1, g.nc[0] - 1);
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
            // the cells x0 .. x1 of one grid row are consecutive keys: one contiguous run of slots, all of this cloud
            const uint32_t row = (DIM > 2 ? (uint32_t)z * (uint32_t)g.nc[1] : 0u) + (uint32_t)y;
            const uint32_t first = cb + row * (uint32_t)g.nc[0] + (uint32_t)x0;
            const int32_t beg = cell_start[first], end = cell_start[first + (uint32_t)(x1 - x0) + 1u];
            for (int32_t m = beg; m < end; ++m) {
                const int32_t j = perm[m];
                if (j <= i) continue;
                if (!joined<DIM>(p, sorted + (int64_t)m * DIM, r2)) continue;       // p_i - p_j, i < j
                if (FILL) key[at + found] = (unsigned long long)i * M + (unsigned long long)(j - first_point);
                ++found;
            }
        }
    if (!FILL) count[i] = found;
}

// edge_offsets[b] = pairs whose i is below offsets[b]: the scan at the cloud starts (b = 0 .. B)
__global__ __launch_bounds__(256) void rgb_edge_offsets_kernel(int32_t B, int32_t n, const int32_t *__restrict__ offsets,
                                                               const unsigned long long *__restrict__ offset,
                                                               const unsigned long long *__restrict__ total,
                                                               long long *__restrict__ edge_offsets)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b > B) return;
    const int32_t v = offsets[b];
    edge_offsets[b] = (long long)(v < n ? offset[v] : *total);
}

// ---- sorted keys -> 1-based pair list [2, E] column-major and coords [E, dim] -------------------------------------------------
__global__ __launch_bounds__(256) void rgb_emit_kernel(int64_t E, int32_t B, const int32_t *__restrict__ offsets, unsigned long long M,
                                                       int dim, const unsigned long long *__restrict__ key,
                                                       const float *__restrict__ pts, int32_t *__restrict__ pairs,
                                                       float *__restrict__ coords)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const unsigned long long k = key[e];
    const int64_t i = (int64_t)(k / M);
    const int64_t j = (int64_t)offsets[cloud_of(B, offsets, (int32_t)i)] + (int64_t)(k % M);
    if (pairs) {
        pairs[2 * e] = (int32_t)i + 1;
        pairs[2 * e + 1] = (int32_t)j + 1;
    }
    if (coords)
        for (int a = 0; a < dim; ++a) coords[e * dim + a] = pts[i * dim + a] - pts[j * dim + a];
}

using amp::Scratch;

template <bool FILL, typename... A> void launch_neighbour(int dim, int32_t n, hipStream_t st, A... a)
{
    if (dim == 1) hipLaunchKernelGGL((rgb_neighbour_kernel<1, FILL>), dim3(blocks(n)), dim3(256), 0, st, n, a...);
    else if (dim == 2) hipLaunchKernelGGL((rgb_neighbour_kernel<2, FILL>), dim3(blocks(n)), dim3(256), 0, st, n, a...);
    else hipLaunchKernelGGL((rgb_neighbour_kernel<3, FILL>), dim3(blocks(n)), dim3(256), 0, st, n, a...);
}

// how an entry speaks of itself in its messages: its name, what it calls its result, and whether it has clouds to name
struct Caller {
    const char *who, *noun;
    bool names_clouds;
};
constexpr Caller kSingle = {"radius_pairs", "graph", false}, kBatched = {"radius_pairs_batched", "batch", true};

// the checks both batched entries make before anything touches the device: 0, or 2 with the message set
int batch_arguments_check(const char *who, int32_t B, const int32_t *offsets, int32_t dim, float radius)
{
    AMP_REQUIRE(dim >= 1 && dim <= 3, "%s: dim = %d outside [1,3]", who, dim);
    AMP_REQUIRE(isfinite(radius) && radius > 0.f, "%s: radius = %g is not a positive finite number", who, (double)radius);
    AMP_REQUIRE(isfinite(radius * radius), "%s: radius = %g squared is not finite in fp32", who, (double)radius);
    return batch_offsets_check(who, B, offsets);
}

} // namespace

namespace amp {

// pairs_dev / coords_dev both null: count only (edge_offsets_out is filled either way).  Everything on the library's stream;
// synchronised on return.
int radius_pairs_batched_core(const Caller &c, int32_t B, int32_t n, const int32_t *offsets, int32_t dim, const float *points_dev,
                              float radius, int32_t *pairs_dev, float *coords_dev, int64_t capacity, int64_t *edge_offsets_out,
                              int64_t *n_pairs_out)
{
    const char *who = c.who;
    AMP_REQUIRE(n_pairs_out != nullptr, "%s: null n_pairs_out", who);
    *n_pairs_out = 0;
    if (int rc = batch_arguments_check(who, B, offsets, dim, radius)) return rc;
    AMP_REQUIRE(offsets[B] == n, "%s: offsets end at %d, the batch has %d points", who, offsets[B], n);
    AMP_REQUIRE(n == 0 || points_dev != nullptr, "%s: null points", who);
    if (edge_offsets_out) std::fill(edge_offsets_out, edge_offsets_out + B + 1, (int64_t)0);
    if (n == 0) return 0;
    const float r2 = radius * radius;
    hipStream_t st = stream();
    const bool fill = pairs_dev != nullptr || coords_dev != nullptr;

    Scratch tmp;
    CellGrid cg;
    if (int rc = build_cell_grid(who, c.names_clouds, B, n, offsets, dim, points_dev, st, tmp,
                                 [&](const Box &box, int32_t m, int32_t) { return make_grid(box, dim, m, radius); }, cg))
        return rc;
    const int32_t *d_off = cg.it.d_off;

    uint32_t *d_count = nullptr;
    unsigned long long *d_tile = nullptr, *d_offset = nullptr;
    long long *d_edge_off = nullptr;
    Pieces pc;
    pc.add(&d_count, (size_t)n), pc.add(&d_tile, (size_t)scan64::tiles(n) + 1), pc.add(&d_offset, (size_t)n), pc.add(&d_edge_off, (size_t)B + 1);
    if (tmp.carve(pc)) return 1;
    const unsigned long long M = (unsigned long long)cg.it.m_max;
    launch_neighbour<false>(dim, n, st, B, d_off, (const Grid *)cg.d_grids, (const uint32_t *)cg.d_cell_base, M, r2,
                            (const float *)cg.d_sorted, (const int32_t *)cg.d_perm, (const uint32_t *)cg.d_key_s,
                            (const int32_t *)cg.d_cell_start, d_count, (const unsigned long long *)nullptr, (unsigned long long *)nullptr);
    const unsigned long long *d_total = scan64::exclusive(n, (const uint32_t *)d_count, d_tile, d_offset, st);
    hipLaunchKernelGGL(rgb_edge_offsets_kernel, dim3(blocks((int64_t)B + 1)), dim3(256), 0, st, B, n, d_off,
                       (const unsigned long long *)d_offset, d_total, d_edge_off);
    AMP_LAUNCH_CHECK();
    unsigned long long total = 0;
    AMP_HIP(hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, st));
    if (edge_offsets_out)
        AMP_HIP(hipMemcpyAsync(edge_offsets_out, d_edge_off, sizeof(int64_t) * ((size_t)B + 1), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    // the limit of csr_from_edges_core, found by the count pass before anything of that size is allocated
    AMP_REQUIRE(total < (1ull << 31) && 2 * (int64_t)total + n < (int64_t)INT32_MAX,
                "%s: %llu pairs among %d points: more than 2^31 CSR entries", who, total, n);
    *n_pairs_out = (int64_t)total;
    if (!fill) return 0;
    AMP_REQUIRE(capacity >= (int64_t)total, "%s: the output buffers hold %lld pairs, the %s has %lld", who, (long long)capacity, c.noun,
                (long long)total);
    if (total == 0) return 0;

    const int64_t E = (int64_t)total;
    unsigned long long *d_pk = nullptr, *d_pk_s = nullptr, *d_pk_t = nullptr;
    int32_t *d_v = nullptr, *d_v_t = nullptr;
    char *d_temp2 = nullptr;
    const size_t EE = (size_t)E;
    Pieces pk;
    pk.add(&d_pk, EE), pk.add(&d_pk_s, EE), pk.add(&d_pk_t, EE), pk.add(&d_v, EE), pk.add(&d_v_t, EE), pk.add(&d_temp2, radix::scratch_bytes(E));
    if (tmp.carve(pk)) return 1;
    launch_neighbour<true>(dim, n, st, B, d_off, (const Grid *)cg.d_grids, (const uint32_t *)cg.d_cell_base, M, r2,
                           (const float *)cg.d_sorted, (const int32_t *)cg.d_perm, (const uint32_t *)cg.d_key_s,
                           (const int32_t *)cg.d_cell_start, (uint32_t *)nullptr, (const unsigned long long *)d_offset, d_pk);
    AMP_LAUNCH_CHECK();
    // rows are already in order of i; the sort of the whole key orders the partners inside every row
    const int key_bits = bits_for((unsigned long long)n * M - 1ull);
    if (int rc = radix::sort_pairs<unsigned long long>((const unsigned long long *)d_pk, nullptr, E, key_bits, d_pk_s, d_v, d_pk_t, d_v_t,
                                                       d_temp2, st))
        return rc;
    hipLaunchKernelGGL(rgb_emit_kernel, dim3(blocks(E)), dim3(256), 0, st, E, B, d_off, M, (int)dim, (const unsigned long long *)d_pk_s,
                       points_dev, pairs_dev, coords_dev);
    AMP_LAUNCH_CHECK();
    AMP_HIP(hipStreamSynchronize(st));   // scratch dies with this scope
    return 0;
}

// One cloud: the checks of the single-cloud entries, in their order, then a batch of one.  n = 0 returns before the square of
// the radius is looked at, as it always did.
int radius_pairs_core(int32_t n, int32_t dim, const float *points_dev, float radius, int32_t *pairs_dev, float *coords_dev,
                      int64_t capacity, int64_t *n_pairs_out)
{
    AMP_REQUIRE(n_pairs_out != nullptr, "radius_pairs: null n_pairs_out");
    *n_pairs_out = 0;
    AMP_REQUIRE(dim >= 1 && dim <= 3, "radius_pairs: dim = %d outside [1,3]", dim);
    AMP_REQUIRE(isfinite(radius) && radius > 0.f, "radius_pairs: radius = %g is not a positive finite number", (double)radius);
    AMP_REQUIRE(n >= 0 && (n == 0 || points_dev != nullptr), "radius_pairs: bad arguments");
    if (n == 0) return 0;
    const int32_t offsets[2] = {0, n};
    return radius_pairs_batched_core(kSingle, 1, n, offsets, dim, points_dev, radius, pairs_dev, coords_dev, capacity, nullptr, n_pairs_out);
}

} // namespace amp

extern "C" int athena_mp_radius_pairs(int32_t n, int32_t dim, const float *points_dev, float radius, int32_t *pairs_dev,
                                      float *coords_dev, int64_t capacity, int64_t *n_pairs_out)
{
    return amp::radius_pairs_core(n, dim, points_dev, radius, pairs_dev, coords_dev, capacity, n_pairs_out);
}

extern "C" int athena_mp_radius_graph_host(int32_t n, int32_t dim, const float *points_host, float radius, int32_t add_self_loops,
                                           int32_t *adj_ia_out, int32_t *adj_ja_out, int64_t capacity, int64_t *nnz_out,
                                           float *coords_out, int64_t coords_capacity, int64_t *n_pairs_out)
{
    AMP_REQUIRE(nnz_out != nullptr && n_pairs_out != nullptr, "radius_graph_host: null output pointer");
    *nnz_out = *n_pairs_out = 0;
    AMP_REQUIRE(n >= 0 && dim >= 1 && dim <= 3 && (n == 0 || points_host != nullptr), "radius_graph_host: bad arguments (n = %d, dim = %d)",
                n, dim);
    hipStream_t st = amp::stream();
    Scratch tmp;
    float *d_pts = nullptr;
    if (tmp.upload(&d_pts, points_host, (size_t)n * dim, st)) return 1;
    int64_t E = 0;
    if (int rc = amp::radius_pairs_core(n, dim, d_pts, radius, nullptr, nullptr, 0, &E)) return rc;
    return amp::graph_host_tail("radius_graph_host", n, dim, E, add_self_loops, adj_ia_out, adj_ja_out, capacity, nnz_out, coords_out,
                           coords_capacity, n_pairs_out, st, [&](int32_t **d_pairs, float **d_coords) {
                               if (tmp.get(d_pairs, 2 * (size_t)E) || tmp.get(d_coords, (size_t)E * dim)) return 1;
                               return amp::radius_pairs_core(n, dim, d_pts, radius, *d_pairs, *d_coords, E, &E);
                           });
}

extern "C" int athena_mp_radius_pairs_batched(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim,
                                              const float *points_dev, float radius, int32_t *pairs_dev, float *coords_dev,
                                              int64_t capacity, int64_t *edge_offsets_host, int64_t *n_pairs_out)
{
    return amp::radius_pairs_batched_core(kBatched, n_clouds, n, offsets_host, dim, points_dev, radius, pairs_dev, coords_dev, capacity,
                                          edge_offsets_host, n_pairs_out);
}

extern "C" int athena_mp_radius_graph_batched_host(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim,
                                                   const float *points_host, float radius, int32_t add_self_loops, int32_t *adj_ia_out,
                                                   int32_t *adj_ja_out, int64_t capacity, int64_t *nnz_out, float *coords_out,
                                                   int64_t coords_capacity, int64_t *n_pairs_out, int64_t *edge_offsets_out)
{
    AMP_REQUIRE(nnz_out != nullptr && n_pairs_out != nullptr, "radius_graph_batched_host: null output pointer");
    *nnz_out = *n_pairs_out = 0;
    AMP_REQUIRE(n >= 0 && (n == 0 || points_host != nullptr), "radius_graph_batched_host: bad arguments (n = %d)", n);
    // before the points are uploaded: dim sizes the copy
    if (int rc = batch_arguments_check("radius_graph_batched_host", n_clouds, offsets_host, dim, radius)) return rc;
    hipStream_t st = amp::stream();
    Scratch tmp;
    float *d_pts = nullptr;
    if (tmp.upload(&d_pts, points_host, (size_t)n * dim, st)) return 1;
    int64_t E = 0;
    if (int rc = amp::radius_pairs_batched_core(kBatched, n_clouds, n, offsets_host, dim, d_pts, radius, nullptr, nullptr, 0,
                                                edge_offsets_out, &E))
        return rc;
    return amp::graph_host_tail("radius_graph_batched_host", n, dim, E, add_self_loops, adj_ia_out, adj_ja_out, capacity, nnz_out, coords_out,
                           coords_capacity, n_pairs_out, st, [&](int32_t **d_pairs, float **d_coords) {
                               if (tmp.get(d_pairs, 2 * (size_t)E) || tmp.get(d_coords, (size_t)E * dim)) return 1;
                               return amp::radius_pairs_batched_core(kBatched, n_clouds, n, offsets_host, dim, d_pts, radius, *d_pairs,
                                                                     *d_coords, E, edge_offsets_out, &E);
                           });
}
