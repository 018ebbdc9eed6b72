// Queries x sources -> radius graph between TWO point sets on the device, a batch of clouds per call: the step in front of
// athena_mp_graph_create_bipartite_dev for graph_nop_layer_type(local_term=False) -- the kernel integral evaluated at points that
// are not the input points (a mesh onto a latent grid, a latent grid onto query points).  Neither graphstruc nor the reference's
// layer has such a call.
//
// The definition (every implementation gives the same arrays; tests compare with np.array_equal):
//   * delta = q_i - p_j component by component in fp32, s = ((d0*d0) + d1*d1) + d2*d2 with every multiply and add rounded to
//     fp32 on its own; query i and source j of ONE cloud are joined iff s <= fl(radius * radius): joined<DIM> of radius_cells.h,
//     the predicate of radius_graph.hip, unchanged.  The two sets have separate index spaces: there is no self-pair rule, a
//     query that coincides with a source is joined to it, and whether i == j is of no interest.
//   * pairs are numbered in lexicographic order of the global (i, j); pairs[:, e] = (i + 1, j + 1); coords[e, :] = q_i - p_j;
//     rowptr[i] = pairs whose query is below i (0-based), rowptr[n_queries] = the pair count;
//     edge_offsets[b] = rowptr[query_offsets[b]] (include/athena_mp.h).
//
// How.  The grid is build_cell_grid of cell_grid.h over the SOURCES only, with make_grid's rule (radius_cells.h): cells at least
// radius * (1 + 2^-10) wide, the per-axis and the per-cloud cap; a source cloud's cells are a disjoint key range.  The queries get
// the finite check of batch_boxes and then ONE key pass that places each in its cloud's source grid (query_cell below) and one
// stable pass of radix_sort.h on (cell, query id): the kernels below walk the queries in that order, as rgb_neighbour_kernel
// walks its points in cell order, so the lanes of a wave read the same source cells.  COUNT: every query counts its partners in
// the source cells in reach, written by query id; an exclusive scan IN QUERY-ID ORDER (64-bit, scan64.h), which is rowptr;
// FILL: keys i * M + (j - source_offsets[b]) with M the largest source cloud, into those rows; one radix sort of the keys orders
// the partners of each row; one pass decodes keys into pairs and coords.  No atomics on data; every access to coordinates is 4
// bytes wide.
//
// The query's cell, and why the margin still holds.  A source's cell on an axis is min(floor(g(p)), nc - 1) with
// g(p) = fl(fl(p - lo) * inv_w) (cell_coord of cell_grid.h); p >= lo there, so g >= 0 and its floor lies in 0 .. nc (p = hi gives
// nc, or nc(1 + 3 * 2^-24), never nc + 1 at nc <= 2048).  A query may lie anywhere: below lo, beyond hi, at +-3e38.  query_cell
// takes the SAME g and clamps it in floating point to [-2, nc + 2] before the floor, so the conversion to an integer never sees
// a negative number it would truncate towards zero, nor a huge one, nor a NaN:
//   * p < lo: fl(p - lo) = -fl(lo - p) (rounding is symmetric), so g is still monotone in p over all finite p and each of its
//     two roundings still within 2^-24 relative; floorf, not truncation, makes the cell.
//   * |p - lo| beyond FLT_MAX gives +-inf, and inf * inv_w is +-inf (clamped like any large value) or, on a one-cell axis
//     (inv_w = 0), NaN; fmaxf(NaN, -2) = -2: the query counts as out of reach, which it is (radius^2 is finite in fp32).
//   * clamping is monotone and does not expand distances: where the unclamped floors of a query and of a source differ by at
//     most one, so do the clamped ones, unless both clamp -- and a source's floor is never clamped here.
// The header of radius_graph.hip shows that a kept pair's exact cell coordinates differ by less than 1 - 2^-10 + 2^-19 and that
// the computed ones are within 3 * 2^-24 * |g| of exact; a query that has a partner lies within one cell of the box, |g| <= nc + 1
// <= 2049, and 6 * 2^-24 * 2049 + 2^-19 < 2^-10 still: the computed g differ by less than one, their floors by at most one.  So
// the partners of a query with floor c have floors in [c - 1, c + 1] /\ [0, nc], i.e. sit in the cells min(., nc - 1) of that
// range.  A range that is empty after the clamp (c = -2 or c = nc + 2, or a cloud without sources) is a query with no source
// cell in reach: it reads no cell.  There is no distance test beside the predicate.
//
// The handle.  bipartite_csr_from_pairs turns such a pair list into the directed rectangular CSR (row i, column j, edge id e: no
// reverse entry, no self loops) and its degrees, for athena_mp_graph_create_bipartite_dev in capi.hip.
#include <math.h>

#include <algorithm>

#include "call_scratch.h"
#include "cell_grid.h"
#include "common.h"
#include "radius_cells.h"
#include "radix_sort.h"
#include "scan64.h"
#include "two_sets.h"

namespace {

// the cells of one axis a query has to read: lo > hi means none
struct CellRange {
    int32_t lo, hi;
};

// the floor of the clamped cell coordinate of a query on one axis (see the file header): -2 .. nc + 2
__device__ inline int32_t query_cell(float p, float lo, float inv_w, int32_t nc)
{
    float q = cell_q(p, lo, inv_w);
    q = fminf(fmaxf(q, -2.f), (float)(nc + 2));       // NaN (inf * 0) -> -2
    return (int32_t)floorf(q);
}

__device__ inline CellRange query_range(int32_t c, int32_t nc)
{
    const int32_t rlo = max(c - 1, 0), rhi = min(c + 1, nc);          // floors of sources in reach: 0 .. nc
    CellRange r;
    r.lo = min(rlo, nc - 1);                                          // their cells
    r.hi = rlo <= rhi ? min(rhi, nc - 1) : r.lo - 1;
    return r;
}

// One wave per work item of the QUERIES (cloud, q0 .. q1-1): the key a query is sorted by = cell_base[cloud] + the cell of its
// cloud's source grid nearest to it.  The key only orders the walk; which cells a query reads is decided in the walk itself.
__global__ __launch_bounds__(64 * kItemWaves) void bip_query_key_kernel(int32_t n_items, const int32_t *__restrict__ items, int dim,
                                                                        const float *__restrict__ q, const Grid *__restrict__ grids,
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
        for (int k = dim - 1; k >= 0; --k) {
            if (g.nc[k] < 1) continue;                                 // a cloud without sources has no grid
            const int32_t cc = min(max(query_cell(q[i * dim + k], g.lo[k], g.inv_w[k], g.nc[k]), 0), g.nc[k] - 1);
            c = c * (uint32_t)g.nc[k] + (uint32_t)cc;
        }
        key[i] = base + c;
    }
}

// One thread per slot of the queries' cell order: query i = qperm[slot] against every source of the cells in reach, in its cloud's
// grid.  FILL = false: count[i] = number of partners.  FILL = true: key[offset[i] + t] = i * M + (j - source_offsets[cloud]) for
// the t-th partner found.
template <int DIM, bool FILL>
__global__ __launch_bounds__(256) void bip_neighbour_kernel(int32_t nq, int32_t B, const int32_t *__restrict__ q_offsets,
                                                            const int32_t *__restrict__ s_offsets, const Grid *__restrict__ grids,
                                                            const uint32_t *__restrict__ cell_base, unsigned long long M, float r2,
                                                            const float *__restrict__ queries, const int32_t *__restrict__ qperm,
                                                            const float *__restrict__ sorted, const int32_t *__restrict__ perm,
                                                            const int32_t *__restrict__ cell_start, uint32_t *__restrict__ count,
                                                            const unsigned long long *__restrict__ offset,
                                                            unsigned long long *__restrict__ key)
{
    const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (slot >= nq) return;
    const int32_t i = qperm[slot];
    const int32_t b = cloud_of(B, q_offsets, i);
    const int32_t first_source = s_offsets[b];
    uint32_t found = 0;
    if (s_offsets[b + 1] > first_source) {
        const Grid g = grids[b];
        const uint32_t cb = cell_base[b];
        float p[3] = {0.f, 0.f, 0.f};
        CellRange r[3] = {{0, 0}, {0, 0}, {0, 0}};
        bool any = true;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            p[a] = queries[(int64_t)i * DIM + a];
            r[a] = query_range(query_cell(p[a], g.lo[a], g.inv_w[a], g.nc[a]), g.nc[a]);
            any = any && r[a].lo <= r[a].hi;
        }
        unsigned long long at = 0;
        if (FILL) at = offset[i];
        if (any)
            for (int z = r[2].lo; z <= r[2].hi; ++z)
                for (int y = r[1].lo; y <= r[1].hi; ++y) {
                    // the cells of one grid row are consecutive keys: one contiguous run of slots, all of this cloud
                    const uint32_t row = (DIM > 2 ? (uint32_t)z * (uint32_t)g.nc[1] : 0u) + (uint32_t)y;
                    const uint32_t first = cb + row * (uint32_t)g.nc[0] + (uint32_t)r[0].lo;
                    const int32_t beg = cell_start[first], end = cell_start[first + (uint32_t)(r[0].hi - r[0].lo) + 1u];
                    for (int32_t m = beg; m < end; ++m) {
                        if (!joined<DIM>(p, sorted + (int64_t)m * DIM, r2)) continue;       // q_i - p_j
                        if (FILL) key[at + found] = (unsigned long long)i * M + (unsigned long long)(perm[m] - first_source);
                        ++found;
                    }
                }
    }
    if (!FILL) count[i] = found;
}

// ---- sorted keys -> 1-based pair list [2, E] column-major and coords [E, dim] -------------------------------------------------
__global__ __launch_bounds__(256) void bip_emit_kernel(int64_t E, int32_t B, const int32_t *__restrict__ q_offsets,
                                                       const int32_t *__restrict__ s_offsets, unsigned long long M, int dim,
                                                       const unsigned long long *__restrict__ key, const float *__restrict__ queries,
                                                       const float *__restrict__ sources, int32_t *__restrict__ pairs,
                                                       float *__restrict__ coords)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const unsigned long long k = key[e];
    const int64_t i = (int64_t)(k / M);
    const int64_t j = (int64_t)s_offsets[cloud_of(B, q_offsets, (int32_t)i)] + (int64_t)(k % M);
    if (pairs) {
        pairs[2 * e] = (int32_t)i + 1;
        pairs[2 * e + 1] = (int32_t)j + 1;
    }
    if (coords)
        for (int a = 0; a < dim; ++a) coords[e * dim + a] = queries[i * dim + a] - sources[j * dim + a];
}

template <bool FILL, typename... A> void launch_bip_neighbour(int dim, int32_t nq, hipStream_t st, A... a)
{
    if (dim == 1) hipLaunchKernelGGL((bip_neighbour_kernel<1, FILL>), dim3(blocks(nq)), dim3(256), 0, st, nq, a...);
    else if (dim == 2) hipLaunchKernelGGL((bip_neighbour_kernel<2, FILL>), dim3(blocks(nq)), dim3(256), 0, st, nq, a...);
    else hipLaunchKernelGGL((bip_neighbour_kernel<3, FILL>), dim3(blocks(nq)), dim3(256), 0, st, nq, a...);
}

// what every entry checks before anything touches the device: 0, or 2 with the message set
int bipartite_arguments_check(const char *who, int32_t B, int32_t nq, const int32_t *q_offsets, int32_t ns, const int32_t *s_offsets,
                              int32_t dim, float radius)
{
    AMP_REQUIRE(dim >= 1 && dim <= 3, "%s: dim = %d outside [1,3]", who, dim);
    AMP_REQUIRE(isfinite(radius) && radius > 0.f, "%s: radius = %g is not a positive finite number", who, (double)radius);
    AMP_REQUIRE(isfinite(radius * radius), "%s: radius = %g squared is not finite in fp32", who, (double)radius);
    AMP_REQUIRE(B >= 0, "%s: n_clouds = %d is negative", who, B);
    AMP_REQUIRE(nq >= 0 && ns >= 0, "%s: n_queries = %d, n_sources = %d: negative", who, nq, ns);
    if (int rc = named_offsets_check(who, "query_offsets", "queries", B, q_offsets, nq)) return rc;
    return named_offsets_check(who, "source_offsets", "sources", B, s_offsets, ns);
}

// ---- pair list -> directed CSR ------------------------------------------------------------------------------------------------
// pair e = (i, j) 1-based: entry e of the CSR is (column j, edge id e + 1); in range and strictly above pair e - 1, or the smallest
// such e is reported.  col_deg[j] counts the entries of column j: an integer count, the same whatever the order of the additions.
__global__ __launch_bounds__(256) void bip_entries_kernel(int64_t E, const int32_t *__restrict__ pairs, int32_t n_rows, int32_t n_cols,
                                                          int32_t *__restrict__ ja, int32_t *__restrict__ col_deg,
                                                          unsigned long long *__restrict__ bad)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int32_t i = pairs[2 * e], j = pairs[2 * e + 1];
    bool ok = i >= 1 && i <= n_rows && j >= 1 && j <= n_cols;
    if (ok && e > 0) {
        const int32_t pi = pairs[2 * e - 2], pj = pairs[2 * e - 1];
        ok = pi < i || (pi == i && pj < j);
    }
    if (!ok) {
        atomicMin(bad, (unsigned long long)e);
        return;
    }
    ja[2 * e] = j;
    ja[2 * e + 1] = (int32_t)e + 1;
    atomicAdd(col_deg + (j - 1), 1);
}

// adj_ia[v] = 1 + the first pair whose row is >= v + 1  (v = 0 .. n_rows), for an ascending list
__global__ __launch_bounds__(256) void bip_rows_kernel(int32_t n_rows, int64_t E, const int32_t *__restrict__ pairs,
                                                       int32_t *__restrict__ adj_ia)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v > n_rows) return;
    int64_t lo = 0, hi = E;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)pairs[2 * mid] < v + 1) lo = mid + 1; else hi = mid;
    }
    adj_ia[v] = (int32_t)lo + 1;
}

} // namespace

namespace amp {

// pairs_dev, coords_dev and rowptr_dev all null: count only (edge_offsets_out is filled either way).  Everything on the library's
// stream; synchronised on return.
int radius_pairs_bipartite_core(const char *who, int32_t B, int32_t nq, const int32_t *q_offsets, int32_t ns, const int32_t *s_offsets,
                                int32_t dim, const float *queries_dev, const float *sources_dev, float radius, int32_t *pairs_dev,
                                float *coords_dev, int64_t capacity, int32_t *rowptr_dev, int64_t *edge_offsets_out, int64_t *n_pairs_out)
{
    AMP_REQUIRE(n_pairs_out != nullptr, "%s: null n_pairs_out", who);
    *n_pairs_out = 0;
    if (int rc = bipartite_arguments_check(who, B, nq, q_offsets, ns, s_offsets, dim, radius)) return rc;
    AMP_REQUIRE(nq == 0 || queries_dev != nullptr, "%s: null queries", who);
    AMP_REQUIRE(ns == 0 || sources_dev != nullptr, "%s: null sources", who);
    if (edge_offsets_out) std::fill(edge_offsets_out, edge_offsets_out + B + 1, (int64_t)0);
    hipStream_t st = stream();
    if (rowptr_dev) AMP_HIP(hipMemsetAsync(rowptr_dev, 0, sizeof(int32_t) * ((size_t)nq + 1), st));
    const float r2 = radius * radius;
    const bool fill = pairs_dev != nullptr || coords_dev != nullptr;

    // both sets are scanned for a non-finite coordinate, the queries first; then the grid of the sources
    Scratch tmp;
    BatchItems qit;
    CellGrid cg;
    if (nq > 0) {
        std::vector<Box> qbox;
        if (int rc = batch_boxes(who, true, B, q_offsets, dim, queries_dev, st, tmp, qit, qbox, "queries")) return rc;
    }
    if (ns > 0)
        if (int rc = build_cell_grid(who, true, B, ns, s_offsets, dim, sources_dev, st, tmp,
                                     [&](const Box &box, int32_t m, int32_t) { return make_grid(box, dim, m, radius); }, cg, "sources"))
            return rc;
    if (nq == 0 || ns == 0) {
        AMP_HIP(hipStreamSynchronize(st));
        return 0;
    }
    const int32_t *d_qoff = qit.d_off, *d_soff = cg.it.d_off;

    // the queries in the order of their cell: one key pass, one stable pass of the sort
    uint32_t *d_qkey = nullptr, *d_qkey_s = nullptr, *d_qkey_t = nullptr, *d_count = nullptr;
    int32_t *d_qperm = nullptr, *d_qperm_t = nullptr;
    char *d_temp = nullptr;
    unsigned long long *d_tile = nullptr, *d_offset = nullptr;
    long long *d_edge_off = nullptr;
    const size_t NQ = (size_t)nq;
    Pieces pc;
    pc.add(&d_qkey, NQ), pc.add(&d_qkey_s, NQ), pc.add(&d_qkey_t, NQ), pc.add(&d_qperm, NQ), pc.add(&d_qperm_t, NQ);
    pc.add(&d_temp, radix::scratch_bytes(nq)), pc.add(&d_count, NQ), pc.add(&d_tile, (size_t)scan64::tiles(nq) + 1), pc.add(&d_offset, NQ);
    pc.add(&d_edge_off, (size_t)B + 1);
    if (tmp.carve(pc)) return 1;
    hipLaunchKernelGGL(bip_query_key_kernel, dim3(qit.item_blocks), dim3(64 * kItemWaves), 0, st, qit.W, (const int32_t *)qit.d_items,
                       (int)dim, queries_dev, (const Grid *)cg.d_grids, (const uint32_t *)cg.d_cell_base, d_qkey);
    AMP_LAUNCH_CHECK();
    // a cloud without sources puts its queries at its (empty) key range's start, which may be n_cells itself
    if (int rc = radix::sort_pairs<uint32_t>((const uint32_t *)d_qkey, nullptr, nq, bits_for(cg.n_cells), d_qkey_s, d_qperm, d_qkey_t,
                                             d_qperm_t, d_temp, st))
        return rc;

    const unsigned long long M = (unsigned long long)cg.it.m_max;
    launch_bip_neighbour<false>(dim, nq, st, B, d_qoff, d_soff, (const Grid *)cg.d_grids, (const uint32_t *)cg.d_cell_base, M, r2,
                                queries_dev, (const int32_t *)d_qperm, (const float *)cg.d_sorted, (const int32_t *)cg.d_perm,
                                (const int32_t *)cg.d_cell_start, d_count, (const unsigned long long *)nullptr,
                                (unsigned long long *)nullptr);
    const unsigned long long *d_total = scan64::exclusive(nq, (const uint32_t *)d_count, d_tile, d_offset, st);
    AMP_LAUNCH_CHECK();
    unsigned long long total = 0;
    AMP_HIP(hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    // the limit of an int32 CSR, found by the count pass before anything of that size is allocated
    AMP_REQUIRE(total < (1ull << 31), "%s: %llu pairs between %d queries and %d sources: more than 2^31 CSR entries", who, total, nq, ns);
    hipLaunchKernelGGL(bip_rowptr_kernel, dim3(blocks((int64_t)std::max(nq, B) + 1)), dim3(256), 0, st, nq, B, d_qoff,
                       (const unsigned long long *)d_offset, d_total, rowptr_dev, d_edge_off);
    AMP_LAUNCH_CHECK();
    if (edge_offsets_out)
        AMP_HIP(hipMemcpyAsync(edge_offsets_out, d_edge_off, sizeof(int64_t) * ((size_t)B + 1), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    *n_pairs_out = (int64_t)total;
    if (!fill) return 0;
    AMP_REQUIRE(capacity >= (int64_t)total, "%s: the output buffers hold %lld pairs, the batch has %lld", who, (long long)capacity,
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
    launch_bip_neighbour<true>(dim, nq, st, B, d_qoff, d_soff, (const Grid *)cg.d_grids, (const uint32_t *)cg.d_cell_base, M, r2,
                               queries_dev, (const int32_t *)d_qperm, (const float *)cg.d_sorted, (const int32_t *)cg.d_perm,
                               (const int32_t *)cg.d_cell_start, (uint32_t *)nullptr, (const unsigned long long *)d_offset, d_pk);
    AMP_LAUNCH_CHECK();
    // rows are already in order of i; the sort of the whole key orders the partners inside every row
    const int key_bits = bits_for((unsigned long long)nq * M - 1ull);
    if (int rc = radix::sort_pairs<unsigned long long>((const unsigned long long *)d_pk, nullptr, E, key_bits, d_pk_s, d_v, d_pk_t, d_v_t,
                                                       d_temp2, st))
        return rc;
    hipLaunchKernelGGL(bip_emit_kernel, dim3(blocks(E)), dim3(256), 0, st, E, B, d_qoff, d_soff, M, (int)dim,
                       (const unsigned long long *)d_pk_s, queries_dev, sources_dev, pairs_dev, coords_dev);
    AMP_LAUNCH_CHECK();
    AMP_HIP(hipStreamSynchronize(st));   // scratch dies with this scope
    return 0;
}

// pairs [2, n_pairs] on the device, strictly ascending in (i, j) -> adj_ia [n_rows + 1] (host, 1-based), the entries
// (column, edge id) [2, n_pairs] on the device (*ja_dev: hipFree it) and on the host when adj_ja_out is given, and the degrees:
// row_deg[i] = the row's length, col_deg[j] = the entries of column j.
int bipartite_csr_from_pairs(const char *who, int32_t n_rows, int32_t n_cols, int64_t n_pairs, const int32_t *pairs_dev,
                             int32_t *adj_ia_out, int32_t *adj_ja_out, int64_t capacity, int32_t **ja_dev, std::vector<int32_t> *row_deg,
                             std::vector<int32_t> *col_deg)
{
    *ja_dev = nullptr;
    AMP_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_pairs >= 0 && adj_ia_out != nullptr && (n_pairs == 0 || pairs_dev != nullptr),
                "%s: bad arguments", who);
    AMP_REQUIRE(n_pairs < (int64_t)INT32_MAX, "%s: %lld pairs: more than 2^31 CSR entries", who, (long long)n_pairs);
    AMP_REQUIRE(adj_ja_out == nullptr || capacity >= n_pairs, "%s: adj_ja buffer holds %lld entries, the graph has %lld", who,
                (long long)capacity, (long long)n_pairs);
    hipStream_t st = stream();
    Scratch tmp;
    int32_t *d_ia = nullptr, *d_cdeg = nullptr, *d_ja = nullptr;
    BadWord word;
    if (tmp.get(&d_ia, (size_t)n_rows + 1) || tmp.get(&d_cdeg, n_cols) || word.arm(tmp, st)) return 1;
    AMP_HIP(hipMalloc((void **)&d_ja, sizeof(int32_t) * 2 * (size_t)std::max<int64_t>(n_pairs, 1)));
    *ja_dev = d_ja;                                                    // the caller frees it on every path from here
    AMP_HIP(hipMemsetAsync(d_cdeg, 0, sizeof(int32_t) * (size_t)std::max(n_cols, 1), st));
    if (n_pairs > 0) {
        hipLaunchKernelGGL(bip_entries_kernel, dim3(blocks(n_pairs)), dim3(256), 0, st, n_pairs, pairs_dev, n_rows, n_cols, d_ja, d_cdeg,
                           word.dev);
        AMP_LAUNCH_CHECK();
    }
    unsigned long long bad = ~0ull;
    if (int rc = word.fetch(&bad, st)) return rc;
    if (bad != ~0ull) {
        int32_t p[4] = {0, 0, 0, 0};                                   // the pair in front of it and the pair itself
        const unsigned long long from = bad > 0 ? bad - 1 : bad;
        AMP_HIP(hipMemcpy(p + 2 * (from == bad), pairs_dev + 2 * from, sizeof(int32_t) * 2 * (size_t)(bad - from + 1), hipMemcpyDeviceToHost));
        if (p[2] < 1 || p[2] > n_rows || p[3] < 1 || p[3] > n_cols)
            set_error("%s: pairs(:,%llu) = (%d, %d) outside [1,%d] x [1,%d]", who, bad + 1, p[2], p[3], n_rows, n_cols);
        else
            set_error("%s: pairs(:,%llu) = (%d, %d) does not ascend from pairs(:,%llu) = (%d, %d): the list must be strictly ascending in "
                      "(query, source)",
                      who, bad + 1, p[2], p[3], bad, p[0], p[1]);
        return 2;
    }
    hipLaunchKernelGGL(bip_rows_kernel, dim3(blocks((int64_t)n_rows + 1)), dim3(256), 0, st, n_rows, n_pairs, pairs_dev, d_ia);
    AMP_LAUNCH_CHECK();
    row_deg->resize((size_t)n_rows);
    col_deg->resize((size_t)n_cols);
    AMP_HIP(hipMemcpyAsync(adj_ia_out, d_ia, sizeof(int32_t) * ((size_t)n_rows + 1), hipMemcpyDeviceToHost, st));
    if (n_cols > 0) AMP_HIP(hipMemcpyAsync(col_deg->data(), d_cdeg, sizeof(int32_t) * (size_t)n_cols, hipMemcpyDeviceToHost, st));
    if (adj_ja_out && n_pairs > 0)
        AMP_HIP(hipMemcpyAsync(adj_ja_out, d_ja, sizeof(int32_t) * 2 * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    for (int32_t v = 0; v < n_rows; ++v) (*row_deg)[v] = adj_ia_out[v + 1] - adj_ia_out[v];
    return 0;
}

} // namespace amp

extern "C" int athena_mp_radius_pairs_bipartite(int32_t n_clouds, int32_t n_queries, const int32_t *query_offsets_host, int32_t n_sources,
                                                const int32_t *source_offsets_host, int32_t dim, const float *queries_dev,
                                                const float *sources_dev, float radius, int32_t *pairs_dev, float *coords_dev,
                                                int64_t capacity, int32_t *rowptr_dev, int64_t *edge_offsets_host, int64_t *n_pairs_out)
{
    return amp::radius_pairs_bipartite_core("radius_pairs_bipartite", n_clouds, n_queries, query_offsets_host, n_sources,
                                            source_offsets_host, dim, queries_dev, sources_dev, radius, pairs_dev, coords_dev, capacity,
                                            rowptr_dev, edge_offsets_host, n_pairs_out);
}

// Fortran arrays in, Fortran arrays out.  Its own tail: graph_host_tail of common.h symmetrises, and this graph is directed.
extern "C" int athena_mp_radius_graph_bipartite_host(int32_t n_clouds, int32_t n_queries, const int32_t *query_offsets_host,
                                                     int32_t n_sources, const int32_t *source_offsets_host, int32_t dim,
                                                     const float *queries_host, const float *sources_host, float radius,
                                                     int32_t *adj_ia_out, int32_t *adj_ja_out, int64_t capacity, float *coords_out,
                                                     int64_t coords_capacity, int64_t *edge_offsets_out, int64_t *n_pairs_out)
{
    const char *who = "radius_graph_bipartite_host";
    AMP_REQUIRE(n_pairs_out != nullptr, "%s: null n_pairs_out", who);
    *n_pairs_out = 0;
    // before the points are uploaded: dim and the counts size the copies
    if (int rc = bipartite_arguments_check(who, n_clouds, n_queries, query_offsets_host, n_sources, source_offsets_host, dim, radius))
        return rc;
    AMP_REQUIRE((n_queries == 0 || queries_host != nullptr) && (n_sources == 0 || sources_host != nullptr), "%s: null points", who);
    hipStream_t st = amp::stream();
    amp::Scratch tmp;
    float *d_q = nullptr, *d_s = nullptr;
    if (tmp.upload(&d_q, queries_host, (size_t)n_queries * dim, st) || tmp.upload(&d_s, sources_host, (size_t)n_sources * dim, st)) return 1;
    int64_t E = 0;
    if (int rc = amp::radius_pairs_bipartite_core(who, n_clouds, n_queries, query_offsets_host, n_sources, source_offsets_host, dim, d_q,
                                                  d_s, radius, nullptr, nullptr, 0, nullptr, edge_offsets_out, &E))
        return rc;
    *n_pairs_out = E;
    if (adj_ja_out == nullptr) return 0;                          // size query
    AMP_REQUIRE(adj_ia_out != nullptr && (coords_out != nullptr || E == 0), "%s: null output array", who);
    AMP_REQUIRE(capacity >= E, "%s: adj_ja buffer holds %lld entries, the graph has %lld", who, (long long)capacity, (long long)E);
    AMP_REQUIRE(coords_capacity >= E, "%s: coords buffer holds %lld pairs, the graph has %lld", who, (long long)coords_capacity, (long long)E);
    int32_t *d_pairs = nullptr;
    float *d_coords = nullptr;
    if (tmp.get(&d_pairs, 2 * (size_t)E) || tmp.get(&d_coords, (size_t)E * dim)) return 1;
    if (int rc = amp::radius_pairs_bipartite_core(who, n_clouds, n_queries, query_offsets_host, n_sources, source_offsets_host, dim, d_q,
                                                  d_s, radius, d_pairs, d_coords, E, nullptr, edge_offsets_out, &E))
        return rc;
    if (tmp.download(coords_out, d_coords, (size_t)E * dim, st)) return 1;
    int32_t *ja_dev = nullptr;
    std::vector<int32_t> row_deg, col_deg;
    const int rc = amp::bipartite_csr_from_pairs(who, n_queries, n_sources, E, d_pairs, adj_ia_out, adj_ja_out, capacity, &ja_dev, &row_deg,
                                                 &col_deg);
    if (ja_dev) (void)hipFree(ja_dev);
    if (rc) return rc;
    AMP_HIP(hipStreamSynchronize(st));
    return 0;
}
