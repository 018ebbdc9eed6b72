// Queries x sources -> k-nearest-neighbour graph between TWO point sets on the device, a batch of clouds per call: every query is
// joined to the k nearest sources of its cloud.  The fourth of the point-cloud builders (radius_graph.hip, knn_graph.hip,
// bipartite_graph.hip), for the rectangular graphs of graph_nop_layer_type(local_term=False) where a fixed radius leaves a query
// in a sparse part of the sources without a partner and makes a hub of one in a dense part; also the join of PointNet++ feature
// propagation and of k-nearest-neighbour interpolation (sqdist is what their weights are made of).
//
// The definition (include/athena_mp.h; every implementation gives the same arrays, tests compare with np.array_equal):
//   * s(i, j) from d = q_i - p_j per component, s = ((d0*d0) + d1*d1) + d2*d2, every operation rounded to fp32 on its own: the
//     squared distance of the other builders, unchanged.
//   * the candidates of query i are ALL sources of its cloud (separate index spaces: no self rule, a query on top of a source is
//     joined to it at s = 0), with a finite radius only those with s <= fl(radius * radius); an s that overflows is +inf, which
//     without a cap is still a candidate and orders last.  Ordered by the key (s, j); N_k(i) is the first min(k, candidates).
//   * nbr [n_queries, k]: N_k(i) as 1-based global source ids in KEY order, padded with 0; sqdist [n_queries, k]: their s, padded
//     with +inf.  pairs: one per (i, j in N_k(i)) in lexicographic order of the global (i, j) -- inside a row the sources ascend
//     by INDEX --, coords[e] = q_i - p_j, rowptr and edge_offsets as in bipartite_graph.hip.
//
// How.  GRID: build_cell_grid over the SOURCES only with make_knn_grid (knn_cells.h: about two sources per cell).  The queries get
// the finite check of batch_boxes, then one key pass (the source cell nearest to the query) and one stable pass of radix_sort.h on
// (cell, query id), so neighbouring waves read the same cells.  SEARCH: one 64-lane wave per query, the best keys ascending across
// the lanes, shells of growing Chebyshev distance rho around the source cell nearest to the query, 64 candidates per step, a ballot
// against the k-th key, bitonic sort and merge in registers (wave_sort / wave_merge of knn_cells.h): the means of
// knn_search_kernel.  No LDS, no atomics, no scratch.  It writes nbr and sqdist in key order and a count per query.  ROWS: an
// exclusive scan of the counts in query-id order (scan64.h) is rowptr.  EMIT: one wave per query orders its row (at most 64
// entries) by source index with the same bitonic network and writes pairs and coords: no global sort of n_queries * k keys.
//
// THE RESULT IS DEFINED BY THE KEY ORDER ALONE; the grid decides only how much is examined.  The stop rule for a query that may
// lie anywhere, and its proof (what knn_graph.hip's header proves for 0 <= x < 2049, re-derived for |g| <= 2050):
//
// Cells.  On an axis with nc > 1 cells a SOURCE j has the cell c_j = min(floor(g_j), nc - 1), g_j = fl(fl(p - lo) * inv_w) (cell_q)
// with lo <= p, 0 <= x_j <= nc (1 + 2^-23) for the exact x = (p - lo) * inv_w, and |g_j - x_j| < e_s := 2049 (2^-23 + 2^-48), as
// there.  A QUERY takes the same function, g_raw = cell_q(q, lo, inv_w), and clamps it in floating point to [-2, nc + 2]:
// g = fminf(fmaxf(g_raw, -2), nc + 2), so the conversion to an integer never sees a huge number or a NaN.  Its centre is
// c = min(max(floor(g), 0), nc - 1): the source cell nearest to it on that axis.
//   * q below lo: fl(q - lo) = -fl(lo - q) (rounding is symmetric), so each of the two roundings is still within 2^-24 relative
//     and |g_raw - x_i| <= (2^-23 + 2^-48) |x_i|.
//   * where the clamp does nothing, |g| <= nc + 2 <= 2050, so |x_i| < 2051 and |g - x_i| < e := 2051 (2^-23 + 2^-48) < 2^-11.9.
//   * where it acts it moves g TOWARDS the grid: g_raw < -2 gives g = -2 with x_i < -2 + e, i.e. g - x_i > -e, and every gap
//     "above" below is formed with -g: it is shorter than with g_raw.  g_raw > nc + 2 likewise for the gaps "below".  A clamped
//     g can shorten a gap, never lengthen one: the bound stays a lower bound.
//   * a difference that overflows, fl(q - lo) = +-inf, gives g_raw = +-inf: clamped like any large value; x_i is finite and
//     beyond the clamp on that side, the case above.  On an axis of one cell inv_w = 0 and inf * 0 = NaN: fmaxf(NaN, -2) = -2.
//     That axis takes no part in the rule (next paragraph), and c = 0 is its only cell.
//
// After shell rho every cell within Chebyshev distance rho of c is read.  A source j of an unread cell differs from c by more
// than rho on some axis a WITH nc > 1 (an axis of one cell has no other cell: it is never "beyond").  On that axis
//   above (exists iff c + rho + 1 <= nc - 1):  c_j >= c + rho + 1 and floor(g_j) >= c_j, so g_j >= c + rho + 1 and
//     x_j - x_i > (c + rho + 1 - g) - (e_s + e).  For a query beyond the last cell c = nc - 1 and this side does not exist.
//   below (exists iff c - rho - 1 >= 0):  c_j <= c - rho - 1 < nc - 1 is not clamped, so g_j < c_j + 1 <= c - rho, and
//     x_i - x_j > (g - (c - rho)) - (e_s + e).  g >= c unless the query lies below the grid -- and then c = 0 and this side does
//     not exist.
// The kernel forms u = fl(fl(gap) - kMargin) with gap one of the two brackets.  -2 <= g <= 2050 and 0 <= c +- rho (+ 1) <= 2047
// on a side that exists, so both results are below 4096 in magnitude, where half an ulp is at most 2^-13: the two roundings add
// at most 2^-12.  e_s + e + 2^-12 < 2^-10.9 + 2^-12 < 2^-10 = kMargin, the margin of the one-set builder unchanged, so
// u <= gap - (e_s + e) whatever the roundings did, and in exact arithmetic
//   |q_i[a] - p_j[a]| > u / inv_w[a] >= u * w_low[a],   w_low[a] = 1 / inv_w[a] rounded DOWN to fp32 (on the host, in double).
// t = the smallest fl(u * w_low[a]) over the axes and sides that exist.  Whether any exists is a flag of its own: "none" is not
// read off t, whose value is then of no interest.
//
// Roundings of s, the bound fl(fl(t * t) * kShrink), its floor of 2^-100 and its cap at FLT_MAX: as in knn_graph.hip's header,
// word for word; nothing there depends on where the query lies.  An s that overflowed is +inf, above every bound (FLT_MAX at most):
// it never satisfies (1), and such a query reads on until (2) or (3).
//
// So after shell rho every source of an unread cell has s >= bound, and the search stops when
//   (1) the list is full and its k-th s is STRICTLY below bound; or
//   (2) there is a cap and bound > fl(radius * radius); or
//   (3) no axis has an unread side: the shells have covered the cloud's source grid.
// (3) holds at the latest at rho = the largest nc - 1, so the search ends.  A cloud without sources has no grid: its queries read
// nothing and get an empty row.
//
// The price outside the box.  The bound counts only ONE axis.  Without a cap a query d cells outside the source box walks about d
// shells before its k-th key can be below the bound (the shells grow on the other axes as well, most of their cells beside the
// query's reach), and a query far away reads the whole grid: correct and slow, as for the one-set builder's far clusters.  With a
// cap, (2) ends the search after a few shells wherever the query lies.  A tighter bound that adds the query's distance to the box
// on the other axes is not built.
#include <float.h>
#include <math.h>

#include <algorithm>

#include "cell_grid.h"
#include "common.h"
#include "knn_cells.h"
#include "radix_sort.h"
#include "scan64.h"
#include "two_sets.h"

namespace {

// the clamped cell coordinate of a query on one axis (file header): -2 .. nc + 2, never NaN
__device__ inline float query_g(float p, float lo, float inv_w, int32_t nc)
{
    return fminf(fmaxf(cell_q(p, lo, inv_w), -2.f), (float)(nc + 2));      // NaN (inf * 0) -> -2
}

// the source cell nearest to a query on one axis
__device__ inline int32_t centre_cell(float g, int32_t nc) { return min(max((int32_t)floorf(g), 0), nc - 1); }

// One wave per work item of the QUERIES (cloud, q0 .. q1-1): the key a query is sorted by = cell_base[cloud] + the cell of its
// cloud's source grid nearest to it, the centre of its shells.  The key only orders the walk.
__global__ __launch_bounds__(64 * kItemWaves) void knnb_query_key_kernel(int32_t n_items, const int32_t *__restrict__ items, int dim,
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
        for (int a = dim - 1; a >= 0; --a) {
            if (g.nc[a] < 1) continue;                                 // a cloud without sources has no grid
            c = c * (uint32_t)g.nc[a] + (uint32_t)centre_cell(query_g(q[i * dim + a], g.lo[a], g.inv_w[a], g.nc[a]), g.nc[a]);
        }
        key[i] = base + c;
    }
}

// One wave per slot of the queries' cell order: the query i = qperm[slot] against the source cells of its cloud, shell by shell
// (header).  nbr[i, 0..k-1] = N_k(i) as 1-based global source ids in key order, padded with 0; sqdist[i, 0..k-1] = their s, padded
// with +inf (either may be null); count[i] = min(k, candidates).  stat[0][slot] = candidates read, stat[1][slot] = cells read,
// stat[2][slot] = the last shell.
template <int DIM>
__global__ __launch_bounds__(64 * kQueryWaves) void knnb_search_kernel(int32_t nq, int32_t B, const int32_t *__restrict__ q_offsets,
                                                                       const int32_t *__restrict__ s_offsets,
                                                                       const Grid *__restrict__ grids, const WLow *__restrict__ wlow,
                                                                       const uint32_t *__restrict__ cell_base, int k, float r2,
                                                                       const float *__restrict__ queries, const int32_t *__restrict__ qperm,
                                                                       const float *__restrict__ sorted, const int32_t *__restrict__ perm,
                                                                       const int32_t *__restrict__ cell_start, int32_t *__restrict__ nbr,
                                                                       float *__restrict__ sqdist, uint32_t *__restrict__ count,
                                                                       uint32_t *__restrict__ stat)
{
    const int lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * kQueryWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (slot >= nq) return;                                  // the whole wave
    const int32_t i = __builtin_amdgcn_readfirstlane(qperm[slot]);
    const int32_t b = __builtin_amdgcn_readfirstlane(cloud_of(B, q_offsets, i));

    unsigned long long list = kNoKey;
    uint32_t n_cand = 0, n_cells = 0;
    int rho = 0;

    if (s_offsets[b + 1] > s_offsets[b]) {                   // a cloud without sources has no grid: nothing to read
        const Grid g = grids[b];
        const WLow wl = wlow[b];
        const uint32_t cb = cell_base[b];
        float p[3] = {0.f, 0.f, 0.f}, q[3] = {0.f, 0.f, 0.f};
        int32_t cc[3] = {0, 0, 0}, nc[3] = {1, 1, 1};
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            p[a] = queries[(int64_t)i * DIM + a];
            nc[a] = __builtin_amdgcn_readfirstlane(g.nc[a]);
            q[a] = query_g(p[a], g.lo[a], g.inv_w[a], nc[a]);
            cc[a] = __builtin_amdgcn_readfirstlane(centre_cell(q[a], nc[a]));
        }
        const bool capped = r2 < INFINITY;

        // the cells x0 .. x1 of grid row (z, y) are consecutive keys: one contiguous run of slots, all of this cloud
        auto read_run = [&](int z, int y, int x0, int x1) {
            const uint32_t first = cb + ((uint32_t)z * (uint32_t)nc[1] + (uint32_t)y) * (uint32_t)nc[0] + (uint32_t)x0;
            const int32_t beg = __builtin_amdgcn_readfirstlane(cell_start[first]);
            const int32_t end = __builtin_amdgcn_readfirstlane(cell_start[first + (uint32_t)(x1 - x0) + 1u]);
            n_cells += (uint32_t)(x1 - x0 + 1);
            n_cand += (uint32_t)(end - beg);
            for (int32_t m0 = beg; m0 < end; m0 += 64) {
                const int32_t m = m0 + lane;
                unsigned long long key = kNoKey;
                if (m < end) {
                    const int32_t j = perm[m];
                    float pj[3] = {0.f, 0.f, 0.f};
#pragma unroll
                    for (int a = 0; a < DIM; ++a) pj[a] = sorted[(int64_t)m * DIM + a];
                    const float s = sq_dist<DIM>(p, pj);         // q_i - p_j
                    if (s <= r2) key = ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(uint32_t)j;
                }
                const unsigned long long kth = __shfl(list, k - 1, 64);
                if (__ballot(key < kth) == 0ull) continue;       // nothing here enters the first k
                list = wave_merge(list, wave_sort(key, lane), lane);
            }
        };

        for (;; ++rho) {
            const int z0 = DIM > 2 ? max(cc[2] - rho, 0) : 0, z1 = DIM > 2 ? min(cc[2] + rho, nc[2] - 1) : 0;
            const int y0 = DIM > 1 ? max(cc[1] - rho, 0) : 0, y1 = DIM > 1 ? min(cc[1] + rho, nc[1] - 1) : 0;
            const int x0 = max(cc[0] - rho, 0), x1 = min(cc[0] + rho, nc[0] - 1);
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const bool face = rho == 0 || (DIM > 2 && abs(z - cc[2]) == rho) || (DIM > 1 && abs(y - cc[1]) == rho);
                    if (face) {
                        read_run(z, y, x0, x1);                  // the whole row lies in the shell
                    } else {                                     // only its two ends do
                        if (cc[0] - rho >= 0) read_run(z, y, cc[0] - rho, cc[0] - rho);
                        if (cc[0] + rho <= nc[0] - 1) read_run(z, y, cc[0] + rho, cc[0] + rho);
                    }
                }
            // the stop rule (header): t = the least distance, on one axis, to a cell not yet read
            float t = INFINITY;
            bool unread = false;                                 // a flag of its own, not t == INFINITY
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                if (nc[a] <= 1) continue;
                if (cc[a] + rho + 1 <= nc[a] - 1) {
                    t = fminf(t, (((float)(cc[a] + rho + 1) - q[a]) - kMargin) * wl.w[a]);
                    unread = true;
                }
                if (cc[a] - rho - 1 >= 0) {
                    t = fminf(t, ((q[a] - (float)(cc[a] - rho)) - kMargin) * wl.w[a]);
                    unread = true;
                }
            }
            if (!unread) break;                                  // (3) the shells have covered the cloud's source grid
            float bound = t > 0.f ? fminf((t * t) * kShrink, FLT_MAX) : 0.f;
            if (bound < 0x1p-100f) bound = 0.f;
            if (capped && bound > r2) break;                     // (2)
            const uint32_t kth_s = (uint32_t)(__shfl(list, k - 1, 64) >> 32);   // 0xffffffff while the list is short
            if (kth_s < __float_as_uint(bound)) break;           // (1) strictly below
        }
    }

    const bool held = lane < k && list != kNoKey;
    if (lane < k) {
        if (nbr) nbr[(int64_t)i * k + lane] = held ? (int32_t)(uint32_t)list + 1 : 0;
        if (sqdist) sqdist[(int64_t)i * k + lane] = held ? __uint_as_float((uint32_t)(list >> 32)) : INFINITY;
    }
    const unsigned long long mask = __ballot(held);
    if (lane == 0) {
        count[i] = (uint32_t)__popcll(mask);
        stat[slot] = n_cand;
        stat[(int64_t)nq + slot] = n_cells;
        stat[2 * (int64_t)nq + slot] = (uint32_t)rho;
    }
}

// One wave per query, in query-id order: the count[i] entries of nbr[i, :] ordered by source index (a row has at most 64: one key
// per lane, the bitonic network of the search) -> pairs and coords of the row, from offset[i] on.
__global__ __launch_bounds__(64 * kQueryWaves) void knnb_emit_kernel(int32_t nq, int k, int dim, const int32_t *__restrict__ nbr,
                                                                     const uint32_t *__restrict__ count,
                                                                     const unsigned long long *__restrict__ offset,
                                                                     const float *__restrict__ queries, const float *__restrict__ sources,
                                                                     int32_t *__restrict__ pairs, float *__restrict__ coords)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kQueryWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= nq) return;                                     // the whole wave
    const uint32_t c = count[i];
    if (c == 0) return;
    int32_t v = 0;
    if (lane < k) v = nbr[i * k + lane];
    const unsigned long long id = wave_sort(v > 0 ? (unsigned long long)(v - 1) : kNoKey, lane);
    if ((uint32_t)lane >= c) return;
    const int64_t at = (int64_t)offset[i] + lane, j = (int64_t)id;
    if (pairs) {
        pairs[2 * at] = (int32_t)i + 1;
        pairs[2 * at + 1] = (int32_t)j + 1;
    }
    if (coords)
        for (int a = 0; a < dim; ++a) coords[at * dim + a] = queries[i * dim + a] - sources[j * dim + a];
}

template <typename... A> void launch_knnb_search(int dim, int32_t nq, hipStream_t st, A... a)
{
    const dim3 grid((unsigned)(((int64_t)nq + kQueryWaves - 1) / kQueryWaves)), block(64 * kQueryWaves);
    if (dim == 1) hipLaunchKernelGGL(knnb_search_kernel<1>, grid, block, 0, st, nq, a...);
    else if (dim == 2) hipLaunchKernelGGL(knnb_search_kernel<2>, grid, block, 0, st, nq, a...);
    else hipLaunchKernelGGL(knnb_search_kernel<3>, grid, block, 0, st, nq, a...);
}

// what every entry checks before anything touches the device: 0, or 2 with the message set
int knn_bipartite_arguments_check(const char *who, int32_t B, int32_t nq, const int32_t *q_offsets, int32_t ns, const int32_t *s_offsets,
                                  int32_t dim, int32_t k, float radius)
{
    AMP_REQUIRE(dim >= 1 && dim <= 3, "%s: dim = %d outside [1,3]", who, dim);
    AMP_REQUIRE(k >= 1 && k <= 64, "%s: k = %d outside [1,64]", who, k);
    AMP_REQUIRE(radius > 0.f, "%s: radius = %g is not a positive number (+infinity: no cap)", who, (double)radius);   // NaN fails too
    AMP_REQUIRE(B >= 0, "%s: n_clouds = %d is negative", who, B);
    AMP_REQUIRE(nq >= 0 && ns >= 0, "%s: n_queries = %d, n_sources = %d: negative", who, nq, ns);
    if (int rc = named_offsets_check(who, "query_offsets", "queries", B, q_offsets, nq)) return rc;
    if (int rc = named_offsets_check(who, "source_offsets", "sources", B, s_offsets, ns)) return rc;
    AMP_REQUIRE((int64_t)nq * k < ((int64_t)1 << 31), "%s: n_queries * k = %lld: more than 2^31 neighbour entries", who, (long long)nq * k);
    return 0;
}

} // namespace

namespace amp {

// All five device outputs null: size query (edge_offsets_out is filled either way); each may be null alone.  Everything on the
// library's stream; synchronised on return.
int knn_pairs_bipartite_core(const char *who, int32_t B, int32_t nq, const int32_t *q_offsets, int32_t ns, const int32_t *s_offsets,
                             int32_t dim, const float *queries_dev, const float *sources_dev, int32_t k, float radius, int32_t *nbr_dev,
                             float *sqdist_dev, int32_t *pairs_dev, float *coords_dev, int64_t capacity, int32_t *rowptr_dev,
                             int64_t *edge_offsets_out, int64_t *n_pairs_out)
{
    AMP_REQUIRE(n_pairs_out != nullptr, "%s: null n_pairs_out", who);
    *n_pairs_out = 0;
    std::fill(g_knn_stats, g_knn_stats + 4, (int64_t)0);
    if (int rc = knn_bipartite_arguments_check(who, B, nq, q_offsets, ns, s_offsets, dim, k, radius)) return rc;
    AMP_REQUIRE(nq == 0 || queries_dev != nullptr, "%s: null queries", who);
    AMP_REQUIRE(ns == 0 || sources_dev != nullptr, "%s: null sources", who);
    if (edge_offsets_out) std::fill(edge_offsets_out, edge_offsets_out + B + 1, (int64_t)0);
    hipStream_t st = stream();
    const float r2 = radius * radius;            // +inf (no cap, or a square beyond fp32): every s passes
    const bool fill = pairs_dev != nullptr || coords_dev != nullptr;
    const bool size_query = !fill && nbr_dev == nullptr && sqdist_dev == nullptr && rowptr_dev == nullptr;
    const int64_t T = (int64_t)nq * k;

    // both sets are scanned for a non-finite coordinate, the queries first
    Scratch tmp;
    BatchItems qit;
    CellGrid cg;
    if (nq > 0) {
        std::vector<Box> qbox;
        if (int rc = batch_boxes(who, true, B, q_offsets, dim, queries_dev, st, tmp, qit, qbox, "queries")) return rc;
    }
    if (size_query && !(r2 < INFINITY)) {
        // without a cap a row holds min(k, sources of the cloud): no grid, no search
        if (ns > 0) {
            BatchItems sit;
            std::vector<Box> sbox;
            if (int rc = batch_boxes(who, true, B, s_offsets, dim, sources_dev, st, tmp, sit, sbox, "sources")) return rc;
        }
        int64_t total = 0;
        for (int32_t b = 0; b < B; ++b) {
            if (edge_offsets_out) edge_offsets_out[b] = total;
            total += (int64_t)(q_offsets[b + 1] - q_offsets[b]) * std::min<int64_t>(k, s_offsets[b + 1] - s_offsets[b]);
        }
        if (edge_offsets_out) edge_offsets_out[B] = total;
        *n_pairs_out = total;
        g_knn_stats[0] = nq;
        AMP_HIP(hipStreamSynchronize(st));
        return 0;
    }
    std::vector<WLow> wlow((size_t)std::max(B, 1));          // a cloud without sources keeps zeros
    if (ns > 0)
        if (int rc = build_cell_grid(who, true, B, ns, s_offsets, dim, sources_dev, st, tmp,
                                     [&](const Box &box, int32_t m, int32_t b) { return make_knn_grid(box, dim, m, &wlow[b]); }, cg, "sources"))
            return rc;
    g_knn_stats[0] = nq;
    if (rowptr_dev) AMP_HIP(hipMemsetAsync(rowptr_dev, 0, sizeof(int32_t) * ((size_t)nq + 1), st));
    if (nq == 0 || ns == 0) {                                // no pairs; every row is padding
        if (nbr_dev && T > 0) AMP_HIP(hipMemsetAsync(nbr_dev, 0, sizeof(int32_t) * (size_t)T, st));
        if (sqdist_dev && T > 0) AMP_HIP(hipMemsetD32Async((hipDeviceptr_t)sqdist_dev, 0x7f800000, (size_t)T, st));
        AMP_HIP(hipStreamSynchronize(st));
        return 0;
    }
    const int32_t *d_qoff = qit.d_off, *d_soff = cg.it.d_off;

    // the queries in the order of their centre cell: one key pass, one stable pass of the sort
    uint32_t *d_qkey = nullptr, *d_qkey_s = nullptr, *d_qkey_t = nullptr, *d_count = nullptr, *d_stat = nullptr;
    int32_t *d_qperm = nullptr, *d_qperm_t = nullptr, *d_nbr = nbr_dev;
    char *d_temp = nullptr;
    unsigned long long *d_tile = nullptr, *d_offset = nullptr, *d_stat_part = nullptr;
    long long *d_edge_off = nullptr;
    WLow *d_wlow = nullptr;
    const size_t NQ = (size_t)nq;
    Pieces pc;
    pc.add(&d_qkey, NQ), pc.add(&d_qkey_s, NQ), pc.add(&d_qkey_t, NQ), pc.add(&d_qperm, NQ), pc.add(&d_qperm_t, NQ);
    pc.add(&d_temp, radix::scratch_bytes(nq)), pc.add(&d_count, NQ), pc.add(&d_stat, 3 * NQ), pc.add(&d_stat_part, 3 * (size_t)kStatBlocks);
    pc.add(&d_tile, (size_t)scan64::tiles(nq) + 1), pc.add(&d_offset, NQ), pc.add(&d_edge_off, (size_t)B + 1), pc.add(&d_wlow, (size_t)B);
    if (fill && d_nbr == nullptr) pc.add(&d_nbr, (size_t)T);                   // the emit pass reads the rows
    if (tmp.carve(pc)) return 1;
    AMP_HIP(hipMemcpyAsync(d_wlow, wlow.data(), sizeof(WLow) * (size_t)B, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(knnb_query_key_kernel, dim3(qit.item_blocks), dim3(64 * kItemWaves), 0, st, qit.W, (const int32_t *)qit.d_items,
                       (int)dim, queries_dev, (const Grid *)cg.d_grids, (const uint32_t *)cg.d_cell_base, d_qkey);
    AMP_LAUNCH_CHECK();
    // a cloud without sources puts its queries at its (empty) key range's start, which may be n_cells itself
    if (int rc = radix::sort_pairs<uint32_t>((const uint32_t *)d_qkey, nullptr, nq, bits_for(cg.n_cells), d_qkey_s, d_qperm, d_qkey_t,
                                             d_qperm_t, d_temp, st))
        return rc;
    launch_knnb_search(dim, nq, st, B, d_qoff, d_soff, (const Grid *)cg.d_grids, (const WLow *)d_wlow, (const uint32_t *)cg.d_cell_base,
                       (int)k, r2, queries_dev, (const int32_t *)d_qperm, (const float *)cg.d_sorted, (const int32_t *)cg.d_perm,
                       (const int32_t *)cg.d_cell_start, d_nbr, sqdist_dev, d_count, d_stat);
    const int stat_blocks = (int)std::min<int64_t>(kStatBlocks, blocks(nq));
    hipLaunchKernelGGL(knn_stat_kernel, dim3(stat_blocks), dim3(256), 0, st, nq, (const uint32_t *)d_stat, d_stat_part);
    const unsigned long long *d_total = scan64::exclusive(nq, (const uint32_t *)d_count, d_tile, d_offset, st);
    hipLaunchKernelGGL(bip_rowptr_kernel, dim3(blocks((int64_t)std::max(nq, B) + 1)), dim3(256), 0, st, nq, B, d_qoff,
                       (const unsigned long long *)d_offset, d_total, rowptr_dev, d_edge_off);
    AMP_LAUNCH_CHECK();
    unsigned long long total = 0, stat_part[3 * kStatBlocks];
    AMP_HIP(hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipMemcpyAsync(stat_part, d_stat_part, sizeof(unsigned long long) * 3 * (size_t)stat_blocks, hipMemcpyDeviceToHost, st));
    if (edge_offsets_out)
        AMP_HIP(hipMemcpyAsync(edge_offsets_out, d_edge_off, sizeof(int64_t) * ((size_t)B + 1), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    knn_stats_fold(nq, stat_blocks, stat_part);
    *n_pairs_out = (int64_t)total;                           // at most n_queries * k < 2^31
    if (!fill) return 0;
    AMP_REQUIRE(capacity >= (int64_t)total, "%s: the output buffers hold %lld pairs, the graph has %lld", who, (long long)capacity,
                (long long)total);
    if (total == 0) return 0;
    hipLaunchKernelGGL(knnb_emit_kernel, dim3((unsigned)(((int64_t)nq + kQueryWaves - 1) / kQueryWaves)), dim3(64 * kQueryWaves), 0, st, nq,
                       (int)k, (int)dim, (const int32_t *)d_nbr, (const uint32_t *)d_count, (const unsigned long long *)d_offset, queries_dev,
                       sources_dev, pairs_dev, coords_dev);
    AMP_LAUNCH_CHECK();
    AMP_HIP(hipStreamSynchronize(st));   // scratch dies with this scope
    return 0;
}

} // namespace amp

extern "C" int athena_mp_knn_pairs_bipartite(int32_t n_clouds, int32_t n_queries, const int32_t *query_offsets_host, int32_t n_sources,
                                             const int32_t *source_offsets_host, int32_t dim, const float *queries_dev,
                                             const float *sources_dev, int32_t k, float radius, int32_t *nbr_dev, float *sqdist_dev,
                                             int32_t *pairs_dev, float *coords_dev, int64_t capacity, int32_t *rowptr_dev,
                                             int64_t *edge_offsets_host, int64_t *n_pairs_out)
{
    return amp::knn_pairs_bipartite_core("knn_pairs_bipartite", n_clouds, n_queries, query_offsets_host, n_sources, source_offsets_host, dim,
                                         queries_dev, sources_dev, k, radius, nbr_dev, sqdist_dev, pairs_dev, coords_dev, capacity, rowptr_dev,
                                         edge_offsets_host, n_pairs_out);
}

// Fortran arrays in, Fortran arrays out: one search into buffers of n_queries * k pairs, narrowed afterwards; the directed CSR by
// bipartite_csr_from_pairs of bipartite_graph.hip.
extern "C" int athena_mp_knn_graph_bipartite_host(int32_t n_clouds, int32_t n_queries, const int32_t *query_offsets_host, int32_t n_sources,
                                                  const int32_t *source_offsets_host, int32_t dim, const float *queries_host,
                                                  const float *sources_host, int32_t k, float radius, int32_t *adj_ia_out,
                                                  int32_t *adj_ja_out, int64_t capacity, float *coords_out, int64_t coords_capacity,
                                                  int32_t *nbr_out, float *sqdist_out, int64_t *edge_offsets_out, int64_t *n_pairs_out)
{
    const char *who = "knn_graph_bipartite_host";
    AMP_REQUIRE(n_pairs_out != nullptr, "%s: null n_pairs_out", who);
    *n_pairs_out = 0;
    // before the points are uploaded: dim and the counts size the copies, n_queries * k the buffers
    if (int rc = knn_bipartite_arguments_check(who, n_clouds, n_queries, query_offsets_host, n_sources, source_offsets_host, dim, k, radius))
        return rc;
    AMP_REQUIRE((n_queries == 0 || queries_host != nullptr) && (n_sources == 0 || sources_host != nullptr), "%s: null points", who);
    hipStream_t st = amp::stream();
    amp::Scratch tmp;
    float *d_q = nullptr, *d_s = nullptr;
    if (tmp.upload(&d_q, queries_host, (size_t)n_queries * dim, st) || tmp.upload(&d_s, sources_host, (size_t)n_sources * dim, st)) return 1;
    int64_t E = 0;
    if (adj_ja_out == nullptr) {                                  // size query
        if (int rc = amp::knn_pairs_bipartite_core(who, n_clouds, n_queries, query_offsets_host, n_sources, source_offsets_host, dim, d_q, d_s,
                                                   k, radius, nullptr, nullptr, nullptr, nullptr, 0, nullptr, edge_offsets_out, &E))
            return rc;
        *n_pairs_out = E;
        return 0;
    }
    const int64_t T = (int64_t)n_queries * k;                     // always enough
    int32_t *d_pairs = nullptr, *d_nbr = nullptr;
    float *d_coords = nullptr, *d_sqdist = nullptr;
    if (tmp.get(&d_pairs, 2 * (size_t)T) || tmp.get(&d_coords, (size_t)T * dim) || (nbr_out && tmp.get(&d_nbr, (size_t)T)) ||
        (sqdist_out && tmp.get(&d_sqdist, (size_t)T)))
        return 1;
    if (int rc = amp::knn_pairs_bipartite_core(who, n_clouds, n_queries, query_offsets_host, n_sources, source_offsets_host, dim, d_q, d_s, k,
                                               radius, d_nbr, d_sqdist, d_pairs, d_coords, T, nullptr, edge_offsets_out, &E))
        return rc;
    *n_pairs_out = E;
    AMP_REQUIRE(adj_ia_out != nullptr && (coords_out != nullptr || E == 0), "%s: null output array", who);
    AMP_REQUIRE(capacity >= E, "%s: adj_ja buffer holds %lld entries, the graph has %lld", who, (long long)capacity, (long long)E);
    AMP_REQUIRE(coords_capacity >= E, "%s: coords buffer holds %lld pairs, the graph has %lld", who, (long long)coords_capacity, (long long)E);
    if (tmp.download(coords_out, d_coords, (size_t)E * dim, st) || tmp.download(nbr_out, d_nbr, (size_t)T, st) ||
        tmp.download(sqdist_out, d_sqdist, (size_t)T, st))
        return 1;
    int32_t *ja_dev = nullptr;
    std::vector<int32_t> row_deg, col_deg;
    const int rc = amp::bipartite_csr_from_pairs(who, n_queries, n_sources, E, d_pairs, adj_ia_out, adj_ja_out, capacity, &ja_dev, &row_deg,
                                                 &col_deg);
    if (ja_dev) (void)hipFree(ja_dev);
    if (rc) return rc;
    AMP_HIP(hipStreamSynchronize(st));
    return 0;
}
