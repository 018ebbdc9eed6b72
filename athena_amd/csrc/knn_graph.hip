// Points -> k-nearest-neighbour graph on the device, one cloud or a batch: the neighbour cap beside the radius graphs of
// radius_graph.hip, for clouds whose density varies by orders of magnitude (adaptive meshes, boundary layers).  The result is a
// pair list with edge ids like theirs, so everything downstream takes it as it is.
//
// The definition (include/athena_mp.h; every implementation gives the same arrays, tests compare with np.array_equal):
//   * s(i, j) is the squared distance of athena_mp_radius_pairs: d = p_i - p_j per component, s = ((d0*d0) + d1*d1) + d2*d2, every
//     operation rounded to fp32 on its own (-ffp-contract=off).  Symmetric bit for bit.
//   * the candidates of i -- the other points of its cloud, with a finite radius only those with s <= fl(radius * radius) -- are
//     ordered by the key (s, j); N_k(i) is the first min(k, candidates) of them.
//   * i < j is an edge iff j in N_k(i) or i in N_k(j) (union), or both (mutual); pairs in lexicographic order of the global (i, j).
// The key is one 64-bit integer: s is not negative (and never NaN for finite points: an overflow gives +inf, which orders last),
// so its bit pattern orders as an unsigned integer; it sits above j.
//
// How.  GRID: per cloud a bounding box and a uniform grid, cell keys in disjoint ranges per cloud, one stable radix sort of
// (cell, point), positions in cell order -- build_cell_grid of cell_grid.h, as in radius_graph.hip.  The cell width is free here:
// about kGridPoints points per cell, at most 2 m cells per cloud and kMaxCellsAxis per axis; an axis of zero extent is one cell.
// SEARCH: one 64-lane wave per query point, in cell order.  The wave holds its best keys ascending across its lanes (one key per
// lane; the first k count) and walks the cells around the point's own in shells of growing Chebyshev distance rho, 64 candidates
// per step.  A ballot against the k-th key skips a step that cannot improve the list; otherwise the step's keys are sorted across
// the lanes (bitonic, __shfl_xor) and merged into the list (min against the reversed step, then a bitonic merge).  No LDS, no
// atomics, no scratch.  SYMMETRISE: the n k entries of nbr become keys min * n + max (padding: n * n), one radix sort, the first
// key of a run is flagged for union and the second for mutual (a pair occurs at most twice), an exclusive scan of the flags
// (scan64.h) numbers the pairs, one pass emits pairs and coords; edge_offsets[b] = the scan at the first key >= offsets[b] * n.
//
// THE RESULT IS DEFINED BY THE KEY ORDER ALONE; the grid decides only how much is examined.  The stop rule and its proof:
//
// Cells.  On an axis with nc > 1 cells the cell of p is c = min(floor(q), nc - 1), q = fl(fl(p - lo) * inv_w) (cell_q: the same
// function gives the sort key and the search its q).  Let x = (p - lo) * inv_w in exact arithmetic with the fp32 inv_w.  Each of
// the two roundings is within 2^-24 relative (p - lo is a difference, never subnormal-inexact; lo <= p, so q >= 0; a product
// that underflows is off by 2^-150 at most), so |q - x| <= (2^-23 + 2^-48) x.  make_knn_grid keeps inv_w a normal number with
// inv_w <= (nc / extent)(1 + 2^-24), so x <= nc (1 + 2^-23) < 2049 and |q - x| < e := 2049 * (2^-23 + 2^-48) < 2^-11.9.
//
// After shell rho, every cell within Chebyshev distance rho of the query's cell c is read.  A point j of an unread cell differs
// from c by more than rho on some axis a WITH nc > 1 (an axis of one cell has no other cell: it is never "beyond").  On that axis
//   above (exists iff c + rho + 1 <= nc - 1):  c_j >= c + rho + 1, and floor(q_j) >= c_j whether or not j sits in the clamped
//     last cell, so q_j >= c + rho + 1.  c < nc - 1 is not clamped.  x_j - x_i > (c + rho + 1 - q_i) - 2 e.
//   below (exists iff c - rho - 1 >= 0):  c_j <= c - rho - 1 < nc - 1 is not clamped, so q_j < c_j + 1 <= c - rho, and
//     q_i >= floor(q_i) >= c (clamped or not).  x_i - x_j > (q_i - (c - rho)) - 2 e.
// The kernel forms u = fl(fl(gap) - kMargin) in fp32 with gap one of the two brackets.  Both results are below 2050, where half
// an ulp is at most 2^-13: the two roundings add at most 2^-12 in absolute terms.  2 e + 2^-12 < 2^-10.9 + 2^-12 < 2^-10 =: kMargin,
// the margin -- derived, not tuned -- so u <= gap - 2 e whatever the roundings did.  Hence, in exact arithmetic,
//   |p_i[a] - p_j[a]| > u_exact / inv_w[a] >= u * w_low[a],   w_low[a] = 1 / inv_w[a] rounded DOWN to fp32 (on the host, in double).
// t = the smallest fl(u * w_low[a]) over the axes and sides that exist; if none exists the shells have covered the cloud's grid.
//
// Roundings of s.  With D = |p_i[a] - p_j[a]| exact: d = fl(p_i - p_j) >= D (1 - 2^-24), d*d and the at most two additions of
// non-negative terms each lose at most 2^-24 relative and are monotone, so s(i, j) >= D^2 (1 - 2^-24)^5 > D^2 (1 - 2^-21.6).
// bound = fl(fl(t * t) * kShrink), kShrink = 1 - 2^-20.  t <= u w_low (1 + 2^-24), so bound <= (u w_low)^2 (1 + 2^-24)^4 (1 - 2^-20)
// < (u w_low)^2 (1 - 2^-20.5) < D^2 (1 - 2^-21.6) <= s(i, j).  Underflow: a bound below 2^-100 is replaced by 0 (never stops
// early), so D^2 > 2^-100 wherever the bound is used and no product above is subnormal.  Overflow: the bound is capped at FLT_MAX,
// which only weakens it.  t <= 0 gives bound 0.
//
// So after shell rho every point of an unread cell has s >= bound, and the search stops when
//   (1) the list is full and its k-th s is STRICTLY below bound: every unread key (s, j) is above the k-th key whatever j is; or
//   (2) there is a cap and bound > fl(radius * radius): every unread point fails the cap; or
//   (3) no axis has an unread side: the shells have covered the cloud's grid.
// (3) holds at the latest at rho = the largest nc - 1, so the search ends.  What was read was merged by key, so the list is N_k(i).
//
// Worst case: with no cap and clusters far apart that hold fewer than k + 1 points each, a query must cross the gap: it visits
// every cell of its cloud, most of them empty.  Correct and slow; the cap is the remedy.
#include <float.h>
#include <math.h>

#include <algorithm>

#include "cell_grid.h"
#include "common.h"
#include "knn_cells.h"
#include "radix_sort.h"
#include "scan64.h"

namespace {

// One wave per slot of the cell order: the point i = perm[slot] against the cells of its cloud, shell by shell (header).
// nbr[i, 0..k-1] = N_k(i) as 1-based global ids in key order, padded with 0.  stat[0][slot] = candidates read, stat[1][slot] =
// cells read, stat[2][slot] = the last shell.
template <int DIM>
__global__ __launch_bounds__(64 * kQueryWaves) void knn_search_kernel(int32_t n, int32_t B, const int32_t *__restrict__ offsets,
                                                                      const Grid *__restrict__ grids, const WLow *__restrict__ wlow,
                                                                      const uint32_t *__restrict__ cell_base, int k, float r2,
                                                                      const float *__restrict__ sorted, const int32_t *__restrict__ perm,
                                                                      const int32_t *__restrict__ cell_start, int32_t *__restrict__ nbr,
                                                                      uint32_t *__restrict__ stat)
{
    const int lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * kQueryWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (slot >= n) return;                                   // the whole wave
    const int32_t i = __builtin_amdgcn_readfirstlane(perm[slot]);
    const int32_t b = __builtin_amdgcn_readfirstlane(cloud_of(B, offsets, i));
    const Grid g = grids[b];
    const WLow wl = wlow[b];
    const uint32_t cb = cell_base[b];
    float p[3] = {0.f, 0.f, 0.f}, q[3] = {0.f, 0.f, 0.f};
    int32_t cc[3] = {0, 0, 0}, nc[3] = {1, 1, 1};
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        p[a] = sorted[slot * DIM + a];
        nc[a] = __builtin_amdgcn_readfirstlane(g.nc[a]);
        q[a] = cell_q(p[a], g.lo[a], g.inv_w[a]);
        cc[a] = __builtin_amdgcn_readfirstlane(cell_coord(p[a], g.lo[a], g.inv_w[a], nc[a]));
    }
    const bool capped = r2 < INFINITY;

    unsigned long long list = kNoKey;
    uint32_t n_cand = 0, n_cells = 0;
    int rho = 0;

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
                const float s = sq_dist<DIM>(p, pj);         // p_i - p_j; symmetric bit for bit
                if (j != i && s <= r2) key = ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(uint32_t)j;
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
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            if (nc[a] <= 1) continue;
            if (cc[a] + rho + 1 <= nc[a] - 1) t = fminf(t, (((float)(cc[a] + rho + 1) - q[a]) - kMargin) * wl.w[a]);
            if (cc[a] - rho - 1 >= 0) t = fminf(t, ((q[a] - (float)(cc[a] - rho)) - kMargin) * wl.w[a]);
        }
        if (t == INFINITY) break;                            // (3) the shells have covered the cloud's grid
        float bound = t > 0.f ? fminf((t * t) * kShrink, FLT_MAX) : 0.f;
        if (bound < 0x1p-100f) bound = 0.f;
        if (capped && bound > r2) break;                     // (2)
        const uint32_t kth_s = (uint32_t)(__shfl(list, k - 1, 64) >> 32);   // 0xffffffff while the list is short
        if (kth_s < __float_as_uint(bound)) break;           // (1) strictly below
    }

    if (lane < k) nbr[(int64_t)i * k + lane] = list != kNoKey ? (int32_t)(uint32_t)list + 1 : 0;
    if (lane == 0) {
        stat[slot] = n_cand;
        stat[(int64_t)n + slot] = n_cells;
        stat[2 * (int64_t)n + slot] = (uint32_t)rho;
    }
}

// ---- symmetrise ---------------------------------------------------------------------------------------------------------------
// entry e = (i, t) of nbr -> min * n + max, padding -> n * n (above every pair)
__global__ __launch_bounds__(256) void knn_pair_key_kernel(int64_t T, int32_t n, int k, const int32_t *__restrict__ nbr,
                                                           unsigned long long *__restrict__ key)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= T) return;
    const unsigned long long i = (unsigned long long)(e / k), N = (unsigned long long)n;
    const int32_t v = nbr[e];
    const unsigned long long j = (unsigned long long)(v - 1);
    key[e] = v <= 0 ? N * N : (i < j ? i * N + j : j * N + i);
}

// union: the first key of a run; mutual: the second (i -> j and j -> i: a pair occurs at most twice)
__global__ __launch_bounds__(256) void knn_flag_kernel(int64_t T, unsigned long long pad, int mode, const unsigned long long *__restrict__ key,
                                                       uint8_t *__restrict__ flag)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= T) return;
    const unsigned long long v = key[e];
    const bool repeat = e > 0 && key[e - 1] == v;
    flag[e] = v != pad && (mode == 0 ? !repeat : repeat);
}

__global__ __launch_bounds__(256) void knn_emit_kernel(int64_t T, int32_t n, int dim, const unsigned long long *__restrict__ key,
                                                       const uint8_t *__restrict__ flag, const unsigned long long *__restrict__ offset,
                                                       const float *__restrict__ pts, int32_t *__restrict__ pairs,
                                                       float *__restrict__ coords)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= T || !flag[e]) return;
    const unsigned long long v = key[e];
    const int64_t at = (int64_t)offset[e];
    const int64_t i = (int64_t)(v / (unsigned long long)n), j = (int64_t)(v % (unsigned long long)n);
    if (pairs) {
        pairs[2 * at] = (int32_t)i + 1;
        pairs[2 * at + 1] = (int32_t)j + 1;
    }
    if (coords)
        for (int a = 0; a < dim; ++a) coords[at * dim + a] = pts[i * dim + a] - pts[j * dim + a];
}

// edge_offsets[b] = pairs whose i is below offsets[b]: the scan at the first key >= offsets[b] * n (b = 0 .. B)
__global__ __launch_bounds__(256) void knn_edge_offsets_kernel(int32_t B, int32_t n, int64_t T, const int32_t *__restrict__ offsets,
                                                               const unsigned long long *__restrict__ key,
                                                               const unsigned long long *__restrict__ offset,
                                                               const unsigned long long *__restrict__ total,
                                                               long long *__restrict__ edge_offsets)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b > B) return;
    const unsigned long long want = (unsigned long long)offsets[b] * (unsigned long long)n;
    int64_t lo = 0, hi = T;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < want) lo = mid + 1; else hi = mid;
    }
    edge_offsets[b] = (long long)(lo < T ? offset[lo] : *total);
}

using amp::Scratch;

template <typename... A> void launch_search(int dim, int32_t n, hipStream_t st, A... a)
{
    const dim3 grid((unsigned)(((int64_t)n + kQueryWaves - 1) / kQueryWaves)), block(64 * kQueryWaves);
    if (dim == 1) hipLaunchKernelGGL(knn_search_kernel<1>, grid, block, 0, st, n, a...);
    else if (dim == 2) hipLaunchKernelGGL(knn_search_kernel<2>, grid, block, 0, st, n, a...);
    else hipLaunchKernelGGL(knn_search_kernel<3>, grid, block, 0, st, n, a...);
}


int knn_arguments_check(const char *who, int32_t B, const int32_t *offsets, int32_t dim, int32_t k, float radius, int32_t mode)
{
    AMP_REQUIRE(dim >= 1 && dim <= 3, "%s: dim = %d outside [1,3]", who, dim);
    AMP_REQUIRE(k >= 1 && k <= 64, "%s: k = %d outside [1,64]", who, k);
    AMP_REQUIRE(radius > 0.f, "%s: radius = %g is not a positive number (+infinity: no cap)", who, (double)radius);   // NaN fails too
    AMP_REQUIRE(mode == 0 || mode == 1, "%s: mode = %d is neither 0 (union) nor 1 (mutual)", who, mode);
    return batch_offsets_check(who, B, offsets);
}

} // namespace

namespace amp {

int64_t g_knn_stats[4] = {0, 0, 0, 0};       // athena_mp_knn_stats: of the last call, of either builder

// nbr_dev, pairs_dev and coords_dev all null: size query (edge_offsets_out is filled either way).  Everything on the library's
// stream; synchronised on return.
int knn_pairs_batched_core(int32_t B, int32_t n, const int32_t *offsets, int32_t dim, const float *points_dev, int32_t k, float radius,
                           int32_t mode, int32_t *nbr_dev, int32_t *pairs_dev, float *coords_dev, int64_t capacity,
                           int64_t *edge_offsets_out, int64_t *n_pairs_out)
{
    static const char who[] = "knn_pairs_batched";
    AMP_REQUIRE(n_pairs_out != nullptr, "knn_pairs_batched: null n_pairs_out");
    *n_pairs_out = 0;
    std::fill(g_knn_stats, g_knn_stats + 4, (int64_t)0);
    if (int rc = knn_arguments_check(who, B, offsets, dim, k, radius, mode)) return rc;
    AMP_REQUIRE(offsets[B] == n, "knn_pairs_batched: offsets end at %d, the batch has %d points", offsets[B], n);
    AMP_REQUIRE(n == 0 || points_dev != nullptr, "knn_pairs_batched: null points");
    AMP_REQUIRE((int64_t)n * k < ((int64_t)1 << 31), "knn_pairs_batched: n * k = %lld: more than 2^31 neighbour entries", (long long)n * k);
    if (edge_offsets_out) std::fill(edge_offsets_out, edge_offsets_out + B + 1, (int64_t)0);
    if (n == 0) return 0;
    const float r2 = radius * radius;            // +inf (no cap, or a square beyond fp32): every s passes
    hipStream_t st = stream();
    const bool fill = pairs_dev != nullptr || coords_dev != nullptr;

    Scratch tmp;
    CellGrid cg;
    std::vector<WLow> wlow((size_t)B);           // an empty cloud keeps zeros
    if (int rc = build_cell_grid(who, true, B, n, offsets, dim, points_dev, st, tmp,
                                 [&](const Box &box, int32_t m, int32_t b) { return make_knn_grid(box, dim, m, &wlow[b]); }, cg))
        return rc;
    const BatchItems &it = cg.it;
    const int64_t T = (int64_t)n * k;

    // the search's arrays, and those of the symmetrisation: one sort of the n k keys, flags, a 64-bit scan in key order
    WLow *d_wlow = nullptr;
    uint32_t *d_stat = nullptr;
    int32_t *d_nbr = nbr_dev, *d_v = nullptr, *d_v_t = nullptr;
    unsigned long long *d_stat_part = nullptr, *d_pk = nullptr, *d_pk_s = nullptr, *d_pk_t = nullptr, *d_tile = nullptr, *d_offset = nullptr;
    uint8_t *d_flag = nullptr;
    long long *d_edge_off = nullptr;
    char *d_temp2 = nullptr;
    const size_t TT = (size_t)T;
    Pieces pc;
    pc.add(&d_wlow, (size_t)B), pc.add(&d_stat, 3 * (size_t)n), pc.add(&d_stat_part, 3 * (size_t)kStatBlocks);
    if (nbr_dev == nullptr) pc.add(&d_nbr, TT);
    pc.add(&d_pk, TT), pc.add(&d_pk_s, TT), pc.add(&d_pk_t, TT), pc.add(&d_v, TT), pc.add(&d_v_t, TT), pc.add(&d_flag, TT);
    pc.add(&d_tile, (size_t)scan64::tiles(T) + 1), pc.add(&d_offset, TT), pc.add(&d_edge_off, (size_t)B + 1);
    pc.add(&d_temp2, radix::scratch_bytes(T));
    if (tmp.carve(pc)) return 1;
    AMP_HIP(hipMemcpyAsync(d_wlow, wlow.data(), sizeof(WLow) * (size_t)B, hipMemcpyHostToDevice, st));
    launch_search(dim, n, st, B, (const int32_t *)it.d_off, (const Grid *)cg.d_grids, (const WLow *)d_wlow,
                  (const uint32_t *)cg.d_cell_base, (int)k, r2, (const float *)cg.d_sorted, (const int32_t *)cg.d_perm,
                  (const int32_t *)cg.d_cell_start, d_nbr, d_stat);
    const int stat_blocks = (int)std::min<int64_t>(kStatBlocks, blocks(n));
    hipLaunchKernelGGL(knn_stat_kernel, dim3(stat_blocks), dim3(256), 0, st, n, (const uint32_t *)d_stat, d_stat_part);
    AMP_LAUNCH_CHECK();

    const unsigned long long pad = (unsigned long long)n * (unsigned long long)n;
    hipLaunchKernelGGL(knn_pair_key_kernel, dim3(blocks(T)), dim3(256), 0, st, T, n, (int)k, (const int32_t *)d_nbr, d_pk);
    AMP_LAUNCH_CHECK();
    if (int rc = radix::sort_pairs<unsigned long long>((const unsigned long long *)d_pk, nullptr, T, bits_for(pad), d_pk_s, d_v, d_pk_t, d_v_t,
                                                       d_temp2, st))
        return rc;
    hipLaunchKernelGGL(knn_flag_kernel, dim3(blocks(T)), dim3(256), 0, st, T, pad, (int)mode, (const unsigned long long *)d_pk_s, d_flag);
    const unsigned long long *d_total = scan64::exclusive(T, (const uint8_t *)d_flag, d_tile, d_offset, st);
    hipLaunchKernelGGL(knn_edge_offsets_kernel, dim3(blocks((int64_t)B + 1)), dim3(256), 0, st, B, n, T, (const int32_t *)it.d_off,
                       (const unsigned long long *)d_pk_s, (const unsigned long long *)d_offset, d_total, d_edge_off);
    AMP_LAUNCH_CHECK();
    unsigned long long total = 0, stat_part[3 * kStatBlocks];
    AMP_HIP(hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipMemcpyAsync(stat_part, d_stat_part, sizeof(unsigned long long) * 3 * (size_t)stat_blocks, hipMemcpyDeviceToHost, st));
    if (edge_offsets_out)
        AMP_HIP(hipMemcpyAsync(edge_offsets_out, d_edge_off, sizeof(int64_t) * ((size_t)B + 1), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    knn_stats_fold(n, stat_blocks, stat_part);
    *n_pairs_out = (int64_t)total;
    if (!fill) return 0;
    AMP_REQUIRE(capacity >= (int64_t)total, "knn_pairs_batched: the output buffers hold %lld pairs, the graph has %lld", (long long)capacity,
                (long long)total);
    if (total == 0) return 0;
    hipLaunchKernelGGL(knn_emit_kernel, dim3(blocks(T)), dim3(256), 0, st, T, n, (int)dim, (const unsigned long long *)d_pk_s,
                       (const uint8_t *)d_flag, (const unsigned long long *)d_offset, points_dev, pairs_dev, coords_dev);
    AMP_LAUNCH_CHECK();
    AMP_HIP(hipStreamSynchronize(st));   // scratch dies with this scope
    return 0;
}

} // namespace amp

extern "C" int athena_mp_knn_pairs_batched(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim, const float *points_dev,
                                           int32_t k, float radius, int32_t mode, int32_t *nbr_dev, int32_t *pairs_dev, float *coords_dev,
                                           int64_t capacity, int64_t *edge_offsets_host, int64_t *n_pairs_out)
{
    return amp::knn_pairs_batched_core(n_clouds, n, offsets_host, dim, points_dev, k, radius, mode, nbr_dev, pairs_dev, coords_dev,
                                       capacity, edge_offsets_host, n_pairs_out);
}

extern "C" int athena_mp_knn_pairs(int32_t n, int32_t dim, const float *points_dev, int32_t k, float radius, int32_t mode,
                                   int32_t *nbr_dev, int32_t *pairs_dev, float *coords_dev, int64_t capacity, int64_t *n_pairs_out)
{
    AMP_REQUIRE(n >= 0, "knn_pairs: n = %d is negative", n);
    const int32_t offsets[2] = {0, n};
    return amp::knn_pairs_batched_core(1, n, offsets, dim, points_dev, k, radius, mode, nbr_dev, pairs_dev, coords_dev, capacity, nullptr,
                                       n_pairs_out);
}

extern "C" int athena_mp_knn_stats(int64_t out[4])
{
    AMP_REQUIRE(out != nullptr, "knn_stats: null output");
    std::copy(amp::g_knn_stats, amp::g_knn_stats + 4, out);
    return 0;
}

extern "C" int athena_mp_knn_graph_batched_host(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim,
                                                const float *points_host, int32_t k, float radius, int32_t mode, int32_t add_self_loops,
                                                int32_t *adj_ia_out, int32_t *adj_ja_out, int64_t capacity, int64_t *nnz_out,
                                                float *coords_out, int64_t coords_capacity, int64_t *n_pairs_out,
                                                int64_t *edge_offsets_out)
{
    AMP_REQUIRE(nnz_out != nullptr && n_pairs_out != nullptr, "knn_graph_batched_host: null output pointer");
    *nnz_out = *n_pairs_out = 0;
    AMP_REQUIRE(n >= 0 && (n == 0 || points_host != nullptr), "knn_graph_batched_host: bad arguments (n = %d)", n);
    // before the points are uploaded: dim sizes the copy, n * k the buffers
    if (int rc = knn_arguments_check("knn_graph_batched_host", n_clouds, offsets_host, dim, k, radius, mode)) return rc;
    AMP_REQUIRE((int64_t)n * k < ((int64_t)1 << 31), "knn_graph_batched_host: n * k = %lld: more than 2^31 neighbour entries",
                (long long)n * k);
    hipStream_t st = amp::stream();
    Scratch tmp;
    float *d_pts = nullptr, *d_coords = nullptr;
    int32_t *d_pairs = nullptr;
    const int64_t T = (int64_t)n * k;            // always enough: one search, narrowed afterwards
    if (tmp.upload(&d_pts, points_host, (size_t)n * dim, st) || tmp.get(&d_pairs, 2 * (size_t)T) || tmp.get(&d_coords, (size_t)T * dim)) return 1;
    int64_t E = 0;
    if (int rc = amp::knn_pairs_batched_core(n_clouds, n, offsets_host, dim, d_pts, k, radius, mode, nullptr, d_pairs, d_coords, T,
                                             edge_offsets_out, &E))
        return rc;
    return amp::graph_host_tail("knn_graph_batched_host", n, dim, E, add_self_loops, adj_ia_out, adj_ja_out, capacity, nnz_out, coords_out,
                           coords_capacity, n_pairs_out, st, [&](int32_t **pairs, float **coords) {      // already there
                               *pairs = d_pairs;
                               *coords = d_coords;
                               return 0;
                           });
}
