// Bond-angle triplets of a neighbour graph on the device, with gradients: for every vertex the ordered pairs of its entries (bonds)
// and the cosine of the angle between them -- the three-body terms of DimeNet, M3GNet and ALIGNN -- as a pair list over the CSR
// ENTRIES of a handle (its line graph), which athena_mp_graph_create_bipartite_dev turns into a handle of its own; and the way back
// from a gradient per triplet to the builders' vec.
//
// The definition (include/athena_mp.h holds the same text; tests/triplets_reference.py is its numpy transcription).  All integer
// results are exact; all arithmetic is fp32, every operation rounded on its own (-ffp-contract=off, correctly rounded / and sqrt).
// g is a square handle with edge columns; entry k is a 0-based position of its forward CSR (rowptr, col, eid), i its row, c = col[k],
// e = eid[k].
//
//   entry vectors:  dir[k] = -vec[e] when i <= c, +vec[e] when i > c, +0 when e < 0: from vertex i to the neighbour of entry k.
//                   Reverse: dvec[e] = acc, acc = +0, then over the entries of edge column e in the order of the edge index (e_rowptr,
//                   e_col): acc = acc - ddir[k] when i <= c, acc = acc + ddir[k] when i > c.
//   participants:   cutoff3 = +inf: every entry with e >= 0.  Else e >= 0 and r < cutoff3, s = ((x0 x0) + x1 x1) + x2 x2 over
//                   x = vec[e], r = sqrt(s).
//   triplets:       every ordered pair (k, k') of distinct participants of one row, numbered in lexicographic order of (k, k'); pairs
//                   [2, T] 1-based, rowptr [nnz + 1] 0-based.  A row of m participants owns one run of m (m - 1) triplets.
//   angle:          a = dir[k], b = dir[k']: sa = ((a0 a0) + a1 a1) + a2 a2, sb alike, dot = ((a0 b0) + a1 b1) + a2 b2 (the first dim
//                   terms), den = sqrt(sa) sqrt(sb), cos[t] = dot / den; den == 0: cos[t] = +0 and ga = gb = +0.  No clamp.
//   its reverse:    ga_c = b_c / den - (cos[t] a_c) / sa, gb_c = a_c / den - (cos[t] b_c) / sb.  ddir[k] = acc, acc = +0; over row k of
//                   the triplet handle in CSR order acc = acc + dcos[t] ga; then over its column k in transposed-CSR order (rows
//                   ascending) acc = acc + dcos[t] gb.
//
// How.  trip_count_kernel: sixteen lanes share a vertex row (row_groups.h); a ballot per round gives every participant its place, and
// the entry ids go, compacted and in CSR order, to the head of the row's slice of a scratch [nnz].  Two scans (scan64.h) follow: of the
// runs m (m - 1) in 64 bits, which is where a count past 2^31 is found before anything of that size exists, and of the work items, a
// run cut every kItemPairs pairs so that a hub does not serialise the launch.  trip_stats_kernel folds the two totals, the participants
// and the longest row into four words: the one host wait.  trip_fill_kernel: a wave per work item finds its row by bisection of the item
// offsets (scalar), then its lanes stride over q in the item's part of [0, m (m - 1)): a = q / (m - 1), b' = q % (m - 1), b = b' + (b'
// >= a), the two entry ids from a register by __shfl where m <= 64 and from the scratch otherwise, one 8-byte pair per lane (two 4-byte
// stores where the list does not start on an 8-byte boundary).  The bytes do not depend on the cut.  No atomics, no device scratch
// memory; LDS only in the one-block statistics.
// The entry vectors and cos_fwd stream over rows in the same lane groups; entry_vectors_bwd is a lane per edge column, cos_bwd a lane per
// entry that walks its row and then its column: the defined order, at the price that the entries of a hub take longer (as in
// grid_clusters.hip).  The partners' dir rows belong to one vertex row and stay in cache.  Rows of dim floats are never 16-byte aligned:
// every access is 4 bytes wide.
#include <math.h>

#include <algorithm>
#include <vector>

#include "cell_start.h"
#include "common.h"
#include "row_groups.h"
#include "scan64.h"

namespace {

constexpr int kG = 16;                          // lanes that share a row
constexpr uint32_t kItemPairs = 4096;           // pairs per work item of the fill: 64 rounds of a wave
constexpr int kFillWaves = 4;                   // work items per 256-thread block

int64_t g_stats[3] = {0, 0, 0};                 // triplets, participants, longest run of the last build

// the participants of every row: their entry ids compacted to part[rowptr[i] ..], their number m[i], the run m (m - 1) and its work
// items; rank[k] (may be null) = the participants of the row before entry k
__global__ __launch_bounds__(256) void trip_count_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ eid,
                                                         int32_t dim, const float *__restrict__ vec, float cutoff3, int all,
                                                         int32_t *__restrict__ part, int32_t *__restrict__ rank, int32_t *__restrict__ m_out,
                                                         unsigned long long *__restrict__ run_out, uint32_t *__restrict__ items_out)
{
    const amp::RowGroup<kG> rg(n, rowptr);
    int32_t m = 0;
    for (int32_t k0 = 0; k0 < rg.rounds; k0 += kG) {
        const bool mine = k0 + rg.sub < rg.len;
        const int64_t k = (int64_t)rg.beg + k0 + rg.sub;
        bool take = false;
        if (mine) {
            const int32_t e = eid[k];
            if (e >= 0) {
                take = true;
                if (!all) {
                    const float *x = vec + (int64_t)e * dim;
                    float s = x[0] * x[0];
                    if (dim > 1) s = s + x[1] * x[1];
                    if (dim > 2) s = s + x[2] * x[2];
                    take = sqrtf(s) < cutoff3;
                }
            }
        }
        const uint32_t bits = (uint32_t)(__ballot(take) >> rg.first) & ((1u << kG) - 1u);
        const int32_t before = m + __popc(bits & ((1u << rg.sub) - 1u));
        if (take) part[(int64_t)rg.beg + before] = (int32_t)k;     // before <= the entry's own place in the row
        if (rank && mine) rank[k] = before;
        m += __popc(bits);
    }
    if (rg.row < n && rg.sub == 0) {
        const unsigned long long run = m > 0 ? (unsigned long long)m * (unsigned long long)(m - 1) : 0ull;
        const unsigned long long items = (run + kItemPairs - 1) / kItemPairs;
        m_out[rg.row] = m;
        run_out[rg.row] = run;
        items_out[rg.row] = (uint32_t)(items < 0x7fffffffull ? items : 0x7fffffffull);   // only read where the runs sum below 2^31
    }
}

// one block: out = {triplets, work items, participants, the longest row's participants}
__global__ __launch_bounds__(256) void trip_stats_kernel(int32_t n, const int32_t *__restrict__ m, const unsigned long long *__restrict__ total,
                                                         const unsigned long long *__restrict__ items, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long s_sum[4];
    __shared__ int32_t s_max[4];
    unsigned long long sum = 0;
    int32_t mx = 0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const int32_t v = m[i];
        sum += (unsigned long long)v;
        mx = max(mx, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        mx = max(mx, __shfl_xor(mx, o));
    }
    if ((threadIdx.x & 63) == 0) {
        s_sum[threadIdx.x >> 6] = sum;
        s_max[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = *total;
        out[1] = *items;
        out[2] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        out[3] = (unsigned long long)max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    }
}

// a wave per work item: the pairs q0 .. q1-1 of one row's run
__global__ __launch_bounds__(64 * kFillWaves) void trip_fill_kernel(int32_t n, uint32_t n_items, const int32_t *__restrict__ rowptr,
                                                                    const int32_t *__restrict__ part, const int32_t *__restrict__ m_arr,
                                                                    const unsigned long long *__restrict__ run_off,
                                                                    const unsigned long long *__restrict__ item_off, int wide,
                                                                    int32_t *__restrict__ pairs)
{
    const int lane = threadIdx.x & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kFillWaves + (threadIdx.x >> 6)));
    if (w >= n_items) return;
    int32_t lo = 0, hi = n;                                         // the last row whose items start at or before w
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (item_off[mid] <= (unsigned long long)w) lo = mid;
        else hi = mid;
    }
    const int32_t row = lo, beg = rowptr[row], m = m_arr[row];
    const uint32_t m1 = (uint32_t)(m - 1), run = (uint32_t)m * m1;  // m >= 2: the row has an item
    const uint32_t q0 = (w - (uint32_t)item_off[row]) * kItemPairs, q1 = min(run, q0 + kItemPairs);
    const int64_t base = (int64_t)run_off[row];
    const bool regs = m <= 64;
    int32_t mine = 0;
    if (regs && lane < m) mine = part[(int64_t)beg + lane];
    for (uint32_t qb = q0; qb < q1; qb += 64) {                     // every lane takes part in the __shfl
        const bool valid = qb + lane < q1;
        const uint32_t q = valid ? qb + lane : q0;
        const uint32_t a = q / m1, bp = q - a * m1, b = bp + (bp >= a ? 1u : 0u);
        int32_t ka, kb;
        if (regs) {
            ka = __shfl(mine, (int)a);
            kb = __shfl(mine, (int)b);
        } else {
            ka = part[(int64_t)beg + a];
            kb = part[(int64_t)beg + b];
        }
        if (valid) {
            int32_t *dst = pairs + 2 * (base + (int64_t)q);
            if (wide) {
                *reinterpret_cast<int2 *>(dst) = make_int2(ka + 1, kb + 1);
            } else {
                dst[0] = ka + 1;
                dst[1] = kb + 1;
            }
        }
    }
}

// trowptr[k] = the triplets whose first entry lies before k; trowptr[nnz] = T
__global__ __launch_bounds__(256) void trip_rowptr_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ rank,
                                                          const int32_t *__restrict__ m_arr, const unsigned long long *__restrict__ run_off,
                                                          int64_t nnz, int32_t T, int32_t *__restrict__ trowptr)
{
    const amp::RowGroup<kG> rg(n, rowptr);
    if (blockIdx.x == 0 && threadIdx.x == 0) trowptr[nnz] = T;
    if (rg.row >= n) return;
    const int32_t m1 = max(m_arr[rg.row] - 1, 0);
    const int32_t base = (int32_t)run_off[rg.row];
    for (int32_t j = rg.sub; j < rg.len; j += kG) {
        const int64_t k = (int64_t)rg.beg + j;
        trowptr[k] = base + rank[k] * m1;
    }
}

// dir[k] = -+ vec[eid[k]] by the order of row and column, +0 without an edge column
__global__ __launch_bounds__(256) void entry_vectors_fwd_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                const int32_t *__restrict__ eid, int32_t dim, const float *__restrict__ vec,
                                                                float *__restrict__ dir)
{
    const amp::RowGroup<kG> rg(n, rowptr);
    if (rg.row >= n) return;
    for (int32_t j = rg.sub; j < rg.len; j += kG) {
        const int64_t k = (int64_t)rg.beg + j;
        const int32_t c = col[k], e = eid[k];
        float *dst = dir + k * dim;
        if (e < 0) {
            for (int32_t d = 0; d < dim; ++d) dst[d] = 0.f;
        } else {
            const float *src = vec + (int64_t)e * dim;
            const bool neg = rg.row <= (int64_t)c;
            for (int32_t d = 0; d < dim; ++d) dst[d] = neg ? -src[d] : src[d];
        }
    }
}

// dvec[e] = the signed sum of ddir over the entries of edge column e, in the order of the edge index
__global__ __launch_bounds__(256) void entry_vectors_bwd_kernel(int32_t E, const int32_t *__restrict__ e_rowptr, const int32_t *__restrict__ e_row,
                                                                const int32_t *__restrict__ e_entry, const int32_t *__restrict__ col,
                                                                int32_t dim, const float *__restrict__ ddir, float *__restrict__ dvec)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int32_t p = e_rowptr[e]; p < e_rowptr[e + 1]; ++p) {
        const int32_t i = e_row[p], k = e_entry[p];
        const float *src = ddir + (int64_t)k * dim;
        const bool neg = i <= col[k];
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (d < dim) acc[d] = neg ? acc[d] - src[d] : acc[d] + src[d];
    }
#pragma unroll
    for (int d = 0; d < 3; ++d)
        if (d < dim) dvec[e * dim + d] = acc[d];
}

struct Vec3 {
    float x[3];
};

__device__ __forceinline__ Vec3 load_row(const float *__restrict__ p, int64_t r, int32_t dim)
{
    Vec3 v = {{0.f, 0.f, 0.f}};
    const float *src = p + r * dim;
    v.x[0] = src[0];
    if (dim > 1) v.x[1] = src[1];
    if (dim > 2) v.x[2] = src[2];
    return v;
}

// the first dim terms of ((u0 v0) + u1 v1) + u2 v2
__device__ __forceinline__ float dot_terms(const Vec3 &u, const Vec3 &v, int32_t dim)
{
    float s = u.x[0] * v.x[0];
    if (dim > 1) s = s + u.x[1] * v.x[1];
    if (dim > 2) s = s + u.x[2] * v.x[2];
    return s;
}

// cos[eid[p]] over the entries p of row k of the triplet handle: a = dir[k], b = dir[col[p]]
__global__ __launch_bounds__(256) void triplet_cos_fwd_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                              const int32_t *__restrict__ eid, int32_t dim, const float *__restrict__ dir,
                                                              float *__restrict__ cosv)
{
    const amp::RowGroup<kG> rg(n, rowptr);
    if (rg.row >= n || rg.len == 0) return;
    const Vec3 a = load_row(dir, rg.row, dim);
    const float ra = sqrtf(dot_terms(a, a, dim));
    for (int32_t j = rg.sub; j < rg.len; j += kG) {
        const int64_t p = (int64_t)rg.beg + j;
        const Vec3 b = load_row(dir, col[p], dim);
        const float den = ra * sqrtf(dot_terms(b, b, dim));
        const float dot = dot_terms(a, b, dim);
        cosv[eid[p]] = den == 0.f ? 0.f : dot / den;
    }
}

// acc = acc + dc (v_c / den - (cs u_c) / su): the term of dir u in the triplet (u, v) or (v, u); +0 terms where den == 0
__device__ __forceinline__ void cos_bwd_term(float (&acc)[3], const Vec3 &u, float su, const Vec3 &v, float sv, int32_t dim, float cs, float dc)
{
    const float den = sqrtf(su) * sqrtf(sv);
#pragma unroll
    for (int d = 0; d < 3; ++d) {                                   // constant indices: the three sums stay in registers
        const float g = den == 0.f ? 0.f : v.x[d] / den - (cs * u.x[d]) / su;
        if (d < dim) acc[d] = acc[d] + dc * g;
    }
}

// a lane per entry k: its row of the triplet handle, then its column
__global__ __launch_bounds__(256) void triplet_cos_bwd_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                              const int32_t *__restrict__ eid, const int32_t *__restrict__ t_rowptr,
                                                              const int32_t *__restrict__ t_src, const int32_t *__restrict__ t_eid, int32_t dim,
                                                              const float *__restrict__ dir, const float *__restrict__ cosv,
                                                              const float *__restrict__ dcos, float *__restrict__ ddir)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    float acc[3] = {0.f, 0.f, 0.f};
    const int32_t r0 = rowptr[k], r1 = rowptr[k + 1], c0 = t_rowptr[k], c1 = t_rowptr[k + 1];
    if (r1 > r0 || c1 > c0) {
        const Vec3 me = load_row(dir, k, dim);
        const float sm = dot_terms(me, me, dim);
        for (int32_t p = r0; p < r1; ++p) {
            const Vec3 b = load_row(dir, col[p], dim);
            const int32_t t = eid[p];
            cos_bwd_term(acc, me, sm, b, dot_terms(b, b, dim), dim, cosv[t], dcos[t]);
        }
        for (int32_t p = c0; p < c1; ++p) {
            const Vec3 a = load_row(dir, t_src[p], dim);
            const int32_t t = t_eid[p];
            cos_bwd_term(acc, me, sm, a, dot_terms(a, a, dim), dim, cosv[t], dcos[t]);
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d)
        if (d < dim) ddir[k * dim + d] = acc[d];
}

// what the entries on g check first: a square handle that carries edge columns, dim in 1..3
int entries_check(const char *who, const athena_mp_graph *g, int32_t dim)
{
    AMP_REQUIRE(g != nullptr, "%s: null graph handle", who);
    AMP_REQUIRE(dim >= 1 && dim <= 3, "%s: dim = %d is outside 1..3", who, dim);
    AMP_REQUIRE(g->n_rows == g->n_cols, "%s: the handle is not square (%d rows, %d columns)", who, g->n_rows, g->n_cols);
    AMP_REQUIRE(!(g->n_edge_cols == 0 && g->nnz > (int64_t)g->n_rows), "%s: the handle has no edge columns: build it with edge ids", who);
    return 0;
}

// ... and the entries on the triplet handle: square, one edge id per entry
int triplet_handle_check(const char *who, const athena_mp_graph *tg, int32_t dim)
{
    if (int rc = amp::edge_form_check(who, tg)) return rc;
    AMP_REQUIRE(dim >= 1 && dim <= 3, "%s: dim = %d is outside 1..3", who, dim);
    AMP_REQUIRE(tg->n_rows == tg->n_cols, "%s: the triplet handle is not square (%d rows, %d columns)", who, tg->n_rows, tg->n_cols);
    return 0;
}

} // namespace

extern "C" int athena_mp_triplet_pairs(const athena_mp_graph *g, int32_t dim, const float *vec_dev, float cutoff3, int32_t *pairs_dev,
                                       int64_t capacity, int32_t *rowptr_dev, int64_t *n_triplets_out)
{
    AMP_REQUIRE(n_triplets_out != nullptr, "triplet_pairs: null n_triplets_out");
    *n_triplets_out = 0;
    if (int rc = entries_check("triplet_pairs", g, dim)) return rc;
    AMP_REQUIRE(!(cutoff3 != cutoff3) && cutoff3 > 0.f, "triplet_pairs: cutoff3 = %g: need a value above 0 (+infinity: every entry)",
                (double)cutoff3);
    const int all = isinf(cutoff3) ? 1 : 0;
    AMP_REQUIRE(all || vec_dev != nullptr || g->n_edge_cols == 0, "triplet_pairs: a finite cutoff3 needs vec");
    const int32_t n = g->n_rows;
    const int64_t nnz = g->nnz;
    const bool fill = pairs_dev != nullptr || rowptr_dev != nullptr;
    hipStream_t st = amp::stream();
    if (n == 0 || nnz == 0) {
        g_stats[0] = g_stats[1] = g_stats[2] = 0;
        if (rowptr_dev) AMP_HIP(hipMemsetAsync(rowptr_dev, 0, sizeof(int32_t), st));
        return 0;
    }

    amp::Scratch tmp;
    int32_t *d_part = nullptr, *d_rank = nullptr, *d_m = nullptr;
    uint32_t *d_items = nullptr;
    unsigned long long *d_run = nullptr, *d_tile = nullptr, *d_run_off = nullptr, *d_tile2 = nullptr, *d_item_off = nullptr, *d_four = nullptr;
    const size_t tiles = (size_t)scan64::tiles(n) + 1, N = (size_t)n;
    amp::Pieces pc;
    pc.add(&d_part, (size_t)nnz), pc.add(&d_m, N), pc.add(&d_items, N), pc.add(&d_run, N), pc.add(&d_tile, tiles), pc.add(&d_run_off, N);
    pc.add(&d_tile2, tiles), pc.add(&d_item_off, N), pc.add(&d_four, 4);
    if (rowptr_dev) pc.add(&d_rank, (size_t)nnz);
    if (tmp.carve(pc)) return 1;
    hipLaunchKernelGGL(trip_count_kernel, amp::group_grid(n, kG), dim3(256), 0, st, n, (const int32_t *)g->rowptr, (const int32_t *)g->eid, dim,
                       vec_dev, cutoff3, all, d_part, d_rank, d_m, d_run, d_items);
    const unsigned long long *d_total = scan64::exclusive(n, (const unsigned long long *)d_run, d_tile, d_run_off, st);
    const unsigned long long *d_n_items = scan64::exclusive(n, (const uint32_t *)d_items, d_tile2, d_item_off, st);
    hipLaunchKernelGGL(trip_stats_kernel, dim3(1), dim3(256), 0, st, n, (const int32_t *)d_m, d_total, d_n_items, d_four);
    AMP_LAUNCH_CHECK();
    unsigned long long four[4] = {0, 0, 0, 0};
    AMP_HIP(hipMemcpyAsync(four, d_four, sizeof(four), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    const unsigned long long T = four[0];
    // what a handle over the triplets can number, found by the count pass before anything of that size is allocated
    AMP_REQUIRE(T < (1ull << 31), "triplet_pairs: %llu triplets over %lld entries: 2^31 or more", T, (long long)nnz);
    *n_triplets_out = (int64_t)T;
    g_stats[0] = (int64_t)T;
    g_stats[1] = (int64_t)four[2];
    g_stats[2] = four[3] > 0 ? (int64_t)(four[3] * (four[3] - 1)) : 0;
    if (!fill) return 0;
    AMP_REQUIRE(pairs_dev == nullptr || capacity >= (int64_t)T, "triplet_pairs: the pair buffer holds %lld triplets, the graph has %lld",
                (long long)capacity, (long long)T);
    const uint32_t n_items = (uint32_t)four[1];
    if (pairs_dev && n_items > 0)
        hipLaunchKernelGGL(trip_fill_kernel, dim3(blocks(n_items, kFillWaves)), dim3(64 * kFillWaves), 0, st, n, n_items,
                           (const int32_t *)g->rowptr, (const int32_t *)d_part, (const int32_t *)d_m, (const unsigned long long *)d_run_off,
                           (const unsigned long long *)d_item_off, ((uintptr_t)pairs_dev & 7) == 0 ? 1 : 0, pairs_dev);
    if (rowptr_dev)
        hipLaunchKernelGGL(trip_rowptr_kernel, amp::group_grid(n, kG), dim3(256), 0, st, n, (const int32_t *)g->rowptr, (const int32_t *)d_rank,
                           (const int32_t *)d_m, (const unsigned long long *)d_run_off, nnz, (int32_t)T, rowptr_dev);
    AMP_LAUNCH_CHECK();
    AMP_HIP(hipStreamSynchronize(st));   // scratch dies with this scope
    return 0;
}

extern "C" int athena_mp_triplet_stats(int64_t *out)
{
    AMP_REQUIRE(out != nullptr, "triplet_stats: null output");
    for (int k = 0; k < 3; ++k) out[k] = g_stats[k];
    return 0;
}

extern "C" int athena_mp_entry_vectors_fwd(const athena_mp_graph *g, int32_t dim, const float *vec_dev, float *dir_dev)
{
    if (int rc = entries_check("entry_vectors_fwd", g, dim)) return rc;
    if (g->nnz == 0) return 0;
    AMP_REQUIRE((g->n_edge_cols == 0 || vec_dev != nullptr) && dir_dev != nullptr, "entry_vectors_fwd: null array");
    hipLaunchKernelGGL(entry_vectors_fwd_kernel, amp::group_grid(g->n_rows, kG), dim3(256), 0, amp::stream(), g->n_rows,
                       (const int32_t *)g->rowptr, (const int32_t *)g->col, (const int32_t *)g->eid, dim, vec_dev, dir_dev);
    AMP_LAUNCH_CHECK();
    return 0;
}

extern "C" int athena_mp_entry_vectors_bwd(const athena_mp_graph *g, int32_t dim, const float *ddir_dev, float *dvec_dev)
{
    if (int rc = entries_check("entry_vectors_bwd", g, dim)) return rc;
    const int32_t E = g->n_edge_cols;
    if (E == 0) return 0;
    AMP_REQUIRE((g->nnz == 0 || ddir_dev != nullptr) && dvec_dev != nullptr, "entry_vectors_bwd: null array");
    hipLaunchKernelGGL(entry_vectors_bwd_kernel, dim3(blocks(E)), dim3(256), 0, amp::stream(), E, (const int32_t *)g->e_rowptr,
                       (const int32_t *)g->e_row, (const int32_t *)g->e_col, (const int32_t *)g->col, dim, ddir_dev, dvec_dev);
    AMP_LAUNCH_CHECK();
    return 0;
}

extern "C" int athena_mp_triplet_cos_fwd(const athena_mp_graph *tg, int32_t dim, const float *dir_dev, float *cos_dev)
{
    if (int rc = triplet_handle_check("triplet_cos_fwd", tg, dim)) return rc;
    if (tg->nnz == 0) return 0;
    AMP_REQUIRE(dir_dev != nullptr && cos_dev != nullptr, "triplet_cos_fwd: null array");
    hipLaunchKernelGGL(triplet_cos_fwd_kernel, amp::group_grid(tg->n_rows, kG), dim3(256), 0, amp::stream(), tg->n_rows,
                       (const int32_t *)tg->rowptr, (const int32_t *)tg->col, (const int32_t *)tg->eid, dim, dir_dev, cos_dev);
    AMP_LAUNCH_CHECK();
    return 0;
}

extern "C" int athena_mp_triplet_cos_bwd(const athena_mp_graph *tg, int32_t dim, const float *dir_dev, const float *cos_dev,
                                         const float *dcos_dev, float *ddir_dev)
{
    if (int rc = triplet_handle_check("triplet_cos_bwd", tg, dim)) return rc;
    if (tg->n_rows == 0) return 0;
    AMP_REQUIRE((tg->nnz == 0 || (dir_dev != nullptr && cos_dev != nullptr && dcos_dev != nullptr)) && ddir_dev != nullptr,
                "triplet_cos_bwd: null array");
    hipLaunchKernelGGL(triplet_cos_bwd_kernel, dim3(blocks(tg->n_rows)), dim3(256), 0, amp::stream(), tg->n_rows, (const int32_t *)tg->rowptr,
                       (const int32_t *)tg->col, (const int32_t *)tg->eid, (const int32_t *)tg->t_rowptr, (const int32_t *)tg->t_src,
                       (const int32_t *)tg->t_eid, dim, dir_dev, cos_dev, dcos_dev, ddir_dev);
    AMP_LAUNCH_CHECK();
    return 0;
}

namespace {

// the triplet handle of (g, vec, cutoff3) with vec on the device; adj_ia [nnz + 1] always, adj_ja [2, capacity] when asked for
int build_triplet_handle(const char *who, const athena_mp_graph *g, int32_t dim, const float *d_vec, float cutoff3, int64_t T,
                         amp::Scratch &tmp, int32_t *adj_ia_out, int32_t *adj_ja_out, int64_t capacity, athena_mp_graph **tg)
{
    int32_t *d_pairs = nullptr;
    if (tmp.get(&d_pairs, 2 * (size_t)T)) return 1;
    int64_t T2 = 0;
    if (int rc = athena_mp_triplet_pairs(g, dim, d_vec, cutoff3, d_pairs, T, nullptr, &T2)) return rc;
    AMP_REQUIRE(g->nnz < (int64_t)INT32_MAX, "%s: %lld entries: more than a handle has rows", who, (long long)g->nnz);
    return athena_mp_graph_create_bipartite_dev((int32_t)g->nnz, (int32_t)g->nnz, T, d_pairs, adj_ia_out, adj_ja_out, capacity, tg);
}

struct HandleGuard {   // the triplet handle of one *_host call
    athena_mp_graph *tg = nullptr;
    ~HandleGuard()
    {
        if (tg) (void)athena_mp_graph_destroy(tg);
    }
};

} // namespace

extern "C" int athena_mp_triplets_host(const athena_mp_graph *g, int32_t dim, const float *vec, float cutoff3, int32_t *adj_ia_out,
                                       int32_t *adj_ja_out, int64_t capacity, float *dir_out, float *cos_out, int64_t *n_triplets_out)
{
    AMP_REQUIRE(n_triplets_out != nullptr, "triplets_host: null n_triplets_out");
    *n_triplets_out = 0;
    if (int rc = entries_check("triplets_host", g, dim)) return rc;
    AMP_REQUIRE(vec != nullptr || !(dir_out || cos_out) || g->n_edge_cols == 0, "triplets_host: dir and cos need vec");
    hipStream_t st = amp::stream();
    amp::Scratch tmp;
    const int64_t E = g->n_edge_cols, nnz = g->nnz;
    float *d_vec = nullptr;
    if (vec && E > 0 && tmp.upload(&d_vec, vec, (size_t)E * dim, st)) return 1;
    int64_t T = 0;
    if (int rc = athena_mp_triplet_pairs(g, dim, d_vec, cutoff3, nullptr, 0, nullptr, &T)) return rc;
    *n_triplets_out = T;
    if (adj_ja_out == nullptr) return 0;                            // size query
    AMP_REQUIRE(adj_ia_out != nullptr, "triplets_host: null adj_ia");
    AMP_REQUIRE(capacity >= T, "triplets_host: adj_ja buffer holds %lld entries, the graph has %lld triplets", (long long)capacity, (long long)T);
    HandleGuard h;
    if (int rc = build_triplet_handle("triplets_host", g, dim, d_vec, cutoff3, T, tmp, adj_ia_out, adj_ja_out, capacity, &h.tg)) return rc;
    if ((dir_out || cos_out) && nnz > 0) {
        float *d_dir = nullptr, *d_cos = nullptr;
        if (tmp.get(&d_dir, (size_t)nnz * dim) || tmp.get(&d_cos, (size_t)T)) return 1;
        if (int rc = athena_mp_entry_vectors_fwd(g, dim, d_vec, d_dir)) return rc;
        if (tmp.download(dir_out, d_dir, (size_t)nnz * dim, st)) return 1;
        if (cos_out && T > 0) {
            if (int rc = athena_mp_triplet_cos_fwd(h.tg, dim, d_dir, d_cos)) return rc;
            if (tmp.download(cos_out, d_cos, (size_t)T, st)) return 1;
        }
    }
    AMP_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" int athena_mp_triplet_cos_bwd_host(const athena_mp_graph *g, int32_t dim, const float *vec, float cutoff3, int64_t n_triplets,
                                              const float *dcos, float *dvec_out)
{
    if (int rc = entries_check("triplet_cos_bwd_host", g, dim)) return rc;
    const int64_t E = g->n_edge_cols, nnz = g->nnz;
    if (E == 0) return 0;                                           // no edge column: dvec is empty
    AMP_REQUIRE(vec != nullptr && dvec_out != nullptr, "triplet_cos_bwd_host: null array");
    hipStream_t st = amp::stream();
    amp::Scratch tmp;
    float *d_vec = nullptr, *d_dir = nullptr, *d_cos = nullptr, *d_dcos = nullptr, *d_ddir = nullptr, *d_dvec = nullptr;
    if (tmp.upload(&d_vec, vec, (size_t)E * dim, st)) return 1;
    int64_t T = 0;
    if (int rc = athena_mp_triplet_pairs(g, dim, d_vec, cutoff3, nullptr, 0, nullptr, &T)) return rc;
    AMP_REQUIRE(n_triplets == T, "triplet_cos_bwd_host: dcos holds %lld triplets, the graph has %lld", (long long)n_triplets, (long long)T);
    AMP_REQUIRE(T == 0 || dcos != nullptr, "triplet_cos_bwd_host: null dcos");
    std::vector<int32_t> ia((size_t)nnz + 1);
    HandleGuard h;
    if (int rc = build_triplet_handle("triplet_cos_bwd_host", g, dim, d_vec, cutoff3, T, tmp, ia.data(), nullptr, 0, &h.tg)) return rc;
    if (tmp.get(&d_dir, (size_t)nnz * dim) || tmp.get(&d_cos, (size_t)T) || tmp.upload(&d_dcos, dcos, (size_t)T, st) ||
        tmp.get(&d_ddir, (size_t)nnz * dim) || tmp.get(&d_dvec, (size_t)E * dim))
        return 1;
    if (int rc = athena_mp_entry_vectors_fwd(g, dim, d_vec, d_dir)) return rc;
    if (int rc = athena_mp_triplet_cos_fwd(h.tg, dim, d_dir, d_cos)) return rc;
    if (int rc = athena_mp_triplet_cos_bwd(h.tg, dim, d_dir, d_cos, d_dcos, d_ddir)) return rc;
    if (int rc = athena_mp_entry_vectors_bwd(g, dim, d_ddir, d_dvec)) return rc;
    if (tmp.download(dvec_out, d_dvec, (size_t)E * dim, st)) return 1;
    AMP_HIP(hipStreamSynchronize(st));
    return 0;
}
