// A pair list relabelled through a vertex map and merged on the device: graph contraction over a cluster map (the pooled graph of a
// graph U-Net level), the induced subgraph of a vertex selection (id 0 drops a vertex), the merge of a multigraph's duplicate pairs
// (identity map), and -- behind athena_mp_cell_pairs -- the edge graph of a mesh given as elements.  One operation: every fine pair
// is relabelled, the distinct results are kept in order, and who fell where is recorded (members / rowptr / edge_pair), which is
// the pooling handle for per-edge features.  Also here: athena_mp_graph_pairs, a handle's pair list written back on the device.
//
// The definition (include/athena_mp.h; tests compare every array with np.array_equal): for fine edge e = (u, v), a =
// row_cluster[u], b = col_cluster[v]; it takes part iff u, v, a, b >= 1 and, in mode 0, a != b; its coarse key is (min, max) in
// mode 0 and (a, b) in mode 1; coarse pairs are the distinct keys in lexicographic order, members in ascending edge id.
//
// How.  THE KEY (ck_key_kernel, one lane per edge): the pair is one 8-byte load, the two ids two gathers, the key
// (a << bits_for(m_cols)) | b in one unsigned long long; an edge that takes no part gets the bit above those set, so it sorts
// behind every coarse pair and the members are a prefix of the sorted order.  A pair index outside 0..n is never followed: the
// smallest such edge lands in a word the host reads.  ck_map_kernel looks at every id of the maps on its own (an id no edge
// touches is still refused), the smallest offending vertex of each map lands beside it.
// THE SORT is radix::sort_pairs on exactly bits_for(m_rows) + bits_for(m_cols) + 1 bits with the edge id as value; it is stable,
// so the members of a coarse pair ascend without a second key.
// THE HEADS (ck_flag_kernel): flag[s] = the slot takes part and its key differs from the slot before; the one slot where the part
// that takes no part begins writes M.  scan64::exclusive numbers the coarse pairs; P, M and the three refusal words come home in
// one wait.  ck_start_kernel then writes where each coarse pair begins (what the weights are counted from).
// THE FILL (ck_fill_kernel, one lane per sorted slot) writes every output: members and the coarse pair as 8-byte stores,
// edge_pair through the permutation, weights = 1 / fl(start[id + 1] - start[id]), and at the heads rowptr and coords.
// No atomics on data (atomicMin only on the refusal words), no LDS beyond radix_sort.h's and scan64.h's, no scratch.
//
// Resources, -Rpass-analysis=kernel-resource-usage, gfx950 (VGPRs / SGPRs / scratch / LDS bytes / waves per SIMD):
//   ck_key_kernel       6 / 24 / 0 / 0 / 8
//   ck_map_kernel       4 / 17 / 0 / 0 / 8
//   ck_flag_kernel      8 / 20 / 0 / 0 / 8
//   ck_start_kernel     4 / 16 / 0 / 0 / 8
//   ck_fill_kernel     28 / 34 / 0 / 0 / 8
//   longest_row_kernel of call_scratch.h (the largest coarse pair of the stats)
//   gp_pairs_kernel     8 / 18 / 0 / 0 / 8
//   cp_cells_kernel    13 / 29 / 0 / 0 / 8
#include <string.h>

#include <algorithm>

#include "call_scratch.h"
#include "cell_start.h"
#include "common.h"
#include "radix_sort.h"
#include "scan64.h"

namespace amp {
int64_t g_contract_stats[4] = {0, 0, 0, 0};             // athena_mp_contract_stats: of the last call
}

namespace {

// two int32 that travel as 8 bytes; alignment 4, which is all a caller's pointer has to have
struct Pair {
    int32_t x, y;
};

// what the host reads in its one wait, beside the scan's total
struct Info {
    unsigned long long members;              // M: the first sorted slot that takes no part (preset to E)
    unsigned long long bad_pair;             // the smallest edge with an index outside 0..n, ~0: none
    unsigned long long bad_row, bad_col;     // the smallest vertex of each map with an id outside 0..m, ~0: none
};

// one lane per fine edge: key[e] = (a << bb) | b, or `out` (the bit above) where the edge takes no part
__global__ __launch_bounds__(256) void ck_key_kernel(int64_t E, const int32_t *__restrict__ pairs, int32_t n_rows, int32_t n_cols,
                                                     const int32_t *__restrict__ row_cluster, const int32_t *__restrict__ col_cluster,
                                                     int32_t m_rows, int32_t m_cols, int mode, int bb, unsigned long long out,
                                                     unsigned long long *__restrict__ key, Info *__restrict__ info)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const Pair p = reinterpret_cast<const Pair *>(pairs)[e];
    if (p.x < 0 || p.x > n_rows || p.y < 0 || p.y > n_cols) {
        atomicMin(&info->bad_pair, (unsigned long long)e);
        key[e] = out;
        return;
    }
    int32_t a = p.x, b = p.y;
    if (row_cluster && a) a = row_cluster[a - 1];
    if (col_cluster && b) b = col_cluster[b - 1];
    // an id outside 0..m is refused through ck_map_kernel's word before anything is made of the keys; here it only takes no part
    const bool part = a >= 1 && a <= m_rows && b >= 1 && b <= m_cols && !(mode == 0 && a == b);
    if (mode == 0 && a > b) {
        const int32_t t = a;
        a = b, b = t;
    }
    key[e] = part ? ((unsigned long long)(uint32_t)a << bb) | (unsigned long long)(uint32_t)b : out;
}

// one lane per vertex of a map: the smallest vertex whose id lies outside 0..m
__global__ __launch_bounds__(256) void ck_map_kernel(int32_t n, const int32_t *__restrict__ cluster, int32_t m, unsigned long long *__restrict__ bad)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int32_t c = cluster[v];
    if (c < 0 || c > m) atomicMin(bad, (unsigned long long)v);
}

// key order: the slots that take part come first.  flag = head of a coarse pair; the slot where the rest begins writes M
__global__ __launch_bounds__(256) void ck_flag_kernel(int64_t E, const unsigned long long *__restrict__ key_s, unsigned long long out,
                                                      uint32_t *__restrict__ flag, Info *__restrict__ info)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= E) return;
    const unsigned long long k = key_s[s], prev = s ? key_s[s - 1] : out;
    const bool part = k < out;
    flag[s] = (part && (s == 0 || k != prev)) ? 1u : 0u;
    if (!part && (s == 0 || prev < out)) info->members = (unsigned long long)s;
}

// start[c] = the first slot of coarse pair c (0-based), start[P] = M
__global__ __launch_bounds__(256) void ck_start_kernel(int64_t E, int32_t P, int32_t M, const uint32_t *__restrict__ flag,
                                                       const unsigned long long *__restrict__ before, int32_t *__restrict__ start)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s > E) return;
    if (s == E) {
        start[P] = M;
        return;
    }
    if (flag[s]) start[before[s]] = (int32_t)s;
}

// one lane per sorted slot; slot s < M holds fine edge perm[s] of coarse pair before[s] + flag[s] (1-based).  Each output may be null
__global__ __launch_bounds__(256) void ck_fill_kernel(int64_t E, int32_t P, int32_t M, int bb, int dim, const unsigned long long *__restrict__ key_s,
                                                      const int32_t *__restrict__ perm, const uint32_t *__restrict__ flag,
                                                      const unsigned long long *__restrict__ before, const int32_t *__restrict__ start,
                                                      const float *__restrict__ row_points, const float *__restrict__ col_points,
                                                      int32_t *__restrict__ coarse_pairs, int32_t *__restrict__ rowptr,
                                                      int32_t *__restrict__ members, float *__restrict__ weights,
                                                      int32_t *__restrict__ edge_pair, float *__restrict__ coords)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s > E) return;
    if (s == E) {
        if (rowptr) rowptr[P] = M;
        return;
    }
    const int32_t e = perm[s];
    if (s >= M) {
        if (edge_pair) edge_pair[e] = 0;
        return;
    }
    const uint32_t head = flag[s];
    const int32_t id = (int32_t)before[s] + (int32_t)head;        // 1-based
    if (members) reinterpret_cast<Pair *>(members)[s] = Pair{id, e + 1};
    if (edge_pair) edge_pair[e] = id;
    if (weights) weights[s] = 1.0f / (float)(start[id] - start[id - 1]);
    if (!head) return;
    const unsigned long long k = key_s[s];
    const int32_t a = (int32_t)(k >> bb), b = (int32_t)(k & ((1ull << bb) - 1ull));
    if (coarse_pairs) reinterpret_cast<Pair *>(coarse_pairs)[id - 1] = Pair{a, b};
    if (rowptr) rowptr[id - 1] = (int32_t)s;
    if (coords)
        for (int c = 0; c < dim; ++c) coords[(int64_t)(id - 1) * dim + c] = row_points[(int64_t)(a - 1) * dim + c] - col_points[(int64_t)(b - 1) * dim + c];
}

// one lane per edge column of a handle: (row + 1, col + 1) of the first entry that carries it, (0, 0) where none does
__global__ __launch_bounds__(256) void gp_pairs_kernel(int32_t n_edge_cols, const int32_t *__restrict__ e_rowptr, const int32_t *__restrict__ e_row,
                                                       const int32_t *__restrict__ e_col, const int32_t *__restrict__ col, int32_t *__restrict__ pairs)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edge_cols) return;
    const int32_t at = e_rowptr[e];
    Pair p{0, 0};
    if (at < e_rowptr[e + 1]) p = Pair{e_row[at] + 1, col[e_col[at]] + 1};
    reinterpret_cast<Pair *>(pairs)[e] = p;
}

// local vertex pairs of the four cell types, packed two bits per end: pair l of the cell is (code >> 4l & 3, code >> (4l + 2) & 3)
__host__ __device__ inline uint32_t cell_code(int cell_type)
{
    // segment 01; triangle 01 02 12; quadrilateral 01 12 23 30; tetrahedron 01 02 03 12 13 23
    return cell_type == 1 ? 0x4u : cell_type == 2 ? 0x984u : cell_type == 3 ? 0x3E94u : 0xED9C84u;
}

// one lane per output slot c * ne + l; a vertex id outside 1..n_vertices is copied but reported: the smallest such cell lands in *bad
__global__ __launch_bounds__(256) void cp_cells_kernel(int64_t total, int32_t nv, int32_t ne, uint32_t code, int32_t n_vertices,
                                                       const int32_t *__restrict__ cells, int32_t *__restrict__ pairs,
                                                       unsigned long long *__restrict__ bad)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int64_t c = t / ne;
    const int l = (int)(t - c * ne);
    const int32_t u = cells[c * nv + ((code >> (4 * l)) & 3u)], v = cells[c * nv + ((code >> (4 * l + 2)) & 3u)];
    if (u < 1 || u > n_vertices || v < 1 || v > n_vertices) atomicMin(bad, (unsigned long long)c);
    if (pairs) reinterpret_cast<Pair *>(pairs)[t] = Pair{u, v};
}

// what every contraction entry checks before anything touches the device: 0, or 2 with the message set
int ck_arguments_check(const char *who, int64_t E, int32_t n_rows, int32_t n_cols, bool has_row_map, bool has_col_map, int32_t m_rows,
                       int32_t m_cols, int32_t mode, int32_t dim, bool has_row_points, bool has_col_points, bool wants_coords)
{
    AMP_REQUIRE(mode == 0 || mode == 1, "%s: mode = %d outside [0,1]", who, mode);
    AMP_REQUIRE(E >= 0, "%s: n_pairs = %lld is negative", who, (long long)E);
    AMP_REQUIRE(E < (1ll << 31), "%s: n_pairs = %lld, 2^31 or more", who, (long long)E);
    AMP_REQUIRE(n_rows >= 0 && n_cols >= 0 && m_rows >= 0 && m_cols >= 0, "%s: n_rows = %d, n_cols = %d, m_rows = %d, m_cols = %d: negative", who,
                n_rows, n_cols, m_rows, m_cols);
    AMP_REQUIRE(mode == 1 || (n_rows == n_cols && m_rows == m_cols), "%s: mode 0 is one set: n_rows = %d, n_cols = %d, m_rows = %d, m_cols = %d", who,
                n_rows, n_cols, m_rows, m_cols);
    AMP_REQUIRE(has_row_map || m_rows == n_rows, "%s: no row map (the identity), but m_rows = %d is not n_rows = %d", who, m_rows, n_rows);
    AMP_REQUIRE(has_col_map || m_cols == n_cols, "%s: no column map (the identity), but m_cols = %d is not n_cols = %d", who, m_cols, n_cols);
    AMP_REQUIRE(has_row_points == has_col_points, "%s: only one of row_points and col_points is given", who);
    AMP_REQUIRE(!has_row_points || (dim >= 1 && dim <= 3), "%s: dim = %d outside [1,3]", who, dim);
    AMP_REQUIRE(!wants_coords || has_row_points, "%s: coords asked for without points", who);
    const int ba = bits_for((unsigned long long)m_rows), bb = bits_for((unsigned long long)m_cols);
    AMP_REQUIRE(ba + bb <= 62, "%s: the keys need %d + %d bits for %d and %d clusters, more than 62", who, ba, bb, m_rows, m_cols);
    return 0;
}

} // namespace

namespace amp {

// Every output may be null alone; all null: the counts only.  Everything on the library's stream; synchronised on return.
int contract_pairs_core(const char *who, int64_t E, const int32_t *pairs_dev, int32_t n_rows, int32_t n_cols, const int32_t *row_cluster_dev,
                        const int32_t *col_cluster_dev, int32_t m_rows, int32_t m_cols, int32_t mode, int32_t dim, const float *row_points_dev,
                        const float *col_points_dev, int64_t capacity, int64_t member_capacity, int32_t *coarse_pairs_dev, int32_t *rowptr_dev,
                        int32_t *members_dev, float *weights_dev, int32_t *edge_pair_dev, float *coords_dev, int64_t *n_coarse_out,
                        int64_t *n_members_out)
{
    std::fill(g_contract_stats, g_contract_stats + 4, (int64_t)0);
    AMP_REQUIRE(n_coarse_out != nullptr && n_members_out != nullptr, "%s: null n_coarse_out or n_members_out", who);
    *n_coarse_out = *n_members_out = 0;
    if (int rc = ck_arguments_check(who, E, n_rows, n_cols, row_cluster_dev != nullptr, col_cluster_dev != nullptr, m_rows, m_cols, mode, dim,
                                    row_points_dev != nullptr, col_points_dev != nullptr, coords_dev != nullptr))
        return rc;
    const bool any_out = coarse_pairs_dev || rowptr_dev || members_dev || weights_dev || edge_pair_dev || coords_dev;
    hipStream_t st = stream();
    if (E == 0) {
        if (rowptr_dev) {
            AMP_REQUIRE(capacity >= 0, "%s: the buffers hold %lld coarse pairs, the list has %lld", who, (long long)capacity, 0ll);
            AMP_HIP(hipMemsetAsync(rowptr_dev, 0, sizeof(int32_t), st));
            AMP_HIP(hipStreamSynchronize(st));
        }
        return 0;
    }
    AMP_REQUIRE(pairs_dev != nullptr, "%s: null pairs", who);
    const int ba = bits_for((unsigned long long)m_rows), bb = bits_for((unsigned long long)m_cols), bits = ba + bb + 1;
    const unsigned long long out = 1ull << (ba + bb);

    // one allocation cut into pieces (pieces.h)
    const size_t N = (size_t)E;
    Info *d_info = nullptr;
    unsigned long long *d_key = nullptr, *d_key_s = nullptr, *d_key_t = nullptr, *d_before = nullptr, *d_tile = nullptr;
    int32_t *d_perm = nullptr, *d_perm_t = nullptr, *d_start = nullptr, *d_longest = nullptr;
    uint32_t *d_flag = nullptr;
    char *d_temp = nullptr;
    Pieces pc;
    pc.add(&d_info, 1), pc.add(&d_key, N), pc.add(&d_key_s, N), pc.add(&d_key_t, N), pc.add(&d_before, N);
    pc.add(&d_tile, (size_t)scan64::tiles(E) + 1), pc.add(&d_perm, N), pc.add(&d_perm_t, N), pc.add(&d_flag, N), pc.add(&d_start, N + 1);
    // longest_row uses kLongestBlocks words; four times that keeps the request what it was when the partials were one per wave
    // (tests/test_pieces.py holds bytes() to it)
    pc.add(&d_longest, 4 * (size_t)kLongestBlocks), pc.add(&d_temp, radix::scratch_bytes(E));
    Scratch tmp;
    if (tmp.carve(pc)) return 1;

    Info info{(unsigned long long)E, ~0ull, ~0ull, ~0ull};
    AMP_HIP(hipMemcpyAsync(d_info, &info, sizeof(Info), hipMemcpyHostToDevice, st));
    if (row_cluster_dev && n_rows > 0)
        hipLaunchKernelGGL(ck_map_kernel, dim3(blocks(n_rows)), dim3(256), 0, st, n_rows, row_cluster_dev, m_rows, &d_info->bad_row);
    if (col_cluster_dev && n_cols > 0)
        hipLaunchKernelGGL(ck_map_kernel, dim3(blocks(n_cols)), dim3(256), 0, st, n_cols, col_cluster_dev, m_cols, &d_info->bad_col);
    hipLaunchKernelGGL(ck_key_kernel, dim3(blocks(E)), dim3(256), 0, st, E, pairs_dev, n_rows, n_cols, row_cluster_dev, col_cluster_dev, m_rows,
                       m_cols, (int)mode, bb, out, d_key, d_info);
    AMP_LAUNCH_CHECK();
    if (int rc = radix::sort_pairs<unsigned long long>((const unsigned long long *)d_key, nullptr, E, bits, d_key_s, d_perm, d_key_t, d_perm_t,
                                                       d_temp, st))
        return rc;
    hipLaunchKernelGGL(ck_flag_kernel, dim3(blocks(E)), dim3(256), 0, st, E, (const unsigned long long *)d_key_s, out, d_flag, d_info);
    const unsigned long long *d_total = scan64::exclusive<uint32_t>(E, (const uint32_t *)d_flag, d_tile, d_before, st);
    AMP_LAUNCH_CHECK();
    unsigned long long heads = 0;
    AMP_HIP(hipMemcpyAsync(&heads, d_total, sizeof(heads), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipMemcpyAsync(&info, d_info, sizeof(Info), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));                                // the one wait
    if (info.bad_pair != ~0ull) {
        int32_t p[2] = {0, 0};
        AMP_HIP(hipMemcpy(p, pairs_dev + 2 * info.bad_pair, sizeof(p), hipMemcpyDeviceToHost));
        set_error("%s: pairs(:,%llu) = (%d, %d) outside [0,%d] x [0,%d]", who, info.bad_pair + 1, p[0], p[1], n_rows, n_cols);
        return 2;
    }
    if (info.bad_row != ~0ull || info.bad_col != ~0ull) {
        const bool row = info.bad_row != ~0ull;
        const unsigned long long v = row ? info.bad_row : info.bad_col;
        int32_t c = 0;
        AMP_HIP(hipMemcpy(&c, (row ? row_cluster_dev : col_cluster_dev) + v, sizeof(c), hipMemcpyDeviceToHost));
        set_error("%s: %s(%llu) = %d outside [0,%d]", who, row ? "row_cluster" : "col_cluster", v + 1, c, row ? m_rows : m_cols);
        return 2;
    }
    const int64_t P64 = (int64_t)heads, M64 = (int64_t)info.members;
    *n_coarse_out = P64;
    *n_members_out = M64;
    g_contract_stats[0] = P64;
    g_contract_stats[1] = M64;
    g_contract_stats[2] = bits;
    if (!any_out) return 0;                                           // size query
    AMP_REQUIRE(!(coarse_pairs_dev || rowptr_dev || coords_dev) || capacity >= P64, "%s: the buffers hold %lld coarse pairs, the list has %lld", who,
                (long long)capacity, (long long)P64);
    AMP_REQUIRE(!(members_dev || weights_dev) || member_capacity >= M64, "%s: the buffers hold %lld members, the list has %lld", who,
                (long long)member_capacity, (long long)M64);
    const int32_t P = (int32_t)P64, M = (int32_t)M64;

    hipLaunchKernelGGL(ck_start_kernel, dim3(blocks(E + 1)), dim3(256), 0, st, E, P, M, (const uint32_t *)d_flag, (const unsigned long long *)d_before,
                       d_start);
    hipLaunchKernelGGL(ck_fill_kernel, dim3(blocks(E + 1)), dim3(256), 0, st, E, P, M, bb, (int)dim, (const unsigned long long *)d_key_s,
                       (const int32_t *)d_perm, (const uint32_t *)d_flag, (const unsigned long long *)d_before, (const int32_t *)d_start,
                       row_points_dev, col_points_dev, coarse_pairs_dev, rowptr_dev, members_dev, weights_dev, edge_pair_dev, coords_dev);
    int32_t longest = 0;
    if (int rc = longest_row(P, (const int32_t *)d_start, d_longest, &longest, st)) return rc;   // the wait; scratch dies with this scope
    g_contract_stats[3] = longest;
    return 0;
}

} // namespace amp

extern "C" int athena_mp_contract_pairs(int64_t n_pairs, const int32_t *pairs_dev, int32_t n_rows, int32_t n_cols,
                                        const int32_t *row_cluster_dev, const int32_t *col_cluster_dev, int32_t m_rows, int32_t m_cols,
                                        int32_t mode, int32_t dim, const float *row_points_dev, const float *col_points_dev, int64_t capacity,
                                        int64_t member_capacity, int32_t *coarse_pairs_dev, int32_t *rowptr_dev, int32_t *members_dev,
                                        float *weights_dev, int32_t *edge_pair_dev, float *coords_dev, int64_t *n_coarse_out,
                                        int64_t *n_members_out)
{
    return amp::contract_pairs_core("contract_pairs", n_pairs, pairs_dev, n_rows, n_cols, row_cluster_dev, col_cluster_dev, m_rows, m_cols, mode,
                                    dim, row_points_dev, col_points_dev, capacity, member_capacity, coarse_pairs_dev, rowptr_dev, members_dev,
                                    weights_dev, edge_pair_dev, coords_dev, n_coarse_out, n_members_out);
}

// Fortran arrays in, Fortran arrays out: one pass into buffers of n_pairs rows (P <= M <= n_pairs), narrowed on the way home
extern "C" int athena_mp_contract_pairs_host(int64_t n_pairs, const int32_t *pairs, int32_t n_rows, int32_t n_cols, const int32_t *row_cluster,
                                             const int32_t *col_cluster, int32_t m_rows, int32_t m_cols, int32_t mode, int32_t dim,
                                             const float *row_points, const float *col_points, int64_t capacity, int64_t member_capacity,
                                             int32_t *coarse_pairs_out, int32_t *rowptr_out, int32_t *members_out, float *weights_out,
                                             int32_t *edge_pair_out, float *coords_out, int64_t *n_coarse_out, int64_t *n_members_out)
{
    const char *who = "contract_pairs_host";
    AMP_REQUIRE(n_coarse_out != nullptr && n_members_out != nullptr, "%s: null n_coarse_out or n_members_out", who);
    *n_coarse_out = *n_members_out = 0;
    // before anything is uploaded: the sizes size the copies
    if (int rc = ck_arguments_check(who, n_pairs, n_rows, n_cols, row_cluster != nullptr, col_cluster != nullptr, m_rows, m_cols, mode, dim,
                                    row_points != nullptr, col_points != nullptr, coords_out != nullptr))
        return rc;
    AMP_REQUIRE(n_pairs == 0 || pairs != nullptr, "%s: null pairs", who);
    hipStream_t st = amp::stream();
    amp::Scratch tmp;
    const size_t N = (size_t)n_pairs, D = row_points ? (size_t)dim : 1;
    const bool one_map = row_cluster && row_cluster == col_cluster, one_set = row_points && row_points == col_points;
    int32_t *d_pairs = nullptr, *d_rc = nullptr, *d_cc = nullptr, *d_cp = nullptr, *d_rowptr = nullptr, *d_mem = nullptr, *d_ep = nullptr;
    float *d_rp = nullptr, *d_cpt = nullptr, *d_w = nullptr, *d_co = nullptr;
    if (tmp.upload(&d_pairs, pairs, 2 * N, st) || (row_cluster && tmp.upload(&d_rc, row_cluster, (size_t)n_rows, st))) return 1;
    if (one_map) d_cc = d_rc;
    else if (col_cluster && tmp.upload(&d_cc, col_cluster, (size_t)n_cols, st)) return 1;
    if (row_points && tmp.upload(&d_rp, row_points, (size_t)m_rows * D, st)) return 1;
    if (one_set) d_cpt = d_rp;
    else if (col_points && tmp.upload(&d_cpt, col_points, (size_t)m_cols * D, st)) return 1;
    if ((coarse_pairs_out && tmp.get(&d_cp, 2 * N)) || (rowptr_out && tmp.get(&d_rowptr, N + 1)) || (members_out && tmp.get(&d_mem, 2 * N)) ||
        (weights_out && tmp.get(&d_w, N)) || (edge_pair_out && tmp.get(&d_ep, N)) || (coords_out && tmp.get(&d_co, N * D)))
        return 1;
    int64_t P = 0, M = 0;
    if (int rc = amp::contract_pairs_core(who, n_pairs, d_pairs, n_rows, n_cols, d_rc, d_cc, m_rows, m_cols, mode, dim, d_rp, d_cpt, n_pairs, n_pairs,
                                          d_cp, d_rowptr, d_mem, d_w, d_ep, d_co, &P, &M))
        return rc;
    *n_coarse_out = P;
    *n_members_out = M;
    AMP_REQUIRE(!(coarse_pairs_out || rowptr_out || coords_out) || capacity >= P, "%s: the buffers hold %lld coarse pairs, the list has %lld", who,
                (long long)capacity, (long long)P);
    AMP_REQUIRE(!(members_out || weights_out) || member_capacity >= M, "%s: the buffers hold %lld members, the list has %lld", who,
                (long long)member_capacity, (long long)M);
    if (tmp.download(coarse_pairs_out, d_cp, 2 * (size_t)P, st) || tmp.download(rowptr_out, d_rowptr, (size_t)P + 1, st) ||
        tmp.download(members_out, d_mem, 2 * (size_t)M, st) || tmp.download(weights_out, d_w, (size_t)M, st) ||
        tmp.download(edge_pair_out, d_ep, N, st) || tmp.download(coords_out, d_co, (size_t)P * D, st))
        return 1;
    AMP_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" int athena_mp_contract_stats(int64_t out[4])
{
    AMP_REQUIRE(out != nullptr, "contract_stats: null output");
    std::copy(amp::g_contract_stats, amp::g_contract_stats + 4, out);
    return 0;
}

extern "C" int athena_mp_graph_pairs(const athena_mp_graph *g, int32_t *pairs_dev, int64_t capacity)
{
    const char *who = "graph_pairs";
    AMP_REQUIRE(g != nullptr, "%s: null graph", who);
    if (g->n_edge_cols == 0) return 0;
    AMP_REQUIRE(pairs_dev != nullptr, "%s: null pairs", who);
    AMP_REQUIRE(capacity >= g->n_edge_cols, "%s: the buffer holds %lld pairs, the handle has %d edge columns", who, (long long)capacity,
                g->n_edge_cols);
    AMP_REQUIRE(g->e_rowptr && g->e_row && g->e_col && g->col, "%s: the handle has no edge-column index", who);
    hipLaunchKernelGGL(gp_pairs_kernel, dim3(blocks(g->n_edge_cols)), dim3(256), 0, amp::stream(), g->n_edge_cols, (const int32_t *)g->e_rowptr,
                       (const int32_t *)g->e_row, (const int32_t *)g->e_col, (const int32_t *)g->col, pairs_dev);
    AMP_LAUNCH_CHECK();
    return 0;
}

extern "C" int athena_mp_cell_pairs(int32_t n_vertices, int64_t n_cells, int32_t cell_type, const int32_t *cells_dev, int32_t *pairs_dev,
                                    int64_t capacity, int64_t *n_pairs_out)
{
    const char *who = "cell_pairs";
    AMP_REQUIRE(n_pairs_out != nullptr, "%s: null n_pairs_out", who);
    *n_pairs_out = 0;
    AMP_REQUIRE(cell_type >= 1 && cell_type <= 4, "%s: cell_type = %d outside [1,4]", who, cell_type);
    AMP_REQUIRE(n_vertices >= 0 && n_cells >= 0, "%s: n_vertices = %d, n_cells = %lld: negative", who, n_vertices, (long long)n_cells);
    static const int32_t kNv[5] = {0, 2, 3, 4, 4}, kNe[5] = {0, 1, 3, 4, 6};
    const int32_t nv = kNv[cell_type], ne = kNe[cell_type];
    AMP_REQUIRE(n_cells < (1ll << 31) / ne, "%s: %lld cells of %d pairs, 2^31 pairs or more", who, (long long)n_cells, ne);
    const int64_t total = n_cells * ne;
    *n_pairs_out = total;
    if (total == 0) return 0;
    AMP_REQUIRE(cells_dev != nullptr, "%s: null cells", who);
    AMP_REQUIRE(pairs_dev == nullptr || capacity >= total, "%s: the buffer holds %lld pairs, the cells have %lld", who, (long long)capacity,
                (long long)total);
    hipStream_t st = amp::stream();
    amp::Scratch tmp;
    BadWord word;
    unsigned long long bad = ~0ull;
    if (int rc = word.arm(tmp, st)) return rc;
    hipLaunchKernelGGL(cp_cells_kernel, dim3(blocks(total)), dim3(256), 0, st, total, nv, ne, cell_code(cell_type), n_vertices, cells_dev, pairs_dev,
                       word.dev);
    AMP_LAUNCH_CHECK();
    if (int rc = word.fetch(&bad, st)) return rc;
    if (bad != ~0ull) {
        int32_t c[4] = {0, 0, 0, 0};
        AMP_HIP(hipMemcpy(c, cells_dev + bad * nv, sizeof(int32_t) * nv, hipMemcpyDeviceToHost));
        int k = 0;
        while (k < nv - 1 && c[k] >= 1 && c[k] <= n_vertices) ++k;
        amp::set_error("%s: cells(%d,%llu) = %d outside [1,%d]", who, k + 1, bad + 1, c[k], n_vertices);
        return 2;
    }
    return 0;
}
