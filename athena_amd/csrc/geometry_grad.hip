// Geometry gradients on the device: the reverse step of the two graph builders.  A layer returns its gradient per EDGE
// (graph_nop_layer's dcoords [E, d], duvenaud_msgpass_layer's de [E, F_e]); these entries carry it back to what the caller owns:
// the points of athena_mp_radius_pairs, or the atoms and the cell of athena_mp_periodic_pairs.
//
// The definition (include/athena_mp.h holds the same text; tests/geometry_reference.py is its numpy transcription).  All
// arithmetic is fp32, every operation rounded on its own (-ffp-contract=off, correctly rounded / and sqrt, as the builders).
// Row i of the handle is its forward CSR as athena_mp_graph_export shows it (rowptr, col, eid; eid = -1: no edge column).
//
//   signed gather:  acc = +0; for k = rowptr[i] .. rowptr[i+1]-1 in order, c = col[k], e = eid[k]: skip the entry when e < 0 (a self
//                   loop) or c == i (a self-image edge: both ends are the same atom); else acc = acc + t_e when i < c, acc = acc - t_e
//                   when i > c.  out[i] = acc; a row without entries gives +0 and every output element is written.
//   points mode:    t_e = dcoords[e, :] (dim 1..3), dpoints [n, dim] = out: the reverse of coords[e] = p_i - p_j.
//   periodic mode:  x = vec[e];  s = ((x0 x0) + x1 x1) + x2 x2, r = sqrt(s) (the builder's own s and r; r > cutoff_min >= 0);
//                   q = (((de[e,0] + de[e,1]) + ...) + de[e,fe_cols-1]) / cutoff_max;  u_c = x_c / r;  gx_c = dvec[e,c] + q u_c
//                   (q u_c alone without dvec, dvec[e,c] alone without dfeature).
//     dcart [n, 3]     signed gather of t_e = gx_e: dE/d(Cartesian position)
//     dfrac [n, 3]     dfrac[i,k] = ((L[k][0] g0) + L[k][1] g1) + L[k][2] g2, g = dcart[i], L the lattice of i's structure
//     virial [B, 3, 3] virial[s][c][d] = sum over the structure's edges of x_c gx_d (summation order free, no atomics)
//     dlat [B, 3, 3]   L^-T virial: dE/dL at fixed fractional coordinates (x = v L); formed in fp64 from the fp32 lattice and the
//                      fp32 virial, rounded once
//
// How.  geo_vertex_gather: rows are short (8 - 100 entries) and what costs is the chain id -> operand, so kGroup lanes share a row:
// each loads the ids and forms the term of ONE entry, then the terms pass through the group in entry order (__shfl, no LDS) and
// every lane of the group adds them in that order -- the sequential sum, bit for bit, whatever the row length (a hub row of hundreds
// of entries just takes more rounds).  No [E, 3] intermediate exists: the periodic term is formed from vec / de / dvec where it is
// used.  dfrac is the epilogue of the same launch.  Rows of three floats are never 16-byte aligned: every access is 4 bytes wide.
// geo_virial_kernel: the host cuts each structure's edge range into items of at most kItemEdges edges; one wave per item keeps
// lane-strided partials of the nine sums, folds them with a fixed __shfl_xor tree and stores the item's nine numbers;
// geo_virial_finish_kernel adds a structure's items in item order and applies L^-T in fp64.  No atomics: two runs are
// byte-identical.
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int kGroup = 8;                       // lanes that share a row
constexpr int kGatherRows = 256 / kGroup;       // rows per 256-thread block
constexpr int kItemEdges = 4096;                // edges per work item of the virial
constexpr int kVirialWaves = 4;                 // work items per 256-thread block
constexpr int kWsTable = 17, kWsPartial = 18;   // workspace slots: the uploaded index tables, the item partials

enum { kPoints = 0, kPeriodic = 1, kSetRows = 2, kSetCols = 3 };   // the last two: the plain sums of a two-set graph, + and -

struct GeoEdge {                                // what the periodic term is formed from
    const float *vec, *de, *dvec;
    int32_t fe_cols;
    float cutoff_max;
};

// x = vec[e] and gx of the definition
__device__ __forceinline__ void geo_edge_term(const GeoEdge &P, int64_t e, float &x0, float &x1, float &x2, float &g0, float &g1,
                                              float &g2)
{
    x0 = P.vec[3 * e];
    x1 = P.vec[3 * e + 1];
    x2 = P.vec[3 * e + 2];
    if (P.de) {
        const float s = ((x0 * x0) + x1 * x1) + x2 * x2;
        const float r = sqrtf(s);
        const float *row = P.de + e * P.fe_cols;
        float sum = row[0];
        for (int32_t k = 1; k < P.fe_cols; ++k) sum = sum + row[k];
        const float q = sum / P.cutoff_max;
        g0 = q * (x0 / r);
        g1 = q * (x1 / r);
        g2 = q * (x2 / r);
        if (P.dvec) {
            g0 = P.dvec[3 * e] + g0;
            g1 = P.dvec[3 * e + 1] + g1;
            g2 = P.dvec[3 * e + 2] + g2;
        }
    } else {
        g0 = P.dvec[3 * e];
        g1 = P.dvec[3 * e + 1];
        g2 = P.dvec[3 * e + 2];
    }
}

// kGroup lanes per row.  kPoints: out [n, dim] from t [E, dim].  kSetRows / kSetCols: the same from a CSR whose rows and columns
// index different sets (no sign by index, no skip: every entry counts, + for kSetRows, - for kSetCols).  kPeriodic: out = dcart [n, 3] (may be null) and dfrac (may be
// null; offsets [B + 1] and lat [B, 3, 3] on the device) from P.
template <int MODE>
__global__ __launch_bounds__(256) void geo_vertex_gather(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                         const int32_t *__restrict__ eid, int32_t dim, const float *__restrict__ t,
                                                         GeoEdge P, float *__restrict__ out, float *__restrict__ dfrac,
                                                         const int32_t *__restrict__ offsets, int32_t B, const float *__restrict__ lat)
{
    const int lane = threadIdx.x & 63;
    const int sub = lane & (kGroup - 1), first = lane & ~(kGroup - 1);
    const int64_t row = (int64_t)blockIdx.x * kGatherRows + threadIdx.x / kGroup;
    int32_t beg = 0, len = 0;
    if (row < n) {
        beg = rowptr[row];
        len = rowptr[row + 1] - beg;
    }
    int32_t rounds = len;                                           // the longest row of the wave: every lane takes part in every round
#pragma unroll
    for (int o = 32; o >= kGroup; o >>= 1) rounds = max(rounds, __shfl_xor(rounds, o));
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int32_t k0 = 0; k0 < rounds; k0 += kGroup) {
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
        bool use = false;
        if (k0 + sub < len) {
            const int64_t k = (int64_t)beg + k0 + sub;
            const int32_t c = col[k], e = eid[k];
            if (e >= 0 && (MODE == kSetRows || MODE == kSetCols || (int64_t)c != row)) {
                use = true;
                if (MODE != kPeriodic) {
                    const float *src = t + (int64_t)e * dim;
                    t0 = src[0];
                    if (dim > 1) t1 = src[1];
                    if (dim > 2) t2 = src[2];
                } else {
                    float x0, x1, x2;
                    geo_edge_term(P, e, x0, x1, x2, t0, t1, t2);
                }
                if (MODE == kSetCols || ((MODE == kPoints || MODE == kPeriodic) && row > (int64_t)c)) {
                    t0 = -t0;
                    t1 = -t1;
                    t2 = -t2;
                }
            }
        }
        const uint32_t bits = (uint32_t)(__ballot(use) >> first) & ((1u << kGroup) - 1u);
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {                          // entry order: k0, k0 + 1, ...
            const float s0 = __shfl(t0, first + j), s1 = __shfl(t1, first + j), s2 = __shfl(t2, first + j);
            if ((bits >> j) & 1u) {
                a0 = a0 + s0;
                a1 = a1 + s1;
                a2 = a2 + s2;
            }
        }
    }
    if (row >= n || sub >= (MODE != kPeriodic ? dim : 3)) return;
    if (out) out[row * (MODE != kPeriodic ? dim : 3) + sub] = sub == 0 ? a0 : sub == 1 ? a1 : a2;
    if (MODE == kPeriodic && dfrac) {
        int32_t lo = 0, hi = B;                                     // the last structure that starts at or before this atom
        while (hi - lo > 1) {
            const int32_t mid = lo + (hi - lo) / 2;
            if ((int64_t)offsets[mid] <= row) lo = mid;
            else hi = mid;
        }
        const float *L = lat + 9 * (int64_t)lo + 3 * sub;
        dfrac[row * 3 + sub] = ((L[0] * a0) + L[1] * a1) + L[2] * a2;
    }
}

// one wave per work item (edges e0 .. e1-1 of one structure): partial[9 * item + 3 c + d] = sum x_c gx_d
__global__ __launch_bounds__(64 * kVirialWaves) void geo_virial_kernel(int32_t n_items, const int32_t *__restrict__ items, GeoEdge P,
                                                                       float *__restrict__ partial)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * kVirialWaves + (threadIdx.x >> 6);
    if (w >= n_items) return;
    const int32_t e0 = items[2 * w], e1 = items[2 * w + 1];
    float p[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int32_t e = e0 + lane; e < e1; e += 64) {
        float x[3], g[3];
        geo_edge_term(P, e, x[0], x[1], x[2], g[0], g[1], g[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = 0; d < 3; ++d) p[3 * c + d] = p[3 * c + d] + x[c] * g[d];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) p[k] = p[k] + __shfl_xor(p[k], o);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) partial[9 * w + k] = p[k];
    }
}

// thread s: the items of structure s in item order -> virial[s]; dlat[s] = L^-T virial[s] in fp64, rounded once
__global__ __launch_bounds__(256) void geo_virial_finish_kernel(int32_t B, const int32_t *__restrict__ item_first,
                                                                const float *__restrict__ partial, const float *__restrict__ lat,
                                                                float *__restrict__ virial, float *__restrict__ dlat)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= B) return;
    float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int32_t w = item_first[s]; w < item_first[s + 1]; ++w) {
#pragma unroll
        for (int k = 0; k < 9; ++k) v[k] = v[k] + partial[9 * (int64_t)w + k];
    }
    if (virial) {
#pragma unroll
        for (int k = 0; k < 9; ++k) virial[9 * s + k] = v[k];
    }
    if (dlat) {
        double L[3][3], X[3][3];                                    // X[a] = L_b x L_c, (a, b, c) cyclic: column a of L^-1 is X[a] / det
#pragma unroll
        for (int k = 0; k < 9; ++k) L[k / 3][k % 3] = (double)lat[9 * s + k];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double *u = L[(a + 1) % 3], *w = L[(a + 2) % 3];
            X[a][0] = u[1] * w[2] - u[2] * w[1];
            X[a][1] = u[2] * w[0] - u[0] * w[2];
            X[a][2] = u[0] * w[1] - u[1] * w[0];
        }
        const double det = L[0][0] * X[0][0] + L[0][1] * X[0][1] + L[0][2] * X[0][2];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double sum = (X[a][0] / det) * (double)v[d] + (X[a][1] / det) * (double)v[3 + d] + (X[a][2] / det) * (double)v[6 + d];
                dlat[9 * s + 3 * a + d] = (float)sum;
            }
    }
}

// a handle whose entries carry no edge column (a Kipf handle): more entries than the one self loop per row that a handle over
// zero edges can hold
bool no_edge_columns(const athena_mp_graph *g) { return g->n_edge_cols == 0 && g->nnz > (int64_t)g->n_rows; }

} // namespace

namespace amp {

int periodic_grad_check(const athena_mp_graph *g, int32_t B, int32_t n, const int32_t *offsets, const int64_t *edge_offsets,
                        float cutoff_max, bool has_dfeature, int32_t fe_cols, bool has_dvec)
{
    AMP_REQUIRE(g != nullptr, "periodic_grad: null graph handle");
    AMP_REQUIRE(B >= 0 && n >= 0 && offsets != nullptr && edge_offsets != nullptr, "periodic_grad: bad arguments");
    AMP_REQUIRE(g->n_rows == g->n_cols, "periodic_grad: the handle is not square (%d rows, %d columns)", g->n_rows, g->n_cols);
    AMP_REQUIRE(n == g->n_rows, "periodic_grad: n_atoms = %d, the handle has %d rows", n, g->n_rows);
    AMP_REQUIRE(offsets[0] == 0, "periodic_grad: offsets(1) = %d, not 0", offsets[0]);
    for (int32_t s = 0; s < B; ++s)
        AMP_REQUIRE(offsets[s + 1] >= offsets[s], "periodic_grad: structure %d: offsets descend from %d to %d", s + 1, offsets[s],
                    offsets[s + 1]);
    AMP_REQUIRE(offsets[B] == n, "periodic_grad: offsets end at %d, the batch has %d atoms", offsets[B], n);
    AMP_REQUIRE(edge_offsets[0] == 0, "periodic_grad: edge_offsets(1) = %lld, not 0", (long long)edge_offsets[0]);
    for (int32_t s = 0; s < B; ++s)
        AMP_REQUIRE(edge_offsets[s + 1] >= edge_offsets[s], "periodic_grad: structure %d: edge_offsets descend from %lld to %lld", s + 1,
                    (long long)edge_offsets[s], (long long)edge_offsets[s + 1]);
    AMP_REQUIRE(!(no_edge_columns(g) || (g->n_edge_cols == 0 && edge_offsets[B] > 0)),
                "periodic_grad: the handle has no edge columns: build it with edge ids (DeviceGraph.from_structures)");
    AMP_REQUIRE(edge_offsets[B] == (int64_t)g->n_edge_cols, "periodic_grad: edge_offsets end at %lld, the handle has %d edge columns",
                (long long)edge_offsets[B], g->n_edge_cols);
    // (without edges both arrays are empty, and an empty array may be a null pointer)
    AMP_REQUIRE(g->n_edge_cols == 0 || has_dfeature || has_dvec,
                "periodic_grad: dfeature and dvec are both null: there is no gradient to carry back");
    AMP_REQUIRE(!has_dfeature || fe_cols >= 1, "periodic_grad: fe_cols = %d with a dfeature: need at least one column", fe_cols);
    AMP_REQUIRE(isfinite(cutoff_max) && cutoff_max > 0.f, "periodic_grad: cutoff_max = %g: need a finite value above 0", (double)cutoff_max);
    return 0;
}

int points_grad_check(const athena_mp_graph *g, int32_t dim)
{
    AMP_REQUIRE(g != nullptr, "edge_grad_to_points: null graph handle");
    AMP_REQUIRE(dim >= 1 && dim <= 3, "edge_grad_to_points: dim = %d is outside 1..3", dim);
    AMP_REQUIRE(g->n_rows == g->n_cols, "edge_grad_to_points: the handle is not square (%d rows, %d columns)", g->n_rows, g->n_cols);
    AMP_REQUIRE(!no_edge_columns(g), "edge_grad_to_points: the handle has no edge columns: build it with edge ids (DeviceGraph.from_points)");
    return 0;
}

int point_sets_grad_check(const athena_mp_graph *g, int32_t dim, bool want_queries, bool want_sources)
{
    AMP_REQUIRE(g != nullptr, "edge_grad_to_point_sets: null graph handle");
    AMP_REQUIRE(dim >= 1 && dim <= 3, "edge_grad_to_point_sets: dim = %d is outside 1..3", dim);
    AMP_REQUIRE(!(g->n_edge_cols == 0 && g->nnz > 0),
                "edge_grad_to_point_sets: the handle has no edge columns: build it with edge ids (DeviceGraph.from_point_sets)");
    AMP_REQUIRE(g->n_with_edge == g->nnz, "edge_grad_to_point_sets: %lld of the handle's %lld entries carry no edge id",
                (long long)(g->nnz - g->n_with_edge), (long long)g->nnz);
    AMP_REQUIRE(want_queries || want_sources, "edge_grad_to_point_sets: dqueries and dsources are both null: nothing to compute");
    return 0;
}

} // namespace amp

// The reverse of athena_mp_radius_pairs_bipartite, coords[e] = q_i - p_j: dqueries[i] = the sum of dcoords over row i in CSR order,
// dsources[j] = acc - dcoords over column j in transposed-CSR order (queries ascending), acc from +0.
extern "C" int athena_mp_edge_grad_to_point_sets(const athena_mp_graph *g, int32_t dim, const float *dcoords_dev, float *dqueries_dev,
                                                 float *dsources_dev)
{
    if (int rc = amp::point_sets_grad_check(g, dim, dqueries_dev != nullptr, dsources_dev != nullptr)) return rc;
    AMP_REQUIRE(g->n_edge_cols == 0 || dcoords_dev != nullptr, "edge_grad_to_point_sets: null dcoords");
    const GeoEdge none = {nullptr, nullptr, nullptr, 0, 1.f};
    if (dqueries_dev && g->n_rows > 0)
        hipLaunchKernelGGL(geo_vertex_gather<kSetRows>, dim3((unsigned)(((int64_t)g->n_rows + kGatherRows - 1) / kGatherRows)), dim3(256), 0,
                           amp::stream(), g->n_rows, (const int32_t *)g->rowptr, (const int32_t *)g->col, (const int32_t *)g->eid, dim,
                           dcoords_dev, none, dqueries_dev, (float *)nullptr, (const int32_t *)nullptr, 0, (const float *)nullptr);
    if (dsources_dev && g->n_cols > 0)
        hipLaunchKernelGGL(geo_vertex_gather<kSetCols>, dim3((unsigned)(((int64_t)g->n_cols + kGatherRows - 1) / kGatherRows)), dim3(256), 0,
                           amp::stream(), g->n_cols, (const int32_t *)g->t_rowptr, (const int32_t *)g->t_src, (const int32_t *)g->t_eid, dim,
                           dcoords_dev, none, dsources_dev, (float *)nullptr, (const int32_t *)nullptr, 0, (const float *)nullptr);
    AMP_LAUNCH_CHECK();
    return 0;
}

extern "C" int athena_mp_edge_grad_to_points(const athena_mp_graph *g, int32_t dim, const float *dcoords_dev, float *dpoints_dev)
{
    if (int rc = amp::points_grad_check(g, dim)) return rc;
    const int32_t n = g->n_rows;
    AMP_REQUIRE((g->n_edge_cols == 0 || dcoords_dev != nullptr) && (n == 0 || dpoints_dev != nullptr), "edge_grad_to_points: null array");
    if (n == 0) return 0;
    const GeoEdge none = {nullptr, nullptr, nullptr, 0, 1.f};
    hipLaunchKernelGGL(geo_vertex_gather<kPoints>, dim3((unsigned)(((int64_t)n + kGatherRows - 1) / kGatherRows)), dim3(256), 0, amp::stream(),
                       n, (const int32_t *)g->rowptr, (const int32_t *)g->col, (const int32_t *)g->eid, dim, dcoords_dev, none, dpoints_dev,
                       (float *)nullptr, (const int32_t *)nullptr, 0, (const float *)nullptr);
    AMP_LAUNCH_CHECK();
    return 0;
}

extern "C" int athena_mp_periodic_grad(const athena_mp_graph *g, int32_t n_structures, int32_t n_atoms, const int32_t *offsets_host,
                                       const int64_t *edge_offsets_host, const float *lat_dev, float cutoff_max, const float *vec_dev,
                                       const float *dfeature_dev, int32_t fe_cols, const float *dvec_dev, float *dcart_dev,
                                       float *dfrac_dev, float *virial_dev, float *dlat_dev)
{
    const int32_t B = n_structures, n = n_atoms;
    if (int rc = amp::periodic_grad_check(g, B, n, offsets_host, edge_offsets_host, cutoff_max, dfeature_dev != nullptr, fe_cols,
                                          dvec_dev != nullptr))
        return rc;
    const int64_t E = g->n_edge_cols;
    AMP_REQUIRE(E == 0 || vec_dev != nullptr, "periodic_grad: null vec");
    AMP_REQUIRE(!((dfrac_dev && n > 0) || (dlat_dev && B > 0)) || lat_dev != nullptr, "periodic_grad: dfrac and dlat need lat");
    hipStream_t st = amp::stream();
    if (dlat_dev && B > 0) {                     // the inverse has to exist: the same fp64 determinant the kernel divides by
        std::vector<float> lat((size_t)9 * B);
        AMP_HIP(hipMemcpyAsync(lat.data(), lat_dev, sizeof(float) * lat.size(), hipMemcpyDeviceToHost, st));
        AMP_HIP(hipStreamSynchronize(st));
        for (int32_t s = 0; s < B; ++s) {
            double L[3][3];
            for (int k = 0; k < 9; ++k) L[k / 3][k % 3] = (double)lat[(size_t)9 * s + k];
            const double *u = L[1], *w = L[2];
            const double det = L[0][0] * (u[1] * w[2] - u[2] * w[1]) + L[0][1] * (u[2] * w[0] - u[0] * w[2]) +
                               L[0][2] * (u[0] * w[1] - u[1] * w[0]);
            AMP_REQUIRE(isfinite(det) && det != 0.0, "periodic_grad: structure %d: det(lat) is zero or not finite: dlat needs the inverse lattice",
                        s + 1);
        }
    }
    const GeoEdge P = {vec_dev, dfeature_dev, dvec_dev, fe_cols, cutoff_max};
    const bool want_virial = (virial_dev || dlat_dev) && B > 0;
    const bool want_gather = (dcart_dev || dfrac_dev) && n > 0;

    // the index tables of this call, uploaded as one array: [offsets B + 1 | item_first B + 1 | items 2 W]
    std::vector<int32_t> table;
    int64_t W = 0;
    if (dfrac_dev) table.insert(table.end(), offsets_host, offsets_host + B + 1);
    const size_t at_first = table.size();
    if (want_virial) {
        table.resize(at_first + (size_t)B + 1);
        std::vector<int32_t> items;
        for (int32_t s = 0; s < B; ++s) {
            table[at_first + s] = (int32_t)(items.size() / 2);
            for (int64_t e = edge_offsets_host[s]; e < edge_offsets_host[s + 1]; e += kItemEdges) {
                items.push_back((int32_t)e);
                items.push_back((int32_t)std::min<int64_t>(e + kItemEdges, edge_offsets_host[s + 1]));
            }
        }
        W = (int64_t)(items.size() / 2);
        table[at_first + B] = (int32_t)W;
        table.insert(table.end(), items.begin(), items.end());
    }
    int32_t *d_table = nullptr;
    if (!table.empty()) {
        void *p = nullptr;
        if (amp::workspace(&p, sizeof(int32_t) * table.size(), kWsTable)) return 1;
        d_table = (int32_t *)p;
        AMP_HIP(hipMemcpyAsync(d_table, table.data(), sizeof(int32_t) * table.size(), hipMemcpyHostToDevice, st));
    }
    if (want_gather) {
        hipLaunchKernelGGL(geo_vertex_gather<kPeriodic>, dim3((unsigned)(((int64_t)n + kGatherRows - 1) / kGatherRows)), dim3(256), 0, st, n,
                           (const int32_t *)g->rowptr, (const int32_t *)g->col, (const int32_t *)g->eid, 3, (const float *)nullptr, P,
                           dcart_dev, dfrac_dev, (const int32_t *)d_table, B, lat_dev);
        AMP_LAUNCH_CHECK();
    }
    if (want_virial) {
        void *p = nullptr;
        if (amp::workspace(&p, sizeof(float) * 9 * (size_t)std::max<int64_t>(W, 1), kWsPartial)) return 1;
        float *partial = (float *)p;
        const int32_t *d_first = d_table + at_first, *d_items = d_first + B + 1;
        if (W > 0)
            hipLaunchKernelGGL(geo_virial_kernel, dim3((unsigned)((W + kVirialWaves - 1) / kVirialWaves)), dim3(64 * kVirialWaves), 0, st,
                               (int32_t)W, d_items, P, partial);
        hipLaunchKernelGGL(geo_virial_finish_kernel, dim3((unsigned)(((int64_t)B + 255) / 256)), dim3(256), 0, st, B, d_first,
                           (const float *)partial, lat_dev, virial_dev, dlat_dev);
        AMP_LAUNCH_CHECK();
    }
    // the tables were read from pageable host memory: the copy has left them when hipMemcpyAsync returns
    return 0;
}
