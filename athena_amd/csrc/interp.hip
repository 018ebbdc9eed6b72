// Inverse-distance interpolation over a two-set graph, with its gradients: the step that carries features from the coarse set back
// to the fine one (PointNet++ feature propagation, the skip path of a U-shaped operator, k-nearest-neighbour interpolation), and
// under it a gather over a handle's CSR with caller-supplied per-edge weights, forward and transposed.
//
// The definition (include/athena_mp.h holds the same text; tests/interp_reference.py is its numpy transcription).  All arithmetic
// is fp32, every operation rounded on its own (-ffp-contract=off, correctly rounded /), subnormals kept.  g is a rectangular handle
// of athena_mp_graph_create_bipartite_dev, coords [E, dim] what its builder wrote (coords[e] = q_i - p_j).  Row i is the forward CSR
// (rowptr, col, eid), column j the transposed one (t_rowptr, t_src, t_eid; queries ascending); those orders are the summation orders.
//
//   weights:     s_e = ((d0 d0) + d1 d1) + d2 d2 (the builder's own sqdist);  w_e = 1 / m_e, m_e = eps where s_e <= eps, else s_e (an
//                s that overflowed gives w = +0);  W_i = +0, then W_i = W_i + w_eid[k] in row order;  weights[e] = w_e / W_i, +0 for
//                every edge of a row whose W_i is 0;  wsum[i] = W_i.
//   fwd:         y[i, f]  = acc, acc = +0, then acc = acc + weights[eid[k]] * x[col[k], f] in row order
//   bwd_x:       dx[j, f] = acc, acc = +0, then acc = acc + weights[t_eid[k]] * dy[t_src[k], f] in column order
//   bwd_coords:  e = (i, j):  g_e = sum_f dy[i, f] * (x[j, f] - y[i, f]) (order free);  t_e = -(weights[e] * w_e) * g_e;
//                dcoords[e, c] = (2 d_c) * t_e;  exactly +0 where s_e <= eps (the clamp) or w_e = 0.
//
// How.  The lane groups of row_groups.h.  interp_gather_kernel is the hot launch, one template for fwd and bwd_x: the group's lanes
// load the column id and the weight of G entries, and every lane adds its own four feature columns in entry order: the sequential
// sum, bit for bit, the same sequence of operations on either load route (a lane past its row's end selects its old sum).
// interp_weights_kernel: eight lanes per row, w_e formed where it is used, the row sum in entry order through the group.
// interp_bwd_coords_kernel: the same groups over the rows, y[i] and dy[i] held in registers; each entry's dot over f is per-lane
// partials over four adjacent columns (16 bytes a load on the same condition) folded by a fixed __shfl_xor tree, and the lane that
// loaded an entry finishes its edge.  It keeps the row set-up and its columns written out, and the gather its columns: through
// the helpers of row_groups.h their register counts moved (profiles/row_groups_isa.txt).
// One entry per edge column is what all of this rests on (athena_mp_graph_create_bipartite_dev builds exactly that): every
// weights[e] and dcoords[e, :] then has one writer.
#include <math.h>

#include "common.h"
#include "row_groups.h"

namespace {

constexpr int kWeightGroup = 8;                 // lanes that share a row of the weights kernel

// d = coords[e, :] (absent components 0) and s_e
__device__ __forceinline__ float interp_sqdist(const float *__restrict__ coords, int64_t e, int32_t dim, float &d0, float &d1, float &d2)
{
    const float *c = coords + e * dim;
    d0 = c[0];
    d1 = dim > 1 ? c[1] : 0.f;
    d2 = dim > 2 ? c[2] : 0.f;
    return ((d0 * d0) + d1 * d1) + d2 * d2;
}

__device__ __forceinline__ float interp_raw_weight(const float *__restrict__ coords, int64_t e, int32_t dim, float eps)
{
    float d0, d1, d2;
    const float s = interp_sqdist(coords, e, dim, d0, d1, d2);
    return 1.f / (s <= eps ? eps : s);
}

__global__ __launch_bounds__(256) void interp_weights_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ eid,
                                                             int32_t dim, const float *__restrict__ coords, float eps,
                                                             float *__restrict__ weights, float *__restrict__ wsum)
{
    constexpr int G = kWeightGroup;
    const amp::RowGroup<G> rg(n, rowptr);
    float W = 0.f, w_first = 0.f;
    for (int32_t k0 = 0; k0 < rg.longest; k0 += G) {                // the per-lane bound: with rg.rounds this kernel's registers move
        float w = 0.f;
        if (k0 + rg.sub < rg.len) w = interp_raw_weight(coords, eid[(int64_t)rg.beg + k0 + rg.sub], dim, eps);
        if (k0 == 0) w_first = w;
#pragma unroll
        for (int j = 0; j < G; ++j) {                               // entry order: k0, k0 + 1, ...
            const float s = __shfl(w, rg.first + j);
            if (k0 + j < rg.len) W = W + s;
        }
    }
    if (rg.row >= n) return;
    if (wsum && rg.sub == 0) wsum[rg.row] = W;
    for (int32_t k = rg.sub; k < rg.len; k += G) {
        const int64_t e = eid[(int64_t)rg.beg + k];
        const float w = k < G ? w_first : interp_raw_weight(coords, e, dim, eps);
        weights[e] = W == 0.f ? 0.f : w / W;
    }
}

// out[r, :] = the weighted sum over row r of (rowptr, idx, eid): G lanes per row, four columns per lane and pass
template <int G, bool VEC>
__global__ __launch_bounds__(256) void interp_gather_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ idx,
                                                            const int32_t *__restrict__ eid, const float *__restrict__ weights,
                                                            const float *__restrict__ x, float *__restrict__ out, int32_t F)
{
    const amp::RowGroup<G> rg(n, rowptr);
    for (int32_t f0 = 0; f0 < F; f0 += 4 * G) {
        // written out: through LaneColumns this kernel's register allocation moves (profiles/row_groups_isa.txt)
        int32_t colv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) colv[a] = VEC ? f0 + 4 * rg.sub + a : f0 + rg.sub + G * a;
        const int32_t at4 = min(colv[0], F - 4);                    // VEC only: F >= 4 there
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int32_t k0 = 0; k0 < rg.rounds; k0 += G) {
            int32_t c = 0;
            float w = 0.f;
            if (k0 + rg.sub < rg.len) {
                const int64_t k = (int64_t)rg.beg + k0 + rg.sub;
                c = idx[k];
                w = weights[eid[k]];
            }
            const int nj = min(G, rg.rounds - k0);
            for (int j0 = 0; j0 < nj; j0 += 4)                      // four entries a step (G is a multiple of 4): their loads fly together
#pragma unroll
            for (int j = j0; j < j0 + 4; ++j) {                     // entry order: k0, k0 + 1, ...
                const int32_t cj = __shfl(c, rg.first + j);
                const float wj = __shfl(w, rg.first + j);
                const float *src = x + (int64_t)cj * F;
                float v[4];
                if (VEC) {
                    const float4 q = *reinterpret_cast<const float4 *>(src + at4);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                } else {
#pragma unroll
                    for (int a = 0; a < 4; ++a) v[a] = src[min(colv[a], F - 1)];
                }
                const bool use = k0 + j < rg.len;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const float sum = acc[a] + wj * v[a];
                    acc[a] = use ? sum : acc[a];
                }
            }
        }
        if (rg.row < n) {
            float *dst = out + rg.row * F;
            if (VEC) {
                if (colv[0] < F) *reinterpret_cast<float4 *>(dst + colv[0]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            } else {
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    if (colv[a] < F) dst[colv[a]] = acc[a];
            }
        }
    }
}

// dcoords of the edges of one row per lane group, G lanes and four columns per lane as in the gather.  The group keeps its slice of
// y[i] and dy[i] in registers; the entries go round by __shfl, four a step so that their x rows are in flight together; each entry's
// dot over f is per-lane partials -- columns 4 sub .. 4 sub + 3, then those 4 G further on, in that order on both load routes --
// folded by a fixed __shfl_xor tree, and lane j of the group keeps the dot of entry j and finishes that edge: one order of the sum
// per F, wherever the operands lie.
template <int G, bool VEC>
__global__ __launch_bounds__(256) void interp_bwd_coords_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ idx,
                                                                const int32_t *__restrict__ eid, int32_t dim, int32_t F,
                                                                const float *__restrict__ coords, float eps, const float *__restrict__ weights,
                                                                const float *__restrict__ x, const float *__restrict__ y,
                                                                const float *__restrict__ dy, float *__restrict__ dcoords)
{
    constexpr int kRows = 256 / G;
    const int lane = threadIdx.x & 63;
    const int sub = lane & (G - 1), first = lane & ~(G - 1);
    const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x / G;
    int32_t beg = 0, len = 0;
    if (row < n) {
        beg = rowptr[row];
        len = rowptr[row + 1] - beg;
    }
    int32_t rounds = len;
#pragma unroll
    for (int o = 32; o >= G; o >>= 1) rounds = max(rounds, __shfl_xor(rounds, o));
    rounds = __builtin_amdgcn_readfirstlane(rounds);
    // this lane's first four columns: a column past F is read at the last valid place and its term is dropped
    const int32_t own = 4 * sub;
    int32_t at[4];
    bool has[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        has[a] = own + a < F;
        at[a] = VEC ? min(own, F - 4) + a : min(own + a, F - 1);
    }
    float yv[4] = {0.f, 0.f, 0.f, 0.f}, dv[4] = {0.f, 0.f, 0.f, 0.f};
    const float *yr = y + row * F, *dr = dy + row * F;
    if (len > 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) yv[a] = yr[at[a]], dv[a] = dr[at[a]];
    }
    for (int32_t k0 = 0; k0 < rounds; k0 += G) {
        int32_t c = 0;
        int64_t e = 0;
        if (k0 + sub < len) {
            const int64_t k = (int64_t)beg + k0 + sub;
            c = idx[k];
            e = eid[k];
        }
        float mine = 0.f;                                           // g_e of this lane's own entry, k0 + sub
        const int nj = min(G, rounds - k0);
        for (int j0 = 0; j0 < nj; j0 += 4)
#pragma unroll
        for (int j = j0; j < j0 + 4; ++j) {
            const float *xr = x + (int64_t)__shfl(c, first + j) * F;
            float xv[4];
            if (VEC) {
                const float4 q = *reinterpret_cast<const float4 *>(xr + at[0]);
                xv[0] = q.x, xv[1] = q.y, xv[2] = q.z, xv[3] = q.w;
            } else {
#pragma unroll
                for (int a = 0; a < 4; ++a) xv[a] = xr[at[a]];
            }
            float part = 0.f;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const float sum = part + dv[a] * (xv[a] - yv[a]);
                part = has[a] ? sum : part;
            }
            if (k0 + j < len)                                       // beyond 4 G columns: the further passes, from memory
                for (int32_t f = own + 4 * G; f < F; f += 4 * G)
                    for (int32_t a = f; a < min(f + 4, F); ++a) part = part + dr[a] * (xr[a] - yr[a]);
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) part = part + __shfl_xor(part, o);
            if (sub == j) mine = part;
        }
        if (k0 + sub < len) {
            float d0, d1, d2, r0 = 0.f, r1 = 0.f, r2 = 0.f;
            const float s = interp_sqdist(coords, e, dim, d0, d1, d2);
            if (!(s <= eps)) {
                const float w = 1.f / s;
                if (w != 0.f) {
                    const float t = -(weights[e] * w) * mine;
                    r0 = (2.f * d0) * t;
                    r1 = (2.f * d1) * t;
                    r2 = (2.f * d2) * t;
                }
            }
            float *dst = dcoords + e * dim;
            dst[0] = r0;
            if (dim > 1) dst[1] = r1;
            if (dim > 2) dst[2] = r2;
        }
    }
}

// out [n, F] over one CSR of the handle; the 16-byte route needs whole float4 columns and both arrays on a 16-byte boundary
int weighted_gather(int32_t n, const int32_t *rowptr, const int32_t *idx, const int32_t *eid, const float *weights, const float *x,
                    float *out, int32_t F)
{
    if (n == 0) return 0;
    const int G = amp::group_width(F);
    amp::dispatch_group(G, F % 4 == 0 && amp::aligned16(x, out), [&](auto g, auto v) {
        hipLaunchKernelGGL((interp_gather_kernel<g(), v()>), amp::group_grid(n, G), dim3(256), 0, amp::stream(), n, rowptr, idx, eid, weights,
                           x, out, F);
    });
    AMP_LAUNCH_CHECK();
    return 0;
}

} // namespace

namespace amp {

int edge_form_check(const char *who, const athena_mp_graph *g)
{
    AMP_REQUIRE(g != nullptr, "%s: null graph handle", who);
    AMP_REQUIRE(!(g->n_edge_cols == 0 && g->nnz > 0),
                "%s: the handle has no edge columns: build it with edge ids (DeviceGraph.from_point_sets, from_point_sets_knn)", who);
    AMP_REQUIRE(g->n_with_edge == g->nnz, "%s: %lld of the handle's %lld entries carry no edge id", who,
                (long long)(g->nnz - g->n_with_edge), (long long)g->nnz);
    AMP_REQUIRE(g->nnz == (int64_t)g->n_edge_cols, "%s: %lld entries over %d edge columns: need one entry per edge column, as athena_mp_graph_create_bipartite_dev builds it",
                who, (long long)g->nnz, g->n_edge_cols);
    return 0;
}

int interp_check(const char *who, const athena_mp_graph *g, const int32_t *dim, const int32_t *F, const float *eps)
{
    if (int rc = edge_form_check(who, g)) return rc;
    AMP_REQUIRE(dim == nullptr || (*dim >= 1 && *dim <= 3), "%s: dim = %d is outside 1..3", who, dim ? *dim : 0);
    AMP_REQUIRE(F == nullptr || *F >= 1, "%s: F = %d: need at least one feature column", who, F ? *F : 0);
    AMP_REQUIRE(eps == nullptr || (isfinite(*eps) && *eps >= 0x1p-60f), "%s: eps = %g: need a finite value of at least 2^-60", who,
                eps ? (double)*eps : 0.0);
    return 0;
}

} // namespace amp

extern "C" int athena_mp_interp_weights(const athena_mp_graph *g, int32_t dim, const float *coords_dev, float eps, float *weights_dev,
                                        float *wsum_dev)
{
    if (int rc = amp::interp_check("interp_weights", g, &dim, nullptr, &eps)) return rc;
    AMP_REQUIRE(g->n_edge_cols == 0 || (coords_dev != nullptr && weights_dev != nullptr), "interp_weights: null array");
    if (g->n_rows == 0) return 0;
    hipLaunchKernelGGL(interp_weights_kernel, amp::group_grid(g->n_rows, kWeightGroup), dim3(256), 0, amp::stream(), g->n_rows,
                       (const int32_t *)g->rowptr, (const int32_t *)g->eid, dim, coords_dev, eps, weights_dev, wsum_dev);
    AMP_LAUNCH_CHECK();
    return 0;
}

extern "C" int athena_mp_interp_fwd(const athena_mp_graph *g, int32_t F, const float *weights_dev, const float *x_dev, float *y_dev)
{
    if (int rc = amp::interp_check("interp_fwd", g, nullptr, &F, nullptr)) return rc;
    AMP_REQUIRE((g->n_edge_cols == 0 || (weights_dev != nullptr && x_dev != nullptr)) && (g->n_rows == 0 || y_dev != nullptr),
                "interp_fwd: null array");
    return weighted_gather(g->n_rows, g->rowptr, g->col, g->eid, weights_dev, x_dev, y_dev, F);
}

extern "C" int athena_mp_interp_bwd_x(const athena_mp_graph *g, int32_t F, const float *weights_dev, const float *dy_dev, float *dx_dev)
{
    if (int rc = amp::interp_check("interp_bwd_x", g, nullptr, &F, nullptr)) return rc;
    AMP_REQUIRE((g->n_edge_cols == 0 || (weights_dev != nullptr && dy_dev != nullptr)) && (g->n_cols == 0 || dx_dev != nullptr),
                "interp_bwd_x: null array");
    return weighted_gather(g->n_cols, g->t_rowptr, g->t_src, g->t_eid, weights_dev, dy_dev, dx_dev, F);
}

extern "C" int athena_mp_interp_bwd_coords(const athena_mp_graph *g, int32_t dim, int32_t F, const float *coords_dev, float eps,
                                           const float *weights_dev, const float *x_dev, const float *y_dev, const float *dy_dev,
                                           float *dcoords_dev)
{
    if (int rc = amp::interp_check("interp_bwd_coords", g, &dim, &F, &eps)) return rc;
    if (g->n_edge_cols == 0) return 0;
    AMP_REQUIRE(coords_dev && weights_dev && x_dev && y_dev && dy_dev && dcoords_dev, "interp_bwd_coords: null array");
    const int G = amp::group_width(F);
    amp::dispatch_group(G, F % 4 == 0 && amp::aligned16(x_dev, y_dev, dy_dev), [&](auto gw, auto v) {
        hipLaunchKernelGGL((interp_bwd_coords_kernel<gw(), v()>), amp::group_grid(g->n_rows, G), dim3(256), 0, amp::stream(), g->n_rows,
                           (const int32_t *)g->rowptr, (const int32_t *)g->col, (const int32_t *)g->eid, dim, F, coords_dev, eps,
                           weights_dev, x_dev, y_dev, dy_dev, dcoords_dev);
    });
    AMP_LAUNCH_CHECK();
    return 0;
}
