// Max pooling over a handle's rows, with its arg-max and both reverse steps: the reduction of PointNet++'s set abstraction (an MLP on
// every (sample, neighbour) pair, then the maximum over the neighbours), of EdgeConv / DGCNN and of GraphSAGE-pool, over the CSR the
// builders leave in HBM.  Nothing is computed on the values: they are compared and copied, so every output is bit-defined.
//
// The definition (include/athena_mp.h holds the same text; tests/pool_reference.py is its numpy transcription).  g is any handle; row i
// is its forward CSR (rowptr, col, eid), column j its transposed one (t_rowptr, t_src, t_eid; rows ascending).  Values are fp32.
//
//   fwd:        for k = rowptr[i] .. in order, v = x[col[k], f] (vertex form) or h[eid[k], f] (edge form): entry k replaces the best so
//               far when there is none yet, or v > best, or v is a NaN and best is not.  y[i, f] = the bits of the chosen value, arg[i, f]
//               = its col[k]; an empty row gives y = +0, arg = -1.  So the first maximum in row order wins, of +0 and -0 the earlier
//               one stays, a NaN wins over every number and the first NaN stays.
//   bwd_x:      dx[j, f] = acc, acc = +0, then for k = t_rowptr[j] .. in order, i = t_src[k]: acc = acc + dy[i, f] where arg[i, f] == j
//   bwd_edges:  the entry k of row i, e = eid[k], j = col[k]: dh[e, f] = dy[i, f] where arg[i, f] == j, else +0
//
// How.  The lane groups of row_groups.h.  pool_fwd_kernel: every lane keeps the best value and its column for its own four feature
// columns: a compare and two selects per column, the chosen value's bits untouched (a select, not a max instruction, which would quiet a
// signalling NaN and may pick either zero).  The 16-byte route needs the arg rows on a 16-byte boundary too.  pool_bwd_x_kernel: the
// same groups over the transposed CSR, each entry loading the group's slice of arg[i] and dy[i].  pool_bwd_edges_kernel: the groups over
// the rows with the slices of arg[i] and dy[i] in registers and one store of dh[e, ..] per entry; one entry per edge column is what
// makes every dh[e, :] written exactly once.
#include "common.h"
#include "row_groups.h"

namespace {

// y[r, :], arg[r, :] = the first maximum over row r of (rowptr, col) and its column; the value's row is col[k] (vertex form) or eid[k]
template <int G, bool VEC, bool EDGE>
__global__ __launch_bounds__(256) void pool_fwd_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                       const int32_t *__restrict__ eid, const float *__restrict__ x, float *__restrict__ y,
                                                       int32_t *__restrict__ arg, int32_t F)
{
    const amp::RowGroup<G> rg(n, rowptr);
    for (int32_t f0 = 0; f0 < F; f0 += 4 * G) {
        // written out: through LaneColumns the encoder's forward at F = 128 ran 0.6 - 1.0 % slower (profiles/row_groups_ab.txt)
        int32_t colv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) colv[a] = VEC ? f0 + 4 * rg.sub + a : f0 + rg.sub + G * a;
        const int32_t at4 = min(colv[0], F - 4);                    // VEC only: F >= 4 there
        float best[4] = {0.f, 0.f, 0.f, 0.f};
        int32_t barg[4] = {-1, -1, -1, -1};
        for (int32_t k0 = 0; k0 < rg.rounds; k0 += G) {
            int32_t c = 0, s = 0;
            if (k0 + rg.sub < rg.len) {
                const int64_t k = (int64_t)rg.beg + k0 + rg.sub;
                c = col[k];
                s = EDGE ? eid[k] : c;
            }
            const int nj = min(G, rg.rounds - k0);
            for (int j0 = 0; j0 < nj; j0 += 4)                      // four entries a step (G is a multiple of 4): their loads fly together
#pragma unroll
            for (int j = j0; j < j0 + 4; ++j) {                     // entry order: k0, k0 + 1, ...
                const int32_t cj = __shfl(c, rg.first + j);
                const int32_t sj = EDGE ? __shfl(s, rg.first + j) : cj;
                const float *src = x + (int64_t)sj * F;
                float v[4];
                if (VEC) {
                    const float4 q = *reinterpret_cast<const float4 *>(src + at4);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                } else {
#pragma unroll
                    for (int a = 0; a < 4; ++a) v[a] = src[min(colv[a], F - 1)];
                }
                const bool use = k0 + j < rg.len, none = k0 + j == 0;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const bool take = use && (none || v[a] > best[a] || (v[a] != v[a] && best[a] == best[a]));
                    best[a] = take ? v[a] : best[a];
                    barg[a] = take ? cj : barg[a];
                }
            }
        }
        if (rg.row < n) {
            float *dst = y + rg.row * F;
            int32_t *adst = arg ? arg + rg.row * F : nullptr;
            if (VEC) {
                if (colv[0] < F) {
                    *reinterpret_cast<float4 *>(dst + colv[0]) = make_float4(best[0], best[1], best[2], best[3]);
                    if (adst) *reinterpret_cast<int4 *>(adst + colv[0]) = make_int4(barg[0], barg[1], barg[2], barg[3]);
                }
            } else {
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    if (colv[a] < F) {
                        dst[colv[a]] = best[a];
                        if (adst) adst[colv[a]] = barg[a];
                    }
            }
        }
    }
}

// dx[r, :] = the sum of dy[i, :] over the entries i of column r of the handle (t_rowptr, t_src), rows ascending, where arg[i, :] == r
template <int G, bool VEC>
__global__ __launch_bounds__(256) void pool_bwd_x_kernel(int32_t n, const int32_t *__restrict__ t_rowptr, const int32_t *__restrict__ t_src,
                                                         const int32_t *__restrict__ arg, const float *__restrict__ dy,
                                                         float *__restrict__ dx, int32_t F)
{
    const amp::RowGroup<G> rg(n, t_rowptr);
    const int32_t me = (int32_t)rg.row;                             // the column this group sums for: what arg must name
    for (int32_t f0 = 0; f0 < F; f0 += 4 * G) {
        // written out: through LaneColumns this kernel's register allocation moves (profiles/row_groups_isa.txt)
        int32_t colv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) colv[a] = VEC ? f0 + 4 * rg.sub + a : f0 + rg.sub + G * a;
        const int32_t at4 = min(colv[0], F - 4);                    // VEC only: F >= 4 there
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int32_t k0 = 0; k0 < rg.rounds; k0 += G) {
            int32_t i = 0;
            if (k0 + rg.sub < rg.len) i = t_src[(int64_t)rg.beg + k0 + rg.sub];
            const int nj = min(G, rg.rounds - k0);
            for (int j0 = 0; j0 < nj; j0 += 4)
#pragma unroll
            for (int j = j0; j < j0 + 4; ++j) {
                const int64_t at = (int64_t)__shfl(i, rg.first + j) * F;
                int32_t w[4];
                float d[4];
                if (VEC) {
                    const int4 qa = *reinterpret_cast<const int4 *>(arg + at + at4);
                    const float4 qd = *reinterpret_cast<const float4 *>(dy + at + at4);
                    w[0] = qa.x, w[1] = qa.y, w[2] = qa.z, w[3] = qa.w;
                    d[0] = qd.x, d[1] = qd.y, d[2] = qd.z, d[3] = qd.w;
                } else {
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const int32_t f = min(colv[a], F - 1);
                        w[a] = arg[at + f];
                        d[a] = dy[at + f];
                    }
                }
                const bool use = k0 + j < rg.len;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const float sum = acc[a] + d[a];
                    acc[a] = use && w[a] == me ? sum : acc[a];
                }
            }
        }
        if (rg.row < n) {
            float *dst = dx + rg.row * F;
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

// dh[eid[k], :] = dy[r, :] where arg[r, :] == col[k], else +0, for the entries k of row r: the group holds its slice of arg[r] and dy[r]
template <int G, bool VEC>
__global__ __launch_bounds__(256) void pool_bwd_edges_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                             const int32_t *__restrict__ eid, const int32_t *__restrict__ arg,
                                                             const float *__restrict__ dy, float *__restrict__ dh, int32_t F)
{
    const amp::RowGroup<G> rg(n, rowptr);
    for (int32_t f0 = 0; f0 < F; f0 += 4 * G) {
        const amp::LaneColumns<G, VEC> cols(rg.sub, f0, F);
        int32_t w[4] = {-1, -1, -1, -1};
        float d[4] = {0.f, 0.f, 0.f, 0.f};
        if (rg.len > 0) cols.load4(arg + rg.row * F, w, dy + rg.row * F, d);   // an empty row has no entry to write for
        for (int32_t k0 = 0; k0 < rg.rounds; k0 += G) {
            int32_t c = 0, e = 0;
            if (k0 + rg.sub < rg.len) {
                const int64_t k = (int64_t)rg.beg + k0 + rg.sub;
                c = col[k];
                e = eid[k];
            }
            const int nj = min(G, rg.rounds - k0);
            for (int j = 0; j < nj; ++j) {                          // entry order, though each dh row has one writer
                const int32_t cj = __shfl(c, rg.first + j);
                const int32_t ej = __shfl(e, rg.first + j);
                if (k0 + j < rg.len) {
                    float out[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) out[a] = w[a] == cj ? d[a] : 0.f;
                    cols.store4(dh + (int64_t)ej * F, out);
                }
            }
        }
    }
}

// the forward of both forms: src names the rows of `values` (col for x, eid for h)
template <bool EDGE>
int pool_forward(const athena_mp_graph *g, int32_t F, const float *values, float *y, int32_t *arg)
{
    if (g->n_rows == 0) return 0;
    const int G = amp::group_width(F);
    amp::dispatch_group(G, F % 4 == 0 && amp::aligned16(values, y) && amp::aligned16(arg), [&](auto gw, auto v) {
        hipLaunchKernelGGL((pool_fwd_kernel<gw(), v(), EDGE>), amp::group_grid(g->n_rows, G), dim3(256), 0, amp::stream(), g->n_rows,
                           (const int32_t *)g->rowptr, (const int32_t *)g->col, (const int32_t *)g->eid, values, y, arg, F);
    });
    AMP_LAUNCH_CHECK();
    return 0;
}

} // namespace

namespace amp {

// what every entry checks first; the edge forms need one entry per edge column
int pool_check(const char *who, const athena_mp_graph *g, int32_t F, bool edge_form)
{
    if (edge_form) {
        if (int rc = edge_form_check(who, g)) return rc;
    } else {
        AMP_REQUIRE(g != nullptr, "%s: null graph handle", who);
    }
    AMP_REQUIRE(F >= 1, "%s: F = %d: need at least one feature column", who, F);
    return 0;
}

} // namespace amp

extern "C" int athena_mp_pool_max_fwd(const athena_mp_graph *g, int32_t F, const float *x_dev, float *y_dev, int32_t *arg_dev)
{
    if (int rc = amp::pool_check("pool_max_fwd", g, F, false)) return rc;
    AMP_REQUIRE((g->nnz == 0 || x_dev != nullptr) && (g->n_rows == 0 || y_dev != nullptr), "pool_max_fwd: null array");
    return pool_forward<false>(g, F, x_dev, y_dev, arg_dev);
}

extern "C" int athena_mp_pool_max_edges_fwd(const athena_mp_graph *g, int32_t F, const float *h_dev, float *y_dev, int32_t *arg_dev)
{
    if (int rc = amp::pool_check("pool_max_edges_fwd", g, F, true)) return rc;
    AMP_REQUIRE((g->nnz == 0 || h_dev != nullptr) && (g->n_rows == 0 || y_dev != nullptr), "pool_max_edges_fwd: null array");
    return pool_forward<true>(g, F, h_dev, y_dev, arg_dev);
}

extern "C" int athena_mp_pool_max_bwd_x(const athena_mp_graph *g, int32_t F, const int32_t *arg_dev, const float *dy_dev, float *dx_dev)
{
    if (int rc = amp::pool_check("pool_max_bwd_x", g, F, false)) return rc;
    AMP_REQUIRE((g->nnz == 0 || (arg_dev != nullptr && dy_dev != nullptr)) && (g->n_cols == 0 || dx_dev != nullptr),
                "pool_max_bwd_x: null array");
    if (g->n_cols == 0) return 0;
    const int G = amp::group_width(F);
    amp::dispatch_group(G, F % 4 == 0 && amp::aligned16(dy_dev, dx_dev) && amp::aligned16(arg_dev), [&](auto gw, auto v) {
        hipLaunchKernelGGL((pool_bwd_x_kernel<gw(), v()>), amp::group_grid(g->n_cols, G), dim3(256), 0, amp::stream(), g->n_cols,
                           (const int32_t *)g->t_rowptr, (const int32_t *)g->t_src, arg_dev, dy_dev, dx_dev, F);
    });
    AMP_LAUNCH_CHECK();
    return 0;
}

extern "C" int athena_mp_pool_max_bwd_edges(const athena_mp_graph *g, int32_t F, const int32_t *arg_dev, const float *dy_dev, float *dh_dev)
{
    if (int rc = amp::pool_check("pool_max_bwd_edges", g, F, true)) return rc;
    if (g->nnz == 0) return 0;                                      // no entry, so no edge column either: dh is empty
    AMP_REQUIRE(arg_dev != nullptr && dy_dev != nullptr && dh_dev != nullptr, "pool_max_bwd_edges: null array");
    const int G = amp::group_width(F);
    amp::dispatch_group(G, F % 4 == 0 && amp::aligned16(dy_dev, dh_dev) && amp::aligned16(arg_dev), [&](auto gw, auto v) {
        hipLaunchKernelGGL((pool_bwd_edges_kernel<gw(), v()>), amp::group_grid(g->n_rows, G), dim3(256), 0, amp::stream(), g->n_rows,
                           (const int32_t *)g->rowptr, (const int32_t *)g->col, (const int32_t *)g->eid, arg_dev, dy_dev, dh_dev, F);
    });
    AMP_LAUNCH_CHECK();
    return 0;
}
