// Attention pooling over a handle's rows: a softmax over each row's entries, per head, then the weighted sum of per-vertex or per-edge
// values with the weight chosen per head, and every reverse step -- the third reduction over a neighbourhood beside the weighted sum
// with one scalar per edge (interp.hip) and the maximum (pool.hip): Point Transformer's vector attention, GAT-style set abstraction,
// the attention kernels of transformer neural operators over a mesh and a latent set.
//
// The definition (include/athena_mp.h holds the same text; tests/attention_reference.py is its numpy transcription).  g is a handle
// with one entry per edge column; row i is the forward CSR (rowptr, col, eid), column j the transposed one (t_rowptr, t_src, t_eid;
// queries ascending).  H >= 1 heads, F >= 1, F % H == 0, C = F / H; the head of feature column c is c / C.  Everything is fp32, every
// operation rounded on its own (-ffp-contract=off, correctly rounded /).
//
//   softmax_fwd:  scores [E, H] -> alpha [E, H].  Row i, head h, over the entries k in CSR order, e = eid[k]: m = the maximum of
//                 scores[e, h];  p_k = exp(scores[e, h] - m);  S = p_0 + p_1 + ... in CSR order;  alpha[e, h] = p_k / S.  A -inf beside
//                 a finite maximum gives exactly +0; a (row, head) whose scores hold a NaN or a +inf, or only -inf, is NaN in all of its
//                 entries and no other (row, head) is touched; a row of one finite entry gives exactly 1; an empty row writes nothing.
//                 exp is the expf of the softmax in elementwise.hip.
//   gather_fwd:   y[i, c] = acc, acc = +0, then acc = acc + alpha[eid[k], c / C] * v in row order, v = x[col[k], c] (vertex form) or
//                 h[eid[k], c] (edge form): bit for bit the sequential sum, an empty row +0; at H = 1 the bytes of athena_mp_interp_fwd.
//   bwd_x:        dx[j, c] = acc, acc = +0, then acc = acc + alpha[t_eid[k], c / C] * dy[t_src[k], c] in column order
//   bwd_edges:    dh[e, c] = alpha[e, c / C] * dy[i, c], one store per entry
//   bwd_alpha:    dalpha[e, h] = the sum over the C columns c of head h of dy[i, c] * v[., c]; the order of this sum is the
//                 implementation's (below); at C = 1 it is the product itself
//   softmax_bwd:  dot = +0, then dot = dot + alpha[e, h] * dalpha[e, h] in row order;  dscores[e, h] = alpha[e, h] * (dalpha[e, h] - dot)
//
// How.  The lane groups of row_groups.h; no LDS, no atomics, no scratch.  The softmax kernels run the groups over the H columns of
// scores (group width from H): three sweeps over a row in entry order -- maximum, sum, write --, the reverse two.  attn_gather_kernel
// is interp_gather_kernel's scheme with the weight chosen per column, one template for the vertex form, the edge form and bwd_x.  Two
// load routes with the same bytes (16 bytes a lane when F % 4 == 0 and the arrays start on 16-byte boundaries, else 4), and on the
// 16-byte route two weight fast paths, the same bytes again: one weight load per entry where a lane's four columns share a head
// (C % 4 == 0), one 16-byte load of four weights where H == F.  attn_row_times_kernel writes a row's dy times a per-entry factor:
// bwd_edges (the factor is alpha by head) and bwd_alpha at C = 1 (the factor is the value row: no reduction).  bwd_alpha with C a
// multiple of 4 and C / 4 a power of two that fits a group: every lane adds its own four terms in column order, then a fixed
// __shfl_xor tree over the C / 4 lanes of a head -- lanes own columns 4 sub .. 4 sub + 3 on both load routes, so one order per (F, H).
// Any other C: one lane per (edge, head) walks its C columns in order.
#include "common.h"
#include "row_groups.h"

namespace {

// how a gather lane reads: 0 four bytes at a time, a weight per column; 1 sixteen bytes, a weight per column; 2 sixteen bytes, the
// lane's four columns share a head: one weight; 3 sixteen bytes, H == F: the four weights in one load
constexpr int kScalar = 0, kVecPerColumn = 1, kVecOneHead = 2, kVecFourHeads = 3;

// the weights of this lane's four columns for the entry whose weight row is `ar`
template <int G, int ROUTE>
__device__ __forceinline__ void lane_weights(const amp::LaneColumns<G, ROUTE != kScalar> &cols, const int32_t (&head)[4],
                                             const float *__restrict__ ar, float (&w)[4])
{
    if (ROUTE == kVecFourHeads) {
        cols.load4(ar, w);
    } else if (ROUTE == kVecOneHead) {
        w[0] = w[1] = w[2] = w[3] = ar[head[0]];
    } else {
#pragma unroll
        for (int a = 0; a < 4; ++a) w[a] = ar[head[a]];
    }
}

// alpha[e, :] over the entries of each row, per head: the groups run over the H columns of scores
template <int G, bool VEC>
__global__ __launch_bounds__(256) void attn_softmax_fwd_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ eid,
                                                               const float *__restrict__ scores, float *__restrict__ alpha, int32_t H)
{
    const amp::RowGroup<G> rg(n, rowptr);
    for (int32_t f0 = 0; f0 < H; f0 += 4 * G) {
        const amp::LaneColumns<G, VEC> cols(rg.sub, f0, H);
        float m[4], S[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < 4; ++a) m[a] = -__builtin_inff();
        for (int sweep = 0; sweep < 3; ++sweep)                     // the maximum, the sum, the quotients: each in entry order
        for (int32_t k0 = 0; k0 < rg.rounds; k0 += G) {
            int32_t e = 0;
            if (k0 + rg.sub < rg.len) e = eid[(int64_t)rg.beg + k0 + rg.sub];
            const int nj = min(G, rg.rounds - k0);
            for (int j0 = 0; j0 < nj; j0 += 4)                      // four entries a step (G is a multiple of 4): their loads fly together
#pragma unroll
            for (int j = j0; j < j0 + 4; ++j) {                     // entry order: k0, k0 + 1, ...
                const int32_t ej = __shfl(e, rg.first + j);
                float v[4];
                cols.load4(scores + (int64_t)ej * H, v);
                const bool use = k0 + j < rg.len;
                if (sweep == 0) {
#pragma unroll
                    for (int a = 0; a < 4; ++a) m[a] = use && v[a] > m[a] ? v[a] : m[a];   // a NaN is never taken: it turns up in p
                } else if (sweep == 1) {
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const float sum = S[a] + expf(v[a] - m[a]);
                        S[a] = use ? sum : S[a];
                    }
                } else if (use) {
                    float out[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) out[a] = expf(v[a] - m[a]) / S[a];
                    cols.store4(alpha + (int64_t)ej * H, out);
                }
            }
        }
    }
}

// dscores[e, :] = alpha (dalpha - dot), dot the row's sum of alpha dalpha in entry order
template <int G, bool VEC>
__global__ __launch_bounds__(256) void attn_softmax_bwd_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ eid,
                                                               const float *__restrict__ alpha, const float *__restrict__ dalpha,
                                                               float *__restrict__ dscores, int32_t H)
{
    const amp::RowGroup<G> rg(n, rowptr);
    for (int32_t f0 = 0; f0 < H; f0 += 4 * G) {
        const amp::LaneColumns<G, VEC> cols(rg.sub, f0, H);
        float dot[4] = {0.f, 0.f, 0.f, 0.f};
        for (int sweep = 0; sweep < 2; ++sweep)
        for (int32_t k0 = 0; k0 < rg.rounds; k0 += G) {
            int32_t e = 0;
            if (k0 + rg.sub < rg.len) e = eid[(int64_t)rg.beg + k0 + rg.sub];
            const int nj = min(G, rg.rounds - k0);
            for (int j0 = 0; j0 < nj; j0 += 4)
#pragma unroll
            for (int j = j0; j < j0 + 4; ++j) {
                const int64_t at = (int64_t)__shfl(e, rg.first + j) * H;
                float y[4], d[4];
                cols.load4(alpha + at, y, dalpha + at, d);
                const bool use = k0 + j < rg.len;
                if (sweep == 0) {
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const float sum = dot[a] + y[a] * d[a];
                        dot[a] = use ? sum : dot[a];
                    }
                } else if (use) {
                    float out[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) out[a] = y[a] * (d[a] - dot[a]);
                    cols.store4(dscores + at, out);
                }
            }
        }
    }
}

// out[r, c] = the sum over row r of (rowptr, idx, eid), in order, of alpha[eid[k], c / C] * values[s, c]; s = eid[k] (EDGE) or idx[k]
template <int G, int ROUTE, bool EDGE>
__global__ __launch_bounds__(256) void attn_gather_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ idx,
                                                          const int32_t *__restrict__ eid, const float *__restrict__ alpha,
                                                          const float *__restrict__ values, float *__restrict__ out, int32_t F, int32_t H,
                                                          int32_t C)
{
    const amp::RowGroup<G> rg(n, rowptr);
    for (int32_t f0 = 0; f0 < F; f0 += 4 * G) {
        const amp::LaneColumns<G, ROUTE != kScalar> cols(rg.sub, f0, F);
        int32_t head[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) head[a] = cols.at(a) / C;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int32_t k0 = 0; k0 < rg.rounds; k0 += G) {
            int32_t c = 0, e = 0;
            if (k0 + rg.sub < rg.len) {
                const int64_t k = (int64_t)rg.beg + k0 + rg.sub;
                e = eid[k];
                c = EDGE ? e : idx[k];
            }
            const int nj = min(G, rg.rounds - k0);
            for (int j0 = 0; j0 < nj; j0 += 4)                      // four entries a step: their loads fly together
#pragma unroll
            for (int j = j0; j < j0 + 4; ++j) {                     // entry order: k0, k0 + 1, ...
                const int32_t ej = __shfl(e, rg.first + j);
                const int32_t sj = EDGE ? ej : __shfl(c, rg.first + j);
                float v[4], w[4];
                cols.load4(values + (int64_t)sj * F, v);
                lane_weights<G, ROUTE>(cols, head, alpha + (int64_t)ej * H, w);
                const bool use = k0 + j < rg.len;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const float sum = acc[a] + w[a] * v[a];
                    acc[a] = use ? sum : acc[a];
                }
            }
        }
        if (rg.row < n) cols.store4(out + rg.row * F, acc);
    }
}

// out[eid[k], c] = dy[r, c] * factor[s, c / C] for the entries k of row r, s = eid[k] (EDGE) or col[k]: the group holds its slice of dy[r].
// bwd_edges: factor = alpha [E, H].  bwd_alpha at C = 1: factor = the values [., F], H = F.
template <int G, int ROUTE, bool EDGE>
__global__ __launch_bounds__(256) void attn_row_times_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                             const int32_t *__restrict__ eid, const float *__restrict__ factor,
                                                             const float *__restrict__ dy, float *__restrict__ out, int32_t F, int32_t H,
                                                             int32_t C)
{
    const amp::RowGroup<G> rg(n, rowptr);
    for (int32_t f0 = 0; f0 < F; f0 += 4 * G) {
        const amp::LaneColumns<G, ROUTE != kScalar> cols(rg.sub, f0, F);
        int32_t head[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) head[a] = cols.at(a) / C;
        float d[4] = {0.f, 0.f, 0.f, 0.f};
        if (rg.len > 0) cols.load4(dy + rg.row * F, d);             // an empty row has no entry to write for
        for (int32_t k0 = 0; k0 < rg.rounds; k0 += G) {
            int32_t c = 0, e = 0;
            if (k0 + rg.sub < rg.len) {
                const int64_t k = (int64_t)rg.beg + k0 + rg.sub;
                e = eid[k];
                c = EDGE ? e : col[k];
            }
            const int nj = min(G, rg.rounds - k0);
            for (int j = 0; j < nj; ++j) {                          // entry order, though each out row has one writer
                const int32_t ej = __shfl(e, rg.first + j);
                const int32_t sj = EDGE ? ej : __shfl(c, rg.first + j);
                if (k0 + j < rg.len) {
                    float w[4], r[4];
                    lane_weights<G, ROUTE>(cols, head, factor + (int64_t)sj * H, w);
#pragma unroll
                    for (int a = 0; a < 4; ++a) r[a] = w[a] * d[a];
                    cols.store4(out + (int64_t)ej * F, r);
                }
            }
        }
    }
}

// dalpha[eid[k], h] for C = 4 L, L a power of two <= G: lane sub owns columns 4 sub .. 4 sub + 3 on both load routes, adds its four
// terms in column order and the L lanes of a head fold theirs by a fixed __shfl_xor tree; the head's first lane stores
template <int G, bool VEC, bool EDGE>
__global__ __launch_bounds__(256) void attn_bwd_alpha_tree_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                  const int32_t *__restrict__ eid, const float *__restrict__ values,
                                                                  const float *__restrict__ dy, float *__restrict__ dalpha, int32_t F,
                                                                  int32_t H, int32_t C)
{
    const amp::RowGroup<G> rg(n, rowptr);
    const int L = C / 4;
    for (int32_t f0 = 0; f0 < F; f0 += 4 * G) {
        const int32_t own = f0 + 4 * rg.sub;                        // F % 4 == 0: the four columns are all below F or none is
        const int32_t at = min(own, F - 4), head = at / C;
        const bool stores = own < F && (rg.sub & (L - 1)) == 0;
        float d[4] = {0.f, 0.f, 0.f, 0.f};
        if (rg.len > 0) {
            const float *dr = dy + rg.row * F + at;
            if (VEC) {
                const float4 q = *reinterpret_cast<const float4 *>(dr);
                d[0] = q.x, d[1] = q.y, d[2] = q.z, d[3] = q.w;
            } else {
#pragma unroll
                for (int a = 0; a < 4; ++a) d[a] = dr[a];
            }
        }
        for (int32_t k0 = 0; k0 < rg.rounds; k0 += G) {
            int32_t c = 0, e = 0;
            if (k0 + rg.sub < rg.len) {
                const int64_t k = (int64_t)rg.beg + k0 + rg.sub;
                e = eid[k];
                c = EDGE ? e : col[k];
            }
            const int nj = min(G, rg.rounds - k0);
            for (int j0 = 0; j0 < nj; j0 += 4)
#pragma unroll
            for (int j = j0; j < j0 + 4; ++j) {
                const int32_t ej = __shfl(e, rg.first + j);
                const int32_t sj = EDGE ? ej : __shfl(c, rg.first + j);
                const float *vr = values + (int64_t)sj * F + at;
                float v[4];
                if (VEC) {
                    const float4 q = *reinterpret_cast<const float4 *>(vr);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                } else {
#pragma unroll
                    for (int a = 0; a < 4; ++a) v[a] = vr[a];
                }
                float part = d[0] * v[0];
#pragma unroll
                for (int a = 1; a < 4; ++a) part = part + d[a] * v[a];
                for (int o = L / 2; o > 0; o >>= 1) part = part + __shfl_xor(part, o);   // every lane of the wave takes part
                if (stores && k0 + j < rg.len) dalpha[(int64_t)ej * H + head] = part;
            }
        }
    }
}

// dalpha[e, h] for any C: one lane per (edge, head) walks its C columns in order
template <bool EDGE>
__global__ __launch_bounds__(256) void attn_bwd_alpha_plain_kernel(int64_t total, const int32_t *__restrict__ e_rowptr,
                                                                   const int32_t *__restrict__ e_row, const int32_t *__restrict__ e_col,
                                                                   const int32_t *__restrict__ col, const float *__restrict__ values,
                                                                   const float *__restrict__ dy, float *__restrict__ dalpha, int32_t F,
                                                                   int32_t H, int32_t C)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int64_t e = t / H;
    const int32_t h = (int32_t)(t - e * H);
    const int32_t q = e_rowptr[e];                                  // the one entry that carries edge column e
    const int64_t s = EDGE ? e : col[e_col[q]];
    const float *d = dy + (int64_t)e_row[q] * F + (int64_t)h * C, *v = values + s * F + (int64_t)h * C;
    float acc = d[0] * v[0];
    for (int32_t c = 1; c < C; ++c) acc = acc + d[c] * v[c];
    dalpha[t] = acc;
}

// f(g, route) with the group width and the read route as compile-time constants
template <typename Fn> void dispatch_route(int G, int route, Fn &&f)
{
    amp::dispatch_group(G, route != kScalar, [&](auto g, auto v) {
        if constexpr (!decltype(v)::value) {
            f(g, std::integral_constant<int, kScalar>{});
        } else {
            if (route == kVecOneHead) f(g, std::integral_constant<int, kVecOneHead>{});
            else if (route == kVecFourHeads) f(g, std::integral_constant<int, kVecFourHeads>{});
            else f(g, std::integral_constant<int, kVecPerColumn>{});
        }
    });
}

// the route of a kernel that moves rows of F columns (`vec`: F % 4 == 0 and those rows on 16-byte boundaries) and reads weights [., H]
int route_of(bool vec, int32_t F, int32_t H, const float *weights)
{
    if (!vec) return kScalar;
    if ((F / H) % 4 == 0) return kVecOneHead;
    return H == F && amp::aligned16(weights) ? kVecFourHeads : kVecPerColumn;
}

template <bool EDGE>
int attn_gather(int32_t n, const int32_t *rowptr, const int32_t *idx, const int32_t *eid, const float *alpha, const float *values, float *out,
                int32_t F, int32_t H)
{
    if (n == 0) return 0;
    const int G = amp::group_width(F);
    dispatch_route(G, route_of(F % 4 == 0 && amp::aligned16(values, out), F, H, alpha), [&](auto g, auto r) {
        hipLaunchKernelGGL((attn_gather_kernel<g(), r(), EDGE>), amp::group_grid(n, G), dim3(256), 0, amp::stream(), n, rowptr, idx, eid, alpha,
                           values, out, F, H, F / H);
    });
    AMP_LAUNCH_CHECK();
    return 0;
}

template <bool EDGE>
int attn_row_times(const athena_mp_graph *g, const float *factor, const float *dy, float *out, int32_t F, int32_t H)
{
    const int G = amp::group_width(F);
    dispatch_route(G, route_of(F % 4 == 0 && amp::aligned16(dy, out), F, H, factor), [&](auto gw, auto r) {
        hipLaunchKernelGGL((attn_row_times_kernel<gw(), r(), EDGE>), amp::group_grid(g->n_rows, G), dim3(256), 0, amp::stream(), g->n_rows,
                           (const int32_t *)g->rowptr, (const int32_t *)g->col, (const int32_t *)g->eid, factor, dy, out, F, H, F / H);
    });
    AMP_LAUNCH_CHECK();
    return 0;
}

template <bool EDGE>
int attn_bwd_alpha(const athena_mp_graph *g, int32_t F, int32_t H, const float *values, const float *dy, float *dalpha)
{
    const int32_t C = F / H;
    const int G = amp::group_width(F);
    if (C == 1) return attn_row_times<EDGE>(g, values, dy, dalpha, F, F);
    if (C % 4 == 0 && ((C / 4) & (C / 4 - 1)) == 0 && C / 4 <= G) {
        amp::dispatch_group(G, amp::aligned16(values, dy), [&](auto gw, auto v) {
            hipLaunchKernelGGL((attn_bwd_alpha_tree_kernel<gw(), v(), EDGE>), amp::group_grid(g->n_rows, G), dim3(256), 0, amp::stream(),
                               g->n_rows, (const int32_t *)g->rowptr, (const int32_t *)g->col, (const int32_t *)g->eid, values, dy, dalpha, F,
                               H, C);
        });
    } else {
        const int64_t total = (int64_t)g->n_edge_cols * H;
        hipLaunchKernelGGL((attn_bwd_alpha_plain_kernel<EDGE>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, amp::stream(), total,
                           (const int32_t *)g->e_rowptr, (const int32_t *)g->e_row, (const int32_t *)g->e_col, (const int32_t *)g->col, values,
                           dy, dalpha, F, H, C);
    }
    AMP_LAUNCH_CHECK();
    return 0;
}

} // namespace

namespace amp {

int attn_check(const char *who, const athena_mp_graph *g, int32_t F, int32_t H)
{
    if (int rc = edge_form_check(who, g)) return rc;
    AMP_REQUIRE(H >= 1, "%s: H = %d: need at least one head", who, H);
    AMP_REQUIRE(F >= 1, "%s: F = %d: need at least one feature column", who, F);
    AMP_REQUIRE(F % H == 0, "%s: F = %d is no multiple of H = %d", who, F, H);
    return 0;
}

} // namespace amp

extern "C" int athena_mp_attn_softmax_fwd(const athena_mp_graph *g, int32_t H, const float *scores_dev, float *alpha_dev)
{
    if (int rc = amp::attn_check("attn_softmax_fwd", g, H, H)) return rc;
    if (g->nnz == 0) return 0;                                      // no entry, so no edge column either: alpha is empty
    AMP_REQUIRE(scores_dev != nullptr && alpha_dev != nullptr, "attn_softmax_fwd: null array");
    const int G = amp::group_width(H);
    amp::dispatch_group(G, H % 4 == 0 && amp::aligned16(scores_dev, alpha_dev), [&](auto gw, auto v) {
        hipLaunchKernelGGL((attn_softmax_fwd_kernel<gw(), v()>), amp::group_grid(g->n_rows, G), dim3(256), 0, amp::stream(), g->n_rows,
                           (const int32_t *)g->rowptr, (const int32_t *)g->eid, scores_dev, alpha_dev, H);
    });
    AMP_LAUNCH_CHECK();
    return 0;
}

extern "C" int athena_mp_attn_softmax_bwd(const athena_mp_graph *g, int32_t H, const float *alpha_dev, const float *dalpha_dev,
                                          float *dscores_dev)
{
    if (int rc = amp::attn_check("attn_softmax_bwd", g, H, H)) return rc;
    if (g->nnz == 0) return 0;
    AMP_REQUIRE(alpha_dev != nullptr && dalpha_dev != nullptr && dscores_dev != nullptr, "attn_softmax_bwd: null array");
    const int G = amp::group_width(H);
    amp::dispatch_group(G, H % 4 == 0 && amp::aligned16(alpha_dev, dalpha_dev, dscores_dev), [&](auto gw, auto v) {
        hipLaunchKernelGGL((attn_softmax_bwd_kernel<gw(), v()>), amp::group_grid(g->n_rows, G), dim3(256), 0, amp::stream(), g->n_rows,
                           (const int32_t *)g->rowptr, (const int32_t *)g->eid, alpha_dev, dalpha_dev, dscores_dev, H);
    });
    AMP_LAUNCH_CHECK();
    return 0;
}

extern "C" int athena_mp_attn_gather_fwd(const athena_mp_graph *g, int32_t F, int32_t H, const float *alpha_dev, const float *x_dev,
                                         float *y_dev)
{
    if (int rc = amp::attn_check("attn_gather_fwd", g, F, H)) return rc;
    AMP_REQUIRE((g->nnz == 0 || (alpha_dev != nullptr && x_dev != nullptr)) && (g->n_rows == 0 || y_dev != nullptr),
                "attn_gather_fwd: null array");
    return attn_gather<false>(g->n_rows, g->rowptr, g->col, g->eid, alpha_dev, x_dev, y_dev, F, H);
}

extern "C" int athena_mp_attn_gather_edges_fwd(const athena_mp_graph *g, int32_t F, int32_t H, const float *alpha_dev, const float *h_dev,
                                               float *y_dev)
{
    if (int rc = amp::attn_check("attn_gather_edges_fwd", g, F, H)) return rc;
    AMP_REQUIRE((g->nnz == 0 || (alpha_dev != nullptr && h_dev != nullptr)) && (g->n_rows == 0 || y_dev != nullptr),
                "attn_gather_edges_fwd: null array");
    return attn_gather<true>(g->n_rows, g->rowptr, g->col, g->eid, alpha_dev, h_dev, y_dev, F, H);
}

extern "C" int athena_mp_attn_gather_bwd_x(const athena_mp_graph *g, int32_t F, int32_t H, const float *alpha_dev, const float *dy_dev,
                                           float *dx_dev)
{
    if (int rc = amp::attn_check("attn_gather_bwd_x", g, F, H)) return rc;
    AMP_REQUIRE((g->nnz == 0 || (alpha_dev != nullptr && dy_dev != nullptr)) && (g->n_cols == 0 || dx_dev != nullptr),
                "attn_gather_bwd_x: null array");
    return attn_gather<false>(g->n_cols, g->t_rowptr, g->t_src, g->t_eid, alpha_dev, dy_dev, dx_dev, F, H);
}

extern "C" int athena_mp_attn_gather_bwd_edges(const athena_mp_graph *g, int32_t F, int32_t H, const float *alpha_dev, const float *dy_dev,
                                               float *dh_dev)
{
    if (int rc = amp::attn_check("attn_gather_bwd_edges", g, F, H)) return rc;
    if (g->nnz == 0) return 0;                                      // dh is empty
    AMP_REQUIRE(alpha_dev != nullptr && dy_dev != nullptr && dh_dev != nullptr, "attn_gather_bwd_edges: null array");
    return attn_row_times<true>(g, alpha_dev, dy_dev, dh_dev, F, H);
}

extern "C" int athena_mp_attn_gather_bwd_alpha(const athena_mp_graph *g, int32_t F, int32_t H, const float *x_dev, const float *h_dev,
                                               const float *dy_dev, float *dalpha_dev)
{
    if (int rc = amp::attn_check("attn_gather_bwd_alpha", g, F, H)) return rc;
    if (g->nnz == 0) return 0;                                      // dalpha is empty
    AMP_REQUIRE((x_dev != nullptr) != (h_dev != nullptr),
                "attn_gather_bwd_alpha: exactly one of x (the vertex form) and h (the edge form) must be given");
    AMP_REQUIRE(dy_dev != nullptr && dalpha_dev != nullptr, "attn_gather_bwd_alpha: null array");
    return h_dev ? attn_bwd_alpha<true>(g, F, H, h_dev, dy_dev, dalpha_dev) : attn_bwd_alpha<false>(g, F, H, x_dev, dy_dev, dalpha_dev);
}
