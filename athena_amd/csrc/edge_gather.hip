// The gather that makes the edge MLP's input over a two-set handle, with its reverse: h[e, :] = (xs[col], xq[row], coords[e]) for every
// entry of the handle, the step between from_point_sets_knn and the MLP of PointNet++'s set abstraction and of EdgeConv (relative: the
// first block is xs[col] - xq[row]), and back from the MLP's input gradient dh to dxs, dxq and dcoords.  Copies are copies -- a load and
// a store, the bits untouched --, the one arithmetic operation of the forward is the fp32 difference, and the reverse sums are the
// sequential fp32 sums in CSR order: every output is bit-defined.
//
// The definition (include/athena_mp.h holds the same text; tests/edge_gather_reference.py is its numpy transcription).  g is a handle that
// the edge forms of interp and pool accept; row i is its forward CSR (rowptr, col, eid), column j its transposed one (t_rowptr, t_src,
// t_eid; rows ascending).  xs [n_cols, Fs], xq [n_rows, Fq], coords [E, dim]; h and dh [E, ld], ld >= W = Fs + Fq + dim the row pitch.
//
//   fwd:      the entry k of row i, j = col[k], e = eid[k]:  h[e, f] = xs[j, f] (relative: xs[j, f] - xq[i, f]) for f < Fs;
//             h[e, Fs + f] = xq[i, f] for f < Fq;  h[e, Fs + Fq + c] = coords[e, c] for c < dim.  Columns W .. ld - 1 are never written.
//   dxs:      dxs[j, f] = acc, acc = +0, then for k = t_rowptr[j] .. in order, e = t_eid[k]: acc = acc + dh[e, f]
//   dxq:      dxq[i, f] = acc, acc = +0, then for k = rowptr[i] .. in order, e = eid[k]: acc = acc + dh[e, Fs + f], and with relative,
//             after that, acc = acc - dh[e, f]
//   dcoords:  dcoords[e, c] = dh[e, Fs + Fq + c].  Columns W .. ld - 1 of dh are never read.
//
// How.  The lane groups of row_groups.h.  edge_gather_fwd_kernel: G is sized from max(Fs, Fq) -- the two blocks are moved by the same
// lanes, so the group is sized from the wider one, not from W.  The group holds its slice of xq[i] in registers.  Four entries are a
// step: first the four slices of xs[col] and the four coords words are loaded, without a branch (a lane past its row's end or past Fs
// reads a valid place and stores nothing), then the slices of h[e, ..] are stored.  The coords tail rides in the first pass -- lane sub
// moves coords[e, sub], and a dim beyond G takes a short loop of its own -- so that the whole of h[e, :] is written by one group at one
// time.  relative is a template argument: the instances that copy hold no arithmetic at all.
// edge_gather_bwd_src_kernel (over the transposed CSR) and edge_gather_bwd_query_kernel (over the rows): the sequential sums of the
// gathered rows dh + e ld at a column offset; the query kernel subtracts the first block's word after it added the second's where
// relative.  dcoords is a launch of its own, one lane per word: it reads what no other lane reads and writes what no other lane
// writes, and it is there whether or not dxq was asked for.
// The 16-byte route needs Fs % 4 == 0, Fq % 4 == 0, ld % 4 == 0 and every array of the call on a 16-byte boundary (the blocks [0, Fs)
// and [Fs, Fs + Fq) then start on one in every row).  One entry per edge column is what makes every h[e, :] written exactly once.
#include "common.h"
#include "row_groups.h"

namespace {

// h[eid[k], :] = (xs[col[k], :] (REL: - xq[r, :]), xq[r, :], coords[eid[k], :]) for the entries k of row r
template <int G, bool VEC, bool REL>
__global__ __launch_bounds__(256) void edge_gather_fwd_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                              const int32_t *__restrict__ eid, int32_t Fs, const float *__restrict__ xs,
                                                              int32_t Fq, const float *__restrict__ xq, int32_t dim,
                                                              const float *__restrict__ coords, int32_t ld, float *__restrict__ h)
{
    const amp::RowGroup<G> rg(n, rowptr);
    const int32_t FM = max(Fs, Fq);
    const int32_t cat = min(rg.sub, dim - 1);                       // the coords word this lane moves (dim > 0), clamped
    int32_t f0 = 0;
    do {                                                            // once even when both blocks are absent: the coords tail
        const amp::LaneColumns<G, VEC> cs(rg.sub, f0, Fs), cq(rg.sub, f0, Fq);   // the same columns of the two blocks
        const bool tail = f0 == 0 && dim > 0;
        float q[4] = {0.f, 0.f, 0.f, 0.f};
        if (Fq > 0 && rg.len > 0) cq.load4(xq + rg.row * Fq, q);   // an empty row has no entry to write for
        for (int32_t k0 = 0; k0 < rg.rounds; k0 += G) {
            int32_t c = 0, e = 0;
            if (k0 + rg.sub < rg.len) {
                const int64_t k = (int64_t)rg.beg + k0 + rg.sub;
                c = col[k];
                e = eid[k];
            }
            const int nj = min(G, rg.rounds - k0);
            for (int j0 = 0; j0 < nj; j0 += 4) {                    // four entries a step (G is a multiple of 4): their loads fly together
                int32_t ej[4];
                float v[4][4], cv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int32_t cj = __shfl(c, rg.first + j0 + j);
                    ej[j] = __shfl(e, rg.first + j0 + j);
                    if (Fs > 0) cs.load4(xs + (int64_t)cj * Fs, v[j]);
                    if (tail) cv[j] = coords[(int64_t)ej[j] * dim + cat];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {                       // entry order, though each row of h has one writer
                    if (k0 + j0 + j >= rg.len) continue;
                    float *dst = h + (int64_t)ej[j] * ld;
                    if (Fs > 0) {
                        float out[4];
#pragma unroll
                        for (int a = 0; a < 4; ++a) out[a] = REL ? v[j][a] - q[a] : v[j][a];
                        cs.store4(dst, out);
                    }
                    if (Fq > 0) cq.store4(dst, q, Fs);
                    if (tail) {
                        float *cdst = dst + Fs + Fq;
                        if (rg.sub < dim) cdst[rg.sub] = cv[j];
                        for (int32_t cc = rg.sub + G; cc < dim; cc += G) cdst[cc] = coords[(int64_t)ej[j] * dim + cc];
                    }
                }
            }
        }
        f0 += 4 * G;
    } while (f0 < FM);
}

// out[r, :] = the sum over row r of (rowptr, ids) of dh[ids[k], off + f], f < F; REL: each entry's dh[ids[k], f] is subtracted after
// its dh[ids[k], off + f] was added.  G lanes per row, four columns per lane and pass.
template <int G, bool VEC, bool REL>
__device__ __forceinline__ void edge_gather_row_sums(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ ids,
                                                     const float *__restrict__ dh, int32_t ld, int32_t off, float *__restrict__ out,
                                                     int32_t F)
{
    const amp::RowGroup<G> rg(n, rowptr);
    for (int32_t f0 = 0; f0 < F; f0 += 4 * G) {
        const amp::LaneColumns<G, VEC> cols(rg.sub, f0, F);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int32_t k0 = 0; k0 < rg.rounds; k0 += G) {
            int32_t e = 0;
            if (k0 + rg.sub < rg.len) e = ids[(int64_t)rg.beg + k0 + rg.sub];
            const int nj = min(G, rg.rounds - k0);
            for (int j0 = 0; j0 < nj; j0 += 4)                      // four entries a step (G is a multiple of 4): their loads fly together
#pragma unroll
            for (int j = j0; j < j0 + 4; ++j) {                     // entry order: k0, k0 + 1, ...
                const float *src = dh + (int64_t)__shfl(e, rg.first + j) * ld;
                float v[4], m[4] = {0.f, 0.f, 0.f, 0.f};
                cols.load4(src, v, off);
                if (REL) cols.load4(src, m);
                const bool use = k0 + j < rg.len;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    float sum = acc[a] + v[a];
                    if (REL) sum = sum - m[a];
                    acc[a] = use ? sum : acc[a];
                }
            }
        }
        if (rg.row < n) cols.store4(out + rg.row * F, acc);
    }
}

// dxs[j, :] over column j of the handle (t_rowptr, t_eid), queries ascending: the first block of dh
template <int G, bool VEC>
__global__ __launch_bounds__(256) void edge_gather_bwd_src_kernel(int32_t n, const int32_t *__restrict__ t_rowptr,
                                                                  const int32_t *__restrict__ t_eid, const float *__restrict__ dh, int32_t ld,
                                                                  float *__restrict__ dxs, int32_t Fs)
{
    edge_gather_row_sums<G, VEC, false>(n, t_rowptr, t_eid, dh, ld, 0, dxs, Fs);
}

// dxq[i, :] over row i of the handle (rowptr, eid): the second block of dh, REL: less the first
template <int G, bool VEC, bool REL>
__global__ __launch_bounds__(256) void edge_gather_bwd_query_kernel(int32_t n, const int32_t *__restrict__ rowptr,
                                                                    const int32_t *__restrict__ eid, const float *__restrict__ dh, int32_t ld,
                                                                    int32_t Fs, float *__restrict__ dxq, int32_t Fq)
{
    edge_gather_row_sums<G, VEC, REL>(n, rowptr, eid, dh, ld, Fs, dxq, Fq);
}

// dcoords[e, c] = dh[e, off + c]: one lane per word
__global__ __launch_bounds__(256) void edge_gather_dcoords_kernel(int64_t words, int32_t dim, const float *__restrict__ dh, int32_t ld,
                                                                  int32_t off, float *__restrict__ dcoords)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= words) return;
    const int64_t e = t / dim;
    dcoords[t] = dh[e * ld + off + (int32_t)(t - e * dim)];
}

} // namespace

namespace amp {

// what both entries and their *_host forms check first: one entry per edge column, then the widths and the pitch
int edge_gather_check(const char *who, const athena_mp_graph *g, int32_t Fs, int32_t Fq, int32_t dim, int32_t relative, int32_t ld)
{
    if (int rc = edge_form_check(who, g)) return rc;
    AMP_REQUIRE(Fs >= 0 && Fq >= 0 && dim >= 0, "%s: Fs = %d, Fq = %d, dim = %d: a negative width", who, Fs, Fq, dim);
    const int64_t W = (int64_t)Fs + Fq + dim;
    AMP_REQUIRE(W >= 1, "%s: Fs + Fq + dim = 0: need at least one column", who);
    AMP_REQUIRE(ld >= W, "%s: ld = %d is less than Fs + Fq + dim = %lld", who, ld, (long long)W);
    AMP_REQUIRE(relative == 0 || relative == 1, "%s: relative = %d is neither 0 nor 1", who, relative);
    AMP_REQUIRE(!relative || Fs > 0, "%s: relative needs a source block: Fs = 0", who);
    AMP_REQUIRE(!relative || Fs == Fq, "%s: relative needs Fs == Fq: Fs = %d, Fq = %d", who, Fs, Fq);
    return 0;
}

} // namespace amp

extern "C" int athena_mp_edge_gather_fwd(const athena_mp_graph *g, int32_t Fs, const float *xs_dev, int32_t Fq, const float *xq_dev,
                                         int32_t dim, const float *coords_dev, int32_t relative, int32_t ld, float *h_dev)
{
    if (int rc = amp::edge_gather_check("edge_gather_fwd", g, Fs, Fq, dim, relative, ld)) return rc;
    AMP_REQUIRE(Fs == 0 || g->n_cols == 0 || xs_dev != nullptr, "edge_gather_fwd: xs is null and Fs = %d", Fs);
    AMP_REQUIRE(Fq == 0 || g->n_rows == 0 || xq_dev != nullptr, "edge_gather_fwd: xq is null and Fq = %d", Fq);
    AMP_REQUIRE(dim == 0 || g->nnz == 0 || coords_dev != nullptr, "edge_gather_fwd: coords is null and dim = %d", dim);
    if (g->nnz == 0) return 0;                                      // no entry, so no edge column either: h is empty
    AMP_REQUIRE(h_dev != nullptr, "edge_gather_fwd: h is null");
    const int G = amp::group_width(Fs > Fq ? Fs : Fq);
    const bool vec = Fs % 4 == 0 && Fq % 4 == 0 && ld % 4 == 0 && amp::aligned16(xs_dev, xq_dev, coords_dev, h_dev);
    amp::dispatch_group(G, vec, relative != 0, [&](auto gw, auto v, auto rel) {
        hipLaunchKernelGGL((edge_gather_fwd_kernel<gw(), v(), rel()>), amp::group_grid(g->n_rows, G), dim3(256), 0, amp::stream(),
                           g->n_rows, (const int32_t *)g->rowptr, (const int32_t *)g->col, (const int32_t *)g->eid, Fs, xs_dev, Fq, xq_dev,
                           dim, coords_dev, ld, h_dev);
    });
    AMP_LAUNCH_CHECK();
    return 0;
}

extern "C" int athena_mp_edge_gather_bwd(const athena_mp_graph *g, int32_t Fs, int32_t Fq, int32_t dim, int32_t relative, int32_t ld,
                                         const float *dh_dev, float *dxs_dev, float *dxq_dev, float *dcoords_dev)
{
    if (int rc = amp::edge_gather_check("edge_gather_bwd", g, Fs, Fq, dim, relative, ld)) return rc;
    AMP_REQUIRE(g->nnz == 0 || dh_dev != nullptr, "edge_gather_bwd: dh is null");
    hipStream_t st = amp::stream();
    const dim3 block(256);
    const bool vec = Fs % 4 == 0 && Fq % 4 == 0 && ld % 4 == 0 && amp::aligned16(dh_dev, dxs_dev, dxq_dev, dcoords_dev);
    if (dxs_dev && Fs > 0 && g->n_cols > 0) {
        const int G = amp::group_width(Fs);
        amp::dispatch_group(G, vec, [&](auto gw, auto v) {
            hipLaunchKernelGGL((edge_gather_bwd_src_kernel<gw(), v()>), amp::group_grid(g->n_cols, G), block, 0, st, g->n_cols,
                               (const int32_t *)g->t_rowptr, (const int32_t *)g->t_eid, dh_dev, ld, dxs_dev, Fs);
        });
        AMP_LAUNCH_CHECK();
    }
    if (dxq_dev && Fq > 0 && g->n_rows > 0) {
        const int G = amp::group_width(Fq);
        amp::dispatch_group(G, vec, relative != 0, [&](auto gw, auto v, auto rel) {
            hipLaunchKernelGGL((edge_gather_bwd_query_kernel<gw(), v(), rel()>), amp::group_grid(g->n_rows, G), block, 0, st, g->n_rows,
                               (const int32_t *)g->rowptr, (const int32_t *)g->eid, dh_dev, ld, Fs, dxq_dev, Fq);
        });
        AMP_LAUNCH_CHECK();
    }
    if (dcoords_dev && dim > 0 && g->nnz > 0) {
        const int64_t words = (int64_t)g->n_edge_cols * dim;
        hipLaunchKernelGGL(edge_gather_dcoords_kernel, dim3((unsigned)((words + 255) / 256)), block, 0, st, words, dim, dh_dev, ld, Fs + Fq,
                           dcoords_dev);
        AMP_LAUNCH_CHECK();
    }
    return 0;
}
