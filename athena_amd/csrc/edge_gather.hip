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
// How.  edge_gather_fwd_kernel: the lane groups of pool_bwd_edges_kernel, G lanes per row, G the smallest power of two from 4 with
// 4 G >= max(Fs, Fq) -- the two blocks are moved by the same lanes, so the group is sized from the wider one, not from W (a full wave
// from 193 columns; more than 256 take further passes).  The group holds its slice of xq[i] in registers; the lanes load col and eid of G
// entries, one entry per lane, and the entries pass through the group in entry order (__shfl, no LDS).  Four entries are a step: first
// the four slices of xs[col] and the four coords words are loaded, without a branch (a lane past its row's end or past Fs reads a valid
// place and stores nothing), then the slices of h[e, ..] are stored; the wave's longest row is a scalar loop bound.  The coords tail
// rides in the first pass -- lane sub moves coords[e, sub], and a dim beyond G takes a short loop of its own -- so that the whole of
// h[e, :] is written by one group at one time.  relative is a template argument: the instances that copy hold no arithmetic at all.
// edge_gather_bwd_src_kernel (over the transposed CSR) and edge_gather_bwd_query_kernel (over the rows): the lane groups of
// interp_gather_kernel without the weight, the gathered row dh + e ld at a column offset; the query kernel subtracts the first block's
// word after it added the second's where relative.  dcoords is a launch of its own, one lane per word: it reads what no other lane
// reads and writes what no other lane writes, and it is there whether or not dxq was asked for.
// Two load/store routes with the same bytes: a lane owns columns 4 sub .. 4 sub + 3 of a block and moves them 16 bytes at a time when
// Fs % 4 == 0, Fq % 4 == 0, ld % 4 == 0 and every array of the call starts on a 16-byte boundary (the blocks [0, Fs) and [Fs, Fs + Fq)
// then start on one in every row); otherwise columns sub + G a, four bytes at a time.  Each column sees the same entries in the same
// order on either route.  No LDS, no atomics, no scratch; one entry per edge column is what makes every h[e, :] written exactly once.
#include "common.h"

namespace {

// the smallest power of two from 4 with 4 G >= F, at most a wave
int edge_gather_group_width(int32_t F)
{
    int G = 4;
    while (G < 64 && 4 * G < F) G *= 2;
    return G;
}

// h[eid[k], :] = (xs[col[k], :] (REL: - xq[r, :]), xq[r, :], coords[eid[k], :]) for the entries k of row r
template <int G, bool VEC, bool REL>
__global__ __launch_bounds__(256) void edge_gather_fwd_kernel(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                              const int32_t *__restrict__ eid, int32_t Fs, const float *__restrict__ xs,
                                                              int32_t Fq, const float *__restrict__ xq, int32_t dim,
                                                              const float *__restrict__ coords, int32_t ld, float *__restrict__ h)
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
    rounds = __builtin_amdgcn_readfirstlane(rounds);               // the same in every lane: a scalar loop bound
    const int32_t FM = max(Fs, Fq);
    const int32_t cat = min(sub, dim - 1);                          // the coords word this lane moves (dim > 0), clamped
    int32_t f0 = 0;
    do {                                                            // once even when both blocks are absent: the coords tail
        // this lane's columns, and where it reads them: a column past a block's width reads the last valid place and is never stored
        int32_t colv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) colv[a] = VEC ? f0 + 4 * sub + a : f0 + sub + G * a;
        const int32_t s4 = min(colv[0], Fs - 4), q4 = min(colv[0], Fq - 4);     // VEC only: a present block holds 4 columns at least
        const bool tail = f0 == 0 && dim > 0;
        float q[4] = {0.f, 0.f, 0.f, 0.f};
        if (Fq > 0 && len > 0) {                                    // an empty row has no entry to write for
            const float *qr = xq + row * Fq;
            if (VEC) {
                const float4 t = *reinterpret_cast<const float4 *>(qr + q4);
                q[0] = t.x, q[1] = t.y, q[2] = t.z, q[3] = t.w;
            } else {
#pragma unroll
                for (int a = 0; a < 4; ++a) q[a] = qr[min(colv[a], Fq - 1)];
            }
        }
        for (int32_t k0 = 0; k0 < rounds; k0 += G) {
            int32_t c = 0, e = 0;
            if (k0 + sub < len) {
                const int64_t k = (int64_t)beg + k0 + sub;
                c = col[k];
                e = eid[k];
            }
            const int nj = min(G, rounds - k0);
            for (int j0 = 0; j0 < nj; j0 += 4) {                    // four entries a step (G is a multiple of 4): their loads fly together
                int32_t ej[4];
                float v[4][4], cv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int32_t cj = __shfl(c, first + j0 + j);
                    ej[j] = __shfl(e, first + j0 + j);
                    if (Fs > 0) {
                        const float *src = xs + (int64_t)cj * Fs;
                        if (VEC) {
                            const float4 t = *reinterpret_cast<const float4 *>(src + s4);
                            v[j][0] = t.x, v[j][1] = t.y, v[j][2] = t.z, v[j][3] = t.w;
                        } else {
#pragma unroll
                            for (int a = 0; a < 4; ++a) v[j][a] = src[min(colv[a], Fs - 1)];
                        }
                    }
                    if (tail) cv[j] = coords[(int64_t)ej[j] * dim + cat];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {                       // entry order, though each row of h has one writer
                    if (k0 + j0 + j >= len) continue;
                    float *dst = h + (int64_t)ej[j] * ld;
                    if (Fs > 0) {
                        float out[4];
#pragma unroll
                        for (int a = 0; a < 4; ++a) out[a] = REL ? v[j][a] - q[a] : v[j][a];
                        if (VEC) {
                            if (colv[0] < Fs) *reinterpret_cast<float4 *>(dst + colv[0]) = make_float4(out[0], out[1], out[2], out[3]);
                        } else {
#pragma unroll
                            for (int a = 0; a < 4; ++a)
                                if (colv[a] < Fs) dst[colv[a]] = out[a];
                        }
                    }
                    if (Fq > 0) {
                        if (VEC) {
                            if (colv[0] < Fq) *reinterpret_cast<float4 *>(dst + Fs + colv[0]) = make_float4(q[0], q[1], q[2], q[3]);
                        } else {
#pragma unroll
                            for (int a = 0; a < 4; ++a)
                                if (colv[a] < Fq) dst[Fs + colv[a]] = q[a];
                        }
                    }
                    if (tail) {
                        float *cdst = dst + Fs + Fq;
                        if (sub < dim) cdst[sub] = cv[j];
                        for (int32_t cc = sub + G; cc < dim; cc += G) cdst[cc] = coords[(int64_t)ej[j] * dim + cc];
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
    rounds = __builtin_amdgcn_readfirstlane(rounds);               // the same in every lane: a scalar loop bound
    for (int32_t f0 = 0; f0 < F; f0 += 4 * G) {
        // this lane's columns, and where it reads them: a column past F reads the last valid place and is never stored
        int32_t colv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) colv[a] = VEC ? f0 + 4 * sub + a : f0 + sub + G * a;
        const int32_t at4 = min(colv[0], F - 4);                    // VEC only: F >= 4 there
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int32_t k0 = 0; k0 < rounds; k0 += G) {
            int32_t e = 0;
            if (k0 + sub < len) e = ids[(int64_t)beg + k0 + sub];
            const int nj = min(G, rounds - k0);
            for (int j0 = 0; j0 < nj; j0 += 4)                      // four entries a step (G is a multiple of 4): their loads fly together
#pragma unroll
            for (int j = j0; j < j0 + 4; ++j) {                     // entry order: k0, k0 + 1, ...
                const float *src = dh + (int64_t)__shfl(e, first + j) * ld;
                float v[4], m[4] = {0.f, 0.f, 0.f, 0.f};
                if (VEC) {
                    const float4 t = *reinterpret_cast<const float4 *>(src + off + at4);
                    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
                    if (REL) {
                        const float4 u = *reinterpret_cast<const float4 *>(src + at4);
                        m[0] = u.x, m[1] = u.y, m[2] = u.z, m[3] = u.w;
                    }
                } else {
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const int32_t f = min(colv[a], F - 1);
                        v[a] = src[off + f];
                        if (REL) m[a] = src[f];
                    }
                }
                const bool use = k0 + j < len;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    float sum = acc[a] + v[a];
                    if (REL) sum = sum - m[a];
                    acc[a] = use ? sum : acc[a];
                }
            }
        }
        if (row < n) {
            float *dst = out + row * F;
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

// one launch per (group width, load route): LAUNCH(W, V) names the kernel instance
#define ATHENA_EDGE_GATHER_DISPATCH(LAUNCH)           \
    do {                                              \
        switch (G) {                                  \
        case 4: if (vec) LAUNCH(4, true); else LAUNCH(4, false); break;    \
        case 8: if (vec) LAUNCH(8, true); else LAUNCH(8, false); break;    \
        case 16: if (vec) LAUNCH(16, true); else LAUNCH(16, false); break; \
        case 32: if (vec) LAUNCH(32, true); else LAUNCH(32, false); break; \
        default: if (vec) LAUNCH(64, true); else LAUNCH(64, false); break; \
        }                                             \
    } while (0)

dim3 edge_gather_grid(int32_t rows, int G) { return dim3((unsigned)(((int64_t)rows + 256 / G - 1) / (256 / G))); }

} // namespace

namespace amp {

// what both entries and their *_host forms check first: the handle through interp_check, then the widths and the pitch
int edge_gather_check(const char *who, const athena_mp_graph *g, int32_t Fs, int32_t Fq, int32_t dim, int32_t relative, int32_t ld)
{
    if (int rc = interp_check(who, g, nullptr, nullptr, nullptr)) return rc;
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
    const int G = edge_gather_group_width(Fs > Fq ? Fs : Fq);
    const dim3 grid = edge_gather_grid(g->n_rows, G), block(256);
    hipStream_t st = amp::stream();
    const bool vec = Fs % 4 == 0 && Fq % 4 == 0 && ld % 4 == 0 && amp::aligned16(xs_dev, xq_dev, coords_dev, h_dev);
#define ATHENA_EDGE_GATHER_FWD(W, V)                                                                                                  \
    do {                                                                                                                              \
        if (relative)                                                                                                                 \
            hipLaunchKernelGGL((edge_gather_fwd_kernel<W, V, true>), grid, block, 0, st, g->n_rows, (const int32_t *)g->rowptr,       \
                               (const int32_t *)g->col, (const int32_t *)g->eid, Fs, xs_dev, Fq, xq_dev, dim, coords_dev, ld, h_dev); \
        else                                                                                                                          \
            hipLaunchKernelGGL((edge_gather_fwd_kernel<W, V, false>), grid, block, 0, st, g->n_rows, (const int32_t *)g->rowptr,      \
                               (const int32_t *)g->col, (const int32_t *)g->eid, Fs, xs_dev, Fq, xq_dev, dim, coords_dev, ld, h_dev); \
    } while (0)
    ATHENA_EDGE_GATHER_DISPATCH(ATHENA_EDGE_GATHER_FWD);
#undef ATHENA_EDGE_GATHER_FWD
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
        const int G = edge_gather_group_width(Fs);
        const dim3 grid = edge_gather_grid(g->n_cols, G);
#define ATHENA_EDGE_GATHER_SRC(W, V)                                                                                                \
    hipLaunchKernelGGL((edge_gather_bwd_src_kernel<W, V>), grid, block, 0, st, g->n_cols, (const int32_t *)g->t_rowptr,             \
                       (const int32_t *)g->t_eid, dh_dev, ld, dxs_dev, Fs)
        ATHENA_EDGE_GATHER_DISPATCH(ATHENA_EDGE_GATHER_SRC);
#undef ATHENA_EDGE_GATHER_SRC
        AMP_LAUNCH_CHECK();
    }
    if (dxq_dev && Fq > 0 && g->n_rows > 0) {
        const int G = edge_gather_group_width(Fq);
        const dim3 grid = edge_gather_grid(g->n_rows, G);
#define ATHENA_EDGE_GATHER_QUERY(W, V)                                                                                              \
    do {                                                                                                                            \
        if (relative)                                                                                                               \
            hipLaunchKernelGGL((edge_gather_bwd_query_kernel<W, V, true>), grid, block, 0, st, g->n_rows, (const int32_t *)g->rowptr, \
                               (const int32_t *)g->eid, dh_dev, ld, Fs, dxq_dev, Fq);                                               \
        else                                                                                                                        \
            hipLaunchKernelGGL((edge_gather_bwd_query_kernel<W, V, false>), grid, block, 0, st, g->n_rows, (const int32_t *)g->rowptr, \
                               (const int32_t *)g->eid, dh_dev, ld, Fs, dxq_dev, Fq);                                               \
    } while (0)
        ATHENA_EDGE_GATHER_DISPATCH(ATHENA_EDGE_GATHER_QUERY);
#undef ATHENA_EDGE_GATHER_QUERY
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
