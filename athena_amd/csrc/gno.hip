// Graph neural operator (athena's graph_nop layer) without the per-edge kernel tensor.
//
// Reference (athena_diffstruc_extd_sub_nop.f90): gno_kernel_eval materialises
//   kappa[:, e] = V relu(U dx_e + b_u) + b_v            ([F_out*F_in, E], :88-93)
// and gno_aggregate contracts it per CSR entry           (m_i += reshape(kappa_e) x_j, :367-378).
// At BASELINE config 4 that tensor is 246 GB.  Here the sum is re-associated:
//   h_e = [relu(U dx_e + b_u) ; 1]                                     (H+1 values per edge column)
//   S_i[k, q] = sum_{(j,e) in row i} h_e[k] x_j[q]                     ((H+1) x F_in per vertex)
//   m_i[o]    = sum_{k,q} Vaug[o + F_out*(q + F_in*k)] S_i[k, q]       (Vaug = [V | b_v], contiguous in theta)
// i.e. a gather + rank-1 accumulation per entry followed by ONE dense contraction with K = (H+1) F_in
// whose B operand is theta's own memory viewed row-major [(k,q)][o].  Same maths, different rounding
// (checked against the materialising oracle at 1e-5).  The backward passes reuse the two pieces:
//   dx_j  : T_j[k,o] = sum_{(i,e) in column j} h_e[k] g_i[o]  (pull over the transposed CSR), dx = T . B2
//   dVaug : S^T g   (dense reduction over vertices)            -> dV and db_v   (:291-300)
//   dU,db_u,dcoords : per entry dh[k] = sum_q G_i[k,q] x_j[q], G = g . Vmat^T, masked by relu' (:303-318, :195-210)
// S / T / G are produced per super-tile of vertices into a bounded HBM workspace.
// This file holds the kernels of any shape, the tiled routes built from them and the C ABI; the kernels that keep S / T / G on
// chip at H = F_in = F_out = 64 and the predicates that say which call takes them are in gno64.hip.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kEB = 8; // entries staged per batch

// S[r][k*Fy + q] = sum_{w in row r} h_{eidx[w]}[k] * y[idx[w]][q],  k in [0,H] (h[H] = 1)
template <int EPT>
__global__ __launch_bounds__(256) void gno_outer_kernel(const int32_t *__restrict__ rowptr,
                                                        const int32_t *__restrict__ idx,
                                                        const int32_t *__restrict__ eidx,
                                                        const float *__restrict__ y, int Fy,
                                                        const float *__restrict__ coords,
                                                        const float *__restrict__ theta, int d, int H,
                                                        int r0, float *__restrict__ S)
{
    extern __shared__ float sm[];
    float *hb = sm;                    // [kEB][H+1]
    float *yb = sm + kEB * (H + 1);    // [kEB][Fy]
    const int row = r0 + blockIdx.x;
    const int R = (H + 1) * Fy;
    const float *U = theta, *bu = theta + (size_t)H * d;
    float acc[EPT];
    int kk[EPT], qq[EPT];
#pragma unroll
    for (int n = 0; n < EPT; ++n) {
        int e = threadIdx.x + 256 * n;
        acc[n] = 0.0f;
        kk[n] = e < R ? e / Fy : 0;
        qq[n] = e < R ? e - kk[n] * Fy : 0;
    }
    const int w0 = rowptr[row], w1 = rowptr[row + 1];
    for (int wb = w0; wb < w1; wb += kEB) {
        const int nb = min(kEB, w1 - wb);
        __syncthreads();
        for (int t = threadIdx.x; t < nb * (H + 1); t += 256) {
            int b = t / (H + 1), k = t - b * (H + 1);
            int e = eidx[wb + b];
            float hv = 0.0f;
            if (e >= 0) {
                if (k == H) hv = 1.0f;
                else {
                    const float *dx = coords + (size_t)e * d;
                    float s = 0.0f;
                    for (int j = 0; j < d; ++j) s = s + U[k + (size_t)H * j] * dx[j];
                    s = s + bu[k];
                    hv = s > 0.0f ? s : 0.0f;
                }
            }
            hb[b * (H + 1) + k] = hv;
        }
        for (int t = threadIdx.x; t < nb * Fy; t += 256) {
            int b = t / Fy, q = t - b * Fy;
            yb[b * Fy + q] = y[(size_t)idx[wb + b] * Fy + q];
        }
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
#pragma unroll
            for (int n = 0; n < EPT; ++n) acc[n] = fmaf(hb[b * (H + 1) + kk[n]], yb[b * Fy + qq[n]], acc[n]);
        }
    }
    float *out = S + (size_t)blockIdx.x * R;
#pragma unroll
    for (int n = 0; n < EPT; ++n) {
        int e = threadIdx.x + 256 * n;
        if (e < R) out[e] = acc[n];
    }
}

// ---- MFMA form of the outer-product accumulation (H, F multiples of 32, <= 64; d <= 4) -----------
// One wave per vertex.  S_i = Hm^T X with the row's entries as the contraction index:
//   v_mfma_f32_32x32x2_f32: A[k][e] = h_e[k] (computed on the fly by the lane that owns k),
//                           B[e][q] = y_j[q] (128 B coalesced loads, two entries per step).
// The bias row S_i[H,:] = sum_j y_j is accumulated on the VALU from the same loads.
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int HT, int QT>
__global__ __launch_bounds__(256) void gno_outer_mfma_kernel(const int32_t *__restrict__ rowptr,
                                                             const int32_t *__restrict__ idx,
                                                             const int32_t *__restrict__ eidx,
                                                             const float *__restrict__ y,
                                                             const float *__restrict__ coords,
                                                             const float *__restrict__ theta, int d, int r0,
                                                             int n_rows_tile, float *__restrict__ S)
{
    constexpr int H = 32 * HT, Fy = 32 * QT, R = (H + 1) * Fy;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r31 = lane & 31, h = lane >> 5;
    const int lr = blockIdx.x * 4 + wave;
    if (lr >= n_rows_tile) return;
    const int row = r0 + lr;
    // this lane's rows of U and b_u (k = 32 t + r31)
    float Uk[HT][4], bk[HT];
#pragma unroll
    for (int t = 0; t < HT; ++t) {
        bk[t] = theta[(size_t)H * d + 32 * t + r31];
#pragma unroll
        for (int j = 0; j < 4; ++j) Uk[t][j] = j < d ? theta[(32 * t + r31) + (size_t)H * j] : 0.0f;
    }
    f32x16 acc[HT][QT];
#pragma unroll
    for (int a = 0; a < HT; ++a)
#pragma unroll
        for (int b = 0; b < QT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;
    float sb[QT];
#pragma unroll
    for (int b = 0; b < QT; ++b) sb[b] = 0.0f;

    const int w0 = rowptr[row], w1 = rowptr[row + 1];
    for (int wb = w0; wb < w1; wb += 64) {
        const int nb = min(64, w1 - wb);
        int my_j = -1, my_e = -1;
        if (lane < nb) { my_j = idx[wb + lane]; my_e = eidx[wb + lane]; }
        constexpr int U4 = 4;
        for (int s0 = 0; s0 < (nb + 1) / 2; s0 += U4) {
            float yv[U4][QT], dx[U4][4];
            bool ok[U4];
#pragma unroll
            for (int u = 0; u < U4; ++u) {
                const int ent = 2 * (s0 + u) + h;
                const int j = __shfl(my_j, ent), e = __shfl(my_e, ent);
                ok[u] = ent < nb && e >= 0;
#pragma unroll
                for (int b = 0; b < QT; ++b) yv[u][b] = ok[u] ? y[(size_t)j * Fy + 32 * b + r31] : 0.0f;
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) dx[u][jj] = (ok[u] && jj < d) ? coords[(size_t)e * d + jj] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < U4; ++u) {
                float hv[HT];
#pragma unroll
                for (int t = 0; t < HT; ++t) {
                    float sacc = 0.0f;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) sacc = sacc + Uk[t][jj] * dx[u][jj];   // j-ordered, as :88-90
                    sacc = sacc + bk[t];
                    hv[t] = (ok[u] && sacc > 0.0f) ? sacc : 0.0f;
                }
#pragma unroll
                for (int b = 0; b < QT; ++b) sb[b] = sb[b] + yv[u][b];
#pragma unroll
                for (int t = 0; t < HT; ++t)
#pragma unroll
                    for (int b = 0; b < QT; ++b)
                        acc[t][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(hv[t], yv[u][b], acc[t][b], 0, 0, 0);
            }
        }
    }
    float *out = S + (size_t)lr * R;
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int b = 0; b < QT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
                out[(size_t)k * Fy + 32 * b + r31] = acc[t][b][r];
            }
#pragma unroll
    for (int b = 0; b < QT; ++b) {
        const float tot = sb[b] + __shfl_xor(sb[b], 32);
        if (h == 0) out[(size_t)H * Fy + 32 * b + r31] = tot;
    }
}

// B2[(k*Fo + o)*Fi + q] = Vaug[F*k + o + Fo*q]
__global__ void gno_perm_kernel(const float *__restrict__ vaug, int H1, int Fi, int Fo, float *__restrict__ B2)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    int n = H1 * Fo * Fi;
    if (t >= n) return;
    int q = t % Fi, ko = t / Fi, o = ko % Fo, k = ko / Fo;
    B2[t] = vaug[(size_t)Fo * Fi * k + o + Fo * q];
}

// Per CSR entry: dh[k] = sum_q G_i[k,q] x_j[q]; gh = relu'(pre_e[k]) dh.  Accumulates dU / db_u partials
// per workgroup (chunk of rows) and optionally stores gh per entry for the coordinate gradient.
__global__ __launch_bounds__(256) void gno_dh_kernel(const int32_t *__restrict__ rowptr,
                                                     const int32_t *__restrict__ col,
                                                     const int32_t *__restrict__ eid,
                                                     const float *__restrict__ x, int Fi,
                                                     const float *__restrict__ coords,
                                                     const float *__restrict__ theta, int d, int H,
                                                     const float *__restrict__ G, int r0, int n_rows_tile,
                                                     int rows_per_block, float *__restrict__ slabs,
                                                     float *__restrict__ ghbuf)
{
    extern __shared__ float sm[];
    const int GP = Fi + 1;                 // padded pitch: column reads of G by consecutive k
    float *Gs = sm;                        // [H][GP]
    float *xs = Gs + H * GP;               // [kEB][Fi]
    float *ghs = xs + kEB * Fi;            // [kEB][H]
    float *part = ghs + kEB * H;           // [H*d + H] this block's dU | db_u partial
    const float *U = theta, *bu = theta + (size_t)H * d;
    const int np = H * d + H;
    for (int t = threadIdx.x; t < np; t += 256) part[t] = 0.0f;
    const int lr0 = blockIdx.x * rows_per_block;
    const int lr1 = min(n_rows_tile, lr0 + rows_per_block);
    for (int lr = lr0; lr < lr1; ++lr) {
        const int row = r0 + lr;
        __syncthreads();
        for (int t = threadIdx.x; t < H * Fi; t += 256) {
            int k = t / Fi, q = t - k * Fi;
            Gs[k * GP + q] = G[(size_t)lr * H * Fi + t];
        }
        const int w0 = rowptr[row], w1 = rowptr[row + 1];
        for (int wb = w0; wb < w1; wb += kEB) {
            const int nb = min(kEB, w1 - wb);
            __syncthreads();
            for (int t = threadIdx.x; t < nb * Fi; t += 256) {
                int b = t / Fi, q = t - b * Fi;
                xs[b * Fi + q] = x[(size_t)col[wb + b] * Fi + q];
            }
            __syncthreads();
            for (int t = threadIdx.x; t < nb * H; t += 256) {
                int b = t / H, k = t - b * H;
                int e = eid[wb + b];
                float gh = 0.0f;
                if (e >= 0) {
                    const float *dx = coords + (size_t)e * d;
                    float s = 0.0f;
                    for (int j = 0; j < d; ++j) s = s + U[k + (size_t)H * j] * dx[j];
                    s = s + bu[k];
                    if (s > 0.0f) {
                        float dh = 0.0f;
                        for (int q = 0; q < Fi; ++q) dh = fmaf(Gs[k * GP + q], xs[b * Fi + q], dh);
                        gh = dh;
                    }
                }
                ghs[b * H + k] = gh;
                if (ghbuf) ghbuf[(size_t)(wb + b) * H + k] = gh;
            }
            __syncthreads();
            // dU[k + H*j] += gh[k] dx_e[j];  db_u[k] += gh[k]   (entries of the batch in order)
            for (int t = threadIdx.x; t < np; t += 256) {
                float s = part[t];
                if (t < H * d) {
                    int j = t / H, k = t - j * H;
                    for (int b = 0; b < nb; ++b) {
                        int e = eid[wb + b];
                        if (e >= 0) s = fmaf(ghs[b * H + k], coords[(size_t)e * d + j], s);
                    }
                } else {
                    int k = t - H * d;
                    for (int b = 0; b < nb; ++b) s = s + ghs[b * H + k];
                }
                part[t] = s;
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < np; t += 256) slabs[(size_t)blockIdx.x * np + t] = part[t];
}

// ---- MFMA form of the kernel-MLP backward (H, F_in multiples of 32, <= 64; d <= 3) -----------------
// One wave per vertex i, entries in tiles of 32:
//   DH^T[e][k] = sum_q x_{j(e)}[q] G_i[k][q]                 (A = gathered neighbour rows, B = G_i^T)
//   GH = relu'(U dx_e + b_u) . DH^T                          (mask applied in the C layout)
//   dU^T[j][k] += sum_e dx_e[j] GH[e][k],  db_u[k] += sum_e GH[e][k]
//        -> second MFMA that takes the GH accumulator tile directly as its B operand (register r of
//           lane half h is row e = (r&3) + 8(r>>2) + 4h), A[j][e] = dx_e[j] for j < d and 1 for j = d.
// dU^T / db_u stay in accumulators across all vertices of the wave: one slab per wave, no atomics.
typedef float v4f_g __attribute__((ext_vector_type(4)));

template <int HT, int QT>
__global__ __launch_bounds__(256) void gno_dh_mfma_kernel(const int32_t *__restrict__ rowptr,
                                                          const int32_t *__restrict__ col,
                                                          const int32_t *__restrict__ eid,
                                                          const float *__restrict__ x,
                                                          const float *__restrict__ coords,
                                                          const float *__restrict__ theta, int d,
                                                          const float *__restrict__ G, int r0, int n_rows_tile,
                                                          float *__restrict__ slabs, float *__restrict__ ghbuf)
{
    constexpr int H = 32 * HT, Fi = 32 * QT, HF = Fi / 2;   // lane half h owns q in [HF*h, HF*h + HF)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r31 = lane & 31, h = lane >> 5;
    const int gw = blockIdx.x * 4 + wave, nw = gridDim.x * 4;
    float Uk[HT][3], bk[HT];
#pragma unroll
    for (int t = 0; t < HT; ++t) {
        bk[t] = theta[(size_t)H * d + 32 * t + r31];
#pragma unroll
        for (int j = 0; j < 3; ++j) Uk[t][j] = j < d ? theta[(32 * t + r31) + (size_t)H * j] : 0.0f;
    }
    f32x16 du[HT];
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) du[t][r] = 0.0f;

    for (int lr = gw; lr < n_rows_tile; lr += nw) {
        const int row = r0 + lr;
        const int w0 = rowptr[row], w1 = rowptr[row + 1];
        if (w0 == w1) continue;
        // B operand: G_i[k = 32t + r31][HF*h + s], s = 0..HF-1
        float gf[HT][HF];
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
            for (int m = 0; m < HF / 4; ++m) {
                const v4f_g v = *reinterpret_cast<const v4f_g *>(G + ((size_t)lr * H + 32 * t + r31) * Fi + HF * h + 4 * m);
                gf[t][4 * m] = v.x; gf[t][4 * m + 1] = v.y; gf[t][4 * m + 2] = v.z; gf[t][4 * m + 3] = v.w;
            }
        for (int wb = w0; wb < w1; wb += 32) {
            const int nb = min(32, w1 - wb);
            const int my_j = r31 < nb ? col[wb + r31] : -1;
            const int my_e = r31 < nb ? eid[wb + r31] : -1;
            // A operand: x_{j(e = r31)}[HF*h + s]
            float xf[HF];
#pragma unroll
            for (int m = 0; m < HF / 4; ++m) {
                v4f_g v = {0.0f, 0.0f, 0.0f, 0.0f};
                if (my_j >= 0 && my_e >= 0) v = *reinterpret_cast<const v4f_g *>(x + (size_t)my_j * Fi + HF * h + 4 * m);
                xf[4 * m] = v.x; xf[4 * m + 1] = v.y; xf[4 * m + 2] = v.z; xf[4 * m + 3] = v.w;
            }
            f32x16 dh[HT];
#pragma unroll
            for (int t = 0; t < HT; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) dh[t][r] = 0.0f;
#pragma unroll
                for (int s2 = 0; s2 < HF; ++s2) dh[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xf[s2], gf[t][s2], dh[t], 0, 0, 0);
            }
            // mask + the A operand of the second product, register by register
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int e_loc = (r & 3) + 8 * (r >> 2) + 4 * h;          // entry of this register's row
                const int ee = __shfl(my_e, e_loc);                        // lanes 0..31 hold the tile's entries
                const bool ok = e_loc < nb && ee >= 0;
                float dx[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (ok && j < d) dx[j] = coords[(size_t)ee * d + j];
                float amat = 0.0f;                                         // A[j = r31][e] : dx_e[j] | 1 | 0
                if (ok) amat = r31 < d ? (r31 == 0 ? dx[0] : (r31 == 1 ? dx[1] : dx[2])) : (r31 == d ? 1.0f : 0.0f);
#pragma unroll
                for (int t = 0; t < HT; ++t) {
                    float pre = 0.0f;
#pragma unroll
                    for (int j = 0; j < 3; ++j) pre = pre + Uk[t][j] * dx[j];
                    pre = pre + bk[t];
                    const float gh = (ok && pre > 0.0f) ? dh[t][r] : 0.0f;
                    if (ghbuf && e_loc < nb) ghbuf[(size_t)(wb + e_loc) * H + 32 * t + r31] = gh;
                    du[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(amat, gh, du[t], 0, 0, 0);
                }
            }
        }
    }
    // slab[j*H + k]: rows j = 0..d of the accumulator (registers 0..3 of lane half 0)
    float *slab = slabs + (size_t)gw * (H * d + H);
    if (h == 0) {
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r <= d) slab[(size_t)r * H + 32 * t + r31] = du[t][r];
    }
}

// dcoords[e, j] = sum_{entries w carrying e} sum_k U[k + H*j] gh[w, k]
__global__ void gno_dcoords_kernel(const int32_t *__restrict__ e_rowptr, const int32_t *__restrict__ e_ent,
                                   const float *__restrict__ ghbuf, const float *__restrict__ theta, int d, int H,
                                   int E, float *__restrict__ dcoords)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= E * d) return;
    int e = t / d, j = t - e * d;
    float s = 0.0f;
    for (int p = e_rowptr[e]; p < e_rowptr[e + 1]; ++p) {
        const float *gh = ghbuf + (size_t)e_ent[p] * H;
        for (int k = 0; k < H; ++k) s = fmaf(theta[k + (size_t)H * j], gh[k], s);
    }
    dcoords[t] = s;
}

int launch_outer(const int32_t *rowptr, const int32_t *idx, const int32_t *eidx, const float *y, int Fy,
                 const float *coords, const float *theta, int d, int H, int r0, int rows, float *S)
{
    const int R = (H + 1) * Fy;
    if (H % 32 == 0 && Fy % 32 == 0 && H <= 64 && Fy <= 64 && d <= 4) {
        dim3 g4((rows + 3) / 4), b4(256);
#define AMP_OM(A_, B_)                                                                                   \
    if (H == 32 * A_ && Fy == 32 * B_)                                                                   \
        hipLaunchKernelGGL((gno_outer_mfma_kernel<A_, B_>), g4, b4, 0, amp::stream(), rowptr, idx, eidx, y, coords, \
                           theta, d, r0, rows, S);
        AMP_OM(1, 1) AMP_OM(1, 2) AMP_OM(2, 1) AMP_OM(2, 2)
#undef AMP_OM
        AMP_LAUNCH_CHECK();
        return 0;
    }
    const size_t lds = sizeof(float) * kEB * (size_t)(H + 1 + Fy);
    dim3 grid(rows), block(256);
#define AMP_OUT(E_)                                                                                      \
    hipLaunchKernelGGL((gno_outer_kernel<E_>), grid, block, lds, amp::stream(), rowptr, idx, eidx, y, Fy, \
                       coords, theta, d, H, r0, S)
    if (R <= 256) AMP_OUT(1);
    else if (R <= 1024) AMP_OUT(4);
    else if (R <= 5120) AMP_OUT(20);
    else if (R <= 17408) AMP_OUT(68);
    else {
        amp::set_error("gno: (H+1)*F = %d exceeds the supported 17408", R);
        return 2;
    }
#undef AMP_OUT
    AMP_LAUNCH_CHECK();
    return 0;
}

int tile_rows_for(int64_t n_rows, int64_t floats_per_row)
{
    constexpr int64_t budget = (int64_t)1024 << 20;   // bytes of S / T / G per super-tile: 1 GiB, two slots in flight (bwd_theta pipeline);
                                                      // 43.8 ms at C4 against 44.4 at 2 GiB
    int64_t t = budget / (4 * std::max<int64_t>(floats_per_row, 1));
    t = std::max<int64_t>(1, std::min<int64_t>(t, n_rows));
    return (int)t;
}

bool gno_args_ok(const athena_mp_graph *g, int d, int H, int Fi, int Fo)
{
    if (!g || d <= 0 || H <= 0 || Fi <= 0 || Fo <= 0) {
        amp::set_error("gno: bad arguments (d=%d H=%d F_in=%d F_out=%d)", d, H, Fi, Fo);
        return false;
    }
    if ((size_t)kEB * (H + 1 + std::max(Fi, Fo)) * 4 > 60000 || ((size_t)H * (Fi + 1) + kEB * (Fi + H) + H * d + H) * 4 > 150000) {
        amp::set_error("gno: H=%d, F=%d exceed the LDS staging of this build", H, std::max(Fi, Fo));
        return false;
    }
    return true;
}

// out[r,:] = S_r . B for the n_rows rows of a CSR, S through HBM one super-tile at a time; B [(H+1) Fy][Fout] row-major
int outer_then_contract(const int32_t *rowptr, const int32_t *idx, const int32_t *eidx, const float *y, int Fy, const float *coords,
                        const float *theta, int d, int H, int n_rows, const float *B, int Fout, float *out)
{
    const int R = (H + 1) * Fy;
    const int tile = tile_rows_for(n_rows, R);
    for (int r0 = 0; r0 < n_rows; r0 += tile) {
        const int rows = std::min(tile, n_rows - r0);
        void *ws = nullptr;
        if (amp::workspace(&ws, sizeof(float) * (size_t)rows * R, 0)) return 1;
        int rc = launch_outer(rowptr, idx, eidx, y, Fy, coords, theta, d, H, r0, rows, (float *)ws);
        if (rc) return rc;
        rc = amp::gemm_dispatch((const float *)ws, B, 0, nullptr, ATHENA_MP_ACT_NONE, out + (size_t)r0 * Fout, rows, R, Fout);
        if (rc) return rc;
    }
    return 0;
}

// the feature gradient in pull form over the n_rows rows of one CSR of g (its own or the transposed one, `order` the row-length
// order of that CSR): dx[r,:] = sum_{w in row r} K_{eidx[w]}^T grad[idx[w],:], grad [y_rows, Fo]
int pull_dx(const athena_mp_graph *g, const int32_t *rowptr, const int32_t *idx, const int32_t *eidx, int n_rows, int y_rows,
            LenOrder *order, int d, int H, int Fi, int Fo, const float *theta, const float *coords, const float *grad, float *dx)
{
    const size_t off_V = (size_t)H * d + H;
    const int R2 = (H + 1) * Fo;
    void *b2 = nullptr;
    if (amp::workspace(&b2, sizeof(float) * (size_t)R2 * Fi, 3)) return 1;
    const int n = R2 * Fi;
    hipLaunchKernelGGL(gno_perm_kernel, dim3((n + 255) / 256), dim3(256), 0, amp::stream(), theta + off_V, H + 1, Fi, Fo, (float *)b2);
    AMP_LAUNCH_CHECK();
    if (amp::gno64_shape(H, Fo, Fi, d, 4) && amp::aligned16(grad, dx))   // rows in and out 16 bytes per lane
        return amp::launch_gno_fused(rowptr, idx, eidx, grad, coords, theta, d, (const float *)b2, n_rows, order, dx, y_rows,
                                     g->n_edge_cols, g->nnz);
    return outer_then_contract(rowptr, idx, eidx, grad, Fo, coords, theta, d, H, n_rows, (const float *)b2, Fi, dx);
}

// kernel-MLP backward of any shape: G through HBM one super-tile at a time
int mlp_backward_tiled(const athena_mp_graph *g, int d, int H, int Fi, int Fo, const float *theta, const float *coords,
                       const float *x, const float *grad, float *dtheta, float *ghbuf)
{
    const size_t off_V = (size_t)H * d + H;
    const int np = H * d + H;
    const int HF = H * Fi;
    const int tile = tile_rows_for(g->n_rows, HF);
    const size_t lds = sizeof(float) * ((size_t)H * (Fi + 1) + (size_t)kEB * (Fi + H) + np);
    static amp::PerDeviceFlag attr;
    if (!attr.get()) {
        AMP_HIP(hipFuncSetAttribute((const void *)gno_dh_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr.get() = true;
    }
    bool first = true;
    for (int r0 = 0; r0 < g->n_rows; r0 += tile) {
        const int rows = std::min(tile, g->n_rows - r0);
        void *gw = nullptr;
        if (amp::workspace(&gw, sizeof(float) * (size_t)rows * HF, 1)) return 1;
        // G[r, (k,q)] = sum_o g[r,o] V[o + Fo*q + F*k]: B stored [N=(k,q)][K=o] = theta + off_V
        int rc = amp::gemm_dispatch(grad + (size_t)r0 * Fo, theta + off_V, 1, nullptr, ATHENA_MP_ACT_NONE,
                                    (float *)gw, rows, Fo, HF);
        if (rc) return rc;
        int nblk;
        void *sl = nullptr;
        const bool mf = H % 32 == 0 && Fi % 32 == 0 && H <= 64 && Fi <= 64 && d <= 3 && amp::aligned16(x);   // x rows 16 bytes per lane
        if (mf) {
            nblk = std::min((rows + 3) / 4, 512);      // 4 waves per workgroup, one slab per wave
            if (amp::workspace(&sl, sizeof(float) * (size_t)nblk * 4 * np, 3)) return 1;
#define AMP_DH(A_, B_)                                                                                     \
    if (H == 32 * A_ && Fi == 32 * B_)                                                                     \
        hipLaunchKernelGGL((gno_dh_mfma_kernel<A_, B_>), dim3(nblk), dim3(256), 0, amp::stream(), g->rowptr, g->col, \
                           g->eid, x, coords, theta, d, (const float *)gw, r0, rows, (float *)sl, ghbuf);
            AMP_DH(1, 1) AMP_DH(1, 2) AMP_DH(2, 1) AMP_DH(2, 2)
#undef AMP_DH
            nblk *= 4;
        } else {
            nblk = std::min(rows, 512);
            int rpb = (rows + nblk - 1) / nblk;
            nblk = (rows + rpb - 1) / rpb;
            if (amp::workspace(&sl, sizeof(float) * (size_t)nblk * np, 3)) return 1;
            hipLaunchKernelGGL(gno_dh_kernel, dim3(nblk), dim3(256), lds, amp::stream(), g->rowptr, g->col, g->eid, x, Fi,
                               coords, theta, d, H, (const float *)gw, r0, rows, rpb, (float *)sl, ghbuf);
        }
        AMP_LAUNCH_CHECK();
        if (dtheta) {
            if (int rc2 = amp::slab_reduce((const float *)sl, nblk, np, dtheta, !first)) return rc2;
        }
        first = false;
    }
    if (dtheta && g->n_rows == 0) AMP_HIP(hipMemsetAsync(dtheta, 0, sizeof(float) * np, amp::stream()));
    return 0;
}

// shared backward of the kernel MLP: dU, db_u (dtheta) and/or dcoords; px / px_half / cvec: the one-call reverse pass also
// takes the feature gradient's per-entry partials from it (gno_dh_pc_kernel<.., PX = true>)
int gno_mlp_backward(const athena_mp_graph *g, int d, int H, int Fi, int Fo, const float *theta,
                     const float *coords, const float *x, const float *grad, float *dtheta, float *dcoords,
                     float *px = nullptr, size_t px_half = 0, const float *cvec = nullptr)
{
    float *ghbuf = nullptr;
    if (dcoords) {
        void *p = nullptr;
        if (amp::workspace(&p, sizeof(float) * (size_t)std::max<int64_t>(g->nnz, 1) * H, 4)) return 1;
        ghbuf = (float *)p;
    }
    const int rc = amp::gno64_shape(H, Fi, Fo, d, 3) && g->n_rows > 0 && amp::aligned16(x, grad)
                       ? amp::gno64_mlp_backward(g, d, theta, coords, x, grad, dtheta, ghbuf, px, px_half, cvec)
                       : mlp_backward_tiled(g, d, H, Fi, Fo, theta, coords, x, grad, dtheta, ghbuf);
    if (rc) return rc;
    if (dcoords && g->n_edge_cols > 0) {
        int64_t n = (int64_t)g->n_edge_cols * d;
        hipLaunchKernelGGL(gno_dcoords_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, amp::stream(),
                           g->e_rowptr, g->e_col, ghbuf, theta, d, H, g->n_edge_cols, dcoords);
        AMP_LAUNCH_CHECK();
    }
    return 0;
}

} // namespace

using namespace amp;

extern "C" {

int athena_mp_gno_aggregate_fwd(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo,
                                const float *theta, const float *coords, const float *x, float *m)
{
    if (!gno_args_ok(g, d, H, Fi, Fo)) return 2;
    AMP_REQUIRE(theta && coords && x && m, "gno_aggregate_fwd: null pointer");
    const size_t off_V = (size_t)H * d + H;
    if (gno64_shape(H, Fi, Fo, d, 4) && aligned16(x, m, theta))   // (theta: gno_fused_kernel reads V 16 bytes per lane)
        return launch_gno_fused(g->rowptr, g->col, g->eid, x, coords, theta, d, theta + off_V, g->n_rows, &g->len_fwd, m, g->n_cols,
                                g->n_edge_cols, g->nnz);
    // m[r,o] = sum_{(k,q)} S[r,(k,q)] Vaug[o + Fo*(q + Fi*k)]: B = theta+off_V viewed [R][Fo] row-major
    return outer_then_contract(g->rowptr, g->col, g->eid, x, Fi, coords, theta, d, H, g->n_rows, theta + off_V, Fo, m);
}

// ---- training-mode pair: the forward pass keeps S for the reverse pass's S^T g ---------------------------------------
int athena_mp_gno_saved_bytes(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo, int64_t *bytes)
{
    if (!gno_args_ok(g, d, H, Fi, Fo)) return 2;
    AMP_REQUIRE(bytes, "gno_saved_bytes: null pointer");
    *bytes = gno64_saved_bytes(g, d, H, Fi, Fo);
    return 0;
}

int athena_mp_gno_aggregate_fwd_save(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo,
                                     const float *theta, const float *coords, const float *x, float *m, float *s_save)
{
    if (!gno_args_ok(g, d, H, Fi, Fo)) return 2;
    AMP_REQUIRE(theta && coords && x && m && s_save, "gno_aggregate_fwd_save: null pointer");
    AMP_REQUIRE(gno64_saved_bytes(g, d, H, Fi, Fo) > 0,
                "gno_aggregate_fwd_save: this shape does not keep S (athena_mp_gno_saved_bytes returned 0)");
    // the one kernel that writes S moves x, m and S 16 bytes per lane, and S has no other producer
    AMP_REQUIRE(aligned16(x, m, s_save), "gno_aggregate_fwd_save: x, m and s_save must be 16-byte aligned (athena_mp_gno_aggregate_fwd "
                                         "takes any alignment)");
    const size_t off_V = (size_t)H * d + H;
    return launch_gno_fused(g->rowptr, g->col, g->eid, x, coords, theta, d, theta + off_V, g->n_rows, &g->len_fwd, m, g->n_cols,
                            g->n_edge_cols, g->nnz, s_save);
}

int athena_mp_gno_aggregate_bwd_theta_saved(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo,
                                            const float *theta, const float *coords, const float *x, const float *grad,
                                            const float *s_save, float *dtheta)
{
    if (!gno_args_ok(g, d, H, Fi, Fo)) return 2;
    AMP_REQUIRE(theta && coords && x && grad && s_save && dtheta, "gno_aggregate_bwd_theta_saved: null pointer");
    AMP_REQUIRE(gno64_saved_bytes(g, d, H, Fi, Fo) > 0,
                "gno_aggregate_bwd_theta_saved: this shape does not keep S (athena_mp_gno_saved_bytes returned 0)");
    if (!aligned16(x, grad, s_save))   // S is a function of x, coords and theta: the entry that rebuilds it takes any alignment
        return athena_mp_gno_aggregate_bwd_theta(g, d, H, Fi, Fo, theta, coords, x, grad, dtheta);
    const size_t off_V = (size_t)H * d + H;
    const int rc = launch_gno_stg(g, x, coords, theta, d, grad, dtheta + off_V, s_save);
    if (rc) {
        if (rc < 0) set_error("gno_aggregate_bwd_theta_saved: tensors beyond the 4 GB a buffer descriptor addresses");
        return rc < 0 ? 2 : rc;
    }
    return gno_mlp_backward(g, d, H, Fi, Fo, theta, coords, x, grad, dtheta, nullptr);
}

int athena_mp_gno_aggregate_bwd_x(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo,
                                  const float *theta, const float *coords, const float *grad, float *dx)
{
    if (!gno_args_ok(g, d, H, Fi, Fo)) return 2;
    AMP_REQUIRE(theta && coords && grad && dx, "gno_aggregate_bwd_x: null pointer");
    return pull_dx(g, g->t_rowptr, g->t_src, g->t_eid, g->n_cols, g->n_rows, &g->len_bwd, d, H, Fi, Fo, theta, coords, grad, dx);
}

/* The reverse pass of gno_aggregate towards the features in PULL form over the graph's OWN rows:
 *     dx[v,:] = sum_{w in row v} K_{eid[w]}^T grad_ext[col[w],:]          v < n_rows, grad_ext [n_cols, Fo]
 * For an undirected graph whose two directions share one edge column (athena's graphs: row u lists (v, e) whenever row v
 * lists (u, e), athena_diffstruc_extd_sub_nop.f90:369-376) this is the reference's scatter dx_j += K_e^T g_i
 * (:419-458) read from the receiving side.  It is what a row block of a partitioned graph can evaluate: the block holds
 * its own rows, and the gradient rows of the remote neighbours arrive by the same halo exchange as the features
 * (athena_mp_shard_create_edges checks the symmetry).  Same kernels as athena_mp_gno_aggregate_bwd_x, walking
 * rowptr / col / eid instead of the transposed arrays. */
int athena_mp_gno_aggregate_bwd_x_pull(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo,
                                       const float *theta, const float *coords, const float *grad_ext, float *dx)
{
    if (!gno_args_ok(g, d, H, Fi, Fo)) return 2;
    AMP_REQUIRE(theta && coords && grad_ext && dx, "gno_aggregate_bwd_x_pull: null pointer");
    return pull_dx(g, g->rowptr, g->col, g->eid, g->n_rows, g->n_cols, &g->len_fwd, d, H, Fi, Fo, theta, coords, grad_ext, dx);
}

int athena_mp_gno_aggregate_bwd_theta(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo,
                                      const float *theta, const float *coords, const float *x, const float *grad,
                                      float *dtheta)
{
    if (!gno_args_ok(g, d, H, Fi, Fo)) return 2;
    AMP_REQUIRE(theta && coords && x && grad && dtheta, "gno_aggregate_bwd_theta: null pointer");
    const size_t off_V = (size_t)H * d + H;
    const int R = (H + 1) * Fi;
    // dVaug = S^T g  (dV and db_v in one contraction; the bias row of S is s_i = sum_j x_j)
    // S goes through HBM one super-tile at a time.  The two kernels of a super-tile lean on different resources -- the
    // outer product is bound by its 2 GiB of writes, the contraction by the matrix pipe and reads -- so they are
    // pipelined over two workspace slots: the outer product of tile t+1 runs on the library's second stream while the
    // contraction of tile t runs on the caller's.
    const int tile = tile_rows_for(g->n_rows, R);
    if (g->n_rows == 0) AMP_HIP(hipMemsetAsync(dtheta + off_V, 0, sizeof(float) * (size_t)R * Fo, stream()));
    if (g->n_rows > 0 && gno64_shape(H, Fi, Fo, d, 3) && aligned16(x, grad)) {   // S stays on chip (gno_stg_kernel)
        const int rc = launch_gno_stg(g, x, coords, theta, d, grad, dtheta + off_V);
        if (rc == 0) return gno_mlp_backward(g, d, H, Fi, Fo, theta, coords, x, grad, dtheta, nullptr);
        if (rc > 0) return rc;
    }
    const int n_tiles = g->n_rows > 0 ? (g->n_rows + tile - 1) / tile : 0;
    if (n_tiles < 2) {
        for (int r0 = 0; r0 < g->n_rows; r0 += tile) {
            const int rows = std::min(tile, g->n_rows - r0);
            void *ws = nullptr;
            if (workspace(&ws, sizeof(float) * (size_t)rows * R, 0)) return 1;
            int rc = launch_outer(g->rowptr, g->col, g->eid, x, Fi, coords, theta, d, H, r0, rows, (float *)ws);
            if (rc) return rc;
            rc = gemm_dw_dispatch(rows, R, Fo, (const float *)ws, grad + (size_t)r0 * Fo, dtheta + off_V, r0 > 0);
            if (rc) return rc;
        }
    } else {
        hipStream_t main_s = stream(), aux = nullptr;
        hipEvent_t *ev = nullptr;
        if (amp::aux_stream(&aux, &ev)) return 1;
        void *wsl[2] = {nullptr, nullptr};
        if (workspace(&wsl[0], sizeof(float) * (size_t)tile * R, 0) || workspace(&wsl[1], sizeof(float) * (size_t)tile * R, 8)) return 1;
        // ev[0]: inputs ready (main -> aux); ev[1 + slot]: S of the slot written (aux -> main); ev[3 + slot]: consumed
        AMP_HIP(hipEventRecord(ev[0], main_s));
        AMP_HIP(hipStreamWaitEvent(aux, ev[0], 0));
        int rc = 0;
        for (int t = 0; t < n_tiles && rc == 0; ++t) {
            const int slot = t & 1, r0 = t * tile, rows = std::min(tile, g->n_rows - r0);
            if (t >= 2) rc = hipStreamWaitEvent(aux, ev[3 + slot], 0) == hipSuccess ? 0 : 1;
            amp::swap_stream(aux);
            if (rc == 0) rc = launch_outer(g->rowptr, g->col, g->eid, x, Fi, coords, theta, d, H, r0, rows, (float *)wsl[slot]);
            amp::swap_stream(main_s);
            if (rc == 0 && hipEventRecord(ev[1 + slot], aux) != hipSuccess) rc = 1;
            if (rc == 0 && hipStreamWaitEvent(main_s, ev[1 + slot], 0) != hipSuccess) rc = 1;
            if (rc == 0) rc = gemm_dw_dispatch(rows, R, Fo, (const float *)wsl[slot], grad + (size_t)r0 * Fo, dtheta + off_V, t > 0);
            if (rc == 0 && hipEventRecord(ev[3 + slot], main_s) != hipSuccess) rc = 1;
        }
        amp::swap_stream(main_s);
        if (rc) {
            if (athena_mp_last_error()[0] == 0) set_error("gno_aggregate_bwd_theta: stream pipeline failed");
            return rc;
        }
    }
    return gno_mlp_backward(g, d, H, Fi, Fo, theta, coords, x, grad, dtheta, nullptr);
}

/* The whole reverse pass of gno_aggregate from ONE G = g . Vmat^T (athena_diffstruc_extd_sub_nop.f90:419-458 features,
 * :235-325 kernel parameters, :137-216 coordinates): any of dx / dtheta / dcoords may be NULL.  Shapes and sizes that take
 * the producer / consumer kernels (H = F_in = F_out = 64, d <= 3, tensors below 4 GB, at most 1 row in 64 longer than 32
 * entries) run:  S^T g (streamed from s_save when given, rebuilt otherwise) -> dVaug;  gno_dh_pc_kernel<PX> -> dU, db_u,
 * the per-entry partials of dx [nnz][64] (and the per-entry dh for dcoords);  gno_px_gather_kernel -> dx.  Everything
 * else is the three separate entry points, one after the other.  *fused (may be NULL) says which it was. */
int athena_mp_gno_aggregate_bwd(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo, const float *theta,
                                const float *coords, const float *x, const float *grad, const float *s_save, float *dx,
                                float *dtheta, float *dcoords, int32_t *fused)
{
    if (!gno_args_ok(g, d, H, Fi, Fo)) return 2;
    AMP_REQUIRE(theta && coords && x && grad, "gno_aggregate_bwd: null pointer");
    if (fused) *fused = 0;
    bool ok = false;
    if (gno64_one_call_reverse(g, d, H, Fi, Fo, dx != nullptr, &ok)) return 1;
    ok = ok && aligned16(x, grad, dx, s_save);   // the one-call kernels move all four 16 bytes per lane
    auto separate = [&]() -> int {   // the three entry points one after the other: no workspace of nnz * 256 bytes
        if (dtheta) {
            const int rc = s_save ? athena_mp_gno_aggregate_bwd_theta_saved(g, d, H, Fi, Fo, theta, coords, x, grad, s_save, dtheta)
                                  : athena_mp_gno_aggregate_bwd_theta(g, d, H, Fi, Fo, theta, coords, x, grad, dtheta);
            if (rc) return rc;
        }
        if (dx)
            if (const int rc = athena_mp_gno_aggregate_bwd_x(g, d, H, Fi, Fo, theta, coords, grad, dx)) return rc;
        if (dcoords)
            if (const int rc = athena_mp_gno_aggregate_bwd_coords(g, d, H, Fi, Fo, theta, coords, x, grad, dcoords)) return rc;
        return 0;
    };
    if (!ok) return separate();
    const size_t off_V = (size_t)H * d + H;
    const size_t px_half = (size_t)std::max<int64_t>(g->nnz, 1) * Fi;
    void *pxp = nullptr, *cvp = nullptr, *dth_tmp = nullptr;
    // The fused route keeps nnz * 256 bytes of per-entry partials (7.6 GB at BASELINE configs[3]) and nnz int32 in the handle.
    // When the device cannot give them -- a larger graph, a smaller device, a layer that also keeps S -- the call does what it
    // did before the fused route existed: the separate entry points, which run in the memory there is.
    // Whichever of the three allocations fails, what the earlier ones took goes back first: the separate entry points must find
    // at least the memory they had before the fused route existed.
    auto give_up = [&]() -> int {
        (void)hipGetLastError();   // the failed allocation must not surface in the next launch check
        if (workspace_release(13) || workspace_release(14)) return 1;
        return separate();
    };
    if (workspace(&pxp, sizeof(float) * px_half, 13) || workspace(&cvp, sizeof(float) * Fi * (size_t)g->n_rows, 14)) return give_up();
    if (const int rc = gno64_t_entry(g)) {
        if (rc < 0) return give_up();
        return rc;
    }
    // c_i = b_v^T g_i for every row (b_v viewed [q][o]): one weight-resident GEMM launch
    if (int rc = gemm_dispatch(grad, theta + off_V + (size_t)Fo * Fi * H, /*b_nk=*/1, nullptr, ATHENA_MP_ACT_NONE, (float *)cvp,
                               g->n_rows, Fo, Fi))
        return rc;
    float *dth = dtheta;
    if (!dth) {   // dx alone still runs the fused kernel; its parameter sums go to a scratch vector
        if (workspace(&dth_tmp, sizeof(float) * (off_V + (size_t)Fo * Fi * (H + 1)), 15)) return 1;
        dth = (float *)dth_tmp;
    }
    // Order: the kernel MLP's launches (they write the partials) -> the gather of the partials and S^T g SIDE BY SIDE.  The two
    // share nothing but grad: the gather is a stream of 16-byte loads without LDS in 56 registers, S^T g leaves exactly that
    // many free per SIMD (3 waves x 152) and is bound by the matrix pipe, so the gather runs on the library's second stream in
    // the slots S^T g cannot use (A/B against everything on the caller's stream: docs/history/DESIGN_r01-r04.md, round 4).
    if (int rc = gno_mlp_backward(g, d, H, Fi, Fo, theta, coords, x, grad, dth, dcoords, (float *)pxp, px_half, (const float *)cvp)) return rc;
    hipStream_t main_s = stream(), gs = main_s;
    hipEvent_t *ev = nullptr;
    if (dtheta) {   // (side by side 26.6 - 27.3 ms against 28.9 with every launch on one stream: profiles/r04_c4_config.jsonl)
        if (amp::aux_stream(&gs, &ev)) return 1;
        AMP_HIP(hipEventRecord(ev[0], main_s));
        AMP_HIP(hipStreamWaitEvent(gs, ev[0], 0));
    }
    const int gather_rc = gno64_px_gather(g, (const float *)pxp, dx, gs);
    if (gs != main_s) AMP_HIP(hipEventRecord(ev[1], gs));
    int rc = 0;
    if (gather_rc == 0 && dtheta) rc = launch_gno_stg(g, x, coords, theta, d, grad, dtheta + off_V, s_save);
    // joined whatever happened above: the caller's stream never leaves this call with work it cannot see
    if (gs != main_s) AMP_HIP(hipStreamWaitEvent(main_s, ev[1], 0));
    if (gather_rc) return gather_rc;
    if (rc) {
        if (rc < 0) set_error("gno_aggregate_bwd: tensors beyond the 4 GB a buffer descriptor addresses");
        return rc < 0 ? 2 : rc;
    }
    if (fused) *fused = 1;
    return 0;
}

int athena_mp_gno_aggregate_bwd_coords(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo,
                                       const float *theta, const float *coords, const float *x,
                                       const float *grad, float *dcoords)
{
    if (!gno_args_ok(g, d, H, Fi, Fo)) return 2;
    AMP_REQUIRE(theta && coords && x && grad && dcoords, "gno_aggregate_bwd_coords: null pointer");
    return gno_mlp_backward(g, d, H, Fi, Fo, theta, coords, x, grad, nullptr, dcoords);
}

} // extern "C"
