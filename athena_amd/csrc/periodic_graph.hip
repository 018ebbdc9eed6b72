// Periodic structures -> neighbour graphs on the device, a whole batch per call: the step in front of
// athena_mp_graph_create_from_edges_dev for the reference's chemical examples.  It replaces get_graph_from_basis
// (example/example_library/src/mod_read_chemical_graphs.f90:196-278), which walks every atom pair i <= j and every lattice image on
// the host, one structure at a time, and appends to the edge array once per edge.
//
// The definition (every implementation gives the same arrays; tests compare with np.array_equal).  Structure s owns the atoms
// offsets[s] .. offsets[s+1]-1; frac [n, 3] are fractional coordinates, lat [B, 3, 3] row-major, row a = lattice vector a in
// Cartesian components; pbc[k] = 0 makes axis k open (neither wrapped nor imaged).  For local atoms i <= j of one structure and an
// integer shift (a, b, c), every operation rounded to fp32 on its own (the library is built with -ffp-contract=off):
//   f_k = frac_i[k] - frac_j[k]
//   w_k = f_k - ceil(f_k - 0.5) on a periodic axis;  w_k = f_k, and only shift 0, on an open axis
//   v   = (w_0 + a, w_1 + b, w_2 + c)
//   x_c = ((v_0 * L[0][c]) + v_1 * L[1][c]) + v_2 * L[2][c]         c = 0, 1, 2
//   s   = ((x_0 * x_0) + x_1 * x_1) + x_2 * x_2,   r = sqrt(s) correctly rounded
// The triple is an edge iff r > cutoff_min and r < cutoff_max, both strict as in the reference.  So the zero-shift self pair is
// never an edge, an atom is joined to its own images (i = j gives +shift and -shift, as the reference's loop does; each is one CSR
// entry under csr_from_edges_core), and a pair carries one edge per image in range.  Edges are ordered by structure and inside a
// structure lexicographically by (i, j, a, b, c), each ascending; the 1-based rank over the batch is the edge id.
//   pairs [2, E] column-major, 1-based global vertex ids, smaller first;  feature [E] = r / cutoff_max (correctly rounded);
//   vec [E, 3] = x (atom i minus the image of atom j: the sign of coords in athena_mp_radius_pairs);  shift [E, 3];
//   first_count [n] = edges whose FIRST index is that vertex (j >= i only: the reference's `degree`, :256, :270);
//   edge_offsets [B+1] (host) = where each structure's edge columns start.
//
// The set of shifts is all of Z^3 on the periodic axes; the search range has to cover every kept one.  With G = L^-1 (columns
// g_a = (L_b x L_c) / det L), v_a = x . g_a exactly, so |v_a| <= |x| |g_a| < cutoff_max |L_b x L_c| / |det L| = h_a for a kept
// triple, and |a| = |v_a - w_a| <= |v_a| + 1/2 < h_a + 1/2: every kept shift has |a| <= floor(h_a + 1/2).  (Open axes change
// nothing: the identity is linear algebra, and their shift is 0.)  The kernel evaluates h_a in fp64 from the fp32 lattice and
// searches floor(h_a + 1/2) + 1: the margin of one covers what rounding adds -- the fp32 w_k lies within an ulp of
// [-1/2, 1/2], and the computed x differs from the exact v . L by at most 3 * 2^-24 * sum_k |v_k| |L_k|, which moves v_a by far
// less than one for any cell that passes the half-range limit below with lattice vectors up to ~10^3 cutoffs long.  A structure
// whose floor(h_a + 1/2) exceeds kMaxHalfRange on some axis is refused: the cell is too small for the cutoff.
//
// How: structures are tiny (8 - 30 atoms) and there are very many, so there is no grid and the enumeration order IS the output
// order.  The host cuts structures into work items (structure, rows i0 .. i1-1) of at most kItemPairs pairs (a structure of up to
// 31 atoms is one item; a row is never cut).  One 64-lane wave owns an item: for each row i it walks the candidates
// (j - i, a, b, c) in linear order, 64 per step -- each lane keeps its candidate as a mixed-radix counter and adds the digits of 64,
// no division in the loop -- decides the predicate, takes a ballot and ranks the kept lanes with mbcnt on a running base.  COUNT
// pass: per-item totals; exclusive 64-bit scan over the items (scan64.h); FILL pass: the same walk writes every output at its
// final position, and first_count per row.  No sort, no atomics: two builds are byte-identical.  The structure's fractional rows
// sit in LDS when it has at most kLdsAtoms atoms; a larger one is read from global memory (correct, not fast; a cell grid for
// large supercells is out of scope).
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "scan64.h"

namespace {

constexpr int kMaxHalfRange = 31;    // floor(h_a + 1/2) above this is refused; the search adds the margin of one
constexpr int kItemPairs = 512;      // pairs (i, j) per work item, unless one row alone has more
constexpr int kLdsAtoms = 128;       // structures with more atoms than this are read from global memory
constexpr int kWaves = 4;            // work items per 256-thread block
constexpr int kCheckBlocks = 256;

struct PgInfo {
    int32_t R[3];      // searched half-range per axis (0 on an open axis); for status 3 the offending floor(h + 1/2) is in R[axis]
    int32_t status;    // 0 good, 1 non-finite lattice entry, 2 det L zero or not finite, 3 half-range above kMaxHalfRange
};

struct PgPbc {
    int32_t p[3];
};

__device__ inline unsigned long long block_min64(unsigned long long v)
{
    __shared__ unsigned long long part[256];
    part[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && part[threadIdx.x + s] < part[threadIdx.x]) part[threadIdx.x] = part[threadIdx.x + s];
        __syncthreads();
    }
    const unsigned long long r = part[0];
    __syncthreads();
    return r;
}

// thread t looks at structure t (lattice, det, half-ranges -> info[t]) and at the coordinates of atom t.
// partial[2 * block] = first structure with a non-zero status, partial[2 * block + 1] = first atom with a non-finite coordinate
__global__ __launch_bounds__(256) void pg_prepare_kernel(int32_t B, int32_t n, const float *__restrict__ frac, const float *__restrict__ lat,
                                                         PgPbc pbc, float cutoff_max, PgInfo *__restrict__ info,
                                                         unsigned long long *__restrict__ partial)
{
    unsigned long long bad_s = ~0ull, bad_a = ~0ull;
    const int64_t top = B > n ? B : n;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < top; t += (int64_t)gridDim.x * 256) {
        if (t < n) {
            const bool ok = isfinite(frac[3 * t]) && isfinite(frac[3 * t + 1]) && isfinite(frac[3 * t + 2]);
            if (!ok && (unsigned long long)t < bad_a) bad_a = (unsigned long long)t;
        }
        if (t < B) {
            double L[3][3];
            bool finite = true;
            for (int k = 0; k < 9; ++k) {
                const float v = lat[9 * t + k];
                finite = finite && isfinite(v);
                L[k / 3][k % 3] = (double)v;
            }
            PgInfo I = {{0, 0, 0}, 0};
            if (!finite) I.status = 1;
            else if (pbc.p[0] || pbc.p[1] || pbc.p[2]) {
                double X[3][3];   // X[a] = L_b x L_c, (a, b, c) cyclic
                for (int a = 0; a < 3; ++a) {
                    const double *u = L[(a + 1) % 3], *w = L[(a + 2) % 3];
                    X[a][0] = u[1] * w[2] - u[2] * w[1];
                    X[a][1] = u[2] * w[0] - u[0] * w[2];
                    X[a][2] = u[0] * w[1] - u[1] * w[0];
                }
                const double det = L[0][0] * X[0][0] + L[0][1] * X[0][1] + L[0][2] * X[0][2];
                if (!(isfinite(det) && det != 0.0)) I.status = 2;
                else
                    for (int a = 0; a < 3; ++a) {
                        if (!pbc.p[a]) continue;
                        const double h = (double)cutoff_max * sqrt(X[a][0] * X[a][0] + X[a][1] * X[a][1] + X[a][2] * X[a][2]) / fabs(det);
                        const double fl = floor(h + 0.5);
                        if (!(fl <= (double)kMaxHalfRange)) {
                            if (I.status == 0) {               // the first such axis, alone in R
                                I.status = 3;
                                I.R[0] = I.R[1] = I.R[2] = 0;
                                I.R[a] = fl < 2.0e9 ? (int32_t)fl : INT32_MAX;
                            }
                        } else if (I.status == 0)
                            I.R[a] = (int32_t)fl + 1;
                    }
            }
            info[t] = I;
            if (I.status != 0 && (unsigned long long)t < bad_s) bad_s = (unsigned long long)t;
        }
    }
    bad_s = block_min64(bad_s);
    bad_a = block_min64(bad_a);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = bad_s;
        partial[2 * blockIdx.x + 1] = bad_a;
    }
}

struct PgOut {
    int32_t *pairs;
    float *feature, *vec;
    int32_t *shift, *first_count;
    unsigned long long total;   // no write at or beyond this rank
};

// The rows i0 .. i1-1 of one structure, walked by one wave.  rows: the structure's fractional coordinates (LDS or global).
// Returns the number of edges found; FILL writes them from rank `base` on.
template <bool FILL>
__device__ __forceinline__ unsigned long long pg_walk_item(const float *rows, int32_t m, int32_t i0, int32_t i1, int32_t v0,
                                                           const float *__restrict__ lat, const PgInfo &I, PgPbc pbc, float cutoff_min,
                                                           float cutoff_max, unsigned long long base, const PgOut &out)
{
    const uint32_t lane = threadIdx.x & 63;
    float L[3][3];
#pragma unroll
    for (int k = 0; k < 9; ++k) L[k / 3][k % 3] = lat[k];
    const int32_t R0 = I.R[0], R1 = I.R[1], R2 = I.R[2];
    const uint32_t S0 = 2 * R0 + 1, S1 = 2 * R1 + 1, S2 = 2 * R2 + 1;
    // candidate t of a row = (((j - i) * S0 + a') * S1 + b') * S2 + c', shift = (a' - R0, b' - R1, c' - R2): the digits of this
    // lane's first candidate (t = lane) and of the step (64)
    uint32_t q = lane;
    const uint32_t c_first = q % S2; q /= S2;
    const uint32_t b_first = q % S1; q /= S1;
    const uint32_t a_first = q % S0;
    const uint32_t j_first = q / S0;
    q = 64;
    const uint32_t c_step = q % S2; q /= S2;
    const uint32_t b_step = q % S1; q /= S1;
    const uint32_t a_step = q % S0;
    const uint32_t j_step = q / S0;

    for (int32_t i = i0; i < i1; ++i) {
        const float fi0 = rows[3 * i], fi1 = rows[3 * i + 1], fi2 = rows[3 * i + 2];
        const uint32_t n_row = (uint32_t)(m - i);
        const unsigned long long row_base = base;
        uint32_t dj = j_first, ia = a_first, ib = b_first, ic = c_first;
        while (true) {
            const bool valid = dj < n_row;
            if (__ballot(valid) == 0ull) break;          // dj ascends with the lane: lane 0 is the last to leave
            const int32_t j = valid ? i + (int32_t)dj : i;
            float w0 = fi0 - rows[3 * j], w1 = fi1 - rows[3 * j + 1], w2 = fi2 - rows[3 * j + 2];
            if (pbc.p[0]) w0 = w0 - ceilf(w0 - 0.5f);
            if (pbc.p[1]) w1 = w1 - ceilf(w1 - 0.5f);
            if (pbc.p[2]) w2 = w2 - ceilf(w2 - 0.5f);
            const int32_t sa = (int32_t)ia - R0, sb = (int32_t)ib - R1, sc = (int32_t)ic - R2;
            const float u0 = w0 + (float)sa, u1 = w1 + (float)sb, u2 = w2 + (float)sc;
            const float x0 = ((u0 * L[0][0]) + u1 * L[1][0]) + u2 * L[2][0];
            const float x1 = ((u0 * L[0][1]) + u1 * L[1][1]) + u2 * L[2][1];
            const float x2 = ((u0 * L[0][2]) + u1 * L[1][2]) + u2 * L[2][2];
            const float s = ((x0 * x0) + x1 * x1) + x2 * x2;
            const float r = sqrtf(s);        // correctly rounded (v_sqrt_f32 + two fma corrections); __fsqrt_rn compiles to the bare 1-ulp v_sqrt_f32
            const bool keep = valid && r > cutoff_min && r < cutoff_max;
            const unsigned long long mask = __ballot(keep);
            if (FILL && keep) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                const unsigned long long e = base + rank;
                if (e < out.total) {
                    if (out.pairs) {
                        out.pairs[2 * e] = v0 + i + 1;
                        out.pairs[2 * e + 1] = v0 + j + 1;
                    }
                    if (out.feature) out.feature[e] = r / cutoff_max;           // IEEE division (v_div_scale / v_div_fmas / v_div_fixup)
                    if (out.vec) {
                        out.vec[3 * e] = x0;
                        out.vec[3 * e + 1] = x1;
                        out.vec[3 * e + 2] = x2;
                    }
                    if (out.shift) {
                        out.shift[3 * e] = sa;
                        out.shift[3 * e + 1] = sb;
                        out.shift[3 * e + 2] = sc;
                    }
                }
            }
            base += (unsigned long long)__popcll(mask);
            // + 64 in mixed radix: every digit and its step are below the radix, so one subtraction settles a carry
            ic += c_step;
            uint32_t carry = ic >= S2 ? 1u : 0u;
            ic -= carry ? S2 : 0u;
            ib += b_step + carry;
            carry = ib >= S1 ? 1u : 0u;
            ib -= carry ? S1 : 0u;
            ia += a_step + carry;
            carry = ia >= S0 ? 1u : 0u;
            ia -= carry ? S0 : 0u;
            dj += j_step + carry;
        }
        if (FILL && out.first_count && lane == 0) out.first_count[v0 + i] = (int32_t)(base - row_base);
    }
    return base;
}

// one wave per work item (structure, i0, i1)
template <bool FILL>
__global__ __launch_bounds__(64 * kWaves) void pg_walk_kernel(int32_t n_items, const int32_t *__restrict__ items,
                                                              const int32_t *__restrict__ offsets, const float *__restrict__ frac,
                                                              const float *__restrict__ lat, const PgInfo *__restrict__ info, PgPbc pbc,
                                                              float cutoff_min, float cutoff_max,
                                                              unsigned long long *__restrict__ item_count,
                                                              const unsigned long long *__restrict__ item_offset, PgOut out)
{
    __shared__ float staged[kWaves][3 * kLdsAtoms];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * kWaves + wave;
    const bool active = w < n_items;
    int32_t s = 0, i0 = 0, i1 = 0, v0 = 0, m = 0;
    if (active) {
        s = items[3 * w];
        i0 = items[3 * w + 1];
        i1 = items[3 * w + 2];
        v0 = offsets[s];
        m = offsets[s + 1] - v0;
    }
    const float *rows = frac + 3 * (int64_t)v0;
    const bool in_lds = active && m <= kLdsAtoms;
    if (in_lds)
        for (int k = lane; k < 3 * m; k += 64) staged[wave][k] = rows[k];
    __syncthreads();
    if (!active) return;
    const PgInfo I = info[s];
    const unsigned long long base = FILL ? item_offset[w] : 0ull;
    unsigned long long end;
    if (in_lds)
        end = pg_walk_item<FILL>(staged[wave], m, i0, i1, v0, lat + 9 * (int64_t)s, I, pbc, cutoff_min, cutoff_max, base, out);
    else
        end = pg_walk_item<FILL>(rows, m, i0, i1, v0, lat + 9 * (int64_t)s, I, pbc, cutoff_min, cutoff_max, base, out);
    if (!FILL && lane == 0) item_count[w] = end;
}

} // namespace

namespace amp {

// Every device output null: the count pass only.  Everything on the library's stream; synchronised on return.
int periodic_pairs_core(int32_t B, int32_t n, const int32_t *offsets, const float *frac_dev, const float *lat_dev, const int32_t *pbc,
                        float cutoff_min, float cutoff_max, int32_t *pairs_dev, float *feature_dev, float *vec_dev, int32_t *shift_dev,
                        int32_t *first_count_dev, int64_t capacity, int64_t *n_pairs_out, int64_t *edge_offsets_out)
{
    AMP_REQUIRE(n_pairs_out != nullptr, "periodic_pairs: null n_pairs_out");
    *n_pairs_out = 0;
    AMP_REQUIRE(B >= 0 && n >= 0 && offsets != nullptr && pbc != nullptr, "periodic_pairs: bad arguments");
    AMP_REQUIRE(offsets[0] == 0, "periodic_pairs: offsets(1) = %d, not 0", offsets[0]);
    for (int32_t s = 0; s < B; ++s)
        AMP_REQUIRE(offsets[s + 1] >= offsets[s], "periodic_pairs: structure %d: offsets descend from %d to %d", s + 1, offsets[s],
                    offsets[s + 1]);
    AMP_REQUIRE(offsets[B] == n, "periodic_pairs: offsets end at %d, the batch has %d atoms", offsets[B], n);
    AMP_REQUIRE(isfinite(cutoff_min) && isfinite(cutoff_max), "periodic_pairs: cutoffs (%g, %g) are not finite", (double)cutoff_min,
                (double)cutoff_max);
    AMP_REQUIRE(cutoff_min >= 0.f && cutoff_max > cutoff_min, "periodic_pairs: cutoffs (%g, %g): need 0 <= cutoff_min < cutoff_max",
                (double)cutoff_min, (double)cutoff_max);
    AMP_REQUIRE((n == 0 || frac_dev != nullptr) && (B == 0 || lat_dev != nullptr), "periodic_pairs: null input array");
    if (edge_offsets_out) std::fill(edge_offsets_out, edge_offsets_out + B + 1, (int64_t)0);
    if (B == 0) return 0;
    hipStream_t st = stream();
    const bool fill_edges = pairs_dev || feature_dev || vec_dev || shift_dev;
    const bool fill = fill_edges || first_count_dev;
    const PgPbc P = {{pbc[0] != 0, pbc[1] != 0, pbc[2] != 0}};

    // work items, in order of (structure, first row); item_first[s] = the first item of structure s or of a later one
    std::vector<int32_t> items;
    std::vector<int64_t> item_first((size_t)B + 1);
    for (int32_t s = 0; s < B; ++s) {
        item_first[s] = (int64_t)(items.size() / 3);
        const int32_t m = offsets[s + 1] - offsets[s];
        for (int32_t i = 0; i < m;) {
            int64_t pairs = 0;
            int32_t i1 = i;
            do {
                pairs += m - i1;
                ++i1;
            } while (i1 < m && pairs + (m - i1) <= kItemPairs);
            items.insert(items.end(), {s, i, i1});
            i = i1;
        }
    }
    const int64_t W = (int64_t)(items.size() / 3);
    item_first[B] = W;
    AMP_REQUIRE(W < (int64_t)INT32_MAX, "periodic_pairs: %lld work items", (long long)W);

    Scratch tmp;
    int32_t *d_off = nullptr, *d_items = nullptr;
    PgInfo *d_info = nullptr;
    unsigned long long *d_partial = nullptr, *d_count = nullptr, *d_tile = nullptr, *d_offset = nullptr;
    const int check_blocks = (int)std::min<int64_t>(kCheckBlocks, ((int64_t)std::max(B, n) + 255) / 256);
    const uint32_t tiles = scan64::tiles(W);
    if (tmp.get(&d_off, (size_t)B + 1) || tmp.get(&d_items, items.size()) || tmp.get(&d_info, B) ||
        tmp.get(&d_partial, 2 * (size_t)check_blocks) || tmp.get(&d_count, W) || tmp.get(&d_tile, (size_t)tiles + 1) ||
        tmp.get(&d_offset, W))
        return 1;
    AMP_HIP(hipMemcpyAsync(d_off, offsets, sizeof(int32_t) * ((size_t)B + 1), hipMemcpyHostToDevice, st));
    if (W > 0) AMP_HIP(hipMemcpyAsync(d_items, items.data(), sizeof(int32_t) * items.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pg_prepare_kernel, dim3(check_blocks), dim3(256), 0, st, B, n, frac_dev, lat_dev, P, cutoff_max, d_info, d_partial);
    AMP_LAUNCH_CHECK();
    std::vector<unsigned long long> partial(2 * (size_t)check_blocks);
    AMP_HIP(hipMemcpyAsync(partial.data(), d_partial, sizeof(unsigned long long) * partial.size(), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    unsigned long long bad_s = ~0ull, bad_a = ~0ull;
    for (int b = 0; b < check_blocks; ++b) {
        bad_s = std::min(bad_s, partial[2 * b]);
        bad_a = std::min(bad_a, partial[2 * b + 1]);
    }
    // the structure of the first bad atom: the last one that starts at or before it (empty structures own no atom)
    const int64_t s_of_atom = bad_a == ~0ull ? INT64_MAX : (std::upper_bound(offsets, offsets + B + 1, (int32_t)bad_a) - offsets) - 1;
    if (bad_a != ~0ull && (bad_s == ~0ull || s_of_atom < (int64_t)bad_s)) {
        float p[3] = {0.f, 0.f, 0.f};
        AMP_HIP(hipMemcpy(p, frac_dev + 3 * bad_a, sizeof(p), hipMemcpyDeviceToHost));
        int k = 0;
        while (k < 2 && isfinite(p[k])) ++k;
        set_error("periodic_pairs: structure %lld: frac(%d,%llu) = %g is not finite", (long long)s_of_atom + 1, k + 1, bad_a + 1, (double)p[k]);
        return 2;
    }
    if (bad_s != ~0ull) {
        PgInfo I;
        float L[9];
        AMP_HIP(hipMemcpy(&I, d_info + bad_s, sizeof(I), hipMemcpyDeviceToHost));
        AMP_HIP(hipMemcpy(L, lat_dev + 9 * bad_s, sizeof(L), hipMemcpyDeviceToHost));
        if (I.status == 1) {
            int k = 0;
            while (k < 8 && isfinite(L[k])) ++k;
            set_error("periodic_pairs: structure %llu: lat(%d,%d) = %g is not finite", bad_s + 1, k / 3 + 1, k % 3 + 1, (double)L[k]);
        } else if (I.status == 2)
            set_error("periodic_pairs: structure %llu: det(lat) is zero or not finite: a periodic cell needs a volume", bad_s + 1);
        else {
            int a = 0;
            while (a < 2 && I.R[a] == 0) ++a;
            set_error("periodic_pairs: structure %llu: half-range %d on axis %d is above %d: the cell is too small for cutoff_max = %g",
                      bad_s + 1, I.R[a], a + 1, kMaxHalfRange, (double)cutoff_max);
        }
        return 2;
    }
    if (W == 0) {                                    // every structure is empty
        if (first_count_dev && n > 0) AMP_HIP(hipMemsetAsync(first_count_dev, 0, sizeof(int32_t) * (size_t)n, st));
        return 0;
    }

    const dim3 grid((unsigned)((W + kWaves - 1) / kWaves)), block(64 * kWaves);
    PgOut none = {nullptr, nullptr, nullptr, nullptr, nullptr, 0ull};
    hipLaunchKernelGGL(pg_walk_kernel<false>, grid, block, 0, st, (int32_t)W, (const int32_t *)d_items, (const int32_t *)d_off, frac_dev,
                       lat_dev, (const PgInfo *)d_info, P, cutoff_min, cutoff_max, d_count, (const unsigned long long *)nullptr, none);
    hipLaunchKernelGGL(scan64::tile_sum_kernel<unsigned long long>, dim3(tiles), dim3(256), 0, st, W, (const unsigned long long *)d_count,
                       d_tile);
    hipLaunchKernelGGL(scan64::scan_tiles_kernel, dim3(1), dim3(256), 0, st, tiles, d_tile);
    AMP_LAUNCH_CHECK();
    unsigned long long total = 0;
    AMP_HIP(hipMemcpyAsync(&total, d_tile + tiles, sizeof(total), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    // the limit of csr_from_edges_core, found by the count pass before anything of that size is allocated
    AMP_REQUIRE(total < (1ull << 31) && 2 * (int64_t)total + n < (int64_t)INT32_MAX,
                "periodic_pairs: %llu edges among %d atoms: more than 2^31 CSR entries", total, n);
    *n_pairs_out = (int64_t)total;
    if (fill_edges)
        AMP_REQUIRE(capacity >= (int64_t)total, "periodic_pairs: the output buffers hold %lld edges, the batch has %lld",
                    (long long)capacity, (long long)total);
    if (!fill && !edge_offsets_out) return 0;

    hipLaunchKernelGGL(scan64::apply_kernel<unsigned long long>, dim3(tiles), dim3(256), 0, st, W, (const unsigned long long *)d_count,
                       (const unsigned long long *)d_tile, d_offset);
    AMP_LAUNCH_CHECK();
    if (fill) {
        PgOut out = {pairs_dev, feature_dev, vec_dev, shift_dev, first_count_dev, total};
        hipLaunchKernelGGL(pg_walk_kernel<true>, grid, block, 0, st, (int32_t)W, (const int32_t *)d_items, (const int32_t *)d_off, frac_dev,
                           lat_dev, (const PgInfo *)d_info, P, cutoff_min, cutoff_max, (unsigned long long *)nullptr,
                           (const unsigned long long *)d_offset, out);
        AMP_LAUNCH_CHECK();
    }
    if (edge_offsets_out) {
        std::vector<unsigned long long> off((size_t)W);
        AMP_HIP(hipMemcpyAsync(off.data(), d_offset, sizeof(unsigned long long) * (size_t)W, hipMemcpyDeviceToHost, st));
        AMP_HIP(hipStreamSynchronize(st));
        for (int32_t s = 0; s <= B; ++s) edge_offsets_out[s] = item_first[s] < W ? (int64_t)off[item_first[s]] : (int64_t)total;
    }
    AMP_HIP(hipStreamSynchronize(st));   // scratch dies with this scope
    return 0;
}

} // namespace amp

extern "C" int athena_mp_periodic_pairs(int32_t n_structures, int32_t n_atoms, const int32_t *offsets_host, const float *frac_dev,
                                        const float *lat_dev, const int32_t *pbc, float cutoff_min, float cutoff_max,
                                        int32_t *pairs_dev, float *feature_dev, float *vec_dev, int32_t *shift_dev,
                                        int32_t *first_count_dev, int64_t capacity, int64_t *n_pairs_out, int64_t *edge_offsets_out)
{
    return amp::periodic_pairs_core(n_structures, n_atoms, offsets_host, frac_dev, lat_dev, pbc, cutoff_min, cutoff_max, pairs_dev,
                                    feature_dev, vec_dev, shift_dev, first_count_dev, capacity, n_pairs_out, edge_offsets_out);
}

extern "C" int athena_mp_periodic_graph_host(int32_t n_structures, int32_t n_atoms, const int32_t *offsets_host, const float *frac_host,
                                             const float *lat_host, const int32_t *pbc, float cutoff_min, float cutoff_max,
                                             int32_t add_self_loops, int32_t *adj_ia_out, int32_t *adj_ja_out, int64_t capacity,
                                             int64_t *nnz_out, float *feature_out, float *vec_out, int32_t *first_count_out,
                                             int64_t edge_capacity, int64_t *n_pairs_out, int64_t *edge_offsets_out)
{
    using amp::Scratch;
    AMP_REQUIRE(nnz_out != nullptr && n_pairs_out != nullptr, "periodic_graph_host: null output pointer");
    *nnz_out = *n_pairs_out = 0;
    const int32_t B = n_structures, n = n_atoms;
    AMP_REQUIRE(B >= 0 && n >= 0 && (n == 0 || frac_host != nullptr) && (B == 0 || lat_host != nullptr),
                "periodic_graph_host: bad arguments (n_structures = %d, n_atoms = %d)", B, n);
    hipStream_t st = amp::stream();
    const bool query = adj_ja_out == nullptr;
    Scratch tmp;
    float *d_frac = nullptr, *d_lat = nullptr, *d_feature = nullptr, *d_vec = nullptr;
    int32_t *d_pairs = nullptr, *d_first = nullptr;
    if (tmp.get(&d_frac, 3 * (size_t)n) || tmp.get(&d_lat, 9 * (size_t)B)) return 1;
    if (n > 0) AMP_HIP(hipMemcpyAsync(d_frac, frac_host, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, st));
    if (B > 0) AMP_HIP(hipMemcpyAsync(d_lat, lat_host, sizeof(float) * 9 * (size_t)B, hipMemcpyHostToDevice, st));
    int64_t E = 0;
    if (int rc = amp::periodic_pairs_core(B, n, offsets_host, d_frac, d_lat, pbc, cutoff_min, cutoff_max, nullptr, nullptr, nullptr, nullptr,
                                          nullptr, 0, &E, nullptr))
        return rc;
    *n_pairs_out = E;
    if (!query) {
        AMP_REQUIRE(adj_ia_out != nullptr, "periodic_graph_host: null adj_ia");
        AMP_REQUIRE(edge_capacity >= E, "periodic_graph_host: the edge buffers hold %lld edges, the batch has %lld", (long long)edge_capacity,
                    (long long)E);
    }
    if (tmp.get(&d_pairs, 2 * (size_t)E)) return 1;
    if (!query && feature_out && tmp.get(&d_feature, (size_t)E)) return 1;
    if (!query && vec_out && tmp.get(&d_vec, 3 * (size_t)E)) return 1;
    if (!query && first_count_out && tmp.get(&d_first, (size_t)n)) return 1;
    if (int rc = amp::periodic_pairs_core(B, n, offsets_host, d_frac, d_lat, pbc, cutoff_min, cutoff_max, d_pairs, d_feature, d_vec, nullptr,
                                          d_first, E, &E, edge_offsets_out))
        return rc;
    // a self-image edge is ONE CSR entry and several edges may join one pair: the entry count comes from the builder
    std::vector<int32_t> ia_query;
    int32_t *ia = adj_ia_out;
    if (ia == nullptr) {
        ia_query.resize((size_t)n + 1);
        ia = ia_query.data();
    }
    int64_t nnz = 0;
    if (int rc = amp::csr_from_edges_core(n, E, d_pairs, add_self_loops, ia, adj_ja_out, capacity, &nnz, nullptr, true)) return rc;
    *nnz_out = nnz;
    if (query) return 0;
    if (d_feature && E > 0) AMP_HIP(hipMemcpyAsync(feature_out, d_feature, sizeof(float) * (size_t)E, hipMemcpyDeviceToHost, st));
    if (d_vec && E > 0) AMP_HIP(hipMemcpyAsync(vec_out, d_vec, sizeof(float) * 3 * (size_t)E, hipMemcpyDeviceToHost, st));
    if (d_first && n > 0) AMP_HIP(hipMemcpyAsync(first_count_out, d_first, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    return 0;
}
