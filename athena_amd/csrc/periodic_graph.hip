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
// How, the WALK route: structures are tiny (8 - 30 atoms) and there are very many, so there is no grid and the enumeration order
// IS the output order.  The host cuts structures into work items (structure, rows i0 .. i1-1) of at most kItemPairs pairs (a
// structure of up to 31 atoms is one item; a row is never cut).  One 64-lane wave owns an item: for each row i it walks the
// candidates (j - i, a, b, c) in linear order, 64 per step -- each lane keeps its candidate as a mixed-radix counter and adds the
// digits of 64, no division in the loop -- decides the predicate, takes a ballot and ranks the kept lanes with mbcnt on a running
// base.  COUNT pass: per-item totals; exclusive 64-bit scan over the items (scan64.h); FILL pass: the same walk writes every
// output at its final position, and first_count per row.  No sort of edges, no atomics: two builds are byte-identical.  The
// structure's fractional rows sit in LDS when it has at most kLdsAtoms atoms; a larger one is read from global memory.
//
// The GRID route, chosen per structure (supercells, slabs, MD snapshots: the walk costs m^2 / 2 pairs), prunes the PAIRS and then
// decides the same predicate, by the same lines of pg_walk_item, on the pairs that are left; the outputs are those of the walk,
// byte for byte.  Its atoms are numbered 0 .. NG-1 over the grid structures of the call ("grid atoms").  Cell ids per atom;
// a stable radix sort of (cell, grid atom) (radix_sort.h) and the cell starts; per atom i the partners j >= i in the cells around
// its own, counted by one binary search per cell (a cell's atoms ascend); a scan of the counts in atom order (scan64.h); a fill
// of keys i * NG + j; one more radix sort, after which row i holds its partners in ascending order.  The host reads the row
// starts, refuses a list it cannot hold, and cuts the rows into work items as above (at most kItemPairs candidate pairs, a row is
// never cut).  Items of both routes stand in ONE array in structure order: one scan gives every edge rank and edge_offsets, and
// runs of items of one route are one launch each.  In a grid item the lane counter runs over (position in the row's partner
// list, a, b, c) and j is read from the list; nothing else differs, first_count is the row's rank difference as in the walk.
//
// The pruning rule and why it loses nothing.  On a periodic axis a of a structure, with h_a in fp64 as above,
//   nc_a = clamp(floor(1 / (h_a * (1 + kGridMargin))), 1, kGridCellsAxis), lowered further (never raised) until the structure has
//          at most 2 m cells, and set to 1 when it is below 3;  an open axis has nc_a = 1;
//   t = frac - floor(frac) in fp32 (exactly 1.0 for a tiny negative frac),  cell = min(nc_a - 1, floor(fl(t * nc_a))).
// An atom is paired with the atoms of the cells -1, 0, +1 (circular) on every axis with nc_a >= 3 and with all atoms along an axis
// of one cell (three distinct cells, or the single one: no cell is visited twice).
// Claim: when (i, j, shift) is kept, the cells of i and j are equal or circularly adjacent on every axis with nc_a >= 3, provided
//   (P1) |frac| <= kGridFracMax = 64 for every coordinate of the structure, and
//   (P2) sum_k U_k |L_k| <= kGridLatticeSum * cutoff_max = 4096 cutoff_max, U_k = searched half-range + 1 on a periodic axis and
//        2 kGridFracMax + 1 on an open one (a bound of |u_k| below),
// which pg_prepare_kernel checks; a structure that fails either, or has no periodic axis (no det L, no h), takes the walk.
// Proof, eps = 2^-24, F the fp32 coordinates as real numbers, D = F_i[a] - F_j[a]:
//   the predicate's u_a = fl(w_a + shift_a) is D - n + e1 with n an integer and |e1| <= 2 eps kGridFracMax (rounding of f) + eps
//   (of w, |w| <= 1/2) + 2 eps (of u: nc_a >= 3 means h_a < 1/3, the searched half-range is 1, |u_a| < 2);
//   the computed x differs from the exact u . L by a vector of length at most g3 sum_k |u_k| |L_k|, g3 = 3 eps / (1 - 3 eps) (three
//   roundings per term), and |x computed| < cutoff_max (1 + 3 eps) when the rounded r is below cutoff_max (three roundings in s, one
//   in the square root); u_a = (u . L) . g_a exactly and |g_a| = h_a / cutoff_max, so with (P2)
//   |u_a| < h_a (1 + 3 eps) + g3 * 4096 * h_a < h_a (1 + 2^-9 * 0.376), and dist(D, Z) <= |u_a| + |e1|;
//   the cell coordinate q = fl(t * nc_a) is nc_a (F - floor F) + e2, |e2| <= 1.5 eps nc_a (t is rounded by at most eps / 2, the
//   product by eps nc_a), so q_i - q_j is within 3 eps nc_a of nc_a (D - integer): circularly (mod nc_a) the two coordinates are
//   less than nc_a (dist(D, Z) + 3 eps) apart;
//   1 / nc_a >= h_a (1 + kGridMargin), so the slack 1 / nc_a - h_a is at least kGridMargin h_a AND at least
//   kGridMargin / ((1 + kGridMargin) kGridCellsAxis) > 2^-15 * 0.99, hence at least half of each;  the relative errors take
//   2^-9 * 0.376 h_a < kGridMargin h_a / 2 (the rest covers the fp64 evaluation of h_a), the absolute ones
//   eps (2 * 64 + 1 + 2 + 3 + 1) = 135 * 2^-24 < 2^-16 * 0.99: the coordinates are circularly LESS than one apart.
//   Two numbers of [0, nc_a] less than one apart (mod nc_a) have floors, the upper end clamped to nc_a - 1, that are equal or
//   circularly adjacent: if they are less than one apart as they stand the floors differ by at most one; otherwise one is above
//   nc_a - 1 (cell nc_a - 1) and the other below 1 (cell 0).  Lowering nc_a only widens the slack.
// tests/periodic_grid_reference.py transcribes the rule; tests/test_periodic_grid.py holds it against the yardstick.
// Route choice: automatic mode sends a structure through the grid when it has more than kGridAtoms atoms and nc_a >= 4 on some
// axis (fewer cells prune nothing worth the sorts); ATHENA_MP_PERIODIC_ROUTE = auto | walk | grid pins it for every non-empty
// structure (tests, read at every call; under `grid` a tiny cell has nc = 1 everywhere and lists all pairs).  The preconditions
// send a structure down the walk in either mode.  athena_mp_periodic_stats reports what the last call did.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "cell_start.h"
#include "common.h"
#include "radix_sort.h"
#include "scan64.h"

namespace {

constexpr int kMaxHalfRange = 31;    // floor(h_a + 1/2) above this is refused; the search adds the margin of one
constexpr int kItemPairs = 512;      // pairs (i, j) per work item, unless one row alone has more
constexpr int kLdsAtoms = 128;       // structures with more atoms than this are read from global memory
constexpr int kWaves = 4;            // work items per 256-thread block
constexpr int kCheckBlocks = 256;
// the grid route (the header proves the four numbers below against each other)
constexpr int kGridAtoms = 128;                  // automatic mode: more atoms than this (and nc >= 4 on some axis) take the grid.
                                                 // Where the walk leaves LDS; not measured yet
constexpr int kGridCellsAxis = 128;
constexpr double kGridMargin = 1.0 / 256.0;
constexpr float kGridFracMax = 64.f;             // (P1)
constexpr double kGridLatticeSum = 4096.0;       // (P2)

struct PgInfo {
    int32_t R[3];      // searched half-range per axis (0 on an open axis); for status 3 the offending floor(h + 1/2) is in R[axis]
    int32_t status;    // 0 good, 1 non-finite lattice entry, 2 det L zero or not finite, 3 half-range above kMaxHalfRange
};

struct PgPbc {
    int32_t p[3];
};

struct PgGrid {        // per structure, from its lattice alone
    int32_t nc[3];     // cells per axis: 1, or 3 .. kGridCellsAxis
    int32_t ok;        // a periodic axis, a usable det L and (P2)
};

struct PgGridS {       // per GRID structure, in structure order; entry G is the end: a0 = NG, c0 = all cells
    int32_t s;         // the structure
    int32_t a0;        // its first grid atom
    int32_t c0;        // its first cell
    int32_t nc[3];
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
// With `grid` also: ginfo[t] for structure t, and far[s] = 1 (every writer stores the same word) for the structure s of an atom
// that breaks (P1); far arrives zeroed.
__global__ __launch_bounds__(256) void pg_prepare_kernel(int32_t B, int32_t n, const float *__restrict__ frac, const float *__restrict__ lat,
                                                         PgPbc pbc, float cutoff_max, PgInfo *__restrict__ info,
                                                         unsigned long long *__restrict__ partial, int32_t grid,
                                                         const int32_t *__restrict__ offsets, PgGrid *__restrict__ ginfo,
                                                         int32_t *__restrict__ far)
{
    unsigned long long bad_s = ~0ull, bad_a = ~0ull;
    const int64_t top = B > n ? B : n;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < top; t += (int64_t)gridDim.x * 256) {
        if (t < n) {
            const bool ok = isfinite(frac[3 * t]) && isfinite(frac[3 * t + 1]) && isfinite(frac[3 * t + 2]);
            if (!ok && (unsigned long long)t < bad_a) bad_a = (unsigned long long)t;
            if (grid && ok && !(fabsf(frac[3 * t]) <= kGridFracMax && fabsf(frac[3 * t + 1]) <= kGridFracMax && fabsf(frac[3 * t + 2]) <= kGridFracMax)) {
                int32_t lo = 0, hi = B;                  // the last structure that starts at or before atom t
                while (hi - lo > 1) {
                    const int32_t mid = lo + ((hi - lo) >> 1);
                    if ((int64_t)offsets[mid] <= t) lo = mid; else hi = mid;
                }
                far[lo] = 1;
            }
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
            double hax[3] = {0.0, 0.0, 0.0};          // h_a of the periodic axes
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
                        hax[a] = h;
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
            if (grid) {
                PgGrid Gd = {{1, 1, 1}, 0};
                if (I.status == 0 && (pbc.p[0] || pbc.p[1] || pbc.p[2])) {
                    double sum = 0.0;
                    for (int a = 0; a < 3; ++a) {
                        const double len = sqrt(L[a][0] * L[a][0] + L[a][1] * L[a][1] + L[a][2] * L[a][2]);
                        sum += (pbc.p[a] ? (double)(I.R[a] + 1) : 2.0 * (double)kGridFracMax + 1.0) * len;
                        if (pbc.p[a]) {
                            const double c = floor(1.0 / (hax[a] * (1.0 + kGridMargin)));
                            Gd.nc[a] = c >= (double)kGridCellsAxis ? kGridCellsAxis : c >= 3.0 ? (int32_t)c : 1;
                        }
                    }
                    Gd.ok = sum <= kGridLatticeSum * (double)cutoff_max ? 1 : 0;
                    const int64_t m2 = 2 * (int64_t)(offsets[t + 1] - offsets[t]);
                    const int64_t cap = m2 > 1 ? m2 : 1;
                    while ((int64_t)Gd.nc[0] * Gd.nc[1] * Gd.nc[2] > cap) {
                        int a = 0;
                        for (int k = 1; k < 3; ++k)
                            if (Gd.nc[k] > Gd.nc[a]) a = k;
                        Gd.nc[a] = (Gd.nc[a] + 1) / 2;
                        if (Gd.nc[a] < 3) Gd.nc[a] = 1;
                    }
                }
                ginfo[t] = Gd;
            }
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

struct PgCand {                          // the partner lists of the grid route
    const unsigned long long *key;       // sorted keys i * NG + j over grid atoms: row i = key[poff[i] .. poff[i + 1])
    const unsigned long long *poff;      // [NG + 1]
    unsigned long long NG;
    int32_t a0;                          // the structure's first grid atom
};

// The rows i0 .. i1-1 of one structure, walked by one wave.  rows: the structure's fractional coordinates (LDS or global).
// GRID: the partners of row i are those of its list, not i .. m-1.  Returns the number of edges found; FILL writes them from
// rank `base` on.
template <bool FILL, bool GRID = false>
__device__ __forceinline__ unsigned long long pg_walk_item(const float *rows, int32_t m, int32_t i0, int32_t i1, int32_t v0,
                                                           const float *__restrict__ lat, const PgInfo &I, PgPbc pbc, float cutoff_min,
                                                           float cutoff_max, unsigned long long base, const PgOut &out,
                                                           const PgCand &cd = PgCand())
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
        uint32_t n_row = (uint32_t)(m - i);
        const unsigned long long *list = nullptr;
        unsigned long long key0 = 0ull;              // key - key0 = local j
        if (GRID) {
            const unsigned long long gi = (unsigned long long)(cd.a0 + i), p0 = cd.poff[gi];
            n_row = (uint32_t)(cd.poff[gi + 1] - p0);
            list = cd.key + p0;
            key0 = gi * cd.NG + (unsigned long long)cd.a0;
        }
        const unsigned long long row_base = base;
        uint32_t dj = j_first, ia = a_first, ib = b_first, ic = c_first;
        while (true) {
            const bool valid = dj < n_row;
            if (__ballot(valid) == 0ull) break;          // dj ascends with the lane: lane 0 is the last to leave
            int32_t j = valid ? i + (int32_t)dj : i;
            if (GRID && valid) j = (int32_t)(list[dj] - key0);
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

// ---- the grid route ----------------------------------------------------------------------------------------------------------
// the grid structure of grid atom ga: the last g with gs[g].a0 <= ga (a0 ascends strictly: grid structures are not empty)
__device__ inline int32_t pg_grid_of_atom(const PgGridS *__restrict__ gs, int32_t G, int32_t ga)
{
    int32_t lo = 0, hi = G;
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (gs[mid].a0 <= ga) lo = mid; else hi = mid;
    }
    return lo;
}

// key[ga] = the cell of grid atom ga, numbered over the grid structures of the call
__global__ __launch_bounds__(256) void pg_cell_key_kernel(int32_t NG, const PgGridS *__restrict__ gs, int32_t G,
                                                          const int32_t *__restrict__ offsets, const float *__restrict__ frac,
                                                          uint32_t *__restrict__ key)
{
    const int64_t ga = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ga >= NG) return;
    const PgGridS S = gs[pg_grid_of_atom(gs, G, (int32_t)ga)];
    const int64_t atom = (int64_t)offsets[S.s] + (ga - S.a0);
    uint32_t c = 0;
    for (int k = 2; k >= 0; --k) {
        int32_t ck = 0;
        if (S.nc[k] > 1) {
            const float f = frac[3 * atom + k];
            const float t = f - floorf(f);                    // [0, 1], both ends included
            const float q = t * (float)S.nc[k];
            ck = (int32_t)q;                                  // q >= 0: truncation is floor
            ck = ck < S.nc[k] - 1 ? ck : S.nc[k] - 1;
        }
        c = c * (uint32_t)S.nc[k] + (uint32_t)ck;
    }
    key[ga] = (uint32_t)S.c0 + c;
}

// One thread per grid atom i: its partners j >= i in the cells -1, 0, +1 (circular) of every axis with more than one cell.  perm
// lists the grid atoms in cell order, ascending inside a cell.  FILL = false: count[i] (and count[NG] = 0, the scan's end).
// FILL = true: key[poff[i] + t] = i * NG + j for the t-th partner met.
template <bool FILL>
__global__ __launch_bounds__(256) void pg_partner_kernel(int32_t NG, const PgGridS *__restrict__ gs, int32_t G,
                                                         const uint32_t *__restrict__ cell_key, const int32_t *__restrict__ perm,
                                                         const int32_t *__restrict__ cell_start, uint32_t *__restrict__ count,
                                                         const unsigned long long *__restrict__ poff,
                                                         unsigned long long *__restrict__ key)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > NG) return;
    if (i == NG) {
        if (!FILL) count[NG] = 0u;
        return;
    }
    const PgGridS S = gs[pg_grid_of_atom(gs, G, (int32_t)i)];
    uint32_t lc = cell_key[i] - (uint32_t)S.c0;
    const int32_t c0 = (int32_t)(lc % (uint32_t)S.nc[0]);
    lc /= (uint32_t)S.nc[0];
    const int32_t c1 = (int32_t)(lc % (uint32_t)S.nc[1]), c2 = (int32_t)(lc / (uint32_t)S.nc[1]);
    const int r0 = S.nc[0] > 1 ? 1 : 0, r1 = S.nc[1] > 1 ? 1 : 0, r2 = S.nc[2] > 1 ? 1 : 0;      // nc is 1 or at least 3
    uint32_t found = 0;
    unsigned long long at = 0;
    if (FILL) at = poff[i];
    for (int dz = -r2; dz <= r2; ++dz) {
        int32_t z = c2 + dz;
        z = z < 0 ? z + S.nc[2] : z >= S.nc[2] ? z - S.nc[2] : z;
        for (int dy = -r1; dy <= r1; ++dy) {
            int32_t y = c1 + dy;
            y = y < 0 ? y + S.nc[1] : y >= S.nc[1] ? y - S.nc[1] : y;
            for (int dx = -r0; dx <= r0; ++dx) {
                int32_t x = c0 + dx;
                x = x < 0 ? x + S.nc[0] : x >= S.nc[0] ? x - S.nc[0] : x;
                const uint32_t cell = (uint32_t)S.c0 + ((uint32_t)z * (uint32_t)S.nc[1] + (uint32_t)y) * (uint32_t)S.nc[0] + (uint32_t)x;
                const int32_t end = cell_start[cell + 1];
                int32_t lo = cell_start[cell], hi = end;             // the first slot of the cell whose atom is >= i
                while (lo < hi) {
                    const int32_t mid = lo + ((hi - lo) >> 1);
                    if ((int64_t)perm[mid] < i) lo = mid + 1; else hi = mid;
                }
                if (FILL)
                    for (int32_t k = lo; k < end; ++k)
                        key[at + found + (uint32_t)(k - lo)] = (unsigned long long)i * (unsigned long long)NG + (unsigned long long)perm[k];
                found += (uint32_t)(end - lo);
            }
        }
    }
    if (!FILL) count[i] = found;
}

// one wave per work item (structure, i0, i1) of a grid structure: pg_walk_item over the partner lists, rows from global memory
template <bool FILL>
__global__ __launch_bounds__(64 * kWaves) void pg_grid_walk_kernel(int32_t n_items, const int32_t *__restrict__ items,
                                                                   const int32_t *__restrict__ offsets, const PgGridS *__restrict__ gs,
                                                                   int32_t G, PgCand cd, const float *__restrict__ frac,
                                                                   const float *__restrict__ lat, const PgInfo *__restrict__ info,
                                                                   PgPbc pbc, float cutoff_min, float cutoff_max,
                                                                   unsigned long long *__restrict__ item_count,
                                                                   const unsigned long long *__restrict__ item_offset, PgOut out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * kWaves + wave;
    if (w >= n_items) return;
    const int32_t s = items[3 * w], i0 = items[3 * w + 1], i1 = items[3 * w + 2];
    const int32_t v0 = offsets[s], m = offsets[s + 1] - v0;
    int32_t lo = 0, hi = G;                                // the grid structure that is structure s (s ascends with g)
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (gs[mid].s <= s) lo = mid; else hi = mid;
    }
    cd.a0 = gs[lo].a0;
    const PgInfo I = info[s];
    const unsigned long long base = FILL ? item_offset[w] : 0ull;
    const unsigned long long end = pg_walk_item<FILL, true>(frac + 3 * (int64_t)v0, m, i0, i1, v0, lat + 9 * (int64_t)s, I, pbc, cutoff_min,
                                                            cutoff_max, base, out, cd);
    if (!FILL && lane == 0) item_count[w] = end;
}

} // namespace

namespace amp {

// what the most recent call did (athena_mp_periodic_stats): structures walked, through the grid, pairs of the walk, candidate
// pairs of the grid, structures that met the grid's conditions of size but not (P1) / (P2)
static int64_t g_periodic_stats[5];

// Every device output null: the count pass only.  Everything on the library's stream; synchronised on return.
int periodic_pairs_core(int32_t B, int32_t n, const int32_t *offsets, const float *frac_dev, const float *lat_dev, const int32_t *pbc,
                        float cutoff_min, float cutoff_max, int32_t *pairs_dev, float *feature_dev, float *vec_dev, int32_t *shift_dev,
                        int32_t *first_count_dev, int64_t capacity, int64_t *n_pairs_out, int64_t *edge_offsets_out)
{
    AMP_REQUIRE(n_pairs_out != nullptr, "periodic_pairs: null n_pairs_out");
    *n_pairs_out = 0;
    std::fill(g_periodic_stats, g_periodic_stats + 5, (int64_t)0);
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

    int mode = 0;                                     // 0 auto, 1 walk, 2 grid: ATHENA_MP_PERIODIC_ROUTE, read at every call (tests)
    if (const char *env = getenv("ATHENA_MP_PERIODIC_ROUTE")) {
        mode = strcmp(env, "auto") == 0 ? 0 : strcmp(env, "walk") == 0 ? 1 : strcmp(env, "grid") == 0 ? 2 : -1;
        AMP_REQUIRE(mode >= 0, "periodic_pairs: ATHENA_MP_PERIODIC_ROUTE = '%s' is none of auto, walk, grid", env);
    }
    int32_t m_max = 0;
    for (int32_t s = 0; s < B; ++s) m_max = std::max(m_max, offsets[s + 1] - offsets[s]);
    const bool maybe_grid = mode == 2 ? m_max > 0 : mode == 0 && m_max > kGridAtoms;

    Scratch tmp;
    int32_t *d_off = nullptr, *d_far = nullptr;
    PgInfo *d_info = nullptr;
    PgGrid *d_ginfo = nullptr;
    unsigned long long *d_partial = nullptr;
    const int check_blocks = (int)std::min<int64_t>(kCheckBlocks, ((int64_t)std::max(B, n) + 255) / 256);
    if (tmp.get(&d_off, (size_t)B + 1) || tmp.get(&d_info, B) || tmp.get(&d_partial, 2 * (size_t)check_blocks)) return 1;
    if (maybe_grid) {
        if (tmp.get(&d_ginfo, B) || tmp.get(&d_far, B)) return 1;
        AMP_HIP(hipMemsetAsync(d_far, 0, sizeof(int32_t) * (size_t)B, st));
    }
    AMP_HIP(hipMemcpyAsync(d_off, offsets, sizeof(int32_t) * ((size_t)B + 1), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pg_prepare_kernel, dim3(check_blocks), dim3(256), 0, st, B, n, frac_dev, lat_dev, P, cutoff_max, d_info, d_partial,
                       (int32_t)maybe_grid, (const int32_t *)d_off, d_ginfo, d_far);
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

    // the route of every structure; the grid structures in structure order, gs[G] the end
    std::vector<PgGridS> gs;
    int64_t NG = 0, NC = 0;
    if (maybe_grid) {
        std::vector<PgGrid> ginfo((size_t)B);
        std::vector<int32_t> far((size_t)B);
        AMP_HIP(hipMemcpyAsync(ginfo.data(), d_ginfo, sizeof(PgGrid) * (size_t)B, hipMemcpyDeviceToHost, st));
        AMP_HIP(hipMemcpyAsync(far.data(), d_far, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, st));
        AMP_HIP(hipStreamSynchronize(st));
        for (int32_t s = 0; s < B; ++s) {
            const int32_t m = offsets[s + 1] - offsets[s];
            const PgGrid &g = ginfo[s];
            if (m == 0 || !(mode == 2 || (m > kGridAtoms && std::max(g.nc[0], std::max(g.nc[1], g.nc[2])) >= 4))) continue;
            if (!g.ok || far[s]) {                   // (P1), (P2), or no periodic axis: the walk
                ++g_periodic_stats[4];
                continue;
            }
            gs.push_back({s, (int32_t)NG, (int32_t)NC, {g.nc[0], g.nc[1], g.nc[2]}});
            NG += m;
            NC += (int64_t)g.nc[0] * g.nc[1] * g.nc[2];
        }
        AMP_REQUIRE(NC < (int64_t)INT32_MAX - 1, "periodic_pairs: %lld grid cells", (long long)NC);
    }
    const int32_t G = (int32_t)gs.size();
    gs.push_back({B, (int32_t)NG, (int32_t)NC, {1, 1, 1}});

    // the grid structures' partner lists: row ga of the sorted keys is d_key[poff[ga] .. poff[ga + 1])
    PgGridS *d_gs = nullptr;
    unsigned long long *d_poff = nullptr, *d_key = nullptr;
    std::vector<unsigned long long> poff;
    if (G > 0) {
        uint32_t *d_ck = nullptr, *d_ck_s = nullptr, *d_ck_t = nullptr, *d_cnt = nullptr;
        int32_t *d_perm = nullptr, *d_perm_t = nullptr, *d_cell_start = nullptr;
        unsigned long long *d_ptile = nullptr;
        char *d_temp = nullptr;
        const size_t NGz = (size_t)NG;
        Pieces pc;
        pc.add(&d_gs, (size_t)G + 1), pc.add(&d_ck, NGz), pc.add(&d_ck_s, NGz), pc.add(&d_ck_t, NGz), pc.add(&d_perm, NGz), pc.add(&d_perm_t, NGz);
        pc.add(&d_cell_start, (size_t)NC + 1), pc.add(&d_cnt, NGz + 1), pc.add(&d_ptile, (size_t)scan64::tiles(NG + 1) + 1);
        pc.add(&d_poff, NGz + 1);
        pc.add(&d_temp, radix::scratch_bytes(NG));
        if (tmp.carve(pc)) return 1;
        AMP_HIP(hipMemcpyAsync(d_gs, gs.data(), sizeof(PgGridS) * ((size_t)G + 1), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(pg_cell_key_kernel, dim3(blocks(NG)), dim3(256), 0, st, (int32_t)NG, (const PgGridS *)d_gs, G,
                           (const int32_t *)d_off, frac_dev, d_ck);
        AMP_LAUNCH_CHECK();
        if (int rc = radix::sort_pairs<uint32_t>((const uint32_t *)d_ck, nullptr, NG, bits_for((unsigned long long)NC - 1ull), d_ck_s, d_perm,
                                                 d_ck_t, d_perm_t, d_temp, st))
            return rc;
        hipLaunchKernelGGL(rg_cell_start_kernel, dim3(blocks(NC + 1)), dim3(256), 0, st, (uint32_t)NC, (const uint32_t *)d_ck_s, (int32_t)NG,
                           d_cell_start);
        hipLaunchKernelGGL(pg_partner_kernel<false>, dim3(blocks(NG + 1)), dim3(256), 0, st, (int32_t)NG, (const PgGridS *)d_gs, G,
                           (const uint32_t *)d_ck, (const int32_t *)d_perm, (const int32_t *)d_cell_start, d_cnt,
                           (const unsigned long long *)nullptr, (unsigned long long *)nullptr);
        (void)scan64::exclusive(NG + 1, (const uint32_t *)d_cnt, d_ptile, d_poff, st);
        AMP_LAUNCH_CHECK();
        poff.resize((size_t)NG + 1);
        AMP_HIP(hipMemcpyAsync(poff.data(), d_poff, sizeof(unsigned long long) * poff.size(), hipMemcpyDeviceToHost, st));
        AMP_HIP(hipStreamSynchronize(st));
        // the list's size is known before anything of that size exists: three key arrays and two index arrays of the sort (32 bytes a
        // pair, 40 with its histograms and some room), and the sort's int32 indices
        size_t free_b = 0, total_b = 0;
        AMP_HIP(hipMemGetInfo(&free_b, &total_b));
        const unsigned long long limit = std::min<unsigned long long>((unsigned long long)INT32_MAX, (unsigned long long)free_b / 40ull);
        for (int32_t g = 0; g < G; ++g)
            AMP_REQUIRE(poff[gs[g + 1].a0] <= limit,
                        "periodic_pairs: structure %d: the cell grid's candidate list reaches %llu atom pairs with this structure, "
                        "%llu can be held", gs[g].s + 1, poff[gs[g + 1].a0], limit);
        const int64_t NP = (int64_t)poff[NG];
        unsigned long long *d_pk = nullptr, *d_pk_t = nullptr;
        int32_t *d_v = nullptr, *d_v_t = nullptr;
        char *d_temp2 = nullptr;
        const size_t NPz = (size_t)NP;
        Pieces pk;
        pk.add(&d_pk, NPz), pk.add(&d_key, NPz), pk.add(&d_pk_t, NPz), pk.add(&d_v, NPz), pk.add(&d_v_t, NPz);
        pk.add(&d_temp2, radix::scratch_bytes(NP));
        if (tmp.carve(pk)) return 1;
        hipLaunchKernelGGL(pg_partner_kernel<true>, dim3(blocks(NG + 1)), dim3(256), 0, st, (int32_t)NG, (const PgGridS *)d_gs, G,
                           (const uint32_t *)d_ck, (const int32_t *)d_perm, (const int32_t *)d_cell_start, (uint32_t *)nullptr,
                           (const unsigned long long *)d_poff, d_pk);
        AMP_LAUNCH_CHECK();
        // rows are already in order of i; the sort of the whole key orders the partners inside every row
        if (int rc = radix::sort_pairs<unsigned long long>((const unsigned long long *)d_pk, nullptr, NP,
                                                           bits_for((unsigned long long)NG * (unsigned long long)NG - 1ull), d_key, d_v,
                                                           d_pk_t, d_v_t, d_temp2, st))
            return rc;
        g_periodic_stats[3] = NP;
    }

    // work items, in order of (structure, first row); item_first[s] = the first item of structure s or of a later one; runs of
    // items of one route (run_route, from item run_first[k] to run_first[k + 1])
    std::vector<int32_t> items;
    std::vector<int64_t> item_first((size_t)B + 1), run_first;
    std::vector<uint8_t> run_route;
    for (int32_t s = 0, g = 0; s < B; ++s) {
        item_first[s] = (int64_t)(items.size() / 3);
        const int32_t m = offsets[s + 1] - offsets[s];
        if (m == 0) continue;
        const bool grid = g < G && gs[g].s == s;
        if (run_route.empty() || run_route.back() != (uint8_t)grid) {
            run_route.push_back((uint8_t)grid);
            run_first.push_back(item_first[s]);
        }
        const unsigned long long *row = grid ? poff.data() + gs[g].a0 : nullptr;       // row[i + 1] - row[i] = partners of row i
        auto row_pairs = [&](int32_t i) -> int64_t { return grid ? (int64_t)(row[i + 1] - row[i]) : (int64_t)(m - i); };
        for (int32_t i = 0; i < m;) {
            int64_t pairs = 0;
            int32_t i1 = i;
            do {
                pairs += row_pairs(i1);
                ++i1;
            } while (i1 < m && pairs + row_pairs(i1) <= kItemPairs);
            items.insert(items.end(), {s, i, i1});
            i = i1;
        }
        if (grid) {
            ++g;
            ++g_periodic_stats[1];
        } else {
            ++g_periodic_stats[0];
            g_periodic_stats[2] += (int64_t)m * ((int64_t)m + 1) / 2;
        }
    }
    const int64_t W = (int64_t)(items.size() / 3);
    item_first[B] = W;
    run_first.push_back(W);
    AMP_REQUIRE(W < (int64_t)INT32_MAX, "periodic_pairs: %lld work items", (long long)W);
    if (W == 0) {                                    // every structure is empty
        if (first_count_dev && n > 0) AMP_HIP(hipMemsetAsync(first_count_dev, 0, sizeof(int32_t) * (size_t)n, st));
        return 0;
    }

    int32_t *d_items = nullptr;
    unsigned long long *d_count = nullptr, *d_tile = nullptr, *d_offset = nullptr;
    const uint32_t tiles = scan64::tiles(W);
    Pieces pw;
    pw.add(&d_items, items.size()), pw.add(&d_count, (size_t)W), pw.add(&d_tile, (size_t)tiles + 1), pw.add(&d_offset, (size_t)W);
    if (tmp.carve(pw)) return 1;
    AMP_HIP(hipMemcpyAsync(d_items, items.data(), sizeof(int32_t) * items.size(), hipMemcpyHostToDevice, st));

    const PgCand cand = {d_key, d_poff, (unsigned long long)NG, 0};
    // one launch per run of items of one route: COUNT (out.total = 0, nothing is written) or FILL
    auto launch_runs = [&](bool fill_pass, const PgOut &out) {
        for (size_t k = 0; k < run_route.size(); ++k) {
            const int64_t w0 = run_first[k], len = run_first[k + 1] - w0;
            const dim3 grid((unsigned)((len + kWaves - 1) / kWaves)), block(64 * kWaves);
            const int32_t *it = d_items + 3 * w0;
            unsigned long long *cnt = fill_pass ? nullptr : d_count + w0;
            const unsigned long long *off = fill_pass ? d_offset + w0 : nullptr;
            if (run_route[k] == 0) {
                if (fill_pass)
                    hipLaunchKernelGGL(pg_walk_kernel<true>, grid, block, 0, st, (int32_t)len, it, (const int32_t *)d_off, frac_dev, lat_dev,
                                       (const PgInfo *)d_info, P, cutoff_min, cutoff_max, cnt, off, out);
                else
                    hipLaunchKernelGGL(pg_walk_kernel<false>, grid, block, 0, st, (int32_t)len, it, (const int32_t *)d_off, frac_dev, lat_dev,
                                       (const PgInfo *)d_info, P, cutoff_min, cutoff_max, cnt, off, out);
            } else {
                if (fill_pass)
                    hipLaunchKernelGGL(pg_grid_walk_kernel<true>, grid, block, 0, st, (int32_t)len, it, (const int32_t *)d_off,
                                       (const PgGridS *)d_gs, G, cand, frac_dev, lat_dev, (const PgInfo *)d_info, P, cutoff_min, cutoff_max,
                                       cnt, off, out);
                else
                    hipLaunchKernelGGL(pg_grid_walk_kernel<false>, grid, block, 0, st, (int32_t)len, it, (const int32_t *)d_off,
                                       (const PgGridS *)d_gs, G, cand, frac_dev, lat_dev, (const PgInfo *)d_info, P, cutoff_min, cutoff_max,
                                       cnt, off, out);
            }
        }
    };
    PgOut none = {nullptr, nullptr, nullptr, nullptr, nullptr, 0ull};
    launch_runs(false, none);
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
        launch_runs(true, out);
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

extern "C" int athena_mp_periodic_stats(int64_t out[5])
{
    AMP_REQUIRE(out != nullptr, "periodic_stats: null output");
    std::copy(amp::g_periodic_stats, amp::g_periodic_stats + 5, out);
    return 0;
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
    if (tmp.upload(&d_frac, frac_host, 3 * (size_t)n, st) || tmp.upload(&d_lat, lat_host, 9 * (size_t)B, st)) return 1;
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
    if (tmp.download(feature_out, d_feature, (size_t)E, st) || tmp.download(vec_out, d_vec, 3 * (size_t)E, st) ||
        tmp.download(first_count_out, d_first, (size_t)n, st))
        return 1;
    AMP_HIP(hipStreamSynchronize(st));
    return 0;
}
