// Lane groups over the rows of a CSR: the kernel scheme of interp.hip, pool.hip, edge_gather.hip and attention.hip, held once.
//
// G lanes share a row, G the smallest power of two from 4 with 4 G >= F (a full wave from F = 193; more columns than 256 take
// further passes), so no lane idles at F = 16, 64, 128, 256.  The group's lanes load what they need of G entries, one entry per
// lane; the entries then pass through the group in entry order (__shfl, no LDS) while every lane works on its own four feature
// columns: whatever a kernel does per entry, it does in row order, bit for bit, whatever the row length -- a hub row takes more
// rounds.  The row loads carry no branch (a lane past its row's end reads row 0 and keeps what it has), so the four entries of an
// unrolled step are in flight together; the wave's longest row is a scalar loop bound.  That entry loop -- k0, nj, four j a step --
// stays written out in each kernel: behind a callable it changed the registers of the kernels that were tried.  So do the
// columns of interp_gather_kernel, pool_fwd_kernel and pool_bwd_x_kernel and the whole of interp_bwd_coords_kernel: with the
// helpers below their register counts moved (profiles/row_groups_isa.txt) or, pool_fwd_kernel, a launch ran slower
// (profiles/row_groups_ab.txt); a change to the scheme has to visit those four as well.
// Two load/store routes with the same bytes: a lane owns columns 4 sub .. 4 sub + 3 and moves them 16 bytes at a time when the
// widths are multiples of 4 and every array of the call starts on a 16-byte boundary (the launcher's `vec`); otherwise columns
// sub + G a, four bytes at a time.  Each column sees the same entries in the same order on either route.  A column past the width
// is read at the last valid place and never stored.  No LDS, no atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace amp {

// the smallest power of two from 4 with 4 G >= F, at most a wave
inline int group_width(int32_t F)
{
    int G = 4;
    while (G < 64 && 4 * G < F) G *= 2;
    return G;
}

// blocks of 256 lanes, 256 / G rows each
inline dim3 group_grid(int32_t rows, int G) { return dim3((unsigned)(((int64_t)rows + 256 / G - 1) / (256 / G))); }

// this lane's place in its group, the group's row of (n, rowptr), and the wave's longest row
template <int G>
struct RowGroup {
    int sub, first;         // the lane within its group; the wave's lane that holds the group's entry 0
    int64_t row;            // may be >= n: then len = 0, and the lane still takes part in every round
    int32_t beg, len;
    int32_t longest;        // the longest row of the wave, as every lane holds it
    int32_t rounds;         // ... and as a scalar loop bound
    __device__ __forceinline__ RowGroup(int32_t n, const int32_t *__restrict__ rowptr)
    {
        const int lane = threadIdx.x & 63;
        sub = lane & (G - 1), first = lane & ~(G - 1);
        row = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
        beg = 0, len = 0;
        if (row < n) {
            beg = rowptr[row];
            len = rowptr[row + 1] - beg;
        }
        longest = len;
#pragma unroll
        for (int o = 32; o >= G; o >>= 1) longest = max(longest, __shfl_xor(longest, o));
        rounds = __builtin_amdgcn_readfirstlane(longest);
    }
};

template <typename T> using Quad = std::conditional_t<std::is_same<T, float>::value, float4, int4>;   // four of float or int32_t

// The four columns of lane `sub` in rows F wide, in the pass that starts at column f0.  The width is the constructor's argument: a
// kernel that moves blocks of two widths holds one set per block.  The forms for two rows and the column offset keep each
// kernel's accesses, and their index arithmetic, in the order in which they were written out: the compiler's register allocation
// follows that order.
template <int G, bool VEC>
struct LaneColumns {
    int32_t F;
    int32_t col[4];         // the column numbers: col[a] < F is what has a value and is stored
    int32_t at4;            // VEC: where the four are read: past F, the last valid place (F >= 4 there)
    __device__ __forceinline__ LaneColumns(int sub, int32_t f0, int32_t width) : F(width)
    {
#pragma unroll
        for (int a = 0; a < 4; ++a) col[a] = VEC ? f0 + 4 * sub + a : f0 + sub + G * a;
        at4 = min(col[0], F - 4);
    }
    // where column a is read: past F, the last valid place
    __device__ __forceinline__ int32_t at(int a) const { return VEC ? at4 + a : min(col[a], F - 1); }
    // v = r[off + column]
    template <typename T> __device__ __forceinline__ void load4(const T *r, T (&v)[4], int32_t off = 0) const
    {
        if (VEC) {
            const Quad<T> q = *reinterpret_cast<const Quad<T> *>(r + off + at4);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a) v[a] = r[off + at(a)];
        }
    }
    // ... of two rows, column by column on the 4-byte route
    template <typename T, typename U> __device__ __forceinline__ void load4(const T *r, T (&v)[4], const U *s, U (&u)[4]) const
    {
        if (VEC) {
            load4(r, v);
            load4(s, u);
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int32_t f = at(a);
                v[a] = r[f];
                u[a] = s[f];
            }
        }
    }
    // r[off + column] = v for the columns below F
    template <typename T> __device__ __forceinline__ void store4(T *r, const T (&v)[4], int32_t off = 0) const
    {
        if (VEC) {
            if (col[0] < F) *reinterpret_cast<Quad<T> *>(r + off + col[0]) = Quad<T>{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (col[a] < F) r[off + col[a]] = v[a];
        }
    }
};

// f(g, v) with the group width and the route as compile-time constants: f is a generic lambda that names its kernel instance,
// kernel<g(), v()>
template <typename Fn> inline void dispatch_group(int G, bool vec, Fn &&f)
{
    auto route = [&](auto g) {
        if (vec) f(g, std::true_type{});
        else f(g, std::false_type{});
    };
    switch (G) {
    case 4: route(std::integral_constant<int, 4>{}); break;
    case 8: route(std::integral_constant<int, 8>{}); break;
    case 16: route(std::integral_constant<int, 16>{}); break;
    case 32: route(std::integral_constant<int, 32>{}); break;
    default: route(std::integral_constant<int, 64>{}); break;
    }
}

// ... and f(g, v, rel), for the kernels that take the edge gather's `relative` as a template argument
template <typename Fn> inline void dispatch_group(int G, bool vec, bool relative, Fn &&f)
{
    dispatch_group(G, vec, [&](auto g, auto v) {
        if (relative) f(g, v, std::true_type{});
        else f(g, v, std::false_type{});
    });
}

} // namespace amp
