// Points -> farthest-point samples on the device, a batch of clouds per call: the builder of the SECOND point set of the two-set
// builders (bipartite_graph.hip, knn_bipartite.hip) -- m of a cloud's own points that cover it whatever its density, every prefix
// of which is a sample too, and the covering radius as a by-product.
//
// The definition (include/athena_mp.h; every implementation gives the same arrays, tests compare with np.array_equal):
//   * s(i, j) from d = p_i - p_j per component, s = ((d0*d0) + d1*d1) + d2*d2, every operation rounded to fp32 on its own: the
//     squared distance of the other builders, unchanged.  An overflow is +inf; finite inputs never give a NaN.
//   * per cloud: dmin[j] = +inf; step 1 chooses start; after choosing c, dmin[j] = min(dmin[j], s(j, c)) for every j of the cloud;
//     the next step chooses, among the points NOT YET CHOSEN, the largest dmin, ties to the SMALLER index.
//   * sample = the chosen points as 1-based global indices in selection order, sample_points their rows bit for bit, sample_sqdist
//     the chosen point's dmin when it was chosen (+inf for the first), cover_sqdist the largest dmin of the cloud after the last
//     update (+inf when nothing was chosen of a cloud that has points, 0 for an empty cloud).
//
// How.  ONE WORKGROUP PER CLOUD runs all its steps: the m dependent arg-max steps are the whole cost, and a launch or a grid-wide
// wait per step would be most of it.  No atomics, no grid-wide synchronisation, no cooperative launch.
// THE KEY is one unsigned long long: dmin's bits in the high word (dmin >= 0 or +inf: the bit pattern is monotone), ~index in the
// low word; a chosen point carries the key 0 (its dmin is kept as -1: min(-1, s) = -1, so it stays chosen, and it counts as 0
// for the cover, which is what s(c, c) makes of it).  One max settles the order and the tie rule: an unchosen point's key is never
// 0 (its index is below 2^31), so it beats every chosen one, and m <= n leaves an unchosen point at every step.
// THE REDUCTION: __shfl_xor inside a wave; each wave writes its best key (the register route: and that point's coordinates) to its
// slot in LDS; two alternating sets of slots, so one barrier per step is enough (a wave can reach the write of step t + 2 only
// through the barrier of step t + 1, which every wave reaches after its reads of step t); every wave reads all slots.  The trip
// count of the barrier is m, uniform over the workgroup.  The reduction of the LAST step is the cover.
// REGISTER ROUTE (fps_registers_kernel, a cloud of at most kFpsThreads * kFpsP = 4096 points): coordinates and dmin are loaded
// once and stay in registers, statically indexed: no scratch.
// STREAM ROUTE (fps_stream_kernel, above that): the points in the cell order of build_cell_grid (a cloud's slots are contiguous
// there, perm gives back the index the key holds), dmin in a workspace, the slots cut into chunks of 64 -- one per wave step --
// each with the bounding box of the points actually in it and its cached best key.  Per step a wave tests 64 of its chunks at
// once, one per lane, and then updates those that are not skipped, one at a time with a point per lane.  Every word of the
// workspace is written and read by one and the same thread: nothing is handed over through memory.
//
// EXACT PRUNING, and its proof.  Let c be the new sample, [lo, hi] a chunk's box, q = clamp(c, lo, hi) per component
// (fminf(fmaxf(c, lo), hi)), sb = s(c, q) by the expression above, D = the chunk's largest live dmin (the high word of its cached
// key; chosen points do not count, they are not updated).  The chunk is skipped iff sb >= D and sb > 0 (or all its points are
// chosen).  Claim: for every point p of the box the COMPUTED s(c, p) >= sb, with no margin.
//   * per axis, in exact arithmetic, q lies between c and p or on c: |c - q| <= |c - p|, and c - q is 0 or has the sign of c - p.
//   * fl(c - x) is monotone in x (round-to-nearest is monotone), and odd: |fl(c - q)| <= |fl(c - p)|.  With finite inputs a
//     difference can overflow to +-inf, never to NaN; |inf| is the largest value and the inequality holds there too.
//   * fl(d * d) is monotone in |d| (inf * inf = inf), and fl(a + b) is monotone in each non-negative argument (inf + x = inf; no
//     term is negative, so inf - inf never occurs): by induction over the two additions sb <= s(c, p).
// So sb >= D gives s(c, p) >= D >= dmin[p] for every live p of the chunk: no dmin is lowered, and the cached key stays exact.
// With D = +inf the chunk is skipped only when sb = +inf, and then every s(c, p) = +inf: min(inf, inf) changes nothing.  sb > 0
// is there for c itself: the chunk that holds c has sb = 0 (c - c = 0 exactly), is therefore read, and marks c chosen.  ANY POINT
// ORDER IS CORRECT; the order decides only how much is skipped.
//
// The price.  One cloud is one workgroup is one compute unit: a batch of many clouds fills the device, one large cloud does not.
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "cell_grid.h"
#include "common.h"
#include "knn_cells.h"
#include "two_sets.h"

namespace amp {
int64_t g_fps_stats[4] = {0, 0, 0, 0};       // athena_mp_fps_stats: of the last call
}

namespace {

constexpr int kFpsThreads = 256;             // register route: 4 waves
constexpr int kFpsP = 16;                    // points per thread held in registers
constexpr int kFpsCapacity = kFpsThreads * kFpsP;
constexpr int kFpsStreamThreads = 1024;      // stream route: 16 waves, the whole compute unit
constexpr int kFpsChunk = 64;                // points per chunk: one per lane
constexpr double kFpsCellPoints = 64.0;      // points per grid cell the stream route aims for -- not tuned
constexpr unsigned long long kInfHigh = 0x7f800000ull << 32;

struct FpsTask {
    int32_t cloud, p0, n, m;                 // the cloud, its first point (= its first slot of the cell order), points, samples
    int32_t s0, start, ch0, pad;             // first sample, the first choice (0-based global), first chunk (stream route)
};

__device__ inline unsigned long long wave_key_max(unsigned long long k)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) k = key_max(k, __shfl_xor(k, d, 64));
    return k;
}

__device__ inline unsigned long long fps_key(float dmin, int32_t index)
{
    return dmin < 0.f ? 0ull : ((unsigned long long)__float_as_uint(dmin) << 32) | (unsigned long long)(~(uint32_t)index);
}

// what thread 0 writes of step t: the choice, its row, its dmin when chosen
template <int DIM>
__device__ inline void fps_write_step(int64_t at, int32_t cur, const float *c, float dcur, int32_t *__restrict__ sample,
                                      float *__restrict__ sample_points, float *__restrict__ sample_sqdist)
{
    if (sample) sample[at] = cur + 1;
    if (sample_points)
#pragma unroll
        for (int a = 0; a < DIM; ++a) sample_points[at * DIM + a] = c[a];
    if (sample_sqdist) sample_sqdist[at] = dcur;
}

template <int DIM>
__global__ __launch_bounds__(kFpsThreads) void fps_registers_kernel(const FpsTask *__restrict__ tasks, const float *__restrict__ pts,
                                                                    int32_t *__restrict__ sample, float *__restrict__ sample_points,
                                                                    float *__restrict__ sample_sqdist, float *__restrict__ cover)
{
    constexpr int W = kFpsThreads / 64;
    __shared__ unsigned long long s_key[2][W];
    __shared__ float s_pos[2][W][3];
    const FpsTask task = tasks[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (task.m == 0) {                                       // the whole workgroup
        if (tid == 0 && cover) cover[task.cloud] = task.n > 0 ? INFINITY : 0.f;
        return;
    }
    float p[kFpsP][3], d[kFpsP];
#pragma unroll
    for (int i = 0; i < kFpsP; ++i) {
        const int32_t j = tid + i * kFpsThreads;
        const bool in = j < task.n;
#pragma unroll
        for (int a = 0; a < 3; ++a) p[i][a] = (a < DIM && in) ? pts[(int64_t)(task.p0 + j) * DIM + a] : 0.f;
        d[i] = in ? INFINITY : -1.f;                         // a slot beyond the cloud: chosen from the start
    }
    int32_t cur = task.start;
    float c[3] = {0.f, 0.f, 0.f}, dcur = INFINITY;
#pragma unroll
    for (int a = 0; a < DIM; ++a) c[a] = pts[(int64_t)cur * DIM + a];
    unsigned long long best = 0;
    for (int32_t t = 0; t < task.m; ++t) {
        if (tid == 0) fps_write_step<DIM>((int64_t)task.s0 + t, cur, c, dcur, sample, sample_points, sample_sqdist);
        best = 0;
        float b[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < kFpsP; ++i) {
            const int32_t g = task.p0 + tid + i * kFpsThreads;
            float dn = fminf(d[i], sq_dist<DIM>(p[i], c));
            dn = g == cur ? -1.f : dn;
            d[i] = dn;
            const unsigned long long key = fps_key(dn, g);
            if (key > best) {
                best = key;
#pragma unroll
                for (int a = 0; a < 3; ++a) b[a] = p[i][a];
            }
        }
        const unsigned long long wbest = wave_key_max(best);
        const unsigned long long owner = __ballot(best == wbest && wbest != 0ull);     // keys of unchosen points are distinct
        const int src = owner ? __builtin_ctzll(owner) : 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) b[a] = __shfl(b[a], src, 64);
        const int set = t & 1;
        if (lane == 0) {
            s_key[set][wave] = wbest;
#pragma unroll
            for (int a = 0; a < 3; ++a) s_pos[set][wave][a] = b[a];
        }
        __syncthreads();
        best = 0;
        int from = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const unsigned long long k = s_key[set][w];
            if (k > best) {
                best = k;
                from = w;
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = s_pos[set][from][a];
        cur = (int32_t)~(uint32_t)best;                      // of no interest after the last step (best may be 0 there)
        dcur = __uint_as_float((uint32_t)(best >> 32));
    }
    if (tid == 0 && cover) cover[task.cloud] = best == 0ull ? 0.f : dcur;
}

// chunk k of a stream cloud is the slots p0 + 64 k .. ; group g = chunks 64 g .. 64 g + 63 belongs to wave g % W, chunk 64 g + l
// of it to lane l of that wave (box and cached key), and slot 64 k + l of any of its chunks to lane l (dmin)
template <int DIM>
__global__ __launch_bounds__(kFpsStreamThreads) void fps_stream_kernel(const FpsTask *__restrict__ tasks, const float *__restrict__ pts,
                                                                       const float *__restrict__ sorted, const int32_t *__restrict__ perm,
                                                                       int64_t n_chunks, float *__restrict__ dmin, float *__restrict__ box,
                                                                       unsigned long long *__restrict__ ckey,
                                                                       unsigned long long *__restrict__ stats, int32_t *__restrict__ sample,
                                                                       float *__restrict__ sample_points, float *__restrict__ sample_sqdist,
                                                                       float *__restrict__ cover)
{
    constexpr int W = kFpsStreamThreads / 64;
    __shared__ unsigned long long s_key[2][W];
    __shared__ unsigned long long s_stat[W][2];
    const FpsTask task = tasks[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int32_t nch = (task.n + kFpsChunk - 1) / kFpsChunk;
    const int64_t slot_end = (int64_t)task.p0 + task.n;
    float *const cbox = box + task.ch0;                      // component a of lo at [a * n_chunks + k], of hi at [(3 + a) * n_chunks + k]
    unsigned long long *const key_of = ckey + task.ch0;

    // boxes of the points actually in each chunk, dmin = +inf, the cached key = the chunk's smallest index at +inf
    for (int32_t g = wave; g * 64 < nch; g += W)
        for (int32_t kk = 0; kk < 64 && g * 64 + kk < nch; ++kk) {
            const int32_t k = g * 64 + kk;
            const int64_t slot = (int64_t)task.p0 + (int64_t)k * kFpsChunk + lane;
            const bool in = slot < slot_end;
            float lo[3], hi[3];
            unsigned long long key = 0;
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                const float v = in ? sorted[slot * DIM + a] : 0.f;
                lo[a] = in ? v : INFINITY;
                hi[a] = in ? v : -INFINITY;
            }
            if (in) {
                dmin[slot] = INFINITY;
                key = kInfHigh | (unsigned long long)(~(uint32_t)perm[slot]);
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1)
#pragma unroll
                for (int a = 0; a < DIM; ++a) {
                    lo[a] = fminf(lo[a], __shfl_xor(lo[a], s, 64));
                    hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], s, 64));
                }
            key = wave_key_max(key);
            if (lane == kk) {
#pragma unroll
                for (int a = 0; a < DIM; ++a) {
                    cbox[(int64_t)a * n_chunks + k] = lo[a];
                    cbox[(int64_t)(3 + a) * n_chunks + k] = hi[a];
                }
                key_of[k] = key;
            }
        }

    int32_t cur = task.start;
    float dcur = INFINITY;
    unsigned long long best = 0, examined = 0, skipped = 0;
    for (int32_t t = 0; t < task.m; ++t) {
        float c[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < DIM; ++a) c[a] = pts[(int64_t)cur * DIM + a];      // cur is uniform: a scalar load
        if (tid == 0) fps_write_step<DIM>((int64_t)task.s0 + t, cur, c, dcur, sample, sample_points, sample_sqdist);
        unsigned long long wbest = 0;
        for (int32_t g = wave; g * 64 < nch; g += W) {
            const int32_t k = g * 64 + lane;
            const bool has = k < nch;
            unsigned long long mine = has ? key_of[k] : 0ull;
            bool read = false;
            if (has && mine != 0ull) {                       // key 0: every point of the chunk is chosen
                float q[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int a = 0; a < DIM; ++a)
                    q[a] = fminf(fmaxf(c[a], cbox[(int64_t)a * n_chunks + k]), cbox[(int64_t)(3 + a) * n_chunks + k]);
                const float sb = sq_dist<DIM>(c, q);
#ifdef ATHENA_MP_FPS_NO_PRUNE
                read = true;                                 // scripts/bench_fps.py: what the pruning saves
#else
                read = !(sb >= __uint_as_float((uint32_t)(mine >> 32)) && sb > 0.f);      // header
#endif
            }
            unsigned long long todo = __ballot(read);
            const unsigned long long all = __ballot(has);
            examined += (unsigned long long)__popcll(all);
            skipped += (unsigned long long)(__popcll(all) - __popcll(todo));
            while (todo) {
                const int kk = __builtin_ctzll(todo);
                todo &= todo - 1;
                const int64_t slot = (int64_t)task.p0 + ((int64_t)g * 64 + kk) * kFpsChunk + lane;
                unsigned long long key = 0;
                if (slot < slot_end) {
                    const float d = dmin[slot];
                    if (d >= 0.f) {                          // -1: chosen
                        const int32_t gi = perm[slot];
                        float pj[3] = {0.f, 0.f, 0.f};
#pragma unroll
                        for (int a = 0; a < DIM; ++a) pj[a] = sorted[slot * DIM + a];
                        float dn = fminf(d, sq_dist<DIM>(pj, c));
                        dn = gi == cur ? -1.f : dn;
                        if (dn != d) dmin[slot] = dn;
                        key = fps_key(dn, gi);
                    }
                }
                key = wave_key_max(key);
                if (lane == kk) {
                    mine = key;
                    key_of[k] = key;
                }
            }
            wbest = key_max(wbest, mine);
        }
        wbest = wave_key_max(wbest);
        const int set = t & 1;
        if (lane == 0) s_key[set][wave] = wbest;
        __syncthreads();
        best = wave_key_max(lane < W ? s_key[set][lane] : 0ull);
        cur = __builtin_amdgcn_readfirstlane(best == 0ull ? task.start : (int32_t)~(uint32_t)best);   // 0: only after the last step
        dcur = __uint_as_float((uint32_t)(best >> 32));
    }
    if (lane == 0) {
        s_stat[wave][0] = examined;
        s_stat[wave][1] = skipped;
    }
    __syncthreads();
    if (tid == 0) {
        if (cover) cover[task.cloud] = best == 0ull ? 0.f : dcur;
        unsigned long long e = 0, s = 0;
        for (int w = 0; w < W; ++w) {
            e += s_stat[w][0];
            s += s_stat[w][1];
        }
        stats[2 * (int64_t)blockIdx.x] = e;
        stats[2 * (int64_t)blockIdx.x + 1] = s;
    }
}

// About kFpsCellPoints points per cell, so that a chunk of consecutive slots of the cell order is a cell or two.  An axis of zero
// extent, or one too long for a sane fp32 cell width, is one cell.  Correctness does not depend on any of this (header).
inline Grid make_fps_grid(const Box &box, int dim, int32_t m)
{
    Grid g;
    double extent[3] = {0, 0, 0}, volume = 1.0;
    int active = 0;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = a < dim ? box.lo[a] : 0.f;
        g.nc[a] = 1;
        g.inv_w[a] = 0.f;
        if (a < dim) extent[a] = (double)box.hi[a] - (double)box.lo[a];
        if (extent[a] > 0.0 && extent[a] < 1e37) {
            volume *= extent[a];
            ++active;
        } else {
            extent[a] = 0.0;
        }
    }
    if (active == 0) return g;
    const double w = pow(volume / std::max(1.0, (double)m / kFpsCellPoints), 1.0 / active);
    for (int a = 0; a < 3; ++a) {
        if (extent[a] == 0.0) continue;
        const double cells = floor(extent[a] / w);
        g.nc[a] = !(cells >= 1.0) ? 1 : cells > (double)kMaxCellsAxis ? kMaxCellsAxis : (int32_t)cells;
        const float inv_w = (float)((double)g.nc[a] / extent[a]);
        if (g.nc[a] > 1 && inv_w >= 1e-30f && inv_w <= 1e30f) g.inv_w[a] = inv_w;
        else g.nc[a] = 1;
    }
    return g;
}

inline Grid one_cell_grid(const Box &box, int dim)
{
    Grid g;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = a < dim ? box.lo[a] : 0.f;
        g.nc[a] = 1;
        g.inv_w[a] = 0.f;
    }
    return g;
}

// what every entry checks before anything touches the device: 0, or 2 with the message set
int fps_arguments_check(const char *who, int32_t B, int32_t n, const int32_t *offsets, int32_t dim, int32_t m_total,
                        const int32_t *sample_offsets, const int32_t *start)
{
    AMP_REQUIRE(dim >= 1 && dim <= 3, "%s: dim = %d outside [1,3]", who, dim);
    AMP_REQUIRE(B >= 0, "%s: n_clouds = %d is negative", who, B);
    AMP_REQUIRE(n >= 0 && m_total >= 0, "%s: n = %d, n_samples = %d: negative", who, n, m_total);
    if (int rc = named_offsets_check(who, "offsets", "points", B, offsets, n)) return rc;
    if (int rc = named_offsets_check(who, "sample_offsets", "samples", B, sample_offsets, m_total)) return rc;
    for (int32_t b = 0; b < B; ++b) {
        const int32_t nb = offsets[b + 1] - offsets[b], mb = sample_offsets[b + 1] - sample_offsets[b];
        AMP_REQUIRE(mb <= nb, "%s: cloud %d: %d samples asked of %d points", who, b + 1, mb, nb);
        if (start && mb > 0 && start[b] != 0)
            AMP_REQUIRE(start[b] > offsets[b] && start[b] <= offsets[b + 1], "%s: cloud %d: start = %d outside its points %d .. %d", who, b + 1,
                        start[b], offsets[b] + 1, offsets[b + 1]);
    }
    return 0;
}

template <typename... A> void launch_fps_registers(int dim, int32_t n_tasks, hipStream_t st, A... a)
{
    const dim3 grid((unsigned)n_tasks), block(kFpsThreads);
    if (dim == 1) hipLaunchKernelGGL(fps_registers_kernel<1>, grid, block, 0, st, a...);
    else if (dim == 2) hipLaunchKernelGGL(fps_registers_kernel<2>, grid, block, 0, st, a...);
    else hipLaunchKernelGGL(fps_registers_kernel<3>, grid, block, 0, st, a...);
}

template <typename... A> void launch_fps_stream(int dim, int32_t n_tasks, hipStream_t st, A... a)
{
    const dim3 grid((unsigned)n_tasks), block(kFpsStreamThreads);
    if (dim == 1) hipLaunchKernelGGL(fps_stream_kernel<1>, grid, block, 0, st, a...);
    else if (dim == 2) hipLaunchKernelGGL(fps_stream_kernel<2>, grid, block, 0, st, a...);
    else hipLaunchKernelGGL(fps_stream_kernel<3>, grid, block, 0, st, a...);
}

} // namespace

namespace amp {

// Every output may be null alone.  Everything on the library's stream; synchronised on return.
int farthest_points_core(const char *who, int32_t B, int32_t n, const int32_t *offsets, int32_t dim, const float *points_dev,
                         int32_t m_total, const int32_t *sample_offsets, const int32_t *start, int32_t *sample_dev,
                         float *sample_points_dev, float *sample_sqdist_dev, float *cover_dev)
{
    std::fill(g_fps_stats, g_fps_stats + 4, (int64_t)0);
    if (int rc = fps_arguments_check(who, B, n, offsets, dim, m_total, sample_offsets, start)) return rc;
    AMP_REQUIRE(n == 0 || points_dev != nullptr, "%s: null points", who);
    int route = 0;                                           // 0 auto, 1 registers, 2 stream: tests pin it, read at every call
    if (const char *env = getenv("ATHENA_MP_FPS_ROUTE")) {
        if (!strcmp(env, "registers")) route = 1;
        else if (!strcmp(env, "stream")) route = 2;
        else AMP_REQUIRE(!strcmp(env, "auto") || !*env, "%s: ATHENA_MP_FPS_ROUTE = \"%s\" is none of auto, registers, stream", who, env);
    }
    if (B == 0) return 0;
    std::vector<FpsTask> reg, stream_tasks;
    int64_t n_chunks = 0;
    for (int32_t b = 0; b < B; ++b) {
        FpsTask t;
        t.cloud = b;
        t.p0 = offsets[b];
        t.n = offsets[b + 1] - offsets[b];
        t.s0 = sample_offsets[b];
        t.m = sample_offsets[b + 1] - sample_offsets[b];
        t.start = (start && start[b] != 0) ? start[b] - 1 : t.p0;
        t.ch0 = 0;
        t.pad = 0;
        const bool fits = t.n <= kFpsCapacity;
        AMP_REQUIRE(route != 1 || t.m == 0 || fits, "%s: cloud %d: ATHENA_MP_FPS_ROUTE = registers holds %d points, the cloud has %d", who,
                    b + 1, kFpsCapacity, t.n);
        if (t.m == 0 || (route != 2 && fits)) {
            reg.push_back(t);
        } else {
            t.ch0 = (int32_t)n_chunks;
            n_chunks += (t.n + kFpsChunk - 1) / kFpsChunk;
            stream_tasks.push_back(t);
        }
    }
    hipStream_t st = stream();
    Scratch tmp;
    CellGrid cg;
    std::vector<char> streamed((size_t)B, 0);
    for (const FpsTask &t : stream_tasks) streamed[t.cloud] = 1;
    if (n > 0) {                                             // either way the points are scanned for a non-finite coordinate
        if (stream_tasks.empty()) {
            BatchItems it;
            std::vector<Box> box;
            if (int rc = batch_boxes(who, true, B, offsets, dim, points_dev, st, tmp, it, box)) return rc;
        } else if (int rc = build_cell_grid(who, true, B, n, offsets, dim, points_dev, st, tmp, [&](const Box &box, int32_t m, int32_t b) {
                       return streamed[b] ? make_fps_grid(box, dim, m) : one_cell_grid(box, dim);
                   }, cg))
            return rc;
    }
    FpsTask *d_tasks = nullptr;
    const size_t n_reg = reg.size(), n_str = stream_tasks.size();
    reg.insert(reg.end(), stream_tasks.begin(), stream_tasks.end());
    if (tmp.get(&d_tasks, reg.size())) return 1;
    AMP_HIP(hipMemcpyAsync(d_tasks, reg.data(), sizeof(FpsTask) * reg.size(), hipMemcpyHostToDevice, st));
    if (n_reg > 0) launch_fps_registers(dim, (int32_t)n_reg, st, (const FpsTask *)d_tasks, points_dev, sample_dev, sample_points_dev,
                                        sample_sqdist_dev, cover_dev);
    std::vector<unsigned long long> stats(2 * n_str);
    if (n_str > 0) {
        float *d_dmin = nullptr, *d_box = nullptr;
        unsigned long long *d_ckey = nullptr, *d_stats = nullptr;
        Pieces pc;
        pc.add(&d_dmin, (size_t)n), pc.add(&d_box, 6 * (size_t)n_chunks), pc.add(&d_ckey, (size_t)n_chunks), pc.add(&d_stats, 2 * n_str);
        if (tmp.carve(pc)) return 1;
        launch_fps_stream(dim, (int32_t)n_str, st, (const FpsTask *)(d_tasks + n_reg), points_dev, (const float *)cg.d_sorted,
                          (const int32_t *)cg.d_perm, n_chunks, d_dmin, d_box, d_ckey, d_stats, sample_dev, sample_points_dev,
                          sample_sqdist_dev, cover_dev);
        AMP_LAUNCH_CHECK();
        AMP_HIP(hipMemcpyAsync(stats.data(), d_stats, sizeof(unsigned long long) * 2 * n_str, hipMemcpyDeviceToHost, st));
    }
    AMP_LAUNCH_CHECK();
    AMP_HIP(hipStreamSynchronize(st));                       // scratch dies with this scope
    g_fps_stats[0] = m_total;
    for (size_t s = 0; s < n_str; ++s) {
        g_fps_stats[1] += (int64_t)stats[2 * s];
        g_fps_stats[2] += (int64_t)stats[2 * s + 1];
    }
    g_fps_stats[3] = (int64_t)n_str;
    return 0;
}

} // namespace amp

extern "C" int athena_mp_farthest_points(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim, const float *points_dev,
                                         int32_t n_samples, const int32_t *sample_offsets_host, const int32_t *start_host,
                                         int32_t *sample_dev, float *sample_points_dev, float *sample_sqdist_dev, float *cover_sqdist_dev)
{
    return amp::farthest_points_core("farthest_points", n_clouds, n, offsets_host, dim, points_dev, n_samples, sample_offsets_host,
                                     start_host, sample_dev, sample_points_dev, sample_sqdist_dev, cover_sqdist_dev);
}

// Fortran arrays in, Fortran arrays out
extern "C" int athena_mp_farthest_points_host(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim,
                                              const float *points_host, int32_t n_samples, const int32_t *sample_offsets_host,
                                              const int32_t *start_host, int32_t *sample_out, float *sample_points_out,
                                              float *sample_sqdist_out, float *cover_sqdist_out)
{
    const char *who = "farthest_points_host";
    // before the points are uploaded: dim and the counts size the copies
    if (int rc = fps_arguments_check(who, n_clouds, n, offsets_host, dim, n_samples, sample_offsets_host, start_host)) return rc;
    AMP_REQUIRE(n == 0 || points_host != nullptr, "%s: null points", who);
    hipStream_t st = amp::stream();
    amp::Scratch tmp;
    const size_t m = (size_t)n_samples, B = (size_t)n_clouds;
    float *d_p = nullptr, *d_sp = nullptr, *d_sq = nullptr, *d_cover = nullptr;
    int32_t *d_s = nullptr;
    if (tmp.upload(&d_p, points_host, (size_t)n * dim, st) || (sample_out && tmp.get(&d_s, m)) || (sample_points_out && tmp.get(&d_sp, m * dim)) ||
        (sample_sqdist_out && tmp.get(&d_sq, m)) || (cover_sqdist_out && tmp.get(&d_cover, B)))
        return 1;
    if (int rc = amp::farthest_points_core(who, n_clouds, n, offsets_host, dim, d_p, n_samples, sample_offsets_host, start_host, d_s, d_sp,
                                           d_sq, d_cover))
        return rc;
    if (tmp.download(sample_out, d_s, m, st) || tmp.download(sample_points_out, d_sp, m * dim, st) || tmp.download(sample_sqdist_out, d_sq, m, st) ||
        tmp.download(cover_sqdist_out, d_cover, B, st))
        return 1;
    AMP_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" int athena_mp_fps_stats(int64_t out[4])
{
    AMP_REQUIRE(out != nullptr, "fps_stats: null output");
    std::copy(amp::g_fps_stats, amp::g_fps_stats + 4, out);
    return 0;
}
