// Top-k vertex selection per graph from learned scores, and the gated rows that go with it: the coarsening step of TopKPooling
// (Graph U-Nets), SAGPool and ASAPool, which works on graphs without coordinates.  The selection is integer-defined: cluster is
// what athena_mp_contract_pairs takes as the map of an induced subgraph (id 0 drops a vertex).
//
// The definition (include/athena_mp.h; tests/topk_reference.py is its numpy transcription, tests compare with np.array_equal):
// inside a graph, value descending, then vertex index ascending; -0 and +0 are equal; every NaN equals every other NaN and lies
// below -inf.  Graph g keeps the first min(k_g, n_g) vertices of that order, and with min_score only those with score >= min_score
// (false for a NaN): a prefix of the order.  The new ids number the kept vertices in ascending vertex index.
//
// How.  THE KEY (tk_asc): the score's bits mapped to a uint32 that ascends with the value -- NaN 0, -0 folded onto +0 (what
// score + 0.0f does, without an add whose subnormals a mode could flush), negatives complemented, the rest with the sign bit set.
// The 32-bit complement descends, and score >= min_score is tk_asc(score) >= tk_asc(min_score) with tk_asc(min_score) != 0.
// PHASE 1 writes flag[v] (kept) and rank[v] (position in its graph's order), by one of two routes chosen per graph on the host:
//   wave (n_g <= 64, tk_wave_kernel): one wave per graph, four per block, one vertex per lane; one 64-bit key per lane, the
//     descending bits on top and the lane below; one wave_sort (knn_cells.h).  The lane at sorted position p holds the key of the
//     vertex of rank p and writes that vertex's two words.  No LDS, no atomics, no scratch.
//   sort (everything else): the vertices of these graphs, compacted in graph order, get (graph << 32) | ~tk_asc with the vertex
//     as value; ONE stable radix::sort_pairs on exactly 32 + bits_for(B - 1) bits -- stability is what gives ties to the smaller
//     index --; tk_rank_kernel: rank = slot - the graph's first slot.
// PHASE 2, shared: scan64::exclusive over the flags numbers the kept vertices; tk_starts_kernel picks the scan's value at every
// graph start and the grand total into sel_offsets [B + 1], which comes home in one copy -- the call's only host wait --;
// tk_fill_kernel (one lane per vertex) writes cluster, selected and order[sel_offsets[g] + rank[v]].  No atomics on data.
//
// THE GATED ROWS use the lane groups of row_groups.h, a group per row sized from F, 16 bytes per lane where F % 4 == 0 and the
// arrays allow it, the same bytes four at a time otherwise.  sr_fwd_kernel: y[r] = x[selected[r] - 1] . gate (without a gate a
// copy, no arithmetic, so every bit is kept).  sr_bwd_x_kernel: dx[v] = dy[cluster[v] - 1] . gate[v], +0 where dropped.
// sr_bwd_gate_kernel: dgate[v] = sum over the columns of fl(dy . x): lane sub owns columns 4 sub .. 4 sub + 3 of every pass on
// BOTH routes and adds them in column order, then a __shfl_xor tree over the group's lanes -- one order whatever the alignment.
// An id outside its range is never followed: the smallest such element lands in a word the host reads (atomicMin, the one atomic).
//
// Resources, -Rpass-analysis=kernel-resource-usage, gfx950 (VGPRs / SGPRs / scratch / LDS bytes / waves per SIMD), the widest
// instance of each template:
//   tk_wave_kernel       16 / 22 / 0 / 0 / 8
//   tk_key_kernel         8 / 20 / 0 / 0 / 8
//   tk_rank_kernel       10 / 22 / 0 / 0 / 8
//   tk_starts_kernel      8 / 22 / 0 / 0 / 8
//   tk_fill_kernel       10 / 21 / 0 / 0 / 8
//   sr_fwd_kernel        21 / 19 / 0 / 0 / 8      (4-byte route without a gate; 16-byte route with one: 14 / 20)
//   sr_bwd_x_kernel      26 / 26 / 0 / 0 / 8      (4-byte route with a gate; 16-byte route: 14 / 26)
//   sr_bwd_gate_kernel   18 / 29 / 0 / 0 / 8      (16-byte route; 4-byte route: 11 / 29)
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "call_scratch.h"
#include "common.h"
#include "knn_cells.h"
#include "radix_sort.h"
#include "row_groups.h"
#include "scan64.h"

namespace amp {
int64_t g_topk_stats[4] = {0, 0, 0, 0};                 // athena_mp_topk_stats: of the last call
}

namespace {

constexpr int kWaveMax = 64;                 // the largest graph of the wave route: one vertex per lane

// the bits of a score -> a uint32 that ascends with the value of the definition: NaN 0, then -inf .. -0 = +0 .. +inf
__host__ __device__ inline uint32_t tk_asc(uint32_t b)
{
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0u;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// score >= min_score on the keys; without a min_score everything passes
__device__ inline bool tk_pass(uint32_t asc, int has_min, uint32_t amin) { return !has_min || (amin != 0u && asc >= amin); }

// the graph of vertex v < off[B]: the first g with off[g + 1] > v
__device__ inline int32_t tk_graph(const int32_t *__restrict__ off, int32_t B, int32_t v)
{
    int32_t lo = 0, hi = B - 1;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid + 1] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one wave per graph of the wave route (gpos[g] < 0), one vertex per lane: the lane at sorted position p writes rank p
__global__ __launch_bounds__(256) void tk_wave_kernel(int32_t B, const int32_t *__restrict__ off, const int32_t *__restrict__ gpos,
                                                      const int32_t *__restrict__ kk, int32_t k_all, const float *__restrict__ score,
                                                      int has_min, uint32_t amin, uint32_t *__restrict__ flag, int32_t *__restrict__ rank)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * kQueryWaves + (threadIdx.x >> 6);
    if (g >= B || gpos[g] >= 0) return;                               // the whole wave
    const int32_t beg = off[g], ng = off[g + 1] - beg;
    if (ng <= 0 || ng > kWaveMax) return;
    const int32_t kg = kk ? kk[g] : k_all;
    unsigned long long key = kNoKey;                                  // no vertex has it: its low word would be a lane
    if (lane < ng) key = ((unsigned long long)(~tk_asc(__float_as_uint(score[beg + lane]))) << 32) | (unsigned long long)lane;
    key = wave_sort(key, lane);
    if (lane < ng) {
        const int32_t v = beg + (int32_t)(key & 63ull);
        rank[v] = lane;
        flag[v] = (lane < kg && tk_pass(~(uint32_t)(key >> 32), has_min, amin)) ? 1u : 0u;
    }
}

// one lane per vertex; a vertex of a sort-route graph writes its key and itself at its compacted place
__global__ __launch_bounds__(256) void tk_key_kernel(int32_t n, int32_t B, const int32_t *__restrict__ off, const int32_t *__restrict__ gpos,
                                                     const float *__restrict__ score, unsigned long long *__restrict__ key,
                                                     int32_t *__restrict__ val)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int32_t g = tk_graph(off, B, (int32_t)v), p = gpos[g];
    if (p < 0) return;
    const int32_t j = p + ((int32_t)v - off[g]);
    key[j] = ((unsigned long long)(uint32_t)g << 32) | (unsigned long long)(~tk_asc(__float_as_uint(score[v])));
    val[j] = (int32_t)v;
}

// one lane per sorted slot: the slots of a graph are its compacted range, in the order of the definition
__global__ __launch_bounds__(256) void tk_rank_kernel(int32_t ns, const unsigned long long *__restrict__ key_s, const int32_t *__restrict__ val_s,
                                                      const int32_t *__restrict__ gpos, const int32_t *__restrict__ kk, int32_t k_all,
                                                      int has_min, uint32_t amin, uint32_t *__restrict__ flag, int32_t *__restrict__ rank)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= ns) return;
    const unsigned long long k = key_s[s];
    const int32_t g = (int32_t)(k >> 32), v = val_s[s], r = (int32_t)s - gpos[g];
    rank[v] = r;
    flag[v] = (r < (kk ? kk[g] : k_all) && tk_pass(~(uint32_t)k, has_min, amin)) ? 1u : 0u;
}

// sel_off[g] = the kept vertices in front of graph g, sel_off[B] = all of them
__global__ __launch_bounds__(256) void tk_starts_kernel(int32_t n, int32_t B, const int32_t *__restrict__ off,
                                                        const unsigned long long *__restrict__ before,
                                                        const unsigned long long *__restrict__ total, int32_t *__restrict__ sel_off)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g > B) return;
    const int32_t o = off[g];
    sel_off[g] = (int32_t)(o < n ? before[o] : total[0]);
}

// one lane per vertex: every output; each may be null
__global__ __launch_bounds__(256) void tk_fill_kernel(int32_t n, int32_t B, const int32_t *__restrict__ off, const uint32_t *__restrict__ flag,
                                                      const int32_t *__restrict__ rank, const unsigned long long *__restrict__ before,
                                                      const int32_t *__restrict__ sel_off, int32_t *__restrict__ cluster,
                                                      int32_t *__restrict__ selected, int32_t *__restrict__ order)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    if (!flag[v]) {
        if (cluster) cluster[v] = 0;
        return;
    }
    const int32_t id = (int32_t)before[v];                            // 0-based
    if (cluster) cluster[v] = id + 1;
    if (selected) selected[id] = (int32_t)v + 1;
    if (order) order[sel_off[tk_graph(off, B, (int32_t)v)] + rank[v]] = (int32_t)v + 1;
}

// y[r, :] = x[selected[r] - 1, :] (. gate[selected[r] - 1]); a group of G lanes per row
template <int G, bool VEC, bool GATE>
__global__ __launch_bounds__(256) void sr_fwd_kernel(int32_t n, int32_t m, const int32_t *__restrict__ selected, const float *__restrict__ x,
                                                     const float *__restrict__ gate, float *__restrict__ y, int32_t F,
                                                     unsigned long long *__restrict__ bad)
{
    const int sub = threadIdx.x & (G - 1);
    const int64_t r = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (r >= m) return;
    const int32_t s = selected[r];
    if (s < 1 || s > n) {
        if (sub == 0) atomicMin(bad, (unsigned long long)r);
        return;
    }
    const float *src = x + (int64_t)(s - 1) * F;
    float *dst = y + r * F;
    const float gv = GATE ? gate[s - 1] : 0.f;
    for (int32_t f0 = 0; f0 < F; f0 += 4 * G) {
        const amp::LaneColumns<G, VEC> cols(sub, f0, F);
        float v[4];
        cols.load4(src, v);
        if (GATE) {
#pragma unroll
            for (int a = 0; a < 4; ++a) v[a] = v[a] * gv;
        }
        cols.store4(dst, v);
    }
}

// dx[v, :] = dy[cluster[v] - 1, :] (. gate[v]), +0 where cluster[v] = 0
template <int G, bool VEC, bool GATE>
__global__ __launch_bounds__(256) void sr_bwd_x_kernel(int32_t n, int32_t m, const int32_t *__restrict__ cluster, const float *__restrict__ dy,
                                                       const float *__restrict__ gate, float *__restrict__ dx, int32_t F,
                                                       unsigned long long *__restrict__ bad)
{
    const int sub = threadIdx.x & (G - 1);
    const int64_t r = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (r >= n) return;
    const int32_t c = cluster[r];
    if (c < 0 || c > m) {
        if (sub == 0) atomicMin(bad, (unsigned long long)r);
        return;
    }
    const float *src = dy + (int64_t)(c > 0 ? c - 1 : 0) * F;
    float *dst = dx + r * F;
    const float gv = GATE ? gate[r] : 0.f;
    for (int32_t f0 = 0; f0 < F; f0 += 4 * G) {
        const amp::LaneColumns<G, VEC> cols(sub, f0, F);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (c > 0) {
            cols.load4(src, v);
            if (GATE) {
#pragma unroll
                for (int a = 0; a < 4; ++a) v[a] = v[a] * gv;
            }
        }
        cols.store4(dst, v);
    }
}

// dgate[v] = the sum over the columns of fl(dy[cluster[v] - 1, col] . x[v, col]), +0 where cluster[v] = 0.  Lane sub adds columns
// f0 + 4 sub .. f0 + 4 sub + 3 of every pass in column order on both routes; then the tree.  No lane leaves before the tree.
template <int G, bool VEC>
__global__ __launch_bounds__(256) void sr_bwd_gate_kernel(int32_t n, int32_t m, const int32_t *__restrict__ cluster, const float *__restrict__ dy,
                                                          const float *__restrict__ x, float *__restrict__ dgate, int32_t F,
                                                          unsigned long long *__restrict__ bad)
{
    const int sub = threadIdx.x & (G - 1);
    const int64_t r = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    int32_t c = 0;
    if (r < n) c = cluster[r];
    const bool refused = c < 0 || c > m;
    if (refused && sub == 0) atomicMin(bad, (unsigned long long)r);
    float acc = 0.f;
    if (c > 0 && !refused) {
        const float *d = dy + (int64_t)(c - 1) * F, *xs = x + r * F;
        for (int32_t f0 = 0; f0 < F; f0 += 4 * G) {
            const int32_t c0 = f0 + 4 * sub;
            if (VEC) {
                if (c0 < F) {                                           // F % 4 == 0: the four are inside together
                    const float4 a = *reinterpret_cast<const float4 *>(d + c0), b = *reinterpret_cast<const float4 *>(xs + c0);
                    acc = acc + a.x * b.x;
                    acc = acc + a.y * b.y;
                    acc = acc + a.z * b.z;
                    acc = acc + a.w * b.w;
                }
            } else {
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    if (c0 + a < F) acc = acc + d[c0 + a] * xs[c0 + a];
            }
        }
    }
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
    if (sub == 0 && r < n && !refused) dgate[r] = acc;
}

// what both selection entries check before anything touches the device: 0, or 2 with the message set.  *room = the sum of
// min(k_g, n_g): what selected and order must hold
int tk_arguments_check(const char *who, int32_t B, int32_t n, const int32_t *off, int32_t k, const int32_t *kk, int64_t *room)
{
    *room = 0;
    AMP_REQUIRE(B >= 0 && n >= 0, "%s: n_graphs = %d, n = %d: negative", who, B, n);
    AMP_REQUIRE(B == 0 || off != nullptr, "%s: null offsets", who);
    AMP_REQUIRE(B > 0 || n == 0, "%s: the offsets end at 0, not at n = %d", who, n);
    if (B == 0) return 0;
    AMP_REQUIRE(off[0] == 0, "%s: offsets(1) = %d, not 0", who, off[0]);
    for (int32_t g = 0; g < B; ++g)
        AMP_REQUIRE(off[g + 1] >= off[g], "%s: offsets(%d) = %d is below offsets(%d) = %d: not ascending", who, g + 2, off[g + 1], g + 1, off[g]);
    AMP_REQUIRE(off[B] == n, "%s: the offsets end at %d, not at n = %d", who, off[B], n);
    AMP_REQUIRE(kk != nullptr || k >= 0, "%s: k = %d is negative", who, k);
    for (int32_t g = 0; g < B; ++g) {
        const int32_t kg = kk ? kk[g] : k;
        AMP_REQUIRE(kg >= 0, "%s: k(%d) = %d is negative", who, g + 1, kg);
        *room += std::min(kg, off[g + 1] - off[g]);
    }
    return 0;
}

// what the gated-row entries check first
int sr_arguments_check(const char *who, int32_t n, int32_t m, int32_t F)
{
    AMP_REQUIRE(n >= 0 && m >= 0, "%s: n = %d, m = %d: negative", who, n, m);
    AMP_REQUIRE(F >= 1, "%s: F = %d: need at least one feature column", who, F);
    return 0;
}

} // namespace

namespace amp {

// Every output may be null alone.  Everything on the library's stream; synchronised on return.
int topk_vertices_core(const char *who, int32_t B, int32_t n, const int32_t *off, const float *score_dev, int32_t k, const int32_t *kk,
                       int32_t has_min, float min_score, int32_t *cluster_dev, int32_t *selected_dev, int32_t *order_dev,
                       int32_t *sel_offsets_out, int64_t *n_selected_out)
{
    std::fill(g_topk_stats, g_topk_stats + 4, (int64_t)0);
    AMP_REQUIRE(n_selected_out != nullptr, "%s: null n_selected_out", who);
    *n_selected_out = 0;
    int64_t room = 0;
    if (int rc = tk_arguments_check(who, B, n, off, k, kk, &room)) return rc;
    // read at every call: a test-only switch
    const char *env = getenv("ATHENA_MP_TOPK_ROUTE");
    const int route = (!env || !*env || !strcmp(env, "auto")) ? 0 : !strcmp(env, "wave") ? 1 : !strcmp(env, "sort") ? 2 : -1;
    AMP_REQUIRE(route >= 0, "%s: ATHENA_MP_TOPK_ROUTE = %s is none of auto, wave, sort", who, env);
    // the route of every graph: gpos[g] = its first compacted slot on the sort route, -1 on the wave route
    std::vector<int32_t> gpos((size_t)B);
    int64_t n_wave = 0, ns = 0, wave_vertices = 0;
    for (int32_t g = 0; g < B; ++g) {
        const int32_t ng = off[g + 1] - off[g];
        AMP_REQUIRE(route != 1 || ng <= kWaveMax, "%s: ATHENA_MP_TOPK_ROUTE = wave, but graph %d has %d vertices, more than %d", who, g + 1, ng,
                    kWaveMax);
        if (route == 1 || (route == 0 && ng <= kWaveMax)) {
            gpos[g] = -1;
            ++n_wave;
            wave_vertices += ng;
        } else {
            gpos[g] = (int32_t)ns;
            ns += ng;
        }
    }
    if (sel_offsets_out) std::fill(sel_offsets_out, sel_offsets_out + B + 1, 0);
    if (n == 0) {
        g_topk_stats[0] = n_wave;
        g_topk_stats[1] = B - n_wave;
        return 0;
    }
    AMP_REQUIRE(score_dev != nullptr, "%s: null score", who);
    const int bits = 32 + bits_for((unsigned long long)(B - 1));
    uint32_t amin = 0;
    if (has_min) {
        uint32_t b;
        memcpy(&b, &min_score, sizeof(b));
        amin = tk_asc(b);
    }

    // one allocation cut into pieces (pieces.h); k's piece is there whether or not it is used
    const size_t N = (size_t)n, S = (size_t)ns, NB = (size_t)B;
    unsigned long long *d_before = nullptr, *d_tile = nullptr, *d_key = nullptr, *d_key_s = nullptr, *d_key_t = nullptr;
    int32_t *d_val = nullptr, *d_val_s = nullptr, *d_val_t = nullptr, *d_rank = nullptr, *d_off = nullptr, *d_gpos = nullptr, *d_k = nullptr,
            *d_soff = nullptr;
    uint32_t *d_flag = nullptr;
    char *d_temp = nullptr;
    Pieces pc;
    pc.add(&d_before, N), pc.add(&d_tile, (size_t)scan64::tiles(n) + 1), pc.add(&d_key, S), pc.add(&d_key_s, S), pc.add(&d_key_t, S);
    pc.add(&d_val, S), pc.add(&d_val_s, S), pc.add(&d_val_t, S), pc.add(&d_flag, N), pc.add(&d_rank, N), pc.add(&d_off, NB + 1);
    pc.add(&d_gpos, NB), pc.add(&d_k, NB), pc.add(&d_soff, NB + 1), pc.add(&d_temp, ns > 0 ? radix::scratch_bytes(ns) : 0);
    Scratch tmp;
    if (tmp.carve(pc)) return 1;
    if (!kk) d_k = nullptr;

    hipStream_t st = stream();
    AMP_HIP(hipMemcpyAsync(d_off, off, sizeof(int32_t) * (NB + 1), hipMemcpyHostToDevice, st));
    AMP_HIP(hipMemcpyAsync(d_gpos, gpos.data(), sizeof(int32_t) * NB, hipMemcpyHostToDevice, st));
    if (kk) AMP_HIP(hipMemcpyAsync(d_k, kk, sizeof(int32_t) * NB, hipMemcpyHostToDevice, st));
    if (wave_vertices > 0)
        hipLaunchKernelGGL(tk_wave_kernel, dim3((unsigned)(((int64_t)B + kQueryWaves - 1) / kQueryWaves)), dim3(64 * kQueryWaves), 0, st, B,
                           (const int32_t *)d_off, (const int32_t *)d_gpos, (const int32_t *)d_k, k, score_dev, (int)has_min, amin, d_flag,
                           d_rank);
    if (ns > 0) {
        hipLaunchKernelGGL(tk_key_kernel, dim3(blocks(n)), dim3(256), 0, st, n, B, (const int32_t *)d_off, (const int32_t *)d_gpos, score_dev,
                           d_key, d_val);
        AMP_LAUNCH_CHECK();
        if (int rc = radix::sort_pairs<unsigned long long>((const unsigned long long *)d_key, (const int32_t *)d_val, ns, bits, d_key_s, d_val_s,
                                                           d_key_t, d_val_t, d_temp, st))
            return rc;
        hipLaunchKernelGGL(tk_rank_kernel, dim3(blocks(ns)), dim3(256), 0, st, (int32_t)ns, (const unsigned long long *)d_key_s,
                           (const int32_t *)d_val_s, (const int32_t *)d_gpos, (const int32_t *)d_k, k, (int)has_min, amin, d_flag, d_rank);
    }
    const unsigned long long *d_total = scan64::exclusive<uint32_t>(n, (const uint32_t *)d_flag, d_tile, d_before, st);
    hipLaunchKernelGGL(tk_starts_kernel, dim3(blocks((int64_t)B + 1)), dim3(256), 0, st, n, B, (const int32_t *)d_off,
                       (const unsigned long long *)d_before, d_total, d_soff);
    // selected and order hold the sum of min(k_g, n_g) elements, and no more than that is kept: the fill needs no count from the host
    if (cluster_dev || selected_dev || order_dev)
        hipLaunchKernelGGL(tk_fill_kernel, dim3(blocks(n)), dim3(256), 0, st, n, B, (const int32_t *)d_off, (const uint32_t *)d_flag,
                           (const int32_t *)d_rank, (const unsigned long long *)d_before, (const int32_t *)d_soff, cluster_dev, selected_dev,
                           order_dev);
    AMP_LAUNCH_CHECK();
    std::vector<int32_t> soff(sel_offsets_out ? 0 : NB + 1);
    int32_t *home = sel_offsets_out ? sel_offsets_out : soff.data();
    AMP_HIP(hipMemcpyAsync(home, d_soff, sizeof(int32_t) * (NB + 1), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));                                // the one wait; scratch dies with this scope
    *n_selected_out = home[B];
    g_topk_stats[0] = n_wave;
    g_topk_stats[1] = B - n_wave;
    g_topk_stats[2] = ns > 0 ? bits : 0;
    g_topk_stats[3] = ns > 0 ? (bits + 7) / 8 : 0;
    return 0;
}

int select_rows_fwd_core(const char *who, int32_t n, int32_t m, int32_t F, const int32_t *selected_dev, const float *x_dev, const float *gate_dev,
                         float *y_dev)
{
    if (int rc = sr_arguments_check(who, n, m, F)) return rc;
    if (m == 0) return 0;
    AMP_REQUIRE(selected_dev != nullptr && y_dev != nullptr && (n == 0 || x_dev != nullptr), "%s: null array", who);
    hipStream_t st = stream();
    Scratch tmp;
    BadWord bad;
    if (int rc = bad.arm(tmp, st)) return rc;
    const int G = group_width(F);
    dispatch_group(G, F % 4 == 0 && aligned16(x_dev, y_dev), gate_dev != nullptr, [&](auto gw, auto v, auto gated) {
        hipLaunchKernelGGL((sr_fwd_kernel<gw(), v(), gated()>), group_grid(m, G), dim3(256), 0, st, n, m, selected_dev, x_dev, gate_dev, y_dev, F,
                           bad.dev);
    });
    AMP_LAUNCH_CHECK();
    return bad.read(who, "selected", selected_dev, 1, n, st);
}

int select_rows_bwd_core(const char *who, int32_t n, int32_t m, int32_t F, const int32_t *cluster_dev, const float *dy_dev, const float *x_dev,
                         const float *gate_dev, float *dx_dev, float *dgate_dev)
{
    if (int rc = sr_arguments_check(who, n, m, F)) return rc;
    if (n == 0) return 0;                                             // empty outputs: a null pointer is what they may be
    AMP_REQUIRE(dx_dev != nullptr || dgate_dev != nullptr, "%s: neither dx nor dgate is asked for", who);
    AMP_REQUIRE(dgate_dev == nullptr || x_dev != nullptr, "%s: dgate needs x", who);
    AMP_REQUIRE(cluster_dev != nullptr && (m == 0 || dy_dev != nullptr), "%s: null array", who);
    hipStream_t st = stream();
    Scratch tmp;
    BadWord bad;
    if (int rc = bad.arm(tmp, st)) return rc;
    const int G = group_width(F);
    if (dx_dev)
        dispatch_group(G, F % 4 == 0 && aligned16(dy_dev, dx_dev), gate_dev != nullptr, [&](auto gw, auto v, auto gated) {
            hipLaunchKernelGGL((sr_bwd_x_kernel<gw(), v(), gated()>), group_grid(n, G), dim3(256), 0, st, n, m, cluster_dev, dy_dev, gate_dev, dx_dev,
                               F, bad.dev);
        });
    if (dgate_dev)
        dispatch_group(G, F % 4 == 0 && aligned16(dy_dev, x_dev), [&](auto gw, auto v) {
            hipLaunchKernelGGL((sr_bwd_gate_kernel<gw(), v()>), group_grid(n, G), dim3(256), 0, st, n, m, cluster_dev, dy_dev, x_dev, dgate_dev, F,
                               bad.dev);
        });
    AMP_LAUNCH_CHECK();
    return bad.read(who, "cluster", cluster_dev, 0, m, st);
}

} // namespace amp

extern "C" int athena_mp_topk_vertices(int32_t n_graphs, int32_t n, const int32_t *offsets_host, const float *score_dev, int32_t k,
                                       const int32_t *k_host, int32_t has_min_score, float min_score, int32_t *cluster_dev,
                                       int32_t *selected_dev, int32_t *order_dev, int32_t *sel_offsets_host, int64_t *n_selected_out)
{
    return amp::topk_vertices_core("topk_vertices", n_graphs, n, offsets_host, score_dev, k, k_host, has_min_score, min_score, cluster_dev,
                                   selected_dev, order_dev, sel_offsets_host, n_selected_out);
}

// Fortran arrays in, Fortran arrays out: selected and order staged with room for the sum of min(k_g, n_g), m of them go home
extern "C" int athena_mp_topk_vertices_host(int32_t n_graphs, int32_t n, const int32_t *offsets, const float *score, int32_t k, const int32_t *k_each,
                                            int32_t has_min_score, float min_score, int32_t *cluster_out, int32_t *selected_out,
                                            int32_t *order_out, int32_t *sel_offsets_out, int64_t *n_selected_out)
{
    const char *who = "topk_vertices_host";
    AMP_REQUIRE(n_selected_out != nullptr, "%s: null n_selected_out", who);
    *n_selected_out = 0;
    int64_t room = 0;
    // before the scores are uploaded: the sizes size the copies
    if (int rc = tk_arguments_check(who, n_graphs, n, offsets, k, k_each, &room)) return rc;
    AMP_REQUIRE(n == 0 || score != nullptr, "%s: null score", who);
    hipStream_t st = amp::stream();
    amp::Scratch tmp;
    const size_t N = (size_t)n, R = (size_t)room;
    float *d_score = nullptr;
    int32_t *d_cluster = nullptr, *d_selected = nullptr, *d_order = nullptr;
    if (tmp.upload(&d_score, score, N, st) || (cluster_out && tmp.get(&d_cluster, N)) || (selected_out && tmp.get(&d_selected, R)) ||
        (order_out && tmp.get(&d_order, R)))
        return 1;
    int64_t m = 0;
    if (int rc = amp::topk_vertices_core(who, n_graphs, n, offsets, d_score, k, k_each, has_min_score, min_score, d_cluster, d_selected, d_order,
                                         sel_offsets_out, &m))
        return rc;
    *n_selected_out = m;
    if (tmp.download(cluster_out, d_cluster, N, st) || tmp.download(selected_out, d_selected, (size_t)m, st) ||
        tmp.download(order_out, d_order, (size_t)m, st))
        return 1;
    AMP_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" int athena_mp_topk_stats(int64_t out[4])
{
    AMP_REQUIRE(out != nullptr, "topk_stats: null output");
    std::copy(amp::g_topk_stats, amp::g_topk_stats + 4, out);
    return 0;
}

extern "C" int athena_mp_select_rows_fwd(int32_t n, int32_t m, int32_t F, const int32_t *selected_dev, const float *x_dev, const float *gate_dev,
                                         float *y_dev)
{
    return amp::select_rows_fwd_core("select_rows_fwd", n, m, F, selected_dev, x_dev, gate_dev, y_dev);
}

extern "C" int athena_mp_select_rows_bwd(int32_t n, int32_t m, int32_t F, const int32_t *cluster_dev, const float *dy_dev, const float *x_dev,
                                         const float *gate_dev, float *dx_dev, float *dgate_dev)
{
    return amp::select_rows_bwd_core("select_rows_bwd", n, m, F, cluster_dev, dy_dev, x_dev, gate_dev, dx_dev, dgate_dev);
}

extern "C" int athena_mp_select_rows_host(int32_t n, int32_t m, int32_t F, const int32_t *selected, const float *x, const float *gate, float *y)
{
    const char *who = "select_rows_host";
    if (int rc = sr_arguments_check(who, n, m, F)) return rc;
    if (m == 0) return 0;
    AMP_REQUIRE(selected != nullptr && y != nullptr && (n == 0 || x != nullptr), "%s: null array", who);
    hipStream_t st = amp::stream();
    amp::Scratch tmp;
    const size_t N = (size_t)n, M = (size_t)m, W = (size_t)F;
    int32_t *d_sel = nullptr;
    float *d_x = nullptr, *d_gate = nullptr, *d_y = nullptr;
    if (tmp.upload(&d_sel, selected, M, st) || tmp.upload(&d_x, x, N * W, st) || (gate && tmp.upload(&d_gate, gate, N, st)) || tmp.get(&d_y, M * W))
        return 1;
    if (int rc = amp::select_rows_fwd_core(who, n, m, F, d_sel, d_x, d_gate, d_y)) return rc;
    if (tmp.download(y, d_y, M * W, st)) return 1;
    AMP_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" int athena_mp_select_rows_bwd_host(int32_t n, int32_t m, int32_t F, const int32_t *cluster, const float *dy, const float *x,
                                              const float *gate, float *dx, float *dgate)
{
    const char *who = "select_rows_bwd_host";
    if (int rc = sr_arguments_check(who, n, m, F)) return rc;
    if (n == 0) return 0;
    AMP_REQUIRE(dx != nullptr || dgate != nullptr, "%s: neither dx nor dgate is asked for", who);
    AMP_REQUIRE(dgate == nullptr || x != nullptr, "%s: dgate needs x", who);
    AMP_REQUIRE(cluster != nullptr && (m == 0 || dy != nullptr), "%s: null array", who);
    hipStream_t st = amp::stream();
    amp::Scratch tmp;
    const size_t N = (size_t)n, M = (size_t)m, W = (size_t)F;
    int32_t *d_cluster = nullptr;
    float *d_dy = nullptr, *d_x = nullptr, *d_gate = nullptr, *d_dx = nullptr, *d_dgate = nullptr;
    if (tmp.upload(&d_cluster, cluster, N, st) || tmp.upload(&d_dy, dy, M * W, st) || (dgate && tmp.upload(&d_x, x, N * W, st)) ||
        (gate && tmp.upload(&d_gate, gate, N, st)) || (dx && tmp.get(&d_dx, N * W)) || (dgate && tmp.get(&d_dgate, N)))
        return 1;
    if (int rc = amp::select_rows_bwd_core(who, n, m, F, d_cluster, d_dy, d_x, d_gate, d_dx, d_dgate)) return rc;
    if (tmp.download(dx, d_dx, N * W, st) || tmp.download(dgate, d_dgate, N, st)) return 1;
    AMP_HIP(hipStreamSynchronize(st));
    return 0;
}
