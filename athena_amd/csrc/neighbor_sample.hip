// Neighbour-sampled mini-batches of ONE large graph on the device (athena_mp_sampler_create / athena_mp_sample_neighbors; the
// definition is in include/athena_mp.h): seeds -> a sampled rectangular block, relabelled, as a handle the layers take as it is.
// batch_select.hip draws whole structures out of a block-diagonal dataset; this draws rows out of a graph that is one piece.
// Integer only: every array equals the numpy transcription (tests/sampling_reference.py) word for word, two runs are byte-identical.
//
// The definition in one paragraph.  Seed vertex r (0-based), entry at position p of its row: z = seed + 0x9E3779B97F4A7C15 *
// (((r << 32) | p) + 1), the splitmix64 finaliser over z, key = (z & ~0xFFFFFFFF) | p.  A row of L <= k entries (or k = 0) is taken
// whole, otherwise the k smallest keys, in ascending p.  The block's columns are the seeds in the order given, then every other
// chosen column ascending by global id.  A vertex's sample depends on (seed, r) alone.
//
// How.  COUNT (ns_count_kernel): one lane per seed, min(L, k); scan64 gives the block's rowptr and nnz before anything is drawn.
// The same stretch writes slot[seed] = s and reads it back (two launches, plain stores): a mismatch is a repeated seed, a seed
// outside the graph never touches slot; either sets a flag word, and the host then names the first offender from the seeds.
// DRAW (ns_draw_kernel): one 64-lane wave per seed, 4 per block, grid-strided.  The row is streamed 64 entries per step, one key
// per lane; the running list is ONE 64-bit register per lane, merged with wave_sort / wave_merge of knn_cells.h.  After the first
// step a step whose lanes hold no key below the current k-th key is skipped by a ballot: on a hub row almost every step is.  At
// the end the low words (positions) of the first k keys are sorted across the lanes and lane `rank` writes entry_map, the global
// column and the parent's edge id to rowptr[s] + rank.  Whole rows are copied lane-strided without hashing.  No LDS, no atomics,
// no scratch memory.
// RELABEL, plain stores only: key = the global column, or n (past the end) for a column that is a seed (slot >= 0); one
// radix::sort_pairs on exactly bits_for(n) bits; heads by a flag, numbered by scan64; head lanes write vertex_map[m + rank] and
// slot; every entry reads its local column from slot.  ns_finish_kernel puts slot back to -1 at vertex_map's entries -- O(block),
// not O(n) -- gathers the parent's degrees and writes the caller's vertex_map.  A refusal after slot was written resets it at the
// seeds.  The only atomics are the integer column counts of `block` degrees, as bipartite_csr_from_pairs counts them.
// HANDLE: ja [2, nnz] in HBM, rowptr and the degrees on the host go into amp::graph_create_dev, the builder behind
// athena_mp_graph_create fed from HBM.
//
// Host waits per hop: THREE of this file -- (1) nnz with the two flags, (2) the number of new columns, with rowptr, the row
// degrees and the draw statistics riding along, (3) the column degrees, whose count (2) gives -- and then those of graph_create
// itself.  Without a handle (block == NULL and no adj_ia) the third is not made.
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "common.h"
#include "knn_cells.h"
#include "radix_sort.h"
#include "scan64.h"

namespace {

constexpr int kDrawWaves = 4;          // seeds per 256-thread block
constexpr int kDrawMaxBlocks = 2048;   // 8192 waves: 8 per SIMD of 256 compute units
constexpr unsigned long long kGolden = 0x9E3779B97F4A7C15ull;

__device__ inline unsigned long long ns_key(unsigned long long seed, uint32_t r, uint32_t p)
{
    unsigned long long z = seed + kGolden * ((((unsigned long long)r << 32) | p) + 1ull);
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (z & 0xFFFFFFFF00000000ull) | p;
}

// one lane per seed (1-based): cnt = min(L, k), the whole row at k = 0.  A seed outside the graph counts nothing and raises flags[0].
__global__ __launch_bounds__(256) void ns_count_kernel(int32_t m, const int32_t *__restrict__ seeds, int32_t n,
                                                       const int32_t *__restrict__ rowptr, int32_t k, uint32_t *__restrict__ cnt,
                                                       int32_t *__restrict__ flags)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int32_t s = seeds[i] - 1;
    if (s < 0 || s >= n) {
        cnt[i] = 0;
        flags[0] = 1;
        return;
    }
    const int32_t L = rowptr[s + 1] - rowptr[s];
    cnt[i] = (uint32_t)((k == 0 || L <= k) ? L : k);
}

// slot[seed] = i: of two equal seeds one store wins, and ns_slot_check_kernel (the next launch) finds the other
__global__ __launch_bounds__(256) void ns_slot_write_kernel(int32_t m, const int32_t *__restrict__ seeds, int32_t n, int32_t *__restrict__ slot)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int32_t s = seeds[i] - 1;
    if (s >= 0 && s < n) slot[s] = (int32_t)i;
}

__global__ __launch_bounds__(256) void ns_slot_check_kernel(int32_t m, const int32_t *__restrict__ seeds, int32_t n,
                                                            const int32_t *__restrict__ slot, int32_t *__restrict__ vm,
                                                            int32_t *__restrict__ flags)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int32_t s = seeds[i] - 1;
    vm[i] = s;
    if (s >= 0 && s < n && slot[s] != (int32_t)i) flags[1] = 1;
}

// brow[i] = the entries in front of seed i, brow[m] = nnz (below 2^31 or the call is refused before brow is read)
__global__ __launch_bounds__(256) void ns_rowptr_kernel(int32_t m, const unsigned long long *__restrict__ off,
                                                        const unsigned long long *__restrict__ total, int32_t *__restrict__ brow)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > m) return;
    brow[i] = (int32_t)(i < m ? off[i] : *total);
}

// One wave per seed (file header).  entry_map / edge_map (the caller's, 1-based, each may be null) and gcol (0-based global column)
// at brow[i] + rank.  stat [waves][4] = rows drawn, rows copied whole, steps, steps skipped of each wave.
__global__ __launch_bounds__(64 * kDrawWaves) void ns_draw_kernel(int32_t m, const int32_t *__restrict__ seeds,
                                                                  const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                  const int32_t *__restrict__ eid, const int32_t *__restrict__ brow,
                                                                  int32_t k, unsigned long long seed, int32_t *__restrict__ entry_map,
                                                                  int32_t *__restrict__ edge_map, int32_t *__restrict__ gcol,
                                                                  uint32_t *__restrict__ stat)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * kDrawWaves + (threadIdx.x >> 6);
    uint32_t drawn = 0, whole = 0, steps = 0, skipped = 0;
    for (int64_t i = wave; i < m; i += (int64_t)gridDim.x * kDrawWaves) {
        const int32_t r = __builtin_amdgcn_readfirstlane(seeds[i] - 1);
        const int32_t beg = __builtin_amdgcn_readfirstlane(rowptr[r]);
        const int32_t L = __builtin_amdgcn_readfirstlane(rowptr[r + 1]) - beg;
        const int32_t out = __builtin_amdgcn_readfirstlane(brow[i]);
        if (k == 0 || L <= k) {
            ++whole;
            for (int32_t p = lane; p < L; p += 64) {
                const int32_t w = beg + p;
                gcol[out + p] = col[w];
                if (entry_map) entry_map[out + p] = w + 1;
                if (edge_map) edge_map[out + p] = eid[w] + 1;
            }
            continue;
        }
        ++drawn;
        unsigned long long list = kNoKey;
        for (int32_t base = 0; base < L; base += 64) {
            const int32_t p = base + lane;
            unsigned long long key = p < L ? ns_key(seed, (uint32_t)r, (uint32_t)p) : kNoKey;
            ++steps;
            if (base > 0) {
                const unsigned long long kth = __shfl(list, k - 1, 64);
                if (!__any(key < kth)) {
                    ++skipped;
                    continue;
                }
                key = wave_sort(key, lane);
                list = wave_merge(list, key, lane);
            } else {
                list = wave_sort(key, lane);
            }
        }
        // lanes 0 .. k-1 hold the k smallest keys; their low words, ascending, are the chosen positions in CSR order
        const unsigned long long pos = wave_sort(lane < k ? (list & 0xFFFFFFFFull) : kNoKey, lane);
        if (lane < k) {
            const int32_t w = beg + (int32_t)(uint32_t)pos;
            gcol[out + lane] = col[w];
            if (entry_map) entry_map[out + lane] = w + 1;
            if (edge_map) edge_map[out + lane] = eid[w] + 1;
        }
    }
    if (lane == 0) {
        uint32_t *s = stat + 4 * wave;
        s[0] = drawn, s[1] = whole, s[2] = steps, s[3] = skipped;
    }
}

// the sort key of a chosen column: its global id, or n (past the end) when it is a seed
__global__ __launch_bounds__(256) void ns_key_kernel(int64_t N, const int32_t *__restrict__ gcol, const int32_t *__restrict__ slot, int32_t n,
                                                     uint32_t *__restrict__ key)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    const int32_t u = gcol[e];
    key[e] = slot[u] >= 0 ? (uint32_t)n : (uint32_t)u;
}

__global__ __launch_bounds__(256) void ns_head_flag_kernel(int64_t N, const uint32_t *__restrict__ key_s, int32_t n, uint32_t *__restrict__ flag)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    const uint32_t key = key_s[e];
    flag[e] = (key < (uint32_t)n && (e == 0 || key != key_s[e - 1])) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void ns_head_kernel(int64_t N, int32_t m, const uint32_t *__restrict__ flag,
                                                      const unsigned long long *__restrict__ before, const uint32_t *__restrict__ key_s,
                                                      int32_t *__restrict__ vm, int32_t *__restrict__ slot)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N || !flag[e]) return;
    const int32_t id = m + (int32_t)before[e];
    vm[id] = (int32_t)key_s[e];
    slot[key_s[e]] = id;
}

// entry e = (local column, edge id e) 1-based, edge id 0 where the parent has no edge columns; cdeg (may be null) counts the
// entries of each column: an integer count, the same whatever the order of the additions
__global__ __launch_bounds__(256) void ns_local_kernel(int64_t N, const int32_t *__restrict__ gcol, const int32_t *__restrict__ slot,
                                                       int32_t has_edges, int32_t *__restrict__ ja, int32_t *__restrict__ cdeg)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    const int32_t c = slot[gcol[e]];
    ja[2 * e] = c + 1;
    ja[2 * e + 1] = has_edges ? (int32_t)e + 1 : 0;
    if (cdeg) atomicAdd(cdeg + c, 1);
}

// column c < m + *n_new of the block: slot goes back to -1, the parent's degrees are gathered (p_deg_row null: block degrees,
// cdeg already holds the counts), and the caller's vertex_map (1-based, may be null) is written as far as its capacity goes
__global__ __launch_bounds__(256) void ns_finish_kernel(int64_t upper, int32_t m, const unsigned long long *__restrict__ n_new,
                                                        const int32_t *__restrict__ vm, int32_t *__restrict__ slot,
                                                        const int32_t *__restrict__ p_deg_row, const int32_t *__restrict__ p_deg_col,
                                                        int32_t *__restrict__ rdeg, int32_t *__restrict__ cdeg,
                                                        int32_t *__restrict__ vertex_map, int64_t capacity)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= upper || c >= (int64_t)m + (int64_t)*n_new) return;
    const int32_t v = vm[c];
    slot[v] = -1;
    if (p_deg_row) {
        if (c < m) rdeg[c] = p_deg_row[v];
        cdeg[c] = p_deg_col[v];
    }
    if (vertex_map && c < capacity) vertex_map[c] = v + 1;
}

// the refusal path: slot back to -1 at every seed inside the graph
__global__ __launch_bounds__(256) void ns_reset_kernel(int32_t m, const int32_t *__restrict__ seeds, int32_t n, int32_t *__restrict__ slot)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int32_t s = seeds[i] - 1;
    if (s >= 0 && s < n) slot[s] = -1;
}

// a device buffer that only grows; the caller waits for the stream before a call ends, so growing never frees memory in use
struct GrowBuffer {
    char *ptr = nullptr;
    size_t bytes = 0;
    int ensure(size_t want)
    {
        if (want <= bytes) return 0;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
        want += want >> 2;
        AMP_HIP(hipMalloc((void **)&ptr, want));
        bytes = want;
        return 0;
    }
};

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

} // namespace

struct athena_mp_sampler {
    const athena_mp_graph *g = nullptr;
    int32_t n = 0;
    bool has_edges = false;
    int32_t *d_slot = nullptr;     // [n], all -1 between calls
    bool slot_dirty = false;       // a call died between writing slot and putting it back: the next one clears all of it
    GrowBuffer head, body;         // scratch of the stretch before / after nnz is known
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
};

namespace {

int64_t g_sample_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // athena_mp_sample_stats: of the last sample, whichever plan drew it

int sampler_free(athena_mp_sampler *p)
{
    for (hipEvent_t e : p->ev)
        if (e) (void)hipEventDestroy(e);
    if (p->d_slot) (void)hipFree(p->d_slot);
    if (p->head.ptr) (void)hipFree(p->head.ptr);
    if (p->body.ptr) (void)hipFree(p->body.ptr);
    delete p;
    return 0;
}

// the stretch every entry starts with: the counts, the scan, slot written and read back; one wait.  On success slot holds the
// seeds (the caller puts it back); on a refusal it is clean again.
struct CountOut {
    int32_t *brow = nullptr;                       // [m + 1] in p->head
    int32_t *flags = nullptr;
    int32_t *seed_vm = nullptr;                    // [m] in p->head: the seeds 0-based
    unsigned long long *zero = nullptr;            // one word of 0 in p->head
    int64_t nnz = 0;
};

int refuse_seed(const char *who, athena_mp_sampler *p, int32_t m, const int32_t *seeds_dev, const int32_t flags[2])
{
    std::vector<int32_t> s((size_t)m);
    AMP_HIP(hipMemcpy(s.data(), seeds_dev, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost));
    if (flags[0]) {
        for (int32_t i = 0; i < m; ++i)
            if (s[i] < 1 || s[i] > p->n) {
                amp::set_error("%s: seeds(%d) = %d outside [1,%d]", who, i + 1, s[i], p->n);
                return 2;
            }
    }
    std::vector<int32_t> first((size_t)p->n <= (size_t)4 * m ? (size_t)p->n : 0, 0);
    if (!first.empty()) {
        for (int32_t i = 0; i < m; ++i) {
            if (first[s[i] - 1]) {
                amp::set_error("%s: seeds(%d) = %d repeats seeds(%d)", who, i + 1, s[i], first[s[i] - 1]);
                return 2;
            }
            first[s[i] - 1] = i + 1;
        }
    } else {
        std::vector<int32_t> order((size_t)m);
        for (int32_t i = 0; i < m; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return s[a] < s[b]; });
        int32_t best = m, of = 0;
        for (int32_t t = 1; t < m; ++t)
            if (s[order[t]] == s[order[t - 1]] && order[t] < best) best = order[t], of = order[t - 1];
        if (best < m) {
            amp::set_error("%s: seeds(%d) = %d repeats seeds(%d)", who, best + 1, s[best], of + 1);
            return 2;
        }
    }
    amp::set_error("%s: the seed check raised a flag the host cannot confirm", who);
    return 1;
}

int count_stretch(const char *who, athena_mp_sampler *p, int32_t m, const int32_t *seeds_dev, int32_t k, bool claim_slots, CountOut *out)
{
    hipStream_t st = amp::stream();
    const int32_t n = p->n;
    const size_t M = (size_t)m;
    uint32_t *d_cnt = nullptr;
    unsigned long long *d_off = nullptr, *d_tile = nullptr;
    amp::Pieces pc;
    pc.add(&d_cnt, M), pc.add(&d_off, M), pc.add(&d_tile, (size_t)scan64::tiles(m) + 1), pc.add(&out->brow, M + 1), pc.add(&out->flags, 4);
    pc.add(&out->zero, 1), pc.add(&out->seed_vm, M);
    if (p->head.ensure(pc.bytes())) return 1;
    pc.place(p->head.ptr);
    AMP_HIP(hipMemsetAsync(out->flags, 0, (char *)out->zero - (char *)out->flags + 8, st));   // the flags and, a piece further, the zero word
    if (p->slot_dirty) {
        AMP_HIP(hipMemsetAsync(p->d_slot, 0xFF, sizeof(int32_t) * (size_t)std::max(n, 1), st));
        p->slot_dirty = false;
    }
    hipLaunchKernelGGL(ns_count_kernel, dim3(blocks(m)), dim3(256), 0, st, m, seeds_dev, n, (const int32_t *)p->g->rowptr, k, d_cnt, out->flags);
    if (claim_slots) {
        p->slot_dirty = true;
        hipLaunchKernelGGL(ns_slot_write_kernel, dim3(blocks(m)), dim3(256), 0, st, m, seeds_dev, n, p->d_slot);
        hipLaunchKernelGGL(ns_slot_check_kernel, dim3(blocks(m)), dim3(256), 0, st, m, seeds_dev, n, (const int32_t *)p->d_slot, out->seed_vm,
                           out->flags);
    }
    const unsigned long long *d_total = scan64::exclusive<uint32_t>(m, (const uint32_t *)d_cnt, d_tile, d_off, st);
    AMP_LAUNCH_CHECK();
    unsigned long long total = 0;
    int32_t flags[2] = {0, 0};
    AMP_HIP(hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipMemcpyAsync(flags, out->flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));                                 // wait 1
    int rc = 0;
    if (flags[0] || flags[1]) rc = refuse_seed(who, p, m, seeds_dev, flags);
    if (rc == 0 && total >= (1ull << 31)) {
        amp::set_error("%s: the block has %llu entries: 2^31 or more", who, total);
        rc = 2;
    }
    if (rc) {
        if (claim_slots) {
            hipLaunchKernelGGL(ns_reset_kernel, dim3(blocks(m)), dim3(256), 0, st, m, seeds_dev, n, p->d_slot);
            if (hipStreamSynchronize(st) == hipSuccess) p->slot_dirty = false;
        }
        return rc;
    }
    hipLaunchKernelGGL(ns_rowptr_kernel, dim3(blocks((int64_t)m + 1)), dim3(256), 0, st, m, (const unsigned long long *)d_off, d_total, out->brow);
    AMP_LAUNCH_CHECK();
    out->nnz = (int64_t)total;
    return 0;
}

int arguments_check(const char *who, const athena_mp_sampler *p, int32_t m, const int32_t *seeds, int32_t k)
{
    AMP_REQUIRE(p != nullptr, "%s: null sampler", who);
    AMP_REQUIRE(m >= 0, "%s: n_seeds = %d is negative", who, m);
    AMP_REQUIRE(m == 0 || seeds != nullptr, "%s: null seeds", who);
    AMP_REQUIRE(k >= 0 && k <= 64, "%s: fan-out k = %d outside [0,64] (0: every entry)", who, k);
    return 0;
}

// one hop.  Device arrays 1-based, each may be null; adj_ia_out [m + 1] / adj_ja_out [2, nnz] host arrays of the _host entry.
int sample_core(const char *who, athena_mp_sampler *p, int32_t m, const int32_t *seeds_dev, int32_t k, uint64_t seed, int32_t degree_mode,
                int32_t *vertex_map_dev, int64_t vertex_capacity, int32_t *entry_map_dev, int64_t entry_capacity, int32_t *edge_map_dev,
                int64_t edge_capacity, int32_t *adj_ia_out, int32_t *adj_ja_out, int32_t *n_cols_out, int64_t *nnz_out,
                athena_mp_graph **block)
{
    if (block) *block = nullptr;
    if (n_cols_out) *n_cols_out = 0;
    if (nnz_out) *nnz_out = 0;
    if (int rc = arguments_check(who, p, m, seeds_dev, k)) return rc;
    AMP_REQUIRE(degree_mode == 0 || degree_mode == 1, "%s: degree mode %d is neither 0 (block) nor 1 (parent)", who, degree_mode);
    AMP_REQUIRE(n_cols_out != nullptr && nnz_out != nullptr, "%s: null n_cols_out / nnz_out", who);
    const athena_mp_graph *g = p->g;
    const int32_t n = p->n;
    const bool parent_deg = degree_mode == 1, want_handle = block != nullptr || adj_ia_out != nullptr;
    if (!p->has_edges) edge_map_dev = nullptr;                         // a parent without edge columns has no edge_map
    hipStream_t st = amp::stream();
    std::fill(g_sample_stats, g_sample_stats + 8, (int64_t)0);
    const int32_t one = 1, none = 0;
    if (m == 0) {
        if (adj_ia_out) adj_ia_out[0] = 1;
        if (block) return amp::graph_create_dev(0, 0, 0, &one, nullptr, 0, &none, &none, block);
        return 0;
    }

    const auto t0 = std::chrono::steady_clock::now();
    CountOut co;
    if (int rc = count_stretch(who, p, m, seeds_dev, k, true, &co)) return rc;
    const int64_t N = co.nnz;
    g_sample_stats[4] = (int64_t)(1000.0 * ms_since(t0));
    auto refuse = [&](int rc) {
        hipLaunchKernelGGL(ns_reset_kernel, dim3(blocks(m)), dim3(256), 0, st, m, seeds_dev, n, p->d_slot);
        if (hipStreamSynchronize(st) == hipSuccess) p->slot_dirty = false;
        return rc;
    };
    const bool entry_short = (entry_map_dev || adj_ja_out) && entry_capacity < N;
    if (entry_short || (edge_map_dev && edge_capacity < N)) {
        amp::set_error("%s: the %s buffer holds %lld entries, the block has %lld", who, entry_short ? "entry_map" : "edge_map",
                       (long long)(entry_short ? entry_capacity : edge_capacity), (long long)N);
        return refuse(2);
    }

    const int draw_blocks = (int)std::min<int64_t>(kDrawMaxBlocks, ((int64_t)m + kDrawWaves - 1) / kDrawWaves);
    const size_t n_waves = (size_t)draw_blocks * kDrawWaves, Nz = (size_t)N, M = (size_t)m;
    int32_t *d_vm = nullptr, *d_gcol = nullptr, *d_perm = nullptr, *d_perm_t = nullptr, *d_ja = nullptr, *d_cdeg = nullptr, *d_rdeg = nullptr;
    uint32_t *d_key = nullptr, *d_key_s = nullptr, *d_key_t = nullptr, *d_flag = nullptr, *d_stat = nullptr;
    unsigned long long *d_before = nullptr, *d_tile = nullptr;
    char *d_temp = nullptr;
    amp::Pieces pc;
    pc.add(&d_vm, M + Nz), pc.add(&d_gcol, Nz), pc.add(&d_key, Nz), pc.add(&d_key_s, Nz), pc.add(&d_key_t, Nz), pc.add(&d_perm, Nz);
    pc.add(&d_perm_t, Nz), pc.add(&d_flag, Nz), pc.add(&d_before, Nz), pc.add(&d_tile, (size_t)scan64::tiles(N) + 1);
    pc.add(&d_temp, amp::radix::scratch_bytes(N)), pc.add(&d_ja, 2 * Nz), pc.add(&d_cdeg, M + Nz), pc.add(&d_rdeg, M), pc.add(&d_stat, 4 * n_waves);
    if (p->body.ensure(pc.bytes())) return refuse(1);
    pc.place(p->body.ptr);

    auto body = [&](unsigned long long *n_new) -> int {
        AMP_HIP(hipMemcpyAsync(d_vm, co.seed_vm, 4 * M, hipMemcpyDeviceToDevice, st));   // vm [m + nnz] could not be sized before nnz
        AMP_HIP(hipEventRecord(p->ev[0], st));
        hipLaunchKernelGGL(ns_draw_kernel, dim3(draw_blocks), dim3(64 * kDrawWaves), 0, st, m, seeds_dev, (const int32_t *)g->rowptr,
                           (const int32_t *)g->col, (const int32_t *)g->eid, (const int32_t *)co.brow, k, (unsigned long long)seed,
                           entry_map_dev, edge_map_dev, d_gcol, d_stat);
        AMP_LAUNCH_CHECK();
        AMP_HIP(hipEventRecord(p->ev[1], st));
        const unsigned long long *d_new = co.zero;
        if (!parent_deg) AMP_HIP(hipMemsetAsync(d_cdeg, 0, 4 * (M + Nz), st));
        if (N > 0) {
            hipLaunchKernelGGL(ns_key_kernel, dim3(blocks(N)), dim3(256), 0, st, N, (const int32_t *)d_gcol, (const int32_t *)p->d_slot, n, d_key);
            if (int rc = amp::radix::sort_pairs<uint32_t>((const uint32_t *)d_key, nullptr, N, bits_for((unsigned long long)n), d_key_s, d_perm,
                                                          d_key_t, d_perm_t, d_temp, st))
                return rc;
            hipLaunchKernelGGL(ns_head_flag_kernel, dim3(blocks(N)), dim3(256), 0, st, N, (const uint32_t *)d_key_s, n, d_flag);
            d_new = scan64::exclusive<uint32_t>(N, (const uint32_t *)d_flag, d_tile, d_before, st);
            hipLaunchKernelGGL(ns_head_kernel, dim3(blocks(N)), dim3(256), 0, st, N, m, (const uint32_t *)d_flag,
                               (const unsigned long long *)d_before, (const uint32_t *)d_key_s, d_vm, p->d_slot);
            hipLaunchKernelGGL(ns_local_kernel, dim3(blocks(N)), dim3(256), 0, st, N, (const int32_t *)d_gcol, (const int32_t *)p->d_slot,
                               (int32_t)p->has_edges, d_ja, parent_deg ? (int32_t *)nullptr : d_cdeg);
        }
        hipLaunchKernelGGL(ns_finish_kernel, dim3(blocks((int64_t)m + N)), dim3(256), 0, st, (int64_t)m + N, m, d_new, (const int32_t *)d_vm,
                           p->d_slot, parent_deg ? (const int32_t *)g->deg_row : (const int32_t *)nullptr, (const int32_t *)g->deg_col, d_rdeg,
                           d_cdeg, vertex_map_dev, vertex_capacity);
        AMP_LAUNCH_CHECK();
        AMP_HIP(hipEventRecord(p->ev[2], st));
        AMP_HIP(hipMemcpyAsync(n_new, d_new, sizeof(*n_new), hipMemcpyDeviceToHost, st));
        return 0;
    };
    unsigned long long n_new = 0;
    std::vector<uint32_t> stat(4 * n_waves);
    std::vector<int32_t> ia(M + 1), rdeg(M + 1, 0);
    int rc = body(&n_new);
    if (rc == 0) {
        auto tail = [&]() -> int {
            AMP_HIP(hipMemcpyAsync(stat.data(), d_stat, 16 * n_waves, hipMemcpyDeviceToHost, st));
            if (want_handle) {
                AMP_HIP(hipMemcpyAsync(ia.data(), co.brow, 4 * (M + 1), hipMemcpyDeviceToHost, st));
                if (parent_deg) AMP_HIP(hipMemcpyAsync(rdeg.data(), d_rdeg, 4 * M, hipMemcpyDeviceToHost, st));
            }
            AMP_HIP(hipStreamSynchronize(st));                         // wait 2: slot is clean from here on
            return 0;
        };
        rc = tail();
    }
    if (rc) {
        (void)hipStreamSynchronize(st);                                // slot_dirty stays set: the next call clears all of slot
        return rc;
    }
    p->slot_dirty = false;
    for (size_t w = 0; w < n_waves; ++w)
        for (int j = 0; j < 4; ++j) g_sample_stats[j] += stat[4 * w + j];
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p->ev[0], p->ev[1]) == hipSuccess) g_sample_stats[5] = (int64_t)(1000.0 * ms);
    if (hipEventElapsedTime(&ms, p->ev[1], p->ev[2]) == hipSuccess) g_sample_stats[6] = (int64_t)(1000.0 * ms);
    const int64_t n_cols = (int64_t)m + (int64_t)n_new;
    AMP_REQUIRE(n_cols < (int64_t)INT32_MAX, "%s: the block has %lld columns: 2^31 or more", who, (long long)n_cols);
    *n_cols_out = (int32_t)n_cols;
    *nnz_out = N;
    AMP_REQUIRE(vertex_map_dev == nullptr || vertex_capacity >= n_cols, "%s: the vertex_map buffer holds %lld vertices, the block has %lld", who,
                (long long)vertex_capacity, (long long)n_cols);
    if (!want_handle) return 0;

    const auto t1 = std::chrono::steady_clock::now();
    std::vector<int32_t> cdeg((size_t)n_cols + 1, 0);
    AMP_HIP(hipMemcpyAsync(cdeg.data(), d_cdeg, 4 * (size_t)n_cols, hipMemcpyDeviceToHost, st));
    if (adj_ja_out && N > 0) AMP_HIP(hipMemcpyAsync(adj_ja_out, d_ja, 8 * Nz, hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));                                 // wait 3
    for (size_t i = 0; i <= M; ++i) ia[i] += 1;                        // 1-based
    if (!parent_deg)
        for (size_t i = 0; i < M; ++i) rdeg[i] = ia[i + 1] - ia[i];
    if (adj_ia_out) memcpy(adj_ia_out, ia.data(), 4 * (M + 1));
    if (block) {
        rc = amp::graph_create_dev(m, (int32_t)n_cols, N, ia.data(), d_ja, p->has_edges ? (int32_t)N : 0, rdeg.data(), cdeg.data(), block);
        if (rc) return rc;
    }
    g_sample_stats[7] = (int64_t)(1000.0 * ms_since(t1));
    return 0;
}

} // namespace

extern "C" {

int athena_mp_sampler_create(const athena_mp_graph *g, athena_mp_sampler **out)
{
    AMP_REQUIRE(out != nullptr, "sampler_create: null out pointer");
    *out = nullptr;
    AMP_REQUIRE(g != nullptr, "sampler_create: null graph");
    AMP_REQUIRE(g->n_rows == g->n_cols, "sampler_create: a rectangular handle (%d x %d) has no vertices to walk on: n_rows != n_cols", g->n_rows,
                g->n_cols);
    athena_mp_sampler *p = new athena_mp_sampler();
    p->g = g;
    p->n = g->n_rows;
    p->has_edges = g->n_edge_cols > 0;
    auto body = [&]() -> int {
        AMP_HIP(hipMalloc((void **)&p->d_slot, sizeof(int32_t) * (size_t)std::max(p->n, 1)));
        AMP_HIP(hipMemsetAsync(p->d_slot, 0xFF, sizeof(int32_t) * (size_t)std::max(p->n, 1), amp::stream()));
        for (hipEvent_t &e : p->ev) AMP_HIP(hipEventCreate(&e));
        AMP_HIP(hipStreamSynchronize(amp::stream()));
        return 0;
    };
    if (int rc = body()) {
        sampler_free(p);
        return rc;
    }
    *out = p;
    return 0;
}

int athena_mp_sampler_destroy(athena_mp_sampler *p)
{
    if (!p) return 0;
    (void)hipStreamSynchronize(amp::stream());
    return sampler_free(p);
}

int athena_mp_sample_count(athena_mp_sampler *p, int32_t n_seeds, const int32_t *seeds_dev, int32_t k, int32_t *rowptr_dev, int64_t *nnz_out)
{
    const char *who = "sample_count";
    AMP_REQUIRE(nnz_out != nullptr, "%s: null nnz_out", who);
    *nnz_out = 0;
    if (int rc = arguments_check(who, p, n_seeds, seeds_dev, k)) return rc;
    hipStream_t st = amp::stream();
    if (n_seeds == 0) {
        if (rowptr_dev) {
            AMP_HIP(hipMemsetAsync(rowptr_dev, 0, sizeof(int32_t), st));
            AMP_HIP(hipStreamSynchronize(st));
        }
        return 0;
    }
    CountOut co;
    if (int rc = count_stretch(who, p, n_seeds, seeds_dev, k, false, &co)) return rc;
    if (rowptr_dev) AMP_HIP(hipMemcpyAsync(rowptr_dev, co.brow, sizeof(int32_t) * ((size_t)n_seeds + 1), hipMemcpyDeviceToDevice, st));
    AMP_HIP(hipStreamSynchronize(st));
    *nnz_out = co.nnz;
    return 0;
}

int athena_mp_sample_neighbors(athena_mp_sampler *p, int32_t n_seeds, const int32_t *seeds_dev, int32_t k, uint64_t seed, int32_t degree_mode,
                               int32_t *vertex_map_dev, int64_t vertex_capacity, int32_t *entry_map_dev, int64_t entry_capacity,
                               int32_t *edge_map_dev, int64_t edge_capacity, int32_t *n_cols_out, int64_t *nnz_out, athena_mp_graph **block)
{
    return sample_core("sample_neighbors", p, n_seeds, seeds_dev, k, seed, degree_mode, vertex_map_dev, vertex_capacity, entry_map_dev,
                       entry_capacity, edge_map_dev, edge_capacity, nullptr, nullptr, n_cols_out, nnz_out, block);
}

// Fortran arrays in, Fortran arrays out, staged through HBM
int athena_mp_sample_neighbors_host(athena_mp_sampler *p, int32_t n_seeds, const int32_t *seeds_host, int32_t k, uint64_t seed,
                                    int32_t degree_mode, int64_t vertex_capacity, int64_t entry_capacity, int32_t *vertex_map_out,
                                    int32_t *entry_map_out, int32_t *edge_map_out, int32_t *adj_ia_out, int32_t *adj_ja_out,
                                    int32_t *n_cols_out, int64_t *nnz_out, athena_mp_graph **block)
{
    const char *who = "sample_neighbors_host";
    if (block) *block = nullptr;
    if (int rc = arguments_check(who, p, n_seeds, seeds_host, k)) return rc;
    AMP_REQUIRE(n_cols_out != nullptr && nnz_out != nullptr, "%s: null n_cols_out / nnz_out", who);
    hipStream_t st = amp::stream();
    amp::Scratch tmp;
    const size_t M = (size_t)n_seeds;
    int32_t *d_seeds = nullptr, *d_vm = nullptr, *d_em = nullptr, *d_ed = nullptr;
    if (tmp.upload(&d_seeds, seeds_host, M, st)) return 1;
    if (adj_ja_out == nullptr)                                         // size query
        return sample_core(who, p, n_seeds, d_seeds, k, seed, degree_mode, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, n_cols_out,
                           nnz_out, nullptr);
    AMP_REQUIRE(adj_ia_out != nullptr, "%s: null adj_ia", who);
    AMP_REQUIRE(vertex_capacity >= 0 && entry_capacity >= 0, "%s: a negative capacity", who);
    const bool want_edges = edge_map_out != nullptr && p->has_edges;
    if ((vertex_map_out && tmp.get(&d_vm, (size_t)vertex_capacity)) || (entry_map_out && tmp.get(&d_em, (size_t)entry_capacity)) ||
        (want_edges && tmp.get(&d_ed, (size_t)entry_capacity)))
        return 1;
    // entry_capacity is adj_ja's too
    if (int rc = sample_core(who, p, n_seeds, d_seeds, k, seed, degree_mode, d_vm, vertex_capacity, d_em, entry_capacity, d_ed, entry_capacity,
                             adj_ia_out, adj_ja_out, n_cols_out, nnz_out, block))
        return rc;
    const size_t C = (size_t)*n_cols_out, N = (size_t)*nnz_out;
    if (tmp.download(vertex_map_out, d_vm, C, st) || tmp.download(entry_map_out, d_em, N, st) || tmp.download(edge_map_out, d_ed, N, st)) return 1;
    AMP_HIP(hipStreamSynchronize(st));
    return 0;
}

int athena_mp_sample_stats(int64_t out[8])
{
    AMP_REQUIRE(out != nullptr, "sample_stats: null output");
    std::copy(g_sample_stats, g_sample_stats + 8, out);
    return 0;
}

} // extern "C"
