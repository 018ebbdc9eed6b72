// Duvenaud degree-bucket plan of a graph handle (the definition is in include/athena_mp.h, athena_mp_duvenaud_plan): the vertices
// sorted by degree bucket (stable), every bucket cut into 16-vertex tiles, and the four copies of the tile slots the kernels of
// duv_mfma.hip read.  Two routes write the same arrays byte for byte (tests/test_gpu_bucket_plan.py compares them):
//   host     one pass over h_deg_row, a counting sort, the tile list, five blocking uploads;
//   device   the host only COUNTS (sizes of the five arrays, the host-side offset tables); keys, the stable sort (one 8-bit counting
//            pass of radix_sort.h, so at most 256 buckets), the tile offsets and the tile slots are made in HBM on the library's
//            stream, with no copy in either direction and no synchronise: a mini-batch child (batch_select.hip) is planned
//            behind its own select without the stream draining.
// ATHENA_MP_BUCKET_PLAN = auto | host | device pins the route (tests only; read at every build).
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "common.h"
#include "radix_sort.h"

namespace {

constexpr int kWsPlan = 19;      // workspace slot: keys [n], sorted keys [n], the sort's histogram
constexpr int kMaxDeviceBuckets = 256;   // one 8-bit digit

std::atomic<int64_t> g_host_builds{0}, g_device_builds{0}, g_reused{0};

__global__ void bucket_key_kernel(int32_t n, const int32_t *__restrict__ deg, int min_deg, int max_deg, uint32_t *__restrict__ key)
{
    const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    key[v] = (uint32_t)(max(min_deg, min(deg[v], max_deg)) - min_deg);
}

// one workgroup of 256: bin_start[b] = first slot of bucket b in bucket_perm (radix_scan_bins left it there), n the end of the
// last bucket; tile_off[b] = tiles of the buckets before b, tile_off[nb] = all tiles
__global__ __launch_bounds__(amp::radix::kThreads) void bucket_tile_off_kernel(const uint32_t *__restrict__ bin_start, int32_t n, int nb,
                                                                              int32_t *__restrict__ tile_off)
{
    const int b = threadIdx.x;
    uint32_t tiles = 0;
    if (b < nb) {
        const uint32_t end = b + 1 < amp::radix::kBins ? bin_start[b + 1] : (uint32_t)n;   // bins past the last bucket are empty: they start at n
        tiles = (end - bin_start[b] + 15u) >> 4;
    }
    uint32_t total;
    const uint32_t before = amp::radix::block_exclusive_scan(tiles, &total);
    if (b < nb) tile_off[b] = (int32_t)before;
    if (b == 0) tile_off[nb] = (int32_t)total;
}

// one lane per tile slot (16 nt of them).  rows: the four copies back to back, [16 nt] each (see duvenaud_buckets_host)
__global__ void bucket_tile_kernel(int32_t nt, int nb, const uint32_t *__restrict__ bin_start, const int32_t *__restrict__ tile_off,
                                   int32_t n, const int32_t *__restrict__ perm, int32_t *__restrict__ tstart,
                                   int32_t *__restrict__ tinfo, int32_t *__restrict__ rows)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (int64_t)16 * nt) return;
    const int32_t t = (int32_t)(s >> 4);
    const int i = (int)(s & 15);
    int lo = 0, hi = nb;   // the LAST bucket whose first tile is <= t (empty buckets repeat an offset): tile_off[lo] <= t < tile_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_off[mid] <= t) lo = mid; else hi = mid;
    }
    const int32_t b_beg = (int32_t)bin_start[lo];
    const int32_t b_end = lo + 1 < amp::radix::kBins ? (int32_t)bin_start[lo + 1] : n;
    const int32_t start = b_beg + 16 * (t - tile_off[lo]);
    const int32_t cnt = min(16, b_end - start);
    const int32_t v = perm[start + (i < cnt ? i : 0)];
    const int32_t sv = i < cnt ? v : ~v;
    const int tp = 4 * (i & 3) + (i >> 2);
    const size_t nt16 = (size_t)16 * nt, base = (size_t)16 * t;
    rows[base + i] = sv;
    rows[nt16 + base + i] = v;
    rows[2 * nt16 + base + tp] = v;
    rows[3 * nt16 + base + tp] = sv;
    if (i == 0) {
        tstart[t] = start;
        tinfo[t] = (lo << 8) | cnt;
    }
}

void free_plan(const athena_mp_graph *g)
{
    for (int32_t **p : {&g->bucket_perm, &g->btile_start, &g->btile_info, &g->btile_rows, &g->btile_off_dev}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    g->n_btiles = 0;
    g->bucket_off.clear();
    g->btile_off.clear();
    g->bucket_min = 0;
    g->bucket_max = -1;
}

// a plan the handle still holds for another (min, max): nothing may read it any more when it goes
int drop_old_plan(const athena_mp_graph *g)
{
    if (!g->bucket_perm) return 0;
    AMP_HIP(hipStreamSynchronize(amp::stream()));
    AMP_HIP(hipFree(g->bucket_perm));
    AMP_HIP(hipFree(g->btile_start));
    AMP_HIP(hipFree(g->btile_info));
    AMP_HIP(hipFree(g->btile_rows));
    AMP_HIP(hipFree(g->btile_off_dev));
    g->bucket_perm = g->btile_start = g->btile_info = g->btile_rows = g->btile_off_dev = nullptr;
    return 0;
}

// stable sort of the vertices by degree bucket (host); each bucket becomes one contiguous run of g->bucket_perm so the bucketed
// update is <= D dense contractions with row indirection
int duvenaud_buckets_host(const athena_mp_graph *g, int min_deg, int max_deg)
{
    const int nb = max_deg - min_deg + 1;
    const int32_t n = g->n_rows;
    std::vector<int64_t> off(nb + 1, 0);
    std::vector<int32_t> bucket(n);
    for (int32_t v = 0; v < n; ++v) {
        int d = std::max(min_deg, std::min(g->h_deg_row[v], max_deg)) - min_deg; // 0-based
        bucket[v] = d;
        off[d + 1]++;
    }
    for (int b = 0; b < nb; ++b) off[b + 1] += off[b];
    std::vector<int32_t> perm(n);
    {
        std::vector<int64_t> pos(off.begin(), off.end() - 1);
        for (int32_t v = 0; v < n; ++v) perm[pos[bucket[v]]++] = v;
    }
    std::vector<int32_t> tstart, tinfo, toff(nb + 1, 0);
    for (int b = 0; b < nb; ++b) {
        for (int64_t i = off[b]; i < off[b + 1]; i += 16) {
            tstart.push_back((int32_t)i);
            tinfo.push_back((b << 8) | (int32_t)std::min<int64_t>(16, off[b + 1] - i));
        }
        toff[b + 1] = (int32_t)tstart.size();
    }
    if (drop_old_plan(g)) return 1;
    const size_t nt = tstart.size();
    // four copies back to back, [16 nt] each:
    //   0  padding slots as ~(first vertex of the tile): the weight-gradient kernel zeroes their gradient rows
    //   1  padding slots as the first vertex itself: the row kernels load and store them as benign duplicates
    //   2  copy 1 transposed 4 x 4 inside each tile (slot 4 i + r at position 4 r + i): a lane that serves rows r, 4 + r,
    //      8 + r, 12 + r of a tile in four coalesced loads fetches its four ids with one 16-byte load
    //   3  copy 0 transposed the same way
    std::vector<int32_t> trows(64 * nt);
    for (size_t t = 0; t < nt; ++t) {
        const int cnt = tinfo[t] & 255;
        for (int i = 0; i < 16; ++i) {
            const int32_t v = i < cnt ? perm[tstart[t] + i] : perm[tstart[t]];
            const int32_t sv = i < cnt ? v : ~v;
            const int tp = 4 * (i & 3) + (i >> 2);
            trows[16 * t + i] = sv;
            trows[16 * (nt + t) + i] = v;
            trows[16 * (2 * nt + t) + tp] = v;
            trows[16 * (3 * nt + t) + tp] = sv;
        }
    }
    AMP_HIP(hipMalloc((void **)&g->btile_rows, sizeof(int32_t) * (nt ? 64 * nt : 1)));
    if (nt) AMP_HIP(hipMemcpy(g->btile_rows, trows.data(), sizeof(int32_t) * 64 * nt, hipMemcpyHostToDevice));
    AMP_HIP(hipMalloc((void **)&g->bucket_perm, sizeof(int32_t) * (n ? n : 1)));
    AMP_HIP(hipMalloc((void **)&g->btile_start, sizeof(int32_t) * (nt ? nt : 1)));
    AMP_HIP(hipMalloc((void **)&g->btile_info, sizeof(int32_t) * (nt ? nt : 1)));
    AMP_HIP(hipMalloc((void **)&g->btile_off_dev, sizeof(int32_t) * (nb + 1)));
    if (n) AMP_HIP(hipMemcpy(g->bucket_perm, perm.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
    if (nt) {
        AMP_HIP(hipMemcpy(g->btile_start, tstart.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice));
        AMP_HIP(hipMemcpy(g->btile_info, tinfo.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice));
    }
    AMP_HIP(hipMemcpy(g->btile_off_dev, toff.data(), sizeof(int32_t) * (nb + 1), hipMemcpyHostToDevice));
    g->n_btiles = (int32_t)nt;
    g->btile_off = toff;
    g->bucket_off = off;
    g->bucket_min = min_deg;
    g->bucket_max = max_deg;
    return 0;
}

// the launches of the device route; the five arrays are allocated, n > 0, nt > 0
int device_launches(const athena_mp_graph *g, int min_deg, int max_deg, int32_t nt)
{
    using namespace amp;
    const int nb = max_deg - min_deg + 1;
    const int32_t n = g->n_rows;
    hipStream_t st = stream();
    void *ws = nullptr;
    const size_t keys_bytes = (sizeof(uint32_t) * (size_t)n + 255) & ~(size_t)255;
    if (workspace(&ws, 2 * keys_bytes + radix::scratch_bytes(n), kWsPlan)) return 1;
    uint32_t *keys = (uint32_t *)ws, *keys_sorted = (uint32_t *)((char *)ws + keys_bytes);
    void *hist = (char *)ws + 2 * keys_bytes;
    const uint32_t *bin_start = (const uint32_t *)hist + (size_t)radix::kBins * radix::tiles_for(n);   // where sort_pairs leaves the bin starts
    hipLaunchKernelGGL(bucket_key_kernel, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, st, n, (const int32_t *)g->deg_row, min_deg,
                       max_deg, keys);
    AMP_LAUNCH_CHECK();
    if (int rc = radix::sort_pairs<uint32_t>(keys, nullptr, n, 8, keys_sorted, g->bucket_perm, nullptr, nullptr, hist, st)) return rc;
    hipLaunchKernelGGL(bucket_tile_off_kernel, dim3(1), dim3(radix::kThreads), 0, st, bin_start, n, nb, g->btile_off_dev);
    hipLaunchKernelGGL(bucket_tile_kernel, dim3((unsigned)(((int64_t)16 * nt + 255) / 256)), dim3(256), 0, st, nt, nb, bin_start,
                       (const int32_t *)g->btile_off_dev, n, (const int32_t *)g->bucket_perm, g->btile_start, g->btile_info,
                       g->btile_rows);
    AMP_LAUNCH_CHECK();
    return 0;
}

int duvenaud_buckets_device(const athena_mp_graph *g, int min_deg, int max_deg)
{
    const int nb = max_deg - min_deg + 1;
    const int32_t n = g->n_rows;
    // the host counts: sizes of the allocations and the host-side tables (the device derives its own copies of them)
    std::vector<int64_t> off(nb + 1, 0);
    for (int32_t v = 0; v < n; ++v) off[std::max(min_deg, std::min(g->h_deg_row[v], max_deg)) - min_deg + 1]++;
    std::vector<int32_t> toff(nb + 1, 0);
    for (int b = 0; b < nb; ++b) {
        toff[b + 1] = toff[b] + (int32_t)((off[b + 1] + 15) / 16);
        off[b + 1] += off[b];
    }
    const int32_t nt = toff[nb];
    if (drop_old_plan(g)) return 1;
    int rc = 0;
    auto alloc = [&](int32_t **p, size_t count) {
        if (rc == 0 && hipMalloc((void **)p, sizeof(int32_t) * (count ? count : 1)) != hipSuccess) {
            (void)hipGetLastError();
            amp::set_error("duvenaud_plan: no device memory for %zu plan entries", count);
            rc = 1;
        }
    };
    alloc(&g->btile_rows, (size_t)64 * nt);
    alloc(&g->bucket_perm, n);
    alloc(&g->btile_start, nt);
    alloc(&g->btile_info, nt);
    alloc(&g->btile_off_dev, (size_t)nb + 1);
    if (rc == 0) rc = device_launches(g, min_deg, max_deg, nt);
    if (rc) {   // no half-built plan stays behind (launches that did go out still write: let them finish first)
        (void)hipStreamSynchronize(amp::stream());
        free_plan(g);
        return rc;
    }
    g->n_btiles = nt;
    g->btile_off = toff;
    g->bucket_off = off;
    g->bucket_min = min_deg;
    g->bucket_max = max_deg;
    return 0;
}

} // namespace

namespace amp {
int duvenaud_buckets(const athena_mp_graph *g, int min_deg, int max_deg)
{
    if (g->bucket_perm && g->bucket_min == min_deg && g->bucket_max == max_deg) {
        g_reused++;
        return 0;
    }
    const int nb = max_deg - min_deg + 1;
    const char *mode = getenv("ATHENA_MP_BUCKET_PLAN");
    const bool pin_host = mode && strcmp(mode, "host") == 0, pin_device = mode && strcmp(mode, "device") == 0;
    AMP_REQUIRE(!mode || !*mode || pin_host || pin_device || strcmp(mode, "auto") == 0,
                "duvenaud_plan: ATHENA_MP_BUCKET_PLAN=%s is none of auto, host, device", mode);
    AMP_REQUIRE(!(pin_device && nb > kMaxDeviceBuckets),
                "duvenaud_plan: the device route sorts one 8-bit digit, at most %d buckets; (%d, %d) makes %d", kMaxDeviceBuckets,
                min_deg, max_deg, nb);
    // an empty handle has nothing to sort: the host route writes its (all zero) offset tables
    const bool on_device = !pin_host && g->n_rows > 0 && nb <= kMaxDeviceBuckets;
    if (on_device) {
        if (int rc = duvenaud_buckets_device(g, min_deg, max_deg)) return rc;
        g_device_builds++;
        return 0;
    }
    if (int rc = duvenaud_buckets_host(g, min_deg, max_deg)) {
        (void)hipStreamSynchronize(stream());
        free_plan(g);
        return rc;
    }
    g_host_builds++;
    return 0;
}
} // namespace amp

extern "C" {

int athena_mp_duvenaud_plan(const athena_mp_graph *g, int32_t min_deg, int32_t max_deg)
{
    AMP_REQUIRE(g != nullptr && max_deg >= min_deg, "duvenaud_plan: bad arguments");
    AMP_REQUIRE((int64_t)max_deg - min_deg < ((int64_t)1 << 22), "duvenaud_plan: (%d, %d) makes more than 2^22 buckets", min_deg, max_deg);
    AMP_REQUIRE(g->h_deg_row.size() == (size_t)g->n_rows, "duvenaud_plan: the handle keeps no host copy of its row degrees");
    return amp::duvenaud_buckets(g, min_deg, max_deg);
}

int athena_mp_duvenaud_plan_export(const athena_mp_graph *g, int32_t which, void *host_dst, int64_t capacity, int64_t *count)
{
    AMP_REQUIRE(g && count, "duvenaud_plan_export: null argument");
    AMP_REQUIRE(g->bucket_perm != nullptr, "duvenaud_plan_export: the handle has no plan (athena_mp_duvenaud_plan builds one)");
    const int64_t nb1 = (int64_t)g->btile_off.size(), nt = g->n_btiles;
    const void *dev = nullptr, *host = nullptr;
    int64_t n = 0;
    size_t width = 4;
    switch (which) {
    case 0: dev = g->bucket_perm; n = g->n_rows; break;
    case 1: dev = g->btile_start; n = nt; break;
    case 2: dev = g->btile_info; n = nt; break;
    case 3: dev = g->btile_rows; n = 64 * nt; break;
    case 4: dev = g->btile_off_dev; n = nb1; break;
    case 5: host = g->bucket_off.data(); n = (int64_t)g->bucket_off.size(); width = 8; break;
    case 6: host = g->btile_off.data(); n = nb1; break;
    default: AMP_REQUIRE(false, "duvenaud_plan_export: unknown array id %d", which);
    }
    *count = n;
    if (host_dst == nullptr) return 0;   // size query
    AMP_REQUIRE(capacity >= n, "duvenaud_plan_export: buffer holds %lld elements, array has %lld", (long long)capacity, (long long)n);
    if (n > 0 && host) memcpy(host_dst, host, width * (size_t)n);
    if (n > 0 && dev) {
        AMP_HIP(hipMemcpyAsync(host_dst, dev, width * (size_t)n, hipMemcpyDeviceToHost, amp::stream()));
        AMP_HIP(hipStreamSynchronize(amp::stream()));
    }
    return 0;
}

int athena_mp_duvenaud_plan_stats(int64_t *host_builds, int64_t *device_builds, int64_t *reused)
{
    if (host_builds) *host_builds = g_host_builds.load();
    if (device_builds) *device_builds = g_device_builds.load();
    if (reused) *reused = g_reused.load();
    return 0;
}

} // extern "C"
