// Shared internals of libathena_mp (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <atomic>
#include <vector>

#include "../../include/athena_mp.h"
#include "pieces.h"

namespace amp {

// ---- error plumbing: C side never aborts, it returns a code + message ---------------------
void set_error(const char *fmt, ...);
hipStream_t stream();
// a second, library-owned stream of the current device and six events (pipelines inside one API call); swap_stream
// redirects the launchers of this library (they all launch on stream()) for the duration of such a pipeline
void swap_stream(hipStream_t s);
int aux_stream(hipStream_t *s, hipEvent_t **events);

#define AMP_HIP(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            amp::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,  \
                           __LINE__);                                                        \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

#define AMP_REQUIRE(cond, ...)          \
    do {                                \
        if (!(cond)) {                  \
            amp::set_error(__VA_ARGS__); \
            return 2;                   \
        }                               \
    } while (0)

#define AMP_LAUNCH_CHECK() AMP_HIP(hipGetLastError())

// The alignment contract (include/athena_mp.h): a caller's device pointer needs only the alignment of its element type.  A route
// whose kernel goes through 16-byte accesses on a caller's array (v4f casts, b128 buffer loads / stores, nontemporal v4f stores)
// carries this term in its host-side predicate; a call that fails it takes the entry's generic route.  Null (an absent
// operand) constrains nothing.
template <typename... P> inline bool aligned16(const P *...p) { return ((... | (uintptr_t)p) & 15) == 0; }

// workspace owned by the library (grown on demand, never shrunk; stream-ordered reuse); per device
int workspace(void **ptr, size_t bytes, int slot = 0);
// hand a slot's memory back to the device (after the stream drained); the next workspace() call of that slot allocates again
int workspace_release(int slot);

// Everything the library keeps on a device belongs to the device athena_mp_init selected: the workspaces above, the
// named buffers below (ticket ring, identity row pointer, zero bias ...) and the "attribute set" flags of kernels with
// more than 64 KB of LDS.  athena_mp_finalize releases the buffers of every device; a second athena_mp_init for
// another device gets buffers of its own.
constexpr int kMaxDevices = 32;
int device();        // the device athena_mp_init selected (0 before the first call)
int num_cus();       // its compute units (256 on MI355X)
// a device buffer of at least `bytes` under `name` on the current device.  *fresh is set when it was (re)allocated --
// its contents are then undefined (or zero with zero_fill) and the caller initialises them.
int named_buffer(const char *name, size_t bytes, bool zero_fill, void **ptr, bool *fresh = nullptr);
struct PerDeviceFlag {
    bool done[kMaxDevices] = {};
    bool &get() { return done[device()]; }
};

// device scratch of one call: every array handed out is returned to the device on every exit path
struct Scratch {
    std::vector<void *> ptrs;
    template <typename T> int get(T **p, size_t count)
    {
        AMP_HIP(hipMalloc((void **)p, sizeof(T) * (count ? count : 1)));
        ptrs.push_back(*p);
        return 0;
    }
    // every array of the list out of one allocation (pieces.h)
    int carve(Pieces &pc)
    {
        char *base = nullptr;
        if (get(&base, pc.bytes())) return 1;
        pc.place(base);
        return 0;
    }
    // host staging of the *_host entries: an input array up (null or empty: allocated, not copied), an output array home
    template <typename T> int upload(T **dev, const T *host, size_t count, hipStream_t st)
    {
        if (get(dev, count)) return 1;
        if (host && count > 0) AMP_HIP(hipMemcpyAsync(*dev, host, sizeof(T) * count, hipMemcpyHostToDevice, st));
        return 0;
    }
    template <typename T> static int download(T *host, const T *dev, size_t count, hipStream_t st)
    {
        if (host && dev && count > 0) AMP_HIP(hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, st));
        return 0;
    }
    ~Scratch()
    {
        for (void *p : ptrs) (void)hipFree(p);
    }
};

} // namespace amp

// Rows longer than kLongRow entries (hubs of heavy-tailed graphs) are cut into segments of kLongRow
// entries that independent lane groups sum in parallel; the segment sums are then added in segment
// order (deterministic).  Shorter rows keep the strictly sequential CSR-order sum.
constexpr int kLongRow = 512;
struct LongPlan {
    int32_t n_tasks = 0, n_long = 0;
    int32_t *task_beg = nullptr, *task_end = nullptr; // [n_tasks] entry ranges
    int32_t *row_id = nullptr;                        // [n_long] the long rows
    int32_t *row_task0 = nullptr;                     // [n_long+1] first task of each long row
};

// rows of a CSR ordered by length, longest first, built on first use by the GNO kernels of gno64.hip: the rows of a tile then
// have (nearly) equal entry counts, so no wave waits at the tile barrier for a longer row
struct LenOrder {
    int32_t *perm = nullptr;      // [rows] device
    int32_t n_long = 0, n_mid = 0;   // rows with more than 32 / more than 16 entries (n_long included): the first slots of perm
};

// ---- graph handle: everything the kernels need, resident in HBM --------------------------------
inline uint64_t next_graph_serial()
{
    static std::atomic<uint64_t> n{0};
    return ++n;
}
struct athena_mp_graph {
    int32_t n_rows = 0, n_cols = 0, n_edge_cols = 0;
    int64_t nnz = 0;
    int32_t max_row_len = 0, max_col_len = 0;
    // max |column - row| over the entries of a square graph (INT32_MAX: not known): a batch of small graphs is block-diagonal, every
    // neighbour of a vertex sits within a few rows of it, and the gathers stage a block's rows in LDS instead of chasing them (agg.hip)
    int32_t band = INT32_MAX;
    // unique per handle for the life of the process (a freed handle's ADDRESS can come back; its serial never does)
    uint64_t serial = next_graph_serial();
    // handle cache (athena_mp_graph_acquire / _release): users of a cached handle, -1 = not cached
    int32_t cache_refs = -1;
    bool cache_linked = false;   // still findable by key (false after athena_mp_graph_evict / athena_mp_finalize)
    uint64_t cache_key = 0;
    uint64_t cache_tick = 0;
    int cache_device = 0;
    // forward CSR, 0-based
    int32_t *rowptr = nullptr;  // [n_rows+1]
    int32_t *col = nullptr;     // [nnz]  neighbour u
    int32_t *eid = nullptr;     // [nnz]  edge-feature column, -1 = none
    float *coef = nullptr;      // [nnz]  (deg_v*deg_u)^-1/2, the Kipf coefficient of each entry
    // transposed CSR (pull form of every scatter): row u lists the (v,w) with col[w]==u, v ascending
    int32_t *t_rowptr = nullptr; // [n_cols+1]
    int32_t *t_src = nullptr;    // [nnz] source row v
    int32_t *t_eid = nullptr;    // [nnz]
    float *t_coef = nullptr;     // [nnz]
    // edge-column index: column e lists the entries that carry it, in w order
    int32_t *e_rowptr = nullptr; // [n_edge_cols+1]
    int32_t *e_row = nullptr;    // [n_with_edge] row v of the entry
    int32_t *e_col = nullptr;    // [n_with_edge] CSR entry index w of the entry
    int32_t *deg_row = nullptr;  // [n_rows]
    int32_t *deg_col = nullptr;  // [n_cols]
    int64_t n_with_edge = 0;
    LongPlan lp_fwd, lp_bwd;        // hub rows of the forward / transposed CSR
    std::vector<int32_t> h_deg_row; // host copy (bucket planning)
    // Duvenaud degree buckets, built on first use for a (min_deg, max_deg) pair: vertices sorted by
    // bucket (stable), so each bucket is one contiguous run of a row-index array
    mutable int bucket_min = 0, bucket_max = -1;
    mutable int32_t *bucket_perm = nullptr;      // [n_rows] device
    mutable std::vector<int64_t> bucket_off;     // [n_buckets+1] host
    mutable LenOrder len_fwd, len_bwd;           // of the forward CSR [n_rows] / the transposed CSR [n_cols]
    // forward entry of every transposed entry (-1: no edge column), built on first use by athena_mp_gno_aggregate_bwd
    mutable int32_t *t_entry = nullptr;          // [nnz] device
    // the same runs cut into 16-vertex tiles (one MFMA column block each), bucket-major
    mutable int32_t n_btiles = 0;
    mutable int32_t *btile_start = nullptr;      // [n_btiles] device: first index into bucket_perm
    mutable int32_t *btile_rows = nullptr;       // [4][16*n_btiles] device: vertex of each tile slot (copies: see duvenaud_buckets); in copy 0 padding slots hold
                                                 //   ~(first vertex of the tile) (negative: load from it, never store)
    mutable int32_t *btile_info = nullptr;       // [n_btiles] device: bucket << 8 | vertices in the tile (1..16)
    mutable int32_t *btile_off_dev = nullptr;    // [n_buckets+1] device: first tile of each bucket
    mutable std::vector<int32_t> btile_off;      // [n_buckets+1] host
};

namespace amp {
// device-side construction of the handle arrays (graph_build.hip); -1 = use the host builder
int graph_build_device(athena_mp_graph *g, const int32_t *adj_ja, const std::vector<int32_t> &rowptr,
                       const std::vector<int32_t> &degr, const std::vector<int32_t> &degc,
                       std::vector<int32_t> *t_rowptr_host, const int32_t *adj_ja_dev = nullptr);
int csr_from_edges_core(int32_t n_vertices, int64_t n_pairs, const int32_t *index_list, int32_t add_self_loops,
                        int32_t *adj_ia_out, int32_t *adj_ja_out, int64_t capacity, int64_t *nnz_out,
                        int32_t **keep_ja_dev, bool list_on_device = false);
// a pair list between two point sets, strictly ascending in (i, j), in HBM -> its directed CSR and degrees (bipartite_graph.hip)
int bipartite_csr_from_pairs(const char *who, int32_t n_rows, int32_t n_cols, int64_t n_pairs, const int32_t *pairs_dev,
                             int32_t *adj_ia_out, int32_t *adj_ja_out, int64_t capacity, int32_t **ja_dev, std::vector<int32_t> *row_deg,
                             std::vector<int32_t> *col_deg);
// athena_mp_graph_create for a CSR whose entries (column, edge id) [2, nnz] lie in HBM; adj_ia and the degrees on the host (capi.hip)
int graph_create_dev(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *adj_ia, const int32_t *adj_ja_dev, int32_t n_edge_cols,
                     const int32_t *row_deg, const int32_t *col_deg, athena_mp_graph **out);
// The end of a point-cloud *_graph_host entry (radius_graph.hip, knn_graph.hip) once the pair count E is known: the sizes out,
// the size query's return, the capacity checks, then pairs(&d_pairs, &d_coords) -- the E pairs [2, E] and coords [E, dim] on the
// device, built or already there -- the coords home and the CSR through csr_from_edges_core.
template <typename Pairs>
int graph_host_tail(const char *who, int32_t n, int32_t dim, int64_t E, int32_t add_self_loops, int32_t *adj_ia_out, int32_t *adj_ja_out,
                    int64_t capacity, int64_t *nnz_out, float *coords_out, int64_t coords_capacity, int64_t *n_pairs_out, hipStream_t st,
                    Pairs pairs)
{
    // no self pair and no duplicate pair: every pair is two entries, every vertex gets its loop when asked
    const int64_t nnz = 2 * E + (add_self_loops ? n : 0);
    *n_pairs_out = E;
    *nnz_out = nnz;
    if (adj_ja_out == nullptr) return 0;                          // size query
    AMP_REQUIRE(adj_ia_out != nullptr && (coords_out != nullptr || E == 0), "%s: null output array", who);
    AMP_REQUIRE(capacity >= nnz, "%s: adj_ja buffer holds %lld entries, the graph has %lld", who, (long long)capacity, (long long)nnz);
    AMP_REQUIRE(coords_capacity >= E, "%s: coords buffer holds %lld pairs, the graph has %lld", who, (long long)coords_capacity,
                (long long)E);
    int32_t *d_pairs = nullptr;
    float *d_coords = nullptr;
    if (int rc = pairs(&d_pairs, &d_coords)) return rc;
    if (E > 0) AMP_HIP(hipMemcpyAsync(coords_out, d_coords, sizeof(float) * (size_t)E * dim, hipMemcpyDeviceToHost, st));
    int64_t nnz_built = 0;
    if (int rc = amp::csr_from_edges_core(n, E, d_pairs, add_self_loops, adj_ia_out, adj_ja_out, capacity, &nnz_built, nullptr, true))
        return rc;
    AMP_HIP(hipStreamSynchronize(st));
    *nnz_out = nnz_built;
    return 0;
}
// argument checks of the geometry gradients (geometry_grad.hip), shared with their *_host entries: 0, or 2 with the message set
int points_grad_check(const athena_mp_graph *g, int32_t dim);
int point_sets_grad_check(const athena_mp_graph *g, int32_t dim, bool want_queries, bool want_sources);
int periodic_grad_check(const athena_mp_graph *g, int32_t B, int32_t n, const int32_t *offsets, const int64_t *edge_offsets,
                        float cutoff_max, bool has_dfeature, int32_t fe_cols, bool has_dvec);
// the handle carries one entry per edge column, as athena_mp_graph_create_bipartite_dev builds it (interp.hip): what the
// interpolation entries, the edge forms of pooling and the edge gather need of it
int edge_form_check(const char *who, const athena_mp_graph *g);
// argument checks of the interpolation entries (interp.hip), shared with their *_host forms: edge_form_check, then dim, F, eps
// (null where the entry takes none)
int interp_check(const char *who, const athena_mp_graph *g, const int32_t *dim, const int32_t *F, const float *eps);
// argument checks of the max-pooling entries (pool.hip), shared with their *_host forms; the edge forms add edge_form_check
int pool_check(const char *who, const athena_mp_graph *g, int32_t F, bool edge_form);
// argument checks of the attention entries (attention.hip), shared with their *_host forms: edge_form_check, then H, F and F % H
int attn_check(const char *who, const athena_mp_graph *g, int32_t F, int32_t H);
// argument checks of the edge-gather entries (edge_gather.hip), shared with their *_host forms: edge_form_check, then the widths
int edge_gather_check(const char *who, const athena_mp_graph *g, int32_t Fs, int32_t Fq, int32_t dim, int32_t relative, int32_t ld);
void graph_cache_clear(); // idle and live handles of athena_mp_graph_acquire (capi.hip)
void host_pool_release();   // staging buffers of the *_host entry points (host.hip)
uint64_t content_hash(const void *p, size_t bytes);   // every byte of a host array (capi.hip)
bool kipf_gather_is_banded(const athena_mp_graph *g, bool transposed, int F, const float *x, const float *y);   // agg.hip
// banded_fused.hip: the Kipf layer step on a banded graph in one launch at 64 -> 64 (0 done, -1 not its shape, > 0 error)
int banded_agg_gemm64(const athena_mp_graph *g, bool transposed, const float *coef, const float *x, const float *W, int b_nk,
                      const float *bias, int act, float *P, float *Z);
int agg_blocks_cap();
void set_agg_blocks_cap(int n);
// shared launchers (defined in agg.hip / gemm.hip)
int gather_agg(const int32_t *rowptr, const int32_t *idx, const float *coef, const float *x, int64_t ldx,
               float *y, int64_t ldy, int32_t n_rows, int32_t F, const LongPlan *lp = nullptr, int act = 0);
int gather_agg_dual(const int32_t *rowptr, const int32_t *idx, const float *coef, const float *x, float *y, float *y2,
                    int32_t n_rows, int32_t F, const LongPlan *lp);
// Z[M,N] = act(A[M,K] . B + bias); b_nk: B stored [N][K] instead of [K][N]
int gemm_dispatch(const float *A, const float *B, int b_nk, const float *bias, int act, float *Z, int64_t M,
                  int K, int N);
// dWt[Fi,Fo] (+)= sum_v P[v,:]^T dZ[v,:]
int gemm_dw_dispatch(int64_t N, int Fi, int Fo, const float *P, const float *dZ, float *dW, bool accumulate);
int slab_reduce(const float *slabs, int n_slabs, int n, float *out, bool accumulate);
// n_segs independent ranges [first[i], first[i]+count[i]) of the same slab array -> out + i*out_stride (count 0 => zeros)
int slab_reduce_segs(const float *slabs, int n, int n_segs, const int *first, const int *count, float *out,
                     int64_t out_stride, bool accumulate);

// reverse pass of a square Kipf step with dW folded in (fused_dw.hip)
bool fused_dw_shape(int Fi, int Fo);
int fused_dw_dispatch(const int32_t *t_rowptr, const int32_t *t_src, const float *t_coef, const float *dZ, const float *W,
                      const float *X, int exact, float *dX, float *dW, int64_t n_cols);

// shape-generic tiled MFMA contraction (gemm_tiled.hip)
struct TiledArgs {
    const float *A = nullptr; int64_t lda = 0; const int32_t *a_idx = nullptr; float a_div = 1.0f;
    const float *B = nullptr; int64_t ldb = 0; int b_nk = 0;
    const float *bias = nullptr; int act = 0; float c_div = 1.0f;
    float *C = nullptr; int64_t ldc = 0; const int32_t *c_idx = nullptr;
    int64_t M = 0; int N = 0; int K = 0;
};
int gemm_tiled(const TiledArgs &p);
int gemm_atb_tiled(const float *A, int64_t lda, const float *B, int64_t ldb, const int32_t *idx, float div, int64_t M,
                   int KI, int NO, float *C, bool accumulate);
// bucket-sorted vertex permutation of a graph for Duvenaud's degree buckets (duvenaud.hip)
int duvenaud_buckets(const athena_mp_graph *g, int min_deg, int max_deg);
// [a_x | a_e] -> a packed in the library's workspace (duvenaud.hip): split a for shapes outside the split kernels
int duv_pack_a(const athena_mp_graph *g, int32_t Fv, int32_t Fe, const float *a_x, const float *a_e, const float **packed);
// register-resident-weight MFMA kernels of the bucketed update (duv_mfma.hip); return -1 when the shape
// is outside what they cover (caller falls back to the tiled route)
int duv_mfma_fwd(const athena_mp_graph *g, int Fi, int Fo, const float *a, const float *w, int act, float *c);
int duv_mfma_bwd_a(const athena_mp_graph *g, int Fi, int Fo, const float *grad, const float *w, float *da);
int duv_mfma_bwd_w(const athena_mp_graph *g, int Fi, int Fo, const float *grad, const float *a, float *dw);
int duv_mfma_fwd_readout(const athena_mp_graph *g, int Fi, int Fo, const float *a, const float *w, int act, float *z,
                         const float *R, int O, float *p, const float *a_tail = nullptr);
int duv_mfma_bwd(const athena_mp_graph *g, int Fi, int Fo, const float *grad, const float *a, const float *w, float *da, float *dw,
                 float *da_tail = nullptr);
// readout reverse + update reverse in one launch (duv_mfma.hip, duv_bwd_ro_kernel); -1: shape outside it
int duv_mfma_bwd_readout(const athena_mp_graph *g, int Fi, int Fo, int O, int act, const float *a, const float *w, const float *z,
                         const float *dz_next, const float *p, const int32_t *tgid, const float *gout, const float *R, float *da,
                         float *da_tail, float *dw, float *dr_slabs, int *n_slabs, bool accumulate_tail,
                         const float *a_tail = nullptr);
// Graph neural operator at H = F_in = F_out = 64 (gno64.hip): the kernels that keep S / T / G on chip.  gno64_shape is the shape
// test with the bound on d as its argument (4: gno_fused_kernel, 3: everything that builds buffer descriptors).
bool gno64_shape(int H, int Fi, int Fo, int d, int d_max);
// bytes of S the forward pass keeps for the reverse pass; 0: this shape or size does not keep S
int64_t gno64_saved_bytes(const athena_mp_graph *g, int d, int H, int Fi, int Fo);
// *ok: the reverse pass runs as ONE call (gno_dh_pc_kernel<.., PX>: dx and dtheta from one G)
int gno64_one_call_reverse(const athena_mp_graph *g, int d, int H, int Fi, int Fo, bool want_dx, bool *ok);
// out[r,:] = S_r . Vaug over the n_rows rows of one CSR (gno_pc_kernel; gno_fused_kernel at d = 4 and beyond 4 GB); save: keeps S
int launch_gno_fused(const int32_t *rowptr, const int32_t *idx, const int32_t *eidx, const float *y, const float *coords,
                     const float *theta, int d, const float *Vaug, int n_rows, LenOrder *order, float *out, int y_rows,
                     int n_edge_cols, int64_t nnz, float *save = nullptr);
// dVaug = S^T g (gno_stg_kernel), S rebuilt or streamed from save; -1: beyond what a buffer descriptor addresses
int launch_gno_stg(const athena_mp_graph *g, const float *x, const float *coords, const float *theta, int d, const float *grad,
                   float *dV, const float *save = nullptr);
// dU, db_u -> dtheta, the masked dh per entry -> ghbuf, the feature gradient's per-entry partials -> px (each may be null)
int gno64_mlp_backward(const athena_mp_graph *g, int d, const float *theta, const float *coords, const float *x, const float *grad,
                       float *dtheta, float *ghbuf, float *px, size_t px_half, const float *cvec);
int gno64_t_entry(const athena_mp_graph *g);   // g->t_entry, built once; -1: the device cannot hold it
int gno64_px_gather(const athena_mp_graph *g, const float *px, float *dx, hipStream_t s);   // dx from the partials, on stream s
} // namespace amp
