/*
 * athena_mp.h -- C ABI of the MI355X (gfx950) message-passing engine for athena.
 *
 * This is the drop-in boundary.  The reference (nedtaylor/athena
 * v2.1.1) is pure Fortran and has no FFI for this path, so each entry point below
 * names the reference procedure whose arithmetic it replaces (paths relative to
 * src/athena/ of the reference).  The Fortran side binds them through
 * ISO_C_BINDING (athena_amd/fortran/athena_mp_c.f90; INTEGRATION.md shows the
 * layer-side stub).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; the message is
 *     available from athena_mp_last_error() (the Fortran wrapper turns it into
 *     coreutils' stop_program(msg), cf. athena_kipf_msgpass_layer.f90:271-274).
 *   - "dev" pointers are device (HBM) pointers; "host" pointers are host memory.
 *     The *_host variants stage through HBM for callers that only hold
 *     array_type%val (phase-1 plumbing); they are never timed.
 *   - feature tensors are athena's val(F, N) column-major == row-major [N][F]
 *     fp32: one vertex row contiguous.  Dense weights are params(t)%val(:,1):
 *     W(Fo,Fi) column-major flat == row-major Wt[Fi][Fo].
 *   - all kernels are enqueued on the stream set with athena_mp_set_stream
 *     (default: the null stream) and return without synchronising.
 *   - not thread-safe by design (the reference's layers are stateful and
 *     single-threaded, SURVEY.md 8b "Threading").
 *   - ALIGNMENT: every float * / int32_t * device argument needs only the natural alignment of its element type (4 bytes): a row
 *     slice x(1, v0) of a larger array, an array carved out of one allocation at an odd element offset, are valid operands.
 *     The fast routes are taken when the operands are 16-byte aligned (what athena_mp_malloc and every allocator return);
 *     other calls take the entry's generic route and compute the same thing.  Two entries refuse instead, with a message
 *     that says so, and say so where they are declared: athena_mp_device_copy (16-byte elements) and
 *     athena_mp_gno_aggregate_fwd_save (S has one producer, which moves x, m and S 16 bytes at a time;
 *     athena_mp_gno_aggregate_fwd takes any alignment).  An s_save_dev that is not 16-byte aligned is never read: the
 *     reverse entries that take one rebuild S then.
 *   - ONE stream at a time per device: scratch workspaces (reduction slabs, the GNO partials, packed halo rows) belong
 *     to the device, not to a stream, and are ordered by the stream the calls are enqueued on.  Switching streams with
 *     athena_mp_set_stream is fine once the work enqueued so far on the old stream is ordered before the new stream's
 *     (an event wait or a synchronize); two streams issuing calls for the same device side by side would share those
 *     workspaces.  The second, library-owned stream some calls use inside (athena_mp_gno_aggregate_bwd, the tiled
 *     athena_mp_gno_aggregate_bwd_theta) is forked from and joined to the caller's stream within the call; the
 *     communication stream is forked by the _start calls and joined by their _finish (athena_mp_halo_*, _allreduce_*).
 */
#ifndef ATHENA_MP_H
#define ATHENA_MP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct athena_mp_graph athena_mp_graph; /* opaque: device CSR + transposed CSR + coefficients */

/* activation kinds understood by the fused epilogues and athena_mp_activation_* */
enum {
    ATHENA_MP_ACT_NONE = 0,    /* athena_activation_none.f90    */
    ATHENA_MP_ACT_RELU = 1,    /* athena_activation_relu.f90    */
    ATHENA_MP_ACT_SIGMOID = 2, /* athena_activation_sigmoid.f90 */
    ATHENA_MP_ACT_TANH = 3     /* athena_activation_tanh.f90    */
};

/* ---- runtime ------------------------------------------------------------ */
int athena_mp_init(int device);            /* hipSetDevice + capability check (gfx950) */
/* the device athena_mp_init selected, -1 before the first successful call (after athena_mp_finalize the selection stands): lets a
 * layer that lives inside a host program it does not own initialise the library on first use WITHOUT overriding the host's choice --
 * nothing in the reference corresponds to it (athena has no device); the drop-in types' set_graph calls it (athena_hip_msgpass_layers.f90) */
int athena_mp_initialized(void);
int athena_mp_finalize(void);
const char *athena_mp_last_error(void);
int athena_mp_set_stream(void *hip_stream); /* hipStream_t; NULL = default stream */
int athena_mp_synchronize(void);
int athena_mp_version(void);

/* device memory helpers so a Fortran caller can keep tensors resident */
int athena_mp_malloc(void **dev_ptr, uint64_t bytes);
int athena_mp_free(void *dev_ptr);
int athena_mp_memcpy_h2d(void *dev_dst, const void *host_src, uint64_t bytes);
int athena_mp_memcpy_d2h(void *host_dst, const void *dev_src, uint64_t bytes);
int athena_mp_memset_zero(void *dev_ptr, uint64_t bytes);

/* ---- graph handle ------------------------------------------------------- *
 * Replaces the per-call CSR copies of set_graph_msgpass
 * (athena_msgpass_layer_sub.f90:144-174) and `c%indices = adj_ia; c%adj_ja =
 * adj_ja` (athena_diffstruc_extd_sub_kipf.f90:48-49): built once, reused.
 *   adj_ia  [n_rows+1]  1-based row pointers            (host)
 *   adj_ja  [2, nnz]    column-major; (1,w) neighbour 1-based in [1,n_cols],
 *                       (2,w) edge-feature column 1-based, 0 = none (host)
 *   row_deg / col_deg   optional global degrees for a row partition with halo
 *                       columns (NULL: degree = CSR row length, needs n_rows ==
 *                       n_cols -- exactly the reference's coefficient,
 *                       athena_diffstruc_extd_sub_kipf.f90:39-42)
 */
int athena_mp_graph_create(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *adj_ia,
                           const int32_t *adj_ja, int32_t n_edge_cols, const int32_t *row_deg,
                           const int32_t *col_deg, athena_mp_graph **out);
/* Edge list -> athena's CSR on the device (what graphstruc's generate_adjacency [+ add_self_loops] produces, in the
 * conventions of SURVEY.md Appendix C): index_list [2, n_pairs] column-major, 1-based vertex pairs, edge id = column.
 * Each pair gives (u -> v, id) and (v -> u, id); a self pair one entry; add_self_loops adds (v, v, id 0) where missing;
 * inside a row entries are ordered by edge id, id-less self loops first.  adj_ia_out [n_vertices+1] (1-based),
 * adj_ja_out [2, nnz] column-major; pass adj_ja_out = NULL to query *nnz_out first. */
int athena_mp_csr_from_edges(int32_t n_vertices, int64_t n_pairs, const int32_t *index_list_host,
                             int32_t add_self_loops, int32_t *adj_ia_out_host, int32_t *adj_ja_out_host,
                             int64_t capacity, int64_t *nnz_out);
/* Copies one array of the handle back to the host (4-byte elements; 0-based indices): which =
 * 0 rowptr, 1 col, 2 eid, 3 coef, 4 t_rowptr, 5 t_src, 6 t_eid, 7 t_coef (transposed CSR: the pull form of the
 * reference's scatters), 8 e_rowptr, 9 e_row, 10 e_entry (edge-column index), 11 deg_row, 12 deg_col.
 * host_dst NULL: size query only.  *count = number of elements. */
/* edge list -> CSR -> handle with the entries staying in HBM in between (generate_adjacency [+ add_self_loops]
 * followed by set_graph in one call).  adj_ia_out (n_vertices + 1, host) is always filled; adj_ja_out
 * (2 x capacity, host, column-major) only when non-null.  with_edge_ids = 0 builds a handle without edge-feature
 * columns (Kipf); 1 keeps the pair index as the edge id of both directed entries (Duvenaud / GNO). */
int athena_mp_graph_create_from_edges(int32_t n_vertices, int64_t n_pairs, const int32_t *index_list_host,
                                      int32_t add_self_loops, int32_t with_edge_ids, int32_t *adj_ia_out,
                                      int32_t *adj_ja_out, int64_t capacity, int64_t *nnz_out,
                                      athena_mp_graph **out);
/* athena_mp_graph_create_from_edges for an index list that is ALREADY IN HBM (the pair list athena_mp_radius_pairs wrote):
 * same arguments otherwise, same results, nothing uploaded. */
int athena_mp_graph_create_from_edges_dev(int32_t n_vertices, int64_t n_pairs, const int32_t *index_list_dev,
                                          int32_t add_self_loops, int32_t with_edge_ids, int32_t *adj_ia_out,
                                          int32_t *adj_ja_out, int64_t capacity, int64_t *nnz_out,
                                          athena_mp_graph **out);
/* Points -> radius graph on the device (radius_graph.hip): the pair list and the edge geometry graph_nop_layer_type works on
 * (its inputs, athena_graph_nop_layer.f90:743-758).  graphstruc has no such call; the step in front of the two builders above.
 *   points [n, dim] fp32 row-major, dim in 1..3; radius fp32 > 0.
 *   delta = p_i - p_j per component in fp32, s = ((d0*d0) + d1*d1) + d2*d2, every multiply and add rounded to fp32 on its own;
 *   i < j are joined iff s <= fl(radius * radius).  No self pairs; two points at the same place are joined.
 *   Pairs are numbered in lexicographic order of (i, j), i < j: pairs [2, capacity] column-major, 1-based (the index_list
 *   of the builders, column = edge id); coords [capacity, dim], coords[e, :] = p_i - p_j (smaller index minus larger).
 * Everything stays in HBM.  pairs_dev == NULL && coords_dev == NULL: size query (the count pass only), as
 * athena_mp_csr_from_edges.  Either of the two may be NULL alone.  Refused with a message: dim outside 1..3, a radius that is
 * not finite or <= 0, a non-finite coordinate (the first such point is named), 2 * pairs + n >= 2^31 (found by the count
 * pass, before anything of that size is allocated), capacity < pairs.  Two builds of the same points are byte-identical. */
int athena_mp_radius_pairs(int32_t n, int32_t dim, const float *points_dev, float radius, int32_t *pairs_dev,
                           float *coords_dev, int64_t capacity, int64_t *n_pairs_out);
/* The same with every array on the host, for callers that hold Fortran arrays: points -> adj_ia [n+1], adj_ja [2, capacity]
 * column-major (what generate_adjacency [+ add_self_loops] makes of the pair list: the neighbours of every row ascend) and
 * coords [coords_capacity, dim].  adj_ja_out == NULL: size query for both counts (*nnz_out, *n_pairs_out). */
int athena_mp_radius_graph_host(int32_t n, int32_t dim, const float *points_host, float radius, int32_t add_self_loops,
                                int32_t *adj_ia_out, int32_t *adj_ja_out, int64_t capacity, int64_t *nnz_out,
                                float *coords_out, int64_t coords_capacity, int64_t *n_pairs_out);
/* A batch of point clouds -> ONE block-diagonal radius graph on the device (radius_graph.hip): what a graph-neural-operator
 * dataset (many meshes, samples of a PDE, molecules without a cell) needs in front of athena_mp_graph_create_from_edges_dev,
 * athena_mp_batch_plan_create and athena_mp_edge_grad_to_points.
 *   points [n, dim] fp32 row-major on the device, dim in 1..3; offsets [n_clouds + 1] int32 on the HOST, 0-based,
 *   0 = offsets[0] <= ... <= offsets[n_clouds] = n: cloud b is the rows offsets[b] .. offsets[b+1]-1, empty clouds are allowed
 *   anywhere; one radius fp32 > 0 for all clouds.
 *   Which pairs join: points i < j are joined iff they lie in the same cloud and s <= fl(radius * radius), with
 *   delta = p_i - p_j per component in fp32 and s = ((d0*d0) + d1*d1) + d2*d2, every multiply and add rounded to fp32 on its own:
 *   the predicate of athena_mp_radius_pairs, unchanged.  No self pairs; coincident points of one cloud are joined.
 *   Numbering: pairs are numbered in lexicographic order of the global (i, j); the 1-based rank is the edge id.  pairs
 *   [2, capacity] column-major, 1-based global indices; coords [capacity, dim], coords[e, :] = p_i - p_j.
 *   edge_offsets [n_clouds + 1] int64 on the HOST (may be NULL): edge_offsets[b] = the number of pairs whose i is below
 *   offsets[b]; edge_offsets[n_clouds] = the number of pairs.
 * Equivalently: the concatenation, in cloud order, of what athena_mp_radius_pairs returns for each slice
 * points[offsets[b] : offsets[b+1]], with offsets[b] added to both indices.
 * pairs_dev == NULL && coords_dev == NULL: size query (the count pass only; edge_offsets is still filled).  Either of the two
 * may be NULL alone.  Refused with a message: dim outside 1..3; a radius that is not finite or <= 0 or whose square is not finite
 * in fp32; n_clouds < 0; offsets[0] != 0; a descending offset (the cloud is named, 1-based); offsets[n_clouds] != n; a non-finite
 * coordinate (cloud, component and point of the first one are named, 1-based); 2 * pairs + n >= 2^31 (found by the count pass,
 * before anything of that size is allocated); capacity < pairs.  The library stays usable after a refusal.  Two builds of the
 * same input are byte-identical. */
int athena_mp_radius_pairs_batched(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim, const float *points_dev,
                                   float radius, int32_t *pairs_dev, float *coords_dev, int64_t capacity,
                                   int64_t *edge_offsets_host, int64_t *n_pairs_out);
/* The same with every array on the host, for callers that hold Fortran arrays: clouds -> adj_ia [n+1], adj_ja [2, capacity]
 * column-major (what generate_adjacency [+ add_self_loops] makes of the pair list), coords [coords_capacity, dim] and
 * edge_offsets [n_clouds + 1] (may be NULL).  adj_ja_out == NULL: size query for both counts (*nnz_out, *n_pairs_out) and
 * edge_offsets. */
int athena_mp_radius_graph_batched_host(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim,
                                        const float *points_host, float radius, int32_t add_self_loops, int32_t *adj_ia_out,
                                        int32_t *adj_ja_out, int64_t capacity, int64_t *nnz_out, float *coords_out,
                                        int64_t coords_capacity, int64_t *n_pairs_out, int64_t *edge_offsets_out);
/* Radius graphs between TWO point sets on the device, a batch of clouds per call (bipartite_graph.hip): every query is joined to
 * the sources of its cloud inside the radius -- the graph a graph neural operator integrates over when its output points are not
 * its input points (a mesh onto a latent grid, a latent grid onto query points, coarse onto fine, sensors onto a mesh).  Every
 * implementation gives the same arrays.
 *   queries [n_queries, dim] and sources [n_sources, dim] fp32 row-major on the device, dim in 1..3; query_offsets and
 *   source_offsets [n_clouds + 1] int32 on the HOST, 0-based, ascending from 0 to n_queries / n_sources: cloud b owns the queries
 *   query_offsets[b] .. query_offsets[b+1]-1 and the sources source_offsets[b] .. source_offsets[b+1]-1; either slice may be
 *   empty, in any cloud; one radius fp32 > 0 for all clouds.
 *   Which pairs join: query i and source j of the same cloud are joined iff s <= fl(radius * radius), with d = q_i - p_j per
 *   component in fp32 and s = ((d0*d0) + d1*d1) + d2*d2, every operation rounded on its own: the predicate of
 *   athena_mp_radius_pairs, unchanged.  The two sets have separate index spaces: there is no self-pair rule, a query that
 *   coincides with a source is joined to it, and i == j means nothing.
 *   Numbering: pairs are numbered in lexicographic order of the global (i, j).  pairs [2, capacity] column-major, 1-based: row 1
 *   the query, row 2 the source; coords [capacity, dim], coords[e, :] = q_i - p_j (query minus source); rowptr [n_queries + 1]
 *   int32 on the device (may be NULL): rowptr[i] = the 0-based number of pairs whose query is below i, rowptr[n_queries] = the
 *   number of pairs; edge_offsets [n_clouds + 1] int64 on the HOST (may be NULL): edge_offsets[b] = rowptr[query_offsets[b]].
 * pairs_dev, coords_dev and rowptr_dev all NULL: size query (the count pass only; edge_offsets is still filled).  Each may be NULL
 * alone.  Refused with a message: dim outside 1..3; a radius that is not finite or <= 0 or whose square is not finite in fp32;
 * n_clouds < 0; for either offset array, named: offsets[0] != 0, a descending offset (the cloud is named, 1-based), an end that
 * is not the set's size; a non-finite coordinate in either set (the set, cloud, component and point of the first one are named,
 * 1-based; the queries are looked at first); pairs >= 2^31 (found by the count pass, before anything of that size is allocated);
 * capacity < pairs.  n_queries == 0 or n_sources == 0 succeeds with no pairs.  The library stays usable after a refusal.  Two
 * builds of the same input are byte-identical. */
int athena_mp_radius_pairs_bipartite(int32_t n_clouds, int32_t n_queries, const int32_t *query_offsets_host, int32_t n_sources,
                                     const int32_t *source_offsets_host, int32_t dim, const float *queries_dev,
                                     const float *sources_dev, float radius, int32_t *pairs_dev, float *coords_dev, int64_t capacity,
                                     int32_t *rowptr_dev, int64_t *edge_offsets_host, int64_t *n_pairs_out);
/* Such a pair list, already in HBM -> the directed, rectangular handle: pair e is the single CSR entry (row i, column j, edge id
 * e); no reverse entry, no self loops.  row_deg[i] is the row's length, col_deg[j] the number of entries in column j: the handle
 * is, array for array, what athena_mp_graph_create(n_rows, n_cols, n_pairs, adj_ia, adj_ja, n_pairs, row_deg, col_deg, ...)
 * builds from the same CSR.  adj_ia_out [n_rows + 1] (host, 1-based) is always filled; adj_ja_out [2, capacity] (host,
 * column-major: column, edge id) only when non-null.  The list must be strictly ascending in (i, j) with 1 <= i <= n_rows and
 * 1 <= j <= n_cols: checked on the device, and the first offending pair is named in the refusal. */
int athena_mp_graph_create_bipartite_dev(int32_t n_rows, int32_t n_cols, int64_t n_pairs, const int32_t *pairs_dev,
                                         int32_t *adj_ia_out, int32_t *adj_ja_out, int64_t capacity, athena_mp_graph **out);
/* athena_mp_radius_pairs_bipartite with every array on the host, for callers that hold Fortran arrays: adj_ia [n_queries + 1]
 * (1-based), adj_ja [2, capacity] column-major (source, edge id: one directed entry per pair), coords [coords_capacity, dim] and
 * edge_offsets [n_clouds + 1] (may be NULL).  adj_ja_out == NULL: size query for *n_pairs_out and edge_offsets. */
int athena_mp_radius_graph_bipartite_host(int32_t n_clouds, int32_t n_queries, const int32_t *query_offsets_host, int32_t n_sources,
                                          const int32_t *source_offsets_host, int32_t dim, const float *queries_host,
                                          const float *sources_host, float radius, int32_t *adj_ia_out, int32_t *adj_ja_out,
                                          int64_t capacity, float *coords_out, int64_t coords_capacity, int64_t *edge_offsets_out,
                                          int64_t *n_pairs_out);
/* k-nearest-neighbour graphs between TWO point sets on the device, a batch of clouds per call (knn_bipartite.hip): every query is
 * joined to the k nearest sources of its cloud -- the rectangular graph of a graph neural operator whose queries may lie where the
 * sources are sparse (a fixed radius finds nothing there) or dense (a fixed radius makes a hub), of PointNet++ feature propagation
 * and of k-nearest-neighbour interpolation.  Every implementation gives the same arrays.
 *   Inputs: those of athena_mp_radius_pairs_bipartite -- queries [n_queries, dim], sources [n_sources, dim] fp32 on the device, dim
 *   in 1..3, query_offsets / source_offsets [n_clouds + 1] on the HOST, either slice of any cloud may be empty -- and 1 <= k <= 64
 *   and a radius, +infinity meaning no cap.
 *   Distance: s(i, j) from d = q_i - p_j per component, s = ((d0*d0) + d1*d1) + d2*d2, every operation rounded to fp32 on its own.
 *   Candidates of query i: ALL sources of its cloud.  There is no self rule (separate index spaces): a query on top of a source is
 *   joined to it at s = 0.  With a finite radius only candidates with s <= fl(radius * radius) count.  An s that overflows is +inf;
 *   without a cap it is still a candidate and orders last.
 *   Order: by the key (s, j), ties to the smaller source index; N_k(i) is the first min(k, candidates).
 *   Directed outputs: nbr [n_queries, k] int32 = N_k(i) as 1-based global source ids in KEY order, padded with 0; sqdist
 *   [n_queries, k] fp32 = the s of each entry, padded with +inf.
 *   Graph outputs, with the conventions of athena_mp_radius_pairs_bipartite: one pair per (i, j in N_k(i)), numbered in
 *   lexicographic order of the global (i, j) -- inside a row the sources ascend by INDEX, not by key; pairs [2, capacity] 1-based,
 *   query first; coords[e, :] = q_i - p_j; rowptr [n_queries + 1] int32 on the device; edge_offsets [n_clouds + 1] int64 on the
 *   HOST, edge_offsets[b] = rowptr[query_offsets[b]].  athena_mp_graph_create_bipartite_dev and
 *   athena_mp_edge_grad_to_point_sets take the result as it is.
 * Each of the five device outputs may be NULL alone; all NULL is a size query that still fills edge_offsets (without a cap a row's
 * length is min(k, sources of the cloud): no search).  capacity = n_queries * k always suffices.  Refused with a message: dim
 * outside 1..3; k outside 1..64; a radius that is NaN or <= 0; the offset errors of athena_mp_radius_pairs_bipartite, in its
 * wording; a non-finite coordinate in either set (set, cloud, component and point named, 1-based; the queries first);
 * n_queries * k >= 2^31; capacity < pairs.  n_queries == 0 or n_sources == 0 succeeds with no pairs.  The library stays usable after
 * a refusal.  Two builds of the same input are byte-identical.  athena_mp_knn_stats reports this search as well.  Cost: without a
 * cap a query d cells outside the box of its cloud's sources walks about d shells of the grid, and one far away reads all of it --
 * correct and slow; with a cap the search ends after a few shells wherever the query lies. */
int athena_mp_knn_pairs_bipartite(int32_t n_clouds, int32_t n_queries, const int32_t *query_offsets_host, int32_t n_sources,
                                  const int32_t *source_offsets_host, int32_t dim, const float *queries_dev, const float *sources_dev,
                                  int32_t k, float radius, int32_t *nbr_dev, float *sqdist_dev, int32_t *pairs_dev, float *coords_dev,
                                  int64_t capacity, int32_t *rowptr_dev, int64_t *edge_offsets_host, int64_t *n_pairs_out);
/* The same with every array on the host, for callers that hold Fortran arrays; it follows athena_mp_radius_graph_bipartite_host:
 * adj_ia [n_queries + 1] (1-based), adj_ja [2, capacity] column-major (source, edge id), coords [coords_capacity, dim],
 * edge_offsets [n_clouds + 1] (may be NULL), and nbr / sqdist [n_queries, k] (each may be NULL).  adj_ja_out == NULL: size query
 * for *n_pairs_out and edge_offsets. */
int athena_mp_knn_graph_bipartite_host(int32_t n_clouds, int32_t n_queries, const int32_t *query_offsets_host, int32_t n_sources,
                                       const int32_t *source_offsets_host, int32_t dim, const float *queries_host,
                                       const float *sources_host, int32_t k, float radius, int32_t *adj_ia_out, int32_t *adj_ja_out,
                                       int64_t capacity, float *coords_out, int64_t coords_capacity, int32_t *nbr_out, float *sqdist_out,
                                       int64_t *edge_offsets_out, int64_t *n_pairs_out);
/* A batch of point clouds -> ONE block-diagonal k-nearest-neighbour graph on the device (knn_graph.hip): the neighbour cap beside
 * the radius graphs above, for clouds whose density varies by orders of magnitude.  Every implementation gives the same arrays.
 *   points [n, dim] fp32 row-major on the device, dim in 1..3; offsets [n_clouds + 1] int32 on the HOST, 0-based, as in
 *   athena_mp_radius_pairs_batched.  The candidates of point i are the other points j != i of its own cloud.
 *   Distance: s(i, j) is the squared distance of athena_mp_radius_pairs, unchanged: d = p_i - p_j per component,
 *   s = ((d0*d0) + d1*d1) + d2*d2, every operation rounded to fp32 on its own.  It is symmetric in i and j bit for bit.
 *   Order: the candidates of i are ordered by the key (s(i, j), j): s first, then the smaller index (on a lattice the tie rule
 *   decides the graph, so it is part of the definition).  N_k(i) is the first min(k, candidates) candidates in that order.
 *   Radius cap: with a finite radius only candidates with s <= fl(radius * radius) count (the radius builder's predicate);
 *   radius = +infinity means no cap.  1 <= k <= 64.
 *   Directed output: nbr [n, k] int32 (may be NULL): row i holds N_k(i) as 1-based global ids in key order, padded with 0.
 *   Undirected output: a pair i < j is an edge in mode 0 (union) iff j in N_k(i) or i in N_k(j), in mode 1 (mutual) iff both.
 *   Pairs are numbered in lexicographic order of the global (i, j): pairs [2, capacity] column-major, 1-based; coords [capacity,
 *   dim], coords[e, :] = p_i - p_j; edge_offsets [n_clouds + 1] int64 on the HOST (may be NULL), edge_offsets[b] = the number of
 *   pairs whose i is below offsets[b] -- the conventions of athena_mp_radius_pairs_batched, so athena_mp_graph_create_from_edges_dev,
 *   athena_mp_batch_plan_create and athena_mp_edge_grad_to_points take the result as it is.
 * nbr_dev, pairs_dev and coords_dev all NULL: size query (edge_offsets is still filled).  capacity = n * k always suffices, so a
 * caller can run the search once and narrow afterwards.  Refused with a message: dim outside 1..3; k outside 1..64; a radius that
 * is NaN or <= 0; a mode other than 0 or 1; n_clouds < 0, offsets[0] != 0, a descending offset, offsets[n_clouds] != n (the
 * wording of athena_mp_radius_pairs_batched); a non-finite coordinate (cloud, component and point of the first one are named,
 * 1-based); n * k >= 2^31; capacity < pairs.  The library stays usable after a refusal.  Two builds of the same input are
 * byte-identical.  Worst case: with no cap and clusters far apart that hold fewer than k + 1 points each, a query visits every
 * cell of its cloud's grid -- correct and slow; the cap is the remedy. */
int athena_mp_knn_pairs_batched(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim, const float *points_dev,
                                int32_t k, float radius, int32_t mode, int32_t *nbr_dev, int32_t *pairs_dev, float *coords_dev,
                                int64_t capacity, int64_t *edge_offsets_host, int64_t *n_pairs_out);
/* The same for one cloud of n points. */
int athena_mp_knn_pairs(int32_t n, int32_t dim, const float *points_dev, int32_t k, float radius, int32_t mode, int32_t *nbr_dev,
                        int32_t *pairs_dev, float *coords_dev, int64_t capacity, int64_t *n_pairs_out);
/* The same with every array on the host, for callers that hold Fortran arrays: clouds -> adj_ia [n+1], adj_ja [2, capacity]
 * column-major (what generate_adjacency [+ add_self_loops] makes of the pair list), coords [coords_capacity, dim] and
 * edge_offsets [n_clouds + 1] (may be NULL).  adj_ja_out == NULL: size query for both counts (*nnz_out, *n_pairs_out) and
 * edge_offsets. */
int athena_mp_knn_graph_batched_host(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim, const float *points_host,
                                     int32_t k, float radius, int32_t mode, int32_t add_self_loops, int32_t *adj_ia_out,
                                     int32_t *adj_ja_out, int64_t capacity, int64_t *nnz_out, float *coords_out,
                                     int64_t coords_capacity, int64_t *n_pairs_out, int64_t *edge_offsets_out);
/* What the search of the last k-nearest-neighbour call (one set or two) did: out[0] = query points, out[1] = candidates examined (distances
 * evaluated), out[2] = grid cells visited, out[3] = the largest shell (Chebyshev cell distance) any query reached. */
int athena_mp_knn_stats(int64_t out[4]);
/* Farthest-point sampling of a batch of point clouds on the device (fps.hip): m_b of a cloud's own points that cover it whatever
 * its density -- the second point set of athena_mp_radius_pairs_bipartite / athena_mp_knn_pairs_bipartite (coarse onto fine, a mesh
 * onto latent points, PointNet++ set abstraction) -- of which every prefix is a sample too, and the covering radius as a
 * by-product.  Every implementation gives the same arrays.
 *   Inputs: points [n, dim] fp32 row-major on the device, dim in 1..3; offsets [n_clouds + 1] int32 on the HOST, 0-based, as in
 *   athena_mp_radius_pairs_batched (empty clouds allowed); sample_offsets [n_clouds + 1] int32 on the HOST, 0-based, ascending from
 *   0 to n_samples: cloud b gets m_b = sample_offsets[b+1] - sample_offsets[b] samples, 0 <= m_b <= n_b; start [n_clouds] int32 on
 *   the HOST, 1-based global indices, or NULL: entry b is used only when m_b > 0 and must then lie in cloud b; NULL, or an entry of
 *   0, means the cloud's first point.
 *   Distance: s(i, j) is the squared distance of athena_mp_radius_pairs, unchanged: d = p_i - p_j per component,
 *   s = ((d0*d0) + d1*d1) + d2*d2, every operation rounded to fp32 on its own.  An overflow is +inf; finite inputs never give NaN.
 *   Selection, per cloud: dmin[j] = +inf for every point; step 1 chooses start; after choosing c, dmin[j] = min(dmin[j], s(j, c))
 *   for every j of the cloud; the next step chooses, among the points NOT YET CHOSEN, the largest dmin, ties to the SMALLER index.
 *   So coincident points are chosen last, in index order, and a lattice, or distances that overflow, is decided by the index.
 *   Outputs, on the device, each may be NULL alone: sample [n_samples] int32 = the chosen points as 1-based global indices in
 *   selection order, cloud after cloud; sample_points [n_samples, dim] = their rows, bit for bit; sample_sqdist [n_samples] = the
 *   chosen point's dmin at the moment it was chosen: +inf for a cloud's first sample, non-increasing after it; cover_sqdist
 *   [n_clouds] = the largest dmin[j] over ALL points of the cloud after the last update: +inf when n_b > 0 = m_b, 0 for an empty
 *   cloud.  Its square root, rounded up, is the radius with which athena_mp_radius_pairs_bipartite (samples as queries) leaves no
 *   point of the cloud without a sample.
 * Refused with a message: dim outside 1..3; n_clouds < 0; for either offset array, named, the offset errors of
 * athena_mp_radius_pairs_bipartite; m_b > n_b (the cloud is named); a start outside its cloud; a non-finite coordinate (cloud,
 * component and point of the first one are named, 1-based).  The library stays usable after a refusal.  Two calls on the same input
 * are byte-identical.  Cost: one cloud is sampled by ONE workgroup, its m_b steps in one launch; a batch of clouds fills the device,
 * one large cloud runs on one compute unit. */
int athena_mp_farthest_points(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim, const float *points_dev,
                              int32_t n_samples, const int32_t *sample_offsets_host, const int32_t *start_host, int32_t *sample_dev,
                              float *sample_points_dev, float *sample_sqdist_dev, float *cover_sqdist_dev);
/* The same with every array on the host, for callers that hold Fortran arrays; each output may be NULL alone. */
int athena_mp_farthest_points_host(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim, const float *points_host,
                                   int32_t n_samples, const int32_t *sample_offsets_host, const int32_t *start_host,
                                   int32_t *sample_out, float *sample_points_out, float *sample_sqdist_out, float *cover_sqdist_out);
/* What the last farthest-point call did: out[0] = samples chosen, out[1] = chunk tests of the stream route (a chunk is 64 points of
 * a cloud too large for the register route; one test per chunk and step), out[2] = the tests that skipped their chunk, out[3] =
 * clouds that took the stream route. */
int athena_mp_fps_stats(int64_t out[4]);
/* Voxel-grid clusters of a batch of point clouds on the device (grid_clusters.hip): every cloud is cut into cubic cells of edge
 * `size`, every non-empty cell is one coarse point -- the centroid of its members -- and the membership is the pooling graph: grid
 * subsampling / voxel pooling, the O(n) coarsening of large clouds beside athena_mp_farthest_points, with no dependent steps.  The
 * membership list is what athena_mp_graph_create_bipartite_dev takes; on that handle athena_mp_pool_max_fwd is max pooling and
 * athena_mp_interp_fwd with `weights` is mean pooling.  Every implementation gives the same arrays.
 *   Inputs: points [n, dim] fp32 row-major on the device, dim in 1..3; offsets [n_clouds + 1] int32 on the HOST, 0-based, as in
 *   athena_mp_radius_pairs_batched (empty clouds allowed anywhere); size fp32 > 0, one for all clouds; origin_host [dim] fp32 on the
 *   HOST, or NULL.
 *   The cell of a point, every operation rounded to fp32 on its own: inv = 1 / size.  Per non-empty cloud b and axis k, lo_k = the
 *   smallest k-th coordinate of the cloud's points with +0 added (-0 becomes +0) and hi_k the largest; with an origin, lo_k =
 *   origin_k for every cloud.  The cell of point j is c_k = floor((p_jk - lo_k) * inv).  The cloud has nc_k = floor((hi_k - lo_k) *
 *   inv) + 1 cells along axis k -- rounding is monotone, so the largest c_k that occurs is exactly nc_k - 1 -- and N_b = nc_0 nc_1
 *   nc_2 cells in all.
 *   Clusters: a cluster is a non-empty cell of a cloud.  Clusters are numbered, 1-based and over the whole batch, in ascending
 *   order of (cloud, c_{dim-1}, ..., c_0): c_0 varies fastest.  Inside a cluster the members are in ascending point index.  m is
 *   the number of clusters, count_c the members of cluster c.
 *   Outputs, on the device unless marked, each may be NULL alone:
 *     cluster [n] int32              the cluster of each point
 *     pairs [2, n] int32             column-major, 1-based: (cluster, point) in lexicographic order -- the list
 *                                    athena_mp_graph_create_bipartite_dev(n_rows = m, n_cols = n, n_pairs = n, ...) takes
 *     rowptr [capacity + 1] int32    0-based: rowptr[c] = the pairs in front of cluster c, rowptr[m] = n; m + 1 entries are written
 *     weights [n] fp32               one per pair: 1 / fl(count) of the pair's cluster (mean pooling through athena_mp_interp_fwd)
 *     centroid [capacity, dim] fp32  lo_k + S_k / fl(count), S_k the SEQUENTIAL sum, from +0, of (p_jk - lo_k) over the members in
 *                                    index order.  Relative to lo on purpose: the plain sum of coordinates around 1e6 loses them
 *     nearest [capacity] int32       the member with the smallest s(p_j, centroid), s the squared distance of
 *                                    athena_mp_radius_pairs (d = p_j - centroid, s = ((d0*d0) + d1*d1) + d2*d2), ties to the smaller
 *                                    index: a 1-based global point id, as `sample` of athena_mp_farthest_points
 *     cell [capacity, dim] int32     the cluster's c_k
 *     cluster_offsets [n_clouds + 1] int32 on the HOST: the clusters in front of each cloud; cluster_offsets[n_clouds] = m
 *     origin_out [n_clouds, dim] fp32 on the HOST: the lo used (0 for an empty cloud)
 *     *n_clusters_out = m (never NULL)
 *   Of the arrays with capacity rows, m are written.  All seven device outputs NULL: a size query (m, cluster_offsets, origin_out).
 * Refused with a message: dim outside 1..3; a size that is not finite or <= 0, or whose inverse is not finite; n_clouds < 0, n < 0
 * and the offset errors of athena_mp_farthest_points, in its wording; an origin that is not finite; a non-finite coordinate (cloud,
 * component and point of the first one are named, 1-based); hi_k - lo_k not finite (cloud and axis named); an origin above a
 * coordinate (cloud, axis and the cloud's first such point named); nc_k > 2^21 on an axis (cloud and axis named);
 * bits_for(n_clouds - 1) + bits_for(max N_b - 1) > 62, bits_for(v) = the bits of v, at least 1; capacity < m with a device output
 * given.  There is no other limit on the number of cells.  n == 0 or n_clouds == 0 succeeds with no clusters.  The library stays
 * usable after a refusal.  Two calls on the same input are byte-identical.  Cost: a cluster is summed by one group of 4 lanes in member order;
 * a cluster of many thousands of points is that group's loop. */
int athena_mp_grid_clusters(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim, const float *points_dev, float size,
                            const float *origin_host, int64_t capacity, int32_t *cluster_dev, int32_t *pairs_dev, int32_t *rowptr_dev,
                            float *weights_dev, float *centroid_dev, int32_t *nearest_dev, int32_t *cell_dev,
                            int32_t *cluster_offsets_host, float *origin_out_host, int64_t *n_clusters_out);
/* The reverse step of centroid: dpoints[j, k] = dcentroid[c, k] / fl(count_c), c = cluster[j], count_c = rowptr[c + 1] - rowptr[c]
 * (only differences of rowptr are used: a 1-based adj_ia serves as well); fp32, / correctly rounded: every bit is defined.  lo is a
 * constant and cancels; nearest and cell carry no gradient.  cluster [n], rowptr [n_clusters + 1], dcentroid [n_clusters, dim] and
 * dpoints [n, dim] on the device.  Refused with a message: dim outside 1..3, a negative count, a cluster id outside 1..n_clusters
 * (the first such point is named; nothing is read through it). */
int athena_mp_grid_clusters_grad(int32_t n, int32_t dim, int32_t n_clusters, const int32_t *cluster_dev, const int32_t *rowptr_dev,
                                 const float *dcentroid_dev, float *dpoints_dev);
/* athena_mp_grid_clusters with every array on the host, for callers that hold Fortran arrays: the membership as adj_ia
 * [capacity + 1] (1-based) and adj_ja [2, n] column-major (point, edge id: pair e is entry e) in the conventions of
 * athena_mp_radius_graph_bipartite_host; cluster, weights [n], centroid, cell [capacity, dim] and nearest [capacity] may each be
 * NULL.  adj_ja_out == NULL: size query for *n_clusters_out, cluster_offsets and origin_out. */
int athena_mp_grid_clusters_host(int32_t n_clouds, int32_t n, const int32_t *offsets_host, int32_t dim, const float *points_host,
                                 float size, const float *origin_host, int64_t capacity, int32_t *cluster_out, int32_t *adj_ia_out,
                                 int32_t *adj_ja_out, float *weights_out, float *centroid_out, int32_t *nearest_out, int32_t *cell_out,
                                 int32_t *cluster_offsets_out, float *origin_out, int64_t *n_clusters_out);
/* athena_mp_grid_clusters_grad with every array on the host, staged through HBM. */
int athena_mp_grid_clusters_grad_host(int32_t n, int32_t dim, int32_t n_clusters, const int32_t *cluster, const int32_t *rowptr,
                                      const float *dcentroid, float *dpoints);
/* What the last athena_mp_grid_clusters call did: out[0] = clusters, out[1] = the key bits sorted (cloud bits + cell bits), out[2] =
 * the 8-bit passes of the radix sort, out[3] = the members of the largest cluster (0 after a size query). */
int athena_mp_grid_clusters_stats(int64_t out[4]);
/* A pair list relabelled through a vertex map and merged, on the device (contract.hip): the contraction of a graph over a cluster
 * map -- the pooled graph of a graph U-Net or multi-scale MeshGraphNet level, which keeps the fine graph's adjacency instead of a
 * new geometric search over the centroids --, the induced subgraph of a vertex selection (id 0 drops a vertex), the merge of a
 * multigraph's duplicate pairs (no maps) and, behind athena_mp_cell_pairs, the edge graph of a mesh.  Every implementation gives
 * the same arrays.
 *   Inputs, on the device: pairs [2, n_pairs] int32, column-major, 1-based -- the index_list every builder writes, column = fine
 *   edge id; an index of 0 is allowed and means "no such edge".  n_rows, n_cols: the index spaces of its two rows (a one-set list
 *   passes the same value twice).  row_cluster [n_rows], col_cluster [n_cols] int32, values in 0 .. m_rows / 0 .. m_cols, 0 = the
 *   vertex is dropped; the two may be the same pointer; NULL = the identity, and then m must equal n.  mode 0: undirected, one
 *   set; mode 1: directed, two sets.  row_points [m_rows, dim], col_points [m_cols, dim] fp32, dim in 1..3: both or neither, may
 *   be the same pointer.
 *   Definition.  For fine edge e = (u, v): a = row_cluster[u], b = col_cluster[v].  The edge takes part iff u >= 1, v >= 1, a >= 1,
 *   b >= 1 and, in mode 0, a != b.  Its coarse key is (min(a, b), max(a, b)) in mode 0 and (a, b) in mode 1.  The coarse pairs are
 *   the distinct keys, numbered 1-based in lexicographic order; P is their number.  The members of a coarse pair are its fine
 *   edges in ascending edge id; M is the number of edges that take part.
 *   Outputs, on the device, each may be NULL alone:
 *     coarse_pairs [2, capacity] int32      column-major, 1-based, strictly ascending (mode 0: a < b): what
 *                                           athena_mp_graph_create_from_edges_dev takes in mode 0 and
 *                                           athena_mp_graph_create_bipartite_dev in mode 1
 *     rowptr [capacity + 1] int32           0-based: the members in front of each coarse pair, rowptr[P] = M; P + 1 entries written
 *     members [2, member_capacity] int32    column-major, 1-based: (coarse pair, fine edge), strictly ascending -- the list
 *                                           athena_mp_graph_create_bipartite_dev(P, n_pairs, M, ...) turns into the edge-pooling
 *                                           handle
 *     weights [member_capacity] fp32        one per member: 1 / fl(count) of its coarse pair (mean pooling through
 *                                           athena_mp_interp_fwd, as athena_mp_grid_clusters)
 *     edge_pair [n_pairs] int32             the coarse pair of each fine edge, 0 where it takes no part
 *     coords [capacity, dim] fp32           row_points[a] - col_points[b] per component in fp32: the builders' convention (smaller
 *                                           index minus larger in mode 0, query minus source in mode 1)
 *     *n_coarse_out = P, *n_members_out = M (never NULL)
 *   Of the arrays with capacity rows, P are written; of those with member_capacity rows, M.  All six NULL: a size query.
 * Refused with a message: a mode outside 0..1; n_pairs >= 2^31 or a negative size; mode 0 with n_rows != n_cols or m_rows !=
 * m_cols; a NULL map with m != n; only one of the point arrays, dim outside 1..3 with points, coords without points;
 * bits_for(m_rows) + bits_for(m_cols) > 62, bits_for(v) = the bits of v, at least 1; a pair index outside 0 .. n (the first such
 * pair is named, nothing is read through it); a cluster id outside 0 .. m (the first such vertex is named; the row map is looked at
 * first); capacity < P or member_capacity < M with a matching output given.  n_pairs == 0 succeeds with nothing (rowptr[0] = 0)
 * before the maps are looked at.  The library stays usable after a refusal.  Two calls on the same input are byte-identical. */
int athena_mp_contract_pairs(int64_t n_pairs, const int32_t *pairs_dev, int32_t n_rows, int32_t n_cols, const int32_t *row_cluster_dev,
                             const int32_t *col_cluster_dev, int32_t m_rows, int32_t m_cols, int32_t mode, int32_t dim,
                             const float *row_points_dev, const float *col_points_dev, int64_t capacity, int64_t member_capacity,
                             int32_t *coarse_pairs_dev, int32_t *rowptr_dev, int32_t *members_dev, float *weights_dev,
                             int32_t *edge_pair_dev, float *coords_dev, int64_t *n_coarse_out, int64_t *n_members_out);
/* athena_mp_contract_pairs with every array on the host, for callers that hold Fortran arrays, staged through HBM; the same
 * arguments, the same arrays.  All six outputs NULL: the size query. */
int athena_mp_contract_pairs_host(int64_t n_pairs, const int32_t *pairs, int32_t n_rows, int32_t n_cols, const int32_t *row_cluster,
                                  const int32_t *col_cluster, int32_t m_rows, int32_t m_cols, int32_t mode, int32_t dim,
                                  const float *row_points, const float *col_points, int64_t capacity, int64_t member_capacity,
                                  int32_t *coarse_pairs_out, int32_t *rowptr_out, int32_t *members_out, float *weights_out,
                                  int32_t *edge_pair_out, float *coords_out, int64_t *n_coarse_out, int64_t *n_members_out);
/* What the last contraction call did: out[0] = P, out[1] = M, out[2] = the key bits sorted (bits_for(m_rows) + bits_for(m_cols) + 1:
 * the bit on top marks the edges that take no part), out[3] = the members of the largest coarse pair (0 after a size query). */
int athena_mp_contract_stats(int64_t out[4]);
/* A handle's pair list, written on the device: pairs [2, n_edge_cols] int32, column-major, 1-based.  For edge column e the pair is
 * (row + 1, col + 1) of the entry with the smallest CSR index that carries it (athena_mp_graph_export 8, 9, 10 and 1); an edge
 * column no entry carries gives (0, 0).  On a handle of athena_mp_graph_create_from_edges_dev that is (min(u, v), max(u, v)) of
 * input pair e; on a handle of athena_mp_graph_create_bipartite_dev the pair itself.  Launched on the library's stream, not
 * synchronised.  Refused: capacity < n_edge_cols. */
int athena_mp_graph_pairs(const athena_mp_graph *g, int32_t *pairs_dev, int64_t capacity);
/* Mesh elements -> a pair list on the device: cells [n_cells, nv] int32 row-major, 1-based.  cell_type 1: segment, nv = 2, 1 pair;
 * 2: triangle, nv = 3, 3 pairs; 3: quadrilateral, nv = 4, the ring 01 12 23 30; 4: tetrahedron, nv = 4, all 6 pairs.  Simplices
 * list their pairs in lexicographic local order.  pairs [2, capacity] int32 column-major: slot c * ne + l holds local pair l of
 * cell c as given, neither ordered nor deduplicated; *n_pairs_out = n_cells * ne; pairs_dev == NULL: the count and the check
 * only.  Fed to athena_mp_contract_pairs(mode 0, no maps) this is the mesh's edge graph: the differences of rowptr count the
 * elements on each edge (1 on the boundary of a triangle mesh), the pooling handle maps element-edge slots to edges, and a cell
 * with a repeated vertex loses that pair by the a != b rule.  Refused with a message: a cell_type outside 1..4; a negative size;
 * n_cells * ne >= 2^31; a vertex id outside 1 .. n_vertices (the first such cell is named); capacity < n_cells * ne. */
int athena_mp_cell_pairs(int32_t n_vertices, int64_t n_cells, int32_t cell_type, const int32_t *cells_dev, int32_t *pairs_dev,
                         int64_t capacity, int64_t *n_pairs_out);
/* Top-k vertex selection per graph from scores, on the device (topk_select.hip): the coarsening rule of TopKPooling (Graph U-Nets),
 * SAGPool and ASAPool, for graphs without coordinates.  It produces the vertex map athena_mp_contract_pairs takes for an induced
 * subgraph (id 0 drops a vertex).  Every implementation gives the same arrays.
 *   Inputs: n_graphs graphs over n vertices; offsets [n_graphs + 1] int32 on the HOST, 0-based, ascending from 0 to n, empty graphs
 *   allowed; score [n] fp32 on the device; k_host [n_graphs] on the host, or NULL and then k for every graph; has_min_score 0 / 1
 *   and min_score.
 *   Order inside a graph: value descending, then vertex index ascending.  -0 and +0 are equal (the value is score + 0.0f).  Every
 *   NaN, of either sign and any payload, equals every other NaN and lies below -inf.
 *   Graph g keeps the first min(k_g, n_g) vertices of that order; with has_min_score a kept vertex also has score >= min_score,
 *   which is false for a NaN (on either side).  Those that pass are a prefix of the order, so the kept set is one too; a graph may
 *   keep nothing.
 *   Outputs, each may be NULL alone:
 *     cluster [n] int32 on the device        the new 1-based id of a kept vertex, 0 otherwise; the new ids number the kept vertices
 *                                            in ascending vertex index, so graphs stay contiguous and in the fine order
 *     selected [m] int32 on the device       the 1-based vertex of new id r + 1
 *     order [m] int32 on the device          per graph its kept vertices, 1-based, in score order: graph g's run starts at
 *                                            sel_offsets[g], and every prefix of a run is that graph's top-k'
 *     sel_offsets [n_graphs + 1] int32 on the HOST, 0-based: the kept vertices in front of each graph
 *     *n_selected_out = m (never NULL)
 *   selected and order need room for the sum of min(k_g, n_g) elements, which the caller can compute; exactly m are written.  There
 *   is no size query.  One host wait per call.
 * Refused with a message: a negative size; offsets that do not start at 0, are not ascending or do not end at n; a negative k (the
 * first such graph is named); ATHENA_MP_TOPK_ROUTE (a test switch, read at every call: auto, wave, sort) naming anything else, or
 * wave with a graph of more than 64 vertices.  n == 0 or n_graphs == 0 succeeds with nothing kept.  The library stays usable after
 * a refusal.  Two calls on the same input are byte-identical. */
int athena_mp_topk_vertices(int32_t n_graphs, int32_t n, const int32_t *offsets_host, const float *score_dev, int32_t k,
                            const int32_t *k_host, int32_t has_min_score, float min_score, int32_t *cluster_dev, int32_t *selected_dev,
                            int32_t *order_dev, int32_t *sel_offsets_host, int64_t *n_selected_out);
/* athena_mp_topk_vertices with every array on the host, for callers that hold Fortran arrays, staged through HBM; the same
 * arguments, the same arrays. */
int athena_mp_topk_vertices_host(int32_t n_graphs, int32_t n, const int32_t *offsets, const float *score, int32_t k,
                                 const int32_t *k_each, int32_t has_min_score, float min_score, int32_t *cluster_out,
                                 int32_t *selected_out, int32_t *order_out, int32_t *sel_offsets_out, int64_t *n_selected_out);
/* What the last selection call did: out[0] = graphs on the wave route (at most 64 vertices, one wave each; empty graphs count
 * here), out[1] = graphs on the sort route, out[2] = the key bits sorted (32 + bits_for(n_graphs - 1); 0 without a sort), out[3] =
 * the 8-bit passes of the radix sort. */
int athena_mp_topk_stats(int64_t out[4]);
/* The rows of a selection, gated (topk_select.hip).  x [n, F] fp32 row-major, F >= 1; gate [n] fp32 or NULL -- the caller makes it
 * with athena_mp_activation_fwd on the scores --; selected [m] and cluster [n] as athena_mp_topk_vertices wrote them.
 *   fwd:  y[r, :] = fl(x[v, :] * gate[v]), v = selected[r] - 1.  Without a gate a copy that keeps every bit: -0, infinities, NaN
 *         payloads.
 *   bwd:  dx[v, :] = fl(dy[c - 1, :] * gate[v]), c = cluster[v]; +0 where c = 0; every element of dx [n, F] is written; without a
 *         gate this is the un-pooling of dy.  dgate[v] = the sum over the columns of fl(dy[c - 1, col] * x[v, col]), exactly +0
 *         where c = 0: the one result whose summation order is free (a tree over the row's lanes), held to 1e-5 of the sum of the
 *         terms' magnitudes.  dx_dev or dgate_dev may be NULL; dgate needs x, dx does not.
 * Launched on the library's stream; the call waits for the check of the ids.  Refused with a message: a negative size; F < 1; a
 * selected id outside 1 .. n or a cluster id outside 0 .. m (the first such element is named; nothing is read through it).  The
 * library stays usable after a refusal.  Two calls on the same input are byte-identical, at any alignment of the arrays. */
int athena_mp_select_rows_fwd(int32_t n, int32_t m, int32_t F, const int32_t *selected_dev, const float *x_dev, const float *gate_dev,
                              float *y_dev);
int athena_mp_select_rows_bwd(int32_t n, int32_t m, int32_t F, const int32_t *cluster_dev, const float *dy_dev, const float *x_dev,
                              const float *gate_dev, float *dx_dev, float *dgate_dev);
/* ... with every array on the host, staged through HBM. */
int athena_mp_select_rows_host(int32_t n, int32_t m, int32_t F, const int32_t *selected, const float *x, const float *gate, float *y);
int athena_mp_select_rows_bwd_host(int32_t n, int32_t m, int32_t F, const int32_t *cluster, const float *dy, const float *x,
                                   const float *gate, float *dx, float *dgate);
/* Periodic structures -> neighbour graphs on the device, a batch per call (periodic_graph.hip).  It replaces get_graph_from_basis
 * of the reference's chemical examples (example/example_library/src/mod_read_chemical_graphs.f90:196-278); the step in front of
 * athena_mp_graph_create_from_edges_dev.
 *   n_structures structures; offsets [n_structures + 1] on the HOST, 0-based, ascending from 0 to n_atoms; frac [n_atoms, 3] fp32
 *   fractional coordinates; lat [n_structures, 3, 3] fp32 row-major, row a = lattice vector a (Cartesian); pbc [3] on the host,
 *   pbc[k] = 0: axis k is open (neither wrapped nor imaged); 0 <= cutoff_min < cutoff_max.
 * Definition, every operation rounded to fp32 on its own: for local atoms i <= j of one structure and an integer shift (a, b, c)
 *   f_k = frac_i[k] - frac_j[k];  w_k = f_k - ceil(f_k - 0.5) on a periodic axis, w_k = f_k and only shift 0 on an open axis;
 *   v = (w_0 + a, w_1 + b, w_2 + c);  x_c = ((v_0 * L[0][c]) + v_1 * L[1][c]) + v_2 * L[2][c];
 *   s = ((x_0 * x_0) + x_1 * x_1) + x_2 * x_2;  r = sqrt(s), correctly rounded.
 * The triple is an edge iff r > cutoff_min and r < cutoff_max (both strict, as the reference): never the zero-shift self pair; an
 * atom is joined to its own images, +shift and -shift both (each one CSR entry in the builders); a pair carries one edge per image.
 * All shifts of Z^3 on the periodic axes count: the result is defined by the predicate, not by a search range (the reference's
 * ceiling(cutoff_max / |L_a|) loses edges of skewed cells).  Edges are ordered by structure, inside one lexicographically by
 * (i, j, a, b, c) ascending; the 1-based rank over the batch is the edge id.  Outputs in HBM, each may be NULL:
 *   pairs [2, capacity] column-major, 1-based global vertex ids, smaller first;  feature [capacity] = r / cutoff_max (correctly
 *   rounded: the reference's edge feature);  vec [capacity, 3] = x (atom i minus the image of atom j, the sign of coords in
 *   athena_mp_radius_pairs);  shift [capacity, 3];  first_count [n_atoms] = edges whose FIRST index is that vertex (j >= i only:
 *   the reference's `degree` vertex feature).  edge_offsets_out [n_structures + 1] on the host (may be NULL): where each
 *   structure's edge columns start.  All five device outputs NULL: the count pass only, a size query.
 * Refused with a message that names the first offending structure where there is one: offsets not ascending from 0 to n_atoms, a
 * non-finite coordinate or lattice entry, det(lat) zero or not finite with a periodic axis, a cutoff that is not finite,
 * cutoff_min < 0 or cutoff_max <= cutoff_min, floor(cutoff_max |L_b x L_c| / |det L| + 1/2) above 31 on a periodic axis (the cell
 * is too small for the cutoff), 2 * edges + n_atoms >= 2^31 (found by the count pass, before anything of that size is allocated),
 * capacity < edges.  Two builds of the same input are byte-identical. */
int athena_mp_periodic_pairs(int32_t n_structures, int32_t n_atoms, const int32_t *offsets_host, const float *frac_dev,
                             const float *lat_dev, const int32_t *pbc, float cutoff_min, float cutoff_max, int32_t *pairs_dev,
                             float *feature_dev, float *vec_dev, int32_t *shift_dev, int32_t *first_count_dev, int64_t capacity,
                             int64_t *n_pairs_out, int64_t *edge_offsets_out);
/* The same with every array on the host, for callers that hold Fortran arrays: structures -> adj_ia [n_atoms + 1], adj_ja
 * [2, capacity] column-major (what generate_adjacency [+ add_self_loops] makes of the pair list), feature [edge_capacity],
 * vec [edge_capacity, 3], first_count [n_atoms] (each of the three may be NULL) and edge_offsets.  adj_ja_out == NULL: size query
 * for both counts (*nnz_out, *n_pairs_out) and edge_offsets. */
int athena_mp_periodic_graph_host(int32_t n_structures, int32_t n_atoms, const int32_t *offsets_host, const float *frac_host,
                                  const float *lat_host, const int32_t *pbc, float cutoff_min, float cutoff_max,
                                  int32_t add_self_loops, int32_t *adj_ia_out, int32_t *adj_ja_out, int64_t capacity,
                                  int64_t *nnz_out, float *feature_out, float *vec_out, int32_t *first_count_out,
                                  int64_t edge_capacity, int64_t *n_pairs_out, int64_t *edge_offsets_out);
/* What the most recent athena_mp_periodic_pairs pass of the process did (athena_mp_periodic_graph_host runs two: the last one
 * counts).  The builder has two routes with the same outputs, byte for byte, chosen per structure: the walk over every pair
 * i <= j, and a cell grid in fractional coordinates that prunes the pairs of large cells first (periodic_graph.hip proves the rule;
 * ATHENA_MP_PERIODIC_ROUTE = auto | walk | grid pins the route in tests).  Empty structures count nowhere.
 *   out[0] structures walked;  out[1] structures through the grid;  out[2] pairs i <= j examined by the walk;
 *   out[3] candidate pairs examined by the grid;  out[4] structures that qualified for the grid but took the walk because a
 *   fractional coordinate is beyond +-64, the lattice vectors are too long for the cutoff, or no axis is periodic. */
int athena_mp_periodic_stats(int64_t out[5]);
/* Geometry gradients (geometry_grad.hip): the reverse step of the two builders above.  The layers return their gradient per edge,
 * in HBM (athena_mp_gno_aggregate_bwd_coords: dcoords [E, d]; athena_mp_duvenaud_propagate_bwd_e: de [E, F_e]); these entries carry
 * it back to the points, the atoms and the cell.  Nothing in the reference corresponds to them (its edge geometry carries no
 * gradient).  g is the handle built from the builder's pair list with edge ids (athena_mp_graph_create_from_edges_dev,
 * with_edge_ids = 1), add_self_loops or not.
 * Definition.  All arithmetic is fp32, every operation rounded on its own, / and sqrt correctly rounded, as the builders.  Row i of
 * the handle is its forward CSR as athena_mp_graph_export shows it (rowptr, col, eid, 0-based, eid = -1: none); that order is the
 * summation order.
 *   Signed gather: acc = +0; for k = rowptr[i] .. rowptr[i+1]-1 in order, c = col[k], e = eid[k]: the entry is skipped when e < 0 (a
 *   self loop) or c == i (a self-image edge: its two ends are the same atom); else acc = acc + t_e when i < c, acc = acc - t_e when
 *   i > c.  out[i] = acc.  A row without entries gives +0; every output element is written.
 *   Points mode, the reverse of athena_mp_radius_pairs: t_e = dcoords[e, :] (dim in 1..3), dpoints [n, dim] = out.
 *   Periodic mode, the reverse of athena_mp_periodic_pairs: lat [B, 3, 3], cutoff_max and vec [E, 3] as the builder took and wrote
 *   them, offsets [B + 1] (int32) and edge_offsets [B + 1] (int64) on the HOST; dfeature [E, fe_cols] (fe_cols >= 1: the de of a
 *   layer whose edge input was `feature` in every column) and dvec [E, 3], each may be NULL, not both.  Per edge, x = vec[e]:
 *     s = ((x0 * x0) + x1 * x1) + x2 * x2, r = sqrt(s)  (the builder's own s and r; r > cutoff_min >= 0)
 *     q = (((de[e,0] + de[e,1]) + ...) + de[e,fe_cols-1]) / cutoff_max;  u_c = x_c / r
 *     gx_c = dvec[e,c] + q * u_c  (q * u_c alone when dvec is NULL, dvec[e,c] alone when dfeature is NULL)
 *   Outputs in HBM, each may be NULL:
 *     dcart [n, 3]      the signed gather of t_e = gx_e: dE/d(Cartesian position); forces are its negative
 *     dfrac [n, 3]      dfrac[i,k] = ((L[k][0] * g0) + L[k][1] * g1) + L[k][2] * g2, g = dcart[i], L the lattice of i's structure (on
 *                       open axes too)
 *     virial [B, 3, 3]  virial[s][c][d] = sum over e in [edge_offsets[s], edge_offsets[s+1]) of x_c * gx_d.  The summation order is
 *                       free; no atomics: two runs are byte-identical.  Not symmetric when dvec is given; an empty structure gives 0.
 *     dlat [B, 3, 3]    L^-T * virial: dE/dL at fixed fractional coordinates (x = v L), formed per structure in fp64 from the fp32
 *                       lattice and the fp32 virial, rounded once
 * Refused with a message: a handle without edge columns, n_atoms != the handle's rows, edge_offsets[B] != the handle's edge columns,
 * offsets / edge_offsets not ascending from 0, dim outside 1..3, fe_cols < 1 with dfeature, both gradients NULL, cutoff_max not
 * finite or <= 0, dlat asked for with det L zero or not finite (the structure is named; virial alone never needs the inverse).
 * n = 0 or E = 0 succeeds (with E = 0 every per-edge array is empty and may be NULL).  The values of the gradients are not scanned: NaN propagates. */
int athena_mp_edge_grad_to_points(const athena_mp_graph *g, int32_t dim, const float *dcoords_dev, float *dpoints_dev);
int athena_mp_periodic_grad(const athena_mp_graph *g, int32_t n_structures, int32_t n_atoms, const int32_t *offsets_host,
                            const int64_t *edge_offsets_host, const float *lat_dev, float cutoff_max, const float *vec_dev,
                            const float *dfeature_dev, int32_t fe_cols, const float *dvec_dev, float *dcart_dev, float *dfrac_dev,
                            float *virial_dev, float *dlat_dev);
/* The reverse of athena_mp_radius_pairs_bipartite (coords[e] = q_i - p_j), on a handle of athena_mp_graph_create_bipartite_dev:
 * rows and columns index different sets, so there is no sign by index and no skipped entry.  fp32, sequential sums:
 *   dqueries [n_rows, dim]: acc = +0; for k = rowptr[i] .. rowptr[i+1]-1 in order, acc = acc + dcoords[eid[k], :].
 *   dsources [n_cols, dim]: acc = +0; for k = t_rowptr[j] .. t_rowptr[j+1]-1 in order (queries ascending), acc = acc - dcoords[t_eid[k], :].
 * Every output element is written.  Each output may be NULL, not both.  Refused with a message: a handle without edge columns, a
 * handle with an entry that carries no edge id, dim outside 1..3.  The _host form takes Fortran arrays, staged through HBM. */
int athena_mp_edge_grad_to_point_sets(const athena_mp_graph *g, int32_t dim, const float *dcoords_dev, float *dqueries_dev,
                                      float *dsources_dev);
int athena_mp_edge_grad_to_point_sets_host(const athena_mp_graph *g, int32_t dim, const float *dcoords, float *dqueries, float *dsources);
/* Inverse-distance interpolation over a two-set graph, with its gradients (interp.hip): features carried from the sources to the
 * queries of athena_mp_radius_pairs_bipartite / athena_mp_knn_pairs_bipartite -- the feature propagation of PointNet++, the skip path
 * of a U-shaped operator's decoder, plain k-nearest-neighbour interpolation -- and, under it, a gather over a handle's CSR with
 * caller-supplied per-edge weights, forward and transposed (mean pooling onto samples and quadrature-weighted transfer are the same
 * call with other weights).  Nothing in the reference corresponds to them.
 * Definition.  All arithmetic is fp32, every operation rounded on its own, / correctly rounded, subnormals kept.  g is a rectangular
 * handle of athena_mp_graph_create_bipartite_dev (from either builder), E its edge columns; coords [E, dim] is what the builder
 * wrote, coords[e] = q_i - p_j, dim in 1..3.  Row i of the handle is its forward CSR as athena_mp_graph_export shows it (rowptr,
 * col, eid), column j its transposed CSR (t_rowptr, t_src, t_eid: queries ascending); those orders are the summation orders.
 *   Weights (athena_mp_interp_weights), d = coords[e]:
 *     s_e = ((d0 * d0) + d1 * d1) + d2 * d2: the builder's own expression, so s_e is its sqdist bit for bit
 *     w_e = 1 / m_e, m_e = eps where s_e <= eps, else s_e (max(s_e, eps); a NaN stays one); an s that overflowed gives w = +0
 *     W_i = +0; for k = rowptr[i] .. rowptr[i+1]-1 in order: W_i = W_i + w_eid[k]
 *     weights[e] = w_e / W_i for the edges of row i, +0 for every edge of a row whose W_i is 0;  wsum[i] = W_i (wsum may be NULL)
 *   Every element of both outputs is written; an empty row gives wsum = +0.  eps must be finite and at least 2^-60: then W cannot
 *   overflow, and weights[e] <= 1 because round-to-nearest sums of non-negative terms are monotone.
 *   Weighted gather, for ANY weights [E], not only the ones above:
 *     athena_mp_interp_fwd    x [n_cols, F] -> y [n_rows, F]:  acc = +0; for k = rowptr[i] .. in order:
 *                             acc = acc + weights[eid[k]] * x[col[k], f];  y[i, f] = acc
 *     athena_mp_interp_bwd_x  dy [n_rows, F] -> dx [n_cols, F]:  acc = +0; for k = t_rowptr[j] .. in order:
 *                             acc = acc + weights[t_eid[k]] * dy[t_src[k], f];  dx[j, f] = acc
 *   Arrays are row-major.  An empty row or column gives +0; every element is written; no atomics: two runs are byte-identical.
 *   Coordinate gradient (athena_mp_interp_bwd_coords), y the forward result, per edge e = (i, j):
 *     g_e = sum over f of dy[i, f] * (x[j, f] - y[i, f])   (the order of this sum is free: the one output that is not bit-defined)
 *     t_e = -(weights[e] * w_e) * g_e;  dcoords[e, c] = (2 * d_c) * t_e
 *   dcoords[e, :] is exactly +0 where s_e <= eps (the clamp) or w_e = 0.  The result is the gradient with respect to coords for
 *   weights made by athena_mp_interp_weights with the same eps, and feeds athena_mp_edge_grad_to_point_sets unchanged.
 * Every edge column must be carried by exactly one entry, which is what athena_mp_graph_create_bipartite_dev builds: each weights[e]
 * and dcoords[e, :] then has one writer.
 * Refused with a message: a handle without edge columns; an entry that carries no edge id; more or fewer entries than edge columns;
 * dim outside 1..3; F < 1; an eps that is not finite or below 2^-60.  The library stays usable after a refusal.  E = 0, n_rows = 0 and n_cols = 0 succeed (empty arrays may
 * be NULL).  Values are not scanned: NaN propagates.  A caller's pointer needs only the alignment of a float. */
int athena_mp_interp_weights(const athena_mp_graph *g, int32_t dim, const float *coords_dev, float eps, float *weights_dev,
                             float *wsum_dev);
int athena_mp_interp_fwd(const athena_mp_graph *g, int32_t F, const float *weights_dev, const float *x_dev, float *y_dev);
int athena_mp_interp_bwd_x(const athena_mp_graph *g, int32_t F, const float *weights_dev, const float *dy_dev, float *dx_dev);
int athena_mp_interp_bwd_coords(const athena_mp_graph *g, int32_t dim, int32_t F, const float *coords_dev, float eps,
                                const float *weights_dev, const float *x_dev, const float *y_dev, const float *dy_dev,
                                float *dcoords_dev);
/* The same for callers that hold Fortran arrays, staged through HBM.  athena_mp_interp_host: the weights of coords, then y; weights
 * [E] may be NULL.  athena_mp_interp_bwd_host: the weights and y again, then dx [n_cols, F] and dcoords [E, dim]; each may be NULL,
 * not both. */
int athena_mp_interp_host(const athena_mp_graph *g, int32_t dim, int32_t F, const float *coords, float eps, const float *x, float *y,
                          float *weights);
int athena_mp_interp_bwd_host(const athena_mp_graph *g, int32_t dim, int32_t F, const float *coords, float eps, const float *x,
                              const float *dy, float *dx, float *dcoords);
/* Max pooling over a handle's rows, with its arg-max and both reverse steps (pool.hip): the maximum over each neighbourhood -- the
 * reduction of PointNet++'s set abstraction (an MLP on every (sample, neighbour) pair, then the maximum over the neighbours), of
 * EdgeConv / DGCNN and of GraphSAGE-pool.  Nothing in the reference corresponds to them.
 * Definition.  g is any handle.  Row i is its forward CSR as athena_mp_graph_export shows it (rowptr, col, eid), column j its
 * transposed CSR (t_rowptr, t_src, t_eid; rows ascending).  Values are fp32.  Nothing is computed on them: they are compared and
 * copied.  Arrays are row-major.
 *   Vertex form (athena_mp_pool_max_fwd), x [n_cols, F] -> y [n_rows, F] and arg [n_rows, F] int32:
 *     for k = rowptr[i] .. rowptr[i+1]-1 in order, v = x[col[k], f]: entry k replaces the best so far when there is none yet, or
 *     v > best, or v is a NaN and best is not.  So the first maximum in row order wins; of +0 and -0, whichever comes first stays; a
 *     NaN wins over every number, and the first NaN stays.  y[i, f] is the bits of the chosen value, arg[i, f] its col[k], 0-based.
 *     An empty row gives y = +0 and arg = -1.  arg may be NULL.
 *   Edge form (athena_mp_pool_max_edges_fwd), h [E, F] -> y, arg: the same walk with v = h[eid[k], f]; arg is again col[k].
 *   Reverse of the vertex form (athena_mp_pool_max_bwd_x), arg, dy [n_rows, F] -> dx [n_cols, F]:
 *     acc = +0; for k = t_rowptr[j] .. t_rowptr[j+1]-1 in order, with i = t_src[k]: where arg[i, f] == j, acc = acc + dy[i, f]; other
 *     entries add nothing.  dx[j, f] = acc: a sequential fp32 sum over the rows ascending, bit-defined.
 *   Reverse of the edge form (athena_mp_pool_max_bwd_edges), arg, dy -> dh [E, F]:
 *     for the entry k of row i with e = eid[k], j = col[k]: dh[e, f] = dy[i, f] where arg[i, f] == j, else +0.
 *   Every element of every output is written.  There are no atomics: two runs are byte-identical.
 * Precondition, not checked: no row holds the same column twice -- every builder of the library guarantees this; with a repeated
 * column arg names both entries and the reverse steps count dy once for each.
 * The edge forms need what the interpolation entries need: edge columns, an edge id on every entry, and exactly as many entries as
 * edge columns (athena_mp_graph_create_bipartite_dev builds exactly that); each dh[e, :] then has one writer.  The vertex forms take
 * square handles too: one-set radius and k-nearest-neighbour graphs, and handles without edge ids.
 * Refused with a message: for the edge forms a handle without edge columns, an entry that carries no edge id, more or fewer entries
 * than edge columns; F < 1.  The library stays usable after a refusal.  E = 0, n_rows = 0 and n_cols = 0 succeed (empty arrays may
 * be NULL).  A caller's pointer needs only 4-byte alignment. */
int athena_mp_pool_max_fwd(const athena_mp_graph *g, int32_t F, const float *x_dev, float *y_dev, int32_t *arg_dev);
int athena_mp_pool_max_edges_fwd(const athena_mp_graph *g, int32_t F, const float *h_dev, float *y_dev, int32_t *arg_dev);
int athena_mp_pool_max_bwd_x(const athena_mp_graph *g, int32_t F, const int32_t *arg_dev, const float *dy_dev, float *dx_dev);
int athena_mp_pool_max_bwd_edges(const athena_mp_graph *g, int32_t F, const int32_t *arg_dev, const float *dy_dev, float *dh_dev);
/* The same for callers that hold Fortran arrays, staged through HBM.  athena_mp_pool_max_host: exactly one of x [n_cols, F] (the
 * vertex form) and h [E, F] (the edge form) is not NULL; arg [n_rows, F] may be NULL.  athena_mp_pool_max_bwd_host: dx [n_cols, F], the
 * reverse of the vertex form, and dh [E, F], the reverse of the edge form, both from the one arg; each may be NULL, not both. */
int athena_mp_pool_max_host(const athena_mp_graph *g, int32_t F, const float *x, const float *h, float *y, int32_t *arg);
int athena_mp_pool_max_bwd_host(const athena_mp_graph *g, int32_t F, const int32_t *arg, const float *dy, float *dx, float *dh);
/* Attention pooling over a handle's rows (attention.hip): a softmax over each row's entries, per head, then the weighted sum of
 * per-vertex or per-edge values with the weight chosen per head, and every reverse step -- the reduction of Point Transformer's
 * vector attention, of GAT-style set abstraction and of the attention kernels of transformer neural operators over a mesh and a
 * latent set.  Nothing in the reference corresponds to them.
 * Definition.  g is a handle with one entry per edge column (what the edge forms of interp and pool accept).  Row i is the forward
 * CSR (rowptr, col, eid), column j the transposed one (t_rowptr, t_src, t_eid; queries ascending).  H >= 1 heads, F >= 1,
 * F % H == 0, C = F / H; the head of feature column c is c / C.  Everything is fp32, every operation rounded on its own, no
 * contraction.  Arrays are row-major; E is the number of edge columns.
 *   athena_mp_attn_softmax_fwd  scores [E, H] -> alpha [E, H].  For row i and head h, over the entries k in CSR order, e = eid[k]:
 *     m = the maximum of scores[e, h];  p_k = exp(scores[e, h] - m);  S = p_0 + p_1 + ... in CSR order;  alpha[e, h] = p_k / S.
 *     So a -inf beside a finite maximum gives alpha exactly +0; a (row, head) whose scores hold a NaN or a +inf, or only -inf, is
 *     NaN in all of its entries and no other (row, head) is touched; a row of one finite entry gives exactly 1; an empty row
 *     writes nothing.  exp is the expf of athena_mp_softmax_fwd; alpha is held to that entry's bound, not to bits.
 *   athena_mp_attn_gather_fwd        alpha, x [n_cols, F] -> y [n_rows, F]:  acc = +0; for k = rowptr[i] .. in order:
 *                                    acc = acc + alpha[eid[k], c / C] * x[col[k], c];  y[i, c] = acc
 *   athena_mp_attn_gather_edges_fwd  alpha, h [E, F] -> y:  the same with h[eid[k], c] in the place of x[col[k], c]
 *     Bit for bit the sequential sum; an empty row gives +0.  At H = 1 the vertex form writes the bytes of athena_mp_interp_fwd.
 *   athena_mp_attn_gather_bwd_x      alpha, dy [n_rows, F] -> dx [n_cols, F]:  acc = +0; for k = t_rowptr[j] .. in order:
 *                                    acc = acc + alpha[t_eid[k], c / C] * dy[t_src[k], c];  dx[j, c] = acc.  A column without
 *                                    entries gives +0.
 *   athena_mp_attn_gather_bwd_edges  alpha, dy -> dh [E, F]:  the entry k of row i, e = eid[k]:  dh[e, c] = alpha[e, c / C] * dy[i, c]
 *   athena_mp_attn_gather_bwd_alpha  exactly one of x and h (the other NULL), dy -> dalpha [E, H]:  the entry k of row i, e = eid[k]:
 *                                    dalpha[e, h] = the sum over the C columns c of head h of dy[i, c] * v, v = x[col[k], c] or
 *                                    h[e, c].  The order of this sum is the implementation's; at C = 1 there is none, and
 *                                    dalpha is the product itself.
 *   athena_mp_attn_softmax_bwd       alpha, dalpha -> dscores [E, H]:  dot = +0; for k in CSR order: dot = dot + alpha[e, h] *
 *                                    dalpha[e, h];  then dscores[e, h] = alpha[e, h] * (dalpha[e, h] - dot).  Bit-defined from the
 *                                    given alpha and dalpha.
 *   Every element of every output is written, but for alpha, dalpha, dh and dscores along an empty row, which has no entry.  No
 *   atomics: two runs are byte-identical.
 * Refused with a message: what athena_mp_pool_max_edges_fwd refuses of a handle; H < 1; F < 1; F % H != 0; for bwd_alpha both or
 * neither of x and h.  The library stays usable after a refusal.  Empty sets succeed (empty arrays may be NULL).  A caller's
 * pointer needs only 4-byte alignment; with F % 4 == 0 (softmax: H % 4 == 0) and every array on a 16-byte boundary the rows move
 * 16 bytes at a time -- the same bytes, sooner. */
int athena_mp_attn_softmax_fwd(const athena_mp_graph *g, int32_t H, const float *scores_dev, float *alpha_dev);
int athena_mp_attn_gather_fwd(const athena_mp_graph *g, int32_t F, int32_t H, const float *alpha_dev, const float *x_dev, float *y_dev);
int athena_mp_attn_gather_edges_fwd(const athena_mp_graph *g, int32_t F, int32_t H, const float *alpha_dev, const float *h_dev,
                                    float *y_dev);
int athena_mp_attn_gather_bwd_x(const athena_mp_graph *g, int32_t F, int32_t H, const float *alpha_dev, const float *dy_dev,
                                float *dx_dev);
int athena_mp_attn_gather_bwd_edges(const athena_mp_graph *g, int32_t F, int32_t H, const float *alpha_dev, const float *dy_dev,
                                    float *dh_dev);
int athena_mp_attn_gather_bwd_alpha(const athena_mp_graph *g, int32_t F, int32_t H, const float *x_dev, const float *h_dev,
                                    const float *dy_dev, float *dalpha_dev);
int athena_mp_attn_softmax_bwd(const athena_mp_graph *g, int32_t H, const float *alpha_dev, const float *dalpha_dev,
                               float *dscores_dev);
/* The same for callers that hold Fortran arrays, staged through HBM.  athena_mp_attention_host: scores [E, H] -> alpha [E, H] (may be
 * NULL) and y [n_rows, F] over exactly one of x [n_cols, F] and h [E, F].  athena_mp_attention_bwd_host: alpha as the forward
 * returned it, the same one of x and h, dy [n_rows, F] -> dx [n_cols, F] (with x) or dh [E, F] (with h), and dscores [E, H] through
 * bwd_alpha and softmax_bwd; a NULL output is skipped, not all three. */
int athena_mp_attention_host(const athena_mp_graph *g, int32_t F, int32_t H, const float *scores, const float *x, const float *h,
                             float *alpha, float *y);
int athena_mp_attention_bwd_host(const athena_mp_graph *g, int32_t F, int32_t H, const float *alpha, const float *x, const float *h,
                                 const float *dy, float *dx, float *dh, float *dscores);
/* The gather that makes the edge MLP's input over a two-set handle, with its reverse (edge_gather.hip): h[e, :] = (xs[col], xq[row],
 * coords[e]) for every entry, the step between athena_mp_knn_pairs_bipartite and the MLP of PointNet++'s set abstraction and of
 * EdgeConv (relative: the first block is xs[col] - xq[row]), whose output athena_mp_pool_max_edges_fwd reduces; and back from the
 * MLP's input gradient to both sets' features and to coords.  Nothing in the reference corresponds to them.
 * Definition.  g is a handle that the edge forms of interp and pool accept:
 *   - it has edge columns;
 *   - every entry has an edge id;
 *   - it has as many entries as edge columns.
 * Row i is the forward CSR rowptr, col, eid.  Column j is the transposed CSR t_rowptr, t_src, t_eid, rows ascending.  All values are
 * fp32.  Arrays are row-major.
 *   Operands:  xs [n_cols, Fs] source features;  xq [n_rows, Fq] query features;  coords [E, dim] the edge input;  h [E, ld] forward
 *   output;  dh [E, ld] reverse input.
 *   - Fs, Fq, dim >= 0 and W = Fs + Fq + dim >= 1.
 *   - ld >= W is the row pitch of h and dh in elements.
 *   - relative is 0 or 1.  relative = 1 needs Fs == Fq >= 1.
 *   - A block of width 0 has a NULL pointer and is skipped.
 *   Forward.  For the entry k of row i, with j = col[k] and e = eid[k]:
 *     h[e, f],           f < Fs:   xs[j, f] bit for bit, or with relative the fp32 difference xs[j, f] - xq[i, f]
 *     h[e, Fs + f],      f < Fq:   xq[i, f] bit for bit
 *     h[e, Fs + Fq + c], c < dim:  coords[e, c] bit for bit
 *   - "Bit for bit" means a copy, not an arithmetic operation.  -0, infinities, NaN payloads and signalling NaNs pass unchanged.
 *   - Every one of the W defined columns of every row is written exactly once.
 *   - Columns W .. ld - 1 are never written.
 *   - When the difference is a NaN (a NaN operand, or inf - inf), the definition requires a NaN and leaves its payload open.
 *   Reverse.  Each of the three outputs is produced when its pointer is non-NULL.
 *   - dxs[j, f]: acc = +0.  Then for k = t_rowptr[j] .. in order, with e = t_eid[k]: acc = acc + dh[e, f].
 *   - dxq[i, f]: acc = +0.  Then for k = rowptr[i] .. in order, with e = eid[k]: acc = acc + dh[e, Fs + f], and with relative, after
 *     that, acc = acc - dh[e, f].
 *   - dcoords[e, c] = dh[e, Fs + Fq + c] bit for bit.
 *   The sums are sequential fp32 sums.  Every element of every requested output is written.  Empty rows and columns give +0.  Columns
 *   W .. ld - 1 of dh are never read.
 *   The kernels use no atomics.  Two runs are byte-identical.
 * Empty sets succeed (empty arrays may be NULL).  Pointers need 4-byte alignment only; with Fs % 4 == 0, Fq % 4 == 0, ld % 4 == 0 and
 * every array on a 16-byte boundary the rows move 16 bytes at a time -- the same bytes, sooner -- so a W that is no multiple of 4 is
 * worth a padded pitch (W = 64 + 3: ld = 68).
 * Refused with a message: what athena_mp_interp_fwd refuses of a handle; ld < W; relative with Fs != Fq; relative with Fs = 0; W < 1;
 * a negative width; a NULL block of positive width; relative outside 0, 1.  The library stays usable after a refusal. */
int athena_mp_edge_gather_fwd(const athena_mp_graph *g, int32_t Fs, const float *xs_dev, int32_t Fq, const float *xq_dev, int32_t dim,
                              const float *coords_dev, int32_t relative, int32_t ld, float *h_dev);
int athena_mp_edge_gather_bwd(const athena_mp_graph *g, int32_t Fs, int32_t Fq, int32_t dim, int32_t relative, int32_t ld,
                              const float *dh_dev, float *dxs_dev, float *dxq_dev, float *dcoords_dev);
/* The same for callers that hold Fortran arrays, staged through HBM.  athena_mp_edge_gather_host: h [E, ld] goes up before the call
 * and comes back after it, so its columns W .. ld - 1 keep what the caller put there.  athena_mp_edge_gather_bwd_host: each of dxs
 * [n_cols, Fs], dxq [n_rows, Fq] and dcoords [E, dim] may be NULL, not all three. */
int athena_mp_edge_gather_host(const athena_mp_graph *g, int32_t Fs, const float *xs, int32_t Fq, const float *xq, int32_t dim,
                               const float *coords, int32_t relative, int32_t ld, float *h);
int athena_mp_edge_gather_bwd_host(const athena_mp_graph *g, int32_t Fs, int32_t Fq, int32_t dim, int32_t relative, int32_t ld,
                                   const float *dh, float *dxs, float *dxq, float *dcoords);
/* Bond-angle triplets of a neighbour graph on the device, with gradients (triplets.hip): for every vertex the ordered pairs of bonds
 * that meet there and the cosine of the angle between them -- the three-body terms of DimeNet, M3GNet and ALIGNN -- and the way back
 * from a gradient per triplet to the builders' vec, which athena_mp_periodic_grad takes as dvec.  The triplets are a graph over the
 * CSR ENTRIES of a handle (its line graph): athena_mp_graph_create_bipartite_dev(nnz, nnz, T, pairs, ...) makes a handle of the pair
 * list, and the row kernels (athena_mp_edge_gather_fwd, athena_mp_interp_fwd, athena_mp_pool_max_edges_fwd, athena_mp_attn_*) run on
 * it over per-entry messages and per-triplet values.  Nothing in the reference corresponds to them.
 * Definition.  All integer results are exact.  All arithmetic is fp32, every operation rounded on its own, / and sqrt correctly
 * rounded.  g is a square handle with edge columns (built with_edge_ids = 1, add_self_loops or not).  Entry k is a 0-based position of
 * its forward CSR as athena_mp_graph_export shows it; i is its row, c = col[k], e = eid[k].
 *   Entry vectors (athena_mp_entry_vectors_fwd), vec [E, dim] -> dir [nnz, dim], the vector from vertex i to the neighbour of entry k:
 *     dir[k] = -vec[e] when i <= c;  dir[k] = +vec[e] when i > c;  dir[k] = +0 when e < 0 (an id-less self loop).
 *     vec has the builders' sign (smaller index minus larger).  A periodic self-image edge (c == i) is one entry per image; +shift and
 *     -shift are separate edges, so -vec[e] is right for both.
 *   Their reverse (athena_mp_entry_vectors_bwd), ddir [nnz, dim] -> dvec [E, dim]:  dvec[e] = acc, acc = +0, then over the entries of
 *     edge column e in the order of the handle's edge index (athena_mp_graph_export 8, 10): acc = acc - ddir[k] when i <= c, acc = acc
 *     + ddir[k] when i > c.  Every element of dvec is written.
 *   Participants (athena_mp_triplet_pairs).  cutoff3 = +infinity: every entry with e >= 0; vec may then be NULL.  Otherwise an entry
 *     takes part iff e >= 0 and r < cutoff3, with s = ((x0 * x0) + x1 * x1) + x2 * x2 over x = vec[e] and r = sqrt(s) -- the builder's
 *     own s and r, the comparison strict: the separate, shorter three-body cutoff of M3GNet.
 *   Triplets.  Every ordered pair (k, k') of distinct participants of one vertex row is a triplet; two images of the same neighbour
 *     (same col, different eid) are distinct entries.  Triplets are numbered in lexicographic order of (k, k').  pairs [2, capacity]
 *     int32, column-major, 1-based, is exactly the list athena_mp_graph_create_bipartite_dev(nnz, nnz, T, pairs, ...) takes: strictly
 *     ascending, one edge id per triplet.  rowptr [nnz + 1] int32, 0-based (may be NULL): rowptr[k] = the triplets whose first entry
 *     lies before k, rowptr[nnz] = T.  A row with m participants gives m (m - 1) triplets in one contiguous run.  Two builds of the
 *     same input are byte-identical.
 *   Angle (athena_mp_triplet_cos_fwd), on the triplet handle tg, dir -> cos [T].  For triplet t = (k, k'), a = dir[k], b = dir[k'],
 *     over the first dim components, dim in 1..3:
 *       sa = ((a0 * a0) + a1 * a1) + a2 * a2, sb likewise;  dot = ((a0 * b0) + a1 * b1) + a2 * b2;  den = sqrt(sa) * sqrt(sb);
 *       cos[t] = dot / den.  Where den == 0 (coincident points of a radius graph; never in a periodic graph), cos[t] = +0 and both
 *     gradient terms below are +0.  There is no clamp: |cos| may exceed 1 by rounding.
 *   Its reverse (athena_mp_triplet_cos_bwd), dir, cos, dcos [T] -> ddir [nnz, dim]:
 *       ga_c = b_c / den - (cos[t] * a_c) / sa;  gb_c = a_c / den - (cos[t] * b_c) / sb.
 *     ddir[k] = acc, acc = +0.  First over the triplets of row k of tg in CSR order: acc = acc + dcos[t] * ga.  Then over the entries of
 *     column k in the order of its transposed CSR (rows ascending): acc = acc + dcos[t] * gb.  An entry in no triplet gives +0; every
 *     element of ddir is written.  No atomics anywhere.
 * athena_mp_triplet_pairs with pairs_dev and rowptr_dev both NULL is a size query (the count pass only).  Refused with a message: a
 * handle without edge columns; a handle that is not square; dim outside 1..3; cutoff3 NaN or <= 0; vec NULL with a finite cutoff3; T
 * >= 2^31 (found by the count pass in 64-bit arithmetic, before anything of that size is allocated; the count is named); capacity < T.
 * nnz = 0 or T = 0 succeeds.  The cos entries are refused unless tg is square and carries one edge id per entry (what
 * athena_mp_pool_max_edges_fwd asks of a handle).  The library stays usable after a refusal.  Pointers need 4-byte alignment only.
 * athena_mp_triplet_stats: out = {triplets, participants, the longest run m (m - 1)} of the last athena_mp_triplet_pairs. */
int athena_mp_triplet_pairs(const athena_mp_graph *g, int32_t dim, const float *vec_dev, float cutoff3, int32_t *pairs_dev,
                            int64_t capacity, int32_t *rowptr_dev, int64_t *n_triplets_out);
int athena_mp_entry_vectors_fwd(const athena_mp_graph *g, int32_t dim, const float *vec_dev, float *dir_dev);
int athena_mp_entry_vectors_bwd(const athena_mp_graph *g, int32_t dim, const float *ddir_dev, float *dvec_dev);
int athena_mp_triplet_cos_fwd(const athena_mp_graph *tg, int32_t dim, const float *dir_dev, float *cos_dev);
int athena_mp_triplet_cos_bwd(const athena_mp_graph *tg, int32_t dim, const float *dir_dev, const float *cos_dev, const float *dcos_dev,
                              float *ddir_dev);
int athena_mp_triplet_stats(int64_t out[3]);
/* The same for callers that hold Fortran arrays.  athena_mp_triplets_host: the triplet CSR in the conventions of
 * athena_mp_radius_graph_bipartite_host -- adj_ia [nnz + 1] (1-based), adj_ja [2, capacity] column-major (second entry k', triplet id:
 * one directed entry per triplet) -- and, each may be NULL, dir [nnz, dim] and cos [T]; vec [E, dim] may be NULL with cutoff3 =
 * +infinity when neither is asked for.  adj_ja_out == NULL: size query for *n_triplets_out.  athena_mp_triplet_cos_bwd_host: dcos
 * [n_triplets] -> dvec [E, dim] in one call (entry vectors, cos, both reverse steps); it builds and frees the triplet handle inside,
 * and refuses an n_triplets that is not the graph's count. */
int athena_mp_triplets_host(const athena_mp_graph *g, int32_t dim, const float *vec, float cutoff3, int32_t *adj_ia_out,
                            int32_t *adj_ja_out, int64_t capacity, float *dir_out, float *cos_out, int64_t *n_triplets_out);
int athena_mp_triplet_cos_bwd_host(const athena_mp_graph *g, int32_t dim, const float *vec, float cutoff3, int64_t n_triplets,
                                   const float *dcos, float *dvec_out);
/* athena_mp_edge_grad_to_points and athena_mp_periodic_grad with every array on the host (a handle plus Fortran arrays), staged
 * through HBM */
int athena_mp_edge_grad_to_points_host(const athena_mp_graph *g, int32_t dim, const float *dcoords, float *dpoints);
int athena_mp_periodic_grad_host(const athena_mp_graph *g, int32_t n_structures, int32_t n_atoms, const int32_t *offsets,
                                 const int64_t *edge_offsets, const float *lat, float cutoff_max, const float *vec,
                                 const float *dfeature, int32_t fe_cols, const float *dvec, float *dcart, float *dfrac, float *virial,
                                 float *dlat);
int athena_mp_graph_export(const athena_mp_graph *g, int32_t which, void *host_dst, int64_t capacity,
                           int64_t *count);
int athena_mp_graph_destroy(athena_mp_graph *g);
int athena_mp_graph_dims(const athena_mp_graph *g, int32_t *n_rows, int32_t *n_cols, int64_t *nnz,
                         int32_t *n_edge_cols);
/* What a cached handle of (adj_ia, adj_ja) is valid for -- the key a layer's set_graph compares before it rebuilds
 * (SURVEY.md 8b "Ownership", F12; the reference re-copies the CSR in every set_graph_msgpass,
 * athena_msgpass_layer_sub.f90:144-174, called before every forward, athena_network_sub.f90:2727-2730).
 * 64-bit hash of the sizes and of EVERY word of both arrays (chunks of 2^20 values hashed by up to 8 host threads -- fewer
 * when the process's affinity mask holds fewer cores -- folded in chunk order: the key does not depend on the thread
 * count; about 2 ms for configs[1]'s 80 MB adj_ja on the GPU box's host): an in-place edit is always seen, which is what
 * the reference's copy-per-call guarantees.  Two different graphs of equal n and nnz get different keys (up to 2^-64).
 * ATHENA_MP_GRAPH_KEY_SAMPLED=1 opts into the cheap key for graphs of 2^18 entries and more (head, tail and 4096
 * strided samples of each array): then an in-place edit outside the samples is NOT seen and the caller must announce it
 * (invalidate_graph / graph_type.touch -> athena_mp_graph_evict).  Host-only, no device call, no library state: the
 * Fortran interface is declared `pure`. */
int athena_mp_graph_key(int32_t n_rows, int64_t nnz, const int32_t *adj_ia, const int32_t *adj_ja, uint64_t *key);
/* set_graph as a cache lookup: returns the handle of this CSR (square graph, degrees = row lengths -- what
 * set_graph_msgpass hands a layer), building it only when no handle with the same (device, n, nnz, n_edge_cols,
 * athena_mp_graph_key) is alive.  Handles are shared and reference counted: every layer of a network that is given
 * the same graph gets the same device arrays; a released handle stays cached (least recently used ones are freed once
 * the idle handles hold more than ATHENA_MP_GRAPH_CACHE_ENTRIES entries, default 2^28; 0 = free on the last release)
 * so the mini-batches of the next epoch find theirs.  athena_mp_graph_destroy on an acquired handle releases it.
 * The calling pattern it serves: athena_network_sub.f90:2727-2730 (set_graph before EVERY forward). */
int athena_mp_graph_acquire(int32_t n, int64_t nnz, const int32_t *adj_ia, const int32_t *adj_ja,
                            int32_t n_edge_cols, athena_mp_graph **out);
int athena_mp_graph_release(athena_mp_graph *g);
/* release, and the cache forgets the handle at once: the next athena_mp_graph_acquire of the same key BUILDS from the
 * arrays.  For callers that announce an in-place edit (layer%invalidate_graph, graph_type.touch) -- needed only under
 * the sampled key, harmless otherwise.  Other holders of the handle keep it (old topology) until they release it; the
 * last one frees it.  A handle that never came from the cache is destroyed. */
int athena_mp_graph_evict(athena_mp_graph *g);
/* cached handles alive or idle, lookups served from the cache, and device graph handles BUILT by this process so far
 * (graph_create / _from_edges / _acquire misses / shard blocks): what the cache tests count */
int athena_mp_graph_cache_stats(int64_t *handles, int64_t *hits, int64_t *builds);
/* Mini-batches out of a dataset handle that stays in HBM (batch_select.hip): what network%train does with get_sample(input_graph,
 * i0, i1) under shuffle_batches, without assembling the batch on the host or searching its neighbours again.  A plan
 * is made once per dataset handle; a select turns a list of structure ids into a new, independent handle plus index maps.
 * Parent: a handle g with n_rows == n_cols whose degrees are its row lengths (not a shard block built with row_deg / col_deg);
 *   offsets [B + 1] int32 on the HOST, 0-based, ascending from 0 to n_rows (empty structures allowed); edge_offsets [B + 1] int64 on
 *   the HOST, ascending from 0 to n_edge_cols, NULL exactly when the handle has no edge columns (a Kipf handle; an all-zero array is
 *   taken as NULL there).
 * Block-diagonal condition: every entry k of the rows [offsets[s], offsets[s+1]) has col[k] in that same range and eid[k] == -1 or
 *   eid[k] in [edge_offsets[s], edge_offsets[s+1]).  Every handle of DeviceGraph.from_structures, of a layer's batched set_graph and
 *   of io.batch_graphs satisfies it.  The transposed CSR and the edge-column index are then cut at the same places.
 * Child, for sel[0..m) (0-based structure ids, repeats allowed, any order): with nv[s], ne[s], nw[s] a structure's vertex, edge-column
 *   and entry counts and cv[t], ce[t], cw[t] their exclusive prefix sums over the selection, child row cv[t] + i is parent row
 *   offsets[s] + i, s = sel[t], entries in the same order:
 *     col' = col - offsets[s] + cv[t];  eid' = eid < 0 ? -1 : eid - edge_offsets[s] + ce[t];  coef' = coef bit for bit (degrees are row
 *     lengths and do not change);  t_rowptr, t_src (a vertex rebase), t_eid, t_coef likewise;  e_rowptr, e_row (a vertex rebase) and
 *     e_entry (an entry rebase: w - rowptr[offsets[s]] + cw[t]) cut at the edge-column boundaries;  deg_row, deg_col copied.
 *     max_row_len, max_col_len: the maximum over the selected structures;  band: the maximum over the selected structures of each
 *     structure's own max |col - row|, INT32_MAX (unknown) above 64, as graph_create;  the long-row plans are rebuilt for the child.
 *   The child is, array for array, the handle athena_mp_graph_create_from_edges builds from the child's own pair list (the selected
 *   structures' pairs in selection order, renumbered, with the parent's add_self_loops and with_edge_ids).  It is a deep copy, never in
 *   the handle cache, freed by athena_mp_graph_destroy, and stays valid after the plan and the parent are gone.  The plan needs the
 *   parent alive.  Note: a child always carries a band; a parent built on the device without its adjacency does not (graph_create
 *   computes the band from adj_ja on the host), so a child may take the banded gathers where its parent does not.
 * athena_mp_batch_select: offsets_out [m + 1] (int32) = cv with the child's vertex count last, edge_offsets_out [m + 1] (int64) = ce,
 *   both on the host, each may be NULL.  out == NULL: size query, only the two host arrays are filled and the device is not touched.
 *   vertex_map_dev [n_child]: vertex_map[cv[t] + i] = offsets[s] + i;  edge_map_dev [ne_child]: edge_map[ce[t] + j] = edge_offsets[s]
 *   + j (int32, 0-based, in HBM; each may be NULL): the rows of the dataset's per-vertex / per-edge tensors the batch uses
 *   (athena_mp_gather_rows).  The plan holds every per-structure table, so a select computes all sizes on the host and needs no
 *   device -> host copy and no synchronise: one upload of the selection's table, one launch (on the library's stream) for the
 *   thirteen arrays and both maps, no atomics; two selects of the same ids are byte-identical.  (It waits only for the stream to have
 *   taken the PREVIOUS select's table out of the plan's pinned staging block.)
 * Refused with a message, which names the structure or the id where there is one: a null argument, a rectangular handle or one with
 * explicit degrees, offsets / edge_offsets not ascending from 0 to the handle's rows / edge columns, edge_offsets given for a handle
 * without edge columns or missing for one with them, an entry that leaves its structure (found by the plan's check kernel, read as a
 * flag by the host), n_sel < 1, an id outside [0, B), a child of 2^31 entries or more. */
typedef struct athena_mp_batch_plan athena_mp_batch_plan;
int athena_mp_batch_plan_create(const athena_mp_graph *g, int32_t n_structures, const int32_t *offsets_host,
                                const int64_t *edge_offsets_host, athena_mp_batch_plan **out);
int athena_mp_batch_plan_destroy(athena_mp_batch_plan *p);
int athena_mp_batch_select(const athena_mp_batch_plan *p, int32_t n_sel, const int32_t *sel_host, athena_mp_graph **out,
                           int32_t *offsets_out, int64_t *edge_offsets_out, int32_t *vertex_map_dev, int32_t *edge_map_dev);
/* Neighbour-sampled mini-batches of ONE large graph that stays in HBM (neighbor_sample.hip): seeds -> a sampled rectangular block
 * per hop, relabelled, as a handle the Kipf, Duvenaud and graph_nop(local_term = false) steps take as it is.  athena_mp_batch_select
 * draws whole structures out of a block-diagonal dataset; this draws rows out of a graph that is one piece (a citation or product
 * graph, a mesh, a LIDAR sweep joined by athena_mp_knn_pairs).  Integer only: every implementation gives the same arrays, two calls
 * on the same input are byte-identical.  Ids are 1-based on this side of the boundary, as `sample` of athena_mp_farthest_points.
 *   Parent: any handle with n_rows == n_cols = n (self loops and multigraphs allowed, with or without edge columns).  A sampler
 *   plan borrows it (the parent must outlive the plan) and owns one int32 slot[n] in HBM, all -1 between calls, and reusable
 *   scratch.  One sample at a time per plan, ordered on the library's stream.
 *   A hop takes seeds [m] (distinct vertices, 1-based, on the device), a fan-out 1 <= k <= 64 or 0 for every entry, a 64-bit seed
 *   and a degree mode (0 = block, 1 = parent).
 *   Key of the entry at position p = w - rowptr[r] of the row of seed vertex r (0-based global row), all arithmetic mod 2^64:
 *       z = seed + 0x9E3779B97F4A7C15 * (((r << 32) | p) + 1)
 *       z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *       key = (z & 0xFFFFFFFF00000000) | p
 *   Selection: a row of length L <= k (or k = 0) is taken whole; otherwise the k entries with the smallest keys.  Chosen entries
 *   keep the parent's CSR order (ascending p).  So row s of the block has min(L, k) entries, rowptr is known before anything is
 *   drawn, and A VERTEX'S SAMPLE DEPENDS ON (seed, r) ALONE, not on which other seeds share the batch.  Entries, not neighbours,
 *   are drawn: a duplicated entry of a multigraph can be chosen twice.
 *   Relabelling: the block has n_rows = m; its columns are the seeds first in the order given (local id = position), then every
 *   other vertex that occurs as a chosen column, ascending by global id.  vertex_map [n_cols] = the global ids (vertex_map[:m] are
 *   the seeds); entry_map [nnz] = the parent CSR position w (1-based) of each block entry.  A parent with edge columns gives a block
 *   with one edge column per entry (edge id = entry index, what the interpolation, pooling and edge-gather entries require) and
 *   edge_map [nnz] = the parent's edge column of that entry, 1-based, 0 for an entry without one; a parent without edge columns
 *   gives a block without, and edge_map is not written.
 *   Degrees: block (0) = the row lengths and the number of block entries in each column, what athena_mp_graph_create_bipartite_dev
 *   would give; parent (1) = the parent's deg_row[seed] and deg_col[vertex_map].  With k = 0 and parent degrees a Kipf step on the
 *   block reproduces the parent's step on the seed rows.
 *   The handle is, array for array (all thirteen of athena_mp_graph_export), what athena_mp_graph_create(m, n_cols, nnz, adj_ia,
 *   adj_ja, n_edge_cols, row_deg, col_deg) builds from the block's CSR with those degrees (it IS that builder, fed from HBM); never
 *   in the handle cache, freed by athena_mp_graph_destroy, valid after the plan and the parent are gone.
 *   Several hops are several calls: hop h (0-based) uses seed_h = seed + 0xD1B54A32D192ED03 * (h + 1) mod 2^64, so a vertex is not
 *   handed the same neighbours twice, and its seeds are hop h - 1's whole vertex_map (the device array as it is).  The layers apply
 *   the blocks outermost first: outer.vertex_map[:outer.n_rows] == inner.vertex_map.
 * athena_mp_sample_count: the count pass alone, nnz of the block these seeds and k give (n_cols <= m + nnz); rowptr_dev [m + 1]
 *   (0-based, may be NULL) receives the block's row pointer.
 * athena_mp_sample_neighbors: vertex_map_dev / entry_map_dev / edge_map_dev are the caller's device buffers with their capacities in
 *   elements, each may be NULL (4-byte alignment is all they need); *n_cols_out and *nnz_out are always set on success; block may be
 *   NULL (the maps alone).  After a capacity refusal the buffers' contents are undefined.  A hop makes three host waits of its own
 *   (nnz and the seed flags; the number of new columns; the column degrees) in front of those of the handle's builder.
 * athena_mp_sample_neighbors_host: seeds and every output on the host (Fortran arrays), staged through HBM; also returns the block's
 *   CSR as adj_ia [m + 1] and adj_ja [2, entry_capacity] (column, edge id; 1-based, edge id 0 without edge columns).  The maps may
 *   each be NULL; block may be NULL.  adj_ja_out == NULL: size query for *n_cols_out and *nnz_out.
 * athena_mp_sample_stats, of the last sample: out[0] = rows drawn by key, out[1] = rows copied whole, out[2] = 64-entry steps of the
 *   drawn rows, out[3] = the steps skipped because no key lay below the current k-th; out[4..7] = microseconds of the count stretch
 *   (host clock, with its wait), the draw kernel, the relabelling (both device events) and the handle (host clock).
 * Refused with a message: n_rows != n_cols; k outside 0..64; a degree mode other than 0 or 1; a seed outside [1, n] (the first one
 * is named); a repeated seed (the first repetition is named); a capacity too small (the buffer is named); nnz or n_cols >= 2^31.
 * The library stays usable after a refusal, slot is put back, and the next sample is correct. */
typedef struct athena_mp_sampler athena_mp_sampler;
int athena_mp_sampler_create(const athena_mp_graph *parent, athena_mp_sampler **out);
int athena_mp_sampler_destroy(athena_mp_sampler *p);
int athena_mp_sample_count(athena_mp_sampler *p, int32_t n_seeds, const int32_t *seeds_dev, int32_t k, int32_t *rowptr_dev,
                           int64_t *nnz_out);
int athena_mp_sample_neighbors(athena_mp_sampler *p, int32_t n_seeds, const int32_t *seeds_dev, int32_t k, uint64_t seed,
                               int32_t degree_mode, int32_t *vertex_map_dev, int64_t vertex_capacity, int32_t *entry_map_dev,
                               int64_t entry_capacity, int32_t *edge_map_dev, int64_t edge_capacity, int32_t *n_cols_out,
                               int64_t *nnz_out, athena_mp_graph **block);
int athena_mp_sample_neighbors_host(athena_mp_sampler *p, int32_t n_seeds, const int32_t *seeds_host, int32_t k, uint64_t seed,
                                    int32_t degree_mode, int64_t vertex_capacity, int64_t entry_capacity, int32_t *vertex_map_out,
                                    int32_t *entry_map_out, int32_t *edge_map_out, int32_t *adj_ia_out, int32_t *adj_ja_out,
                                    int32_t *n_cols_out, int64_t *nnz_out, athena_mp_graph **block);
int athena_mp_sample_stats(int64_t out[8]);

/* The Duvenaud degree-bucket plan of a handle (bucket_plan.hip): what the bucketed update kernels (duv_mfma.hip) read.  A layer call
 * builds it on first use for its (min_deg, max_deg); athena_mp_duvenaud_plan builds it NOW, on the library's stream -- a training loop
 * calls it right after athena_mp_batch_select, so the first layer call on the fresh child finds it.  A no-op when the handle already
 * holds the plan of that (min_deg, max_deg); another pair replaces the plan (that waits for the stream, then frees the old arrays).
 * Definition, with deg[0..n) the handle's row degrees (athena_mp_graph_export 11), min_deg <= max_deg, nb = max_deg - min_deg + 1:
 *     bucket[v] = clamp(deg[v], min_deg, max_deg) - min_deg
 *     bucket_perm [n]     the vertices sorted by bucket, STABLE: equal buckets keep vertex order
 *     bucket_off [nb + 1] (int64, host) the bucket starts in bucket_perm
 *     tiles: every bucket cut into runs of 16, bucket-major, nt of them;  btile_start[t] = first index into bucket_perm,
 *     btile_info[t] = bucket << 8 | count (count 1..16),  btile_off [nb + 1] = first tile of each bucket (on the host and in HBM)
 *     btile_rows [4][16 nt]: slot i of tile t has v = bucket_perm[start + (i < count ? i : 0)], sv = i < count ? v : ~v;
 *       copy 0 holds sv at 16 t + i, copy 1 holds v there, copies 2 and 3 are copies 1 and 0 transposed 4 x 4 inside the tile
 *       (slot i at position 4 (i & 3) + (i >> 2))
 * Two routes write these arrays byte for byte alike.  host: one pass over the handle's host copy of the degrees, a counting sort,
 * five blocking uploads.  device: the host only counts (the sizes and the two host tables); the keys, one stable 8-bit counting pass
 * (hence nb <= 256), the tile offsets and the tile slots are made in HBM with no copy in either direction and no synchronise on a
 * handle's first plan (the library's scratch for the sort grows with the largest handle planned so far; growing it waits for the
 * stream).  ATHENA_MP_BUCKET_PLAN = auto | host | device pins the route (tests only, read at every build).  auto: device when
 * n_rows > 0 and nb <= 256, host otherwise; device with nb > 256 is refused with a message that names the limit.  A failed build
 * leaves no plan behind.
 * athena_mp_duvenaud_plan_export: one array of the plan on the host, with athena_mp_graph_export's convention (host_dst == NULL
 * queries count; capacity and count in elements).  which: 0 bucket_perm, 1 btile_start, 2 btile_info, 3 btile_rows (64 nt),
 * 4 btile_off in HBM, 5 bucket_off (int64, the host table), 6 btile_off (the host table); int32 except 5.  Refused when the handle
 * has no plan.
 * athena_mp_duvenaud_plan_stats: plans this process built on the host / on the device, and requests served by the plan a handle
 * already held (each may be NULL). */
int athena_mp_duvenaud_plan(const athena_mp_graph *g, int32_t min_deg, int32_t max_deg);
int athena_mp_duvenaud_plan_export(const athena_mp_graph *g, int32_t which, void *host_dst, int64_t capacity, int64_t *count);
int athena_mp_duvenaud_plan_stats(int64_t *host_builds, int64_t *device_builds, int64_t *reused);

/* ---- Kipf --------------------------------------------------------------- */
/* kipf_propagate, athena_diffstruc_extd_sub_kipf.f90:7-59
 *   y[v,:] = sum_w ((deg_v*deg_u)^-1/2) x[u,:]        x [n_cols,F], y [n_rows,F] */
int athena_mp_kipf_propagate_fwd(const athena_mp_graph *g, int32_t F, const float *x_dev, float *y_dev);
/* y = act(kipf_propagate(x)), act in {none, relu, sigmoid, tanh}: the activation of a time step whose dense step ran
 * before the aggregation, applied in the aggregation's store */
int athena_mp_kipf_propagate_act_fwd(const athena_mp_graph *g, int32_t F, const float *x_dev, int32_t act, float *y_dev);
/* get_partial_kipf_propagate_left_val, ..._sub_kipf.f90:85-111
 *   dx[u,:] = sum_{(v,w): ja(1,w)=u} grad[v,:]   (exact=0: the reference, NO coefficient;
 *   exact=1: multiplied by the coefficient, the mathematically exact adjoint) */
int athena_mp_kipf_propagate_bwd(const athena_mp_graph *g, int32_t F, const float *grad_dev,
                                 float *dx_dev, int32_t exact);
/* reverse_kipf_propagate, ..._sub_kipf.f90:116-158 (the node the higher-order path builds; grad_reverse does not
 * reach it):   c[u,:] = sum_{(v,w): ja(1,w)=u} a[v,:]   -- the coefficient-free scatter again, a [n_rows,F] -> c [n_cols,F].
 * Its partials: the FUNCTION form get_partial_left_reverse_kipf_propagate (:159-175) is kipf_propagate(upstream)
 * (with the coefficient), upstream [n_cols,F] -> out [n_rows,F]; the _val form (:176-205) is the same scatter as the
 * op itself.  Thin named entry points over the two kernels above. */
int athena_mp_reverse_kipf_propagate_fwd(const athena_mp_graph *g, int32_t F, const float *a_dev, float *c_dev);
int athena_mp_reverse_kipf_propagate_partial(const athena_mp_graph *g, int32_t F, const float *upstream_dev,
                                             float *out_dev);
int athena_mp_reverse_kipf_propagate_partial_val(const athena_mp_graph *g, int32_t F, const float *upstream_dev,
                                                 float *out_dev);
/* both reverse forms from ONE gather of the upstream rows: dx_plain = the reference's coefficient-free scatter
 * (exact = 0 above), dx_coef = the adjoint of the forward (exact = 1).  What a layer step needs when it applies
 * the dense step BEFORE the aggregation (F_out < F_in): dX = dx_plain . W,  dW = dx_coef^T . X */
int athena_mp_kipf_propagate_bwd_dual(const athena_mp_graph *g, int32_t F, const float *grad_dev,
                                      float *dx_plain_dev, float *dx_coef_dev);
/* the same pair in pull form over the FORWARD rows (a row shard of an undirected graph, whose transposed rows are
 * its own rows): y_plain[v] = sum_w x[col w], y_coef[v] = sum_w coef_w x[col w]; x has n_cols rows (local + halo) */
int athena_mp_kipf_propagate_fwd_dual(const athena_mp_graph *g, int32_t F, const float *x_dev,
                                      float *y_plain_dev, float *y_coef_dev);

/* out[r,:] = x[idx[r],:]  (r < n; idx 0-based device array).  Packs the halo rows a row partition
 * sends to its peers; same gather kernel as the aggregation. */
int athena_mp_gather_rows(int64_t n, int32_t F, const int32_t *idx_dev, const float *x_dev, float *out_dev);

/* ---- dense contraction (diffstruc matmul at athena_kipf_msgpass_layer.f90:951,
 *      athena_duvenaud_msgpass_layer.f90:842, athena_graph_nop_layer.f90:761) -- fp32 MFMA */
/* Z[N,Fo] = act( P[N,Fi] . Wt[Fi,Fo] (+ bias[Fo]) );  bias may be NULL */
int athena_mp_gemm_fwd(int64_t N, int32_t Fi, int32_t Fo, const float *P_dev, const float *W_dev,
                       const float *bias_dev, int32_t act, float *Z_dev);
/* dW(Fo,Fi) = dZ^T-contract: dWt[i,o] = sum_v P[v,i] dZ[v,o] */
int athena_mp_gemm_dw(int64_t N, int32_t Fi, int32_t Fo, const float *P_dev, const float *dZ_dev,
                      float *dW_dev);
/* dP[N,Fi] = dZ[N,Fo] . W  (dP[v,i] = sum_o dZ[v,o] Wt[i,o]) */
int athena_mp_gemm_dx(int64_t N, int32_t Fi, int32_t Fo, const float *dZ_dev, const float *W_dev,
                      float *dP_dev);

/* ---- fused Kipf layer step (one launch: aggregation + dense contraction, W resident in LDS) ------
 * update_message_kipf, athena_kipf_msgpass_layer.f90:943-952, one time step:
 *   P = kipf_propagate(X) (returned: the reverse pass needs it for dW; P_dev may be NULL when the reverse pass is
 *   athena_mp_kipf_layer_bwd, which works from X),  Z = act(P . Wt + bias)
 * One launch at 64 / 128 / 256 features on graphs without hub rows -- except on BANDED graphs (a block-diagonal batch of small
 * graphs: every neighbour within 32 rows, rows of at most 8 entries), where the aggregation gathers from LDS: one launch of its
 * own at 64 -> 64 (banded_fused.hip: the tile goes from LDS into the dense step), the gather and the dense step as two launches at
 * 128 features (profiles/r06_kipf_banded_ab.txt); same P bit for bit, Z within the order of the dense step's sums.  _bwd_x likewise. */
int athena_mp_kipf_layer_fwd(const athena_mp_graph *g, int32_t Fi, int32_t Fo, const float *x_dev,
                             const float *W_dev, const float *bias_dev, int32_t act, float *P_dev,
                             float *Z_dev);
/* reverse of the same step wrt its input: dX = A^T (dZ . W) evaluated as (A^T dZ) . W
 * (dZ = gradient at the pre-activation; exact as in athena_mp_kipf_propagate_bwd) */
int athena_mp_kipf_layer_bwd_x(const athena_mp_graph *g, int32_t Fi, int32_t Fo, const float *dZ_dev,
                               const float *W_dev, int32_t exact, float *dX_dev);

/* the whole reverse pass of one step from the step's INPUT X (no stored P): dX as above (may be NULL) and
 *   dW = dZ . P^T with P = A^ X (matmul reverse wrt params(t), athena_kipf_msgpass_layer.f90:951), evaluated as
 *   sum_u (A^^T dZ)[u] (x) X[u] -- both sums come from ONE gather of dZ over the transposed CSR.  With it the forward call
 *   may pass P_dev = NULL.  128 -> 128 without hub rows: one launch; otherwise a dual gather + two contractions. */
int athena_mp_kipf_layer_bwd(const athena_mp_graph *g, int32_t Fi, int32_t Fo, const float *dZ_dev,
                             const float *W_dev, const float *X_dev, int32_t exact, float *dX_dev, float *dW_dev);

/* same contraction over the FORWARD rows of a (rectangular) shard graph: dX[v,:] = (sum_w [coef] dZ[col[w],:]) . W
 * -- the backward of a row partition whose rows list their sources (athena_amd/dist.py) */
int athena_mp_pull_gemm(const athena_mp_graph *g, int32_t Fi, int32_t Fo, const float *dZ_dev,
                        const float *W_dev, int32_t exact, float *dX_dev);

/* ---- element-wise brackets of the path -------------- */
int athena_mp_activation_fwd(int32_t act, int64_t n, const float *z_dev, float *y_dev);
int athena_mp_activation_bwd(int32_t act, int64_t n, const float *y_dev, const float *g_dev, float *dz_dev);
int athena_mp_axpy(int64_t n, float alpha, const float *x_dev, float *y_dev); /* y += alpha x */
int athena_mp_add_row_bias(int64_t n_rows, int32_t F, const float *b_dev, float *y_dev); /* y[v, :] += b, y [n_rows, F] row-major */
/* dst = src on the device, one 16-byte element per thread in launch order (stream-ordered; 16-byte aligned pointers): the
 * copy form that reaches the HBM's streaming ceiling -- bench.py --full times it on 1 GiB and prints the rate beside the roofline
 * as the measured ceiling of the box it ran on (SURVEY.md 8d "report the measured stream ceiling alongside") */
int athena_mp_device_copy(void *dst_dev, const void *src_dev, uint64_t bytes);

/* ---- Duvenaud ------------------------------------------------------------ */
/* duvenaud_propagate, athena_diffstruc_extd_sub_duvenaud.f90:7-59
 *   c[v,:] = sum_w [ x[u,:] ; e[ja(2,w),:] ]     c [n_rows, Fv+Fe]; edge id 0 => zero vector */
int athena_mp_duvenaud_propagate_fwd(const athena_mp_graph *g, int32_t Fv, int32_t Fe,
                                     const float *x_dev, const float *e_dev, float *c_dev);
/* get_partial_duvenaud_propagate_left_val :115-141 / _right_val :143-171.  grad is [n_rows, Fv + Fe]; _bwd_x with Fe = 0 takes
 * the vertex part alone [n_rows, Fv], _bwd_e with Fv = 0 the edge part alone [n_rows, Fe] (athena_mp_duvenaud_update_bwd_split) */
int athena_mp_duvenaud_propagate_bwd_x(const athena_mp_graph *g, int32_t Fv, int32_t Fe,
                                       const float *grad_dev, float *dx_dev);
int athena_mp_duvenaud_propagate_bwd_e(const athena_mp_graph *g, int32_t Fv, int32_t Fe,
                                       const float *grad_dev, float *de_dev);
/* duvenaud_update :176-228;  weight [Fo*Fi*(max_deg-min_deg+1)] packed per degree bucket */
int athena_mp_duvenaud_update_fwd(const athena_mp_graph *g, int32_t Fi, int32_t Fo, int32_t min_deg,
                                  int32_t max_deg, const float *a_dev, const float *weight_dev,
                                  float *c_dev);
/* the same with the message activation applied in the epilogue (athena_duvenaud_msgpass_layer.f90
 * :790-803: duvenaud_update then activation%apply): z = act(W_d (a/d)); only z is written */
int athena_mp_duvenaud_update_act_fwd(const athena_mp_graph *g, int32_t Fi, int32_t Fo, int32_t min_deg,
                                      int32_t max_deg, const float *a_dev, const float *weight_dev,
                                      int32_t act, float *z_dev);
/* get_partial_duvenaud_update_val :284-324 */
int athena_mp_duvenaud_update_bwd_a(const athena_mp_graph *g, int32_t Fi, int32_t Fo, int32_t min_deg,
                                    int32_t max_deg, const float *grad_dev, const float *weight_dev,
                                    float *da_dev);
/* get_partial_duvenaud_update_weight_val :326-368 */
int athena_mp_duvenaud_update_bwd_w(const athena_mp_graph *g, int32_t Fi, int32_t Fo, int32_t min_deg,
                                    int32_t max_deg, const float *grad_dev, const float *a_dev,
                                    float *dweight_dev);
/* update + activation + the per-vertex part of the readout, p = softmax_over_outputs(R z) (update_readout_duvenaud,
 * athena_duvenaud_msgpass_layer.f90:838-855), in one launch; z [n_rows, Fo], R = params(T+t)%val(:,1) = R(O, Fo) flat,
 * p [n_rows, O].  The per-graph sums: athena_mp_segment_sum(O, n_rows, S, seg, p, out, accumulate). */
int athena_mp_duvenaud_update_readout_fwd(const athena_mp_graph *g, int32_t Fi, int32_t Fo, int32_t min_deg, int32_t max_deg,
                                          const float *a_dev, const float *weight_dev, int32_t act, float *z_dev, int32_t O,
                                          const float *R_dev, float *p_dev);
/* both partials above from ONE pass over grad (the pair is bound by the bytes it moves: 1.95 GB instead of 2.55 GB at
 * configs[2]); da [n_rows, Fi], dweight [Fo*Fi*D].  Shapes outside the fused kernel run the two entry points above. */
int athena_mp_duvenaud_update_bwd(const athena_mp_graph *g, int32_t Fi, int32_t Fo, int32_t min_deg, int32_t max_deg,
                                  const float *grad_dev, const float *a_dev, const float *weight_dev, float *da_dev,
                                  float *dweight_dev);
/* the same pair with da SPLIT where it is written: da_x [n_rows, Fv] and da_e [n_rows, Fe] instead of [n_rows, Fv + Fe].  The
 * reverse kernel visits the vertices in bucket order; rows of 288 bytes (64 + 8 floats) written in that order are partial
 * cache lines, and the propagate reverse that follows gathers its edge part as 32-byte slivers of them.  Split, the vertex
 * part is 256-byte rows and the edge part a dense array: athena_mp_duvenaud_propagate_bwd_x(g, Fv, 0, da_x, dx) and
 * athena_mp_duvenaud_propagate_bwd_e(g, 0, Fe, da_e, de) take the two halves (same sums, same order: bit-identical dx / de).
 * One launch at F_v = 64 and the fused kernel's widths (BASELINE configs[2]); other shapes go through the packed form. */
int athena_mp_duvenaud_update_bwd_split(const athena_mp_graph *g, int32_t Fv, int32_t Fe, int32_t Fo, int32_t min_deg,
                                        int32_t max_deg, const float *grad_dev, const float *a_dev, const float *weight_dev,
                                        float *da_x_dev, float *da_e_dev, float *dweight_dev);

/* One time step of the Duvenaud layer's reverse pass in one call: the readout's reverse (softmax over the outputs ->
 * matmul(R, z) -> the message activation; athena_duvenaud_msgpass_layer.f90:838-855 through diffstruc's grad_reverse,
 * athena_diffstruc_extd_sub.f90:309-313) and the update's reverse (get_partial_duvenaud_update_val / _weight_val,
 * athena_diffstruc_extd_sub_duvenaud.f90:284-368) -- what athena_mp_duvenaud_readout_bwd followed by
 * athena_mp_duvenaud_update_bwd_split compute, without dc [n_rows, Fv] between them where the shape allows it (F_v = 64,
 * F_v + F_e <= 96, O <= 16: ONE launch); other shapes run the two through a workspace.  Device pointers.
 * z [n_rows, Fv] the ACTIVATED update output of this time step, p [n_rows, O] its softmax(R z), gout [S, O] the gradient of the
 * per-graph readout, dz_next [n_rows, Fv] or NULL the next time step's gradient with respect to z, a [n_rows, Fv + Fe],
 * weight as athena_mp_duvenaud_update_fwd; out: da_x [n_rows, Fv], da_e [n_rows, Fe], dweight, dR [O, Fv] flat o + O f
 * (accumulate_dR != 0: added to; accumulate_da_e != 0: da_e is added to as well -- get_partial_duvenaud_propagate_right_val,
 * athena_diffstruc_extd_sub_duvenaud.f90:143-171, is linear in its upstream, so a layer that owns its reverse pass sums da_e over
 * its time steps and scatters the sum to the edge features once).  a_e != NULL: a arrives split as
 * athena_mp_duvenaud_update_readout_fwd_split takes it -- a = a_x [n_rows, Fv], a_e [n_rows, Fe]. */
int athena_mp_duvenaud_readout_update_bwd(const athena_mp_graph *g, int32_t Fv, int32_t Fe, int32_t min_deg, int32_t max_deg,
                                          int32_t O, int32_t S, const int32_t *seg, const float *z, const float *R, const float *p,
                                          const float *gout, const float *dz_next, int32_t act, const float *a,
                                          const float *weight, float *da_x, float *da_e, float *dweight, float *dR,
                                          int32_t accumulate_dR, int32_t accumulate_da_e, const float *a_e);

/* athena_mp_duvenaud_update_readout_fwd with a split where duvenaud_propagate (athena_diffstruc_extd_sub_duvenaud.f90:7-59)
 * concatenates: a_x [n_rows, Fv] = the neighbour sums of the vertex features (athena_mp_duvenaud_propagate_fwd with Fe = 0),
 * a_e [n_rows, Fe] = those of the edge features (athena_mp_duvenaud_propagate_fwd with Fv = 0).  The edge features of a layer do
 * not change from time step to time step (update_message_duvenaud, athena_duvenaud_msgpass_layer.f90:755-836, passes the same
 * edge_features to every duvenaud_propagate), so a layer that owns its tape gathers a_e once.  One launch at F_v = F_o = 64,
 * F_e <= 16, O <= 16; other shapes pack a into a workspace and take athena_mp_duvenaud_update_readout_fwd.  Device pointers. */
int athena_mp_duvenaud_update_readout_fwd_split(const athena_mp_graph *g, int32_t Fv, int32_t Fe, int32_t Fo, int32_t min_deg,
                                                int32_t max_deg, const float *a_x, const float *a_e, const float *weight,
                                                int32_t act, float *z, int32_t O, const float *R, float *p);
/* readout, athena_duvenaud_msgpass_layer.f90:838-855 over a block-diagonal batch:
 *   p[v,:] = softmax_over_outputs(logits[v,:]); out[s,:] (+)= sum_{v in seg s} p[v,:]
 *   seg_dev [S+1] 0-based vertex offsets of the graphs */
int athena_mp_softmax_segsum_fwd(int32_t O, int64_t N, int32_t S, const int32_t *seg_dev,
                                 const float *logits_dev, float *p_dev, float *out_dev,
                                 int32_t accumulate);
/* dlogits[v,:] = p (g_s - <g_s,p>) for v in segment s */
int athena_mp_softmax_segsum_bwd(int32_t O, int64_t N, int32_t S, const int32_t *seg_dev,
                                 const float *p_dev, const float *gout_dev, float *dlogits_dev);

/* readout with a readout activation other than softmax: activate with athena_mp_activation_* / _swish_*, then
 * out[s,:] (+)= sum_{v in seg s} p[v,:];  reverse: dp[v,:] = gout[graph of v,:] */
int athena_mp_segment_sum(int32_t O, int64_t N, int32_t S, const int32_t *seg_dev, const float *p_dev,
                          float *out_dev, int32_t accumulate);
int athena_mp_segment_sum_bwd(int32_t O, int64_t N, int32_t S, const int32_t *seg_dev, const float *gout_dev,
                              float *dp_dev);
/* The same readout with the logits contraction fused in (one launch per direction, logits and
 * dlogits never reach HBM).  R is the readout matrix R(O,Fv) in Fortran order, z [N,Fv] the step's
 * vertex features:   p = softmax(z R^T) per vertex;  out[s,:] (+)= sum_{v in s} p[v,:]            */
int athena_mp_duvenaud_readout_fwd(int64_t N, int32_t Fv, int32_t O, int32_t S, const int32_t *seg_dev,
                                   const float *z_dev, const float *R_dev, float *p_dev, float *out_dev,
                                   int32_t accumulate);
/* reverse of readout + the message activation that produced z (athena_duvenaud_msgpass_layer.f90
 * :790-803 then :838-855, reversed):  dl = p (g_s - <g_s,p>);  dR (+)= dl^T z;
 *   dc = act'(z) * (dl R + dz_next)      dz_next: gradient arriving from step t+1, or NULL       */
int athena_mp_duvenaud_readout_bwd(int64_t N, int32_t Fv, int32_t O, int32_t S, const int32_t *seg_dev,
                                   const float *z_dev, const float *R_dev, const float *p_dev,
                                   const float *gout_dev, const float *dz_next_dev, int32_t act,
                                   float *dc_dev, float *dR_dev, int32_t accumulate);

/* ---- Graph neural operator ------------------------------------------------
 * gno_kernel_eval + gno_aggregate, athena_diffstruc_extd_sub_nop.f90:26-115, :330-397,
 * re-associated so the [Fo*Fi, E] edge-kernel tensor is never materialised:
 *   m[i,:] = sum_{(j,e) in row i} reshape(V relu(U dx_e + b_u) + b_v,[Fo,Fi]) x[j,:]
 * theta = [U(H,d) | b_u(H) | V(Fo*Fi,H) | b_v(Fo*Fi)]  (:74-82);  coords [E,d]. */
int athena_mp_gno_aggregate_fwd(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo,
                                const float *theta_dev, const float *coords_dev, const float *x_dev,
                                float *m_dev);
/* gradients (:137-216, :235-325, :419-458, :480-526 composed through the same re-association) */
int athena_mp_gno_aggregate_bwd_x(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo,
                                  const float *theta_dev, const float *coords_dev,
                                  const float *grad_dev, float *dx_dev);
/* get_partial_gno_agg_features_val (:419-458) in PULL form over the graph's own rows:
 *   dx[v,:] = sum_{w in row v} K_{eid[w]}^T grad_ext[col[w],:]      dx [n_rows, Fi], grad_ext [n_cols, Fo]
 * equal to the scatter of athena_mp_gno_aggregate_bwd_x on an undirected graph whose two directions share one edge column
 * (athena's graphs, :369-376) -- the form a row block of a partitioned graph evaluates after the halo exchange of grad */
int athena_mp_gno_aggregate_bwd_x_pull(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo,
                                       const float *theta_dev, const float *coords_dev,
                                       const float *grad_ext_dev, float *dx_dev);
int athena_mp_gno_aggregate_bwd_theta(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi,
                                      int32_t Fo, const float *theta_dev, const float *coords_dev,
                                      const float *x_dev, const float *grad_dev, float *dtheta_dev);
int athena_mp_gno_aggregate_bwd_coords(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi,
                                       int32_t Fo, const float *theta_dev, const float *coords_dev,
                                       const float *x_dev, const float *grad_dev, float *dcoords_dev);
/* Training-mode pair (the reference keeps every forward intermediate on its tape for grad_reverse:
 * gno_aggregate's result node holds kappa [Fo*Fi, E], athena_diffstruc_extd_sub_nop.f90:330-397 -- 246 GB at
 * BASELINE configs[3]).  Here the forward pass may keep the re-associated S = sum_e [h_e;1] x_j^T per vertex
 * (n_tiles * 133120 floats: 33 GB at configs[3], sized for 288 GB of HBM) so that the reverse pass's
 * dVaug = S^T g streams it instead of rebuilding it.  Same m, same dtheta (bit for bit) as the pair above.
 *   _saved_bytes: *bytes = size of s_save_dev for this graph and shape, 0 if the shape does not take the
 *                 kernels that keep S (then use the pair above);
 *   _fwd_save:    athena_mp_gno_aggregate_fwd that also fills s_save_dev; x_dev, m_dev and s_save_dev must be 16-byte aligned
 *                 (refused otherwise, the outputs untouched: athena_mp_gno_aggregate_fwd takes any alignment);
 *   _bwd_theta_saved: athena_mp_gno_aggregate_bwd_theta reading the s_save_dev of the SAME graph, theta, coords, x. */
int athena_mp_gno_saved_bytes(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo,
                              int64_t *bytes);
int athena_mp_gno_aggregate_fwd_save(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo,
                                     const float *theta_dev, const float *coords_dev, const float *x_dev,
                                     float *m_dev, float *s_save_dev);
int athena_mp_gno_aggregate_bwd_theta_saved(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi,
                                            int32_t Fo, const float *theta_dev, const float *coords_dev,
                                            const float *x_dev, const float *grad_dev,
                                            const float *s_save_dev, float *dtheta_dev);

/* The whole reverse pass of gno_aggregate in ONE call, from one G = g . Vmat^T: dx (get_partial_gno_agg_features_val,
 * athena_diffstruc_extd_sub_nop.f90:419-458), dtheta (:480-526 composed with get_partial_gno_kernel_params_val :235-325) and,
 * on request, dcoords (:137-216).  Any of the three outputs may be NULL; s_save_dev is the S of
 * athena_mp_gno_aggregate_fwd_save (NULL: S is rebuilt).  The separate entry points above compute G twice -- once inside
 * the dx launch (as T . B2), once for the kernel MLP's gradient; here the kernel that holds a piece of G_i in LDS also
 * emits every entry's partial h_e^T G_i of dx, and a gather over the transposed CSR sums them.  Shapes
 * outside the fused kernels run the separate entry points; *fused_out (may be NULL) reports which it was.  Same values
 * as the separate entry points to fp32 rounding (the sums associate differently).  The per-entry partials live in a
 * library workspace of nnz * 256 bytes (7.6 GB at BASELINE configs[3]; grown on demand, reused by every call, released
 * by athena_mp_finalize), the transposed-entry map (nnz int32) in the graph handle.
 * STREAMS: with dtheta requested, the gather of the partials runs on a second, library-owned stream beside the S^T g launch
 * (fork after the kernel MLP's launches, join before the call returns: the caller's stream waits for it, so the outputs are
 * ordered on the caller's stream like any other call's, and the pattern can be captured into a HIP graph). */
int athena_mp_gno_aggregate_bwd(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo,
                                const float *theta_dev, const float *coords_dev, const float *x_dev,
                                const float *grad_dev, const float *s_save_dev, float *dx_dev, float *dtheta_dev,
                                float *dcoords_dev, int32_t *fused_out);

/* ---- activations with their own shape and the 'concatenate' merge (8f-2) -----
 * swish_array / get_partial_swish_val, athena_diffstruc_extd_sub.f90:424-492: y = x/(1+exp(-beta x));
 * the reverse pass differentiates at the INPUT x */
int athena_mp_swish_fwd(int64_t n, float beta, const float *x_dev, float *y_dev);
int athena_mp_swish_bwd(int64_t n, float beta, const float *x_dev, const float *grad_dev, float *dx_dev);
/* the activations that carry attributes (athena_activation_{linear,relu,sigmoid,tanh,leaky_relu,selu,gaussian,
 * piecewise}.f90 `apply`): y = f(x; p0, p1) * scale; the reverse pass differentiates at the INPUT x.
 *   kind        p0          p1       f
 *   LINEAR      -           -        x                                            (linear.f90:194)
 *   RELU        threshold   -        max(x, threshold)                            (relu.f90:201)
 *   SIGMOID     -           -        1/(1+exp(-x))
 *   TANH        -           -        tanh(x)
 *   LEAKY_RELU  alpha       -        max(x*alpha, x)                              (leaky_relu.f90:204)
 *   SELU        alpha       lambda   x>0 ? lambda x : alpha lambda (exp(x)-1)     (selu.f90:227-229)
 *   GAUSSIAN    sigma       mu       exp(-((x-mu)/sigma)^2/2) / (sqrt(2 pi) sigma) (gaussian.f90:8,221)
 *   PIECEWISE   gradient    limit    piecewise_array, athena_diffstruc_extd_sub.f90:216-254; its reverse factor
 *                                    follows get_partial_piecewise_val :275-290 AS WRITTEN (the test
 *                                    `x <= limit .or. x >= -limit` holds everywhere for limit >= 0, so the
 *                                    gradient passes through unchanged -- DESIGN.md 3.7) */
typedef enum {
    ATHENA_MP_ACTP_LINEAR = 0,
    ATHENA_MP_ACTP_RELU = 1,
    ATHENA_MP_ACTP_SIGMOID = 2,
    ATHENA_MP_ACTP_TANH = 3,
    ATHENA_MP_ACTP_LEAKY_RELU = 4,
    ATHENA_MP_ACTP_SELU = 5,
    ATHENA_MP_ACTP_GAUSSIAN = 6,
    ATHENA_MP_ACTP_PIECEWISE = 7
} athena_mp_activation_param;
int athena_mp_activation_param_fwd(int32_t kind, int64_t n, float scale, float p0, float p1, const float *x_dev,
                                   float *y_dev);
int athena_mp_activation_param_bwd(int32_t kind, int64_t n, float scale, float p0, float p1, const float *x_dev,
                                   const float *grad_dev, float *dx_dev);
/* softmax(val, dim=2): over the F features of each vertex (athena_activation_softmax.f90:183-203,
 * athena_diffstruc_extd_sub.f90:295-379); reverse: dz = y*g - y*sum(y*g) */
int athena_mp_softmax_fwd(int64_t N, int32_t F, const float *z_dev, float *y_dev);
int athena_mp_softmax_bwd(int64_t N, int32_t F, const float *y_dev, const float *grad_dev, float *dz_dev);
/* network%add(layer, input_list=[..], operator='concatenate') (example/msgpass_euler/src/main.f90:192-255):
 * out[v,:] = [a[v,:], b[v,:]]; the reverse pass splits grad (da_dev or db_dev may be NULL) */
int athena_mp_concat_fwd(int64_t N, int32_t Fa, int32_t Fb, const float *a_dev, const float *b_dev,
                         float *out_dev);
int athena_mp_concat_bwd(int64_t N, int32_t Fa, int32_t Fb, const float *grad_dev, float *da_dev,
                         float *db_dev);

/* ---- tail of a train step, device resident -----------------
 * compute_mse, athena_loss.f90:393-430:  *loss_dev = mean((p-e)^2)/2 ; dpred = (p-e)/n (may be NULL) */
int athena_mp_mse_loss(int64_t n, const float *pred_dev, const float *expected_dev, float *loss_dev,
                       float *dpred_dev);
/* apply_clip, athena_clipper.f90:165-210 on the flat gradient vector (athena_network_sub.f90:2903) */
int athena_mp_clip(int64_t n, float *grad_dev, int32_t l_min_max, float clip_min, float clip_max,
                   int32_t l_norm, float clip_norm);
/* minimise_sgd, athena_optimiser.f90:634-673.  reg_kind 0 none / 1 l1 / 2 l2 / 3 l1l2
 * (athena_regulariser.f90:85-138); grad is overwritten with -lr*grad as the reference does */
int athena_mp_sgd_step(int64_t n, float lr, float momentum, int32_t nesterov, int32_t reg_kind, float l1,
                       float l2, float *param_dev, float *grad_dev, float *velocity_dev);
/* minimise_adam, athena_optimiser.f90:1027-1091; iter >= 1 is optimiser%iter AFTER the increment of
 * network%update; decoupled selects the AdamW branch of the l2 regulariser */
int athena_mp_adam_step(int64_t n, float lr, float beta1, float beta2, float epsilon, int32_t iter,
                        int32_t reg_kind, float l1, float l2, int32_t decoupled, float *param_dev,
                        float *grad_dev, float *m_dev, float *v_dev);

/* ---- host-pointer staging variants (phase-1 Fortran callbacks) ------------- */
int athena_mp_kipf_propagate_fwd_host(const athena_mp_graph *g, int32_t F, const float *x_host, float *y_host);
int athena_mp_kipf_propagate_bwd_host(const athena_mp_graph *g, int32_t F, const float *grad_host,
                                      float *dx_host, int32_t exact);
int athena_mp_gemm_fwd_host(int64_t N, int32_t Fi, int32_t Fo, const float *P_host, const float *W_host,
                            const float *bias_host, int32_t act, float *Z_host);

/* more host-pointer staging variants (same semantics as the device entry points above; host.hip) */
int athena_mp_gemm_dw_host(int64_t N, int32_t Fi, int32_t Fo, const float *P, const float *dZ, float *dW);
int athena_mp_gemm_dx_host(int64_t N, int32_t Fi, int32_t Fo, const float *dZ, const float *W, float *dP);
int athena_mp_activation_fwd_host(int32_t act, int64_t n, const float *z, float *y);
int athena_mp_activation_bwd_host(int32_t act, int64_t n, const float *y, const float *g, float *dz);
int athena_mp_duvenaud_propagate_fwd_host(const athena_mp_graph *g, int32_t Fv, int32_t Fe, const float *x, const float *e, float *c);
int athena_mp_duvenaud_propagate_bwd_x_host(const athena_mp_graph *g, int32_t Fv, int32_t Fe, const float *grad, float *dx);
int athena_mp_duvenaud_propagate_bwd_e_host(const athena_mp_graph *g, int32_t Fv, int32_t Fe, const float *grad, float *de);
int athena_mp_duvenaud_update_fwd_host(const athena_mp_graph *g, int32_t Fi, int32_t Fo, int32_t mn, int32_t mx, const float *a, const float *w, float *c);
int athena_mp_duvenaud_update_bwd_a_host(const athena_mp_graph *g, int32_t Fi, int32_t Fo, int32_t mn, int32_t mx, const float *grad, const float *w, float *da);
int athena_mp_duvenaud_update_bwd_w_host(const athena_mp_graph *g, int32_t Fi, int32_t Fo, int32_t mn, int32_t mx, const float *grad, const float *a, float *dw);
int athena_mp_softmax_segsum_fwd_host(int32_t O, int64_t N, int32_t S, const int32_t *seg, const float *logits, float *p, float *out, int32_t accumulate);
int athena_mp_softmax_segsum_bwd_host(int32_t O, int64_t N, int32_t S, const int32_t *seg, const float *p, const float *gout, float *dlogits);
int athena_mp_gno_aggregate_fwd_host(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo, const float *theta, const float *coords, const float *x, float *m);
int athena_mp_gno_aggregate_bwd_x_host(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo, const float *theta, const float *coords, const float *grad, float *dx);
int athena_mp_gno_aggregate_bwd_theta_host(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo, const float *theta, const float *coords, const float *x, const float *grad, float *dtheta);
int athena_mp_gno_aggregate_bwd_coords_host(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo, const float *theta, const float *coords, const float *x, const float *grad, float *dcoords);

/* host-pointer variants of the composites and shaped activations */
int athena_mp_duvenaud_update_act_fwd_host(const athena_mp_graph *g, int32_t Fi, int32_t Fo, int32_t mn, int32_t mx, const float *a, const float *w, int32_t act, float *z);
int athena_mp_duvenaud_readout_fwd_host(int64_t N, int32_t Fv, int32_t O, int32_t S, const int32_t *seg, const float *z, const float *R, float *p, float *out, int32_t accumulate);
int athena_mp_duvenaud_readout_bwd_host(int64_t N, int32_t Fv, int32_t O, int32_t S, const int32_t *seg, const float *z, const float *R, const float *p, const float *gout, const float *dz_next, int32_t act, float *dc, float *dR, int32_t accumulate);
int athena_mp_softmax_fwd_host(int64_t N, int32_t F, const float *z, float *y);
int athena_mp_softmax_bwd_host(int64_t N, int32_t F, const float *y, const float *g, float *dz);
int athena_mp_swish_fwd_host(int64_t n, float beta, const float *x, float *y);
int athena_mp_swish_bwd_host(int64_t n, float beta, const float *x, const float *g, float *dx);
int athena_mp_activation_param_fwd_host(int32_t kind, int64_t n, float scale, float p0, float p1, const float *x,
                                        float *y);
int athena_mp_activation_param_bwd_host(int32_t kind, int64_t n, float scale, float p0, float p1, const float *x,
                                        const float *g, float *dx);

/* ---- the FUSED entry points behind diffstruc's one-partial-at-a-time callbacks (host pointers) ------------------------
 * update_message_duvenaud / update_readout_duvenaud (athena_duvenaud_msgpass_layer.f90:790-803, 838-855) in one launch:
 * z = act(duvenaud_update(a, w)) and the readout's per-vertex p = softmax(R z) -- host form of
 * athena_mp_duvenaud_update_readout_fwd; z becomes the value of the activation node, p the value of the readout's softmax node. */
int athena_mp_duvenaud_update_readout_fwd_host(const athena_mp_graph *g, int32_t Fi, int32_t Fo, int32_t mn, int32_t mx,
                                               const float *a, const float *w, int32_t act, float *z, int32_t O,
                                               const float *R, float *p);
/* grad_reverse asks a two-operand node for its partials ONE AT A TIME, each through a `pure` callback with an intent(in)
 * node (get_partial_left_val / get_partial_right_val: athena_diffstruc_extd_sub_duvenaud.f90:284-368,
 * athena_diffstruc_extd_sub_nop.f90:419-526) -- the callback can keep nothing, while the fused reverse kernels produce BOTH
 * partials from one pass over the upstream gradient.  A *_pair_host entry point computes both on the first request, returns
 * the one asked for (`which`) and parks the other on the device; the second request gets the parked one if and only if it
 * names the same graph handle, the same shapes and operand arrays with the same CONTENT (a 64-bit hash of every byte of each
 * operand, or the residency table's (id, version) for an array that lives on the device).  A request that does not match
 * recomputes.  A parked partial is handed over once.
 *   athena_mp_duvenaud_update_bwd_pair_host   which 0: da [n_rows, Fi] | 1: dweight [Fo Fi D]     (athena_mp_duvenaud_update_bwd)
 *                                             act != ATHENA_MP_ACT_NONE: the node is update + message activation in one (value
 *                                             z = act(duvenaud_update(a, w))); grad is then the gradient w.r.t. z and act'(z)
 *                                             is applied on the device first (z_or_null = z [n_rows, Fo])
 *   athena_mp_gno_aggregate_bwd_pair_host     which 0: dx [n_cols, Fi] | 1: dtheta | 2: dcoords [n_edge_cols, d]
 *                                             (athena_mp_gno_aggregate_bwd; dcoords is computed only when asked for)
 *   athena_mp_pair_stats                      fused passes run / partials handed over from a slot (tests, diagnostics) */
int athena_mp_duvenaud_update_bwd_pair_host(const athena_mp_graph *g, int32_t Fi, int32_t Fo, int32_t mn, int32_t mx,
                                            int32_t act, const float *z_or_null, const float *grad, const float *a,
                                            const float *w, int32_t which, float *out);
int athena_mp_gno_aggregate_bwd_pair_host(const athena_mp_graph *g, int32_t d, int32_t H, int32_t Fi, int32_t Fo,
                                          const float *theta, const float *coords, const float *x, const float *grad,
                                          int32_t which, float *out);
int athena_mp_pair_stats(int64_t *fused_passes, int64_t *handed_over);

/* ---- multi-GPU: communicator, row-partition shard, halo exchange (comm.hip) -----------------------------------------
 * The reference has no distributed code; these are the entry points SURVEY.md 8b/8e ask the
 * boundary to export (athena_mp_comm_create / graph_partition / halo_exchange) so that a Fortran host reaches the
 * 8-GPU Kipf step through ISO_C_BINDING, one process per GPU.  Transport: RCCL over xGMI -- grouped ncclSend /
 * ncclRecv to every peer on a communication stream, event-ordered against the compute stream; ncclAllReduce for dW.
 * (ATHENA_MP_COMM_TRANSPORT=shm swaps in a host-staged TEST transport for one-GPU boxes; never the default.)
 * What the sharded step replaces: the per-sample loop of update_message_kipf, athena_kipf_msgpass_layer.f90:940-957,
 * run on the rank's rows. */
typedef struct athena_mp_comm athena_mp_comm;
typedef struct athena_mp_shard athena_mp_shard;

/* 128 opaque bytes (an ncclUniqueId) drawn by ONE rank and handed to all (MPI_Bcast, a file, a torch store ...) */
int athena_mp_comm_unique_id(void *id128);
/* collective; uses the device athena_mp_init selected */
int athena_mp_comm_create(int32_t rank, int32_t world, const void *id128, athena_mp_comm **out);
/* MPI-free bootstrap: rank 0 publishes the id in `path`, the others wait for it.  Safe against files a crashed run left
 * behind: ranks > 0 announce themselves with a random nonce in `path`.hello.<rank> (re-written as a heartbeat), rank 0
 * accepts only hello files it has seen change and publishes id + nonces, a rank accepts `path` only when it carries its
 * own nonce.  Every wait is bounded by ATHENA_MP_COLLECTIVE_TIMEOUT_S when set, 300 s otherwise. */
int athena_mp_comm_create_from_file(int32_t rank, int32_t world, const char *path, athena_mp_comm **out);
int athena_mp_comm_destroy(athena_mp_comm *c);
int athena_mp_comm_info(const athena_mp_comm *c, int32_t *rank, int32_t *world, char *transport, int32_t transport_len);
/* What this rank's communicator has actually done, so that a multi-GPU line proves what it used: ranks_seen = the
 * transport's OWN count of ranks (RCCL: ncclCommCount; -1 unavailable), library_version (RCCL: ncclGetVersion, e.g. 22606),
 * transfers started, all-reduce payload bytes, and the bytes put on the wire to every peer (grouped ncclSend rows and this
 * rank's block of every whole-block all-gather); sent_bytes_per_peer [n_peers] may be NULL with n_peers 0. */
int athena_mp_comm_stats(const athena_mp_comm *c, int32_t *ranks_seen, int32_t *library_version, int64_t *transfers,
                         int64_t *allreduce_bytes, int64_t *sent_bytes_per_peer, int32_t n_peers);
/* Every transfer these entry points start has a deadline (ATHENA_MP_COLLECTIVE_TIMEOUT_S seconds from the moment it actually
 * starts on the device; default 1800, 0 = none): a rank whose peer is missing ends with a message on stderr / in
 * athena_mp_last_error and exit code 3 instead of hanging in its next synchronize.  A handler registered here is called first,
 * once, on the library's monitor thread -- the host's chance to flush its own state; the process ends when it returns.  Nothing
 * is ever written on the host program's stdout. */
int athena_mp_set_stall_handler(void (*handler)(int32_t rank, const char *what, double seconds));
int athena_mp_comm_barrier(athena_mp_comm *c);
/* in-place float32 sum over ranks (dW, d theta): _start enqueues it on the communication stream behind the work the
 * compute stream holds so far, _finish makes the compute stream wait for it; the host never blocks */
int athena_mp_allreduce_start(athena_mp_comm *c, float *buf_dev, int64_t count);
int athena_mp_allreduce_finish(athena_mp_comm *c);
int athena_mp_allreduce(athena_mp_comm *c, float *buf_dev, int64_t count);

/* the rank's rows of the global graph: adj_ia [n_local+1] 1-based, adj_ja [2,nnz] column-major with adj_ja(1,w) = GLOBAL
 * neighbour id (1-based; graph_type%adj_ja of the whole graph restricted to the rank's rows), adj_ja(2,.) ignored.
 * Rows are contiguous blocks in rank order.  Builds the [local | halo] renumbering (interior rows first), the halo
 * degrees and the four row blocks as graph handles, and decides HOW the halo travels:
 *   p2p        grouped ncclSend / ncclRecv of the distinct rows each peer needs, packed by a gather kernel;
 *              x_ext = [n local | n_halo distinct remote rows, grouped by owner]
 *   all-gather when the ranks together need more than tau (default 0.7, ATHENA_MP_HALO_ALLGATHER_FRACTION) of all remote
 *              rows anyway: ONE ncclAllGather of whole blocks, no pack kernel, no send lists;
 *              x_ext = [max_n local slots, n used | world blocks of max_n slots, block p in rank p's own row order] --
 *              a halo row is a view into its owner's block
 *   ATHENA_MP_HALO_MODE = auto | p2p | allgather overrides the choice.  Either way a caller allocates n_local + n_halo
 *   rows (athena_mp_shard_dims) and uses the shard's graphs; nothing else differs on its side.
 * Collective: argument errors are agreed on before any data moves, so all ranks return the error together.  The reverse
 * pass of a shard is a pull over the rank's own rows (exact for undirected graphs: row u lists v as often as row v lists
 * u) -- checked across all ranks with one 64-bit signed hash sum; a directed graph is an error on every rank. */
int athena_mp_shard_create(athena_mp_comm *c, int32_t n_local, int64_t nnz, const int32_t *adj_ia, const int32_t *adj_ja,
                           athena_mp_shard **out);
/* The same for ONE graph WITH edge features cut by rows (graph_nop_layer on a partitioned mesh -- SURVEY.md 8e "GNO: as
 * Kipf plus replicated theta and all-reduce of dtheta"; BASELINE configs[3] is one 2 M-vertex mesh, which sharding by whole
 * graphs cannot split).  adj_ja(2,w) = GLOBAL edge id (1-based, 0 = none) as graph_type%adj_ja carries it
 * (athena_diffstruc_extd_sub_nop.f90:367-378 reads it as the kernel column).  The four row-block handles keep the edge
 * columns, renumbered to the rank's own set: the distinct ids its rows reference, ascending -- athena_mp_shard_export(7)
 * lists them, athena_mp_shard_edge_cols counts them, and the rank holds coords [n_edge_cols, d] for exactly those.
 * Forward:  halo exchange of x, athena_mp_gno_aggregate_fwd on blocks 0 / 1 (interior rows under the transfer).
 * Reverse:  halo exchange of g = dL/dm, athena_mp_gno_aggregate_bwd_x_pull on blocks 2 / 3 (the pull over the rank's own
 *           rows -- requires row u to list (v, e) whenever row v lists (u, e), which is CHECKED here across all ranks and
 *           is an error on every rank otherwise); athena_mp_gno_aggregate_bwd_theta on blocks 0 / 1 needs local g rows
 *           only; theta is replicated and d theta (+ dW, db) all-reduced (athena_mp_allreduce). */
int athena_mp_shard_create_edges(athena_mp_comm *c, int32_t n_local, int64_t nnz, const int32_t *adj_ia,
                                 const int32_t *adj_ja, athena_mp_shard **out);
int athena_mp_shard_edge_cols(const athena_mp_shard *s, int32_t *n_edge_cols);
int athena_mp_shard_destroy(athena_mp_shard *s);
int athena_mp_shard_dims(const athena_mp_shard *s, int32_t *n_local, int32_t *n_interior, int32_t *n_halo, int64_t *nnz,
                         int64_t *row_offset, int64_t *n_total);
/* *mode 0 = p2p, 1 = all-gather; *fraction = distinct halo rows summed over the ranks / ((world-1) * n_total); *tau = the
 * threshold in force; *recv_rows = rows that cross a link into this rank per exchange */
int athena_mp_shard_info(const athena_mp_shard *s, int32_t *mode, double *fraction, double *tau, int64_t *recv_rows);
/* which: 0 / 1 = interior rows [0,n_int) / boundary rows [n_int,n) of the forward graph, 2 / 3 = the same blocks of the
 * backward (pull) graph; columns index x_ext = [n local rows | n_halo halo rows]; owned by the shard */
int athena_mp_shard_graph(const athena_mp_shard *s, int32_t which, athena_mp_graph **g);
/* 0 order [n] int32 | 1 halo_ids [distinct remote rows referenced] int64 | 2 send_idx [n_send] int32 |
 * 3 col_deg [n+n_halo] int32 | 4 send_counts [world] int64 | 5 recv_counts [world] int64 |
 * 6 ext_ids [n_halo] int64: global id held by each row of x_ext beyond the local ones, -1 = padding slot (== 1 in p2p mode);
 * 7 edge_ids [n_edge_cols] int64: global edge id (0-based) of each local edge column (shards built by _create_edges);
 * 8 cut edge columns [..] int32 (local ids grouped by peer) | 9 their offsets per peer [world+1] int64;
 * host_dst NULL = size query (count in elements) */
int athena_mp_shard_export(const athena_mp_shard *s, int32_t which, void *host_dst, int64_t capacity, int64_t *count);
/* x_ext [n + n_halo, F]: p2p mode packs + posts the grouped send/recv into the halo rows, all-gather mode posts one
 * ncclAllGather of the blocks; returns at once (kernels enqueued before _finish run under the transfer); slot 0 / 1 = two
 * exchanges may be outstanding */
int athena_mp_halo_start(athena_mp_shard *s, int32_t slot, int32_t F, float *x_ext_dev);
int athena_mp_halo_finish(athena_mp_shard *s, int32_t slot);
/* Halo REDUCE, the transpose of the exchange: y_ext [n + n_halo, F] (F a multiple of 4) holds in its rows beyond the local
 * ones what this rank computed FOR remote vertices -- the feature gradient of a scatter-form reverse pass
 * (athena_mp_gno_aggregate_bwd on a forward row block: get_partial_gno_agg_features_val, athena_diffstruc_extd_sub_nop.f90:419-458,
 * writes dx of every neighbour, local or not).  _start sends each such row to its owner (p2p mode: the contiguous segment of
 * every owner; all-gather mode: the whole block of every owner) and receives what the peers computed for this rank's rows;
 * _finish adds them into y_local [n, F] on the compute stream, peer by peer in rank order (deterministic).  Streams, events,
 * deadline and slots as athena_mp_halo_start / _finish; a slot carries one exchange OR one reduce at a time.  With it the
 * reverse pass of a partitioned graph needs no exchange of the upstream gradient and no symmetry of the graph. */
int athena_mp_halo_reduce_start(athena_mp_shard *s, int32_t slot, int32_t F, const float *y_ext_dev);
int athena_mp_halo_reduce_finish(athena_mp_shard *s, int32_t slot, float *y_local_dev);
/* Sum over the partition of a per-edge-column quantity -- the coordinate gradient of graph_nop_layer
 * (get_partial_gno_kernel_coords_val, athena_diffstruc_extd_sub_nop.f90:137-216): e_dev [n_edge_cols, F] holds this rank's share
 * (the sum over its own rows' entries); an edge column CUT by the partition has a share on both sides.  The cut columns are
 * exchanged with the one peer that shares them and added in: afterwards both ranks hold the full sum (the same bits).
 * Stream-ordered, the host does not block.  Shards of athena_mp_shard_create_edges only; athena_mp_shard_export(8 / 9) lists
 * the cut columns per peer. */
int athena_mp_shard_edge_reduce(athena_mp_shard *s, int32_t F, float *e_dev);
/* DEADLINES.  No RCCL collective has a completion deadline of its own, and the host never blocks in _halo_start /
 * _allreduce_start, so a rank whose peer is missing would hang in its next synchronize, far from the cause.  Every transfer
 * this library starts (halo exchange, gradient all-reduce, the metadata collectives of athena_mp_shard_create,
 * athena_mp_comm_barrier) is therefore watched through its completion event by a monitor thread: still pending
 * ATHENA_MP_COLLECTIVE_TIMEOUT_S seconds (default 1800 -- one rank may legitimately write a checkpoint, run an evaluation pass or
 * sit in a debugger; bench.py sets 120 for itself; x5 for the metadata collectives and the barrier; 0 = no monitor) after it
 * actually STARTED (an event just in front of it on the communication stream has completed: a host that enqueues many steps
 * ahead of the device is not mistaken for a stall) the PROCESS ends -- "[athena_mp] rank r stalled in <transfer> ..." on stderr
 * and in athena_mp_last_error, the handler of athena_mp_set_stall_handler if one is registered, exit code 3; no retry, no
 * cleanup that could block in the same communicator, nothing on the host program's stdout.  (The file bootstrap of
 * _comm_create_from_file waits ATHENA_MP_COLLECTIVE_TIMEOUT_S when set, 300 s otherwise.) */

/* ---- residency of host arrays: the *_host entry points without the PCIe round trip per op ---------------------------- *
 * athena's layers exchange array_type nodes whose %val lives on the host (athena_network_sub.f90:2752,2761: forward_generic2d
 * hands layer%output on; :2856: the optimiser reads the gradients).  With athena_mp_resident_mode(1) the result of a *_host
 * call stays in HBM, registered under its host array's (address, byte length), and a later *_host call that receives the
 * same array as an input uses the device copy: a chain of HIP ops moves its first input up once and nothing else until
 * athena_mp_resident_flush(host_ptr) materialises an array at the edge of the HIP island (NULL: all of them).
 * FORWARD results park; the outputs of the REVERSE entry points (every *_bwd_*_host, *_dw_host, *_dx_host and the *_pair_host
 * calls) are always copied home as well: they are the partials diffstruc's grad_reverse accumulates with host arithmetic the
 * moment a get_partial_*_val callback returns -- inside the island only as far as their INPUTS go.
 * Safety: an array whose only valid copy is on the device carries a 16-byte sentinel at both ends of its host storage; if
 * host code wrote it (or the allocator handed the address to another array) the sentinel is gone and the host content is
 * uploaded instead -- and a flush (explicit, forced by an overlapping argument, or athena_mp_resident_mode(0)) then leaves the
 * host array ALONE: the host content is the newer one (round 3 copied the stale device data over it).  The sentinel guards
 * the two ENDS of the array: host code that rewrites only interior elements of a parked result without touching its first
 * or last 16 bytes is outside the contract (flush the array before writing into it).  An argument that merely overlaps a
 * registered array (a slice) materialises that array first.
 * Arrays under 64 bytes are always staged.  athena_mp_resident_mode(0) flushes everything and releases the device copies.
 * LIFETIME CONTRACT: the table holds host ADDRESSES.  An array must be dropped (athena_mp_resident_drop) before its host
 * storage is deallocated -- in the finaliser of the node / layer that owns it -- because a flush (explicit, at
 * athena_mp_resident_mode(0), or forced by an overlapping argument) WRITES to that address.  athena_mp_resident_drop(NULL)
 * forgets everything without touching host memory (the safe way out when lifetimes are unknown: flush what you read first).
 * Explicit form for a shim that manages an array itself: _acquire (dirty_host = 1: upload now; 0: allocate / trust the
 * device copy) -> device pointer for the *_dev entry points; _release(dirty_dev = 1) marks the device copy as the valid
 * one; _drop forgets an array WITHOUT copying back (call it when the host array is deallocated). */
int athena_mp_resident_mode(int32_t on);
int athena_mp_resident_acquire(const void *host_ptr, uint64_t bytes, int32_t dirty_host, void **dev_ptr);
int athena_mp_resident_release(const void *host_ptr, int32_t dirty_dev);
int athena_mp_resident_flush(const void *host_ptr);
int athena_mp_resident_drop(const void *host_ptr);
int athena_mp_resident_stats(int64_t *arrays, int64_t *h2d_bytes, int64_t *d2h_bytes, int64_t *reused_inputs,
                             int64_t *lazy_outputs);

#ifdef __cplusplus
}
#endif
#endif /* ATHENA_MP_H */
